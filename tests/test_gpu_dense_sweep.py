"""The dense sweep (tests/dense_sweep.py, -m gpu): the dense kernels around the attention path -- weight gradients,
LayerNorm / feed-forward, the table sum, the combine and its backward, bwd_reduce / d sqrt_w, rpe_scale -- bit for bit
against exact float64 sums on integer inputs, and against float64 within measured bounds where the arithmetic is not a
sum of products.  One test per case (a failure names it); the worst figure of every bounded quantity, with torch
float32's beside it, is printed at the end of the module (pytest -s).  Then the staged API's row arguments: a strided
view or a view at an odd storage offset gives the result of a dense, aligned clone, or is refused."""
import pytest
import torch

import dense_sweep as ds
import shape_sweep as sw

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_worst):
        ours, t32, cid = _worst[key]
        print(f"dense sweep worst {key}: {ours:.3e} (torch float32 {t32:.3e}) at {cid}")


@pytest.mark.parametrize("cid", [c.id for c in ds.CASES])
def test_dense_kernel_vs_float64(cid, gpu_device):
    case = ds.BY_ID[cid]
    fig = ds.measure(case, gpu_device)
    for key, (ours, t32) in fig.items():
        if ours > _worst.get(key, (-1.0, 0.0, ""))[0]:
            _worst[key] = (ours, t32, cid)
    ds.assert_bounds(case, fig)


# H * C = 64 exactly: the last shape whose d sqrt_w comes out of dsw_kernel (hept_amd/autograd.py:141); two ragged clouds
HC64 = sw.Shape("h16d16c4-b40", (40 * 2 + 7, 40 + 13), 40, 2, 16, 16, 4, 641, True)


@pytest.mark.parametrize("tiles", sw.TRAIN_TILES)
def test_training_step_at_64_dsw_lanes(tiles, gpu_device):
    assert HC64.H * HC64.C == 64 and "bwd-dsw-kernel" in sw.cells(HC64)
    sw.check_backward(HC64, tiles, gpu_device)


# ---------------------------------------------------------------------------------------------------------------------
# the stage functions read what they are given
# ---------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    """Equal bit for bit (16-bit rows hold f32 words in two halves: read as 16-bit numbers some of them are NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def strided(t):
    """The same values in every other slot of a buffer twice as large along the leading dimension."""
    assert t.shape[0] > 1
    buf = torch.zeros(2 * t.shape[0], *t.shape[1:], dtype=t.dtype, device=t.device)
    buf[::2] = t
    view = buf[::2]
    assert not view.is_contiguous() and _same_bits(view, t)
    return view


def shifted(t):
    """A contiguous view at a storage offset of one element."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    view = buf[1:].view(t.shape)
    assert view.is_contiguous() and view.storage_offset() == 1 and _same_bits(view, t)
    return view


_stage = {}


def _stage_inputs(dev):
    """One small cloud through the stages (two tables, so that every row tensor has a leading dimension above 1)."""
    if _stage:
        return _stage
    from hept_amd import ops
    from hept_amd.synthetic import make_inputs

    h, d, c, b, t = 8, 24, 6, 64, 2
    inp = make_inputs([200, 120], block_size=b, n_hashes=t, coords_dim=c, h_dim=d, num_heads=h, seed=77)
    g = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
    n = g["q"].shape[0]
    sqrt_w = ops.rpe_scale(g["w_rpe_weight"], h, d, 10)
    gen = torch.Generator().manual_seed(78)
    _stage.update(g=g, dims=(n, h, d, c, b, t))
    for prec in ("fp32", "bf16", "mixed16"):
        ph = ops.prep_hash(g["q"] * 0.3, g["k"] * 0.3, g["v"], g["coords"] * 0.2, sqrt_w, g["alpha"],
                           g["combined_shifts"], prec)
        qpos, kpos = ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"])
        part = ops.block_attn(ph["qhat"], ph["kvhat"], qpos, kpos, d, b)
        _stage[prec] = dict(ph=ph, qpos=qpos, kpos=kpos, part=part)
    # the src variant's keys (tests/test_gpu_src.py): region indices per (table, head, point), region counts per (table, head)
    eta = torch.randint(0, 4, (t * h, n), generator=gen).float().to(dev)
    phi = torch.randint(0, 4, (t * h, n), generator=gen).float().to(dev)
    regions_h = torch.full((2, t * h), 3.5).to(dev)
    _stage["geo"] = ops.geo_args((eta, phi), regions_h, t, h, n)
    _stage["gacc"] = torch.randn(n, h, 32, generator=gen).to(dev)
    _stage["ffn"] = [torch.randn(s, generator=gen).to(dev) * 0.2 for s in ((n, d), (d,), (d,), (d, d), (d,), (d, d), (d,))]
    return _stage


def _call(name, st, over):
    """The stage function ``name`` with the arguments named in ``over`` replaced (the table of test_stage_layouts)."""
    from hept_amd import ops

    n, h, d, c, b, t = st["dims"]
    g = st["g"]
    fn, _, prec = name.partition(":")
    s = st[prec or "fp32"]
    ph = dict(s["ph"], **{k: v for k, v in over.items() if k in s["ph"]})
    part = over.get("part", s["part"])
    if fn == "reduce_tables":
        return ops.reduce_tables(part, d)
    if fn == "reduce_tables_packed":
        return ops.reduce_tables(part, d, packed=True)
    if fn == "combine_out":
        return ops.combine_out(part, d, g["out_weight"], g["out_bias"])
    if fn == "combine_ffn":
        x, lw, lb, w1, b1, w2, b2 = st["ffn"]
        return ops.combine_ffn(part, d, g["out_weight"], g["out_bias"], x, lw + 1.0, lb, 1e-5, w1, b1, w2, b2)
    if fn == "block_attn":
        return ops.block_attn(ph["qhat"], ph["kvhat"], s["qpos"], s["kpos"], d, b)
    if fn == "block_attn_bwd":
        return torch.cat([x.reshape(-1) for x in ops.block_attn_bwd(ph["qhat"], ph["kvhat"], s["qpos"], s["kpos"],
                                                                    st["gacc"], d, c, b)])
    if fn == "sort_tables":
        return torch.stack(ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"]))
    if fn == "sort_tables_src":
        return torch.stack(ops.sort_tables_src(ph["qproj"], ph["kproj"], *st["geo"], ph["minmax"]))
    raise KeyError(name)


# (stage function[:precision of the rows], the row arguments it hands to C)
LAYOUTS = [("reduce_tables", ("part",)), ("reduce_tables:bf16", ("part",)), ("reduce_tables_packed:bf16", ("part",)),
           ("combine_out", ("part",)), ("combine_out:bf16", ("part",)), ("combine_ffn", ("part",)),
           ("combine_ffn:bf16", ("part",)), ("block_attn", ("qhat", "kvhat")), ("block_attn:bf16", ("qhat", "kvhat")),
           ("block_attn:mixed16", ("qhat", "kvhat")), ("block_attn_bwd", ("qhat", "kvhat")),
           ("block_attn_bwd:bf16", ("qhat", "kvhat")), ("sort_tables", ("qproj", "kproj", "minmax")),
           ("sort_tables_src", ("qproj", "kproj", "minmax"))]


@pytest.mark.parametrize("view", [strided, shifted], ids=["strided", "shifted"])
@pytest.mark.parametrize("name,arg", [(n, a) for n, args in LAYOUTS for a in args])
def test_stage_layouts(name, arg, view, gpu_device):
    """A non-contiguous view, or a contiguous one that is not 16-byte aligned, of a row argument: the result of a dense,
    aligned clone, or a refusal in Python -- never other numbers."""
    st = _stage_inputs(gpu_device)
    s = st[name.partition(":")[2] or "fp32"]
    dense = (s["part"] if arg == "part" else s["ph"][arg]).clone()
    assert dense.is_contiguous() and dense.data_ptr() % 16 == 0
    want = _call(name, st, {arg: dense})
    try:
        got = _call(name, st, {arg: view(dense)})
    except (ValueError, TypeError):
        return
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"{name}: a {view.__name__} {arg} gives other numbers than its dense clone"
