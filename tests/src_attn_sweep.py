"""Deterministic shape sweep of the src variant's fused ``Attn`` block (``SrcAttn``, ``Attn(..., variant="src")``): every
element of the eval block and every gradient of the training block against a float64 evaluation of the reference's src
block on the GPU's own permutations (run by tests/test_gpu_src_attn_sweep.py, coverage pinned on CPU by
tests/test_src_attn_cells.py).  A plain module, not a conftest, built like tests/attn_sweep.py and reusing its
parameters, precisions and bounds.

The src block differs from the example block in its caller-side input (``prepare_input_src``: one cloud padded up to a
multiple of B, ``raw_size`` real rows, region ids per (table, head)) and in the operator's padding rows (zero q^, k^, v,
hash +inf, sort key hash + get_geo_shift).  ``SHAPES`` crosses the coordinate count, the table chunking of the row
builder and the sort, the sort's one-workgroup and two-launch paths and the kind of ``raw_size`` (N: no padding, N - 1,
N - B + 1: one real point in the last block, 1 point in a cloud of one block), with padding rows of ``x`` zero (the
first layer, as ``prepare_input_src`` pads) or not (a later layer, whose padding rows carry the previous block's
residual and feed-forward).  Nothing here touches the GPU at import time."""
from collections import namedtuple

import torch

import attn_sweep as asw
from attn_sweep import ATOL, COORDS, D, EPS, GRAD_PARAMS, H, K, MAX_TABLES, PRECISIONS, RTOL, ROW16_64, TRAIN, \
    TRAIN_ROW, TRAIN_ROW_CANCEL, TRAIN_TENSOR, CANCEL, SMALL_CAP, COST_CAP, ILL_WEIGHT, chunks, tmax, row_x, _cached

Shape = namedtuple("SrcShape", "id N raw B T C later seed bwd")
KINDS = ("full", "minus1", "one-in-last-block", "single")


def raw_kind(s):
    if s.N == s.B and s.raw == 1:
        return "single"
    if s.raw == s.N:
        return "full"
    if s.raw == s.N - 1:
        return "minus1"
    assert s.raw == s.N - s.B + 1, s
    return "one-in-last-block"


def _shapes():
    out = []

    def add(n, kind, b, t, c, later=False, bwd=False):
        raw = {"full": n, "minus1": n - 1, "one-in-last-block": n - b + 1, "single": 1}[kind]
        assert kind != "single" or n == b
        sid = f"n{n}-{kind}-b{b}-t{t}-c{c}" + ("-later" if later else "")
        out.append(Shape(sid, n, raw, b, t, c, later, 1200 + len(out), bwd))

    # small clouds: every kind of raw_size at every coordinate count, one chunk of tables and several
    add(1000, "full", 100, 3, 6, bwd=True)
    add(1000, "minus1", 100, 3, 6, later=True, bwd=True)
    add(1000, "one-in-last-block", 100, 3, 6)
    add(1024, "minus1", 128, 1, 4, bwd=True)
    add(1280, "one-in-last-block", 128, 3, 4, later=True, bwd=True)
    add(896, "full", 128, 3, 2, later=True)
    add(768, "one-in-last-block", 256, 1, 2, bwd=True)
    add(1024, "minus1", 256, 3, 6, later=True)
    add(660, "minus1", 33, 8, 4, bwd=True)
    add(396, "one-in-last-block", 33, 9, 2, later=True, bwd=True)
    add(500, "minus1", 50, 17, 6, later=True)
    add(720, "full", 72, 17, 4)
    add(800, "minus1", 100, 8, 2, bwd=True)
    # a cloud of one block holding one real point
    add(100, "single", 100, 3, 6, bwd=True)
    add(128, "single", 128, 9, 4, later=True)
    add(33, "single", 33, 1, 2, later=True, bwd=True)
    # around the one-workgroup sort's capacity (6144): below, at, above; above with chunks of tables
    add(6016, "minus1", 128, 3, 6)
    add(6144, "one-in-last-block", 128, 1, 4, later=True)
    add(6144, "full", 128, 3, 2)
    add(6272, "full", 128, 1, 6, later=True, bwd=True)
    add(6272, "minus1", 128, 3, 4)
    add(6400, "one-in-last-block", 256, 1, 2, later=True, bwd=True)
    add(6272, "one-in-last-block", 32, 9, 6)
    add(6300, "minus1", 50, 9, 4, later=True)
    add(6176, "minus1", 32, 9, 2, bwd=True)
    return out


SHAPES = _shapes()
BY_ID = {s.id: s for s in SHAPES}
BWD_SHAPES = [s for s in SHAPES if s.bwd]


def cost(s):
    """float64 elements of the oracle's largest intermediate (T, H, N/B, B, B)."""
    return s.T * H * s.N * s.B


def cells(s):
    """The sweep's axes: coordinates x table chunking x sort path x kind of raw_size, and the branches of each."""
    chunking = "table-chunks" if s.T > MAX_TABLES else "tables-one-chunk"        # csrc/capi.hip attn_block_impl
    sort = "sort-two-launch" if s.N > SMALL_CAP else "sort-one-workgroup"         # csrc/sort_tables.hip
    kind = raw_kind(s)
    out = {f"coords{s.C}", chunking, sort, f"raw-{kind}", "pad-later" if s.later else "pad-zero",
           f"{chunking}/{sort}", f"coords{s.C}/raw-{kind}", f"{sort}/raw-{kind}", f"coords{s.C}/{chunking}",
           f"coords{s.C}/{sort}", f"B{s.B}", f"T{s.T}"}
    for tl in chunks(s.T):
        out.add(f"prep<{s.C},{tmax(tl)}>")                                        # csrc/prep_hash.hip launch_prep_fused
    if s.bwd:
        out |= {f"bwd-coords{s.C}", f"bwd-raw-{kind}", f"bwd-{sort}", f"bwd-{chunking}"}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def params(s):
    """A default-initialised block's state dict as attn_sweep draws it, plus the src checkpoint's ``attn.e2lsh.beta``."""
    p = asw.default_params(s.C, s.T, s.seed)
    with torch.random.fork_rng():
        torch.manual_seed(s.seed + 2)
        p["attn.e2lsh.beta"] = torch.rand(1, s.T)
    return p


def inputs(s):
    """x, the kwargs of ``prepare_input_src`` on synthetic coordinates, and the parameters."""
    from hept_amd.prep import get_regions, prepare_input_src

    g = torch.Generator().manual_seed(s.seed)
    x = torch.randn(s.raw, D, generator=g)
    coords = torch.randn(s.raw, s.C, generator=g) * asw.COORD_SCALE
    regions = get_regions(max(4, s.N // (2 * s.B)), s.T, H, generator=g)
    x_p, kw = prepare_input_src(x, coords, {"block_size": s.B, "regions": regions})
    assert x_p.shape[0] == s.N and kw["raw_size"] == s.raw
    if s.later:
        # a later layer: the padding rows hold what the block before wrote into them (residual + feed-forward)
        x_p = x_p.clone()
        x_p[s.raw:] = torch.randn(s.N - s.raw, D, generator=g)
    eta, phi = kw["region_indices"]
    return dict(x=x_p.contiguous(), coords=kw["coords"].contiguous(), raw_size=s.raw, eta=eta.float().contiguous(),
                phi=phi.float().contiguous(), regions_h=kw["regions_h"].float().contiguous(), params=params(s))


def _gpu(inp, dev):
    out = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items() if k != "params"}
    out["params"] = {k: v.to(dev) for k, v in inp["params"].items()}
    return out


def kwargs_of(g, coords=None):
    """The block's forward kwargs, as ``prepare_input_src`` returns them."""
    return {"raw_size": g["raw_size"], "coords": g["coords"] if coords is None else coords,
            "region_indices": [g["eta"], g["phi"]], "regions_h": g["regions_h"]}


def module(s, inp, precision, dev):
    """``SrcAttn`` of the shape with the shape's parameters (precision: an ops precision)."""
    from hept_amd import SrcAttn

    blk = SrcAttn("hept", s.C, precision=precision, h_dim=D, num_heads=H, block_size=s.B, n_hashes=s.T,
                  num_w_per_dist=K, pe_type="none")
    blk.load_state_dict(inp["params"], strict=True)
    return blk.to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# GPU checks (imports deferred: the CPU suite imports this module without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
def staged(s, g, precision):
    """The src block as its kernels: prep_hash_fused(raw_size) -> sort_tables_src (chunks of MAX_TABLES tables, rows
    reused) -> block_attn -> combine_ffn.  Checks that the padding rows hash to +inf and that every chunk's
    permutations are torch's stable sort of the GPU's own keys (hash + geo shift)."""
    import hept_oracle as ho
    from hept_amd import ops

    prec, f32_mfma, _ = PRECISIONS[precision]
    p, n, raw = g["params"], s.N, g["raw_size"]
    sqrt_w = ops.rpe_scale(p["w_rpe.weight"], H, D, K)
    eta, phi, cfac = ops.geo_args((g["eta"], g["phi"]), g["regions_h"], s.T, H, n)
    rows, qs, ks = None, [], []
    for c0 in range(0, s.T, MAX_TABLES):
        tc = min(MAX_TABLES, s.T - c0)
        ph = ops.prep_hash_fused(g["x"], p["norm1.weight"], p["norm1.bias"], EPS, p["w_q.weight"], p["w_k.weight"],
                                 p["w_v.weight"], g["coords"], sqrt_w, p["attn.e2lsh.alpha"], None, prec, t0=c0, tl=tc,
                                 raw_size=raw, rows=rows)
        rows = (ph["qhat"], ph["kvhat"])
        qp, kp = ops.sort_tables_src(ph["qproj"], ph["kproj"], eta, phi, cfac, ph["minmax"], t0=c0)
        mm = ph["minmax"].cpu()
        span = (mm[..., 1].amax(-1) - mm[..., 0].amin(-1))[..., None]
        r0, r1 = c0 * H, (c0 + tc) * H
        shift = ho.geo_shift(g["regions_h"][:, r0:r1].cpu(), span, (g["eta"][r0:r1].cpu(), g["phi"][r0:r1].cpu()), tc)
        for pos, proj in ((qp, ph["qproj"].cpu()), (kp, ph["kproj"].cpu())):
            assert bool(torch.isinf(proj[..., raw:]).all()) and bool(torch.isfinite(proj[..., :raw]).all()), (s.id, c0)
            assert torch.equal(pos.long().cpu(), torch.sort(proj + shift, dim=-1, stable=True).indices), \
                (s.id, precision, c0)
        qs.append(qp)
        ks.append(kp)
    qpos, kpos = torch.cat(qs), torch.cat(ks)
    part = ops.block_attn(rows[0], rows[1], qpos, kpos, D, s.B, f32_mfma=f32_mfma)
    y = ops.combine_ffn(part, D, p["attn.out_linear.weight"], p["attn.out_linear.bias"], g["x"], p["norm2.weight"],
                        p["norm2.bias"], EPS, p["ff.0.weight"], p["ff.0.bias"], p["ff.2.weight"], p["ff.2.bias"])
    return dict(y=y, part=part, qpos=qpos, kpos=kpos)


def one_call(s, g, precision, workspace=None):
    from hept_amd import ops

    return ops.attn_block_forward_src(g["x"], g["coords"], (g["eta"], g["phi"]), g["regions_h"], g["raw_size"],
                                      g["params"], num_heads=H, block_size=s.B, w_per_dist=K, eps1=EPS, eps2=EPS,
                                      precision=PRECISIONS[precision][0], workspace=workspace)


def geo(inp):
    return dict(raw_size=inp["raw_size"], region_indices=(inp["eta"], inp["phi"]), regions_h=inp["regions_h"])


def oracle64(s, inp, qp, kp, **kw):
    import hept_oracle as ho

    p64 = {k: v.double() for k, v in inp["params"].items()}
    return ho.attn_block(inp["x"].double(), inp["coords"].double(), None, p64, num_heads=H, block_size=s.B,
                         w_per_dist=K, eps=EPS, q_positions=qp, k_positions=kp, geo=geo(inp), **kw)


def reference(s, inp, qpos, kpos):
    """float64 src block on the GPU permutations (cached per permutation pair), with the conditioning check."""
    from shape_sweep import _cache

    qp, kp = qpos.long().cpu(), kpos.long().cpu()
    for r in (v for key, v in _cache.items() if key != "shape" and key[1] == "src64"):
        if torch.equal(r["q_positions"], qp) and torch.equal(r["k_positions"], kp):
            return r
    r = oracle64(s, inp, qp, kp, keep=False)
    total = r["denom"].sum(0).squeeze(-1)          # (H, N): every table's weight of the row
    ill = int((total < ILL_WEIGHT).any(0).sum())
    assert ill == 0, f"{s.id}: {ill} rows with total weight < {ILL_WEIGHT}: rescale the shape"
    r = dict(y=r["y"], aggr=r["aggr"], q_positions=qp, k_positions=kp)
    _cache[(s.id, "src64", len(_cache))] = r
    return r


def check_forward(s, precision, dev, note=lambda k, v: None):
    """The one-call src block and ``SrcAttn.eval()`` bit-identical to the staged kernels; every element of y (padding
    rows included) against float64 on the GPU's permutations, within attn_sweep's bounds."""
    from hept_amd import ops

    prec = PRECISIONS[precision][0]
    inp = _cached((s.id, "inp"), lambda: inputs(s))
    g = _cached((s.id, "gpu"), lambda: _gpu(inp, dev))
    blk = module(s, inp, prec, dev).eval()
    with asw._diff_mfma(precision), torch.no_grad():
        st = staged(s, g, precision)
        one = one_call(s, g, precision)
        assert blk._fused_ok(g["x"])
        mod = blk(g["x"], kwargs_of(g))
        torch.cuda.synchronize()
    y = st["y"].cpu()
    assert bool(torch.isfinite(y).all()), (s.id, precision)
    assert torch.equal(one.cpu(), y), f"{s.id} {precision}: one-call src block differs from the staged kernels"
    assert torch.equal(mod.cpu(), y), f"{s.id} {precision}: SrcAttn.eval() differs from the staged kernels"
    wide = ops.unpack_part(st["part"])
    assert bool((wide[..., D] > 0).all()), (s.id, precision)
    ref = reference(s, inp, st["qpos"], st["kpos"])
    if prec.startswith("fp32"):
        err = (y.double() - ref["y"]).abs()
        x = float((err / (ATOL + RTOL * ref["y"].abs())).max())
        note("x", x)
        where = [tuple(i) for i in (err > ATOL + RTOL * ref["y"].abs()).nonzero()[:5].tolist()]
        assert x <= 1.0, f"{s.id} {precision}: worst element {x:.3f}x the tolerance, first (row, col): {where}"
        return dict(x=x)
    w64 = asw._row16(y, ref)
    note("row64", w64)
    assert w64 <= ROW16_64[prec], f"{s.id} {precision}: worst row error vs float64 {w64:.3e} of the row's |aggr|"
    return dict(row64=w64)


# Clouds whose last block holds ONE real point among B - 1 padding rows ("single", "one-in-last-block"): that point's
# dq, dk are a weighted sum over the block's keys whose -q^ terms cancel exactly (the weights' sum of g.(v_j - out) is
# zero), and with one real row a weight gradient row such as w_q.weight's is rank one, so the per-row measure (floor
# 1e-2 of the tensor's max) sees that cancellation's round-off directly.  Those gradients are held to their own per-row
# bound there, about twice the measured worst (fp32 tiles 4.0e-4 w_q.weight at n33-single-b33-t1-c2-later, f32-MFMA
# tiles 4.3e-4 and bf16 tiles 0.81 w_rpe.weight at n768-one-in-last-block-b256-t1-c2; bf16 w_q.weight 0.42 at
# n100-single-b100-t3-c6); per-tensor bounds stay those of attn_sweep
PAD_ROW = {"fp32": 9e-4, "fp32_mfma": 9e-4, "bf16": 1.7}
PAD_ROW_GRADS = ("w_q.weight", "w_k.weight", "w_v.weight", "w_rpe.weight", "coords")


def row_bound(s, nm, mode):
    if raw_kind(s) in ("single", "one-in-last-block") and nm in PAD_ROW_GRADS:
        return max(PAD_ROW[mode], (TRAIN_ROW_CANCEL if nm in CANCEL else TRAIN_ROW)[mode])
    return (TRAIN_ROW_CANCEL if nm in CANCEL else TRAIN_ROW)[mode]


def _fused_node_ran(y):
    """Whether HeptPartialSumsFused is in y's autograd graph."""
    seen, todo = {}, [y.grad_fn]     # (seen holds the nodes: a freed node's id could be handed to another one)
    while todo:
        fn = todo.pop()
        if fn is None or id(fn) in seen:
            continue
        seen[id(fn)] = fn
        if type(fn).__name__ == "HeptPartialSumsFusedBackward":
            return True
        todo.extend(f for f, _ in fn.next_functions)
    return False


def train_once(s, inp, g, mode, dev):
    """SrcAttn.train() with dropout 0: y and the gradients of x, coords and every parameter that receives one."""
    prec, tiles = TRAIN[mode]
    blk = module(s, inp, prec, dev).train()
    blk.dropout.p = 0.0
    blk.attn.train_tiles = tiles
    x = g["x"].clone().requires_grad_(True)
    coords = g["coords"].clone().requires_grad_(True)
    kw = kwargs_of(g, coords)
    assert blk.attn._train_fused_ok(x, kw)
    y = blk(x, kw)
    assert _fused_node_ran(y), f"{s.id} {mode}: the fused training node did not run"
    y.backward(asw._g_out(y.shape).to(dev))
    got = {nm: p.grad.detach().cpu() for nm, p in blk.named_parameters() if p.grad is not None}
    assert set(got) == set(GRAD_PARAMS), sorted(set(got) ^ set(GRAD_PARAMS))
    got.update(y=y.detach().cpu(), x=x.grad.detach().cpu(), coords=coords.grad.detach().cpu())
    return got


def grads64(s, inp, qp, kp):
    """float64 autograd of the reference's src block on the given permutations."""
    import hept_oracle as ho

    p64 = {k: v.double().requires_grad_(k in GRAD_PARAMS) for k, v in inp["params"].items()}
    x = inp["x"].double().requires_grad_(True)
    coords = inp["coords"].double().requires_grad_(True)
    res = ho.attn_block(x, coords, None, p64, num_heads=H, block_size=s.B, w_per_dist=K, eps=EPS, q_positions=qp,
                        k_positions=kp, keep=False, grad=True, geo=geo(inp))
    res["y"].backward(asw._g_out(res["y"].shape).double())
    want = {k: p64[k].grad for k in GRAD_PARAMS}
    want.update(y=res["y"].detach(), x=x.grad, coords=coords.grad)
    return want


def check_backward(s, mode, dev, note=lambda k, v: None):
    """Every gradient of the src training block against float64 autograd on the GPU's permutations, per tensor and
    per row, with attn_sweep's bounds."""
    inp = _cached((s.id, "inp"), lambda: inputs(s))
    g = _cached((s.id, "gpu"), lambda: _gpu(inp, dev))
    st = _cached((s.id, "perm"), lambda: staged(s, g, "fp32"))
    qp, kp = st["qpos"].long().cpu(), st["kpos"].long().cpu()
    want = _cached((s.id, "grads64"), lambda: grads64(s, inp, qp, kp))
    got = train_once(s, inp, g, mode, dev)
    worst_t, worst_r = {}, {}
    for nm, r in want.items():
        a = got[nm]
        assert bool(torch.isfinite(a).all()), (s.id, mode, nm)
        worst_t[nm] = float((a.double() - r).abs().max()) / (float(r.abs().max()) + 1e-300)
        worst_r[nm] = row_x(a, r)
        note(f"{nm} tensor", worst_t[nm])
        note(f"{nm} row", worst_r[nm])
    if mode != "bf16":
        y_x = float(((got["y"].double() - want["y"]).abs() / (ATOL + RTOL * want["y"].abs())).max())
        note("y x", y_x)
        assert y_x <= 1.0, f"{s.id} {mode}: training forward, worst element {y_x:.3f}x the fp32 tolerance"
    bad = {nm: w for nm, w in worst_t.items() if w > TRAIN_TENSOR[mode]}
    assert not bad, f"{s.id} {mode}: per-tensor errors over {TRAIN_TENSOR[mode]}: {bad}"
    grads = {nm: w for nm, w in worst_r.items() if nm != "y"}
    rbad = {nm: w for nm, w in grads.items() if w > row_bound(s, nm, mode)}
    assert not rbad, f"{s.id} {mode}: per-row errors over the bound: {rbad}"
    return dict(tensor=max(w for nm, w in worst_t.items() if nm != "y"), row=max(grads.values()))
