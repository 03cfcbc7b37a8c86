"""bf16 / fp16 query, key, value read natively by the row builder and the v-row riders.

Every bf16 and every fp16 value is a float32 value, so the yardstick throughout is the float32-input path of the SAME
call on ``x.float()`` and the criterion is ``torch.equal``: no tolerance appears anywhere.  (That path is what the rest
of the suite pins to the reference.)  Inputs are N(0, 1) draws rounded to the 16-bit type with about 1 % of the entries
overwritten by -0.0, +-the largest value below 8 and, for fp16, subnormals (6e-8 .. 6e-5)."""
import functools

import pytest
import torch

from hept_amd import HEPTAttention, _lib, ops
from hept_amd.synthetic import make_inputs, make_inputs_src
from shape_sweep import MAX_TABLES, SMALL_CAP, TUNED, direct_v, riders

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
TILES = ("fp32", "bf16", "mixed16")
ALL_PRECISIONS = ("fp32", "fp32_mfma", "fp32_diff", "bf16", "mixed16")


def _round16(x, dt, seed):
    """x rounded to dt, ~1 % of the entries replaced by the special values (no inf, no NaN)."""
    g = torch.Generator().manual_seed(seed)
    flat = x.to(dt).reshape(-1).clone()
    n = flat.numel()
    idx = torch.randperm(n, generator=g)[:max(8, n // 100)]
    big = (torch.tensor([8.0], dtype=dt).view(torch.int16) - 1).view(dt)   # the largest value below 8
    pool = [torch.tensor([-0.0], dtype=dt), big, -big]
    if dt is torch.float16:
        bits = torch.randint(1, 0x400, (64,), generator=g, dtype=torch.int16)   # every fp16 subnormal exponent
        sub = bits.view(dt)
        assert 5.9e-8 <= float(sub.float().min()) and float(sub.float().max()) < 6.2e-5
        pool += [sub, -sub]
        pool.append(torch.tensor([1, 0x3FF], dtype=torch.int16).view(dt))       # the smallest and the largest
    vals = torch.cat(pool)
    flat[idx] = vals[torch.arange(idx.numel()) % vals.numel()]
    out = flat.reshape(x.shape)
    assert bool(torch.isfinite(out.float()).all())
    return out


def _bits(t):
    """Bit patterns (row buffers hold f32 words inside 16-bit tagged tensors: compare them as integers)."""
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@functools.lru_cache(maxsize=16)
def _example(sizes, b, t, h, d, c, seed=3):
    inp = make_inputs(list(sizes), block_size=b, n_hashes=t, coords_dim=c, h_dim=d, num_heads=h, seed=seed)
    inp["q"], inp["k"], inp["coords"] = inp["q"] * 0.3, inp["k"] * 0.3, inp["coords"] * 0.2
    return inp


@functools.lru_cache(maxsize=4)
def _src(raw, b, t, seed=5):
    return make_inputs_src(raw, block_size=b, n_hashes=t, seed=seed, qk_scale=0.3, coords_scale=0.2)


def _qkv16(inp, dt, dev):
    return [_round16(inp[x], dt, s).to(dev) for s, x in enumerate(("q", "k", "v"))]


def _gpu(inp, dev, *names):
    return [inp[x].to(dev) for x in names]


# ---- 1, 2: stage level -------------------------------------------------------------------------------------------------
def _check_prep(inp, h, d, c, tile, dt, dev, raw_size=None, codes=True):
    q, k, v = _qkv16(inp, dt, dev)
    coords, w, alpha = _gpu(inp, dev, "coords", "w_rpe_weight", "alpha")
    cs = inp["combined_shifts"].to(dev) if codes else None
    sw = ops.rpe_scale(w, h, d, 10)
    got = ops.prep_hash(q, k, v, coords, sw, alpha, cs, tile, raw_size=raw_size)
    want = ops.prep_hash(q.float(), k.float(), v.float(), coords, sw, alpha, cs, tile, raw_size=raw_size)
    torch.cuda.synchronize()
    for nm in ("qhat", "kvhat", "qproj", "kproj"):
        assert got[nm].dtype == want[nm].dtype and torch.equal(_bits(got[nm]), _bits(want[nm])), nm
    # the reduced hash range (and the code maximum that scales the sort's bucket ids)
    for mm_g, mm_w in ((got["minmax"], want["minmax"]),):
        assert torch.equal(mm_g[..., 0].amin(-1), mm_w[..., 0].amin(-1))
        assert torch.equal(mm_g[..., 1].amax(-1), mm_w[..., 1].amax(-1))
        assert torch.equal(mm_g[..., 2].amax(-1), mm_w[..., 2].amax(-1))
    return got


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("d,c", TUNED)
def test_tuned_row_builder_reads_16bit_rows(d, c, tile, dt, gpu_device):
    """N = 100: 12 full tiles of 8 points and one of 4 (the valid-pieces mask of the tile load)."""
    inp = _example((100,), 20, 3, 8, d, c)
    assert inp["q"].shape[0] == 100 and (d, c) in TUNED
    _check_prep(inp, 8, d, c, tile, DTYPES[dt], gpu_device)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("h,d,c", [(3, 5, 3), (16, 27, 3), (12, 8, 4)])
def test_generic_row_builder_reads_16bit_rows(h, d, c, tile, dt, gpu_device):
    """(3, 5, 3): a row stride of 30 bytes; (12, 8, 4): D % 4 == 0 without being a tuned shape."""
    assert not (h == 8 and (d, c) in TUNED)
    inp = _example((96,), 32, 2, h, d, c)
    assert inp["q"].shape[0] == 96
    _check_prep(inp, h, d, c, tile, DTYPES[dt], gpu_device)


# ---- 3: the whole operator ---------------------------------------------------------------------------------------------
# id: (sizes, B, T, H, D, C, precisions)
CASES = {
    "a-one-launch-sort": ((512,), 128, 3, 8, 24, 6, ALL_PRECISIONS),
    "b-riders": ((6400,), 128, 2, 8, 24, 6, ("fp32", "bf16", "mixed16")),
    "c-v-role-long-cloud": ((6400,), 128, 1, 8, 24, 6, ("bf16",)),
    "d-riders-8B-source": ((6400,), 128, 2, 12, 12, 4, ("fp32", "bf16")),
    "e-direct-v-shape": ((512,), 256, 2, 8, 24, 6, ("fp32",)),
    "f-table-chunks": ((256,), 64, 9, 8, 24, 6, ("fp32", "bf16")),
    # the riders' 1.0 at column D in the second quad of piece 0, with a run-time head count (rows_sweep.TWO_ROLE_COLUMN_D;
    # D = 28 is refused by hept_check_shape)
    "g-riders-d4": ((10912,), 32, 2, 3, 4, 3, ("fp32", "bf16", "mixed16")),
}


def _branch_checks(name, n, b, t, h, d, c, precision):
    if name.startswith("a-"):
        assert n <= SMALL_CAP and not riders(n, h, d, t, precision, b) and not direct_v(d, precision, b)
    elif name.startswith("b-"):
        assert riders(n, h, d, t, precision, b) and h == 8 and (d, c) in TUNED
    elif name.startswith("c-"):
        assert n > SMALL_CAP and not riders(n, h, d, t, precision, b) and not direct_v(d, precision, b)
    elif name.startswith("d-"):
        assert riders(n, h, d, t, precision, b) and d % 4 == 0 and (d * 2) % 16 == 8   # head rows start at 8-byte steps
    elif name.startswith("g-"):
        assert riders(n, h, d, t, precision, b) and (h, d) == (3, 4)
    elif name.startswith("e-"):
        assert direct_v(d, precision, b)      # what the f32 inputs take; 16-bit inputs must fall back to built rows
    elif name.startswith("f-"):
        assert t > MAX_TABLES


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,precision", [(nm, p) for nm, cs in CASES.items() for p in cs[-1]])
def test_forward_on_16bit_inputs_equals_forward_on_widened(name, precision, dt, gpu_device):
    sizes, b, t, h, d, c, _ = CASES[name]
    inp = _example(sizes, b, t, h, d, c)
    n = inp["q"].shape[0]
    assert n == sum(sizes)
    _branch_checks(name, n, b, t, h, d, c, precision)
    dev = gpu_device
    q, k, v = _qkv16(inp, DTYPES[dt], dev)
    rest = _gpu(inp, dev, "coords", "combined_shifts", "w_rpe_weight", "alpha", "out_weight", "out_bias")
    kw = dict(block_size=b, w_per_dist=10, precision=precision)
    got = ops.forward(q, k, v, *rest, **kw)
    want = ops.forward(q.float(), k.float(), v.float(), *rest, **kw)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and bool(torch.isfinite(want).all())
    assert torch.equal(got, want)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,precision", [(512, "fp32"), (512, "bf16"), (512, "mixed16"), (6400, "fp32"), (6400, "bf16")])
def test_forward_src_on_16bit_inputs_with_padding_rows(n, precision, dt, gpu_device):
    """src variant, raw_size = N - 37: the padding rows are zero rows whatever q, k, v hold there."""
    b, t = 128, 2
    inp = _src(n - 37, b, t)
    assert inp["q"].shape[0] == n and inp["raw_size"] == n - 37
    assert riders(n, 8, 24, t, precision, b) == (n > SMALL_CAP)
    dev = gpu_device
    q, k, v = _qkv16(inp, DTYPES[dt], dev)
    coords, eta, phi, rh, w, alpha, ow, ob = _gpu(inp, dev, "coords", "eta_idx", "phi_idx", "regions_h", "w_rpe_weight",
                                                  "alpha", "out_weight", "out_bias")
    kw = dict(block_size=b, w_per_dist=10, precision=precision)
    got = ops.forward_src(q, k, v, coords, (eta, phi), rh, n - 37, w, alpha, ow, ob, **kw)
    want = ops.forward_src(q.float(), k.float(), v.float(), coords, (eta, phi), rh, n - 37, w, alpha, ow, ob, **kw)
    assert torch.equal(got, want)
    if n == 512:   # the rows themselves: equal before raw_size; from there on q^ = k^ = v = 0 whatever the inputs hold,
        # and the v half keeps the 1.0 of column D that every row carries (the float32 path writes it there as well)
        rows = _check_prep(inp, 8, 24, 6, precision, DTYPES[dt], dev, raw_size=n - 37, codes=False)
        pad_kv = rows["kvhat"][:, n - 37:]
        v_half = pad_kv[..., 32:]
        if precision == "mixed16":   # (the buffer is tagged fp16 for its k^ half: the v half holds bf16)
            v_half = v_half.view(torch.bfloat16)
        want_v = torch.zeros(32, device=dev)
        want_v[24] = 1.0
        assert torch.equal(v_half.float(), want_v.expand(8, 37, 32))
        assert float(pad_kv[..., :32].float().abs().max()) == 0.0
        assert float(rows["qhat"][:, n - 37:].float().abs().max()) == 0.0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("precision,packed", [("fp32", False), ("bf16", True)])
def test_forward_partial_on_16bit_inputs(precision, packed, dt, gpu_device):
    sizes, b, t, h, d, c, _ = CASES["a-one-launch-sort"]
    inp = _example(sizes, b, t, h, d, c)
    dev = gpu_device
    q, k, v = _qkv16(inp, DTYPES[dt], dev)
    coords, cs, w, alpha = _gpu(inp, dev, "coords", "combined_shifts", "w_rpe_weight", "alpha")
    kw = dict(block_size=b, w_per_dist=10, t0=1, tl=2, precision=precision, packed=packed)
    assert torch.equal(ops.forward_partial(q, k, v, coords, cs, w, alpha, **kw),
                       ops.forward_partial(q.float(), k.float(), v.float(), coords, cs, w, alpha, **kw))
    s = _src(512 - 37, 128, 2)
    q, k, v = _qkv16(s, DTYPES[dt], dev)
    coords, eta, phi, rh, w, alpha = _gpu(s, dev, "coords", "eta_idx", "phi_idx", "regions_h", "w_rpe_weight", "alpha")
    kw.update(t0=0, tl=1)
    assert torch.equal(ops.forward_partial_src(q, k, v, coords, (eta, phi), rh, 512 - 37, w, alpha, **kw),
                       ops.forward_partial_src(q.float(), k.float(), v.float(), coords, (eta, phi), rh, 512 - 37, w,
                                               alpha, **kw))


# ---- 4: the module -----------------------------------------------------------------------------------------------------
def _module(inp, dev, variant, precision, b, t):
    h, e, _ = inp["alpha"].shape
    m = HEPTAttention(e, variant=variant, h_dim=24, num_heads=h, block_size=b, n_hashes=t, num_w_per_dist=10,
                      precision=precision)
    sd = {"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"], "e2lsh.alpha": inp["alpha"]}
    if variant == "src":
        sd["e2lsh.beta"] = torch.zeros(1, t)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    w_rpe = torch.nn.Linear(inp["w_rpe_weight"].shape[1], inp["w_rpe_weight"].shape[0]).to(dev)
    with torch.no_grad():
        w_rpe.weight.copy_(inp["w_rpe_weight"])
    if variant == "src":
        kw = dict(raw_size=inp["raw_size"], regions_h=inp["regions_h"].to(dev),
                  region_indices=[inp["eta_idx"].to(dev), inp["phi_idx"].to(dev)])
    else:
        kw = dict(combined_shifts=inp["combined_shifts"].to(dev))
    return m, dict(w_rpe=w_rpe, coords=inp["coords"].to(dev), **kw)


def _module_inputs(variant, n=2048, b=128, t=3):
    return _src(n - 37, b, t) if variant == "src" else _example((n,), b, t, 8, 24, 6)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["example", "src"])
def test_module_takes_16bit_inputs_without_float32_copies(variant, precision, dt, gpu_device):
    dev, n = gpu_device, 2048
    inp = _module_inputs(variant)
    m, kw = _module(inp, dev, variant, precision, 128, 3)
    q, k, v = _qkv16(inp, DTYPES[dt], dev)
    with torch.no_grad():
        want = m(q.float(), k.float(), v.float(), **kw).to(q.dtype)
        m.reserve(n, 6, dev)
        m(q, k, v, **kw)                                   # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        got = m(q, k, v, **kw)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        assert got.dtype == q.dtype and torch.equal(got, want)
        # one float32 copy of query alone would be N * H * D * 4 bytes (the widening path makes three)
        assert peak < n * 8 * 24 * 4, f"forward allocated {peak} bytes above the level before the call"
        # (N, H, D) inputs: the reshape is a view
        got3 = m(q.view(n, 8, 24), k.view(n, 8, 24), v.view(n, 8, 24), **kw)
        assert torch.equal(got3, want)


def test_module_mixed_dtypes_take_the_widening_path(gpu_device):
    dev = gpu_device
    inp = _module_inputs("example")
    m, kw = _module(inp, dev, "example", "bf16", 128, 3)
    q = _round16(inp["q"], torch.bfloat16, 0).to(dev)
    k = _round16(inp["k"], torch.float16, 1).to(dev)
    v = inp["v"].to(dev)
    with torch.no_grad():
        got = m(q, k, v, **kw)
        want = m(q.float(), k.float(), v, **kw).to(q.dtype)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)


def test_module_training_with_bf16_inputs_keeps_its_gradients(gpu_device):
    """The training path widens in torch, as before: the gradients of bf16 leaves are the float32 path's, rounded."""
    dev = gpu_device
    inp = _example((512,), 128, 3, 8, 24, 6)
    m, kw = _module(inp, dev, "example", "fp32", 128, 3)
    m.train()
    q16, k16, v16 = _qkv16(inp, torch.bfloat16, dev)
    # (representable in bf16: the bf16 output's cast rounds the incoming gradient, and that is not what is compared)
    g_out = torch.randn(512, 24, generator=torch.Generator().manual_seed(9)).bfloat16().float().to(dev)
    grads = []
    for leaves in ([q16, k16, v16], [q16.float(), k16.float(), v16.float()]):
        leaves = [x.detach().clone().requires_grad_(True) for x in leaves]
        m.zero_grad()
        kw["w_rpe"].zero_grad()
        out = m(*leaves, **kw)
        out.float().backward(g_out)
        grads.append([x.grad for x in leaves] + [kw["w_rpe"].weight.grad.clone(), m.out_linear.weight.grad.clone()])
    for got, want in zip(*grads):
        assert torch.equal(got, want.to(got.dtype))
    assert grads[0][0].dtype == torch.bfloat16


@pytest.mark.parametrize("variant", ["example", "src"])
def test_module_under_torch_compile_passes_16bit_inputs_through(variant, gpu_device):
    import torch._dynamo

    inp = _module_inputs(variant)
    m, kw = _module(inp, gpu_device, variant, "bf16", 128, 3)
    q, k, v = _qkv16(inp, torch.bfloat16, gpu_device)

    def run(mod):
        with torch.no_grad():
            return mod(q, k, v, **kw)

    eager = run(m)
    torch._dynamo.reset()
    out = run(torch.compile(m, backend="aot_eager", fullgraph=True))
    assert out.dtype == torch.bfloat16 and torch.equal(out, eager)


# ---- 5: refusals -------------------------------------------------------------------------------------------------------
def test_mixed_16bit_dtypes_are_a_type_error(gpu_device):
    inp = _example((512,), 128, 3, 8, 24, 6)
    dev = gpu_device
    rest = _gpu(inp, dev, "coords", "combined_shifts", "w_rpe_weight", "alpha", "out_weight", "out_bias")
    q = inp["q"].to(dev)
    with pytest.raises(TypeError, match="bfloat16.*float16.*bfloat16"):
        ops.forward(q.bfloat16(), q.half(), q.bfloat16(), *rest, block_size=128, w_per_dist=10)
    with pytest.raises(TypeError, match="must be float32"):
        ops.forward(q.double(), q.double(), q.double(), *rest, block_size=128, w_per_dist=10)


def test_misaligned_16bit_base_is_repaired_by_ops_and_refused_by_the_c_call(gpu_device):
    inp = _example((512,), 128, 3, 8, 24, 6)
    dev, n, hd = gpu_device, 512, 192
    q, k, v = _qkv16(inp, torch.bfloat16, dev)
    big = torch.zeros(n * hd + 8, dtype=torch.bfloat16, device=dev)
    assert big.data_ptr() % 16 == 0
    q_off = big[1:1 + n * hd].view(n, hd)                 # a contiguous view two bytes into the buffer
    q_off.copy_(q)
    assert q_off.is_contiguous() and q_off.data_ptr() % 16 == 2
    coords, cs, w, alpha, ow, ob = _gpu(inp, dev, "coords", "combined_shifts", "w_rpe_weight", "alpha", "out_weight",
                                        "out_bias")
    kw = dict(block_size=128, w_per_dist=10, precision="bf16")
    assert torch.equal(ops.forward(q_off, k, v, coords, cs, w, alpha, ow, ob, **kw),
                       ops.forward(q, k, v, coords, cs, w, alpha, ow, ob, **kw))
    lib = _lib.load()
    ws = torch.empty(ops.workspace_bytes(n, 8, 24, 6, 3, 128, "bf16"), dtype=torch.uint8, device=dev)
    out = torch.empty(n, 24, device=dev)
    st = ops.current_stream_ptr(torch.device(dev))

    def call(qq, in_dtype):
        return lib.hept_forward_in(qq.data_ptr(), k.data_ptr(), v.data_ptr(), in_dtype, coords.data_ptr(), cs.data_ptr(),
                                   w.data_ptr(), alpha.data_ptr(), ow.data_ptr(), ob.data_ptr(), n, 8, 24, 6, 10, 3, 128,
                                   _lib.PREC_BF16, ws.data_ptr(), ws.numel(), out.data_ptr(), st)

    assert call(q_off, ops.IN_BF16) == 3                  # HEPT_ERR_ARG, before any launch
    assert call(q, 7) == 3                                # an unknown element type
    assert call(q, ops.IN_BF16) == 0
    torch.cuda.synchronize()
