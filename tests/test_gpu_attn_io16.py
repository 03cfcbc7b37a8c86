"""The fused Attn block on bfloat16 / float16 activations: ``x`` read and ``y`` written in the 16-bit type by the row
builder and the combine epilogue themselves (``hept_prep_hash_fused_in``, ``hept_combine_ffn_io``,
``hept_attn_block_forward_io`` / ``_src_io``).

Every bf16 and every fp16 value is a float32 value and the float32 result is rounded once on its way out, so the
yardstick throughout is the float32 path of the SAME call on ``x.float()`` followed by ``.to(dtype)`` (that path is what
the rest of the suite pins to the reference), and the criterion is equality of bit patterns: no tolerance appears
anywhere.  Inputs are N(0, 1) draws rounded to the type with about 1 % of the entries overwritten by -0.0, +- the
largest value below 8 and, for fp16, subnormals including the smallest and the largest (tests/io16_inputs.py)."""
import ctypes
import functools

import pytest
import torch

import attn_sweep as asw
import src_attn_sweep as ssw
from attn_sweep import CMB_FLAT_FROM, D, EPS, H, K
from hept_amd import Attn, _lib, ops
from io16_inputs import DTYPES, IO_CODE, bits, partial_rows, round16, same_bits
from shape_sweep import MAX_TABLES, PRECISIONS, SMALL_CAP

pytestmark = pytest.mark.gpu

TILES = ("fp32", "bf16", "mixed16")
ERR_ARG = 3


@functools.lru_cache(maxsize=16)
def _example(sizes, b, t, c, seed=900):
    """CPU inputs of an example-variant block (x float32; the tests round it)."""
    return asw.inputs(asw.Shape("io16", tuple(sizes), b, t, c, seed, False, False))


@functools.lru_cache(maxsize=8)
def _src(n, raw, b, t, c, seed=950):
    return ssw.inputs(ssw.Shape("io16-src", n, raw, b, t, c, True, seed, False))


def _x16(inp, dt, dev, seed=11):
    return round16(inp["x"], dt, seed)[0].to(dev)


def _block(g, x, b, precision, **kw):
    prec, _, _ = PRECISIONS[precision]
    with asw._diff_mfma(precision):
        return ops.attn_block_forward(x, g["coords"], g["combined_shifts"], g["params"], num_heads=H, block_size=b,
                                      w_per_dist=K, eps1=EPS, eps2=EPS, precision=prec, **kw)


def _block_src(g, x, b, precision, **kw):
    prec, _, _ = PRECISIONS[precision]
    return ops.attn_block_forward_src(x, g["coords"], (g["eta"], g["phi"]), g["regions_h"], g["raw_size"], g["params"],
                                      num_heads=H, block_size=b, w_per_dist=K, eps1=EPS, eps2=EPS, precision=prec, **kw)


# ---- 1: the fused row builder ----------------------------------------------------------------------------------------
def _check_prep(x16, p, coords, codes, tile, t, raw_size=None):
    sw_ = ops.rpe_scale(p["w_rpe.weight"], H, D, K)
    args = (p["norm1.weight"], p["norm1.bias"], EPS, p["w_q.weight"], p["w_k.weight"], p["w_v.weight"], coords, sw_,
            p["attn.e2lsh.alpha"], codes, tile)
    got = ops.prep_hash_fused(x16, *args, raw_size=raw_size)
    want = ops.prep_hash_fused(x16.float(), *args, raw_size=raw_size)
    torch.cuda.synchronize()
    for nm in ("qhat", "kvhat", "qproj", "kproj"):
        assert same_bits(got[nm], want[nm]), nm
    mm_g, mm_w = got["minmax"], want["minmax"]     # the reduced hash range and the code maximum, as test_gpu_in16
    assert torch.equal(mm_g[..., 0].amin(-1), mm_w[..., 0].amin(-1))
    assert torch.equal(mm_g[..., 1].amax(-1), mm_w[..., 1].amax(-1))
    assert torch.equal(mm_g[..., 2].amax(-1), mm_w[..., 2].amax(-1))
    assert got["qproj"].shape[0] == t


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("t", [3, 5])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("c", [6, 4, 2])
def test_fused_row_builder_reads_16bit_rows(c, tile, t, dt, gpu_device):
    """N = 100: 12 full tiles of 8 points and one of 4 (the ``live ? n : n0`` clamp of the row load); T = 3 / 5: the
    kernel instances with 4 and 8 table slots."""
    inp = _example((100,), 20, t, c)
    assert inp["x"].shape == (100, D) and asw.tmax(t) == (4 if t == 3 else MAX_TABLES)
    g = asw._gpu(inp, gpu_device)
    _check_prep(_x16(inp, DTYPES[dt], gpu_device), g["params"], g["coords"], g["combined_shifts"], tile, t)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("tile", TILES)
def test_fused_row_builder_src_padding_rows(tile, dt, gpu_device):
    """The src variant with raw_size = 90 < N = 100: the padding rows (zero rows, hash +inf) from 16-bit input."""
    inp = _src(100, 90, 20, 3, 6)
    assert inp["x"].shape == (100, D) and inp["raw_size"] == 90
    g = ssw._gpu(inp, gpu_device)
    _check_prep(_x16(inp, DTYPES[dt], gpu_device), g["params"], g["coords"], None, tile, 3, raw_size=90)


# ---- 2: the combine epilogue -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _ffn_params(seed=31):
    return asw.default_params(6, 3, seed)


def _ffn(part, p, x, **kw):
    return ops.combine_ffn(part, D, p["attn.out_linear.weight"], p["attn.out_linear.bias"], x, p["norm2.weight"],
                           p["norm2.bias"], EPS, p["ff.0.weight"], p["ff.0.bias"], p["ff.2.weight"], p["ff.2.bias"], **kw)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("packed", [False, True], ids=["f32-rows", "packed-rows"])
@pytest.mark.parametrize("n,t", [(100, 3), (32780, 2)])
def test_combine_epilogue_reads_and_writes_16bit_rows(n, t, packed, dt, gpu_device):
    """N = 100: three full 32-point tiles and one of 4, and the slice n0 = 32, n_count = 50 (x and y point at row n0, the
    last tile is ragged); N = 32 780: 1024 full tiles + 12 on the flat grid instead of the split one."""
    assert (n >= CMB_FLAT_FROM) == (n == 32780) and n % 32 in (4, 12)
    dev, dtype = gpu_device, DTYPES[dt]
    p = {k: v.to(dev) for k, v in _ffn_params().items()}
    part = partial_rows(t, n, H, 5, packed, dev)
    x16 = round16(torch.randn(n, D, generator=torch.Generator().manual_seed(6)), dtype, 7)[0].to(dev)
    got, want = _ffn(part, p, x16), _ffn(part, p, x16.float())
    assert got.dtype == dtype and want.dtype == torch.float32 and got.shape == (n, D)
    assert same_bits(got, want.to(dtype))
    if n == 100:
        got2 = _ffn(part, p, x16, n0=32, n_count=50)
        assert got2.dtype == dtype and got2.shape == (50, D)
        assert same_bits(got2, _ffn(part, p, x16.float(), n0=32, n_count=50).to(dtype))
        assert same_bits(got2, got[32:82])


# ---- 3: rounding edges -----------------------------------------------------------------------------------------------
def _edge_block(dev, ff2_bias=None):
    """A block whose out_linear and ff.2 are zero: y = (x + 0) + ff.2.bias in float32, exactly."""
    inp = _example((100,), 20, 3, 6)
    g = asw._gpu(inp, dev)
    p = dict(g["params"])
    for nm in ("attn.out_linear.weight", "attn.out_linear.bias", "ff.2.weight", "ff.2.bias"):
        p[nm] = torch.zeros_like(p[nm])
    if ff2_bias is not None:
        p["ff.2.bias"] = ff2_bias.to(dev)
    g["params"] = p
    return inp, g


@pytest.mark.parametrize("dt", DTYPES)
def test_identity_block_reproduces_every_special_value(dt, gpu_device):
    dtype = DTYPES[dt]
    inp, g = _edge_block(gpu_device)
    x16, idx = round16(inp["x"], dtype, 11)
    x16 = x16.to(gpu_device)
    for tile in ("fp32", "bf16"):
        want = _block(g, x16.float(), 20, tile)
        got = _block(g, x16, 20, tile)
        assert torch.equal(want, x16.float())                # the yardstick itself is the identity (x + 0 in float32)
        assert got.dtype == dtype and same_bits(got, want.to(dtype))
        # every special value comes back, subnormals included (x + 0 turns -0.0 into +0.0, in the yardstick as well)
        sp_in, sp_out = x16.reshape(-1)[idx.to(gpu_device)], got.reshape(-1)[idx.to(gpu_device)]
        nonzero = sp_in.float() != 0
        assert int(nonzero.sum()) > 0 and torch.equal(bits(sp_in[nonzero]), bits(sp_out[nonzero]))
        if dtype is torch.float16:
            sub = (sp_in.float().abs() < 2.0 ** -14) & nonzero
            assert int(sub.sum()) >= 4 and torch.equal(bits(sp_in[sub]), bits(sp_out[sub]))
            assert float(sp_out[sub].float().abs().min()) == 2.0 ** -24


@pytest.mark.parametrize("dt", DTYPES)
def test_fp16_overflow_goes_to_inf(dt, gpu_device):
    """ff.2.bias = 7e4 on columns 0, 5, 13, 23 (both lane halves): beyond the largest fp16 -> inf, not 65504."""
    dtype = DTYPES[dt]
    bias = torch.zeros(D)
    bias[[0, 5, 13, 23]] = 7e4
    inp, g = _edge_block(gpu_device, bias)
    x16 = _x16(inp, dtype, gpu_device)
    want = _block(g, x16.float(), 20, "fp32").to(dtype)
    if dtype is torch.float16:
        assert bool(torch.isinf(want[:, [0, 5, 13, 23]]).all()) and bool(torch.isfinite(want[:, 1]).all())
    got = _block(g, x16, 20, "fp32")
    assert got.dtype == dtype and same_bits(got, want)


@pytest.mark.parametrize("dt", DTYPES)
def test_exact_ties_round_to_even(dt, gpu_device):
    """x restricted to multiples of 2^-4 and ff.2.bias = odd multiples of half an ulp of [0.5, 1) (2^-9 for bf16, 2^-12
    for fp16): every result in [0.5, 1) lies exactly half-way between two neighbours of the type."""
    dtype = DTYPES[dt]
    half_ulp, low_mask, low_half = {"bf16": (2.0 ** -9, 0xFFFF, 0x8000), "fp16": (2.0 ** -12, 0x1FFF, 0x1000)}[dt]
    bias = (2 * torch.arange(D) + 1).float() * half_ulp
    inp, g = _edge_block(gpu_device, bias)
    xq = (torch.round(inp["x"] * 16) / 16).clamp(-4, 4)
    x16 = xq.to(dtype).to(gpu_device)
    assert torch.equal(x16.float().cpu(), xq)
    want32 = _block(g, x16.float(), 20, "fp32")
    assert torch.equal(want32.cpu(), xq + bias)              # exact in float32
    w = want32.view(torch.int32)
    tie = ((w & low_mask) == low_half) & (want32.abs() >= 2.0 ** -14)
    kept_odd = ((w >> (low_half.bit_length())) & 1).bool()
    assert int(tie.sum()) >= 100 and int((tie & kept_odd).sum()) >= 1 and int((tie & ~kept_odd).sum()) >= 1
    got = _block(g, x16, 20, "fp32")
    assert got.dtype == dtype and same_bits(got, want32.to(dtype))
    # ties to even: the kept last bit of every tie's result is 0
    assert int((bits(got)[tie] & 1).sum()) == 0


# ---- 4: the whole block at the call level ------------------------------------------------------------------------------
BLOCK_CASES = {
    "a-512": ((512,), 128, 3, tuple(PRECISIONS), ("bf16", "fp16")),
    "b-two-launch-sort": ((6400,), 128, 2, ("fp32", "bf16"), ("bf16", "fp16")),
    "c-table-chunks": ((256,), 64, 10, ("fp32", "bf16"), ("bf16", "fp16")),
}


@pytest.mark.parametrize("name,precision,dt", [(nm, p, dt) for nm, cs in BLOCK_CASES.items() for p in cs[3] for dt in cs[4]])
def test_block_on_16bit_x_equals_block_on_widened_x_rounded(name, precision, dt, gpu_device):
    sizes, b, t, _, _ = BLOCK_CASES[name]
    inp = _example(sizes, b, t, 6)
    n = inp["x"].shape[0]
    assert (n > SMALL_CAP) == name.startswith("b-") and (t > MAX_TABLES) == name.startswith("c-")
    g = asw._gpu(inp, gpu_device)
    dtype = DTYPES[dt]
    x16 = _x16(inp, dtype, gpu_device)
    want = _block(g, x16.float(), b, precision)
    got = _block(g, x16, b, precision)
    assert want.dtype == torch.float32 and got.dtype == dtype and bool(torch.isfinite(want).all())
    assert same_bits(got, want.to(dtype))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("precision", ["fp32", "mixed16"])
def test_src_block_on_16bit_x(precision, dt, gpu_device):
    """raw_size = 1000 padded to 1024: the padding rows are zero inside the operator but still get the residual and the
    feed-forward of their (16-bit) x rows."""
    inp = _src(1024, 1000, 128, 3, 6)
    g = ssw._gpu(inp, gpu_device)
    dtype = DTYPES[dt]
    x16 = _x16(inp, dtype, gpu_device)
    want = _block_src(g, x16.float(), 128, precision)
    got = _block_src(g, x16, 128, precision)
    assert got.dtype == dtype and same_bits(got, want.to(dtype))


# ---- 5: the modules ----------------------------------------------------------------------------------------------------
def _modules(dev, precision="bf16"):
    """(module, forward kwargs, x float32 on the CPU) for Attn and SrcAttn."""
    s = asw.Shape("io16", (512,), 128, 3, 6, 900, False, False)
    inp = _example(s.sizes, s.B, s.T, s.C)
    g = asw._gpu(inp, dev)
    yield "Attn", asw.module(s, inp, precision, dev).eval(), \
        {"coords": g["coords"], "combined_shifts": g["combined_shifts"]}, inp["x"]
    ss = ssw.Shape("io16-src", 1024, 1000, 128, 3, 6, True, 950, False)
    sinp = _src(ss.N, ss.raw, ss.B, ss.T, ss.C)
    yield "SrcAttn", ssw.module(ss, sinp, precision, dev).eval(), ssw.kwargs_of(ssw._gpu(sinp, dev)), sinp["x"]


@pytest.mark.parametrize("dt", DTYPES)
def test_modules_keep_the_dtype_and_equal_the_yardstick(dt, gpu_device):
    dtype = DTYPES[dt]
    for name, blk, kw, x in _modules(gpu_device):
        x16 = round16(x, dtype, 11)[0].to(gpu_device)
        with torch.no_grad():
            want = blk(x16.float(), kw)
            got = blk(x16, kw)
        assert want.dtype == torch.float32 and got.dtype == dtype, name
        assert same_bits(got, want.to(dtype)), name


def test_modules_under_autocast(gpu_device):
    """What a HEPT model does under autocast: the encoder's nn.Linear hands the block a bfloat16 x."""
    for name, blk, kw, x in _modules(gpu_device):
        torch.manual_seed(3)
        enc = torch.nn.Linear(D, D).to(gpu_device)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            x16 = enc(x.to(gpu_device))
            assert x16.dtype == torch.bfloat16
            got = blk(x16, kw)
            want = blk(x16.float(), kw)
        assert got.dtype == torch.bfloat16 and want.dtype == torch.float32, name
        assert same_bits(got, want.to(torch.bfloat16)), name


def test_compiled_module_on_bf16_x_equals_eager(gpu_device):
    import torch._dynamo

    name, blk, kw, x = next(_modules(gpu_device))
    x16 = round16(x, torch.bfloat16, 11)[0].to(gpu_device)
    with torch.no_grad():
        eager = blk(x16, kw)
        torch._dynamo.reset()
        out = torch.compile(blk, backend="aot_eager", fullgraph=True)(x16, kw)
    assert out.dtype == torch.bfloat16 and same_bits(out, eager)


def test_float64_x_still_goes_through_the_widening_path(gpu_device):
    name, blk, kw, x = next(_modules(gpu_device))
    x32 = x.to(gpu_device)
    with torch.no_grad():
        got = blk(x32.double(), kw)
        want = blk(x32, kw)
    assert got.dtype == torch.float64 and torch.equal(got, want.double())


# ---- 6: no float32 temporaries -----------------------------------------------------------------------------------------
def test_no_float32_temporaries(gpu_device):
    """One forward on bfloat16 x allocates less than ONE float32 activation tensor (N x 24 x 4 bytes) above what was
    live before it: the result itself (half of that) and nothing else.  Widening in torch allocates two plus the result."""
    n = 6016
    s = asw.Shape("io16-mem", (n,), 128, 3, 6, 901, False, False)
    inp = _example(s.sizes, s.B, s.T, s.C, s.seed)
    g = asw._gpu(inp, gpu_device)
    blk = asw.module(s, inp, "bf16", gpu_device).eval()
    kw = {"coords": g["coords"], "combined_shifts": g["combined_shifts"]}
    x16 = _x16(inp, torch.bfloat16, gpu_device)
    with torch.no_grad():
        y = blk(x16, kw)                       # warm-up: the workspace is allocated here
        del y
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(gpu_device)
        torch.cuda.reset_peak_memory_stats(gpu_device)
        y = blk(x16, kw)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(gpu_device)
    assert y.dtype == torch.bfloat16
    print(f"peak - before = {peak - before} bytes; one float32 activation tensor = {n * D * 4}")
    assert peak - before < n * D * 4


# ---- 7: refusals -------------------------------------------------------------------------------------------------------
def test_misaligned_view_is_repaired_by_ops_and_refused_by_the_c_call(gpu_device):
    inp = _example((512,), 128, 3, 6)
    g = asw._gpu(inp, gpu_device)
    n = inp["x"].shape[0]
    x16 = _x16(inp, torch.bfloat16, gpu_device)
    big = torch.zeros(n * D + 8, dtype=torch.bfloat16, device=gpu_device)
    assert big.data_ptr() % 16 == 0
    x_off = big[1:1 + n * D].view(n, D)                     # a contiguous view two bytes into the buffer
    x_off.copy_(x16)
    assert x_off.is_contiguous() and x_off.data_ptr() % 16 == 2
    assert same_bits(_block(g, x_off, 128, "bf16"), _block(g, x16, 128, "bf16"))
    # the raw C call on the same view: HEPT_ERR_ARG, before any launch (y stays untouched)
    lib = _lib.load()
    x_ok, coords, st, (n_, h, d, c, t), prec, ws, _keep = ops._block_args(
        x16, g["coords"], g["params"], H, 128, K, EPS, EPS, "bf16", None)
    codes = g["combined_shifts"].contiguous()
    y = torch.full((n, D), 7.0, dtype=torch.bfloat16, device=gpu_device)

    def raw(x_ptr, io, y_ptr):
        return lib.hept_attn_block_forward_io(x_ptr, io, coords.data_ptr(), codes.data_ptr(), ctypes.byref(st), n_, h, d,
                                              c, K, t, 128, prec, ws.data_ptr(), ws.numel(), y_ptr, ops._stream(x16))

    assert raw(x_off.data_ptr(), IO_CODE[torch.bfloat16], y.data_ptr()) == ERR_ARG
    assert raw(x_ok.data_ptr(), IO_CODE[torch.bfloat16], y.data_ptr() + 2) == ERR_ARG
    assert raw(x_ok.data_ptr(), 3, y.data_ptr()) == ERR_ARG              # an unknown io_dtype
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert raw(x_ok.data_ptr(), IO_CODE[torch.bfloat16], y.data_ptr()) == 0
    assert same_bits(y, _block(g, x16, 128, "bf16"))


def test_float64_is_a_type_error_at_the_ops_level(gpu_device):
    inp = _example((512,), 128, 3, 6)
    g = asw._gpu(inp, gpu_device)
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        _block(g, g["x"].double(), 128, "fp32")
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        ops.combine_ffn(partial_rows(1, 512, H, 5, False, gpu_device), D, *[g["params"][k] for k in (
            "attn.out_linear.weight", "attn.out_linear.bias")], g["x"].double(), g["params"]["norm2.weight"],
            g["params"]["norm2.bias"], EPS, g["params"]["ff.0.weight"], g["params"]["ff.0.bias"],
            g["params"]["ff.2.weight"], g["params"]["ff.2.bias"])
