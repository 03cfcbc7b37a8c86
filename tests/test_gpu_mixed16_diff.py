"""precision="mixed16_diff" on the GPU (-m gpu): "mixed16" rows and matrix products for the D feature columns, the
coordinate part of every logit in float32 as explicit differences of sqrt_w * coords (csrc/block_attn_coords.hip).

The file carries a torch model of that arithmetic (``model``): fp16 feature columns with f32 norms of the rounded values,
f32 coordinate differences, weights and values in bf16, bf16 per-table numerators at D = 24.  The staged pipeline
prep_hash -> sort_tables -> block_attn_coords -> combine_out is held to the model and to float64 per row
(``shape_sweep._row_scaled``: worst row of max|out - ref| / (row max|ref| + 1e-3)); the one-call operator, the fused
blocks, the stack and the module must be bit-identical to the staged kernels.  Bounds marked "measured" are set at
<= 2x the worst row measured on the MI355X, the measured value beside them."""
import ctypes

import numpy as np
import pytest
import torch

import attn_sweep as asw
import cases
import hept_oracle as ho
import scratch_sweep as ss
import shape_sweep as sw
import src_attn_sweep as ssw
from attn_sweep import D, EPS, H, K
from hept_amd import AttnStack, HEPTAttention, _lib, ops
from shape_sweep import MAX_TABLES, _cached, _row_scaled
from test_gpu_parity import REL16_ALL_ROWS_FULL, _gpu, _staged

pytestmark = pytest.mark.gpu
PREC = "mixed16_diff"

# worst row of the staged kernels against the model below (bounds at <= 2x the measured worst row, as MODEL16_ROW): a last-bit
# f32 difference in a logit flips the bf16 rounding of a weight or of a stored numerator.  Measured on the MI355X: sweep
# cells 1.04e-3 (b128); G1 8.4e-4, G3 5.88e-3, G7 5.43e-3 (the checkpoint's |out| ~ 2..8 and larger logits)
MODEL_ROW = 2.0e-3
MODEL_ROW_GOLDEN = {"g1_rand512": 1.6e-3, "g3_ckpt6k": 1.1e-2, "g7_ckpt_rawcoords": 1.0e-2}
# ... against float64 on the GPU's own permutations: the bound "mixed16" meets on these inputs (the new mode has strictly
# fewer roundings).  Measured worst row: 6.73e-3 (h3d10c6)
ROW64 = REL16_ALL_ROWS_FULL["mixed16"]
# G7 (shipped layer-0 weights, raw coordinates), fixture permutations, against out_fp64.  CPU emulation of the arithmetic:
# 2.83e-2; measured: 2.831e-2, no row off by more than 0.5 (plain mixed16 in the same run: 2.93 with 10 such rows)
G7_ROW = 5.6e-2
# G7 with coords x 12 (|sqrt_w coords| up to 3.1e5: outside the fp16 range), GPU permutations, against a float64 oracle.
# Emulation: 2.93e-2; measured: 2.932e-2
G7X12_ROW = 5.8e-2
# G1 / G3 with fixture permutations against the reference's fp32 output.  Emulation 6.2e-3 / 2.10e-2; measured 6.151e-3 /
# 2.103e-2 (REL16_ALL_ROWS' range).  G3 sits slightly above mixed16's 1.68e-2: in that mode the rounding of the stored
# coordinates happens to cancel part of the rounding of the features in the worst row; nothing cancels it here
GOLDEN_ROW = {"g1_rand512": 1.2e-2, "g3_ckpt6k": 4.2e-2}
G7X12_MIN_WEIGHT = 1e-15

SWEEP = ["b8", "b32", "b33", "b100", "b128", "b129", "b225", "b256", "h16d27c3", "h7d17c3", "h3d10c6", "h5d20c5",
         "t9-n6272", "cloud-b-b1-100"]


# ---------------------------------------------------------------------------------------------------------------------
# the model (CPU, float32 unless said otherwise)
# ---------------------------------------------------------------------------------------------------------------------
def model(q, k, v, coords, w_rpe_weight, alpha, out_weight, out_bias, qp, kp, block_size, raw_size=None):
    """The arithmetic of HEPT_PREC_MIXED16_DIFF on given permutations (T, H, N)."""
    h = alpha.shape[0]
    n, d = q.shape[0], q.shape[1] // h
    raw = n if raw_size is None else int(raw_size)
    sqrt_w = ho.rpe_scale(w_rpe_weight, h, d, K)
    heads = lambda x: x.reshape(n, h, d).permute(1, 0, 2)                          # noqa: E731
    qf = heads(q).to(torch.float16).float().clone()                                # the stored fp16 feature columns
    kf = heads(k).to(torch.float16).float().clone()
    vf = heads(v).to(torch.bfloat16).float().clone()
    cs = (sqrt_w[None] * coords[:, None]).permute(1, 0, 2).clone()                 # (H, N, C): rounded f32 products
    for x in (qf, kf, vf, cs):
        x[:, raw:] = 0.0                                                           # the reference zero-fills q^, k^, v there
    sq, sk, sv = (ho.gather_blocks(x, p, block_size) for x, p in ((qf, qp), (kf, kp), (vf, kp)))
    cq, ck = ho.gather_blocks(cs, qp, block_size), ho.gather_blocks(cs, kp, block_size)
    qn = -0.5 * (sq ** 2).sum(-1, keepdim=True)
    kn = -0.5 * (sk ** 2).sum(-1, keepdim=True)
    feat = torch.matmul(sq, sk.transpose(-1, -2)) + qn + kn.transpose(-1, -2)
    dsq = torch.zeros_like(feat)
    for c in range(cs.shape[-1]):
        dl = cq[..., c].unsqueeze(-1) - ck[..., c].unsqueeze(-2)
        dsq = dsq + dl * dl
    p = (feat - 0.5 * dsq).clamp(max=0.0).exp().to(torch.bfloat16).float()
    denom = p.sum(-1, keepdim=True) + 1e-20
    numer = torch.matmul(p, sv)
    if d == 24:                                                                    # packed partial rows: bf16 numerators
        numer = numer.to(torch.bfloat16).float()
    per_head = ho.combine_tables(ho.unsort_tables(numer, qp), ho.unsort_tables(denom, qp))
    return ho.out_projection(per_head, out_weight, out_bias)


def _model_of(inp, qp, kp, block_size, raw_size=None):
    return model(inp["q"], inp["k"], inp["v"], inp["coords"], inp["w_rpe_weight"], inp["alpha"], inp["out_weight"],
                 inp["out_bias"], qp.long().cpu(), kp.long().cpu(), block_size, raw_size)


# ---------------------------------------------------------------------------------------------------------------------
# the staged pipeline
# ---------------------------------------------------------------------------------------------------------------------
def staged(g, h, d, block_size, qpos=None, kpos=None, coords=None):
    """prep_hash -> sort_tables (chunks of MAX_TABLES tables, rows reused; or injected permutations) ->
    block_attn_coords -> combine_out."""
    coords = g["coords"] if coords is None else coords
    t = g["alpha"].shape[2]
    sqrt_w = ops.rpe_scale(g["w_rpe_weight"], h, d, K)
    rows, qs, ks = None, [], []
    for c0 in range(0, t, MAX_TABLES):
        tc = min(MAX_TABLES, t - c0)
        ph = ops.prep_hash(g["q"], g["k"], g["v"], coords, sqrt_w, g["alpha"], g["combined_shifts"], PREC, t0=c0, tl=tc,
                           rows=rows)
        rows = (ph["qhat"], ph["kvhat"])
        if qpos is None:
            qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"], t0=c0)
            qs.append(qp)
            ks.append(kp)
    if qpos is None:
        qpos, kpos = torch.cat(qs), torch.cat(ks)
    assert rows[0].dtype is torch.float16                                          # "mixed16" rows
    part = ops.block_attn_coords(rows[0], rows[1], qpos, kpos, coords, sqrt_w, d, block_size)
    out = ops.combine_out(part, d, g["out_weight"], g["out_bias"])
    return dict(out=out, part=part, qpos=qpos, kpos=kpos, rows=rows, sqrt_w=sqrt_w)


def _fixture_perms(fx, dev):
    return (torch.from_numpy(fx["q_positions"].astype(np.int32)).to(dev),
            torch.from_numpy(fx["k_positions"].astype(np.int32)).to(dev))


# ---------------------------------------------------------------------------------------------------------------------
# 1 + 2: the model and float64, cell by cell
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", SWEEP)
def test_sweep_cells_against_the_model_and_float64(sid, gpu_device):
    s = sw.BY_ID[sid]
    inp = _cached((s.id, "inp"), lambda: sw.inputs(s))
    g = _cached((s.id, "gpu"), lambda: sw._gpu(inp, gpu_device))
    st = staged(g, s.H, s.D, s.B)
    one = ops.forward(g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"],
                      g["out_weight"], g["out_bias"], block_size=s.B, w_per_dist=K, precision=PREC)
    torch.cuda.synchronize()
    out = st["out"].cpu()
    assert bool(torch.isfinite(out).all())
    assert torch.equal(one.cpu(), out), f"{sid}: one-call forward differs from the staged kernels"
    wide = ops.unpack_part(st["part"])
    packed = st["part"].dtype == torch.int32
    assert packed == (s.D == 24)
    assert bool((wide[..., s.D] > 0).all())
    assert float(wide[..., s.D + 1:].abs().max()) == 0.0
    if packed:
        assert float(st["part"][..., 13:].abs().max()) == 0.0
    ref = sw._reference(s, inp, st["qpos"], st["kpos"])["out"]
    w64 = _row_scaled(out, ref)
    wm = _row_scaled(out, _model_of(inp, st["qpos"], st["kpos"], s.B))
    print(f"mixed16_diff {sid}: worst row vs float64 {w64:.3e}, vs the model {wm:.3e}")
    assert w64 <= ROW64, f"{sid}: worst row-scaled error vs float64 {w64:.3e}"
    assert wm <= MODEL_ROW, f"{sid}: worst row-scaled error vs the model {wm:.3e}"


# ---------------------------------------------------------------------------------------------------------------------
# 3 - 5: the golden cases
# ---------------------------------------------------------------------------------------------------------------------
def _rows(out, ref):
    return (out.double() - ref.double()).abs().amax(-1) / (ref.double().abs().amax(-1) + 1e-3)


def test_g7_raw_coordinates_every_row(gpu_device):
    """G7, fixture permutations, against out_fp64: finite, no row off by more than 0.5, the worst row strictly below that of
    plain mixed16 (computed here) and within G7_ROW."""
    inp, fx = cases.load_case("g7_ckpt_rawcoords")
    g = _gpu(inp, gpu_device)
    qp, kp = _fixture_perms(fx, gpu_device)
    h, d = inp["alpha"].shape[0], 24
    got = staged(g, h, d, inp["block_size"], qp, kp)["out"].cpu()
    plain = _staged(g, inp, "mixed16", qp, kp)["out"].cpu()
    ref64 = torch.from_numpy(fx["out_fp64"])
    assert bool(torch.isfinite(got).all())
    r_new, r_old = _rows(got, ref64), _rows(plain, ref64)
    far_new, far_old = int(((got.double() - ref64).abs().amax(-1) > 0.5).sum()), int(((plain.double() - ref64).abs().amax(-1) > 0.5).sum())
    wm = _row_scaled(got, _model_of(inp, qp, kp, inp["block_size"]))
    print(f"g7 mixed16_diff vs float64: worst row {float(r_new.max()):.3e} (median {float(r_new.median()):.3e}), rows off by "
          f"more than 0.5: {far_new}; plain mixed16: {float(r_old.max()):.3e} (median {float(r_old.median()):.3e}), {far_old} far "
          f"rows; vs the model {wm:.3e}")
    # (the columns of DESIGN.md section 4's G7 table: rows inside the G3 tolerance, median / mean / worst |row error|)
    e_new = (got.double() - ref64).abs()
    in_tol = float((e_new <= 1e-3 + 1e-4 * ref64.abs()).all(1).float().mean())
    r_abs = e_new.amax(1)
    print(f"g7 mixed16_diff table row: rows {in_tol:.4f}, median {float(r_abs.median()):.2e}, mean {float(r_abs.mean()):.2e}, "
          f"worst {float(r_abs.max()):.2e}, far rows {far_new}")
    assert far_new == 0
    assert wm <= MODEL_ROW_GOLDEN["g7_ckpt_rawcoords"]
    assert float(r_new.max()) < float(r_old.max())
    assert float(r_new.max()) <= G7_ROW


def test_g7_coordinates_beyond_the_fp16_range(gpu_device):
    """G7 with coords x 12: the stored fp16 coordinates overflow, the logits do not see them.  The GPU's own permutations go
    into a float64 oracle; no row is excluded (every row's float64 total weight stays above 1e-15, checked here)."""
    inp, _ = cases.load_case("g7_ckpt_rawcoords")
    inp = dict(inp, coords=(inp["coords"] * 12.0).contiguous())
    g = _gpu(inp, gpu_device)
    h, d, b = inp["alpha"].shape[0], 24, inp["block_size"]
    st = staged(g, h, d, b)
    one = ops.forward(g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"],
                      g["out_weight"], g["out_bias"], block_size=b, w_per_dist=K, precision=PREC)
    got = st["out"].cpu()
    assert torch.equal(one.cpu(), got)
    assert bool(torch.isfinite(got).all())
    sc = (st["sqrt_w"].cpu()[None] * inp["coords"][:, None]).abs().max()
    assert float(sc) > 65504.0, "the case must leave the fp16 range"
    qp, kp = st["qpos"].long().cpu(), st["kpos"].long().cpu()
    d64 = {k_: (v_.double() if v_.is_floating_point() else v_) for k_, v_ in inp.items() if torch.is_tensor(v_)}
    r = ho.forward(d64["q"], d64["k"], d64["v"], d64["coords"], d64["combined_shifts"], d64["w_rpe_weight"], d64["alpha"],
                   d64["out_weight"], d64["out_bias"], block_size=b, w_per_dist=K, q_positions=qp, k_positions=kp,
                   keep=False)
    total = r["denom"].sum(0).squeeze(-1)
    assert float(total.min()) > G7X12_MIN_WEIGHT, float(total.min())
    rr = _rows(got, r["out"])
    far = int(((got.double() - r["out"]).abs().amax(-1) > 0.5).sum())
    print(f"g7 x12 mixed16_diff vs float64: worst row {float(rr.max()):.3e} (median {float(rr.median()):.3e}), far rows {far}, "
          f"smallest float64 row weight {float(total.min()):.3e}, largest |sqrt_w coords| {float(sc):.3e}")
    assert far == 0
    assert float(rr.max()) <= G7X12_ROW


@pytest.mark.parametrize("name", ["g1_rand512", "g3_ckpt6k"])
def test_golden_cases_every_row(name, gpu_device):
    inp, fx = cases.load_case(name)
    g = _gpu(inp, gpu_device)
    qp, kp = _fixture_perms(fx, gpu_device)
    got = staged(g, inp["alpha"].shape[0], 24, inp["block_size"], qp, kp)["out"].cpu()
    ref = torch.from_numpy(fx["out"])
    w = _row_scaled(got, ref)
    wm = _row_scaled(got, _model_of(inp, qp, kp, inp["block_size"]))
    print(f"{name} mixed16_diff vs the reference's fp32 out: worst row {w:.3e}; vs the model {wm:.3e}")
    assert bool(torch.isfinite(got).all())
    assert w <= GOLDEN_ROW[name]
    assert wm <= MODEL_ROW_GOLDEN[name]


# ---------------------------------------------------------------------------------------------------------------------
# 6: the src variant
# ---------------------------------------------------------------------------------------------------------------------
def _src_staged(s, g):
    p, n, raw = g["params"], s.N, g["raw_size"]
    sqrt_w = ops.rpe_scale(p["w_rpe.weight"], H, D, K)
    eta, phi, cfac = ops.geo_args((g["eta"], g["phi"]), g["regions_h"], s.T, H, n)
    rows, qs, ks = None, [], []
    for c0 in range(0, s.T, MAX_TABLES):
        tc = min(MAX_TABLES, s.T - c0)
        ph = ops.prep_hash_fused(g["x"], p["norm1.weight"], p["norm1.bias"], EPS, p["w_q.weight"], p["w_k.weight"],
                                 p["w_v.weight"], g["coords"], sqrt_w, p["attn.e2lsh.alpha"], None, PREC, t0=c0, tl=tc,
                                 raw_size=raw, rows=rows)
        rows = (ph["qhat"], ph["kvhat"])
        qp, kp = ops.sort_tables_src(ph["qproj"], ph["kproj"], eta, phi, cfac, ph["minmax"], t0=c0)
        qs.append(qp)
        ks.append(kp)
    qpos, kpos = torch.cat(qs), torch.cat(ks)
    part = ops.block_attn_coords(rows[0], rows[1], qpos, kpos, g["coords"], sqrt_w, D, s.B, raw_size=raw)
    y = ops.combine_ffn(part, D, p["attn.out_linear.weight"], p["attn.out_linear.bias"], g["x"], p["norm2.weight"],
                        p["norm2.bias"], EPS, p["ff.0.weight"], p["ff.0.bias"], p["ff.2.weight"], p["ff.2.bias"])
    return dict(y=y, part=part, qpos=qpos, kpos=kpos)


@pytest.mark.parametrize("sid", ["n1000-one-in-last-block-b100-t3-c6", "n1000-full-b100-t3-c6"])
def test_src_variant(sid, gpu_device):
    """SrcAttn.eval() and the one-call src block: bit-identical to the staged kernels, within the mixed16 bound of float64
    on their own permutations; the rows at and after raw_size equal what mixed16 gives for them bit for bit.

    (A padding query's own coordinates are zero in both modes, but its logit against a real key of its block is
    -|k^|^2 / 2 of THAT key: the kernel takes the key's stored norm for such queries, as mixed16 does.)"""
    s = ssw.BY_ID[sid]
    inp = _cached((s.id, "inp"), lambda: ssw.inputs(s))
    g = _cached((s.id, "gpu"), lambda: ssw._gpu(inp, gpu_device))
    blk = ssw.module(s, inp, PREC, gpu_device).eval()
    with torch.no_grad():
        st = _src_staged(s, g)
        one = ops.attn_block_forward_src(g["x"], g["coords"], (g["eta"], g["phi"]), g["regions_h"], g["raw_size"],
                                         g["params"], num_heads=H, block_size=s.B, w_per_dist=K, eps1=EPS, eps2=EPS,
                                         precision=PREC)
        assert blk._fused_ok(g["x"])
        mod = blk(g["x"], ssw.kwargs_of(g))
        plain = ssw.module(s, inp, "mixed16", gpu_device).eval()(g["x"], ssw.kwargs_of(g))
        torch.cuda.synchronize()
    y = st["y"].cpu()
    assert bool(torch.isfinite(y).all())
    assert torch.equal(one.cpu(), y) and torch.equal(mod.cpu(), y)
    ref = ssw.reference(s, inp, st["qpos"], st["kpos"])
    w64 = asw._row16(y, ref)
    pad_diff = int((mod[s.raw:] != plain[s.raw:]).any(-1).sum())
    pad_gap = float((mod[s.raw:] - plain[s.raw:]).abs().max()) if s.raw < s.N else 0.0
    print(f"src {sid} mixed16_diff: worst row vs float64 {w64:.3e}; padding rows that differ from mixed16: {pad_diff} of "
          f"{s.N - s.raw}, largest |difference| {pad_gap:.3e}")
    assert w64 <= asw.ROW16_64["mixed16"]
    assert torch.equal(mod[s.raw:], plain[s.raw:])


# ---------------------------------------------------------------------------------------------------------------------
# 7: fused block and stack
# ---------------------------------------------------------------------------------------------------------------------
def _attn_staged(s, g, params=None, x=None):
    p, codes = g["params"] if params is None else params, g["combined_shifts"]
    x = g["x"] if x is None else x
    sqrt_w = ops.rpe_scale(p["w_rpe.weight"], H, D, K)
    rows, qs, ks = None, [], []
    for c0 in range(0, s.T, MAX_TABLES):
        tc = min(MAX_TABLES, s.T - c0)
        ph = ops.prep_hash_fused(x, p["norm1.weight"], p["norm1.bias"], EPS, p["w_q.weight"], p["w_k.weight"],
                                 p["w_v.weight"], g["coords"], sqrt_w, p["attn.e2lsh.alpha"], codes, PREC, t0=c0, tl=tc,
                                 rows=rows)
        rows = (ph["qhat"], ph["kvhat"])
        qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], codes, ph["minmax"], t0=c0)
        qs.append(qp)
        ks.append(kp)
    qpos, kpos = torch.cat(qs), torch.cat(ks)
    part = ops.block_attn_coords(rows[0], rows[1], qpos, kpos, g["coords"], sqrt_w, D, s.B)
    y = ops.combine_ffn(part, D, p["attn.out_linear.weight"], p["attn.out_linear.bias"], x, p["norm2.weight"],
                        p["norm2.bias"], EPS, p["ff.0.weight"], p["ff.0.bias"], p["ff.2.weight"], p["ff.2.bias"])
    return dict(y=y, part=part, qpos=qpos, kpos=kpos)


@pytest.mark.parametrize("sid", ["b8-c6-t2", "b33-c4-t3", "b32-c2-t1"])
def test_attn_block_one_call(sid, gpu_device):
    s = asw.BY_ID[sid]
    inp = _cached((s.id, "inp"), lambda: asw.inputs(s))
    g = _cached((s.id, "gpu"), lambda: asw._gpu(inp, gpu_device))
    blk = asw.module(s, inp, PREC, gpu_device).eval()
    with torch.no_grad():
        st = _attn_staged(s, g)
        one = ops.attn_block_forward(g["x"], g["coords"], g["combined_shifts"], g["params"], num_heads=H, block_size=s.B,
                                     w_per_dist=K, eps1=EPS, eps2=EPS, precision=PREC)
        assert blk._fused_ok(g["x"])
        mod = blk(g["x"], {"coords": g["coords"], "combined_shifts": g["combined_shifts"]})
        torch.cuda.synchronize()
    y = st["y"].cpu()
    assert bool(torch.isfinite(y).all())
    assert torch.equal(one.cpu(), y) and torch.equal(mod.cpu(), y)
    w64 = asw._row16(y, asw.reference(s, inp, st["qpos"], st["kpos"]))
    print(f"attn {sid} mixed16_diff: worst row vs float64 {w64:.3e}")
    assert w64 <= asw.ROW16_64["mixed16"]


@pytest.mark.parametrize("sid", ["n100-single-b100-t3-c6", "n128-single-b128-t9-c4-later", "n33-single-b33-t1-c2-later"])
def test_src_attn_block_one_call(sid, gpu_device):
    s = ssw.BY_ID[sid]
    inp = _cached((s.id, "inp"), lambda: ssw.inputs(s))
    g = _cached((s.id, "gpu"), lambda: ssw._gpu(inp, gpu_device))
    blk = ssw.module(s, inp, PREC, gpu_device).eval()
    with torch.no_grad():
        st = _src_staged(s, g)
        one = ops.attn_block_forward_src(g["x"], g["coords"], (g["eta"], g["phi"]), g["regions_h"], g["raw_size"],
                                         g["params"], num_heads=H, block_size=s.B, w_per_dist=K, eps1=EPS, eps2=EPS,
                                         precision=PREC)
        mod = blk(g["x"], ssw.kwargs_of(g))
        torch.cuda.synchronize()
    y = st["y"].cpu()
    assert bool(torch.isfinite(y).all())
    assert torch.equal(one.cpu(), y) and torch.equal(mod.cpu(), y)
    w64 = asw._row16(y, ssw.reference(s, inp, st["qpos"], st["kpos"]))
    print(f"src attn {sid} mixed16_diff: worst row vs float64 {w64:.3e}")
    assert w64 <= asw.ROW16_64["mixed16"]


def test_two_layer_stack(gpu_device):
    """AttnStack of two layers: bit-identical to the composed modules under the same precision, every layer within the
    attn_sweep 16-bit bound of float64 on its own input and permutations."""
    s = asw.BY_ID["b100-c6-t3"]
    inp = asw.inputs(s)
    g = asw._gpu(inp, gpu_device)
    stack = AttnStack(s.C, precision=PREC, h_dim=D, num_heads=H, block_size=s.B, n_hashes=s.T, num_w_per_dist=K,
                      n_layers=2)
    stack.attns[0].load_state_dict(inp["params"], strict=True)
    stack.attns[1].load_state_dict(asw.default_params(s.C, s.T, s.seed + 10), strict=True)
    stack = stack.to(gpu_device).eval()
    kwargs = {"coords": g["coords"], "combined_shifts": g["combined_shifts"]}
    with torch.no_grad():
        assert stack._fused_ok(g["x"])
        got = stack(g["x"], kwargs)
        outs = [g["x"]]
        for layer in stack.attns:
            outs.append(layer(outs[-1], kwargs))
        torch.cuda.synchronize()
    loop = torch.cat(outs, dim=-1)
    assert got.shape == loop.shape and torch.equal(got, loop)
    for i, layer in enumerate(stack.attns):
        params = {k_: v_.detach() for k_, v_ in layer.state_dict().items()}
        with torch.no_grad():
            st = _attn_staged(s, g, params, outs[i].contiguous())
        assert torch.equal(st["y"], outs[i + 1])
        li = dict(inp, x=outs[i].cpu(), params={k_: v_.cpu() for k_, v_ in params.items()})
        sw._cache.clear()
        ref = asw.reference(s._replace(id=f"stack-layer{i}"), li, st["qpos"], st["kpos"])
        w64 = asw._row16(st["y"].cpu(), ref)
        print(f"stack layer {i} mixed16_diff: worst row vs float64 {w64:.3e}")
        assert w64 <= asw.ROW16_64["mixed16"]


def test_bf16_activations_in_and_out(gpu_device):
    s = asw.BY_ID["b33-c4-t3"]
    inp = asw.inputs(s)
    g = asw._gpu(inp, gpu_device)
    blk = asw.module(s, inp, PREC, gpu_device).eval()
    x16 = g["x"].to(torch.bfloat16)
    kw = dict(num_heads=H, block_size=s.B, w_per_dist=K, eps1=EPS, eps2=EPS, precision=PREC)
    with torch.no_grad():
        mod = blk(x16, {"coords": g["coords"], "combined_shifts": g["combined_shifts"]})
        one = ops.attn_block_forward(x16, g["coords"], g["combined_shifts"], g["params"], **kw)
        wide = ops.attn_block_forward(x16.float(), g["coords"], g["combined_shifts"], g["params"], **kw)
    assert mod.dtype is torch.bfloat16 and torch.equal(mod, one)
    assert torch.equal(one, wide.to(torch.bfloat16))


def _op_module(s, inp, precision, dev):
    m = HEPTAttention(s.D + s.C, h_dim=s.D, num_heads=s.H, block_size=s.B, n_hashes=s.T, num_w_per_dist=K,
                      precision=precision)
    m.load_state_dict({"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"],
                       "e2lsh.alpha": inp["alpha"]}, strict=True)
    w_rpe = torch.nn.Linear(inp["w_rpe_weight"].shape[1], inp["w_rpe_weight"].shape[0])
    with torch.no_grad():
        w_rpe.weight.copy_(inp["w_rpe_weight"])
    return m.to(dev), w_rpe.to(dev)


def test_module_forward_graph_capture_and_replay(gpu_device):
    """One linear chain on one stream (the scale launch included): captured, replayed, and replayed on changed inputs."""
    s = sw.BY_ID["b100"]
    inp = sw.inputs(s)
    g = sw._gpu(inp, gpu_device)
    m, w_rpe = _op_module(s, inp, PREC, gpu_device)
    m.eval()
    kw = dict(w_rpe=w_rpe, coords=g["coords"], combined_shifts=g["combined_shifts"])
    with torch.no_grad():
        eager = m(g["q"], g["k"], g["v"], **kw)
        assert torch.equal(eager, staged(g, s.H, s.D, s.B)["out"])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(g["q"], g["k"], g["v"], **kw)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(g["q"], g["k"], g["v"], **kw)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        w_rpe.weight.mul_(1.01)                            # nothing derived from a parameter is cached across calls
        graph.replay()
        torch.cuda.synchronize()
        again = m(g["q"], g["k"], g["v"], **kw)
        assert torch.equal(out, again) and not torch.equal(out, eager)


# ---------------------------------------------------------------------------------------------------------------------
# 8: training
# ---------------------------------------------------------------------------------------------------------------------
def _train(s, inp, precision, dev):
    m, w_rpe = _op_module(s, inp, precision, dev)
    m.train()
    q, k, v, coords = (inp[x].to(dev).requires_grad_(True) for x in ("q", "k", "v", "coords"))
    out = m(q, k, v, w_rpe=w_rpe, coords=coords, combined_shifts=inp["combined_shifts"].to(dev))
    out.backward(sw._g_out(out.shape).to(dev))
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dcoords=coords.grad, dw_rpe=w_rpe.weight.grad,
                dW_out=m.out_linear.weight.grad, db_out=m.out_linear.bias.grad)


@pytest.mark.parametrize("sid", ["b8", "b100"])
def test_trains_as_fp32_diff(sid, gpu_device):
    s = sw.BY_ID[sid]
    inp = sw.inputs(s)
    new, ref = _train(s, inp, PREC, gpu_device), _train(s, inp, "fp32_diff", gpu_device)
    for nm, t in ref.items():
        assert t is not None and bool(torch.isfinite(t).all()), nm
        assert torch.equal(new[nm], t), f"{sid}: {nm} differs from the fp32_diff module's"


def test_eval_mode_with_grad_enabled_takes_the_inference_path(gpu_device):
    s = sw.BY_ID["b8"]
    inp = sw.inputs(s)
    g = sw._gpu(inp, gpu_device)
    m, w_rpe = _op_module(s, inp, PREC, gpu_device)
    m.eval()
    kw = dict(w_rpe=w_rpe, coords=g["coords"], combined_shifts=g["combined_shifts"])
    with pytest.warns(UserWarning, match="inference path"):
        out = m(g["q"], g["k"], g["v"], **kw)
    assert not out.requires_grad
    with torch.no_grad():
        assert torch.equal(out, m(g["q"], g["k"], g["v"], **kw))


# ---------------------------------------------------------------------------------------------------------------------
# 9: the scratch contract
# ---------------------------------------------------------------------------------------------------------------------
def _scratch_runs(run):
    clean = run()
    torch.cuda.synchronize()
    with ss.scratch("record") as donor:
        run()
    donor.check()
    for pattern in ss.PATTERNS:
        with ss.scratch(pattern, donor.pool if pattern == "leftover" else None) as ledger:
            got = run()
        ledger.check()
        assert ss.same_bits(got, clean), f"{pattern}: the result depends on what scratch memory held before"
    return clean


@pytest.mark.parametrize("sid", ["b100", "n6272"])
def test_module_forward_under_scratch_patterns(sid, gpu_device):
    s = sw.BY_ID[sid]
    inp = sw.inputs(s)
    g = sw._gpu(inp, gpu_device)
    kw = dict(coords=g["coords"], combined_shifts=g["combined_shifts"])

    def run():
        m, w_rpe = _op_module(s, inp, PREC, gpu_device)     # a fresh module: its workspace comes from the patched allocator
        with torch.no_grad():
            return m.eval()(g["q"], g["k"], g["v"], w_rpe=w_rpe, **kw)

    clean = _scratch_runs(run)
    assert bool(torch.isfinite(clean).all())
    # a workspace one byte short is refused by the C call, before anything is launched
    n, h, d, c, t = g["q"].shape[0], s.H, s.D, s.C, s.T
    need = ops.workspace_bytes(n, h, d, c, t, s.B, PREC)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    out = torch.full((n, d), -7.25, device=gpu_device)
    args = lambda nbytes: (g["q"].data_ptr(), g["k"].data_ptr(), g["v"].data_ptr(), _lib.IN_F32, g["coords"].data_ptr(),  # noqa: E731
                           g["combined_shifts"].data_ptr(), g["w_rpe_weight"].data_ptr(), g["alpha"].data_ptr(),
                           g["out_weight"].data_ptr(), g["out_bias"].data_ptr(), n, h, d, c, K, t, s.B,
                           _lib.PREC_MIXED16_DIFF, ws.data_ptr(), nbytes, out.data_ptr(),
                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    lib = _lib.load()
    assert lib.hept_forward_in(*args(need - 1)) == 3
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())
    assert lib.hept_forward_in(*args(need)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, clean)


@pytest.mark.parametrize("sid", ["b100-c6-t3", "n6272-c6"])
def test_one_call_block_under_scratch_patterns(sid, gpu_device):
    s = asw.BY_ID[sid]
    inp = asw.inputs(s)
    g = asw._gpu(inp, gpu_device)

    def run():
        return ops.attn_block_forward(g["x"], g["coords"], g["combined_shifts"], g["params"], num_heads=H, block_size=s.B,
                                      w_per_dist=K, eps1=EPS, eps2=EPS, precision=PREC)

    clean = _scratch_runs(run)
    assert bool(torch.isfinite(clean).all())
