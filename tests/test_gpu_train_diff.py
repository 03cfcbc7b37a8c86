"""Training in ``precision="fp32_diff"`` (-m gpu): the difference-form block-attention backward
(``hept_block_attn_bwd_diff``) behind ``ops.block_attn_bwd(f32_mfma="diff")``, ``autograd.HeptPartialSums`` and the module.

The yardstick is float64 autograd of the oracle (the reference's arithmetic) on the same permutations.  Case G7 -- the
shipped checkpoint's layer-0 weights on raw coordinates, sqrt_w up to 5.8e3 -- is the regime the mode exists for: there
the oracle's own float32 gradients are 8e-3 .. 5e-2 of their tensor's scale away from float64 (the expanded logit is
rounding noise, and so is a P recomputed from it); the tests assert that regime on the CPU before they hold the GPU to
bounds at least ten times tighter.  Every error below is ``max |a - r| / max |r|`` over a whole tensor, no row excluded."""
import numpy as np
import pytest
import torch

import cases
import hept_oracle as ho
import shape_sweep as sw
from hept_amd import HEPTAttention, ops
from hept_amd.autograd import HeptPartialSums, rpe_scale_torch
from shape_sweep import BWD_ROW_X, DCOORDS_ROW_X, FP32_TENSOR

pytestmark = pytest.mark.gpu

G3_ATOL, G3_RTOL = 1e-3, 1e-4          # tests/test_gpu_parity.py: ATOL["g3_ckpt6k"], rtol
NAMES = dict(q="dq", k="dk", v="dv", w_rpe_weight="dw_rpe", out_weight="dW_out", out_bias="db_out", coords="dcoords")
REGIME = ("dq", "dk", "dv", "dcoords")  # the gradients on which the float32 oracle must be >= 10x the bound in use
# one tenth of the float32 oracle's error on G7 (reference permutations, g_out seed 5): no bound may exceed it
G7_CAP = dict(dq=9.5e-4, dk=8.3e-4, dv=5.4e-3, dcoords=4.9e-3, dw_rpe=2.4e-4)
# G7, stage level and through the module: the project's per-tensor bound for fp32 tiles (FP32_TENSOR = 2e-4) holds for
# every tensor.  Measured on the MI355X, stage level / module: dq 6.2e-6 / 6.1e-6, dk 8.7e-6 / 8.5e-6, dv 3.6e-5 / 3.7e-5,
# dcoords 1.5e-5 / 1.5e-5, dw_rpe 1.4e-4 / 7.7e-6 (stage level: sqrt_w and its backward in torch), dW_out 2.4e-6 / 3.9e-7,
# db_out 1.7e-7 / 2.6e-7; out 0.23x / 0.10x the G3 tolerance.  (The float32 oracle: 9.5e-3, 8.3e-3, 5.4e-2, 4.9e-2, 2.4e-3.)
G7_BOUND = {nm: FP32_TENSOR for nm in ("dq", "dk", "dv", "dcoords", "dw_rpe", "dW_out", "db_out")}
# leading slices of G7 (first 4 B points, T = 3, the float64 oracle's own sort): measured worst on the MI355X, and the
# bound = 2x that; never above one tenth of the float32 oracle's error on the same slice (computed in the test: 3e-3 ..
# 7e-3 on dq, dk, dv, dcoords, 3e-4 .. 1.4e-3 on dw_rpe).  dW_out and db_out come from torch's linear backward, not from
# the kernels under test: the project's bound.
SLICE_MEASURED = {
    100: dict(dq=5.55e-6, dk=4.33e-6, dv=4.18e-6, dcoords=7.78e-6, dw_rpe=5.60e-6),
    128: dict(dq=4.44e-6, dk=4.36e-6, dv=4.30e-6, dcoords=1.08e-5, dw_rpe=7.51e-6),
    225: dict(dq=5.60e-6, dk=7.74e-6, dv=6.64e-6, dcoords=1.82e-5, dw_rpe=1.83e-6),
    256: dict(dq=4.41e-6, dk=7.13e-6, dv=6.64e-6, dcoords=2.14e-5, dw_rpe=7.23e-6),
}
SLICE_BOUND = {b: dict({nm: 2 * w for nm, w in m.items()}, dW_out=FP32_TENSOR, db_out=FP32_TENSOR)
               for b, m in SLICE_MEASURED.items()}

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _tensor_err(a, r):
    return float((a.double().cpu() - r).abs().max()) / (float(r.abs().max()) + 1e-300)


def _oracle_grads(inp, qp, kp, dtype, seed, geo=None):
    """Autograd of the oracle in ``dtype`` (coords a leaf); permutations injected, or the oracle's own sort (None)."""
    d = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
    leaves = {k: d[k].clone().requires_grad_(True) for k in NAMES}
    res = ho.forward(leaves["q"], leaves["k"], leaves["v"], leaves["coords"], d["combined_shifts"], leaves["w_rpe_weight"],
                     d["alpha"], leaves["out_weight"], leaves["out_bias"], block_size=inp["block_size"], w_per_dist=10,
                     q_positions=qp, k_positions=kp, keep=False, grad=True)
    res["out"].backward(torch.randn(res["out"].shape, generator=torch.Generator().manual_seed(seed)).to(dtype))
    got = {NAMES[k]: t.grad.double() for k, t in leaves.items()}
    got["out"] = res["out"].detach().double()
    got["q_positions"], got["k_positions"] = res["q_positions"], res["k_positions"]
    return got


def _stage_level(inp, qp, kp, dev, seed, flag="diff"):
    """prep_hash("fp32") -> block_attn -> reduce_tables -> divide + linear in torch -> block_attn_bwd, as
    tests/test_gpu_backward.py test_backward_with_injected_permutations composes them."""
    g = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
    h = inp["alpha"].shape[0]
    d, c, b = inp["q"].shape[1] // h, inp["coords"].shape[1], inp["block_size"]
    w_rpe = g["w_rpe_weight"].clone().requires_grad_(True)
    sqrt_w = rpe_scale_torch(w_rpe, h, d, 10)
    ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sqrt_w.detach(), g["alpha"], g["combined_shifts"], "fp32")
    qpos, kpos = qp.to(dev).int(), kp.to(dev).int()
    part = ops.block_attn(ph["qhat"], ph["kvhat"], qpos, kpos, d, b, f32_mfma=flag)
    acc = ops.reduce_tables(part, d).requires_grad_(True)
    ow, ob = g["out_weight"].clone().requires_grad_(True), g["out_bias"].clone().requires_grad_(True)
    out = torch.nn.functional.linear((acc[..., :d] / acc[..., d:d + 1]).reshape(-1, h * d), ow, ob)
    g_out = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed))
    out.backward(g_out.to(dev))
    dq, dk, dv, dcs = ops.block_attn_bwd(ph["qhat"], ph["kvhat"], qpos, kpos, acc.grad, d, c, b, f32_mfma=flag)
    sqrt_w.backward(torch.einsum("nhc,nc->hc", dcs, g["coords"]))
    dcoords = (dcs * sqrt_w.detach()[None]).sum(dim=1)
    return dict(out=out.detach(), dq=dq, dk=dk, dv=dv, dw_rpe=w_rpe.grad, dW_out=ow.grad, db_out=ob.grad, dcoords=dcoords)


def _module(inp, dev, precision="fp32_diff", **kw):
    h, e, t = inp["alpha"].shape
    m = HEPTAttention(e, h_dim=inp["q"].shape[1] // h, num_heads=h, block_size=inp["block_size"], n_hashes=t,
                      num_w_per_dist=10, precision=precision, **kw)
    sd = {"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"], "e2lsh.alpha": inp["alpha"]}
    if kw.get("variant") == "src":
        sd["e2lsh.beta"] = torch.zeros(1, t)
    m.load_state_dict(sd, strict=True)
    w_rpe = torch.nn.Linear(inp["w_rpe_weight"].shape[1], inp["w_rpe_weight"].shape[0]).to(dev)
    with torch.no_grad():
        w_rpe.weight.copy_(inp["w_rpe_weight"])
    return m.to(dev), w_rpe


def _module_level(inp, dev, seed):
    """HEPTAttention(precision="fp32_diff").train(), its own sort; then the same module in eval mode, grad enabled."""
    m, w_rpe = _module(inp, dev)
    m.train()
    q, k, v, coords = (inp[x].to(dev).requires_grad_(True) for x in ("q", "k", "v", "coords"))
    codes = inp["combined_shifts"].to(dev)
    out = m(q, k, v, w_rpe=w_rpe, coords=coords, combined_shifts=codes)
    out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).to(dev))
    got = dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dw_rpe=w_rpe.weight.grad, dW_out=m.out_linear.weight.grad,
               db_out=m.out_linear.bias.grad, dcoords=coords.grad)
    m.eval()
    assert torch.is_grad_enabled()
    got["out_eval"] = m(q.detach(), k.detach(), v.detach(), w_rpe=w_rpe, coords=coords.detach(), combined_shifts=codes).detach()
    return got


def _gpu_permutations(inp, dev):
    """The permutations the module's forward uses: the staged kernels on the same inputs (shape_sweep.check_backward)."""
    g = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
    h = inp["alpha"].shape[0]
    sqrt_w = ops.rpe_scale(g["w_rpe_weight"], h, inp["q"].shape[1] // h, 10)
    ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sqrt_w, g["alpha"], g["combined_shifts"], "fp32")
    qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"])
    return qp.long().cpu(), kp.long().cpu()


def _check(tag, got, want64, want32, bound, cap, check_out=True):
    """Print every figure, then: out inside the G3 tolerance on every element, each gradient inside its bound, each
    bound at most its cap, and the float32 oracle at least ten times the bound on the REGIME gradients."""
    worst = {nm: _tensor_err(got[nm], want64[nm]) for nm in bound}
    oracle32 = {nm: _tensor_err(want32[nm], want64[nm]) for nm in bound}
    out_err = (got["out"].double().cpu() - want64["out"]).abs()
    out_x = float((out_err / (G3_ATOL + G3_RTOL * want64["out"].abs())).max())
    print(f"{tag}: out worst element {out_x:.3f}x the G3 tolerance; worst error over the tensor's scale "
          + ", ".join(f"{nm} {worst[nm]:.2e} (float32 oracle {oracle32[nm]:.2e}, bound {bound[nm]:.1e})" for nm in bound))
    for nm in bound:
        assert bool(torch.isfinite(got[nm]).all()), (tag, nm)
        assert bound[nm] <= cap.get(nm, bound[nm]), f"{tag}: the bound of {nm} exceeds its cap {cap[nm]:.1e}"
    for nm in REGIME:
        assert oracle32[nm] >= 10 * bound[nm], f"{tag}: float32 oracle error of {nm} {oracle32[nm]:.2e}: not the regime"
    assert out_x <= 1.0 or not check_out, f"{tag}: out, worst element {out_x:.3f}x the G3 tolerance"
    bad = {nm: w for nm, w in worst.items() if w > bound[nm]}
    assert not bad, f"{tag}: errors over the bound: {bad}"
    return worst


def _g7():
    inp, fx = cases.load_case("g7_ckpt_rawcoords")
    qp = torch.from_numpy(fx["q_positions"].astype(np.int64))
    kp = torch.from_numpy(fx["k_positions"].astype(np.int64))
    return inp, qp, kp


# ---- (a) G7, stage level, the reference's permutations
def test_g7_stage_level_gradients_against_float64(gpu_device):
    inp, qp, kp = _g7()
    want64 = _once("g7-ref-64", lambda: _oracle_grads(inp, qp, kp, torch.float64, 5))
    want32 = _once("g7-ref-32", lambda: _oracle_grads(inp, qp, kp, torch.float32, 5))
    got = _stage_level(inp, qp, kp, gpu_device, 5)
    _check("g7 stage level", got, want64, want32, G7_BOUND, G7_CAP)


# ---- (b) G7 through the module (its own sort); eval mode with grad enabled returns the same forward
def test_g7_module_gradients_against_float64(gpu_device):
    inp, _, _ = _g7()
    qp, kp = _gpu_permutations(inp, gpu_device)
    want64 = _oracle_grads(inp, qp, kp, torch.float64, 5)
    want32 = _oracle_grads(inp, qp, kp, torch.float32, 5)
    got = _module_level(inp, gpu_device, 5)
    _check("g7 module", got, want64, want32, G7_BOUND, G7_CAP)
    assert torch.equal(got["out_eval"], got["out"]), "eval mode with grad enabled differs from the training forward"
    tol = G3_ATOL + G3_RTOL * want64["out"].abs()
    assert bool(((got["out_eval"].double().cpu() - want64["out"]).abs() <= tol).all())


# ---- (c), (d): every instantiation of the kernel
HAND = [s for s in sw.BWD_SHAPES if not s.id.startswith("r")]
# a row wider than one launch's six coordinate columns (two launches of the backward kernel), ragged blocks
WIDE = sw.Shape("h4d12c8-b40", (40 * 7 + 3, 90), 40, 2, 4, 12, 8, 571, True)
ALL = HAND + [WIDE]


def _train_once(s, inp, dev):
    m, w_rpe = _module(dict(inp, block_size=s.B), dev)
    m.train()
    q, k, v, coords = (inp[x].to(dev).requires_grad_(True) for x in ("q", "k", "v", "coords"))
    out = m(q, k, v, w_rpe=w_rpe, coords=coords, combined_shifts=inp["combined_shifts"].to(dev))
    out.backward(sw._g_out(out.shape).to(dev))
    return dict(zip(("out", "dq", "dk", "dv", "dw_rpe", "dW_out", "db_out", "dcoords"),
                    (x.detach().cpu() for x in (out, q.grad, k.grad, v.grad, w_rpe.weight.grad, m.out_linear.weight.grad,
                                                m.out_linear.bias.grad, coords.grad))))


def test_shapes_cover_every_instantiation():
    """Tile counts 1-8, each with full and with ragged blocks; the head dimensions and head counts; more than 8 tables."""
    assert {(-(-s.B // 32), s.B % 32 == 0) for s in HAND} == {(k, full) for k in range(1, 9) for full in (True, False)}
    assert {s.D for s in HAND} >= {8, 16, 17, 20, 24, 27} and {s.H for s in HAND} >= {3, 5, 7, 8, 16}
    assert any(s.T > sw.MAX_TABLES for s in HAND) and {"n6272", "t9-n6272", "cloud-b-b1-100"} <= {s.id for s in HAND}
    assert WIDE.C > 6 and WIDE.D + WIDE.C <= 30


@pytest.mark.parametrize("s", ALL, ids=lambda s: s.id)
def test_node_forward_is_the_inference_kernel(s, gpu_device):
    """(c) ``HeptPartialSums`` with the module's flag returns the table sum of ``block_attn(f32_mfma="diff")`` on the
    staged rows and permutations, bit for bit, and two backward passes are bit-identical (no float atomics)."""
    dev = gpu_device
    inp = sw._cached((s.id, "inp"), lambda: sw.inputs(s))
    g = sw._cached((s.id, "gpu"), lambda: sw._gpu(inp, dev))
    st = sw.staged(s, g, "fp32_diff_split")
    m, _ = _module(dict(inp, block_size=s.B), dev)
    flag = m._train_f32_mfma()
    assert flag == "diff"
    sqrt_w = ops.rpe_scale(g["w_rpe_weight"], s.H, s.D, 10)
    acc = HeptPartialSums.apply(g["q"], g["k"], g["v"], g["coords"], sqrt_w, g["alpha"], g["combined_shifts"], s.B, None,
                                flag, m._train_tiles())
    assert torch.equal(acc, ops.reduce_tables(st["part"], s.D)), f"{s.id}: the node's forward is not block_attn(diff)"
    first, second = _train_once(s, inp, dev), _train_once(s, inp, dev)
    for nm in first:
        assert torch.equal(first[nm], second[nm]), (s.id, nm)


@pytest.mark.parametrize("s", ALL, ids=lambda s: s.id)
def test_shape_gradients_against_float64(s, gpu_device):
    """(d) module gradients against ``shape_sweep._grads64`` on the GPU's permutations, the sweep's fp32 bounds."""
    dev = gpu_device
    inp = sw._cached((s.id, "inp"), lambda: sw.inputs(s))
    g = sw._cached((s.id, "gpu"), lambda: sw._gpu(inp, dev))
    st = sw._cached((s.id, "perm"), lambda: sw.staged(s, g, "fp32"))
    qp, kp = st["qpos"].long().cpu(), st["kpos"].long().cpu()
    want = sw._cached((s.id, "grads64"), lambda: sw._grads64(s, inp, qp, kp))
    got = _train_once(s, inp, dev)
    worst_t = {nm: _tensor_err(got[nm], r) for nm, r in want.items()}
    worst_r = {nm: sw.row_x(got[nm], r) for nm, r in want.items() if nm != "out"}
    out_x = float(((got["out"].double() - want["out"]).abs() / (sw.ATOL + sw.RTOL * want["out"].abs())).max())
    print(f"{s.id} fp32_diff: out {out_x:.3f}x the fp32 tolerance; worst tensor "
          f"{max(w for nm, w in worst_t.items() if nm != 'out'):.2e}, worst row {max(worst_r.values()):.2e}, "
          f"dcoords tensor {worst_t['dcoords']:.2e} row {worst_r['dcoords']:.2e} (row bound {DCOORDS_ROW_X['fp32']:.1e})")
    assert all(bool(torch.isfinite(a).all()) for a in got.values())
    assert out_x <= 1.0, f"{s.id}: training forward, worst element {out_x:.3f}x the fp32 tolerance"
    bad = {nm: w for nm, w in worst_t.items() if nm != "out" and w > FP32_TENSOR}
    assert not bad, f"{s.id}: per-tensor errors over the bound {bad}"
    rbad = {nm: w for nm, w in worst_r.items() if w > (DCOORDS_ROW_X if nm == "dcoords" else BWD_ROW_X)["fp32"]}
    assert not rbad, f"{s.id}: per-row errors over the bound: {rbad}"


# ---- (e) golden gradients of the real reference: the form changes how a logit is summed, not what it is
def _close(a, b, rel=2e-4):
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30) <= rel


@pytest.mark.parametrize("name", ["g1_rand512", "g6_block100", "g4_pileup"])
def test_golden_gradients_with_injected_permutations(name, gpu_device):
    inp, fx = cases.load_case(name)
    qp = torch.from_numpy(fx["q_positions"].astype(np.int64))
    kp = torch.from_numpy(fx["k_positions"].astype(np.int64))
    want = _oracle_grads(inp, qp, kp, torch.float32, 11)
    got = {k: v.cpu() for k, v in _stage_level(inp, qp, kp, gpu_device, 11).items()}
    assert _close(got["dq"], want["dq"]) and _close(got["dk"], want["dk"]) and _close(got["dv"], want["dv"])
    assert _close(got["dw_rpe"], want["dw_rpe"], rel=1e-3)
    assert _close(got["dW_out"], want["dW_out"]) and _close(got["db_out"], want["db_out"])
    if "ref_grad_rows" in fx:  # gradients of the REAL reference (stored by make_golden.py) for the same g_out
        rows = torch.from_numpy(fx["ref_grad_rows"].astype(np.int64))
        assert _close(got["dq"][rows], torch.from_numpy(fx["ref_dq_rows"]))
        assert _close(got["dk"][rows], torch.from_numpy(fx["ref_dk_rows"]))
        assert _close(got["dv"][rows], torch.from_numpy(fx["ref_dv_rows"]))
        assert _close(got["dw_rpe"], torch.from_numpy(fx["ref_dw_rpe"]), rel=1e-3)


def test_golden_gradients_of_the_src_variant(gpu_device):
    """``s1_src1000`` through the module, the checks of tests/test_gpu_src.py test_src_module_forward_backward."""
    from hept_amd.prep import prepare_input_src

    inp, fx = cases.load_case_src("s1_src1000")
    dev = gpu_device
    m, w_rpe = _module(inp, dev, variant="src")
    m.train()
    raw = inp["raw_size"]
    _, kw = prepare_input_src(torch.zeros(raw, 1, device=dev), inp["coords_raw"].to(dev),
                              {"block_size": inp["block_size"], "regions": inp["regions"].to(dev)})
    q, k, v = (inp[x].to(dev).requires_grad_(True) for x in ("q", "k", "v"))
    out = m(q, k, v, w_rpe=w_rpe, pe=kw["coords"], **kw)
    ref = torch.from_numpy(fx["out"])
    err = (out.detach().cpu()[:raw] - ref[:raw]).abs()
    assert float((err <= 1e-5 + 1e-4 * ref[:raw].abs()).all(-1).float().mean()) >= 0.99
    out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(11)).to(dev))
    rows = torch.from_numpy(fx["rows"].astype(np.int64))
    for got, key in ((q.grad, "ref_dq_rows"), (k.grad, "ref_dk_rows"), (v.grad, "ref_dv_rows")):
        want = torch.from_numpy(fx[key])
        err = (got.cpu()[rows] - want).abs().amax(-1)
        assert (err <= 2e-4 * float(want.abs().max())).float().mean() >= 0.98
        assert raw == got.shape[0] or float(got[raw:].abs().max()) == 0.0
    want = torch.from_numpy(fx["ref_dw_rpe"])
    assert float((w_rpe.weight.grad.cpu() - want).abs().max()) <= 2e-2 * float(want.abs().max())
    want = torch.from_numpy(fx["ref_dout_w"])
    assert float((m.out_linear.weight.grad.cpu() - want).abs().max()) <= 5e-3 * float(want.abs().max())


# ---- (f) leading slices of G7: rows with total weight near 1e-10 among them, per-tensor bounds, no row filtered
@pytest.mark.parametrize("b", [100, 128, 225, 256])
def test_g7_leading_slices(b, gpu_device):
    full, _, _ = _g7()
    n = 4 * b
    inp = dict(full, block_size=b)
    for key in ("q", "k", "v", "coords"):
        inp[key] = full[key][:n].contiguous()
    inp["combined_shifts"] = full["combined_shifts"][..., :n].contiguous()
    assert inp["alpha"].shape[2] == 3
    want64 = _oracle_grads(inp, None, None, torch.float64, 5)           # the float64 oracle's own sort
    qp, kp = want64["q_positions"], want64["k_positions"]
    want32 = _oracle_grads(inp, qp, kp, torch.float32, 5)
    got = _stage_level(inp, qp, kp, gpu_device, 5)
    cap = {nm: 0.1 * _tensor_err(want32[nm], want64[nm]) for nm in ("dq", "dk", "dv", "dcoords", "dw_rpe")}
    _check(f"g7[:{n}] B={b}", got, want64, want32, SLICE_BOUND[b], cap, check_out=False)   # (the gradients are what is held)
