"""The fused ``Attn`` block in training mode with ``precision="fp32_diff"`` (-m gpu): ``HeptPartialSumsFused`` carries the
difference form in both directions.  One backward shape per coordinate count of tests/attn_sweep.py and one of
tests/src_attn_sweep.py whose cloud ends in padding rows; every gradient (x, coords, the 14 parameters) against those
sweeps' float64 block on the GPU's own permutations, within the bounds the sweeps state for fp32 training tiles."""
import pytest
import torch

import attn_sweep as asw
import src_attn_sweep as ssw
from attn_sweep import CANCEL, GRAD_PARAMS, TRAIN_ROW, TRAIN_ROW_CANCEL, TRAIN_TENSOR
from shape_sweep import ATOL, RTOL, _cached, row_x

pytestmark = pytest.mark.gpu

MODE = "fp32"   # the sweeps' bounds for fp32 training tiles
EXAMPLE = [asw.BY_ID[i] for i in ("b96-c6-t2", "b33-c4-t3", "b225-c2-t2")]        # C = 6, 4, 2; full and ragged blocks
SRC = [ssw.BY_ID["n1280-one-in-last-block-b128-t3-c4-later"]]                     # B - 1 padding rows in the last block


def _train(sweep, s, g, inp, dev, kwargs):
    blk = sweep.module(s, inp, "fp32_diff", dev).train()
    blk.dropout.p = 0.0
    assert blk.attn._train_tiles() == "fp32"
    x = g["x"].clone().requires_grad_(True)
    coords = g["coords"].clone().requires_grad_(True)
    kw = kwargs(coords)
    assert blk.attn._train_fused_ok(x, kw)
    y = blk(x, kw)
    assert ssw._fused_node_ran(y), f"{s.id}: the fused training node did not run"
    y.backward(asw._g_out(y.shape).to(dev))
    got = {nm: p.grad.detach().cpu() for nm, p in blk.named_parameters() if p.grad is not None}
    assert set(got) == set(GRAD_PARAMS), sorted(set(got) ^ set(GRAD_PARAMS))
    got.update(y=y.detach().cpu(), x=x.grad.detach().cpu(), coords=coords.grad.detach().cpu())
    return got


def _hold(s, got, want, row_bound):
    worst_t = {nm: float((got[nm].double() - r).abs().max()) / (float(r.abs().max()) + 1e-300) for nm, r in want.items()}
    worst_r = {nm: row_x(got[nm], r) for nm, r in want.items() if nm != "y"}
    y_x = float(((got["y"].double() - want["y"]).abs() / (ATOL + RTOL * want["y"].abs())).max())
    print(f"{s.id} fp32_diff: y {y_x:.3f}x the fp32 tolerance; worst tensor "
          f"{max(worst_t, key=worst_t.get)} {max(worst_t.values()):.2e}, worst row {max(worst_r, key=worst_r.get)} "
          f"{max(worst_r.values()):.2e}, coords tensor {worst_t['coords']:.2e} row {worst_r['coords']:.2e}")
    assert all(bool(torch.isfinite(a).all()) for a in got.values())
    assert y_x <= 1.0, f"{s.id}: training forward, worst element {y_x:.3f}x the fp32 tolerance"
    bad = {nm: w for nm, w in worst_t.items() if w > TRAIN_TENSOR[MODE]}
    assert not bad, f"{s.id}: per-tensor errors over {TRAIN_TENSOR[MODE]}: {bad}"
    rbad = {nm: w for nm, w in worst_r.items() if w > row_bound(nm)}
    assert not rbad, f"{s.id}: per-row errors over the bound: {rbad}"


@pytest.mark.parametrize("s", EXAMPLE, ids=lambda s: s.id)
def test_attn_block_trains_in_the_difference_form(s, gpu_device):
    dev = gpu_device
    assert s.bwd and not s.ckpt
    inp = _cached((s.id, "inp"), lambda: asw.inputs(s))
    g = _cached((s.id, "gpu"), lambda: asw._gpu(inp, dev))
    st = _cached((s.id, "perm"), lambda: asw.staged(s, g, "fp32"))
    qp, kp = st["qpos"].long().cpu(), st["kpos"].long().cpu()
    want = _cached((s.id, "grads64"), lambda: asw.grads64(s, inp, qp, kp))
    got = _train(asw, s, g, inp, dev, lambda coords: {"coords": coords, "combined_shifts": g["combined_shifts"]})
    _hold(s, got, want, lambda nm: (TRAIN_ROW_CANCEL if nm in CANCEL else TRAIN_ROW)[MODE])


@pytest.mark.parametrize("s", SRC, ids=lambda s: s.id)
def test_src_attn_block_trains_in_the_difference_form(s, gpu_device):
    dev = gpu_device
    assert s.bwd and s.raw < s.N
    inp = _cached((s.id, "inp"), lambda: ssw.inputs(s))
    g = _cached((s.id, "gpu"), lambda: ssw._gpu(inp, dev))
    st = _cached((s.id, "perm"), lambda: ssw.staged(s, g, "fp32"))
    qp, kp = st["qpos"].long().cpu(), st["kpos"].long().cpu()
    want = _cached((s.id, "grads64"), lambda: ssw.grads64(s, inp, qp, kp))
    got = _train(ssw, s, g, inp, dev, lambda coords: ssw.kwargs_of(g, coords))
    _hold(s, got, want, lambda nm: ssw.row_bound(s, nm, MODE))
