"""``train_tiles = "mixed16"`` on the GPU: the 16-bit difference-form backward (csrc/block_attn_bwd_coords.hip) cell by cell
(tests/train16_sweep.py), the reason the mode exists, raw coordinates under a checkpoint's ``sqrt_w``, and the module-level
contract of ``HEPTAttention(precision="mixed16_diff")`` in training mode."""
import pytest
import torch

import autograd_sweep as aus
import cases
import shape_sweep as sw
import src_attn_sweep as ssw
import attn_sweep as asw
import train16_sweep as ts
from hept_amd import HEPTAttention, ops
from hept_amd.autograd import HeptCombine

pytestmark = pytest.mark.gpu
PREC = "mixed16_diff"


# ---- the kernel, instantiation by instantiation
@pytest.mark.parametrize("cid", [c.id for c in ts.EXACT])
def test_exact_cells(cid, gpu_device):
    ts.check_exact(ts.EXACT_BY_ID[cid], gpu_device)


@pytest.mark.parametrize("cid", [c.id for c in ts.RANDOM])
def test_random_cells_against_float64(cid, gpu_device):
    ts.check_random(ts.RANDOM_BY_ID[cid], gpu_device)


# ---- module level helpers
def _oracle64(inp, qp, kp, seed=5, geo=None):
    import hept_oracle as ho

    names = ("q", "k", "v", "coords", "w_rpe_weight", "out_weight", "out_bias")
    leaves = {k: inp[k].double().clone().requires_grad_(True) for k in names}
    res = ho.forward(leaves["q"], leaves["k"], leaves["v"], leaves["coords"], inp.get("combined_shifts"),
                     leaves["w_rpe_weight"], inp["alpha"].double(), leaves["out_weight"], leaves["out_bias"],
                     block_size=inp["block_size"], w_per_dist=10, q_positions=qp, k_positions=kp, keep=False, grad=True)
    res["out"].backward(aus.g_out(res["out"].shape, seed).double())
    return dict({k: t.grad for k, t in leaves.items()}, out=res["out"].detach())


def _train_module(inp, precision, tiles, dev, rec, seed=5):
    """One training step of HEPTAttention on ``inp``; returns the gradients by input name and the run's permutations."""
    h, e, t = inp["alpha"].shape
    m = HEPTAttention(e, h_dim=inp["q"].shape[1] // h, num_heads=h, block_size=inp["block_size"], n_hashes=t,
                      num_w_per_dist=10, precision=precision)
    m.load_state_dict({"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"],
                       "e2lsh.alpha": inp["alpha"]}, strict=True)
    m = m.to(dev).train()
    m.train_tiles = tiles
    w_rpe = torch.nn.Linear(inp["w_rpe_weight"].shape[1], inp["w_rpe_weight"].shape[0]).to(dev)
    with torch.no_grad():
        w_rpe.weight.copy_(inp["w_rpe_weight"])
    q, k, v, coords = (inp[x].to(dev).requires_grad_(True) for x in ("q", "k", "v", "coords"))
    n0 = len(rec.calls)
    out = m(q, k, v, w_rpe=w_rpe, coords=coords, combined_shifts=inp["combined_shifts"].to(dev))
    out.backward(aus.g_out(out.shape, seed).to(dev))
    calls = rec.calls[n0:]
    qp = torch.cat([c[0] for c in calls]).long().cpu()
    kp = torch.cat([c[1] for c in calls]).long().cpu()
    got = dict(q=q.grad, k=k.grad, v=v.grad, coords=coords.grad, w_rpe_weight=w_rpe.weight.grad,
               out_weight=m.out_linear.weight.grad, out_bias=m.out_linear.bias.grad, out=out.detach())
    return {k_: t_.cpu() for k_, t_ in got.items()}, (qp, kp)


# ---- the reason the mode exists
def test_tight_clusters_beat_the_bf16_tiles(gpu_device, monkeypatch):
    """The tight-cluster input of test_bf16_training_tiles_with_other_head_counts at (H, D, C) = (8, 24, 6): k^ - q^ inside a
    block is comparable to the bf16 spacing of the rows, and the bf16 tiles differentiate the ROUNDED forward.  Against
    float64 on the unrounded inputs (each run's own permutations) the new mode's dq and dk errors must be no larger than
    those of train_tiles="bf16" under precision="bf16"."""
    from hept_amd.synthetic import make_inputs

    rec = aus.Recorder(monkeypatch)
    inp = make_inputs([700, 420], block_size=64, n_hashes=2, coords_dim=6, h_dim=24, num_heads=8, seed=31, cluster_size=8)
    inp["block_size"] = 64
    new, perms_new = _train_module(inp, PREC, "mixed16", gpu_device, rec)
    old, perms_old = _train_module(inp, "bf16", "bf16", gpu_device, rec)
    want_new = _oracle64(inp, *perms_new)
    want_old = want_new if all(torch.equal(a, b) for a, b in zip(perms_new, perms_old)) else _oracle64(inp, *perms_old)
    fig = {nm: (ts.tensor_err(new[nm], want_new[nm]), ts.tensor_err(old[nm], want_old[nm])) for nm in ("q", "k", "v", "coords")}
    print("train16 tight clusters, max error / tensor scale vs float64: "
          + ", ".join(f"d{k} mixed16 {a:.3e} bf16 {b:.3e}" for k, (a, b) in fig.items()))
    for nm in ("q", "k"):
        assert bool(torch.isfinite(new[nm]).all())
        assert fig[nm][0] <= fig[nm][1], f"d{nm}: train_tiles='mixed16' {fig[nm][0]:.3e}, train_tiles='bf16' {fig[nm][1]:.3e}"


# ---- raw coordinates under the checkpoint's sqrt_w
def test_g7_slice_raw_coordinates(gpu_device, monkeypatch):
    """The leading 768 points of G7 (the shipped checkpoint's w_rpe on raw coordinates, sqrt_w up to 5.8e3; B = 128): every
    gradient finite and within 0.15 of its tensor's scale of the float64 oracle on the run's permutations."""
    rec = aus.Recorder(monkeypatch)
    full, _ = cases.load_case("g7_ckpt_rawcoords")
    n, b = 768, 128
    inp = dict(full, block_size=b)
    for key in ("q", "k", "v", "coords"):
        inp[key] = full[key][:n].contiguous()
    inp["combined_shifts"] = full["combined_shifts"][..., :n].contiguous()
    got, (qp, kp) = _train_module(inp, PREC, "mixed16", gpu_device, rec)
    want = _oracle64(inp, qp, kp)
    fig = {nm: ts.tensor_err(got[nm], want[nm]) for nm in got}
    print("train16 g7[:768] B=128, max error / tensor scale vs float64: " + ", ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    for nm, a in got.items():
        assert bool(torch.isfinite(a).all()), nm
    bad = {k: v for k, v in fig.items() if v > ts.TENSOR_16}
    assert not bad, f"over 0.15 of the tensor's scale: {bad}"


# ---- module level: both variants, the fused and the composed block, B = 8, 100, 128 x T = 1, 3, 9 (a latin square)
def _op(name, sizes, b, t, seed):
    s = sw.Shape(name, tuple(sizes), b, t, 8, 24, 6, seed, True)
    return aus.Case(name, "op", "example", None, 1, s, s._replace(seed=seed + 1), ())


def _src(name, n, raw, b, t, seed):
    s = aus.SrcOp(name, n, raw, b, t, 8, 24, 6, seed)
    return aus.Case(name, "op", "src", None, 1, s, s._replace(seed=seed + 1), ())


def _blk(name, sizes, b, t, seed, fused):
    s = asw.Shape(name, tuple(sizes), b, t, 4, seed, True, False)
    return aus.Case(name, "blk", "example", fused, 1, s, s._replace(seed=seed + 1), ())


def _blk_src(name, n, raw, b, t, seed):
    s = ssw.Shape(name, n, raw, b, t, 4, False, seed, True)
    return aus.Case(name, "blk", "src", True, 1, s, s._replace(seed=seed + 1), ())


MODULE_CASES = [
    _op("m16-op-b8-t1", [50, 38], 8, 1, 700), _op("m16-op-b100-t3", [250, 130], 100, 3, 710),
    _op("m16-op-b128-t9", [200, 100], 128, 9, 720),
    _src("m16-src-b8-t3", 96, 91, 8, 3, 730), _src("m16-src-b100-t9", 400, 333, 100, 9, 740),
    _src("m16-src-b128-t1", 384, 300, 128, 1, 750),
    _blk("m16-blk-b8-t9", [50, 38], 8, 9, 760, True), _blk("m16-blk-b100-t1", [250, 130], 100, 1, 770, True),
    _blk("m16-blk-b128-t3", [200, 100], 128, 3, 780, True),
    _blk("m16-blkc-b100-t3", [150, 60], 100, 3, 790, False), _blk("m16-blkc-b8-t9", [40, 20], 8, 9, 800, False),
    _blk_src("m16-blksrc-b128-t9", 384, 300, 128, 9, 810),
]
MODULE_BY_ID = {c.id: c for c in MODULE_CASES}


def _rig(case, dev, rec, precision=PREC, tiles="mixed16"):
    rig = aus.Rig(case, "fp32_diff" if precision == PREC else "bf16", dev, rec, precision=precision)
    for a in rig.ops_:
        a.train_tiles = tiles
        assert a.precision == precision
    return rig


def _errors(case, run, which="X"):
    want = aus.ref64(case, which, run.perms)
    got = dict(run.grads, out=run.out)
    fig = {}
    for nm, r in want.items():
        if nm == "perms" or r is None:
            continue
        assert got[nm] is not None and bool(torch.isfinite(got[nm]).all()), (case.id, nm)
        fig[nm] = ts.tensor_err(got[nm], r)
    return fig


def _staged_forward(case, rig):
    """The training forward staged by hand: prep_hash("mixed16") (the fused block: prep_hash_fused) -> sort ->
    block_attn_coords -> reduce_tables -> HeptCombine on the module's own parameters; for a block, its residual adds and
    norm2 / ff around that (dropout is 0): what the module's training forward must equal bit for bit."""
    g, s = rig.data("X"), case.shape
    blk = rig.net if case.kind == "blk" else None
    attn = rig.net.attn
    h, d = (asw.H, asw.D) if blk is not None else (s.H, s.D)
    w_rpe = (blk if blk is not None else rig.net).w_rpe.weight.detach()
    with torch.no_grad():
        sqrt_w = ops.rpe_scale(w_rpe.float(), h, d, 10)
        coords = g["coords"].float()
        n = coords.shape[0]
        raw = g["raw_size"] if case.variant == "src" else None
        geo = ops.geo_args([g["eta"], g["phi"]], g["regions_h"], s.T, h, n) if case.variant == "src" else None
        codes = None if geo is not None else g["combined_shifts"]
        alpha = attn.e2lsh.alpha.detach()
        if blk is not None and not case.fused:    # the composed block: torch norm1 and projections, then the operator
            xn = blk.norm1(g["x"])
            q, k, v = blk.w_q(xn), blk.w_k(xn), blk.w_v(xn)
        elif blk is None:
            q, k, v = g["q"], g["k"], g["v"]
        rows, qs, ks = None, [], []
        for c0 in range(0, s.T, sw.MAX_TABLES):
            tc = min(sw.MAX_TABLES, s.T - c0)
            if blk is not None and case.fused:
                ph = ops.prep_hash_fused(g["x"], blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, blk.w_q.weight, blk.w_k.weight,
                                         blk.w_v.weight, coords, sqrt_w, alpha, codes, "mixed16", t0=c0, tl=tc,
                                         raw_size=n if raw is None else raw, rows=rows)
            else:
                ph = ops.prep_hash(q, k, v, coords, sqrt_w, alpha, codes, "mixed16", t0=c0, tl=tc, raw_size=raw, rows=rows)
            rows = (ph["qhat"], ph["kvhat"])
            if geo is None:
                qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], codes, ph["minmax"], t0=c0)
            else:
                qp, kp = ops.sort_tables_src(ph["qproj"], ph["kproj"], geo[0], geo[1], geo[2], ph["minmax"], t0=c0)
            qs.append(qp)
            ks.append(kp)
        part = ops.block_attn_coords(rows[0], rows[1], torch.cat(qs), torch.cat(ks), coords, sqrt_w, d, s.B, raw_size=raw)
        acc = ops.reduce_tables(part, d)
        out = HeptCombine.apply(acc, attn.out_linear.weight.detach(), attn.out_linear.bias.detach())
        if blk is None:
            return out
        x1 = g["x"] + out
        if case.fused:
            ff = ops.ln_ffn_fwd(x1, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, blk.ff[0].weight, blk.ff[0].bias,
                                blk.ff[2].weight, blk.ff[2].bias)
        else:
            ff = blk.ff(blk.norm2(x1))
        return x1 + ff


@pytest.mark.parametrize("cid", [c.id for c in MODULE_CASES])
def test_module_trains_on_its_own_rows(cid, gpu_device, monkeypatch):
    case = MODULE_BY_ID[cid]
    dev = gpu_device
    rec = aus.Recorder(monkeypatch)
    rig = _rig(case, dev, rec)
    a = rig.step()
    # the bf16 tiles of a bf16 module on the same inputs: the error class the bound is taken from
    twin = _rig(case, dev, rec, precision="bf16", tiles="bf16").step()
    fig, fig16 = _errors(case, a), _errors(case, twin)
    print(f"train16 {cid}: " + ", ".join(f"{k} {v:.3e} (bf16 {fig16[k]:.3e})" for k, v in fig.items()))
    bad = {k: (v, fig16[k]) for k, v in fig.items() if v > min(ts.CLASS_FACTOR * fig16[k], ts.TENSOR_16)}
    assert not bad, f"{cid}: error over min(2 x the bf16 tiles', 0.15) of the tensor's scale (error, bf16 error): {bad}"
    # the training forward is the staged inference pipeline of the precision, bit for bit
    n0 = len(rec.calls)
    staged = _staged_forward(case, rig)
    del rec.calls[n0:]
    assert torch.equal(staged.cpu(), a.out), f"{cid}: max |diff| {float((staged.cpu() - a.out).abs().max()):.3e}"
    # two runs are bit-identical
    b = rig.step()
    assert torch.equal(a.out, b.out)
    aus.same(case, "mixed16", "repeat", b.grads, a.grads)
    # any leaf subset receives the gradient it has when all require grad
    subsets = aus.subsets(case)
    for name in ("inputs-only", "params-only", "all-but-v", f"only-{rig.input_names[-1]}"):
        req = subsets[name]
        run = rig.step(req=req)
        want = {nm: (a.grads[nm] if nm in req else None) for nm in a.grads}
        aus.same(case, "mixed16", f"subset {name}", run.grads, want)
    # create_graph=True is refused
    ins = rig.leaves()
    out = rig.call(*(ins[nm] for nm in rig.input_names))
    del rec.calls[:]
    with pytest.raises(RuntimeError, match="not differentiable"):
        torch.autograd.grad(out.sum(), [ins[rig.input_names[0]]], create_graph=True)


@pytest.mark.parametrize("cid", ["m16-op-b100-t3", "m16-src-b8-t3", "m16-blk-b128-t3"])
def test_default_training_is_unchanged(cid, gpu_device, monkeypatch):
    """With train_tiles left alone (and with "bf16", which this precision ignores) the module trains as precision
    "fp32_diff" does, bit for bit: the f32 difference-form kernels on f32 rows."""
    case = MODULE_BY_ID[cid]
    rec = aus.Recorder(monkeypatch)
    base = aus.Rig(case, "fp32_diff", gpu_device, rec).step()
    for tiles in ("fp32", "bf16"):
        run = _rig(case, gpu_device, rec, tiles=tiles).step()
        assert torch.equal(run.out, base.out), (cid, tiles)
        aus.same(case, tiles, "default", run.grads, base.grads)
