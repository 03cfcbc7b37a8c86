"""The 16-bit difference-form training path (``HEPTAttention.train_tiles = "mixed16"`` under ``precision="mixed16_diff"``,
csrc/block_attn_bwd_coords.hip): cases, float64 yardsticks and checks, run by tests/test_gpu_train_mixed16.py, the coverage
pinned on the CPU by tests/test_train_mixed16_host.py.  A plain module, not a conftest; nothing here touches the GPU at
import time.

Exact cells: the design of tests/block_sweep.py's backward cells (one-hot groups with weights exactly 0 or 1 on injected
permutations, a neighbouring block's key baited at every block boundary) on every instantiation of the new kernel --
tile counts 1 .. 8, full and ragged, C = 2, 4, 6 compile-time and the runtime path, D = 24 (the forward's packed partial
rows) and other D (f32 partial rows): dq, dk, the coordinate gradient and d sqrt_w exactly 0, dv exact.  Random cells: one
per instantiation, against float64 autograd of the difference-form operator on the stored rounded rows, with the bf16
backward on the same cell as the measure of the error class."""
from collections import namedtuple

import torch

import block_sweep as bs
import shape_sweep as sw

H, TL = bs.H, bs.TL
CTS = (2, 4, 6, 0)           # compile-time coordinate counts of block_attn_bwd_coords_kernel; 0: the runtime path
# (D, C) a CT rotates over: D = 24 and other D; (2, 28) is the widest row (H * C = 84 > 64: d sqrt_w summed in torch).  The
# rotations keep it off the eight-tile blocks, where C >= 26 needs more LDS than a CU has (refused: HEPT_ERR_SHAPE); at
# B = 223 it is the largest LDS request of the sweep, 148 KB
PAIRS = {2: [(24, 2), (27, 2), (8, 2)], 4: [(24, 4), (8, 4), (20, 4)], 6: [(24, 6), (17, 6), (3, 6)],
         0: [(24, 3), (24, 5), (20, 5), (2, 28), (17, 3)]}
LDS_MAX = 160 * 1024


def lds_bytes(b, c):
    """csrc/block_attn_bwd_coords.hip: bwdc_lds"""
    nkt = (b + 31) // 32
    cs = {2: 2, 4: 4, 6: 8}.get(c, c)
    return 5 * 32 * nkt * 64 + 32 * nkt * 20 + 3 * 32 * nkt * cs * 4


TENSOR_16 = 0.15             # the project's bound for 16-bit training tiles (tests/test_gpu_backward.py:307)
# against the bf16 backward on the same cell: both kernels round P and dS to bf16 and write bf16 per-table rows (the new one
# keeps G in two bf16 pieces and q^ / k^ at fp16, so it can only be the more accurate of the two); the factor covers the
# summation order
CLASS_FACTOR = 2.0


def ct_of(c):
    return c if c in (2, 4, 6) else 0   # csrc/block_attn_bwd_coords.hip: hept_block_attn_bwd_coords


def cells(case):
    nkt = (case.B + 31) // 32
    return (ct_of(case.C), nkt, case.B == 32 * nkt)


def all_instantiations():
    return {(ct, nkt, full) for ct in CTS for nkt in range(1, 9) for full in (True, False)}


def _exact_cases():
    out = []
    for ct in CTS:
        for nkt in range(1, 9):
            for ki, kind in enumerate(("full", "one" if nkt % 2 else "short")):
                d, c = PAIRS[ct][(2 * nkt + ki) % len(PAIRS[ct])]
                b = bs.block_of(nkt, kind)
                out.append(bs.Case(f"m16bwd-ct{ct}-k{nkt}{kind}-b{b}-d{d}c{c}", "m16bwd", nkt, kind, b, d, c, "bwd", None))
    for ct, nkt, kind, (d, c) in ((2, 3, "short", (24, 2)), (4, 2, "full", (8, 4)), (6, 5, "short", (24, 6))):
        b = bs.block_of(nkt, kind)   # coordinates beyond the fp16 range: |sqrt_w coords| multiples of 2^17
        out.append(bs.Case(f"m16bwd-ct{ct}-k{nkt}{kind}-b{b}-d{d}c{c}-big", "m16bwd", nkt, kind, b, d, c, "big", None))
    b = bs.block_of(2, "short")      # raw_size < N (N - B - 1): padding rows with a non-zero upstream gradient
    out.append(bs.Case(f"m16bwd-ct6-k2short-b{b}-d24c6-raw{2 * b - 1}", "m16bwd", 2, "short", b, 24, 6, "raw", 2 * b - 1))
    return out


EXACT = _exact_cases()
EXACT_BY_ID = {c.id: c for c in EXACT}

RandomCase = namedtuple("RandomCase", "id ct nkt kind shape")


def _random_cases():
    out = []
    for ct in CTS:
        for nkt in range(1, 9):
            for ki, kind in enumerate(("full", "short")):
                d, c = PAIRS[ct][(2 * nkt + ki + 3) % len(PAIRS[ct])]
                b = bs.block_of(nkt, kind)
                cid = f"m16bwd-ct{ct}-k{nkt}{kind}-b{b}-d{d}c{c}-f64"
                out.append(RandomCase(cid, ct, nkt, kind, sw.Shape(cid, (3 * b,), b, TL, H, d, c, 9000 + len(out), True)))
    return out


RANDOM = _random_cases()
RANDOM_BY_ID = {c.id: c for c in RANDOM}


def random_cells(rc):
    s = rc.shape
    return cells(bs.Case(rc.id, "m16bwd", rc.nkt, rc.kind, s.B, s.D, s.C, "f64", None))


# ---------------------------------------------------------------------------------------------------------------------
# exact cells (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def check_exact(case, dev):
    import dense_sweep as ds
    from hept_amd import _lib, ops

    d = bs.bwd_design(case)
    n, dd, c, raw = d["n"], case.D, case.C, d["raw"]
    g = {k: d[k].to(dev) for k in ("q", "k", "v", "coords", "sqrt_w", "alpha", "qpos", "kpos", "gacc")}
    ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], g["sqrt_w"], g["alpha"], None, "mixed16", raw_size=raw)
    nan = float("nan")
    dq_part = torch.full((TL, n, H, 32), nan, device=dev, dtype=torch.bfloat16)
    dkv_part = torch.full((TL, n, H, 64), nan, device=dev, dtype=torch.bfloat16)
    if case.variant == "big":
        assert float((g["coords"][:, None, :] * g["sqrt_w"][None]).abs().max()) > 65504.0
    if case.variant == "raw":
        assert raw < n and float(g["gacc"][raw:].abs().max()) > 0.0
    with torch.cuda.device(dev):
        rc = _lib.load().hept_block_attn_bwd_coords(
            ph["qhat"].data_ptr(), ph["kvhat"].data_ptr(), g["qpos"].data_ptr(), g["kpos"].data_ptr(), g["gacc"].data_ptr(),
            g["coords"].data_ptr(), g["sqrt_w"].data_ptr(), raw, n, H, dd, c, TL, case.B, dq_part.data_ptr(),
            dkv_part.data_ptr(), ops.current_stream_ptr(dev))
    assert rc == 0, (case.id, rc)
    want_dsw = H * c <= 64
    rc, dq, dk, dv, dcs, dsw = ds.bwd_reduce_call(True, dq_part, dkv_part, TL, n, H, dd, c, g["coords"], raw, want_dsw)
    assert rc == 0, (case.id, rc)
    torch.cuda.synchronize()
    for name, x in (("dq", dq), ("dk", dk), ("dcs", dcs), ("dv", dv)) + ((("d_sqrt_w", dsw),) if want_dsw else ()):
        assert bool(torch.isfinite(x).all()), f"{case.id}: {name} is not finite"
    for name, x in (("dq", dq), ("dk", dk), ("dcs", dcs)) + ((("d_sqrt_w", dsw),) if want_dsw else ()):
        bad = ~(x == 0)
        assert not bool(bad.any()), f"{case.id}: {name} must be exactly 0, {int(bad.sum())} elements are not, first at " \
                                    f"{tuple(bad.nonzero()[0].tolist())}: {x[tuple(bad.nonzero()[0].tolist())].item()!r}"
    want = d["dv"].clone()
    want[raw:] = 0.0            # the padding rows' own gradients
    bs._same(dv.cpu(), want, f"{case.id}: dv (point, head x column)")
    # the public entry on the same cell: the same bits
    got = ops.block_attn_bwd_coords(ph["qhat"], ph["kvhat"], g["qpos"], g["kpos"], g["gacc"], g["coords"], g["sqrt_w"], dd,
                                    case.B, raw_size=raw)
    assert torch.equal(got[2], dv) and not bool((got[0] != 0).any()) and not bool((got[4] != 0).any()), case.id


# ---------------------------------------------------------------------------------------------------------------------
# float64 yardsticks
# ---------------------------------------------------------------------------------------------------------------------
def tensor_err(a, r):
    return float((a.double().cpu() - r).abs().max()) / (float(r.abs().max()) + 1e-300)


def ref64_rows(qf, kf, vf, cq, ck, coords, qpos, kpos, b, gacc):
    """float64 autograd of the block attention of the given float64 rows (features (H, N, D), scaled coordinates
    (H, N, C) per role) on the given permutations, summed over the tables, against the upstream rows gacc (N, H, 32): dq,
    dk, dv (N, H * D), dcs (N, H * C) (both roles' coordinate gradients added) and d sqrt_w (H, C) = sum_n dcs * coords.
    In float64 the expanded logit is the difference form to 1e-12."""
    import hept_oracle as ho

    h, n, d = qf.shape
    qf, kf, vf, cq, ck = (x.double().clone().requires_grad_(True) for x in (qf, kf, vf, cq, ck))
    qp, kp = qpos.long().cpu(), kpos.long().cpu()
    den, num = ho.block_rbf_attention(ho.gather_blocks(torch.cat([qf, cq], -1), qp, b),
                                      ho.gather_blocks(torch.cat([kf, ck], -1), kp, b), ho.gather_blocks(vf, kp, b))
    num, den = ho.unsort_tables(num, qp).sum(0), ho.unsort_tables(den, qp).sum(0)
    g64 = gacc.double().cpu().permute(1, 0, 2)
    ((num * g64[..., :d]).sum() + (den[..., 0] * g64[..., d]).sum()).backward()
    flat = lambda x: x.permute(1, 0, 2).reshape(n, -1)                             # noqa: E731
    dcs = (cq.grad + ck.grad).permute(1, 0, 2)                                     # (N, H, C)
    return dict(dq=flat(qf.grad), dk=flat(kf.grad), dv=flat(vf.grad), dcs=dcs.reshape(n, -1),
                dsw=(dcs * coords.double().cpu()[:, None, :]).sum(0))


def check_random(rc, dev):
    """The new backward on a random cell against float64 on its own stored rows; the bf16 backward on the same cell (the
    coordinates of shape_sweep.inputs are inside its valid range) against float64 on ITS stored rows.  Returns
    {tensor: (error, bf16 error)} after asserting error <= min(2 x bf16 error, 0.15) per tensor (dq, dk, dv, dcs, d sqrt_w)."""
    from hept_amd import ops

    s = rc.shape
    inp = sw._cached((s.id, "inp"), lambda: sw.inputs(s))
    g = sw._cached((s.id, "gpu"), lambda: sw._gpu(inp, dev))
    n, d, c = g["q"].shape[0], s.D, s.C
    sqrt_w = ops.rpe_scale(g["w_rpe_weight"], s.H, d, 10)
    gacc = torch.zeros(n, s.H, 32)
    gacc[..., :d + 1] = torch.randn(n, s.H, d + 1, generator=torch.Generator().manual_seed(s.seed))
    gacc = gacc.to(dev)
    cs64 = (sqrt_w.double().cpu()[None] * inp["coords"].double()[:, None]).permute(1, 0, 2)      # (H, N, C)

    ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sqrt_w, g["alpha"], g["combined_shifts"], "mixed16")
    qpos, kpos = ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"])
    got = ops.block_attn_bwd_coords(ph["qhat"], ph["kvhat"], qpos, kpos, gacc, g["coords"], sqrt_w, d, s.B)
    torch.cuda.synchronize()
    qh, kvh = ph["qhat"].cpu(), ph["kvhat"].cpu()
    v16 = kvh[..., 32:].contiguous().view(torch.bfloat16)
    want = ref64_rows(qh[..., :d], kvh[..., :d], v16[..., :d], cs64, cs64, inp["coords"], qpos, kpos, s.B, gacc)

    ph16 = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sqrt_w, g["alpha"], g["combined_shifts"], "bf16")
    qpos16, kpos16 = ops.sort_tables(ph16["qproj"], ph16["kproj"], g["combined_shifts"], ph16["minmax"])
    got16 = ops.block_attn_bwd(ph16["qhat"], ph16["kvhat"], qpos16, kpos16, gacc, d, c, s.B, coords=g["coords"]) \
        if s.H * c <= 64 else ops.block_attn_bwd(ph16["qhat"], ph16["kvhat"], qpos16, kpos16, gacc, d, c, s.B)
    torch.cuda.synchronize()
    q16, kv16 = ph16["qhat"].cpu(), ph16["kvhat"].cpu()
    want16 = ref64_rows(q16[..., :d], kv16[..., :d], kv16[..., 32:32 + d], q16[..., d:d + c], kv16[..., d:d + c],
                        inp["coords"], qpos16, kpos16, s.B, gacc)

    names = ("dq", "dk", "dv", "dcs", "dsw")
    fig = {}
    for i, nm in enumerate(names):
        a = got[i]
        assert bool(torch.isfinite(a).all()), (s.id, nm)
        if nm == "dsw" and len(got16) < 5:
            a16 = (got16[3] * g["coords"][:, None, :]).sum(0)
        else:
            a16 = got16[i]
        fig[nm] = (tensor_err(a.reshape(want[nm].shape), want[nm]), tensor_err(a16.reshape(want16[nm].shape), want16[nm]))
    print(f"train16 {s.id}: " + ", ".join(f"{k} {v[0]:.3e} (bf16 {v[1]:.3e})" for k, v in fig.items()))
    bad = {k: v for k, v in fig.items() if v[0] > min(CLASS_FACTOR * v[1], TENSOR_16)}
    assert not bad, f"{s.id}: error over min(2 x the bf16 backward's, 0.15) (error, bf16 error): {bad}"
    return fig
