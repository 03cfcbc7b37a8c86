"""Deterministic shape sweep: every element of the HIP operator, forward and backward, against a float64 evaluation of the
reference arithmetic on the GPU's own permutations (run by tests/test_gpu_shape_sweep.py, coverage pinned on CPU by
tests/test_shape_sweep_cells.py).  A plain module, not a conftest: pytest's default import mode puts tests/ on the path.

``SHAPES`` holds hand-picked cells (every block-size tile count FULL and ragged, point counts around the one-workgroup
sort's capacity, table counts across the 8-table chunk, tuned and free head shapes, clouds of exactly B and B + 1 points)
and seeded random draws built like tests/op_stress.py's.  ``cells(shape)`` names the dispatch branches a shape takes,
mirroring the rules in csrc/.  Nothing here touches the GPU at import time."""
import os
from collections import namedtuple

import torch

Shape = namedtuple("Shape", "id sizes B T H D C seed bwd")

MAX_TABLES = 8          # HEPT_MAX_TABLES (include/hept_hip.h): prep_hash and the sort take at most this many tables
SMALL_CAP = 6144        # csrc/sort_tables.hip:961: N <= SMALL_CAP sorts each segment in one workgroup
REGION_MAX_N = 131072   # csrc/sort_tables.hip:179: the small-tile bucket kernel's range (the riders' range)
TUNED = [(24, 6), (24, 4), (24, 2), (16, 6), (16, 4), (8, 4)]   # H = 8 with these: csrc/prep_hash.hip:802-807
FREE = [(4, 24, 6), (16, 24, 6), (16, 12, 3), (2, 27, 3), (5, 20, 5), (12, 8, 4), (1, 24, 6), (3, 10, 6), (16, 16, 4),
        (7, 17, 3)]     # the free head shapes of tests/op_stress.py
# precision ids of the forward sweep: (ops precision, block_attn's f32_mfma argument, HEPT_DIFF_MFMA)
PRECISIONS = {
    "fp32": ("fp32", False, None),
    "fp32_mfma": ("fp32_mfma", True, None),
    "fp32_diff_split": ("fp32_diff", "diff", "0"),
    "fp32_diff_mfma": ("fp32_diff", "diff", "1"),
    "bf16": ("bf16", False, None),
    "mixed16": ("mixed16", False, None),
}
TRAIN_TILES = ("fp32", "bf16")
# float64 elements of the oracle's largest intermediate (T, H, N/B, B, B): keeps one shape's oracle within ~0.5 GB
COST_CAP = 2.5e7


def n_points(s):
    """make_inputs pads every cloud to a multiple of B."""
    return sum(-(-n // s.B) * s.B for n in s.sizes)


def _hand():
    out = []

    def add(name, sizes, b, t, h, d, c, bwd=False):
        out.append(Shape(name, tuple(sizes), b, t, h, d, c, 500 + len(out), bwd))

    # every tile count nkt = ceil(B/32) 1..8, FULL (B = 32 nkt) and ragged; several clouds, the tuned (D, C) in turn
    add("b8", [200, 77], 8, 2, 8, 24, 6, bwd=True)
    add("b31", [31 * 5, 31 * 3 + 5], 31, 3, 8, 24, 4)
    add("b32", [32 * 9], 32, 1, 8, 24, 2, bwd=True)
    add("b33", [33 * 4 + 1, 70], 33, 2, 8, 16, 6, bwd=True)
    add("b64", [64 * 6, 100], 64, 8, 8, 16, 4, bwd=True)
    add("b65", [65 * 4, 65 * 2 + 9], 65, 9, 8, 8, 4, bwd=True)
    add("b96", [96 * 5, 200], 96, 2, 8, 24, 6, bwd=True)
    add("b97", [97 * 3 + 10, 97 * 2], 97, 2, 8, 24, 4)
    add("b100", [1000, 377, 250], 100, 3, 8, 24, 6, bwd=True)
    add("b128", [128 * 7], 128, 1, 8, 24, 2, bwd=True)
    add("b129", [129 * 4, 129], 129, 2, 8, 16, 6, bwd=True)
    add("b160", [160 * 3 + 50, 160 * 2], 160, 3, 8, 16, 4, bwd=True)
    add("b180", [180 * 3, 200], 180, 2, 8, 8, 4, bwd=True)
    add("b192", [192 * 4], 192, 2, 8, 24, 6, bwd=True)
    add("b200", [200 * 3 + 1, 300], 200, 2, 8, 24, 4, bwd=True)
    add("b224", [224 * 3, 230], 224, 1, 8, 24, 6, bwd=True)
    add("b225", [225 * 3, 225 * 2 + 100], 225, 2, 8, 24, 2, bwd=True)
    add("b255", [255 * 4], 255, 1, 8, 16, 6)
    add("b256", [256 * 2 + 10, 256], 256, 2, 8, 24, 6, bwd=True)
    # point counts around the one-workgroup sort's capacity (multiples of B), and ~9000 (two-launch sort, riders)
    add("n6016", [6016], 128, 2, 8, 24, 6)
    add("n6144", [3072, 3072], 128, 3, 8, 24, 6)
    add("n6272", [6272], 128, 1, 8, 24, 6, bwd=True)
    add("n9000", [9000], 100, 2, 8, 24, 6)
    add("n9000-b225", [4500, 4500], 225, 1, 8, 8, 4)
    # tables: 17 (three chunks), 9 beside two-launch sorts (the chunk copy of run_begin)
    add("t17", [1280], 64, 17, 8, 16, 4)
    add("t9-n6272", [6272], 128, 9, 3, 16, 4, bwd=True)
    # free head shapes (generic row builder, generic-D combine, the torch d sqrt_w at H*C > 64)
    add("h1d24c6", [700, 300], 100, 2, 1, 24, 6)
    add("h16d27c3", [33 * 10, 33 * 3 + 2], 33, 3, 16, 27, 3, bwd=True)
    add("h5d20c5", [6400], 160, 2, 5, 20, 5, bwd=True)
    add("h7d17c3", [97 * 6 + 3], 97, 2, 7, 17, 3, bwd=True)
    add("h3d10c6", [255 * 3, 400], 255, 2, 3, 10, 6)
    add("h16d8c4", [64 * 8, 64 * 3 + 1], 64, 2, 16, 8, 4)
    add("h16d24c6", [64 * 6, 130], 64, 2, 16, 24, 6, bwd=True)
    # a cloud of exactly B points beside one of B + 1 (its second block holds one real point and B - 1 pad copies)
    add("cloud-b-b1-100", [100, 101, 300], 100, 2, 8, 24, 6, bwd=True)
    add("cloud-b-b1-225", [225, 226], 225, 3, 8, 16, 4)
    return out


def _random(count=30):
    """Seeded draws as tests/op_stress.py makes them: B in 8..256, 1..8 tables, 1..3 clouds of B..4B+39 points, the tuned
    pairs with every third draw a free head shape.  The table count is lowered where the float64 oracle would be large."""
    g = torch.Generator().manual_seed(4242)
    out = []
    for it in range(count):
        h, (d, c) = 8, TUNED[it % len(TUNED)]
        if it % 3 == 2:
            h, d, c = FREE[(it // 3) % len(FREE)]
        b = int(torch.randint(8, 257, (1,), generator=g))
        t = int(torch.randint(1, 9, (1,), generator=g))
        n_clouds = int(torch.randint(1, 4, (1,), generator=g))
        sizes = tuple(int(torch.randint(b, 4 * b + 40, (1,), generator=g)) for _ in range(n_clouds))
        s = Shape(f"r{it:02d}", sizes, b, t, h, d, c, 3000 + it, it % 10 == 0)
        while s.T > 1 and s.T * s.H * n_points(s) * s.B > COST_CAP:
            s = s._replace(T=s.T - 1)
        out.append(s._replace(id=f"r{it:02d}-b{b}-t{s.T}-h{h}d{d}c{c}"))
    return out


SHAPES = _hand() + _random()
BY_ID = {s.id: s for s in SHAPES}
BWD_SHAPES = [s for s in SHAPES if s.bwd]


def riders(n, h, d, t, precision, b):
    """run_begin (csrc/capi.hip:135-138): the bucket-sort launch writes the v rows (hept_sort_carries_rows,
    csrc/sort_tables.hip:1304) unless the f32 split kernel reads v in place (direct v)."""
    carries = SMALL_CAP < n <= REGION_MAX_N and 4 <= d <= 28 and d % 4 == 0 and h >= 1
    f32_rows = precision.startswith("fp32")
    return not direct_v(d, precision, b) and t <= MAX_TABLES and (t >= 2 or f32_rows) and carries


def direct_v(d, precision, b):
    """csrc/capi.hip:104,135: precision "fp32" (HEPT_PREC_F32 only), B > 128, D % 4 == 0."""
    return precision == "fp32" and b > 128 and d % 4 == 0


def cells(s):
    """Names of the dispatch branches the shape takes; precision-dependent ones as "<branch>:<precision id>"."""
    n = n_points(s)
    nkt = -(-s.B // 32)                                            # csrc/block_attn.hip:786
    out = {f"nkt{nkt}-{'full' if s.B == 32 * nkt else 'ragged'}",  # launch_attn / launch_attn_split: B == 32 nkt
           "sort-two-launch" if n > SMALL_CAP else "sort-one-workgroup",   # csrc/sort_tables.hip:1340
           "rows-tuned" if s.H == 8 and (s.D, s.C) in TUNED else "rows-generic",   # csrc/prep_hash.hip:802
           "table-chunks" if s.T > MAX_TABLES else "tables-one-chunk",          # csrc/capi.hip:141-160
           "clouds-one" if len(s.sizes) == 1 else "clouds-several"}
    if s.B in s.sizes:
        out.add("cloud-of-B")
    if s.B + 1 in s.sizes:
        out.add("cloud-of-B+1")
    for p in PRECISIONS:
        if riders(n, s.H, s.D, s.T, p, s.B):
            out.add(f"riders:{p}")
        if direct_v(s.D, p, s.B):
            out.add(f"direct-v:{p}")
        sixteen = p in ("bf16", "mixed16")
        out.add(f"{'part-packed' if sixteen and s.D == 24 else 'part-f32'}:{p}")    # hept_part_precision, capi.hip
    if s.D == 24:
        out.add("diff-split-kernel")                               # csrc/block_attn.hip:815-823
    if s.bwd:
        out.add("bwd-dsw-torch" if s.H * s.C > 64 else "bwd-dsw-kernel")   # hept_amd/autograd.py:137-141
    return out


# ---------------------------------------------------------------------------------------------------------------------
# GPU checks (imports deferred: the CPU suite imports this module without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
# fp32 tiles: atol / rtol on every element against float64
ATOL, RTOL = 1e-5, 1e-4
ILL_WEIGHT = 1e-6   # a row whose float64 total weight (any head) is below this would be ill-conditioned: none allowed
# 16-bit modes against the oracle's model of their arithmetic (same rounded tiles, f32 accumulation): worst row error
# over (row max |model| + 1e-3), set at <= 2x the measured worst row of the sweep on the MI355X
# (measured worst row: bf16 6.96e-3, mixed16 5.93e-3, both at n9000-b225)
MODEL16_ROW = {"bf16": 1.2e-2, "mixed16": 1.1e-2}
# backward: per row, max |a - r| <= X * (row max |r| + 1e-2 * tensor max |r|), X set at <= 2x the measured worst row
# (measured worst row: fp32 tiles 2.75e-5 at b128, bf16 tiles 0.210 at b8 -- the dq rows of the tight B = 8 blocks, where
# k^ - q^ is comparable to the bf16 spacing of the rows; see tests/test_gpu_backward.py)
BWD_ROW_X = {"fp32": 5e-5, "bf16": 0.4}
# the coordinate gradient per row: a sum of terms that cancel down to the difference of neighbouring points' scaled
# coordinates (the backward differentiates the expanded logit), worst at C = 2 where sqrt_w is largest (measured worst
# row: fp32 tiles 8.2e-5 at b225, bf16 tiles 0.166 at b225)
DCOORDS_ROW_X = {"fp32": 1.6e-4, "bf16": 0.33}
# bf16 training tiles, per tensor (tests/test_gpu_backward.py test_bf16_training_tiles_with_other_head_counts)
BF16_TENSOR = {"out": 0.05, "dq": 0.4, "dk": 0.25, "dv": 0.05, "dw_rpe": 0.35, "dW_out": 0.05, "db_out": 0.05,
               "dcoords": 0.025}   # (dcoords: measured worst 1.2e-2)
FP32_TENSOR = 2e-4    # tests/test_gpu_backward.py _close

_cache = {}


def inputs(s):
    """CPU inputs of a shape (float32), scaled as tests/op_stress.py scales them."""
    from hept_amd.synthetic import make_inputs

    inp = make_inputs(list(s.sizes), block_size=s.B, n_hashes=s.T, coords_dim=s.C, h_dim=s.D, num_heads=s.H,
                      seed=s.seed)
    inp["q"], inp["k"] = inp["q"] * 0.3, inp["k"] * 0.3
    inp["coords"] = inp["coords"] * 0.2
    assert inp["q"].shape[0] == n_points(s)
    return inp


def _cached(key, make):
    """One shape at a time (the parametrisation is shape-major): drop everything of the previous shape."""
    if key[0] != _cache.get("shape"):
        _cache.clear()
        _cache["shape"] = key[0]
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _gpu(inp, dev):
    return {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}


def staged(s, g, precision):
    """prep_hash -> sort_tables (chunks of MAX_TABLES tables, rows reused) -> block_attn -> combine_out.  Checks that
    every chunk's permutations are torch's stable sort of the GPU's own keys."""
    from hept_amd import ops

    prec, f32_mfma, _ = PRECISIONS[precision]
    n = g["q"].shape[0]
    sw = ops.rpe_scale(g["w_rpe_weight"], s.H, s.D, 10)
    rows, qs, ks = None, [], []
    for c0 in range(0, s.T, MAX_TABLES):
        tc = min(MAX_TABLES, s.T - c0)
        ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sw, g["alpha"], g["combined_shifts"], prec, t0=c0, tl=tc,
                           rows=rows)
        rows = (ph["qhat"], ph["kvhat"])
        qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"], t0=c0)
        mm = ph["minmax"]
        span = mm[..., 1].amax(-1) - mm[..., 0].amin(-1)
        offs = g["combined_shifts"][c0:c0 + tc].float() * span[..., None]
        for pos, proj in ((qp, ph["qproj"]), (kp, ph["kproj"])):
            assert torch.equal(pos.long(), torch.sort(proj + offs, dim=-1, stable=True).indices), (s.id, precision, c0)
            assert torch.equal(torch.sort(pos.long(), -1).values, torch.arange(n, device=pos.device).expand_as(pos))
        qs.append(qp)
        ks.append(kp)
    qpos, kpos = torch.cat(qs), torch.cat(ks)
    part = ops.block_attn(rows[0], rows[1], qpos, kpos, s.D, s.B, f32_mfma=f32_mfma)
    out = ops.combine_out(part, s.D, g["out_weight"], g["out_bias"])
    return dict(out=out, part=part, qpos=qpos, kpos=kpos)


def _oracle64(s, inp, qp, kp, **kw):
    import hept_oracle as ho

    d64 = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items() if torch.is_tensor(v)}
    return ho.forward(d64["q"], d64["k"], d64["v"], d64["coords"], d64["combined_shifts"], d64["w_rpe_weight"],
                      d64["alpha"], d64["out_weight"], d64["out_bias"], block_size=s.B, w_per_dist=10, q_positions=qp,
                      k_positions=kp, **kw)


def _reference(s, inp, qpos, kpos):
    """float64 oracle on the GPU permutations (cached per permutation pair), with the conditioning and sortedness checks
    that depend on the permutations only."""
    from test_gpu_parity import _almost_sorted

    qp, kp = qpos.long().cpu(), kpos.long().cpu()
    for r in (v for key, v in _cache.items() if key != "shape" and key[1] == "ref64"):
        if torch.equal(r["q_positions"], qp) and torch.equal(r["k_positions"], kp):
            return r
    r = _oracle64(s, inp, qp, kp, keep=True)
    # the GPU's order is sorted under the oracle's (float64) keys up to the round-off of the fp32 hash
    hash_scale = float(r["q_hashed"].abs().max())
    for pos, keys in ((qp, r["q_keys"]), (kp, r["k_keys"])):
        tol = 8e-6 * hash_scale + 4 * 2.0 ** -23 * float(keys.abs().max())
        assert _almost_sorted(keys, pos, tol) <= tol, s.id
    total = r["denom"].sum(0).squeeze(-1)          # (H, N): every table's weight of the row
    ill = int((total < ILL_WEIGHT).any(0).sum())
    assert ill == 0, f"{s.id}: {ill} rows with total weight < {ILL_WEIGHT}: rescale the shape"
    r = dict(out=r["out"], q_positions=qp, k_positions=kp)
    _cache[(s.id, "ref64", len(_cache))] = r
    return r


def _row_scaled(out, ref):
    return float(((out.double() - ref.double()).abs().amax(-1) / (ref.double().abs().amax(-1) + 1e-3)).max())


def check_forward(s, precision, dev):
    """Every element of the staged kernels against float64 on their own permutations; the one-call operator must be
    bit-identical to the staged kernels.  Returns the worst error (fp32: multiple of the tolerance; 16-bit: row-scaled
    against float64 and against the oracle's model)."""
    import hept_oracle as ho
    from hept_amd import ops
    from test_gpu_parity import REL16_ALL_ROWS_FULL, _model_kw

    prec, _, env = PRECISIONS[precision]
    inp = _cached((s.id, "inp"), lambda: inputs(s))
    g = _cached((s.id, "gpu"), lambda: _gpu(inp, dev))
    old = os.environ.get("HEPT_DIFF_MFMA")
    if env is not None:
        os.environ["HEPT_DIFF_MFMA"] = env
    try:
        st = staged(s, g, precision)
        one = ops.forward(g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"],
                          g["out_weight"], g["out_bias"], block_size=s.B, w_per_dist=10, precision=prec)
        torch.cuda.synchronize()
    finally:
        if env is not None:
            if old is None:
                os.environ.pop("HEPT_DIFF_MFMA", None)
            else:
                os.environ["HEPT_DIFF_MFMA"] = old
    out = st["out"].cpu()
    assert bool(torch.isfinite(out).all()), (s.id, precision)
    assert torch.equal(one.cpu(), out), f"{s.id} {precision}: one-call forward differs from the staged kernels"
    # partial rows: positive denominators, the unused columns exactly zero
    wide = ops.unpack_part(st["part"])
    assert bool((wide[..., s.D] > 0).all()), (s.id, precision)
    assert float(wide[..., s.D + 1:].abs().max()) == 0.0, (s.id, precision)
    if st["part"].dtype == torch.int32:
        assert float(st["part"][..., 13:].abs().max()) == 0.0, (s.id, precision)
    ref = _reference(s, inp, st["qpos"], st["kpos"])["out"]
    if prec.startswith("fp32"):
        x = float(((out.double() - ref).abs() / (ATOL + RTOL * ref.abs())).max())
        bad = ~((out.double() - ref).abs() <= ATOL + RTOL * ref.abs())
        where = [tuple(i) for i in bad.nonzero()[:5].tolist()]
        assert x <= 1.0, f"{s.id} {precision}: worst element {x:.3f}x the tolerance, first (row, col): {where}"
        return dict(x=x)
    w64 = _row_scaled(out, ref)
    assert w64 <= REL16_ALL_ROWS_FULL[prec], f"{s.id} {precision}: worst row-scaled error vs float64 {w64:.3e}"
    qp, kp = st["qpos"].long().cpu(), st["kpos"].long().cpu()
    model = ho.forward(inp["q"], inp["k"], inp["v"], inp["coords"], inp["combined_shifts"], inp["w_rpe_weight"],
                       inp["alpha"], inp["out_weight"], inp["out_bias"], block_size=s.B, w_per_dist=10, q_positions=qp,
                       k_positions=kp, keep=False, **_model_kw(prec))["out"]
    wm = _row_scaled(out, model)
    assert wm <= MODEL16_ROW[prec], f"{s.id} {precision}: worst row-scaled error vs the 16-bit model {wm:.3e}"
    return dict(row64=w64, model=wm)


def train_once(s, inp, tiles, dev):
    """HEPTAttention in train mode (as tests/test_gpu_backward.py _train_once), the bias gradient included."""
    from hept_amd import HEPTAttention

    m = HEPTAttention(s.D + s.C, h_dim=s.D, num_heads=s.H, block_size=s.B, n_hashes=s.T, num_w_per_dist=10)
    m.load_state_dict({"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"],
                       "e2lsh.alpha": inp["alpha"]}, strict=True)
    m = m.to(dev).train()
    m.train_tiles = tiles
    w_rpe = torch.nn.Linear(inp["w_rpe_weight"].shape[1], inp["w_rpe_weight"].shape[0]).to(dev)
    with torch.no_grad():
        w_rpe.weight.copy_(inp["w_rpe_weight"])
    q, k, v, coords = (inp[x].to(dev).requires_grad_(True) for x in ("q", "k", "v", "coords"))
    out = m(q, k, v, w_rpe=w_rpe, coords=coords, combined_shifts=inp["combined_shifts"].to(dev))
    out.backward(_g_out(out.shape).to(dev))
    return dict(zip(("out", "dq", "dk", "dv", "dw_rpe", "dW_out", "db_out", "dcoords"),
                    (x.detach().cpu() for x in (out, q.grad, k.grad, v.grad, w_rpe.weight.grad,
                                                m.out_linear.weight.grad, m.out_linear.bias.grad, coords.grad))))


def _g_out(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(5))


def _grads64(s, inp, qp, kp):
    import hept_oracle as ho

    d64 = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items() if torch.is_tensor(v)}
    leaves = {k: d64[k].clone().requires_grad_(True)
              for k in ("q", "k", "v", "w_rpe_weight", "out_weight", "out_bias", "coords")}
    res = ho.forward(leaves["q"], leaves["k"], leaves["v"], leaves["coords"], d64["combined_shifts"], leaves["w_rpe_weight"],
                     d64["alpha"], leaves["out_weight"], leaves["out_bias"], block_size=s.B, w_per_dist=10,
                     q_positions=qp, k_positions=kp, keep=False, grad=True)
    res["out"].backward(_g_out(res["out"].shape).double())
    names = dict(q="dq", k="dk", v="dv", w_rpe_weight="dw_rpe", out_weight="dW_out", out_bias="db_out",
                 coords="dcoords")
    want = {names[k]: t.grad for k, t in leaves.items()}
    want["out"] = res["out"].detach()
    return want


def row_x(a, r):
    """Worst row of a gradient: max |a - r| over (row max |r| + 1e-2 tensor max |r|)."""
    a, r = a.double().reshape(a.shape[0], -1), r.reshape(r.shape[0], -1)
    if a.shape[1] == 1:                            # a vector (the bias gradient): one row
        a, r = a.T, r.T
    return float(((a - r).abs().amax(1) / (r.abs().amax(1) + 1e-2 * float(r.abs().max()) + 1e-300)).max())


def check_backward(s, tiles, dev):
    """Module gradients (q, k, v, w_rpe.weight, out_linear.weight, out_linear.bias) and the coordinate gradient against
    float64 autograd of the oracle on the GPU's permutations.  Returns the worst per-tensor and per-row errors."""
    inp = _cached((s.id, "inp"), lambda: inputs(s))
    g = _cached((s.id, "gpu"), lambda: _gpu(inp, dev))
    st = _cached((s.id, "perm"), lambda: staged(s, g, "fp32"))
    qp, kp = st["qpos"].long().cpu(), st["kpos"].long().cpu()
    want = _cached((s.id, "grads64"), lambda: _grads64(s, inp, qp, kp))
    got = train_once(s, inp, tiles, dev)
    worst_t, worst_r = {}, {}
    for nm, r in want.items():
        a = got[nm]
        assert bool(torch.isfinite(a).all()), (s.id, tiles, nm)
        worst_t[nm] = float((a.double() - r).abs().max()) / (float(r.abs().max()) + 1e-300)
        worst_r[nm] = row_x(a, r)
    if tiles == "fp32":
        out_x = float(((got["out"].double() - want["out"]).abs() / (ATOL + RTOL * want["out"].abs())).max())
        assert out_x <= 1.0, f"{s.id}: training forward, worst element {out_x:.3f}x the fp32 tolerance"
        bad = {nm: w for nm, w in worst_t.items() if nm != "out" and w > FP32_TENSOR}
    else:
        bad = {nm: w for nm, w in worst_t.items() if w > BF16_TENSOR[nm]}
    assert not bad, f"{s.id} {tiles} tiles: per-tensor errors over the bound {bad}"
    grads = {nm: w for nm, w in worst_r.items() if nm != "out"}
    rbad = {nm: w for nm, w in grads.items() if w > (DCOORDS_ROW_X if nm == "dcoords" else BWD_ROW_X)[tiles]}
    assert not rbad, f"{s.id} {tiles} tiles: per-row errors over the bound: {rbad}"
    return dict(tensor=max(w for nm, w in worst_t.items() if nm != "out"), row=max(grads.values()),
                dcoords_tensor=worst_t["dcoords"], dcoords_row=worst_r["dcoords"])
