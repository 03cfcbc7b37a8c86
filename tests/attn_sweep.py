"""Deterministic shape sweep of the fused ``Attn`` block: every element of the eval block and every gradient of the
training block against a float64 evaluation of the reference block on the GPU's own permutations (run by
tests/test_gpu_attn_sweep.py, coverage pinned on CPU by tests/test_attn_sweep_cells.py).  A plain module, not a conftest,
built like tests/shape_sweep.py and reusing its helpers.

The fused block exists for H = 8, D = 24 and C in {6, 4, 2} (``hept_prep_hash_fused_rpe``, csrc/prep_hash.hip), so
``SHAPES`` varies the coordinate count, the block size (every tile count FULL and ragged), the point count (around the
one-workgroup sort's capacity and the combine's flat grid), the table count (1-4 and 5-8 table slots of the row builder,
chunks of 8 beyond), clouds of exactly B and B + 1 points, and the parameters (a seeded default-initialised block, or
case A1's checkpoint weights).  ``cells(shape)`` names the dispatch branches a shape takes, mirroring csrc/.  Nothing
here touches the GPU at import time."""
import os
from collections import namedtuple

import torch

import shape_sweep as sw
from shape_sweep import COST_CAP, ILL_WEIGHT, MAX_TABLES, PRECISIONS, SMALL_CAP, _cached, n_points, row_x

Shape = namedtuple("Shape", "id sizes B T C seed bwd ckpt")
H, D, K = 8, 24, 10          # the fused block's heads, head dimension and w_rpe distances per coordinate
COORDS = (6, 4, 2)           # hept_prep_hash_fused_rpe: HEPT_FUSED_CASE(6), (4), (2)
# prep_fused_kernel<C, TILE, TMAX>: the tile format of each precision id (fp32_mfma / fp32_diff build f32 rows)
TILE = {"fp32": "f32", "fp32_mfma": "f32", "fp32_diff_split": "f32", "fp32_diff_mfma": "f32", "bf16": "bf16",
        "mixed16": "mixed16"}
# training configurations: (Attn precision, attn.train_tiles); "fp32_mfma" runs f32 tiles on the f32-MFMA backward
TRAIN = {"fp32": ("fp32", "fp32"), "bf16": ("fp32", "bf16"), "fp32_mfma": ("fp32_mfma", "fp32")}
CMB_FLAT_FROM = 1024 * 32    # csrc/combine.hip:908: fewer than 1024 tiles of 32 points -> the split combine grid
EPS = 1e-5


def _hand():
    out = []

    def add(name, sizes, b, t, c, bwd=False, ckpt=False):
        out.append(Shape(name, tuple(sizes), b, t, c, 700 + len(out), bwd, ckpt))

    # every tile count nkt = ceil(B/32) 1..8, FULL (B = 32 nkt) and ragged, the coordinate counts and 1-4 / 5-8 tables in turn
    add("b8-c6-t2", [200, 77], 8, 2, 6, bwd=True)
    add("b32-c2-t1", [32 * 9], 32, 1, 2, bwd=True)
    add("b33-c4-t3", [33 * 4 + 1, 70], 33, 3, 4, bwd=True)
    add("b64-c4-t6", [64 * 6, 100], 64, 6, 4, bwd=True)
    add("b65-c2-t9", [65 * 4, 65 * 2 + 9], 65, 9, 2, bwd=True)
    add("b96-c6-t2", [96 * 5, 200], 96, 2, 6, bwd=True)
    add("b100-c6-t3", [1000, 377, 250], 100, 3, 6)
    add("b128-c2-t1", [128 * 7], 128, 1, 2, bwd=True)
    add("b129-c4-t2", [129 * 4, 129], 129, 2, 4, bwd=True)
    add("b160-c4-t5", [160 * 3 + 50, 160 * 2], 160, 5, 4, bwd=True)
    add("b180-c2-t2", [180 * 3, 200], 180, 2, 2, bwd=True)
    add("b192-c6-t7", [192 * 4], 192, 7, 6, bwd=True)
    add("b200-c4-t3", [200 * 3 + 1, 300], 200, 3, 4, bwd=True)
    add("b224-c6-t1", [224 * 3, 230], 224, 1, 6, bwd=True)
    add("b225-c2-t2", [225 * 3, 225 * 2 + 100], 225, 2, 2, bwd=True)
    add("b256-c6-t8", [256 * 2 + 10, 256], 256, 8, 6, bwd=True)
    # point counts around the one-workgroup sort's capacity (multiples of B), ~9000, and the combine's flat grid
    add("n6016-c4", [6016], 128, 2, 4)
    add("n6144-c2", [3072, 3072], 128, 3, 2)
    add("n6272-c6", [6272], 128, 1, 6, bwd=True)
    add("n9000-c4", [9000], 100, 3, 4)
    add("n33000-c2", [33000], 8, 1, 2)
    add("n33024-c4", [20000, 13000], 32, 2, 4, bwd=True)
    # tables: 17 (three chunks of the row builder and the sort, the pos_chunk copy), 9 beside the two-launch sort, 6 and 17
    # with two coordinates
    add("t17-c4", [1280], 64, 17, 4)
    add("t17-c2", [900, 300], 32, 17, 2, bwd=True)
    add("t9-n6272-c6", [6272], 32, 9, 6, bwd=True)
    add("t6-c2", [500, 333], 50, 6, 2)
    add("t6-c6", [700], 100, 6, 6, bwd=True)
    # a cloud of exactly B points beside one of B + 1 (its second block holds one real point and B - 1 pad copies)
    add("cloud-b-b1-100-c4", [100, 101, 300], 100, 3, 4, bwd=True)
    add("cloud-b-b1-225-c2", [225, 226], 225, 6, 2)
    add("cloud-b-b1-64-c6", [64, 65, 200], 64, 5, 6)
    # case A1's checkpoint weights (the shipped model's layer 0: C = 6, three tables)
    add("a1-b128", [1500, 700], 128, 3, 6, ckpt=True)
    add("a1-b100", [1000, 377], 100, 3, 6, bwd=True, ckpt=True)
    add("a1-b33", [33 * 20 + 5], 33, 3, 6, ckpt=True)
    return out


def _random(count=12):
    """Seeded draws: B in 8..256, 1..12 tables, 1..3 clouds of B..4B+39 points, C in turn; the table count is lowered
    where the float64 oracle would be large."""
    g = torch.Generator().manual_seed(4343)
    out = []
    for it in range(count):
        c = COORDS[it % 3]
        b = int(torch.randint(8, 257, (1,), generator=g))
        t = int(torch.randint(1, 13, (1,), generator=g))
        n_clouds = int(torch.randint(1, 4, (1,), generator=g))
        sizes = tuple(int(torch.randint(b, 4 * b + 40, (1,), generator=g)) for _ in range(n_clouds))
        s = Shape("", sizes, b, t, c, 3500 + it, it % 4 == 0, False)
        while s.T > 1 and cost(s) > COST_CAP:
            s = s._replace(T=s.T - 1)
        out.append(s._replace(id=f"r{it:02d}-b{b}-t{s.T}-c{c}"))
    return out


def cost(s):
    """float64 elements of the oracle's largest intermediate (T, H, N/B, B, B)."""
    return s.T * H * n_points(s) * s.B


SHAPES = _hand() + _random()
BY_ID = {s.id: s for s in SHAPES}
BWD_SHAPES = [s for s in SHAPES if s.bwd]


def train_modes(s):
    """Training configurations of a shape.  bf16 tiles are not run on case A1's weights: sqrt_w up to 5.8e3 puts |q^|
    near 1e2, whose bf16 rounding moves a logit by O(1) (measured: gradient rows off by twice their own scale) -- there
    is no accuracy there to assert."""
    return [m for m in TRAIN if not (s.ckpt and m == "bf16")]


def chunks(t):
    """Table counts of the row builder / sort calls: hept_attn_block_forward walks chunks of HEPT_MAX_TABLES."""
    return [min(MAX_TABLES, t - c0) for c0 in range(0, t, MAX_TABLES)]


def tmax(tl):
    """Table slots of prep_fused_kernel (launch_prep_fused): 4 for 1-4 tables per call, else HEPT_MAX_TABLES."""
    return 4 if tl <= 4 else MAX_TABLES


def cells(s):
    """Names of the dispatch branches the shape takes; precision-dependent ones as "<branch>:<precision id>"."""
    n = n_points(s)
    nkt = -(-s.B // 32)                                            # csrc/block_attn.hip:786
    kind = "full" if s.B == 32 * nkt else "ragged"                 # launch_attn / launch_attn_split: B == 32 nkt
    out = {f"nkt{nkt}-{kind}", f"coords{s.C}",
           "sort-two-launch" if n > SMALL_CAP else "sort-one-workgroup",   # csrc/sort_tables.hip:1340
           "table-chunks" if s.T > MAX_TABLES else "tables-one-chunk",          # csrc/capi.hip hept_attn_block_forward
           "combine-flat" if n >= CMB_FLAT_FROM else "combine-split",           # csrc/combine.hip combine_launch_impl
           "combine-last-tile-ragged" if n % 32 else "combine-last-tile-full",
           "clouds-one" if len(s.sizes) == 1 else "clouds-several",
           "params-ckpt" if s.ckpt else "params-init"}
    if s.T > MAX_TABLES and n > SMALL_CAP:
        out.add("table-chunks-two-launch")
    if s.B in s.sizes:
        out.add("cloud-of-B")
    if s.B + 1 in s.sizes:
        out.add("cloud-of-B+1")
    for p in PRECISIONS:
        for tl in chunks(s.T):
            out.add(f"prep<{s.C},{TILE[p]},{tmax(tl)}>")           # csrc/prep_hash.hip launch_prep_fused
        out.add(f"attn-nkt{nkt}-{kind}:{p}")                       # the block_attn kernel of the precision at this tile count
        # hept_part_precision (D = 24): 16-bit tiles write packed rows, combine_launch<true, true, 24> reads them
        out.add(f"{'part-packed' if p in ('bf16', 'mixed16') else 'part-f32'}:{p}")
    if s.bwd:
        out.add(f"bwd-coords{s.C}")
        out.add(f"bwd-nkt{nkt}-{kind}")
        for tr, (_, tiles) in TRAIN.items():
            for tl in chunks(s.T):
                out.add(f"bwd-prep<{s.C},{'bf16' if tiles == 'bf16' else 'f32'},{tmax(tl)}>")
        if s.T > MAX_TABLES:
            out.add("bwd-table-chunks")
        if n > SMALL_CAP:
            out.add("bwd-sort-two-launch")
        if s.B + 1 in s.sizes:
            out.add("bwd-cloud-of-B+1")
        if s.ckpt:
            out.add("bwd-params-ckpt")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# GPU checks (imports deferred: the CPU suite imports this module without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
ATOL, RTOL = sw.ATOL, sw.RTOL       # fp32 tiles: atol / rtol on every element of y against float64
# 16-bit modes: worst row error of y over (row max |aggr| + 1e-3) -- the error lives in the operator's output aggr, not
# in the residual x that dominates |y| -- against float64 and against the oracle's model of the 16-bit arithmetic
# (bounds <= 2x the measured worst row on the MI355X: against float64 bf16 1.57e-2 at r08-b66-t10-c2, mixed16 8.6e-3 at
# n6272-c6; against the model bf16 2.7e-3 at r07-b250-t2-c4, mixed16 2.6e-3 at n33000-c2).  fp32 modes: the worst element
# is 0.14x ATOL / RTOL (fp32, fp32_diff_split at n33000-c2), 0.10x (fp32_mfma), 0.03x (fp32_diff_mfma)
ROW16_64 = {"bf16": 3.1e-2, "mixed16": 1.7e-2}
ROW16_MODEL = {"bf16": 5.4e-3, "mixed16": 5.2e-3}
# case A1's checkpoint weights: sqrt_w reaches 5.8e3, so a logit is the difference of large terms and the fp32 round-off
# of q^, k^ reaches it (measured worst element 9.6x ATOL / RTOL, f32-MFMA tiles; the difference form fp32_diff 0.84x):
# those shapes are held to ten times the fp32 tolerance -- still 10x tighter than tests/test_gpu_attn_block.py's A1 atol
CKPT_TOL_X = 10.0
CKPT16_64 = {"bf16": 0.18, "mixed16": 7.6e-2}       # measured worst row: bf16 9.1e-2, mixed16 3.8e-2
CKPT16_MODEL = {"bf16": 3.0e-2, "mixed16": 4.4e-2}  # measured worst row: bf16 1.5e-2, mixed16 2.2e-2
# training: per tensor max |a - r| / max |r| and per row (row_x) against float64 autograd of the block
# (measured worst, all at a1-b100: fp32 tiles tensor 8.3e-5 (w_rpe.weight), row 4.4e-5 (w_q.weight); f32-MFMA tiles
# tensor 3.9e-5, row 7.2e-5 (y); bf16 tiles tensor 0.116 (ff.0.weight at t6-c6), row 0.178 (ff.0.weight at t6-c6))
TRAIN_TENSOR = {"fp32": 1.7e-4, "fp32_mfma": 8e-5, "bf16": 0.23}
TRAIN_ROW = {"fp32": 9e-5, "fp32_mfma": 1.5e-4, "bf16": 0.35}
# ... except the coordinate gradient and w_rpe.weight's (through sqrt_w): the backward differentiates the expanded
# logit q^.k^ - |q^|^2/2 - |k^|^2/2, so a point's coordinate gradient is a sum of O(|s|) terms that cancel down to the
# difference of neighbouring points' scaled coordinates -- worst at C = 2, where sqrt_w is largest (measured worst row:
# coords 3.3e-4 at b32-c2-t1, w_rpe.weight 1.7e-4 at t17-c2, fp32 tiles; coords 1.6e-4 with f32-MFMA tiles; bf16 tiles
# coords 0.353 at n33024-c4)
TRAIN_ROW_CANCEL = {"fp32": 6.6e-4, "fp32_mfma": 3.2e-4, "bf16": 0.7}
CANCEL = ("coords", "w_rpe.weight")
# the module's parameters that receive gradients (w_rpe.bias and attn.e2lsh.alpha never do, as in the reference)
GRAD_PARAMS = ("norm1.weight", "norm1.bias", "w_q.weight", "w_k.weight", "w_v.weight", "w_rpe.weight",
               "attn.out_linear.weight", "attn.out_linear.bias", "norm2.weight", "norm2.bias", "ff.0.weight", "ff.0.bias",
               "ff.2.weight", "ff.2.bias")
QK_SCALE = 0.5        # w_q, w_k of the default-initialised block: |q|, |k| ~ 0.3 like tests/shape_sweep.py's inputs
COORD_SCALE = 0.2     # as tests/shape_sweep.py


def default_params(c, t, seed):
    """A default-initialised Attn block's state dict (CPU), norm weights / biases drawn away from 1 / 0."""
    from hept_amd import Attn

    with torch.random.fork_rng():
        torch.manual_seed(seed)
        blk = Attn(c, h_dim=D, num_heads=H, block_size=8, n_hashes=t, num_w_per_dist=K)
        p = {k: v.detach().clone() for k, v in blk.state_dict().items()}
        for nm in ("norm1", "norm2"):
            p[f"{nm}.weight"] = 1.0 + 0.2 * torch.randn(D)
            p[f"{nm}.bias"] = 0.1 * torch.randn(D)
    p["w_q.weight"] = p["w_q.weight"] * QK_SCALE
    p["w_k.weight"] = p["w_k.weight"] * QK_SCALE
    return p


def inputs(s):
    """CPU inputs of a shape: x (one row per raw point, padded as make_inputs pads), coords, codes and parameters."""
    from hept_amd.synthetic import make_inputs

    inp = make_inputs(list(s.sizes), block_size=s.B, n_hashes=s.T, coords_dim=s.C, h_dim=D, num_heads=H, seed=s.seed)
    n_raw = sum(s.sizes)
    x = torch.randn(n_raw, D, generator=torch.Generator().manual_seed(s.seed + 1))[inp["pad_seq"]].contiguous()
    if s.ckpt:
        import cases

        a1 = cases.load_case_attn("a1_attn_ckpt6k")[0]
        params = {k: v.clone() for k, v in a1["params"].items()}
        assert params["attn.e2lsh.alpha"].shape[2] == s.T and s.C == 6
        # the checkpoint's sqrt_w reaches 5.8e3 on the coordinate columns the data keeps small: N(0,1) coordinates
        # scaled per column like case A1's own (COORD_SCALE would leave rows ill-conditioned)
        coord_scale = a1["coords"].std(0)
    else:
        params = default_params(s.C, s.T, s.seed)
        params["attn.e2lsh.alpha"] = inp["alpha"]
        coord_scale = COORD_SCALE
    out = dict(x=x, coords=inp["coords"] * coord_scale, combined_shifts=inp["combined_shifts"], params=params)
    assert x.shape[0] == n_points(s)
    return out


def _gpu(inp, dev):
    return dict(x=inp["x"].to(dev), coords=inp["coords"].to(dev), combined_shifts=inp["combined_shifts"].to(dev),
                params={k: v.to(dev) for k, v in inp["params"].items()})


def module(s, inp, precision, dev):
    """The Attn block of a shape with the shape's parameters (precision: an ops precision)."""
    from hept_amd import Attn

    blk = Attn(s.C, precision=precision, h_dim=D, num_heads=H, block_size=s.B, n_hashes=s.T, num_w_per_dist=K)
    blk.load_state_dict(inp["params"], strict=True)
    return blk.to(dev)


class _diff_mfma:
    """HEPT_DIFF_MFMA for the duration of a call (read by hept_block_attn on every call)."""

    def __init__(self, precision):
        self.env = PRECISIONS[precision][2]

    def __enter__(self):
        self.old = os.environ.get("HEPT_DIFF_MFMA")
        if self.env is not None:
            os.environ["HEPT_DIFF_MFMA"] = self.env

    def __exit__(self, *exc):
        if self.env is not None:
            if self.old is None:
                os.environ.pop("HEPT_DIFF_MFMA", None)
            else:
                os.environ["HEPT_DIFF_MFMA"] = self.old


def staged(s, g, precision):
    """The block as its kernels: prep_hash_fused -> sort_tables (chunks of MAX_TABLES tables, rows reused) -> block_attn ->
    combine_ffn.  Checks that every chunk's permutations are torch's stable sort of the GPU's own keys."""
    from hept_amd import ops

    prec, f32_mfma, _ = PRECISIONS[precision]
    p, codes = g["params"], g["combined_shifts"]
    n = g["x"].shape[0]
    sqrt_w = ops.rpe_scale(p["w_rpe.weight"], H, D, K)
    rows, qs, ks = None, [], []
    for c0 in range(0, s.T, MAX_TABLES):
        tc = min(MAX_TABLES, s.T - c0)
        ph = ops.prep_hash_fused(g["x"], p["norm1.weight"], p["norm1.bias"], EPS, p["w_q.weight"], p["w_k.weight"],
                                 p["w_v.weight"], g["coords"], sqrt_w, p["attn.e2lsh.alpha"], codes, prec, t0=c0, tl=tc,
                                 rows=rows)
        rows = (ph["qhat"], ph["kvhat"])
        qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], codes, ph["minmax"], t0=c0)
        mm = ph["minmax"]
        span = mm[..., 1].amax(-1) - mm[..., 0].amin(-1)
        offs = codes[c0:c0 + tc].float() * span[..., None]
        for pos, proj in ((qp, ph["qproj"]), (kp, ph["kproj"])):
            assert torch.equal(pos.long(), torch.sort(proj + offs, dim=-1, stable=True).indices), (s.id, precision, c0)
            assert torch.equal(torch.sort(pos.long(), -1).values, torch.arange(n, device=pos.device).expand_as(pos))
        qs.append(qp)
        ks.append(kp)
    qpos, kpos = torch.cat(qs), torch.cat(ks)
    part = ops.block_attn(rows[0], rows[1], qpos, kpos, D, s.B, f32_mfma=f32_mfma)
    y = ops.combine_ffn(part, D, p["attn.out_linear.weight"], p["attn.out_linear.bias"], g["x"], p["norm2.weight"],
                        p["norm2.bias"], EPS, p["ff.0.weight"], p["ff.0.bias"], p["ff.2.weight"], p["ff.2.bias"])
    return dict(y=y, part=part, qpos=qpos, kpos=kpos)


def _d64(inp):
    return {k: v.double() if v.is_floating_point() else v for k, v in inp.items()}


def oracle64(s, inp, qp, kp, **kw):
    import hept_oracle as ho

    p64 = {k: v.double() for k, v in inp["params"].items()}
    return ho.attn_block(inp["x"].double(), inp["coords"].double(), inp["combined_shifts"], p64, num_heads=H,
                         block_size=s.B, w_per_dist=K, eps=EPS, q_positions=qp, k_positions=kp, **kw)


def almost_sorted_tol(hash_scale, key_scale):
    """How far the GPU's order may lie from sorted under the float64 keys.  tests/shape_sweep.py allows 8e-6 of the hash
    scale (the fp32 summation of the 30-term projection) plus the rounding of the key addition; the fused row builder
    adds its fp32 LayerNorm and 24-term projections in front of the hash -- both within the same few-ulp relative error of
    q, so the same allowance holds: the measured worst is 0.20x of it (n6144-c2) -- no widening needed."""
    return 8e-6 * hash_scale + 4 * 2.0 ** -23 * key_scale


def reference(s, inp, qpos, kpos, note=None):
    """float64 block on the GPU permutations (cached per permutation pair), with the conditioning and sortedness checks
    that depend on the permutations only."""
    from test_gpu_parity import _almost_sorted

    qp, kp = qpos.long().cpu(), kpos.long().cpu()
    for r in (v for key, v in sw._cache.items() if key != "shape" and key[1] == "block64"):
        if torch.equal(r["q_positions"], qp) and torch.equal(r["k_positions"], kp):
            return r
    r = oracle64(s, inp, qp, kp, keep=True)
    hash_scale = float(r["q_hashed"].abs().max())
    for pos, keys in ((qp, r["q_keys"]), (kp, r["k_keys"])):
        tol = almost_sorted_tol(hash_scale, float(keys.abs().max()))
        got = _almost_sorted(keys, pos, tol)
        if note is not None:
            note("keys out of order / tolerance", got / tol)
        assert got <= tol, (s.id, got, tol)
    total = r["denom"].sum(0).squeeze(-1)          # (H, N): every table's weight of the row
    ill = int((total < ILL_WEIGHT).any(0).sum())
    assert ill == 0, f"{s.id}: {ill} rows with total weight < {ILL_WEIGHT}: rescale the shape"
    r = dict(y=r["y"], aggr=r["aggr"], q_positions=qp, k_positions=kp)
    sw._cache[(s.id, "block64", len(sw._cache))] = r
    return r


def _row16(y, ref):
    """Worst row of y's error over (row max |aggr| + 1e-3)."""
    return float(((y.double() - ref["y"]).abs().amax(-1) / (ref["aggr"].abs().amax(-1) + 1e-3)).max())


def check_forward(s, precision, dev, note=lambda k, v: None):
    """Every element of the staged block against float64 on its own permutations; the one-call block and Attn.eval()
    must be bit-identical to the staged kernels.  ``note(name, value)`` sees every measured error before it is asserted."""
    import hept_oracle as ho
    from hept_amd import ops
    from test_gpu_parity import _model_kw

    prec = PRECISIONS[precision][0]
    inp = _cached((s.id, "inp"), lambda: inputs(s))
    g = _cached((s.id, "gpu"), lambda: _gpu(inp, dev))
    blk = module(s, inp, prec, dev).eval()
    kwargs = {"coords": g["coords"], "combined_shifts": g["combined_shifts"]}
    with _diff_mfma(precision), torch.no_grad():
        st = staged(s, g, precision)
        one = ops.attn_block_forward(g["x"], g["coords"], g["combined_shifts"], g["params"], num_heads=H, block_size=s.B,
                                     w_per_dist=K, eps1=EPS, eps2=EPS, precision=prec)
        assert blk._fused_ok(g["x"])
        mod = blk(g["x"], kwargs)
        torch.cuda.synchronize()
    y = st["y"].cpu()
    assert bool(torch.isfinite(y).all()), (s.id, precision)
    # the one-call block computes sqrt_w from w_rpe.weight in the row builder's prologue (rpe_scale_lds), the staged
    # block takes hept_rpe_scale's: the same arithmetic in the same order, so the outputs are identical bit for bit
    assert torch.equal(one.cpu(), y), f"{s.id} {precision}: one-call block differs from the staged kernels"
    assert torch.equal(mod.cpu(), y), f"{s.id} {precision}: Attn.eval() differs from the staged kernels"
    wide = ops.unpack_part(st["part"])
    assert bool((wide[..., D] > 0).all()), (s.id, precision)
    assert float(wide[..., D + 1:].abs().max()) == 0.0, (s.id, precision)
    ref = reference(s, inp, st["qpos"], st["kpos"], note)
    tol_x = CKPT_TOL_X if s.ckpt else 1.0
    if s.ckpt:
        note = _ckpt_note(note)
    if prec.startswith("fp32"):
        err = (y.double() - ref["y"]).abs()
        x = float((err / (ATOL + RTOL * ref["y"].abs())).max()) / tol_x
        note("x", x)
        where = [tuple(i) for i in (err > tol_x * (ATOL + RTOL * ref["y"].abs())).nonzero()[:5].tolist()]
        assert x <= 1.0, f"{s.id} {precision}: worst element {x:.3f}x the tolerance, first (row, col): {where}"
        return dict(x=x)
    w64 = _row16(y, ref)
    note("row64", w64)
    qp, kp = st["qpos"].long().cpu(), st["kpos"].long().cpu()
    model = ho.attn_block(inp["x"], inp["coords"], inp["combined_shifts"], inp["params"], num_heads=H, block_size=s.B,
                          w_per_dist=K, eps=EPS, q_positions=qp, k_positions=kp, keep=False, **_model_kw(prec))
    wm = _row16(y, dict(y=model["y"].double(), aggr=ref["aggr"]))
    note("model", wm)
    b64, bm = (CKPT16_64[prec], CKPT16_MODEL[prec]) if s.ckpt else (ROW16_64[prec], ROW16_MODEL[prec])
    assert w64 <= b64, f"{s.id} {precision}: worst row error vs float64 {w64:.3e} of the row's |aggr|"
    assert wm <= bm, f"{s.id} {precision}: worst row error vs the 16-bit model {wm:.3e}"
    return dict(row64=w64, model=wm)


def _ckpt_note(note):
    return lambda k, v: note(f"ckpt {k}", v)


def _g_out(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(5))


def train_once(s, inp, g, mode, dev):
    """Attn.train() with dropout 0: y and the gradients of x, coords and every parameter that receives one."""
    prec, tiles = TRAIN[mode]
    blk = module(s, inp, prec, dev).train()
    blk.dropout.p = 0.0
    blk.attn.train_tiles = tiles
    x = g["x"].clone().requires_grad_(True)
    coords = g["coords"].clone().requires_grad_(True)
    assert blk.attn._train_fused_ok(x, {"coords": coords, "combined_shifts": g["combined_shifts"]})
    y = blk(x, {"coords": coords, "combined_shifts": g["combined_shifts"]})
    y.backward(_g_out(y.shape).to(dev))
    got = {nm: p.grad.detach().cpu() for nm, p in blk.named_parameters() if p.grad is not None}
    assert set(got) == set(GRAD_PARAMS), sorted(set(got) ^ set(GRAD_PARAMS))
    got.update(y=y.detach().cpu(), x=x.grad.detach().cpu(), coords=coords.grad.detach().cpu())
    return got


def grads64(s, inp, qp, kp):
    """float64 autograd of the reference block on the given permutations."""
    import hept_oracle as ho

    p64 = {k: v.double().requires_grad_(k in GRAD_PARAMS) for k, v in inp["params"].items()}
    x = inp["x"].double().requires_grad_(True)
    coords = inp["coords"].double().requires_grad_(True)
    res = ho.attn_block(x, coords, inp["combined_shifts"], p64, num_heads=H, block_size=s.B, w_per_dist=K, eps=EPS,
                        q_positions=qp, k_positions=kp, keep=False, grad=True)
    res["y"].backward(_g_out(res["y"].shape).double())
    want = {k: p64[k].grad for k in GRAD_PARAMS}
    want.update(y=res["y"].detach(), x=x.grad, coords=coords.grad)
    return want


def check_backward(s, mode, dev, note=lambda k, v: None):
    """Every gradient of the training block against float64 autograd on the GPU's permutations, per tensor and per row.
    Returns the worst per-tensor and per-row errors."""
    inp = _cached((s.id, "inp"), lambda: inputs(s))
    g = _cached((s.id, "gpu"), lambda: _gpu(inp, dev))
    st = _cached((s.id, "perm"), lambda: staged(s, g, "fp32"))
    qp, kp = st["qpos"].long().cpu(), st["kpos"].long().cpu()
    want = _cached((s.id, "grads64"), lambda: grads64(s, inp, qp, kp))
    got = train_once(s, inp, g, mode, dev)
    if s.ckpt:
        note = _ckpt_note(note)
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
        y_x /= CKPT_TOL_X if s.ckpt else 1.0
        note("y x", y_x)
        assert y_x <= 1.0, f"{s.id} {mode}: training forward, worst element {y_x:.3f}x the fp32 tolerance"
    bad = {nm: w for nm, w in worst_t.items() if w > TRAIN_TENSOR[mode]}
    assert not bad, f"{s.id} {mode}: per-tensor errors over {TRAIN_TENSOR[mode]}: {bad}"
    grads = {nm: w for nm, w in worst_r.items() if nm != "y"}
    rbad = {nm: w for nm, w in grads.items() if w > (TRAIN_ROW_CANCEL if nm in CANCEL else TRAIN_ROW)[mode]}
    assert not rbad, f"{s.id} {mode}: per-row errors over the bound: {rbad}"
    return dict(tensor=max(w for nm, w in worst_t.items() if nm != "y"), row=max(grads.values()))
