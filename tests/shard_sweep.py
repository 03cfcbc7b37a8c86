"""Deterministic sweep of the table-sharded rank stages on ONE GPU: one process plays every rank of a ``world`` in turn
(run by tests/test_gpu_shard_sweep.py, coverage pinned on CPU by tests/test_shard_sweep_cells.py).  A plain module, not a
conftest, built like tests/shape_sweep.py and reusing its inputs, cache, float64 oracle and tolerances.

What a rank runs that the single-GPU operator never does: ``partial_begin`` / ``partial_begin_src`` at ``t0 > 0``,
``partial_heads`` head group by head group into rows padded to ``per * world`` points (f32 rows of 32 or packed int32
rows of 16), ``combine_groups`` on the ``world`` received slices of its own points with a non-zero group stride, and
``forward_partial[_src]`` at ``t0 > 0`` with either accumulator format.  The exchange is a pure permutation of rows, so
it is done here by indexing.  No process group, no communicator.

``SHAPES`` holds the hand-picked cells; every shape lists the (world, head groups) pairs it is run at.  ``cells(shape)``
names the dispatch branches a shape takes, mirroring csrc/capi.hip and csrc/combine.hip.  Nothing here touches the GPU
at import time."""
from collections import namedtuple

import torch

import shape_sweep as sw
from shape_sweep import ATOL, COST_CAP, ILL_WEIGHT, MAX_TABLES, RTOL, SMALL_CAP, TUNED, _cached
from src_attn_sweep import KINDS           # the raw-size kinds of the src variant

# variant "example" (sizes = the clouds) or "src" (sizes = (raw_size,): one cloud padded up to a multiple of B)
Shape = namedtuple("ShardShape", "id variant sizes B T H D C seed configs extra")

BASE_PRECISIONS = ("fp32", "bf16")
EXTRA_PRECISIONS = ("mixed16", "fp32_mfma", "fp32_diff")
F32_MFMA = {"fp32": False, "fp32_mfma": True, "fp32_diff": "diff", "bf16": False, "mixed16": False}
CMB_SPLIT_TILES = 1024     # csrc/combine.hip HEPT_CMB_SPLIT_BELOW: fewer 32-point tiles take the split launch
POISON_I32 = 0x7FC07FC0    # two bf16 NaNs: no packed row the kernels write holds it

# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
# check b: a rank's f32 rows [numer | denom] summed over its tables against float64 on the rank's own permutations, per
# row max |a - r| <= X * (row max |r|); X at <= 2x the worst row measured on the MI355X
# (measured worst row of the whole sweep: fp32 9.80e-6 at src-n6272-minus1 W=3, fp32_mfma 7.49e-6 at t3 W=3, fp32_diff
# 8.73e-6 at h16d24c6 W=2, bf16 4.07e-2 at n9000 W=4 -- one table per rank, so a row is one table's bf16 numerators --,
# mixed16 1.07e-2 at t17-d24 W=17, one table per rank again)
ROW64_X = {"fp32": 1.9e-5, "fp32_mfma": 1.4e-5, "fp32_diff": 1.7e-5, "bf16": 8e-2, "mixed16": 2e-2}
# check e, packed exchange (the rank's table sum rounded to bf16 once more before it travels): worst row of the
# assembled output against float64, row-scaled as shape_sweep._row_scaled; at <= 2x the measured worst row.  Against
# the PLAIN forward tests/test_gpu_dist.py records 4e-3 (99.9 % of the rows) and 1e-2 (every row) at the full size
# (measured worst row of the whole sweep: bf16 1.48e-2 at h1d24c6 W=2 G=1, mixed16 7.60e-3 at src-n1000-full W=3 G=4;
# mixed16 with f32 rows measures the same 7.60e-3 there -- the second rounding does not show beside the 16-bit tiles'
# own error; bf16 with f32 rows: 1.98e-2 at h12d8c4 W=2 G=4, held to REL16_ALL_ROWS_FULL)
PACKED_ROW64 = {"bf16": 2.9e-2, "mixed16": 1.5e-2}


def n_points(s):
    if s.variant == "src":
        return s.sizes[0] + (-s.sizes[0]) % s.B
    return sum(-(-n // s.B) * s.B for n in s.sizes)


def raw_kind(s):
    n, raw = n_points(s), s.sizes[0]
    if n == s.B and raw == 1:
        return "single"
    if raw == n:
        return "full"
    if raw == n - 1:
        return "minus1"
    assert raw == n - s.B + 1, s
    return "one-in-last-block"


def _shapes():
    out = []

    def add(name, sizes, b, t, h, d, c, configs, variant="example", extra=()):
        out.append(Shape(name, variant, tuple(sizes), b, t, h, d, c, 700 + len(out), tuple(configs), tuple(extra)))

    def src(name, n, kind, b, t, h, d, c, configs, extra=()):
        raw = {"full": n, "minus1": n - 1, "one-in-last-block": n - b + 1, "single": 1}[kind]
        add(f"src-{name}-{kind}", [raw], b, t, h, d, c, configs, "src", extra)

    # table slices.  T = 3 over 2 ranks: a reduce rank and a direct rank; over 3: every rank direct, a short last rank
    add("t3", [1000, 377, 250], 100, 3, 8, 24, 6, [(2, 2), (2, 8), (3, 4), (1, 1)], extra=EXTRA_PRECISIONS)
    add("t8-direct", [32 * 9], 32, 8, 8, 24, 2, [(8, 2), (8, 1), (1, 2)])
    # 17 tables: 17 ranks of one table (N = 40: per = 3, rank 13 has one point, ranks 14-16 none); 2 ranks: 9 + 8 tables,
    # rank 0 crosses the 8-table chunk and rank 1 starts beyond it
    add("t17", [40], 8, 17, 8, 16, 4, [(17, 4), (2, 2), (2, 8), (1, 1)])
    add("t17-d24", [40], 8, 17, 8, 24, 6, [(17, 2), (2, 4)], extra=EXTRA_PRECISIONS)
    add("t10", [33 * 4 + 1, 70], 33, 10, 8, 16, 6, [(4, 2), (4, 8)])
    add("t9", [65 * 4, 65 * 2 + 9], 65, 9, 8, 8, 4, [(2, 2), (3, 8), (3, 1)])
    add("t9-d24", [64 * 3, 70], 64, 9, 8, 24, 4, [(2, 4), (3, 2)])
    # head shapes: odd head counts, odd and even heads per group, H = 16 and 12 in groups, every combine_groups D
    add("h1d24c6", [700, 300], 100, 2, 1, 24, 6, [(2, 1), (1, 1)])
    add("h5d20c5", [640], 160, 2, 5, 20, 5, [(2, 5), (2, 1)])
    add("h3d10c6", [255 * 3], 255, 2, 3, 10, 6, [(2, 3), (1, 1)])
    add("h7d17c3", [97 * 6 + 3], 97, 3, 7, 17, 3, [(2, 7), (3, 1)])
    add("h16d27c3", [33 * 10, 33 * 3 + 2], 33, 3, 16, 27, 3, [(2, 4), (3, 8), (2, 16)])
    add("h12d8c4", [64 * 8, 64 * 3 + 1], 64, 2, 12, 8, 4, [(2, 4), (2, 3)])
    add("h16d24c6", [64 * 6, 130], 64, 3, 16, 24, 6, [(2, 4), (3, 8), (2, 16)], extra=EXTRA_PRECISIONS)
    add("h12d24c6", [320], 32, 2, 12, 24, 6, [(2, 4), (2, 2)])
    add("h16d16c4", [128 * 4], 128, 2, 16, 16, 4, [(2, 8), (2, 4)])
    add("h2d27c3", [31 * 5, 31 * 3 + 5], 31, 4, 2, 27, 3, [(2, 2), (3, 1)])
    # blocks above 128 points: forward_partial reads the value rows in place, partial_begin builds them
    add("b200", [200 * 3 + 1, 300], 200, 3, 8, 24, 4, [(2, 2), (3, 4)])
    # the two-launch sort (N > 6144) at t0 > 0; one table per rank: the riders depend on the row type
    add("n6272-t9", [6272], 128, 9, 3, 16, 4, [(3, 3), (3, 1)])
    add("n9000", [9000], 100, 4, 4, 24, 6, [(2, 2), (4, 4), (4, 1)])
    # the combine's one-tile-per-wave launch (>= 1024 tiles of 32 points) at D = 16 with groups
    add("n32800", [32800], 32, 2, 4, 16, 4, [(1, 2)])
    # src variant: every kind of raw_size at t0 > 0, chunks of tables, the two-launch sort, free heads
    src("n1000", 1000, "full", 100, 3, 8, 24, 6, [(2, 2), (3, 4)], extra=EXTRA_PRECISIONS)
    src("n256-t17", 256, "minus1", 32, 17, 8, 24, 4, [(2, 2), (17, 4)])
    src("n660", 660, "one-in-last-block", 33, 4, 8, 24, 2, [(4, 2), (2, 8), (1, 1)])
    src("n100", 100, "single", 100, 3, 8, 24, 6, [(3, 2), (2, 1)])
    src("n6272", 6272, "minus1", 32, 3, 8, 24, 6, [(3, 2), (2, 4)])
    src("n6400-d16", 6400, "one-in-last-block", 64, 2, 8, 16, 4, [(2, 8)])
    src("h5d20c5", 640, "minus1", 160, 3, 5, 20, 5, [(3, 5), (2, 1)])
    return out


SHAPES = _shapes()
BY_ID = {s.id: s for s in SHAPES}


def table_slice(t, r, w):
    from hept_amd.sharding import table_slice as ts

    return ts(t, r, w)


def point_slice(n, r, w):
    """TableSharding.point_slice: equal slices, the last may be short or empty."""
    per = (n + w - 1) // w
    n0 = min(r * per, n)
    return n0, min(per, n - n0)


def packs(precision, d):
    """hept_part_precision (csrc/capi.hip): 16-bit tiles with D = 24 write packed partial rows."""
    return precision in ("bf16", "mixed16") and d == 24


def precisions(s):
    return BASE_PRECISIONS + s.extra


def formats(s, precision):
    return ("f32", "packed") if packs(precision, s.D) else ("f32",)


def runs(s):
    """Every (world, groups, precision, row format) a shape is run at."""
    return [(w, g, p, f) for (w, g) in s.configs for p in precisions(s) for f in formats(s, p)]


def begin_riders(n, h, d, tl, precision):
    """run_begin as partial_begin calls it (no direct v): the bucket-sort launch carries the v rows."""
    carries = SMALL_CAP < n <= sw.REGION_MAX_N and 4 <= d <= 28 and d % 4 == 0 and h >= 1
    return tl <= MAX_TABLES and (tl >= 2 or precision.startswith("fp32")) and carries


def cells(s):
    """Names of the dispatch branches the shape takes over its configs; precision-dependent ones as "<branch>:<prec>"."""
    n = n_points(s)
    tuned = s.H == 8 and (s.D, s.C) in TUNED
    dt = {24: "dt24", 16: "dt16"}.get(s.D, "generic")
    out = {s.variant, "rows-tuned" if tuned else "rows-generic", f"D{s.D}", f"H{s.H}"}
    if s.H % 2:
        out.add("H-odd")
    if s.variant == "src":
        out.add(f"src-raw-{raw_kind(s)}")
        if not tuned:
            out.add("src-free-heads")
    for w, g in s.configs:
        assert s.H % g == 0 and s.T >= w, (s.id, w, g)
        hg = s.H // g
        slices = [table_slice(s.T, r, w) for r in range(w)]
        kinds = {"direct" if tl == 1 else "reduce" for _, tl in slices}
        out.add(f"T{s.T}-W{w}")
        out.add("slices-mixed" if len(kinds) == 2 else f"slices-all-{kinds.pop()}")
        if any(tl > MAX_TABLES for _, tl in slices):
            out.add("rank-crosses-chunk")
        if any(t0 >= MAX_TABLES for t0, _ in slices):
            out.add("rank-starts-beyond-chunk")
        sort = "sort-two-launch" if n > SMALL_CAP else "sort-one-workgroup"
        out.add(sort)
        if w > 1:
            out.add(f"{sort}:t0>0")
            if s.variant == "src":
                out |= {"src:t0>0", f"src-raw-{raw_kind(s)}:t0>0", f"src-{sort}"}
        else:
            out.add("W1")
        cnts = [point_slice(n, r, w)[1] for r in range(w)]
        if n % w == 0:
            out.add("points-even")
        elif min(cnts) == 0:
            out.add("points-empty-rank")
        else:
            out.add("points-short-last")
        for cnt in cnts:
            if cnt:
                out.add("combine-split" if -(-cnt // 32) < CMB_SPLIT_TILES else "combine-tile-per-wave")
        # combine_launch (csrc/combine.hip): D = 24 with an even head count per group stages whole rows in LDS
        staged = s.D == 24 and hg % 2 == 0 and s.H % 2 == 0
        out.add("combine-staged" if staged else "combine-lanes")
        out.add("hg-even" if hg % 2 == 0 else "hg-odd")
        out.add("G1" if g == 1 else f"combine-{dt}-groups")
        if g > 1:
            out.add(f"{'combine-staged' if staged else 'combine-lanes'}-{dt}-groups")
        if s.H == 16:
            out.add(f"H16-G{g}")
        if s.H == 12 and g == 4:
            out.add("H12-G4")
        for p in precisions(s):
            for fmt in formats(s, p):
                out.add(f"prec:{p}:{fmt}")
                if s.variant == "src":
                    out.add(f"src-prec:{p}:{fmt}")
            for _, tl in slices:
                if begin_riders(n, s.H, s.D, tl, p):
                    out.add(f"begin-riders:{p}" + (":one-table" if tl == 1 else ""))
                elif n > SMALL_CAP and tl == 1:
                    out.add(f"begin-v-role:{p}:one-table")
                # a direct rank writes block_attn's rows straight into the group's rows of the padded buffer
                for fmt in formats(s, p):
                    direct = tl == 1 and (fmt == "packed") == packs(p, s.D)
                    out.add(f"{'heads-direct' if direct else 'heads-reduce'}:{fmt}")
                    if direct and w * (-(-n // w)) > n:
                        out.add(f"heads-direct-padded:{fmt}")
        if sw.direct_v(s.D, "fp32", s.B):
            out.add("partial-direct-v:fp32")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def inputs(s):
    """CPU inputs of a shape (float32): shape_sweep's for the example variant; the src variant's are drawn as
    src_attn_sweep draws them (one cloud through ``prepare_input_src``, max(4, N / 2B) regions) with the same scaling."""
    if s.variant == "example":
        return sw.inputs(sw.Shape(s.id, s.sizes, s.B, s.T, s.H, s.D, s.C, s.seed, False))
    from hept_amd.synthetic import make_inputs_src

    n = n_points(s)
    inp = make_inputs_src(s.sizes[0], block_size=s.B, n_hashes=s.T, coords_dim=s.C, num_heads=s.H, h_dim=s.D,
                          num_regions=max(4, n // (2 * s.B)), seed=s.seed, qk_scale=0.3, coords_scale=0.2)
    assert inp["q"].shape[0] == n
    inp["eta_idx"], inp["phi_idx"] = inp["eta_idx"].float().contiguous(), inp["phi_idx"].float().contiguous()
    inp["regions_h"] = inp["regions_h"].float().contiguous()
    return inp


def _geo(inp):
    return dict(raw_size=inp["raw_size"], region_indices=(inp["eta_idx"], inp["phi_idx"]), regions_h=inp["regions_h"])


# ---------------------------------------------------------------------------------------------------------------------
# GPU checks (imports deferred: the CPU suite imports this module without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _gpu(inp, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}


def _op_args(s, g):
    """(positional arguments up to alpha of forward_partial[_src], geo of partial_begin)."""
    if s.variant == "src":
        return (g["q"], g["k"], g["v"], g["coords"], (g["eta_idx"], g["phi_idx"]), g["regions_h"], g["raw_size"],
                g["w_rpe_weight"], g["alpha"]), ((g["eta_idx"], g["phi_idx"]), g["regions_h"], g["raw_size"])
    return (g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"]), None


def forward_partial(s, g, precision, t0, tl, packed):
    from hept_amd import ops

    args, _ = _op_args(s, g)
    fn = ops.forward_partial_src if s.variant == "src" else ops.forward_partial
    return fn(*args, block_size=s.B, w_per_dist=10, t0=t0, tl=tl, precision=precision, packed=packed)


def forward_whole(s, g, precision):
    from hept_amd import ops

    args, _ = _op_args(s, g)
    fn = ops.forward_src if s.variant == "src" else ops.forward
    return fn(*args, g["out_weight"], g["out_bias"], block_size=s.B, w_per_dist=10, precision=precision)


def staged_rank(s, g, precision, t0, tl):
    """The rank's tables as the public stages: prep_hash -> sort_tables[_src] in chunks of MAX_TABLES tables starting at
    the rank's t0 (as run_begin chunks), every chunk's permutations torch's stable sort of the GPU's own keys; then
    reduce_tables(block_attn).  Returns (qpos, kpos, acc)."""
    import hept_oracle as ho
    from hept_amd import ops

    n = g["q"].shape[0]
    sqrt_w = ops.rpe_scale(g["w_rpe_weight"], s.H, s.D, 10)
    is_src = s.variant == "src"
    if is_src:
        eta, phi, cfac = ops.geo_args((g["eta_idx"], g["phi_idx"]), g["regions_h"], s.T, s.H, n)
        cpu = {k: g[k].cpu() for k in ("regions_h", "eta_idx", "phi_idx")}
    rows, qs, ks = None, [], []
    for c0 in range(t0, t0 + tl, MAX_TABLES):
        tc = min(MAX_TABLES, t0 + tl - c0)
        ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sqrt_w, g["alpha"],
                           None if is_src else g["combined_shifts"], precision, t0=c0, tl=tc,
                           raw_size=g["raw_size"] if is_src else None, rows=rows)
        rows = (ph["qhat"], ph["kvhat"])
        mm = ph["minmax"]
        span = mm[..., 1].amax(-1) - mm[..., 0].amin(-1)
        if is_src:
            qp, kp = ops.sort_tables_src(ph["qproj"], ph["kproj"], eta, phi, cfac, ph["minmax"], t0=c0)
            r0, r1 = c0 * s.H, (c0 + tc) * s.H
            offs = ho.geo_shift(cpu["regions_h"][:, r0:r1], span.cpu()[..., None],
                                (cpu["eta_idx"][r0:r1], cpu["phi_idx"][r0:r1]), tc).to(span.device)
            raw = g["raw_size"]
            for proj in (ph["qproj"], ph["kproj"]):
                assert bool(torch.isinf(proj[..., raw:]).all()) and bool(torch.isfinite(proj[..., :raw]).all()), (s.id, c0)
        else:
            qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"], t0=c0)
            offs = g["combined_shifts"][c0:c0 + tc].float() * span[..., None]
        for pos, proj in ((qp, ph["qproj"]), (kp, ph["kproj"])):
            assert torch.equal(pos.long(), torch.sort(proj + offs, dim=-1, stable=True).indices), (s.id, precision, c0)
            assert torch.equal(torch.sort(pos.long(), -1).values, torch.arange(n, device=pos.device).expand_as(pos))
        qs.append(qp)
        ks.append(kp)
    qpos, kpos = torch.cat(qs), torch.cat(ks)
    part = ops.block_attn(rows[0], rows[1], qpos, kpos, s.D, s.B, f32_mfma=F32_MFMA[precision])
    return qpos, kpos, ops.reduce_tables(part, s.D)


def partials64(s, inp, qpos, kpos):
    """float64 per-table numerators (T, N, H, D) and denominators (T, N, H) on the GPU's permutations of all T tables
    (cached per permutation pair) and the float64 output, with the conditioning check of the shape."""
    import hept_oracle as ho

    qp, kp = qpos.long().cpu(), kpos.long().cpu()
    for r in (v for key, v in sw._cache.items() if key != "shape" and key[1] == "shard64"):
        if torch.equal(r["q_positions"], qp) and torch.equal(r["k_positions"], kp):
            return r
    d64 = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items() if torch.is_tensor(v)}
    kw = dict(geo=_geo({**d64, "raw_size": inp["raw_size"]})) if s.variant == "src" else {}
    p = ho.forward_partials(d64["q"], d64["k"], d64["v"], d64["coords"], d64.get("combined_shifts"),
                            d64["w_rpe_weight"], d64["alpha"], block_size=s.B, w_per_dist=10, q_positions=qp,
                            k_positions=kp, keep=False, **kw)
    numer, denom = p["numer"], p["denom"]              # (T, H, N, D), (T, H, N, 1)
    total = denom.sum(0).squeeze(-1)                   # (H, N): every table's weight of the row
    ill = int((total < ILL_WEIGHT).any(0).sum())
    assert ill == 0, f"{s.id}: {ill} rows with total weight < {ILL_WEIGHT}: rescale the shape"
    out = ho.out_projection(ho.combine_tables(numer, denom), d64["out_weight"], d64["out_bias"])
    r = dict(numer=numer.permute(0, 2, 1, 3).contiguous(), denom=denom.squeeze(-1).permute(0, 2, 1).contiguous(),
             out=out, q_positions=qp, k_positions=kp)
    sw._cache[(s.id, "shard64", len(sw._cache))] = r
    return r


def row_x(a, r):
    """Worst row: max |a - r| over the row's max |r| (rows of [numer | denom]: the denominator keeps it positive)."""
    return float(((a.double() - r).abs().amax(-1) / r.abs().amax(-1)).max())


def ranks(s, g, inp, w, precision):
    """Step 5 and the f32 accumulators of every rank of a world (shared by the head-group counts and row formats):
    check a's first half (forward_partial == the staged stages, bit for bit) and check b (float64, per row)."""
    out = []
    for r in range(w):
        t0, tl = table_slice(s.T, r, w)
        qpos, kpos, acc_staged = staged_rank(s, g, precision, t0, tl)
        acc = forward_partial(s, g, precision, t0, tl, False)
        assert torch.equal(acc, acc_staged), \
            f"{s.id} {precision} rank {r}/{w}: forward_partial(t0={t0}, tl={tl}) differs from the staged kernels"
        out.append(dict(t0=t0, tl=tl, qpos=qpos, kpos=kpos, acc=acc))
    ref = partials64(s, inp, torch.cat([x["qpos"] for x in out]), torch.cat([x["kpos"] for x in out]))
    worst = 0.0
    for r, x in enumerate(out):
        t0, tl = x["t0"], x["tl"]
        want = torch.cat([ref["numer"][t0:t0 + tl].sum(0), ref["denom"][t0:t0 + tl].sum(0)[..., None]], -1)
        got = x["acc"].cpu()
        assert float(got[..., s.D + 1:].abs().max()) == 0.0 and bool((got[..., s.D] > 0).all()), (s.id, precision, r)
        x["row_x"] = row_x(got[..., :s.D + 1], want)
        worst = max(worst, x["row_x"])
        bound = ROW64_X[precision]
        assert x["row_x"] <= bound, \
            f"{s.id} {precision} rank {r}/{w}: worst row of the table sum vs float64 {x['row_x']:.3e} > {bound:.1e}"
    return dict(ranks=out, ref=ref, row_x=worst)


def _poisoned(shape, packed, dev):
    if packed:
        return torch.full(shape, POISON_I32, device=dev, dtype=torch.int32)
    return torch.full(shape, float("nan"), device=dev, dtype=torch.float32)


def _combine64(rows, s, g):
    """(sum_r numer / sum_r denom) @ W_out^T + b in float64 from unpacked rows (W, cnt, H, 32)."""
    import hept_oracle as ho

    wide = rows.double().cpu()
    per_head = wide[..., :s.D].sum(0) / wide[..., s.D:s.D + 1].sum(0)          # (cnt, H, D)
    return ho.out_projection(per_head.permute(1, 0, 2), g["out_weight"].double().cpu(), g["out_bias"].double().cpu())


def _elem_x(out, ref):
    return float(((out.double() - ref).abs() / (ATOL + RTOL * ref.abs())).max()) if out.numel() else 0.0


def check(s, w, ng, precision, fmt, dev):
    """One shape, world, head-group count, precision and row format: the simulation and checks a-f of the module
    docstring's stages.  Returns the figures measured on the way."""
    from hept_amd import ops
    from test_gpu_parity import REL16_ALL_ROWS_FULL

    packed = fmt == "packed"
    inp = _cached((s.id, "inp"), lambda: inputs(s))
    g = _cached((s.id, "gpu"), lambda: _gpu(inp, dev))
    rk = _cached((s.id, "ranks", w, precision), lambda: ranks(s, g, inp, w, precision))
    n, hg = n_points(s), s.H // ng
    per = -(-n // w)
    n_pad, row = per * w, 16 if packed else 32
    tag = f"{s.id} W={w} G={ng} {precision} {fmt}"
    _, geo = _op_args(s, g)
    res = dict(row_x=rk["row_x"])

    # 1. ranks: partial_begin, then partial_heads group by group into poisoned rows
    send, accs = [], []
    for r, x in enumerate(rk["ranks"]):
        t0, tl = x["t0"], x["tl"]
        ws = torch.empty(ops.workspace_bytes(n, s.H, s.D, s.C, tl, s.B, precision), device=dev, dtype=torch.uint8)
        dims = ops.partial_begin(g["q"], g["k"], g["v"], g["coords"], g.get("combined_shifts"), g["w_rpe_weight"],
                                 g["alpha"], block_size=s.B, w_per_dist=10, t0=t0, tl=tl, precision=precision,
                                 workspace=ws, geo=geo)
        assert dims == (n, s.H, s.D, s.C)
        buf = _poisoned((ng, n_pad, hg, row), packed, dev)
        for grp in range(ng):
            ops.partial_heads(ws, dims, tl, s.B, precision, grp * hg, buf[grp])
        send.append(buf)
        acc = forward_partial(s, g, precision, t0, tl, True) if packed else x["acc"]
        accs.append(acc)
        # check a: the travelling rows are forward_partial's, bit for bit; zero padding rows; no poison; zero spare columns
        for grp in range(ng):
            assert torch.equal(buf[grp, :n], acc[:, grp * hg:(grp + 1) * hg]), \
                f"{tag}: rank {r} group {grp} rows differ from forward_partial(t0={t0}, tl={tl})"
        if packed:
            assert not bool((buf == POISON_I32).any()), f"{tag}: rank {r} left rows unwritten"
            assert not bool(buf[..., 13:].any()), f"{tag}: rank {r} packed columns 13-15 not zero"
        else:
            assert not bool(torch.isnan(buf).any()), f"{tag}: rank {r} left rows unwritten"
            assert not bool(buf[..., s.D + 1:].any()), f"{tag}: rank {r} columns above D not zero"
        assert not bool(buf[:, n:].any()), f"{tag}: rank {r} padding rows [{n}, {n_pad}) not zero"
        wide = ops.unpack_part(buf[:, :n])
        assert bool((wide[..., s.D] > 0).all()), f"{tag}: rank {r} denominators"
        # check c: packed rows are the f32 rows with the numerators rounded once (RNE) and the denominator exact
        if packed:
            for grp in range(ng):
                f32 = x["acc"][:, grp * hg:(grp + 1) * hg]
                assert torch.equal(wide[grp, ..., 24], f32[..., 24]), f"{tag}: rank {r} group {grp} packed denominators"
                assert torch.equal(wide[grp, ..., :24], f32[..., :24].to(torch.bfloat16).float()), \
                    f"{tag}: rank {r} group {grp} packed numerators"
            assert torch.equal(ops.unpack_part(acc)[..., :25], torch.cat(
                [x["acc"][..., :24].to(torch.bfloat16).float(), x["acc"][..., 24:25]], -1)), f"{tag}: rank {r} packed acc"

    # 2 - 4. exchange by indexing, combine of every rank's own points; the non-pipelined forms of TableSharding.finish
    pad = [torch.cat([a, a.new_zeros((n_pad - n,) + tuple(a.shape[1:]))]) if n_pad > n else a for a in accs]
    total = sum(accs) if not packed else None
    outs, x_cmb = [], 0.0
    for d in range(w):
        n0, cnt = point_slice(n, d, w)
        recv = torch.stack([send[r][:, d * per:(d + 1) * per] for r in range(w)], dim=1).contiguous()
        assert tuple(recv.shape) == (ng, w, per, hg, row)
        out_d = ops.combine_groups(recv, s.D, g["out_weight"], g["out_bias"], 0, cnt)
        assert tuple(out_d.shape) == (cnt, s.D), f"{tag}: rank {d} combine_groups shape {tuple(out_d.shape)}"
        outs.append(out_d)
        a2a = ops.combine_out(torch.stack([p[d * per:(d + 1) * per] for p in pad]).contiguous(), s.D, g["out_weight"],
                              g["out_bias"], 0, cnt)
        forms = {"combine_groups": out_d, "all_to_all": a2a}
        if total is not None:
            forms["reduce"] = ops.combine_out(total, s.D, g["out_weight"], g["out_bias"], n0, cnt)
        if cnt == 0:
            assert all(v.numel() == 0 for v in forms.values()), tag
            continue
        # check d: float64 from the combine's own input -- the received rows, heads back in order
        rows = ops.unpack_part(recv[:, :, :cnt]).permute(1, 2, 0, 3, 4).reshape(w, cnt, s.H, 32)
        ref = _combine64(rows, s, g)
        for nm, got in forms.items():
            got = got.cpu()
            assert bool(torch.isfinite(got).all()), (tag, nm, d)
            x = _elem_x(got, ref)
            x_cmb = max(x_cmb, x)
            assert x <= 1.0, f"{tag}: {nm} of rank {d} vs float64 of its own rows, worst element {x:.3f}x the tolerance"
    res["combine_x"] = x_cmb
    out = torch.cat(outs).cpu()
    assert tuple(out.shape) == (n, s.D), tag

    # check e: the assembled output against float64 on all T tables' GPU permutations
    ref = rk["ref"]["out"]
    if precision.startswith("fp32"):
        res["out_x"] = _elem_x(out, ref)
        bad = ~((out.double() - ref).abs() <= ATOL + RTOL * ref.abs())
        where = [tuple(i) for i in bad.nonzero()[:5].tolist()]
        assert res["out_x"] <= 1.0, f"{tag}: worst element {res['out_x']:.3f}x the tolerance, first (row, col): {where}"
    else:
        r64 = sw._row_scaled(out, ref)
        res["packed_row64" if packed else "row64"] = r64
        bound = PACKED_ROW64[precision] if packed else REL16_ALL_ROWS_FULL[precision]
        assert r64 <= bound, f"{tag}: worst row-scaled error vs float64 {r64:.3e} > {bound:.1e}"
    # check f: one rank, one group, f32 rows: the plain operator up to the association of the table sum
    if w == 1 and ng == 1 and not packed:
        torch.testing.assert_close(out, forward_whole(s, g, precision).cpu(), rtol=1e-5, atol=1e-6)
    return res
