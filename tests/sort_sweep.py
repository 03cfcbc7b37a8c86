"""The sort sweep: every reachable instantiation and every data-dependent branch of csrc/sort_tables.hip on PLANTED
populations, every permutation held to ``torch.sort(stable=True)`` of float64 keys computed on the host from the cell's
inputs (``torch.equal`` on the whole permutation, q and k halves; no tolerances).  Run by tests/test_gpu_sort_sweep.py,
the coverage and the exactness pinned on the CPU by tests/test_sort_sweep_cells.py.  A plain module, not a conftest;
nothing here touches the GPU at import time.  ``python tests/sort_sweep.py`` (a child process of the GPU test, started
with HEPT_SORT_LINEAR=1) runs the region-size cells in the linear layout.

The lever.  ``ops.sort_tables`` takes the projections and the range partials from the caller.  Partials that reduce to
lo = 0, hi = 1, cmax = 255 (three different slots of the 1 024, one of them the last, every other slot neutral) give
span = 1, width = 256, scale = 2^17 / 256 = 512, every step exact: for proj in [0, 1) and an integer code c in [0, 255]
the 17-bit id of the key c + proj is trunc((c + proj) * 512) -- the code is the top-level bucket, floor(proj * 512) the
low-id bin, equal proj an id group of ties.  MODE 2 (raw keys) gets the same map from keys c + proj with a 0.0 and a
256.0 planted in every segment; the one-workgroup sort has 4 096 bins and scale 16.  MODE 1 (the src variant) bounds the
shift by m * 1.0001f + 1, no power of two: there the float32 mirror below inverts the map (a key in the middle part of
the wanted id's interval, on the 2^-16 grid) and verifies every population.  All keys lie on the 2^-16 grid below 256, so
the float32 key is exact however it is rounded and equals the float64 host key bit for bit.

A cell is a list of hot buckets (population, how it spreads over the 512 low-id bins, which chunks it comes from) next to
an ordinary background; ``stats`` runs the float32 mirror of the dispatch and of bucket_id<BUCKETS> over the cell's
actual inputs and returns the instantiations, per (segment, bucket) the population, the low-half count and the largest id
group, and per (chunk, bucket) the run length; ``tags`` derives the branch names from those numbers alone."""
import os
import sys
import zlib
from collections import namedtuple

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------------------------------
# constants of csrc/sort_tables.hip (tests/test_sort_sweep_cells.py parses the file and compares)
# ---------------------------------------------------------------------------------------------------------------------
ID_BITS, TOP_BITS = 17, 8
ID_BUCKETS, NTOP, LOBINS = 1 << ID_BITS, 1 << TOP_BITS, 1 << (ID_BITS - TOP_BITS)
BKT_THREADS, BKT_CAP, LEAN_SLOTS = 128, 1024, 4
LARGE_TILE = 6                         # BKT_CAP_LARGE = 6 * HEPT_BKT_CAP
SORT_CHUNK = 4096
SMALL_CAP, SMALL_BINS, SMALL_SPLIT, SMALL_THREADS = 6144, 4096, 4, 1024
REGION_MAX_N, EMBED_SHIFT = 131072, 20
WAVE = 64
PREP_GRID = 1024
LEAN_MAX = LEAN_SLOTS * BKT_THREADS    # 512


def region_cap(n):
    c = 1024
    while c * 32 < n:
        c <<= 1
    return c


# file:line references of the rules the mirror restates (tests/test_sort_sweep_cells.py checks the text)
REFS = [
    ("hept_amd/csrc/sort_tables.hip", 41, "constexpr int SORT_CHUNK = SORT_THREADS * SORT_ITEMS;"),
    ("hept_amd/csrc/sort_tables.hip", 62, "if (key == 0.f) key = 0.f;"),
    ("hept_amd/csrc/sort_tables.hip", 73, "fminf((from_ordered(u) - kmin) * scale, (float)(BUCKETS - 1))"),
    ("hept_amd/csrc/sort_tables.hip", 79, "float scale = width > 0.f ? (float)buckets / width : 0.f;"),
    ("hept_amd/csrc/sort_tables.hip", 80, "if (!(scale < 3.0e38f)) scale = 0.f;"),
    ("hept_amd/csrc/sort_tables.hip", 91, "float off = (float)code * span;"),
    ("hept_amd/csrc/sort_tables.hip", 100, "t2 = t2 * cf;"),
    ("hept_amd/csrc/sort_tables.hip", 107, "return m * 1.0001f + 1.f;"),
    ("hept_amd/csrc/sort_tables.hip", 182, "while ((size_t)c * 32 < (size_t)N) c <<= 1;"),
    ("hept_amd/csrc/sort_tables.hip", 249, "const bool vec_ok = (N % 4) == 0;"),
    ("hept_amd/csrc/sort_tables.hip", 314, "const float width = (hi + cmax * span) - lo;"),
    ("hept_amd/csrc/sort_tables.hip", 384, "const unsigned int ov = end > rg.capb ? end - (gbase > rg.capb ? gbase : rg.capb) : 0u;"),
    ("hept_amd/csrc/sort_tables.hip", 423, "pool[over_s[d] + (slot - (gb > rg.capb ? gb : rg.capb))] = stage_s[lp];"),
    ("hept_amd/csrc/sort_tables.hip", 584, "if (n_chunks <= HEPT_WAVE) {"),
    ("hept_amd/csrc/sort_tables.hip", 559, "const bool table_in_lds = REGION || n_chunks <= MAXR;"),
    ("hept_amd/csrc/sort_tables.hip", 641, "if (nb <= LEAN_SLOTS * BKT_THREADS) {"),
    ("hept_amd/csrc/sort_tables.hip", 651, "if (nb > (int)rga.capb) {"),
    ("hept_amd/csrc/sort_tables.hip", 714, "while ((2 << lpr_log) * n_chunks <= BKT_THREADS) ++lpr_log;"),
    ("hept_amd/csrc/sort_tables.hip", 715, "longest <= (ITEMS << lpr_log);"),
    ("hept_amd/csrc/sort_tables.hip", 755, "bool in_lds = nb <= 2 * CAP;"),
    ("hept_amd/csrc/sort_tables.hip", 785, "if (n_low > CAP || nb - n_low > CAP) in_lds = false;"),
    ("hept_amd/csrc/sort_tables.hip", 1064, "if (Q == 1 || b / BQ == (unsigned int)part) {"),
    ("hept_amd/csrc/sort_tables.hip", 1168, "if (SMALL_SPLIT > 1 && !no_split && segs <= 128 && N > SMALL_THREADS) {"),
    ("hept_amd/csrc/sort_tables.hip", 1196, "inline bool region_range(int N) { return N > SMALL_CAP && N <= REGION_MAX_N; }"),
    ("hept_amd/csrc/sort_tables.hip", 1249, "if (b.rg.region && !region_sort_off()) {"),
    ("hept_amd/csrc/sort_tables.hip", 1264, "if ((size_t)N <= (size_t)NTOP * (BKT_CAP_SMALL / 2))"),
    ("hept_amd/csrc/sort_tables.hip", 1276, "if (ks.N <= (1 << EMBED_SHIFT))"),
    ("hept_amd/csrc/sort_tables.hip", 1340, "if (N <= SMALL_CAP)"),
]

ALL_TAGS = {"lean", "general-one-pass", "two-pass", "two-pass-refused-low", "two-pass-refused-high", "splitters",
            "region-overflow-straddle", "region-overflow-whole-run", "gathered", "by-run", "by-position", "table-wave",
            "table-lds", "table-global", "small-q1", "small-q4", "small-quarter-edge", "scale-zero", "clamp-high",
            "vec-load", "scalar-load", "ragged-empty-chunk"}


def all_instantiations():
    """The reachable ones, which are also the compiled ones: REGION and the small tile serve N <= 131 072 < 2^20 only,
    so run_passes_impl instantiates chunk_sort_kernel<MODE, EMBED, true> and bucket_sort_kernel<1024, EMBED, 64, *>
    with EMBED alone."""
    out = set()
    for mode in (0, 1, 2):
        out |= {("chunk", mode, True, True), ("chunk", mode, True, False), ("chunk", mode, False, False)}
        out |= {("small", mode, 1), ("small", mode, SMALL_SPLIT)}
    out |= {("bucket", BKT_CAP, True, 64, True), ("bucket", BKT_CAP, True, 64, False),
            ("bucket", LARGE_TILE * BKT_CAP, True, 1024, False), ("bucket", LARGE_TILE * BKT_CAP, False, 1024, False)}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cells
# ---------------------------------------------------------------------------------------------------------------------
# Hot: one planted bucket.  ``bucket`` is rotated per segment group (+ 11 per group); ``spread``:
#   "all"             every bin in turn, alternating between the halves; fractions cycling (ties once n > 512 * 15)
#   ("halves", a, b)  a pairs over bins 0..255, b pairs over bins 256..511
#   "edge"            half the pairs in bin 255, half in bin 256
#   ("groups", ...)   id groups of the given sizes of EQUAL keys, one bin each (bins 2, 3, ...)
#   ("pile", bin)     all pairs one key
# ``chunks``: None (positions at random) or ((chunk, count), ...).
Hot = namedtuple("Hot", "bucket n spread chunks")
# mode 0 / 1: segs = 2 * Tl * H (q then k);  mode 2: S segments.  ``lens``: ragged argsort.  ``opt``: a frozenset of
# flags -- "span0", "cmax0", "negzero", "inftail", "small-edges", "small-quarter", "all-equal"
Cell = namedtuple("Cell", "id part mode N Tl H S hots lens linear opt")

GROUPS = (1, 2, 3, 4, 5, 8, 9)
HB = 100                                # the first hot bucket; a second one sits at 37, a third at 180


def _cell(cid, part, mode, n, hots=(), tl=1, h=None, s=None, lens=None, linear=False, opt=()):
    if h is None:
        h = 2 if n <= REGION_MAX_N else 1
    if s is None:
        s = 2 if n <= (1 << 21) else 1
    return Cell(cid, part, mode, n, tl, h, s, tuple(hots), lens, linear, frozenset(opt))


def _region_plants():
    """(name, N, hots) of part 2's region-layout cells."""
    out = []
    for nb in (0, 1, 2, 511, 512, 513, 1023, 1024, 1025):
        out.append((f"nb{nb}", 6148, [Hot(HB, nb, "all", None)]))
    for n in (6400, 32769):
        for nb in (2047, 2048, 2049):
            out.append((f"n{n}-nb{nb}", n, [Hot(HB, nb, "all", None)]))
    for nb in (4096, 4097):
        out.append((f"n65537-nb{nb}", 65537, [Hot(HB, nb, "all", None)]))
    cap = BKT_CAP
    for name, a, b in (("1024-1024", cap, cap), ("1024-1", cap, 1), ("1-1024", 1, cap), ("1025-1", cap + 1, 1),
                       ("1-1025", 1, cap + 1)):
        out.append((f"halves-{name}", 6400, [Hot(HB, a + b, ("halves", a, b), None)]))
    out.append(("lower-half", 6400, [Hot(HB, 1500, ("halves", 1500, 0), None)]))
    out.append(("upper-half", 6400, [Hot(HB, 1500, ("halves", 0, 1500), None)]))
    out.append(("half-edge", 6400, [Hot(HB, 1500, "edge", None)]))
    out.append(("groups-lean", 6148, [Hot(HB, sum(GROUPS) + 200, ("groups",) + GROUPS + (200,), None)]))
    out.append(("groups-600", 6148, [Hot(HB, sum(GROUPS) + 600, ("groups",) + GROUPS + (600,), None)]))
    four = tuple((c, 600) for c in range(4))
    out.append(("pool3", 16384, [Hot(HB, 2400, "all", four), Hot(37, 2400, ("halves", 2400, 0), four),
                                 Hot(180, 2400, ("pile", 77), four)]))
    out.append(("straddle", 6148, [Hot(HB, 1200, "all", ((0, 600), (1, 600)))]))
    out.append(("whole-run", 12292, [Hot(HB, 1800, "all", ((0, 600), (1, 600), (2, 600)))]))
    return out


def _linear_plants():
    big = LARGE_TILE * BKT_CAP
    out = []
    for nb in (big - 1, big, big + 1):
        out.append((f"nb{nb}", [Hot(HB, nb, "all", None)]))
    out.append((f"nb{2 * big}", [Hot(HB, 2 * big, ("halves", big, big), None)]))
    out.append((f"nb{2 * big + 1}", [Hot(HB, 2 * big + 1, "all", None)]))
    # a hot bucket drawn from every chunk but number 16: a run of length 0 in the middle of the chunk list
    out.append(("zero-run", [Hot(HB, 3100, "all", tuple((c, 100) for c in range(32) if c != 16))]))
    return out


RAGGED_LENS = (0, 1, 4095, 4096, 4097, 6144, 6145)
SLOW = ("pool3", "halves-1024-1024", "lower-half")       # part 4: pool + gathered (+ splitters), two-pass, splitters


def _cells():
    out = []
    # ---- part 1: every instantiation at the smallest N that selects it
    for mode in (0, 1, 2):
        for n in (1, 2, 3, 1023, 1024, 1025, 6143, 6144):
            out.append(_cell(f"inst-m{mode}-n{n}", "inst", mode, n))
        # Q = 4 needs at most 128 segments and N > 1 024: 128 / 130 segments at 1 025, 128 at 1 024
        for n, tl, h in ((1025, 4, 16), (1025, 5, 13), (1024, 4, 16)):
            out.append(_cell(f"inst-m{mode}-n{n}-s{2 * tl * h}", "inst", mode, n, tl=tl, h=h, s=2 * tl * h))
        for n in (6145, 6148, 32768, 32769, 65536, 65537, 131072, 131073, 262144, 262145, 1 << 20, (1 << 20) + 1):
            out.append(_cell(f"inst-m{mode}-n{n}", "inst", mode, n))
    for n in (4194304, 4194305):
        out.append(_cell(f"inst-m2-n{n}", "inst", 2, n))
    # ---- part 2: planted populations
    for mode in (0, 1, 2):
        for name, n, hots in _region_plants():
            out.append(_cell(f"region-m{mode}-{name}", "region", mode, n, hots))
    for mode in (0, 2):
        for name, hots in _linear_plants():
            out.append(_cell(f"linear-m{mode}-{name}", "linear", mode, 131073, hots))
    for mode in (0, 1, 2):
        out.append(_cell(f"small-m{mode}-quarter-edges", "small", mode, 6000, opt=("small-edges",)))
        out.append(_cell(f"small-m{mode}-one-quarter", "small", mode, 6000, opt=("small-quarter",)))
        out.append(_cell(f"small-m{mode}-all-equal", "small", mode, 6144, opt=("all-equal",)))
        out.append(_cell(f"small-m{mode}-groups", "small", mode, 6144, [Hot(HB, sum(GROUPS) + 600, ("groups",) + GROUPS + (600,), None)]))
    for mode in (0, 1):
        out.append(_cell(f"degen-m{mode}-span0", "degen", mode, 6148, opt=("span0",)))
        out.append(_cell(f"degen-m{mode}-span0-small", "degen", mode, 3000, opt=("span0",)))
        out.append(_cell(f"degen-m{mode}-inftail", "degen", mode, 6400, [Hot(HB, 3000, ("pile", 5), None)], opt=("inftail",)))
    out.append(_cell("degen-m0-cmax0", "degen", 0, 6148, [Hot(HB, 1025, "all", None)], opt=("cmax0",)))
    for mode in (0, 1, 2):
        out.append(_cell(f"degen-m{mode}-negzero", "degen", mode, 6148, opt=("negzero",)))
        out.append(_cell(f"degen-m{mode}-negzero-small", "degen", mode, 2000, opt=("negzero",)))
    # ---- part 3: ragged argsort on planted rows
    for length in (8200, 6144):
        lens = tuple(x for x in RAGGED_LENS if x <= length) + (length - 1, length)
        out.append(_cell(f"ragged-l{length}", "ragged", 2, length, [Hot(HB, 1300, "all", None)], s=len(lens), lens=lens))
    # ---- part 6: the region-size cells in the linear layout (HEPT_SORT_LINEAR=1, one child process)
    for mode in (0, 2):
        for name, n, hots in _region_plants():
            out.append(_cell(f"ab-m{mode}-{name}", "ab", mode, n, hots, linear=True))
    return out


CELLS = _cells()
BY_ID = {c.id: c for c in CELLS}
GPU_CELLS = [c for c in CELLS if not c.linear]
AB_CELLS = [c for c in CELLS if c.linear]
SCRATCH_CELLS = [BY_ID[f"region-m{m}-{name}"] for m in (0, 2) for name in SLOW] + \
                [BY_ID[f"linear-m{m}-nb{LARGE_TILE * BKT_CAP - 1}"] for m in (0, 2)]
SCRATCH_PATTERNS = ("zero", "ff")


def n_segs(c):
    return c.S if c.mode == 2 else 2 * c.Tl * c.H


def n_groups(c):
    """Key sets a cell draws: one per (table, head) -- the q and the k segment share codes -- or one per raw segment."""
    return c.S if c.mode == 2 else c.Tl * c.H


def t0_of(c):
    return 1


def tables_of(c):
    return t0_of(c) + c.Tl + 1            # T > t0 + Tl: a table on either side of the slab


# ---------------------------------------------------------------------------------------------------------------------
# the float32 mirror of the dispatch and of the id map
# ---------------------------------------------------------------------------------------------------------------------
F = np.float32


def dispatch(c):
    """What the host code launches: instantiations, layout, tile, region capacity, chunks."""
    n, segs = c.N, n_segs(c)
    if n <= SMALL_CAP:
        q = SMALL_SPLIT if segs <= 128 and n > SMALL_THREADS else 1
        return dict(layout="small", inst={("small", c.mode, q)}, q=q, bins=SMALL_BINS)
    embed = n <= (1 << EMBED_SHIFT)
    region = n <= REGION_MAX_N and not c.linear
    n_chunks = -(-n // SORT_CHUNK)
    if region:
        bucket = ("bucket", BKT_CAP, embed, 64, True)
    elif n <= NTOP * (BKT_CAP // 2):
        bucket = ("bucket", BKT_CAP, embed, 64, False)
    else:
        bucket = ("bucket", LARGE_TILE * BKT_CAP, embed, 1024, False)
    return dict(layout="region" if region else "linear", inst={("chunk", c.mode, embed, region), bucket}, cap=bucket[1],
                maxr=bucket[3], capb=region_cap(n) if region else None, n_chunks=n_chunks, bins=ID_BUCKETS)


def _scale(width, bins):
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        scale = F(bins) / width if width > 0 else F(0)
    return scale if scale < F(3.0e38) else F(0)


def range_of(c, d, g):
    """(lo, span, scale) of group g as the kernels compute them, in float32."""
    bins = dispatch(c)["bins"]
    if c.mode == 2:
        k = d["keys"][g]
        if c.lens is not None:
            k = k[:c.lens[g]]
        k = k[np.isfinite(k)]
        lo, hi = (F(k.min()), F(k.max())) if k.size else (F(0), F(0))
        return lo, F(0), _scale(hi - lo, bins)
    mm = d["minmax"].reshape(-1, PREP_GRID, 4)[g]
    lo, hi, cmax = F(mm[:, 0].min()), F(mm[:, 1].max()), F(max(mm[:, 2].max(), 0))
    if c.mode == 1:
        t, h = divmod(g, c.H)
        eta, phi, cf = d["eta"][t0_of(c) + t, h], d["phi"][t0_of(c) + t, h], d["cfac"][t0_of(c) + t, h]
        ok = np.isfinite(eta) & np.isfinite(phi)
        m = F(max(F(0), (phi[ok].astype(np.float64) * float(cf) + eta[ok]).astype(F).max())) if ok.any() else F(0)   # fmaf: one rounding
        cmax = F(F(m * F(1.0001)) + F(1))
        if c.N > SMALL_CAP:
            cmax = max(cmax, F(np.delete(mm[:, 2], 0).max()))       # slot 0 column 2 is overwritten with the bound
    span = F(hi - lo)
    width = F(F(hi + F(cmax * span)) - lo)
    return lo, span, _scale(width, bins)


def keys32(c, d, g):
    """float32 keys of group g, every operation rounded on its own: (q keys, k keys) or (raw keys,)."""
    if c.mode == 2:
        return (d["keys"][g],)
    t, h = divmod(g, c.H)
    _, span, _ = range_of(c, d, g)
    with np.errstate(invalid="ignore"):
        if c.mode == 0:
            off = d["codes"][t0_of(c) + t, h].astype(F) * span
        else:
            t1 = d["eta"][t0_of(c) + t, h] * span
            t2 = d["phi"][t0_of(c) + t, h] * span
            t2 = t2 * d["cfac"][t0_of(c) + t, h]
            off = t2 + t1
        return (d["qproj"][t, h] + off).astype(F), (d["kproj"][t, h] + off).astype(F)


def ids_of(k32, lo, scale, bins):
    """bucket_id<bins>: (ids, keys whose scaled value lies at or beyond the id range)."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = (k32 - lo).astype(F) * scale
    x = np.where(np.isnan(x), F(bins - 1), x)                 # fminf(NaN, b) = b: inf * 0
    beyond = x >= bins
    return np.clip(np.minimum(x, F(bins - 1)).astype(np.int64), 0, bins - 1), beyond


def segments(c, d):
    """Every segment of the cell in the kernels' order: (group, float32 keys, length that takes part)."""
    ng = n_groups(c)
    if c.mode == 2:
        return [(g, d["keys"][g], c.N if c.lens is None else c.lens[g]) for g in range(ng)]
    ks = [keys32(c, d, g) for g in range(ng)]
    return [(g, ks[g][0], c.N) for g in range(ng)] + [(g, ks[g][1], c.N) for g in range(ng)]


_stats = {}


def stats(c):
    """The mirror's numbers: per segment ``pop``, ``low``, ``group`` (per bucket) and ``runs`` (chunk, bucket); ``ids``."""
    if c.id in _stats:
        return _stats[c.id]
    d, dp = data(c), dispatch(c)
    bins = dp["bins"]
    top = bins // NTOP
    segs = []
    for g, k32, length in segments(c, d):
        lo, _, scale = range_of(c, d, g)
        ids, beyond = ids_of(k32[:length], lo, scale, bins)
        bucket = ids // top
        per_id = np.bincount(ids, minlength=bins).reshape(NTOP, top)
        rec = dict(group=g, scale=float(scale), pop=per_id.sum(1), low=per_id[:, :top // 2].sum(1), maxgroup=per_id.max(1),
                   beyond=int(beyond.sum()), len=length, present=per_id.reshape(-1) > 0)
        if dp["layout"] != "small":
            chunk = np.arange(length) // SORT_CHUNK
            rec["runs"] = np.bincount(chunk * NTOP + bucket, minlength=dp["n_chunks"] * NTOP).reshape(dp["n_chunks"], NTOP)
        segs.append(rec)
    if len(_stats) > 8:
        _stats.clear()
    _stats[c.id] = dict(dispatch=dp, segs=segs)
    return _stats[c.id]


def bucket_tags(dp, nb, n_low, runs):
    """The branches one bucket of nb > 0 pairs takes in bucket_sort_kernel."""
    out = set()
    cap = dp["cap"]
    if dp["layout"] == "region":
        if nb <= LEAN_MAX:
            return {"lean"}
        capb = dp["capb"]
        if nb > capb:
            out.add("gathered")
            # whatever order the chunks' atomics arrive in: with every run longer than capb / 2 and shorter than capb the
            # second run to arrive straddles the end of the region and every later one starts beyond it
            r = runs[runs > 0]
            if len(r) >= 2 and bool(((2 * r > capb) & (r < capb)).all()):
                out.add("region-overflow-straddle")
                if len(r) >= 3:
                    out.add("region-overflow-whole-run")
    else:
        n_chunks = dp["n_chunks"]
        lpr_log = 0
        while (2 << lpr_log) * n_chunks <= BKT_THREADS:
            lpr_log += 1
        by_run = n_chunks <= WAVE and int(runs.max()) <= ((cap // BKT_THREADS) << lpr_log)
        out.add("by-run" if by_run else "by-position")
    if nb <= cap:
        out.add("general-one-pass")
    elif nb <= 2 * cap:
        if n_low > cap:
            out |= {"two-pass-refused-low", "splitters"}
        elif nb - n_low > cap:
            out |= {"two-pass-refused-high", "splitters"}
        else:
            out.add("two-pass")
    else:
        out.add("splitters")
    return out


def tags(c):
    """Branch names of the cell, from the mirror's numbers alone."""
    st = stats(c)
    dp, out = st["dispatch"], set()
    if any(s["scale"] == 0.0 for s in st["segs"]):
        out.add("scale-zero")
    if c.mode != 2 and any(s["beyond"] for s in st["segs"]):
        out.add("clamp-high")
    if dp["layout"] == "small":
        out.add(f"small-q{dp['q']}")
        bq = SMALL_BINS // SMALL_SPLIT
        for s in st["segs"]:
            if dp["q"] > 1 and all(s["present"][b - 1] and s["present"][b] for b in (bq, 2 * bq, 3 * bq)):
                out.add("small-quarter-edge")
        return out
    out.add("vec-load" if c.N % 4 == 0 else "scalar-load")
    if c.lens is not None and any(length <= ch * SORT_CHUNK for length in c.lens for ch in range(dp["n_chunks"])):
        out.add("ragged-empty-chunk")
    if dp["layout"] == "linear":
        nc = dp["n_chunks"]
        out.add("table-wave" if nc <= WAVE else "table-lds" if nc <= dp["maxr"] else "table-global")
    for s in st["segs"]:
        seen = set()
        for b in np.nonzero(s["pop"])[0]:
            nb, n_low, runs = int(s["pop"][b]), int(s["low"][b]), s["runs"][:, b]
            if dp["layout"] == "linear":                     # (by-run depends on the longest run only)
                key = (nb, n_low, int(runs.max()))
            else:
                key = (nb, n_low, tuple(runs)) if nb > dp["capb"] else (nb, n_low)
            if key not in seen:
                seen.add(key)
                out |= bucket_tags(dp, nb, n_low, runs)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
GRID = 65536.0                            # keys are multiples of 2^-16 below 256: 24 bits
NFR = 15                                  # fractions 1/16 .. 15/16 of an id's interval


def _rng(c, g):
    return np.random.default_rng(zlib.crc32(f"{c.id}/{g}".encode()))


def hot_bucket(c, hot, g):
    return (hot.bucket + 11 * g) % 240


def nominal_scale(c):
    """The id map the plan is drawn for: ids per unit of key (float64).  Mode 1: the mirror's own float32 scale for shifts
    up to 255."""
    bins = dispatch(c)["bins"]
    if c.mode != 1:
        return bins / 256.0
    cmax = F(F(F(255) * F(1.0001)) + F(1))
    return float(_scale(F(F(F(1) + F(cmax * F(1))) - F(0)), bins))


def _hot_ids(c, hot, g, top):
    """(low-id bin, fraction index) of the hot bucket's pairs."""
    n, sp = hot.n, hot.spread
    j = np.arange(n)
    if sp == "all":
        return (j * (top // 2 + 1)) % top, (j // top) % NFR      # (odd stride: alternates between the halves)
    if sp == "edge":
        return np.where(j % 2 == 0, top // 2 - 1, top // 2), (j // 2) % NFR
    if sp[0] == "halves":
        a = sp[1]
        half = top // 2
        ja, jb = np.arange(a), np.arange(n - a)
        return np.concatenate([ja % half, half + jb % half]), np.concatenate([(ja // half) % NFR, (jb // half) % NFR])
    if sp[0] == "groups":
        sizes = sp[1:]
        assert sum(sizes) == n
        return np.repeat(2 + np.arange(len(sizes)), sizes), np.repeat((3 + np.arange(len(sizes))) % NFR, sizes)
    if sp[0] == "pile":
        return np.full(n, sp[1] % top), np.full(n, 7)
    raise AssertionError(sp)


def plan(c, g):
    """Keys of group g as float64 on the grid, in point order, and the group's intended hot populations."""
    n, rng = c.N, _rng(c, g)
    dp = dispatch(c)
    bins = dp["bins"]
    top = bins // NTOP                                       # ids per top-level bucket (quarters: 4 buckets of 64 ... )
    scale = nominal_scale(c)
    key = np.full(n, -1.0)
    free = np.ones(n, bool)

    def to_key(ids, fr):
        return np.round((ids + (fr + 1) / 16.0) / scale * GRID) / GRID

    if "span0" in c.opt:
        return np.full(n, 0.25), {}
    if "all-equal" in c.opt:
        return np.full(n, 77.5), {}
    # anchors: the smallest and the largest key of the nominal range (mode 2: they ARE the range; mode 1: the largest
    # shift fixes the bound)
    anchors = {0: 0.0}
    if n >= 2:
        anchors[1] = 256.0 if c.mode == 2 else 255.5
    if c.mode != 2 and ("small-quarter" in c.opt):
        anchors = {0: 255.5} if c.mode == 1 else {}
    for i, v in anchors.items():
        key[i], free[i] = v, False
    max_bucket = (int(255.0 * scale) // top) if c.mode == 1 else NTOP       # mode 1: keys below 255 only (bound = 255)
    hot_set, want = set(), {}
    for hot in c.hots:
        b = hot_bucket(c, hot, g)
        hot_set.add(b)
        want[b] = hot.n
        lo_id, fr = _hot_ids(c, hot, g, top)
        k = to_key(b * top + lo_id, fr)
        if hot.chunks is None:
            pos = rng.choice(np.nonzero(free)[0], hot.n, replace=False) if hot.n else np.zeros(0, int)
            pos.sort()
            pos = pos[rng.permutation(hot.n)] if hot.n else pos
        else:
            assert sum(cnt for _, cnt in hot.chunks) == hot.n
            parts = []
            for ch, cnt in hot.chunks:
                cand = np.nonzero(free[ch * SORT_CHUNK:(ch + 1) * SORT_CHUNK])[0] + ch * SORT_CHUNK
                parts.append(rng.choice(cand, cnt, replace=False))
            pos = np.concatenate(parts)
            k = k[rng.permutation(hot.n)]
        key[pos], free[pos] = k, False
    rest = np.nonzero(free)[0]
    r = len(rest)
    if r:
        j = np.arange(r) // 2                                # every background key at least twice: ties in every bucket
        hsh = (j * 2654435761 + zlib.crc32(c.id.encode()) + 977 * g) % (1 << 32)
        if "small-edges" in c.opt:                           # ids on either side of every quarter boundary, and elsewhere
            bq = bins // SMALL_SPLIT
            pool_ids = np.array([q * bq + e for q in (1, 2, 3) for e in (-2, -1, 0, 1)] + [5, bq + 9, 2 * bq + 9, bins - 200])
            ids = pool_ids[hsh % len(pool_ids)]
        elif "small-quarter" in c.opt:                       # all keys in the second quarter of the id range
            bq = bins // SMALL_SPLIT
            ids = bq + 8 + hsh % (bq - 16)
        else:
            bg = np.array([b for b in range(max_bucket) if b not in hot_set])
            ids = bg[j % len(bg)] * top + (hsh >> 8) % top
        k = to_key(ids, (hsh >> 20) % NFR)
        key[rest] = k[rng.permutation(r)]
    if "negzero" in c.opt:                                   # -0.0 and +0.0 interleaved at the bottom of the range
        z = np.nonzero((np.arange(n) % 5 == 2) & (np.arange(n) > 1))[0]
        key[z] = np.where(np.arange(len(z)) % 2 == 0, -0.0, 0.0)
    assert (key >= 0).all()
    return key, want


_data = {}


def data(c):
    """The cell's inputs as numpy arrays (what the GPU call gets) -- cached, a few cells at a time."""
    if c.id in _data:
        return _data[c.id]
    n, ng = c.N, n_groups(c)
    keys, wants = zip(*(plan(c, g) for g in range(ng)))
    keys = np.stack(keys)
    d = dict(want=wants)
    if c.mode == 2:
        k32 = keys.astype(F)
        assert (k32.astype(np.float64) == keys).all()
        d["clean"] = k32
        if c.lens is not None:                               # NaN and -1e30 behind lens
            k32 = k32.copy()
            for s_, length in enumerate(c.lens):
                k32[s_, length:] = np.nan if s_ % 2 else -1e30
        d["keys"] = k32
    else:
        tl, h, t0, t = c.Tl, c.H, t0_of(c), tables_of(c)
        keys = keys.reshape(tl, h, n)
        code = np.floor(keys)
        code = np.where(keys == 0, 0.0, code)                 # (-0.0)
        proj_q = keys - code
        proj_q = np.where(np.signbit(keys) & (keys == 0), -0.0, proj_q)
        # k: the same codes (a point has one code), the projections of its (code, chunk) group in reverse point order --
        # the same keys in every chunk, so the runs are the planted ones in the k segments as well
        idx = np.arange(n)
        proj_k = np.empty_like(proj_q)
        for a in range(tl):
            for b in range(h):
                grp = code[a, b] * (n // SORT_CHUNK + 1) + idx // SORT_CHUNK
                up, down = np.lexsort((idx, grp)), np.lexsort((-idx, grp))
                proj_k[a, b, up] = proj_q[a, b, down]
        if "inftail" in c.opt:                               # the src variant's padding rows: +inf behind everything
            proj_k[..., n - 200:] = np.inf
            proj_q[..., n - 200:] = np.inf
        full = np.empty((t, h, n))
        full[t0:t0 + tl] = code
        for tt in list(range(t0)) + list(range(t0 + tl, t)):  # other tables: other codes (a wrong row offset shows)
            full[tt] = 255.0 - code[(tt + 1) % tl]
        span = 0.0 if "span0" in c.opt else 1.0
        lo = 0.25 if "span0" in c.opt else 0.0
        mm = np.zeros((tl, h, PREP_GRID, 4), F)
        mm[..., 0], mm[..., 1] = np.inf, -np.inf
        for a in range(tl):
            for b in range(h):
                # lo, hi and cmax in three different slots, one of them the last; which holds which rotates
                slots = [(3 + 5 * b + a) % 500, 511 + ((7 * b + a) % 400), PREP_GRID - 1]
                r = (a + b) % 3
                s_lo, s_hi, s_c = slots[r], slots[(r + 1) % 3], slots[(r + 2) % 3]
                mm[a, b, s_lo, :2] = lo
                mm[a, b, s_hi, :2] = lo + span
                if c.mode == 0:
                    mm[a, b, s_c, 2] = 0.0 if "cmax0" in c.opt else 255.0
        d.update(qproj=proj_q.astype(F), kproj=proj_k.astype(F), minmax=mm)
        assert (d["qproj"].astype(np.float64) == proj_q).all() and (d["kproj"].astype(np.float64) == proj_k).all()
        if c.mode == 0:
            d["codes"] = full.astype(np.int64)
        else:
            cf = np.array([[F(2 << ((tt + hh) % 3)) for hh in range(h)] for tt in range(t)], F)    # 2, 4, 8
            low = np.mod(full, 8.0)
            d["eta"] = (full - low).astype(F)
            d["phi"] = (low / cf[..., None]).astype(F)
            d["cfac"] = cf
    if len(_data) > 4:
        _data.clear()
    _data[c.id] = d
    return d


def host_keys(c, d):
    """float64 keys of every segment, computed from the inputs alone: list of 1-D arrays in the kernels' segment order
    (ragged: the prefix that takes part, from the rows before they were poisoned)."""
    if c.mode == 2:
        src = d["clean"].astype(np.float64)
        return [src[s_, :(c.N if c.lens is None else c.lens[s_])] for s_ in range(c.S)]
    t0, tl = t0_of(c), c.Tl
    mm = d["minmax"].astype(np.float64)
    span = (mm[..., 1].max(-1) - mm[..., 0].min(-1))[..., None]
    with np.errstate(invalid="ignore"):
        if c.mode == 0:
            shift = d["codes"][t0:t0 + tl].astype(np.float64) * span
        else:
            cf = d["cfac"][t0:t0 + tl].astype(np.float64)[..., None]
            shift = d["phi"][t0:t0 + tl].astype(np.float64) * span * cf + d["eta"][t0:t0 + tl].astype(np.float64) * span
        q, k = d["qproj"].astype(np.float64) + shift, d["kproj"].astype(np.float64) + shift
    return [x for x in q.reshape(-1, c.N)] + [x for x in k.reshape(-1, c.N)]


def expected(c, d):
    """torch.sort(stable=True) of the float64 host keys: one index tensor per segment."""
    return [torch.sort(torch.from_numpy(np.ascontiguousarray(k)), stable=True).indices for k in host_keys(c, d)]


# ---------------------------------------------------------------------------------------------------------------------
# GPU (imports deferred)
# ---------------------------------------------------------------------------------------------------------------------
def run(c, d, dev):
    """The cell's one call; returns the permutations as a (segments, N) int32 tensor on the device."""
    from hept_amd import ops

    up = lambda name: torch.from_numpy(d[name]).to(dev)
    if c.mode == 2:
        lens = None if c.lens is None else torch.tensor(c.lens, dtype=torch.int32, device=dev)
        return ops.segmented_argsort(up("keys"), lens)
    if c.mode == 0:
        qp, kp = ops.sort_tables(up("qproj"), up("kproj"), up("codes"), up("minmax"), t0=t0_of(c))
    else:
        qp, kp = ops.sort_tables_src(up("qproj"), up("kproj"), up("eta"), up("phi"), up("cfac"), up("minmax"), t0=t0_of(c))
    assert qp.shape == kp.shape == (c.Tl, c.H, c.N) and qp.dtype == torch.int32
    return torch.cat([qp.reshape(-1, c.N), kp.reshape(-1, c.N)])


def compare(c, pos, want):
    pos = pos.long().cpu()
    assert pos.shape[0] == len(want)
    half = len(want) // 2
    for s_, w in enumerate(want):
        name = f"segment {s_}" if c.mode == 2 else f"{'q' if s_ < half else 'k'} segment {s_ % half}"
        assert torch.equal(pos[s_, :len(w)], w), \
            f"{c.id}: {name}: the permutation differs from the stable sort of the float64 host keys"


def check(c, dev):
    d = data(c)
    want = expected(c, d)
    compare(c, run(c, d, dev), want)
    if "cmax0" in c.opt:
        # the code bound is only a scale: with the true bound every key keeps its own bucket -- the same permutation
        mm = d["minmax"].copy()
        mm[..., 2] = 0.0
        mm[..., 5, 2] = 255.0
        compare(c, run(c, dict(d, minmax=mm), dev), want)


def check_scratch(c, pattern, dev):
    """Part 4: the same permutation with every buffer of the call guarded and pre-filled, and intact guards."""
    import scratch_sweep as ss

    d = data(c)
    want = expected(c, d)
    with ss.scratch(pattern) as ledger:
        pos = run(c, d, dev)
    ledger.check()
    assert len(ledger.entries) >= 2                          # workspace and permutations
    compare(c, pos, want)


# ---- part 5: the forward's own sort launch (region counters zeroed by the row builder, riders in the grid) ------------
LAUNCH_N = 10944
LAUNCH_PRECISIONS = ("fp32", "bf16")
DUP_SHARE = 0.3


def dup_index(n, seed):
    """Point indices that become exact duplicates of point ``src``: 30 % of the points, spread over all chunks."""
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(np.arange(1, n), int(DUP_SHARE * n), replace=False))
    return 0, torch.from_numpy(idx)


def check_launch(precision, dev):
    """Example variant: the one-call forward equals the staged pipeline bit for bit on a cloud whose id group of ~3 300
    ties overflows its 1 024-slot region in every segment, and the staged sort equals the float64 host keys."""
    import rows_sweep as rs
    import shape_sweep as sw
    from hept_amd import ops

    s = rs.two_role_shape(LAUNCH_N, (8, 24, 6))._replace(id="sort-launch", T=2)
    assert sw.riders(LAUNCH_N, s.H, s.D, s.T, precision, s.B) and region_cap(LAUNCH_N) == 1024
    inp = sw.inputs(s)
    src, idx = dup_index(LAUNCH_N, 5)
    for name in ("q", "k", "coords"):
        inp[name] = inp[name].clone()
        inp[name][idx] = inp[name][src].clone()
    inp["combined_shifts"] = inp["combined_shifts"].clone()
    inp["combined_shifts"][..., idx] = inp["combined_shifts"][..., src:src + 1].clone()
    assert len(torch.unique(inp["v"][idx], dim=0)) == len(idx)          # distinct v rows: the output depends on the tie order
    g = sw._gpu(inp, dev)
    prec = sw.PRECISIONS[precision][0]
    sqrt_w = ops.rpe_scale(g["w_rpe_weight"], s.H, s.D, 10)
    ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sqrt_w, g["alpha"], g["combined_shifts"], prec)
    qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"])
    # (random inputs: the host key takes the kernel's two float32 roundings, one eager CPU operation each)
    mm = ph["minmax"].cpu()
    span = (mm[..., 1].amax(-1) - mm[..., 0].amin(-1))[..., None]
    off = inp["combined_shifts"].float() * span
    for nm, pos, proj in (("q", qp, ph["qproj"]), ("k", kp, ph["kproj"])):
        key = (proj.cpu() + off).double()
        assert int((key[0, 0] == key[0, 0, src]).sum()) >= len(idx)     # the pile is one id group of equal keys
        assert torch.equal(pos.long().cpu(), torch.sort(key, dim=-1, stable=True).indices), \
            f"sort-launch {precision}: {nm} permutation differs from the stable sort of the float64 host keys"
    st = sw.staged(s, g, precision)
    assert torch.equal(st["qpos"], qp) and torch.equal(st["kpos"], kp)
    one = ops.forward(g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"],
                      g["out_weight"], g["out_bias"], block_size=s.B, w_per_dist=10, precision=prec)
    assert bool(torch.isfinite(one).all())
    assert rs._same_bits(one, st["out"]), f"sort-launch {precision}: one-call forward differs from the staged kernels"


def check_launch_src(precision, dev):
    """The src variant of ``check_launch``: the one-call ``ops.forward_src`` against its staged kernels."""
    import rows_sweep as rs
    import shape_sweep as sw
    import src_attn_sweep as ssw
    from hept_amd import ops

    s = ssw.Shape("sort-launch-src", LAUNCH_N, LAUNCH_N - 5, 32, 2, 6, False, 77, False)
    assert sw.riders(LAUNCH_N, ssw.H, ssw.D, s.T, precision, s.B)
    inp = ssw.inputs(s)
    src, idx = dup_index(s.raw, 6)
    inp["coords"] = inp["coords"].clone()
    inp["coords"][idx] = inp["coords"][src].clone()
    for nm in ("eta", "phi"):
        shape = inp[nm].shape
        e = inp[nm].reshape(-1, s.N).clone()
        e[:, idx] = e[:, src:src + 1].clone()
        inp[nm] = e.reshape(shape)
    g = ssw._gpu(inp, dev)
    p = g["params"]
    prec = sw.PRECISIONS[precision][0]
    # q and k of the duplicates are those of the source point, v stays the point's own: the stages take q, k, v
    xn = torch.nn.functional.layer_norm(g["x"], (ssw.D,), p["norm1.weight"], p["norm1.bias"], ssw.EPS)
    q, k, v = [(xn @ p[f"w_{n}.weight"].t()).contiguous() for n in "qkv"]
    di = idx.to(dev)
    q[di], k[di] = q[src].clone(), k[src].clone()
    assert len(torch.unique(v[di], dim=0)) == len(idx)
    sqrt_w = ops.rpe_scale(p["w_rpe.weight"], ssw.H, ssw.D, ssw.K)
    eta, phi, cfac = ops.geo_args((g["eta"], g["phi"]), g["regions_h"], s.T, ssw.H, s.N)
    ph = ops.prep_hash(q, k, v, g["coords"], sqrt_w, p["attn.e2lsh.alpha"], None, prec, raw_size=s.raw)
    qp, kp = ops.sort_tables_src(ph["qproj"], ph["kproj"], eta, phi, cfac, ph["minmax"].clone())
    # (random inputs: the host key takes the kernel's four float32 roundings, one eager CPU operation each)
    mm = ph["minmax"].cpu()
    span = (mm[..., 1].amax(-1) - mm[..., 0].amin(-1))[..., None]
    e32, f32 = eta.cpu().reshape(s.T, ssw.H, s.N), phi.cpu().reshape(s.T, ssw.H, s.N)
    shift = (f32 * span) * cfac.cpu().reshape(s.T, ssw.H, 1) + e32 * span
    for nm, pos, proj in (("q", qp, ph["qproj"]), ("k", kp, ph["kproj"])):
        key = (proj.cpu() + shift).double()
        assert torch.equal(pos.long().cpu(), torch.sort(key, dim=-1, stable=True).indices), \
            f"sort-launch-src {precision}: {nm} permutation differs from the stable sort of the host keys"
    part = ops.block_attn(ph["qhat"], ph["kvhat"], qp, kp, ssw.D, s.B, f32_mfma=sw.PRECISIONS[precision][1])
    staged = ops.combine_out(part, ssw.D, p["attn.out_linear.weight"], p["attn.out_linear.bias"])
    one = ops.forward_src(q, k, v, g["coords"], (g["eta"], g["phi"]), g["regions_h"], s.raw, p["w_rpe.weight"],
                          p["attn.e2lsh.alpha"], p["attn.out_linear.weight"], p["attn.out_linear.bias"], block_size=s.B,
                          w_per_dist=ssw.K, precision=prec)
    assert bool(torch.isfinite(one).all())
    assert rs._same_bits(one, staged), f"sort-launch-src {precision}: one-call forward_src differs from the staged kernels"


# ---- part 6: the child process --------------------------------------------------------------------------------------
def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.dirname(os.path.abspath(__file__))]
    if os.environ.get("HEPT_SORT_LINEAR", "") in ("", "0"):
        print("HEPT_SORT_LINEAR is not set: the linear layout at region sizes needs it")
        return 2
    dev = torch.device("cuda", 0)
    for c in AB_CELLS:
        try:
            d = data(c)
            compare(c, run(c, d, dev), expected(c, d))
        except AssertionError as e:
            print(f"MISMATCH {e}", flush=True)
            return 1
    print(f"{len(AB_CELLS)} cells in the linear layout, 0 mismatches")
    return 0


if __name__ == "__main__":
    sys.exit(main())
