"""Deterministic edge-shape sweep of the caller-side preparation (run by tests/test_gpu_prepare_sweep.py, coverage and
reference anchors pinned on CPU by tests/test_prepare_sweep_cells.py): hept_prepare_probe, hept_prepare_input and
hept_prepare_input_src in csrc/prepare.hip behind hept_amd/prep.py.

Three links.  REFERENCE -> MIRROR: tests/golden/make_golden_prepare.py ran the reference's own prepare_input (and the
src variant's caller-side statements) on every case below and stored digests of its codes in
tests/golden/prepare_sweep.npz; the host mirror (hept_amd.prep, CPU) must reproduce them.  The reference's argsort is
unstable, so the comparison is tie-aware: a real point whose eta and whose phi are unique in its cloud has ranks that
do not depend on how ties elsewhere are broken, and its codes must equal the reference's exactly (``unique_mask``).
MIRROR -> HIP: both use stable sorts, so every output is compared bit for bit, tie cases included.  INVARIANTS that need
neither: real slots keep their order, every pad slot holds the code the reference's window defines.

``cells(case)`` names the branches a case takes, mirroring the rules in csrc/prepare.hip, hept_amd/prep.py and the sort's
one-workgroup limit (csrc/sort_tables.hip SMALL_CAP).  Inputs come from a seeded CPU generator; nothing here touches the
GPU at import."""
import hashlib
import os
from collections import namedtuple

import numpy as np
import torch

Case = namedtuple("Case", "id seed path a")      # path: "example" | "src"; a: Ex | Src
# example path: sizes = points per cloud; regions / coords / dtype / batch / view: see build(); refuse: None or the
# exception the GPU front end must raise
Ex = namedtuple("Ex", "sizes B T H regions coords dtype batch view refuse",
                defaults=(("draw", 30), "randn", "f32", "i64", "contig", None))
# src path: raw = raw_size; F = feature columns; x: "f32" | "bf16" | "grad"
Src = namedtuple("Src", "raw B T H regions coords F x", defaults=(("draw", 30), "randn", 3, "f32"))

SMALL_CAP = 6144          # csrc/sort_tables.hip: segments up to this many keys are sorted by one workgroup
PROBE_CLOUDS = 255        # csrc/prepare.hip: clouds the probe kernel resolves; hept_amd/prep.py _MAX_CLOUDS_ONE_TRIP
KEY_BITS = 24             # csrc/prepare.hip code_sort_key / hept_amd/prep.py: packed codes are exact fp32 sort keys
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prepare_sweep.npz")

# integer-valued tables: every count divides 300, 150 and 450.  With 15 and 30 regions (and with 7 regions over clouds
# of 49, 98 and 343 points, the "regions-recip" cases) torch's reciprocal-times-n width is one above the true quotient:
# float32(1 / 15) * 300 rounds above 20 (cells(): "width-recip-differs")
INT_ETA = (3, 5, 6, 10, 15, 25, 30, 50)
INT_PHI = (50, 30, 25, 15, 10, 6, 5, 3)


def _many(n, lo=1, span=12):
    """n cloud sizes lo .. lo + span - 1 in a fixed pattern (no RNG: the cell rules depend on them)."""
    return tuple(lo + (i * 7 + i // 5) % span for i in range(n))


def _build_cases():
    out = []

    def ex(cid, *a, **k):
        out.append(Case(cid, len(out) + 101, "example", Ex(*a, **k)))

    def src(cid, *a, **k):
        out.append(Case(cid, len(out) + 101, "src", Src(*a, **k)))

    # ---- cloud sizes against the block
    ex("size-eqB", (64, 130), 64, 2, 3)
    ex("size-B+1", (65, 20), 64, 1, 8)
    ex("size-B-1", (63, 64, 63), 64, 3, 1)
    ex("size-multiples", (32, 96, 64), 32, 2, 8)
    ex("block-1", (5, 1, 9), 1, 2, 3)
    ex("one-point-clouds", (1, 1, 1, 70), 8, 3, 3)
    ex("forty-of-7", (7,) * 40, 8, 1, 8)
    # ---- the wrap of the first cloud's pad window.  size0 + n_raw >= B is legal (the reference wraps once); below it
    # the reference raises IndexError.  (5, 10) and (5, 11) with B = 16 lie on the legal side (5 + 15 and 5 + 16)
    ex("wrap-into-last", (3, 40), 16, 2, 3)
    ex("wrap-5-11", (5, 11), 16, 2, 3)
    ex("wrap-5-10", (5, 10), 16, 1, 3)
    ex("wrap-boundary", (5, 6), 16, 2, 3)                    # 5 + 11 == 16: the last legal batch
    ex("wrap-one-cloud-boundary", (32,), 64, 1, 1)           # 32 + 32 == 64
    ex("wrap-refused-5-5", (5, 5), 16, 2, 3, refuse="IndexError")         # 5 + 10 < 16: the first illegal one
    ex("wrap-refused-1-12", (1, 12), 16, 2, 3, refuse="IndexError")
    ex("wrap-refused-10", (10,), 64, 1, 8, refuse="IndexError")
    ex("wrap-refused-300x1", (1,) * 300, 1000, 1, 1, refuse="IndexError")  # the torch path's refusal
    # ---- region arithmetic
    ex("regions-integer", (300, 150, 450, 7), 32, 1, 8, ("table", INT_ETA, INT_PHI))
    ex("regions-recip", (49, 98, 150, 343), 16, 2, 3, ("table", (7, 7, 15, 49, 7, 10), (7, 49, 7, 7, 15, 7)))
    ex("regions-thirds", (211, 97, 350), 32, 3, 8, ("draw", 150))
    ex("regions-over-cloud", (7, 12, 30), 8, 2, 3, ("table", (50, 13, 31), (40, 50, 12)))
    ex("regions-below-2", (40, 33), 8, 3, 3, ("table", (1, 1.5, 2, 1 / 3, 1.6666666), (1.3333334, 1, 3, 1, 1)))
    ex("regions-nine-tables", (120, 77), 16, 9, 3, ("draw", 30))
    ex("regions-nine-tables-h8", (90, 61, 5), 16, 9, 8, ("draw", 150))
    # ---- ties
    ex("ties-eta", (200, 130), 32, 2, 3, coords=("grid", (0,), 0.4))
    ex("ties-phi", (90, 260), 32, 2, 3, coords=("grid", (1,), 0.4))
    ex("ties-both", (150, 150, 40), 32, 3, 8, coords=("grid", (0, 1), 0.2))
    ex("ties-negzero", (80, 50), 16, 2, 3, coords="negzero")
    ex("ties-identical-cloud", (60, 25, 70), 16, 2, 3, coords=("identical", 1))
    # ---- code width: 3 clouds (2 bits) x 1500 x 1500 regions (11 + 11 bits) = 24 bits, k = 0, 3 << 22 < 2^24;
    # a fourth cloud is the first table beyond the guard
    ex("key-k0", (1500, 40, 9), 16, 1, 1, ("table", (1500,), (1500,)))
    ex("key-guard-refused", (1500, 40, 9, 5), 16, 1, 1, ("table", (1500,), (1500,)), refuse="ValueError")
    ex("key-sh-pos", _many(254, 4, 10), 8, 1, 3, ("table", (5,), (5,)))     # 8 + 6 code bits, > 2048 points: sh > 0
    # ---- cloud count and the batch vector's type
    ex("clouds-1", (333,), 32, 2, 3, batch="i32")
    ex("clouds-2", (17, 40), 8, 2, 3, batch="i32")
    ex("clouds-254", _many(254), 8, 1, 3)
    ex("clouds-255", _many(255), 8, 2, 3)
    ex("clouds-255-i32", _many(255), 8, 1, 8, batch="i32")
    ex("clouds-256", _many(256), 8, 2, 3)
    ex("clouds-256-i32", _many(256), 8, 1, 1, batch="i32")
    ex("clouds-300", _many(300), 8, 1, 8)
    ex("clouds-300-i32", _many(300), 16, 2, 3, batch="i32")
    # ---- sort paths: the ragged per-cloud argsort (longest cloud) and the bounded code sort (n_raw) around 6144
    ex("sort-cloud-6144", (6144,), 128, 1, 3)
    ex("sort-cloud-6145", (6145,), 128, 1, 3)
    ex("sort-nraw-6144", (6100, 44), 100, 1, 3)
    ex("sort-nraw-6145", (6100, 45), 100, 1, 3)
    # ---- input dtype and views
    ex("coords-f64", (140, 75), 16, 2, 3, dtype="f64")
    ex("coords-bf16", (120, 60), 16, 2, 3, dtype="bf16")
    ex("coords-f16", (120, 60), 16, 2, 3, dtype="f16")
    ex("coords-strided", (100, 45), 16, 2, 8, view="strided")
    ex("regions-view", (100, 45), 16, 3, 3, view="regions-view")
    ex("coords-f64-strided", (33, 90), 8, 1, 3, dtype="f64", view="strided")

    # ---- the src variant: one cloud, padded once at its end
    for b in (8, 100, 128):
        for raw in (1, b - 1, b, b + 1, 2 * b):
            src(f"src-b{b}-raw{raw}", raw, b, 2, 3)
    src("src-n6144", 6144, 128, 1, 3)
    src("src-n6272", 6145, 128, 1, 3)
    src("src-n6144-padded", 6101, 128, 1, 8)
    src("src-ties-eta", 300, 64, 2, 3, coords=("grid", (0,), 0.4))
    src("src-ties-both", 250, 100, 2, 3, coords=("grid", (0, 1), 0.2))
    src("src-negzero", 90, 16, 2, 3, coords="negzero")
    src("src-real-inf", 120, 50, 2, 3, coords="inf")
    src("src-real-inf-no-pads", 128, 64, 1, 3, coords="inf")
    src("src-f1", 77, 8, 1, 3, F=1)
    src("src-f24", 200, 128, 3, 8, F=24)
    src("src-f24-big", 3000, 128, 1, 1, F=24)
    src("src-x-bf16", 77, 8, 2, 3, x="bf16")
    src("src-x-grad", 77, 8, 2, 3, x="grad")
    src("src-regions-integer", 300, 100, 1, 8, ("table", INT_ETA, INT_PHI))
    src("src-regions-recip", 49, 7, 2, 3, ("table", (7, 7, 49, 15, 7, 10), (7, 49, 7, 7, 15, 7)))
    src("src-regions-thirds", 411, 100, 3, 8, ("draw", 150))
    src("src-regions-over-cloud", 11, 8, 2, 3, ("table", (50, 17, 31), (40, 50, 16)))
    src("src-regions-below-2", 40, 8, 3, 3, ("table", (1, 1.5, 2, 1 / 3, 1.6666666), (1.3333334, 1, 3, 1, 1)))
    src("src-nine-tables", 130, 16, 9, 3, ("draw", 30))
    return out


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
EXAMPLE = [c for c in CASES if c.path == "example"]
SRC = [c for c in CASES if c.path == "src"]
REFUSED = [c for c in EXAMPLE if c.a.refuse]
RUNS = [c for c in CASES if c.path == "src" or not c.a.refuse]


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
_DT = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}


def _regions(spec, t, h, g):
    from hept_amd.prep import get_regions

    if spec[0] == "draw":
        return get_regions(spec[1], t, h, generator=g)
    _, eta, phi = spec
    r = torch.empty(t, 2, h)
    for i in range(t):
        for j in range(h):
            r[i, 0, j] = eta[(i * h + j) % len(eta)]
            r[i, 1, j] = phi[(i * h + j) % len(phi)]
    return r


def _coords(spec, starts, n, c_dim, dtype, g):
    """(n, c_dim) coordinates of clouds starting at ``starts`` (the last entry is n)."""
    wide = torch.randn(n, c_dim, generator=g, dtype=torch.float64 if dtype == torch.float64 else torch.float32)
    kind = spec if isinstance(spec, str) else spec[0]
    if kind == "grid":            # a fraction of the points snapped to a grid of 1/4: groups of equal values
        _, axes, frac = spec
        for a in axes:
            sel = torch.rand(n, generator=g) < frac
            wide[sel, a] = (wide[sel, a] * 4).round() / 4
    elif kind == "negzero":       # every ninth point at -0.0 (eta) / every eleventh at +0.0, and the other way in phi
        wide[0::9, 0], wide[3::11, 0] = -0.0, 0.0
        wide[1::11, 1], wide[2::9, 1] = 0.0, -0.0
    elif kind == "identical":     # every point of one cloud is the same point
        s, e = starts[spec[1]], starts[spec[1] + 1]
        wide[s:e] = wide[s]
    elif kind == "inf":           # one real eta and another point's phi at +inf: they sort before the padding's +inf
        wide[n // 3, 0] = float("inf")
        wide[n // 2, 1] = float("inf")
    else:
        assert kind == "randn", spec
    return wide.to(dtype)


def build(case):
    """The seeded inputs of a case (CPU tensors), as the caller would hold them."""
    g = torch.Generator().manual_seed(case.seed)
    a = case.a
    if case.path == "src":
        regions = _regions(a.regions, a.T, a.H, g)
        coords = _coords(a.coords, (0, a.raw), a.raw, 4, torch.float32, g)
        x = torch.randn(a.raw, a.F, generator=g)
        if a.x == "bf16":
            x = x.to(torch.bfloat16)
        return dict(x=x, coords=coords, regions=regions, B=a.B, T=a.T, H=a.H, raw=a.raw)
    sizes = torch.tensor(a.sizes)
    n = int(sizes.sum())
    starts = [0] + sizes.cumsum(0).tolist()
    regions = _regions(a.regions, a.T, a.H, g)
    dtype = _DT[a.dtype]
    if a.view == "strided":       # columns 1, 3, 5 of a six-column tensor
        coords = _coords(a.coords, starts, n, 6, dtype, g)[:, 1::2]
        assert not coords.is_contiguous()
    else:
        coords = _coords(a.coords, starts, n, 3, dtype, g)
    if a.view == "regions-view":  # every second head of a table twice as wide
        wide = torch.randn(a.T, 2, 2 * a.H, generator=g)
        wide[..., ::2] = regions
        regions = wide[..., ::2]
        assert not regions.is_contiguous()
    batch = torch.repeat_interleave(torch.arange(len(a.sizes)), sizes).to(torch.int32 if a.batch == "i32" else torch.int64)
    return dict(x=torch.arange(n), coords=coords, batch=batch, regions=regions, B=a.B, T=a.T, H=a.H, sizes=sizes,
                n_raw=n, starts=starts)


def _digest(t):
    """First 8 bytes of SHA-256 of a tensor's bytes (contiguous, little-endian as stored)."""
    raw = t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    return int.from_bytes(hashlib.sha256(raw).digest()[:8], "little")


def input_checksum(inp):
    parts = [inp["coords"], inp["regions"].float()] + ([inp["batch"].long()] if "batch" in inp else [inp["x"].float()])
    return np.array([_digest(p) for p in parts], dtype=np.uint64)


def row_digests(rows):
    """(R, n) -> (R,) uint64; int64 rows for the codes, float32 rows for the src region ids."""
    return np.array([_digest(r) for r in rows], dtype=np.uint64)


def unique_mask(inp):
    """Real points whose eta and whose phi are unique in their cloud (-0.0 equals +0.0; the src cloud includes its +inf
    padding).  Their ranks, hence their codes, do not depend on how ties are broken."""
    coords = inp["coords"].double()
    if "batch" in inp:
        bounds, n_pad = inp["starts"], 0
    else:
        bounds, n_pad = [0, inp["raw"]], (-inp["raw"]) % inp["B"]
    mask = torch.ones(coords.shape[0], dtype=torch.bool)
    for s, e in zip(bounds[:-1], bounds[1:]):
        for axis in (0, 1):
            v = coords[s:e, axis]
            if n_pad:
                v = torch.cat([v, torch.full((n_pad,), float("inf"), dtype=v.dtype)])
            val, idx = torch.sort(v)
            dup = torch.zeros(len(v), dtype=torch.bool)
            same = val[1:] == val[:-1]
            dup[idx[1:][same]] = True
            dup[idx[:-1][same]] = True
            mask[s:e] &= ~dup[: e - s]
    return mask


# ---------------------------------------------------------------------------------------------------------------------
# the branches a case takes
# ---------------------------------------------------------------------------------------------------------------------
def _f32(v):
    return np.float32(v)


def width_recip(n, r):
    """region_of's width (csrc/prepare.hip; hept_amd/prep.py quantile_partition): ceil of float32 (1 / r) * n."""
    return int(np.ceil((_f32(1.0) / _f32(r)) * _f32(n)))


def width_true(n, r):
    """The width a true float32 division would give."""
    return int(np.ceil(_f32(n) / _f32(r)))


def region_max(n, r):
    return (n - 1) // width_recip(n, r) + 1


def key_shifts(sizes, regions):
    """code_sort_key's (code_bits, k, sh) for a batch (csrc/prepare.hip), from row 0 = (table 0, head 0)."""
    n_clouds, n_raw = len(sizes), sum(sizes)
    eta = max(region_max(n, float(regions[0, 0, 0])) for n in sizes)
    phi = max(region_max(n, float(regions[0, 1, 0])) for n in sizes)
    packed = (phi << eta.bit_length()) | eta
    code_bits = (n_clouds - 1).bit_length() + packed.bit_length()
    k = max(KEY_BITS - code_bits, 0)
    sh = max((n_raw - 1).bit_length() - k, 0)
    return code_bits, k, sh


def guard_refuses(n_clouds, regions):
    """hept_amd/prep.py: (n_clouds << bits) >= 2^24 with bits from the largest region count per axis."""
    import math

    bits = sum((int(math.ceil(float(regions[:, a].max()))) + 1).bit_length() for a in (0, 1))
    return (n_clouds << bits) >= (1 << KEY_BITS)


def _region_cells(spec, regions, sizes):
    out = {"regions-draw" if spec[0] == "draw" else "regions-table"}
    vals = [float(v) for v in regions.reshape(-1)]
    if all(v == int(v) for v in vals):
        out.add("regions-integer")
    if any(v != int(v) and abs(v * 3 - round(v * 3)) < 1e-4 for v in vals):
        out.add("regions-thirds")
    if any(v < 2 for v in vals):
        out.add("regions-below-2")
    for n in set(sizes):
        for v in set(vals):
            if v > n:
                out.add("regions-over-cloud")           # width 1: region id = rank + 1
            if v == int(v) and v >= 2 and n % int(v) == 0:
                out.add("width-exact-multiple")
            if width_recip(n, v) != width_true(n, v):
                out.add("width-recip-differs")          # true division would give another width
    return out


def cells(case):
    a = case.a
    inp_regions = _regions(a.regions, a.T, a.H, torch.Generator().manual_seed(case.seed))
    out = {case.path, f"T{a.T}", f"H{a.H}"}
    kind = a.coords if isinstance(a.coords, str) else a.coords[0]
    if kind == "grid":
        out.add("ties-" + {(0,): "eta", (1,): "phi", (0, 1): "both"}[a.coords[1]])
    elif kind != "randn":
        out.add({"negzero": "ties-negzero", "identical": "ties-identical-cloud", "inf": "real-inf"}[kind])
    if case.path == "src":
        n = a.raw + (-a.raw) % a.B
        out |= _region_cells(a.regions, inp_regions, [n])
        out |= {f"src-B{a.B}", f"src-F{a.F}", f"src-x-{a.x}", "src-x-kernel-pad" if a.x == "f32" else "src-x-torch-pad",
                "src-sort-small" if n <= SMALL_CAP else "src-sort-large", "src-padded" if n > a.raw else "src-no-pads"}
        for name, v in (("1", 1), ("B-1", a.B - 1), ("B", a.B), ("B+1", a.B + 1), ("2B", 2 * a.B)):
            if a.raw == v:
                out.add(f"src-raw-{name}")
        if n in (6144, 6272):
            out.add(f"src-N{n}")
        return out
    sizes, b = list(a.sizes), a.B
    n_clouds, n_raw, longest = len(sizes), sum(sizes), max(sizes)
    out |= _region_cells(a.regions, inp_regions, sizes)
    # cloud sizes against the block
    for name, v in (("eqB", b), ("B+1", b + 1), ("B-1", b - 1)):
        if v in sizes and b > 1:
            out.add(f"size-{name}")
    if all(s % b == 0 for s in sizes):
        out.add("no-pads")
    if b == 1:
        out.add("block-1")
    if 1 in sizes and b > 1:
        out.add("one-point-cloud")
    if n_clouds >= 40 and all(s < b for s in sizes):
        out.add("every-cloud-below-B")
    # the wrap: pad slot positions raw_end - B + j, negative ones wrap once (pad_gather_kernel)
    ends = np.cumsum(sizes)
    for i, (s, e) in enumerate(zip(sizes, ends)):
        if s % b and e - b < 0:
            out.add("wrap-first-cloud" if i == 0 else "wrap-later-cloud")
            if n_clouds > 1 and e - b + n_raw >= ends[-2]:
                out.add("wrap-into-last-cloud")
    if sizes[0] % b and sizes[0] + n_raw == b:
        out.add("wrap-boundary")
    if sizes[0] + n_raw < b:
        out.add("wrap-refused")
        out.add("wrap-refused-by-entry" if 2 * n_raw - (n_clouds - 1) < b else "wrap-refused-by-caller-only")
    # the sort key of the pad sort
    code_bits, k, sh = key_shifts(sizes, inp_regions)
    out |= {"key-k0" if k == 0 else "key-k-pos", "key-sh0" if sh == 0 else "key-sh-pos"}
    if code_bits == KEY_BITS:
        out.add("key-24-bits")
    if guard_refuses(n_clouds, inp_regions):
        out.add("guard-refused")
    # cloud count, batch type
    if n_clouds in (1, 2, 254, 255, 256, 300):
        out.add(f"clouds-{n_clouds}")
    out |= {"probe-path" if n_clouds <= PROBE_CLOUDS else "torch-path", f"batch-{a.batch}"}
    # sort paths
    out |= {"argsort-one-workgroup" if longest <= SMALL_CAP else "argsort-two-launch",
            "codesort-one-workgroup" if n_raw <= SMALL_CAP else "codesort-two-launch"}
    if longest in (SMALL_CAP, SMALL_CAP + 1):
        out.add(f"longest-{longest}")
    if n_raw in (SMALL_CAP, SMALL_CAP + 1):
        out.add(f"n_raw-{n_raw}")
    out |= {f"coords-{a.dtype}", f"view-{a.view}"}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# mirror, anchors
# ---------------------------------------------------------------------------------------------------------------------
def mirror(case, inp=None):
    """The host mirror's outputs on the CPU (the specification the HIP path is held to)."""
    from hept_amd.prep import prepare_input, prepare_input_src

    inp = inp or build(case)
    if case.path == "src":
        return prepare_input_src(inp["x"], inp["coords"], {"block_size": inp["B"], "regions": inp["regions"]})
    helper = {"block_size": inp["B"], "num_heads": inp["H"], "regions": inp["regions"]}
    return prepare_input(inp["x"], inp["coords"], inp["batch"].long(), helper)


def window_codes(code00, sizes, b):
    """Per pad slot, in slot order, the (table 0, head 0) code the reference's window defines: the code at sorted
    position raw_end[i] - B + j of the ascending codes (negative positions wrap once).  The sorted VALUES do not depend
    on how equal codes are ordered."""
    ordered = torch.sort(code00).values
    out = []
    end = 0
    for s in sizes:
        end += s
        pads = (-s) % b
        pos = end - b + torch.arange(pads)
        out.append(ordered[pos])          # torch indexing: the reference's own wrap (IndexError beyond it)
    return torch.cat(out) if out else code00[:0]


def anchors_example(inp, codes, pad_seq, unpad):
    """What is stored of one run of prepare_input (the reference's at fixture time, the mirror's at test time): codes
    (T, H, n_pad), pad_seq, unpad as returned."""
    mask = unique_mask(inp)
    real = codes[..., unpad].reshape(-1, inp["n_raw"])
    sel = real[:, mask]
    pads = codes[0, 0][~unpad]
    # sorted per cloud: the reference's choice among equal codes is arbitrary, and so is the slot it puts them in
    per_cloud, at = [], 0
    for s in inp["sizes"].tolist():
        k = (-s) % inp["B"]
        per_cloud.append(torch.sort(pads[at:at + k]).values)
        at += k
    return {"digest": row_digests(sel), "row_sum": sel.sum(-1).numpy(), "row_max": sel.amax(-1).numpy() if sel.shape[1]
            else np.zeros(sel.shape[0], np.int64), "unpad": np.packbits(unpad.numpy()),
            "pad_codes": torch.cat(per_cloud).numpy().astype(np.int32) if per_cloud else np.zeros(0, np.int32),
            "mask": np.packbits(mask.numpy()), "row00": row_digests(real[:1]), "real_first": np.array(
                [bool(torch.equal(pad_seq[unpad], torch.arange(inp["n_raw"])))])}


def anchors_src(inp, eta, phi):
    mask = unique_mask(inp)
    rows = torch.cat([eta, phi])[:, : inp["raw"]].float()
    sel = rows[:, mask]
    return {"digest": row_digests(sel), "row_sum": sel.double().sum(-1).numpy(),
            "row_max": sel.amax(-1).numpy() if sel.shape[1] else np.zeros(sel.shape[0], np.float32),
            "mask": np.packbits(mask.numpy())}


def save_golden(path, records):
    """records: "<case id>/<key>" -> 1-D array.  Stored per (path, key) as one concatenated array with the ids and the
    lengths beside it: hundreds of tiny archive members would cost more than their contents."""
    groups = {}
    for name, arr in records.items():
        cid, key = name.split("/")
        groups.setdefault(f"{BY_ID[cid].path}.{key}", []).append((cid, np.atleast_1d(arr)))
    stored = {}
    for group, items in groups.items():
        stored[group] = np.concatenate([arr for _, arr in items])
        stored[group + ".ids"] = np.array([cid for cid, _ in items])
        stored[group + ".len"] = np.array([len(arr) for _, arr in items], dtype=np.int32)
    np.savez_compressed(path, **stored)


def load_golden():
    """"<case id>/<key>" -> array, as save_golden was given them."""
    out = {}
    with np.load(GOLDEN) as z:
        for group in z.files:
            if group.endswith((".ids", ".len")):
                continue
            key, at = group.split(".", 1)[1], 0
            flat = z[group]
            for cid, n in zip(z[group + ".ids"], z[group + ".len"]):
                out[f"{cid}/{key}"] = flat[at:at + n]
                at += n
    return out


def check_anchors(case, golden):
    """CPU: the generator reproduces the stored inputs and the mirror the stored reference anchors (tie-aware)."""
    inp = build(case)
    pre = case.id + "/"
    assert np.array_equal(input_checksum(inp), golden[pre + "input"]), f"{case.id}: the generator drifted"
    mask = unique_mask(inp)
    assert np.array_equal(np.packbits(mask.numpy()), golden[pre + "mask"]), case.id
    out = mirror(case, inp)
    if case.path == "src":
        x_p, kw = out
        mine = anchors_src(inp, *kw["region_indices"])
        keys = ("digest", "row_sum", "row_max")
    else:
        _, kw, unpad = out
        mine = anchors_example(inp, kw["combined_shifts"], out[0], unpad)     # x = arange(n_raw): x[pad_seq] is pad_seq
        keys = ("digest", "row_sum", "row_max", "unpad", "real_first")
        # pad slots: the same multiset of (table 0, head 0) codes per cloud.  Where coordinate ties made the reference
        # give tied points other codes than the mirror (row 0 differs on some real point), the multisets may differ
        # legitimately: then only their sizes are compared
        if np.array_equal(mine["row00"], golden[pre + "row00"]):
            keys += ("pad_codes",)
        else:
            assert not bool(mask.all()), f"{case.id}: tie-free, yet row 0 differs from the reference"
            assert mine["pad_codes"].shape == golden[pre + "pad_codes"].shape, case.id
    for key in keys:
        assert np.array_equal(mine[key], golden[pre + key]), f"{case.id}: {key} differs from the reference's"
    return mask


# ---------------------------------------------------------------------------------------------------------------------
# GPU checks
# ---------------------------------------------------------------------------------------------------------------------
def _to(inp, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) and k != "sizes" else v) for k, v in inp.items()}


def _same(a, b, what, cid):
    assert a.dtype == b.dtype and a.shape == b.shape, f"{cid}: {what} is {a.dtype} {tuple(a.shape)}, want {b.dtype} {tuple(b.shape)}"
    # bit for bit: equal as integers of the same width (-0.0 is not +0.0, and a NaN would equal itself)
    ia, ib = (t.contiguous().reshape(-1).view(torch.uint8) for t in (a, b))
    assert torch.equal(ia, ib), f"{cid}: {what} differs from the host mirror in {int((ia != ib).sum())} bytes"


def gpu_example(case, dev):
    from hept_amd.prep import prepare_input_hip

    inp = build(case)
    a = case.a
    want_x, want_kw, want_mask = mirror(case, inp)
    gin = _to(inp, dev)
    if a.view == "strided":       # the device copy keeps the view
        gin["coords"] = _coords_view(inp, dev)
    if a.view == "regions-view":
        wide = torch.zeros(a.T, 2, 2 * a.H, device=dev)
        wide[..., ::2] = inp["regions"].to(dev)
        gin["regions"] = wide[..., ::2]
    assert gin["coords"].is_contiguous() == (a.view != "strided") and gin["regions"].is_contiguous() == (a.view != "regions-view")
    keep = {k: gin[k].clone() for k in ("x", "coords", "batch", "regions")}
    helper = {"block_size": inp["B"], "num_heads": inp["H"], "regions": gin["regions"]}
    runs = [prepare_input_hip(gin["x"], gin["coords"], gin["batch"], helper) for _ in range(2)]
    torch.cuda.synchronize()
    n_raw, n_pad = inp["n_raw"], int(want_mask.numel())
    for x_p, kw, mask in runs:
        got = dict(pad_seq=x_p.cpu(), mask=mask.cpu(), codes=kw["combined_shifts"].cpu(), coords=kw["coords"].cpu())
        # documented dtypes and shapes
        assert got["pad_seq"].dtype == torch.int64 and got["pad_seq"].shape == (n_pad,), case.id
        assert got["mask"].dtype == torch.bool and got["mask"].shape == (n_pad,), case.id
        assert got["codes"].dtype == torch.int64 and got["codes"].shape == (a.T, a.H, n_pad), case.id
        assert got["coords"].dtype == inp["coords"].dtype and got["coords"].shape == (n_pad, inp["coords"].shape[1]), case.id
        assert n_pad % inp["B"] == 0 and set(kw) == {"combined_shifts", "coords"}, case.id
        # bit for bit against the mirror
        _same(got["pad_seq"], want_x, "pad_seq", case.id)
        _same(got["mask"], want_mask, "the un-pad mask", case.id)
        _same(got["codes"], want_kw["combined_shifts"], "combined_shifts", case.id)
        _same(got["coords"], want_kw["coords"], "coords", case.id)
        # invariants that need no mirror
        assert torch.equal(got["pad_seq"][got["mask"]], torch.arange(n_raw)), f"{case.id}: real slots out of order"
        _same(got["coords"], inp["coords"][got["pad_seq"]], "coords against coords[pad_seq]", case.id)
        assert torch.equal(got["codes"][..., ~got["mask"]], got["codes"][..., got["mask"]][..., got["pad_seq"][~got["mask"]]]), \
            f"{case.id}: a pad slot's codes are not those of the point it copies"
        code00 = got["codes"][0, 0][got["mask"]]
        assert torch.equal(got["codes"][0, 0][~got["mask"]], window_codes(code00, list(a.sizes), inp["B"])), \
            f"{case.id}: a pad slot lies outside the window the reference defines"
        per_cloud = got["mask"].reshape(-1, inp["B"]).sum(-1)
        assert int(per_cloud.sum()) == n_raw, case.id
    for name, t in keep.items():
        _same(gin[name], t, f"the input {name} after the call", case.id)


def _coords_view(inp, dev):
    wide = torch.zeros(inp["n_raw"], 6, device=dev, dtype=inp["coords"].dtype)
    wide[:, 1::2] = inp["coords"].to(dev)
    return wide[:, 1::2]


def gpu_src(case, dev):
    from hept_amd.prep import prepare_input_src_hip

    inp = build(case)
    a = case.a
    want_x, want_kw = mirror(case, inp)
    x = inp["x"].to(dev)
    if a.x == "grad":
        x.requires_grad_(True)
    coords, regions = inp["coords"].to(dev), inp["regions"].to(dev)
    keep = (x.detach().clone(), coords.clone(), regions.clone())
    n = a.raw + (-a.raw) % a.B
    th = a.T * a.H
    for _ in range(2):
        x_p, kw = prepare_input_src_hip(x, coords, a.B, regions)
        torch.cuda.synchronize()
        assert set(kw) == {"raw_size", "coords", "region_indices", "regions_h"} and kw["raw_size"] == a.raw, case.id
        assert x_p.shape == (n, a.F) and x_p.dtype == inp["x"].dtype and kw["coords"].shape == (n, 4), case.id
        assert len(kw["region_indices"]) == 2 and all(r.shape == (th, n) and r.dtype == torch.float32
                                                      for r in kw["region_indices"]), case.id
        assert kw["regions_h"].shape == (2, th), case.id
        _same(x_p.detach().cpu(), want_x, "x_pad", case.id)
        _same(kw["coords"].cpu(), want_kw["coords"], "coords", case.id)
        _same(kw["region_indices"][0].cpu(), want_kw["region_indices"][0], "region_indices[eta]", case.id)
        _same(kw["region_indices"][1].cpu(), want_kw["region_indices"][1], "region_indices[phi]", case.id)
        _same(kw["regions_h"].cpu(), want_kw["regions_h"], "regions_h", case.id)
        # invariants: real rows first and unchanged, zero rows behind them; every row of ids is a rank partition
        assert torch.equal(x_p.detach()[: a.raw], x.detach()) and float(x_p.detach()[a.raw:].float().abs().sum()) == 0.0, case.id
        assert float(kw["coords"][a.raw:].abs().sum()) == 0.0, case.id
        for axis in (0, 1):
            ids = kw["region_indices"][axis].cpu()
            order = torch.sort(torch.cat([inp["coords"][:, axis], torch.full((n - a.raw,), float("inf"))]), stable=True).indices
            assert bool((ids[:, order][:, 1:] >= ids[:, order][:, :-1]).all()) and float(ids.min()) == 1.0, \
                f"{case.id}: region ids are not monotone in the coordinate"
        if a.x == "grad":     # the torch padding path keeps the caller's tensor in the graph
            assert x_p.requires_grad
            (g,) = torch.autograd.grad(x_p.sum(), x)
            assert torch.equal(g, torch.ones_like(g)), case.id
    for got, t, name in zip((x.detach(), coords, regions), keep, ("x", "coords", "regions")):
        _same(got, t, f"the input {name} after the call", case.id)


def gpu_refused(case, dev, monkeypatch):
    """The front end raises what the reference raises (IndexError) or the pad sort's own limit (ValueError), before
    any output is allocated and before hept_prepare_input is launched."""
    import pytest
    from hept_amd import prep

    inp = build(case)
    gin = _to(inp, dev)
    helper = {"block_size": inp["B"], "num_heads": inp["H"], "regions": gin["regions"]}
    reached = []
    monkeypatch.setattr(prep, "_prepare_outputs", lambda *args, **kw: reached.append(1))
    err = {"IndexError": IndexError, "ValueError": ValueError}[case.a.refuse]
    with pytest.raises(err, match="first cloud" if err is IndexError else r"2\^24"):
        prep.prepare_input_hip(gin["x"], gin["coords"], gin["batch"], helper)
    torch.cuda.synchronize()
    assert not reached, f"{case.id}: the outputs were allocated for a refused batch"
