"""The rows sweep: every instantiation of the row builder (csrc/prep_hash.hip: 108 tuned prep_hash_kernel instantiations,
9 of prep_generic_kernel) on inputs whose float32 results are exact in any order, every output bit for bit against a
float64 evaluation of the oracle's stages; run by tests/test_gpu_rows_sweep.py, the coverage and the exactness of every
cell's inputs pinned on the CPU by tests/test_rows_sweep_cells.py.  A plain module, not a conftest.  Nothing here touches
the GPU at import time.

The exact design.  q, k, v and the coordinates are multiples of 1/8 in [-4, 4]; ``sqrt_w`` is passed directly (the staged
entry has K = 0) and holds powers of two 2^j, j in -2..2, drawn per (head, column); ``alpha`` holds integers in -7..7
drawn per (head, e, table) -- the columns of any two (head, table) pairs differ, so a wrong table slot, a wrong ``t0``
offset or a wrong head changes the hash.  Then

    rows          products of at most 6 bits: exact in float32, bf16 and fp16
    projections   at most 30 terms of |.| <= 112 on a 2^-5 grid: 17 bits
    norms         at most 30 squares of |.| <= 256 on a 2^-10 grid: 23 bits
    keys          proj + code * span, codes <= 15 (src variant: phi * cfac + eta <= 15): within 24 bits

so the kernel's fmaf chains, its LDS atomics and any reordering give the bits of the float64 evaluation.
``prove_exact`` repeats that proof on the CPU for the actual inputs of a cell (shuffled float32 accumulation orders against
float64, representability in every tile and input type, the keys of the sort).

The float64 reference is oracle/hept_oracle.py evaluated in float64: ``augment_qk``, ``e2lsh_project``, ``hash_range``,
``shifted_keys`` / ``geo_shift`` and ``sort_keys``, composed as ``forward_partials`` composes them (the zero fill of the
rows at and after ``raw_size``, their +inf hashes).  ``forward_partials`` itself derives ``sqrt_w`` from ``w_rpe.weight``
through an exp that no float32 input makes an exact power of two, and asks for N to be a multiple of the block size; the
stage functions take ``sqrt_w`` as it is.  The permutations are held to ``torch.sort(stable=True)`` of the float64 keys
computed on the host from the INPUTS -- nothing of the GPU's own hashes or range partials enters the expected order.

Rows at and after ``raw_size`` hold large finite junk in q, k, v and the coordinates; no result may depend on it.  Every
output buffer is allocated through tests/scratch_sweep.py's guarded, 0xFF-filled buffers (NaN in every float type): a word
that should have been written and was not fails the bit comparison, and a store outside a buffer fails the guard check.

The rounding cells (random float32 inputs with elements planted on rounding ties of the 16-bit row type) hold the stored
16-bit elements to torch's round-to-nearest-even cast bit for bit, the norm word to the norm of the ROUNDED values and the
projections to the UNROUNDED row, at the two a-priori bounds of a 30-term float32 fmaf accumulation, 31 * 2^-24 times the
sum of the terms' magnitudes."""
import zlib
from collections import namedtuple

import torch

Cell = namedtuple("Cell", "id kind H D C N T t0 Tl tile intype raw codes")

TUNED = [(24, 6), (24, 4), (24, 2), (16, 6), (16, 4), (8, 4)]      # H = 8 with these: HEPT_PREP_CASE
GENERIC = [(3, 5, 3), (16, 27, 3), (12, 8, 4), (1, 24, 6)]         # (H, D, C); H = 3, D = 5: a 30-byte 16-bit input row
TILES = ("fp32", "bf16", "mixed16")
INS = ("f32", "bf16", "fp16")
IN_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
QK_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "mixed16": torch.float16}   # q^ / k^ elements; v is bf16 in both 16-bit types
JUNK = {"f32": 1e30, "bf16": 1e30, "fp16": 60000.0}                # large, finite in the input type

PREP_GRID = 1024            # HEPT_PREP_GRID: partial slots of a (table, head); the q role owns the first half
SLOTS = PREP_GRID // 2
POINTS, WAVES = 8, 4        # points per wave iteration, waves per workgroup
WGS3 = 341                  # HEPT_PREP_WGS: workgroups per role of the three-role launch
WGS2 = 512                  # HEPT_PREP_WGS2: of the two-role launch
SMALL_CAP = 6144            # the one-workgroup sort's capacity
N_INST = 77                 # 9 full tiles and one of 5 points: three workgroups, the last with two idle waves
EDGE_N = (1, 7, 8, 9, 31, 32, 33, 10912, 10913, 10920, 10944, 21833)
EDGE_SHAPES = [(8, 24, 6), (8, 16, 4), (16, 27, 3)]                # (24, 6), another tuned pair, a generic shape (16 points per step)
RAW_N = (6100, 6200)        # either side of SMALL_CAP
ROUND_SHAPES = [(8, 24, 6), (3, 5, 3)]
ROUND_N = 203
TL_ROT = {4: (1, 3, 4), 8: (5, 7, 8)}
NORM_BOUND = 31 * 2.0 ** -24    # a 30-term float32 fmaf accumulation: gamma_30 < 31 u, u = 2^-24, times the sum of magnitudes
# two-role launch (one-call forward only): B = 32, T = 2
TWO_ROLE_N = (10912, 10944, 16384, 16416, 32800)
TWO_ROLE_GENERIC = (16416, (16, 24, 6))
TWO_ROLE_PRECISIONS = ("fp32", "bf16", "mixed16")
# the riders' 1.0 at column D (csrc/rows_rider.h), at TWO_ROLE_N[0]: D = 4 is the second quad of piece 0 of a 16-bit row
# half, D = 20 of piece 2; H = 3: the run-time head count, with a trip that runs past the last head.  (D = 28, the last
# piece of an f32 row half, cannot be reached: hept_check_shape refuses D > 27 for every H and C, csrc/capi.hip:284.)
TWO_ROLE_COLUMN_D = ((3, 4, 3), (3, 20, 4))

# file:line references of the rules cells() and prep_wgs() mirror (tests/test_rows_sweep_cells.py checks the text)
REFS = [
    ("hept_amd/csrc/prep_hash.hip", 25, "constexpr int PREP_POINTS = 8;"),
    ("hept_amd/csrc/prep_hash.hip", 225, "tile_i += gridDim.x * WAVES"),
    ("hept_amd/csrc/prep_hash.hip", 303, "const bool is_pad = n >= raw_size;"),
    ("hept_amd/csrc/prep_hash.hip", 313, "ROLE == 0 && codes"),
    ("hept_amd/csrc/prep_hash.hip", 467, "for (int s2 = slot + (int)gridDim.x;"),
    ("hept_amd/csrc/prep_hash.hip", 477, "#define HEPT_PREP_WGS 341"),
    ("hept_amd/csrc/prep_hash.hip", 481, "#define HEPT_PREP_WGS2 512"),
    ("hept_amd/csrc/prep_hash.hip", 496, "if (!even || roles != 2) return cap;"),
    ("hept_amd/csrc/prep_hash.hip", 644, "if (Tl <= 4) HEPT_PREP_IN(TILE, 4);"),
    ("hept_amd/csrc/prep_hash.hip", 688, "const int ppw = PREP_THREADS / H;"),
    ("hept_amd/csrc/prep_hash.hip", 710, "n += gridDim.x * ppw"),
    ("hept_amd/csrc/prep_hash.hip", 801, "const dim3 grid(HEPT_PREP_GRID / 2, roles);"),
    ("hept_amd/csrc/prep_hash.hip", 862, "if (H == 8 && D == DD && C == CC) {"),
    ("hept_amd/csrc/prep_hash.hip", 884, "kvhat, qproj, kproj, minmax, stream, 3, nullptr, 0);"),
    ("hept_amd/_lib.py", 21, "PREP_GRID = 1024"),
]


def _cells():
    out = []

    def add(kind, name, h, d, c, n, tl, tile, intype, raw=None, codes=True, i=0):
        t0 = 1 + i % 2
        out.append(Cell(f"{kind}-{name}-h{h}d{d}c{c}-n{n}-tl{tl}-{tile}-{intype}", kind, h, d, c, n, t0 + tl + 1, t0, tl,
                        tile, intype, n if raw is None else raw, codes))

    # one cell per tuned instantiation; Tl rotates over the TMAX class, Tl == TMAX included
    for pi, (d, c) in enumerate(TUNED):
        for ti, tile in enumerate(TILES):
            for tmax in (4, 8):
                for ii, intype in enumerate(INS):
                    i = pi + ti + ii
                    add("inst", f"tmax{tmax}", 8, d, c, N_INST, TL_ROT[tmax][i % 3], tile, intype, i=i)
    # the generic kernel: every instantiation on every free head shape
    for gi, (h, d, c) in enumerate(GENERIC):
        for ti, tile in enumerate(TILES):
            for ii, intype in enumerate(INS):
                i = gi + ti + ii
                add("inst", "generic", h, d, c, N_INST, (TL_ROT[4] + TL_ROT[8])[i % 6], tile, intype, i=i)
    # boundary sizes: every (tile type, input type) on three head shapes; the table count alternates between the TMAX classes
    for ni, n in enumerate(EDGE_N):
        for h, d, c in EDGE_SHAPES:
            for tile in TILES:
                for intype in INS:
                    add("edge", "n", h, d, c, n, 2 if ni % 2 == 0 else 5, tile, intype, i=ni)
    # the src rule: rows at and after raw_size are padding, no AND codes, then sort_tables_src
    for ni, n in enumerate(RAW_N):
        for raw in (n, n - 1, n - 37, 6000, 0):
            for h, d, c in EDGE_SHAPES:
                for tile in TILES:
                    for intype in INS:
                        add("raw", f"raw{raw}", h, d, c, n, 2, tile, intype, raw=raw, codes=False, i=ni)
    # the code bound is only a scale: one cell per sort path, with codes
    for ni, n in enumerate(RAW_N):
        add("bound", "cmax", 8, 24, 6, n, 2, "fp32", "f32", i=ni)
    return out


def _round_cells():
    out = []
    for h, d, c in ROUND_SHAPES:
        for tile in ("bf16", "mixed16"):
            for intype in INS:
                out.append(Cell(f"round-h{h}d{d}c{c}-n{ROUND_N}-{tile}-{intype}", "round", h, d, c, ROUND_N, 4, 1, 2, tile,
                                intype, ROUND_N, True))
    return out


CELLS = _cells()
ROUND_CELLS = _round_cells()
BY_ID = {c.id: c for c in CELLS + ROUND_CELLS}
BOUND_CELLS = [c for c in CELLS if c.kind == "bound"]
# without codes the bound column is 0: the first cell of either TMAX class and of the generic kernel, run with codes=None
CODES_NONE_CELLS = [next(c for c in CELLS if c.id.startswith(f"inst-{name}")) for name in ("tmax4", "tmax8", "generic")]


def tuned(cell):
    return cell.H == 8 and (cell.D, cell.C) in TUNED                      # prep_hash.hip:862


def prep_wgs(n, roles=3):
    """Workgroups per role of the tuned launch (prep_hash.hip:485-499, default environment)."""
    tiles = -(-n // POINTS)
    want, cap = -(-tiles // WAVES), WGS2 if roles == 2 else WGS3
    if want <= cap:
        return max(want, 1)
    if roles != 2:
        return cap
    trips = -(-tiles // (cap * WAVES))
    return -(-tiles // (trips * WAVES))


def instantiation(cell):
    """The kernel instantiation a cell runs, as hept_prep_hash_rpe, launch_prep and launch_prep_generic choose it."""
    if tuned(cell):
        return ("tuned", cell.D, cell.C, cell.tile, 4 if cell.Tl <= 4 else 8, cell.intype)    # prep_hash.hip:644
    return ("generic", cell.tile, cell.intype)


def all_instantiations():
    out = {("tuned", d, c, tile, tmax, i) for d, c in TUNED for tile in TILES for tmax in (4, 8) for i in INS}
    return out | {("generic", tile, i) for tile in TILES for i in INS}


def cells(cell):
    """Names of the branches a cell takes (three-role launch: the staged entry, prep_hash.hip:884)."""
    out = {f"tile:{cell.tile}", f"in:{cell.intype}", "t0>0" if cell.t0 > 0 else "t0=0",
           "codes" if cell.codes else "codes-none",
           "sort-one-workgroup" if cell.N <= SMALL_CAP else "sort-two-launch"}
    if cell.raw < cell.N:
        out.add("pad-rows")
        if cell.raw % POINTS == 0:
            out.add("pad-rows-from-a-tile-boundary")
        if cell.raw == 0:
            out.add("pad-rows-only")
    if tuned(cell):
        tmax = 4 if cell.Tl <= 4 else 8
        tiles, wgs = -(-cell.N // POINTS), prep_wgs(cell.N)
        out |= {"tuned", f"tmax{tmax}"}
        if cell.Tl == tmax:
            out.add("tl==tmax")
        if cell.N % POINTS:
            out.add("ragged-last-tile")                                    # rows < PREP_POINTS
        if tiles < wgs * WAVES:
            out.add("idle-wave")                                           # a wave whose tile loop runs zero times
        if tiles > wgs * WAVES:
            out.add("grid-stride")                                         # prep_hash.hip:225
            if tiles % (wgs * WAVES):
                out.add("grid-stride-ragged-trip")
        if wgs < SLOTS:
            out.add("spare-slot-fill")                                     # prep_hash.hip:467
        if wgs == WGS3 and -(-tiles // WAVES) > WGS3:
            out.add("wgs-capped")
    else:
        ppw = 256 // cell.H                                                # prep_hash.hip:688
        out.add("generic")
        if 256 % cell.H:
            out.add("generic-idle-threads")                                # slot >= ppw
        if cell.N > SLOTS * ppw:
            out.add("grid-stride")                                         # prep_hash.hip:710
        if cell.N < SLOTS * ppw:
            out.add("generic-empty-workgroup")                             # writes the neutral range itself
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the inputs (CPU)
# ---------------------------------------------------------------------------------------------------------------------
_data = {}


def data_key(cell):
    return (cell.kind == "round", cell.tile if cell.kind == "round" else "", cell.H, cell.D, cell.C, cell.N, cell.T)


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g)


def data(cell):
    """CPU inputs of a cell, float32 (the last data set built is kept: the parametrisation is data-major)."""
    key = data_key(cell)
    if _data.get("key") == key:
        return _data["d"]
    h, d, c, n, t = cell.H, cell.D, cell.C, cell.N, cell.T
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    out = {"sqrt_w": 2.0 ** _ints(g, -2, 2, (h, c)).float()}
    if cell.kind == "round":
        for nm, shape in (("q", (n, h * d)), ("k", (n, h * d)), ("v", (n, h * d)), ("coords", (n, c))):
            out[nm] = _with_ties(torch.randn(shape, generator=g) * 1.5, tie_type(cell, nm), g)
        out["alpha"] = torch.randn(h, d + c, t, generator=g)
    else:
        for nm, shape in (("q", (n, h * d)), ("k", (n, h * d)), ("v", (n, h * d)), ("coords", (n, c))):
            out[nm] = _ints(g, -32, 32, shape).float() / 8
        out["alpha"] = _ints(g, -7, 7, (h, d + c, t)).float()
    # AND codes: the largest code of a (table, head) sits at point 0 and nowhere else (tile 0 is in every sample); it
    # depends on the table (3 dt != 0 mod 8 for a slip of 1..7 tables) and on the head (neighbouring heads differ; heads 8
    # apart cannot: codes stay <= 15)
    maxc = 8 + (3 * torch.arange(t)[:, None] + torch.arange(h)[None, :]) % 8
    codes = _ints(g, 0, 2 ** 30, (t, h, n)) % maxc[..., None]
    codes[..., 0] = maxc
    out["codes"], out["maxc"] = codes, maxc
    # the src variant's region tables: small integers, cfac = ceil(regions_h[0]) + 1 in 2..4, phi * cfac + eta <= 15
    out["eta"] = _ints(g, 0, 3, (t * h, n)).float()
    out["phi"] = _ints(g, 0, 3, (t * h, n)).float()
    out["regions_h"] = torch.stack([_ints(g, 1, 3, (t * h,)).float() - 0.25, torch.ones(t * h)])
    _data.update(key=key, d=out)
    return out


def tie_type(cell, name):
    """The 16-bit type a tensor of a rounding cell is stored in: v rows are bf16 in both 16-bit tile types."""
    return "bf16" if name == "v" else cell.tile


def _with_ties(x, tile, g):
    """Normal, finite values with 2^-6 <= |x| < 8; about 300 elements on rounding ties of the row type (bf16: low 16 bits
    0x8000; fp16: the low 13 bits 0x1000, a half ulp of a normal fp16 value), whatever the bits above hold; a few +-0.0."""
    x = torch.where(x < 0, -1.0, 1.0) * x.abs().clamp(2.0 ** -6, 7.5)
    flat = x.reshape(-1).clone()
    count = min(300, flat.numel() // 3)
    idx = torch.randperm(flat.numel(), generator=g)[:count + 8]
    bits = flat.view(torch.int32)
    low, half = (0xFFFF, 0x8000) if tile == "bf16" else (0x1FFF, 0x1000)
    bits[idx[:count]] = (bits[idx[:count]] & ~low) | half
    flat[idx[count:count + 4]] = -0.0
    flat[idx[count + 4:]] = 0.0
    return flat.reshape(x.shape)


def tie_count(x, tile):
    low, half = (0xFFFF, 0x8000) if tile == "bf16" else (0x1FFF, 0x1000)
    on = (x.contiguous().view(torch.int32) & low) == half
    above = (x.contiguous().view(torch.int32) >> (16 if tile == "bf16" else 13)) & 1
    return int((on & (above == 0)).sum()), int((on & (above == 1)).sum())


def unrounded_rows(cell, d, dtype=torch.float64):
    """q^, k^ (H, N, E) and v (H, N, D) as the kernel forms them before any rounding: the input widened from its own type,
    ``sqrt_w * coords`` one product; computed in ``dtype`` (float32 for the rounding cells: that product is exact)."""
    import hept_oracle as ho

    it = IN_DTYPE[cell.intype]
    q, k, v = (d[x].to(it).to(dtype) for x in ("q", "k", "v"))
    q_hat, k_hat = ho.augment_qk(q, k, d["coords"].to(dtype), d["sqrt_w"].to(dtype))
    v_h = v.reshape(cell.N, cell.H, cell.D).permute(1, 0, 2)
    return q_hat.clone(), k_hat.clone(), v_h.clone()


def reference(cell, d):
    """float64 evaluation of the oracle's stages for tables t0 .. t0 + Tl of the cell."""
    import hept_oracle as ho

    t0, tl, raw = cell.t0, cell.Tl, cell.raw
    q_hat, k_hat, v_h = unrounded_rows(cell, d)
    q_hat[:, raw:] = 0.0                                 # forward_partials: the zero fill of the padding rows
    k_hat[:, raw:] = 0.0
    v_h[:, raw:] = 0.0
    alpha = d["alpha"][:, :, t0:t0 + tl].double()
    qh, kh = ho.e2lsh_project(q_hat, alpha), ho.e2lsh_project(k_hat, alpha)     # padding rows take part with hash 0
    span = ho.hash_range(qh, kh)
    qproj, kproj = qh.clone(), kh.clone()
    qproj[..., raw:] = float("inf")
    kproj[..., raw:] = float("inf")
    if cell.codes:
        q_keys, k_keys = ho.shifted_keys(qproj, kproj, d["codes"][t0:t0 + tl], span)
    else:
        sl = slice(t0 * cell.H, (t0 + tl) * cell.H)
        shift = ho.geo_shift(d["regions_h"][:, sl].double(), span, (d["eta"][sl].double(), d["phi"][sl].double()), tl)
        q_keys, k_keys = qproj + shift, kproj + shift
    return dict(q_hat=q_hat, k_hat=k_hat, v=v_h, qn=-0.5 * (q_hat ** 2).sum(-1), kn=-0.5 * (k_hat ** 2).sum(-1),
                qh=qh, kh=kh, qproj=qproj, kproj=kproj, span=span, q_keys=q_keys, k_keys=k_keys,
                qpos=ho.sort_keys(q_keys), kpos=ho.sort_keys(k_keys))


def _f32_sum(term, order):
    """Sequential float32 sum of term(e) in the given order of e."""
    acc = None
    for e in order:
        acc = term(e) if acc is None else acc + term(e)
    return acc


def proof_key(cell):
    """Cells with the same key share inputs and reference: the proof covers every tile and input type at once."""
    return data_key(cell) + (cell.t0, cell.Tl, cell.raw, cell.codes)


def prove_exact(cell):
    """The premises of the exact design on the cell's actual inputs (whatever its tile and input type: every type is
    checked); returns the figures the CPU test asserts."""
    d = data(cell)
    r = reference(cell._replace(intype="f32"), d)
    g = torch.Generator().manual_seed(11)
    e_dim = cell.D + cell.C
    alpha32 = d["alpha"][:, :, cell.t0:cell.t0 + cell.Tl].permute(2, 0, 1)        # (Tl, H, E)
    orders = [torch.randperm(e_dim, generator=g).tolist() for _ in range(2)] + [list(range(e_dim))]
    ok = {}
    for nm, hat, hashed, norm in (("q", r["q_hat"], r["qh"], r["qn"]), ("k", r["k_hat"], r["kh"], r["kn"])):
        a32 = hat.float()
        ok[nm + "f32"] = torch.equal(a32.double(), hat)

        def prod(e):                                                              # (Tl, H, N) float32 products
            return a32[None, :, :, e] * alpha32[:, :, None, e]

        def square(e):
            return a32[:, :, e] * a32[:, :, e]

        ok[nm + "terms"] = all(torch.equal(prod(e).double(), hat[None, :, :, e] * alpha32[:, :, None, e].double())
                               for e in range(e_dim))
        ok[nm + "proj"] = all(torch.equal(_f32_sum(prod, o).double(), hashed) for o in orders)
        ok[nm + "norm"] = all(torch.equal((-0.5 * _f32_sum(square, o)).double(), norm) for o in orders)
        ok[nm + "tile"] = all(torch.equal(a32.to(dt).float(), a32) for dt in QK_DTYPE.values())
    v32 = r["v"].float()
    ok["vtile"] = torch.equal(v32.to(torch.bfloat16).float(), v32)
    ok["in"] = all(torch.equal(d[x].to(it).float(), d[x]) for x in ("q", "k", "v") for it in IN_DTYPE.values())
    # the keys as the sort forms them in float32, every operation rounded on its own
    span32 = r["span"].float()
    ok["span"] = torch.equal(span32.double(), r["span"])
    if cell.codes:
        offs = d["codes"][cell.t0:cell.t0 + cell.Tl].float() * span32
        keys = (r["qproj"].float() + offs, r["kproj"].float() + offs)
        ok["codes"] = int(d["codes"].max()) <= 15 and int(d["codes"].min()) >= 0
    else:
        sl = slice(cell.t0 * cell.H, (cell.t0 + cell.Tl) * cell.H)
        cf = (torch.ceil(d["regions_h"][0, sl]) + 1).reshape(cell.Tl, cell.H, 1)
        eta, phi = (d[x][sl].reshape(cell.Tl, cell.H, cell.N) for x in ("eta", "phi"))
        shift = (phi * span32) * cf + eta * span32
        keys = (r["qproj"].float() + shift, r["kproj"].float() + shift)
        ok["codes"] = float((phi * cf + eta).max()) <= 15
    ok["keys"] = torch.equal(keys[0].double(), r["q_keys"]) and torch.equal(keys[1].double(), r["k_keys"])
    real = r["q_keys"][..., :cell.raw]
    distinct = min(len(torch.unique(seg)) for seg in real.reshape(-1, cell.raw)) if cell.raw else 0
    cols = d["alpha"].permute(0, 2, 1).reshape(-1, e_dim)                       # one column per (head, table)
    return dict(ok=ok, distinct=distinct, alpha_distinct=len(torch.unique(cols, dim=0)) == cols.shape[0],
                sqrt_w=d["sqrt_w"], max_abs_proj=float(r["qh"].abs().max()), span=r["span"])


# ---------------------------------------------------------------------------------------------------------------------
# GPU checks (imports deferred: the CPU suite imports this module without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
_gpu = {}


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _device_data(cell, dev):
    key = data_key(cell)
    if _gpu.get("dkey") != key:
        _gpu.clear()
        d = data(cell)
        _gpu.update(dkey=key, g={k: v.to(dev) for k, v in d.items()})
    return _gpu["g"]


def _device_reference(cell, dev):
    _device_data(cell, dev)
    key = data_key(cell) + (cell.t0, cell.Tl, cell.raw, cell.codes)
    if _gpu.get("rkey") != key:
        _gpu["rkey"] = key
        _gpu["r"] = {k: v.to(dev) for k, v in reference(cell, data(cell)).items()}
    return _gpu["r"]


def run_builder(cell, dev, codes="cell"):
    """ops.prep_hash on the cell with every output buffer guarded and filled with 0xFF; junk in the padding rows."""
    import scratch_sweep as ss
    from hept_amd import ops

    g = _device_data(cell, dev)
    it = IN_DTYPE[cell.intype]
    q, k, v, coords = g["q"].to(it), g["k"].to(it), g["v"].to(it), g["coords"]
    if cell.raw < cell.N:
        q, k, v, coords = (x.clone() for x in (q, k, v, coords))
        for x in (q, k, v):
            x[cell.raw:] = JUNK[cell.intype]
        coords[cell.raw:] = 1e30
    cd = (g["codes"] if cell.codes else None) if codes == "cell" else codes
    with ss.scratch("ff") as ledger:
        ph = ops.prep_hash(q, k, v, coords, g["sqrt_w"], g["alpha"], cd, cell.tile, t0=cell.t0, tl=cell.Tl, raw_size=cell.raw)
    ledger.check()                                       # rows beyond N do not exist: nothing was stored past a buffer
    assert len(ledger.entries) >= 5                      # qhat, kvhat, qproj, kproj, minmax
    h, n, tl = cell.H, cell.N, cell.Tl
    assert ph["qhat"].shape == (h, n, 32) and ph["kvhat"].shape == (h, n, 64) and ph["qhat"].dtype == QK_DTYPE[cell.tile]
    assert ph["qproj"].shape == ph["kproj"].shape == (tl, h, n) and ph["minmax"].shape == (tl, h, PREP_GRID, 4)
    return ph


def expected_rows(cell, q_hat, k_hat, v, qn=None, kn=None):
    """(qhat, kvhat) images of the cell's tile type from float32-representable rows: the 16-bit elements are torch's
    round-to-nearest-even cast; the norm word is written where it is given (float32 values)."""
    h, n, d, e = cell.H, cell.N, cell.D, cell.D + cell.C
    dev = q_hat.device
    if cell.tile == "fp32":
        qhat = torch.zeros(h, n, 32, device=dev)
        kvhat = torch.zeros(h, n, 64, device=dev)
        qhat[..., :e], kvhat[..., :e], kvhat[..., 32:32 + d], kvhat[..., 32 + d] = q_hat.float(), k_hat.float(), v.float(), 1.0
        if qn is not None:
            qhat[..., 31], kvhat[..., 31] = qn.float(), kn.float()
        return qhat, kvhat
    dt = QK_DTYPE[cell.tile]
    qhat = torch.zeros(h, n, 32, device=dev, dtype=torch.int16)
    kvhat = torch.zeros(h, n, 64, device=dev, dtype=torch.int16)
    qhat[..., :e] = _bits(q_hat.float().to(dt))
    kvhat[..., :e] = _bits(k_hat.float().to(dt))
    kvhat[..., 32:32 + d] = _bits(v.float().to(torch.bfloat16))
    kvhat[..., 32 + d] = 0x3F80                          # bf16 1.0
    if qn is not None:                                   # word 15: the float32 bits in elements 30 (low half) and 31
        qhat[..., 30:32] = qn.float().contiguous().view(torch.int16).reshape(h, n, 2)
        kvhat[..., 30:32] = kn.float().contiguous().view(torch.int16).reshape(h, n, 2)
    return qhat, kvhat


def _row_bits(t):
    return _bits(t) if t.dtype == torch.float32 else t.contiguous().view(torch.int16)


def check_minmax(cell, mm, r, g, with_codes):
    """Checks 6 and 7: the range partials and the code-bound column."""
    inf = float("inf")
    assert not bool(torch.isnan(mm).any()), f"{cell.id}: a minmax slot keeps the poison"
    lo, hi, cb = mm[..., 0], mm[..., 1], mm[..., 2]
    assert float(mm[..., 3].abs().max()) == 0.0, f"{cell.id}: minmax column 3"
    neutral = (lo == inf) & (hi == -inf) & (cb == 0)
    ranged = torch.isfinite(lo) & torch.isfinite(hi) & (lo <= hi)
    assert bool((neutral | ranged).all()), f"{cell.id}: a slot that is neither a finite range nor the neutral one"
    for nm, half, hashed in (("q", slice(0, SLOTS), r["qh"]), ("k", slice(SLOTS, PREP_GRID), r["kh"])):
        # (padding rows are in `hashed` with projection 0: prep_hash.hip:301-303)
        assert torch.equal(lo[..., half].amin(-1).double(), hashed.amin(-1)), f"{cell.id}: {nm} range minimum"
        assert torch.equal(hi[..., half].amax(-1).double(), hashed.amax(-1)), f"{cell.id}: {nm} range maximum"
    assert float(cb.min()) >= 0.0 and float(cb[..., SLOTS:].abs().max()) == 0.0, f"{cell.id}: code bound"
    if with_codes:
        true_max = g["maxc"][cell.t0:cell.t0 + cell.Tl].float()
        assert bool((cb <= true_max[..., None]).all()), f"{cell.id}: code bound above the largest code"
        assert torch.equal(cb.amax(-1), true_max), f"{cell.id}: code bound of tile 0 (point 0 holds the largest code)"
    else:
        assert float(cb.abs().max()) == 0.0, f"{cell.id}: code bound without codes"


def check_sort(cell, ph, r, g, minmax=None):
    """Check 9: the sort fed by the builder's outputs against the stable sort of the float64 host keys."""
    from hept_amd import ops

    mm = ph["minmax"].clone() if minmax is None else minmax
    if cell.codes:
        qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], g["codes"], mm, t0=cell.t0)
    else:
        eta, phi, cfac = ops.geo_args((g["eta"], g["phi"]), g["regions_h"], cell.T, cell.H, cell.N)
        qp, kp = ops.sort_tables_src(ph["qproj"], ph["kproj"], eta, phi, cfac, mm, t0=cell.t0)
    assert qp.dtype == torch.int32 and qp.shape == (cell.Tl, cell.H, cell.N)
    assert torch.equal(qp.long(), r["qpos"]), f"{cell.id}: q permutation differs from the stable sort of the float64 keys"
    assert torch.equal(kp.long(), r["kpos"]), f"{cell.id}: k permutation differs from the stable sort of the float64 keys"
    return qp, kp


def check_exact(cell, dev):
    """Checks 1-9 of an exact cell, every one bit for bit."""
    g = _device_data(cell, dev)
    r = _device_reference(cell, dev)
    ph = run_builder(cell, dev)
    for nm in ("qproj", "kproj"):                        # 1, 2 (+inf at and after raw_size is in the reference)
        assert ph[nm].dtype == torch.float32 and torch.equal(ph[nm].double(), r[nm]), f"{cell.id}: {nm}"
    if cell.raw < cell.N:
        assert bool((ph["qproj"][..., cell.raw:] == float("inf")).all() and (ph["kproj"][..., cell.raw:] == float("inf")).all())
    want_q, want_kv = expected_rows(cell, r["q_hat"], r["k_hat"], r["v"], r["qn"], r["kn"])     # 3, 4, 5
    got_q, got_kv = _row_bits(ph["qhat"]), _row_bits(ph["kvhat"])
    e = cell.D + cell.C
    wq, wkv = _row_bits(want_q), _row_bits(want_kv)
    assert torch.equal(got_q[..., :e], wq[..., :e]), f"{cell.id}: q^ elements"
    assert torch.equal(got_kv[..., :e], wkv[..., :e]), f"{cell.id}: k^ elements"
    last = 31 if cell.tile == "fp32" else 30
    assert not bool((got_q[..., e:last] != 0).any() or (got_kv[..., e:last] != 0).any()), f"{cell.id}: columns E.. are not +0"
    assert torch.equal(got_q[..., last:], wq[..., last:]), f"{cell.id}: q^ norm word"
    assert torch.equal(got_kv[..., last:32], wkv[..., last:32]), f"{cell.id}: k^ norm word"
    assert torch.equal(got_kv[..., 32:], wkv[..., 32:]), f"{cell.id}: v half"
    assert torch.equal(got_q, wq) and torch.equal(got_kv, wkv), cell.id
    if cell.raw < cell.N:                                # 5: all-zero q^ / k^ / v rows, count column 1
        one = 0x3F800000 if cell.tile == "fp32" else 0x3F80
        assert not bool((got_q[:, cell.raw:, :last] != 0).any() or (got_kv[:, cell.raw:, :last] != 0).any()), cell.id
        pad_v = got_kv[:, cell.raw:, 32:]
        assert bool((pad_v[..., cell.D] == one).all()) and int((pad_v != 0).sum()) == cell.H * (cell.N - cell.raw), cell.id
    check_minmax(cell, ph["minmax"], r, g, cell.codes)  # 6, 7
    check_sort(cell, ph, r, g)                           # 9
    return ph


def check_codes_none(cell, dev):
    """Check 7, last item: without codes the bound column is 0 and nothing else changes."""
    g = _device_data(cell, dev)
    r = _device_reference(cell, dev)
    ph = run_builder(cell, dev, codes=None)
    check_minmax(cell, ph["minmax"], r, g, False)
    for nm in ("qproj", "kproj"):
        assert torch.equal(ph[nm].double(), r[nm]), f"{cell.id}: {nm}"


def check_code_bound(cell, dev):
    """The code bound is only a scale (prep_hash.hip:314-317): column 2 of a copy of minmax overwritten with 0, 1 and the
    true maximum -- values a sample can return -- gives the identical permutation, the stable sort of the float64 keys."""
    g = _device_data(cell, dev)
    r = _device_reference(cell, dev)
    ph = run_builder(cell, dev)
    true_max = g["maxc"][cell.t0:cell.t0 + cell.Tl].float()
    for value in (torch.zeros_like(true_max), torch.ones_like(true_max), true_max):
        mm = ph["minmax"].clone()
        mm[..., 2] = value[..., None]
        check_sort(cell, ph, r, g, minmax=mm)


def check_round(cell, dev):
    """A rounding cell: stored elements bit for bit torch's RNE cast; norm word and projections at the derived bounds."""
    g = _device_data(cell, dev)
    d = data(cell)
    q32, k32, v32 = (x.to(dev) for x in unrounded_rows(cell, d, torch.float32))   # a[e]: exact or once-rounded f32 products
    ph = run_builder(cell, dev)
    want_q, want_kv = expected_rows(cell, q32, k32, v32)
    got_q, got_kv = _row_bits(ph["qhat"]), _row_bits(ph["kvhat"])
    e, dt = cell.D + cell.C, QK_DTYPE[cell.tile]
    assert torch.equal(got_q[..., :30], want_q[..., :30]), f"{cell.id}: q^ elements are not the round-to-nearest-even cast"
    assert torch.equal(got_kv[..., :30], want_kv[..., :30]), f"{cell.id}: k^ elements are not the round-to-nearest-even cast"
    assert torch.equal(got_kv[..., 32:], want_kv[..., 32:]), f"{cell.id}: v half is not the bf16 round-to-nearest-even cast"
    figures = {}
    alpha = g["alpha"][:, :, cell.t0:cell.t0 + cell.Tl].double()
    for nm, a32, rows, proj in (("q", q32, ph["qhat"], ph["qproj"]), ("k", k32, ph["kvhat"][..., :32], ph["kproj"])):
        word = rows.contiguous().view(torch.int32)[..., 15].view(torch.float32).double()
        rr = a32.to(dt).double()
        ss_r, ss_a = (rr ** 2).sum(-1), (a32.double() ** 2).sum(-1)
        err = (word + 0.5 * ss_r).abs()
        figures[nm + "norm"] = float((err / (NORM_BOUND * ss_r)).max())
        assert bool((err <= NORM_BOUND * ss_r).all()), f"{cell.id}: {nm} norm word is not the norm of the rounded values"
        # ... and the bound tells the two norms apart: on some row the word is farther than it from the unrounded norm
        assert bool(((word + 0.5 * ss_a).abs() > NORM_BOUND * ss_a).any()), f"{cell.id}: {nm}: rounding moved no norm"
        ref = torch.einsum("hne,het->thn", a32.double(), alpha)
        mag = torch.einsum("hne,het->thn", a32.double().abs(), alpha.abs())
        perr = (proj.double() - ref).abs()
        figures[nm + "proj"] = float((perr / (NORM_BOUND * mag)).max())
        assert bool((perr <= NORM_BOUND * mag).all()), f"{cell.id}: {nm} projections are not those of the unrounded row"
    assert not bool(torch.isnan(ph["minmax"]).any()) and float(ph["minmax"][..., 3].abs().max()) == 0.0
    return figures


# ---------------------------------------------------------------------------------------------------------------------
# the two-role launch and the in-kernel scale (the one-call forward)
# ---------------------------------------------------------------------------------------------------------------------
def two_role_cases():
    out = [(n, (8, 24, 6), p) for n in TWO_ROLE_N for p in TWO_ROLE_PRECISIONS]
    out += [(TWO_ROLE_GENERIC[0], TWO_ROLE_GENERIC[1], "fp32")]
    return out + [(TWO_ROLE_N[0], hdc, p) for hdc in TWO_ROLE_COLUMN_D for p in TWO_ROLE_PRECISIONS]


def two_role_shape(n, hdc):
    import shape_sweep as sw

    h, d, c = hdc
    return sw.Shape(f"two-role-n{n}-h{h}d{d}c{c}", (n,), 32, 2, h, d, c, 7000 + n % 997, False)


_two = {}


def check_two_role(n, hdc, precision, dev):
    """One-call forward == staged kernels, bit for bit, where the one-call forward launches the row builder with two roles
    (the bucket-sort launch's riders write the v rows) and computes sqrt_w in the kernel (K > 0).  This is the only path
    to ``roles == 2``: the staged entry always launches three (prep_hash.hip:884).  Output identity only, random inputs as
    shape_sweep.inputs makes them."""
    import shape_sweep as sw
    from hept_amd import ops

    s = two_role_shape(n, hdc)
    assert sw.riders(n, s.H, s.D, s.T, precision, s.B)
    if _two.get("id") != s.id:
        _two.clear()
        inp = sw.inputs(s)
        _two.update(id=s.id, g={k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)})
    g = _two["g"]
    st = sw.staged(s, g, precision)
    one = ops.forward(g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"],
                      g["out_weight"], g["out_bias"], block_size=s.B, w_per_dist=10, precision=precision)
    assert bool(torch.isfinite(one).all()), (s.id, precision)
    assert _same_bits(one, st["out"]), f"{s.id} {precision}: one-call forward (two-role row builder) differs from the staged kernels"
