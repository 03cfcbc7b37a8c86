"""The block sweep: every instantiation of the block-attention kernels (csrc/block_attn.hip, csrc/block_attn_coords.hip,
and csrc/block_attn_bwd.hip: the section at the end of this file) at the smallest shapes that reach it, bit for bit
against a float64 result that is exact by construction; run by
tests/test_gpu_block_sweep.py, the coverage and the exactness of the design pinned on the CPU by
tests/test_block_sweep_cells.py.  A plain module, not a conftest.  Nothing here touches the GPU at import time.

The exact design.  Every point n has a group g(n), and q^_n = k^_n is the group's row: +-s e_col one-hot over the D feature
columns (s = 16) or over the C coordinate columns (integer ``coords`` of +-16 against power-of-two ``sqrt_w[h, c]`` = 1, 2
or 4, which depend on the head), the all-zero row (the zero group), or -- for D >= 2 -- one of two PAIR rows s e_f + s' e_c0
that share their coordinate column and differ in the feature column (a product that let the coordinate columns of the
stored rows in beside the f32 coordinate part would give two such points the logit 0).  Same group: the logit is exactly 0
in the expanded form (s^2 - s^2/2 - s^2/2) and in the difference form, the weight exactly 1.0.  Different groups: the
logit is an integer <= -128 (zero group against a one-hot row: -s^2/2), and exp(-128) = 2^-184.7 is exactly 0 in float32
(below the smallest subnormal) and therefore in bf16.  ``v`` is integer in -3..3 (-1..1 where a block could otherwise
sum past 256: the packed rows hold bf16 numerators, and every integer up to 256 is a bf16 value).  So

    numer[i] = sum of v[j] over the keys j of the query's block with the query's group
    denom[i] = that count + 1e-20      (= the count for count >= 1, exactly 1e-20f for an empty set)

hold in ANY summation order, and the expected rows come from group membership alone, in float64.  ``bounds(case)`` proves
the premises on the CPU from an emulation of each family's arithmetic in torch float32 on the groups' rows (all points of
a group hold the same row, so the G x G table of logits is the whole story).

The rows go through ``ops.prep_hash`` and the block kernels run on INJECTED permutations, two tables with different ones
(both index maps of HeadRange.tl then see distinct data), N = 3 B (first, middle and last block), H = 3.  The permutations
are seeded draws with fix-ups: the queries and keys of a block are different point sets; point 0 carries a group of its own
and its key copy sits in another block than its query copy (an empty set: the 1e-20 row); the key just before and the key
just behind every block (for ragged B the slot just past B) carries the group of a query of the block, so that a leak over
a block boundary shows as count + 1.  (Past the LAST block of a table there is no key slot to bait.  The padded slots of a
ragged tile are zero-filled while they are staged, value row and 1.0 column included: whatever weight such a slot were
given would multiply zeros.)

"mixed16_diff" edge cases at nkt in {1, 2, 5, 8}, full and ragged, every CT: coordinates beyond the fp16 range (sqrt_w *
coords multiples of 2^17: the stored fp16 columns hold +-65504, where the row builder saturates, and must never meet the
matrix pipe -- the pair rows would get the logit 0 for -s^2), and raw_size < N (src
variant: rows at and after raw_size count as the zero group with v = 0, and must equal what "mixed16" writes for them).

One random-valued float64 cell per (family, nkt, fullness) runs the staged pipeline as shape_sweep.check_forward /
test_gpu_mixed16_diff hold it, at the bounds those modules already have (imported, not copied).

Equality is asserted on the float32 VALUES first and on the bits second (the expected zeros are +0: an accumulator that
starts at +0 cannot reach -0 under round-to-nearest)."""
import zlib
from collections import namedtuple

import torch

Case = namedtuple("Case", "id family nkt kind B D C variant raw")

H, TL, S = 3, 2, 16.0
KINDS = ("full", "one", "short")            # B = 32 nkt | 32 (nkt - 1) + 1 (one key in the last tile) | 32 nkt - 1
PAIRS = [(1, 2), (2, 28), (8, 4), (17, 3), (20, 5), (27, 3), (28, 2)]   # (D, C) of the f32-part families, D + C <= 30
EDGE_NKT = (1, 2, 5, 8)
BIG = 2.0 ** 17                             # |sqrt_w coords| of the overflow cases: beyond the fp16 range
ZERO_WEIGHT_LOGIT = -128.0                  # the least negative logit between two groups: exp() is exactly 0 in f32

# family -> (precision of the rows, block_attn's f32_mfma argument, HEPT_DIFF_MFMA, kernel, tag of the instantiation,
#            the (D, C) the family rotates over)
_C24 = [(24, 6), (24, 4), (24, 2), (24, 5), (24, 3), (24, 1)]
FAMILIES = {
    "fp32": ("fp32", False, None, "split", "DIFF=0", PAIRS),
    "fp32_mfma": ("fp32_mfma", True, None, "attn", "F32 DIFF=0", PAIRS),
    "fp32_diff_split": ("fp32_diff", "diff", "0", "split", "DIFF=1", _C24),
    "fp32_diff_mfma": ("fp32_diff", "diff", "1", "attn", "F32 DIFF=1", PAIRS + [(24, 6)]),   # D = 24 under HEPT_DIFF_MFMA=1
    "bf16_packed": ("bf16", False, None, "attn", "P16=1 F16QK=0", _C24),
    "bf16_f32": ("bf16", False, None, "attn", "P16=0 F16QK=0", PAIRS),
    "mixed16_packed": ("mixed16", False, None, "attn", "P16=1 F16QK=1", _C24),
    "mixed16_f32": ("mixed16", False, None, "attn", "P16=0 F16QK=1", PAIRS),
    "m16d_c2": ("mixed16_diff", False, None, "coords", "P16=1 CT=2", [(24, 2)]),
    "m16d_c4": ("mixed16_diff", False, None, "coords", "P16=1 CT=4", [(24, 4)]),
    "m16d_c6": ("mixed16_diff", False, None, "coords", "P16=1 CT=6", [(24, 6)]),
    "m16d_crt": ("mixed16_diff", False, None, "coords", "P16=1 CT=0", [(24, 3), (24, 5)]),   # packed rows, runtime C
    "m16d_f32": ("mixed16_diff", False, None, "coords", "P16=0 CT=0", PAIRS),
}
M16D = [f for f in FAMILIES if f.startswith("m16d")]
# file:line references of the dispatch rules cells() mirrors (tests/test_block_sweep_cells.py checks the text)
REFS = [
    ("hept_amd/csrc/block_attn.hip", 758, "if (B == 32 * nkt)"),
    ("hept_amd/csrc/block_attn.hip", 766, "int block_attn_impl("),
    ("hept_amd/csrc/block_attn.hip", 786, "nkt = (B + 31) / 32"),
    ("hept_amd/csrc/block_attn.hip", 800, "precision == HEPT_PREC_BF16 && D == 24"),
    ("hept_amd/csrc/block_attn.hip", 804, "precision == HEPT_PREC_MIXED16 && D == 24"),
    ("hept_amd/csrc/block_attn.hip", 811, "launch_attn_split<true, 3>"),
    ("hept_amd/csrc/block_attn.hip", 815, "launch_attn<false, false, false>"),
    ("hept_amd/csrc/block_attn.hip", 821, "if (D == 24 && !mfma)"),
    ("hept_amd/csrc/block_attn.hip", 827, "launch_attn<false, false, false, true>"),
    ("hept_amd/csrc/block_attn.hip", 835, "hept_block_attn_coords_launch("),
    ("hept_amd/csrc/block_attn_coords.hip", 39, "w = (f0 ? (w & 0x0000FFFFu) : 0u)"),
    ("hept_amd/csrc/block_attn_coords.hip", 153, "const bool kreal = kvalid && src < raw_size;"),
    ("hept_amd/csrc/block_attn_coords.hip", 240, ">= B) pr[r] = 0.f;"),
    ("hept_amd/csrc/block_attn_coords.hip", 345, "const bool full = B == 32 * nkt;"),
    ("hept_amd/csrc/block_attn_coords.hip", 352, "if (D == 24) {"),
    ("hept_amd/csrc/block_attn_coords.hip", 353, "if (C == 2) HEPT_COORDS_GO(true, 2);"),
    ("hept_amd/csrc/block_attn_coords.hip", 356, "HEPT_COORDS_GO(true, 0);"),
    ("hept_amd/csrc/block_attn_coords.hip", 358, "HEPT_COORDS_GO(false, 0);"),
]


def block_of(nkt, kind):
    return {"full": 32 * nkt, "one": 32 * (nkt - 1) + 1, "short": 32 * nkt - 1}[kind]


def _cases():
    out = []
    for fi, (fam, spec) in enumerate(FAMILIES.items()):
        dcs = spec[5]
        for nkt in range(1, 9):
            for ki, kind in enumerate(KINDS):
                # (the coords kernel's f32-part family starts the rotation where C = 28 meets B = 256: its largest LDS request)
                d, c = dcs[((nkt - 1) * 3 + ki + (1 if fam == "m16d_f32" else fi)) % len(dcs)]
                b = block_of(nkt, kind)
                out.append(Case(f"{fam}-k{nkt}{kind}-b{b}-d{d}c{c}", fam, nkt, kind, b, d, c, "exact", None))
    for fi, fam in enumerate(M16D):
        dcs = FAMILIES[fam][5]
        for ni, nkt in enumerate(EDGE_NKT):
            for ki, kind in enumerate(("full", "short")):
                d, c = dcs[(ni * 2 + ki + fi) % len(dcs)]
                b = block_of(nkt, kind)
                out.append(Case(f"{fam}-k{nkt}{kind}-b{b}-d{d}c{c}-big", fam, nkt, kind, b, d, c, "big", None))
                for raw in (3 * b - 1, 2 * b - 1, 1):               # N - 1, N - B - 1, 1
                    out.append(Case(f"{fam}-k{nkt}{kind}-b{b}-d{d}c{c}-raw{raw}", fam, nkt, kind, b, d, c, "raw", raw))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def cells(case):
    """The kernel instantiation a case runs: (kernel, NKT, FULL, tag), as block_attn_impl (csrc/block_attn.hip:766-839)
    and hept_block_attn_coords_launch (csrc/block_attn_coords.hip:341-360) choose it."""
    prec, _, env, _, _, _ = FAMILIES[case.family]
    nkt = (case.B + 31) // 32                                      # block_attn.hip:786
    full = case.B == 32 * nkt                                      # block_attn.hip:758, block_attn_coords.hip:345
    if prec == "fp32":
        return ("split", nkt, full, "DIFF=0")
    if prec == "fp32_mfma":
        return ("attn", nkt, full, "F32 DIFF=0")
    if prec == "fp32_diff":
        if case.D == 24 and env != "1":                            # block_attn.hip:821
            return ("split", nkt, full, "DIFF=1")
        return ("attn", nkt, full, "F32 DIFF=1")
    if prec in ("bf16", "mixed16"):
        return ("attn", nkt, full, f"P16={int(case.D == 24)} F16QK={int(prec == 'mixed16')}")
    if case.D == 24:                                               # block_attn_coords.hip:352-356
        return ("coords", nkt, full, f"P16=1 CT={case.C if case.C in (2, 4, 6) else 0}")
    return ("coords", nkt, full, "P16=0 CT=0")


def all_instantiations():
    tags = {(spec[3], spec[4]) for spec in FAMILIES.values()}
    return {(k, nkt, full, tag) for k, tag in tags for nkt in range(1, 9) for full in (True, False)}


# ---------------------------------------------------------------------------------------------------------------------
# the design (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def group_rows(case):
    """(feature rows (G, D), coordinate signs (G, C)) of the groups: 0 = the zero group, then the one-hot rows, then the pair
    rows.  The scaled coordinate of head h is sign * mag * sqrt_w[h, c]."""
    d, c = case.D, case.C
    feats, cds = [torch.zeros(d)], [torch.zeros(c)]
    for col in range(d + c):
        for sign in (1.0, -1.0):
            f, x = torch.zeros(d), torch.zeros(c)
            if col < d:
                f[col] = sign * S
            else:
                x[col - d] = sign
            feats.append(f)
            cds.append(x)
    if d >= 2:
        for fcol in (0, 1):
            f, x = torch.zeros(d), torch.zeros(c)
            f[fcol], x[0] = S, 1.0
            feats.append(f)
            cds.append(x)
    return torch.stack(feats), torch.stack(cds)


def sqrt_w_of(case):
    return torch.tensor([[2.0 ** ((h + c) % 3) for c in range(case.C)] for h in range(H)])


def coord_mag(case):
    return BIG if case.variant == "big" else 16.0


_design = {}


def design(case):
    """CPU inputs, permutations and the expected partial rows of a case (the last case built is kept)."""
    if _design.get("id") == case.id:
        return _design["d"]
    n, b, d, c = 3 * case.B, case.B, case.D, case.C
    raw = n if case.raw is None else case.raw
    feats, cds = group_rows(case)
    n_groups = feats.shape[0]
    seed = zlib.crc32(case.id.encode())
    gen = torch.Generator().manual_seed(seed)
    order = (1 + torch.randperm(n_groups - 1, generator=gen)).tolist()      # the non-zero groups, shuffled
    if n >= 12:
        # point 0: a one-hot group that no other point has; the others round-robin over the rest, the zero group included
        rare = next(g for g in order if g <= 2 * (d + c))
        rest = [0] + [g for g in order if g != rare]
        grp = torch.tensor([rare] + [rest[i % len(rest)] for i in range(n - 1)])
    else:
        rare = None
        grp = torch.tensor([order[i % 2] for i in range(n)])               # B = 1: two groups over three points
    eff = grp.clone()
    eff[raw:] = 0                                                           # padding rows count as the zero group
    q = feats[grp].repeat(1, H)                                             # (N, H * D): the same row in every head
    coords = cds[grp] * coord_mag(case)
    sqrt_w = sqrt_w_of(case)
    pgen = torch.Generator().manual_seed(seed + 7919)
    qs, ks = [], []
    for _ in range(TL * H):
        for _attempt in range(400):                                         # (a handful of draws at B = 1, one elsewhere)
            qp, kp = _permutation_pair(eff, rare, n, b, pgen)
            # (B = 1 has few draws that pass: the second table must still differ from the first, head by head)
            twin = len(qs) >= H and (torch.equal(qp, qs[len(qs) - H]) or torch.equal(kp, ks[len(ks) - H]))
            if not twin and perm_facts(eff, qp.reshape(1, 1, n), kp.reshape(1, 1, n), b)["ok"]:
                break
        else:
            raise AssertionError(f"{case.id}: no permutation draw meets the bait conditions")
        qs.append(qp)
        ks.append(kp)
    qpos, kpos = (torch.stack(x).reshape(TL, H, n).to(torch.int32) for x in (qs, ks))
    facts = perm_facts(eff, qpos, kpos, b)
    assert facts["ok"], case.id
    # values: -3..3, narrowed to -1..1 where a block's same-group keys could sum past 256
    lim = 3 if 3 * facts["max_count"] <= 256 else 1
    v = torch.randint(-lim, lim + 1, (n, H * d), generator=gen).float()
    v_eff = v.clone()
    v_eff[raw:] = 0.0
    alpha = torch.randint(-2, 3, (H, d + c, TL), generator=gen).float()
    out = dict(n=n, raw=raw, grp=grp, eff=eff, q=q, k=q.clone(), v=v, coords=coords, sqrt_w=sqrt_w, alpha=alpha,
               qpos=qpos, kpos=kpos, facts=facts, vlim=lim, feats=feats, cds=cds,
               want=expected(eff, v_eff, qpos, kpos, b, d))
    _design.update(id=case.id, d=out)
    return out


def _permutation_pair(eff, rare, n, b, gen):
    """(qpos, kpos) of one (table, head), each (N,): seeded draws, then the fix-ups of the module docstring on the key side."""
    nb = n // b
    qp, kp = torch.randperm(n, generator=gen), torch.randperm(n, generator=gen)
    locked = torch.zeros(n, dtype=torch.bool)
    if rare is not None:
        bq = int((qp == 0).nonzero()) // b
        at = int((kp == 0).nonzero())
        if at // b == bq:                                           # the key copy of point 0 leaves its query's block
            to = ((bq + 1) % nb) * b + b // 2
            kp[[at, to]] = kp[[to, at]]
            at = to
        locked[at] = True
    for blk in range(nb):
        targets = torch.unique(eff[qp[blk * b:(blk + 1) * b]])
        for slot in (blk * b - 1, (blk + 1) * b):
            if not 0 <= slot < n or locked[slot]:
                continue
            if not bool(torch.isin(eff[kp[slot]], targets)):
                free = (torch.isin(eff[kp], targets) & ~locked).nonzero().flatten()
                free = free[free != slot]
                if free.numel() == 0:
                    continue
                other = int(free[int(torch.randint(0, free.numel(), (1,), generator=gen))])
                kp[[slot, other]] = kp[[other, slot]]
            locked[slot] = True
    return qp, kp


def perm_facts(eff, qpos, kpos, b):
    """What bounds() asserts of the permutations: per (table, head) an empty-set row and a block whose queries and keys are
    different point sets; per block a boundary bait (a neighbouring block's adjacent key with the group of one of the
    block's queries); the largest same-group key count of a block."""
    tl, h, n = qpos.shape
    nb = n // b
    empty, differ, baits, max_count = [], [], [], 0
    for t in range(tl):
        for hh in range(h):
            qp, kp = qpos[t, hh].long(), kpos[t, hh].long()
            gq, gk = eff[qp].reshape(nb, b), eff[kp].reshape(nb, b)
            count = (gq[:, :, None] == gk[:, None, :]).sum(-1)
            max_count = max(max_count, int(count.max()))
            empty.append(int((count == 0).sum()))
            differ.append(any(set(qp[i * b:(i + 1) * b].tolist()) != set(kp[i * b:(i + 1) * b].tolist()) for i in range(nb)))
            for blk in range(nb):
                hit = 0
                for slot in (blk * b - 1, (blk + 1) * b):
                    if 0 <= slot < n and bool((gq[blk] == eff[kp[slot]]).any()):
                        hit += 1
                baits.append(hit)
    perms = all(torch.equal(torch.sort(p.long(), -1).values, torch.arange(n).expand(tl, h, n)) for p in (qpos, kpos))
    ok = perms and all(differ) and min(baits) >= 1 and min(empty) >= 1
    return dict(ok=ok, empty=empty, differ=differ, baits=baits, max_count=max_count, perms=perms)


def expected(eff, v_eff, qpos, kpos, b, d):
    """The partial rows (TL, N, H, 32) float32 from group membership alone, in float64."""
    tl, h, n = qpos.shape
    nb = n // b
    want = torch.zeros(tl, n, h, 32, dtype=torch.float64)
    vh = v_eff.double().reshape(n, h, d)
    for t in range(tl):
        for hh in range(h):
            qp, kp = qpos[t, hh].long(), kpos[t, hh].long()
            gq, gk = eff[qp].reshape(nb, b), eff[kp].reshape(nb, b)
            same = (gq[:, :, None] == gk[:, None, :]).double()
            numer = torch.matmul(same, vh[kp, hh].reshape(nb, b, d)) + 0.0
            want[t, qp, hh, :d] = numer.reshape(n, d)
            want[t, qp, hh, d] = same.sum(-1).reshape(n) + 1e-20
    out = want.float()
    assert torch.equal(out.double()[..., :d], want[..., :d])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the families' arithmetic on the groups' rows (CPU, float32)
# ---------------------------------------------------------------------------------------------------------------------
def emulate_logits(case):
    """(H, G + 1, G + 1) float32: the logit each family forms between a query of group i and a key of group j, from the rows
    as the row builder stores them; index G is a padding row (src variant, all zero).  The backward kernels recompute the
    logits of their forward: "fp32" rows expanded (split and f32 MFMA), "fp32_diff", "bf16"."""
    prec = FAMILIES[case.family][0] if case.family in FAMILIES else BWD_FAMILIES[case.family][1]
    feats, cds = group_rows(case)
    g = feats.shape[0]
    feats = torch.cat([feats, torch.zeros(1, case.D)])
    cds = torch.cat([cds * coord_mag(case), torch.zeros(1, case.C)])
    tile = {"bf16": torch.bfloat16, "mixed16": torch.float16, "mixed16_diff": torch.float16}.get(prec, torch.float32)
    out = []
    for h in range(H):
        cs = sqrt_w_of(case)[h][None] * cds                                        # f32 products
        rows = torch.cat([feats, cs], 1)
        if tile == torch.float16:
            rows = rows.clamp(-65504.0, 65504.0)                                   # hept_pack_f16 (csrc/common.h:103) saturates
        rows = rows.to(tile).float()                                               # the stored rows
        f, cst = rows[:, :case.D], rows[:, case.D:]
        stored = -0.5 * (rows ** 2).sum(-1)                                        # the norm in the row tail
        if prec in ("fp32", "fp32_mfma", "bf16", "mixed16"):
            x = rows @ rows.T + stored[:, None] + stored[None, :]
        else:
            fn = -0.5 * (f ** 2).sum(-1)
            x = f @ f.T + fn[:, None] + fn[None, :]
            cc = cst if prec == "fp32_diff" else cs                                # stored values | the f32 products
            for c in range(case.C):
                dl = cc[:, c][:, None] - cc[:, c][None, :]
                x = x - 0.5 * dl * dl
            if prec == "mixed16_diff":
                x[g, :] = stored                                                   # a padding query: the key's stored norm
        out.append(x)
    return torch.stack(out)


def bounds(case):
    """The premises of the exact design: weights in {0, 1} (the emulated logit is exactly 0 within a group and at most
    ZERO_WEIGHT_LOGIT across groups, padding rows standing in for the zero group), numerators and counts within 256,
    an empty-set row and the baits."""
    d = design(case)
    x = emulate_logits(case)
    g = x.shape[1] - 1
    same = torch.eye(g + 1, dtype=torch.bool)
    same[0, g] = same[g, 0] = True                                 # padding = zero group
    same = same.expand_as(x)
    w = x.clamp(max=0.0).exp()
    weights_ok = bool(torch.isfinite(x[same]).all()) and bool((x[same] == 0).all()) and bool((w[same] == 1).all()) \
        and bool((x[~same] <= ZERO_WEIGHT_LOGIT).all()) and bool((w[~same] == 0).all()) and not bool(torch.isnan(x).any())
    want = d["want"]
    return dict(weights_ok=weights_ok, max_numer=float(want[..., :case.D].abs().max()),
                max_count=float(want[..., case.D].max()), empty_rows=int((want[..., case.D] == 1e-20).sum()),
                baits=d["facts"]["baits"], facts=d["facts"], least_negative=float(x[~same].max()))


# ---------------------------------------------------------------------------------------------------------------------
# GPU checks (imports deferred)
# ---------------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    got, want = got.contiguous(), want.contiguous()
    if got.dtype.is_floating_point:
        bad = ~(got == want)
        if bool(bad.any()):
            idx = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first at {idx}: got {got[idx].item()!r}, "
                                 f"expected {want[idx].item()!r}")
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), f"{what}: equal values, other bits"


def _check_rows(case, d, ph):
    """The finite stored columns decode to the design (a failure here is the row builder's, not the block kernel's)."""
    n, dd, c = d["n"], case.D, case.C
    cs = d["sqrt_w"][:, None, :] * d["coords"][None]                               # (H, N, C)
    want = torch.cat([d["q"].reshape(n, H, dd).permute(1, 0, 2), cs], -1)
    want[:, d["raw"]:] = 0.0
    for name in ("qhat", "kvhat"):
        got = ph[name][..., :dd + c].float().cpu()
        fits = want.abs() <= 65504.0                                               # all of them but in the "big" cases
        assert bool(fits.all()) or (case.variant == "big" and ph[name].dtype == torch.float16), case.id
        assert torch.equal(got[fits], want[fits]), f"{case.id}: stored {name} columns differ from the design"
        assert bool((got[~fits].abs() >= 65504.0).all()), f"{case.id}: {name}, columns beyond the fp16 range"
    vhalf = ph["kvhat"][..., 32:]
    if vhalf.dtype == torch.float16:
        vhalf = vhalf.contiguous().view(torch.bfloat16)
    vgot = vhalf[..., :dd + 1].float().cpu()
    vwant = torch.cat([d["v"].reshape(n, H, dd).permute(1, 0, 2), torch.ones(H, n, 1)], -1)
    vwant[:, d["raw"]:, :dd] = 0.0
    assert torch.equal(vgot, vwant), f"{case.id}: stored v rows differ from the design"


def check_exact(case, dev):
    """The case's kernel on its design: every partial row bit for bit.  HEPT_DIFF_MFMA is the caller's to set."""
    from hept_amd import ops

    prec, f32_mfma, _, _, _, _ = FAMILIES[case.family]
    d = design(case)
    g = {k: d[k].to(dev) for k in ("q", "k", "v", "coords", "sqrt_w", "alpha", "qpos", "kpos")}
    raw = None if case.raw is None else case.raw
    ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], g["sqrt_w"], g["alpha"], None, prec, raw_size=raw)
    _check_rows(case, d, ph)
    if prec == "mixed16_diff":
        part = ops.block_attn_coords(ph["qhat"], ph["kvhat"], g["qpos"], g["kpos"], g["coords"], g["sqrt_w"], case.D,
                                     case.B, raw_size=raw)
    else:
        part = ops.block_attn(ph["qhat"], ph["kvhat"], g["qpos"], g["kpos"], case.D, case.B, f32_mfma=f32_mfma)
    torch.cuda.synchronize()
    packed = part.dtype == torch.int32
    assert packed == ("P16=1" in cells(case)[3]), case.id
    if packed:
        assert int(part[..., 13:].abs().max()) == 0, f"{case.id}: dwords 13-15 of the packed rows"
    wide = ops.unpack_part(part).cpu()
    _same(wide, d["want"], f"{case.id}: partial rows (table, point, head, column)")
    if case.variant == "raw":
        plain = ops.block_attn(ph["qhat"], ph["kvhat"], g["qpos"], g["kpos"], case.D, case.B)
        torch.cuda.synchronize()
        _same(part[:, case.raw:].cpu(), plain[:, case.raw:].cpu(), f"{case.id}: rows at and after raw_size against mixed16")


# ---- the float64 cells ------------------------------------------------------------------------------------------------
F64_PAIRS = [(8, 4), (17, 3), (20, 5), (27, 3), (16, 6), (12, 3), (10, 6)]   # head shapes the shape sweep runs as well
F64Case = namedtuple("F64Case", "id family nkt kind shape")
# Cells whose worst row against the "mixed16_diff" model exceeds test_gpu_mixed16_diff.MODEL_ROW (2.0e-3, set at 2x the worst
# row measured on that file's cells) although the kernel is right: the bound is a bound on last-bit flips -- a logit that
# differs in its last f32 bit moves a weight by one bf16 step -- and the EMULATION moves by more than that on these inputs.
# Cell bound = 2x the emulation's own worst row when every logit of the model is moved one f32 ulp up, against the model as
# it stands.  d16c6 at B = 128: emulated 2.150e-3 (one row of 512 over 1e-3; one ulp down: 4.7e-4); measured kernel against
# the model 2.150e-3 (the same row), against the one-ulp-up model 3.9e-4, against float64 5.190e-3 (the model: 5.192e-3).
F64_MODEL_ROW_CELL = {"m16d_f32-k4full-b128-d16c6-f64": 4.3e-3}


def _f64_cases():
    import shape_sweep as sw

    out = []
    for fi, (fam, spec) in enumerate(FAMILIES.items()):
        dcs = F64_PAIRS + ([(24, 6)] if fam == "fp32_diff_mfma" else []) if spec[5] is PAIRS or fam == "fp32_diff_mfma" \
            else spec[5]
        dcs = [dc for dc in dcs if dc[1] >= 2]
        for nkt in range(1, 9):
            for ki, kind in enumerate(("full", "short")):
                d, c = dcs[((nkt - 1) * 2 + ki + fi) % len(dcs)]
                b = block_of(nkt, kind)
                cid = f"{fam}-k{nkt}{kind}-b{b}-d{d}c{c}-f64"
                shape = sw.Shape(cid, (4 * b,), b, TL, H, d, c, 7000 + len(out), False)
                out.append(F64Case(cid, fam, nkt, kind, shape))
    return out


F64_CASES = _f64_cases()
F64_BY_ID = {c.id: c for c in F64_CASES}


def f64_cells(fc):
    s = fc.shape
    return cells(Case(fc.id, fc.family, fc.nkt, fc.kind, s.B, s.D, s.C, "f64", None))


def check_f64(fc, dev):
    """One random-valued cell: the staged pipeline on the GPU's own (sorted) permutations against float64, at the bounds of
    shape_sweep (f32 tiles: ATOL / RTOL per element; bf16 / mixed16: REL16_ALL_ROWS_FULL and MODEL16_ROW against the
    16-bit model) and of test_gpu_mixed16_diff (ROW64, MODEL_ROW against ``model``).  Returns the measured figures."""
    import shape_sweep as sw

    s = fc.shape
    prec = FAMILIES[fc.family][0]
    if prec != "mixed16_diff":
        sid = {"fp32_diff_split": "fp32_diff_split", "fp32_diff_mfma": "fp32_diff_mfma"}.get(fc.family, prec)
        return sw.check_forward(s, sid, dev)
    import test_gpu_mixed16_diff as md
    from hept_amd import ops

    inp = sw._cached((s.id, "inp"), lambda: sw.inputs(s))
    g = sw._cached((s.id, "gpu"), lambda: sw._gpu(inp, dev))
    st = md.staged(g, s.H, s.D, s.B)
    torch.cuda.synchronize()
    out = st["out"].cpu()
    assert bool(torch.isfinite(out).all()), s.id
    wide = ops.unpack_part(st["part"])
    assert (st["part"].dtype == torch.int32) == (s.D == 24)
    assert bool((wide[..., s.D] > 0).all()) and float(wide[..., s.D + 1:].abs().max()) == 0.0, s.id
    ref = sw._reference(s, inp, st["qpos"], st["kpos"])["out"]
    w64 = sw._row_scaled(out, ref)
    wm = sw._row_scaled(out, md._model_of(inp, st["qpos"], st["kpos"], s.B))
    print(f"block sweep {s.id}: worst row vs float64 {w64:.3e}, vs the model {wm:.3e}")
    assert w64 <= md.ROW64, f"{s.id}: worst row-scaled error vs float64 {w64:.3e}"
    assert wm <= F64_MODEL_ROW_CELL.get(fc.id, md.MODEL_ROW), f"{s.id}: worst row-scaled error vs the model {wm:.3e}"
    return dict(row64=w64, model=wm)


# ---------------------------------------------------------------------------------------------------------------------
# the backward (csrc/block_attn_bwd.hip): the same design through the four block-backward entries
# ---------------------------------------------------------------------------------------------------------------------
# With P in {0, 1} and q^_i = k^_j wherever P_ij = 1, dS_ij = P_ij (gnum_i . v_j + gden_i) is an integer and every term
# dS_ij (k^_j - q^_i) of d q^ / d k^ is exactly 0: dq, dk, the coordinate gradient dcs and d sqrt_w must be EXACTLY 0 (the
# kernels form Z - rowsum(dS) q^ from two equal integers below 2^24), and
#     dv[j] = sum over the tables and over the queries i of the key's block with the key's group of gnum[i]
# exact integers.  The same-group logit sits on the clamp point 0, where the two conventions for the derivative of
# min(S, 0) differ: it multiplies k^ - q^ = 0, so either gives 0, and dv does not see the mask.  The partial-row buffers
# start as NaN, the outputs of the reduction too (dense_sweep.bwd_reduce_call): an element that is not written shows.
# family -> (precision of the rows, the forward arithmetic the kernel recomputes its logits in, C entry, kernel of cells())
BWD_FAMILIES = {
    "bwd_split": ("fp32", "fp32", "hept_block_attn_bwd", "bwd_split"),
    "bwd_f32mfma": ("fp32", "fp32_mfma", "hept_block_attn_bwd_f32mfma", "bwd DIFF=0"),
    "bwd_diff": ("fp32", "fp32_diff", "hept_block_attn_bwd_diff", "bwd DIFF=1"),
    "bwd_bf16": ("bf16", "bf16", "hept_block_attn_bwd_bf16", "bwd_bf16"),
}
BWD_PAIRS = PAIRS + [(24, 6)]
BWD_REFS = [
    ("hept_amd/csrc/block_attn_bwd.hip", 951, "c0 += BWD_DIFF_COLS"),
    ("hept_amd/csrc/block_attn_bwd.hip", 1044, "nkt = (B + 31) / 32"),
    ("hept_amd/csrc/block_attn_bwd.hip", 1047, "const bool full = B == 32 * nkt;"),
    ("hept_amd/csrc/block_attn_bwd.hip", 1091, "return B == 32 * nkt ? launch_bwd_bf16<true>"),
    ("hept_amd/csrc/block_attn_bwd.hip", 1102, "if (d_sqrt_w && H * C > 64) return HEPT_ERR_SHAPE;"),
]


def _bwd_cases():
    out = []
    for fi, fam in enumerate(BWD_FAMILIES):
        for nkt in range(1, 9):
            for ki, kind in enumerate(KINDS):
                d, c = BWD_PAIRS[((nkt - 1) * 3 + ki + 3 * fi) % len(BWD_PAIRS)]
                b = block_of(nkt, kind)
                out.append(Case(f"{fam}-k{nkt}{kind}-b{b}-d{d}c{c}", fam, nkt, kind, b, d, c, "bwd", None))
    return out


BWD_CASES = _bwd_cases()
BWD_BY_ID = {c.id: c for c in BWD_CASES}


def bwd_cells(case):
    nkt = (case.B + 31) // 32                                      # block_attn_bwd.hip:1044
    return (BWD_FAMILIES[case.family][3], nkt, case.B == 32 * nkt)  # block_attn_bwd.hip:1047, 1091


def bwd_design(case):
    """The forward design of the case plus the upstream rows gacc (N, H, 32) = [gnum (D) | gden | 0], integers in -3..3
    (-1..1 where a key's per-table dv could otherwise pass 256, the largest run of integers a bf16 per-table row holds),
    and the expected dv (N, H * D)."""
    d = design(case)
    n, b, dd = d["n"], case.B, case.D
    nb = n // b
    sames = {}
    qmax = 0
    for t in range(TL):
        for hh in range(H):
            qp, kp = d["qpos"][t, hh].long(), d["kpos"][t, hh].long()
            same = (d["eff"][qp].reshape(nb, b)[:, :, None] == d["eff"][kp].reshape(nb, b)[:, None, :]).double()
            sames[t, hh] = (same, qp, kp)
            qmax = max(qmax, int(same.sum(1).max()))
    glim = 3 if 3 * qmax <= 256 else 1
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode()) + 1)
    gacc = torch.zeros(n, H, 32)
    gacc[..., :dd + 1] = torch.randint(-glim, glim + 1, (n, H, dd + 1), generator=gen).float()
    dv = torch.zeros(n, H, dd, dtype=torch.float64)
    table_max = 0.0
    for (t, hh), (same, qp, kp) in sames.items():
        mine = torch.matmul(same.transpose(1, 2), gacc[qp, hh, :dd].double().reshape(nb, b, dd)).reshape(n, dd)
        table_max = max(table_max, float(mine.abs().max()))
        dv[kp, hh] += mine
    # the largest |dS| = |gnum . v + gden| and the largest partial sum of Z = sum_j dS_ij k^_j (|k^| <= 64)
    ds_max = dd * glim * d["vlim"] + glim
    z_max = d["facts"]["max_count"] * ds_max * 64.0
    return dict(d, gacc=gacc, dv=dv.float().reshape(n, H * dd), glim=glim, table_max=table_max, ds_max=ds_max, z_max=z_max)


def check_bwd(case, dev):
    import dense_sweep as ds
    from hept_amd import _lib, ops

    rows_prec, _, entry, _ = BWD_FAMILIES[case.family]
    d = bwd_design(case)
    n, dd, c = d["n"], case.D, case.C
    g = {k: d[k].to(dev) for k in ("q", "k", "v", "coords", "sqrt_w", "alpha", "qpos", "kpos", "gacc")}
    ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], g["sqrt_w"], g["alpha"], None, rows_prec)
    _check_rows(case, d, ph)
    rows16 = rows_prec == "bf16"
    tile = torch.bfloat16 if rows16 else torch.float32
    nan = float("nan")
    dq_part = torch.full((TL, n, H, 32), nan, device=dev, dtype=tile)
    dkv_part = torch.full((TL, n, H, 64), nan, device=dev, dtype=tile)
    dims = (n, H, dd, c, TL, case.B) if case.family == "bwd_diff" else (n, H, dd, TL, case.B)
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), entry)(ph["qhat"].data_ptr(), ph["kvhat"].data_ptr(), g["qpos"].data_ptr(),
                                         g["kpos"].data_ptr(), g["gacc"].data_ptr(), *dims, dq_part.data_ptr(),
                                         dkv_part.data_ptr(), ops.current_stream_ptr(dev))
    assert rc == 0, (case.id, rc)
    want_dsw = H * c <= 64          # block_attn_bwd.hip:1102: wider rows leave d sqrt_w to the caller (autograd.py: torch)
    rc, dq, dk, dv, dcs, dsw = ds.bwd_reduce_call(rows16, dq_part, dkv_part, TL, n, H, dd, c, g["coords"], n, want_dsw)
    assert rc == 0, (case.id, rc)
    torch.cuda.synchronize()
    for name, x in (("dq", dq), ("dk", dk), ("dcs", dcs)) + ((("d_sqrt_w", dsw),) if want_dsw else ()):
        bad = ~(x == 0)
        assert not bool(bad.any()), f"{case.id}: {name} must be exactly 0, {int(bad.sum())} elements are not, first at " \
                                    f"{tuple(bad.nonzero()[0].tolist())}: {x[tuple(bad.nonzero()[0].tolist())].item()!r}"
    _same(dv.cpu(), d["dv"], f"{case.id}: dv (point, head x column)")


# ---- float64 cells of the backward: ops.block_attn_bwd on random rows against float64 autograd of the block attention ---
BwdF64Case = namedtuple("BwdF64Case", "id family nkt kind shape")


def _bwd_f64_cases():
    import shape_sweep as sw

    out = []
    for fi, fam in enumerate(BWD_FAMILIES):
        for nkt in range(1, 9):
            for ki, kind in enumerate(("full", "short")):
                d, c = F64_PAIRS[((nkt - 1) * 2 + ki + fi) % len(F64_PAIRS)]
                b = block_of(nkt, kind)
                cid = f"{fam}-k{nkt}{kind}-b{b}-d{d}c{c}-f64"
                out.append(BwdF64Case(cid, fam, nkt, kind, sw.Shape(cid, (4 * b,), b, TL, H, d, c, 8000 + len(out), True)))
    return out


BWD_F64_CASES = _bwd_f64_cases()
BWD_F64_BY_ID = {c.id: c for c in BWD_F64_CASES}


def bwd_f64_cells(fc):
    s = fc.shape
    return bwd_cells(Case(fc.id, fc.family, fc.nkt, fc.kind, s.B, s.D, s.C, "f64", None))


def check_bwd_f64(fc, dev):
    """dq, dk, dv and dcs of ops.block_attn_bwd on random inputs (scaled as shape_sweep.inputs, the GPU's own sorted
    permutations, random upstream rows) against float64 autograd of the oracle's block attention on the float64 rows, per
    row at shape_sweep.BWD_ROW_X / DCOORDS_ROW_X (f32 rows: "fp32", bf16 rows: "bf16").  Returns the measured figures."""
    import hept_oracle as ho
    import shape_sweep as sw
    from hept_amd import ops

    s = fc.shape
    rows_prec = BWD_FAMILIES[fc.family][0]
    f32_mfma = {"bwd_split": False, "bwd_f32mfma": True, "bwd_diff": "diff", "bwd_bf16": False}[fc.family]
    inp = sw._cached((s.id, "inp"), lambda: sw.inputs(s))
    g = sw._cached((s.id, "gpu"), lambda: sw._gpu(inp, dev))
    n = g["q"].shape[0]
    sqrt_w = ops.rpe_scale(g["w_rpe_weight"], s.H, s.D, 10)
    ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sqrt_w, g["alpha"], g["combined_shifts"], rows_prec)
    qpos, kpos = ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"])
    gacc = torch.zeros(n, s.H, 32)
    gacc[..., :s.D + 1] = torch.randn(n, s.H, s.D + 1, generator=torch.Generator().manual_seed(s.seed))
    got = ops.block_attn_bwd(ph["qhat"], ph["kvhat"], qpos, kpos, gacc.to(dev), s.D, s.C, s.B, f32_mfma=f32_mfma)
    torch.cuda.synchronize()
    dq, dk, dv, dcs = (x.cpu() for x in got)
    # float64: the block attention of the float64 rows on the same permutations, summed over the tables
    qp, kp = qpos.long().cpu(), kpos.long().cpu()
    sw64 = ho.rpe_scale(inp["w_rpe_weight"].double(), s.H, s.D, 10)
    heads = lambda x: x.double().reshape(n, s.H, s.D).permute(1, 0, 2)             # noqa: E731
    qf, kf, vf = (heads(inp[x]).clone().requires_grad_(True) for x in ("q", "k", "v"))
    cs = (sw64[None] * inp["coords"].double()[:, None]).permute(1, 0, 2).clone().requires_grad_(True)   # (H, N, C)
    q_hat, k_hat = torch.cat([qf, cs], -1), torch.cat([kf, cs], -1)
    den, num = ho.block_rbf_attention(ho.gather_blocks(q_hat, qp, s.B), ho.gather_blocks(k_hat, kp, s.B),
                                      ho.gather_blocks(vf, kp, s.B))
    num, den = ho.unsort_tables(num, qp).sum(0), ho.unsort_tables(den, qp).sum(0)  # (H, N, D), (H, N, 1)
    g64 = gacc.double().permute(1, 0, 2)
    ((num * g64[..., :s.D]).sum() + (den[..., 0] * g64[..., s.D]).sum()).backward()
    flat = lambda x: x.permute(1, 0, 2).reshape(n, -1)                             # noqa: E731
    want = dict(dq=flat(qf.grad), dk=flat(kf.grad), dv=flat(vf.grad), dcs=cs.grad.permute(1, 0, 2).reshape(n, -1))
    tiles = "bf16" if rows_prec == "bf16" else "fp32"
    fig = {}
    for name, a in (("dq", dq), ("dk", dk), ("dv", dv), ("dcs", dcs.reshape(n, -1))):
        assert bool(torch.isfinite(a).all()), (s.id, name)
        fig[name] = sw.row_x(a, want[name])
    print(f"block sweep {s.id}: worst rows " + ", ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    bad = {k: v for k, v in fig.items() if v > (sw.DCOORDS_ROW_X if k == "dcs" else sw.BWD_ROW_X)[tiles]}
    assert not bad, f"{s.id}: per-row errors over the bound: {bad}"
    return fig
