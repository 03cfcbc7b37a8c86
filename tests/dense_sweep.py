"""Deterministic sweep of the dense stage kernels around the attention path (run by tests/test_gpu_dense_sweep.py, coverage
pinned on CPU by tests/test_dense_sweep_cells.py): csrc/block_train.hip, the table sum, the combine and its backward in
csrc/combine.hip, bwd_reduce / dsw in csrc/block_attn_bwd.hip and rpe_scale{,_bwd} in csrc/prep_hash.hip.

Two kinds of check.  EXACT: whatever is a sum of products gets small integers (activations, gradients, weights in -3..3,
denominators 1, 2 or 4, numerators integer multiples of their denominator, all of them bf16 values), so that every
product and every partial sum is an integer below 2^24 and the float32 result is the same in any summation order; the
kernel must then equal the float64 result bit for bit -- one dropped, doubled or misplaced point fails.  ``bounds(case)``
gives the magnitude chain of every exact case, asserted on the CPU.  F64: what is not a sum of products (LayerNorm, the
feed-forward, rpe_scale) and one random-valued case per exact kernel are held to float64: per-point outputs to the
atol / rtol the older tests use for them, reduced outputs per element to X * sum_n |term_n| (the sum of magnitudes in
float64: the bound follows the conditioning of each entry and has no absolute floor), with X at <= 2x the worst value
measured over this sweep on the MI355X; torch's own float32 evaluation of the same expression is measured beside it.

``cells(case)`` names the branches a case takes, mirroring the rules in csrc/.  Nothing here touches the GPU at import."""
import zlib
from collections import namedtuple

import torch

Case = namedtuple("Case", "id kernel check a")   # check: "exact" | "f64"; a: the kernel's own sizes
LIMIT = 2 ** 24                                  # integers below it are float32 values
EPS = 1e-5

# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
WG_N = (1, 2, 15, 16, 17, 127, 128, 129, 2047, 2048, 2049, 131200)
WG_O = (1, 24, 31, 32, 33, 72, 191, 192, 193, 384, 400)
LN_N = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 66000)
LN_EDGES = ("const", "mean1e4", "w1zero")       # at N = 257
LN_KERNELS = ("ln_bwd", "ln_ffn_fwd", "ln_ffn_bwd")
CB_N = (1, 127, 128, 129, 2047, 2048, 2049)
CB_TUNED_H = (1, 2, 3, 5, 7, 8)
CB_GENERIC = ((9, 24), (16, 24), (16, 27), (11, 26), (5, 20), (8, 16), (12, 8), (1, 1))
CB_STRIDE = ((131200, 8, 24), (65700, 16, 24))
RT_T = (1, 2, 3, 8, 9)
RT_FORMS = ("f32-d1", "f32-d24", "f32-d28", "packed-f32", "packed-packed")
RT_SMALL = ((1, 1), (127, 1), (16, 8), (43, 3))                  # (N, H): N * H = 1, 127, 128, 129
RT_BIG = ((65536, 8), (524289, 1))                               # N * H = 524 288 (the grid exactly full), 524 289
RT_STRIDE = (65600, 8, 2)
CO_COUNTS = (1, 31, 32, 33, 32736, 32767, 32768, 32769, 262144, 262200)
CO_HEADS24 = (8, 7, 16, 1)
CO_GENERIC = ((5, 20), (16, 27), (1, 1))
CO_T = (1, 3, 4)
CO_SLICES = ((0, 129), (32, 50), (45, 33), (128, 1))             # of N = 129
CF_COUNTS = (1, 33, 32768, 262200)
BR_N = (1, 255, 256, 257, 4095, 4096, 4097)
BR_T = (1, 3)
BR_SHAPES = ((1, 24, 2), (8, 24, 6), (9, 8, 7), (16, 16, 4), (5, 21, 5))   # (H, D, C): H * C = 2, 48, 63, 64; odd D
RPE_TERMS = ((1, 2, 1), (11, 4, 31), (16, 5, 16))                # (H, C, K): H (C - 1) K = 1, 1023, 1024
RPE_D = (1, 7, 8, 9, 27)

# per-table denominators in {1, 2, 4} whose sum is a power of two, with an integer vector e, sum_t den_t e_t = 0: the
# numerators den_t * (k + r e_t) sum to (sum den) * k, so the combine's quotient is the integer k exactly
PATTERNS = {
    1: (((1,), (0,)), ((2,), (0,)), ((4,), (0,))),
    3: (((1, 1, 2), (1, 1, -1)), ((2, 1, 1), (-1, 1, 1)), ((2, 2, 4), (1, 1, -1)), ((4, 2, 2), (-1, 1, 1)),
        ((1, 2, 1), (1, -1, 1))),
    4: (((1, 1, 1, 1), (1, -1, 1, -1)), ((2, 2, 2, 2), (1, 1, -1, -1)), ((4, 4, 4, 4), (1, -1, -1, 1)),
        ((1, 1, 2, 4), (2, 0, 1, -1)), ((4, 2, 1, 1), (-1, 1, 2, 0))),
}
K_MAX, R_MAX = 3, 2          # |k| <= 3, |r| <= 2: |numerator| <= 4 * (3 + 2 * 2) = 28, a bf16 value


def _build():
    out = []

    def add(cid, kernel, check, *a):
        if all(c.id != cid for c in out):        # (two axes of a table may meet in one case)
            out.append(Case(cid, kernel, check, tuple(a)))

    # rows_wgrad: every N with O in {24, 192}, every O with N in {129, 2049}
    pairs = [(n, o) for n in WG_N for o in (24, 192)] + [(n, o) for o in WG_O for n in (129, 2049)]
    for n, o in dict.fromkeys(pairs):
        add(f"wgrad-n{n}-o{o}", "rows_wgrad", "exact", n, o)
    add("wgrad-n2049-o193-rand", "rows_wgrad", "f64", 2049, 193)
    add("wgrad-n131200-o24-rand", "rows_wgrad", "f64", 131200, 24)
    # LayerNorm backward, feed-forward forward and backward
    for kern in LN_KERNELS:
        for n in LN_N:
            add(f"{kern}-n{n}", kern, "f64", n, None)
        for edge in LN_EDGES:
            if not (kern == "ln_bwd" and edge == "w1zero"):      # (norm1's backward has no feed-forward weights)
                add(f"{kern}-n257-{edge}", kern, "f64", 257, edge)
    # combine backward
    for n in CB_N:
        for h in CB_TUNED_H:
            add(f"cbwd-n{n}-h{h}d24", "combine_bwd", "exact", n, h, 24)
        for h, d in CB_GENERIC:
            add(f"cbwd-n{n}-h{h}d{d}", "combine_bwd", "exact", n, h, d)
    for n, h, d in CB_STRIDE:
        add(f"cbwd-n{n}-h{h}d{d}", "combine_bwd", "exact", n, h, d)
    add("cbwd-n2049-h8d24-rand", "combine_bwd", "f64", 2049, 8, 24)
    add("cbwd-n2049-h16d27-rand", "combine_bwd", "f64", 2049, 16, 27)
    # reduce_tables: the small row counts with every table count and form; the grid-filling ones with two tables
    for form in RT_FORMS:
        for n, h in RT_SMALL:
            for t in RT_T:
                add(f"rt-{form}-t{t}-n{n}h{h}", "reduce_tables", "exact", t, n, h, form)
        for n, h in RT_BIG:
            add(f"rt-{form}-t2-n{n}h{h}", "reduce_tables", "exact", 2, n, h, form)
        n, h, t = RT_STRIDE
        add(f"rt-{form}-t{t}-n{n}h{h}", "reduce_tables", "exact", t, n, h, form)
        add(f"rt-{form}-t3-n43h3-rand", "reduce_tables", "f64", 3, 43, 3, form)
    # combine_out on synthetic rows
    for rows in ("f32", "packed"):
        for cnt in CO_COUNTS:
            add(f"co-{rows}-t1-h8d24-n{cnt}", "combine_out", "exact", 1, cnt, 8, 24, rows, 0, cnt)
        for h in CO_HEADS24:
            for t in CO_T:
                add(f"co-{rows}-t{t}-h{h}d24-n33", "combine_out", "exact", t, 33, h, 24, rows, 0, 33)
            add(f"co-{rows}-t3-h{h}d24-n32769", "combine_out", "exact", 3, 32769, h, 24, rows, 0, 32769)
        add(f"co-{rows}-t4-h8d24-n32769", "combine_out", "exact", 4, 32769, 8, 24, rows, 0, 32769)
        for n0, cnt in CO_SLICES:
            add(f"co-{rows}-t3-h8d24-n129-slice{n0}+{cnt}", "combine_out", "exact", 3, 129, 8, 24, rows, n0, cnt)
        add(f"co-{rows}-t3-h8d24-n1057-rand", "combine_out", "f64", 3, 1057, 8, 24, rows, 0, 1057)
    for h, d in CO_GENERIC:
        for t in CO_T:
            add(f"co-f32-t{t}-h{h}d{d}-n33", "combine_out", "exact", t, 33, h, d, "f32", 0, 33)
        add(f"co-f32-t3-h{h}d{d}-n32769", "combine_out", "exact", 3, 32769, h, d, "f32", 0, 32769)
        for n0, cnt in CO_SLICES[1:]:
            add(f"co-f32-t3-h{h}d{d}-n129-slice{n0}+{cnt}", "combine_out", "exact", 3, 129, h, d, "f32", n0, cnt)
    add("co-f32-t3-h16d27-n1057-rand", "combine_out", "f64", 3, 1057, 16, 27, "f32", 0, 1057)
    # combine_ffn (f32 rows, H = 8, D = 24)
    for cnt in CF_COUNTS:
        t = 1 if cnt > 100000 else 3
        add(f"cffn-t{t}-n{cnt}", "combine_ffn", "f64", t, cnt, 0, cnt)
    add("cffn-t3-n129-slice45+33", "combine_ffn", "f64", 3, 129, 45, 33)
    # bwd_reduce / bwd_reduce16 with d_sqrt_w (each case walks raw_size in {N, N - 1, 1, 0})
    for rows16 in (False, True):
        tag = "br16" if rows16 else "br"
        for h, d, c in BR_SHAPES:
            for n in BR_N:
                for t in BR_T:
                    add(f"{tag}-n{n}-t{t}-h{h}d{d}c{c}", "bwd_reduce", "exact", rows16, n, t, h, d, c)
        add(f"{tag}-n4097-t3-h8d24c6-rand", "bwd_reduce", "f64", rows16, 4097, 3, 8, 24, 6)
    # rpe_scale and its backward
    for h, c, k in RPE_TERMS:
        for d in RPE_D:
            add(f"rpe-h{h}c{c}k{k}-d{d}", "rpe_scale", "f64", h, c, k, d, None)
    add("rpe-h8c6k10-d24-clamp", "rpe_scale", "f64", 8, 6, 10, 24, "clamp")
    add("rpe-h2c3k4-d2-at50", "rpe_scale", "f64", 2, 3, 4, 2, "at50")
    add("rpe-h1c2k1025-d1-refused", "rpe_scale", "f64", 1, 2, 1025, 1, "refused")
    return out


CASES = _build()
BY_ID = {c.id: c for c in CASES}


def of_kernel(kernel, check=None):
    return [c for c in CASES if c.kernel == kernel and (check is None or c.check == check)]


# ---------------------------------------------------------------------------------------------------------------------
# the branches a case takes
# ---------------------------------------------------------------------------------------------------------------------
FSUM_SLICES = 16                   # csrc/common.h:66 HEPT_FSUM_SLICES
GRID_CAP = 4096                    # csrc/combine.hip:887,1113,1121: blocks < 4096 ? blocks : 4096
CMB_SPLIT_BELOW, CMB_MAX_WGS, CMB_WAVES = 1024, 2048, 4      # csrc/combine.hip:929,970,23


def _fsum(n_parts):
    """hept_fixed_sum (csrc/common.h:72): slice s takes g = s, s + 16, ...; more than 16 parts is a slice wrapping."""
    return "fsum-slices-wrap" if n_parts > FSUM_SLICES else "fsum-one-trip"


def dsw_refused(rows16, n, t, h):
    """csrc/block_attn_bwd.hip:1105: the per-workgroup d_sqrt_w sums reuse dq_part; a cloud too small for them is
    refused."""
    return -(-n // 256) * 64 * 4 > t * n * h * 32 * (2 if rows16 else 4)


def combine_bwd_tuned(h, d):
    return d == 24 and h <= 8      # csrc/combine.hip:1090


def cells(case):
    k, a = case.kernel, case.a
    out = {f"{k}:{case.check}"}
    if k == "rows_wgrad":
        n, o = a
        cols, groups = (192, 4) if o > 32 else (32, 16)                        # csrc/block_train.hip:356-362
        wgs = -(-n // 128)                                                     # :350 BT_POINTS
        out |= {f"wgrad-cols{cols}x{groups}", f"wgrad-grid-rows{-(-o // cols)}",          # :358
                "wgrad-dead-cols" if o % cols else "wgrad-cols-full",          # :43 live
                "wgrad-points-ragged" if n % 128 else "wgrad-points-full",     # :44 n_end
                _fsum(wgs), f"wgrad-wgs{wgs}" if wgs in (1, 16, 17) else "wgrad-wgs-many"}
        if n < groups:
            out.add("wgrad-idle-groups")                                       # :52 a thread group without a point
        if (n % 128) % (groups * 4):
            out.add("wgrad-unroll-tail")                                       # :57 n < n_end inside the 4-point unroll
    elif k in LN_KERNELS:
        n, edge = a
        wgs = -(-n // 256)                                                     # csrc/block_train.hip:195,351
        out |= {"ln-rows-ragged" if n % 256 else "ln-rows-full",               # :209,:297 valid
                "ln-wave-ragged" if n % 64 else "ln-wave-full", _fsum(wgs),    # :182 wave_sum of valid lanes; :405,:448
                f"ln-wgs{wgs}" if wgs in (1, 16, 17) else "ln-wgs-many"}
        if wgs * 256 - n >= 64:
            out.add("ln-idle-waves")
        if edge:
            out.add(f"ln-edge-{edge}")
    elif k == "combine_bwd":
        n, h, d = a
        wgs = -(-n // 128)                                                     # csrc/combine.hip:718,1109 CBW_POINTS
        out |= {"cb-tuned" if combine_bwd_tuned(h, d) else "cb-generic",       # :1111
                "cb-rows-grid-stride" if -(-n * h // 256) > GRID_CAP else "cb-rows-one-trip",      # :1108,:674,:811
                "cb-points-ragged" if n % 128 else "cb-points-full", _fsum(wgs)}
        if combine_bwd_tuned(h, d):
            out.add("cb-tuned-dead-cols" if h * d < 192 else "cb-tuned-cols-full")        # :733 live
            out.add(f"cb-tuned-h{h}")
        else:
            out.add("cb-generic-col-loop-2" if h * d > 256 else "cb-generic-col-loop-1")  # :840
            out.add(f"cb-generic-h{h}d{d}")
    elif k == "reduce_tables":
        t, n, h, form = a
        blocks = -(-n * h * 2 // 256)                                          # csrc/combine.hip:886
        out |= {f"rt-{form}", f"rt-tables{t}", f"rt-rows{n * h}" if n * h < 1000 else "rt-rows-many",
                "rt-grid-stride" if blocks > GRID_CAP else "rt-grid-full" if blocks == GRID_CAP else "rt-one-trip",
                "rt-block-ragged" if n * h * 2 % 256 else "rt-block-full"}                # (:887 the grid, :577 the loop)
    elif k in ("combine_out", "combine_ffn"):
        if k == "combine_ffn":
            (t, n, n0, cnt), h, d, rows = a, 8, 24, "f32"
        else:
            t, n, h, d, rows, n0, cnt = a
        tiles = -(-cnt // 32)                                                  # csrc/combine.hip:947
        if tiles < CMB_SPLIT_BELOW:                                            # :948
            out.add("co-split")
            if tiles == CMB_SPLIT_BELOW - 1:
                out.add("co-split-last")
        else:
            wgs = -(-tiles // CMB_WAVES)                                       # :968
            out.add("co-flat-striding" if wgs > CMB_MAX_WGS else "co-flat-grid-full" if wgs == CMB_MAX_WGS
                    else "co-flat")                                            # :972 the grid, :208,:294 the step
            if tiles == CMB_SPLIT_BELOW:
                out.add("co-flat-first")
            if tiles % CMB_WAVES:
                out.add("co-flat-idle-waves")                                  # :202 tile_first >= n_tiles
        staged = d == 24 and h % 2 == 0                                        # :988-989
        out |= {"co-tile-ragged" if cnt % 32 else "co-tile-full", "co-staged" if staged else "co-lanes",
                f"co-dt{d}" if d in (24, 16) else "co-dt-generic", f"co-rows-{rows}", f"co-tables{t}",   # :1009-1016
                f"co-h{h}d{d}"}
        if staged and t > 3:
            out.add("co-staged-tables-wrap")                                   # :122 three tables in flight
        if n0 > 0:
            out.add("co-slice-n0")
        if n0 + cnt < n:
            out.add("co-slice-short")
        if (n0, cnt) == (n - 1, 1) and n > 1:
            out.add("co-slice-last-point")
    elif k == "bwd_reduce":
        rows16, n, t, h, d, c = a
        threads = n * h * (16 if rows16 else 32)                               # csrc/block_attn_bwd.hip:1111,1115
        wgs = -(-n // 256)                                                     # :905 DSW_POINTS
        out |= {"br-rows16" if rows16 else "br-rows32", f"br-tables{t}", f"dsw-lanes{h * c}",          # :912 lane < HC
                "br-block-ragged" if threads % 256 else "br-block-full",
                "dsw-points-ragged" if n % 256 else "dsw-points-full", _fsum(wgs),
                "dsw-refused" if dsw_refused(rows16, n, t, h) else "dsw-kernel"}
        if rows16 and d % 2:
            out.add("br16-odd-d")                                              # :865 a column pair astride D
        if (n % 256) % 32:
            out.add("dsw-unroll-tail")                                         # :920 n < n_end inside the 8-point unroll
    elif k == "rpe_scale":
        h, c, kk, d, edge = a
        terms = h * (c - 1) * kk                                               # csrc/prep_hash.hip:823
        out |= {f"rpe-terms{terms}", "rpe-d<8" if d < 8 else "rpe-d8" if d == 8 else "rpe-d>8",     # :43 unroll 8
                "rpe-refused" if terms > 1024 else "rpe-runs"}
        if edge:
            out.add(f"rpe-edge-{edge}")
    return out


def bounds(case):
    """Magnitude chain of an exact case: (what, max |a|, max |b|, number of terms); each product stays below 2^24."""
    k, a = case.kernel, case.a
    assert case.check == "exact"
    if k == "rows_wgrad":
        n, _ = a
        return [("d_weight", 3, 3, n), ("d_bias", 3, 1, n)]
    if k == "combine_bwd":
        n, h, d = a
        # per_head = numer / den = k, |k| <= 3; |numer| <= 12; dph = sum_c W g; dot = sum_j dph_j numer_j
        return [("dph", 3, 3, d), ("dot", 9 * d, 12, d), ("d_weight", 3, 3, n), ("d_bias", 3, 1, n)]
    if k == "reduce_tables":
        t = a[0]
        return [("numerators", 3, 1, t), ("denominator", 4, 1, t)]
    if k == "combine_out":
        t, _, h, d = a[:4]
        num = 4 * (K_MAX + R_MAX * 2)
        return [("numerators", num, 1, t), ("denominator", 4, 1, t),
                ("linear", K_MAX, 3, h * d), ("linear + bias", K_MAX * 3 * h * d + 3, 1, 1)]
    if k == "bwd_reduce":
        _, n, t, h, d, c = a
        return [("table sum", 3, 1, t), ("dcs", 3 * t, 1, 2), ("d_sqrt_w", 6 * t, 3, n)]
    raise KeyError(k)


# ---------------------------------------------------------------------------------------------------------------------
# float64 references (plain torch; run on whatever device the inputs live on)
# ---------------------------------------------------------------------------------------------------------------------
def ln_parts(x, eps):
    """LayerNorm(24) as torch computes it (biased variance, eps inside the root): xhat and rstd."""
    xc = x - x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    return xc * rstd, rstd


def ffn_terms(x, go, lw, lb, w1, b1, w2, b2, eps=EPS):
    """The rows the feed-forward backward multiplies (all in the dtype of ``x``): xhat, z = norm2(x), a = ff.0(z),
    h = relu(a), dh = d a, dz = d z."""
    xhat, rstd = ln_parts(x, eps)
    z = xhat * lw + lb
    a = z @ w1.t() + b1
    h = a.clamp_min(0)
    dh = (go @ w2) * (a > 0)
    dz = dh @ w1
    return dict(xhat=xhat, rstd=rstd, z=z, a=a, h=h, dh=dh, dz=dz)


def ffn_forward(x, lw, lb, w1, b1, w2, b2, eps=EPS):
    import torch.nn.functional as F

    return F.linear(F.relu(F.linear(F.layer_norm(x, (x.shape[-1],), lw, lb, eps), w1, b1)), w2, b2)


def ffn_grads(x, go, lw, lb, w1, b1, w2, b2, eps=EPS):
    """torch autograd of ff.2(relu(ff.0(norm2(x)))) in the dtype of ``x``: gradients in ops.ln_ffn_bwd's order."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, lw, lb, w1, b1, w2, b2)]
    ffn_forward(*leaves, eps=eps).backward(go)
    return [t.grad for t in leaves]


def ffn_magnitudes(x, go, lw, lb, w1, b1, w2, b2, eps=EPS):
    """sum_n |term_n| of every reduced output of ops.ln_ffn_bwd, in its order (d_ln_w, d_ln_b, d_w1, d_b1, d_w2, d_b2)."""
    p = ffn_terms(x, go, lw, lb, w1, b1, w2, b2, eps)
    return [(p["dz"] * p["xhat"]).abs().sum(0), p["dz"].abs().sum(0), p["dh"].abs().t() @ p["z"].abs(),
            p["dh"].abs().sum(0), go.abs().t() @ p["h"].abs(), go.abs().sum(0)]


def ln_grads(x, dxn, lw, lb, eps=EPS):
    """torch autograd of LayerNorm in the dtype of ``x``: (dx, xn, d_ln_w, d_ln_b) as ops.ln_bwd returns them."""
    import torch.nn.functional as F

    leaves = [t.detach().clone().requires_grad_(True) for t in (x, lw, lb)]
    xn = F.layer_norm(leaves[0], (x.shape[-1],), leaves[1], leaves[2], eps)
    xn.backward(dxn)
    return leaves[0].grad, xn.detach(), leaves[1].grad, leaves[2].grad


def rpe_formula(w, h, d, k):
    """sqrt(2 sum_k exp(min(sum_d w, 50))) with column 0 duplicated (hept_amd.autograd.rpe_scale_torch's formula)."""
    qw = w.reshape(h, d, -1, k).sum(dim=1).clamp(max=50).exp().sum(dim=-1)
    return torch.sqrt(2 * torch.cat([qw[:, :1], qw], dim=-1))


def combine_reference(wide, d, w, b, n0, cnt, chunk=65536):
    """float64 (sum_t numer / sum_t denom) -> Linear over points [n0, n0 + cnt) of wide f32 rows (T, N, H, 32)."""
    outs = []
    w64, b64 = w.double(), None if b is None else b.double()
    for i0 in range(n0, n0 + cnt, chunk):
        s = wide[:, i0:min(i0 + chunk, n0 + cnt)].double().sum(0)
        ph = (s[..., :d] / s[..., d:d + 1]).reshape(s.shape[0], -1)
        o = ph @ w64.t()
        outs.append(o if b64 is None else o + b64)
    return torch.cat(outs)


def pack_rows(wide):
    """f32 rows (..., 32) of head dimension 24 as packed rows (..., 16) int32: 24 bf16 numerators (torch's own rounding),
    the f32 denominator in dword 12, zeros."""
    out = torch.zeros(*wide.shape[:-1], 16, dtype=torch.int32, device=wide.device)
    out[..., :12] = wide[..., :24].to(torch.bfloat16).contiguous().view(torch.int32)
    out[..., 12] = wide[..., 24].contiguous().view(torch.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# GPU checks
# ---------------------------------------------------------------------------------------------------------------------
# Per-point outputs: (atol, rtol) on every element against float64, the values the older tests use against torch
# (tests/test_gpu_attn_block.py test_block_train_kernels_match_torch_autograd, test_combine_ffn_epilogue;
# tests/test_gpu_backward.py test_combine_backward_kernel_vs_autograd).  "*scale": atol is that multiple of max |ref|.
# Measured worst element, as a multiple of the tolerance (torch float32 on the same inputs): ln_bwd.xn 0.022 (0.052),
# ln_bwd.dx 0.33 (0.55), ln_ffn_fwd.out 0.045 (0.042), ln_ffn_bwd.d_x1 0.78 (1.10) -- both at the constant rows, where
# rstd = 1 / sqrt(eps) = 316 --, combine_bwd.gacc_numer 0.107 (0.107), gacc_den 0.012 (0.0073), combine_out.out 0.101
# (0.107), combine_ffn.y 0.023 (0.019).  The rows of mean 1e4 and spread 1e-2: xn 0.015, dx 0.18, d_x1 0.34, out 0.019 --
# torch float32 misses them by 4e4 to 2.6e6 tolerances, as this project's one-step row mean did (csrc/block_train.hip
# ln_stats).
POINT_TOL = {
    "ln_bwd.xn": (1e-5, 1e-5), "ln_bwd.dx": (2e-5, 1e-4), "ln_ffn_fwd.out": (1e-5, 1e-4), "ln_ffn_bwd.d_x1": (2e-5, 1e-4),
    "combine_bwd.gacc_numer": (1e-5, 1e-4), "combine_bwd.gacc_den": ("2e-5*scale", 0.0), "combine_out.out": (1e-5, 1e-5),
    "combine_ffn.y": ("2e-5*scale", 2e-5),
}
# Reduced outputs: per element |got - float64| <= X * sum |term| (float64), X at <= 2x the measured worst of the sweep on
# the MI355X.  Beside each: that worst value, torch float32's figure for the same case, and the case.  (With one term
# -- N = 1 -- the figure is the relative error of the term itself: the feed-forward gradients' worst cases.  The packed
# table sum rounds its numerators to bf16 again: its figure is bf16's unit round-off 2^-8 = 3.9e-3.  rpe_scale's "sum of
# magnitudes" is the value times 1 + sum_d |w|: exp turns the round-off of a column sum into a relative error.)
SUM_X = {
    "rows_wgrad.d_weight": 4.2e-08,     # 2.143e-08  torch 1.728e-07  wgrad-n2049-o193-rand
    "rows_wgrad.d_bias": 2.5e-08,       # 1.259e-08  torch 1.225e-08  wgrad-n2049-o193-rand
    "ln_bwd.d_ln_w": 1.6e-07,           # 8.391e-08  torch 1.502e-07  ln_bwd-n1
    "ln_bwd.d_ln_b": 4.6e-08,           # 2.308e-08  torch 6.008e-08  ln_bwd-n65
    "ln_ffn_bwd.d_ln_w": 4.4e-06,       # 2.232e-06  torch 2.255e-06  ln_ffn_bwd-n1
    "ln_ffn_bwd.d_ln_b": 4.2e-06,       # 2.147e-06  torch 3.531e-07  ln_ffn_bwd-n1
    "ln_ffn_bwd.d_w1": 3.5e-06,         # 1.754e-06  torch 2.513e-06  ln_ffn_bwd-n1
    "ln_ffn_bwd.d_b1": 3.1e-06,         # 1.593e-06  torch 2.349e-06  ln_ffn_bwd-n1
    "ln_ffn_bwd.d_w2": 9.7e-07,         # 4.895e-07  torch 2.232e-02  ln_ffn_bwd-n257-const
    "ln_ffn_bwd.d_b2": 9.0e-08,         # 4.525e-08  torch 4.043e-08  ln_ffn_bwd-n63
    "combine_bwd.d_weight": 1.7e-07,    # 8.728e-08  torch 4.509e-07  cbwd-n2049-h16d27-rand
    "combine_bwd.d_bias": 3.5e-08,      # 1.761e-08  torch 7.000e-09  cbwd-n2049-h16d27-rand
    "reduce_tables.f32": 1.7e-07,       # 8.865e-08  torch 8.865e-08  rt-packed-f32-t3-n43h3-rand
    "reduce_tables.packed": 4.0e-03,    # 3.891e-03  torch 3.891e-03  rt-packed-packed-t3-n43h3-rand
    "bwd_reduce.dq": 2.2e-07,           # 1.148e-07  torch 1.148e-07  br-n4097-t3-h8d24c6-rand
    "bwd_reduce.dk": 2.3e-07,           # 1.159e-07  torch 1.159e-07  br-n4097-t3-h8d24c6-rand
    "bwd_reduce.dv": 2.3e-07,           # 1.157e-07  torch 1.157e-07  br-n4097-t3-h8d24c6-rand
    "bwd_reduce.dcs": 2.5e-07,          # 1.275e-07  torch 1.275e-07  br-n4097-t3-h8d24c6-rand
    "bwd_reduce.d_sqrt_w": 1.2e-07,     # 6.359e-08  torch 6.359e-08  br-n4097-t3-h8d24c6-rand
    "rpe_scale.sqrt_w": 1.7e-07,        # 8.896e-08  torch 5.729e-08  rpe-h16c5k16-d1
    "rpe_scale.d_w": 2.6e-07,           # 1.320e-07  torch 9.644e-08  rpe-h11c4k31-d1
}
ILL_PRE = 1e-4    # a pre-activation of ff.0 nearer to zero than this could fall on the other side of the ReLU in float32


def _gen(case, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(zlib.crc32(case.id.encode()))
    return g


def _ints(shape, g, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g, device=g.device).float()


def _randn(shape, g):
    return torch.randn(shape, generator=g, device=g.device)


def _dens(shape, g):
    return (2 ** torch.randint(0, 3, shape, generator=g, device=g.device)).float()


def _ratio(got, ref, mag):
    """Worst |got - ref| / mag; an entry whose sum of magnitudes is zero must be exact."""
    err = (got.double() - ref).abs()
    inf = torch.full_like(err, float("inf"))
    return float(torch.where(mag > 0, err / mag.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf)).max())


def _tol(key, got, ref):
    """Worst element as a multiple of the per-point tolerance."""
    atol, rtol = POINT_TOL[key]
    if isinstance(atol, str):
        atol = float(atol.split("*")[0]) * float(ref.abs().max())
    return float(((got.double() - ref).abs() / (atol + rtol * ref.abs())).max())


def _exact(got, ref64, what, case):
    assert torch.equal(got, ref64.to(torch.float32)), \
        f"{case.id}: {what} differs from the exact sum at {int((got != ref64.float()).sum())} of {got.numel()} elements"


class Figures(dict):
    """key -> (this project's figure, torch float32's figure or None)."""

    def put(self, key, ours, torch32):
        a, b = self.get(key, (0.0, 0.0))
        self[key] = (max(a, ours), max(b, torch32))


def _m_rows_wgrad(case, dev, fig):
    from hept_amd import ops

    n, o = case.a
    g = _gen(case, dev)
    dy, x = (_ints((n, o), g), _ints((n, 24), g)) if case.check == "exact" else (_randn((n, o), g), _randn((n, 24), g))
    dw, db = ops.rows_wgrad(dy, x, need_bias=True)
    assert torch.equal(ops.rows_wgrad(dy, x), dw), case.id        # without the bias: the same weight gradient
    ref_w, ref_b = dy.double().t() @ x.double(), dy.double().sum(0)
    if case.check == "exact":
        _exact(dw, ref_w, "d_weight", case)
        _exact(db, ref_b, "d_bias", case)
        return
    mag_w, mag_b = dy.double().abs().t() @ x.double().abs(), dy.double().abs().sum(0)
    fig.put("rows_wgrad.d_weight", _ratio(dw, ref_w, mag_w), _ratio(dy.t() @ x, ref_w, mag_w))
    fig.put("rows_wgrad.d_bias", _ratio(db, ref_b, mag_b), _ratio(dy.sum(0), ref_b, mag_b))


def _ln_inputs(case, g, ffn):
    """x (N, 24) and the parameters; the rows whose ff.0 pre-activations (float64) come nearer to zero than ILL_PRE are
    drawn again (the feed-forward backward only: d relu is discontinuous there, in any precision)."""
    n, edge = case.a

    def rows(m):
        if edge == "const":      # small integers: the row mean is exact, so the variance is exactly 0
            return _ints((m, 1), g).expand(m, 24).contiguous()
        if edge == "mean1e4":
            return 1e4 + 1e-2 * _randn((m, 24), g)
        return _randn((m, 24), g)

    x = rows(n)
    lw, lb = _randn((24,), g) * 0.3 + 1.0, _randn((24,), g) * 0.1
    w1, w2 = _randn((24, 24), g) * 0.2, _randn((24, 24), g) * 0.2
    b1, b2 = _randn((24,), g) * 0.1, _randn((24,), g) * 0.1
    if edge == "w1zero":
        w1, b1 = torch.zeros_like(w1), torch.zeros_like(b1)
    elif ffn:
        for _ in range(20):
            xhat, _r = ln_parts(x.double(), EPS)
            a = (xhat * lw.double() + lb.double()) @ w1.double().t() + b1.double()
            ill = (a.abs() < ILL_PRE).any(-1)
            if not bool(ill.any()):
                break
            assert edge != "const", f"{case.id}: constant rows share one ill-conditioned pre-activation: another seed"
            x[ill] = rows(int(ill.sum()))
        else:
            raise AssertionError(f"{case.id}: ill-conditioned rows remain")
    return x, (lw, lb, w1, b1, w2, b2)


def _m_ln_bwd(case, dev, fig):
    from hept_amd import ops

    g = _gen(case, dev)
    x, (lw, lb, *_) = _ln_inputs(case, g, ffn=False)
    dxn = _randn(tuple(x.shape), g)
    got = ops.ln_bwd(x, dxn, lw, lb, EPS)
    assert all(torch.equal(a, b) for a, b in zip(ops.ln_bwd(x, dxn, lw, lb, EPS), got)), case.id   # fixed association
    ref = ln_grads(x.double(), dxn.double(), lw.double(), lb.double())
    t32 = ln_grads(x, dxn, lw, lb)
    xhat, _r = ln_parts(x.double(), EPS)
    mags = (None, None, (dxn.double() * xhat).abs().sum(0), dxn.double().abs().sum(0))
    for name, a, r, t, m in zip(("dx", "xn", "d_ln_w", "d_ln_b"), got, ref, t32, mags):
        assert bool(torch.isfinite(a).all()), (case.id, name)
        if m is None:
            fig.put(f"ln_bwd.{name}", _tol(f"ln_bwd.{name}", a, r), _tol(f"ln_bwd.{name}", t, r))
        else:
            fig.put(f"ln_bwd.{name}", _ratio(a, r, m), _ratio(t, r, m))
    if case.a[1] == "const":     # xhat is exactly 0: the rows are the bias, the weight gradient is 0
        assert torch.equal(got[1], lb.expand_as(x)) and float(got[2].abs().max()) == 0.0, case.id


def _m_ln_ffn_fwd(case, dev, fig):
    from hept_amd import ops

    g = _gen(case, dev)
    x, p = _ln_inputs(case, g, ffn=False)
    out = ops.ln_ffn_fwd(x, p[0], p[1], EPS, *p[2:])
    ref = ffn_forward(x.double(), *(t.double() for t in p))
    assert bool(torch.isfinite(out).all()), case.id
    fig.put("ln_ffn_fwd.out", _tol("ln_ffn_fwd.out", out, ref), _tol("ln_ffn_fwd.out", ffn_forward(x, *p), ref))
    if case.a[1] == "w1zero":    # relu(0) = 0: the output is ff.2's bias
        assert torch.equal(out, p[5].expand_as(out)), case.id


def _m_ln_ffn_bwd(case, dev, fig):
    from hept_amd import ops

    g = _gen(case, dev)
    x, p = _ln_inputs(case, g, ffn=True)
    go = _randn(tuple(x.shape), g)
    got = ops.ln_ffn_bwd(x, go, p[0], p[1], EPS, *p[2:])
    assert all(torch.equal(a, b) for a, b in zip(ops.ln_ffn_bwd(x, go, p[0], p[1], EPS, *p[2:]), got)), case.id
    p64 = [t.double() for t in p]
    ref = ffn_grads(x.double(), go.double(), *p64)
    t32 = ffn_grads(x, go, *p)
    mags = [None] + ffn_magnitudes(x.double(), go.double(), *p64)
    names = ("d_x1", "d_ln_w", "d_ln_b", "d_w1", "d_b1", "d_w2", "d_b2")
    for name, a, r, t, m in zip(names, got, ref, t32, mags):
        assert bool(torch.isfinite(a).all()), (case.id, name)
        if m is None:
            fig.put(f"ln_ffn_bwd.{name}", _tol(f"ln_ffn_bwd.{name}", a, r), _tol(f"ln_ffn_bwd.{name}", t, r))
        else:
            fig.put(f"ln_ffn_bwd.{name}", _ratio(a, r, m.reshape(r.shape)), _ratio(t, r, m.reshape(r.shape)))
    if case.a[1] == "w1zero":    # every pre-activation is exactly 0 and relu'(0) = 0, in torch and here
        for name, a in zip(names[:6], got[:6]):
            assert float(a.abs().max()) == 0.0, (case.id, name)


def _m_combine_bwd(case, dev, fig):
    from hept_amd import ops

    n, h, d = case.a
    g = _gen(case, dev)
    acc = torch.zeros(n, h, 32, device=dev)
    if case.check == "exact":
        den = _dens((n, h), g)
        acc[..., :d] = _ints((n, h, d), g) * den[..., None]
        acc[..., d] = den
        w, b, g_out = _ints((d, h * d), g), _ints((d,), g), _ints((n, d), g)
    else:   # as tests/test_gpu_backward.py test_combine_backward_kernel_vs_autograd draws them
        acc[..., :d] = _randn((n, h, d), g)
        acc[..., d] = torch.rand(n, h, generator=g, device=dev) * 3 + 0.05
        w, b, g_out = _randn((d, h * d), g) * 0.1, _randn((d,), g), _randn((n, d), g)
    gacc, dw, db = ops.combine_bwd(acc, g_out, w, need_bias=True)
    gacc2, dw2, none = ops.combine_bwd(acc, g_out, w, need_bias=False)
    assert none is None and torch.equal(gacc2, gacc) and torch.equal(dw2, dw), case.id
    numer, den = acc[..., :d].double(), acc[..., d:d + 1].double()
    dph = (g_out.double() @ w.double()).reshape(n, h, d)
    ref_g = torch.zeros(n, h, 32, dtype=torch.float64, device=dev)
    ref_g[..., :d] = dph / den
    ref_g[..., d] = -(dph * numer).sum(-1) / den[..., 0] ** 2
    ph = (numer / den).reshape(n, h * d)
    ref_w, ref_b = g_out.double().t() @ ph, g_out.double().sum(0)
    assert float(gacc[..., d + 1:].abs().max()) == 0.0, case.id
    if case.check == "exact":
        _exact(gacc, ref_g, "gacc", case)
        _exact(dw, ref_w, "d_weight", case)
        _exact(db, ref_b, "d_bias", case)
        return
    ph32 = (acc[..., :d] / acc[..., d:d + 1]).reshape(n, h * d)
    dph32 = (g_out @ w).reshape(n, h, d)
    fig.put("combine_bwd.gacc_numer", _tol("combine_bwd.gacc_numer", gacc[..., :d], ref_g[..., :d]),
            _tol("combine_bwd.gacc_numer", dph32 / acc[..., d:d + 1], ref_g[..., :d]))
    fig.put("combine_bwd.gacc_den", _tol("combine_bwd.gacc_den", gacc[..., d], ref_g[..., d]),
            _tol("combine_bwd.gacc_den", -(dph32 * acc[..., :d]).sum(-1) / acc[..., d] ** 2, ref_g[..., d]))
    mag_w, mag_b = g_out.double().abs().t() @ ph.abs(), g_out.double().abs().sum(0)
    fig.put("combine_bwd.d_weight", _ratio(dw, ref_w, mag_w), _ratio(g_out.t() @ ph32, ref_w, mag_w))
    fig.put("combine_bwd.d_bias", _ratio(db, ref_b, mag_b), _ratio(g_out.sum(0), ref_b, mag_b))


def _m_reduce_tables(case, dev, fig):
    from hept_amd import ops

    t, n, h, form = case.a
    d = {"f32-d1": 1, "f32-d28": 28}.get(form, 24)
    packed_in, packed_out = form.startswith("packed"), form == "packed-packed"
    g = _gen(case, dev)
    wide = torch.zeros(t, n, h, 32, device=dev)
    if case.check == "exact":
        wide[..., :d] = _ints((t, n, h, d), g)
        wide[..., d] = _dens((t, n, h), g)
    else:
        wide[..., :d] = _randn((t, n, h, d), g).to(torch.bfloat16).float()     # (bf16 values: the packed form holds them)
        wide[..., d] = torch.rand(t, n, h, generator=g, device=dev) + 0.5
    part = pack_rows(wide) if packed_in else wide
    got = ops.reduce_tables(part, d, packed=packed_out)
    ref = wide.double().sum(0)
    if case.check == "exact":
        if packed_out:   # torch's own .to(bfloat16) of the exact sum, repacked
            assert got.dtype == torch.int32 and torch.equal(got, pack_rows(ref.float())), case.id
        else:
            _exact(got, ref, "acc", case)
        return
    mag = wide.double().abs().sum(0)
    t32 = wide.sum(0)
    if packed_out:
        fig.put("reduce_tables.packed", _ratio(ops.unpack_part(got), ref, mag),
                _ratio(ops.unpack_part(pack_rows(t32)), ref, mag))
    else:
        fig.put("reduce_tables.f32", _ratio(got, ref, mag), _ratio(t32, ref, mag))


def exact_part(t, n, h, d, g):
    """Wide f32 partial rows (T, N, H, 32) whose table sums divide exactly: see PATTERNS."""
    dev = g.device
    pats = PATTERNS[t]
    dens = torch.tensor([p[0] for p in pats], dtype=torch.float32, device=dev)
    null = torch.tensor([p[1] for p in pats], dtype=torch.float32, device=dev)
    pi = torch.randint(0, len(pats), (n, h), generator=g, device=dev)
    den, e = dens[pi].permute(2, 0, 1), null[pi].permute(2, 0, 1)            # (T, N, H)
    k, r = _ints((n, h, d), g, -K_MAX, K_MAX), _ints((n, h, d), g, -R_MAX, R_MAX)
    part = torch.zeros(t, n, h, 32, device=dev)
    part[..., :d] = (k[None] + r[None] * e[..., None]) * den[..., None]
    part[..., d] = den
    return part


def _random_part(t, n, h, d, g, bf16):
    part = torch.zeros(t, n, h, 32, device=g.device)
    numer = _randn((t, n, h, d), g)
    part[..., :d] = numer.to(torch.bfloat16).float() if bf16 else numer
    part[..., d] = torch.rand(t, n, h, generator=g, device=g.device) + 0.5
    return part


def _m_combine_out(case, dev, fig):
    from hept_amd import ops

    t, n, h, d, rows, n0, cnt = case.a
    g = _gen(case, dev)
    exact = case.check == "exact"
    wide = exact_part(t, n, h, d, g) if exact else _random_part(t, n, h, d, g, rows == "packed")
    w, b = (_ints((d, h * d), g), _ints((d,), g)) if exact else (_randn((d, h * d), g) * 0.1, _randn((d,), g))
    part = pack_rows(wide) if rows == "packed" else wide
    got = ops.combine_out(part, d, w, b, n0=n0, n_count=cnt)
    got_nb = ops.combine_out(part, d, w, None, n0=n0, n_count=cnt)
    assert got.shape == (cnt, d) and got_nb.shape == (cnt, d), case.id
    if (n0, cnt) != (0, n):     # a slice: the same rows of the whole call
        assert torch.equal(got, ops.combine_out(part, d, w, b)[n0:n0 + cnt]), case.id
    ref, ref_nb = combine_reference(wide, d, w, b, n0, cnt), combine_reference(wide, d, w, None, n0, cnt)
    if exact:
        _exact(got, ref, "out", case)
        _exact(got_nb, ref_nb, "out without bias", case)
        return
    s32 = wide[:, n0:n0 + cnt].sum(0)
    t32 = (s32[..., :d] / s32[..., d:d + 1]).reshape(cnt, -1) @ w.t()
    fig.put("combine_out.out", max(_tol("combine_out.out", got, ref), _tol("combine_out.out", got_nb, ref_nb)),
            _tol("combine_out.out", t32 + b, ref))


def _m_combine_ffn(case, dev, fig):
    import torch.nn.functional as F
    from hept_amd import ops

    t, n, n0, cnt = case.a
    h, d = 8, 24
    g = _gen(case, dev)
    wide = _random_part(t, n, h, d, g, False)
    x = _randn((n, d), g)
    w, b = _randn((d, h * d), g) * 0.1, _randn((d,), g) * 0.1
    lw, lb = _randn((d,), g) * 0.3 + 1.0, _randn((d,), g) * 0.1
    w1, w2 = _randn((d, d), g) * 0.2, _randn((d, d), g) * 0.2
    b1, b2 = _randn((d,), g) * 0.1, _randn((d,), g) * 0.1
    got = ops.combine_ffn(wide, d, w, b, x, lw, lb, EPS, w1, b1, w2, b2, n0=n0, n_count=cnt)
    assert got.shape == (cnt, d) and bool(torch.isfinite(got).all()), case.id
    if (n0, cnt) != (0, n):
        whole = ops.combine_ffn(wide, d, w, b, x, lw, lb, EPS, w1, b1, w2, b2)
        assert torch.equal(got, whole[n0:n0 + cnt]), case.id

    def expr(aggr, x_, p):   # tests/test_gpu_attn_block.py test_combine_ffn_epilogue
        x1 = x_ + aggr
        return x1 + F.linear(F.relu(F.linear(F.layer_norm(x1, (d,), p[0], p[1], EPS), p[2], p[3])), p[4], p[5])

    params = (lw, lb, w1, b1, w2, b2)
    ref = expr(combine_reference(wide, d, w, b, n0, cnt), x[n0:n0 + cnt].double(), [p.double() for p in params])
    s32 = wide[:, n0:n0 + cnt].sum(0)
    aggr32 = F.linear((s32[..., :d] / s32[..., d:d + 1]).reshape(cnt, -1), w, b)
    t32 = expr(aggr32, x[n0:n0 + cnt], params)
    fig.put("combine_ffn.y", _tol("combine_ffn.y", got, ref), _tol("combine_ffn.y", t32, ref))


def bwd_reduce_call(rows16, dq_part, dkv_part, t, n, h, d, c, coords, raw_size, want_dsw):
    """hept_bwd_reduce{,16} with the argument order of ops.block_attn_bwd; returns (rc, dq, dk, dv, dcs, d_sqrt_w).  The
    outputs start as NaN: an element the kernel does not write shows.  ``dq_part`` is the kernel's scratch afterwards."""
    from hept_amd import _lib, ops

    lib = _lib.load()
    dev = dq_part.device
    nan = float("nan")
    dq, dk, dv = (torch.full((n, h * d), nan, device=dev) for _ in range(3))
    dcs = torch.full((n, h, c), nan, device=dev)
    dsw = torch.full((h, c), nan, device=dev) if want_dsw else None
    fn = lib.hept_bwd_reduce16 if rows16 else lib.hept_bwd_reduce
    with torch.cuda.device(dev):
        rc = fn(dq_part.data_ptr(), dkv_part.data_ptr(), t, n, h, d, c, coords.data_ptr(), int(raw_size), dq.data_ptr(),
                dk.data_ptr(), dv.data_ptr(), dcs.data_ptr(), None if dsw is None else dsw.data_ptr(),
                ops.current_stream_ptr(dev))
    return rc, dq, dk, dv, dcs, dsw


def _m_bwd_reduce(case, dev, fig):
    rows16, n, t, h, d, c = case.a
    g = _gen(case, dev)
    exact = case.check == "exact"

    def draw(shape, g_):   # (random values: bf16 values where the rows are bf16)
        if exact:
            return _ints(shape, g_)
        return _randn(shape, g_).to(torch.bfloat16).float() if rows16 else _randn(shape, g_)

    dq_wide, dkv_wide, coords = draw((t, n, h, 32), g), draw((t, n, h, 64), g), draw((n, c), g)
    tile = torch.bfloat16 if rows16 else torch.float32
    refuse = dsw_refused(rows16, n, t, h)
    for raw in sorted({n, n - 1, 1, 0} & set(range(n + 1)), reverse=True):
        dkv_part = dkv_wide.to(tile)
        if refuse:   # the d_sqrt_w scratch would not fit: refused with HEPT_ERR_SHAPE (1), the rest runs without it
            rc = bwd_reduce_call(rows16, dq_wide.to(tile).clone(), dkv_part, t, n, h, d, c, coords, raw, True)[0]
            assert rc == 1, (case.id, rc)
        rc, dq, dk, dv, dcs, dsw = bwd_reduce_call(rows16, dq_wide.to(tile).clone(), dkv_part, t, n, h, d, c, coords, raw,
                                                   not refuse)
        assert rc == 0, (case.id, raw, rc)
        live = (torch.arange(n, device=dev) < raw).double()[:, None, None]
        sq, sk = dq_wide.double().sum(0) * live, dkv_wide[..., :32].double().sum(0) * live
        sv = dkv_wide[..., 32:].double().sum(0) * live
        ref = dict(dq=sq[..., :d].reshape(n, h * d), dk=sk[..., :d].reshape(n, h * d), dv=sv[..., :d].reshape(n, h * d),
                   dcs=(sq + sk)[..., d:d + c])
        ref["d_sqrt_w"] = (ref["dcs"] * coords.double()[:, None, :]).sum(0)
        got = dict(dq=dq, dk=dk, dv=dv, dcs=dcs, d_sqrt_w=dsw)
        if raw < n:   # rows at and after raw_size are exactly 0
            assert all(float(got[k][raw:].abs().max()) == 0.0 for k in ("dq", "dk", "dv", "dcs")), (case.id, raw)
        if exact:
            for key, r in ref.items():
                if got[key] is not None:
                    _exact(got[key], r, f"{key} at raw_size {raw}", case)
            continue
        mq, mk = dq_wide.double().abs().sum(0) * live, dkv_wide[..., :32].double().abs().sum(0) * live
        mv = dkv_wide[..., 32:].double().abs().sum(0) * live
        mag = dict(dq=mq[..., :d].reshape(n, h * d), dk=mk[..., :d].reshape(n, h * d), dv=mv[..., :d].reshape(n, h * d),
                   dcs=(mq + mk)[..., d:d + c])
        mag["d_sqrt_w"] = (mag["dcs"] * coords.double().abs()[:, None, :]).sum(0)
        l32 = live.float()
        q32, k32, v32 = dq_wide.sum(0) * l32, dkv_wide[..., :32].sum(0) * l32, dkv_wide[..., 32:].sum(0) * l32
        t32 = dict(dq=q32[..., :d].reshape(n, h * d), dk=k32[..., :d].reshape(n, h * d), dv=v32[..., :d].reshape(n, h * d),
                   dcs=(q32 + k32)[..., d:d + c])
        t32["d_sqrt_w"] = (t32["dcs"] * coords[:, None, :]).sum(0)
        for key, r in ref.items():
            if got[key] is not None:
                fig.put(f"bwd_reduce.{key}", _ratio(got[key], r, mag[key]), _ratio(t32[key], r, mag[key]))


def _m_rpe_scale(case, dev, fig):
    import pytest
    from hept_amd import ops

    h, c, k, d, edge = case.a
    g = _gen(case, dev)
    w = _randn((h * d, (c - 1) * k), g) * 0.3
    up = _randn((h, c), g)
    if edge == "refused":       # 1025 terms: more than the one workgroup of 1024 threads
        with pytest.raises(RuntimeError, match="HEPT_ERR_SHAPE"):
            ops.rpe_scale(w, h, d, k)
        with pytest.raises(RuntimeError, match="HEPT_ERR_SHAPE"):
            ops.rpe_scale_bwd(w, up, h, d, k)
        return
    if edge == "clamp":
        w[:d, 0] += 3.0         # head 0, term 0: a column sum of about 72, clamped at 50
    if edge == "at50":
        w[:d, 0] = 25.0         # D = 2: the sum is exactly 50.0, where torch's clamp passes the gradient
    got = ops.rpe_scale(w, h, d, k)
    got_g = ops.rpe_scale_bwd(w, up, h, d, k)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_g).all()), case.id
    w64 = w.double().requires_grad_(True)
    ref = rpe_formula(w64, h, d, k)
    (ref * up.double()).sum().backward()
    ref, ref_g = ref.detach(), w64.grad
    w32 = w.clone().requires_grad_(True)
    t32 = rpe_formula(w32, h, d, k)
    (t32 * up).sum().backward()
    # conditioning: exp turns the absolute round-off of a D-term column sum into a relative error; 1 + sum_d |w| per term
    w4 = w.double().reshape(h, d, c - 1, k)
    amag = 1.0 + w4.abs().sum(1).amax(-1)                                     # (H, C - 1)
    amag_c = torch.cat([amag[:, :1], amag], -1)
    fig.put("rpe_scale.sqrt_w", _ratio(got, ref, ref * amag_c), _ratio(t32.detach(), ref, ref * amag_c))
    a = w4.sum(1)                                                             # (H, C - 1, K)
    term = a.clamp(max=50).exp()
    s = torch.sqrt(2 * term.sum(-1, keepdim=True))
    gabs = up.double().abs()[:, 1:].clone()
    gabs[:, 0] += up.double().abs()[:, 0]
    mag = (gabs[..., None] / s * term * (a <= 50) * amag[..., None])          # (H, C - 1, K), the same for every d
    mag = mag[:, None].expand(h, d, c - 1, k).reshape(h * d, (c - 1) * k)
    fig.put("rpe_scale.d_w", _ratio(got_g, ref_g, mag), _ratio(w32.grad, ref_g, mag))
    if edge == "clamp":
        assert float(got_g[:d, 0].abs().max()) == 0.0 and float(a[0, 0, 0]) > 50, case.id
    if edge == "at50":
        assert float(a[0, 0, 0]) == 50.0 and float(got_g[:d, 0].abs().min()) > 0.0, case.id


_MEASURE = {"rows_wgrad": _m_rows_wgrad, "ln_bwd": _m_ln_bwd, "ln_ffn_fwd": _m_ln_ffn_fwd, "ln_ffn_bwd": _m_ln_ffn_bwd,
            "combine_bwd": _m_combine_bwd, "reduce_tables": _m_reduce_tables, "combine_out": _m_combine_out,
            "combine_ffn": _m_combine_ffn, "bwd_reduce": _m_bwd_reduce, "rpe_scale": _m_rpe_scale}


def measure(case, dev):
    """Runs the case: the exact checks and the structural ones assert here; returns the Figures of the bounded ones."""
    fig = Figures()
    _MEASURE[case.kernel](case, dev, fig)
    torch.cuda.synchronize()
    return fig


def assert_bounds(case, fig):
    """Per-point figures are multiples of their tolerance, reduced ones are held to SUM_X; every figure is printed first."""
    for key, (ours, t32) in fig.items():
        print(f"dense sweep {case.id} {key}: {ours:.3e} (torch float32 {t32:.3e})")
    for key, (ours, _t32) in fig.items():
        bound = 1.0 if key in POINT_TOL else SUM_X[key]
        assert bound is not None, f"{key}: no measured bound yet"
        assert ours <= bound, f"{case.id}: {key} is {ours:.3e}, over the bound {bound:.3e}"
