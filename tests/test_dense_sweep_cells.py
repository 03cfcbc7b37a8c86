"""CPU: the dense sweep (tests/dense_sweep.py) holds every case it was built for, every exact case keeps its products
and partial sums below 2^24, and every branch cells() names is reached -- so that shrinking a table fails here, not
silently on the GPU.  Also: the float64 reference expressions of the sweep against torch autograd, on the CPU."""
import torch

import dense_sweep as ds


def _ids(kernel, check=None):
    return {c.id for c in ds.of_kernel(kernel, check)}


def _args(kernel, check="exact"):
    return {c.a for c in ds.of_kernel(kernel, check)}


def _all_cells(kernel):
    out = set()
    for c in ds.of_kernel(kernel):
        out |= ds.cells(c)
    return out


def _has(kernel, *names):
    return any(set(names) <= ds.cells(c) for c in ds.of_kernel(kernel))


# the number of cases per kernel: a case deleted from any table changes one of them
COUNTS = {"rows_wgrad": 44, "ln_bwd": 13, "ln_ffn_fwd": 14, "ln_ffn_bwd": 14, "combine_bwd": 102, "reduce_tables": 120,
          "combine_out": 84, "combine_ffn": 5, "bwd_reduce": 142, "rpe_scale": 18}


def test_case_ids_are_unique_and_counted():
    assert len(ds.BY_ID) == len(ds.CASES) == sum(COUNTS.values())
    for kernel, count in COUNTS.items():
        assert len(ds.of_kernel(kernel)) == count, kernel
    assert {c.kernel for c in ds.CASES} == set(COUNTS)
    assert {c.check for c in ds.CASES} == {"exact", "f64"}


def test_exact_cases_stay_below_2_pow_24():
    exact = [c for c in ds.CASES if c.check == "exact"]
    assert {c.kernel for c in exact} == {"rows_wgrad", "combine_bwd", "reduce_tables", "combine_out", "bwd_reduce"}
    for c in exact:
        chain = ds.bounds(c)
        assert chain, c.id
        for what, a, b, terms in chain:
            assert a * b * terms < ds.LIMIT, (c.id, what, a * b * terms)
    # every one of them has a random-valued companion that sees full mantissas
    for kernel in {c.kernel for c in exact}:
        assert ds.of_kernel(kernel, "f64"), kernel
    # what is not a sum of products is never "exact"
    for kernel in ds.LN_KERNELS + ("combine_ffn", "rpe_scale"):
        assert not ds.of_kernel(kernel, "exact"), kernel


def test_combine_patterns_divide_exactly():
    assert set(ds.PATTERNS) == set(ds.CO_T)
    for t, pats in ds.PATTERNS.items():
        for dens, e in pats:
            assert len(dens) == len(e) == t and set(dens) <= {1, 2, 4}
            total = sum(dens)
            assert total & (total - 1) == 0                       # a power of two: its reciprocal is exact
            assert sum(a * b for a, b in zip(dens, e)) == 0       # the r-part of the numerators cancels over the tables
            assert max(abs(x) for x in e) <= 2
    worst = 4 * (ds.K_MAX + 2 * ds.R_MAX)
    assert worst <= 256                                           # every integer up to 256 is a bf16 value
    g = torch.Generator().manual_seed(1)
    for t in ds.CO_T:
        part = ds.exact_part(t, 50, 3, 5, g)
        s = part.double().sum(0)
        q = s[..., :5] / s[..., 5:6]
        assert torch.equal(q, q.round()) and float(q.abs().max()) <= ds.K_MAX and float(part.abs().max()) <= worst
        assert torch.equal(part[..., :5] % part[..., 5:6], torch.zeros_like(part[..., :5]))   # multiples of their denominator
        wide = torch.zeros(t, 50, 3, 32)
        wide[..., :24] = ds.exact_part(t, 50, 3, 24, g)[..., :24]
        assert torch.equal(wide[..., :24].to(torch.bfloat16).float(), wide[..., :24])


def test_rows_wgrad_table():
    assert ds.WG_N == (1, 2, 15, 16, 17, 127, 128, 129, 2047, 2048, 2049, 131200)
    assert ds.WG_O == (1, 24, 31, 32, 33, 72, 191, 192, 193, 384, 400)
    want = {(n, o) for n in ds.WG_N for o in (24, 192)} | {(n, o) for o in ds.WG_O for n in (129, 2049)}
    assert _args("rows_wgrad") == want
    got = _all_cells("rows_wgrad")
    want = {"wgrad-cols32x16", "wgrad-cols192x4", "wgrad-grid-rows1", "wgrad-grid-rows2", "wgrad-grid-rows3",
            "wgrad-dead-cols", "wgrad-cols-full", "wgrad-points-ragged", "wgrad-points-full", "fsum-one-trip",
            "fsum-slices-wrap", "wgrad-wgs1", "wgrad-wgs16", "wgrad-wgs17", "wgrad-wgs-many", "wgrad-idle-groups",
            "wgrad-unroll-tail"}
    assert not want - got, sorted(want - got)
    for inst in ("wgrad-cols32x16", "wgrad-cols192x4"):
        assert _has("rows_wgrad", inst, "fsum-slices-wrap") and _has("rows_wgrad", inst, "wgrad-idle-groups")
        assert _has("rows_wgrad", inst, "wgrad-dead-cols", "wgrad-wgs17")
    assert _has("rows_wgrad", "wgrad-grid-rows3", "wgrad-dead-cols", "fsum-slices-wrap")


def test_layernorm_and_ffn_tables():
    assert ds.LN_N == (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 66000)
    for kern in ds.LN_KERNELS:
        edges = ds.LN_EDGES[:2] if kern == "ln_bwd" else ds.LN_EDGES
        assert _args(kern, "f64") == {(n, None) for n in ds.LN_N} | {(257, e) for e in edges}
        got = _all_cells(kern)
        want = {"ln-rows-ragged", "ln-rows-full", "ln-wave-ragged", "ln-wave-full", "ln-idle-waves", "fsum-one-trip",
                "fsum-slices-wrap", "ln-wgs1", "ln-wgs16", "ln-wgs17", "ln-wgs-many"} | {f"ln-edge-{e}" for e in edges}
        assert not want - got, (kern, sorted(want - got))


def test_combine_bwd_table():
    want = {(n, h, 24) for n in ds.CB_N for h in ds.CB_TUNED_H} | {(n, h, d) for n in ds.CB_N for h, d in ds.CB_GENERIC}
    assert _args("combine_bwd") == want | set(ds.CB_STRIDE)
    assert ds.CB_N == (1, 127, 128, 129, 2047, 2048, 2049) and ds.CB_TUNED_H == (1, 2, 3, 5, 7, 8)
    assert set(ds.CB_GENERIC) == {(9, 24), (16, 24), (16, 27), (11, 26), (5, 20), (8, 16), (12, 8), (1, 1)}
    assert set(ds.CB_STRIDE) == {(131200, 8, 24), (65700, 16, 24)}
    assert all(ds.combine_bwd_tuned(h, 24) for h in ds.CB_TUNED_H)
    assert not any(ds.combine_bwd_tuned(h, d) for h, d in ds.CB_GENERIC)
    got = _all_cells("combine_bwd")
    want = {"cb-tuned", "cb-generic", "cb-rows-grid-stride", "cb-rows-one-trip", "cb-points-ragged", "cb-points-full",
            "fsum-one-trip", "fsum-slices-wrap", "cb-tuned-dead-cols", "cb-tuned-cols-full", "cb-generic-col-loop-1",
            "cb-generic-col-loop-2"}
    assert not want - got, sorted(want - got)
    for kind in ("cb-tuned", "cb-generic"):
        assert _has("combine_bwd", kind, "cb-rows-grid-stride") and _has("combine_bwd", kind, "fsum-slices-wrap")
    assert sum(h * d > 256 for h, d in ds.CB_GENERIC) >= 3


def test_reduce_tables_table():
    assert ds.RT_T == (1, 2, 3, 8, 9) and len(ds.RT_FORMS) == 5
    assert {n * h for n, h in ds.RT_SMALL + ds.RT_BIG} == {1, 127, 128, 129, 524288, 524289}
    assert ds.RT_STRIDE == (65600, 8, 2)
    want = {(t, n, h, f) for f in ds.RT_FORMS for n, h in ds.RT_SMALL for t in ds.RT_T}
    want |= {(2, n, h, f) for f in ds.RT_FORMS for n, h in ds.RT_BIG} | {(2, 65600, 8, f) for f in ds.RT_FORMS}
    assert _args("reduce_tables") == want
    for form in ds.RT_FORMS:
        for cell in ("rt-one-trip", "rt-grid-full", "rt-grid-stride", "rt-block-ragged", "rt-block-full", "rt-rows1",
                     "rt-rows127", "rt-rows128", "rt-rows129") + tuple(f"rt-tables{t}" for t in ds.RT_T):
            assert _has("reduce_tables", f"rt-{form}", cell), (form, cell)
        assert _has("reduce_tables", f"rt-{form}", "reduce_tables:f64")
    # the largest input stays near 270 MB
    assert max(t * n * h * 128 for t, n, h, _ in _args("reduce_tables")) <= 270e6


def test_combine_out_table():
    assert ds.CO_COUNTS == (1, 31, 32, 33, 32736, 32767, 32768, 32769, 262144, 262200)
    assert ds.CO_HEADS24 == (8, 7, 16, 1) and set(ds.CO_GENERIC) == {(5, 20), (16, 27), (1, 1)} and ds.CO_T == (1, 3, 4)
    assert ds.CO_SLICES == ((0, 129), (32, 50), (45, 33), (128, 1))
    args = _args("combine_out")
    for rows in ("f32", "packed"):
        assert {(1, n, 8, 24, rows, 0, n) for n in ds.CO_COUNTS} <= args
        assert {(t, 33, h, 24, rows, 0, 33) for h in ds.CO_HEADS24 for t in ds.CO_T} <= args
        assert {(3, 32769, h, 24, rows, 0, 32769) for h in ds.CO_HEADS24} | {(4, 32769, 8, 24, rows, 0, 32769)} <= args
        assert {(3, 129, 8, 24, rows, n0, cnt) for n0, cnt in ds.CO_SLICES} <= args
    assert {(t, 33, h, d, "f32", 0, 33) for h, d in ds.CO_GENERIC for t in ds.CO_T} <= args
    assert {(3, 32769, h, d, "f32", 0, 32769) for h, d in ds.CO_GENERIC} <= args
    assert {(3, 129, h, d, "f32", n0, cnt) for h, d in ds.CO_GENERIC for n0, cnt in ds.CO_SLICES[1:]} <= args
    # the two largest point counts run only at H = 8, D = 24, one table; the largest input stays near 270 MB
    assert all((t, h, d) == (1, 8, 24) for t, n, h, d, *_ in args if n > 100000)
    assert max(t * n * h * 128 for t, n, h, *_ in args) <= 270e6
    for rows in ("co-rows-f32", "co-rows-packed"):
        for cell in ("co-split", "co-split-last", "co-flat-first", "co-flat", "co-flat-grid-full", "co-flat-striding",
                     "co-flat-idle-waves", "co-tile-ragged", "co-tile-full", "co-staged", "co-lanes",
                     "co-staged-tables-wrap", "co-slice-n0", "co-slice-short", "co-slice-last-point", "co-tables1",
                     "co-tables3", "co-tables4"):
            assert _has("combine_out", rows, cell), (rows, cell)
        for kernel in ("co-split", "co-flat"):      # both launches with staged rows, lane-by-lane loads and three tables
            assert _has("combine_out", rows, kernel, "co-staged", "co-tables3")
            assert _has("combine_out", rows, kernel, "co-lanes", "co-tables3")
        assert _has("combine_out", rows, "co-flat", "co-staged-tables-wrap")
    for kernel in ("co-split", "co-flat"):
        assert _has("combine_out", "co-dt-generic", kernel, "co-h16d27") and _has("combine_out", "co-dt-generic", kernel, "co-h1d1")
    assert _has("combine_out", "co-dt-generic", "co-slice-last-point")
    assert _has("combine_out", "combine_out:f64", "co-rows-packed") and _has("combine_out", "combine_out:f64", "co-dt-generic")


def test_combine_ffn_table():
    assert ds.CF_COUNTS == (1, 33, 32768, 262200)
    args = _args("combine_ffn", "f64")
    assert {(n, n0, cnt) for _, n, n0, cnt in args} == {(n, 0, n) for n in ds.CF_COUNTS} | {(129, 45, 33)}
    got = _all_cells("combine_ffn")
    assert {"co-split", "co-flat", "co-flat-striding", "co-slice-n0", "co-slice-short", "co-tile-ragged", "co-tile-full"} <= got
    assert max(t * n * 8 * 128 for t, n, _, _ in args) <= 270e6


def test_bwd_reduce_table():
    assert ds.BR_N == (1, 255, 256, 257, 4095, 4096, 4097) and ds.BR_T == (1, 3)
    assert ds.BR_SHAPES == ((1, 24, 2), (8, 24, 6), (9, 8, 7), (16, 16, 4), (5, 21, 5))
    assert {h * c for h, _, c in ds.BR_SHAPES[:4]} == {2, 48, 63, 64}
    assert all(d + c <= 30 and h * c <= 64 for h, d, c in ds.BR_SHAPES)
    want = {(r, n, t, h, d, c) for r in (False, True) for n in ds.BR_N for t in ds.BR_T for h, d, c in ds.BR_SHAPES}
    assert _args("bwd_reduce") == want
    for rows in ("br-rows32", "br-rows16"):
        for cell in ("dsw-lanes2", "dsw-lanes48", "dsw-lanes63", "dsw-lanes64", "br-tables1", "br-tables3",
                     "br-block-ragged", "br-block-full", "dsw-points-ragged", "dsw-points-full", "fsum-one-trip",
                     "fsum-slices-wrap", "dsw-kernel", "dsw-refused", "dsw-unroll-tail", "bwd_reduce:f64"):
            assert _has("bwd_reduce", rows, cell), (rows, cell)
        assert _has("bwd_reduce", rows, "dsw-lanes64", "fsum-slices-wrap", "br-tables3")
    assert _has("bwd_reduce", "br16-odd-d", "fsum-slices-wrap")
    # the refusal is the small-cloud rule only: nothing from 255 points on is refused
    assert all(n == 1 for r, n, t, h, d, c in want if ds.dsw_refused(r, n, t, h))
    assert ds.dsw_refused(False, 1, 1, 1) and not ds.dsw_refused(False, 1, 3, 1) and ds.dsw_refused(True, 1, 3, 1)


def test_training_step_shape_sits_on_the_64_lane_gate():
    import shape_sweep as sw
    from test_gpu_dense_sweep import HC64

    assert (HC64.H, HC64.D, HC64.C, HC64.B, HC64.T) == (16, 16, 4, 40, 2) and HC64.H * HC64.C == 64
    assert len(HC64.sizes) == 2 and all(n % HC64.B for n in HC64.sizes)
    assert "bwd-dsw-kernel" in sw.cells(HC64) and "bwd-dsw-torch" in sw.cells(HC64._replace(C=5))
    assert HC64.id not in sw.BY_ID
    assert HC64.T * HC64.H * sw.n_points(HC64) * HC64.B <= sw.COST_CAP


def test_rpe_scale_table():
    assert {h * (c - 1) * k for h, c, k in ds.RPE_TERMS} == {1, 1023, 1024} and ds.RPE_D == (1, 7, 8, 9, 27)
    args = _args("rpe_scale", "f64")
    assert {(h, c, k, d, None) for h, c, k in ds.RPE_TERMS for d in ds.RPE_D} <= args
    assert {a[4] for a in args} == {None, "clamp", "at50", "refused"}
    got = _all_cells("rpe_scale")
    assert {"rpe-terms1", "rpe-terms1023", "rpe-terms1024", "rpe-terms1025", "rpe-refused", "rpe-d<8", "rpe-d8", "rpe-d>8",
            "rpe-edge-clamp", "rpe-edge-at50", "rpe-edge-refused"} <= got
    assert all(("rpe-refused" in ds.cells(c)) == (c.a[4] == "refused") for c in ds.of_kernel("rpe_scale"))
    at50 = [a for a in args if a[4] == "at50"]
    assert at50 and all(a[3] == 2 for a in at50)                  # D = 2, both entries 25.0


def test_every_sum_bound_is_measured():
    for key, x in ds.SUM_X.items():
        assert x is not None and 0 < x < 1e-2, key


def test_row_guard_refuses_host_tensors_and_other_types():
    """ops._rowsc, the guard of the stage functions' row arguments: no host address and no foreign element type reaches C."""
    import pytest
    from hept_amd import ops

    for dtype in (torch.float32, torch.bfloat16, torch.float16, torch.int32):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            ops._rowsc(torch.zeros(2, 3, 32, dtype=dtype), "part")
    for dtype in (torch.float64, torch.int64, torch.uint8):
        with pytest.raises((TypeError, RuntimeError)):
            ops._rowsc(torch.zeros(2, 3, 32, dtype=dtype), "part")


def test_reference_expressions_against_autograd():
    """The float64 expressions the sweep takes its magnitudes and references from, against torch autograd (CPU)."""
    g = torch.Generator().manual_seed(5)
    n = 37
    x, go = torch.randn(n, 24, generator=g).double(), torch.randn(n, 24, generator=g).double()
    lw, lb = torch.randn(24, generator=g).double() * 0.3 + 1, torch.randn(24, generator=g).double() * 0.1
    w1, w2 = torch.randn(24, 24, generator=g).double() * 0.2, torch.randn(24, 24, generator=g).double() * 0.2
    b1, b2 = torch.randn(24, generator=g).double() * 0.1, torch.randn(24, generator=g).double() * 0.1
    p = ds.ffn_terms(x, go, lw, lb, w1, b1, w2, b2)
    grads = ds.ffn_grads(x, go, lw, lb, w1, b1, w2, b2)
    signed = [(p["dz"] * p["xhat"]).sum(0), p["dz"].sum(0), p["dh"].t() @ p["z"], p["dh"].sum(0), go.t() @ p["h"], go.sum(0)]
    for a, b in zip(signed, grads[1:]):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    mags = ds.ffn_magnitudes(x, go, lw, lb, w1, b1, w2, b2)
    assert all(bool((m >= s.abs() - 1e-12).all()) for m, s in zip(mags, signed))
    dx, xn, dlw, dlb = ds.ln_grads(x, go, lw, lb)
    xhat, _ = ds.ln_parts(x, ds.EPS)
    torch.testing.assert_close(xn, xhat * lw + lb, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dlw, (go * xhat).sum(0), rtol=1e-12, atol=1e-12)
    # the combine: packed rows hold what torch's bf16 rounding gives; the reference divides the table sums
    wide = torch.zeros(3, 5, 2, 32)
    wide[..., :24] = torch.randn(3, 5, 2, 24, generator=g)
    wide[..., 24] = torch.rand(3, 5, 2, generator=g) + 0.5
    packed = ds.pack_rows(wide)
    assert packed.dtype == torch.int32 and packed.shape == (3, 5, 2, 16) and float(packed[..., 13:].abs().max()) == 0
    lo = (packed[..., :12] << 16).view(torch.float32)
    assert torch.equal(lo, wide[..., 0:24:2].to(torch.bfloat16).float())
    assert torch.equal(packed[..., 12].view(torch.float32), wide[..., 24])
    w, b = torch.randn(24, 48, generator=g), torch.randn(24, generator=g)
    ref = ds.combine_reference(wide, 24, w, b, 1, 3, chunk=2)
    s = wide.double().sum(0)[1:4]
    want = torch.nn.functional.linear((s[..., :24] / s[..., 24:25]).reshape(3, 48), w.double(), b.double())
    torch.testing.assert_close(ref, want, rtol=1e-13, atol=1e-13)
    from hept_amd.autograd import rpe_scale_torch

    wr = torch.randn(3 * 5, 2 * 4, generator=g).double()
    assert torch.equal(ds.rpe_formula(wr, 3, 5, 4), rpe_scale_torch(wr, 3, 5, 4))
