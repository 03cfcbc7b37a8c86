"""CPU: the rows sweep (tests/rows_sweep.py) reaches all 117 instantiations of the row builder and every branch it names,
its exact inputs are exact (``prove_exact``: shuffled float32 accumulation orders against float64, representability in
every tile and input type, the keys of the sort), the rounding cells hold the planted ties, the file:line references into
csrc/ still match, and importing the module touches no GPU."""
import os
import subprocess
import sys

import pytest
import torch

import rows_sweep as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROOFS = {}
for _c in rs.CELLS:
    PROOFS.setdefault(rs.proof_key(_c), _c)


def test_cell_ids_and_counts():
    assert len(rs.BY_ID) == len(rs.CELLS) + len(rs.ROUND_CELLS)
    inst = [c for c in rs.CELLS if c.kind == "inst"]
    assert len([c for c in inst if rs.tuned(c)]) == 108 and len([c for c in inst if not rs.tuned(c)]) == 9 * 4
    assert len([c for c in rs.CELLS if c.kind == "edge"]) == 12 * 3 * 9
    assert len([c for c in rs.CELLS if c.kind == "raw"]) == 2 * 5 * 3 * 9
    assert len(rs.BOUND_CELLS) == 2 and len(rs.ROUND_CELLS) == 2 * 2 * 3 and len(rs.CODES_NONE_CELLS) == 3
    for c in rs.CELLS + rs.ROUND_CELLS:
        assert 1 <= c.H <= 16 and c.D + c.C <= 30 and 1 <= c.D <= 28 and c.N >= 1, c
        assert c.t0 > 0 and c.T > c.t0 + c.Tl and 1 <= c.Tl <= 8 and 0 <= c.raw <= c.N, c      # tables on either side of the slab
    assert all(c.N == rs.N_INST for c in inst)
    assert rs.N_INST == 9 * 8 + 5 and rs.prep_wgs(rs.N_INST) == 3 and -(-rs.N_INST // 8) == 2 * 4 + 2   # last workgroup: two idle waves


def test_every_instantiation_is_reached():
    want = rs.all_instantiations()
    assert len(want) == 117
    inst = [c for c in rs.CELLS if c.kind == "inst"]
    assert {rs.instantiation(c) for c in inst} == want
    assert len({rs.instantiation(c) for c in inst if rs.tuned(c)}) == len([c for c in inst if rs.tuned(c)])   # one cell each
    # the generic kernel: every instantiation on every free head shape
    assert {(c.H, c.D, c.C) + rs.instantiation(c)[1:] for c in inst if not rs.tuned(c)} \
        == {hdc + (t, i) for hdc in rs.GENERIC for t in rs.TILES for i in rs.INS}
    # Tl rotates over {1, 3, 4} and {5, 7, 8} within every tile type, Tl == TMAX included
    for tile in rs.TILES:
        assert {c.Tl for c in inst if rs.tuned(c) and c.tile == tile} == {1, 3, 4, 5, 7, 8}, tile
    assert {c.Tl for c in inst if not rs.tuned(c)} == {1, 3, 4, 5, 7, 8}
    # boundary and padding cells: every (tile type, input type) on every shape at every size
    for kind, sizes in (("edge", set(rs.EDGE_N)), ("raw", set(rs.RAW_N))):
        got = {(c.N, (c.H, c.D, c.C), c.tile, c.intype) for c in rs.CELLS if c.kind == kind}
        assert got == {(n, s, t, i) for n in sizes for s in rs.EDGE_SHAPES for t in rs.TILES for i in rs.INS}, kind
    assert sum(rs.tuned(rs.Cell("", "", h, d, c, 1, 1, 0, 1, "fp32", "f32", 1, True)) for h, d, c in rs.EDGE_SHAPES) == 2
    for n in rs.RAW_N:
        assert {c.raw for c in rs.CELLS if c.kind == "raw" and c.N == n} == {n, n - 1, n - 37, 6000, 0}
    assert all(not c.codes for c in rs.CELLS if c.kind == "raw") and 6000 % 8 == 0
    assert min(rs.RAW_N) <= rs.SMALL_CAP < max(rs.RAW_N) <= 16000
    assert [rs.cells(c) >= {"codes", "tuned"} for c in rs.BOUND_CELLS] == [True, True]
    assert {("sort-one-workgroup" in rs.cells(c)) for c in rs.BOUND_CELLS} == {True, False}


def test_every_branch_is_reached():
    want = {"tuned", "generic", "tmax4", "tmax8", "tl==tmax", "ragged-last-tile", "idle-wave", "grid-stride",
            "grid-stride-ragged-trip", "spare-slot-fill", "wgs-capped", "pad-rows", "pad-rows-from-a-tile-boundary",
            "pad-rows-only", "codes", "codes-none", "t0>0", "sort-one-workgroup", "sort-two-launch", "generic-idle-threads",
            "generic-empty-workgroup"} | {f"tile:{t}" for t in rs.TILES} | {f"in:{i}" for i in rs.INS}
    got = set().union(*(rs.cells(c) for c in rs.CELLS))
    assert got == want, (sorted(want - got), sorted(got - want))
    # grid-stride in both kernels, in every tile and input type
    for kernel in ("tuned", "generic"):
        stride = [c for c in rs.CELLS if {"grid-stride", kernel} <= rs.cells(c)]
        assert {(c.tile, c.intype) for c in stride} == {(t, i) for t in rs.TILES for i in rs.INS}, kernel
    # the sizes around the first grid-stride trip of the three-role launch: 341 workgroups x 4 waves x 8 points
    assert rs.WGS3 * rs.WAVES * rs.POINTS == 10912
    by_n = {n: rs.cells(next(c for c in rs.CELLS if c.kind == "edge" and c.N == n and rs.tuned(c))) for n in rs.EDGE_N}
    assert "grid-stride" not in by_n[10912] and all("grid-stride" in by_n[n] for n in (10913, 10920, 10944, 21833))
    assert "ragged-last-tile" in by_n[10913] and "ragged-last-tile" not in by_n[10920]
    assert 21833 == 2 * 10912 + 9 and "ragged-last-tile" in by_n[21833]
    # both TMAX classes run the grid-stride loop
    assert {"tmax4", "tmax8"} <= set().union(*(rs.cells(c) for c in rs.CELLS if "grid-stride" in rs.cells(c)))


def test_two_role_sizes_take_both_branches_of_prep_wgs():
    import shape_sweep as sw

    assert [rs.prep_wgs(n, 2) for n in rs.TWO_ROLE_N] == [341, 342, 512, 257, 342]     # as wanted | even trips (2, 3)
    assert [rs.prep_wgs(n, 3) for n in rs.TWO_ROLE_N] == [341, 341, 341, 341, 341]
    cases = rs.two_role_cases()
    column_d = [x for x in cases if x[1] in rs.TWO_ROLE_COLUMN_D]
    cases = [x for x in cases if x[1] not in rs.TWO_ROLE_COLUMN_D]
    assert len(cases) == 16 and sum(1 for n, hdc, p in cases if hdc != (8, 24, 6)) == 1
    # the riders' column-D cases: every shape in every tile type, accepted by the library's own shape check
    assert sorted(column_d) == sorted((10912, hdc, p) for hdc in ((3, 4, 3), (3, 20, 4)) for p in ("fp32", "bf16", "mixed16"))
    from hept_amd import _lib
    for n, (h, d, c), p in column_d:
        s = rs.two_role_shape(n, (h, d, c))
        assert _lib.load().hept_check_shape(n, h, d, c, s.T, s.B) == 0, (n, h, d, c)
    assert _lib.load().hept_check_shape(10912, 8, 28, 2, 2, 32) != 0         # D = 28: no shape the operator accepts
    for n, hdc, p in cases + column_d:
        s = rs.two_role_shape(n, hdc)
        assert sw.n_points(s) == n and n % 32 == 0 and sw.riders(n, s.H, s.D, s.T, p, s.B), (n, hdc, p)
        assert ("rows-tuned" in sw.cells(s)) == (hdc == (8, 24, 6))


def test_source_references():
    for path, line, text in rs.REFS:
        with open(os.path.join(ROOT, path)) as f:
            lines = f.read().splitlines()
        assert text in lines[line - 1], f"{path}:{line} no longer holds {text!r}: {lines[line - 1]!r}"


@pytest.mark.parametrize("cid", [c.id for c in PROOFS.values()])
def test_inputs_are_exact(cid):
    c = rs.BY_ID[cid]
    r = rs.prove_exact(c)
    assert all(r["ok"].values()), (cid, r["ok"])
    assert r["alpha_distinct"], cid                       # no two (head, table) pairs share their alpha column
    sw = r["sqrt_w"]
    assert bool(((sw.log2() == sw.log2().round()) & (sw >= 0.25) & (sw <= 4)).all())
    if c.H > 1:
        assert len(torch.unique(sw, dim=0)) > 1, cid      # a swapped head changes the row
    assert len(torch.unique(sw)) > 1, cid                 # ... and so does a swapped column
    assert r["max_abs_proj"] <= 30 * 112
    d = rs.data(c)
    for x in ("q", "k", "v", "coords"):
        assert float(d[x].abs().max()) <= 4 and torch.equal(d[x] * 8, (d[x] * 8).round())
    assert float(d["alpha"].abs().max()) <= 7 and torch.equal(d["alpha"], d["alpha"].round())
    # the largest code of every (table, head) sits at point 0 alone; in every head it differs between any two tables a
    # slip of up to 7 tables could confuse (a read at table t for t0 + t, a neighbouring table), and within a table it
    # differs between neighbouring heads (all heads where H <= 8)
    codes, maxc = d["codes"], d["maxc"]
    assert torch.equal(codes[..., 0], maxc) and (c.N == 1 or bool((codes[..., 1:] < maxc[..., None]).all()))
    assert 8 <= int(maxc.min()) and int(maxc.max()) <= 15
    for t in range(c.T):
        for t2 in range(t + 1, min(c.T, t + 8)):
            assert bool((maxc[t] != maxc[t2]).all()), (cid, t, t2)
        for h in range(c.H):
            for h2 in range(h + 1, min(c.H, h + 8)):
                assert int(maxc[t, h]) != int(maxc[t, h2]), (cid, t, h, h2)
    for slip in (-1, 1, -c.t0):                           # the expected bound of the cell's tables changes under each slip
        lo = c.t0 + slip
        if 0 <= lo and lo + c.Tl <= c.T:
            assert bool((maxc[lo:lo + c.Tl] != maxc[c.t0:c.t0 + c.Tl]).all()), (cid, slip)
    if c.raw >= 2000:
        assert r["distinct"] < c.raw, cid                 # ties: the stability of the sort is exercised
        assert bool((r["span"] > 0).all())


@pytest.mark.parametrize("cid", [c.id for c in rs.ROUND_CELLS])
def test_rounding_cells_hold_the_ties(cid):
    c = rs.BY_ID[cid]
    d = rs.data(c)
    sw = d["sqrt_w"]
    assert bool((sw.log2() == sw.log2().round()).all())
    for x in ("q", "k", "v", "coords"):
        t = d[x]
        even, odd = rs.tie_count(t, rs.tie_type(c, x))     # v is stored as bf16 in both 16-bit tile types
        assert even >= 50 and odd >= 50 and even + odd >= min(300, t.numel() // 3) - 8, (cid, x, even, odd)
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) < 8
        nz = t[t != 0].abs()
        assert float(nz.min()) >= 2.0 ** -6                # normal in fp16, also after the scale 2^-2 .. 2^2
        neg0 = (t == 0) & (t.view(torch.int32) < 0)
        assert int(neg0.sum()) >= 1 and int(((t == 0) & ~neg0).sum()) >= 1 and bool((t < 0).any() and (t > 0).any())
    # the ties survive the input cast where the input type is wider than the row type, and the scale by a power of two
    q_hat, k_hat, v_h = rs.unrounded_rows(c, d, torch.float32)
    assert float(q_hat.abs().max()) < 32 and bool(torch.isfinite(q_hat.to(rs.QK_DTYPE[c.tile])).all())
    even, odd = rs.tie_count(q_hat[..., c.D:], c.tile)     # the coordinate part is float32 whatever the input type
    assert even >= 20 and odd >= 20, (cid, even, odd)
    # the two norms are further apart than the bound on some row: the GPU test can tell them apart
    rr = q_hat.to(rs.QK_DTYPE[c.tile]).double()
    gap = (0.5 * ((rr ** 2).sum(-1) - (q_hat.double() ** 2).sum(-1))).abs()
    assert bool((gap > 2 * rs.NORM_BOUND * (q_hat.double() ** 2).sum(-1)).any()), cid


def test_norm_bound_is_the_a_priori_one():
    # 30 fmaf terms: |fl(sum) - sum| <= gamma_30 * sum |terms|, gamma_n = n u / (1 - n u) < (n + 1) u, u = 2^-24
    u = 2.0 ** -24
    assert 30 * u / (1 - 30 * u) < rs.NORM_BOUND == 31 * u


def test_import_touches_no_gpu():
    code = ("import sys, torch; sys.path[:0] = [%r, %r, %r]; import rows_sweep as rs; "
            "rs.prove_exact(rs.CELLS[0]); assert not torch.cuda.is_initialized(); "
            "assert 'scratch_sweep' not in sys.modules; print(len(rs.CELLS))"
            % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout.strip()) == len(rs.CELLS)
