"""CPU: the shard sweep (tests/shard_sweep.py) reaches every cell it was built for and every dispatch branch cells()
names, in both variants and in every precision and row format where the branch applies -- so that shrinking the sweep
fails here, not silently on the GPU."""
import shard_sweep as sh
import shape_sweep as sw


def _all_cells(shapes):
    out = set()
    for s in shapes:
        out |= sh.cells(s)
    return out


def _has(*names, shapes=None):
    """Some shape takes all the named cells at once."""
    return any(set(names) <= sh.cells(s) for s in (sh.SHAPES if shapes is None else shapes))


N_RUNS = 206   # the test count of tests/test_gpu_shard_sweep.py (README's parity row)
EXAMPLE = [s for s in sh.SHAPES if s.variant == "example"]
SRC = [s for s in sh.SHAPES if s.variant == "src"]


def test_shape_ids_are_unique_and_shapes_valid():
    assert len(sh.BY_ID) == len(sh.SHAPES) and 25 <= len(sh.SHAPES) <= 40
    for s in sh.SHAPES:
        n = sh.n_points(s)
        assert 8 <= s.B <= 256 and n % s.B == 0 and 1 <= s.H <= 16 and 1 <= s.D <= 27 and s.D + s.C <= 30, s
        assert s.T * s.H * n * s.B <= sw.COST_CAP, s          # the float64 oracle stays small
        for w, g in s.configs:
            assert 1 <= w <= min(s.T, 17) and s.H % g == 0, s
        if s.variant == "src":
            assert sh.raw_kind(s) in sh.KINDS


def test_slices_mirror_the_sharding():
    assert [sh.table_slice(3, r, 2) for r in range(2)] == [(0, 2), (2, 1)]
    assert [sh.table_slice(17, r, 2) for r in range(2)] == [(0, 9), (9, 8)]
    assert [sh.table_slice(10, r, 4)[1] for r in range(4)] == [3, 3, 2, 2]
    assert [sh.point_slice(40, r, 17) for r in (0, 12, 13, 14, 16)] == [(0, 3), (36, 3), (39, 1), (40, 0), (40, 0)]
    assert sh.point_slice(455, 1, 2) == (228, 227)


def test_table_and_point_slices():
    got = _all_cells(sh.SHAPES)
    want = {"T3-W2", "T8-W8", "T17-W17", "T17-W2", "T10-W4", "T9-W2", "T9-W3", "W1", "slices-mixed", "slices-all-direct",
            "slices-all-reduce", "rank-crosses-chunk", "rank-starts-beyond-chunk", "points-even", "points-short-last",
            "points-empty-rank"}
    assert not want - got, sorted(want - got)
    assert _has("T3-W2", "slices-mixed") and _has("T17-W17", "points-empty-rank", "slices-all-direct")
    assert _has("T17-W2", "rank-crosses-chunk", "rank-starts-beyond-chunk")
    # each of them in both variants and with packed rows
    for group in (EXAMPLE, SRC):
        for cell in ("slices-mixed", "slices-all-direct", "slices-all-reduce", "rank-crosses-chunk",
                     "rank-starts-beyond-chunk", "points-even", "points-short-last", "points-empty-rank"):
            assert _has(cell, "prec:fp32:f32", "prec:bf16:packed", "prec:bf16:f32", shapes=group), (cell, group[0].variant)


def test_head_groups_and_head_dimension():
    got = _all_cells(sh.SHAPES)
    want = {"combine-staged", "combine-lanes", "hg-even", "hg-odd", "H-odd", "G1", "H16-G4", "H16-G8", "H12-G4",
            "combine-dt24-groups", "combine-dt16-groups", "combine-generic-groups", "combine-staged-dt24-groups",
            "combine-lanes-dt24-groups", "combine-lanes-dt16-groups", "combine-lanes-generic-groups", "rows-tuned",
            "rows-generic"}
    want |= {f"H{h}" for h in (1, 3, 5, 7, 8, 12, 16)} | {f"D{d}" for d in (24, 16, 20, 27, 10, 8)}
    assert not want - got, sorted(want - got)
    # every generic D of the issue under head groups; the lane-by-lane combine with packed rows (odd heads per group)
    for d in (20, 27, 10, 8):
        assert _has(f"D{d}", "combine-generic-groups"), d
    assert _has("combine-lanes-dt24-groups", "hg-odd", "prec:bf16:packed")
    assert _has("combine-staged-dt24-groups", "prec:bf16:packed") and _has("H16-G4", "H16-G8", "D24")
    for cell in ("combine-staged", "combine-lanes", "hg-odd", "hg-even", "G1"):
        assert _has(cell, shapes=SRC) and _has(cell, shapes=EXAMPLE), cell


def test_sort_paths_riders_and_launches():
    got = _all_cells(sh.SHAPES)
    want = {"sort-one-workgroup:t0>0", "sort-two-launch:t0>0", "begin-riders:fp32", "begin-riders:bf16",
            "begin-riders:fp32:one-table", "begin-v-role:bf16:one-table", "combine-split", "combine-tile-per-wave",
            "partial-direct-v:fp32", "heads-direct:f32", "heads-direct:packed", "heads-reduce:f32", "heads-reduce:packed",
            "heads-direct-padded:f32", "heads-direct-padded:packed"}
    assert not want - got, sorted(want - got)
    assert _has("sort-two-launch:t0>0", "begin-riders:fp32:one-table", "begin-v-role:bf16:one-table", "prec:bf16:packed")
    assert _has("sort-two-launch:t0>0", "T9-W3", "H3", "D16")
    assert _has("combine-tile-per-wave", "W1", "D16", "combine-dt16-groups")
    assert _has("sort-two-launch:t0>0", "rows-generic") and _has("sort-two-launch:t0>0", "rows-tuned")


def test_src_variant():
    got = _all_cells(SRC)
    want = {f"src-raw-{k}" for k in sh.KINDS} | {f"src-raw-{k}:t0>0" for k in sh.KINDS}
    want |= {"src:t0>0", "src-sort-two-launch", "src-sort-one-workgroup", "src-free-heads", "rank-crosses-chunk",
             "rank-starts-beyond-chunk", "src-prec:fp32:f32", "src-prec:bf16:f32", "src-prec:bf16:packed"}
    assert not want - got, sorted(want - got)
    assert _has("src-sort-two-launch", "src:t0>0", shapes=SRC)


def test_precisions():
    for s in sh.SHAPES:
        runs = sh.runs(s)
        for w, g in s.configs:
            assert (w, g, "fp32", "f32") in runs and (w, g, "bf16", "f32") in runs, s
            assert ((w, g, "bf16", "packed") in runs) == (s.D == 24), s
    for p in sh.EXTRA_PRECISIONS:
        assert sum(p in sh.precisions(s) for s in sh.SHAPES) >= 3, p
        assert any(p in sh.precisions(s) for s in SRC), p
    assert sum(len(sh.runs(s)) for s in sh.SHAPES) == N_RUNS
