"""CPU: the shape sweep (tests/shape_sweep.py) reaches every cell it was built for and every dispatch branch cells()
names, in every precision where the branch applies -- so that shrinking the sweep fails here, not silently on the GPU."""
import shape_sweep as sw


def _all_cells(shapes):
    out = set()
    for s in shapes:
        out |= sw.cells(s)
    return out


def test_shape_ids_are_unique_and_shapes_valid():
    assert len(sw.BY_ID) == len(sw.SHAPES)
    for s in sw.SHAPES:
        n = sw.n_points(s)
        assert 8 <= s.B <= 256 and n % s.B == 0 and 1 <= s.H <= 16 and 1 <= s.D and s.D + s.C <= 30, s
        assert s.T * s.H * n * s.B <= sw.COST_CAP, s          # the float64 oracle stays small


def test_hand_picked_axes():
    blocks = {s.B for s in sw.SHAPES}
    assert {8, 31, 32, 33, 64, 65, 97, 100, 128, 129, 160, 225, 255, 256} <= blocks
    ns = {sw.n_points(s) for s in sw.SHAPES}
    assert any(n < sw.SMALL_CAP for n in ns) and sw.SMALL_CAP in ns
    assert any(sw.SMALL_CAP < n <= sw.SMALL_CAP + 256 for n in ns)          # just above, one block or two
    assert any(8500 <= n <= 9500 for n in ns)
    assert {1, 2, 8, 9, 17} <= {s.T for s in sw.SHAPES}
    heads = {(s.H, s.D, s.C) for s in sw.SHAPES}
    assert {(8, d, c) for d, c in sw.TUNED} <= heads
    assert {(1, 24, 6), (16, 27, 3), (5, 20, 5), (7, 17, 3), (3, 10, 6), (16, 8, 4), (16, 24, 6)} <= heads


def test_every_branch_in_every_precision_that_has_it():
    got = _all_cells(sw.SHAPES)
    want = {f"nkt{k}-{kind}" for k in range(1, 9) for kind in ("full", "ragged")}
    want |= {"sort-one-workgroup", "sort-two-launch", "rows-tuned", "rows-generic", "table-chunks", "tables-one-chunk",
             "clouds-one", "clouds-several", "cloud-of-B", "cloud-of-B+1", "diff-split-kernel"}
    want |= {f"riders:{p}" for p in sw.PRECISIONS}
    want |= {"direct-v:fp32"}
    want |= {f"part-f32:{p}" for p in sw.PRECISIONS} | {"part-packed:bf16", "part-packed:mixed16"}
    want |= {"bwd-dsw-torch", "bwd-dsw-kernel"}
    assert not want - got, sorted(want - got)
    # riders with one table are f32-row only; riders beside a generic row builder; chunked tables beside the two-launch sort
    assert any("riders:fp32" in sw.cells(s) and s.T == 1 for s in sw.SHAPES)
    assert any("riders:bf16" in sw.cells(s) and "rows-generic" in sw.cells(s) for s in sw.SHAPES)
    assert any({"table-chunks", "sort-two-launch"} <= sw.cells(s) for s in sw.SHAPES)
    assert any("direct-v:fp32" in sw.cells(s) and "sort-two-launch" in sw.cells(s) for s in sw.SHAPES)
    assert len([s for s in sw.SHAPES if s.id.startswith("r")]) >= 30


def test_backward_subset():
    got = _all_cells(sw.BWD_SHAPES)
    want = {f"nkt{k}-{kind}" for k in range(1, 9) for kind in ("full", "ragged")}
    want |= {"table-chunks", "sort-two-launch", "rows-generic", "bwd-dsw-torch", "bwd-dsw-kernel", "cloud-of-B+1"}
    assert not want - got, sorted(want - got)
    assert any(s.T == 9 for s in sw.BWD_SHAPES)
    free = {(s.H, s.D, s.C) for s in sw.BWD_SHAPES if (s.H, s.D, s.C) not in {(8, d, c) for d, c in sw.TUNED}}
    assert len(free) >= 4


def test_riders_and_direct_v_mirror_run_begin():
    # csrc/capi.hip:135-138 on a few points of the rule
    assert sw.riders(6272, 8, 24, 1, "fp32", 128) and not sw.riders(6272, 8, 24, 1, "bf16", 128)
    assert sw.riders(6272, 8, 24, 2, "bf16", 128) and not sw.riders(6144, 8, 24, 2, "bf16", 128)
    assert not sw.riders(9000, 8, 24, 2, "fp32", 225) and sw.riders(9000, 8, 24, 2, "fp32_mfma", 225)
    assert not sw.riders(9000, 8, 17, 2, "fp32", 100) and not sw.riders(9000, 8, 24, 9, "fp32", 100)
    assert sw.direct_v(24, "fp32", 129) and not sw.direct_v(24, "fp32", 128) and not sw.direct_v(27, "fp32", 256)
    assert not sw.direct_v(24, "fp32_diff_split", 256)
