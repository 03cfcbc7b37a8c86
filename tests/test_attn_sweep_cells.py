"""CPU: the fused Attn block's sweep (tests/attn_sweep.py) reaches every cell it was built for and every dispatch branch
cells() names -- all 18 prep_fused_kernel<C, TILE, TMAX> instantiations among them -- so that shrinking the sweep fails
here, not silently on the GPU."""
import attn_sweep as asw


def _all_cells(shapes):
    out = set()
    for s in shapes:
        out |= asw.cells(s)
    return out


def test_shape_ids_are_unique_and_shapes_valid():
    assert len(asw.BY_ID) == len(asw.SHAPES)
    for s in asw.SHAPES:
        n = asw.n_points(s)
        assert 8 <= s.B <= 256 and n % s.B == 0 and s.C in asw.COORDS, s
        assert asw.cost(s) <= asw.COST_CAP, s          # the float64 oracle stays small
        assert not s.ckpt or (s.C == 6 and s.T == 3), s  # case A1's weights: six coordinates, three tables


def test_hand_picked_axes():
    assert {8, 32, 33, 64, 65, 96, 100, 128, 129, 160, 180, 192, 200, 224, 225, 256} <= {s.B for s in asw.SHAPES}
    ns = {asw.n_points(s) for s in asw.SHAPES}
    assert any(n < asw.SMALL_CAP for n in ns) and asw.SMALL_CAP in ns
    assert any(asw.SMALL_CAP < n <= asw.SMALL_CAP + 256 for n in ns)          # just above, one block or two
    assert any(8500 <= n <= 9500 for n in ns)
    assert {1, 3, 6, 9, 17} <= {s.T for s in asw.SHAPES}
    assert any(5 <= s.T <= 8 for s in asw.SHAPES) and any(s.T > 8 for s in asw.SHAPES)
    for c in asw.COORDS:
        assert len([s for s in asw.SHAPES if s.C == c]) >= 8, c
    assert len([s for s in asw.SHAPES if s.ckpt]) >= 3
    assert len([s for s in asw.SHAPES if s.id.startswith("r")]) >= 12


def test_every_branch_in_every_precision_that_has_it():
    got = _all_cells(asw.SHAPES)
    nkts = {f"nkt{k}-{kind}" for k in range(1, 9) for kind in ("full", "ragged")}
    want = set(nkts) | {f"attn-{c}:{p}" for c in nkts for p in asw.PRECISIONS}
    want |= {f"prep<{c},{tile},{tm}>" for c in (6, 4, 2) for tile in ("f32", "bf16", "mixed16") for tm in (4, 8)}
    assert len([c for c in want if c.startswith("prep<")]) == 18
    want |= {"coords6", "coords4", "coords2", "sort-one-workgroup", "sort-two-launch", "table-chunks", "tables-one-chunk",
             "table-chunks-two-launch", "combine-flat", "combine-split", "combine-last-tile-ragged",
             "combine-last-tile-full", "clouds-one", "clouds-several", "cloud-of-B", "cloud-of-B+1", "params-ckpt",
             "params-init"}
    want |= {f"part-f32:{p}" for p in asw.PRECISIONS if not p.endswith("16")}
    want |= {"part-packed:bf16", "part-packed:mixed16"}
    assert not want - got, sorted(want - got)
    # chunked tables at every coordinate count; ragged combine tiles beside the flat grid
    for c in asw.COORDS:
        assert any("table-chunks" in asw.cells(s) and s.C == c for s in asw.SHAPES), c
    assert any({"combine-flat", "combine-last-tile-ragged"} <= asw.cells(s) for s in asw.SHAPES)


def test_training_subset():
    got = _all_cells(asw.BWD_SHAPES)
    want = {f"bwd-nkt{k}-{kind}" for k in range(1, 9) for kind in ("full", "ragged")}
    want |= {f"bwd-prep<{c},{tile},{tm}>" for c in (6, 4, 2) for tile in ("f32", "bf16") for tm in (4, 8)}
    want |= {"bwd-coords6", "bwd-coords4", "bwd-coords2", "bwd-table-chunks", "bwd-sort-two-launch",
             "bwd-cloud-of-B+1", "bwd-params-ckpt"}
    assert not want - got, sorted(want - got)
    assert set(asw.TRAIN) == {"fp32", "bf16", "fp32_mfma"}


def test_tmax_and_chunks_mirror_launch_prep_fused():
    # csrc/prep_hash.hip launch_prep_fused: 4 table slots for 1-4 tables per call, else HEPT_MAX_TABLES
    assert [asw.tmax(t) for t in range(1, 9)] == [4] * 4 + [8] * 4
    assert asw.chunks(17) == [8, 8, 1] and asw.chunks(8) == [8] and asw.chunks(9) == [8, 1]
