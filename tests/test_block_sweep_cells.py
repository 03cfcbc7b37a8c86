"""CPU: the block sweep (tests/block_sweep.py) reaches every instantiation of the block-attention kernels, forward and
backward, its exact design is exact in every family's arithmetic (``bounds``), every case holds an empty-set row and a
boundary bait per block, the file:line references into csrc/ still match, and importing the module touches no GPU."""
import os
import subprocess
import sys

import pytest
import torch

import block_sweep as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = [c for c in bs.CASES if c.variant == "exact"]


def test_case_ids_and_counts():
    assert len(bs.BY_ID) == len(bs.CASES) and len(bs.F64_BY_ID) == len(bs.F64_CASES)
    assert len(bs.FAMILIES) == 13 and len(EXACT) == 13 * 8 * 3 == 312
    assert len([c for c in bs.CASES if c.variant == "big"]) == 5 * 4 * 2
    assert len([c for c in bs.CASES if c.variant == "raw"]) == 5 * 4 * 2 * 3
    assert len(bs.F64_CASES) == 13 * 8 * 2
    for c in bs.CASES:
        assert 3 * c.B <= 768 and c.D + c.C <= 30 and 1 <= c.D <= 28, c
        assert c.B == bs.block_of(c.nkt, c.kind) and (c.B + 31) // 32 == c.nkt, c
        if c.family in bs.M16D:
            assert c.C >= 2, c
    for f in bs.F64_CASES:
        assert sum(f.shape.sizes) == 4 * f.shape.B and f.shape.H == bs.H and f.shape.T == bs.TL, f


def test_every_instantiation_is_reached():
    want = bs.all_instantiations()
    assert len(want) == 13 * 16
    for name, cases, cell in (("exact", EXACT, bs.cells), ("float64", bs.F64_CASES, bs.f64_cells)):
        got = {cell(c) for c in cases}
        assert got == want, (name, sorted(want - got), sorted(got - want))
    # every block kind in every family at every tile count; the family's own kernel and tag
    for fam, spec in bs.FAMILIES.items():
        mine = [c for c in EXACT if c.family == fam]
        assert {(c.nkt, c.kind) for c in mine} == {(k, kind) for k in range(1, 9) for kind in bs.KINDS}, fam
        assert {bs.cells(c)[0] for c in mine} == {spec[3]} and {bs.cells(c)[3] for c in mine} == {spec[4]}, fam
    # the edge cases: every CT at nkt 1, 2, 5, 8, full and ragged
    for variant in ("big", "raw"):
        got = {bs.cells(c) for c in bs.CASES if c.variant == variant}
        tags = {bs.FAMILIES[f][4] for f in bs.M16D}
        assert got == {("coords", k, full, tag) for k in bs.EDGE_NKT for full in (True, False) for tag in tags}, variant
    raws = {(c.family, c.nkt, c.kind) for c in bs.CASES if c.variant == "raw"}
    for fam, nkt, kind in raws:
        b = bs.block_of(nkt, kind)
        assert {c.raw for c in bs.CASES if c.variant == "raw" and (c.family, c.nkt, c.kind) == (fam, nkt, kind)} \
            == {3 * b - 1, 2 * b - 1, 1}


def test_head_shapes_rotate_through_every_f32_part_family():
    for fam in ("fp32", "fp32_mfma", "fp32_diff_mfma", "bf16_f32", "mixed16_f32", "m16d_f32"):
        got = {(c.D, c.C) for c in EXACT if c.family == fam}
        assert set(bs.PAIRS) <= got, (fam, sorted(set(bs.PAIRS) - got))
    assert (24, 6) in {(c.D, c.C) for c in EXACT if c.family == "fp32_diff_mfma"}      # HEPT_DIFF_MFMA=1 at D = 24
    assert {c.C for c in EXACT if c.family == "m16d_crt"} == {3, 5}
    assert {(c.D, c.C) for c in bs.CASES if c.family == "m16d_crt" and c.variant != "exact"} == {(24, 3), (24, 5)}
    # the largest LDS request of the coords kernel stays below the 64 KiB that needs no raise (C = 28 at nkt = 8)
    big = [c for c in EXACT if c.family == "m16d_f32" and c.C == 28 and c.nkt == 8]
    assert big and 2 * 256 * 64 + 256 * 12 + 256 * 4 * 28 == 64512 < 65536


def test_source_references():
    for path, line, text in bs.REFS:
        with open(os.path.join(ROOT, path)) as f:
            lines = f.read().splitlines()
        assert text in lines[line - 1], f"{path}:{line} no longer holds {text!r}: {lines[line - 1]!r}"


@pytest.mark.parametrize("family", list(bs.FAMILIES))
def test_bounds_of_every_exact_case(family):
    for c in (c for c in bs.CASES if c.family == family):
        r = bs.bounds(c)
        assert r["weights_ok"], c.id
        assert r["least_negative"] <= bs.ZERO_WEIGHT_LOGIT and float(torch.tensor(bs.ZERO_WEIGHT_LOGIT).exp()) == 0.0
        assert r["max_numer"] <= 256 and 1 <= r["max_count"] <= 256, (c.id, r["max_numer"], r["max_count"])
        assert r["empty_rows"] >= bs.TL * bs.H, c.id                 # one per (table, head)
        facts = r["facts"]
        assert facts["perms"] and all(facts["differ"]), c.id
        assert len(facts["baits"]) == bs.TL * bs.H * 3 and min(facts["baits"]) >= 1, c.id
        d = bs.design(c)
        assert float(d["v"].abs().max()) <= 3 and d["vlim"] in (1, 3)
        assert not torch.equal(d["qpos"][0], d["qpos"][1]) and not torch.equal(d["kpos"][0], d["kpos"][1])
        if c.variant == "big":
            assert float((d["sqrt_w"][:, None] * d["coords"][None]).abs().max()) > 65504.0
        if c.variant == "raw":
            assert int(d["eff"][c.raw:].abs().max()) == 0, c.id
            if c.raw < d["n"] - 1:      # padding points keep non-zero coordinates in the caller's array: the kernel must drop them
                assert float(d["coords"][c.raw:].abs().max()) > 0, c.id


def test_backward_cases_reach_every_instantiation_and_stay_exact():
    want = {(spec[3], k, full) for spec in bs.BWD_FAMILIES.values() for k in range(1, 9) for full in (True, False)}
    assert len(want) == 64 and len(bs.BWD_CASES) == 4 * 8 * 3 and len(bs.BWD_F64_CASES) == 4 * 8 * 2
    assert {bs.bwd_cells(c) for c in bs.BWD_CASES} == want == {bs.bwd_f64_cells(c) for c in bs.BWD_F64_CASES}
    assert len(bs.BWD_BY_ID) == len(bs.BWD_CASES) and not set(bs.BWD_BY_ID) & set(bs.BY_ID)
    for fam in bs.BWD_FAMILIES:
        mine = [c for c in bs.BWD_CASES if c.family == fam]
        assert {(c.nkt, c.kind) for c in mine} == {(k, kind) for k in range(1, 9) for kind in bs.KINDS}, fam
        assert {(c.D, c.C) for c in mine} == set(bs.BWD_PAIRS), fam
    assert any(c.C > 6 for c in bs.BWD_CASES if c.family == "bwd_diff")     # more than one launch of six coordinate columns
    for path, line, text in bs.BWD_REFS:
        with open(os.path.join(ROOT, path)) as f:
            assert text in f.read().splitlines()[line - 1], (path, line)
    for c in bs.BWD_CASES:
        r = bs.bounds(c)
        assert r["weights_ok"] and min(r["baits"]) >= 1 and r["empty_rows"] >= bs.TL * bs.H, c.id
        d = bs.bwd_design(c)
        # a bf16 per-table row holds every integer up to 256; dS is rounded to bf16 by the bf16 kernel; Z and the reduced
        # sums are f32 integers
        assert d["table_max"] <= 256 and d["ds_max"] <= 256 and d["z_max"] < 2 ** 24, c.id
        assert float(d["dv"].abs().max()) <= bs.TL * 256 and float(d["dv"].abs().max()) > 0, c.id
        assert float(d["gacc"][..., c.D + 1:].abs().max()) == 0 and float(d["gacc"].abs().max()) == d["glim"], c.id


def test_cell_bounds_are_recorded_cells_at_twice_the_emulation():
    assert set(bs.F64_MODEL_ROW_CELL) <= set(bs.F64_BY_ID)
    assert all(bs.F64_BY_ID[c].family in bs.M16D for c in bs.F64_MODEL_ROW_CELL)
    assert bs.F64_MODEL_ROW_CELL == {"m16d_f32-k4full-b128-d16c6-f64": 4.3e-3} and 4.3e-3 <= 2 * 2.150e-3


def test_pair_groups_catch_a_leaked_coordinate_column():
    """Two pair rows share their coordinate column: a feature product that kept the stored coordinate columns beside the
    f32 coordinate part would give them the logit 0 instead of -s^2."""
    c = next(c for c in EXACT if c.family == "m16d_c6")
    feats, cds = bs.group_rows(c)
    a, b = feats.shape[0] - 2, feats.shape[0] - 1
    x = bs.emulate_logits(c)
    assert float(x[0, a, b]) == -bs.S * bs.S
    leak = (bs.sqrt_w_of(c)[0] * cds[a] * 16.0) @ (bs.sqrt_w_of(c)[0] * cds[b] * 16.0)
    assert float(x[0, a, b] + leak) == 0.0


def test_import_touches_no_gpu():
    code = ("import sys, torch; sys.path[:0] = [%r, %r]; import block_sweep as bs; "
            "bs.bounds(bs.CASES[0]); assert not torch.cuda.is_initialized(); print(len(bs.CASES))"
            % (os.path.join(ROOT, "tests"), ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout.strip()) == len(bs.CASES)
