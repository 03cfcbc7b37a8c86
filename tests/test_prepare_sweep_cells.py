"""CPU: the prepare_input sweep (tests/prepare_sweep.py) reaches every branch it was built for, its cell rules agree with
the constants in the sources, its generator reproduces the stored inputs, and the host mirror reproduces the anchors
that tests/golden/make_golden_prepare.py took from the REAL reference on every case (tie-aware: see prepare_sweep)."""
import os
import re

import numpy as np
import pytest
import torch

import prepare_sweep as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _has(cases, *names):
    return any(set(names) <= ps.cells(c) for c in cases)


@pytest.fixture(scope="module")
def golden():
    return ps.load_golden()


def test_case_ids_are_unique_and_counted():
    assert len(ps.BY_ID) == len(ps.CASES) == 84
    assert len(ps.EXAMPLE) == 50 and len(ps.SRC) == 34 and len(ps.REFUSED) == 5
    assert len({c.seed for c in ps.CASES}) == len(ps.CASES)
    # at most a few thousand points, except the sort-boundary cases
    for c in ps.EXAMPLE:
        assert sum(c.a.sizes) <= 3000 or c.id.startswith("sort-"), c.id
    assert {c.a.T for c in ps.EXAMPLE} == {1, 2, 3, 9} and {c.a.H for c in ps.EXAMPLE} == {1, 3, 8}


def test_cell_rules_agree_with_the_sources():
    sort = _src("hept_amd", "csrc", "sort_tables.hip")
    prepare = _src("hept_amd", "csrc", "prepare.hip")
    prep = _src("hept_amd", "prep.py")
    assert int(re.search(r"constexpr int SMALL_CAP = (\d+);", sort).group(1)) == ps.SMALL_CAP
    assert "if (L <= SMALL_CAP)" in sort                       # both argsort forms branch on the segment length
    assert int(re.search(r"constexpr int PROBE_CLOUDS = (\d+);", prepare).group(1)) == ps.PROBE_CLOUDS
    assert int(re.search(r"_MAX_CLOUDS_ONE_TRIP = (\d+)", prep).group(1)) == ps.PROBE_CLOUDS
    assert f"code_bits < {ps.KEY_BITS} ? {ps.KEY_BITS} - code_bits : 0" in prepare
    assert prep.count(f"(n_clouds << bits) >= (1 << {ps.KEY_BITS})") == 2        # the guard, on the probe path and on the torch path
    assert "16777216.f" in prepare and 2 ** ps.KEY_BITS == 16777216
    # the wrap rule, in the probe, in the entry and in the front end
    assert "size0 + n_raw < B" in prepare and "2 * n_raw - (n_clouds - 1) < (long long)B" in prepare
    assert "int(sizes[0]) + n_raw < block_size" in prep and "rec[4] & 2" in prep


def test_every_example_cell_is_taken():
    ex = [c for c in ps.EXAMPLE if not c.a.refuse]
    want = {
        # cloud sizes against the block
        "size-eqB", "size-B+1", "size-B-1", "no-pads", "block-1", "one-point-cloud", "every-cloud-below-B",
        # the wrap
        "wrap-first-cloud", "wrap-later-cloud", "wrap-into-last-cloud", "wrap-boundary",
        # region arithmetic
        "width-exact-multiple", "width-recip-differs", "regions-integer", "regions-thirds", "regions-over-cloud",
        "regions-below-2", "regions-draw", "regions-table",
        # ties
        "ties-eta", "ties-phi", "ties-both", "ties-negzero", "ties-identical-cloud",
        # code width
        "key-k0", "key-k-pos", "key-sh0", "key-sh-pos", "key-24-bits",
        # cloud count
        "clouds-1", "clouds-2", "clouds-254", "clouds-255", "clouds-256", "clouds-300", "probe-path", "torch-path",
        "batch-i32", "batch-i64",
        # sort paths
        "argsort-one-workgroup", "argsort-two-launch", "codesort-one-workgroup", "codesort-two-launch",
        "longest-6144", "longest-6145", "n_raw-6144", "n_raw-6145",
        # dtype, views
        "coords-f32", "coords-f64", "coords-bf16", "coords-f16", "view-strided", "view-regions-view",
        "T1", "T2", "T3", "T9", "H1", "H3", "H8",
    }
    got = set().union(*(ps.cells(c) for c in ex))
    assert not want - got, sorted(want - got)
    assert not any({"wrap-refused", "guard-refused"} & ps.cells(c) for c in ex)
    # joint cells: the boundary counts with both batch types, on both sides of the probe; a wrap into the last cloud of
    # two; the code sort's two-launch path under a one-workgroup argsort; k = 0 at exactly 24 bits; a strided float64
    for path, count in (("probe-path", "clouds-255"), ("torch-path", "clouds-256"), ("torch-path", "clouds-300")):
        assert _has(ex, path, count, "batch-i32") and _has(ex, path, count, "batch-i64"), (path, count)
    assert _has(ex, "wrap-first-cloud", "wrap-into-last-cloud", "clouds-2")
    assert _has(ex, "wrap-boundary", "clouds-1") and _has(ex, "wrap-boundary", "clouds-2")
    assert _has(ex, "argsort-one-workgroup", "codesort-two-launch") and _has(ex, "n_raw-6144", "codesort-one-workgroup")
    assert _has(ex, "key-k0", "key-24-bits", "key-sh-pos") and _has(ex, "key-k-pos", "key-sh-pos")
    assert _has(ex, "coords-f64", "view-strided")
    assert _has(ex, "width-recip-differs", "regions-integer", "width-exact-multiple")
    # the sizes the issue names
    sizes = {c.a.sizes: c.a.B for c in ps.EXAMPLE}
    for s, b in (((1, 1, 1, 70), 8), ((7,) * 40, 8), ((3, 40), 16), ((5, 11), 16), ((5, 10), 16), ((1, 12), 16),
                 ((10,), 64), ((6100, 45), 100), ((300, 150, 450, 7), 32)):
        assert sizes.get(s) == b, (s, b)


def test_refusal_cells():
    by = {c.id: ps.cells(c) for c in ps.REFUSED}
    wrap = {cid: cells for cid, cells in by.items() if "wrap-refused" in cells}
    assert len(wrap) == 4 and all("guard-refused" not in cells for cells in wrap.values())
    # refused on the probe path and on the torch path; by the C entry's own host check and by the caller alone
    assert any("probe-path" in c for c in wrap.values()) and any("torch-path" in c for c in wrap.values())
    assert any("wrap-refused-by-entry" in c for c in wrap.values())
    assert any("wrap-refused-by-caller-only" in c for c in wrap.values())
    # the first illegal batches: one point fewer than a legal case of the sweep
    legal = {(c.a.sizes, c.a.B) for c in ps.EXAMPLE if "wrap-boundary" in ps.cells(c)}
    assert ((5, 6), 16) in legal and ps.BY_ID["wrap-refused-5-5"].a.sizes == (5, 5)
    guard = [cid for cid, cells in by.items() if "guard-refused" in cells]
    assert guard == ["key-guard-refused"]
    # ... and the first table beyond the guard: one cloud fewer is the k = 0 case
    assert ps.BY_ID["key-guard-refused"].a.sizes[:-1] == ps.BY_ID["key-k0"].a.sizes
    assert ps.BY_ID["key-guard-refused"].a.regions == ps.BY_ID["key-k0"].a.regions


def test_every_src_cell_is_taken():
    want = {f"src-raw-{r}" for r in ("1", "B-1", "B", "B+1", "2B")} | {"src-B8", "src-B100", "src-B128", "src-N6144",
            "src-N6272", "src-sort-small", "src-sort-large", "src-padded", "src-no-pads", "ties-eta", "ties-both",
            "ties-negzero", "real-inf", "src-F1", "src-F3", "src-F24", "src-x-f32", "src-x-bf16", "src-x-grad",
            "src-x-kernel-pad", "src-x-torch-pad", "regions-integer", "regions-thirds", "regions-over-cloud",
            "regions-below-2", "width-exact-multiple", "width-recip-differs", "T1", "T2", "T3", "T9", "H1", "H3", "H8"}
    got = set().union(*(ps.cells(c) for c in ps.SRC))
    assert not want - got, sorted(want - got)
    for b in (8, 100, 128):
        for r in ("1", "B-1", "B", "B+1", "2B"):
            assert _has(ps.SRC, f"src-B{b}", f"src-raw-{r}"), (b, r)
    assert _has(ps.SRC, "real-inf", "src-padded") and _has(ps.SRC, "real-inf", "src-no-pads")
    assert _has(ps.SRC, "src-N6144", "src-padded") and _has(ps.SRC, "src-N6144", "src-no-pads")


def test_width_rule_and_key_shifts():
    """The Python restatements cells() uses, against torch's own float32 arithmetic and hand-worked values."""
    from hept_amd.prep import quantile_partition

    for n, r in ((49, 7.0), (150, 10.0), (150, 15.0), (300, 3.0), (7, 50.0), (40, 1.0), (33, 1 / 3), (211, 12.333333)):
        ids = quantile_partition(torch.arange(n), torch.tensor([[r]]))
        assert int(ids.max()) == ps.region_max(n, r), (n, r)
        width = int(torch.ceil(torch.tensor([r]).reciprocal() * n))
        assert width == ps.width_recip(n, r), (n, r)
    assert ps.width_recip(49, 7.0) == 8 and ps.width_true(49, 7.0) == 7      # float32(1 / 7) * 49 > 7
    assert ps.width_recip(300, 3.0) == ps.width_true(300, 3.0) == 100
    regions = torch.full((1, 2, 1), 1500.0)
    assert ps.key_shifts([1500, 40, 9], regions) == (24, 0, 11)
    assert not ps.guard_refuses(3, regions) and ps.guard_refuses(4, regions)
    assert ps.key_shifts(list(ps.BY_ID["key-sh-pos"].a.sizes), torch.full((1, 2, 3), 5.0))[1:] == (10, 2)


def test_golden_file_is_small_and_complete(golden):
    assert os.path.getsize(ps.GOLDEN) < 100 * 1024
    for c in ps.CASES:
        assert c.id + "/input" in golden, c.id
        assert (c.id + "/digest" in golden) != (c.id + "/raised" in golden and golden[c.id + "/raised"][0] != ""), c.id
    assert {k.split("/")[0] for k in golden} == set(ps.BY_ID)


@pytest.mark.parametrize("case", ps.RUNS, ids=lambda c: c.id)
def test_mirror_matches_the_reference_anchors(case, golden):
    mask = ps.check_anchors(case, golden)
    inp = ps.build(case)
    kind = case.a.coords if isinstance(case.a.coords, str) else case.a.coords[0]
    # tie cases leave at least half of each cloud's real points comparable (one cloud of "identical" is one point
    # repeated: none of it is, by construction)
    bounds = inp["starts"] if case.path == "example" else [0, inp["raw"]]
    for i, (s, e) in enumerate(zip(bounds[:-1], bounds[1:])):
        if kind == "identical" and i == case.a.coords[1]:
            assert not bool(mask[s:e].any())
            continue
        assert int(mask[s:e].sum()) * 2 >= e - s, (case.id, i, int(mask[s:e].sum()), e - s)
    if case.path == "example" and case.a.dtype == "f64":
        # the float32 roundings of the float64 values do not tie: the HIP path ranks what the mirror ranks
        f32 = dict(inp, coords=inp["coords"].float())
        assert bool(ps.unique_mask(f32).all()) and bool(mask.all()), case.id


@pytest.mark.parametrize("case", ps.REFUSED, ids=lambda c: c.id)
def test_refused_cases_raise_in_the_mirror_what_the_reference_raises(case, golden):
    name, message = golden[case.id + "/raised"]
    assert np.array_equal(ps.input_checksum(ps.build(case)), golden[case.id + "/input"])
    if case.a.refuse == "ValueError":       # this project's own limit (exact fp32 sort keys): the reference and the
        assert name == ""                   # CPU mirror, which sorts integers, both run the case
        ps.check_anchors(case, golden)
        return
    assert name == case.a.refuse == "IndexError"
    with pytest.raises(IndexError) as err:
        ps.mirror(case)
    # the same error about the same dimension; the reference names its first bad index (cloud 0's first pad slot), the
    # mirror's one gather whichever it meets first
    tail = " is out of bounds for dimension 0 with size %d" % sum(case.a.sizes)
    assert str(err.value).startswith("index -") and str(err.value).endswith(tail) and message.endswith(tail)
    a = case.a
    assert a.sizes[0] + sum(a.sizes) < a.B and f"index {a.sizes[0] - a.B} is out of bounds" in message


def test_window_codes_restates_the_reference_rule():
    """window_codes (the GPU test's pad-slot invariant) against pad_and_unpad on a case with wraps and equal codes."""
    case = ps.BY_ID["one-point-clouds"]
    inp = ps.build(case)
    pad_seq, kw, unpad = ps.mirror(case, inp)
    codes = kw["combined_shifts"]
    assert torch.equal(codes[0, 0][~unpad], ps.window_codes(codes[0, 0][unpad], list(case.a.sizes), case.a.B))
    assert int((~unpad).sum()) == 7 + 7 + 7 + 2
