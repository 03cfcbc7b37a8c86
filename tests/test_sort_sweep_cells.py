"""CPU: the sort sweep (tests/sort_sweep.py) rests on the constants csrc/sort_tables.hip really has, its float32 mirror of
the dispatch and of bucket_id / bin_of puts every planted population where the cell says, the cells reach every reachable
instantiation and every branch tag (derived from the mirror's numbers, not declared), every float64 host key is exact
(the float32 key, every operation rounded on its own, equals it bit for bit after conversion), the file:line references
into csrc/ still match, and importing the module touches no GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sort_sweep as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "hept_amd", "csrc", "sort_tables.hip")) as _f:
    SRC = _f.read()


def _define(name):
    return int(re.search(rf"#define {name} (\d+)", SRC).group(1))


def _constexpr(name):
    return re.search(rf"constexpr (?:int|unsigned int|size_t) {name} = ([^;]+);", SRC).group(1).strip()


def test_constants_the_cells_rest_on():
    assert _define("HEPT_ID_BITS") == so.ID_BITS == 17 and _define("HEPT_TOP_BITS") == so.TOP_BITS == 8
    assert _define("HEPT_BKT_THREADS") == so.BKT_THREADS == 128 and _define("HEPT_BKT_CAP") == so.BKT_CAP == 1024
    assert _define("HEPT_LEAN_SLOTS") == so.LEAN_SLOTS == 4 and _define("HEPT_SMALL_SPLIT") == so.SMALL_SPLIT == 4
    assert int(_constexpr("SMALL_CAP")) == so.SMALL_CAP == 6144 and int(_constexpr("SMALL_BINS")) == so.SMALL_BINS == 4096
    assert int(_constexpr("SMALL_THREADS")) == so.SMALL_THREADS == 1024
    assert int(_constexpr("REGION_MAX_N")) == so.REGION_MAX_N == 131072 and int(_constexpr("EMBED_SHIFT")) == so.EMBED_SHIFT == 20
    assert _constexpr("BKT_CAP_LARGE") == "6 * HEPT_BKT_CAP" and so.LARGE_TILE == 6
    assert _constexpr("SORT_CHUNK") == "SORT_THREADS * SORT_ITEMS"
    assert int(_constexpr("SORT_THREADS")) * int(_constexpr("SORT_ITEMS")) == so.SORT_CHUNK == 4096
    # region_cap: the body, and the values the cells use
    body = re.search(r"constexpr unsigned int region_cap\(int N\) \{(.*?)\n\}", SRC, re.S).group(1)
    assert "unsigned int c = 1024;" in body and "while ((size_t)c * 32 < (size_t)N) c <<= 1;" in body
    assert [so.region_cap(n) for n in (6145, 32768, 32769, 65536, 65537, 131072)] == [1024, 1024, 2048, 2048, 4096, 4096]
    assert so.LOBINS == 512 and so.LEAN_MAX == 512 and so.NTOP == 256
    # the exact map: scale = 2^17 / 256 and 4096 / 256 are powers of two
    assert so.nominal_scale(so.BY_ID["inst-m0-n6145"]) == 512.0 and so.nominal_scale(so.BY_ID["inst-m2-n6144"]) == 16.0
    m1 = so.nominal_scale(so.BY_ID["inst-m1-n6145"])
    assert 509.9 < m1 < 510.0                                # the src bound 255 * 1.0001f + 1: no power of two


def test_source_references():
    for path, line, text in so.REFS:
        with open(os.path.join(ROOT, path)) as f:
            lines = f.read().splitlines()
        assert text in lines[line - 1], f"{path}:{line} no longer holds {text!r}: {lines[line - 1]!r}"


def test_cell_list():
    assert len(so.BY_ID) == len(so.CELLS)
    for c in so.CELLS:
        assert so.t0_of(c) >= 1 and so.tables_of(c) > so.t0_of(c) + c.Tl, c.id
        if c.N > so.REGION_MAX_N:
            assert so.n_segs(c) <= 2, c.id                   # above 131 072 keys at most two segments per call
        if c.N >= 4194304:
            assert c.mode == 2 and c.S == 1, c.id
        assert c.linear == (c.part == "ab")
    sizes = {m: {c.N for c in so.CELLS if c.part == "inst" and c.mode == m} for m in (0, 1, 2)}
    want = {1, 2, 3, 1023, 1024, 1025, 6143, 6144, 6145, 6148, 32768, 32769, 65536, 65537, 131072, 131073, 262144, 262145,
            1 << 20, (1 << 20) + 1}
    assert sizes[0] == sizes[1] == want and sizes[2] == want | {4194304, 4194305}
    for m in (0, 1, 2):                                      # Q = 1 on both sides: 128 / 130 segments, N = 1 024 / 1 025
        got = {(c.N, so.n_segs(c)): so.dispatch(c)["q"] for c in so.CELLS if c.part == "inst" and c.mode == m and c.N in (1024, 1025)}
        assert got[(1025, 128)] == 4 and got[(1025, 130)] == 1 and got[(1024, 128)] == 1
    # the region-size cells of part 2 run in both layouts, modes 0 and 2
    assert {c.id[3:] for c in so.AB_CELLS} == {c.id[7:] for c in so.CELLS if c.part == "region" and c.mode != 1}
    assert [c.lens for c in so.CELLS if c.part == "ragged"] == [(0, 1, 4095, 4096, 4097, 6144, 6145, 8199, 8200),
                                                                 (0, 1, 4095, 4096, 4097, 6144, 6143, 6144)]
    assert len(so.SCRATCH_CELLS) == 8 and so.SCRATCH_PATTERNS == ("zero", "ff")
    import scratch_sweep as ss
    assert set(so.SCRATCH_PATTERNS) <= set(ss.PATTERNS)


def test_every_instantiation_is_reached():
    want = so.all_instantiations()
    assert len(want) == 9 + 4 + 6
    got = set().union(*(so.dispatch(c)["inst"] for c in so.CELLS))
    assert got == want, (sorted(map(str, want - got)), sorted(map(str, got - want)))
    # ... by the part-1 cells and the child process alone, each at the smallest N that selects it
    inst = [c for c in so.CELLS if c.part in ("inst", "ab")]
    assert set().union(*(so.dispatch(c)["inst"] for c in inst)) == want
    only_ab = want - set().union(*(so.dispatch(c)["inst"] for c in so.GPU_CELLS))
    assert only_ab == {("bucket", 1024, True, 64, False)}    # below 131 073 keys the linear layout needs HEPT_SORT_LINEAR
    assert {("chunk", m, True, False) for m in (0, 2)} <= set().union(*(so.dispatch(c)["inst"] for c in so.AB_CELLS))


_tags = {}


@pytest.mark.parametrize("cid", [c.id for c in so.CELLS])
def test_cell_is_exact_and_planted(cid):
    c = so.BY_ID[cid]
    d = so.data(c)
    st = so.stats(c)
    _tags[cid] = so.tags(c)
    dp = st["dispatch"]
    # every float64 host key is exact: the float32 key evaluated with separate roundings equals it bit for bit
    host = so.host_keys(c, d)
    segs = so.segments(c, d)
    assert len(host) == len(segs) == so.n_segs(c)
    for (g, k32, length), k64 in zip(segs, host):
        k = (d["clean"][g] if c.mode == 2 else k32)[:length]
        assert k.dtype == np.float32 and k64.dtype == np.float64 and len(k64) == length
        same = k.astype(np.float64).view(np.int64) == k64.view(np.int64)
        zero = (k == 0) & (k64 == 0)                         # (-0.0 + 0.0 = +0.0 in either width; raw keys keep their sign)
        assert bool((same | zero).all()), cid
        fin = k64[np.isfinite(k64)]
        assert bool((fin * so.GRID == np.round(fin * so.GRID)).all()) and (fin.size == 0 or fin.max() <= 256.0), cid
    # the planted populations are where the cell says, in every segment (mode 1: through the inverted float32 map)
    if c.hots and dp["layout"] != "small" and not ({"cmax0", "inftail"} & c.opt) and c.lens is None:
        for s in st["segs"]:
            for hot in c.hots:
                b = so.hot_bucket(c, hot, s["group"])
                assert int(s["pop"][b]) == hot.n, (cid, s["group"], b, int(s["pop"][b]))
                if hot.spread == "all":
                    assert abs(2 * int(s["low"][b]) - hot.n) <= 1
                elif hot.spread == "edge":
                    assert int(s["maxgroup"][b]) == (hot.n + 1) // 2
                elif hot.spread[0] == "halves":
                    assert (int(s["low"][b]), hot.n - int(s["low"][b])) == hot.spread[1:]
                elif hot.spread[0] == "groups":
                    assert int(s["maxgroup"][b]) == max(hot.spread[1:])
                elif hot.spread[0] == "pile":
                    assert int(s["maxgroup"][b]) == hot.n
                if hot.chunks is not None:
                    want = np.zeros(dp["n_chunks"], int)
                    for ch, cnt in hot.chunks:
                        want[ch] = cnt
                    assert (s["runs"][:, b] == want).all(), (cid, b)
    assert max(int(s["maxgroup"].max()) for s in st["segs"]) <= 60032       # no pile beyond what is known to be quick
    assert _tags[cid] <= so.ALL_TAGS, _tags[cid] - so.ALL_TAGS


def test_every_branch_tag_is_reached():
    for c in so.CELLS:                                       # (when run alone)
        if c.id not in _tags:
            _tags[c.id] = so.tags(c)
    got = set().union(*_tags.values())
    assert got == so.ALL_TAGS, (sorted(so.ALL_TAGS - got), sorted(got - so.ALL_TAGS))
    gpu = set().union(*(_tags[c.id] for c in so.GPU_CELLS))
    assert gpu == so.ALL_TAGS                                 # ... without the child process
    t = lambda cid: _tags[cid]
    for m in (0, 1, 2):
        r = f"region-m{m}-"
        for nb in (1, 2, 511, 512):
            assert "general-one-pass" not in t(f"{r}nb{nb}") and "lean" in t(f"{r}nb{nb}")
        for nb in (513, 1023, 1024):
            assert {"general-one-pass", "lean"} <= t(f"{r}nb{nb}") and "two-pass" not in t(f"{r}nb{nb}") and "gathered" not in t(f"{r}nb{nb}")
        assert {"two-pass", "gathered"} <= t(f"{r}nb1025")    # capb == CAP: the collection and the two-pass path together
        for n in (6400, 32769):
            assert "two-pass" in t(f"{r}n{n}-nb2047") and "two-pass" in t(f"{r}n{n}-nb2048") and "splitters" not in t(f"{r}n{n}-nb2048")
            assert "splitters" in t(f"{r}n{n}-nb2049") and "two-pass" not in t(f"{r}n{n}-nb2049")
        assert "gathered" in t(f"{r}n6400-nb2047") and "gathered" not in t(f"{r}n32769-nb2048") and "gathered" in t(f"{r}n32769-nb2049")
        assert "gathered" not in t(f"{r}n65537-nb4096") and "gathered" in t(f"{r}n65537-nb4097")
        for name in ("1024-1024", "1024-1", "1-1024", "half-edge"):
            cid = f"{r}halves-{name}" if name != "half-edge" else f"{r}{name}"
            assert "two-pass" in t(cid) and not {"two-pass-refused-low", "two-pass-refused-high"} & t(cid), cid
        assert "two-pass-refused-low" in t(f"{r}halves-1025-1") and "two-pass-refused-low" in t(f"{r}lower-half")
        assert "two-pass-refused-high" in t(f"{r}halves-1-1025") and "two-pass-refused-high" in t(f"{r}upper-half")
        assert {"region-overflow-straddle", "region-overflow-whole-run", "gathered", "splitters"} <= t(f"{r}pool3")
        assert "region-overflow-straddle" in t(f"{r}straddle") and "region-overflow-whole-run" not in t(f"{r}straddle")
        assert "region-overflow-whole-run" in t(f"{r}whole-run")
        assert "scalar-load" in t(f"inst-m{m}-n6145") and "vec-load" in t(f"inst-m{m}-n6148")
        assert "table-wave" in t(f"inst-m{m}-n131073") and "table-wave" in t(f"inst-m{m}-n262144") and "table-lds" in t(f"inst-m{m}-n262145")
        assert "small-quarter-edge" in t(f"small-m{m}-quarter-edges") and "small-q4" in t(f"small-m{m}-one-quarter")
        assert "scale-zero" in t(f"small-m{m}-all-equal") if m == 2 else True
    assert "table-lds" in t("inst-m2-n4194304") and "table-global" in t("inst-m2-n4194305")
    for m in (0, 2):
        ln = f"linear-m{m}-"
        assert {"by-run", "by-position"} <= t(f"{ln}nb6143") and "two-pass" not in t(f"{ln}nb6144")
        assert "two-pass" in t(f"{ln}nb6145") and "two-pass" in t(f"{ln}nb12288") and "splitters" not in t(f"{ln}nb12288")
        assert "splitters" in t(f"{ln}nb12289")
        assert {"by-run", "by-position", "table-wave"} <= t(f"ab-m{m}-nb1025") and "lean" not in t(f"ab-m{m}-nb1025")
    for m in (0, 1):
        assert "scale-zero" in t(f"degen-m{m}-span0") and "scale-zero" in t(f"degen-m{m}-span0-small")
        assert "clamp-high" in t(f"degen-m{m}-inftail")
    assert {"clamp-high", "splitters", "gathered"} <= t("degen-m0-cmax0")
    assert "ragged-empty-chunk" in t("ragged-l8200") and "small-q4" in t("ragged-l6144")


def test_special_cells():
    # a run of length 0 in the middle of the chunk list
    for m in (0, 2):
        c = so.BY_ID[f"linear-m{m}-zero-run"]
        for s in so.stats(c)["segs"]:
            runs = s["runs"][:, so.hot_bucket(c, c.hots[0], s["group"])]
            assert runs[16] == 0 and runs[15] == 100 and runs[17] == 100 and len(runs) == 33
    # span 0: the identity; -0.0 next to +0.0; +inf behind a pile; the hot bucket of the ragged rows lies partly behind lens
    for m in (0, 1):
        c = so.BY_ID[f"degen-m{m}-span0"]
        assert all((w.numpy() == np.arange(c.N)).all() for w in so.expected(c, so.data(c)))
        c = so.BY_ID[f"degen-m{m}-inftail"]
        d = so.data(c)
        assert np.isinf(d["kproj"][..., -200:]).all() and np.isfinite(d["kproj"][..., :-200]).all()
    for m in (0, 1, 2):
        c = so.BY_ID[f"degen-m{m}-negzero"]
        d = so.data(c)
        x = d["keys"] if m == 2 else d["qproj"]
        neg = (x == 0) & np.signbit(x)
        assert neg.sum() > 100 and ((x == 0) & ~np.signbit(x)).sum() > 100
    c = so.BY_ID["ragged-l8200"]
    d = so.data(c)
    st = so.stats(c)
    assert np.isnan(d["keys"][1, 1:]).all() and (d["keys"][2, 4095:] == np.float32(-1e30)).all()
    full = so.stats(c)["segs"][8]
    part = st["segs"][3]
    b = so.hot_bucket(c, c.hots[0], 3)
    assert 0 < int(part["pop"][b]) < 1300 and int(full["pop"][so.hot_bucket(c, c.hots[0], 8)]) == 1300


def test_import_touches_no_gpu():
    code = ("import sys, torch; sys.path[:0] = [%r, %r]; import sort_sweep as so; "
            "so.stats(so.CELLS[0]); assert not torch.cuda.is_initialized(); "
            "assert 'scratch_sweep' not in sys.modules and 'hept_amd' not in sys.modules; print(len(so.CELLS))"
            % (os.path.join(ROOT, "tests"), ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout.strip()) == len(so.CELLS)
