"""CPU checks of the scratch sweep (tests/scratch_sweep.py): every GPU allocation site of the Python layer is covered by a
case, the case list takes every combination of v-half writer, sort branch, table chunking and counter-clearing path, no
word of a final result is masked, and the proxy and the ledger do what the GPU test relies on."""
import ast
import os

import pytest
import torch

import scratch_sweep as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLOC = ("empty", "empty_like", "new_empty")


def _alloc_sites():
    """``file:function`` of every call of empty / empty_like / new_empty in hept_amd/*.py (the innermost named function)."""
    out = {}
    pkg = os.path.join(ROOT, "hept_amd")
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py"):
            continue
        tree = ast.parse(open(os.path.join(pkg, fn)).read())

        def visit(node, func):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                func = node.name
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ALLOC:
                out.setdefault(f"{fn}:{func}", []).append(node.lineno)
            for child in ast.iter_child_nodes(node):
                visit(child, func)

        visit(tree, "<module>")
    return out


def test_audit_table_is_complete_and_printed():
    print(f"\nscratch audit ({len(ss.AUDIT)} regions), findings: {ss.AUDIT_FINDINGS}")
    for region, writer, w_at, reader, r_at, note in ss.AUDIT:
        assert region and writer and reader and ":" in w_at and ":" in r_at, region
        print(f"  {region}\n      written first by {writer} ({w_at})\n      read first by    {reader} ({r_at})"
              + (f"\n      {note}" if note else ""))
    text = " ".join(r[0] for r in ss.AUDIT)
    for region in ("qhat", "kvhat v half", "qproj", "minmax", "ws.pos", "pos_chunk", "ws.part",            # carve()
                   "sort.pa", "sort.pb", "sort.tab", "sort.range", "sort.params", "rg.cnt", "rg.region"):   # carve_sort()
        assert region in text, f"the audit does not cover {region}"


def test_every_gpu_allocation_site_is_covered_by_a_case():
    found = _alloc_sites()
    assert sum(len(v) for v in found.values()) >= 60, "the AST walk lost the allocation calls"
    entries = {c.entry for c in ss.CASES}
    for site, lines in found.items():
        if site in ss.NOT_DRIVEN:
            assert ss.NOT_DRIVEN[site], site
            continue
        assert site in ss.SITES, (f"hept_amd/{site} (line {lines}) allocates with empty: add it to scratch_sweep.SITES with "
                                  f"a case that reaches it")
        assert set(ss.SITES[site]) & entries, f"{site}: no case of {ss.SITES[site]} in the case list"
    gone = (set(ss.SITES) | set(ss.NOT_DRIVEN)) - set(found)
    assert not gone, f"sites listed in scratch_sweep that no longer exist: {sorted(gone)}"
    assert not set(ss.SITES) & set(ss.NOT_DRIVEN)
    # what is left out is the host mirrors, the meta-tensor shape functions and the multi-GPU exchange, nothing else
    assert {s.split(":")[0] for s in ss.NOT_DRIVEN} <= {"prep.py", "library.py", "sharding.py", "ops.py"}
    assert [s for s in ss.NOT_DRIVEN if s.startswith("ops.py")] == ["ops.py:forward_sharded"]
    for c in ss.CASES:
        assert ss.expected_sites(c), f"{c.id} is expected to reach no allocation site"


def test_case_ids_are_unique_small_and_from_the_sweeps():
    assert len(ss.BY_ID) == len(ss.CASES)
    for c in ss.CASES:
        assert ss.case_points(c) <= ss.MAX_POINTS, c.id
        assert c.entry in ss.RUN, c.id
        d = ss.donor_of(c)
        assert d.entry == c.entry and d.id != c.id, (c.id, d.id)
        if c.entry != "prepare":
            assert ss.case_points(d) != ss.case_points(c), f"{c.id}: the donor {d.id} has the same point count"
    for sid in ss.OP_IDS + ss.TRAIN_OP_IDS:
        assert sid in ss.sw.BY_ID
    for sid in ss.SRC_IDS + ss.TRAIN_SRC_IDS:
        assert sid in ss.ssw.BY_ID
    # the issue's list of operator shapes and src shapes, all of them, in every precision whose scratch differs
    ops = {(c.shape, c.precision) for c in ss.CASES if c.entry == "op"}
    for sid in ("b8", "b33", "b100", "cloud-b-b1-100", "b256", "n6272", "t9-n6272", "t17", "h7d17c3", "h16d27c3", "n9000-b225"):
        s = ss.sw.BY_ID[sid]
        sigs = {ss.op_signature(s, p) for p in ss.PRECISIONS}
        assert {ss.op_signature(s, p) for (i, p) in ops if i == sid} == sigs, sid
    assert {c.shape for c in ss.CASES if c.entry == "src"} == set(ss.SRC_IDS)
    assert {c.precision for c in ss.CASES if c.entry == "train_op"} == {"fp32", "fp32_mfma", "fp32_diff", "bf16"}
    for entry in ("train_attn", "train_src"):
        assert {c.precision for c in ss.CASES if c.entry == entry} == set(ss.asw.TRAIN)
        pts = sorted({ss.case_points(c) for c in ss.CASES if c.entry == entry})
        assert pts[0] <= ss.SMALL_CAP < pts[-1], entry
    assert {c.extra for c in ss.CASES if c.entry == "attn"} >= {"bfloat16", "float16", None}
    for entry in ("stack", "stack_src"):
        pts = sorted(ss.case_points(c) for c in ss.CASES if c.entry == entry)
        assert pts[0] <= ss.SMALL_CAP < pts[-1] and all(c.extra[4] == 3 for c in ss.CASES if c.entry == entry)
    assert {(c.extra[0] > ss.SMALL_CAP, c.extra[1]) for c in ss.CASES if c.entry == "argsort"} == {
        (False, False), (False, True), (True, False), (True, True)}


def test_attn_cases_cover_every_row_builder_and_sort_cell():
    want = set()
    for s in ss.asw.SHAPES:
        if ss.sw.n_points(s) <= ss.MAX_POINTS:
            want |= {c for c in ss.asw.cells(s) if c.startswith(("prep<", "sort-", "table-chunks", "tables-one-chunk"))}
    got = set()
    for c in ss.CASES:
        if c.entry == "attn":
            got |= ss.asw.cells(ss.asw.BY_ID[c.shape])
    assert want <= got, sorted(want - got)


def test_branch_combinations():
    """Computed with the sweeps' own cells(): each v-half writer with each sort branch, each sort branch with one and with
    several table chunks, the stand-alone and the row-builder zero path, the src bounds in minmax."""
    cells = set()
    for c in ss.CASES:
        cells |= ss.case_cells(c)
    for sort in ("sort-one-workgroup", "sort-two-launch"):
        for writer in ("v-row-builder", "v-direct"):
            assert f"{writer}/{sort}" in cells, (writer, sort)
        for chunks in ("tables-one-chunk", "table-chunks"):
            assert f"{sort}/{chunks}" in cells, (sort, chunks)
    # riders exist only where the sort has a bucket launch to carry them (csrc/sort_tables.hip hept_sort_carries_rows)
    assert "v-riders/sort-two-launch" in cells and "v-riders/sort-one-workgroup" not in cells
    assert {"zero-stand-alone", "zero-row-builder", "src-bounds-in-minmax", "src-bounds-in-kernel"} <= cells
    # ... and the two-launch sort inside table chunks with the counters cleared per chunk, in every family
    for entry in ("op", "attn", "src"):
        assert any("sort-two-launch/table-chunks" in ss.case_cells(c) for c in ss.CASES if c.entry == entry), entry
    # the riders at one table run with f32 rows only (n9000-b225: "fp32" reads v in place at B = 225, the f32-MFMA rows
    # ride), and the 16-bit row types keep the v role there
    n9 = {c.precision: ss.case_cells(c) for c in ss.CASES if c.entry == "op" and c.shape == "n9000-b225"}
    assert "v-direct" in n9["fp32"] and "v-riders" in n9["fp32_mfma"] and "v-row-builder" in n9["bf16"]
    # direct v leaves the v half to nobody: b256 in "fp32" only
    b256 = {c.precision: ss.case_cells(c) for c in ss.CASES if c.entry == "op" and c.shape == "b256"}
    assert "v-direct" in b256["fp32"] and all("v-direct" not in v for p, v in b256.items() if p != "fp32")


def test_no_word_of_a_final_result_is_masked():
    for name, what, where in ss.MASKS:
        assert not any(f in name for f in ss.FINAL_RESULTS), f"mask {name!r} {what} names a final result"
        assert ":" in where, f"mask {name!r} needs the file:line that shows no kernel reads the words"
    for name, what, where in ss.ZERO_WORDS:
        assert ":" in where and what
    assert set(ss.IN_OUT) == {"sort_tables_src", "prep_hash", "attn_stack_forward", "attn_stack_forward_src"}
    assert ss.PATTERNS == ("leftover", "zero", "ff")


# ---- the proxy and the ledger, on CPU tensors ------------------------------------------------------------------------
def _cpu_guarded(dev):
    return dev.type == "cpu"


def test_proxy_fills_guards_and_payload_and_names_the_site():
    import hept_amd.ops as ops_mod

    real = ops_mod.torch
    with ss.scratch("ff", guarded=_cpu_guarded) as ledger:
        proxy = ops_mod.torch
        assert proxy is not real and proxy.float32 is torch.float32 and proxy.cat is torch.cat
        a = proxy.empty(3, 5, dtype=torch.float32, device="cpu")
        b = proxy.empty((2, 7), dtype=torch.int32, device="cpu")
        c = proxy.empty_like(a, dtype=torch.bfloat16)
        d = proxy.new_empty(a, (4,), dtype=torch.int64)
        e = proxy.Tensor.new_empty(a, 6)
        f = proxy.empty(0, dtype=torch.uint8, device="cpu")
        assert isinstance(a, proxy.Tensor)
    assert ops_mod.torch is real                      # the patch is undone, torch itself was never touched
    assert a.shape == (3, 5) and b.shape == (2, 7) and c.shape == (3, 5) and d.shape == (4,) and e.shape == (6,)
    assert (a.dtype, b.dtype, c.dtype, d.dtype, e.dtype) == (torch.float32, torch.int32, torch.bfloat16, torch.int64,
                                                             torch.float32)
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(c).all()) and bool((b == -1).all()) and bool((d == -1).all())
    assert f.numel() == 0 and len(ledger.entries) == 6
    assert ledger.sites == {"test_scratch_cells.py:test_proxy_fills_guards_and_payload_and_names_the_site"}
    for raw, nbytes, _ in ledger.entries:
        assert raw.numel() == nbytes + 2 * ss.GUARD and raw.data_ptr() % 16 == 0
        assert bool((raw[:ss.GUARD] == ss.GUARD_BYTE).all()) and bool((raw[ss.GUARD + nbytes:] == ss.GUARD_BYTE).all())
    assert a.data_ptr() == ledger.entries[0][0].data_ptr() + ss.GUARD
    ledger.check()
    with ss.scratch("zero", guarded=_cpu_guarded) as ledger:
        z = ops_mod.torch.empty(9, dtype=torch.float16, device="cpu")
    assert not bool(z.any())
    ledger.check()


def _overrun_here(proxy):
    return proxy.empty(8, dtype=torch.float32, device="cpu")


def test_ledger_reports_an_overrun_with_its_site_side_and_offset():
    with ss.scratch("zero", guarded=_cpu_guarded) as ledger:
        import hept_amd.ops as ops_mod

        ok = ops_mod.torch.empty(4, dtype=torch.float32, device="cpu")
        t = _overrun_here(ops_mod.torch)
    ok.fill_(1.0)
    ledger.check()
    raw, nbytes, site = ledger.entries[1]
    assert site == "test_scratch_cells.py:_overrun_here" and nbytes == 32
    wide = raw[ss.GUARD:].view(torch.float32)         # the same memory, deliberately viewed past its end
    wide[8 + 2] = 3.0                                 # the third float behind the payload
    with pytest.raises(AssertionError, match=r"_overrun_here.*after the end.*offset 8 "):
        ledger.check()
    wide[8 + 2] = torch.tensor([ss.GUARD_BYTE] * 4, dtype=torch.uint8).view(torch.float32)[0]
    ledger.check()
    raw[ss.GUARD - 1] = 0                             # one byte in front of the payload
    with pytest.raises(AssertionError, match=r"_overrun_here.*before the start.*offset -1 "):
        ledger.check()
    assert bool((t == 0).all())


def test_allocations_on_other_devices_pass_through_untouched():
    import hept_amd.ops as ops_mod

    with ss.scratch("ff") as ledger:                  # the default: GPU allocations only
        a = ops_mod.torch.empty(5, dtype=torch.float32, device="cpu")
        b = ops_mod.torch.empty_like(a)
        c = ops_mod.torch.new_empty(a, (2,))
        m = ops_mod.torch.empty(3, 4, device="meta")
    assert not ledger.entries and a.shape == (5,) and b.shape == (5,) and c.shape == (2,) and m.device.type == "meta"
    assert a.untyped_storage().nbytes() == 20         # no guards around it
    ledger.check()


def test_leftover_hands_out_the_donors_buffers():
    import hept_amd.ops as ops_mod

    def alloc(proxy, n):
        return proxy.empty(n, dtype=torch.float32, device="cpu")

    with ss.scratch("record", guarded=_cpu_guarded) as donor:
        big = alloc(ops_mod.torch, 100)
        big.copy_(torch.arange(100.0))
        small = alloc(ops_mod.torch, 10)
        small.fill_(7.0)
    donor.check()
    with ss.scratch("leftover", donor.pool, guarded=_cpu_guarded) as ledger:
        a = alloc(ops_mod.torch, 40)                  # fits the donor's first buffer: the same memory, as it stands
        b = alloc(ops_mod.torch, 25)                  # larger than the donor's second: its bytes repeated
        c = alloc(ops_mod.torch, 3)                   # a third allocation of the site: the last donor buffer again
    assert a.data_ptr() == big.data_ptr() and torch.equal(a, torch.arange(40.0))
    assert b.data_ptr() != small.data_ptr() and bool((b == 7.0).all()) and bool((c == 7.0).all())
    ledger.check()
    for raw, nbytes, _ in ledger.entries:
        assert bool((raw[ss.GUARD + nbytes:ss.GUARD + nbytes + ss.GUARD] == ss.GUARD_BYTE).all())
