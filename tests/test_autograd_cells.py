"""CPU: the autograd sweep (tests/autograd_sweep.py) covers every contract cell on every module it applies to and in the
modes it was built for, its predicates agree with the source text they mirror, its float64 reference is the existing
sweeps' on their own ground, and the premises of its exact cells hold on the float64 oracle itself -- so that shrinking
the sweep, or a premise that was never true, fails here and not silently on the GPU."""
import os
import re

import pytest
import torch

import attn_sweep as asw
import autograd_sweep as ags
import shape_sweep as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_case_table():
    assert [c.id for c in ags.CASES] == ["op-generic", "op-tuned", "op-wide", "op-chunks", "op-src", "blk", "blk-composed",
                                         "blk-src", "stack2"]
    shape = {c.id: c.shape for c in ags.CASES}
    assert [(shape[i].H, shape[i].D, shape[i].C, shape[i].B, shape[i].T, shape[i].sizes) for i in
            ("op-generic", "op-tuned", "op-wide", "op-chunks")] == [
        (3, 5, 3, 32, 2, (100, 60)), (8, 24, 6, 32, 2, (100, 60)), (16, 8, 6, 32, 2, (128,)), (8, 24, 4, 32, 9, (96, 40))]
    assert ags.n_points(ags.BY_ID["op-generic"]) == 192
    for i in ("op-src", "blk-src"):
        assert (shape[i].N, shape[i].raw, shape[i].B, shape[i].T) == (224, 219, 32, 2)
    for i in ("blk", "blk-composed", "stack2"):
        assert (shape[i].C, shape[i].B, shape[i].T, shape[i].sizes) == (4, 32, 3, (100, 60))
    assert shape["blk-src"].C == 4 and ags.BY_ID["stack2"].layers == 2 and not ags.BY_ID["blk-composed"].fused
    for c in ags.CASES:     # Y: the next seed, another split of as many points (so other permutations)
        assert c.y.seed == c.shape.seed + 1 and c.y != c.shape._replace(seed=c.y.seed)
        assert ags.n_points(c, "Y") == ags.n_points(c, "X")
        assert len({x.shape.seed for x in ags.CASES}) == len(ags.CASES)
    assert ags.BY_ID["op-tuned"].modes == ags.BY_ID["blk"].modes == ("fp32", "fp32_mfma", "fp32_diff", "bf16")
    assert all(c.modes == ("fp32", "fp32_diff") for c in ags.CASES if c.id not in ("op-tuned", "blk"))
    assert len(ags.PARAMS) == len(set(ags.PARAMS))


def test_every_cell_on_every_module_and_mode():
    got = {c.id: ags.cells(c) for c in ags.CASES}
    every = set().union(*got.values())
    want = {"module:HEPTAttention", "module:HEPTAttention-src", "module:Attn", "module:SrcAttn", "module:AttnStack",
            "variant:example", "variant:src", "fused", "composed", "bwd-dsw-kernel", "bwd-dsw-torch", "table-chunks",
            "tables-one-chunk", "rows-tuned", "rows-generic"}
    want |= {f"precision:{m}" for m in ags.MODES}
    want |= {f"cell:{cell}" for cell in ags.CONTRACT}
    want |= {f"cell:{cell}/fp32_diff" for cell in ags.CONTRACT}
    want |= {f"cell:{cell}/bf16" for cell in ("subsets", "two-forwards", "upstream", "repeat", "twice", "leaf16")}
    assert not want - every, sorted(want - every)
    assert got["op-wide"] >= {"bwd-dsw-torch"} and got["op-chunks"] >= {"table-chunks", "bwd-dsw-kernel"}
    # every contract cell x every module it applies to
    modules = {m: [c for c in ags.CASES if f"module:{m}" in got[c.id]] for m in ags.MODULE.values()}
    for cell in ags.CONTRACT:
        for m, cs in modules.items():
            if cell == "onehot" and not m.startswith("HEPTAttention"):
                continue
            if cell == "leaf16" and m == "AttnStack":
                continue
            if cell == "checkpoint" and m in ("HEPTAttention-src", "AttnStack"):
                continue
            assert any(f"cell:{cell}" in got[c.id] for c in cs), (cell, m)
    for cid in ("op-tuned", "blk", "blk-src"):
        assert "cell:checkpoint" in got[cid]
    # the baseline of op-tuned and blk in all four training modes, of the others in fp32 and fp32_diff
    for cid in ("op-tuned", "blk"):
        assert {f"cell:baseline/{m}" for m in ags.MODES} <= got[cid]
    for c in ags.CASES:
        assert {"cell:baseline/fp32", "cell:baseline/fp32_diff", "cell:subsets/fp32", "cell:subsets/fp32_diff"} <= got[c.id]
    # cell 1 holds bias-only and coords-only on the operator, every single leaf and the trainer's subsets everywhere
    for c in ags.CASES:
        ins, params = ags.leaf_names(c)
        names = ags.subsets(c)
        assert {f"only-{nm}" for nm in ins + params} <= set(names)
        assert {"inputs-only", "params-only", "biases-only", "all-but-v"} <= set(names)
        if c.kind == "op":
            assert names["only-coords"] == {"coords"} and names["only-attn.out_linear.bias"] == {"attn.out_linear.bias"}
            assert names["biases-only"] == {"attn.out_linear.bias"}
        else:
            assert {"x-front-end-frozen", "operator-only-front-end-frozen", "ff-only"} <= set(names)
            assert len(params) == 14 * c.layers
            front = {nm for nm in params if nm.split(".", 2)[-1] in ags.FRONT or nm in ags.FRONT}
            assert not names["x-front-end-frozen"] & front and not names["operator-only-front-end-frozen"] & (front | {"x"})
            assert all(nm.rsplit(".", 2)[-2] in ("norm2", "0", "2") for nm in names["ff-only"])
    assert set(ags.FRONT) | set(ags.FF) | {"w_rpe.weight", "attn.out_linear.weight", "attn.out_linear.bias"} == \
        set(asw.GRAD_PARAMS)


def test_predicates_agree_with_the_sources():
    autograd = _src("hept_amd", "autograd.py")
    hept = _src("hept_amd", "hept.py")
    block = _src("hept_amd", "attn_block.py")
    assert f"if h * c <= {ags.DSW_LANES}:" in autograd
    assert re.search(r"^MAX_TABLES = (\d+)$", _src("hept_amd", "_lib.py"), re.M).group(1) == str(ags.MAX_TABLES) == "8"
    assert autograd.count("range(0, n_tables, MAX_TABLES)") == 2 and autograd.count("rows=rows") == 3
    # the tensors the dispatch consults: the seven leaves of the dispatch table, in the table's order
    m = re.search(r"if torch\.is_grad_enabled\(\) and any\(\s*t\.requires_grad for t in \(([^)]*)\)", hept)
    consulted = [x.strip() for x in m.group(1).replace("\n", " ").split(",")]
    assert consulted == ["query", "key", "value", 'kwargs["coords"]', 'kwargs["w_rpe"].weight', "self.out_linear.weight",
                         "self.out_linear.bias"]
    assert len(consulted) == len(ags.DISPATCH_LEAVES)
    assert 'light = self.precision in ("fp32", "fp32_mfma", "fp32_diff") and self.sharding is None' in hept
    assert set(ags.LIGHT) == {"fp32", "fp32_mfma", "fp32_diff"}
    assert 'any(t.requires_grad for t in (query, key, value, kwargs["coords"]))' in hept
    assert "not self.training and not torch.is_grad_enabled()" in block
    # the front end whose backward HeptPartialSumsFused skips when none of it requires grad: x, norm1, w_q, w_k, w_v
    assert "if any(need[i] for i in (0, 1, 2, 4, 5, 6)):" in autograd
    # every hand-written backward refuses a second derivative
    n_backward = len(re.findall(r"^    def backward\(", autograd, re.M))
    assert n_backward == 7 == len(re.findall(r"^    @staticmethod\n    @_first_order_only\n    def backward\(", autograd, re.M))
    assert "once_differentiable(backward)" in autograd


def test_dispatch_expectations():
    for prec in ags.DISPATCH_PRECISIONS:
        for training in (True, False):
            assert ags.expect_dispatch(prec, training, False, {"q"}) == (False, False)
            assert ags.expect_dispatch(prec, training, True, set()) == (False, False)
            for leaf in ags.OP_INPUTS:
                assert ags.expect_dispatch(prec, training, True, {leaf}) == (True, False)
    for leaf in ags.OP_PARAMS:
        assert ags.expect_dispatch("bf16", False, True, {leaf}) == (False, True)       # the one documented exception
        assert ags.expect_dispatch("bf16", True, True, {leaf}) == (True, False)
        assert ags.expect_dispatch("fp32_diff", False, True, {leaf}) == (True, False)
    assert set(ags.DISPATCH_LEAVES) == set(ags.OP_INPUTS) | set(ags.OP_PARAMS)


@pytest.fixture(scope="module")
def generic():
    """op-generic on the float64 oracle's own permutations: the baseline and the one-hot run of cell 5."""
    case = ags.BY_ID["op-generic"]
    a = ags.ref64(case, "X", None)
    return case, a


def test_reference_is_the_existing_sweeps_reference(generic):
    """ags.ref64 with the seed-5 upstream gradient is shape_sweep._grads64 / attn_sweep.grads64 on the same permutations."""
    case, a = generic
    qp, kp = a["perms"][0]
    old = sw._grads64(case.shape, ags.inputs(case), qp, kp)
    for nm, key in ags.OP16.items():
        assert torch.equal(a[nm], old[key]), nm
    blk = ags.BY_ID["blk"]
    b = ags.ref64(blk, "X", None)
    old = asw.grads64(blk.shape, ags.inputs(blk), *b["perms"][0])
    assert torch.equal(b["out"], old["y"])
    for nm in ("x", "coords") + asw.GRAD_PARAMS:
        assert torch.equal(b[nm], old[nm]), nm


def test_one_hot_premise_on_the_oracle(generic):
    case, a = generic
    n, r = ags.n_points(case), ags.ONE_HOT_ROW
    for r in (ags.ONE_HOT_ROW, ags.pad_row(case)):
        rows = ags.one_hot_rows(a["perms"][0], r, case.shape.B)
        got = ags.ref64(case, "X", a["perms"], ags.one_hot((n, case.shape.D), r))
        for nm, allowed in rows.items():
            assert ags.outside(got[nm], allowed) == 0.0, (r, nm)
            assert float(got[nm].abs().max()) > 0.0, (r, nm)
        assert r in rows["coords"] and len(rows["q"]) == 1
        assert case.shape.B <= len(rows["k"]) < n
        if r == ags.ONE_HOT_ROW:
            assert len(rows["coords"]) == ONE_HOT_ALLOWED, len(rows["coords"])
    assert ags.pad_row(case) == 100 and not bool(ags.inputs(case)["unpad_seq"][100])
    assert ags.pad_row(ags.BY_ID["op-wide"]) is None and ags.pad_row(ags.BY_ID["op-src"]) == 219


ONE_HOT_ALLOWED = 69  # rows of 192 that row 37's one-hot upstream gradient reaches on op-generic (the oracle's own sort)


def test_zero_upstream_gradient_on_the_oracle(generic):
    case, a = generic
    got = ags.ref64(case, "X", a["perms"], torch.zeros(ags.n_points(case), case.shape.D))
    for nm in ags.OP_INPUTS + ags.OP_PARAMS:
        assert bool(torch.isfinite(got[nm]).all()) and float(got[nm].abs().max()) == 0.0, nm


def test_subset_gradients_are_the_all_leaves_gradients_on_the_oracle(generic):
    case, a = generic
    for req in ({"coords"}, {"attn.out_linear.bias"}, {"q", "w_rpe.weight"}):
        got = ags.ref64(case, "X", a["perms"], req=req)
        for nm in ags.OP_INPUTS + ags.OP_PARAMS:
            if nm in req:
                assert torch.equal(got[nm], a[nm]), (req, nm)
            else:
                assert got[nm] is None, (req, nm)


def test_two_layers_carry_gradient_through_the_second():
    """stack2's reference: layer 1's parameters see their own column block of the upstream gradient plus what flows back
    through layer 2 -- its gradients change when layer 2's columns of the upstream gradient are zeroed."""
    case = ags.BY_ID["stack2"]
    full = ags.ref64(case, "X", None)
    assert full["out"].shape == (ags.n_points(case), 3 * asw.D)
    g = ags.g_out(full["out"].shape)
    g[:, 2 * asw.D:] = 0.0
    cut = ags.ref64(case, "X", full["perms"], g)
    assert float(cut["attns.1.ff.2.weight"].abs().max()) == 0.0
    assert not torch.equal(cut["attns.0.w_q.weight"], full["attns.0.w_q.weight"])
    assert float(cut["attns.0.w_q.weight"].abs().max()) > 0.0 and len(full["perms"]) == 2
