"""CPU: the src block's drop-in class (constructor refusals, the reference's state-dict layout) and the reach of its
shape sweep (tests/src_attn_sweep.py): every coordinate count x table chunking x sort path x kind of raw_size cell the
kernels can reach, so that shrinking the sweep fails here, not silently on the GPU."""
import pytest
import torch

import src_attn_sweep as ssw
from hept_amd import Attn, HEPTAttention, SrcAttn

CFG = dict(h_dim=24, num_heads=8, block_size=100, n_hashes=3, num_w_per_dist=10, n_layers=4, num_regions=150)

# The src block's state dict with attn_type="hept", pe_type="none", C = 6 (src/models/baselines/transformer.py:160-206):
# w_q/w_k/w_v (:168-170), attn = HEPTAttention(h_dim + coords_dim) (:174) with out_linear
# (src/models/attention/hept.py:64) and e2lsh alpha/beta (src/models/model_utils/hash_utils.py:343-344), norm1/norm2
# and ff (:196-202), w_rpe (:205)
SRC_STATE = [
    ("w_q.weight", (192, 24)), ("w_k.weight", (192, 24)), ("w_v.weight", (192, 24)),
    ("attn.out_linear.weight", (24, 192)), ("attn.out_linear.bias", (24,)),
    ("attn.e2lsh.alpha", (8, 30, 3)), ("attn.e2lsh.beta", (1, 3)),
    ("norm1.weight", (24,)), ("norm1.bias", (24,)), ("norm2.weight", (24,)), ("norm2.bias", (24,)),
    ("ff.0.weight", (24, 24)), ("ff.0.bias", (24,)), ("ff.2.weight", (24, 24)), ("ff.2.bias", (24,)),
    ("w_rpe.weight", (192, 50)), ("w_rpe.bias", (192,)),
]


def test_constructor_refusals():
    for attn_type in ("performer", "reformer", "smyrf", "sb", "flt", "pct", "flatformer", "full"):
        with pytest.raises(NotImplementedError):
            SrcAttn(attn_type, 6, pe_type="none", **CFG)
    for pe in ("learned", "fixed"):
        with pytest.raises(NotImplementedError, match="pe_type"):
            SrcAttn("hept", 6, pe_type=pe, **CFG)
    with pytest.raises(ValueError):
        SrcAttn("hept", 6, variant="example", **CFG)
    SrcAttn("hept", 6, **CFG)                      # no pe_type: the reference's pe_func = None
    blk = SrcAttn("hept", 6, pe_type="none", precision="bf16", **CFG)
    assert isinstance(blk, Attn) and isinstance(blk.attn, HEPTAttention)
    assert blk.attn.variant == "src" and blk.attn.precision == "bf16" and blk.attn_type == "hept"
    assert blk.pe_func is None


def test_state_dict_matches_the_reference_layout():
    blk = SrcAttn("hept", 6, pe_type="none", **CFG)
    got = [(k, tuple(v.shape)) for k, v in blk.state_dict().items()]
    assert sorted(got) == sorted(SRC_STATE)
    # a src checkpoint's entries load strictly; the frozen hash parameters stay frozen
    sd = {k: torch.randn(shape) for k, shape in SRC_STATE}
    blk.load_state_dict(sd, strict=True)
    assert not blk.attn.e2lsh.alpha.requires_grad and not blk.attn.e2lsh.beta.requires_grad
    assert torch.equal(blk.attn.e2lsh.beta, sd["attn.e2lsh.beta"])
    # Attn(c, variant="src") carries the same layout
    same = Attn(6, variant="src", **CFG)
    assert sorted((k, tuple(v.shape)) for k, v in same.state_dict().items()) == sorted(SRC_STATE)


def test_shape_ids_are_unique_and_shapes_valid():
    assert len(ssw.BY_ID) == len(ssw.SHAPES) and 20 <= len(ssw.SHAPES) <= 30
    for s in ssw.SHAPES:
        assert 8 <= s.B <= 256 and s.N % s.B == 0 and s.C in ssw.COORDS, s
        assert 1 <= s.raw <= s.N and s.N - s.raw < s.B, s    # prepare_input_src pads less than one block
        assert ssw.cost(s) <= ssw.COST_CAP, s
        ssw.raw_kind(s)


def _all(shapes):
    out = set()
    for s in shapes:
        out |= ssw.cells(s)
    return out


def test_every_cell():
    got = _all(ssw.SHAPES)
    kinds = [f"raw-{k}" for k in ssw.KINDS]
    want = {f"coords{c}/{k}" for c in ssw.COORDS for k in kinds}
    want |= {f"coords{c}/{ch}" for c in ssw.COORDS for ch in ("table-chunks", "tables-one-chunk")}
    want |= {f"coords{c}/{so}" for c in ssw.COORDS for so in ("sort-two-launch", "sort-one-workgroup")}
    want |= {f"{ch}/{so}" for ch in ("table-chunks", "tables-one-chunk") for so in ("sort-two-launch", "sort-one-workgroup")}
    # a single-point cloud has N = B <= 256 points: the one-workgroup sort only
    want |= {f"{so}/{k}" for so in ("sort-two-launch", "sort-one-workgroup") for k in kinds
             if not (so == "sort-two-launch" and k == "raw-single")}
    want |= {f"prep<{c},{tm}>" for c in ssw.COORDS for tm in (4, 8)}
    want |= {"pad-zero", "pad-later", "T1", "T3", "T8", "T9", "T17", "B100", "B128", "B256"}
    assert not want - got, sorted(want - got)
    assert any(s.B not in (100, 128, 256) and s.B % 32 for s in ssw.SHAPES)          # a small ragged block
    ns = {s.N for s in ssw.SHAPES}
    assert any(n < ssw.SMALL_CAP for n in ns) and ssw.SMALL_CAP in ns and any(n > ssw.SMALL_CAP for n in ns)
    for k in ssw.KINDS:                                  # both kinds of padding rows at every kind of raw_size
        if k != "full":
            assert {(ssw.raw_kind(s), s.later) for s in ssw.SHAPES} >= {(k, False), (k, True)}, k


def test_training_subset():
    got = _all(ssw.BWD_SHAPES)
    want = {f"bwd-coords{c}" for c in ssw.COORDS} | {f"bwd-raw-{k}" for k in ssw.KINDS}
    want |= {"bwd-sort-two-launch", "bwd-sort-one-workgroup", "bwd-table-chunks", "bwd-tables-one-chunk"}
    assert not want - got, sorted(want - got)
    assert set(ssw.TRAIN) == {"fp32", "bf16", "fp32_mfma"}


def test_padding_row_bound_only_where_one_real_point_shares_the_last_block():
    full = ssw.BY_ID["n1000-full-b100-t3-c6"]
    single = ssw.BY_ID["n100-single-b100-t3-c6"]
    for mode in ssw.TRAIN:
        assert ssw.row_bound(full, "w_q.weight", mode) == ssw.TRAIN_ROW[mode]
        assert ssw.row_bound(single, "ff.0.weight", mode) == ssw.TRAIN_ROW[mode]
        assert ssw.row_bound(single, "w_q.weight", mode) == ssw.PAD_ROW[mode]
