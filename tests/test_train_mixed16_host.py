"""Host side of the 16-bit difference-form training path (``train_tiles = "mixed16"``, csrc/block_attn_bwd_coords.hip): the
C ABI, the module's dispatch table, the argument checks of ``ops.block_attn_bwd_coords`` and the coverage of the GPU
cells (tests/train16_sweep.py).  No GPU."""
import os
import re
import subprocess

import pytest
import torch

import train16_sweep as ts
from hept_amd import HEPTAttention, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ("fp32", "fp32_mfma", "fp32_diff", "bf16", "mixed16", "mixed16_diff")
F32_ONLY = ("fp32_mfma", "fp32_diff", "mixed16_diff")   # precisions whose default training ignores train_tiles = "bf16"


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "hept_hip.h")).read()
    assert re.search(r"\bint hept_block_attn_bwd_coords\(", header)
    assert "hept_block_attn_bwd_coords" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["hept_block_attn_bwd_coords"]
    assert len(args) == 17      # 7 pointers, raw_size, N, H, D, C, Tl, B, 2 pointers, the stream
    if os.path.exists(_lib.LIB_PATH):
        names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT hept_block_attn_bwd_coords\b", names)
    assert "block_attn_bwd_coords.hip" in open(os.path.join(ROOT, "hept_amd", "csrc", "Makefile")).read()


def test_abi_version_is_22():
    assert _lib.ABI_VERSION == 22
    assert 'hept_abi_version(void) { return 22; }' in open(os.path.join(ROOT, "hept_amd", "csrc", "capi.hip")).read()


def _module(precision):
    return HEPTAttention(30, precision=precision, h_dim=24, num_heads=8, block_size=32, n_hashes=2, num_w_per_dist=10)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_train_tiles_table(precision):
    m = _module(precision)
    assert m.train_tiles == "fp32"
    assert m._train_tiles() == "fp32"
    m.train_tiles = "bf16"
    assert m._train_tiles() == ("fp32" if precision in F32_ONLY else "bf16")
    m.train_tiles = "mixed16"
    if precision == "mixed16_diff":
        assert m._train_tiles() == "mixed16"
        assert m._train_f32_mfma() == "diff"
    else:
        with pytest.raises(ValueError, match="train_tiles"):
            m._train_tiles()
    m.train_tiles = "fp16"
    with pytest.raises(ValueError, match="train_tiles"):
        m._train_tiles()
    assert type(m).train_tiles == "fp32"     # the class default is untouched


def test_autograd_nodes_refuse_mixed16_tiles_without_the_difference_form():
    from hept_amd.autograd import _coords_tiles

    assert _coords_tiles("mixed16", "diff") is True
    assert _coords_tiles("fp32", "diff") is False and _coords_tiles("bf16", False) is False
    for flag in (False, True):
        with pytest.raises(ValueError, match="mixed16"):
            _coords_tiles("mixed16", flag)
    # a shape the backward cannot hold in LDS is refused by the node's forward, and by the op before anything is loaded
    assert _coords_tiles("mixed16", "diff", 28, 224) is True and _coords_tiles("mixed16", "diff", 6, 256) is True
    assert _coords_tiles("fp32", "diff", 28, 256) is False
    for c, b in ((26, 225), (28, 256)):
        assert ts.lds_bytes(b, c) > ts.LDS_MAX
        with pytest.raises(ValueError, match="LDS"):
            _coords_tiles("mixed16", "diff", c, b)
    for c, b in ((25, 256), (28, 224), (6, 256)):
        assert ts.lds_bytes(b, c) <= ts.LDS_MAX
        ops.check_bwd_coords_shape(c, b)


def _args(n=64, h=2, c=3, tl=2):
    return dict(qhat=torch.zeros(h, n, 32, dtype=torch.float16), kvhat=torch.zeros(h, n, 64, dtype=torch.float16),
                qpos=torch.zeros(tl, h, n, dtype=torch.int32), kpos=torch.zeros(tl, h, n, dtype=torch.int32),
                gacc=torch.zeros(n, h, 32), coords=torch.zeros(n, c), sqrt_w=torch.ones(h, c))


def _call(a, **kw):
    return ops.block_attn_bwd_coords(a["qhat"], a["kvhat"], a["qpos"], a["kpos"], a["gacc"], a["coords"], a["sqrt_w"], 24, 32, **kw)


BAD_SHAPES = {
    "qhat": torch.zeros(2, 64, 16, dtype=torch.float16), "kvhat": torch.zeros(2, 63, 64, dtype=torch.float16),
    "qpos": torch.zeros(2, 2, 63, dtype=torch.int32), "kpos": torch.zeros(1, 2, 64, dtype=torch.int32),
    "gacc": torch.zeros(64, 2, 31), "coords": torch.zeros(63, 3), "sqrt_w": torch.ones(2, 4),
}
BAD_TYPES = {
    "qhat": torch.zeros(2, 64, 32, dtype=torch.bfloat16), "kvhat": torch.zeros(2, 64, 64), "qpos": torch.zeros(2, 2, 64),
    "kpos": torch.zeros(2, 2, 64, dtype=torch.int16), "gacc": torch.zeros(64, 2, 32, dtype=torch.float64),
    "coords": torch.zeros(64, 3, dtype=torch.float16), "sqrt_w": torch.ones(2, 3, dtype=torch.float64),
}


@pytest.mark.parametrize("name", sorted(BAD_SHAPES))
def test_wrong_shapes_are_refused_before_anything_is_loaded(name, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded before the arguments were checked"))
    with pytest.raises(ValueError, match=name.replace("kpos", "qpos and kpos")):
        _call(dict(_args(), **{name: BAD_SHAPES[name]}))


@pytest.mark.parametrize("name", sorted(BAD_TYPES))
def test_wrong_dtypes_are_refused_before_anything_is_loaded(name, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded before the arguments were checked"))
    with pytest.raises(TypeError, match=name):
        _call(dict(_args(), **{name: BAD_TYPES[name]}))


def test_raw_size_out_of_range_is_refused(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded before the arguments were checked"))
    for raw in (-1, 65):
        with pytest.raises(ValueError, match="raw_size"):
            _call(_args(), raw_size=raw)


def test_block_attn_bwd_still_refuses_float16_rows():
    a = _args()
    with pytest.raises(TypeError, match="f32 or bf16 tiles"):
        ops.block_attn_bwd(a["qhat"], a["kvhat"], a["qpos"], a["kpos"], a["gacc"], 24, 3, 32)


# ---- the GPU cells of tests/train16_sweep.py
def test_cells_cover_every_instantiation():
    want = ts.all_instantiations()
    assert len(want) == 64
    assert {ts.cells(c) for c in ts.EXACT if c.variant == "bwd"} == want
    assert {ts.random_cells(c) for c in ts.RANDOM} == want
    assert len({c.id for c in ts.EXACT}) == len(ts.EXACT) and len({c.id for c in ts.RANDOM}) == len(ts.RANDOM)
    # the dispatch the cells mirror, and every compiled instantiation in the source
    src = open(os.path.join(ROOT, "hept_amd", "csrc", "block_attn_bwd_coords.hip")).read()
    for line in ("if (C == 2) HEPT_BWDC_GO(2);", "if (C == 4) HEPT_BWDC_GO(4);", "if (C == 6) HEPT_BWDC_GO(6);",
                 "HEPT_BWDC_GO(0);", "const bool full = B == 32 * nkt;", "nkt = (B + 31) / 32"):
        assert line in src, line
    assert [f"HEPT_BWDC_CASE({k})" in src for k in range(1, 9)] == [True] * 8
    # D = 24 (the forward writes packed partial rows) and another D in every CT; every case within the ABI's shape rules
    for ct in ts.CTS:
        ds_ = {c.D for c in ts.EXACT if c.variant == "bwd" and ts.ct_of(c.C) == ct}
        assert 24 in ds_ and len(ds_) >= 2, ct
    for c in ts.EXACT:
        assert 1 <= c.D <= 27 and c.C >= 2 and c.D + c.C <= 30 and 3 * c.B <= 768, c.id
    for c in ts.RANDOM:
        assert 1 <= c.shape.D <= 27 and c.shape.C >= 2 and c.shape.D + c.shape.C <= 30 and 3 * c.shape.B <= 768, c.id
    assert {ts.ct_of(c.C) for c in ts.EXACT if c.variant == "big"} == {2, 4, 6}
    assert [c for c in ts.EXACT if c.variant == "raw" and c.raw < 3 * c.B]
    # every cell fits the LDS of a CU; the widest row (d sqrt_w summed in torch: H * C > 64) is there, beyond 128 KB once
    every = [(c.B, c.C) for c in ts.EXACT] + [(c.shape.B, c.shape.C) for c in ts.RANDOM]
    assert max(ts.lds_bytes(b, c) for b, c in every) <= ts.LDS_MAX
    assert any(ts.lds_bytes(b, c) > 128 * 1024 and ts.H * c > 64 for b, c in every)
    assert "(size_t)5 * 32 * nkt * BPROW + 32 * nkt * 20 + (size_t)3 * 32 * nkt * cs * 4" in src


def test_rows_too_wide_for_the_lds_are_refused_before_any_launch():
    """C >= 26 on eight-tile blocks: HEPT_ERR_SHAPE from the size check alone (the pointers are never read)."""
    lib, fake = _lib.load(), 4096
    assert ts.lds_bytes(256, 28) > ts.LDS_MAX >= ts.lds_bytes(224, 28)
    rc = lib.hept_block_attn_bwd_coords(fake, fake, fake, fake, fake, fake, fake, 256, 256, 2, 2, 28, 1, 256, fake, fake, None)
    assert rc == 1
    assert lib.hept_block_attn_bwd_coords(fake, fake, fake, fake, fake, fake, fake, 257, 256, 2, 2, 28, 1, 128, fake, fake, None) == 1
    assert lib.hept_block_attn_bwd_coords(None, fake, fake, fake, fake, fake, fake, 256, 256, 2, 2, 28, 1, 128, fake, fake, None) == 3


@pytest.mark.parametrize("cid", [c.id for c in ts.EXACT if c.nkt in (1, 8) or c.variant != "bwd"])
def test_exact_design_premises(cid):
    """dS, the partial sums of dS . K^ and the per-table dv are integers that bf16 / f32 hold exactly."""
    import block_sweep as bs

    case = ts.EXACT_BY_ID[cid]
    d = bs.bwd_design(case)
    assert d["ds_max"] <= 256 and d["table_max"] <= 256 and d["z_max"] < 2 ** 24, (cid, d["ds_max"], d["table_max"], d["z_max"])
    assert d["facts"]["ok"]
    if case.variant == "raw":
        assert float(d["gacc"][case.raw:].abs().max()) > 0
