"""precision="mixed16_diff" (HEPT_PREC_MIXED16_DIFF = 5) as far as it goes without a GPU: the constant and its string, the
new staged entry in header / library / ctypes table, the workspace size, and what refuses the mode -- the table-sharded
entries and the block attention entries that have no coordinates to give the kernel (dummy pointers, never
dereferenced: every call is refused before any HIP call, as in test_capi_refusals_host.py)."""
import ctypes
import os
import re

import pytest

import test_capi_refusals_host as rh
from hept_amd import HEPTAttention, _lib, ops
from hept_amd.build import LIB_PATH, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG, PTR = rh.SHAPE, rh.ARG, rh.PTR
N, H, D, C, T, B = rh.N, rh.H, rh.D, rh.C, rh.T, rh.B
M16D = 5


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def test_constant_and_string():
    assert _lib.PREC_MIXED16_DIFF == M16D
    text = open(os.path.join(ROOT, "include", "hept_hip.h")).read()
    assert re.search(r"#define HEPT_PREC_MIXED16_DIFF 5\b", text)
    assert ops.precision_code("mixed16_diff") == M16D and ops.precision_code(M16D) == M16D
    with pytest.raises(ValueError, match="mixed16_diff"):
        ops.precision_code("fp8")
    with pytest.raises(ValueError):
        ops.precision_code(9)


def test_abi_version_stays_22(lib):
    assert lib.hept_abi_version() == 22 and _lib.ABI_VERSION == 22


def test_new_entry_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hept_hip.h")).read(), flags=re.S)
    decl = re.search(r"int hept_block_attn_coords\s*\((.*?)\);", text, flags=re.S)
    assert decl, "hept_block_attn_coords is not declared in include/hept_hip.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES["hept_block_attn_coords"]
    assert res is ctypes.c_int and len(argtypes) == len(args) == 15
    for a, ty in zip(args, argtypes):   # pointers as void*, sizes as int, in the header's order
        assert (ty is ctypes.c_void_p) == ("*" in a), a
    assert hasattr(ctypes.CDLL(LIB_PATH), "hept_block_attn_coords")


def test_part_rows_follow_the_16_bit_rule(lib):
    assert lib.hept_part_precision(M16D, 24) == _lib.PREC_BF16
    assert lib.hept_part_precision(M16D, 16) == _lib.PREC_F32
    assert ops.packed_partials("mixed16_diff", 24) and not ops.packed_partials("mixed16_diff", 20)


@pytest.mark.parametrize("shape", [(60032, 8, 24, 6, 3, 128), (256, 8, 24, 6, 3, 128), (800, 16, 27, 3, 2, 100),
                                   (6272, 8, 24, 6, 9, 128), (512, 3, 10, 6, 1, 256), (64, 5, 2, 28, 1, 32)])
def test_workspace_is_the_mixed16_size_plus_the_record(lib, shape):
    n, h, d, c, t, b = shape
    base = lib.hept_workspace_bytes(n, h, d, c, t, b, _lib.PREC_MIXED16)
    record = (h * c * 4 + 255) // 256 * 256
    assert lib.hept_workspace_bytes(n, h, d, c, t, b, M16D) == base + record
    assert ops.workspace_bytes(n, h, d, c, t, b, "mixed16_diff") == base + record
    # every other precision keeps its size
    assert lib.hept_workspace_bytes(n, h, d, c, t, b, _lib.PREC_BF16) == base


@pytest.mark.parametrize("entry", rh.PART + rh.BEGIN + rh.HEADS + rh.SHARDED)
def test_table_sharded_entries_refuse_the_mode(lib, entry):
    over = dict(precision=M16D)
    if entry in rh.SHARDED:   # a dummy communicator: the refusal comes before anything reads it
        over["comm"] = PTR
    assert rh.call(lib, entry, over) == SHAPE
    # ... in the existing order: the sizes come first, and the mode before the workspace
    assert rh.call(lib, entry, dict(over, workspace_bytes=16)) == SHAPE
    if "acc_precision" in rh.SIG[entry]:
        assert rh.call(lib, entry, dict(over, acc_precision=_lib.PREC_BF16)) == SHAPE
    if entry not in rh.SHARDED:
        null = "workspace" if entry in rh.HEADS else "q"
        assert rh.call(lib, entry, dict(over, **{null: None})) == ARG


def test_whole_operator_entries_take_the_mode_to_the_workspace_check(lib):
    """hept_forward* and the one-call blocks run the mode: with dummy pointers they get as far as the workspace check."""
    for entry in rh.FWD + rh.BLOCK:
        assert rh.call(lib, entry, dict(precision=M16D, workspace_bytes=16)) == ARG
        need = lib.hept_workspace_bytes(N, H, D, C, T, B, M16D)
        assert rh.call(lib, entry, dict(precision=M16D, workspace_bytes=need - 1)) == ARG


def test_block_attn_without_coordinates_refuses_the_mode(lib):
    assert lib.hept_block_attn(PTR, PTR, PTR, PTR, N, H, D, T, B, M16D, PTR, None) == SHAPE
    assert lib.hept_block_attn_heads(PTR, PTR, PTR, PTR, N, H, D, T, B, M16D, 0, H, H, 0, N, PTR, None) == SHAPE
    assert lib.hept_block_attn(PTR, PTR, PTR, PTR, N, H, D, T, B, 9, PTR, None) == SHAPE


def test_block_attn_coords_checks_its_arguments(lib):
    f = lib.hept_block_attn_coords
    good = dict(qhat=PTR, kvhat=PTR, qpos=PTR, kpos=PTR, coords=PTR, sqrt_w=PTR, raw_size=N, N=N, H=H, D=D, C=C, Tl=T,
                B=B, part=PTR, stream=None)

    def call(**over):
        return f(*dict(good, **over).values())

    for name in ("qhat", "kvhat", "qpos", "kpos", "coords", "sqrt_w", "part"):
        assert call(**{name: None}) == ARG, name
    assert call(N=250) == SHAPE and call(B=257) == SHAPE and call(D=29) == SHAPE
    assert call(C=1) == SHAPE and call(C=7) == SHAPE          # D + C > 30
    assert call(raw_size=-1) == SHAPE and call(raw_size=N + 1) == SHAPE


def test_custom_ops_pass_the_string_through():
    """hept_amd/library.py: the torch.compile nodes take the precision as a string; under FakeTensorMode they run their
    shape-only kernels."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode

    from hept_amd import library  # noqa: F401  (registers the ops)

    with FakeTensorMode():
        n = 1024
        f = lambda *s, dt=torch.float32: torch.empty(*s, device="cuda", dtype=dt)  # noqa: E731
        out = torch.ops.hept_amd.forward(f(n, 192), f(n, 192), f(n, 192), f(n, 6), f(3, 8, n, dt=torch.int64),
                                         f(192, 50), f(8, 30, 3), f(24, 192), f(24), 128, 10, "mixed16_diff")
        assert tuple(out.shape) == (n, 24) and out.dtype == torch.float32


def test_module_refuses_a_process_group():
    kw = dict(h_dim=24, num_heads=8, block_size=64, n_hashes=2, num_w_per_dist=10)
    m = HEPTAttention(30, precision="mixed16_diff", **kw)
    assert m._train_f32_mfma() == "diff" and m._train_tiles() == "fp32"
    m.train_tiles = "bf16"
    assert m._train_tiles() == "fp32"
    with pytest.raises(ValueError, match="mixed16_diff.*not table-sharded"):
        HEPTAttention(30, precision="mixed16_diff", process_group=object(), **kw)
