"""Training in ``precision="fp32_diff"``, the parts that need no GPU: the C entry of the difference-form backward
(``hept_block_attn_bwd_diff``) is exported, declared and refuses what its siblings refuse, with their codes and in their
order, before any HIP call; ``ops.block_attn_bwd`` routes ``f32_mfma="diff"`` to it; the module trains f32 tiles.

Pointers are dummy 16-byte aligned host addresses, never dereferenced (tests/test_capi_refusals_host.py)."""
import os
import re

import pytest
import torch

from hept_amd import HEPTAttention, _lib, ops
from hept_amd.build import build

SHAPE, ARG = 1, 3
PTR = 0x10000
N, H, D, C, T, B = 256, 8, 24, 6, 3, 128
POINTERS = ("qhat", "kvhat", "qpos", "kpos", "gacc", "dq_part", "dkv_part")
DIFF = "qhat kvhat qpos kpos gacc N H D C Tl B dq_part dkv_part stream".split()
SIBLING = [a for a in DIFF if a != "C"]
ENTRIES = {"hept_block_attn_bwd_diff": DIFF, "hept_block_attn_bwd_f32mfma": SIBLING, "hept_block_attn_bwd": SIBLING}
BASE = dict({p: PTR for p in POINTERS}, N=N, H=H, D=D, C=C, Tl=T, B=B, stream=None)

# (fault, overrides, code): every one is refused by all three entries alike
COMMON = [(f"null {p}", {p: None}, ARG) for p in POINTERS] + [
    ("N=0", dict(N=0), SHAPE), ("H=0", dict(H=0), SHAPE), ("Tl=0", dict(Tl=0), SHAPE), ("B=0", dict(B=0), SHAPE),
    ("B=257", dict(B=257, N=257), SHAPE), ("N=250", dict(N=250), SHAPE), ("D=0", dict(D=0), SHAPE),
    ("D=29", dict(D=29, C=1), SHAPE),
    ("null qhat, N=250", dict(qhat=None, N=250), ARG),        # two faults: the pointers are checked first
    ("null dkv_part, D=0", dict(dkv_part=None, D=0), ARG),
]
# the coordinate range, which only the difference form takes
OWN = [("C=0", dict(C=0), SHAPE), ("C=-1", dict(C=-1), SHAPE), ("D+C=31", dict(C=7), SHAPE), ("D=28, C=3", dict(D=28, C=3), SHAPE),
       ("null gacc, C=0", dict(gacc=None, C=0), ARG)]


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def _call(lib, entry, overrides):
    vals = dict(BASE, **overrides)
    return getattr(lib, entry)(*[vals[a] for a in ENTRIES[entry]])


def test_symbol_is_exported_declared_and_bound(lib):
    assert hasattr(lib, "hept_block_attn_bwd_diff")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "hept_hip.h")).read()
    decl = re.search(r"int hept_block_attn_bwd_diff\(([^;]*)\);", header)
    assert decl, "hept_block_attn_bwd_diff is not declared in include/hept_hip.h"
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).replace("\n", " ").split(",")]
    assert names == DIFF
    assert len(_lib.SIGNATURES["hept_block_attn_bwd_diff"][1]) == len(DIFF)
    # one int (C) more than the siblings, which stay as they were
    assert len(_lib.SIGNATURES["hept_block_attn_bwd_f32mfma"][1]) == len(DIFF) - 1


def test_abi_version_is_unchanged(lib):
    assert _lib.ABI_VERSION == 22 and lib.hept_abi_version() == 22


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("fault", range(len(COMMON)), ids=lambda i: COMMON[i][0])
def test_refused_like_the_siblings(lib, entry, fault):
    _, overrides, code = COMMON[fault]
    overrides = {k: v for k, v in overrides.items() if k in ENTRIES[entry]}
    assert _call(lib, entry, overrides) == code


@pytest.mark.parametrize("fault", range(len(OWN)), ids=lambda i: OWN[i][0])
def test_coordinate_range_is_checked(lib, fault):
    _, overrides, code = OWN[fault]
    assert _call(lib, "hept_block_attn_bwd_diff", overrides) == code


class _Called(Exception):
    pass


class _FakeLib:
    """Stands in for the loaded library: records which backward entry ``ops.block_attn_bwd`` calls, and with what."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            raise _Called(name)
        return fn


@pytest.mark.parametrize("flag,entry,n_ints", [("diff", "hept_block_attn_bwd_diff", 6), (True, "hept_block_attn_bwd_f32mfma", 5),
                                               (False, "hept_block_attn_bwd", 5)])
def test_ops_maps_the_flag_to_the_entry(monkeypatch, flag, entry, n_ints):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(ops, "_stream", lambda t: None)
    monkeypatch.setattr(ops, "_f32c", lambda t, name: t)   # (host tensors: nothing is dereferenced)
    n, h, d, c, t, b = 64, 2, 8, 4, 3, 32
    qhat, kvhat = torch.zeros(h, n, 32), torch.zeros(h, n, 64)
    pos = torch.zeros(t, h, n, dtype=torch.int32)
    fn = getattr(ops.block_attn_bwd, "__wrapped__", ops.block_attn_bwd)
    with pytest.raises(_Called):
        fn(qhat, kvhat, pos, pos, torch.zeros(n, h, 32), d, c, b, f32_mfma=flag)
    (name, args), = fake.calls
    assert name == entry
    ints = args[5:5 + n_ints]
    assert ints == ((n, h, d, c, t, b) if flag == "diff" else (n, h, d, t, b))


def test_ops_reads_strided_permutations_densely(monkeypatch):
    """A permutation tensor that is a strided view (an argsort of permuted keys is one) reaches the kernel as a dense
    int32 copy, as ``ops.block_attn`` passes it: the kernel indexes it as (Tl, H, N) rows."""
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(ops, "_stream", lambda t: None)
    monkeypatch.setattr(ops, "_f32c", lambda t, name: t)
    n, h, t = 64, 2, 3
    pos = torch.zeros(h, n, t, dtype=torch.int64).permute(2, 0, 1)
    assert not pos.is_contiguous()
    fn = getattr(ops.block_attn_bwd, "__wrapped__", ops.block_attn_bwd)
    with pytest.raises(_Called):
        fn(torch.zeros(h, n, 32), torch.zeros(h, n, 64), pos, pos, torch.zeros(n, h, 32), 8, 4, 32, f32_mfma="diff")
    (_, args), = fake.calls
    assert args[2] != pos.data_ptr() and args[3] != pos.data_ptr()


def test_ops_refuses_an_unknown_flag(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _FakeLib())
    monkeypatch.setattr(ops, "_stream", lambda t: None)
    monkeypatch.setattr(ops, "_f32c", lambda t, name: t)
    fn = getattr(ops.block_attn_bwd, "__wrapped__", ops.block_attn_bwd)
    pos = torch.zeros(1, 1, 32, dtype=torch.int32)
    with pytest.raises(ValueError, match="f32_mfma"):
        fn(torch.zeros(1, 32, 32), torch.zeros(1, 32, 64), pos, pos, torch.zeros(32, 1, 32), 8, 4, 32, f32_mfma="dif")


@pytest.mark.parametrize("precision,tiles,flag", [("fp32_diff", "fp32", "diff"), ("fp32_mfma", "fp32", True),
                                                  ("fp32", "fp32", False), ("bf16", "fp32", False)])
def test_module_training_flags(precision, tiles, flag):
    m = HEPTAttention(30, h_dim=24, num_heads=8, block_size=100, n_hashes=3, num_w_per_dist=10, precision=precision)
    assert m._train_tiles() == tiles
    assert m._train_f32_mfma() == flag
    m.train_tiles = "bf16"   # the opt-in 16-bit training tiles do not apply to the f32-MFMA precisions
    assert m._train_tiles() == ("fp32" if precision in ("fp32_mfma", "fp32_diff") else "bf16")
