"""bf16 / fp16 query, key, value at the C ABI (the ``*_in`` entry points): declared, exported, bound, numbered.
Host side only: no compute call is made here."""
import ctypes
import os
import re

import pytest

from hept_amd import _lib, ops
from hept_amd.build import LIB_PATH, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_SYMBOLS = ("hept_forward_in", "hept_forward_src_in", "hept_forward_partial_in", "hept_forward_partial_src_in",
              "hept_prep_hash_in")


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "hept_hip.h")).read()


def test_in_entry_points_declared_exported_and_bound(lib):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    raw = ctypes.CDLL(LIB_PATH)
    for nm in IN_SYMBOLS:
        assert re.search(rf"\bint {nm}\s*\(\s*const void\* q, const void\* k, const void\* v, int in_dtype,", code), nm
        assert hasattr(raw, nm), f"{nm} is not exported"
        assert nm in _lib.SIGNATURES, f"{nm} has no ctypes signature"
        # one argument (in_dtype) more than the f32 twin, everything else in the twin's order
        twin = _lib.SIGNATURES[nm[:-3]][1]
        assert _lib.SIGNATURES[nm][1] == twin[:3] + [ctypes.c_int] + twin[3:], nm


def test_in_constants_and_abi_version(lib):
    text = _header()
    for macro, val in (("HEPT_IN_F32", ops.IN_F32), ("HEPT_IN_BF16", ops.IN_BF16), ("HEPT_IN_F16", ops.IN_F16)):
        assert re.search(rf"#define {macro} {val}\b", text), macro
    assert (ops.IN_F32, ops.IN_BF16, ops.IN_F16) == (0, 1, 2)
    assert _lib.ABI_VERSION == 22
    assert lib.hept_abi_version() == 22


def test_in_entry_points_reject_null_pointers_before_any_launch(lib):
    assert lib.hept_forward_in(None, None, None, ops.IN_BF16, *([None] * 6), 128, 8, 24, 6, 10, 3, 128, 0, None, 0, None,
                               None) == 3
    assert lib.hept_prep_hash_in(None, None, None, ops.IN_F16, *([None] * 4), 128, 128, 8, 24, 6, 3, 0, 3, 0,
                                 *([None] * 6)) == 3
