"""The 16-bit entry points of the Attn block without a GPU: declared in the header in the stated argument order,
exported, bound with the twin's signature plus one ``c_int`` behind ``x``, ABI version unchanged, and refused on dummy
host addresses before any HIP call (null pointers, an unknown element type, a misaligned 16-bit base)."""
import ctypes
import os
import re

import pytest

from hept_amd import _lib, ops
from hept_amd.build import build

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hept_hip.h")
# new entry point -> (its f32 twin, index of x among the arguments)
TWINS = {
    "hept_prep_hash_fused_in": ("hept_prep_hash_fused", 0),
    "hept_combine_ffn_io": ("hept_combine_ffn", 10),
    "hept_attn_block_forward_io": ("hept_attn_block_forward", 0),
    "hept_attn_block_forward_src_io": ("hept_attn_block_forward_src", 0),
}
HAS_Y = {"hept_combine_ffn_io", "hept_attn_block_forward_io", "hept_attn_block_forward_src_io"}
OK, ERR_SHAPE, ERR_ARG = 0, 1, 3
N, H, D, C, K, T, B = 256, 8, 24, 6, 10, 3, 128
PTR = 0x10000   # 16-byte aligned, never dereferenced: every call below is refused first
F32, BF16, F16 = _lib.IN_F32, _lib.IN_BF16, _lib.IN_F16


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def _declared_args(name):
    """[(type, name), ...] of a prototype in include/hept_hip.h."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/hept_hip.h"
    out = []
    for arg in m.group(1).split(","):
        typ, nm = re.match(r"\s*(.*?)(\w+)\s*$", arg, flags=re.S).groups()
        out.append((" ".join(typ.split()), nm))
    return out


@pytest.mark.parametrize("name", TWINS)
def test_declared_like_the_twin_with_io_dtype_behind_x(name):
    twin, xi = TWINS[name]
    new, old = _declared_args(name), _declared_args(twin)
    assert len(new) == len(old) + 1
    assert new[xi] == ("const void*", "x") and new[xi + 1] == ("int", "io_dtype") and old[xi] == ("const float*", "x")
    rest_new, rest_old = new[:xi] + new[xi + 2:], old[:xi] + old[xi + 1:]
    for (tn, nn), (to, no) in zip(rest_new, rest_old):
        assert nn == no
        if nn == "y":
            assert (tn, to) == ("void*", "float*")
        else:
            assert tn == to, (name, nn)
    assert ("y" in [nm for _, nm in new]) == (name in HAS_Y)


@pytest.mark.parametrize("name", TWINS)
def test_bound_signature_is_the_twins_plus_one_int(lib, name):
    twin, xi = TWINS[name]
    res, args = _lib.SIGNATURES[name]
    tres, targs = _lib.SIGNATURES[twin]
    assert res is tres and list(args) == list(targs[:xi + 1]) + [ctypes.c_int] + list(targs[xi + 1:])
    fn = getattr(lib, name)      # exported (AttributeError otherwise) and bound by _lib.load
    assert fn.restype is res and list(fn.argtypes) == list(args)


def test_abi_version_is_unchanged(lib):
    assert _lib.ABI_VERSION == 22 and lib.hept_abi_version() == 22
    assert (F32, BF16, F16) == (0, 1, 2) and ops._IN_CODE[__import__("torch").bfloat16] == BF16


def _params(null_field=None):
    st = _lib.AttnParams()
    for f, _ in _lib.AttnParams._fields_:
        if f not in ("eps1", "eps2"):
            setattr(st, f, PTR)
    st.eps1 = st.eps2 = 1e-5
    if null_field:
        setattr(st, null_field, None)
    return st


def _block(lib, src, x=PTR, io=BF16, y=PTR, st=None, d=D, n=N, ws_bytes=1 << 40, codes=PTR):
    st = _params() if st is None else st
    tail = (ctypes.byref(st), n, H, d, C, K, T, B, _lib.PREC_BF16, PTR, ws_bytes, y, None)
    if src:
        return lib.hept_attn_block_forward_src_io(x, io, PTR, codes, PTR, PTR, N - 3, *tail)
    return lib.hept_attn_block_forward_io(x, io, PTR, codes, *tail)


def _prep(lib, x=PTR, io=BF16, d=D, kvhat=PTR):
    return lib.hept_prep_hash_fused_in(x, io, PTR, PTR, 1e-5, PTR, PTR, PTR, PTR, PTR, PTR, PTR, N, N, H, d, C, T, 0, T,
                                       _lib.PREC_F32, PTR, kvhat, PTR, PTR, PTR, None)


def _ffn(lib, x=PTR, io=BF16, y=PTR, d=D, part=PTR):
    return lib.hept_combine_ffn_io(part, _lib.PREC_F32, T, N, H, d, 0, N, PTR, PTR, x, io, PTR, PTR, 1e-5, PTR, PTR, PTR,
                                   PTR, y, None)


@pytest.mark.parametrize("io", [F32, BF16, F16])
def test_null_pointers_are_refused_before_any_launch(lib, io):
    for src in (False, True):
        assert _block(lib, src, x=None, io=io) == ERR_ARG
        assert _block(lib, src, y=None, io=io) == ERR_ARG
        assert _block(lib, src, codes=None, io=io) == ERR_ARG        # (src: eta_idx)
        assert _block(lib, src, st=_params("ff2_w"), io=io) == ERR_ARG
        assert _block(lib, src, x=None, d=20, io=io) == ERR_ARG      # nulls come first
    assert _prep(lib, x=None, io=io) == ERR_ARG and _prep(lib, kvhat=None, io=io) == ERR_ARG
    assert _ffn(lib, x=None, io=io) == ERR_ARG and _ffn(lib, y=None, io=io) == ERR_ARG
    assert _ffn(lib, part=None, io=io) == ERR_ARG


def test_unknown_element_type_and_misaligned_16bit_base_are_argument_errors(lib):
    for bad in (3, -1, 7):
        assert _block(lib, False, io=bad) == ERR_ARG and _block(lib, True, io=bad) == ERR_ARG
        assert _prep(lib, io=bad) == ERR_ARG and _ffn(lib, io=bad) == ERR_ARG
    for io in (BF16, F16):
        for off in (2, 4, 8):
            assert _block(lib, False, x=PTR + off, io=io) == ERR_ARG
            assert _block(lib, True, x=PTR + off, io=io) == ERR_ARG
            assert _block(lib, False, y=PTR + off, io=io) == ERR_ARG
            assert _prep(lib, x=PTR + off, io=io) == ERR_ARG
            assert _ffn(lib, x=PTR + off, io=io) == ERR_ARG and _ffn(lib, y=PTR + off, io=io) == ERR_ARG


@pytest.mark.parametrize("io", [F32, BF16, F16])
def test_shape_refusals_are_those_of_the_f32_calls(lib, io):
    for src in (False, True):
        assert _block(lib, src, d=20, io=io) == ERR_SHAPE            # the fused block exists for D = 24
        assert _block(lib, src, n=N + 1, io=io) == ERR_SHAPE         # hept_check_shape: N % B
        assert _block(lib, src, ws_bytes=16, io=io) == ERR_ARG       # a short workspace
    assert _prep(lib, d=16, io=io) == ERR_SHAPE and _ffn(lib, d=16, io=io) == ERR_SHAPE


def test_ops_names_the_three_types_for_any_other():
    import torch

    with pytest.raises(RuntimeError, match="no CPU path"):
        ops._inc(torch.zeros(4, 24, dtype=torch.bfloat16), "x")
