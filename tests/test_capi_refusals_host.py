"""What the whole-operator entry points of the C ABI refuse, and with which code, without a GPU.

Every pointer is a dummy 16-byte aligned host address (never dereferenced: the call is refused before any HIP call),
except the ``hept_attn_params`` record, which the block entries read.  The ORDER of the refusals is part of the ABI --
a call with two faults answers with the code of the one that is checked first -- so the expected codes below are
literals, recorded from the library before its entry checks were gathered into shared helpers.
"""
import ctypes

import pytest

from hept_amd import _lib
from hept_amd.build import build

SHAPE, ARG = 1, 3
PTR = 0x10000   # 16-byte aligned
N, H, D, C, K, T, B = 256, 8, 24, 6, 10, 3, 128
F32, BF16 = _lib.PREC_F32, _lib.PREC_BF16

_OP = "N H D C K T B precision workspace workspace_bytes"
_PART = "N H D C K T t0 Tl B precision"
_SRC = "eta_idx phi_idx cfac raw_size"
# argument names of every covered entry point, in the order of include/hept_hip.h
SIG = {
    "hept_forward": f"q k v coords codes w_rpe alpha out_weight out_bias {_OP} out stream",
    "hept_forward_in": f"q k v in_dtype coords codes w_rpe alpha out_weight out_bias {_OP} out stream",
    "hept_forward_src": f"q k v coords {_SRC} w_rpe alpha out_weight out_bias {_OP} out stream",
    "hept_forward_src_in": f"q k v in_dtype coords {_SRC} w_rpe alpha out_weight out_bias {_OP} out stream",
    "hept_forward_partial": f"q k v coords codes w_rpe alpha {_PART} acc_precision workspace workspace_bytes acc stream",
    "hept_forward_partial_in":
        f"q k v in_dtype coords codes w_rpe alpha {_PART} acc_precision workspace workspace_bytes acc stream",
    "hept_forward_partial_src":
        f"q k v coords {_SRC} w_rpe alpha {_PART} acc_precision workspace workspace_bytes acc stream",
    "hept_forward_partial_src_in":
        f"q k v in_dtype coords {_SRC} w_rpe alpha {_PART} acc_precision workspace workspace_bytes acc stream",
    "hept_partial_begin": f"q k v coords codes w_rpe alpha {_PART} workspace workspace_bytes stream",
    "hept_partial_begin_src": f"q k v coords {_SRC} w_rpe alpha {_PART} workspace workspace_bytes stream",
    "hept_partial_heads":
        "workspace workspace_bytes N H D C Tl B precision h0 hg n_pad acc_precision dst stream",
    "hept_attn_block_forward": f"x coords codes p {_OP} y stream",
    "hept_attn_block_forward_io": f"x io_dtype coords codes p {_OP} y stream",
    "hept_attn_block_forward_src": f"x coords {_SRC} p {_OP} y stream",
    "hept_attn_block_forward_src_io": f"x io_dtype coords {_SRC} p {_OP} y stream",
    "hept_forward_sharded": f"comm q k v coords codes w_rpe alpha out_weight out_bias {_PART} head_groups transport "
                            "workspace workspace_bytes xbuf xbuf_bytes out_full stream",
    "hept_forward_sharded_src": f"comm q k v coords {_SRC} w_rpe alpha out_weight out_bias {_PART} head_groups "
                                "transport workspace workspace_bytes xbuf xbuf_bytes out_full stream",
}
SIG = {name: names.split() for name, names in SIG.items()}

# the base call: valid in every argument (the sharded entries have no communicator without a device: `comm` stays null)
_POINTERS = ("q k v coords codes eta_idx phi_idx cfac w_rpe alpha out_weight out_bias workspace out acc dst x y xbuf "
             "out_full").split()
BASE = dict({name: PTR for name in _POINTERS}, N=N, H=H, D=D, C=C, K=K, T=T, t0=0, Tl=T, B=B, precision=F32,
            acc_precision=F32, in_dtype=_lib.IN_F32, io_dtype=_lib.IN_F32, raw_size=200, workspace_bytes=1 << 40,
            h0=0, hg=H, n_pad=N, head_groups=1, transport=_lib.TRANSPORT_RCCL, xbuf_bytes=1 << 40, comm=None,
            stream=None)
PARAM_FIELDS = [f for f, _ in _lib.AttnParams._fields_ if f not in ("eps1", "eps2")]

FWD = ["hept_forward", "hept_forward_in", "hept_forward_src", "hept_forward_src_in"]
PART = ["hept_forward_partial", "hept_forward_partial_in", "hept_forward_partial_src", "hept_forward_partial_src_in"]
BEGIN = ["hept_partial_begin", "hept_partial_begin_src"]
HEADS = ["hept_partial_heads"]
BLOCK = ["hept_attn_block_forward", "hept_attn_block_forward_io", "hept_attn_block_forward_src",
         "hept_attn_block_forward_src_io"]
SHARDED = ["hept_forward_sharded", "hept_forward_sharded_src"]
IN = [e for e in FWD + PART if e.endswith("_in")]
IO = [e for e in BLOCK if e.endswith("_io")]
SRC = [e for e in FWD + PART + BEGIN + BLOCK if "_src" in e]
EXAMPLE = [e for e in FWD + PART + BEGIN + BLOCK if "_src" not in e]
OPS = FWD + PART + BEGIN   # the entries that take q, k, v


def _nulls(names, code, entries):
    return [(f"null {n}", {n: None}, code, [e for e in entries if n.split(".")[0] in SIG[e]]) for n in names]


# (fault, overrides of the base call, expected code, entry points it is made at)
CASES = [
    # ---- single faults: every required pointer in turn ...
    *_nulls("q k v coords w_rpe alpha workspace".split(), ARG, OPS),
    *_nulls(["codes"], ARG, EXAMPLE),
    *_nulls(["eta_idx", "phi_idx", "cfac"], ARG, SRC),
    *_nulls(["out_weight", "out"], ARG, FWD),
    *_nulls(["acc"], ARG, PART),
    *_nulls(["workspace", "dst"], ARG, HEADS),
    *_nulls(["x", "coords", "p", "workspace", "y"], ARG, BLOCK),
    *_nulls([f"p.{f}" for f in PARAM_FIELDS if f != "out_b"], ARG, BLOCK),
    # ... but not the optional bias: a call without one gets past the pointer checks and is refused for its bad N
    ("null out_bias, N=250", dict(out_bias=None, N=250), SHAPE, FWD),
    ("null p.out_b, N=250", {"p.out_b": None, "N": 250}, SHAPE, BLOCK),
    # ---- ... the element type, the sizes, the table range, the key arguments, the workspace
    ("in_dtype=3", dict(in_dtype=3), ARG, IN),
    ("io_dtype=3", dict(io_dtype=3), ARG, IO),
    ("N=250", dict(N=250), SHAPE, OPS + HEADS + BLOCK),
    ("H=17", dict(H=17), SHAPE, OPS + HEADS + BLOCK),
    ("D=28", dict(D=28), SHAPE, OPS + HEADS + BLOCK),
    ("Tl=0", dict(Tl=0), SHAPE, PART + BEGIN + HEADS),
    ("t0=-1", dict(t0=-1), SHAPE, PART + BEGIN),
    ("t0+Tl=T+1", dict(t0=1), SHAPE, PART + BEGIN),
    ("raw_size=-1", dict(raw_size=-1), SHAPE, SRC),
    ("raw_size=N+1", dict(raw_size=N + 1), SHAPE, SRC),
    ("acc_precision=BF16 under F32", dict(acc_precision=BF16), SHAPE, PART + HEADS),
    ("workspace_bytes=16", dict(workspace_bytes=16), ARG, OPS + HEADS + BLOCK),
    # (K and the precision code are refused by the row builder's host side, before it launches anything)
    ("K=-1", dict(K=-1), SHAPE, OPS + BLOCK),
    ("K=200", dict(K=200), SHAPE, OPS + BLOCK),
    ("precision=9", dict(precision=9), SHAPE, OPS + HEADS + BLOCK),
    # ---- the fused block: D = 24 and H = 8 only, 16-bit rows 16-byte aligned
    ("D=20", dict(D=20), SHAPE, BLOCK),
    ("H=4", dict(H=4), SHAPE, BLOCK),
    ("x at +2, bf16 rows", dict(x=PTR + 2, io_dtype=_lib.IN_BF16), ARG, IO),
    # ---- the head range of hept_partial_heads
    ("h0=-1", dict(h0=-1), SHAPE, HEADS),
    ("hg=0", dict(hg=0), SHAPE, HEADS),
    ("h0+hg=H+1", dict(h0=1), SHAPE, HEADS),
    ("n_pad=N-1", dict(n_pad=N - 1), SHAPE, HEADS),
    # ---- two faults: the one that is checked first answers
    ("null q, N=250", dict(q=None, N=250), ARG, OPS),
    ("null x, N=250", dict(x=None, N=250), ARG, BLOCK),
    ("null dst, N=250", dict(dst=None, N=250), ARG, HEADS),
    ("acc_precision=BF16, workspace_bytes=16", dict(acc_precision=BF16, workspace_bytes=16), SHAPE, PART + HEADS),
    ("t0=-1, workspace_bytes=16", dict(t0=-1, workspace_bytes=16), SHAPE, PART + BEGIN),
    ("null eta_idx, raw_size=-1", dict(eta_idx=None, raw_size=-1), ARG, SRC),
    # ---- the sharded entries, as far as they go without a communicator: the key arguments come before it
    ("null comm", dict(), ARG, SHARDED),
    ("null comm, null codes", dict(codes=None), ARG, ["hept_forward_sharded"]),
    ("null comm, null eta_idx", dict(eta_idx=None), ARG, ["hept_forward_sharded_src"]),
    ("null comm, raw_size=-1", dict(raw_size=-1), SHAPE, ["hept_forward_sharded_src"]),
    ("null comm, raw_size=N+1", dict(raw_size=N + 1), SHAPE, ["hept_forward_sharded_src"]),
    ("null comm, null eta_idx, raw_size=-1", dict(eta_idx=None, raw_size=-1), ARG, ["hept_forward_sharded_src"]),
]


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


def call(lib, entry, overrides):
    vals = dict(BASE)
    params = _lib.AttnParams(**{f: PTR for f in PARAM_FIELDS}, eps1=1e-5, eps2=1e-5)
    vals["p"] = ctypes.byref(params)
    for name, value in overrides.items():
        if name.startswith("p."):
            setattr(params, name[2:], value)
        else:
            assert name in SIG[entry], f"{entry} has no argument {name}"
            vals[name] = value
    return getattr(lib, entry)(*[vals[name] for name in SIG[entry]])


def test_signatures_cover_every_argument():
    for entry, names in SIG.items():
        assert len(names) == len(_lib.SIGNATURES[entry][1]), entry
    assert all(entries for _, _, _, entries in CASES)


def test_base_call_has_valid_sizes(lib):
    """The size and workspace queries of the ABI accept the base call that every case above varies."""
    assert lib.hept_check_shape(N, H, D, C, T, B) == 0
    assert lib.hept_workspace_bytes(N, H, D, C, T, B, F32) <= BASE["workspace_bytes"]


@pytest.mark.parametrize("fault,entry", [(i, e) for i, (_, _, _, entries) in enumerate(CASES) for e in entries],
                         ids=lambda v: CASES[v][0] if isinstance(v, int) else v[5:])
def test_refused_with_the_recorded_code(lib, fault, entry):
    _, overrides, code, _ = CASES[fault]
    assert call(lib, entry, overrides) == code


def test_prepare_input_refuses_a_pad_window_before_the_batch(lib):
    """hept_prepare_input: pad positions wrap once, and the first cloud's may not start more than n_raw in front of the
    batch (cloud 0 + n_raw >= B, include/hept_hip.h).  The cloud sizes are device data; what the host arguments decide,
    2 * n_raw - (n_clouds - 1) < B, is refused with HEPT_ERR_SHAPE before any HIP call.  EVERY call carries a 16-byte
    workspace: the size checks come first, and a call that passes them is refused for its workspace (HEPT_ERR_ARG), so
    nothing is ever launched on the dummy pointers, whatever the rule decides."""
    def call_prepare(n_clouds, n_raw, max_cloud, n_pad, b):
        return lib.hept_prepare_input(PTR, 3, PTR, PTR, n_clouds, n_raw, max_cloud, n_pad, PTR, 2, 3, b, PTR, 16, PTR,
                                      PTR, PTR, PTR, None)

    assert call_prepare(1, 10, 10, 64, 64) == SHAPE            # one cloud of 10, B = 64: 10 + 10 < 64
    assert call_prepare(1, 31, 31, 64, 64) == SHAPE            # 31 + 31 < 64
    assert call_prepare(1, 32, 32, 64, 64) == ARG              # 32 + 32 == 64: legal
    assert call_prepare(2, 8, 4, 32, 16) == SHAPE              # two clouds, 8 points: at most 7 + 8 < 16
    assert call_prepare(300, 300, 1, 300000, 1000) == SHAPE    # 300 clouds of 1, B = 1000
    # clouds (5, 5) or (1, 12) with B = 16 break the rule (5 + 10, 1 + 13 < 16), but (9, 1) and (12, 1) would not: the
    # host arguments cannot tell, the caller must (hept_prepare_probe's flag; hept_amd.prep raises IndexError), and the
    # kernel clamps
    assert call_prepare(2, 10, 5, 32, 16) == ARG
    assert call_prepare(2, 13, 12, 32, 16) == ARG
