"""AttnStack without a GPU: state-dict layout, the refusals of the two C entry points (made before any HIP call, on
dummy host addresses) and the Python-side refusals."""
import ctypes

import pytest
import torch

from hept_amd import Attn, AttnStack, _lib, ops
from hept_amd.build import build

CFG = dict(h_dim=24, num_heads=8, block_size=128, n_hashes=3, num_w_per_dist=10, pe_type="none")
OK, ERR_SHAPE, ERR_ARG = 0, 1, 3
N, H, D, C, K, T, B = 256, 8, 24, 6, 10, 3, 128


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.load()


@pytest.mark.parametrize("variant", ["example", "src"])
@pytest.mark.parametrize("n_layers", [1, 4])
def test_state_dict_is_the_reference_models_attns_slice(variant, n_layers):
    stack = AttnStack(C, variant=variant, n_layers=n_layers, **CFG)
    layers = [Attn(C, variant=variant, n_layers=n_layers, **CFG) for _ in range(n_layers)]
    layer_keys = list(layers[0].state_dict())
    assert ("attn.e2lsh.beta" in layer_keys) == (variant == "src")
    assert list(stack.state_dict()) == [f"attns.{i}.{k}" for i in range(n_layers) for k in layer_keys]
    sd = {f"attns.{i}.{k}": v for i, layer in enumerate(layers) for k, v in layer.state_dict().items()}
    stack.load_state_dict(sd, strict=True)
    for i, layer in enumerate(layers):
        for k, v in layer.state_dict().items():
            assert torch.equal(stack.state_dict()[f"attns.{i}.{k}"], v)
    assert len(stack.attns) == n_layers and all(isinstance(m, Attn) for m in stack.attns)


def test_missing_n_layers_raises():
    with pytest.raises(ValueError, match="n_layers"):
        AttnStack(C, **CFG)
    with pytest.raises(ValueError, match="n_layers"):
        AttnStack(C, n_layers=0, **CFG)


# ---- C entry points: every pointer is a dummy (never dereferenced: the call is refused first), except `layers` -----
PTR = 0x10000   # 16-byte aligned


def _layers(n_layers, null_field=None):
    fields = [f for f, _ in _lib.AttnParams._fields_ if f not in ("eps1", "eps2")]
    arr = (_lib.AttnParams * max(n_layers, 1))()
    for i in range(max(n_layers, 1)):
        for f in fields:
            setattr(arr[i], f, PTR)
        arr[i].eps1 = arr[i].eps2 = 1e-5
    if null_field is not None:
        setattr(arr[null_field[0]], null_field[1], None)
    return arr


def _call(lib, src=False, xcat=PTR, ld=None, layers="default", n_layers=2, n=N, d=D, raw_size=N - 3, ws_bytes=1 << 40,
          null_field=None, geo=PTR):
    ld = (n_layers + 1) * d if ld is None else ld
    arr = _layers(n_layers, null_field) if layers == "default" else layers
    tail = (arr, n_layers, n, H, d, C, K, T, B, _lib.PREC_F32, PTR, ws_bytes, None)
    if src:
        return lib.hept_attn_stack_forward_src(xcat, ld, PTR, geo, PTR, PTR, raw_size, *tail)
    return lib.hept_attn_stack_forward(xcat, ld, PTR, PTR, *tail)


@pytest.mark.parametrize("src", [False, True], ids=["example", "src"])
def test_c_entry_refuses_null_pointers(lib, src):
    assert _call(lib, src, xcat=None) == ERR_ARG
    assert _call(lib, src, layers=None) == ERR_ARG
    assert _call(lib, src, null_field=(1, "ff2_w")) == ERR_ARG
    assert _call(lib, src, null_field=(1, "norm1_w")) == ERR_ARG
    # out_linear.bias is the one optional tensor of a block (include/hept_hip.h: out_b may be NULL): a null bias passes
    # the pointer check and the call is refused for the next reason (a short workspace) instead of running
    assert _call(lib, src, null_field=(0, "out_b"), ws_bytes=16) == ERR_ARG
    # nulls come first: a null buffer beside a bad size is still an argument error
    assert _call(lib, src, xcat=None, n_layers=0) == ERR_ARG
    if src:
        assert _call(lib, src, geo=None) == ERR_ARG


@pytest.mark.parametrize("src", [False, True], ids=["example", "src"])
def test_c_entry_refuses_bad_sizes(lib, src):
    assert _call(lib, src, n_layers=0, ld=48) == ERR_SHAPE
    assert _call(lib, src, n_layers=-1, ld=48) == ERR_SHAPE
    assert _call(lib, src, ld=3 * D - 4) == ERR_SHAPE       # the last layer's columns would not fit
    assert _call(lib, src, ld=3 * D + 2) == ERR_SHAPE       # rows of the second point on would start off 16 bytes
    assert _call(lib, src, d=20) == ERR_SHAPE               # the fused block exists for D = 24
    assert _call(lib, src, n=N + 1) == ERR_SHAPE            # hept_check_shape: N % B
    if src:
        assert _call(lib, src, raw_size=N + 1) == ERR_SHAPE
        assert _call(lib, src, raw_size=-1) == ERR_SHAPE


@pytest.mark.parametrize("src", [False, True], ids=["example", "src"])
def test_c_entry_refuses_misaligned_buffer_and_short_workspace(lib, src):
    assert _call(lib, src, xcat=PTR + 4) == ERR_ARG
    need = lib.hept_workspace_bytes(N, H, D, C, T, B, _lib.PREC_F32)
    assert _call(lib, src, ws_bytes=need - 1) == ERR_ARG
    # sizes come before these: a misaligned buffer with a bad pitch is a shape error
    assert _call(lib, src, xcat=PTR + 4, ld=3 * D + 2) == ERR_SHAPE


def test_single_block_entries_keep_their_refusals(lib):
    """The refactored block (strides inside) refuses what it refused before, still without a HIP call."""
    st = _layers(1)
    blk = lib.hept_attn_block_forward
    assert blk(None, PTR, PTR, st, N, H, D, C, K, T, B, 0, PTR, 1 << 40, PTR, None) == ERR_ARG
    assert blk(PTR, PTR, PTR, st, N, H, 20, C, K, T, B, 0, PTR, 1 << 40, PTR, None) == ERR_SHAPE
    assert blk(PTR, PTR, PTR, st, N, H, D, C, K, T, B, 0, PTR, 16, PTR, None) == ERR_ARG
    assert blk(PTR, PTR, PTR, _layers(1, (0, "w_q")), N, H, D, C, K, T, B, 0, PTR, 1 << 40, PTR, None) == ERR_ARG


# ---- Python side ---------------------------------------------------------------------------------------------------
def _params(n_layers):
    return [Attn(C, **CFG)._block_params() for _ in range(n_layers)]


def test_ops_refuses_a_view_without_unit_column_stride(lib):
    xcat = torch.zeros(3 * D, N).t()
    assert xcat.shape == (N, 3 * D) and xcat.stride(1) != 1
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        ops.attn_stack_forward(xcat, torch.zeros(N, C), torch.zeros(T, H, N, dtype=torch.int64), _params(2),
                               num_heads=H, block_size=B, w_per_dist=K)
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        ops.attn_stack_forward_src(xcat, torch.zeros(N, C), (torch.zeros(T * H, N), torch.zeros(T * H, N)),
                                   torch.ones(2, T * H), N, _params(2), num_heads=H, block_size=B, w_per_dist=K)


def test_ops_refuses_wrong_dtype_and_no_layers(lib):
    with pytest.raises(TypeError, match="float32"):
        ops.attn_stack_forward(torch.zeros(N, 3 * D, dtype=torch.bfloat16), torch.zeros(N, C),
                               torch.zeros(T, H, N, dtype=torch.int64), _params(2), num_heads=H, block_size=B,
                               w_per_dist=K)
    with pytest.raises(ValueError, match="at least one layer"):
        ops.attn_stack_forward(torch.zeros(N, 3 * D), torch.zeros(N, C), torch.zeros(T, H, N, dtype=torch.int64), [],
                               num_heads=H, block_size=B, w_per_dist=K)


def test_cpu_tensors_are_refused(lib):
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attn_stack_forward(torch.zeros(N, 3 * D), torch.zeros(N, C), torch.zeros(T, H, N, dtype=torch.int64),
                               _params(2), num_heads=H, block_size=B, w_per_dist=K)
    stack = AttnStack(C, n_layers=2, **CFG).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        stack(torch.zeros(N, D), {"coords": torch.zeros(N, C),
                                  "combined_shifts": torch.zeros(T, H, N, dtype=torch.int64)})
    assert stack._workspace is None and all(m._workspace is None and m.attn._workspace is None for m in stack.attns)


def test_bindings_declare_the_stack_entries():
    for name in ("hept_attn_stack_forward", "hept_attn_stack_forward_src"):
        assert name in _lib.SIGNATURES
    assert "attn_stack_forward" in ops.__all__ and "attn_stack_forward_src" in ops.__all__
    assert ctypes.sizeof(_lib.AttnParams) == 15 * ctypes.sizeof(ctypes.c_void_p) + 8
