"""AttnStack on the GPU (-m gpu): the model's layer loop in one C call on one workspace.

Reference of every comparison: the single-block call (``ops.attn_block_forward`` / ``ops.attn_block_forward_src``, pinned
by tests/test_gpu_attn_block.py and the float64 sweeps) run layer by layer with a workspace of its own, layer i fed layer
i - 1's output as a contiguous tensor, results joined by ``torch.cat``.  The stack runs the same kernels on the same
values -- only the row pitch of the block's input and output differs -- so every column block must be ``torch.equal``;
there is no tolerance.  Shapes are the smallest that reach each branch the pitches touch (the ragged and the full tile of
the row builder and of the combine, the split and the flat combine grid, the two-launch sort, the table-slot
instantiations and the chunked tables, the coordinate counts, every precision id)."""
import gc

import pytest
import torch

import attn_sweep as asw
import cases
import src_attn_sweep as ssw
from attn_sweep import D, EPS, H, K, PRECISIONS
from hept_amd import Attn, AttnStack, ops
from test_gpu_attn_block import ATOL as A1_ATOL   # the bound of the existing golden test of case A1

pytestmark = pytest.mark.gpu

_cache = {}


def _example(n, b, t, c, n_layers, dev):
    """Inputs of an example-variant stack (attn_sweep's generator) and one parameter set per layer, on the GPU."""
    key = ("ex", n, b, t, c, n_layers)
    if key not in _cache:
        s = asw.Shape(f"stack-n{n}-b{b}-t{t}-c{c}", (n,), b, t, c, 9100 + t + c, False, False)
        inp = asw.inputs(s)
        g = asw._gpu(inp, dev)
        layers = [g["params"]] + [{k: v.to(dev) for k, v in asw.default_params(c, t, s.seed + 10 * i).items()}
                                  for i in range(1, n_layers)]
        _cache.clear()   # one shape at a time
        _cache[key] = (g, layers)
    return _cache[key]


def _kw(b, precision, **extra):
    return dict(num_heads=H, block_size=b, w_per_dist=K, eps1=EPS, eps2=EPS, precision=PRECISIONS[precision][0], **extra)


def _ref_example(g, layers, b, precision):
    outs = [g["x"]]
    for p in layers:
        outs.append(ops.attn_block_forward(outs[-1].contiguous(), g["coords"], g["combined_shifts"], p, **_kw(b, precision)))
    return torch.cat(outs, dim=-1)


def _stack_example(g, layers, b, precision, extra_cols=0, sentinel=-7.25):
    n, n_layers = g["x"].shape[0], len(layers)
    cols = (n_layers + 1) * D
    buf = torch.full((n, cols + extra_cols), sentinel, device=g["x"].device)
    view = buf[:, :cols]
    view[:, :D].copy_(g["x"])
    out = ops.attn_stack_forward(view, g["coords"], g["combined_shifts"], layers, **_kw(b, precision))
    assert out.data_ptr() == buf.data_ptr()   # written in place
    return buf


def _assert_blocks_equal(got, ref, n_layers):
    assert got.shape == ref.shape and bool(torch.isfinite(ref).all())
    for i in range(n_layers + 1):
        assert torch.equal(got[:, i * D:(i + 1) * D], ref[:, i * D:(i + 1) * D]), f"column block {i}"


EXAMPLE_CASES = [
    # (id, N, B, T, C, L, precision)
    ("pitch48-ragged", 1300, 100, 3, 6, 1, "fp32"),
    ("pitch72-ragged", 1300, 100, 3, 6, 2, "fp32"),
    ("pitch120-ragged", 1300, 100, 3, 6, 4, "fp32"),
    ("full-tiles", 1024, 128, 3, 6, 2, "fp32"),
    ("two-launch-sort", 6272, 32, 3, 6, 2, "fp32"),
    ("flat-combine", 33024, 32, 2, 4, 2, "fp32"),
    ("flat-combine-packed", 33024, 32, 2, 4, 2, "bf16"),
    ("tables1", 1300, 100, 1, 6, 2, "fp32"),
    ("tables5", 1300, 100, 5, 6, 2, "fp32"),
    ("tables10-chunks", 1300, 100, 10, 6, 2, "fp32"),
    ("coords4", 1300, 100, 3, 4, 2, "fp32"),
    ("coords2", 1300, 100, 3, 2, 2, "fp32"),
] + [(f"precision-{p}", 1300, 100, 3, 6, 2, p) for p in PRECISIONS if p != "fp32"]


@pytest.mark.parametrize("n,b,t,c,n_layers,precision", [pytest.param(*cs[1:], id=cs[0]) for cs in EXAMPLE_CASES])
def test_stack_equals_layer_by_layer_blocks(n, b, t, c, n_layers, precision, gpu_device):
    g, layers = _example(n, b, t, c, n_layers, gpu_device)
    with asw._diff_mfma(precision):
        ref = _ref_example(g, layers, b, precision)
        got = _stack_example(g, layers, b, precision)
    _assert_blocks_equal(got, ref, n_layers)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_wider_buffer_keeps_its_extra_columns(precision, gpu_device):
    """ld = (L + 1) D + 8 through a column-sliced view: the same results, and the 8 trailing columns are never touched."""
    n, b, t, c, n_layers = 1300, 100, 3, 6, 2
    g, layers = _example(n, b, t, c, n_layers, gpu_device)
    ref = _ref_example(g, layers, b, precision)
    buf = _stack_example(g, layers, b, precision, extra_cols=8, sentinel=-7.25)
    assert buf.stride(0) == (n_layers + 1) * D + 8
    _assert_blocks_equal(buf[:, :(n_layers + 1) * D], ref, n_layers)
    assert bool((buf[:, (n_layers + 1) * D:] == -7.25).all())


@pytest.mark.parametrize("raw", [1250, 1300])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_src_stack_equals_layer_by_layer_blocks(raw, precision, gpu_device):
    """raw_size < N: the padding rows are blanked inside the operator of every layer but still get the residual and the
    feed-forward, so they carry values from layer to layer."""
    n, b, t, c, n_layers = 1300, 100, 3, 6, 2
    s = ssw.Shape(f"stack-src-{raw}", n, raw, b, t, c, False, 9300 + raw, False)
    g = ssw._gpu(ssw.inputs(s), gpu_device)
    layers = [g["params"]] + [{k: v.to(gpu_device) for k, v in ssw.params(s._replace(seed=s.seed + 10 * i)).items()}
                              for i in range(1, n_layers)]
    geo = ((g["eta"], g["phi"]), g["regions_h"], g["raw_size"])
    outs = [g["x"]]
    for p in layers:
        outs.append(ops.attn_block_forward_src(outs[-1].contiguous(), g["coords"], *geo, p, **_kw(b, precision)))
    ref = torch.cat(outs, dim=-1)
    buf = torch.empty(n, (n_layers + 1) * D, device=gpu_device)
    buf[:, :D].copy_(g["x"])
    ops.attn_stack_forward_src(buf, g["coords"], *geo, layers, **_kw(b, precision))
    _assert_blocks_equal(buf, ref, n_layers)
    if raw < n:
        assert bool((buf[raw:, D:] != 0).any())   # padding rows are written too


# ---- the module ----------------------------------------------------------------------------------------------------
def _module(n, b, t, c, n_layers, precision, dev, h_dim=D):
    torch.manual_seed(77)
    stack = AttnStack(c, precision=precision, h_dim=h_dim, num_heads=H, block_size=b, n_hashes=t, num_w_per_dist=K,
                      n_layers=n_layers)
    return stack.to(dev).eval()


def _module_inputs(n, b, t, c, dev, h_dim=D):
    from hept_amd.synthetic import make_inputs

    inp = make_inputs([n], block_size=b, n_hashes=t, coords_dim=c, h_dim=h_dim, num_heads=H, seed=31)
    x = torch.randn(n, h_dim, generator=torch.Generator().manual_seed(32))[inp["pad_seq"]].contiguous()
    kwargs = {"coords": (inp["coords"] * asw.COORD_SCALE).to(dev), "combined_shifts": inp["combined_shifts"].to(dev)}
    return x.to(dev), kwargs


def _loop(stack, x, kwargs):
    outs = [x]
    for layer in stack.attns:
        outs.append(layer(outs[-1], kwargs))
    return torch.cat(outs, dim=-1)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_module_equals_its_own_layers_and_repeats(precision, gpu_device):
    """The module's fast path against a loop over its own layers (each a pinned one-call block with its own workspace), twice
    in a row (workspace and sort state reused across layers and calls) and again on a second stream."""
    n, b, t, c, n_layers = 6272, 128, 3, 6, 4
    stack = _module(n, b, t, c, n_layers, precision, gpu_device)
    x, kwargs = _module_inputs(n, b, t, c, gpu_device)
    with torch.no_grad():
        ref = _loop(stack, x, kwargs)
        y1 = stack(x, kwargs)
        y2 = stack(x, kwargs)
        assert y1.shape == (n, (n_layers + 1) * D) and y1.dtype == torch.float32
        assert torch.equal(y1, ref) and torch.equal(y2, y1)
        ws = stack._workspace
        assert ws is not None and ws.numel() == ops.workspace_bytes(n, H, D, c, t, b, precision)
        side = torch.cuda.Stream(gpu_device)
        side.wait_stream(torch.cuda.current_stream(gpu_device))
        with torch.cuda.stream(side):
            y3 = stack(x, kwargs)
        torch.cuda.current_stream(gpu_device).wait_stream(side)
        y4 = stack(x, kwargs)   # and back on the first stream
        torch.cuda.synchronize(gpu_device)
        assert torch.equal(y3, y1) and torch.equal(y4, y1)
        assert stack._workspace is ws


def test_bf16_input_is_widened_and_the_result_rounded(gpu_device):
    n, b, t, c, n_layers = 1300, 100, 3, 6, 2
    stack = _module(n, b, t, c, n_layers, "fp32", gpu_device)
    x, kwargs = _module_inputs(n, b, t, c, gpu_device)
    x16 = x.bfloat16()
    with torch.no_grad():
        y16 = stack(x16, kwargs)
        y32 = stack(x16.float(), kwargs)
    assert y16.dtype == torch.bfloat16 and y32.dtype == torch.float32
    assert torch.equal(y16, y32.bfloat16())
    assert torch.equal(y16[:, :D], x16)


def test_fallback_with_grad_enabled_is_the_plain_loop(gpu_device):
    n, b, t, c, n_layers = 1300, 100, 3, 6, 2
    stack = _module(n, b, t, c, n_layers, "fp32", gpu_device)
    x, kwargs = _module_inputs(n, b, t, c, gpu_device)
    assert torch.is_grad_enabled()
    y = stack(x, kwargs)
    assert y.requires_grad and stack._workspace is None   # not the fast path, nothing lent
    ref = _loop(stack, x, kwargs)
    assert torch.equal(y.detach(), ref.detach())
    stack.train()
    torch.manual_seed(5)
    y = stack(x, kwargs)
    torch.manual_seed(5)
    ref = _loop(stack, x, kwargs)
    assert torch.equal(y.detach(), ref.detach())


def test_fallback_outside_the_fused_shapes_lends_the_workspace(gpu_device):
    """D = 16: every layer composes the block around the operator; in eval under no_grad the operators use the stack's
    workspace for the duration of the call instead of one each, and hold nothing of it afterwards."""
    n, b, t, c, n_layers, d = 1300, 100, 3, 6, 3, 16
    stack = _module(n, b, t, c, n_layers, "fp32", gpu_device, h_dim=d)
    x, kwargs = _module_inputs(n, b, t, c, gpu_device, h_dim=d)
    ws_bytes = ops.workspace_bytes(n, H, d, c, t, b, "fp32")
    used = []
    hooks = [layer.attn.register_forward_hook(lambda m, a, o: used.append(m._workspace)) for layer in stack.attns]
    with torch.no_grad():
        stack.attns[0].w_q(x)   # (the BLAS library allocates its own workspace at the first GEMM of a process)
        torch.cuda.synchronize(gpu_device)
        before = torch.cuda.memory_allocated(gpu_device)
        y = stack(x, kwargs)
        torch.cuda.synchronize(gpu_device)
        grown = torch.cuda.memory_allocated(gpu_device) - before
        for hk in hooks:
            hk.remove()
        ws = stack._workspace
        assert ws is not None and ws.numel() == ws_bytes
        assert len(used) == n_layers and all(w is ws for w in used)       # every operator ran on the stack's buffer ...
        for layer in stack.attns:
            assert layer.attn._workspace is None and layer._workspace is None   # ... and gave it back
        print(f"grown {grown} B, one workspace {ws_bytes} B")
        assert ws_bytes <= grown < 2 * ws_bytes                            # what stays: one workspace + y, not three
        ref = _loop(stack, x, kwargs)
    assert y.shape == (n, (n_layers + 1) * d)
    assert torch.equal(y, ref)


def test_golden_anchor_case_a1(gpu_device):
    """L = 1 with case A1's checkpoint weights: columns [D, 2D) against the golden y of the real reference block.  The
    bound is the existing A1 test's, not a restatement: the stack's output must be the ``Attn`` module's output bit for
    bit (which tests/test_gpu_attn_block.py::test_attn_block_module_vs_reference holds against the golden y), and the two
    golden bounds that test applies to fp32 are applied here as well, with its ATOL imported."""
    name = "a1_attn_ckpt6k"
    inp, fx = cases.load_case_attn(name)
    cfg = dict(precision="fp32", h_dim=24, num_heads=8, block_size=inp["block_size"], n_hashes=3, num_w_per_dist=10,
               n_layers=1)
    stack = AttnStack(inp["coords"].shape[1], **cfg)
    stack.load_state_dict({f"attns.0.{k}": v for k, v in inp["params"].items()}, strict=True)
    stack = stack.to(gpu_device).eval()
    blk = Attn(inp["coords"].shape[1], **cfg)
    blk.load_state_dict(inp["params"], strict=True)
    blk = blk.to(gpu_device).eval()
    kwargs = {"coords": inp["coords"].to(gpu_device), "combined_shifts": inp["combined_shifts"].to(gpu_device)}
    with torch.no_grad():
        out = stack(inp["x"].to(gpu_device), kwargs).cpu()
        y_blk = blk(inp["x"].to(gpu_device), kwargs).cpu()
    assert torch.equal(out[:, :D], inp["x"])
    y, ref = out[:, D:], torch.from_numpy(fx["y"])
    assert torch.equal(y, y_blk)
    assert y.shape == ref.shape and bool(torch.isfinite(y).all())
    err = (y - ref).abs()
    ok = (err <= A1_ATOL[name] + 1e-4 * ref.abs()).all(-1).float().mean()
    gross = (err.amax(-1) <= 5e-2 * (ref.abs().amax(-1) + 1)).float().mean()
    print(f"a1 anchor: rows within the bound {float(ok):.4f}, rows within 5e-2 of their scale {float(gross):.4f}")
    assert float(ok) >= 0.97
    assert float(gross) >= 0.995


def test_one_workspace_for_four_layers(gpu_device):
    """L = 4, tracking-6k, bf16: from before construction to after reserve + one forward the allocation grows by less than
    two workspaces plus the parameters (one workspace and the output -- not four workspaces), and no layer owns scratch."""
    n, b, t, c, n_layers, precision = 6016, 128, 3, 6, 4, "bf16"
    x, kwargs = _module_inputs(n, b, t, c, gpu_device)
    _cache.clear()
    gc.collect()
    torch.cuda.synchronize(gpu_device)
    before = torch.cuda.memory_allocated(gpu_device)
    stack = _module(n, b, t, c, n_layers, precision, gpu_device)
    stack.reserve(n, c, gpu_device)
    with torch.no_grad():
        y = stack(x, kwargs)
    torch.cuda.synchronize(gpu_device)
    grown = torch.cuda.memory_allocated(gpu_device) - before
    ws_bytes = ops.workspace_bytes(n, H, D, c, t, b, precision)
    param_bytes = sum(p.numel() * p.element_size() for p in stack.parameters())
    print(f"grown {grown} B, workspace {ws_bytes} B, parameters {param_bytes} B, output {y.numel() * 4} B")
    assert grown >= ws_bytes                       # the workspace exists ...
    assert grown < 2 * ws_bytes + param_bytes      # ... once
    own = stack._workspace.untyped_storage().data_ptr()
    for layer in stack.attns:
        for w in (layer._workspace, layer.attn._workspace):
            assert w is None or w.untyped_storage().data_ptr() == own
