"""The src variant's Attn block end to end (-m gpu): ``Attn(c, variant="src")`` and ``SrcAttn`` in eval (one C call),
under torch.compile, under torch.utils.checkpoint as the src model runs its blocks
(``src/models/baselines/transformer.py:138-139``), outside the fused shapes, and with one module across clouds of
different ``raw_size``."""
import pytest
import torch

import src_attn_sweep as ssw
from hept_amd import Attn, SrcAttn

pytestmark = pytest.mark.gpu

D, H, K = ssw.D, ssw.H, ssw.K


def _shape(raw, b, t, c, seed, later=False):
    n = raw + (-raw) % b
    return ssw.Shape(f"blk-{raw}-{b}-{t}-{c}", n, raw, b, t, c, later, seed, False)


def _block(cls_src, s, inp, dev, precision="fp32"):
    if cls_src:
        blk = SrcAttn("hept", s.C, precision=precision, h_dim=D, num_heads=H, block_size=s.B, n_hashes=s.T,
                      num_w_per_dist=K, pe_type="none", n_layers=4, num_regions=150)
    else:
        blk = Attn(s.C, precision=precision, variant="src", h_dim=D, num_heads=H, block_size=s.B, n_hashes=s.T,
                   num_w_per_dist=K)
    blk.load_state_dict(inp["params"], strict=True)
    return blk.to(dev)


def _vs_float64(s, inp, y, qpos, kpos):
    ref = ssw.oracle64(s, inp, qpos.long().cpu(), kpos.long().cpu(), keep=False)["y"]
    x = float(((y.cpu().double() - ref).abs() / (ssw.ATOL + ssw.RTOL * ref.abs())).max())
    assert x <= 1.0, f"{s.id}: worst element {x:.3f}x the fp32 tolerance"


@pytest.mark.parametrize("c", [6, 2])
def test_attn_variant_src_eval_is_the_one_call_block(c, gpu_device):
    """Attn(c, variant="src") in eval under no_grad takes the fused block (it raised KeyError: 'combined_shifts' before
    the block dispatched on the variant) and equals the staged kernels and float64."""
    s = _shape(901, 100, 3, c, 3100 + c, later=True)
    inp = ssw.inputs(s)
    g = ssw._gpu(inp, gpu_device)
    blk = _block(False, s, inp, gpu_device).eval()
    with torch.no_grad():
        assert blk._fused_ok(g["x"])
        y = blk(g["x"], ssw.kwargs_of(g))
        st = ssw.staged(s, g, "fp32")
    assert torch.equal(y, st["y"])
    _vs_float64(s, inp, y, st["qpos"], st["kpos"])


def test_src_attn_strict_loads_a_src_state_dict(gpu_device):
    """SrcAttn loads a src-shaped state dict (attn.e2lsh.beta included) with strict=True and its eval block is the
    one-call block on those weights."""
    s = _shape(1023, 128, 3, 4, 3200)
    inp = ssw.inputs(s)
    sd = {k: v.clone() for k, v in inp["params"].items()}
    assert "attn.e2lsh.beta" in sd
    blk = _block(True, s, dict(inp, params=sd), gpu_device).eval()
    g = ssw._gpu(inp, gpu_device)
    with torch.no_grad():
        y = blk(g["x"], ssw.kwargs_of(g))
        one = ssw.one_call(s, g, "fp32")
    assert torch.equal(y, one)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_src_block_under_torch_compile_is_one_graph(precision, gpu_device):
    """torch.compile(fullgraph=True) of the src block (the registered attn_block_src op) is one graph and equals eager."""
    import torch._dynamo

    s = _shape(1250, 100, 3, 6, 3300)
    inp = ssw.inputs(s)
    blk = _block(True, s, inp, gpu_device, precision).eval()
    g = ssw._gpu(inp, gpu_device)
    kw = ssw.kwargs_of(g)
    with torch.no_grad():
        eager = blk(g["x"], kw)
        torch._dynamo.reset()
        explained = torch._dynamo.explain(blk)(g["x"], kw)
        assert explained.graph_count == 1 and explained.graph_break_count == 0, explained
        torch._dynamo.reset()
        out = torch.compile(blk, backend="aot_eager", fullgraph=True)(g["x"], kw)
    assert torch.equal(out, eager)


def _grads(blk, x, kw, ckpt):
    from torch.utils.checkpoint import checkpoint

    blk.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    torch.manual_seed(11)           # the same dropout masks in every run (checkpoint replays the RNG state)
    y = blk(x, kw) if ckpt is None else checkpoint(blk, x, kw, use_reentrant=ckpt)
    if ckpt is None:
        assert ssw._fused_node_ran(y)
    y.backward(ssw.asw._g_out(y.shape).to(x.device))
    out = {nm: p.grad.detach().clone() for nm, p in blk.named_parameters() if p.grad is not None}
    out.update(x=x.grad.detach().clone(), y=y.detach().clone())
    return out


@pytest.mark.parametrize("use_reentrant", [True, False])
def test_src_block_under_activation_checkpointing(use_reentrant, gpu_device):
    """torch.utils.checkpoint around the training block (dropout on) gives the gradients of the plain call."""
    s = _shape(1100, 100, 3, 6, 3400, later=True)
    inp = ssw.inputs(s)
    blk = _block(True, s, inp, gpu_device).train()
    g = ssw._gpu(inp, gpu_device)
    kw = ssw.kwargs_of(g)
    plain = _grads(blk, g["x"], kw, None)
    ck = _grads(blk, g["x"], kw, use_reentrant)
    assert set(ck) == set(plain) and set(plain) >= set(ssw.GRAD_PARAMS)
    for nm, r in plain.items():
        err = float((ck[nm] - r).abs().max()) / (float(r.abs().max()) + 1e-30)
        assert err <= ssw.TRAIN_TENSOR["fp32"], (nm, err)


def test_src_block_outside_the_fused_shapes_composes(gpu_device):
    """C = 3 has no fused row builder: eval and training take the composed block around the src operator and equal
    that composition written out."""
    from hept_amd import ops

    s = _shape(901, 100, 3, 3, 3500, later=True)
    inp = ssw.inputs(s)
    blk = _block(True, s, inp, gpu_device).eval()
    g = ssw._gpu(inp, gpu_device)
    kw = ssw.kwargs_of(g)
    with torch.no_grad():
        assert not blk._fused_ok(g["x"])
        y = blk(g["x"], kw)
        xn = blk.norm1(g["x"])
        q, k, v = blk.w_q(xn), blk.w_k(xn), blk.w_v(xn)
        aggr = ops.forward_src(q, k, v, g["coords"], (g["eta"], g["phi"]), g["regions_h"], s.raw, blk.w_rpe.weight,
                               blk.attn.e2lsh.alpha, blk.attn.out_linear.weight, blk.attn.out_linear.bias,
                               block_size=s.B, w_per_dist=K)
        x1 = g["x"] + aggr
        want = x1 + blk.ff(blk.norm2(x1))
    assert torch.equal(y, want)
    blk.train()
    x = g["x"].clone().requires_grad_(True)
    assert not blk.attn._train_fused_ok(x, kw)
    yt = blk(x, kw)
    assert not ssw._fused_node_ran(yt)
    yt.sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_one_module_across_raw_sizes(precision, gpu_device):
    """One SrcAttn (its workspace cached on the module) on clouds of the same padded size with different raw_size, and
    a larger and a smaller one: every call equals the one-call block on a fresh workspace, and (fp32) float64."""
    shapes = [_shape(raw, 100, 3, 4, 3600 + i) for i, raw in enumerate([901, 1000, 950, 3000, 150, 901])]
    first = ssw.inputs(shapes[0])
    blk = _block(True, shapes[0], first, gpu_device, precision).eval()
    for s in shapes:
        inp = ssw.inputs(s)
        inp["params"] = first["params"]
        g = ssw._gpu(inp, gpu_device)
        with torch.no_grad():
            y = blk(g["x"], ssw.kwargs_of(g))
            one = ssw.one_call(s, g, precision)
            st = ssw.staged(s, g, precision)
        assert torch.equal(y, one) and torch.equal(y, st["y"]), s.id
        if precision == "fp32":
            _vs_float64(s, inp, y, st["qpos"], st["kpos"])
