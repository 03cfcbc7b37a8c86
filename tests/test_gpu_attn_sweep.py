"""The fused Attn block's shape sweep (tests/attn_sweep.py, -m gpu): every element of the eval block in every precision
and every gradient of the training block against the reference block evaluated in float64 on the GPU's own
permutations; the gates between the fused and the composed block; one module across shapes; torch.compile.  The worst
error of every precision and gradient is printed at the end of the module (pytest -s)."""
import pytest
import torch

import attn_sweep as asw
import hept_oracle as ho
import shape_sweep as sw
from hept_amd import Attn

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_worst):
        val, sid = _worst[key]
        print(f"attn sweep worst {key}: {val:.3e} ({sid})")


def _noter(prefix, sid):
    def note(key, val):
        k = f"{prefix} {key}"
        if val > _worst.get(k, (-1.0, ""))[0]:
            _worst[k] = (val, sid)
    return note


FWD = [pytest.param(s.id, p, id=f"{s.id}-{p}") for s in asw.SHAPES for p in asw.PRECISIONS]
BWD = [pytest.param(s.id, m, id=f"{s.id}-{m}") for s in asw.BWD_SHAPES for m in asw.train_modes(s)]


@pytest.mark.parametrize("sid,precision", FWD)
def test_block_forward_every_element_vs_float64(sid, precision, gpu_device):
    asw.check_forward(asw.BY_ID[sid], precision, gpu_device, _noter(f"forward {precision}", sid))


@pytest.mark.parametrize("sid,mode", BWD)
def test_block_training_every_gradient_vs_float64(sid, mode, gpu_device):
    asw.check_backward(asw.BY_ID[sid], mode, gpu_device, _noter(f"backward {mode}", sid))


# ---------------------------------------------------------------------------------------------------------------------
# gates and reuse: blocks outside the fused shapes, one module across shapes, torch.compile
# ---------------------------------------------------------------------------------------------------------------------
def _composed_inputs(sizes, b, t, h, d, c, seed):
    """Inputs and a default-initialised block (CPU state dict) of any head shape, scaled as attn_sweep.inputs."""
    from hept_amd.synthetic import make_inputs

    inp = make_inputs(list(sizes), block_size=b, n_hashes=t, coords_dim=c, h_dim=d, num_heads=h, seed=seed)
    x = torch.randn(sum(sizes), d, generator=torch.Generator().manual_seed(seed + 1))[inp["pad_seq"]].contiguous()
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        blk = Attn(c, h_dim=d, num_heads=h, block_size=b, n_hashes=t, num_w_per_dist=10)
        p = {k: v.detach().clone() for k, v in blk.state_dict().items()}
        p["norm1.weight"], p["norm1.bias"] = 1.0 + 0.2 * torch.randn(d), 0.1 * torch.randn(d)
    p["w_q.weight"], p["w_k.weight"] = p["w_q.weight"] * asw.QK_SCALE, p["w_k.weight"] * asw.QK_SCALE
    p["attn.e2lsh.alpha"] = inp["alpha"]
    return dict(x=x, coords=inp["coords"] * asw.COORD_SCALE, combined_shifts=inp["combined_shifts"], params=p)


def _composed_perms(blk, g, b, t, h, d):
    """The permutations of the composed block's operator: prep_hash + sort_tables on torch's own q, k, v (the same
    torch ops on the same device as Attn's composition) -- checked against a stable sort of the GPU keys."""
    with torch.no_grad():
        xn = blk.norm1(g["x"])
        q, k, v = blk.w_q(xn), blk.w_k(xn), blk.w_v(xn)
    s = sw.Shape("composed", (g["x"].shape[0],), b, t, h, d, g["coords"].shape[1], 0, False)
    gg = dict(q=q, k=k, v=v, coords=g["coords"], w_rpe_weight=blk.w_rpe.weight.detach(), alpha=blk.attn.e2lsh.alpha,
              combined_shifts=g["combined_shifts"], out_weight=blk.attn.out_linear.weight.detach(),
              out_bias=blk.attn.out_linear.bias.detach())
    st = sw.staged(s, gg, "fp32")
    return st["qpos"].long().cpu(), st["kpos"].long().cpu()


def _vs_float64(y, inp, qp, kp, b, h):
    p64 = {k: v.double() for k, v in inp["params"].items()}
    ref = ho.attn_block(inp["x"].double(), inp["coords"].double(), inp["combined_shifts"], p64, num_heads=h,
                        block_size=b, w_per_dist=10, q_positions=qp, k_positions=kp, keep=False)["y"]
    x = float(((y.cpu().double() - ref).abs() / (asw.ATOL + asw.RTOL * ref.abs())).max())
    assert x <= 1.0, f"worst element {x:.3f}x the fp32 tolerance"
    return x


@pytest.mark.parametrize("h,d,c", [(8, 24, 3), (8, 24, 5), (8, 16, 4), (4, 24, 6), (8, 20, 6)])
def test_block_outside_the_fused_shapes_composes_and_equals_float64(h, d, c, gpu_device):
    """The fused row builder exists for D = 24, H = 8, C in {6, 4, 2}: any other shape must take the composed block in
    eval mode and under torch.compile (C = 3 and C = 5 raised HEPT_ERR_SHAPE from the fused call before the gate
    checked C) and equal float64 on every element."""
    import torch._dynamo

    dev = gpu_device
    b, t = 64, 3
    inp = _composed_inputs([400, 170], b, t, h, d, c, seed=40 + c)
    blk = Attn(c, h_dim=d, num_heads=h, block_size=b, n_hashes=t, num_w_per_dist=10)
    blk.load_state_dict(inp["params"], strict=True)
    blk = blk.to(dev).eval()
    g = asw._gpu(inp, dev)
    kwargs = {"coords": g["coords"], "combined_shifts": g["combined_shifts"]}
    assert not blk._fused_ok(g["x"])
    qp, kp = _composed_perms(blk, g, b, t, h, d)
    with torch.no_grad():
        eager = blk(g["x"], kwargs)
        torch._dynamo.reset()
        compiled = torch.compile(blk, backend="aot_eager", fullgraph=True)(g["x"], kwargs)
    _vs_float64(eager, inp, qp, kp, b, h)
    _vs_float64(compiled, inp, qp, kp, b, h)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_one_module_across_shapes(precision, gpu_device):
    """One Attn instance (its workspace cached on the module) called on a large cloud, then smaller ones, then the large
    one again: every call bit-identical to the staged kernels on fresh buffers, and (fp32) every element within the
    fp32 tolerance of float64."""
    dev = gpu_device
    shapes = [asw.Shape(f"reuse-{i}", sz, 64, 3, 4, 900 + i, False, False)
              for i, sz in enumerate([(7000,), (3000, 200), (64,), (130, 65), (7000,)])]
    first = asw.inputs(shapes[0])
    blk = Attn(4, precision=precision, h_dim=24, num_heads=8, block_size=64, n_hashes=3, num_w_per_dist=10)
    blk.load_state_dict(first["params"], strict=True)
    blk = blk.to(dev).eval()
    for s in shapes:
        inp = asw.inputs(s)
        inp["params"] = first["params"]
        g = asw._gpu(inp, dev)
        with torch.no_grad():
            y = blk(g["x"], {"coords": g["coords"], "combined_shifts": g["combined_shifts"]})
            st = asw.staged(s, g, precision)
        assert torch.equal(y, st["y"]), s.id
        if precision == "fp32":
            qp, kp = st["qpos"].long().cpu(), st["kpos"].long().cpu()
            _vs_float64(y, inp, qp, kp, 64, 8)


@pytest.mark.parametrize("c", [4, 2])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fused_block_under_torch_compile_equals_eager(c, precision, gpu_device):
    """torch.compile(fullgraph=True) of the fused block at C = 4 and C = 2 (the registered attn_block op) equals eager."""
    import torch._dynamo

    dev = gpu_device
    s = asw.Shape(f"compile-c{c}", (700, 300), 100, 3, c, 950 + c, False, False)
    inp = asw.inputs(s)
    blk = asw.module(s, inp, precision, dev).eval()
    g = asw._gpu(inp, dev)
    kwargs = {"coords": g["coords"], "combined_shifts": g["combined_shifts"]}
    with torch.no_grad():
        assert blk._fused_ok(g["x"])
        eager = blk(g["x"], kwargs)
        torch._dynamo.reset()
        out = torch.compile(blk, backend="aot_eager", fullgraph=True)(g["x"], kwargs)
    assert torch.equal(out, eager)
