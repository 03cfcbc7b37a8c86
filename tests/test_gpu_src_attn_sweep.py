"""The src variant's fused Attn block swept over shapes (tests/src_attn_sweep.py, -m gpu): in the six forward
precisions of tests/attn_sweep.py the one-call block and SrcAttn.eval() equal the staged kernels bit for bit, the
permutations are the stable sort of the GPU's own keys (padding rows hash to +inf), and every element of y, padding rows
included, stays within attn_sweep's bounds of the float64 reference; in the three training modes every gradient matches
float64 autograd.  The worst error of every precision and gradient is printed at the end of the module (pytest -s)."""
import pytest

import src_attn_sweep as ssw

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_worst):
        val, sid = _worst[key]
        print(f"src attn sweep worst {key}: {val:.3e} ({sid})")


def _noter(prefix, sid):
    def note(key, val):
        k = f"{prefix} {key}"
        if val > _worst.get(k, (-1.0, ""))[0]:
            _worst[k] = (val, sid)
    return note


FWD = [pytest.param(s.id, p, id=f"{s.id}-{p}") for s in ssw.SHAPES for p in ssw.PRECISIONS]
BWD = [pytest.param(s.id, m, id=f"{s.id}-{m}") for s in ssw.BWD_SHAPES for m in ssw.TRAIN]


@pytest.mark.parametrize("sid,precision", FWD)
def test_src_block_forward_every_element_vs_float64(sid, precision, gpu_device):
    ssw.check_forward(ssw.BY_ID[sid], precision, gpu_device, _noter(f"forward {precision}", sid))


@pytest.mark.parametrize("sid,mode", BWD)
def test_src_block_training_every_gradient_vs_float64(sid, mode, gpu_device):
    ssw.check_backward(ssw.BY_ID[sid], mode, gpu_device, _noter(f"backward {mode}", sid))
