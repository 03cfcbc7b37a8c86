"""The shape sweep (tests/shape_sweep.py, -m gpu): every element of every precision's output, and every module gradient,
against the reference arithmetic evaluated in float64 on the GPU's own permutations.  One test per shape and precision
(a failure names its shape); the worst error of every precision is printed at the end of the module (pytest -s)."""
import pytest
import torch

import shape_sweep as sw

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_worst):
        val, sid = _worst[key]
        print(f"shape sweep worst {key}: {val:.3e} ({sid})")


def _note(key, val, sid):
    if val > _worst.get(key, (-1.0, ""))[0]:
        _worst[key] = (val, sid)


FWD = [pytest.param(s.id, p, id=f"{s.id}-{p}") for s in sw.SHAPES for p in sw.PRECISIONS]
BWD = [pytest.param(s.id, t, id=f"{s.id}-{t}") for s in sw.BWD_SHAPES for t in sw.TRAIN_TILES]


@pytest.mark.parametrize("sid,precision", FWD)
def test_forward_every_element_vs_float64(sid, precision, gpu_device):
    res = sw.check_forward(sw.BY_ID[sid], precision, gpu_device)
    for k, v in res.items():
        _note(f"forward {precision} {k}", v, sid)


@pytest.mark.parametrize("sid,tiles", BWD)
def test_backward_every_gradient_vs_float64(sid, tiles, gpu_device):
    res = sw.check_backward(sw.BY_ID[sid], tiles, gpu_device)
    for k, v in res.items():
        _note(f"backward {tiles} tiles {k}", v, sid)
