"""Edge-shape sweep of the caller-side preparation on the GPU (-m gpu): hept_prepare_probe, hept_prepare_input and
hept_prepare_input_src against the host mirror, bit for bit, on every case of tests/prepare_sweep.py -- the mirror
itself is pinned on the real reference's anchors by tests/test_prepare_sweep_cells.py.  Each case runs twice and must
give identical bits; real slots keep their order, every pad slot holds the code the reference's window defines, outputs
have the documented dtypes and shapes, inputs are untouched.  The batches the reference refuses with IndexError are
refused by the front end before anything is allocated or launched for them."""
import pytest

import prepare_sweep as ps

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [c for c in ps.EXAMPLE if not c.a.refuse], ids=lambda c: c.id)
def test_prepare_input_equals_the_mirror(case, gpu_device):
    ps.gpu_example(case, gpu_device)


@pytest.mark.parametrize("case", ps.SRC, ids=lambda c: c.id)
def test_prepare_input_src_equals_the_mirror(case, gpu_device):
    ps.gpu_src(case, gpu_device)


@pytest.mark.parametrize("case", ps.REFUSED, ids=lambda c: c.id)
def test_refused_before_anything_is_launched(case, gpu_device, monkeypatch):
    ps.gpu_refused(case, gpu_device, monkeypatch)
