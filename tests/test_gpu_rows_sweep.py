"""The rows sweep (tests/rows_sweep.py, -m gpu): every instantiation of prep_hash_kernel (6 (D, C) x tile type x TMAX 4 / 8 x
input type = 108) and of prep_generic_kernel (9, on four free head shapes) at N = 77, and every (tile type, input type) at
the boundary sizes (1 .. 33 points, the last size without grid-stride and one point, tile and workgroup beyond it, two
trips and a ragged third, raw_size < N on either side of the one-workgroup sort's capacity), on inputs whose float32
results are exact in any order: projections, rows, norm words, value rows, range partials and the code bound bit for bit
against float64, and the sort that follows against the stable sort of float64 keys computed on the host from the inputs.
Rounding cells hold the 16-bit rows to round-to-nearest-even on planted ties; the one-call forward is held to the staged
kernels where it launches the row builder with two roles.  One test per cell (a failure names the instantiation); the
worst figures of the rounding cells are printed at the end (pytest -s)."""
import pytest

import rows_sweep as rs

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_worst):
        val, cid = _worst[key]
        print(f"rows sweep worst {key}: {val:.3f} of the bound at {cid}")


@pytest.mark.parametrize("cid", [c.id for c in rs.CELLS if c.kind != "bound"])
def test_row_builder_exact(cid, gpu_device):
    rs.check_exact(rs.BY_ID[cid], gpu_device)


@pytest.mark.parametrize("cid", [c.id for c in rs.CODES_NONE_CELLS])
def test_code_bound_is_zero_without_codes(cid, gpu_device):
    rs.check_codes_none(rs.BY_ID[cid], gpu_device)


@pytest.mark.parametrize("cid", [c.id for c in rs.BOUND_CELLS])
def test_code_bound_is_only_a_scale(cid, gpu_device):
    rs.check_exact(rs.BY_ID[cid], gpu_device)
    rs.check_code_bound(rs.BY_ID[cid], gpu_device)


@pytest.mark.parametrize("cid", [c.id for c in rs.ROUND_CELLS])
def test_row_builder_rounding(cid, gpu_device):
    for name, val in rs.check_round(rs.BY_ID[cid], gpu_device).items():
        key = f"{rs.BY_ID[cid].tile} {name}"
        if val > _worst.get(key, (-1.0, ""))[0]:
            _worst[key] = (val, cid)


@pytest.mark.parametrize("n,hdc,precision", rs.two_role_cases(),
                         ids=[f"n{n}-h{h}d{d}c{c}-{p}" for n, (h, d, c), p in rs.two_role_cases()])
def test_two_role_launch_equals_staged(n, hdc, precision, gpu_device):
    rs.check_two_role(n, hdc, precision, gpu_device)
