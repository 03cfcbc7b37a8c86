"""The block sweep (tests/block_sweep.py, -m gpu): every instantiation of block_attn_kernel, block_attn_split_kernel and
block_attn_coords_kernel -- precision x nkt = ceil(B/32) 1..8 x {B = 32 nkt, one key in the last tile, one key short} --
on inputs whose float32 result is an exact integer in any summation order, bit for bit against float64 from group
membership; the "mixed16_diff" edge cases (coordinates beyond the fp16 range, raw_size < N) per instantiation; and one
random-valued float64 cell per (family, nkt, fullness) at the bounds the project already has.  One test per case (a
failure names the instantiation); the worst figure of the float64 cells per family is printed at the end (pytest -s)."""
import pytest

import block_sweep as bs

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_worst):
        val, cid = _worst[key]
        print(f"block sweep worst {key}: {val:.3e} at {cid}")


def _env(monkeypatch, family):
    env = bs.FAMILIES[family][2]
    if env is None:
        monkeypatch.delenv("HEPT_DIFF_MFMA", raising=False)
    else:
        monkeypatch.setenv("HEPT_DIFF_MFMA", env)     # read on every call (csrc/block_attn.hip:819)


@pytest.mark.parametrize("cid", [c.id for c in bs.CASES])
def test_block_kernel_exact(cid, gpu_device, monkeypatch):
    case = bs.BY_ID[cid]
    _env(monkeypatch, case.family)
    bs.check_exact(case, gpu_device)


def _note(family, cid, fig):
    for name, val in fig.items():
        key = f"{family} {name}"
        if val > _worst.get(key, (-1.0, ""))[0]:
            _worst[key] = (val, cid)


@pytest.mark.parametrize("cid", [c.id for c in bs.F64_CASES])
def test_block_kernel_vs_float64(cid, gpu_device, monkeypatch):
    fc = bs.F64_BY_ID[cid]
    _env(monkeypatch, fc.family)
    _note(fc.family, cid, bs.check_f64(fc, gpu_device))


@pytest.mark.parametrize("cid", [c.id for c in bs.BWD_CASES])
def test_block_backward_exact(cid, gpu_device):
    bs.check_bwd(bs.BWD_BY_ID[cid], gpu_device)


@pytest.mark.parametrize("cid", [c.id for c in bs.BWD_F64_CASES])
def test_block_backward_vs_float64(cid, gpu_device):
    fc = bs.BWD_F64_BY_ID[cid]
    _note(fc.family, cid, bs.check_bwd_f64(fc, gpu_device))
