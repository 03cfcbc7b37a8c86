"""The scratch contract on the GPU (tests/scratch_sweep.py, -m gpu): every case once on untouched allocations and once
under each pattern -- ``leftover`` (the buffers of a donor case of another size, seed and precision), ``zero`` and ``ff``
(NaN in every float format, -1 in every integer) -- with every allocation of the Python layer guarded.  All assertions
are bitwise: (a) every returned tensor, gradient and permutation equals the clean run and holds no pattern word, (b) no
guard byte around any buffer or workspace -- each sized at exactly what its ``*_bytes`` function returns -- is touched,
(c) no input changes (the documented in-out arguments are idempotent instead), (d) the gradients of A do not change when
forward(B) runs on the same module between forward(A) and backward(A).  One test per case and pattern; the slowest
cases are printed at the end of the module (pytest -s)."""
import time

import pytest
import torch

import scratch_sweep as ss

pytestmark = pytest.mark.gpu

_times = {}
_faulted = []     # a HIP error ends the sweep: nothing more is started on a GPU that has faulted


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    print(f"scratch sweep: {len(ss.CASES)} cases x {len(ss.PATTERNS)} patterns in {time.perf_counter() - t0:.1f} s; slowest:")
    for key in sorted(_times, key=_times.get, reverse=True)[:8]:
        print(f"  {_times[key]:6.2f} s  {key}")


# pattern-major inside a case, in the order of ss.PATTERNS: the clean run of a case is computed once and shared
PARAMS = [pytest.param(c.id, p, id=f"{c.id}-{p}") for c in ss.CASES for p in ss.PATTERNS]


@pytest.mark.parametrize("cid,pattern", PARAMS)
def test_results_do_not_depend_on_scratch(cid, pattern, gpu_device):
    if _faulted:
        pytest.fail(f"not run: {_faulted[0]} ended with a HIP error")
    case = ss.BY_ID[cid]
    t0 = time.perf_counter()
    try:
        hit = ss.check(case, pattern, gpu_device)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP" in str(e) or "hip" in str(e) or "illegal memory access" in str(e):
            _faulted.append(f"{cid}-{pattern}")
        raise
    finally:
        _times[f"{cid}-{pattern}"] = time.perf_counter() - t0
    # the mirror of tests/test_scratch_cells.py: the sites the SITES table lists for the case were reached
    missing = ss.expected_sites(case) - hit
    assert not missing, f"{cid}: allocation sites listed in SITES but not reached: {sorted(missing)} (reached {sorted(hit)})"
