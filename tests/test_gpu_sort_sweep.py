"""The sort sweep (tests/sort_sweep.py, -m gpu): every reachable instantiation of chunk_sort_kernel, bucket_sort_kernel
and small_sort_kernel at the smallest N that selects it, and planted bucket populations at every branch of the bucket
kernels in all three key modes (example keys, the src variant's float shift, raw keys) -- whole permutations, q and k
halves, ``torch.equal`` against ``torch.sort(stable=True)`` of float64 keys computed on the host from the cell's inputs.
The slow paths run once more with their workspace guarded and pre-filled (tests/scratch_sweep.py's instrument), the
forward's own sort launch (region counters zeroed by the row builder, rider workgroups in the grid) on a cloud with a
pile of exact duplicates, and the region-size cells in the linear layout in one child process (HEPT_SORT_LINEAR is read
once per process).  One test per cell: a failure names the cell."""
import os
import subprocess
import sys

import pytest

import sort_sweep as so

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", [c.id for c in so.GPU_CELLS])
def test_sort_cell(cid, gpu_device):
    so.check(so.BY_ID[cid], gpu_device)


@pytest.mark.parametrize("pattern", so.SCRATCH_PATTERNS)
@pytest.mark.parametrize("cid", [c.id for c in so.SCRATCH_CELLS])
def test_slow_paths_under_the_scratch_contract(cid, pattern, gpu_device):
    so.check_scratch(so.BY_ID[cid], pattern, gpu_device)


@pytest.mark.parametrize("precision", so.LAUNCH_PRECISIONS)
def test_forward_sort_launch_on_a_pile_of_duplicates(precision, gpu_device):
    so.check_launch(precision, gpu_device)


@pytest.mark.parametrize("precision", so.LAUNCH_PRECISIONS)
def test_forward_src_sort_launch_on_a_pile_of_duplicates(precision, gpu_device):
    so.check_launch_src(precision, gpu_device)


def test_region_size_cells_in_the_linear_layout(gpu_device):
    """One fresh child with HEPT_SORT_LINEAR=1 (tests/sort_sweep.py's main): bucket_sort_kernel<1024, true, 64, false> and
    chunk_sort_kernel<*, true, false> below 131 073 keys, which no other call reaches."""
    env = dict(os.environ, HEPT_SORT_LINEAR="1")
    run = subprocess.run([sys.executable, os.path.abspath(so.__file__)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert f"{len(so.AB_CELLS)} cells in the linear layout, 0 mismatches" in run.stdout
