"""The autograd contract of the training path (tests/autograd_sweep.py, -m gpu): leaf subsets, accumulation, retain_graph,
two forwards before a backward, one module twice in a graph, stride-0 / transposed / scaled / zero / one-hot upstream
gradients, 16-bit leaves, checkpointing, the dispatch table and the refusal of a second derivative, on the operator (both
variants, both row builders, both d sqrt_w branches, table chunks), the fused and the composed ``Attn`` block, ``SrcAttn``
and a two-layer ``AttnStack``.  The baseline of every case is held to float64 autograd of the oracle on the permutations
the run itself used; every other cell to that baseline bit for bit.  One test per (case, mode, cell); the worst measured
errors against float64 are printed at the end of the module (pytest -s)."""
import pytest
import torch

import autograd_sweep as ags

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_worst):
        val, what = _worst[key]
        print(f"autograd sweep worst {key}: {val:.3e} ({what})")
    ags._base.clear()


def _noter(cid, mode):
    def note(key, val):
        key = f"{cid} {mode} {key}"
        if val > _worst.get(key, (-1.0, ""))[0]:
            _worst[key] = (val, f"{cid}-{mode}")

    return note


@pytest.mark.parametrize("cid,mode,cell", [pytest.param(*p, id="-".join(p)) for p in ags.PARAMS])
def test_contract_cell(cid, mode, cell, gpu_device, monkeypatch):
    ags.Cells(ags.BY_ID[cid], mode, gpu_device, monkeypatch, _noter(cid, mode)).run(cell)
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ags.DISPATCH_PRECISIONS)
@pytest.mark.parametrize("cid", ["op-generic", "op-src"])
def test_dispatch_table_of_the_operator(cid, precision, gpu_device):
    """Cell 8: training x grad mode x every subset of the seven leaves x precision."""
    n = ags.check_dispatch_op(ags.BY_ID[cid], precision, gpu_device)
    assert n == 2 * 2 * 128


@pytest.mark.parametrize("precision", ags.DISPATCH_PRECISIONS)
@pytest.mark.parametrize("cid", ["blk", "blk-composed", "blk-src", "stack2"])
def test_dispatch_table_of_the_blocks(cid, precision, gpu_device, monkeypatch):
    ags.check_dispatch_block(ags.BY_ID[cid], precision, gpu_device, monkeypatch)
