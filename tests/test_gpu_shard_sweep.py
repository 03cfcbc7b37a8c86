"""The shard sweep (tests/shard_sweep.py, -m gpu): one process plays every rank of a table-sharded world in turn -- the
rows every rank sends bit for bit against forward_partial and the staged kernels, per row against float64 on the rank's
own permutations, the packed rows exactly, every combine against float64 of its own input, and every element of the
assembled output against float64 on the GPU's permutations.  One test per shape, world, head-group count, precision and
row format (a failure names them); the worst figure of every kind is printed at the end of the module (pytest -s)."""
import pytest

import shard_sweep as sh

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_worst):
        val, sid = _worst[key]
        print(f"shard sweep worst {key}: {val:.3e} ({sid})")


def _note(key, val, sid):
    if val > _worst.get(key, (-1.0, ""))[0]:
        _worst[key] = (val, sid)


RUNS = [pytest.param(s.id, w, g, p, f, id=f"{s.id}-w{w}-g{g}-{p}-{f}") for s in sh.SHAPES for (w, g, p, f) in sh.runs(s)]


@pytest.mark.parametrize("sid,world,groups,precision,fmt", RUNS)
def test_every_rank_of_a_world_vs_float64(sid, world, groups, precision, fmt, gpu_device):
    res = sh.check(sh.BY_ID[sid], world, groups, precision, fmt, gpu_device)
    for k, v in res.items():
        _note(f"{precision} {k}", v, f"{sid} W={world} G={groups} {fmt}")
