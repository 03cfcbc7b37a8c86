"""bench.py's output contract (-m gpu): exactly one line on stdout, valid JSON, every key the driver reads; the
forced-exchange path (1-rank RCCL group) keeps stdout clean of RCCL's banner."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline"}
ROOF = {"bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "frac_of_copy", "traffic_source"}


def _run(*args, **env_extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", **env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "2", *args],
                         capture_output=True, text=True, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, run.stdout
    return json.loads(lines[0])


def _check_traffic(roof):
    """round 6: a PMC record is copied only for ITS (workload, template) -- pmc_record compares WRITE_SIZE with the launch's
    partial rows -- so the counters' traffic must sit near the launch's algorithmic bytes: at least the rows written plus
    every gathered row once (the three tables' gathers of a row can meet in L2: >= 0.45), at most 1.5x (round 5 shipped a
    6k cloud carrying the 60k cloud's 751 MB: 11.9x)."""
    ratio = roof["traffic"] / roof["algorithmic_bytes"]
    assert 0.45 <= ratio <= 1.5, ratio


def _check_whole_step(rec, n_launches):
    """round 5: every launch of the step with its algorithmic bytes, and the step's bytes over the timed step time"""
    ks = rec["kernels"]
    assert len(ks) == n_launches and all(k["ms"] > 0 and k["algorithmic_bytes"] > 0 and 0.0 < k["frac"] < 1.5 for k in ks)
    sr = rec["step_roofline"]
    assert sr["algorithmic_bytes"] == sum(k["algorithmic_bytes"] for k in ks)
    assert abs(sr["achieved"] - sr["algorithmic_bytes"] / (rec["ms_per_step"] * 1e-3) / 1e9) / sr["achieved"] < 1e-6
    assert 0.0 < sr["frac"] < 1.0 and abs(sr["frac"] - sr["achieved"] / 8000.0) < 1e-9
    # the event-timed launches add up to about the step (no gaps between them; the brackets' own cost is taken off)
    assert 0.7 < sum(k["ms"] for k in ks) / rec["ms_per_step"] < 1.3


def _check_headline(d, precision, dtype):
    """The contract's fields and the headline roofline (read off the timed region's own HIP events): in every line"""
    assert d["config"]["rccl_ranks"] == 0
    assert KEYS <= set(d) and ROOF <= set(d["roofline"])
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["metric"] == "attention-fwd points/sec" and d["unit"] == "points/s" and d["scaling"] == "weak"
    assert d["dtype"].startswith(dtype) and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "tracking-60k" in d["config"]["workload"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and 0.0 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert abs(r["frac_of_copy"] - r["achieved"] / 6290.0) < 1e-9
    # PMC traffic is copied from profiles/ only when the record belongs to this build and this kernel template
    src = r["traffic_source"]
    assert src["kernel_launched"].startswith("block_attn_split_kernel<4" if precision == "fp32" else "block_attn_kernel<4")
    if r["traffic"] is None:
        # refused for a reason that is not this test's business (a stale digest on a tree under development) -- but never
        # because bench.py and the library disagree about the NAME of the kernel that ran (round 6 shipped that twice)
        assert "refused" in src and "no PMC pass" not in src["refused"], src
    else:
        assert "refused" not in src and src["kernel_launched"] in src["kernel_measured"].replace(" ", "")
        assert src["workload_key"] == f"c3/{precision}"
        _check_traffic(r)
    assert 0.0 < r["frac"] <= r["frac_adjusted"] < 1.0 and "HIP events" in r["timing_method"]
    assert 1e7 < d["value"] < 1e10 and abs(d["value"] - 60000 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6


@pytest.mark.parametrize("precision,dtype", [("bf16", "bf16"), ("fp32", "f32")])
def test_bench_line(precision, dtype, gpu_device):
    d = _run("--full", "--precision", precision, "--no-cpu-baseline")
    _check_whole_step(d, 5)
    assert [k["name"].split()[0] for k in d["kernels"]][1:3] == ["chunk_sort_kernel", "bucket_sort_kernel"]
    if precision == "bf16":  # the --full run carries the reference-precision record and BASELINE config 4
        f = d["fp32"]
        assert f["dtype"].startswith("f32 rows") and "split-bf16" in f["dtype"]
        assert f["ms_per_step"] > d["ms_per_step"] and 0.0 < f["roofline"]["frac"] < 1.0
        assert f["roofline"]["bound"] in ("hbm", "mfma") and f["roofline"]["kernel"] == "block_attn_split_kernel"
        _check_whole_step(f, 5)
        assert d["c4"]["ms_per_step"] < d["ms_per_step"] and "n_hashes=1" in d["c4"]["workload"]
        assert 0.5 < d["mixed16"]["ms_per_step"] / d["ms_per_step"] < 1.5      # the every-row-tight 16-bit mode
        # every other BASELINE configuration: c1, c2, c5, the reference's own block size and (round 5) ten tracking-6k
        # clouds batched into one call, both precisions.  (No cross-precision timing ratio for the short clouds: those
        # forwards are 35-55 us against 33 us of host issue, medians of three 20-step regions on a shared host.)
        for key, n_raw, bs in (("c1", 4096, 64), ("c2", 6000, 128), ("c2x10", 60000, 128), ("c5", 60000, 256),
                               ("b100", 60000, 100)):
            for prec in ("fp32", "bf16"):
                rec = d[key][prec]
                assert rec["n_raw"] == n_raw and rec["block_size"] == bs and rec["ms_per_step"] > 0
                assert abs(rec["value"] - n_raw / (rec["ms_per_step"] * 1e-3)) / rec["value"] < 1e-6
                roof = rec["roofline"]
                assert roof["bound"] in ("hbm", "mfma") and 0.0 < roof["frac"] < 1.0
                # the bound is read off counters when a PMC record of this build exists for the launched template
                if roof["traffic"] is None:
                    assert roof["bound"] == "hbm" and roof["traffic_refused"]
                else:
                    ev = roof["bound_evidence"]
                    assert (roof["bound"] == "hbm") == (ev["hbm_frac_of_copy_on_traffic"] >= ev["issue_frac"])
                    _check_traffic(roof)
        # the batched call runs ten 6k clouds at the per-point rate of one 60k cloud, not of one 6k cloud
        assert d["c2x10"]["bf16"]["value"] > 2.0 * d["c2"]["bf16"]["value"]
    _check_headline(d, precision, dtype)
    # the driver keeps the last 8 KB of stdout: the reference-precision record, the per-launch list and the summary close
    # the line, the long per-configuration records open it
    keys = list(d)
    assert keys[-1] == "summary" and d["summary"]["ms_per_step"] == d["ms_per_step"]
    assert keys.index("step_roofline") > keys.index("metric")
    if precision == "bf16":
        assert keys.index("fp32") > keys.index("c5") and keys.index("fp32") > keys.index("metric")
        assert d["summary"]["fp32_ms_per_step"] == d["fp32"]["ms_per_step"]
        tail = json.dumps(d)[-8192:]
        assert '"fp32": {"ms_per_step"' in tail and '"step_roofline"' in tail and '"kernels"' in tail


@pytest.mark.parametrize("precision,dtype", [("bf16", "bf16"), ("fp32", "f32")])
def test_plain_bench_line_is_the_headline_alone(precision, dtype, gpu_device):
    """Without --full the line carries the contract's fields, the headline roofline and the summary, and nothing that
    takes runs of its own: no other precision or configuration, no per-launch list, no CPU baseline."""
    d = _run("--precision", precision)
    _check_headline(d, precision, dtype)
    assert list(d) == ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                       "vs_baseline", "dtype", "data", "config", "roofline", "summary"]
    assert d["config"]["comm_world"] == 0 and d["config"]["transport"] is None
    assert set(d["summary"]) == {"ms_per_step", "points_per_s", "block_attn_ms", "roofline_frac", "traffic", "mfma_busy_frac"}
    assert d["summary"]["ms_per_step"] == d["ms_per_step"] and d["summary"]["points_per_s"] == d["value"]


def test_bench_dumps_the_output_of_its_last_timed_step(tmp_path, gpu_device):
    """--dump-outputs DIR: the headline forward's output (what its caller receives) as DIR/out.npy in float32, equal to
    the plain operator on the same seeded inputs -- so two builds can be compared output for output."""
    import numpy as np
    import torch

    from hept_amd import ops
    from hept_amd.synthetic import workload_inputs

    d = _run("--no-extra", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "dump"))
    assert d["steps"] == 20 and d["ms_per_step"] > 0
    out = np.load(tmp_path / "dump" / "out.npy")
    inp = workload_inputs("tracking-60k", seed=0)
    g = {k: v.to(gpu_device) for k, v in inp.items() if torch.is_tensor(v)}
    plain = ops.forward(g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"],
                        g["out_weight"], g["out_bias"], block_size=128, w_per_dist=10, precision="bf16").cpu()
    assert out.dtype == np.float32 and out.shape == tuple(plain.shape) and np.isfinite(out).all()
    torch.testing.assert_close(torch.from_numpy(out), plain, rtol=1e-5, atol=1e-6)


def test_bench_line_with_the_exchange_forced_on(gpu_device):
    d = _run("--force-dist", "--no-cpu-baseline")
    assert KEYS <= set(d) and "exchange" in d["config"]["parallelism"] and d["config"]["rccl_ranks"] == 1


@pytest.mark.parametrize("ranks", [2, 8])
def test_bench_launches_its_own_ranks(ranks, gpu_device):
    """`python bench.py --gpus N` with WORLD_SIZE unset: the parent starts N ranks (here they share the one GPU through
    a gloo group: RCCL refuses two ranks per device), relays rank 0's line and exits 0.  (The 8-GPU case runs 4 ranks
    here: a GPU machine takes at most 6 processes with a device open at once, and this pytest process holds one too.)"""
    ranks = min(ranks, 4)
    # (HEPT_EXCHANGE=torch: the collectives go through gloo.  The one-sided transport polls arrival flags on the GPU,
    # and N processes polling on ONE shared GPU crawl from time slice to time slice; it is covered on small inputs by
    # tests/test_gpu_two_process.py.)
    d = _run("--full", "--gpus", str(ranks), "--no-cpu-baseline", HEPT_BENCH_BACKEND="gloo", HEPT_BENCH_EXCHANGE="all_to_all",
             HEPT_EXCHANGE="torch")
    assert KEYS <= set(d) and d["n_gpus"] == ranks and d["scaling"] == "weak"
    assert f"({3 * ranks} total)" in d["config"]["workload"] and "all_to_all" in d["config"]["parallelism"]
    assert abs(d["value"] - ranks * 60000 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    assert f"n_hashes={ranks}" in d["c4"]["workload"]


def test_bench_walks_down_the_transport_ladder(gpu_device):
    """A one-sided wait that times out (here: a 1-microsecond bound with two ranks sharing the GPU) must not hang or
    poison the run: the status word reports it, every rank steps down to the next transport together, and the line
    names the exchange that actually ran."""
    d = _run("--gpus", "2", "--no-cpu-baseline", "--no-extra", HEPT_BENCH_BACKEND="gloo",
             HEPT_BENCH_EXCHANGE="all_to_all", HEPT_P2P_TIMEOUT_S="0.000001")
    assert d["n_gpus"] == 2 and "torch.distributed" in d["config"]["parallelism"]


def test_bench_launcher_reports_a_failing_rank(gpu_device):
    env = dict(os.environ, HEPT_BENCH_BACKEND="gloo", HEPT_BENCH_FAIL_RANK="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "1",
                          "--no-cpu-baseline"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert run.returncode != 0 and not [ln for ln in run.stdout.splitlines() if ln.startswith("{")]


def test_bench_as_a_rank_under_torch_distributed_run(gpu_device):
    """The driver's own multi-GPU command: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
    127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W` -- bench.py finds WORLD_SIZE set and is a rank
    (here 2 ranks share the GPU through a gloo group); exactly one JSON line, from rank 0."""
    env = dict(os.environ, HEPT_BENCH_BACKEND="gloo", HEPT_BENCH_EXCHANGE="all_to_all", HEPT_EXCHANGE="torch")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29643", os.path.join(ROOT, "bench.py"),
                          "--gpus", "2", "--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline"],
                         capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, run.stdout
    d = json.loads(lines[0])
    assert KEYS <= set(d) and d["n_gpus"] == 2 and d["steps"] == 20 and d["warmup"] == 5
    assert "(6 total)" in d["config"]["workload"] and d["c4"]["ms_per_step"] > 0
