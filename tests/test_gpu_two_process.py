"""Several processes sharing ONE GPU (-m gpu): rank-dependent table slices computed by the HIP kernels in separate
processes and combined through torch.distributed -- including the production exchange (all-to-all of packed rows,
HIP combine of the received slices, all-gather).  RCCL refuses two ranks on one device, so the group is gloo (which
moves device tensors through the host); the RCCL collectives themselves are covered by tests/test_gpu_dist.py on a
1-rank group."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cases

pytestmark = pytest.mark.gpu

# Most ranks one test starts on the shared GPU: a GPU machine takes at most 6 processes with the device open at once,
# and this pytest process and the mp.Manager server forked from it hold it as well.  A case written for the 8 GPUs of
# a node runs min(8, MAX_RANKS) ranks here, with the same tables per rank and the same checks.
MAX_RANKS = 4


def _worker(rank, world, port, name, precision, mode, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from hept_amd import HEPTAttention

        dev = torch.device("cuda", 0)
        inp, _ = cases.load_case(name)
        g = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
        h, e, t = inp["alpha"].shape
        m = HEPTAttention(e, h_dim=24, num_heads=h, block_size=inp["block_size"], n_hashes=t, num_w_per_dist=10,
                          precision=precision, process_group=dist.group.WORLD)
        assert m.sharding.mode == "all_reduce" and m.sharding.local_tables()[1] in (1, 2)
        if mode != "all_reduce":
            from hept_amd.sharding import TableSharding

            m.sharding = TableSharding(t, dist.group.WORLD, mode=mode)
        m.load_state_dict({"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"],
                           "e2lsh.alpha": inp["alpha"]})
        m = m.to(dev).eval()
        w_rpe = torch.nn.Linear(inp["w_rpe_weight"].shape[1], inp["w_rpe_weight"].shape[0]).to(dev)
        with torch.no_grad():
            w_rpe.weight.copy_(g["w_rpe_weight"])
            out = m(g["q"], g["k"], g["v"], w_rpe=w_rpe, coords=g["coords"], combined_shifts=g["combined_shifts"])
        ret[rank] = out.cpu()
    finally:
        dist.destroy_process_group()


def _train_worker(rank, world, port, name, ret):
    """Table sharding under autograd: every rank differentiates its own tables, the ranks' gradients are summed."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from hept_amd import HEPTAttention

        dev = torch.device("cuda", 0)
        inp, _ = cases.load_case(name)
        g = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
        h, e, t = inp["alpha"].shape
        m = HEPTAttention(e, h_dim=24, num_heads=h, block_size=inp["block_size"], n_hashes=t, num_w_per_dist=10,
                          precision="bf16", process_group=dist.group.WORLD)  # 16-bit inference precision: trains in f32
        m.load_state_dict({"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"],
                           "e2lsh.alpha": inp["alpha"]})
        m = m.to(dev).train()
        w_rpe = torch.nn.Linear(inp["w_rpe_weight"].shape[1], inp["w_rpe_weight"].shape[0]).to(dev)
        with torch.no_grad():
            w_rpe.weight.copy_(g["w_rpe_weight"])
        q, k, v = (g[x].clone().requires_grad_(True) for x in "qkv")
        out = m(q, k, v, w_rpe=w_rpe, coords=g["coords"], combined_shifts=g["combined_shifts"])
        gen = torch.Generator().manual_seed(11)
        out.backward(torch.randn(out.shape, generator=gen).to(dev))
        ret[rank] = {"out": out.detach().cpu(), "dq": q.grad.cpu(), "dk": k.grad.cpu(), "dv": v.grad.cpu(),
                     "dw_rpe": w_rpe.weight.grad.cpu(), "dW": m.out_linear.weight.grad.cpu()}
    finally:
        dist.destroy_process_group()


def test_sharded_training_matches_single_process(gpu_device):
    name, world = "g6_block100", 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_train_worker, args=(world, port, name, ret), nprocs=world, join=True)
    from hept_amd import HEPTAttention

    inp, _ = cases.load_case(name)
    g = {k: v.to(gpu_device) for k, v in inp.items() if torch.is_tensor(v)}
    h, e, t = inp["alpha"].shape
    m = HEPTAttention(e, h_dim=24, num_heads=h, block_size=inp["block_size"], n_hashes=t, num_w_per_dist=10)
    m.load_state_dict({"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"],
                       "e2lsh.alpha": inp["alpha"]})
    m = m.to(gpu_device).train()
    w_rpe = torch.nn.Linear(inp["w_rpe_weight"].shape[1], inp["w_rpe_weight"].shape[0]).to(gpu_device)
    with torch.no_grad():
        w_rpe.weight.copy_(g["w_rpe_weight"])
    q, k, v = (g[x].clone().requires_grad_(True) for x in "qkv")
    out = m(q, k, v, w_rpe=w_rpe, coords=g["coords"], combined_shifts=g["combined_shifts"])
    gen = torch.Generator().manual_seed(11)
    out.backward(torch.randn(out.shape, generator=gen).to(gpu_device))
    want = {"out": out.detach().cpu(), "dq": q.grad.cpu(), "dk": k.grad.cpu(), "dv": v.grad.cpu(),
            "dw_rpe": w_rpe.weight.grad.cpu(), "dW": m.out_linear.weight.grad.cpu()}
    for r in range(world):
        for key, ref in want.items():
            scale = ref.abs().max().item() + 1e-30
            err = (ret[r][key] - ref).abs().max().item() / scale
            # same kernels on the same tables; only the association of the table sums differs (f32 round-off)
            assert err < 2e-5, (r, key, err)


# HEPT_TEST_BIG=<points>: the 8-rank test at a larger size (slow on a shared GPU: every rank polls its flags
# from time slice to time slice; a one-off check, not part of the default suite's sizes)
_SIZES = [int(os.environ["HEPT_TEST_BIG"])] if os.environ.get("HEPT_TEST_BIG") else [1500, 700]


def _synthetic_worker(rank, world, port, precision, exchange, ret, groups=2, view=False):
    """BASELINE config 4 in miniature: n_hashes = world, one table per rank, the production exchange."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["HEPT_EXCHANGE"] = exchange
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from hept_amd import HEPTAttention
        from hept_amd.sharding import TableSharding
        from hept_amd.synthetic import make_inputs

        dev = torch.device("cuda", 0)
        inp = make_inputs(_SIZES, block_size=128, n_hashes=world, seed=5, cluster_size=8)
        g = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
        m = HEPTAttention(30, h_dim=24, num_heads=8, block_size=128, n_hashes=world, num_w_per_dist=10,
                          precision=precision, process_group=dist.group.WORLD)
        m.sharding = TableSharding(world, dist.group.WORLD, mode="all_to_all", head_groups=groups, out_view=view)
        m.load_state_dict({"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"],
                           "e2lsh.alpha": inp["alpha"]})
        m = m.to(dev).eval()
        w_rpe = torch.nn.Linear(50, 192).to(dev)
        with torch.no_grad():
            w_rpe.weight.copy_(g["w_rpe_weight"])
            prev = kept = None
            for j in range(3):  # epochs advance, buffers are reused
                # (view mode: other values every step, the last step's are the ones compared with the plain operator;
                #  the output of step j must survive step j + 1, which writes the other region)
                v = g["v"] * float(3 - j) if view else g["v"]
                out = m(g["q"], g["k"], v, w_rpe=w_rpe, coords=g["coords"], combined_shifts=g["combined_shifts"])
                if view and prev is not None:
                    assert out.data_ptr() != prev.data_ptr() and torch.equal(prev, kept)
                prev, kept = out, out.clone()
        torch.cuda.synchronize()
        m.sharding.check()
        ret[rank] = (out.cpu(), m.sharding.describe())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("precision,groups,view", [("fp32", 2, False), ("bf16", 2, False), ("bf16", None, False),
                                                   ("mixed16", 1, False), ("bf16", None, True), ("fp32", 2, True)])
def test_eight_ranks_one_table_each_match_the_unsharded_operator(precision, groups, view, gpu_device):
    """An 8-GPU node's layout run as min(8, MAX_RANKS) processes sharing this GPU (see MAX_RANKS): n_hashes = #ranks,
    one table per rank, rows exchanged with the one-sided transport (buffers mapped across processes through HIP IPC) -- against the plain
    operator on all the tables.  One table per
    rank takes the DIRECT path: the block attention stores its rows straight into the owners' receive buffers and
    raises the flags itself (no table sum, no separate push); groups = None is the transport's own choice (1 launch).
    view: TableSharding(out_view=True) -- the output is read in the exchange buffer (two regions taken in turn)."""
    world = min(8, MAX_RANKS)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_synthetic_worker, args=(world, port, precision, "p2p", ret, groups, view), nprocs=world, join=True)
    assert all(torch.equal(ret[0][0], ret[r][0]) for r in range(1, world))
    assert "one-sided" in ret[0][1] and (groups is not None or "in auto head" in ret[0][1])
    from hept_amd import ops
    from hept_amd.synthetic import make_inputs

    inp = make_inputs(_SIZES, block_size=128, n_hashes=world, seed=5, cluster_size=8)
    g = {k: v.to(gpu_device) for k, v in inp.items() if torch.is_tensor(v)}
    plain = ops.forward(g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"],
                        g["out_weight"], g["out_bias"], block_size=128, w_per_dist=10, precision=precision).cpu()
    # one table per rank: block_attn's own rows travel (f32 rows, or packed rows without a second rounding); only the
    # association of the table sum differs from the unsharded combine
    torch.testing.assert_close(ret[0][0], plain, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("world,precision,groups", [(8, "bf16", None), (8, "fp32", 2), (3, "bf16", 2)])
def test_producer_signal_fallback_of_the_one_sided_exchange(world, precision, groups, gpu_device, monkeypatch):
    """HEPT_P2P_PRODUCER_SIGNAL=1: the protocol of rounds 2-4 -- every producing workgroup drains its
    stores and counts itself in, the last one raises the flags after a system-scope fence; the waiting kernels raise
    nothing -- kept as an A/B and a fallback beside "a kernel boundary is the completion signal".  Same outputs as the
    plain operator, on the direct-scatter path (one table per rank) with one and several head groups."""
    world = min(world, MAX_RANKS)
    monkeypatch.setenv("HEPT_P2P_PRODUCER_SIGNAL", "1")   # inherited by the spawned ranks; read once per process
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_synthetic_worker, args=(world, port, precision, "p2p", ret, groups, False), nprocs=world, join=True)
    assert all(torch.equal(ret[0][0], ret[r][0]) for r in range(1, world)) and "one-sided" in ret[0][1]
    from hept_amd import ops
    from hept_amd.synthetic import make_inputs

    inp = make_inputs(_SIZES, block_size=128, n_hashes=world, seed=5, cluster_size=8)
    g = {k: v.to(gpu_device) for k, v in inp.items() if torch.is_tensor(v)}
    plain = ops.forward(g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"],
                        g["out_weight"], g["out_bias"], block_size=128, w_per_dist=10, precision=precision).cpu()
    torch.testing.assert_close(ret[0][0], plain, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_producer_signal_fallback_with_several_tables_per_rank(precision, gpu_device, monkeypatch):
    """... and on the carried-push path (two ranks, the tables of g6 split between them: the table sum + push of a head
    group rides in the next group's block-attention launch and signals from there)."""
    monkeypatch.setenv("HEPT_P2P_PRODUCER_SIGNAL", "1")
    name, world = "g6_block100", 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, port, name, precision, "all_to_all", ret), nprocs=world, join=True)
    assert torch.equal(ret[0], ret[1])
    from hept_amd import ops

    inp, _ = cases.load_case(name)
    g = {k: v.to(gpu_device) for k, v in inp.items() if torch.is_tensor(v)}
    plain = ops.forward(g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"],
                        g["out_weight"], g["out_bias"], block_size=inp["block_size"], w_per_dist=10,
                        precision=precision).cpu()
    if precision != "fp32":
        err = (ret[0] - plain).abs().amax(-1)
        assert bool((err <= 4e-3 * (plain.abs().amax(-1) + 1e-2)).all())
    else:
        torch.testing.assert_close(ret[0], plain, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("world,mode,precision", [(2, "all_reduce", "fp32"), (2, "all_reduce", "bf16"),
                                                  (2, "all_to_all", "fp32"), (2, "all_to_all", "bf16"),
                                                  (3, "all_to_all", "bf16"), (3, "all_to_all", "mixed16")])
def test_processes_sharing_one_gpu(world, mode, precision, gpu_device):
    name = "g6_block100"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, port, name, precision, mode, ret), nprocs=world, join=True)
    assert all(torch.equal(ret[0], ret[r]) for r in range(1, world))
    from hept_amd import ops

    inp, _ = cases.load_case(name)
    g = {k: v.to(gpu_device) for k, v in inp.items() if torch.is_tensor(v)}
    plain = ops.forward(g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"],
                        g["out_weight"], g["out_bias"], block_size=inp["block_size"], w_per_dist=10,
                        precision=precision).cpu()
    if mode == "all_to_all" and precision != "fp32" and world < 3:
        # each rank's table sum travels as packed rows: numerators rounded to bf16 once more (world 3 = one table per
        # rank: block_attn's own packed rows are the exchange buffer, no extra rounding)
        err = (ret[0] - plain).abs().amax(-1)
        assert bool((err <= 4e-3 * (plain.abs().amax(-1) + 1e-2)).all())
    else:
        torch.testing.assert_close(ret[0], plain, rtol=1e-5, atol=1e-6)


def _lost_peer_worker(rank, world, port, ret):
    """Two ranks, one table each; after two good steps rank 1 stops taking part.  Rank 0's next step must not return
    plausible numbers: its waits time out (HEPT_P2P_TIMEOUT_S), the output is NaN, check() raises, and the step after
    that is refused by the C call without touching the GPU."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["HEPT_EXCHANGE"] = "p2p"
    os.environ["HEPT_P2P_TIMEOUT_S"] = "1.0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from hept_amd import HEPTAttention
        from hept_amd.sharding import TableSharding
        from hept_amd.synthetic import make_inputs

        dev = torch.device("cuda", 0)
        inp = make_inputs([700, 300], block_size=128, n_hashes=world, seed=5, cluster_size=8)
        g = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
        m = HEPTAttention(30, h_dim=24, num_heads=8, block_size=128, n_hashes=world, num_w_per_dist=10,
                          precision="bf16", process_group=dist.group.WORLD)
        m.sharding = TableSharding(world, dist.group.WORLD, mode="all_to_all")
        m.load_state_dict({"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"],
                           "e2lsh.alpha": inp["alpha"]})
        m = m.to(dev).eval()
        w_rpe = torch.nn.Linear(50, 192).to(dev)
        kw = dict(w_rpe=w_rpe, coords=g["coords"], combined_shifts=g["combined_shifts"])
        with torch.no_grad():
            w_rpe.weight.copy_(g["w_rpe_weight"])
            for _ in range(2):
                good = m(g["q"], g["k"], g["v"], **kw)
            torch.cuda.synchronize()
            m.sharding.check()
            dist.barrier()
            res = {"good_finite": bool(torch.isfinite(good).all())}
            if rank == 0:
                lost = m(g["q"], g["k"], g["v"], **kw)     # rank 1 never comes
                torch.cuda.synchronize()
                res["lost_all_nan"] = bool(torch.isnan(lost).all())
                try:
                    m(g["q"], g["k"], g["v"], **kw)
                    res["refused"] = "no"
                except RuntimeError as exc:
                    res["refused"] = str(exc)
                try:
                    m.sharding.check()
                    res["check"] = "no"
                except RuntimeError as exc:
                    res["check"] = str(exc)
            dist.barrier()
        ret[rank] = res
    finally:
        dist.destroy_process_group()


def test_a_lost_peer_poisons_the_output_and_is_reported(gpu_device):
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_lost_peer_worker, args=(world, port, ret), nprocs=world, join=True)
    assert ret[0]["good_finite"] and ret[1]["good_finite"]
    assert ret[0]["lost_all_nan"] is True
    assert "HEPT_ERR_COMM" in ret[0]["refused"] and "timed out" in ret[0]["refused"]
    assert "timed out" in ret[0]["check"]
