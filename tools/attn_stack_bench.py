"""The model's layer loop, L = 4 Attn blocks, on one GPU: (a) L ``Attn`` calls + ``torch.cat`` (every block owns a
workspace) against (b) ``AttnStack`` (one C call, one workspace, the concatenation written in place).  One process,
tracking-60k (B = 128, T = 3) and tracking-6k, bf16 and fp32; the two variants alternate a/b/a/b for three rounds, every
timing is 20 warm-ups and then REPS repetitions ending in a synchronise.  Prints ``torch.equal`` of the two results and
``torch.cuda.max_memory_allocated`` of each (measured in a fresh phase: its own modules, peak statistics reset).
python tools/attn_stack_bench.py [reps]"""
import gc
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hept_amd import Attn, AttnStack, ops  # noqa: E402
from hept_amd.synthetic import workload_inputs  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
L, ROUNDS = 4, 3
dev = torch.device("cuda", 0)
cfg = dict(h_dim=24, num_heads=8, block_size=128, n_hashes=3, num_w_per_dist=10, n_layers=L)


def build(kind, prec, alpha):
    torch.manual_seed(0)
    if kind == "stack":
        m = AttnStack(6, precision=prec, **cfg)
        layers = m.attns
    else:
        m = layers = torch.nn.ModuleList(Attn(6, precision=prec, **cfg) for _ in range(L))
    with torch.no_grad():
        for blk in layers:   # synthetic features: scale q/k so that the attention is not degenerate
            blk.attn.e2lsh.alpha.copy_(alpha)
            blk.w_q.weight.mul_(0.3)
            blk.w_k.weight.mul_(0.3)
    return m.to(dev).eval()


def loop(layers, x, kwargs):
    outs = [x]
    for blk in layers:
        outs.append(blk(outs[-1], kwargs))
    return torch.cat(outs, dim=-1)


def timeit(fn):
    with torch.no_grad():
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / REPS * 1e6


def peak(kind, prec, alpha, x, kwargs):
    """max_memory_allocated of building the modules and running three forwards, above what was allocated before."""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    m = build(kind, prec, alpha)
    with torch.no_grad():
        for _ in range(3):
            y = m(x, kwargs) if kind == "stack" else loop(m, x, kwargs)
    torch.cuda.synchronize()
    out = torch.cuda.max_memory_allocated(dev) - base
    del m, y
    return out


print(f"attn_stack_bench: L = {L}, {ROUNDS} rounds a/b, 20 warm-ups + {REPS} repetitions per timing; "
      f"{torch.cuda.get_device_name(0)}")
for workload in ("tracking-60k", "tracking-6k"):
    inp = workload_inputs(workload, seed=0)
    n = inp["q"].shape[0]
    x = torch.randn(n, 24, device=dev)
    kwargs = {"coords": inp["coords"].to(dev), "combined_shifts": inp["combined_shifts"].to(dev)}
    for prec in ("bf16", "fp32"):
        ws = ops.workspace_bytes(n, 8, 24, 6, 3, 128, prec)
        pk_a = peak("loop", prec, inp["alpha"], x, kwargs)
        pk_b = peak("stack", prec, inp["alpha"], x, kwargs)
        a, b = build("loop", prec, inp["alpha"]), build("stack", prec, inp["alpha"])
        with torch.no_grad():
            same = torch.equal(loop(a, x, kwargs), b(x, kwargs))
        ta, tb = [], []
        for _ in range(ROUNDS):
            ta.append(timeit(lambda: loop(a, x, kwargs)))
            tb.append(timeit(lambda: b(x, kwargs)))
        fmt = lambda ts: " ".join(f"{t:7.1f}" for t in ts)  # noqa: E731
        print(f"{workload} {prec} (N {n}, one workspace {ws / 1e6:.1f} MB): torch.equal {same}")
        print(f"  (a) {L} x Attn + cat  us/forward: {fmt(ta)}   peak memory {pk_a / 1e6:8.1f} MB")
        print(f"  (b) AttnStack        us/forward: {fmt(tb)}   peak memory {pk_b / 1e6:8.1f} MB"
              f"   (a - b = {(pk_a - pk_b) / ws:.2f} workspaces)")
        del a, b
