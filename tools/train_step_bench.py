"""fwd + bwd of HEPTAttention (autograd path) at tracking-60k: ms per training step with fp32 tiles (default) and with
the opt-in bf16 tiles (``train_tiles = "bf16"``), and how far the bf16 gradients are from the fp32 ones.

``--precisions fp32,fp32_mfma,fp32_diff [--rounds 3]``: instead, the step time of each module precision (f32 training
tiles), the precisions alternating in one process for the given number of rounds; prints every round and the median.

``--modes mixed16_diff:fp32,mixed16_diff:mixed16,bf16:bf16 [--rounds 3]``: the same for (precision, train_tiles) pairs --
the way to time ``train_tiles = "mixed16"`` (the 16-bit difference-form step of "mixed16_diff") against that precision's
default f32 step and against the bf16-tiles step of a bf16 module, in one session."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hept_amd import HEPTAttention  # noqa: E402
from hept_amd.synthetic import workload_inputs  # noqa: E402

dev = torch.device("cuda", 0)
inp = workload_inputs("tracking-60k", seed=0)
g = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
m = HEPTAttention(30, h_dim=24, num_heads=8, block_size=128, n_hashes=3, num_w_per_dist=10).to(dev).train()
with torch.no_grad():
    m.e2lsh.alpha.copy_(g["alpha"])
w_rpe = torch.nn.Linear(50, 192).to(dev)
q, k, v = (g[x].clone().requires_grad_(True) for x in ("q", "k", "v"))
kw = dict(w_rpe=w_rpe, coords=g["coords"], combined_shifts=g["combined_shifts"])
gout = torch.randn(q.shape[0], 24, device=dev)


def step():
    out = m(q, k, v, **kw)
    out.backward(gout)
    q.grad = k.grad = v.grad = None


def grads():
    w_rpe.weight.grad = m.out_linear.weight.grad = None   # (step() lets the parameter gradients accumulate)
    out = m(q, k, v, **kw)
    out.backward(gout)
    res = [q.grad.clone(), k.grad.clone(), v.grad.clone(), w_rpe.weight.grad.clone(), m.out_linear.weight.grad.clone()]
    q.grad = k.grad = v.grad = w_rpe.weight.grad = m.out_linear.weight.grad = None
    return out.detach().clone(), res


def timed(steps=30, warmup=5):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


if "--precisions" in sys.argv:
    precisions = sys.argv[sys.argv.index("--precisions") + 1].split(",")
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
    times = {p: [] for p in precisions}
    for r in range(rounds):
        for p in precisions:
            m.precision = p
            times[p].append(timed())
            print(f"round {r} train step (fwd+bwd, precision {p}): {times[p][-1]:.3f} ms", flush=True)
    for p in precisions:
        print(f"train step (fwd+bwd, precision {p}): median {sorted(times[p])[len(times[p]) // 2]:.3f} ms, "
              f"min {min(times[p]):.3f}, max {max(times[p]):.3f} over {rounds} rounds")
    sys.exit(0)

if "--modes" in sys.argv:
    modes = [tuple(x.split(":")) for x in sys.argv[sys.argv.index("--modes") + 1].split(",")]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
    times = {md: [] for md in modes}
    for r in range(rounds):
        for md in modes:
            m.precision, m.train_tiles = md
            times[md].append(timed())
            print(f"round {r} train step (fwd+bwd, precision {md[0]}, train_tiles {md[1]}): {times[md][-1]:.3f} ms", flush=True)
    for md in modes:
        print(f"train step (fwd+bwd, precision {md[0]}, train_tiles {md[1]}): median {sorted(times[md])[len(times[md]) // 2]:.3f} ms, "
              f"min {min(times[md]):.3f}, max {max(times[md]):.3f} over {rounds} rounds")
    sys.exit(0)

ref_out, ref = None, None
for tiles in ("fp32", "bf16"):
    m.train_tiles = tiles
    out, gr = grads()
    if tiles == "fp32":
        ref_out, ref = out, gr
    else:   # the 16-bit training mode against the fp32 one: max error relative to each tensor's own scale
        rel = [float((a - b).abs().max() / b.abs().max()) for a, b in zip([out] + gr, [ref_out] + ref)]
        print("bf16 tiles vs fp32 tiles, max error / tensor scale: out %.2e  dq %.2e  dk %.2e  dv %.2e  dw_rpe %.2e  dW_out %.2e" % tuple(rel))
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(30):
        step()
    torch.cuda.synchronize()
    print(f"train step (fwd+bwd, {tiles} tiles): {(time.perf_counter() - t0) / 30 * 1e3:.3f} ms")
