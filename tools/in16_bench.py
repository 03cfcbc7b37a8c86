"""The module forward at tracking-60k (N = 60 032, B = 128, three tables) fed float32, bfloat16 and float16 query / key /
value, bf16 and fp32 tiles: what the natively read 16-bit rows buy against widening them in torch.  One
GPU process; every figure is the median of three timed regions after warm-up (the regions of the three input types
alternate), the spread is max - min of the three; every region runs under its own time limit.  Also the hept_profile_*
stage times of the row builder and the sort.  ``--tree DIR`` times the package of another checkout (a parent commit
built in DIR) with the same script:  python tools/in16_bench.py [--tree DIR] [--reps 1000]"""
import argparse
import os
import signal
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=1000)
ap.add_argument("--limit", type=int, default=60, help="seconds allowed to one region")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

import hept_amd  # noqa: E402
from hept_amd import HEPTAttention, _lib, ops  # noqa: E402
from hept_amd.synthetic import workload_inputs  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("in16_bench: no GPU visible (there is no CPU path to time)")
dev = torch.device("cuda", 0)
DTYPES = (("f32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16))


def _expired(signum, frame):
    raise TimeoutError("region exceeded its time limit")


signal.signal(signal.SIGALRM, _expired)


def region(fn, reps):
    """Seconds per call over `reps` calls that end in a device synchronise, under the time limit."""
    signal.alarm(args.limit)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    finally:
        signal.alarm(0)


inp = workload_inputs("tracking-60k", seed=0)
n = inp["q"].shape[0]
w_rpe = torch.nn.Linear(inp["w_rpe_weight"].shape[1], inp["w_rpe_weight"].shape[0]).to(dev)
with torch.no_grad():
    w_rpe.weight.copy_(inp["w_rpe_weight"])
kw = dict(w_rpe=w_rpe, coords=inp["coords"].to(dev), combined_shifts=inp["combined_shifts"].to(dev))
print(f"in16_bench: package {os.path.dirname(hept_amd.__file__)}  ABI {_lib.load().hept_abi_version()}  "
      f"tracking-60k N={n} B=128 T=3  {args.reps} forwards per region, 3 regions per figure", flush=True)

for tiles in ("bf16", "fp32"):
    m = HEPTAttention(30, h_dim=24, num_heads=8, block_size=128, n_hashes=3, num_w_per_dist=10, precision=tiles)
    m.load_state_dict({"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"],
                       "e2lsh.alpha": inp["alpha"]}, strict=True)
    m = m.to(dev).eval()
    m.reserve(n, 6, dev)
    qkv = {nm: [inp[x].to(dev).to(dt) for x in ("q", "k", "v")] for nm, dt in DTYPES}
    with torch.no_grad():
        calls = {nm: (lambda a=qkv[nm]: m(a[0], a[1], a[2], **kw)) for nm, _ in DTYPES}
        outs = {nm: calls[nm]() for nm, _ in DTYPES}
        for nm, _ in DTYPES:          # warm-up of every input type the timed regions use
            region(calls[nm], 50)
        times = {nm: [] for nm, _ in DTYPES}
        for _ in range(3):            # the input types alternate
            for nm, _ in DTYPES:
                times[nm].append(region(calls[nm], args.reps) * 1e6)
        stages = {}
        for nm, _ in DTYPES:
            ops.profile_enable(2, 100)
            region(calls[nm], 100)
            st, cnt = ops.profile_read()
            ops.profile_enable(0)
            stages[nm] = {k: v / max(cnt, 1) * 1e3 for k, v in st.items()}
    for nm, _ in DTYPES:
        t, s = times[nm], stages[nm]
        print(f"tiles {tiles:4s} inputs {nm:4s}: forward {statistics.median(t):7.1f} us  (regions "
              f"{' '.join(f'{x:.1f}' for x in t)}; spread {max(t) - min(t):.1f})   stages us: row builder "
              f"{s['prep_hash']:.1f}  sort {s['sort_tables']:.1f} (chunk sort {s['chunk_sort']:.1f}, bucket sort + riders "
              f"{s['sort_tables'] - s['chunk_sort']:.1f})  block attention {s['block_attn']:.1f}  combine {s['combine']:.1f}"
              f"   output dtype {str(outs[nm].dtype).replace('torch.', '')}", flush=True)
