"""The inference precisions side by side at tracking-60k (block 128, 3 tables), in one process, timed with HIP events.

python tools/precision_bench.py [--out profiles/mixed16_diff_bench.txt] [--reps 7] [--iters 50]

For "mixed16", "mixed16_diff", "fp32" and "fp32_diff" (a mode the library does not know is skipped, so the same file
measures an older checkout): the module forward, the fused ``Attn`` block in eval mode, and the block-attention stage of
the forward from ``hept_profile_*``.  Every figure is the median of ``--reps`` repetitions of ``--iters`` back-to-back
calls after a warm-up, with the spread (min .. max) of the repetitions beside it; the modes are interleaved inside a
repetition so that a drift of the box hits all of them alike."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hept_amd import Attn, HEPTAttention, ops  # noqa: E402
from hept_amd.synthetic import WORKLOADS, workload_inputs  # noqa: E402

MODES = ("mixed16", "mixed16_diff", "fp32", "fp32_diff")
WORKLOAD = "tracking-60k"


def known(mode):
    try:
        ops.precision_code(mode)
        return True
    except ValueError:
        return False


def timed(fn, iters):
    """Microseconds per call of ``iters`` back-to-back calls, between two HIP events on the current stream."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def stage_us(fn, iters):
    """The block-attention stage of ``fn``'s forward, microseconds per call (hept_profile_*, all stages bracketed)."""
    ops.profile_enable(2, iters)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    ms, n = ops.profile_read()
    ops.profile_enable(0)
    return ms["block_attn"] * 1e3 / max(n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mixed16_diff_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    inp = workload_inputs(WORKLOAD, seed=0)
    g = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
    h, e, t = inp["alpha"].shape
    c, n, b = inp["coords"].shape[1], inp["q"].shape[0], WORKLOADS[WORKLOAD]["block_size"]
    w_rpe = torch.nn.Linear((c - 1) * 10, h * 24).to(dev)
    with torch.no_grad():
        w_rpe.weight.copy_(g["w_rpe_weight"])
    x = torch.randn(n, 24, generator=torch.Generator().manual_seed(1)).to(dev)
    kw = dict(coords=g["coords"], combined_shifts=g["combined_shifts"])

    modes = [m for m in MODES if known(m)]
    runs = {}
    for mode in modes:
        op = HEPTAttention(e, h_dim=24, num_heads=h, block_size=b, n_hashes=t, num_w_per_dist=10, precision=mode)
        op.load_state_dict({"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"],
                            "e2lsh.alpha": inp["alpha"]})
        op = op.to(dev).eval()
        torch.manual_seed(3)
        blk = Attn(c, precision=mode, h_dim=24, num_heads=h, block_size=b, n_hashes=t, num_w_per_dist=10).to(dev).eval()
        runs[mode] = {"forward": (lambda op=op: op(g["q"], g["k"], g["v"], w_rpe=w_rpe, **kw)),
                      "attn_block": (lambda blk=blk: blk(x, kw))}

    samples = {(mode, what): [] for mode in modes for what in ("forward", "attn_block", "block_attn_stage")}
    with torch.no_grad():
        for mode in modes:
            for fn in runs[mode].values():
                for _ in range(args.warmup):
                    fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for mode in modes:
                for what, fn in runs[mode].items():
                    samples[(mode, what)].append(timed(fn, args.iters))
                samples[(mode, "block_attn_stage")].append(stage_us(runs[mode]["forward"], args.iters))

    # "mixed16_diff" with K > 0 launches hept_rpe_scale in front of its block attention (inside the stage figure above)
    with torch.no_grad():
        scale = [timed(lambda: ops.rpe_scale(g["w_rpe_weight"], h, 24, 10), args.iters) for _ in range(args.reps)]

    lines = [f"# tools/precision_bench.py: {WORKLOAD} (N = {n}, block {b}, {t} tables, C = {c}), {torch.cuda.get_device_name(0)}",
             f"# microseconds per call: median of {args.reps} repetitions of {args.iters} calls (min .. max), HIP events",
             f"# {'mode':14s} {'forward':>26s} {'Attn block (eval)':>26s} {'block_attn stage':>26s}"]
    for mode in modes:
        cells = []
        for what in ("forward", "attn_block", "block_attn_stage"):
            v = samples[(mode, what)]
            cells.append(f"{statistics.median(v):8.1f} ({min(v):6.1f} .. {max(v):6.1f})")
        lines.append(f"  {mode:14s} " + " ".join(f"{cell:>26s}" for cell in cells))
    lines.append(f"# hept_rpe_scale (one workgroup) with its output allocation, back to back: {statistics.median(scale):.1f} "
                 f"({min(scale):.1f} .. {max(scale):.1f}) us per call")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
