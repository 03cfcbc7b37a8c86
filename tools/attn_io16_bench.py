"""The one-call Attn block on bfloat16 activations (DESIGN: "16-bit activations in the block"), tracking-60k and
tracking-6k (B = 128, T = 3), bf16 and fp32 tiles, one GPU process:
  (a) the native call: ``ops.attn_block_forward(x16, ...)`` -- x read and y written as bfloat16 by the kernels;
  (b) the composition it replaces, spelled out on this tree: ``ops.attn_block_forward(x16.float(), ...).to(bfloat16)``;
  (c) with ``--parent-lib PATH`` (a ``libhept_hip.so`` built from the parent commit): the float32 block through the raw C
      entry ``hept_attn_block_forward`` of this tree's library and of the parent's, same pointers, same workspace -- the
      two kernel templates behind it were touched.
The variants alternate for ``--series`` series (at least two per variant; every other series runs them in the opposite
order, so that a variant's place in the sequence does not favour it); every timing is 20 warm-ups and then ``--reps``
calls ending in a device synchronise, under its own time limit.  Reported per variant: the median of its series and
their spread (max - min); the conditions compare against that spread.  The report goes to stdout and to ``--out``.
python tools/attn_io16_bench.py [--reps 300] [--series 3] [--parent-lib PATH] [--out profiles/attn_io16_bench.txt]"""
import argparse
import ctypes
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--series", type=int, default=3)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_io16_bench.txt"))
ap.add_argument("--limit", type=int, default=60, help="seconds allowed to one timing")
args = ap.parse_args()
if args.series < 2:
    sys.exit("attn_io16_bench: at least two series per variant (the spread is their difference)")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hept_amd import Attn, _lib, ops  # noqa: E402
from hept_amd.synthetic import workload_inputs  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("attn_io16_bench: no GPU visible (there is no CPU path to time)")
dev = torch.device("cuda", 0)
H, D, K, B = 8, 24, 10, 128
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def _expired(signum, frame):
    raise TimeoutError("timing exceeded its time limit")


signal.signal(signal.SIGALRM, _expired)


def timeit(fn):
    """us per call: 20 warm-ups, then --reps calls that end in a device synchronise."""
    signal.alarm(args.limit)
    try:
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e6
    finally:
        signal.alarm(0)


def parent_entry(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    fn = lib.hept_attn_block_forward
    fn.restype, fn.argtypes = _lib.SIGNATURES["hept_attn_block_forward"]
    lib.hept_abi_version.restype = ctypes.c_int
    return fn, lib.hept_abi_version()


def stage_us(fn):
    ops.profile_enable(2, 100)
    for _ in range(100):
        fn()
    torch.cuda.synchronize()
    st, cnt = ops.profile_read()
    ops.profile_enable(0)
    return {k: v / max(cnt, 1) * 1e3 for k, v in st.items()}


lib = _lib.load()
parent, parent_abi = parent_entry(args.parent_lib) if args.parent_lib else (None, None)
say(f"attn_io16_bench: {torch.cuda.get_device_name(0)}; bfloat16 x; {args.series} alternating series per variant, 20 warm-ups "
    f"+ {args.reps} calls per timing; spread = max - min of a variant's series"
    + (f"; parent library ABI {parent_abi}" if parent else "; no parent library given: (c) not measured"))
verdicts = []
for workload in ("tracking-60k", "tracking-6k"):
    inp = workload_inputs(workload, seed=0)
    n = inp["q"].shape[0]
    coords, codes = inp["coords"].to(dev), inp["combined_shifts"].to(dev)
    x32 = torch.randn(n, D, generator=torch.Generator().manual_seed(21)).to(dev)
    x16 = x32.bfloat16()
    for prec in ("bf16", "fp32"):
        torch.manual_seed(0)
        blk = Attn(6, precision=prec, h_dim=D, num_heads=H, block_size=B, n_hashes=3, num_w_per_dist=K)
        with torch.no_grad():   # synthetic features: scale q/k so that the attention is not degenerate
            blk.attn.e2lsh.alpha.copy_(inp["alpha"])
            blk.w_q.weight.mul_(0.3)
            blk.w_k.weight.mul_(0.3)
        blk = blk.to(dev).eval()
        params = {k: v.detach() for k, v in blk._block_params().items()}
        ws = torch.empty(ops.workspace_bytes(n, H, D, 6, 3, B, prec), device=dev, dtype=torch.uint8)
        common = dict(num_heads=H, block_size=B, w_per_dist=K, precision=prec, workspace=ws)

        def native():
            return ops.attn_block_forward(x16, coords, codes, params, **common)

        def composed():
            return ops.attn_block_forward(x16.float(), coords, codes, params, **common).to(torch.bfloat16)

        variants = {"(a) native bf16 x / y": native, "(b) x.float() -> block -> .to(bf16)": composed}
        if parent:
            _x, _c, st, (n_, h, d, c, t), pc, _ws, keep = ops._block_args(x32, coords, params, H, B, K, 1e-5, 1e-5, prec, ws)
            y32 = torch.empty(n, D, device=dev)
            raw_args = (x32.data_ptr(), coords.data_ptr(), codes.data_ptr(), ctypes.byref(st), n_, h, d, c, K, t, B, pc,
                        ws.data_ptr(), ws.numel(), y32.data_ptr(), ops.current_stream_ptr(dev))
            variants["(c) f32 block, this tree  "] = lambda: _lib.check(lib.hept_attn_block_forward(*raw_args), "this tree")
            variants["(c) f32 block, parent lib "] = lambda: _lib.check(parent(*raw_args), "parent")
        with torch.no_grad():
            same = torch.equal(native().view(torch.int16), composed().view(torch.int16))
            if parent:
                variants["(c) f32 block, this tree  "]()
                y_new = y32.clone()
                variants["(c) f32 block, parent lib "]()
                same_c = torch.equal(y_new.view(torch.int32), y32.view(torch.int32))
            times = {nm: [] for nm in variants}
            for i in range(args.series):          # the variants alternate, in the opposite order every other series
                order = list(variants.items())
                for nm, fn in (order if i % 2 == 0 else order[::-1]):
                    times[nm].append(timeit(fn))
            st_a, st_b = stage_us(native), stage_us(composed)
        say(f"{workload} tiles {prec} (N {n}): native == composed bit for bit: {same}"
            + (f"; f32 block this tree == parent bit for bit: {same_c}" if parent else ""))
        med, spr = {}, {}
        for nm, ts in times.items():
            med[nm], spr[nm] = statistics.median(ts), max(ts) - min(ts)
            say(f"  {nm:38s} us/call: {' '.join(f'{t:7.1f}' for t in ts)}   median {med[nm]:7.1f}  spread {spr[nm]:5.1f}")
        for nm, s in (("(a)", st_a), ("(b)", st_b)):
            say(f"  {nm} stages us: row builder {s['prep_hash']:.1f}  sort {s['sort_tables']:.1f}  block attention "
                f"{s['block_attn']:.1f}  combine + ffn {s['combine']:.1f}")
        ka, kb = list(variants)[:2]
        ok = med[ka] - med[kb] <= max(spr[ka], spr[kb])
        verdicts.append(ok)
        say(f"  condition (a) not slower than (b) by more than the spread: {'met' if ok else 'NOT met'} "
            f"((a) - (b) = {med[ka] - med[kb]:+.1f} us, spread {max(spr[ka], spr[kb]):.1f})")
        if parent:
            kc, kp = list(variants)[2:]
            ok = abs(med[kc] - med[kp]) <= max(spr[kc], spr[kp])
            verdicts.append(ok)
            say(f"  condition (c) f32 block within the spread of the parent's: {'met' if ok else 'NOT met'} "
                f"(this tree - parent = {med[kc] - med[kp]:+.1f} us, spread {max(spr[kc], spr[kp]):.1f})")
say(f"conditions met: {sum(verdicts)} of {len(verdicts)}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
