"""The src variant's Attn block at tracking-60k (raw_size = 60000, three tables) on one GPU: the one-call block
(``SrcAttn`` in eval, ``hept_attn_block_forward_src``) against the reference's composition (torch LayerNorm / Linear
around ``HEPTAttention(variant="src")``), at B = 100 and 128 in fp32 and bf16, with the fused call's stage times; then
one training step (forward + backward, dropout 0.1) with norm1 and the projections folded into the row builder against
the composed step (``Attn.fuse_training = False``).  python tools/src_attn_block_bench.py"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hept_amd import SrcAttn, ops  # noqa: E402
from hept_amd.prep import prepare_input_src  # noqa: E402
from hept_amd.synthetic import make_inputs_src  # noqa: E402

RAW, T = 60000, 3
dev = torch.device("cuda", 0)


def setup(b, precision, train=False):
    inp = make_inputs_src(RAW, block_size=b, n_hashes=T, seed=0)
    torch.manual_seed(0)
    blk = SrcAttn("hept", 6, precision=precision, h_dim=24, num_heads=8, block_size=b, n_hashes=T, num_w_per_dist=10,
                  pe_type="none").to(dev)
    with torch.no_grad():
        blk.attn.e2lsh.alpha.copy_(inp["alpha"])
        blk.w_q.weight.mul_(0.3)
        blk.w_k.weight.mul_(0.3)
    x_raw = torch.randn(RAW, 24, device=dev)
    x, kw = prepare_input_src(x_raw, inp["coords_raw"].to(dev), {"block_size": b, "regions": inp["regions"]})
    return (blk.train() if train else blk.eval()), x.contiguous(), kw


def composed(blk, x, kw):
    xn = blk.norm1(x)
    q, k, v = blk.w_q(xn), blk.w_k(xn), blk.w_v(xn)
    x1 = x + blk.attn(q, k, v, pe=kw["coords"], w_rpe=blk.w_rpe, **kw)
    return x1 + blk.ff(blk.norm2(x1))


def timeit(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


for b in (100, 128):
    for prec in ("fp32", "bf16"):
        blk, x, kw = setup(b, prec)
        with torch.no_grad():
            a, c = blk(x, kw), composed(blk, x, kw)
            err = (a - c).abs().amax(-1)
            ok = float((err <= 1e-3 * (c.abs().amax(-1) + 1)).float().mean())
            fused_us = timeit(lambda: blk(x, kw), 200) * 1e6
            comp_us = timeit(lambda: composed(blk, x, kw), 200) * 1e6
            ops.profile_enable(2, 100)
            for _ in range(100):
                blk(x, kw)
            torch.cuda.synchronize()
            stages, calls = ops.profile_read()
            ops.profile_enable(0)
        st = "  ".join(f"{k} {v / max(calls, 1) * 1e3:.1f}" for k, v in stages.items() if k in
                       ("prep_hash", "sort_tables", "block_attn", "combine"))
        print(f"src block B={b} {prec}: one call {fused_us:.1f} us   composed {comp_us:.1f} us   "
              f"(rows agreeing to 1e-3: {ok:.4f}; stages us: {st})", flush=True)

for b in (100, 128):
    blk, x0, kw = setup(b, "fp32", train=True)
    x = x0.clone().requires_grad_(True)
    gout = torch.randn_like(x0)

    def step():
        y = blk(x, kw)
        y.backward(gout)
        x.grad = None
        for p in blk.parameters():
            p.grad = None

    for fuse in (True, False, True, False):
        blk.fuse_training = fuse
        ms = timeit(step, 30, warm=5) * 1e3
        print(f"src block B={b} train step (fwd+bwd, fp32 tiles, dropout 0.1), norm1 + projections "
              f"{'folded into the row builder' if fuse else 'composed (torch modules)'}: {ms:.3f} ms", flush=True)
