"""Shared inputs of the 16-bit Attn block tests (tests/test_gpu_attn_io16.py): seeded 16-bit activations with special
values, and the yardstick's bit comparison.  A plain module, not a conftest; nothing here touches the GPU at import."""
import torch

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
IO_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}   # HEPT_IN_*


def specials(dt):
    """-0.0, +- the largest value below 8 and, for fp16, subnormals including the smallest and the largest."""
    big = (torch.tensor([8.0], dtype=dt).view(torch.int16) - 1).view(dt)
    pool = [torch.tensor([-0.0], dtype=dt), big, -big]
    if dt is torch.float16:
        g = torch.Generator().manual_seed(77)
        sub = torch.randint(1, 0x400, (64,), generator=g, dtype=torch.int16).view(dt)
        edge = torch.tensor([1, 0x3FF], dtype=torch.int16).view(dt)      # the smallest and the largest subnormal
        pool += [sub, -sub, edge, -edge]
    return torch.cat(pool)


def round16(x, dt, seed):
    """x rounded to dt with ~1 % of the entries replaced by the special values (no inf, no NaN).  Returns the tensor
    and the flat indices of the replaced entries."""
    g = torch.Generator().manual_seed(seed)
    flat = x.to(dt).reshape(-1).clone()
    n = flat.numel()
    vals = specials(dt)
    idx = torch.randperm(n, generator=g)[:max(vals.numel(), n // 100)]
    flat[idx] = vals[torch.arange(idx.numel()) % vals.numel()]
    out = flat.reshape(x.shape)
    assert bool(torch.isfinite(out.float()).all())
    return out, idx


def bits(t):
    """Bit patterns: -0.0 and +0.0 differ, row buffers that hold f32 words inside 16-bit tagged tensors compare whole."""
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got), bits(want))


def partial_rows(tl, n, h, seed, packed, dev):
    """Seeded partial rows of the block attention: (tl, n, h, 32) f32 [24 numerators | denominator | 0], or the packed
    form of 16-bit tiles (tl, n, h, 16) int32 that ``ops.unpack_part`` widens: 12 words of bf16 numerator pairs (even
    column in the low half), the f32 denominator in word 12, zeros behind it."""
    g = torch.Generator().manual_seed(seed)
    num = torch.randn(tl, n, h, 24, generator=g)
    den = torch.rand(tl, n, h, generator=g) + 0.5
    if not packed:
        part = torch.zeros(tl, n, h, 32)
        part[..., :24] = num
        part[..., 24] = den
        return part.to(dev)
    words = num.bfloat16().view(torch.int16).to(torch.int32) & 0xFFFF
    part = torch.zeros(tl, n, h, 16, dtype=torch.int32)
    part[..., :12] = words[..., 0::2] | (words[..., 1::2] << 16)
    part[..., 12] = den.view(torch.int32)
    return part.to(dev)
