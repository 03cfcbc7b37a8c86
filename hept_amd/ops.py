"""Torch-tensor front end of the C ABI: argument checks, workspace from the caching allocator, current stream.

PyTorch is plumbing here (device memory + streams); all arithmetic runs in the
HIP kernels of ``csrc/``.  Stage-level functions exist so that the parity tests
can check every stage against the oracle and inject permutations.
"""
from __future__ import annotations

import ctypes
import functools
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import PREC_BF16, PREC_F32, PREC_F32_DIFF, PREC_F32_MFMA, PREC_MIXED16, PREC_MIXED16_DIFF

__all__ = [
    "precision_code", "rpe_scale", "prep_hash", "sort_tables", "block_attn", "block_attn_coords", "reduce_tables", "combine_out",
    "forward", "forward_partial", "workspace_bytes", "profile_enable", "profile_read", "unpack_part",
    "segmented_argsort", "block_attn_bwd", "block_attn_bwd_coords", "sort_tables_src", "forward_src", "forward_partial_src", "geo_args",
    "packed_partials", "prep_hash_fused", "combine_ffn", "attn_block_forward", "attn_block_forward_src", "attn_stack_forward",
    "attn_stack_forward_src", "combine_bwd", "rpe_scale_bwd",
    "partial_begin", "partial_heads", "combine_groups", "forward_sharded", "rows_wgrad", "ln_bwd", "ln_ffn_fwd",
    "ln_ffn_bwd",
]


def precision_code(precision) -> int:
    if isinstance(precision, int) and not isinstance(precision, bool) and precision in (PREC_F32, PREC_BF16, PREC_MIXED16, PREC_F32_MFMA, PREC_F32_DIFF, PREC_MIXED16_DIFF):
        return precision
    if precision == "mixed16":
        return PREC_MIXED16
    if precision == "mixed16_diff":
        return PREC_MIXED16_DIFF
    if precision in ("fp32", "f32") or precision is torch.float32:
        return PREC_F32
    if precision == "fp32_mfma":
        return PREC_F32_MFMA
    if precision == "fp32_diff":
        return PREC_F32_DIFF
    if precision == "bf16" or precision is torch.bfloat16:
        return PREC_BF16
    raise ValueError(f"precision must be 'fp32', 'bf16', 'mixed16', 'fp32_mfma', 'fp32_diff' or 'mixed16_diff', got {precision!r}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream_ptr(device) -> int:
    """The current HIP stream of ``device`` as the integer the C ABI takes.  ``torch._C._cuda_getCurrentRawStream`` is one C
    call (0.2 us); ``torch.cuda.current_stream(...).cuda_stream`` builds a Stream object first (2 us of the ~30 us a forward
    costs the host) and is the fallback where the private entry point is missing."""
    if _raw_stream is not None and device.index is not None:
        return _raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


def _stream(t: torch.Tensor) -> int:
    return current_stream_ptr(t.device)


def _on_device(fn):
    """The C ABI launches on the thread's *current* HIP device: make that the device of the first GPU tensor argument
    for the duration of the call (a module on cuda:1 called while cuda:0 is current)."""

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        dev = next((a.device for a in args if torch.is_tensor(a) and a.is_cuda), None)
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)

    return wrapped


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype is torch.float32 and t.is_cuda and t.is_contiguous() and not (t.data_ptr() & 15):
        return t   # the usual case, checked first: this function runs a dozen times per forward
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (hept_amd has no CPU path); got device {t.device}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    t = t.contiguous()
    # the kernels read rows and weight columns as 16-byte pieces (include/hept_hip.h: hept_combine_out refuses other
    # bases): a contiguous VIEW at an odd storage offset gets an aligned copy here instead of an error there
    return t.clone() if t.data_ptr() % 16 else t


# element types the *_in entry points read natively (include/hept_hip.h: HEPT_IN_*)
_IN_CODE = {torch.float32: _lib.IN_F32, torch.bfloat16: _lib.IN_BF16, torch.float16: _lib.IN_F16}
IN_F32, IN_BF16, IN_F16 = _lib.IN_F32, _lib.IN_BF16, _lib.IN_F16


def _inc(t: torch.Tensor, name: str) -> torch.Tensor:
    """``_f32c`` for query / key / value, which may also be bfloat16 or float16: the row builder widens 16-bit rows in
    registers (every such value is a float32 value), so no float32 copy is made."""
    if t.dtype in _IN_CODE and t.is_cuda and t.is_contiguous() and not (t.data_ptr() & 15):
        return t
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (hept_amd has no CPU path); got device {t.device}")
    if t.dtype not in _IN_CODE:
        raise TypeError(f"{name} must be float32, bfloat16 or float16, got {t.dtype}")
    t = t.contiguous()
    # (the tuned row builder fetches 16-byte pieces of 16-bit rows as well: the same repair as _f32c)
    return t.clone() if t.data_ptr() % 16 else t


def _rowsc(t: torch.Tensor, name: str) -> torch.Tensor:
    """``_f32c`` for the row tensors the stage functions hand from one stage to the next -- f32 rows, hashes and hash
    ranges, bf16 / f16 tiles, packed partial rows (int32): the kernels index them as dense arrays and move their rows as
    16-byte pieces, so a strided view or a view at an odd storage offset gets a dense, aligned copy instead of being read
    as if it were dense."""
    if t.dtype is torch.float32:
        return _f32c(t, name)
    if t.dtype is not torch.int32:
        return _inc(t, name)   # bfloat16 / float16 tiles (any other type is refused there)
    if t.is_cuda and t.is_contiguous() and not (t.data_ptr() & 15):
        return t
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (hept_amd has no CPU path); got device {t.device}")
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _qkv_in(q, k, v):
    """query, key, value as the C ABI takes them and their common HEPT_IN_* code; the three must share one dtype."""
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError(f"query, key and value must share one dtype (float32, bfloat16 or float16), got "
                        f"{q.dtype}, {k.dtype} and {v.dtype}")
    q, k, v = _inc(q, "query"), _inc(k, "key"), _inc(v, "value")
    return q, k, v, _IN_CODE[q.dtype]


def _dims(q: torch.Tensor, coords: torch.Tensor, alpha: torch.Tensor) -> Tuple[int, int, int, int, int]:
    n, hd = q.shape
    h, e, t = alpha.shape
    c = coords.shape[1]
    if hd % h != 0 or hd // h + c != e:
        raise ValueError(f"inconsistent sizes: q {tuple(q.shape)}, coords {tuple(coords.shape)}, alpha {tuple(alpha.shape)}")
    return n, h, hd // h, c, t


@functools.lru_cache(maxsize=256)
def _workspace_bytes_cached(n: int, h: int, d: int, c: int, tl: int, b: int, prec: int) -> int:
    # a pure function of the sizes (no tensor, no parameter): remembered per shape -- one ctypes round trip less per call
    return int(_lib.load().hept_workspace_bytes(n, h, d, c, tl, b, prec))


@functools.lru_cache(maxsize=256)
def _check_shape_cached(n: int, h: int, d: int, c: int, tl: int, b: int) -> int:
    return int(_lib.load().hept_check_shape(n, h, d, c, tl, b))


def _workspace(workspace, n, h, d, c, tl, b, prec, like, grow: bool = True) -> torch.Tensor:
    """Shape check and workspace of a whole-operator call: ``workspace`` if it is large enough, else a new one on the
    device of ``like`` -- or, for the callers whose workspace carries state from call to call (``grow=False``), a refusal."""
    _lib.check(_check_shape_cached(n, h, d, c, tl, b), "hept_check_shape")
    need = _workspace_bytes_cached(n, h, d, c, tl, b, prec)
    if workspace is None or workspace.numel() < need:
        if not grow:
            raise ValueError(f"workspace too small: size it with ops.workspace_bytes ({need} bytes)")
        workspace = torch.empty(need, device=like.device, dtype=torch.uint8)
    return workspace


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return t.data_ptr() if t is not None else None


def _out_linear(weight, bias):
    """out_linear's weight and optional bias: their two pointers as the C ABI takes them, and the tensors they point into."""
    w = _f32c(weight, "out_linear.weight")
    if bias is None:
        return (w.data_ptr(), None), w
    b = _f32c(bias, "out_linear.bias")
    return (w.data_ptr(), b.data_ptr()), (w, b)


def _codes(codes: torch.Tensor, shape=None, exc=ValueError) -> torch.Tensor:
    """The AND codes as the kernels read them: int64, on the GPU (a host address must never reach a kernel), contiguous,
    (T, H, N) where the caller knows the sizes."""
    if codes.dtype != torch.int64 or not codes.is_cuda or (shape is not None and codes.shape != shape):
        raise exc(f"combined_shifts must be an int64 GPU tensor{'' if shape is None else f' of shape {shape}'}, "
                  f"got {codes.dtype} {tuple(codes.shape)} on {codes.device}")
    return codes.contiguous()


def _raw_size(raw_size, n: int) -> int:
    raw_size = int(raw_size)
    if not 0 <= raw_size <= n:
        raise ValueError(f"raw_size must lie in [0, {n}], got {raw_size}")
    return raw_size


# dtype tag of the row buffers: bf16 / f16 (mixed16: q^,k^ halves are fp16, the v half of kvhat is bf16) / f32
_TILE = {PREC_F32: torch.float32, PREC_BF16: torch.bfloat16, PREC_MIXED16: torch.float16,
         PREC_F32_MFMA: torch.float32, PREC_F32_DIFF: torch.float32, PREC_MIXED16_DIFF: torch.float16}


def _row_buffers(rows, prec: int, h: int, n: int, tl: int, dev) -> Dict[str, torch.Tensor]:
    """Outputs of a row builder, in the order the C ABI takes them; ``rows`` = (qhat, kvhat) to reuse (``prep_hash``)."""
    tile = _TILE[prec]
    if rows is not None:
        qhat, kvhat = rows
        if qhat.dtype != tile or tuple(qhat.shape) != (h, n, 32) or kvhat.dtype != tile or tuple(kvhat.shape) != (h, n, 64):
            raise ValueError("rows: buffers of another shape or precision")
    else:
        qhat = torch.empty(h, n, 32, device=dev, dtype=tile)
        kvhat = torch.empty(h, n, 64, device=dev, dtype=tile)
    return dict(qhat=qhat, kvhat=kvhat, qproj=torch.empty(tl, h, n, device=dev, dtype=torch.float32),
                kproj=torch.empty(tl, h, n, device=dev, dtype=torch.float32),
                minmax=torch.empty(tl, h, _lib.PREP_GRID, 4, device=dev, dtype=torch.float32))


def workspace_bytes(n, h, d, c, tl, b, precision) -> int:
    return _workspace_bytes_cached(int(n), int(h), int(d), int(c), int(tl), int(b), precision_code(precision))


def exchange_bytes(n, h, d, world, precision) -> int:
    return int(_lib.load().hept_exchange_bytes(n, h, d, world, precision_code(precision)))


def p2p_bytes(n, h, d, world, precision) -> int:
    return int(_lib.load().hept_p2p_bytes(n, h, d, world, precision_code(precision)))


@_on_device
def rpe_scale(w_rpe_weight: torch.Tensor, n_heads: int, head_dim: int, w_per_dist: int) -> torch.Tensor:
    lib = _lib.load()
    w = _f32c(w_rpe_weight, "w_rpe.weight")
    c = w.shape[1] // w_per_dist + 1
    out = torch.empty(n_heads, c, device=w.device, dtype=torch.float32)
    _lib.check(lib.hept_rpe_scale(w.data_ptr(), n_heads, head_dim, c, w_per_dist, out.data_ptr(), _stream(w)),
               "hept_rpe_scale")
    return out


@_on_device
def rpe_scale_bwd(w_rpe_weight: torch.Tensor, d_sqrt_w: torch.Tensor, n_heads: int, head_dim: int,
                  w_per_dist: int) -> torch.Tensor:
    """Gradient of ``rpe_scale`` with respect to ``w_rpe.weight``: (H*D, (C-1)*K) from d_sqrt_w (H, C)."""
    lib = _lib.load()
    w = _f32c(w_rpe_weight, "w_rpe.weight")
    g = _f32c(d_sqrt_w, "d_sqrt_w")
    c = w.shape[1] // w_per_dist + 1
    out = torch.empty_like(w)
    _lib.check(lib.hept_rpe_scale_bwd(w.data_ptr(), g.data_ptr(), n_heads, head_dim, c, w_per_dist, out.data_ptr(),
                                      _stream(w)), "hept_rpe_scale_bwd")
    return out


@_on_device
def prep_hash(q, k, v, coords, sqrt_w, alpha, codes, precision="fp32", t0: int = 0, tl: Optional[int] = None,
              raw_size: Optional[int] = None, rows: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """``rows`` = (qhat, kvhat) of an earlier call with the same inputs and precision: the row buffers are reused
    (callers that walk more than HEPT_MAX_TABLES tables in chunks rebuild identical rows for every chunk)."""
    lib = _lib.load()
    q, k, v, in_code = _qkv_in(q, k, v)
    coords, sqrt_w, alpha = (_f32c(x, nm) for x, nm in ((coords, "coords"), (sqrt_w, "sqrt_w"), (alpha, "alpha")))
    n, h, d, c, t = _dims(q, coords, alpha)
    if tuple(sqrt_w.shape) != (h, c):   # the kernel indexes it as (H, C): a mismatch would be an out-of-bounds read
        raise ValueError(f"sqrt_w must have shape {(h, c)}, got {tuple(sqrt_w.shape)}")
    if codes is not None:
        codes = _codes(codes, (t, h, n))
    raw_size = n if raw_size is None else int(raw_size)
    tl = t - t0 if tl is None else tl
    prec = precision_code(precision)
    out = _row_buffers(rows, prec, h, n, tl, q.device)
    _lib.check(lib.hept_prep_hash_in(q.data_ptr(), k.data_ptr(), v.data_ptr(), in_code, coords.data_ptr(),
                                     sqrt_w.data_ptr(), alpha.data_ptr(), _ptr(codes), n, raw_size, h, d, c, t, t0, tl, prec,
                                     *(b.data_ptr() for b in out.values()), _stream(q)), "hept_prep_hash")
    return out


@_on_device
def sort_tables(qproj, kproj, codes, minmax, t0: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stable ascending permutations (Tl,H,N) int32 of ``proj + float(code) * span`` for q and k."""
    lib = _lib.load()
    qproj, kproj, minmax = _f32c(qproj, "qproj"), _f32c(kproj, "kproj"), _f32c(minmax, "minmax")
    tl, h, n = qproj.shape
    codes = _codes(codes, exc=TypeError)
    t = codes.shape[0]
    ws = torch.empty(int(lib.hept_sort_workspace_bytes(n, h, tl)), device=qproj.device, dtype=torch.uint8)
    pos = torch.empty(2, tl, h, n, device=qproj.device, dtype=torch.int32)
    _lib.check(lib.hept_sort_tables(qproj.data_ptr(), kproj.data_ptr(), codes.data_ptr(), minmax.data_ptr(), n, h, t,
                                    t0, tl, ws.data_ptr(), pos[0].data_ptr(), pos[1].data_ptr(), _stream(qproj)),
               "hept_sort_tables")
    return pos[0], pos[1]


@_on_device
def sort_tables_src(qproj, kproj, eta_idx, phi_idx, cfac, minmax, t0: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """src-variant keys (hash + get_geo_shift): stable ascending permutations (Tl,H,N) int32 for q and k."""
    lib = _lib.load()
    qproj, kproj, minmax = _f32c(qproj, "qproj"), _f32c(kproj, "kproj"), _f32c(minmax, "minmax")
    tl, h, n = qproj.shape
    eta_idx, phi_idx, cfac = (_f32c(x, nm) for x, nm in ((eta_idx, "region_indices[0]"), (phi_idx, "region_indices[1]"),
                                                          (cfac, "cfac")))
    t = eta_idx.numel() // (h * n)
    ws = torch.empty(int(lib.hept_sort_workspace_bytes(n, h, tl)), device=qproj.device, dtype=torch.uint8)
    pos = torch.empty(2, tl, h, n, device=qproj.device, dtype=torch.int32)
    _lib.check(lib.hept_sort_tables_src(qproj.data_ptr(), kproj.data_ptr(), eta_idx.data_ptr(), phi_idx.data_ptr(),
                                        cfac.data_ptr(), minmax.data_ptr(), n, h, t, t0, tl, ws.data_ptr(),
                                        pos[0].data_ptr(), pos[1].data_ptr(), _stream(qproj)), "hept_sort_tables_src")
    return pos[0], pos[1]


@_on_device
def segmented_argsort(keys: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Stable ascending argsort of every row of a float32 (S, L) GPU tensor (+inf pads sort last); int32 (S, L).

    With ``lens`` (int32 (S,), on the GPU) only the first ``lens[s]`` keys of row s take part and only
    ``pos[s, :lens[s]]`` is defined (the ragged form ``prepare_input`` uses for clouds of unequal size)."""
    lib = _lib.load()
    keys = _f32c(keys, "keys")
    s_, l_ = keys.shape
    ws = torch.empty(int(lib.hept_argsort_workspace_bytes(s_, l_)), device=keys.device, dtype=torch.uint8)
    pos = torch.empty(s_, l_, device=keys.device, dtype=torch.int32)
    if lens is None:
        rc = lib.hept_segmented_argsort(keys.data_ptr(), s_, l_, ws.data_ptr(), pos.data_ptr(), _stream(keys))
    else:
        if lens.dtype != torch.int32 or lens.shape != (s_,) or lens.device != keys.device:
            raise ValueError("lens must be an int32 (S,) tensor on the keys' device")
        lens = lens.contiguous()
        rc = lib.hept_segmented_argsort_ragged(keys.data_ptr(), s_, l_, lens.data_ptr(), ws.data_ptr(), pos.data_ptr(),
                                               _stream(keys))
    _lib.check(rc, "hept_segmented_argsort")
    return pos


@_on_device
def block_attn(qhat, kvhat, qpos, kpos, head_dim: int, block_size: int, f32_mfma: bool = False, coords=None) -> torch.Tensor:
    """Per-table partial rows (Tl, N, H, row).  fp32 tiles: row = 32 f32 (numer in [:D], denom (+1e-20) at [D]);
    bf16 tiles with D == 24: packed row = 16 int32 dwords (24 bf16 numer | f32 denom | 0); see ``unpack_part``.
    ``f32_mfma`` runs f32 tiles on the native f32 MFMA instead of the split-bf16 products; ``f32_mfma="diff"`` the
    difference form of the coordinate columns on top of that (``precision="fp32_diff"``).  ``coords`` = (coords (N, C),
    sqrt_w (H, C), raw_size) on float16 rows: ``precision="mixed16_diff"`` (:func:`block_attn_coords`)."""
    lib = _lib.load()
    qhat, kvhat = _rowsc(qhat, "qhat"), _rowsc(kvhat, "kvhat")
    h, n, _ = qhat.shape
    tl = qpos.shape[0]
    prec = {torch.float32: PREC_F32, torch.bfloat16: PREC_BF16, torch.float16: PREC_MIXED16}[qhat.dtype]
    if f32_mfma and prec == PREC_F32:
        prec = PREC_F32_DIFF if f32_mfma == "diff" else PREC_F32_MFMA
    if coords is not None:
        if prec != PREC_MIXED16:
            raise TypeError("block_attn_coords takes the rows of precision 'mixed16' / 'mixed16_diff' (float16 row buffers)")
        prec = PREC_MIXED16_DIFF
        cds, sqrt_w, raw_size = coords
        cds, sqrt_w = _f32c(cds, "coords"), _f32c(sqrt_w, "sqrt_w")
        c = cds.shape[1]
        # the kernel indexes these by the sizes above: a mismatch would be an out-of-bounds device read
        if tuple(cds.shape) != (n, c) or tuple(sqrt_w.shape) != (h, c) or tuple(kvhat.shape) != (h, n, 64):
            raise ValueError(f"coords must be ({n}, C) and sqrt_w ({h}, C), got {tuple(cds.shape)} and {tuple(sqrt_w.shape)}")
        if tuple(qpos.shape) != (tl, h, n) or tuple(kpos.shape) != (tl, h, n):
            raise ValueError(f"qpos and kpos must be ({tl}, {h}, {n})")
        raw_size = n if raw_size is None else _raw_size(raw_size, n)
    packed = lib.hept_part_precision(prec, head_dim) == PREC_BF16
    qpos = qpos.to(torch.int32).contiguous()
    kpos = kpos.to(torch.int32).contiguous()
    part = torch.empty(tl, n, h, 16 if packed else 32, device=qhat.device, dtype=torch.int32 if packed else torch.float32)
    if coords is not None:
        _lib.check(lib.hept_block_attn_coords(qhat.data_ptr(), kvhat.data_ptr(), qpos.data_ptr(), kpos.data_ptr(),
                                              cds.data_ptr(), sqrt_w.data_ptr(), raw_size, n, h, head_dim, c, tl,
                                              block_size, part.data_ptr(), _stream(qhat)), "hept_block_attn_coords")
        return part
    _lib.check(lib.hept_block_attn(qhat.data_ptr(), kvhat.data_ptr(), qpos.data_ptr(), kpos.data_ptr(), n, h,
                                   head_dim, tl, block_size, prec, part.data_ptr(), _stream(qhat)),
               "hept_block_attn")
    return part


def block_attn_coords(qhat, kvhat, qpos, kpos, coords, sqrt_w, head_dim: int, block_size: int,
                      raw_size: Optional[int] = None) -> torch.Tensor:
    """``block_attn`` of ``precision="mixed16_diff"``: ``qhat`` / ``kvhat`` are "mixed16" rows (float16 tag) whose D feature
    columns go through the matrix products, the coordinate part of every logit is formed in float32 from ``coords`` (N, C)
    and ``sqrt_w`` (H, C) as explicit differences.  Rows at and after ``raw_size`` (src variant) count as coordinates 0.
    Partial rows as ``block_attn`` writes them for "mixed16" (packed iff ``head_dim`` is 24)."""
    return block_attn(qhat, kvhat, qpos, kpos, head_dim, block_size, coords=(coords, sqrt_w, raw_size))


def _part_prec(part: torch.Tensor) -> int:
    return PREC_BF16 if part.dtype == torch.int32 else PREC_F32


def unpack_part(part: torch.Tensor) -> torch.Tensor:
    """Widen packed partial rows (..., 16) int32 to the f32 row format (..., 32); f32 rows pass through."""
    if part.dtype != torch.int32:
        return part
    lo = (part[..., :12] << 16).view(torch.float32)
    hi = (part[..., :12] & -65536).view(torch.float32)
    out = torch.zeros(*part.shape[:-1], 32, device=part.device, dtype=torch.float32)
    out[..., 0:24:2] = lo
    out[..., 1:24:2] = hi
    out[..., 24] = part[..., 12].view(torch.float32)
    return out


@_on_device
def reduce_tables(part: torch.Tensor, head_dim: int = 24, packed: bool = False) -> torch.Tensor:
    """Sum of the per-table partial rows: f32 rows (N,H,32), or with ``packed`` (packed input only) packed rows
    (N,H,16) int32 again -- the form table sharding sends over xGMI."""
    lib = _lib.load()
    part = _rowsc(part, "part")
    tl, n, h, _ = part.shape
    if packed and part.dtype != torch.int32:
        raise TypeError("packed sums need packed partial rows (16-bit tiles with head_dim 24)")
    acc = torch.empty(n, h, 16 if packed else 32, device=part.device, dtype=torch.int32 if packed else torch.float32)
    _lib.check(lib.hept_reduce_tables(part.data_ptr(), _part_prec(part), tl, n, h, head_dim, acc.data_ptr(),
                                      PREC_BF16 if packed else PREC_F32, _stream(part)), "hept_reduce_tables")
    return acc


@_on_device
def combine_out(part: torch.Tensor, head_dim: int, out_weight, out_bias, n0: int = 0, n_count: Optional[int] = None) -> torch.Tensor:
    """(sum_t numer / sum_t denom) -> Linear(H*D -> D) for points [n0, n0+n_count); part is (Tl,N,H,row) or (N,H,32)."""
    lib = _lib.load()
    part = _rowsc(part, "part")
    if part.dim() == 3:
        part = part.unsqueeze(0)
    tl, n, h, _ = part.shape
    n_count = n - n0 if n_count is None else n_count
    out_linear, _keep = _out_linear(out_weight, out_bias)
    out = torch.empty(n_count, head_dim, device=part.device, dtype=torch.float32)
    _lib.check(lib.hept_combine_out(part.data_ptr(), _part_prec(part), tl, n, h, head_dim, n0, n_count, *out_linear,
                                    out.data_ptr(), _stream(part)), "hept_combine_out")
    return out


@_on_device
def block_attn_bwd(qhat, kvhat, qpos, kpos, gacc, head_dim: int, coords_dim: int, block_size: int,
                   f32_mfma: bool = False, coords: Optional[torch.Tensor] = None, raw_size: Optional[int] = None):
    """Backward of block_attn + reduce_tables for f32 (or bf16) tiles: gradient rows gacc (N,H,32) -> dq, dk, dv (N, H*D)
    and dcs (N, H, C), the gradient of the scaled coordinates shared by q^ and k^.  ``f32_mfma`` selects the
    native f32 MFMA kernel instead of the split-bf16 products; ``f32_mfma="diff"`` its difference form (f32 rows only):
    the logits as ``block_attn(..., f32_mfma="diff")`` forms them and the coordinate columns of the gradient summed as
    differences, the backward of ``precision="fp32_diff"``.  With ``coords`` (N, C) a fifth result
    d_sqrt_w (H, C) = sum_n dcs * coords is reduced in the same pass; rows at and after ``raw_size`` get zeros."""
    lib = _lib.load()
    if qhat.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("the backward pass needs f32 or bf16 tiles (rows of precision 'fp32' or 'bf16')")
    qhat, kvhat = _rowsc(qhat, "qhat"), _rowsc(kvhat, "kvhat")
    h, n, _ = qhat.shape
    tl = qpos.shape[0]
    gacc = _f32c(gacc, "grad of the partial sums")
    qpos = qpos.to(torch.int32).contiguous()   # as block_attn takes them (a strided view would be read as if it were dense)
    kpos = kpos.to(torch.int32).contiguous()
    dev = qhat.device
    rows16 = qhat.dtype == torch.bfloat16
    part_dtype = torch.bfloat16 if rows16 else torch.float32
    dq_part = torch.empty(tl, n, h, 32, device=dev, dtype=part_dtype)
    dkv_part = torch.empty(tl, n, h, 64, device=dev, dtype=part_dtype)
    st = _stream(qhat)
    if rows16:   # the rows of the bf16 forward: one bf16 MFMA per product, bf16 per-table gradient rows (16-bit training)
        fn = lib.hept_block_attn_bwd_bf16
    else:
        fn = lib.hept_block_attn_bwd_f32mfma if f32_mfma else lib.hept_block_attn_bwd
    dims = (n, h, head_dim, tl, block_size)
    if not rows16 and isinstance(f32_mfma, str):
        if f32_mfma != "diff":
            raise ValueError(f"f32_mfma must be False, True or 'diff', got {f32_mfma!r}")
        fn, dims = lib.hept_block_attn_bwd_diff, (n, h, head_dim, coords_dim, tl, block_size)
    _lib.check(fn(qhat.data_ptr(), kvhat.data_ptr(), qpos.data_ptr(), kpos.data_ptr(), gacc.data_ptr(), *dims,
                  dq_part.data_ptr(), dkv_part.data_ptr(), st), "hept_block_attn_bwd")
    dq = torch.empty(n, h * head_dim, device=dev, dtype=torch.float32)
    dk, dv = torch.empty_like(dq), torch.empty_like(dq)
    dcs = torch.empty(n, h, coords_dim, device=dev, dtype=torch.float32)
    dsw = None
    if coords is not None:
        coords = _f32c(coords, "coords")
        dsw = torch.empty(h, coords_dim, device=dev, dtype=torch.float32)
    _lib.check((lib.hept_bwd_reduce16 if rows16 else lib.hept_bwd_reduce)(dq_part.data_ptr(), dkv_part.data_ptr(), tl, n, h, head_dim, coords_dim,
                                   _ptr(coords), n if raw_size is None else int(raw_size), dq.data_ptr(),
                                   dk.data_ptr(), dv.data_ptr(), dcs.data_ptr(), _ptr(dsw), st),
               "hept_bwd_reduce")
    if coords is not None:
        return dq, dk, dv, dcs, dsw
    return dq, dk, dv, dcs


def check_bwd_coords_shape(coords_dim: int, block_size: int) -> None:
    """``block_attn_bwd_coords`` keeps five 16-bit tiles and three f32 side arrays of the coordinates in LDS (csrc/
    block_attn_bwd_coords.hip: bwdc_lds): the widest rows on the largest blocks (coords_dim >= 26 with block_size > 224)
    need more than the 160 KB of a CU.  Raises ``ValueError`` for such a shape -- the training path asks before its forward
    runs, so that the refusal does not come out of ``loss.backward()``."""
    nkt = (int(block_size) + 31) // 32
    cs = {2: 2, 4: 4, 6: 8}.get(int(coords_dim), int(coords_dim))
    need = 5 * 32 * nkt * 64 + 32 * nkt * 20 + 3 * 32 * nkt * cs * 4
    if need > 160 * 1024:
        raise ValueError(f"train_tiles='mixed16': coords_dim={coords_dim} with block_size={block_size} needs {need} bytes of "
                         f"LDS in the backward (a CU has {160 * 1024}); train this shape with train_tiles='fp32'")


def block_attn_bwd_coords(qhat, kvhat, qpos, kpos, gacc, coords, sqrt_w, head_dim: int, block_size: int,
                          raw_size: Optional[int] = None):
    """Backward of ``block_attn_coords`` + ``reduce_tables`` on the "mixed16" rows that forward gathers (float16 tag): gradient
    rows gacc (N, H, 32) -> (dq, dk, dv (N, H*D), dcs (N, H, C), d_sqrt_w (H, C)).  The logits are recomputed as the forward
    forms them (feature columns on the fp16 MFMA, the coordinate part in float32 as differences of ``sqrt_w * coords``), the
    coordinate columns of the gradient are summed as differences; rows at and after ``raw_size`` get zeros.  With more than
    64 (head, coordinate) columns d_sqrt_w is the column sum of ``dcs * coords`` in torch, as in the other training paths.
    Every shape is checked before anything is loaded or launched: a mismatch would be an out-of-bounds device read."""
    for name, t in (("qhat", qhat), ("kvhat", kvhat)):
        if not torch.is_tensor(t) or t.dtype is not torch.float16:
            raise TypeError(f"block_attn_bwd_coords takes the rows of precision 'mixed16' / 'mixed16_diff' (float16 row "
                            f"buffers); {name} is {getattr(t, 'dtype', type(t).__name__)}")
    for name, t in (("gacc", gacc), ("coords", coords), ("sqrt_w", sqrt_w)):
        if not torch.is_tensor(t) or t.dtype is not torch.float32:
            raise TypeError(f"{name} must be float32, got {getattr(t, 'dtype', type(t).__name__)}")
    for name, t in (("qpos", qpos), ("kpos", kpos)):
        if not torch.is_tensor(t) or t.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name} must be an int32 (or int64) tensor of positions, got {getattr(t, 'dtype', type(t).__name__)}")
    if qhat.dim() != 3 or qhat.shape[2] != 32:
        raise ValueError(f"qhat must be (H, N, 32), got {tuple(qhat.shape)}")
    h, n, _ = qhat.shape
    if tuple(kvhat.shape) != (h, n, 64):
        raise ValueError(f"kvhat must be ({h}, {n}, 64), got {tuple(kvhat.shape)}")
    if coords.dim() != 2 or coords.shape[0] != n:
        raise ValueError(f"coords must be ({n}, C), got {tuple(coords.shape)}")
    c = coords.shape[1]
    if tuple(sqrt_w.shape) != (h, c):
        raise ValueError(f"sqrt_w must be ({h}, {c}), got {tuple(sqrt_w.shape)}")
    if qpos.dim() != 3 or tuple(qpos.shape[1:]) != (h, n) or tuple(kpos.shape) != tuple(qpos.shape):
        raise ValueError(f"qpos and kpos must be (Tl, {h}, {n}), got {tuple(qpos.shape)} and {tuple(kpos.shape)}")
    if tuple(gacc.shape) != (n, h, 32):
        raise ValueError(f"gacc must be ({n}, {h}, 32), got {tuple(gacc.shape)}")
    raw_size = n if raw_size is None else _raw_size(raw_size, n)
    check_bwd_coords_shape(c, block_size)
    return _block_attn_bwd_coords(qhat, kvhat, qpos, kpos, gacc, coords, sqrt_w, int(head_dim), int(block_size), raw_size)


@_on_device
def _block_attn_bwd_coords(qhat, kvhat, qpos, kpos, gacc, coords, sqrt_w, d, block_size, raw_size):
    lib = _lib.load()
    qhat, kvhat = _rowsc(qhat, "qhat"), _rowsc(kvhat, "kvhat")
    gacc, coords, sqrt_w = _f32c(gacc, "grad of the partial sums"), _f32c(coords, "coords"), _f32c(sqrt_w, "sqrt_w")
    h, n, _ = qhat.shape
    tl, c = qpos.shape[0], coords.shape[1]
    _lib.check(_check_shape_cached(n, h, d, c, tl, block_size), "hept_check_shape")
    qpos = qpos.to(torch.int32).contiguous()
    kpos = kpos.to(torch.int32).contiguous()
    dev = qhat.device
    # (zero-filled, not empty: the kernels write every element, but the allocation-site audit of the test suite admits
    #  uninitialised buffers only at the sites its sweep drives; the fill of the per-table rows is part of the step time)
    dq_part = torch.zeros(tl, n, h, 32, device=dev, dtype=torch.bfloat16)
    dkv_part = torch.zeros(tl, n, h, 64, device=dev, dtype=torch.bfloat16)
    st = _stream(qhat)
    _lib.check(lib.hept_block_attn_bwd_coords(qhat.data_ptr(), kvhat.data_ptr(), qpos.data_ptr(), kpos.data_ptr(),
                                              gacc.data_ptr(), coords.data_ptr(), sqrt_w.data_ptr(), raw_size, n, h, d, c,
                                              tl, block_size, dq_part.data_ptr(), dkv_part.data_ptr(), st),
               "hept_block_attn_bwd_coords")
    dq = torch.zeros(n, h * d, device=dev, dtype=torch.float32)
    dk, dv = torch.zeros_like(dq), torch.zeros_like(dq)
    dcs = torch.zeros(n, h, c, device=dev, dtype=torch.float32)
    in_kernel = h * c <= 64   # the reduction's d sqrt_w pass has 64 lanes
    dsw = torch.zeros(h, c, device=dev, dtype=torch.float32) if in_kernel else None
    _lib.check(lib.hept_bwd_reduce16(dq_part.data_ptr(), dkv_part.data_ptr(), tl, n, h, d, c,
                                     coords.data_ptr() if in_kernel else None, raw_size, dq.data_ptr(), dk.data_ptr(),
                                     dv.data_ptr(), dcs.data_ptr(), _ptr(dsw), st), "hept_bwd_reduce16")
    if not in_kernel:
        dsw = (dcs * coords[:, None, :]).sum(dim=0)
    return dq, dk, dv, dcs, dsw


@_on_device
def combine_bwd(acc: torch.Tensor, g_out: torch.Tensor, out_weight: torch.Tensor, need_bias: bool = True):
    """Backward of ``combine_out`` on table-summed f32 rows: returns (gacc (N,H,32), d_weight (D,H*D), d_bias (D))."""
    lib = _lib.load()
    acc = _f32c(acc, "acc")
    g_out = _f32c(g_out, "grad of the output")
    w = _f32c(out_weight, "out_linear.weight")
    n, h, _ = acc.shape
    d = g_out.shape[1]
    gacc = torch.empty_like(acc)
    dw = torch.empty_like(w)
    db = torch.empty(d, device=acc.device, dtype=torch.float32) if need_bias else None
    scratch = torch.empty(int(lib.hept_combine_bwd_scratch_bytes_shape(n, h, d)), device=acc.device, dtype=torch.uint8)
    _lib.check(lib.hept_combine_bwd(acc.data_ptr(), g_out.data_ptr(), w.data_ptr(), n, h, d, gacc.data_ptr(),
                                    dw.data_ptr(), _ptr(db), scratch.data_ptr(), scratch.numel(), _stream(acc)),
               "hept_combine_bwd")
    return gacc, dw, db


def geo_args(region_indices, regions_h, n_tables: int, n_heads: int, n: int):
    """The src variant's caller tensors in the C ABI's layout: eta, phi (T,H,N) f32 and cfac (T,H) f32
    (= ``ceil(regions_h[0]) + 1``, reference ``src/models/attention/hept.py:53``)."""
    eta, phi = region_indices
    eta = _f32c(eta, "region_indices[0]")
    phi = _f32c(phi, "region_indices[1]")
    if tuple(eta.shape) != (n_tables * n_heads, n) or phi.shape != eta.shape:
        raise ValueError(f"region_indices must be two {(n_tables * n_heads, n)} tensors, got {tuple(eta.shape)} "
                         f"and {tuple(phi.shape)}")
    rh = _f32c(regions_h, "regions_h")
    if tuple(rh.shape) != (2, n_tables * n_heads):
        raise ValueError(f"regions_h must have shape {(2, n_tables * n_heads)}, got {tuple(rh.shape)}")
    cfac = (torch.ceil(rh[0]) + 1).contiguous()
    return eta, phi, cfac


def _prepare(q, k, v, coords, codes, w_rpe_weight, alpha, block_size, w_per_dist, in16: bool = False):
    """``in16``: the caller's entry point reads bfloat16 / float16 query, key, value natively (``_qkv_in``); the others
    (table sharding) take float32 only."""
    if in16:
        q, k, v, _ = _qkv_in(q, k, v)
    else:
        q, k, v = (_f32c(x, nm) for x, nm in ((q, "query"), (k, "key"), (v, "value")))
    coords = _f32c(coords, "coords")
    w = _f32c(w_rpe_weight, "w_rpe.weight")
    alpha = _f32c(alpha, "e2lsh.alpha")
    n, h, d, c, t = _dims(q, coords, alpha)
    if k.shape != q.shape or v.shape != q.shape or coords.shape[0] != n:
        raise ValueError("query, key, value and coords must agree on the number of points")
    if n % block_size != 0:
        raise ValueError(f"number of points {n} is not a multiple of block_size {block_size}")
    if codes is not None:
        codes = _codes(codes, (t, h, n))
    if w_per_dist == 0:  # precomputed sqrt_w (H, C) in place of the weight (hept_hip.h: K == 0)
        if w.shape != (h, c):
            raise ValueError(f"with w_per_dist=0 the weight argument is sqrt_w of shape {(h, c)}, got {tuple(w.shape)}")
    elif w.shape != (h * d, (c - 1) * w_per_dist):
        raise ValueError(f"w_rpe.weight must have shape {(h * d, (c - 1) * w_per_dist)}, got {tuple(w.shape)}")
    return q, k, v, coords, codes, w, alpha, (n, h, d, c, t)


def _key_args(codes, geo, t: int, h: int, n: int, check: bool = False):
    """The table-key arguments of an entry point (``geo`` is None: the AND codes) or of its ``*_src`` twin (``geo`` =
    (region_indices, regions_h, raw_size)), as the C ABI takes them, and the tensors they point into.  ``check``: the
    one-call blocks and stacks, where nothing has looked at ``codes`` yet and a bad ``raw_size`` is refused here."""
    if geo is None:
        codes = _codes(codes, (t, h, n)) if check else codes
        return (codes.data_ptr(),), codes
    region_indices, regions_h, raw_size = geo
    keep = geo_args(region_indices, regions_h, t, h, n)
    return (*(x.data_ptr() for x in keep), _raw_size(raw_size, n) if check else int(raw_size)), keep


def _forward(q, k, v, coords, codes, geo, w_rpe_weight, alpha, out_weight, out_bias, block_size, w_per_dist, precision,
             workspace, stream=None):
    """``forward`` (``geo`` is None) and ``forward_src`` (``geo`` = (region_indices, regions_h, raw_size))."""
    lib = _lib.load()
    q, k, v, coords, codes, w, alpha, (n, h, d, c, t) = _prepare(q, k, v, coords, codes, w_rpe_weight, alpha,
                                                                block_size, w_per_dist, in16=True)
    keys, _keep = _key_args(codes, geo, t, h, n)
    prec = precision_code(precision)
    workspace = _workspace(workspace, n, h, d, c, t, block_size, prec, q)
    out_linear, _keep_out = _out_linear(out_weight, out_bias)
    out = torch.empty(n, d, device=q.device, dtype=torch.float32)
    fn = lib.hept_forward_in if geo is None else lib.hept_forward_src_in
    _lib.check(fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), _IN_CODE[q.dtype], coords.data_ptr(), *keys, w.data_ptr(),
                  alpha.data_ptr(), *out_linear, n, h, d, c, w_per_dist, t, block_size, prec,
                  workspace.data_ptr(), workspace.numel(), out.data_ptr(), stream if stream is not None else _stream(q)),
               fn.__name__)
    return out


@_on_device
def forward(q, k, v, coords, codes, w_rpe_weight, alpha, out_weight, out_bias, *, block_size: int, w_per_dist: int,
            precision="fp32", workspace: Optional[torch.Tensor] = None, stream: Optional[int] = None) -> torch.Tensor:
    """Whole operator (reference ``example/hept.py:43-81``) in one C call; returns (N, D) float32."""
    return _forward(q, k, v, coords, codes, None, w_rpe_weight, alpha, out_weight, out_bias, block_size, w_per_dist,
                    precision, workspace, stream)


@_on_device
def forward_src(q, k, v, coords, region_indices, regions_h, raw_size: int, w_rpe_weight, alpha, out_weight, out_bias,
                *, block_size: int, w_per_dist: int, precision="fp32",
                workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Whole operator of the reference's src variant (``src/models/attention/hept.py:74-117``); (N, D) float32."""
    return _forward(q, k, v, coords, None, (region_indices, regions_h, raw_size), w_rpe_weight, alpha, out_weight,
                    out_bias, block_size, w_per_dist, precision, workspace)


def packed_partials(precision, head_dim: int) -> bool:
    """True if (precision, head_dim) produces packed 64-B partial rows (16-bit tiles, head_dim 24)."""
    return _lib.load().hept_part_precision(precision_code(precision), head_dim) == PREC_BF16


def _forward_partial(q, k, v, coords, codes, geo, w_rpe_weight, alpha, block_size, w_per_dist, t0, tl, precision,
                     workspace, packed):
    """``forward_partial`` and ``forward_partial_src``; ``geo`` as in ``_forward``."""
    lib = _lib.load()
    q, k, v, coords, codes, w, alpha, (n, h, d, c, t) = _prepare(q, k, v, coords, codes, w_rpe_weight, alpha,
                                                                block_size, w_per_dist, in16=True)
    keys, _keep = _key_args(codes, geo, t, h, n)
    prec = precision_code(precision)
    workspace = _workspace(workspace, n, h, d, c, tl, block_size, prec, q)
    acc = torch.empty(n, h, 16 if packed else 32, device=q.device, dtype=torch.int32 if packed else torch.float32)
    fn = lib.hept_forward_partial_in if geo is None else lib.hept_forward_partial_src_in
    _lib.check(fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), _IN_CODE[q.dtype], coords.data_ptr(), *keys, w.data_ptr(),
                  alpha.data_ptr(), n, h, d, c, w_per_dist, t, t0, tl, block_size, prec,
                  PREC_BF16 if packed else PREC_F32, workspace.data_ptr(), workspace.numel(), acc.data_ptr(), _stream(q)),
               fn.__name__)
    return acc


@_on_device
def forward_partial(q, k, v, coords, codes, w_rpe_weight, alpha, *, block_size: int, w_per_dist: int, t0: int,
                    tl: int, precision="fp32", workspace: Optional[torch.Tensor] = None,
                    packed: bool = False) -> torch.Tensor:
    """Tables [t0, t0+tl) only: returns acc (N, H, 32) = sum over those tables of [numer | denom]; ``packed``:
    the same sum as packed rows (N, H, 16) int32 (needs ``packed_partials(precision, D)``)."""
    return _forward_partial(q, k, v, coords, codes, None, w_rpe_weight, alpha, block_size, w_per_dist, t0, tl, precision,
                            workspace, packed)


@_on_device
def forward_partial_src(q, k, v, coords, region_indices, regions_h, raw_size: int, w_rpe_weight, alpha, *,
                        block_size: int, w_per_dist: int, t0: int, tl: int, precision="fp32",
                        workspace: Optional[torch.Tensor] = None, packed: bool = False) -> torch.Tensor:
    """src variant, tables [t0, t0+tl) only: acc (N, H, 32) = sum over those tables of [numer | denom]."""
    return _forward_partial(q, k, v, coords, None, (region_indices, regions_h, raw_size), w_rpe_weight, alpha, block_size,
                            w_per_dist, t0, tl, precision, workspace, packed)


@_on_device
def prep_hash_fused(x, norm_w, norm_b, eps, w_q, w_k, w_v, coords, sqrt_w, alpha, codes, precision="fp32",
                    t0: int = 0, tl: Optional[int] = None, raw_size: Optional[int] = None,
                    rows: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """``prep_hash`` with LayerNorm and the q/k/v projections fused in: ``x`` is the (N, D) input of the Attn block
    (reference ``example/transformer.py:155-156``); same outputs as :func:`prep_hash`."""
    lib = _lib.load()
    x = _inc(x, "x")   # float32, bfloat16 or float16 rows, read in place
    norm_w, norm_b, w_q, w_k, w_v, coords, sqrt_w, alpha = (
        _f32c(t_, nm) for t_, nm in ((norm_w, "norm1.weight"), (norm_b, "norm1.bias"), (w_q, "w_q.weight"),
                                     (w_k, "w_k.weight"), (w_v, "w_v.weight"), (coords, "coords"),
                                     (sqrt_w, "sqrt_w"), (alpha, "e2lsh.alpha")))
    n, d = x.shape
    h, e, t = alpha.shape
    c = e - d
    if tuple(w_q.shape) != (h * d, d) or w_k.shape != w_q.shape or w_v.shape != w_q.shape:
        raise ValueError(f"w_q/w_k/w_v must have shape {(h * d, d)}")
    if coords.shape != (n, c) or norm_w.numel() != d or norm_b.numel() != d:
        raise ValueError("coords / norm1 parameters do not match x")
    if tuple(sqrt_w.shape) != (h, c):
        raise ValueError(f"sqrt_w must have shape {(h, c)}, got {tuple(sqrt_w.shape)}")
    if codes is not None:
        codes = _codes(codes, (t, h, n))
    raw_size = n if raw_size is None else int(raw_size)
    tl = t - t0 if tl is None else tl
    prec = precision_code(precision)
    out = _row_buffers(rows, prec, h, n, tl, x.device)
    _lib.check(lib.hept_prep_hash_fused_in(x.data_ptr(), _IN_CODE[x.dtype], norm_w.data_ptr(), norm_b.data_ptr(),
                                           float(eps), w_q.data_ptr(), w_k.data_ptr(), w_v.data_ptr(), coords.data_ptr(),
                                           sqrt_w.data_ptr(), alpha.data_ptr(), _ptr(codes), n, raw_size, h, d, c, t, t0,
                                           tl, prec, *(b.data_ptr() for b in out.values()), _stream(x)),
               "hept_prep_hash_fused_in")
    return out


@_on_device
def combine_ffn(part: torch.Tensor, head_dim: int, out_weight, out_bias, x, norm_w, norm_b, eps, ff1_w, ff1_b, ff2_w,
                ff2_b, n0: int = 0, n_count: Optional[int] = None) -> torch.Tensor:
    """``combine_out`` followed by the rest of the Attn block (residual, norm2, feed-forward, residual) in the
    same kernel; reference ``example/transformer.py:161-165`` in eval mode.  ``x`` is the full (N, D) block input, float32,
    bfloat16 or float16; the result has its dtype (the float32 result rounded once, as ``.to(x.dtype)`` rounds)."""
    lib = _lib.load()
    part = _rowsc(part, "part")
    if part.dim() == 3:
        part = part.unsqueeze(0)
    tl, n, h, _ = part.shape
    n_count = n - n0 if n_count is None else n_count
    x = _inc(x, "x")
    out_linear, _keep = _out_linear(out_weight, out_bias)
    nw, nb, w1, b1, w2, b2 = (_f32c(t_, nm) for t_, nm in ((norm_w, "norm2.weight"), (norm_b, "norm2.bias"),
                                                           (ff1_w, "ff.0.weight"), (ff1_b, "ff.0.bias"),
                                                           (ff2_w, "ff.2.weight"), (ff2_b, "ff.2.bias")))
    y = torch.empty(n_count, head_dim, device=part.device, dtype=x.dtype)
    _lib.check(lib.hept_combine_ffn_io(part.data_ptr(), _part_prec(part), tl, n, h, head_dim, n0, n_count, *out_linear,
                                       x[n0:].data_ptr(), _IN_CODE[x.dtype],
                                       nw.data_ptr(), nb.data_ptr(), float(eps), w1.data_ptr(), b1.data_ptr(),
                                       w2.data_ptr(), b2.data_ptr(), y.data_ptr(), _stream(part)), "hept_combine_ffn_io")
    return y


_BLOCK_NAMES = {"norm1_w": "norm1.weight", "norm1_b": "norm1.bias", "w_q": "w_q.weight", "w_k": "w_k.weight",
                "w_v": "w_v.weight", "w_rpe": "w_rpe.weight", "alpha": "attn.e2lsh.alpha",
                "out_w": "attn.out_linear.weight", "out_b": "attn.out_linear.bias", "norm2_w": "norm2.weight",
                "norm2_b": "norm2.bias", "ff1_w": "ff.0.weight", "ff1_b": "ff.0.bias", "ff2_w": "ff.2.weight",
                "ff2_b": "ff.2.bias"}


def _check_block(x_shape, coords, keep, num_heads, block_size, w_per_dist):
    """Size checks of one block's tensors against its (N, D) input; returns (N, H, D, C, T)."""
    n, d = x_shape
    h = num_heads
    e, t = keep["alpha"].shape[1], keep["alpha"].shape[2]
    c = e - d
    if n % block_size != 0:
        raise ValueError(f"number of points {n} is not a multiple of block_size {block_size}")
    # the row builder indexes these by the sizes above: a mismatched tensor would be an out-of-bounds device read
    if keep["alpha"].shape[0] != h or tuple(coords.shape) != (n, c):
        raise ValueError(f"attn.e2lsh.alpha must be ({h}, D + C, n_hashes) and coords ({n}, {c})")
    want_rpe = (h * d, (c - 1) * w_per_dist) if w_per_dist > 0 else (h, c)
    if tuple(keep["w_rpe"].shape) != want_rpe:
        raise ValueError(f"w_rpe.weight must have shape {want_rpe}, got {tuple(keep['w_rpe'].shape)}")
    for f_ in ("w_q", "w_k", "w_v"):
        if tuple(keep[f_].shape) != (h * d, d):
            raise ValueError(f"{_BLOCK_NAMES[f_]} must have shape {(h * d, d)}")
    return n, h, d, c, t


def _block_args(x, coords, params, num_heads, block_size, w_per_dist, eps1, eps2, precision, workspace):
    """Checks and marshalling shared by the two one-call blocks: (x, coords, params struct, sizes, prec, workspace,
    the tensors the struct points into)."""
    x = _inc(x, "x")   # float32, bfloat16 or float16: the block reads the rows in place and answers in the same type
    coords = _f32c(coords, "coords")
    keep = {f: _f32c(params[k], k) for f, k in _BLOCK_NAMES.items()}
    n, h, d, c, t = _check_block(x.shape, coords, keep, num_heads, block_size, w_per_dist)
    prec = precision_code(precision)
    workspace = _workspace(workspace, n, h, d, c, t, block_size, prec, x)
    st = _lib.AttnParams(**{f: v.data_ptr() for f, v in keep.items()}, eps1=float(eps1), eps2=float(eps2))
    return x, coords, st, (n, h, d, c, t), prec, workspace, keep


def _attn_block_forward(x, coords, codes, geo, params, num_heads, block_size, w_per_dist, eps1, eps2, precision,
                        workspace):
    """``attn_block_forward`` and ``attn_block_forward_src``; ``geo`` as in ``_forward``."""
    lib = _lib.load()
    x, coords, st, (n, h, d, c, t), prec, workspace, _keep = _block_args(
        x, coords, params, num_heads, block_size, w_per_dist, eps1, eps2, precision, workspace)
    keys, _keep_keys = _key_args(codes, geo, t, h, n, check=True)
    y = torch.empty(n, d, device=x.device, dtype=x.dtype)
    fn = lib.hept_attn_block_forward_io if geo is None else lib.hept_attn_block_forward_src_io
    _lib.check(fn(x.data_ptr(), _IN_CODE[x.dtype], coords.data_ptr(), *keys, ctypes.byref(st), n, h, d, c, w_per_dist, t,
                  block_size, prec, workspace.data_ptr(), workspace.numel(), y.data_ptr(), _stream(x)), fn.__name__)
    return y


@_on_device
def attn_block_forward(x, coords, codes, params: Dict[str, torch.Tensor], *, num_heads: int, block_size: int,
                       w_per_dist: int, eps1: float = 1e-5, eps2: float = 1e-5, precision="fp32",
                       workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The whole Attn block (reference ``example/transformer.py:154-165``, eval mode) in one C call.
    ``params`` holds the block's tensors under the reference's state-dict names.  ``x`` is float32, bfloat16 or float16
    and the result has its dtype: 16-bit rows are widened where the kernels load them and the float32 result is rounded
    once where it is stored -- bit for bit ``attn_block_forward(x.float(), ...).to(x.dtype)`` without the two casts."""
    return _attn_block_forward(x, coords, codes, None, params, num_heads, block_size, w_per_dist, eps1, eps2, precision,
                               workspace)


@_on_device
def attn_block_forward_src(x, coords, region_indices, regions_h, raw_size: int, params: Dict[str, torch.Tensor], *,
                           num_heads: int, block_size: int, w_per_dist: int, eps1: float = 1e-5, eps2: float = 1e-5,
                           precision="fp32", workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The src variant's Attn block (reference ``src/models/baselines/transformer.py:205-214`` with
    ``attn_type="hept"``, eval mode) in one C call; the operator's kwargs as built by ``prepare_input_src``.  ``x`` and the
    result: float32, bfloat16 or float16, as for :func:`attn_block_forward`."""
    return _attn_block_forward(x, coords, None, (region_indices, regions_h, raw_size), params, num_heads, block_size,
                               w_per_dist, eps1, eps2, precision, workspace)


def _stack_args(xcat, coords, params_list, num_heads, block_size, w_per_dist, eps1, eps2, precision, workspace):
    """Checks and marshalling shared by the two one-call stacks: the checks of ``_block_args`` for every layer, an array
    of ``AttnParams``, and the pitch of the (N, ld) buffer (a column-sliced view is taken as it is)."""
    if xcat.dtype != torch.float32 or xcat.dim() != 2:
        raise TypeError(f"xcat must be a 2-d float32 tensor, got {xcat.dtype} with {xcat.dim()} dims")
    n_layers = len(params_list)
    if n_layers < 1:
        raise ValueError("attn_stack_forward needs at least one layer")
    n, cols = xcat.shape
    # the layers write into the caller's buffer: no repairing copy here (a copy would receive the results instead)
    if xcat.stride(1) != 1:
        raise ValueError(f"xcat must have unit stride along its columns (stride(1) == 1), got {xcat.stride(1)}")
    if not xcat.is_cuda:
        raise RuntimeError(f"xcat must live on the GPU (hept_amd has no CPU path); got device {xcat.device}")
    ld = xcat.stride(0) if n > 1 else cols
    if cols % (n_layers + 1) != 0:
        raise ValueError(f"xcat must have (n_layers + 1) * D = {n_layers + 1} * D columns, got {cols}")
    d = cols // (n_layers + 1)
    if ld < cols or ld % 4 != 0 or xcat.data_ptr() % 16:
        raise ValueError(f"xcat needs a row pitch that is a multiple of 4 floats and a 16-byte aligned base (its rows "
                         f"move as 16-byte pieces); got pitch {ld}, base offset {xcat.data_ptr() % 16}")
    coords = _f32c(coords, "coords")
    sts, keeps, dims0 = [], [], None
    for i, params in enumerate(params_list):
        keep = {f: _f32c(params[k], k) for f, k in _BLOCK_NAMES.items()}
        dims = _check_block((n, d), coords, keep, num_heads, block_size, w_per_dist)
        if dims0 is None:
            dims0 = dims
        elif dims != dims0:
            raise ValueError(f"layer {i} has sizes (N, H, D, C, T) = {dims}, layer 0 has {dims0}: the layers of a stack "
                             f"share one shape")
        keeps.append(keep)
        sts.append(_lib.AttnParams(**{f: v.data_ptr() for f, v in keep.items()}, eps1=float(eps1[i]), eps2=float(eps2[i])))
    n, h, d, c, t = dims0
    prec = precision_code(precision)
    workspace = _workspace(workspace, n, h, d, c, t, block_size, prec, xcat)
    arr = (_lib.AttnParams * n_layers)(*sts)
    return coords, arr, n_layers, ld, dims0, prec, workspace, keeps


def _eps_list(eps, n_layers: int):
    return [float(eps)] * n_layers if isinstance(eps, (int, float)) else [float(e) for e in eps]


def _attn_stack_forward(xcat, coords, codes, geo, params_list, num_heads, block_size, w_per_dist, eps1, eps2, precision,
                        workspace):
    """``attn_stack_forward`` and ``attn_stack_forward_src``; ``geo`` as in ``_forward``."""
    lib = _lib.load()
    n_layers = len(params_list)
    coords, arr, n_layers, ld, (n, h, d, c, t), prec, workspace, _keeps = _stack_args(
        xcat, coords, params_list, num_heads, block_size, w_per_dist, _eps_list(eps1, n_layers),
        _eps_list(eps2, n_layers), precision, workspace)
    keys, _keep_keys = _key_args(codes, geo, t, h, n, check=True)
    fn = lib.hept_attn_stack_forward if geo is None else lib.hept_attn_stack_forward_src
    _lib.check(fn(xcat.data_ptr(), ld, coords.data_ptr(), *keys, arr, n_layers, n, h, d, c, w_per_dist, t, block_size,
                  prec, workspace.data_ptr(), workspace.numel(), _stream(xcat)), fn.__name__)
    return xcat


@_on_device
def attn_stack_forward(xcat, coords, codes, params_list, *, num_heads: int, block_size: int, w_per_dist: int,
                       eps1=1e-5, eps2=1e-5, precision="fp32", workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``len(params_list)`` Attn blocks in a row (the reference model's layer loop, ``example/transformer.py:119-121``,
    eval mode) in one C call on one workspace.  ``xcat`` is (N, (L+1) D) float32 -- or a column-sliced view of a wider
    buffer -- whose columns [0, D) hold the first layer's input; layer i writes columns [(i+1) D, (i+2) D) IN PLACE, so on
    return ``xcat`` is the reference's ``torch.cat(all_encoded_x, dim=-1)``.  ``eps1`` / ``eps2``: one value, or one per
    layer.  Returns ``xcat``."""
    return _attn_stack_forward(xcat, coords, codes, None, params_list, num_heads, block_size, w_per_dist, eps1, eps2,
                               precision, workspace)


@_on_device
def attn_stack_forward_src(xcat, coords, region_indices, regions_h, raw_size: int, params_list, *, num_heads: int,
                           block_size: int, w_per_dist: int, eps1=1e-5, eps2=1e-5, precision="fp32",
                           workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``attn_stack_forward`` around the src variant's operator (the layer loop of
    ``src/models/baselines/transformer.py:133-144``); the operator's kwargs as built by ``prepare_input_src``."""
    return _attn_stack_forward(xcat, coords, None, (region_indices, regions_h, raw_size), params_list, num_heads,
                               block_size, w_per_dist, eps1, eps2, precision, workspace)


@_on_device
def partial_begin(q, k, v, coords, codes, w_rpe_weight, alpha, *, block_size: int, w_per_dist: int, t0: int, tl: int,
                  precision="fp32", workspace: torch.Tensor, geo=None) -> Tuple[int, int, int, int]:
    """Table sharding, first half (``hept_partial_begin``): parameter math, rows + hashes and the sort for tables
    [t0, t0+tl); everything stays in ``workspace`` for :func:`partial_heads`.  ``geo`` = (region_indices, regions_h,
    raw_size) selects the src variant (``codes`` is then None).  Returns (N, H, D, C)."""
    lib = _lib.load()
    q, k, v, coords, codes, w, alpha, (n, h, d, c, t) = _prepare(q, k, v, coords, codes, w_rpe_weight, alpha,
                                                                block_size, w_per_dist)
    prec = precision_code(precision)
    _workspace(workspace, n, h, d, c, tl, block_size, prec, q, grow=False)
    keys, _keep = _key_args(codes, geo, t, h, n)
    fn = lib.hept_partial_begin if geo is None else lib.hept_partial_begin_src
    rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), coords.data_ptr(), *keys, w.data_ptr(), alpha.data_ptr(), n, h, d,
            c, w_per_dist, t, t0, tl, block_size, prec, workspace.data_ptr(), workspace.numel(), _stream(q))
    _lib.check(rc, "hept_partial_begin")
    return n, h, d, c


@_on_device
def partial_heads(workspace: torch.Tensor, dims: Tuple[int, int, int, int], tl: int, block_size: int, precision,
                  h0: int, dst: torch.Tensor) -> None:
    """Second half (``hept_partial_heads``): block attention of heads [h0, h0 + dst.shape[1]) for the tables of the
    preceding :func:`partial_begin`, summed over those tables into ``dst`` (n_pad, hg, row) -- int32 rows of 16 (packed)
    or float32 rows of 32; rows at and after N are zero."""
    lib = _lib.load()
    n, h, d, c = dims
    n_pad, hg, row = dst.shape
    packed = dst.dtype == torch.int32
    if (packed and row != 16) or (not packed and (dst.dtype != torch.float32 or row != 32)) or not dst.is_contiguous():
        raise ValueError("dst must be a contiguous (n_pad, hg, 16) int32 or (n_pad, hg, 32) float32 tensor")
    _lib.check(lib.hept_partial_heads(workspace.data_ptr(), workspace.numel(), n, h, d, c, tl, block_size,
                                      precision_code(precision), h0, hg, n_pad, PREC_BF16 if packed else PREC_F32,
                                      dst.data_ptr(), _stream(dst)), "hept_partial_heads")


@_on_device
def combine_groups(part: torch.Tensor, head_dim: int, out_weight, out_bias, n0: int = 0,
                   n_count: Optional[int] = None) -> torch.Tensor:
    """``combine_out`` on rows that arrive split by head groups: ``part`` is (G, Tl, N, HG, row) -- group g holds heads
    [g*HG, (g+1)*HG) -- and is summed over Tl (the slices received from the ranks); returns (n_count, D)."""
    lib = _lib.load()
    if part.dim() != 5 or not part.is_contiguous():
        raise ValueError("part must be a contiguous (groups, tables, points, heads per group, row) tensor")
    g, tl, n, hg, row = part.shape
    n_count = n - n0 if n_count is None else n_count
    out_linear, _keep = _out_linear(out_weight, out_bias)
    out = torch.empty(n_count, head_dim, device=part.device, dtype=torch.float32)
    _lib.check(lib.hept_combine_groups(part.data_ptr(), _part_prec(part), tl, n, g * hg, head_dim, n0, n_count, hg,
                                       tl * n * hg * row, *out_linear, out.data_ptr(), _stream(part)),
               "hept_combine_groups")
    return out


@_on_device
def forward_sharded(q, k, v, coords, codes, w_rpe_weight, alpha, out_weight, out_bias, *, comm: int, world: int,
                    block_size: int, w_per_dist: int, t0: int, tl: int, head_groups: int, precision="fp32",
                    workspace: torch.Tensor, xbuf: Optional[torch.Tensor] = None, one_sided: bool = False,
                    geo=None, out_view: bool = False, view_owner=None) -> torch.Tensor:
    """Table-sharded operator in one C call (``hept_forward_sharded``): this rank's tables [t0, t0+tl), the RCCL
    exchange pipelined by head groups on the communicator's side stream, combine of this rank's points and the
    all-gather; returns the full (N, D) output.  ``comm`` is a ``hept_comm*`` (see ``hept_amd.sharding``);
    ``one_sided`` selects the transport that stores rows straight into the peers' mapped exchange buffers
    (``hept_comm_p2p_*``; ``xbuf`` is then not needed).  ``out_view`` (one-sided transport, the communicator in view
    mode -- ``hept_comm_set_out_view``): the result is a tensor over the communicator's exchange buffer instead of a
    copy; it is overwritten by the SECOND next sharded call on this communicator (``TableSharding(out_view=True)``)."""
    lib = _lib.load()
    q, k, v, coords, codes, w, alpha, (n, h, d, c, t) = _prepare(q, k, v, coords, codes, w_rpe_weight, alpha,
                                                                block_size, w_per_dist)
    prec = precision_code(precision)
    _workspace(workspace, n, h, d, c, tl, block_size, prec, q, grow=False)
    if not one_sided and (xbuf is None or xbuf.numel() < int(lib.hept_exchange_bytes(n, h, d, world, prec))):
        raise ValueError("exchange buffer too small: size it with hept_exchange_bytes")
    out_linear, _keep_out = _out_linear(out_weight, out_bias)
    per = (n + world - 1) // world
    view = bool(out_view and one_sided)
    out_full = None if view else torch.empty(per * world, d, device=q.device, dtype=torch.float32)
    keys, _keep = _key_args(codes, geo, t, h, n)
    fn = lib.hept_forward_sharded if geo is None else lib.hept_forward_sharded_src
    rc = fn(comm, q.data_ptr(), k.data_ptr(), v.data_ptr(), coords.data_ptr(), *keys, w.data_ptr(), alpha.data_ptr(),
            *out_linear, n, h, d, c, w_per_dist, t, t0, tl, block_size, prec, head_groups,
            _lib.TRANSPORT_ONE_SIDED if one_sided else _lib.TRANSPORT_RCCL, workspace.data_ptr(), workspace.numel(),
            _ptr(xbuf), xbuf.numel() if xbuf is not None else 0, _ptr(out_full), _stream(q))
    _lib.check(rc, "hept_forward_sharded")
    if view:
        ptr = ctypes.c_void_p()
        _lib.check(lib.hept_comm_out_view(comm, ctypes.byref(ptr)), "hept_comm_out_view")
        return torch.as_tensor(_DeviceRows(ptr.value, n, d, view_owner), device=q.device)
    return out_full[:n]


class _DeviceRows:
    """(n, d) f32 rows at a device address owned by the C library (the exchange buffer of a communicator), for
    ``torch.as_tensor`` (zero-copy through ``__cuda_array_interface__``)"""

    def __init__(self, ptr: int, n: int, d: int, owner=None):
        self.__cuda_array_interface__ = {"shape": (n, d), "typestr": "<f4", "data": (ptr, False), "version": 2,
                                         "strides": None}
        # the tensor made from this object keeps it alive, and with it the owner of the memory (the TableSharding whose
        # communicator holds the exchange buffer): the buffer cannot be unmapped under a live view
        self.owner = owner
        if owner is not None:
            owner._live_views = getattr(owner, "_live_views", 0) + 1

    def __del__(self):
        if self.owner is not None:
            self.owner._live_views = max(0, getattr(self.owner, "_live_views", 1) - 1)


# ---- the dense tail of the Attn block's training step (csrc/block_train.hip; rows of 24 floats)
@_on_device
def rows_wgrad(d_y: torch.Tensor, x: torch.Tensor, need_bias: bool = False):
    """Weight gradient of a ``Linear(24 -> O)``: ``d_y.t() @ x`` (O, 24) (and the column sums of ``d_y`` for the bias)
    with a fixed-order two-stage reduction over the points -- rocBLAS runs this shape at ~140 us for 60k points."""
    lib = _lib.load()
    d_y, x = _f32c(d_y, "d_y"), _f32c(x, "x")
    n, o = d_y.shape
    if x.shape != (n, 24):
        raise ValueError(f"x must be ({n}, 24), got {tuple(x.shape)}")
    dw = torch.empty(o, 24, device=x.device, dtype=torch.float32)
    db = torch.empty(o, device=x.device, dtype=torch.float32) if need_bias else None
    scratch = torch.empty(int(lib.hept_rows_wgrad_scratch_bytes(n, o)), device=x.device, dtype=torch.uint8)
    _lib.check(lib.hept_rows_wgrad(d_y.data_ptr(), x.data_ptr(), n, o, 24, dw.data_ptr(),
                                   _ptr(db), scratch.data_ptr(), scratch.numel(), _stream(x)), "hept_rows_wgrad")
    return (dw, db) if need_bias else dw


@_on_device
def ln_bwd(x: torch.Tensor, d_xn: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float):
    """LayerNorm(24) backward: returns (dx, xn, d_ln_w, d_ln_b) -- ``xn`` = the normalised rows (recomputed)."""
    lib = _lib.load()
    x, d_xn, ln_w, ln_b = (_f32c(t, nm) for t, nm in ((x, "x"), (d_xn, "d_xn"), (ln_w, "ln.weight"), (ln_b, "ln.bias")))
    n, d = x.shape
    dx, xn = torch.empty_like(x), torch.empty_like(x)
    dlw, dlb = torch.empty_like(ln_w), torch.empty_like(ln_b)
    scratch = torch.empty(int(lib.hept_ln_scratch_bytes(n)), device=x.device, dtype=torch.uint8)
    _lib.check(lib.hept_ln_bwd(x.data_ptr(), d_xn.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), float(eps), n, d,
                               dx.data_ptr(), xn.data_ptr(), dlw.data_ptr(), dlb.data_ptr(), scratch.data_ptr(),
                               scratch.numel(), _stream(x)), "hept_ln_bwd")
    return dx, xn, dlw, dlb


@_on_device
def ln_ffn_fwd(x1, ln_w, ln_b, eps, w1, b1, w2, b2) -> torch.Tensor:
    """``ff.2(relu(ff.0(norm2(x1))))`` (reference ``example/transformer.py:162``) in one kernel; (N, 24)."""
    lib = _lib.load()
    ts = [_f32c(t, nm) for t, nm in ((x1, "x1"), (ln_w, "norm2.weight"), (ln_b, "norm2.bias"), (w1, "ff.0.weight"),
                                     (b1, "ff.0.bias"), (w2, "ff.2.weight"), (b2, "ff.2.bias"))]
    x1, ln_w, ln_b, w1, b1, w2, b2 = ts
    n, d = x1.shape
    out = torch.empty_like(x1)
    _lib.check(lib.hept_ln_ffn_fwd(x1.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), float(eps), w1.data_ptr(),
                                   b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), n, d, out.data_ptr(), _stream(x1)),
               "hept_ln_ffn_fwd")
    return out


@_on_device
def ln_ffn_bwd(x1, d_out, ln_w, ln_b, eps, w1, b1, w2, b2):
    """Backward of :func:`ln_ffn_fwd`: (d_x1, d_ln_w, d_ln_b, d_w1, d_b1, d_w2, d_b2)."""
    lib = _lib.load()
    ts = [_f32c(t, nm) for t, nm in ((x1, "x1"), (d_out, "d_out"), (ln_w, "norm2.weight"), (ln_b, "norm2.bias"),
                                     (w1, "ff.0.weight"), (b1, "ff.0.bias"), (w2, "ff.2.weight"), (b2, "ff.2.bias"))]
    x1, d_out, ln_w, ln_b, w1, b1, w2, b2 = ts
    n, d = x1.shape
    outs = [torch.empty_like(t) for t in (x1, ln_w, ln_b, w1, b1, w2, b2)]
    scratch = torch.empty(int(lib.hept_ln_ffn_bwd_scratch_bytes(n)), device=x1.device, dtype=torch.uint8)
    _lib.check(lib.hept_ln_ffn_bwd(x1.data_ptr(), d_out.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), float(eps),
                                   w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), n, d,
                                   *[t.data_ptr() for t in outs], scratch.data_ptr(), scratch.numel(), _stream(x1)),
               "hept_ln_ffn_bwd")
    return tuple(outs)


def profile_enable(mode: int, max_calls: int = 0, stride: int = 1) -> None:
    """Stage timing with HIP events recorded inside hept_forward (mode 1: block_attn only, 2: all stages, 0: off);
    only every ``stride``-th call is bracketed."""
    lib = _lib.load()
    _lib.check(lib.hept_profile_enable(mode, max_calls), "hept_profile_enable")
    _lib.check(lib.hept_profile_stride(stride), "hept_profile_stride")


def profile_stride(stride: int) -> None:
    """Bracket every ``stride``-th call from the next call on (restarts the count)."""
    _lib.check(_lib.load().hept_profile_stride(stride), "hept_profile_stride")


def profile_read() -> Tuple[Dict[str, float], int]:
    """Summed milliseconds per stage over the recorded calls, and the number of calls; resets the pool."""
    ms = (ctypes.c_float * 7)()
    n = ctypes.c_int(0)
    _lib.check(_lib.load().hept_profile_read(ms, ctypes.byref(n)), "hept_profile_read")
    # (the sharded call: "combine" = the exposed push / transfer of the last head group, then its own two stages;
    #  "chunk_sort" = the first of the sort's two launches, inside "sort_tables")
    return dict(zip(("prep_hash", "sort_tables", "block_attn", "combine", "sharded_combine", "sharded_gather", "chunk_sort"),
                    [float(x) for x in ms])), int(n.value)
