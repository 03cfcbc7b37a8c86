"""Scratch-contract sweep: no result of the HIP code may depend on what its scratch memory held before the call, no
kernel may store outside the buffer it was given, and no call may change its inputs (run by tests/test_gpu_scratch.py,
coverage pinned on CPU by tests/test_scratch_cells.py).  A plain module like the other sweeps; nothing here touches the
GPU at import time.

The float64 sweeps (shape_sweep, attn_sweep, src_attn_sweep, shard_sweep, dense_sweep) run the same shape back to back,
so the caching allocator hands every call a block that already holds the right rows, hashes, range partials and
permutations: a kernel that reads a word it was meant to rewrite finds the correct value there.  Here every case runs
once on untouched allocations (``clean``) and once under each pattern of ``PATTERNS`` with every ``torch.empty`` /
``empty_like`` / ``new_empty`` of the Python layer replaced by a guarded, pre-filled buffer (``scratch``); all
comparisons are bitwise.  The clean numbers themselves are held to float64 by the other sweeps: the cases are taken
from them by id and this module adds no second oracle.

``AUDIT`` is the read-through that came before the first GPU run: for every region of ``carve`` / ``carve_sort``
(csrc/capi.hip, csrc/sort_tables.hip), every buffer the Python layer allocates with ``empty`` and every scratch block
of the training kernels, the kernel that writes it first and the one that reads it first.  Finding: none -- every
region has a writer in front of its first reader on every dispatch path; the only device counters that start a store
address (the REGION sort's ``cnt`` / cursors, the ragged argsort's range words) are cleared by the row builder's
``zero_block``, by ``zero_words_kernel`` or by a fill on every path that reads them."""
import contextlib
import os
import sys
from collections import namedtuple

import torch

import attn_sweep as asw
import shape_sweep as sw
import shard_sweep as shw
import src_attn_sweep as ssw
from attn_sweep import D, EPS, H, K
from shape_sweep import MAX_TABLES, PRECISIONS, SMALL_CAP

# ---------------------------------------------------------------------------------------------------------------------
# 1. the audit (by reading; printed by tests/test_scratch_cells.py)
# ---------------------------------------------------------------------------------------------------------------------
# (region, first writer, file:line, first reader, file:line, note)
AUDIT = [
    # ---- carve(), csrc/capi.hip:28-50
    ("ws.qhat", "prep_role<ROLE 0> / prep_generic_kernel role 0 / fused row builder", "prep_hash.hip:425,772",
     "block_attn_kernel / block_attn_split_kernel", "block_attn.hip:73,386", "whole 32-column rows are stored, zeros beyond E"),
    ("ws.kvhat k half", "prep_role<ROLE 1> / prep_generic_kernel role 1", "prep_hash.hip:425,772",
     "block_attn kernels", "block_attn.hip:73,386", ""),
    ("ws.kvhat v half", "one of: row builder v role (roles == 3), rider workgroups of bucket_sort_kernel, nobody (direct v)",
     "capi.hip:214-226, sort_tables.hip:1247, rows_rider.h:73", "block_attn kernels; direct v: block_attn_split_kernel reads the caller's v",
     "block_attn.hip:386", "direct v: the v half keeps whatever the workspace held and must never be read (ff pattern = NaN)"),
    ("ws.qproj / ws.kproj", "row builder, q and k roles", "prep_hash.hip:744", "chunk_sort_kernel / small sort",
     "sort_tables.hip:218,1025", "padding rows of the src variant get +inf"),
    ("ws.minmax [Tc][H][PREP_GRID][4]", "row builder: own slot + the filler loop for the slots of workgroups not launched",
     "prep_hash.hip:466-468,792", "chunk_sort_kernel, small sort (read whole)", "sort_tables.hip:304,1028",
     "4th float stored as 0; src: src_bound_kernel rewrites slot 0 column 2 (sort_tables.hip:912) before KA reads it"),
    ("ws.pos", "bucket_sort_kernel / small sort, or the chunk copy of walk_tables", "capi.hip:172-184",
     "block_attn kernels", "block_attn.hip:73", ""),
    ("ws.pos_chunk", "bucket_sort_kernel / small sort of one chunk", "capi.hip:172", "hipMemcpyAsync of walk_tables",
     "capi.hip:181", "only with more than HEPT_MAX_TABLES tables"),
    ("ws.part", "block_attn kernels (every row of every table)", "block_attn.hip:832", "combine / reduce kernels",
     "combine.hip:131,573,612", ""),
    # ---- carve_sort(), csrc/sort_tables.hip:1197-1195
    ("sort.pa / rg.pool", "chunk_sort_kernel (runs; REGION: overflow pairs behind the cursor)", "sort_tables.hip:217",
     "bucket_sort_kernel", "sort_tables.hip:875", "read only below the counts KA published"),
    ("sort.pb", "bucket_sort_kernel (streaming scratch)", "sort_tables.hip:875", "bucket_sort_kernel", "sort_tables.hip:875", ""),
    ("sort.tab", "chunk_sort_kernel", "sort_tables.hip:217", "bucket_sort_kernel", "sort_tables.hip:875", ""),
    ("sort.range", "hipMemsetAsync 0xFF, then raw_range_kernel atomicMin", "sort_tables.hip:1387,950",
     "chunk_sort_kernel<MODE 2>", "sort_tables.hip:288", "segmented_argsort only; skipped with caller bounds"),
    ("sort.params", "chunk_sort_kernel, chunk 0", "sort_tables.hip:317", "bucket_sort_kernel", "sort_tables.hip:875", ""),
    ("sort.rg.cnt + cursors (zero block)", "zero_block of the row builder (3 call sites) or zero_words_kernel",
     "prep_hash.hip:137,514,558,682; sort_tables.hip:1252-1255", "chunk_sort_kernel atomicAdd", "sort_tables.hip:346,409",
     "size recomputed per table chunk (capi.hip:165-168) from the same carve_sort(2 tc H, N) the sort uses"),
    ("sort.rg.region / rg.gathered", "chunk_sort_kernel / bucket_sort_kernel", "sort_tables.hip:346,661",
     "bucket_sort_kernel", "sort_tables.hip:875", "read only below cnt"),
    # ---- buffers of the Python layer
    ("ops._row_buffers qhat/kvhat/qproj/kproj/minmax", "row builder, all three roles (stage call: roles == 3)",
     "prep_hash.hip:878-948", "sort / block_attn stage calls", "ops.py:276,332", "rows= reuses the buffers: rewritten identically"),
    ("ops.sort_tables ws, pos", "zero_words_kernel + chunk_sort_kernel; sort kernels", "sort_tables.hip:1252",
     "bucket_sort_kernel; caller", "sort_tables.hip:875", "stand-alone zero path"),
    ("ops.segmented_argsort ws, pos", "memset + raw_range_kernel + sort kernels", "sort_tables.hip:1387",
     "sort kernels; caller", "sort_tables.hip:288", "ragged: pos[s, lens[s]:] is documented undefined and not written"),
    ("ops.block_attn part", "block_attn kernels", "block_attn.hip:840", "caller", "ops.py:347", ""),
    ("ops.reduce_tables / _forward_partial acc", "reduce_tables_kernel or block_attn (one table, same format)",
     "combine.hip:573, capi.hip:294", "caller", "ops.py:380,575", ""),
    ("ops out / y (combine_out, _forward, combine_ffn, _attn_block_forward, combine_groups)", "combine kernels",
     "combine.hip:131,997,1034,1043", "caller", "ops.py:396,535,655,710,868", ""),
    ("ops.block_attn_bwd dq_part / dkv_part", "block_attn_bwd kernels", "block_attn_bwd.hip:54,422,652",
     "bwd_reduce_kernel / bwd_reduce16_kernel", "block_attn_bwd.hip:842,875", ""),
    ("ops.block_attn_bwd dq, dk, dv, dcs, dsw", "bwd_reduce kernels (+ dsw_kernel / dsw_sum_kernel)",
     "block_attn_bwd.hip:875,906,932", "caller", "ops.py:437-443", "rows at and after raw_size are stored as zeros"),
    ("ops.combine_bwd gacc, dw, db, scratch", "combine_bwd_rows / weight kernels write partials, *_sum kernels read them",
     "combine.hip:662,723,785", "caller", "ops.py:462-465", ""),
    ("ops.rows_wgrad dw, db, scratch", "wgrad_kernel partials", "block_train.hip:36", "wgrad_sum_kernel",
     "block_train.hip:92", ""),
    ("ops.ln_bwd dx, xn, dlw, dlb, scratch", "ln_bwd_kernel partials + dump row", "block_train.hip:199",
     "partial_sum_kernel", "block_train.hip:107", "the dump row is write-only"),
    ("ops.ln_ffn_fwd out / ln_ffn_bwd outs, scratch (z, h, dh, ln_part, wg_part)", "ln_ffn_bwd_kernel",
     "block_train.hip:288", "wgrad / partial_sum kernels", "block_train.hip:36,107", ""),
    ("ops.rpe_scale out / rpe_scale_bwd out", "rpe_scale_kernel / rpe_scale_bwd_kernel", "prep_hash.hip:35,105", "caller",
     "ops.py:232,246", ""),
    ("module workspaces (hept.py:_scratch, attn_block.py:forward, attn_stack.py:_scratch)", "as carve()", "capi.hip:28",
     "as carve()", "capi.hip:28", "the layers of an AttnStack share one: every block re-establishes what it reads (capi.hip:738-741)"),
    ("attn_stack.py:_forward_impl buf", "buf[:, :D].copy_(x); layer i's combine writes column block i + 1",
     "attn_stack.py:126, capi.hip:760", "layer i's row builder reads column block i", "capi.hip:760", ""),
    ("prep.py bounds (cloud_start | pad_start)", "probe_kernel, all 257 entries of each", "prepare.hip:296-306",
     "coord_keys_kernel and the kernels after it", "prepare.hip:28", "indices: every entry read has been written"),
    ("prep.py _prepare_outputs ws (keys, pos, seg_len, rank, row_max, codes_raw, ckeys, by_code), outputs",
     "coord_keys_kernel, ragged argsort, rank_scatter_kernel, codes_kernel, bounded argsort", "prepare.hip:23-104",
     "the kernel after each; pad_gather_kernel", "prepare.hip:135", "keys / pos are read below seg_len only"),
    ("prep.py prepare_input_src_hip x_pad, coords_pad, eta, phi, ws", "src_pad_keys_kernel, argsort, src_rank_kernel, src_region_kernel",
     "prepare.hip:173-201", "the kernel after each; caller", "prepare.hip:239", ""),
    # ---- entry points
    ("partial_begin -> partial_heads", "run_begin leaves rows and permutations in the workspace", "capi.hip:302-307",
     "hept_partial_heads", "capi.hip:412-445", "state carried between the two calls on purpose: poison before partial_begin only"),
]
AUDIT_FINDINGS = "none"

# ---------------------------------------------------------------------------------------------------------------------
# 2. the instrument
# ---------------------------------------------------------------------------------------------------------------------
MODULES = ("hept_amd.ops", "hept_amd.hept", "hept_amd.attn_block", "hept_amd.attn_stack", "hept_amd.autograd",
           "hept_amd.prep")
GUARD = 4096          # bytes on either side of a payload: the payload keeps the allocator's alignment
GUARD_BYTE = 0xA5
PATTERNS = ("leftover", "zero", "ff")     # run in this order
_FILL = {"zero": 0x00, "ff": 0xFF}
_HERE = os.path.abspath(__file__)


def _site():
    """``file:function`` of the frame that asked for memory (the first one outside this module; comprehensions and
    lambdas are named by the function around them)."""
    f = sys._getframe(1)
    while f is not None and (os.path.abspath(f.f_code.co_filename) == _HERE or f.f_code.co_name.startswith("<")):
        f = f.f_back
    if f is None:
        return "?:?"
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_code.co_name}"


class Ledger:
    """Every guarded buffer with the site that asked for it; ``check`` asserts that no guard byte was touched."""

    def __init__(self, pattern, donor_pool=None, guarded=lambda dev: dev.type == "cuda"):
        assert pattern in PATTERNS or pattern == "record", pattern
        self.pattern = pattern
        self.entries = []                     # (raw uint8 buffer, payload bytes, site)
        self.pool = donor_pool or {}          # leftover: site -> raw buffers of the donor case, in allocation order
        self._last = {}
        self.guarded = guarded

    @property
    def sites(self):
        return {e[2] for e in self.entries}

    def _leftover(self, nbytes, site, device):
        """The donor's buffer of the same site if it is large enough, as it stands; else a buffer of the case's own need
        whose payload repeats the donor's bytes."""
        queue = self.pool.get(site) or []
        own = bool(queue)                     # a donor buffer is handed out once: two live tensors never share one
        src = queue.pop(0) if own else self._last.get(site)
        if src is None:                       # a site the donor never reached: stale bytes of any of its buffers
            rest = [r for q in self.pool.values() for r in q] + list(self._last.values())
            assert rest, f"leftover: the donor case left no buffer at all (site {site})"
            src = max(rest, key=lambda r: r.numel())
        # (a copy: the buffer handed out is about to be overwritten, later allocations of the site still get the donor's bytes)
        self._last[site] = src.clone() if own else src
        if own and src.device == device and src.numel() >= nbytes + 2 * GUARD:
            return src[:nbytes + 2 * GUARD]
        raw = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=device)
        old = src[GUARD:src.numel() - GUARD].to(device)
        if nbytes:
            raw[GUARD:GUARD + nbytes] = old.repeat(-(-nbytes // max(1, old.numel())))[:nbytes] if old.numel() else 0xFF
        return raw

    def alloc(self, shape, dtype, device, site=None):
        """A typed, shaped view of ``guard | payload | guard``; the payload holds the pattern."""
        site = site or _site()
        shape = tuple(int(x) for x in shape)
        numel = 1
        for x in shape:
            numel *= x
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        if self.pattern == "leftover":
            raw = self._leftover(nbytes, site, device)
        else:
            raw = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=device)
            raw[GUARD:GUARD + nbytes] = _FILL.get(self.pattern, 0x00)
        raw[:GUARD] = GUARD_BYTE
        raw[GUARD + nbytes:] = GUARD_BYTE
        self.entries.append((raw, nbytes, site))
        if self.pattern == "record":
            self.pool.setdefault(site, []).append(raw)
        return raw[GUARD:GUARD + nbytes].view(dtype).view(shape)

    def check(self):
        if not self.entries:
            return
        if any(e[0].is_cuda for e in self.entries):
            torch.cuda.synchronize()
        guards = torch.stack([g for raw, nbytes, _ in self.entries for g in (raw[:GUARD], raw[GUARD + nbytes:])])
        bad = (guards != GUARD_BYTE)
        if not bool(bad.any()):
            return
        i = int(bad.any(1).nonzero()[0])
        raw, nbytes, site = self.entries[i // 2]
        off = int(bad[i].nonzero()[0])
        side = "after the end" if i % 2 else "before the start"
        where = off if i % 2 else off - GUARD
        raise AssertionError(f"guard bytes of the buffer allocated at {site} ({nbytes} bytes) were overwritten {side}: "
                             f"first at byte offset {where} relative to that edge ({int(bad[i].sum())} bytes in all)")


class _TensorMeta(type):
    def __instancecheck__(cls, obj):
        return isinstance(obj, torch.Tensor)

    def __getattr__(cls, name):
        return getattr(torch.Tensor, name)


class TorchProxy:
    """Stands in for the ``torch`` name of a module: forwards everything but the allocation calls."""

    def __init__(self, ledger):
        self._ledger = ledger
        proxy = self

        class Tensor(metaclass=_TensorMeta):
            @staticmethod
            def new_empty(t, *size, **kw):
                return proxy.new_empty(t, *size, **kw)

        self.Tensor = Tensor

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _shape(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            return tuple(size[0])
        return tuple(size)

    def empty(self, *size, dtype=None, device=None, **kw):
        dev = torch.device(device) if device is not None else torch.empty(0).device
        if not self._ledger.guarded(dev):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return self._ledger.alloc(self._shape(size), dtype or torch.get_default_dtype(), dev)

    def empty_like(self, t, dtype=None, device=None, **kw):
        dev = torch.device(device) if device is not None else t.device
        if not self._ledger.guarded(dev):
            return torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._ledger.alloc(t.shape, dtype or t.dtype, dev)

    def new_empty(self, t, *size, dtype=None, device=None, **kw):
        dev = torch.device(device) if device is not None else t.device
        if not self._ledger.guarded(dev):
            return t.new_empty(*size, dtype=dtype, device=device, **kw)
        return self._ledger.alloc(self._shape(size), dtype or t.dtype, dev)


@contextlib.contextmanager
def scratch(pattern, donor_pool=None, guarded=None, modules=MODULES):
    """Replace the ``torch`` name inside the modules of the Python layer by a proxy for the duration of the block; yields
    the ledger.  ``torch`` itself is not touched."""
    import importlib

    import pytest

    ledger = Ledger(pattern, donor_pool, **({"guarded": guarded} if guarded else {}))
    proxy = TorchProxy(ledger)
    mp = pytest.MonkeyPatch()
    try:
        for name in modules:
            mp.setattr(importlib.import_module(name), "torch", proxy)
        yield ledger
    finally:
        mp.undo()


# ---------------------------------------------------------------------------------------------------------------------
# 3. masks, in-out arguments, sites
# ---------------------------------------------------------------------------------------------------------------------
# Spare words of intermediate stage outputs that nobody is meant to read would be listed here as
# (tensor name, slice description, file:line that shows no kernel reads them).  There are none: every stage output is
# compared whole.  The words one might have masked are documented as zero and asserted to be zero instead (ZERO_WORDS).
MASKS = []
FINAL_RESULTS = ("out", "y", "acc", "qpos", "kpos", "pos", "grad")     # no word of these may ever be masked
ZERO_WORDS = [
    ("minmax", "[..., 3]", "csrc/prep_hash.hip:466-468,793"),
    ("part (f32 rows)", "[..., D + 1:]", "hept_amd/ops.py:333"),
    ("part (packed rows)", "[..., 13:]", "hept_amd/ops.py:334"),
    ("qhat", "[..., E:31]", "csrc/prep_hash.hip:759,769"),
    ("dq, dk, dv, dcs of block_attn_bwd", "[raw_size:]", "hept_amd/ops.py:410"),
    ("rows of partial_heads", "[N:n_pad]", "hept_amd/ops.py:845"),
]
# documented in-out arguments: left out of the inputs-untouched check, held to idempotence instead
# stage outputs that hold infinities by contract (the neutral range of a spare minmax slot, the +inf hash of a padding
# row): "no pattern word" means no NaN there, finite everywhere else
INF_BY_CONTRACT = ("minmax", "qproj", "kproj")
IN_OUT = {"sort_tables_src": "minmax", "prep_hash": "rows", "attn_stack_forward": "xcat", "attn_stack_forward_src": "xcat"}

# allocation site -> the entries (``Case.entry``) every case of which reaches it
SITES = {
    "ops.py:_workspace": ("op", "attn", "src", "stack", "stack_src"),
    "ops.py:_row_buffers": ("op", "attn", "src", "bwd", "train_op", "train_attn", "train_src"),
    "ops.py:rpe_scale": ("op", "attn", "src", "bwd", "train_op", "train_attn", "train_src"),
    "ops.py:rpe_scale_bwd": ("train_op", "train_attn", "train_src"),
    "ops.py:sort_tables": ("op", "attn", "sort_tables", "train_op", "train_attn"),
    "ops.py:sort_tables_src": ("src", "sort_tables_src", "bwd", "train_src"),
    "ops.py:segmented_argsort": ("argsort",),
    "ops.py:block_attn": ("op", "attn", "src", "train_op", "train_attn", "train_src"),
    "ops.py:reduce_tables": ("op", "train_op", "train_attn", "train_src"),
    "ops.py:combine_out": ("op", "train_op", "train_attn", "train_src"),
    "ops.py:block_attn_bwd": ("bwd", "train_op", "train_attn", "train_src"),
    "ops.py:combine_bwd": ("train_op", "train_attn", "train_src"),
    "ops.py:_forward": ("op", "src"),
    "ops.py:_forward_partial": ("op",),
    "ops.py:combine_ffn": ("attn", "src"),
    "ops.py:_attn_block_forward": ("attn", "src"),
    "ops.py:combine_groups": ("partial",),
    "ops.py:rows_wgrad": ("train_attn", "train_src"),
    "ops.py:ln_bwd": ("train_attn", "train_src"),
    "ops.py:ln_ffn_fwd": ("train_attn", "train_src"),
    "ops.py:ln_ffn_bwd": ("train_attn", "train_src"),
    "hept.py:_scratch": ("op",),
    "attn_block.py:forward": ("attn", "src"),
    "attn_stack.py:_scratch": ("stack", "stack_src"),
    "attn_stack.py:_forward_impl": ("stack", "stack_src"),
    "prep.py:prepare_input_hip": ("prepare",),
    "prep.py:_prepare_outputs": ("prepare",),
    "prep.py:prepare_input_src_hip": ("prepare_src",),
}
# ``empty`` calls of hept_amd/*.py that this sweep does not drive, each with the reason
NOT_DRIVEN = {
    "prep.py:quantile_partition": "host mirror: GPU tensors take prepare_input_src_hip (prep.py:267-268)",
    "prep.py:_rank_within_cloud": "host mirror: GPU tensors take prepare_input_hip (prep.py:220-221)",
    "library.py:_": "the shape functions torch.library registers for the four custom ops: meta tensors only",
    "ops.py:forward_sharded": "needs a communicator of several GPUs: out of scope (the sharded stages run as 'partial')",
    "sharding.py:exchange_buffer": "multi-GPU exchange: out of scope",
    "sharding.py:pipelined": "multi-GPU exchange: out of scope",
    "sharding.py:finish": "multi-GPU exchange: out of scope",
}

# ---------------------------------------------------------------------------------------------------------------------
# 4. cases
# ---------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id entry shape precision extra")
OP_IDS = ("b8", "b33", "b100", "cloud-b-b1-100", "b256", "n6272", "t9-n6272", "t17", "h7d17c3", "h16d27c3", "n9000-b225")
SRC_IDS = ("n1000-minus1-b100-t3-c6-later", "n100-single-b100-t3-c6", "n396-one-in-last-block-b33-t9-c2-later",
           "n6272-full-b128-t1-c6-later", "n6176-minus1-b32-t9-c2")
TRAIN_OP_IDS = ("b33", "n6272", "h7d17c3")
# HEPTAttention.train(): tiles id -> (module precision, train_tiles)
TRAIN_OP_TILES = {"fp32": ("fp32", "fp32"), "fp32_mfma": ("fp32_mfma", "fp32"), "fp32_diff": ("fp32_diff", "fp32"),
                  "bf16": ("fp32", "bf16")}
BWD_IDS = ("n1000-minus1-b100-t3-c6-later", "n6400-one-in-last-block-b256-t1-c2-later")
TRAIN_ATTN_IDS = ("b33-c4-t3", "n6272-c6")
TRAIN_SRC_IDS = ("n1000-minus1-b100-t3-c6-later", "n6272-full-b128-t1-c6-later")
MAX_POINTS = 10240


def _tile(p):
    return {"bf16": "bf16", "mixed16": "mixed16"}.get(p, "f32")


def op_signature(s, p):
    """What the scratch of a whole-operator call depends on in a precision: the row type, who writes the v half, the
    format of the partial rows.  One precision per distinct signature is run."""
    n = sw.n_points(s)
    return (_tile(p), sw.riders(n, s.H, s.D, s.T, p, s.B), sw.direct_v(s.D, p, s.B), _tile(p) != "f32" and s.D == 24)


def op_precisions(s):
    seen, out = set(), []
    for p in PRECISIONS:
        sig = op_signature(s, p)
        if sig not in seen:
            seen.add(sig)
            out.append(p)
    return out


def attn_cases():
    """One attn_sweep shape per cell of its ``cells()`` that names a row-builder or sort branch (greedy, in list order)."""
    want = lambda c: c.startswith(("prep<", "sort-", "table-chunks", "tables-one-chunk"))
    seen, out = set(), []
    for s in asw.SHAPES:
        if sw.n_points(s) > MAX_POINTS:
            continue
        new = {c for c in asw.cells(s) if want(c)} - seen
        if new:
            seen |= new
            out.append(s)
    return out


def _cases():
    out = []
    for sid in OP_IDS:
        for p in op_precisions(sw.BY_ID[sid]):
            out.append(Case(f"op-{sid}-{p}", "op", sid, p, None))
    for sid in ("b100", "n6272"):                     # below and above SMALL_CAP keys per segment
        out.append(Case(f"sort_tables-{sid}", "sort_tables", sid, "fp32", None))
    for sid in ("n1000-minus1-b100-t3-c6-later", "n6272-full-b128-t1-c6-later"):
        out.append(Case(f"sort_tables_src-{sid}", "sort_tables_src", sid, "fp32", None))
    for length in (500, 7000):
        for ragged in (False, True):
            out.append(Case(f"argsort-l{length}-{'ragged' if ragged else 'plain'}", "argsort", None, None, (length, ragged)))
    precs = ("fp32", "bf16", "mixed16", "fp32_mfma")
    for i, s in enumerate(attn_cases()):
        # (the 16-bit x of the io path on the first two cases, one per type)
        io = {0: "bfloat16", 1: "float16"}.get(i)
        out.append(Case(f"attn-{s.id}-{precs[i % len(precs)]}", "attn", s.id, precs[i % len(precs)], io))
    for i, sid in enumerate(SRC_IDS):
        out.append(Case(f"src-{sid}-{precs[i % len(precs)]}", "src", sid, precs[i % len(precs)], None))
    for n, b in ((1300, 100), (6272, 32)):            # below and above SMALL_CAP points, three layers
        out.append(Case(f"stack-n{n}", "stack", None, "fp32" if n > SMALL_CAP else "bf16", (n, b, 3, 6, 3)))
        out.append(Case(f"stack_src-n{n}", "stack_src", None, "bf16" if n > SMALL_CAP else "fp32", (n, b, 3, 6, 3)))
    for sid, w, ng, p in (("t3", 2, 2, "fp32"), ("t3", 3, 4, "bf16"), ("n6272-t9", 3, 3, "fp32"), ("t17", 2, 2, "bf16"),
                          ("src-n1000-full", 2, 2, "mixed16"), ("src-n6272-minus1", 3, 2, "fp32")):
        out.append(Case(f"partial-{sid}-w{w}-g{ng}-{p}", "partial", sid, p, (w, ng)))
    for sid in BWD_IDS:                                # the stage backward on padding rows: its documented zero rows
        for tiles in TRAIN_OP_TILES:
            out.append(Case(f"bwd-{sid}-{tiles}", "bwd", sid, tiles, None))
    for sid in TRAIN_OP_IDS:
        for tiles in TRAIN_OP_TILES:
            out.append(Case(f"train_op-{sid}-{tiles}", "train_op", sid, tiles, None))
    for sid in TRAIN_ATTN_IDS:
        for mode in asw.TRAIN:
            out.append(Case(f"train_attn-{sid}-{mode}", "train_attn", sid, mode, None))
    for sid in TRAIN_SRC_IDS:
        for mode in asw.TRAIN:
            out.append(Case(f"train_src-{sid}-{mode}", "train_src", sid, mode, None))
    for name in ("g2_example4k", "clouds7", "clouds255"):
        out.append(Case(f"prepare-{name}", "prepare", name, None, None))
    for sid in ("n1000-minus1-b100-t3-c6-later", "n6176-minus1-b32-t9-c2"):
        out.append(Case(f"prepare_src-{sid}", "prepare_src", sid, None, None))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
INTERLEAVED = ("train_op", "train_attn", "train_src")     # assertion (d)


def case_points(c):
    if c.entry in ("op", "sort_tables", "train_op"):
        return sw.n_points(sw.BY_ID[c.shape])
    if c.entry in ("attn", "train_attn"):
        return sw.n_points(asw.BY_ID[c.shape])
    if c.entry in ("src", "sort_tables_src", "train_src", "prepare_src", "bwd"):
        return ssw.BY_ID[c.shape].N
    if c.entry in ("stack", "stack_src"):
        return c.extra[0]
    if c.entry == "partial":
        return shw.n_points(shw.BY_ID[c.shape])
    if c.entry == "argsort":
        return c.extra[0]
    return {"g2_example4k": 4096, "clouds7": 1000, "clouds255": 6000}[c.shape]


def case_cells(c):
    """The dispatch branches a case takes, computed by the sweeps' own ``cells()`` -- the rules are not restated here --
    plus the scratch-specific ones: who writes the v half, which sort, one or several table chunks, who clears the
    REGION sort's counters."""
    out = set()
    if c.entry in ("op", "train_op", "sort_tables"):
        s = sw.BY_ID[c.shape]
        cl = sw.cells(s)
        sort = "sort-two-launch" if "sort-two-launch" in cl else "sort-one-workgroup"
        chunks = "table-chunks" if "table-chunks" in cl else "tables-one-chunk"
        out |= {sort, chunks, f"{sort}/{chunks}"}
        if c.entry == "op":
            p = c.precision
            writer = "v-direct" if f"direct-v:{p}" in cl else "v-riders" if f"riders:{p}" in cl else "v-row-builder"
            out |= {writer, f"{writer}/{sort}"}
            if sort == "sort-two-launch":             # (the one-workgroup sort has no counters to clear)
                out |= {"zero-row-builder", "zero-stand-alone"}      # the one-call forward, the staged sort_tables
        elif sort == "sort-two-launch":
            out.add("zero-stand-alone")
    elif c.entry in ("attn", "train_attn"):
        cl = asw.cells(asw.BY_ID[c.shape])
        sort = "sort-two-launch" if "sort-two-launch" in cl else "sort-one-workgroup"
        chunks = "table-chunks" if "table-chunks" in cl else "tables-one-chunk"
        out |= {sort, chunks, f"{sort}/{chunks}", "v-row-builder", f"v-row-builder/{sort}"}
        if sort == "sort-two-launch":
            out |= {"zero-stand-alone"} | ({"zero-row-builder"} if c.entry == "attn" else set())
    elif c.entry in ("src", "train_src", "sort_tables_src", "bwd"):
        cl = ssw.cells(ssw.BY_ID[c.shape])
        sort = "sort-two-launch" if "sort-two-launch" in cl else "sort-one-workgroup"
        chunks = "table-chunks" if "table-chunks" in cl else "tables-one-chunk"
        out |= {sort, chunks, f"{sort}/{chunks}", "src-bounds-in-minmax" if sort == "sort-two-launch" else "src-bounds-in-kernel"}
        if sort == "sort-two-launch":
            out |= {"zero-stand-alone"} | ({"zero-row-builder"} if c.entry == "src" else set())
    return out


def expected_sites(c):
    return {site for site, entries in SITES.items() if c.entry in entries}


def donor_of(c):
    """The case whose leftovers ``c`` runs on: the next case of the same entry with another point count and, where the
    list allows it, another precision (so other parameters and another seed as well)."""
    same = [x for x in CASES if x.entry == c.entry and x.id != c.id]
    i = [x.id for x in CASES if x.entry == c.entry].index(c.id)
    same = same[i % max(1, len(same)):] + same[:i % max(1, len(same))]
    other_n = [x for x in same if case_points(x) != case_points(c)] or same
    best = [x for x in other_n if x.precision != c.precision] or other_n
    return best[0] if best else c


# ---------------------------------------------------------------------------------------------------------------------
# 5. runners (GPU; imports deferred).  run(case, g) -> {name: tensor}; inputs(case, dev) -> g (nested tensors)
# ---------------------------------------------------------------------------------------------------------------------
_inputs = {}
_clean = {}


def _walk(obj, prefix=""):
    """(name, tensor) of every tensor in a nest of dicts / lists / tuples / modules."""
    if torch.is_tensor(obj):
        yield prefix, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _walk(v, f"{prefix}.{k}" if prefix else str(k))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _walk(v, f"{prefix}[{i}]")


def bits(t):
    """A tensor's bytes: NaN compares equal to the same NaN, -0 differs from +0."""
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def inputs(c, dev):
    key = (c.entry in ("op", "sort_tables", "train_op") and "sw") or (c.entry in ("attn", "train_attn") and "asw") or \
        (c.entry in ("src", "sort_tables_src", "train_src", "prepare_src", "bwd") and "ssw") or c.entry, c.shape, c.extra
    if key in _inputs:
        return _inputs[key]
    if len(_inputs) > 6:
        _inputs.clear()
    if key[0] == "sw":
        s = sw.BY_ID[c.shape]
        g = sw._gpu(sw.inputs(s), dev)
    elif key[0] == "asw":
        g = asw._gpu(asw.inputs(asw.BY_ID[c.shape]), dev)
    elif key[0] == "ssw":
        g = ssw._gpu(ssw.inputs(ssw.BY_ID[c.shape]), dev)
    elif c.entry == "partial":
        g = shw._gpu(shw.inputs(shw.BY_ID[c.shape]), dev)
    elif c.entry in ("stack", "stack_src"):
        n, b, t, cc, n_layers = c.extra
        if c.entry == "stack":
            s = asw.Shape(c.id, (n,), b, t, cc, 9100 + n, False, False)
            g = asw._gpu(asw.inputs(s), dev)
            g["layers"] = [g["params"]] + [{k: v.to(dev) for k, v in asw.default_params(cc, t, s.seed + 10 * i).items()}
                                           for i in range(1, n_layers)]
        else:
            s = ssw.Shape(c.id, n, n - 1, b, t, cc, True, 9300 + n, False)
            g = ssw._gpu(ssw.inputs(s), dev)
            g["layers"] = [g["params"]] + [{k: v.to(dev) for k, v in ssw.params(s._replace(seed=s.seed + 10 * i)).items()}
                                           for i in range(1, n_layers)]
    elif c.entry == "argsort":
        length, ragged = c.extra
        gen = torch.Generator().manual_seed(length + ragged)
        keys = torch.randn(5, length, generator=gen)
        keys[1, length // 2:] = float("inf")           # +inf pads sort last
        keys[2] = keys[2].round()                      # ties
        lens = torch.tensor([length, length // 2, 1, length - 1, length // 3], dtype=torch.int32)
        g = dict(keys=keys.to(dev), lens=lens.to(dev) if ragged else None)
    elif c.entry == "prepare":
        import cases as golden

        if c.shape == "g2_example4k":
            inp, _ = golden.load_case(c.shape)
            g = dict(coords=inp["coords_raw"].to(dev), batch=inp["batch"].to(dev), regions=inp["regions"].to(dev),
                     block_size=golden.CASES[c.shape]["block_size"], num_heads=golden.NUM_HEADS)
        else:                                          # tests/test_gpu_prepare.py test_cloud_boundaries_from_the_probe_kernel
            n_clouds = int(c.shape[len("clouds"):])
            gen = torch.Generator().manual_seed(n_clouds)
            sizes = torch.randint(1, 40, (n_clouds,), generator=gen)
            sizes[0], sizes[-1] = 1, 333
            batch = torch.repeat_interleave(torch.arange(n_clouds), sizes)
            coords = torch.randn(int(sizes.sum()), 4, generator=gen)
            regions = torch.tensor([[[2.0] * golden.NUM_HEADS, [3.0] * golden.NUM_HEADS]] * 2)
            g = dict(coords=coords.to(dev), batch=batch.to(dev, torch.int32 if n_clouds == 7 else torch.int64),
                     regions=regions.to(dev), block_size=16, num_heads=golden.NUM_HEADS)
        g["x"] = torch.arange(g["coords"].shape[0], device=dev)
    else:
        raise AssertionError(c)
    _inputs[key] = g
    return g


def _op_staged(s, g, precision, out):
    """prep_hash -> sort_tables (chunks, rows reused) -> block_attn -> reduce_tables / combine_out, every stage output kept."""
    from hept_amd import ops

    prec, f32_mfma, _ = PRECISIONS[precision]
    sqrt_w = ops.rpe_scale(g["w_rpe_weight"], s.H, s.D, 10)
    rows, qs, ks = None, [], []
    for c0 in range(0, s.T, MAX_TABLES):
        tc = min(MAX_TABLES, s.T - c0)
        ph = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sqrt_w, g["alpha"], g["combined_shifts"], prec, t0=c0, tl=tc,
                           rows=rows)
        rows = (ph["qhat"], ph["kvhat"])
        qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"], t0=c0)
        out.update({f"qproj@{c0}": ph["qproj"], f"kproj@{c0}": ph["kproj"], f"minmax@{c0}": ph["minmax"]})
        qs.append(qp)
        ks.append(kp)
    if s.T > MAX_TABLES:
        # rows= is an in-out argument: a further call on the same buffers must leave the same bits
        before = [r.clone() for r in rows]
        ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sqrt_w, g["alpha"], g["combined_shifts"], prec, t0=0,
                      tl=MAX_TABLES, rows=rows)
        assert all(same_bits(a, b) for a, b in zip(before, rows)), f"{s.id} {precision}: prep_hash(rows=) is not idempotent"
    qpos, kpos = torch.cat(qs), torch.cat(ks)
    part = ops.block_attn(rows[0], rows[1], qpos, kpos, s.D, s.B, f32_mfma=f32_mfma)
    out.update(sqrt_w=sqrt_w, qhat=rows[0], kvhat=rows[1], qpos=qpos, kpos=kpos, part=part,
               acc_staged=ops.reduce_tables(part, s.D), out_staged=ops.combine_out(part, s.D, g["out_weight"], g["out_bias"]))
    # the words documented as zero
    for k_, v_ in out.items():
        if k_.startswith("minmax@"):
            assert not bool(v_[..., 3].any()), f"{s.id} {precision}: {k_}[..., 3] is documented as zero"
    wide = ops.unpack_part(part)
    assert not bool(wide[..., s.D + 1:].any()), f"{s.id} {precision}: part columns above D are documented as zero"
    if part.dtype == torch.int32:
        assert not bool(part[..., 13:].any()), f"{s.id} {precision}: packed part columns 13-15 are documented as zero"
    e = s.D + s.C
    if rows[0].dtype == torch.float32:
        assert not bool(rows[0][..., e:31].any()), f"{s.id} {precision}: qhat columns [E:31] are documented as zero"


def run_op(c, g):
    from hept_amd import HEPTAttention, ops

    s, p = sw.BY_ID[c.shape], c.precision
    prec = PRECISIONS[p][0]
    out = {}
    with asw._diff_mfma(p), torch.no_grad():
        _op_staged(s, g, p, out)
        args = (g["q"], g["k"], g["v"], g["coords"], g["combined_shifts"], g["w_rpe_weight"], g["alpha"])
        kw = dict(block_size=s.B, w_per_dist=10, precision=prec)
        out["out"] = ops.forward(*args, g["out_weight"], g["out_bias"], **kw)
        out["acc"] = ops.forward_partial(*args, t0=0, tl=s.T, **kw)
        if s.T > 1:
            out["acc_tail"] = ops.forward_partial(*args, t0=1, tl=s.T - 1, **kw)     # t0 > 0; one table: the direct scatter
        if ops.packed_partials(prec, s.D):
            out["acc_packed"] = ops.forward_partial(*args, t0=0, tl=s.T, packed=True, **kw)
            out["acc_packed_t1"] = ops.forward_partial(*args, t0=s.T - 1, tl=1, packed=True, **kw)
        m = HEPTAttention(s.D + s.C, precision=prec, h_dim=s.D, num_heads=s.H, block_size=s.B, n_hashes=s.T,
                          num_w_per_dist=10)
        m.load_state_dict({"out_linear.weight": g["out_weight"], "out_linear.bias": g["out_bias"], "e2lsh.alpha": g["alpha"]})
        m = m.to(g["q"].device).eval()
        w_rpe = torch.nn.Linear(g["w_rpe_weight"].shape[1], g["w_rpe_weight"].shape[0], device=g["q"].device)
        w_rpe.weight.copy_(g["w_rpe_weight"])
        out["out_module"] = m(g["q"], g["k"], g["v"], w_rpe=w_rpe, coords=g["coords"], combined_shifts=g["combined_shifts"])
        out["out_module_again"] = m(g["q"], g["k"], g["v"], w_rpe=w_rpe, coords=g["coords"],
                                    combined_shifts=g["combined_shifts"])              # on the workspace the call before left
    return out


def _stage_inputs(c, g):
    """Rows, hashes and range partials of a clean row-builder call: the inputs of the stand-alone sorts."""
    from hept_amd import ops

    key = ("stage", c.id)
    if key not in _inputs:
        if c.entry == "sort_tables":
            s = sw.BY_ID[c.shape]
            sqrt_w = ops.rpe_scale(g["w_rpe_weight"], s.H, s.D, 10)
            _inputs[key] = ops.prep_hash(g["q"], g["k"], g["v"], g["coords"], sqrt_w, g["alpha"], g["combined_shifts"], "fp32")
        else:
            s, p = ssw.BY_ID[c.shape], g["params"]
            sqrt_w = ops.rpe_scale(p["w_rpe.weight"], H, D, K)
            tc = min(s.T, MAX_TABLES)
            ph = ops.prep_hash_fused(g["x"], p["norm1.weight"], p["norm1.bias"], EPS, p["w_q.weight"], p["w_k.weight"],
                                     p["w_v.weight"], g["coords"], sqrt_w, p["attn.e2lsh.alpha"], None, "fp32", t0=0, tl=tc,
                                     raw_size=g["raw_size"])
            ph["geo"] = ops.geo_args((g["eta"], g["phi"]), g["regions_h"], s.T, H, s.N)
            _inputs[key] = ph
    return _inputs[key]


def run_sort_tables(c, g):
    from hept_amd import ops

    ph = _stage_inputs(c, g)
    qp, kp = ops.sort_tables(ph["qproj"], ph["kproj"], g["combined_shifts"], ph["minmax"])
    return dict(qpos=qp, kpos=kp)


def run_sort_tables_src(c, g):
    from hept_amd import ops

    ph = _stage_inputs(c, g)
    eta, phi, cfac = ph["geo"]
    minmax = ph["minmax"].clone()            # the documented in-out argument: the sort writes the src bounds into it
    qp, kp = ops.sort_tables_src(ph["qproj"], ph["kproj"], eta, phi, cfac, minmax)
    first = minmax.clone()
    qp2, kp2 = ops.sort_tables_src(ph["qproj"], ph["kproj"], eta, phi, cfac, minmax)
    assert same_bits(qp, qp2) and same_bits(kp, kp2) and same_bits(first, minmax), f"{c.id}: sort_tables_src is not idempotent"
    return dict(qpos=qp, kpos=kp, minmax=minmax)


def run_argsort(c, g):
    from hept_amd import ops

    pos = ops.segmented_argsort(g["keys"], g["lens"])
    if g["lens"] is None:
        return dict(pos=pos)
    # ragged: only pos[s, :lens[s]] is defined (hept_amd/ops.py:312-313); the tail is not a result and is not written
    lens = g["lens"].tolist()
    out = {f"pos[{i}]": pos[i, :n] for i, n in enumerate(lens)}
    out["_tail"] = torch.cat([pos[i, n:] for i, n in enumerate(lens)])
    return out


def run_bwd(c, g):
    """The stage backward of the src variant: rows at and after raw_size of dq, dk, dv and dcs are documented as zero
    (hept_amd/ops.py:410) whatever the gradient rows and the result buffers held."""
    from hept_amd import ops

    s, p = ssw.BY_ID[c.shape], g["params"]
    prec, tiles = TRAIN_OP_TILES[c.precision]
    f32_mfma = {"fp32": False, "fp32_mfma": True, "fp32_diff": "diff"}[prec]
    raw, tc = g["raw_size"], min(s.T, MAX_TABLES)
    sqrt_w = ops.rpe_scale(p["w_rpe.weight"], H, D, K)
    eta, phi, cfac = ops.geo_args((g["eta"], g["phi"]), g["regions_h"], s.T, H, s.N)
    ph = ops.prep_hash_fused(g["x"], p["norm1.weight"], p["norm1.bias"], EPS, p["w_q.weight"], p["w_k.weight"],
                             p["w_v.weight"], g["coords"], sqrt_w, p["attn.e2lsh.alpha"], None, tiles, t0=0, tl=tc,
                             raw_size=raw)
    qp, kp = ops.sort_tables_src(ph["qproj"], ph["kproj"], eta, phi, cfac, ph["minmax"])
    if "gacc" not in g:
        g["gacc"] = torch.randn(s.N, H, 32, generator=torch.Generator().manual_seed(s.seed + 7)).to(g["x"].device)
    dq, dk, dv, dcs, dsw = ops.block_attn_bwd(ph["qhat"], ph["kvhat"], qp, kp, g["gacc"], D, s.C, s.B, f32_mfma=f32_mfma,
                                              coords=g["coords"], raw_size=raw)
    assert raw < s.N
    for nm, t in (("dq", dq), ("dk", dk), ("dv", dv), ("dcs", dcs)):
        assert not bool(t[raw:].any()), f"{c.id}: {nm}[raw_size:] is documented as zero"
    return {"grad q": dq, "grad k": dk, "grad v": dv, "grad cs": dcs, "grad sqrt_w": dsw, "qpos": qp, "kpos": kp}


def _x_io(c, g):
    return g["x"] if not c.extra else g["x"].to(getattr(torch, c.extra))


def run_attn(c, g):
    from hept_amd import ops

    s, p = asw.BY_ID[c.shape], c.precision
    prec = PRECISIONS[p][0]
    x = _x_io(c, g)
    with asw._diff_mfma(p), torch.no_grad():
        st = asw.staged(s, g, p)
        y = ops.attn_block_forward(x, g["coords"], g["combined_shifts"], g["params"], num_heads=H, block_size=s.B,
                                   w_per_dist=K, eps1=EPS, eps2=EPS, precision=prec)
        blk = asw.module(s, {"params": g["params"]}, prec, x.device).eval()
        kwargs = {"coords": g["coords"], "combined_shifts": g["combined_shifts"]}
        y_mod = blk(x, kwargs)
        y_again = blk(x, kwargs)
    return dict(y=y, y_module=y_mod, y_module_again=y_again, y_staged=st["y"], part=st["part"], qpos=st["qpos"], kpos=st["kpos"])


def _qkv(g):
    p = g["params"]
    xn = torch.nn.functional.layer_norm(g["x"], (D,), p["norm1.weight"], p["norm1.bias"], EPS)
    return [(xn @ p[f"w_{n}.weight"].t()).contiguous() for n in "qkv"]


def run_src(c, g):
    from hept_amd import ops

    s, p = ssw.BY_ID[c.shape], c.precision
    prec = PRECISIONS[p][0]
    pr = g["params"]
    with asw._diff_mfma(p), torch.no_grad():
        st = ssw.staged(s, g, p)
        y = ssw.one_call(s, g, p)
        blk = ssw.module(s, {"params": pr}, prec, g["x"].device).eval()
        y_mod = blk(g["x"], ssw.kwargs_of(g))
        y_again = blk(g["x"], ssw.kwargs_of(g))
        q, k, v = g["qkv"]
        out = ops.forward_src(q, k, v, g["coords"], (g["eta"], g["phi"]), g["regions_h"], g["raw_size"], pr["w_rpe.weight"],
                              pr["attn.e2lsh.alpha"], pr["attn.out_linear.weight"], pr["attn.out_linear.bias"],
                              block_size=s.B, w_per_dist=K, precision=prec)
    return dict(y=y, y_module=y_mod, y_module_again=y_again, y_staged=st["y"], part=st["part"], qpos=st["qpos"],
                kpos=st["kpos"], out=out)


def run_stack(c, g):
    from hept_amd import AttnStack, ops

    n, b, t, cc, n_layers = c.extra
    prec = c.precision
    src = c.entry == "stack_src"
    dev = g["x"].device
    kw = dict(num_heads=H, block_size=b, w_per_dist=K, eps1=EPS, eps2=EPS, precision=prec)
    buf = torch.full((n, (n_layers + 1) * D), -7.25, device=dev)
    buf[:, :D].copy_(g["x"])
    with torch.no_grad():
        if src:
            geo = ((g["eta"], g["phi"]), g["regions_h"], g["raw_size"])
            ops.attn_stack_forward_src(buf, g["coords"], *geo, g["layers"], **kw)
            first = buf.clone()
            ops.attn_stack_forward_src(buf, g["coords"], *geo, g["layers"], **kw)    # xcat is in-out: idempotent
            kwargs = ssw.kwargs_of(g)
        else:
            ops.attn_stack_forward(buf, g["coords"], g["combined_shifts"], g["layers"], **kw)
            first = buf.clone()
            ops.attn_stack_forward(buf, g["coords"], g["combined_shifts"], g["layers"], **kw)
            kwargs = {"coords": g["coords"], "combined_shifts": g["combined_shifts"]}
        assert same_bits(first, buf), f"{c.id}: attn_stack_forward on its own result buffer is not idempotent"
        stack = AttnStack(cc, precision=prec, variant="src" if src else "example", h_dim=D, num_heads=H, block_size=b,
                          n_hashes=t, num_w_per_dist=K, n_layers=n_layers)
        for layer, params in zip(stack.attns, g["layers"]):
            layer.load_state_dict(params, strict=True)
        stack = stack.to(dev).eval()
        y_mod = stack(g["x"], kwargs)
        y_again = stack(g["x"], kwargs)
    return dict(y=buf, y_module=y_mod, y_module_again=y_again)


def run_partial(c, g, ledger=None):
    """partial_begin, then partial_heads group by group into rows that hold the pattern, as shard_sweep drives them; the
    workspace is sized at exactly ops.workspace_bytes and poisoned before partial_begin only."""
    from hept_amd import ops

    s, (w, ng), prec = shw.BY_ID[c.shape], c.extra, c.precision
    dev = g["q"].device
    n, hg = shw.n_points(s), s.H // ng
    per = -(-n // w)
    n_pad = per * w
    _, geo = shw._op_args(s, g)
    out = {}
    for packed in ([False, True] if shw.packs(prec, s.D) else [False]):
        row, dt = (16, torch.int32) if packed else (32, torch.float32)
        for r in range(w):
            t0, tl = shw.table_slice(s.T, r, w)
            need = ops.workspace_bytes(n, s.H, s.D, s.C, tl, s.B, prec)
            if ledger is None:
                ws = torch.empty(need, device=dev, dtype=torch.uint8)
                buf = torch.empty((ng, n_pad, hg, row), device=dev, dtype=dt)
            else:
                ws = ledger.alloc((need,), torch.uint8, dev, site="scratch_sweep.py:partial.workspace")
                buf = ledger.alloc((ng, n_pad, hg, row), dt, dev, site="scratch_sweep.py:partial.rows")
            dims = ops.partial_begin(g["q"], g["k"], g["v"], g["coords"], g.get("combined_shifts"), g["w_rpe_weight"],
                                     g["alpha"], block_size=s.B, w_per_dist=10, t0=t0, tl=tl, precision=prec, workspace=ws,
                                     geo=geo)
            for grp in range(ng):
                ops.partial_heads(ws, dims, tl, s.B, prec, grp * hg, buf[grp])
            assert not bool(buf[:, n:].any()), f"{c.id}: rank {r} padding rows [{n}, {n_pad}) are documented as zero"
            out[f"rows-r{r}-{'packed' if packed else 'f32'}"] = buf
        send = [out[f"rows-r{r}-{'packed' if packed else 'f32'}"] for r in range(w)]
        for d_ in range(w):
            _, cnt = shw.point_slice(n, d_, w)
            recv = torch.stack([send[r][:, d_ * per:(d_ + 1) * per] for r in range(w)], dim=1).contiguous()
            out[f"out-d{d_}-{'packed' if packed else 'f32'}"] = ops.combine_groups(recv, s.D, g["out_weight"], g["out_bias"],
                                                                                     0, cnt)
    return out


def _train_op(s, g, tiles, first=None):
    """HEPTAttention.train(): out and every gradient of input A.  ``first`` = inputs B: forward(A), forward(B) on the same
    instance, then backward(A)."""
    from hept_amd import HEPTAttention

    dev = g["q"].device
    prec, tt = TRAIN_OP_TILES[tiles]
    m = HEPTAttention(s.D + s.C, precision=prec, h_dim=s.D, num_heads=s.H, block_size=s.B, n_hashes=s.T, num_w_per_dist=10)
    m.load_state_dict({"out_linear.weight": g["out_weight"], "out_linear.bias": g["out_bias"], "e2lsh.alpha": g["alpha"]})
    m = m.to(dev).train()
    m.train_tiles = tt
    w_rpe = torch.nn.Linear(g["w_rpe_weight"].shape[1], g["w_rpe_weight"].shape[0], device=dev)
    with torch.no_grad():
        w_rpe.weight.copy_(g["w_rpe_weight"])
    q, k, v, coords = (g[x].clone().requires_grad_(True) for x in ("q", "k", "v", "coords"))
    out = m(q, k, v, w_rpe=w_rpe, coords=coords, combined_shifts=g["combined_shifts"])
    if first is not None:
        m(*(first[x].clone().requires_grad_(True) for x in ("q", "k", "v")), w_rpe=w_rpe,
          coords=first["coords"].clone().requires_grad_(True), combined_shifts=first["combined_shifts"])
    out.backward(sw._g_out(out.shape).to(dev))
    return {"out": out.detach(), "grad q": q.grad, "grad k": k.grad, "grad v": v.grad, "grad w_rpe": w_rpe.weight.grad,
            "grad W_out": m.out_linear.weight.grad, "grad b_out": m.out_linear.bias.grad, "grad coords": coords.grad}


def run_train_op(c, g, interleave=False):
    s = sw.BY_ID[c.shape]
    other = None
    if interleave:
        s2 = s._replace(sizes=(s.sizes[0] + s.B,), seed=s.seed + 1)      # another point count, another seed
        other = sw._gpu(sw.inputs(s2), g["q"].device)
    return _train_op(s, g, c.precision, other)


def _train_block(blk, x0, coords0, kwargs_fn, first=None):
    dev = x0.device
    blk = blk.train()
    blk.dropout.p = 0.0
    x = x0.clone().requires_grad_(True)
    coords = coords0.clone().requires_grad_(True)
    y = blk(x, kwargs_fn(coords))
    if first is not None:
        xb, kwb = first
        blk(xb.clone().requires_grad_(True), kwb)
    y.backward(asw._g_out(y.shape).to(dev))
    got = {f"grad {nm}": p.grad for nm, p in blk.named_parameters() if p.grad is not None}
    assert {k[5:] for k in got} == set(asw.GRAD_PARAMS), sorted(got)
    got.update({"y": y.detach(), "grad x": x.grad, "grad coords": coords.grad})
    return got


def run_train_attn(c, g, interleave=False):
    s = asw.BY_ID[c.shape]
    prec, tiles = asw.TRAIN[c.precision]
    dev = g["x"].device
    blk = asw.module(s, {"params": g["params"]}, prec, dev)
    blk.attn.train_tiles = tiles
    first = None
    if interleave:
        s2 = s._replace(sizes=(s.sizes[0] + s.B,), seed=s.seed + 1)
        g2 = asw._gpu(asw.inputs(s2), dev)
        first = (g2["x"], {"coords": g2["coords"].clone().requires_grad_(True), "combined_shifts": g2["combined_shifts"]})
    return _train_block(blk, g["x"], g["coords"], lambda co: {"coords": co, "combined_shifts": g["combined_shifts"]}, first)


def run_train_src(c, g, interleave=False):
    s = ssw.BY_ID[c.shape]
    prec, tiles = asw.TRAIN[c.precision]
    dev = g["x"].device
    blk = ssw.module(s, {"params": g["params"]}, prec, dev)
    blk.attn.train_tiles = tiles
    first = None
    if interleave:
        s2 = s._replace(N=s.N + s.B, raw=s.raw + s.B - 3, seed=s.seed + 1, id=s.id + "-other")
        g2 = ssw._gpu(ssw.inputs(s2), dev)
        first = (g2["x"], ssw.kwargs_of(g2, g2["coords"].clone().requires_grad_(True)))
    return _train_block(blk, g["x"], g["coords"], lambda co: ssw.kwargs_of(g, co), first)


def run_prepare(c, g):
    from hept_amd.prep import prepare_input_hip

    helper = {"block_size": g["block_size"], "num_heads": g["num_heads"], "regions": g["regions"]}
    pad, kw, mask = prepare_input_hip(g["x"], g["coords"], g["batch"], helper)
    return dict(pad_seq=pad, mask=mask, combined_shifts=kw["combined_shifts"], coords=kw["coords"])


def run_prepare_src(c, g):
    from hept_amd.prep import get_regions, prepare_input_src

    s = ssw.BY_ID[c.shape]
    regions = get_regions(max(4, s.N // (2 * s.B)), s.T, H, generator=torch.Generator().manual_seed(s.seed))
    x, coords = g["x"][:s.raw].contiguous(), g["coords"][:s.raw].contiguous()
    x_p, kw = prepare_input_src(x, coords, {"block_size": s.B, "regions": regions.to(x.device)})
    return dict(x=x_p, coords=kw["coords"], eta=kw["region_indices"][0], phi=kw["region_indices"][1], regions_h=kw["regions_h"])


RUN = {"op": run_op, "sort_tables": run_sort_tables, "sort_tables_src": run_sort_tables_src, "argsort": run_argsort,
       "attn": run_attn, "src": run_src, "bwd": run_bwd, "stack": run_stack, "stack_src": run_stack, "partial": run_partial,
       "train_op": run_train_op, "train_attn": run_train_attn, "train_src": run_train_src, "prepare": run_prepare,
       "prepare_src": run_prepare_src}


def _ready(c, dev):
    g = inputs(c, dev)
    if c.entry == "src" and "qkv" not in g:
        g["qkv"] = _qkv(g)
    if c.entry in ("sort_tables", "sort_tables_src"):
        _stage_inputs(c, g)
    if c.entry == "bwd" and "gacc" not in g:
        s = ssw.BY_ID[c.shape]
        g["gacc"] = torch.randn(s.N, H, 32, generator=torch.Generator().manual_seed(s.seed + 7)).to(dev)
    return g


def _run(c, g, ledger=None, **kw):
    if c.entry == "partial":
        return run_partial(c, g, ledger)
    return RUN[c.entry](c, g, **kw)


def _no_pattern_word(nm, t):
    if nm in ("qhat", "kvhat") and t.dtype != torch.float32:
        return True       # 16-bit rows carry an f32 word (the norm term) in their last two columns: bits, not bf16 values
    if nm.startswith(INF_BY_CONTRACT):
        return not bool(torch.isnan(t).any())
    return bool(torch.isfinite(t).all())


def clean(c, dev):
    """The case on untouched allocations, once per session: every returned tensor, and the interleaved gradients' reference."""
    if c.id not in _clean:
        if len(_clean) > 8:
            _clean.clear()
        g = _ready(c, dev)
        res = _run(c, g)
        torch.cuda.synchronize()
        for nm, t in res.items():
            if t.is_floating_point() and not nm.startswith("_"):
                assert _no_pattern_word(nm, t), f"{c.id}: clean {nm} is not finite"
        _clean[c.id] = res
    return _clean[c.id]


def check(c, pattern, dev, note=lambda k, v: None):
    """Assertions (a)-(d) of one case under one pattern; returns the set of allocation sites the case reached."""
    g = _ready(c, dev)
    want = clean(c, dev)
    held = [g] + ([_stage_inputs(c, g)] if c.entry in ("sort_tables", "sort_tables_src") else [])
    snapshot = [(nm, t, t.clone()) for nm, t in _walk(held)]
    pool = None
    if pattern == "leftover":
        d = donor_of(c)
        gd = _ready(d, dev)
        with scratch("record") as donor:
            _run(d, gd, donor)
        donor.check()
        pool = donor.pool
        note("donor", d.id)
    with scratch(pattern, pool) as ledger:
        got = _run(c, g, ledger)
        inter = _run(c, g, interleave=True) if c.entry in INTERLEAVED else None
    ledger.check()                                                            # (b), after a synchronize
    assert set(got) == set(want), (c.id, sorted(set(got) ^ set(want)))
    for nm, t in got.items():                                                 # (a)
        if nm == "_tail":     # the undefined tail of a ragged argsort: never written, so it still holds the pattern
            if pattern in _FILL:
                assert bool((bits(t) == _FILL[pattern]).all()), f"{c.id} {pattern}: the ragged tail of pos was written"
            continue
        if t.is_floating_point():
            assert _no_pattern_word(nm, t), f"{c.id} {pattern}: {nm} holds non-finite words"
        if not same_bits(t, want[nm]):
            diff = (bits(t.reshape(want[nm].shape)) != bits(want[nm])).nonzero()
            raise AssertionError(f"{c.id} {pattern}: {nm} differs from the clean run in {diff.numel()} bytes, first at byte "
                                 f"{int(diff[0])} of {bits(t).numel()}")
    if inter is not None:                                                     # (d)
        for nm, t in inter.items():
            assert same_bits(t, want[nm]), f"{c.id} {pattern}: {nm} of A changes when forward(B) runs before backward(A)"
    for nm, t, before in snapshot:                                            # (c)
        assert same_bits(t, before), f"{c.id} {pattern}: input {nm} was changed by the call"
    return ledger.sites
