"""``AttnStack``: the model's ``n_layers`` Attn blocks as one module on one workspace.

The reference model loops its blocks in Python, keeps every layer's output and feeds their concatenation to ``W``
(``example/transformer.py:119-121``, ``src/models/baselines/transformer.py:133-144``)::

    all_encoded_x = [encoded_x]
    for i in range(self.n_layers):
        encoded_x = self.attns[i](encoded_x, kwargs)
        all_encoded_x.append(encoded_x)
    encoded_x = self.W(torch.cat(all_encoded_x, dim=-1))

``AttnStack(coords_dim, **model_kwargs)`` holds the same ``attns`` (same state-dict keys ``attns.{i}.*``) and its
``forward(x, kwargs)`` returns that concatenation, (N, (n_layers + 1) D).  In eval mode under ``torch.no_grad()`` the
whole loop is ONE C call (``hept_attn_stack_forward``): layer i reads columns [i D, (i+1) D) of the result buffer and
writes columns [(i+1) D, (i+2) D) of the same rows, so there is no ``torch.cat`` and no per-layer (N, D) tensor, and all
layers share one workspace (they run one after the other on one stream) instead of owning one each.  Every other case
(training, gradients, shapes outside the fused block, table sharding, ``torch.compile``) runs the reference loop over
``self.attns``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .attn_block import Attn

__all__ = ["AttnStack"]


class AttnStack(nn.Module):
    def __init__(self, coords_dim, *, precision: str = "fp32", variant: str = "example", **kwargs):
        super().__init__()
        if "n_layers" not in kwargs:
            raise ValueError("hept_amd.AttnStack needs n_layers (the reference model config's key) among its kwargs")
        self.n_layers = int(kwargs["n_layers"])
        if self.n_layers < 1:
            raise ValueError(f"hept_amd.AttnStack: n_layers must be at least 1, got {self.n_layers}")
        self.attns = nn.ModuleList(Attn(coords_dim, precision=precision, variant=variant, **kwargs)
                                   for _ in range(self.n_layers))
        self.precision = precision
        self.variant = variant
        self._workspace = None
        self._ws_stream_ptr = None   # stream of the last forward that used the workspace (HEPTAttention._scratch)
        self._busy = False           # a forward of this instance is being issued (two host threads at once: refused)

    def _scratch(self, nbytes: int, device) -> torch.Tensor:
        ws = self._workspace
        if ws is None or ws.numel() < nbytes or ws.device != device:
            ws = self._workspace = torch.empty(nbytes, device=device, dtype=torch.uint8)
        # one workspace for the whole stack: a forward issued on another stream than the one before it waits for that
        # stream first (the earlier forward may still be reading its rows) -- see HEPTAttention._scratch
        ptr = ops.current_stream_ptr(device)
        last = self._ws_stream_ptr
        if last is not None and last != ptr:
            torch.cuda.current_stream(device).wait_stream(torch.cuda.ExternalStream(last, device=device))
        self._ws_stream_ptr = ptr
        return ws

    def _workspace_bytes(self, n_points: int, n_coords: int) -> int:
        a = self.attns[0].attn
        return ops.workspace_bytes(int(n_points), a.num_heads, a.dim_per_head, int(n_coords), a.n_hashes, a.block_size,
                                   a.precision)

    def reserve(self, n_points: int, n_coords: int, device) -> None:
        """Allocate the stack's one workspace for clouds of up to ``n_points`` (padded) points now, so the first forward
        does not pay for a device allocation; optional -- forward() grows the workspace on demand."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._scratch(self._workspace_bytes(n_points, n_coords), device)

    def _fused_ok(self, x) -> bool:
        return not torch.compiler.is_compiling() and all(layer._fused_ok(x) for layer in self.attns)

    def forward(self, x, kwargs):
        if self._busy:   # (a flag, not a lock: the point is to refuse a second host thread, not to queue it)
            raise RuntimeError("hept_amd.AttnStack: this instance is being called from two threads at once; it owns one "
                               "workspace -- use one instance per thread")
        self._busy = True
        try:
            return self._forward_impl(x, kwargs)
        finally:
            self._busy = False

    def _lend_workspace(self, x, kwargs):
        """Eval, no-grad calls of the composed path: for the duration of this forward the layers (and their operators)
        use the stack's workspace instead of allocating one each -- they run one after the other on the current stream.
        Returns what the layers held before; ``_return_workspace`` puts it back, so the stack's buffer has one owner and
        one stream guard (``_scratch``), and a layer called on its own afterwards behaves as if it had never been in a
        stack."""
        ws = self._scratch(self._workspace_bytes(x.shape[0], kwargs["coords"].shape[1]), x.device)
        held = []
        for layer in self.attns:
            held.append((layer._workspace, layer.attn._workspace, layer.attn._ws_stream_ptr))
            layer._workspace = ws
            layer.attn._workspace = ws
            layer.attn._ws_stream_ptr = self._ws_stream_ptr
        return held

    def _return_workspace(self, held) -> None:
        for layer, (own, op_own, op_stream) in zip(self.attns, held):
            layer._workspace, layer.attn._workspace, layer.attn._ws_stream_ptr = own, op_own, op_stream

    def _forward_impl(self, x, kwargs):
        if not self._fused_ok(x):
            # the reference's loop (example/transformer.py:119-121), block by block
            held = None
            if (x.is_cuda and not self.training and not torch.is_grad_enabled()
                    and not torch.compiler.is_compiling()):
                held = self._lend_workspace(x, kwargs)
            try:
                outs = [x]
                for layer in self.attns:
                    x = layer(x, kwargs)
                    outs.append(x)
                return torch.cat(outs, dim=-1)
            finally:
                if held is not None:
                    self._return_workspace(held)
        first = self.attns[0]
        a = first.attn
        n, d = x.shape[0], first.dim_per_head
        coords = kwargs["coords"]
        buf = torch.empty(n, (self.n_layers + 1) * d, device=x.device, dtype=torch.float32)
        buf[:, :d].copy_(x)   # (widens 16-bit activations on the way)
        ws = self._scratch(self._workspace_bytes(n, coords.shape[1]), x.device)
        common = dict(num_heads=first.num_heads, block_size=a.block_size, w_per_dist=a.num_w_per_dist,
                      eps1=[layer.norm1.eps for layer in self.attns], eps2=[layer.norm2.eps for layer in self.attns],
                      precision=a.precision, workspace=ws)
        params = [layer._block_params() for layer in self.attns]
        if a.variant == "src":
            ops.attn_stack_forward_src(buf, coords.float(), kwargs["region_indices"], kwargs["regions_h"],
                                       kwargs["raw_size"], params, **common)
        else:
            ops.attn_stack_forward(buf, coords.float(), kwargs["combined_shifts"], params, **common)
        return buf if x.dtype is torch.float32 else buf.to(x.dtype)
