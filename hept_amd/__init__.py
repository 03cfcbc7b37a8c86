"""hept_amd — MI355X (gfx950) implementation of HEPT's LSH block-attention hot path.

``HEPTAttention`` is a drop-in for the reference module (``example/hept.py``);
``prepare_input`` mirrors the caller-side preparation (``example/transformer.py``);
``Attn`` is the fused transformer block around the operator (``example/transformer.py:131-165``), ``SrcAttn`` the
same block as the src variant's drop-in (``src/models/baselines/transformer.py:160-229``), ``AttnStack`` the model's
layer loop over such blocks (``example/transformer.py:119-121``) as one call on one workspace.
The compute path is the HIP library ``csrc/libhept_hip.so`` (C ABI in
``include/hept_hip.h``); there is no CPU or eager-PyTorch fallback.
"""
from .attn_block import Attn, SrcAttn
from .attn_stack import AttnStack
from .hept import E2LSH, HEPTAttention
from .prep import (bit_shift, get_regions, pad_and_unpad, prepare_input, prepare_input_hip, prepare_input_src,
                   quantile_partition)

__all__ = [
    "HEPTAttention", "E2LSH", "Attn", "SrcAttn", "AttnStack", "prepare_input", "prepare_input_hip", "prepare_input_src", "get_regions",
    "quantile_partition", "bit_shift", "pad_and_unpad",
]
