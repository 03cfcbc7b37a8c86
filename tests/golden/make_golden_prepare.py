"""Reference anchors of the prepare_input edge sweep (tests/prepare_sweep.py), made by running the REAL reference.

Run once where the reference checkout exists (``python tests/golden/make_golden_prepare.py``), as make_golden_codes.py
and make_golden_src.py are.  For every case of the sweep that is not refused it runs

* the reference's own ``prepare_input`` (example/transformer.py:35-63), or
* the src variant's caller-side statements (src/models/baselines/transformer.py:43-57, replayed with the reference's
  helper functions by ``make_golden_src.reference_prepare``)

on the case's seeded inputs and stores, in one small file ``tests/golden/prepare_sweep.npz``: a SHA-256 row digest of
the reference's ``combined_shifts`` (of the float region ids for src) on the real points whose eta and phi are unique in
their cloud, those rows' sums and maxima, the mask itself, ``unpad_seq``, the sorted (table 0, head 0) codes of the pad
slots per cloud, a digest of row 0 on all real points and a checksum of the inputs.  For the refused cases it stores
what the reference raised.  Digests and small integer arrays only; tests read the committed file.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import prepare_sweep as ps  # noqa: E402
from make_golden import import_reference  # noqa: E402
import make_golden_src  # noqa: E402


def main():
    _, _, transformer = import_reference()
    _, hash_utils = make_golden_src.import_reference()
    stored = {}
    for case in ps.CASES:
        inp = ps.build(case)
        pre = case.id + "/"
        stored[pre + "input"] = ps.input_checksum(inp)
        if case.path == "src":
            _, kw = make_golden_src.reference_prepare(hash_utils, inp["x"], inp["coords"].clone(), inp["B"], inp["regions"])
            got = ps.anchors_src(inp, *kw["region_indices"])
            n_mask = int(ps.unique_mask(inp).sum())
            print(f"{case.id}: N = {kw['coords'].shape[0]}, {n_mask} of {inp['raw']} real points unique in eta and phi")
        else:
            helper = {"block_size": inp["B"], "num_heads": inp["H"], "regions": inp["regions"]}
            try:
                x_p, kw, unpad = transformer.prepare_input(inp["x"], inp["coords"], inp["batch"].long(), helper)
            except Exception as e:  # noqa: BLE001 -- what the reference raises is the record
                stored[pre + "raised"] = np.array([type(e).__name__, str(e)])
                print(f"{case.id}: the reference raises {type(e).__name__}: {e}")
                continue
            if case.a.refuse:
                stored[pre + "raised"] = np.array(["", ""])   # refused by this project's own limit only
            got = ps.anchors_example(inp, kw["combined_shifts"], x_p, unpad)
            assert torch.equal(kw["coords"], inp["coords"][x_p]) and kw["coords"].dtype == inp["coords"].dtype
            n_mask = int(ps.unique_mask(inp).sum())
            print(f"{case.id}: n_pad = {unpad.numel()}, {n_mask} of {inp['n_raw']} real points unique in eta and phi")
        for key, val in got.items():
            stored[pre + key] = val
    path = os.path.join(HERE, "prepare_sweep.npz")
    ps.save_golden(path, stored)
    print(f"{path}: {os.path.getsize(path) / 1e3:.1f} kB, {len(ps.CASES)} cases")


if __name__ == "__main__":
    main()
