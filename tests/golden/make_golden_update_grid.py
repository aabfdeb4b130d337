#!/usr/bin/env python3
"""Generate tests/golden/update_grid.npz: the reference's own KANLinear.update_grid (models/effkan.py:189-242) on two layers.
Imports the REAL reference on the CPU, located as make_golden.py does (KANVIT_REFERENCE):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_update_grid.py

For (M, in, out, grid_size, spline_order) = (512, 8, 8, 5, 3) and (300, 6, 7, 8, 2), x ~ randn: x (bf16-representable values
stored as bf16 bits), the layer's initial state_dict, the reference's `grid` and `spline_weight` after update_grid(x), and its
forward output on x before and after, at every YSTRIDE-th row (the file stays small).  Data only; nothing of the reference's
source travels."""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = os.environ.get("KANVIT_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np
import torch

from models.effkan import KANLinear                 # noqa: E402  (reference)

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = {"a": (512, 8, 8, 5, 3), "b": (300, 6, 7, 8, 2)}
YSTRIDE = 2
torch.set_num_threads(8)


def npy(t):
    return t.detach().cpu().numpy()


def bf16_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


def bf16_bits(t):
    return npy(t.to(torch.bfloat16).view(torch.int16)).astype(np.uint16)


if __name__ == "__main__":
    blob = {}
    for salt, (tag, (m, i, o, gs, order)) in enumerate(CASES.items()):
        torch.manual_seed(41 + salt)
        layer = KANLinear(i, o, grid_size=gs, spline_order=order)
        x = bf16_exact(torch.randn(m, i))
        blob[f"{tag}.cfg"] = np.array([m, i, o, gs, order], dtype=np.int64)
        blob[f"{tag}.x"] = bf16_bits(x)
        for k, v in layer.state_dict().items():
            blob[f"{tag}.sd.{k}"] = npy(v).copy()
        with torch.no_grad():
            blob[f"{tag}.y_before"] = npy(layer(x)[::YSTRIDE])
            layer.update_grid(x)
            blob[f"{tag}.y_after"] = npy(layer(x)[::YSTRIDE])
        blob[f"{tag}.grid_after"] = npy(layer.grid).copy()
        blob[f"{tag}.spline_weight_after"] = npy(layer.spline_weight).copy()
        print(tag, "max |y_after - y_before|", float(np.abs(blob[f"{tag}.y_after"] - blob[f"{tag}.y_before"]).max()))
    path = os.path.join(OUT, "update_grid.npz")
    np.savez_compressed(path, **blob)
    print("update_grid done", len(blob), os.path.getsize(path), "bytes")
