#!/usr/bin/env python3
"""Generate tests/golden/base_act.npz: the reference's own outputs and gradients for KANLinear and FastKANLayer with each base
activation the port implements (SiLU as the control), and for small VisionTransformers whose KAN layers were given another
activation after construction.  Imports the REAL reference on the CPU, located as make_golden.py does (KANVIT_REFERENCE):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_act.py

Layers: KANLinear(13, 7) and FastKANLayer(11, 5) on a ragged 3-D input [2, 5, I], loss sum(y * linspace): y, the input gradient
and every parameter gradient.  Models: VisionTransformer((1, 28, 28), 7, 2, 64, 2, 10, type) with nn.GELU() in every KANLinear
('efficientkan') or F.gelu in every FastKANLayer ('fast'), cross-entropy on 4 images: logits, loss and every parameter gradient
at every WSTRIDE-th element.  The file stays small: inputs are bf16-representable values stored as bf16 bits, and trainable
parameters are not stored but filled by det_fill() (the tests fill theirs the same way).  Data only; nothing of the reference's
source travels."""
import functools
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = os.environ.get("KANVIT_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from model import VisionTransformer                 # noqa: E402  (reference)
from models.effkan import KANLinear                 # noqa: E402
from models.fastkan import FastKANLayer             # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
WSTRIDE = 37
torch.set_num_threads(8)

ACTS = {   # name -> (KANLinear's class argument, FastKANLayer's callable)
    "silu": (nn.SiLU, F.silu),
    "gelu": (nn.GELU, F.gelu),
    "gelu-tanh": (functools.partial(nn.GELU, approximate="tanh"), functools.partial(F.gelu, approximate="tanh")),
    "relu": (nn.ReLU, F.relu),
    "tanh": (nn.Tanh, torch.tanh),
    "identity": (nn.Identity, nn.Identity()),
}


def npy(t):
    return t.detach().cpu().numpy()


def bf16_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


def bf16_bits(t):
    return npy(t.to(torch.bfloat16).view(torch.int16)).astype(np.uint16)


def det_fill(shape, salt):
    """Exact float32 values in [-0.125, 0.125] from integer arithmetic (the same on every host); mirrored in
    tests/test_base_activation_gpu.py."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    return torch.from_numpy((((i * 7919 + salt * 104729) % 4093 - 2046) / 16384.0).astype(np.float32).reshape(shape))


def fill(module):
    with torch.no_grad():
        for salt, (name, p) in enumerate(sorted(module.named_parameters())):
            if p.requires_grad:
                p.copy_(det_fill(p.shape, salt))


def gen_layers(blob):
    g = torch.Generator().manual_seed(31)
    for name, (mod_cls, fn) in ACTS.items():
        for kind, layer, i in (("eff", KANLinear(13, 7, base_activation=mod_cls), 13),
                               ("fast", FastKANLayer(11, 5, base_activation=fn), 11)):
            fill(layer)
            x = bf16_exact(torch.randn(2, 5, i, generator=g) * 1.5).requires_grad_(True)
            y = layer(x)
            (y * torch.linspace(-1, 1, y.numel()).reshape(y.shape)).sum().backward()
            tag = f"{kind}.{name}"
            blob[f"{tag}.x"], blob[f"{tag}.y"], blob[f"{tag}.grad_x"] = bf16_bits(x), npy(y), npy(x.grad)
            for pn, p in layer.named_parameters():
                if p.grad is not None:
                    blob[f"{tag}.grad.{pn}"] = npy(p.grad)


def gen_models(blob):
    g = torch.Generator().manual_seed(37)
    for typ in ("efficientkan", "fast"):
        torch.manual_seed(0)
        vit = VisionTransformer((1, 28, 28), 7, 2, 64, 2, 10, typ)
        for m in vit.modules():
            if isinstance(m, KANLinear):
                m.base_activation = nn.GELU()
            elif isinstance(m, FastKANLayer) and m.use_base_update:
                m.base_activation = F.gelu
        fill(vit)
        x = bf16_exact(torch.rand(4, 1, 28, 28, generator=g))
        labels = torch.arange(4) % 10
        logits = vit(x)
        loss = F.cross_entropy(logits, labels)
        loss.backward()
        blob[f"vit.{typ}.x"], blob[f"vit.{typ}.labels"] = bf16_bits(x), npy(labels)
        blob[f"vit.{typ}.logits"], blob[f"vit.{typ}.loss"] = npy(logits), npy(loss)
        for pn, p in vit.named_parameters():
            if p.grad is not None:
                gr = p.grad.reshape(-1)
                blob[f"vit.{typ}.grad.{pn}"] = npy(gr if gr.numel() <= 64 else gr[::WSTRIDE])


if __name__ == "__main__":
    blob = {}
    gen_layers(blob)
    gen_models(blob)
    np.savez_compressed(os.path.join(OUT, "base_act.npz"), **blob)
    print("base_act done", len(blob))
