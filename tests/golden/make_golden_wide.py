#!/usr/bin/env python3
"""Generate tests/golden/flash_wide.npz: the reference's own outputs and gradients for attention heads wider than 64, which the
general attention kernels (csrc/attention_x.hip) take up to D = 128.  Imports the REAL reference on the CPU, located as
make_golden.py does (KANVIT_REFERENCE):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide.py

Cases: FlashAttentionFunction at D = 128 and D = 80; at each head size one case combines q_len != k_len with key padding or
with causal (k_len <= q_len), the other is self-attention with the remaining feature.  One MSA (type vanilla) with d_head = 128.
The file stays small: inputs are bf16-representable values stored as bf16 bits, the MSA's parameters are not stored but
filled by det_fill() (the test fills its MSA the same way), and its weight gradients are kept at every WSTRIDE-th element.
Data only; nothing of the reference's source travels."""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = os.environ.get("KANVIT_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np
import torch

from attention import MSA                      # noqa: E402  (reference)
from utils import FlashAttentionFunction       # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
WSTRIDE = 37
torch.set_num_threads(8)


def npy(t):
    return t.detach().cpu().numpy()


def bf16_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


def bf16_bits(t):
    return npy(t.to(torch.bfloat16).view(torch.int16)).astype(np.uint16)


def det_fill(shape, salt):
    """Exact float32 values in [-0.125, 0.125] from integer arithmetic (the same on every host); mirrored in
    tests/test_attention_wide_gpu.py."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    return torch.from_numpy((((i * 7919 + salt * 104729) % 4093 - 2046) / 16384.0).astype(np.float32).reshape(shape))


def gen_flash_wide(blob):
    g = torch.Generator().manual_seed(23)
    cases = {
        # tag: (q_len, k_len, d, causal, key padding, (q_bucket, k_bucket))
        "cross_keypad128": (9, 20, 128, False, True, (4, 8)),
        "causal128": (14, 14, 128, True, False, (512, 1024)),
        "cross_causal80": (19, 11, 80, True, False, (8, 4)),
        "keypad80": (13, 13, 80, False, True, (512, 1024)),
    }
    for tag, (nq, nk, d, causal, keypad, (qb, kb)) in cases.items():
        q = bf16_exact(torch.randn(1, 1, nq, d, generator=g)).requires_grad_(True)
        k = bf16_exact(torch.randn(1, 1, nk, d, generator=g)).requires_grad_(True)
        v = bf16_exact(torch.randn(1, 1, nk, d, generator=g)).requires_grad_(True)
        do = bf16_exact(torch.randn(1, 1, nq, d, generator=g))
        mask = None
        if keypad:
            mask = torch.rand(1, nk, generator=g) > 0.3
            mask[:, 0] = True
        o = FlashAttentionFunction.apply(q, k, v, mask, causal, qb, kb)
        o.backward(do)
        for n, t in (("q", q), ("k", k), ("v", v), ("do", do)):
            blob[f"{tag}.{n}"] = bf16_bits(t)
        blob[f"{tag}.o"], blob[f"{tag}.dq"], blob[f"{tag}.dk"], blob[f"{tag}.dv"] = npy(o), npy(q.grad), npy(k.grad), npy(v.grad)
        blob[f"{tag}.causal"] = np.array(int(causal))
        if mask is not None:
            blob[f"{tag}.mask"] = mask.numpy()


def gen_msa_wide(blob):
    msa = MSA(128, 1, type="vanilla")          # d_head = 128
    with torch.no_grad():
        for salt, (name, p) in enumerate(sorted(msa.named_parameters())):
            p.copy_(det_fill(p.shape, salt))
    x = bf16_exact(torch.randn(2, 8, 128, generator=torch.Generator().manual_seed(17))).requires_grad_(True)
    y = msa(x)
    (y * torch.linspace(-1, 1, y.numel()).reshape(y.shape)).sum().backward()
    blob["msa.x"], blob["msa.y"], blob["msa.grad_x"] = bf16_bits(x), npy(y), npy(x.grad)
    for name, p in msa.named_parameters():
        g = p.grad.reshape(-1)
        blob["msa.grad." + name] = npy(g if p.dim() == 1 else g[::WSTRIDE])


if __name__ == "__main__":
    blob = {}
    gen_flash_wide(blob)
    gen_msa_wide(blob)
    np.savez_compressed(os.path.join(OUT, "flash_wide.npz"), **blob)
    print("flash_wide done")
