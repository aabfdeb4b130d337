#!/usr/bin/env python3
"""Generate tests/golden/attention_map.npz: the reference's own attention maps, as a forward hook on MSA.softmax collects them
(attention.py:199 calls the module once per sample and head, sample-major).  Imports the REAL reference on the CPU, located as
make_golden.py does (KANVIT_REFERENCE):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attention_map.py

Reference MSA(16, 2, type=t) for t in vanilla, cheby, fast on one [3, 5, 16] input; the hook's 6 [5, 5] matrices are stacked to
[3, 2, 5, 5].  The parameters are not stored: every trainable one is filled by det_fill() in name order (the test fills its MSA
the same way); the input is bf16-representable and stored as bf16 bits.  Data only; nothing of the reference's source travels."""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = os.environ.get("KANVIT_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np
import torch

from attention import MSA                      # noqa: E402  (reference)

OUT = os.path.dirname(os.path.abspath(__file__))
TYPES = ["vanilla", "cheby", "fast"]
torch.set_num_threads(8)


def det_fill(shape, salt):
    """Exact float32 values in [-0.5, 0.5] from integer arithmetic (the same on every host); mirrored in
    tests/test_attention_map_gpu.py."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    return torch.from_numpy((((i * 7919 + salt * 104729) % 4093 - 2046) / 4096.0).astype(np.float32).reshape(shape))


if __name__ == "__main__":
    x = torch.randn(3, 5, 16, generator=torch.Generator().manual_seed(29)).to(torch.bfloat16)
    blob = {"x": x.view(torch.int16).numpy().astype(np.uint16)}
    for t in TYPES:
        msa = MSA(16, 2, type=t)
        with torch.no_grad():
            for salt, (name, p) in enumerate(sorted((n, p) for n, p in msa.named_parameters() if p.requires_grad)):
                p.copy_(det_fill(p.shape, salt))
        seen = []
        hook = msa.softmax.register_forward_hook(lambda mod, args, out: seen.append(out.detach().clone()))
        with torch.no_grad():
            msa(x.float())
        hook.remove()
        assert len(seen) == 6 and all(tuple(s.shape) == (5, 5) for s in seen)
        blob[t + ".maps"] = torch.stack(seen).reshape(3, 2, 5, 5).numpy()
    np.savez_compressed(os.path.join(OUT, "attention_map.npz"), **blob)
    print("attention_map done")
