"""Event-timed general attention kernels (csrc/attention_x.hip) next to the tuned ViT kernels: python tools/time_attn_x.py
Prints ms and algorithmic TFLOP/s (forward 2 products, backward 5) for self-attention at N = 197 (both kernel families) and at lengths only
the chunked kernels take (N = 577: ViT-B/16 at 384 x 384), then heads wider than 64, which only the general kernels take (ViT-H/14:
D = 80 at N = 257; D = 128 at N = 197; N = 577 at D = 64 and at D = 128 side by side).  Heads of D <= 64 also run in bf16 mode
(KANVIT_FLAG_BF16_MFMA: the ViT kernels' bf16 forms, the general kernels' bf16 twins), timed interleaved with the exact fp32 form
(ROUNDS alternating rounds, median of each), plus causal at N = 577."""
import os
import sys
R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(R, 'kan-vit_amd'))
import torch
from kanvit import ops


def run(fn, n_it=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n_it):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n_it


SHAPES = ((128, 12, 197, 64, False, False), (128, 12, 197, 64, True, False), (32, 12, 577, 64, True, False),
          (32, 12, 577, 64, True, True), (8, 12, 1025, 64, True, False), (32, 16, 257, 80, True, False), (128, 6, 197, 128, True, False),
          (32, 12, 577, 128, True, False))
ROUNDS = 5
BF = ops._lib.FLAG_BF16_MFMA
for (B, H, N, D, general, causal) in SHAPES:
    q, k, v = (torch.randn(B, H, N, D, device="cuda") for _ in range(3))
    o = torch.empty_like(q)
    do = torch.randn_like(q)
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    sc = D ** -0.5
    modes = (0, BF) if D <= 64 else (0,)
    times = {m: ([], []) for m in modes}
    for _ in range(ROUNDS):
        for m in modes:
            if general:
                f = lambda: ops._attn_x_fwd(q, k, v, o, None, causal, sc, flags=m)
                lse = f()
                b = lambda: ops._attn_x_bwd(q, k, v, o, lse, do, dq, dk, dv, None, causal, sc, flags=m)
            else:
                f = lambda: ops._attn_fwd(q, k, v, o, causal, sc, m)
                lse = f()
                b = lambda: ops._attn_bwd(q, k, v, o, lse, do, dq, dk, dv, causal, sc, m)
            times[m][0].append(run(f))
            times[m][1].append(run(b))
    fl = 4.0 * B * H * N * N * D * (0.5 if causal else 1.0)
    line = f"{'general' if general else 'ViT    '} B={B} H={H} N={N} D={D}{' causal' if causal else ''}:"
    med = {m: (sorted(t[0])[ROUNDS // 2], sorted(t[1])[ROUNDS // 2]) for m, t in times.items()}
    for m, (tf, tb) in med.items():
        line += f"  {'bf16' if m else 'fp32'} fwd {tf:.3f} ms ({fl / tf / 1e9:.1f} TF/s) bwd {tb:.3f} ms ({2.5 * fl / tb / 1e9:.1f} TF/s)"
    if BF in med:
        line += f"  bf16 speed-up fwd {med[0][0] / med[BF][0]:.2f}x bwd {med[0][1] / med[BF][1]:.2f}x"
    print(line, flush=True)
