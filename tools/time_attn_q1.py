"""Event-timed single-query attention (kanvit_attn_q1_*, csrc/attention_x.hip) next to the general q_len != k_len kernels on the
same problem: python tools/time_attn_q1.py [B H N D]
One query per (sample, head) against N keys at the headline head (128, 12, 197, 64) by default.  Both routes read the k and v
halves of one packed kv[B, N, 2, H, D] in place.  ROUNDS alternating rounds, median of each; the single-query lines also give
the HBM rate over the bytes the pass has to move (forward: k and v read once; backward: k, v read and dk, dv written)."""
import os
import sys
R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(R, 'kan-vit_amd'))
import ctypes as C

import torch
from kanvit import _lib, ops


def run(fn, n_it=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n_it):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n_it


B, H, N, D = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (128, 12, 197, 64)
ROUNDS = 5
sc = D ** -0.5
q0 = torch.randn(B, H, D, device="cuda")
kv = torch.randn(B, N, 2, H, D, device="cuda")
do = torch.randn(B, H, D, device="cuda")
o, dq = torch.empty_like(q0), torch.empty_like(q0)
p = torch.empty(B, H, N, device="cuda")
dkv = torch.empty_like(kv)
d, e = ops._attn_q1_desc(q0, kv, o, sc)
L = _lib.lib()
P, st = ops._ptr, ops._stream


def q1_fwd():
    _lib.check(L.kanvit_attn_q1_fwd(C.byref(d), C.byref(e), P(q0), P(kv[:, :, 0]), P(kv[:, :, 1]), P(o), P(p), st()), "q1_fwd")


def q1_bwd():
    _lib.check(L.kanvit_attn_q1_bwd(C.byref(d), C.byref(e), P(q0), P(kv[:, :, 0]), P(kv[:, :, 1]), P(o), P(p), P(do), P(dq), P(dkv[:, :, 0]),
                                    P(dkv[:, :, 1]), st()), "q1_bwd")


# the general route on the same operands: q, o, do, dq as [B, H, 1, D]; k, v, dk, dv as [B, H, N, D] views of the packed tensors
q4, o4, do4, dq4 = (t.view(B, H, 1, D) for t in (q0, torch.empty_like(q0), do, torch.empty_like(q0)))
k4, v4, dk4, dv4 = (t[:, :, i].permute(0, 2, 1, 3) for t in (kv, torch.empty_like(kv)) for i in range(2))
lse = ops._attn_x_fwd(q4, k4, v4, o4, None, False, sc)


def x_fwd():
    ops._attn_x_fwd(q4, k4, v4, o4, None, False, sc)


def x_bwd():
    ops._attn_x_bwd(q4, k4, v4, o4, lse, do4, dq4, dk4, dv4, None, False, sc)


q1_fwd()
times = {f.__name__: [] for f in (q1_fwd, x_fwd, q1_bwd, x_bwd)}
for _ in range(ROUNDS):
    for f in (q1_fwd, x_fwd, q1_bwd, x_bwd):
        times[f.__name__].append(run(f))
med = {n: sorted(t)[ROUNDS // 2] for n, t in times.items()}
kv_bytes = 4 * 2 * B * H * N * D
print(f"B={B} H={H} N={N} D={D}: k and v hold {kv_bytes / 1e6:.1f} MB")
print(f"  forward   single-query {med['q1_fwd'] * 1e3:8.1f} us ({kv_bytes / med['q1_fwd'] / 1e6:7.1f} GB/s over {kv_bytes / 1e6:.0f} MB)   "
      f"general {med['x_fwd'] * 1e3:8.1f} us   ratio {med['x_fwd'] / med['q1_fwd']:.2f}x")
print(f"  backward  single-query {med['q1_bwd'] * 1e3:8.1f} us ({2 * kv_bytes / med['q1_bwd'] / 1e6:7.1f} GB/s over {2 * kv_bytes / 1e6:.0f} MB)   "
      f"general {med['x_bwd'] * 1e3:8.1f} us   ratio {med['x_bwd'] / med['q1_bwd']:.2f}x")
print("  rounds (us): " + "  ".join(f"{n} {[round(t * 1e3, 1) for t in ts]}" for n, ts in times.items()), flush=True)
