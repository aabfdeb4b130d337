"""Single-query attention (kanvit_attn_q1_fwd / _bwd through kanvit.ops.attention_q1): one query per (sample, head) against the
k and v halves of a packed kv[B, N, 2, H, D], which the kernels read in place; dk and dv come back in one packed tensor of the
same layout and are checked there.

Reference: softmax attention in float64 torch.  Tolerances are the project's: forward 2e-5 (of max(1, max|ref|)), gradients 1e-4
normwise (tests/_util.rel_err).  The arithmetic is plain fp32 sums of at most N = 300 products, so both are far away."""
import functools

import pytest
import torch

from tests._util import max_err, record_kernels, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, H, N, D): the smallest shape, train.py's geometry, the MNIST geometry, the headline head, a full tile multiple, the widest
# head with N several times the 16 lane groups x lanes; then D % 4 != 0 (8-byte row pieces) -- the 16-byte form takes the others
CASES = [(1, 1, 1, 2), (3, 2, 17, 8), (2, 2, 50, 32), (2, 3, 197, 64), (2, 12, 208, 64), (1, 2, 300, 128), (2, 2, 19, 6)]


def _inputs(case, spike=False, misaligned=False):
    B, H, N, D = case
    g = torch.Generator().manual_seed(1000 * N + D + (7 if spike else 0))
    q0 = torch.randn(B, H, D, generator=g)
    kv = torch.randn(B, N, 2, H, D, generator=g)
    do = torch.randn(B, H, D, generator=g)
    scale = D ** -0.5
    if spike:
        # every key gets a component along its query worth a logit of +40, key 5 one worth +100: the softmax is one-hot up to
        # e^-60, and exp() of a raw score would overflow fp32 (e^100) where the maximum is not subtracted first
        unit = q0 / (q0 * q0).sum(-1, keepdim=True)                       # scale * q0 . (c * unit / scale) = c
        kv[:, :, 0] = 0.1 * kv[:, :, 0] + (40.0 / scale) * unit.unsqueeze(1)
        kv[:, 5, 0] = (100.0 / scale) * unit
    if misaligned:
        # the same values one float off the 8-byte grid: contiguous, so the kernels read this very buffer (4-byte row pieces)
        buf = torch.empty(kv.numel() + 1, device=DEV)
        kvd = buf[1:].view(kv.shape)
        kvd.copy_(kv)
        assert kvd.is_contiguous() and kvd.data_ptr() % 8 == 4
    else:
        kvd = kv.to(DEV)
    return q0, kv, do, scale, kvd


@functools.lru_cache(maxsize=None)
def _reference(case, spike=False):
    """o, p, dq0, dkv of sum(o * do) in float64 (computed once per case, shared by the tests below, never modified)."""
    q0, kv, do, scale, _ = _inputs(case, spike)
    q = q0.double().requires_grad_(True)
    kvr = kv.double().requires_grad_(True)
    k, v = kvr[:, :, 0].permute(0, 2, 1, 3), kvr[:, :, 1].permute(0, 2, 1, 3)          # [B, H, N, D]
    p = torch.softmax(scale * torch.einsum("bhd,bhnd->bhn", q, k), dim=-1)
    o = torch.einsum("bhn,bhnd->bhd", p, v)
    (o * do.double()).sum().backward()
    return o.detach(), p.detach(), q.grad, kvr.grad


def _run(case, spike=False, misaligned=False):
    from kanvit import ops
    q0, _, do, scale, kvd = _inputs(case, spike, misaligned)
    q = q0.to(DEV).requires_grad_(True)
    kvd = kvd.requires_grad_(True)
    o = ops.attention_q1(q, kvd, scale)
    (o * do.to(DEV)).sum().backward()
    return o.detach(), q.grad, kvd.grad


def _check(case, got, spike=False):
    o, dq, dkv = (t.cpu() for t in got)
    ro, _, rdq, rdkv = _reference(case, spike)
    B, H, N, D = case
    assert tuple(o.shape) == (B, H, D) and tuple(dq.shape) == (B, H, D) and tuple(dkv.shape) == (B, N, 2, H, D)
    e = max_err(o, ro) / max(1.0, float(ro.abs().max()))
    eq, ek, ev = rel_err(dq, rdq), rel_err(dkv[:, :, 0], rdkv[:, :, 0]), rel_err(dkv[:, :, 1], rdkv[:, :, 1])
    print(f"attention_q1 {case} spike={spike}: o {e:.2e} dq0 {eq:.2e} dk {ek:.2e} dv {ev:.2e}")
    assert e <= 2e-5, (case, e)
    assert eq <= 1e-4 and ek <= 1e-4 and ev <= 1e-4, (case, eq, ek, ev)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_attention_q1_against_float64_softmax(case):
    _check(case, _run(case))


def test_attention_q1_score_spike_needs_the_maximum_subtracted():
    case = (2, 3, 197, 64)
    _, rp, _, _ = _reference(case, True)
    assert float(rp[:, :, 5].min()) >= 1.0 - 1e-12                      # the reference itself is one-hot on the spiked key
    got = _run(case, spike=True)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    _check(case, got, spike=True)


def test_attention_q1_operands_off_the_8_byte_grid():
    """k and v start 4 bytes off the 8-byte grid: the scalar-load form runs, on the caller's buffer, with the same results."""
    case = (2, 3, 197, 64)
    with record_kernels() as names:
        got = _run(case, misaligned=True)
    assert {"attn_q1_fwd_kernel<1>", "attn_q1_bwd_kernel<1>"} <= names, names
    _check(case, got)


def test_attention_q1_row_piece_follows_the_head_size():
    with record_kernels() as names:
        _run((2, 3, 197, 64))
    assert {"attn_q1_fwd_kernel<4>", "attn_q1_bwd_kernel<4>"} <= names, names
    with record_kernels() as names:
        _run((2, 2, 19, 6))
    assert {"attn_q1_fwd_kernel<2>", "attn_q1_bwd_kernel<2>"} <= names, names


@pytest.mark.parametrize("case", [(2, 3, 197, 64), (1, 2, 300, 128), (3, 2, 17, 8)], ids=lambda c: "-".join(map(str, c)))
def test_attention_q1_is_bitwise_reproducible(case):
    a, b = _run(case), _run(case)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_attention_q1_empty_batch_launches_nothing():
    from kanvit import ops
    q = torch.zeros(0, 3, 64, device=DEV, requires_grad=True)
    kv = torch.zeros(0, 197, 2, 3, 64, device=DEV, requires_grad=True)
    with record_kernels() as names:
        torch.zeros(4, device=DEV).add_(1.0)                             # the recorder wants to see a kernel
        o = ops.attention_q1(q, kv)
        o.sum().backward()
    assert tuple(o.shape) == (0, 3, 64) and tuple(q.grad.shape) == (0, 3, 64) and tuple(kv.grad.shape) == (0, 197, 2, 3, 64)
    assert not [n for n in names if n.startswith("attn_q1")], names


@pytest.mark.parametrize("D", [3, 130])
def test_attention_q1_refuses_odd_and_oversized_heads(D):
    from kanvit import _lib, ops
    q = torch.randn(2, 2, D, device=DEV)
    kv = torch.randn(2, 9, 2, 2, D, device=DEV)
    with pytest.raises(_lib.KanvitError, match=r"code -22.*kanvit_attn_q1_fwd: D=%d must be even and <= 128" % D):
        ops.attention_q1(q, kv)
