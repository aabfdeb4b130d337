"""GPU parity of the general attention kernels' bf16 mode (csrc/attention_x.hip, KANVIT_FLAG_BF16_MFMA, D <= 64): self-attention
heads too long for the one-head-per-work-group kernels (N > 224 at D = 64, N > 256 at D <= 32) run on the bf16 matrix cores under
torch.autocast(bfloat16).  Checked against a float64 oracle with the bf16 kernels' rounding points (written here: it needs causal
masking and a mask, which oracle/kan_oracle.py::_RoundedAttention does not take), at the bounds of
tests/test_bf16_oracle_gpu.py::test_attention_bf16, then at the ABI level (cross-attention, masks), for reproducibility, through
the packed MSA layout, a VisionTransformer and train.main."""
import numpy as np
import pytest
import torch

from oracle import kan_oracle as ko
from tests._util import record_kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIGHT = 2e-3          # max |err| / max |ref| against the rounded oracle
LOOSE = 1e-2          # ||err||_F / ||ref||_F against the unrounded oracle


def fro(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def oracle(q, k, v, do, causal=False, mask=None, rounded=True):
    """float64 attention and its gradients with the rounding points of the bf16 kernels (rounded=True) or none:
    S = r(q) r(k)^T; p = exp(scale S - max) unrounded; o = r(p) r(v) / sum(p);  P = exp(scale S - lse), dP = r(do) r(v)^T,
    delta = rowsum(do * o), dS = P scale (dP - delta); dq = r(dS) r(k), dk = r(dS)^T r(q), dv = r(P)^T r(do).
    mask: bool [B, H, Nq, Nk] (True = attend) or None.  A query with no live key: o = 0 and zero gradients."""
    r = ko.bf16_round if rounded else (lambda t: t)
    q, k, v, do = (t.detach().double().cpu() for t in (q, k, v, do))
    nq, nk, d = q.shape[2], k.shape[2], q.shape[3]
    scale = d ** -0.5
    dead = torch.zeros(nq, nk, dtype=torch.bool)
    if causal:
        dead = torch.arange(nk)[None, :] > torch.arange(nq)[:, None]
    dead = dead.expand(q.shape[0], q.shape[1], nq, nk)
    if mask is not None:
        dead = dead | ~mask.cpu()
    s = (r(q) @ r(k).transpose(-1, -2)) * scale
    s = s.masked_fill(dead, -float("inf"))
    mx = s.amax(dim=-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    p = torch.exp(s - mx)
    lsum = p.sum(dim=-1, keepdim=True)
    live = lsum > 0
    o = torch.where(live, (r(p) @ r(v)) / torch.where(live, lsum, torch.ones_like(lsum)), torch.zeros_like(q))
    lse = torch.log(torch.where(live, lsum, torch.ones_like(lsum))) + mx
    pb = torch.where(dead | ~live, torch.zeros_like(s), torch.exp(s - lse))
    dp = r(do) @ r(v).transpose(-1, -2)
    delta = (do * o).sum(dim=-1, keepdim=True)
    ds = pb * scale * (dp - delta)
    return o, r(ds) @ r(k), r(ds).transpose(-1, -2) @ r(q), r(pb).transpose(-1, -2) @ r(do)


def _autocast_attention(q, k, v, do, causal):
    from kanvit import ops
    qg, kg, vg = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        o = ops.attention(qg, kg, vg, causal=causal)
    o.backward(do.to(DEV))
    return o.detach(), qg.grad, kg.grad, vg.grad


@pytest.mark.parametrize("n,d", [(225, 64), (577, 64), (257, 32), (1025, 16), (300, 40)])
@pytest.mark.parametrize("causal", [False, True])
def test_autocast_attention_of_long_heads_against_rounded_oracle(n, d, causal):
    """ops.attention under bf16 autocast where the general kernels take the head: forward and all three gradients within TIGHT of
    the rounded oracle, and within bf16 noise of -- but not equal to -- the exact result (the strict lower bound: exact fp32 ran
    here before the bf16 twins)."""
    from kanvit import ops
    assert not ops._attn_fits_one_workgroup(n, d)
    torch.manual_seed(n + d)
    b, h = 2, 3
    q, k, v = (torch.randn(b, h, n, d) for _ in range(3))
    do = torch.randn(b, h, n, d)
    with record_kernels() as names:
        got = _autocast_attention(q, k, v, do, causal)
    assert {"attn_x_fwd_bf16_kernel<%d>" % (1 if d <= 32 else 2), "attn_x_bwd_q_bf16_kernel<%d>" % (1 if d <= 32 else 2)} <= names, names
    ref_t = oracle(q, k, v, do, causal)
    ref_e = oracle(q, k, v, do, causal, rounded=False)
    for name, a, bt, be in zip(("o", "dq", "dk", "dv"), got, ref_t, ref_e):
        assert maxrel(a, bt) < TIGHT, (name, maxrel(a, bt))
        assert 1e-5 < fro(a, be) < 1.5 * LOOSE, (name, fro(a, be))


def test_packed_layout_equals_separate_tensors_bitwise():
    """attention_packed (the MSA layout qkv[B, N, 3, H, D]) at N = 577 under autocast: the same bf16 kernels, the same numbers."""
    from kanvit import ops
    torch.manual_seed(7)
    b, n, h, d = 2, 577, 3, 64
    qkv = torch.randn(b, n, 3, h, d, device=DEV)
    do = torch.randn(b, n, h * d, device=DEV)
    x = qkv.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        op = ops.attention_packed(x)
    op.backward(do)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).contiguous().requires_grad_(True) for i in range(3))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        o = ops.attention(q, k, v)
    o.backward(do.view(b, n, h, d).permute(0, 2, 1, 3))
    assert torch.equal(op.view(b, n, h, d).permute(0, 2, 1, 3), o)
    for i, t in enumerate((q, k, v)):
        assert torch.equal(x.grad[:, :, i].permute(0, 2, 1, 3), t.grad), i


def _x_run(q, k, v, do, mask, causal, flags):
    from kanvit import ops
    q, k, v, do = (t.to(DEV) for t in (q, k, v, do))
    o = torch.empty_like(q)
    lse = ops._attn_x_fwd(q, k, v, o, mask, causal, q.shape[3] ** -0.5, flags=flags)
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    ops._attn_x_bwd(q, k, v, o, lse, do, dq, dk, dv, mask, causal, q.shape[3] ** -0.5, flags=flags)
    return o, lse, dq, dk, dv


@pytest.mark.parametrize("nq,nk,d", [(100, 300, 64), (300, 100, 64), (130, 260, 30), (7, 50, 16)])
@pytest.mark.parametrize("kind", ["none", "keypad", "full"])
def test_abi_cross_attention_and_masks(nq, nk, d, kind):
    """_attn_x_fwd / _bwd with FLAG_BF16_MFMA: q_len != k_len both ways, a [B, Nk] key-padding mask and a full [B, H, Nq, Nk]
    mask with one fully masked sample, against the rounded oracle with the mask.  D = 30 takes the unaligned (scalar) fills."""
    from kanvit import _lib
    g = torch.Generator().manual_seed(nq * 3 + nk + d)
    b, h = 2, 3
    q = torch.randn(b, h, nq, d, generator=g)
    k = torch.randn(b, h, nk, d, generator=g)
    v = torch.randn(b, h, nk, d, generator=g)
    do = torch.randn(b, h, nq, d, generator=g)
    mask = None
    if kind == "keypad":
        km = torch.rand(b, nk, generator=g) > 0.35
        km[:, 0] = True
        mask = km.view(b, 1, 1, nk).expand(b, h, nq, nk)
    elif kind == "full":
        mask = torch.rand(b, h, nq, nk, generator=g) > 0.5
        mask[1] = False                                      # sample 1: every query of every head sees no key
    got = _x_run(q, k, v, do, None if mask is None else mask.to(DEV), False, _lib.FLAG_BF16_MFMA)
    o, lse, dq, dk, dv = got
    ref = oracle(q, k, v, do, mask=mask)
    for name, a, r in zip(("o", "dq", "dk", "dv"), (o, dq, dk, dv), ref):
        sel = slice(0, 1) if kind == "full" else slice(None)         # the live sample (sample 1 is all zero: checked below)
        assert maxrel(a[sel], r[sel]) < TIGHT, (name, maxrel(a[sel], r[sel]))
    if kind == "full":
        assert float(o[1].abs().max()) == 0.0 and float(dq[1].abs().max()) == 0.0
        assert float(dk[1].abs().max()) == 0.0 and float(dv[1].abs().max()) == 0.0
        assert bool((lse[1] == -torch.finfo(torch.float32).max).all())
    assert all(bool(torch.isfinite(t).all()) for t in got)
    if kind == "none":                                       # an all-true mask is the same launch without a mask
        ones = torch.ones(b, h, nq, nk, dtype=torch.bool, device=DEV)
        for a, c in zip(got, _x_run(q, k, v, do, ones, False, _lib.FLAG_BF16_MFMA)):
            assert torch.equal(a, c)


def test_abi_fully_masked_query_and_causal():
    """One query with every key masked inside a causal, padded launch: o = 0, lse = -FLT_MAX, zero gradient through it."""
    from kanvit import _lib
    torch.manual_seed(1)
    b, h, n, d = 2, 2, 300, 64
    q, k, v, do = (torch.randn(b, h, n, d) for _ in range(4))
    mask = torch.ones(b, h, n, n, dtype=torch.bool)
    mask[1, 0, 5] = False
    o, lse, dq, dk, dv = _x_run(q, k, v, do, mask.to(DEV), True, _lib.FLAG_BF16_MFMA)
    assert float(o[1, 0, 5].abs().max()) == 0.0 and float(dq[1, 0, 5].abs().max()) == 0.0
    assert float(lse[1, 0, 5]) == -torch.finfo(torch.float32).max
    ref = oracle(q, k, v, do, causal=True, mask=mask)
    for name, a, r in zip(("o", "dq", "dk", "dv"), (o, dq, dk, dv), ref):
        assert maxrel(a, r) < TIGHT, (name, maxrel(a, r))


def test_bf16_general_attention_is_bitwise_reproducible():
    torch.manual_seed(2)
    q, k, v, do = (torch.randn(2, 3, 577, 64) for _ in range(4))
    first = _autocast_attention(q, k, v, do, True)
    second = _autocast_attention(q, k, v, do, True)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("t", ["vanilla", "cheby"])
def test_vit_with_long_sequence_under_bf16_autocast(t):
    """The (1, 32, 32) / 16-patch model of test_vit_with_more_tokens_than_one_workgroup_holds (N = 257, dh = 32) under bf16
    autocast: the attention runs the bf16 twins; logits and gradients within the loose bounds of the bf16 model tests against
    oracle.vit_forward in float64, and different from the same model's fp32 run."""
    from model import VisionTransformer
    torch.manual_seed(5)
    m = VisionTransformer((1, 32, 32), n_patches=16, n_blocks=1, d_hidden=64, n_heads=2, out_d=10, type=t).to(DEV)
    x = torch.rand(3, 1, 32, 32)
    y = torch.arange(3) % 10
    sd = {k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu() for k, v in m.state_dict().items()}
    params = {k: v.clone().requires_grad_(not ko.is_buffer_key(k)) for k, v in sd.items()}
    ref = ko.vit_forward(params, x.double(), 16, 2, t)
    ref_loss = torch.nn.functional.cross_entropy(ref, y)
    ref_loss.backward()
    logits32 = m(x.to(DEV)).detach()
    with record_kernels() as names:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = m(x.to(DEV))
            loss = torch.nn.functional.cross_entropy(logits.float(), y.to(DEV))
        loss.backward()
    assert "attn_x_fwd_bf16_kernel<1>" in names and "attn_x_bwd_kv_bf16_kernel<1>" in names, names
    assert not torch.equal(logits.float(), logits32)
    assert fro(logits.float(), ref.detach()) < 2 * LOOSE, fro(logits.float(), ref.detach())
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < 2e-2
    gmax = max(float(v.grad.norm()) for v in params.values() if v.grad is not None)
    report = []
    for k, p in m.named_parameters():
        g = params[k].grad
        if g is None or p.grad is None or float(g.norm()) < 1e-3 * gmax:
            continue
        a, b = p.grad.detach().double().cpu().flatten(), g.flatten()
        report.append((float(torch.dot(a, b) / (a.norm() * b.norm())), float(a.norm() / b.norm()), k))
    assert min(report)[0] > 0.99, min(report)
    assert all(0.95 < r < 1.05 for _, r, _ in report), [x for x in report if not 0.95 < x[1] < 1.05]


def test_train_main_bf16_with_long_sequence_eager_equals_graph(tmp_path):
    """train.py --amp bf16 at 32 x 32 images in 2 x 2 patches (N = 257): eager and --graph replay bitwise equal, finite loss."""
    import train
    geom = ["--synthetic", "--in-chans", "1", "--image-size", "32", "--n-patches", "16", "--n-blocks", "1", "--n-heads", "2",
            "--d-hidden", "64", "--out-d", "10", "--batch-size", "4", "--amp", "bf16"]
    x, y = torch.rand(4, 1, 32, 32), torch.arange(4) % 10
    runs = []
    for extra in ((), ("--graph",)):
        args = train.parse(["--model-type", "cheby", "--epochs", "1", "--steps-per-epoch", "3", "--no-step-metrics", "--log-dir",
                            str(tmp_path / f"logs{len(runs)}"), "--no-tuned-gemms", *geom, *extra])
        torch.manual_seed(9)
        runs.append(train.main(args, batches=[(x, y)] * 3)["losses"])
    assert runs[0] == runs[1], runs
    assert len(runs[0]) == 3 and all(np.isfinite(runs[0])), runs
