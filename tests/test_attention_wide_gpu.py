"""GPU parity of attention heads wider than 64 (64 < D <= 128): the DT = 3, 4 forms of the general kernels (csrc/attention_x.hip)
against the float64 oracle and the reference's own outputs (tests/golden/flash_wide.npz), through every layer that reaches them --
FlashAttentionFunction, ops.attention / attention_packed, the FlashAttention module, MSA, VisionTransformer and train.main."""
import numpy as np
import pytest
import torch

from oracle import kan_oracle as ko
from tests._util import T, bf16_bits_to_f32, close, grads_from, load_npz, max_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("nq,nk", [(1, 1), (7, 50), (50, 7), (130, 97), (197, 197), (257, 257), (577, 577), (300, 700)])
@pytest.mark.parametrize("d", [66, 80, 96, 128])
@pytest.mark.parametrize("kind", ["none", "keypad", "full_heads", "causal", "causal_keypad"])
def test_wide_general_attention_against_fp64_oracle(nq, nk, d, kind):
    """Ragged tiles on both sides, several 128-row chunks, padded head columns (66, 80 pad to 96), (b, n) key padding and
    (b, h, q, k) masks: forward and all three gradients against the float64 oracle, bitwise run to run."""
    from utils import FlashAttentionFunction
    causal = kind.startswith("causal")
    if causal and nk > nq:
        pytest.skip("causal with k_len > q_len is refused (ill-defined in the reference)")
    g = torch.Generator().manual_seed(nq * 131 + nk * 7 + d)
    b, h = 2, 3
    q = torch.randn(b, h, nq, d, generator=g) * 1.3
    k = torch.randn(b, h, nk, d, generator=g) * 1.3
    v = torch.randn(b, h, nk, d, generator=g)
    do = torch.randn(b, h, nq, d, generator=g)
    mask = None
    if kind in ("keypad", "causal_keypad"):
        mask = torch.rand(b, nk, generator=g) > 0.35
        mask[:, 0] = True
    elif kind == "full_heads":
        mask = torch.rand(b, h, nq, nk, generator=g) > 0.5
        mask[..., 0] = True
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref, _ = ko.attention_reference(qd, kd, vd, causal=causal, mask=mask)
    o_ref.backward(do.double())
    outs = []
    for _ in range(2):
        qg, kg, vg = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
        o = FlashAttentionFunction.apply(qg, kg, vg, None if mask is None else mask.to(DEV), causal, 512, 1024)
        o.backward(do.to(DEV))
        outs.append((o.detach(), qg.grad, kg.grad, vg.grad))
    assert max_err(outs[0][0].cpu(), o_ref) < 1e-5
    assert close(outs[0][1], qd.grad) and close(outs[0][2], kd.grad) and close(outs[0][3], vd.grad)
    for a_, b_ in zip(outs[0], outs[1]):
        assert torch.equal(a_, b_)


def test_wide_fully_masked_query_gives_zero():
    """A query with every key masked: o = 0, lse = -FLT_MAX, no gradient through it."""
    from kanvit import ops
    torch.manual_seed(1)
    b, h, nq, nk, d = 2, 2, 40, 70, 128
    q, k, v = (torch.randn(b, h, n, d, device=DEV) for n in (nq, nk, nk))
    mask = torch.ones(b, h, nq, nk, dtype=torch.bool, device=DEV)
    mask[1, 0, 5] = False
    mask[0, 1] = False
    o = torch.empty_like(q)
    lse = ops._attn_x_fwd(q, k, v, o, mask, False, d ** -0.5)
    assert float(o[1, 0, 5].abs().max()) == 0.0 and float(o[0, 1].abs().max()) == 0.0
    assert float(lse[1, 0, 5]) == -torch.finfo(torch.float32).max and bool((lse[0, 1] == -torch.finfo(torch.float32).max).all())
    do = torch.randn_like(o)
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    ops._attn_x_bwd(q, k, v, o, lse, do, dq, dk, dv, mask, False, d ** -0.5)
    assert float(dq[1, 0, 5].abs().max()) == 0.0 and float(dq[0, 1].abs().max()) == 0.0
    assert float(dk[0, 1].abs().max()) == 0.0 and float(dv[0, 1].abs().max()) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in (o, dq, dk, dv))


@pytest.mark.parametrize("n", [17, 197, 257])
@pytest.mark.parametrize("d", [80, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_wide_self_attention(n, d, causal):
    """ops.attention and the packed q|k|v form MSA uses, at head sizes the ViT kernels do not take: routed to the general kernels
    in the forward and the backward alike."""
    from kanvit import ops
    torch.manual_seed(n + d)
    b, h = 2, 2
    q, k, v = (torch.randn(b, h, n, d) * 1.2 for _ in range(3))
    do = torch.randn(b, h, n, d)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref, _ = ko.attention_reference(qd, kd, vd, causal=causal)
    o_ref.backward(do.double())
    qg, kg, vg = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    o = ops.attention(qg, kg, vg, causal=causal)
    o.backward(do.to(DEV))
    assert max_err(o.cpu(), o_ref) < 1e-5
    assert close(qg.grad, qd.grad) and close(kg.grad, kd.grad) and close(vg.grad, vd.grad)
    qkv = torch.stack([q, k, v], dim=0).permute(1, 3, 0, 2, 4).contiguous().to(DEV).requires_grad_(True)      # [B, N, 3, H, D]
    op = ops.attention_packed(qkv, causal=causal)                   # o[B, N, H*D]
    op.backward(do.permute(0, 2, 1, 3).reshape(b, n, h * d).to(DEV))
    assert max_err(op.reshape(b, n, h, d).permute(0, 2, 1, 3).cpu(), o_ref) < 1e-5
    dqkv = qkv.grad.cpu()
    for i, ref in enumerate((qd.grad, kd.grad, vd.grad)):
        assert close(dqkv[:, :, i].permute(0, 2, 1, 3), ref)


def test_wide_packed_attention_under_bf16_autocast_runs_the_exact_kernels():
    """The general kernels are exact fp32: under bf16 autocast D = 128 takes them without the bf16 flag, bitwise as without."""
    from kanvit import ops
    torch.manual_seed(4)
    qkv = torch.randn(2, 197, 3, 2, 128, device=DEV)
    do = torch.randn(2, 197, 256, device=DEV)
    res = []
    for amp in (False, True):
        x = qkv.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            o = ops.attention_packed(x)
        o.backward(do)
        res.append((o.detach().float(), x.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_wide_flash_attention_module_with_context_and_mask():
    """FlashAttention(dim_head=128) with context= and mask= (attention.py:59-109) against the same computation in float64."""
    from attention import FlashAttention
    torch.manual_seed(3)
    H, dh = 2, 128
    m = FlashAttention(dim=96, heads=H, dim_head=dh).to(DEV)
    x = torch.randn(2, 21, 96, device=DEV, requires_grad=True)
    ctxt = torch.randn(2, 77, 96, device=DEV, requires_grad=True)
    mask = torch.rand(2, 77, device=DEV) > 0.3
    mask[:, 0] = True
    y = m(x, context=ctxt, mask=mask)
    y.square().sum().backward()
    W = {n: p.detach().cpu().double() for n, p in m.named_parameters()}
    xd, cd = x.detach().cpu().double().requires_grad_(True), ctxt.detach().cpu().double().requires_grad_(True)
    qd = (xd @ W["to_q.weight"].T).view(2, 21, H, dh).permute(0, 2, 1, 3)
    kd, vd = ((cd @ W["to_kv.weight"].T).chunk(2, dim=-1)[i].reshape(2, 77, H, dh).permute(0, 2, 1, 3) for i in range(2))
    od, _ = ko.attention_reference(qd, kd, vd, mask=mask.cpu())
    yd = od.permute(0, 2, 1, 3).reshape(2, 21, H * dh) @ W["to_out.weight"].T
    yd.square().sum().backward()
    assert rel_err(y.detach().cpu(), yd.detach()) < 1e-5
    assert rel_err(x.grad.cpu(), xd.grad) < 1e-4 and rel_err(ctxt.grad.cpu(), cd.grad) < 1e-4


WIDE_CASES = ["cross_keypad128", "causal128", "cross_causal80", "keypad80"]
WSTRIDE = 37         # make_golden_wide.py keeps every WSTRIDE-th element of each weight gradient


def _det_fill(shape, salt):
    """tests/golden/make_golden_wide.py::det_fill: exact float32 values from integer arithmetic."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    return torch.from_numpy((((i * 7919 + salt * 104729) % 4093 - 2046) / 16384.0).astype(np.float32).reshape(shape))


@pytest.mark.parametrize("tag", WIDE_CASES)
def test_wide_flash_function_against_reference_fixture(tag):
    """FlashAttentionFunction at D = 128 and 80 against the reference's own outputs and gradients (tests/golden/flash_wide.npz,
    make_golden_wide.py): q_len != k_len with key padding or causal, self-attention with causal or key padding."""
    from utils import FlashAttentionFunction
    f = load_npz("flash_wide.npz")
    q, k, v = (bf16_bits_to_f32(f[f"{tag}.{n}"]).to(DEV).requires_grad_(True) for n in ("q", "k", "v"))
    do = bf16_bits_to_f32(f[f"{tag}.do"]).to(DEV)
    causal = bool(int(f[f"{tag}.causal"]))
    mask = torch.from_numpy(f[f"{tag}.mask"]).to(DEV) if f"{tag}.mask" in f else None
    o = FlashAttentionFunction.apply(q, k, v, mask, causal, 512, 1024)
    o.backward(do)
    assert max_err(o.cpu(), T(f[f"{tag}.o"])) < 5e-6
    assert max_err(q.grad.cpu(), T(f[f"{tag}.dq"])) < 2e-5
    assert max_err(k.grad.cpu(), T(f[f"{tag}.dk"])) < 2e-5
    assert max_err(v.grad.cpu(), T(f[f"{tag}.dv"])) < 2e-5


def test_wide_msa_against_reference_fixture():
    """MSA(128, 1): d_head = 128 against the reference's MSA (tests/golden/flash_wide.npz).  The parameters are not stored: both
    sides fill them with _det_fill; the weight gradients are compared at every WSTRIDE-th element, the bias gradients whole."""
    from attention import MSA
    blob = load_npz("flash_wide.npz")
    msa = MSA(128, 1, type="vanilla")
    with torch.no_grad():
        for salt, (name, p) in enumerate(sorted(msa.named_parameters())):
            p.copy_(_det_fill(p.shape, salt))
    msa = msa.to(DEV)
    x = bf16_bits_to_f32(blob["msa.x"]).to(DEV).requires_grad_(True)
    y = msa(x)
    (y * torch.linspace(-1, 1, y.numel(), device=DEV).reshape(y.shape)).sum().backward()
    assert max_err(y.cpu(), T(blob["msa.y"])) < 1e-5
    assert rel_err(x.grad.cpu(), T(blob["msa.grad_x"])) < 1e-4
    got = {k: v.grad.cpu().reshape(-1) for k, v in msa.named_parameters()}
    ref = grads_from(blob, "msa.")
    assert set(ref) == set(got)
    for k, g in ref.items():
        mine = got[k] if g.numel() == got[k].numel() else got[k][::WSTRIDE]
        assert mine.shape == g.shape and close(mine, g, rtol=1e-4, atol=5e-6), (k, rel_err(mine, g))


@pytest.mark.parametrize("t", ["vanilla", "cheby", "efficientkan", "fast", "sine"])
@pytest.mark.parametrize("d", [256, 160])
@pytest.mark.parametrize("n_patches", [7, 14])
def test_vit_with_wide_heads(t, d, n_patches):
    """VisionTransformer with two heads of 128 (d = 256) or 80 (d = 160), 3 x 56 x 56 images in 7 x 7 (N = 50) or 14 x 14
    (N = 197) patches: logits, loss and every parameter gradient against oracle.vit_forward in float64."""
    from model import VisionTransformer
    torch.manual_seed(5 + d + n_patches)
    m = VisionTransformer((3, 56, 56), n_patches=n_patches, n_blocks=1, d_hidden=d, n_heads=2, out_d=10, type=t).to(DEV)
    x = torch.rand(2, 3, 56, 56)
    y = torch.arange(2) % 10
    logits = m(x.to(DEV))
    loss = torch.nn.functional.cross_entropy(logits, y.to(DEV))
    loss.backward()
    sd = {k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu() for k, v in m.state_dict().items()}
    params = {k: v.clone().requires_grad_(not ko.is_buffer_key(k)) for k, v in sd.items()}
    ref = ko.vit_forward(params, x.double(), n_patches, 2, t)
    ref_loss = torch.nn.functional.cross_entropy(ref, y)
    ref_loss.backward()
    assert max_err(logits.detach().cpu(), ref.detach()) < 1e-4 and abs(float(loss.detach()) - float(ref_loss.detach())) < 1e-5
    for k, p in m.named_parameters():
        if not p.requires_grad:                              # FastKAN's frozen rbf.grid
            continue
        assert rel_err(p.grad.cpu(), params[k].grad) < 1e-4, k


def test_train_main_with_wide_heads_eager_equals_graph(tmp_path):
    """train.py --model-type cheby --d-hidden 256 --n-heads 2 (d_head = 128): eager and --graph replay bitwise equal, finite loss."""
    import train
    geom = ["--synthetic", "--in-chans", "1", "--image-size", "28", "--n-patches", "7", "--n-blocks", "1", "--n-heads", "2",
            "--d-hidden", "256", "--out-d", "10", "--batch-size", "4"]
    torch.manual_seed(9)
    x, y = torch.rand(4, 1, 28, 28), torch.arange(4) % 10
    runs = []
    for extra in ((), ("--graph",)):
        args = train.parse(["--model-type", "cheby", "--epochs", "1", "--steps-per-epoch", "3", "--no-step-metrics", "--log-dir",
                            str(tmp_path / f"logs{len(runs)}"), "--no-tuned-gemms", *geom, *extra])
        torch.manual_seed(9)
        runs.append(train.main(args, batches=[(x, y)] * 3)["losses"])
    assert runs[0] == runs[1], runs
    assert len(runs[0]) == 3 and all(np.isfinite(runs[0])), runs
