"""Attention maps from the fused path: kanvit.ops.attention_probs(_packed), MSA / FlashAttention / TransformerBlock.attention_map,
VisionTransformer.attention_maps / attention_rollout.  Bounds (none of them fitted to what the kernel gives):
  * P against the float64 statement (tests/_attention_map_ref.py): 1e-5, the bound test_attention_wide_gpu.py holds o = P.v to
    for the same randn inputs -- an entry of P carries no more error than the sum built from it;
  * a live row sums to 1 within (Nk + 8) * 2^-24: sum_j e_j / fl(sum e_j) has the relative error of one fp32 sum of Nk
    non-negative terms in any order (<= (Nk - 1) * 2^-24) plus a few ulps for the reciprocal, the product and the final rounding;
  * P.v against the module's output: 2e-5, the project's 1e-5 applied once to each side;
  * rollout: n_blocks * N * 2^-23 -- every factor is non-negative with rows summing to 1, so an fp32 dot product of N terms has
    relative error <= N * 2^-24 without cancellation, entries are <= 1, and the normalisation adds a few ulps per factor.
Every test prints the largest figure it saw (pytest -s) before it asserts."""
import numpy as np
import pytest
import torch

from tests._attention_map_ref import attention_probs_ref, rollout_ref
from tests._util import bf16_bits_to_f32, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 2, 3
LENGTHS = [(1, 1), (1, 7), (5, 5), (33, 33), (64, 64), (65, 129), (130, 7), (197, 197), (257, 257)]
HEAD_SIZES = [2, 16, 34, 64, 66, 128]


def _qk(nq, nk, d, seed, gain=1.0):
    g = torch.Generator().manual_seed(seed)
    return gain * torch.randn(B, H, nq, d, generator=g), gain * torch.randn(B, H, nk, d, generator=g)


def _masks(nq, nk, seed):
    """kind -> (mask or None, causal)"""
    g = torch.Generator().manual_seed(1000 + seed)
    keypad = torch.rand(B, nk, generator=g) > 0.3
    keypad[0, 0] = True
    keypad[1] = False                                   # one sample fully padded
    full = torch.rand(B, H, nq, nk, generator=g) > 0.4
    full[0, 0, 0] = False                               # several all-dead rows
    full[1, 2, nq // 2] = False
    full[1, 1, nq - 1] = False
    full[0, 1, 0, nk - 1] = True
    bcast = torch.rand(1, 1, nq, nk, generator=g) > 0.4
    bcast[0, 0, 0, 0] = True
    kinds = {"none": (None, False), "keypad": (keypad, False), "full": (full, False), "broadcast": (bcast, False)}
    if nk <= nq:
        kinds["causal"] = (None, True)
    return kinds


def _check(p, q, k, mask, causal, tag):
    """The three properties of the parity sweep; returns (max |P - ref|, max |row sum - 1| / its bound)."""
    from oracle import kan_oracle as ko
    nk = k.shape[2]
    assert p.dtype == torch.float32 and tuple(p.shape) == (B, H, q.shape[2], nk)
    ref = attention_probs_ref(q, k, mask, causal)
    pc = p.cpu()
    assert bool(torch.isfinite(pc).all()), tag
    err = float((pc.double() - ref).abs().max())
    dead = ko.attention_dead(q, k, causal, mask)
    live_rows = torch.ones(p.shape[:3], dtype=torch.bool)
    if dead is not None:
        dead = dead.expand(p.shape)
        assert bool((pc[dead] == 0.0).all()), f"{tag}: a dead position is not exactly 0"
        live_rows = ~dead.all(dim=-1)
        assert bool((pc[~live_rows] == 0.0).all()), f"{tag}: a fully dead row is not all-zero"
    sums = pc.double().sum(dim=-1)[live_rows]
    bound = (nk + 8) * 2.0 ** -24
    srel = float((sums - 1).abs().max()) / bound if sums.numel() else 0.0
    print(f"MEASURED probs {tag}: max|P-ref|={err:.3e} (bound 1e-5)  max|rowsum-1|={srel * bound:.3e} (bound {bound:.3e})")
    assert err < 1e-5, tag
    assert srel <= 1.0, tag
    return err, srel


@pytest.mark.parametrize("d", HEAD_SIZES)
@pytest.mark.parametrize("nq,nk", LENGTHS)
def test_parity_sweep(nq, nk, d):
    from kanvit import ops
    q, k = _qk(nq, nk, d, seed=nq * 1000 + nk + d)
    qd, kd = q.to(DEV), k.to(DEV)
    for kind, (mask, causal) in _masks(nq, nk, d).items():
        p = ops.attention_probs(qd, kd, mask=None if mask is None else mask.to(DEV), causal=causal)
        _check(p, q, k, mask, causal, f"Nq={nq} Nk={nk} D={d} {kind}")


@pytest.mark.parametrize("kind", ["none", "full", "causal"])
def test_saturated_scores(kind):
    """q and k scaled by 8: scores reach tens to hundreds and most of a row underflows; finite, same bounds."""
    from kanvit import ops
    nq, nk, d = (129, 65, 64) if kind == "causal" else (65, 129, 64)
    q, k = _qk(nq, nk, d, seed=77, gain=8.0)
    mask, causal = _masks(nq, nk, 3)[kind]
    p = ops.attention_probs(q.to(DEV), k.to(DEV), mask=None if mask is None else mask.to(DEV), causal=causal)
    _check(p, q, k, mask, causal, f"saturated Nq={nq} Nk={nk} D={d} {kind}")


@pytest.mark.parametrize("nq,nk", [(65, 129), (197, 197)])
def test_rows_are_the_leading_rows_bitwise(nq, nk):
    from kanvit import ops
    q, k = (t.to(DEV) for t in _qk(nq, nk, 64, seed=5))
    for kind, (mask, causal) in _masks(nq, nk, 9).items():
        mask = None if mask is None else mask.to(DEV)
        full = ops.attention_probs(q, k, mask=mask, causal=causal)
        for rows in (1, 3, nq):
            part = ops.attention_probs(q, k, mask=mask, causal=causal, rows=rows)
            assert tuple(part.shape) == (B, H, rows, nk)
            assert torch.equal(part, full[:, :, :rows]), (kind, rows)


@pytest.mark.parametrize("n,d", [(50, 32), (197, 64), (70, 34)])
def test_layout_and_placement_do_not_change_the_bits(n, d):
    from kanvit import ops
    qkv = torch.randn(B, n, 3, H, d, generator=torch.Generator().manual_seed(n + d)).to(DEV)
    packed = ops.attention_probs_packed(qkv)
    q, k = (qkv[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(2))
    sep = ops.attention_probs(q, k)
    assert tuple(packed.shape) == (B, H, n, n) and torch.equal(packed, sep)
    assert torch.equal(ops.attention_probs_packed(qkv), packed)                       # run to run
    assert torch.equal(ops.attention_probs_packed(qkv, rows=1), packed[:, :, :1])
    buf = torch.empty(q.numel() + 1, device=DEV)                                       # 4 bytes off: the scalar tile fills
    assert torch.equal(ops.attention_probs(buf[1:].view_as(q).copy_(q), k), packed)
    for b in range(B):                                                                 # a sample alone
        assert torch.equal(ops.attention_probs_packed(qkv[b:b + 1].contiguous()), packed[b:b + 1])
        assert torch.equal(ops.attention_probs(q[b:b + 1, 1:2], k[b:b + 1, 1:2]), packed[b:b + 1, 1:2])      # a head alone, strided


def test_result_has_no_history_and_is_fp32_under_autocast():
    from kanvit import ops
    q, k = (t.to(DEV).requires_grad_(True) for t in _qk(9, 11, 16, seed=3))
    p = ops.attention_probs(q, k)
    assert not p.requires_grad and p.grad_fn is None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pa = ops.attention_probs(q, k)
        pb = ops.attention_probs(q.detach().bfloat16(), k.detach().bfloat16())
    assert pa.dtype == torch.float32 and torch.equal(pa, p)
    assert pb.dtype == torch.float32
    with pytest.raises(ops.KanvitError):
        ops.attention_probs(q, k, rows=0)
    with pytest.raises(ops.KanvitError):
        ops.attention_probs(q[:, :, :5], k, causal=True)                              # Nk > Nq


# (d, H, N): the one-work-group route, the 16-row-tile route (D = 64, N = 197) and the general route (D = 80)
MSA_GEOMETRIES = [(64, 2, 50), (128, 2, 197), (160, 2, 257)]


@pytest.mark.parametrize("d,heads,n", MSA_GEOMETRIES)
@pytest.mark.parametrize("kind", ["vanilla", "cheby", "efficientkan"])
def test_msa_map_is_the_map_of_the_attention_that_runs(kind, d, heads, n):
    from attention import MSA
    from kanvit import grouped
    torch.manual_seed(11)
    msa = MSA(d, heads, type=kind).to(DEV)
    x = torch.randn(2, n, d, generator=torch.Generator().manual_seed(n)).to(DEV)
    with torch.no_grad():
        y = msa(x)
        qkv = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x.reshape(2 * n, d)).view(2, n, 3, heads, d // heads)
    p = msa.attention_map(x)
    assert tuple(p.shape) == (2, heads, n, n) and p.dtype == torch.float32 and not p.requires_grad
    v = qkv[:, :, 2].permute(0, 2, 1, 3).double().cpu()
    o = (p.double().cpu() @ v).permute(0, 2, 1, 3).reshape(2, n, d)
    err = float((o - y.double().cpu()).abs().max())
    print(f"MEASURED msa {kind} d={d} H={heads} N={n}: max|P.v - msa(x)|={err:.3e} (bound 2e-5)")
    assert err < 2e-5
    assert torch.equal(msa.attention_map(x, rows=1), p[:, :, :1])
    assert all(prm.grad is None for prm in msa.parameters())


def test_flash_attention_map_with_context_and_key_padding():
    from attention import FlashAttention
    torch.manual_seed(13)
    fa = FlashAttention(dim=48, heads=3, dim_head=16).to(DEV)
    g = torch.Generator().manual_seed(2)
    x, ctx = torch.randn(2, 21, 48, generator=g).to(DEV), torch.randn(2, 37, 48, generator=g).to(DEV)
    mask = torch.rand(2, 37, generator=g) > 0.3
    mask[:, 0] = True
    mask = mask.to(DEV)
    seen = []
    hook = fa.to_out.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach()))
    with torch.no_grad():
        fa(x, context=ctx, mask=mask)
        v = fa.to_kv(ctx).chunk(2, dim=-1)[1].view(2, 37, 3, 16).permute(0, 2, 1, 3)
    hook.remove()
    p = fa.attention_map(x, context=ctx, mask=mask)
    assert tuple(p.shape) == (2, 3, 21, 37) and p.dtype == torch.float32
    assert bool((p[~mask[:, None, None, :].expand_as(p)] == 0.0).all())
    o = (p.double().cpu() @ v.double().cpu()).permute(0, 2, 1, 3).reshape(2, 21, 48)
    err = float((o - seen[0].double().cpu()).abs().max())
    print(f"MEASURED flash context+keypad: max|P.v - o|={err:.3e} (bound 2e-5)")
    assert err < 2e-5
    fc = FlashAttention(dim=48, heads=3, dim_head=16, causal=True).to(DEV)
    pc = fc.attention_map(x, rows=4)
    assert tuple(pc.shape) == (2, 3, 4, 21) and bool((pc.triu(1) == 0.0).all())


def _det_fill(shape, salt):
    """tests/golden/make_golden_attention_map.py::det_fill: exact float32 values from integer arithmetic."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    return torch.from_numpy((((i * 7919 + salt * 104729) % 4093 - 2046) / 4096.0).astype(np.float32).reshape(shape))


@pytest.mark.parametrize("kind,bound", [("vanilla", 1e-5), ("cheby", 1e-4), ("fast", 1e-4)])
def test_maps_against_the_reference_softmax_hook(kind, bound):
    """tests/golden/attention_map.npz: what a forward hook on the reference's MSA.softmax collects, stacked to [3, 2, 5, 5]."""
    from attention import MSA
    blob = load_npz("attention_map.npz")
    msa = MSA(16, 2, type=kind)
    with torch.no_grad():
        for salt, (name, p) in enumerate(sorted((n, p) for n, p in msa.named_parameters() if p.requires_grad)):
            p.copy_(_det_fill(p.shape, salt))
    msa = msa.to(DEV)
    got = msa.attention_map(bf16_bits_to_f32(blob["x"]).to(DEV))
    want = torch.from_numpy(blob[kind + ".maps"])
    assert tuple(got.shape) == tuple(want.shape) == (3, 2, 5, 5)
    err = float((got.double().cpu() - want.double()).abs().max())
    print(f"MEASURED golden {kind}: max|map - reference hook|={err:.3e} (bound {bound:g})")
    assert err < bound


def _block_inputs(model, images):
    """The stream every block receives.  A forward pre-hook on each block records it during a plain model(images) where the model
    calls its blocks ('flash-attn'); VisionTransformer.forward drives TransformerBlocks through run(), which carries the previous
    feed-forward output as a pending add and never calls the block, so there the hooks record the same stream while the blocks
    are called one after the other on the embedded tokens.  Returns (inputs, logits of the plain forward)."""
    seen = {}
    hooks = [blk.register_forward_pre_hook(lambda mod, args, l=l: seen.__setitem__(l, args[0].detach().clone()))
             for l, blk in enumerate(model.blocks)]
    with torch.no_grad():
        logits = model(images)
        if len(seen) != len(model.blocks):
            seen.clear()
            x = model._embed(images)
            for blk in model.blocks:
                x = blk(x)
    for h in hooks:
        h.remove()
    return [seen[l] for l in range(len(model.blocks))], logits


@pytest.mark.parametrize("kind", ["cheby", "efficientkan", "sine,fourier", "flash-attn"])
def test_model_maps_and_rollout(kind):
    from model import VisionTransformer
    torch.manual_seed(3)
    model = VisionTransformer((3, 32, 32), n_patches=4, n_blocks=2, d_hidden=64, n_heads=8, type=kind).to(DEV)
    images = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(8)).to(DEV)
    n, nb = 17, 2
    inputs, logits = _block_inputs(model, images)
    for training in (True, False):
        model.train(training)
        maps = model.attention_maps(images)
        assert model.training is training
    assert tuple(maps.shape) == (nb, 2, 8, n, n) and maps.dtype == torch.float32 and not maps.requires_grad
    for l, blk in enumerate(model.blocks):
        assert torch.equal(maps[l], blk.attention_map(inputs[l])), l
    assert torch.equal(model.attention_maps(images, rows=1), maps[:, :, :, :1])
    worst = 0.0
    bound = nb * n * 2.0 ** -23
    for f in ("mean", "max", "min"):
        roll = model.attention_rollout(images, f)
        assert tuple(roll.shape) == (2, n, n) and roll.dtype == torch.float32
        assert torch.equal(roll, VisionTransformer.rollout(maps, f))
        err = float((roll.double().cpu() - rollout_ref(maps, f)).abs().max())
        rs = float((roll.double().cpu().sum(-1) - 1).abs().max())
        worst = max(worst, err, rs)
        print(f"MEASURED model {kind} rollout {f}: max|rollout - ref|={err:.3e}  max|rowsum-1|={rs:.3e} (bound {bound:.3e})")
        assert err <= bound and rs <= bound
    assert tuple(model.cls_saliency(roll).shape) == (2, 4, 4)
    with torch.no_grad():
        assert torch.equal(model(images), logits)
    assert all(p.grad is None for p in model.parameters())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        amaps = model.attention_maps(images)
        aroll = model.attention_rollout(images)
    assert amaps.dtype == torch.float32 and aroll.dtype == torch.float32
    assert bool(torch.isfinite(amaps).all()) and bool(torch.isfinite(aroll).all())
    srow = float((amaps.double().sum(-1) - 1).abs().max())
    print(f"MEASURED model {kind} autocast: max|rowsum-1|={srow:.3e} (bound {(n + 8) * 2.0 ** -24:.3e})")
    assert srow <= (n + 8) * 2.0 ** -24
