"""GPU parity of the attention kernels against the reference's FlashAttentionFunction outputs
(tests/golden/flash.npz) and the float64 oracle, over sequence lengths / head sizes / layouts."""
import pytest
import torch

from oracle import kan_oracle as ko
from tests._util import T, close, load_npz, max_err, record_kernels, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_flash_function_against_reference_fixture():
    from utils import FlashAttentionFunction
    f = load_npz("flash.npz")
    q, k, v = (T(f[n]).to(DEV).requires_grad_(True) for n in ("q", "k", "v"))
    do = T(f["do"]).to(DEV)
    for tag, causal in (("big", False), ("small", False), ("causal", True)):
        for t in (q, k, v):
            t.grad = None
        o = FlashAttentionFunction.apply(q, k, v, None, causal, 512, 1024)
        o.backward(do)
        assert max_err(o.cpu(), T(f[tag + ".o"])) < 5e-6, tag
        assert max_err(q.grad.cpu(), T(f[tag + ".dq"])) < 2e-5, tag
        assert max_err(k.grad.cpu(), T(f[tag + ".dk"])) < 2e-5, tag
        assert max_err(v.grad.cpu(), T(f[tag + ".dv"])) < 2e-5, tag


@pytest.mark.parametrize("n", [1, 2, 17, 31, 32, 33, 50, 64, 100, 197, 224])
@pytest.mark.parametrize("d", [2, 8, 32, 64])
@pytest.mark.parametrize("causal", [False, True])
def test_attention_against_oracle(n, d, causal):
    from kanvit import ops
    torch.manual_seed(n * 7 + d)
    b, h = 2, 3
    q, k, v = (torch.randn(b, h, n, d) * 1.3 for _ in range(3))
    do = torch.randn(b, h, n, d)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref, _ = ko.attention_reference(qd, kd, vd, causal=causal)
    o_ref.backward(do.double())
    qg, kg, vg = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    o = ops.attention(qg, kg, vg, causal=causal)
    o.backward(do.to(DEV))
    assert max_err(o.cpu(), o_ref) < 1e-5
    assert close(qg.grad, qd.grad) and close(kg.grad, kd.grad) and close(vg.grad, vd.grad)


def test_large_score_spike_is_stable():
    """One query aligned with one key at a large scale: softmax must not overflow."""
    from kanvit import ops
    torch.manual_seed(0)
    q, k, v = (torch.randn(1, 2, 197, 64) for _ in range(3))
    q[0, 0, 5] = k[0, 0, 100] * 40.0
    o = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV)).cpu()
    o_ref, _ = ko.attention_reference(q.double(), k.double(), v.double())
    assert torch.isfinite(o).all() and max_err(o, o_ref) < 1e-4


def test_packed_layout_matches_separate():
    from kanvit import ops
    torch.manual_seed(1)
    b, n, h, d = 3, 50, 2, 32
    qkv = torch.randn(b, n, 3, h, d, device=DEV, requires_grad=True)
    w = torch.randn(b, n, h * d, device=DEV)
    o = ops.attention_packed(qkv)
    (o * w).sum().backward()
    q, k, v = (qkv.detach()[:, :, i].permute(0, 2, 1, 3).cpu().double().requires_grad_(True) for i in range(3))
    o_ref, _ = ko.attention_reference(q, k, v)
    (o_ref.permute(0, 2, 1, 3).reshape(b, n, h * d) * w.cpu().double()).sum().backward()
    assert max_err(o.cpu(), o_ref.permute(0, 2, 1, 3).reshape(b, n, h * d)) < 1e-5
    g = qkv.grad.cpu()
    for i, t in enumerate((q, k, v)):
        assert rel_err(g[:, :, i].permute(0, 2, 1, 3), t.grad) < 1e-4


def test_bitwise_reproducible():
    from kanvit import ops
    q, k, v = (torch.randn(4, 12, 197, 64, device=DEV, requires_grad=True) for _ in range(3))
    res = []
    for _ in range(2):
        for t in (q, k, v):
            t.grad = None
        o = ops.attention(q, k, v)
        o.sum().backward()
        res.append((o.detach().clone(), q.grad.clone(), k.grad.clone(), v.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n,d", [(50, 32), (197, 64), (17, 16)])
def test_bf16_mfma_attention_close_to_fp32(n, d):
    from kanvit import ops
    torch.manual_seed(3)
    q, k, v = (torch.randn(2, 3, n, d, device=DEV, requires_grad=True) for _ in range(3))
    do = torch.randn(2, 3, n, d, device=DEV)
    outs = []
    for amp in (False, True):
        for t in (q, k, v):
            t.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            o = ops.attention(q, k, v)
        o.backward(do)
        outs.append((o.detach().clone(), q.grad.clone(), k.grad.clone(), v.grad.clone()))
    for a, b in zip(outs[1], outs[0]):
        err = float((a - b).abs().max()) / float(b.abs().max())
        if n <= 32 and d <= 32:      # one-wave-per-head kernels: exact fp32 under either mode (the flag allows bf16, never requires it)
            assert err == 0.0, err
        else:
            assert 0 < err < 3e-2, err


@pytest.mark.parametrize("n,d", [(50, 32), (65, 64), (197, 64), (224, 64), (256, 32)])
def test_bf16_ds_handoff_equals_recomputation(n, d, monkeypatch):
    """bf16 mode, backward (the two-kernel form; at (197, 64) the default is the one-kernel form of round 4, checked against both here):
    the key-stationary kernel hands dS to the dQ kernel as bf16 (one product, attn_bwd_dq_bf16_kernel)
    instead of the dQ kernel recomputing S, dP and the exponentials (KANVIT_ATTN_NO_DS=1: attn_bwd_q2_kernel).  dK / dV come from
    the same kernel either way -> bitwise equal; dQ is the same product of the same bf16-rounded factors up to where the rounding
    of dS happens -> both within the bf16 bound of the exact fp32 gradient, and close to each other."""
    from kanvit import _lib, ops
    torch.manual_seed(n + d)
    q, k, v = (torch.randn(3, 4, n, d, device=DEV, requires_grad=True) for _ in range(3))
    do = torch.randn(3, 4, n, d, device=DEV)

    def run(amp):
        for t in (q, k, v):
            t.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            o = ops.attention(q, k, v)
        o.backward(do)
        return q.grad.clone(), k.grad.clone(), v.grad.clone()

    exact = run(False)
    monkeypatch.delenv("KANVIT_ATTN_NO_DS", raising=False)
    _lib.reload_config()
    handoff = run(True)
    monkeypatch.setenv("KANVIT_ATTN_NO_DS", "1")
    _lib.reload_config()
    recomputed = run(True)
    monkeypatch.delenv("KANVIT_ATTN_NO_DS", raising=False)
    _lib.reload_config()
    if d == 64 and 193 <= n <= 204:     # round 4: this shape's default is the ONE-kernel backward on the bf16 matrix cores (csrc/attention16.hip):
        for i in (1, 2):                # dK / dV come from other kernels than the recompute path's -- same rounding points, another summation order
            sc_ = float(exact[i].abs().max())
            assert float((handoff[i] - recomputed[i]).abs().max()) / sc_ < 1e-2
            assert 0 < float((handoff[i] - exact[i]).abs().max()) / sc_ < 3e-2
    else:
        assert torch.equal(handoff[1], recomputed[1]) and torch.equal(handoff[2], recomputed[2])
    scale = float(exact[0].abs().max())
    e_new = float((handoff[0] - exact[0]).abs().max()) / scale
    e_old = float((recomputed[0] - exact[0]).abs().max()) / scale
    assert 0 < e_new < 3e-2 and e_new < 1.5 * e_old + 1e-3, (e_new, e_old)
    assert float((handoff[0] - recomputed[0]).abs().max()) / scale < 2e-2
    again = run(True)
    assert all(torch.equal(a, b) for a, b in zip(handoff, again))      # deterministic


@pytest.mark.parametrize("b,h,n,d,causal", [(128, 8, 17, 8, False), (3, 5, 32, 32, True), (2, 2, 1, 2, False), (7, 3, 31, 18, True),
                                                 (128, 2, 50, 32, False), (3, 3, 33, 32, True), (5, 1, 64, 16, False), (2, 7, 47, 8, True)])
def test_small_head_kernels_packed_layout_and_determinism(b, h, n, d, causal):
    """N <= 32, D <= 32 (train.py's default geometry is N = 17, D = 8): one wave per head (the cases with N > 32 run the
    third-form kernels through the same checks).  Against the fp64 oracle through the
    packed qkv layout MSA uses, bitwise run-to-run, and equal to the general kernels (KANVIT_ATTN_V1) to fp32 rounding."""
    import os
    from kanvit import _lib, ops
    torch.manual_seed(b + n)
    qkv = torch.randn(b, n, 3, h, d, device=DEV, requires_grad=True)
    do = torch.randn(b, n, h * d, device=DEV)

    def run():
        qkv.grad = None
        o = ops.attention_packed(qkv, causal=causal, scale=d ** -0.5)
        o.backward(do)
        return o.detach().clone(), qkv.grad.clone()

    o1, g1 = run()
    o2, g2 = run()
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    q64 = qkv.detach().double().cpu().requires_grad_(True)
    qq, kk, vv = (q64[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ref, _ = ko.attention_reference(qq * 1.0, kk, vv, causal=causal)
    ref = ref.permute(0, 2, 1, 3).reshape(b, n, h * d)
    (ref * do.double().cpu()).sum().backward()
    assert max_err(o1.cpu(), ref) < 2e-6 * max(1.0, float(ref.abs().max()))
    assert rel_err(g1.cpu(), q64.grad) < 1e-5
    os.environ["KANVIT_ATTN_V1"] = "1"
    _lib.reload_config()
    try:
        o0, g0 = run()
    finally:
        del os.environ["KANVIT_ATTN_V1"]
        _lib.reload_config()
    assert rel_err(o1, o0) < 1e-5 and rel_err(g1, g0) < 1e-5


def test_self_attention_binding_refuses_other_shapes():
    """kanvit_attn_desc carries ONE sequence length: through the self-attention binding a shorter k/v would be read out of bounds
    and a longer one silently truncated, so ops.attention raises before anything is launched (FlashAttentionFunction routes
    q_len != k_len and masks to the general kernels instead, below)."""
    from kanvit import ops
    from kanvit._lib import KanvitError
    from utils import FlashAttentionFunction
    q = torch.randn(2, 2, 40, 32, device=DEV)
    for nk in (24, 56):
        k = torch.randn(2, 2, nk, 32, device=DEV)
        with pytest.raises(KanvitError):
            ops.attention(q, k, k)
    with pytest.raises(KanvitError):                                    # head-size mismatch
        ops.attention(q, torch.randn(2, 2, 40, 16, device=DEV), torch.randn(2, 2, 40, 16, device=DEV))
    with pytest.raises(ValueError):
        FlashAttentionFunction.apply(q, torch.randn(2, 2, 40, 16, device=DEV), torch.randn(2, 2, 40, 16, device=DEV), None, False, 512, 512)
    # causal with k_len > q_len: the reference's diagonal runs the wrong way (utils.py:169,183) -- refused, at both levels
    k = torch.randn(2, 2, 56, 32, device=DEV)
    with pytest.raises(NotImplementedError):
        FlashAttentionFunction.apply(q, k, k, None, True, 512, 512)
    with pytest.raises(KanvitError, match="ill-defined"):
        ops._attn_x_fwd(q, k, k, torch.empty_like(q), None, True, 32 ** -0.5)


FLASH_X_CASES = ["keypad", "cross", "cross_mask4", "short_causal", "keypad_causal"]


@pytest.mark.parametrize("tag", FLASH_X_CASES)
def test_flash_function_masks_and_cross_lengths_against_reference_fixture(tag):
    """FlashAttentionFunction with a key-padding / full mask and with q_len != k_len (utils.py:141-195, 229-295) against the
    reference's own outputs and gradients (tests/golden/flash_x.npz): the general kernels of csrc/attention_x.hip."""
    from utils import FlashAttentionFunction
    f = load_npz("flash_x.npz")
    q, k, v = (T(f[f"{tag}.{n}"]).to(DEV).requires_grad_(True) for n in ("q", "k", "v"))
    do = T(f[f"{tag}.do"]).to(DEV)
    causal = bool(int(f[f"{tag}.causal"]))
    mask = torch.from_numpy(f[f"{tag}.mask"]).to(DEV) if f"{tag}.mask" in f else None
    o = FlashAttentionFunction.apply(q, k, v, mask, causal, 512, 1024)
    o.backward(do)
    assert max_err(o.cpu(), T(f[f"{tag}.o"])) < 5e-6
    assert max_err(q.grad.cpu(), T(f[f"{tag}.dq"])) < 2e-5
    assert max_err(k.grad.cpu(), T(f[f"{tag}.dk"])) < 2e-5
    assert max_err(v.grad.cpu(), T(f[f"{tag}.dv"])) < 2e-5


def test_flash_function_fully_masked_sample():
    from utils import FlashAttentionFunction
    f = load_npz("flash_x.npz")
    q, k, v = (T(f[f"allmasked.{n}"]).to(DEV).requires_grad_(True) for n in ("q", "k", "v"))
    mask = torch.from_numpy(f["allmasked.mask"]).to(DEV)
    o = FlashAttentionFunction.apply(q, k, v, mask, False, 512, 1024)
    assert max_err(o.cpu(), T(f["allmasked.o"])) < 5e-6 and float(o[1].abs().max()) == 0.0
    o.sum().backward()
    for t in (q, k, v):
        assert torch.isfinite(t.grad).all() and float(t.grad[1].abs().max()) == 0.0     # nothing flows through the masked sample


@pytest.mark.parametrize("nq,nk", [(1, 1), (7, 50), (50, 7), (33, 64), (64, 33), (197, 50), (50, 197), (224, 224), (130, 97), (577, 577), (300, 700), (1000, 64)])
@pytest.mark.parametrize("d", [2, 8, 32, 64])
@pytest.mark.parametrize("kind", ["none", "keypad", "full", "full_heads", "causal", "causal_keypad"])
def test_general_attention_against_fp64_oracle(nq, nk, d, kind):
    """The general kernels over lengths (ragged tiles on both sides, one side longer than the other, sequences of several 128-row
    LDS chunks: the running (max, sum) rescale of the forward, accumulators carried across chunks in the backward), head sizes and mask
    layouts -- (b, n) key padding, (b, 1, q, k) and (b, h, q, k) masks, strided (expanded) mask views -- against the float64
    oracle, forward and all three gradients; bitwise run-to-run."""
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
    elif kind == "full":
        mask = torch.rand(b, 1, nq, nk, generator=g) > 0.5
        mask[..., 0] = True
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
    if nq == nk and mask is None:
        pass                                        # (self-attention without a mask: the ViT kernels, covered above)
    assert max_err(outs[0][0].cpu(), o_ref) < 1e-5
    assert close(outs[0][1], qd.grad) and close(outs[0][2], kd.grad) and close(outs[0][3], vd.grad)
    for a_, b_ in zip(outs[0], outs[1]):
        assert torch.equal(a_, b_)


def test_flash_attention_module_with_context_and_mask():
    """FlashAttention(x, context=..., mask=...) (attention.py:59-109): projections around the general attention core, against
    the same computation in float64 with the oracle's attention."""
    from attention import FlashAttention
    torch.manual_seed(3)
    m = FlashAttention(dim=48, heads=3, dim_head=32).to(DEV)
    x = torch.randn(2, 21, 48, device=DEV, requires_grad=True)
    ctxt = torch.randn(2, 77, 48, device=DEV, requires_grad=True)
    mask = torch.rand(2, 77, device=DEV) > 0.3
    mask[:, 0] = True
    y = m(x, context=ctxt, mask=mask)
    y.square().sum().backward()
    W = {n: p.detach().cpu().double() for n, p in m.named_parameters()}
    xd, cd = x.detach().cpu().double().requires_grad_(True), ctxt.detach().cpu().double().requires_grad_(True)
    qd = (xd @ W["to_q.weight"].T).view(2, 21, 3, 32).permute(0, 2, 1, 3)
    kd, vd = ((cd @ W["to_kv.weight"].T).chunk(2, dim=-1)[i].reshape(2, 77, 3, 32).permute(0, 2, 1, 3) for i in range(2))
    od, _ = ko.attention_reference(qd, kd, vd, mask=mask.cpu())
    yd = od.permute(0, 2, 1, 3).reshape(2, 21, 96) @ W["to_out.weight"].T
    yd.square().sum().backward()
    assert rel_err(y.detach().cpu(), yd.detach()) < 1e-5
    assert rel_err(x.grad.cpu(), xd.grad) < 1e-4 and rel_err(ctxt.grad.cpu(), cd.grad) < 1e-4


# key-tile buckets of the forward / of attn_bwd_dq3_kernel at the sequence lengths of the two form tests below (D = 64)
FWD_BUCKET = {65: 4, 96: 4, 127: 4, 128: 4, 129: 7, 160: 7, 197: 7, 200: 7, 201: 7, 208: 7}
DQ3_BUCKET = {65: 4, 80: 4, 96: 4, 127: 4, 128: 4, 129: 8, 160: 8, 176: 8, 192: 8, 197: 8, 200: 8, 201: 8, 208: 8}
KV2_Q2_EXACT = {"attn_delta_kernel", "attn_bwd_kv2_kernel<2, false, false>", "attn_bwd_q2_kernel<2, false>"}


def _attn_kernels(names):
    return {x for x in names if x.startswith("attn")}


@pytest.mark.parametrize("n", [65, 96, 127, 128, 129, 160, 197, 200, 201, 208])
@pytest.mark.parametrize("causal", [False, True])
def test_fourth_form_ring_kernels(n, causal, monkeypatch):
    """The LDS-DMA ring kernels (attn_fwd4 / attn_bwd_kv4: D = 64, 64 < N <= 200) at every tile-count / ragged-tile case, with
    MORE heads than work-groups (KANVIT_ATTN_GRID = 5: each persistent work-group walks 6 heads, i.e. the three-buffer ring, the
    loader wave's progressive dO fill and the tile counters wrap around twice) -- against the fp64 oracle, and against the
    third-form kernels (KANVIT_ATTN_V3) on the same inputs.  The kernels of the first run of each arm are recorded and asserted:
    at N = 201 and 208 three images of a head no longer fit the LDS, so both arms run the third forms there (kept as the cases
    just past the ring kernels' upper edge, N = 200)."""
    from kanvit import _lib, ops
    torch.manual_seed(1000 + n)
    b, h, d = 5, 6, 64
    q, k, v = (torch.randn(b, h, n, d) * 1.2 for _ in range(3))
    do = torch.randn(b, h, n, d)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref, _ = ko.attention_reference(qd, kd, vd, causal=causal)
    o_ref.backward(do.double())

    def run():
        qg, kg, vg = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
        o = ops.attention(qg, kg, vg, causal=causal)
        o.backward(do.to(DEV))
        return o.detach().cpu(), qg.grad.cpu(), kg.grad.cpu(), vg.grad.cpu()

    monkeypatch.setenv("KANVIT_ATTN_GRID", "5")
    monkeypatch.setenv("KANVIT_ATTN_V4", "1")          # (since round 4 the default for these shapes is the 16-row-tile form: next test)
    assert "attn_grid=5" in _lib.reload_config()
    try:
        with record_kernels() as ring_names:
            ring = run()
        again = run()
        monkeypatch.setenv("KANVIT_ATTN_V3", "1")
        assert "attn_v3=1" in _lib.reload_config()
        with record_kernels() as third_names:
            third = run()
    finally:
        monkeypatch.delenv("KANVIT_ATTN_GRID")
        monkeypatch.delenv("KANVIT_ATTN_V4")
        monkeypatch.delenv("KANVIT_ATTN_V3", raising=False)
        _lib.reload_config()
    third_form = {"attn_fwd3_kernel<2, %d>" % FWD_BUCKET[n]} | (
        KV2_Q2_EXACT if causal else {"attn_bwd_kv3_kernel<2, %d>" % DQ3_BUCKET[n], "attn_bwd_dq3_kernel<2, %d>" % DQ3_BUCKET[n]})
    ring_form = {"attn_fwd4_kernel<2, %d>" % FWD_BUCKET[n]} | (
        KV2_Q2_EXACT if causal else {"attn_bwd_kv4_kernel<2>", "attn_bwd_dq3_kernel<2, %d>" % DQ3_BUCKET[n]})
    assert _attn_kernels(ring_names) == (ring_form if n <= 200 else third_form), sorted(ring_names)
    assert _attn_kernels(third_names) == third_form, sorted(third_names)
    assert all(torch.equal(a, c) for a, c in zip(ring, again))            # no atomics, fixed order: bitwise run to run
    assert max_err(ring[0], o_ref) < 1e-5
    for g, ref in zip(ring[1:], (qd.grad, kd.grad, vd.grad)):
        assert close(g, ref)
    for a, c in zip(ring, third):                                        # same mathematics, same summation order per tile
        assert max_err(a, c) < 2e-6 * max(1.0, float(c.abs().max()))


@pytest.mark.parametrize("n", [65, 80, 96, 127, 128, 129, 160, 176, 192, 193, 197, 200, 201, 204])
@pytest.mark.parametrize("bh", [(5, 6), (1, 7), (1, 3)])
def test_sixteen_row_tile_kernels(n, bh, monkeypatch):
    """csrc/attention16.hip (round 4): the forward on 16-row tiles for every tile count 5..13 (twelve waves own a tile each, the
    thirteenth tile is cut into key quarters), and -- for 13 tiles, N = 193..204 -- the one-kernel backward (streamed query slices,
    dS tiles crossing the LDS, dQ units on the waves of the lighter SIMDs, hand-offs by LDS counters).  Persistent work-groups
    walk several heads (30 heads on 5 work-groups: every ring and counter wraps), an uneven share (7 on 5) and a single head each
    (3 on 5: two work-groups idle): against the fp64 oracle, bitwise run to run, and against the fourth-form kernels."""
    from kanvit import _lib, ops
    b, h = bh
    torch.manual_seed(2000 + n + 7 * h)
    d = 64
    q, k, v = (torch.randn(b, h, n, d) * 1.2 for _ in range(3))
    do = torch.randn(b, h, n, d)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref, lse_ref = ko.attention_reference(qd, kd, vd, causal=False)
    o_ref.backward(do.double())

    def run():
        qg, kg, vg = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
        o = ops.attention(qg, kg, vg, causal=False)
        o.backward(do.to(DEV))
        return o.detach().cpu(), qg.grad.cpu(), kg.grad.cpu(), vg.grad.cpu()

    monkeypatch.setenv("KANVIT_ATTN_GRID", "5")
    assert "attn_grid=5" in _lib.reload_config() and "attn_v4=0" in _lib.active_config()
    try:
        with record_kernels() as names:
            new = run()
        again = run()
        monkeypatch.setenv("KANVIT_ATTN_V4", "1")
        assert "attn_v4=1" in _lib.reload_config()
        fourth = run()
    finally:
        monkeypatch.delenv("KANVIT_ATTN_GRID")
        monkeypatch.delenv("KANVIT_ATTN_V4", raising=False)
        _lib.reload_config()
    # the first run: the 16-row forward; the one-kernel backward where a head is 13 tiles, below that the ring kernel + dQ from its dS
    backward = {"attn16_bwd_kernel<false>"} if n >= 193 else {"attn_bwd_kv4_kernel<2>", "attn_bwd_dq3_kernel<2, %d>" % DQ3_BUCKET[n]}
    forward = _attn_kernels(names) - backward
    assert backward <= names and len(forward) == 1 and next(iter(forward)).startswith("attn16_fwd_kernel<"), sorted(names)
    assert all(torch.equal(a, c) for a, c in zip(new, again))             # counters order the hand-offs, sums have a fixed order: bitwise
    assert max_err(new[0], o_ref) < 1e-5
    for g_, ref in zip(new[1:], (qd.grad, kd.grad, vd.grad)):
        assert close(g_, ref)
    for a_, c in zip(new, fourth):
        assert max_err(a_, c) < 4e-6 * max(1.0, float(c.abs().max()))


@pytest.mark.parametrize("n,d", [(257, 32), (225, 64), (577, 64), (1025, 16)])
@pytest.mark.parametrize("causal", [False, True])
def test_self_attention_longer_than_one_workgroup(n, d, causal):
    """Heads that do not fit the ViT kernels' one-work-group-per-head form (N > 224 at D = 64, > 256 at D <= 32; ViT-B/16 at
    384 x 384 is N = 577) run through the chunked general kernels: ops.attention and the packed q|k|v form MSA uses, against the
    float64 oracle."""
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
    if not causal:
        qkv = torch.stack([q, k, v], dim=0).permute(1, 3, 0, 2, 4).contiguous().to(DEV).requires_grad_(True)      # [B, N, 3, H, D]
        op = ops.attention_packed(qkv)                   # o[B, N, H*D]
        assert max_err(op.reshape(b, n, h, d).permute(0, 2, 1, 3).cpu(), o_ref) < 1e-5


@pytest.mark.parametrize("t", ["vanilla", "cheby"])
def test_vit_with_more_tokens_than_one_workgroup_holds(t):
    """A model whose sequence does not fit the one-head-per-work-group attention kernels (32 x 32 images in 2 x 2 patches: N = 257,
    dh = 32) runs through MSA -> attention_packed -> the chunked general kernels: logits, loss and every gradient against
    oracle.vit_forward in float64 (the reference handles any length; round 2 raised here)."""
    from model import VisionTransformer
    torch.manual_seed(5)
    m = VisionTransformer((1, 32, 32), n_patches=16, n_blocks=1, d_hidden=64, n_heads=2, out_d=10, type=t).to(DEV)
    x = torch.rand(3, 1, 32, 32)
    y = torch.arange(3) % 10
    logits = m(x.to(DEV))
    loss = torch.nn.functional.cross_entropy(logits, y.to(DEV))
    loss.backward()
    sd = {k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu() for k, v in m.state_dict().items()}
    params = {k: v.clone().requires_grad_(not ko.is_buffer_key(k)) for k, v in sd.items()}
    ref = ko.vit_forward(params, x.double(), 16, 2, t)
    ref_loss = torch.nn.functional.cross_entropy(ref, y)
    ref_loss.backward()
    assert max_err(logits.detach().cpu(), ref.detach()) < 1e-4 and abs(float(loss) - float(ref_loss)) < 1e-5
    for k, p in m.named_parameters():
        assert rel_err(p.grad.cpu(), params[k].grad) < 1e-4, k
