"""Opt-in bf16x3 feed-forward (kanvit_split3_bf16 + bf16 GEMMs with fp32 accumulate): the split image is exact to 2^-16,
the block matches the fp32 block to a few 1e-6, and a whole model stays inside BASELINE's 1e-4 budget."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("pattern", [0, 1])
def test_split_image_reconstructs_the_input(pattern):
    from kanvit import dense as D
    torch.manual_seed(0)
    x = torch.randn(37, 64, device=DEV) * torch.logspace(-3, 3, 64, device=DEV)
    img = D._split3(x, pattern).float()
    K = x.shape[1]
    hi = img[:, :K]
    lo = img[:, 2 * K:] if pattern == 0 else img[:, K:2 * K]
    dup = img[:, K:2 * K] if pattern == 0 else img[:, 2 * K:]
    assert torch.equal(dup, hi)
    assert torch.equal(hi, x.bfloat16().float())
    assert float(((hi + lo) - x).abs().max() / x.abs().max()) < 2.0 ** -15
    assert float((((hi + lo) - x).abs() / x.abs().clamp_min(1e-30)).max()) < 2.0 ** -15


def _restate(x, pattern, bias=None, relu=False, mask=None):
    """kanvit_split3_bf16 in CPU torch on the device's own operands: one fp32 add, ReLU (+0 for -0 and for every negative value, as the
    device's maximum orders the zeros), the mask `hi of the saved activation > 0` (+0 where it is not), hi = bf16(v) and
    lo = bf16(v - hi) rounded to nearest even, the three K-wide blocks in the pattern's order.  Returns the image's int16 bits."""
    v = x.detach().cpu().clone()
    K = v.shape[1]
    if bias is not None:
        v = v + bias.detach().cpu()
    if relu:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    if mask is not None:
        v = torch.where(mask.detach().cpu()[:, :K].float() > 0, v, torch.zeros_like(v))
    assert v.dtype == torch.float32
    hi = v.bfloat16()
    lo = (v - hi.float()).bfloat16()
    return torch.cat([hi, hi, lo] if pattern == 0 else [hi, lo, hi], 1).view(torch.int16)


def _bits(img):
    assert img.dtype == torch.bfloat16
    return img.cpu().view(torch.int16)


SPLIT_CAP_ITEMS = 4096 * 256        # split3_kernel: at most 4096 work-groups of 256 threads, one item of eight columns each per lap


def test_split_image_bias_relu_mask():
    """Every combination of bias, ReLU and mask, bit for bit.  Row 0 holds +0, -0, values whose lo is zero (1.5, -1.5, 2^-3), a
    pre-activation that the bias turns negative, one it turns into -0 + -0 and one it cancels to +0; the mask is the image of another
    activation, with zeros and negative zeros in its hi part."""
    from kanvit import dense as D
    torch.manual_seed(1)
    M, K = 9, 24
    x = torch.randn(M, K) * torch.logspace(-3, 3, K)
    b = torch.randn(K)
    x[0, :8] = torch.tensor([0.0, -0.0, 1.5, -1.5, 0.125, 0.25, -0.0, 0.75])
    b[:8] = torch.tensor([0.0, 0.0, -0.0, 0.5, -0.0, -1.0, -0.0, -0.75])
    x, b = x.to(DEV), b.to(DEV)
    act = torch.randn(M, K, device=DEV)
    act[1, :4] = torch.tensor([0.0, -0.0, 1e-3, -1e-3])
    saved = D._split3(act, 0, relu=False)                # hi of both signs, +0 and -0: what `> 0` has to tell apart
    assert bool((saved[:, :K].float() < 0).any()) and bool((saved[:, :K].float() == 0).any())
    for pattern in (0, 1):
        seen = set()
        for bias in (None, b):
            for relu in (False, True):
                for mask in (None, saved):
                    img = D._split3(x, pattern, bias=bias, relu=relu, mask=mask)
                    want = _restate(x, pattern, bias, relu, mask)
                    assert img.shape == (M, 3 * K) and torch.equal(_bits(img), want), (pattern, bias is not None, relu, mask is not None)
                    seen.add(tuple(want.reshape(-1).tolist()))
                    lo = want[:, 2 * K:] if pattern == 0 else want[:, K:2 * K]
                    assert bool((lo[0, :8] == 0).sum() >= 3) and bool((lo != 0).any())         # some lo is zero, not every one
        assert len(seen) == 8                                # the eight combinations are eight different images
        plain = _restate(x, pattern)
        assert int(plain[0, 1]) == -0x8000 and int(plain[0, 0]) == 0                     # -0 keeps its sign through hi
        assert bool((_restate(x, pattern, b).view(torch.bfloat16).float()[:, :K] < 0).any())         # negative pre-activations are there


@pytest.mark.parametrize("pattern,fused", [(0, "bias_relu"), (1, "mask")])
def test_split_image_past_the_grid_cap_wraps_the_stride_loop(pattern, fused):
    """M = 4200, K = 2048: 1 075 200 items of eight columns against the 1 048 576 threads of a full grid, so the last rows come from a
    thread's second lap.  Same restatement, bit for bit."""
    from kanvit import dense as D
    M, K = 4200, 2048
    assert M * (K // 8) > SPLIT_CAP_ITEMS
    g = torch.Generator().manual_seed(7 + pattern)
    x = (torch.randn(M, K, generator=g) * torch.logspace(-2, 2, K)).to(DEV)
    if fused == "bias_relu":
        b = torch.randn(K, generator=g).to(DEV)
        img, want = D._split3(x, pattern, bias=b, relu=True), _restate(x, pattern, b, True)
    else:
        saved = torch.relu(torch.randn(M, K, generator=g)).bfloat16().to(DEV)          # the hi part alone, made without the kernel: mask_ld = K
        img, want = D._split3(x, pattern, mask=saved), _restate(x, pattern, mask=saved)
    first_lap_rows = SPLIT_CAP_ITEMS // (K // 8)
    assert first_lap_rows < M and bool((want[first_lap_rows:] != 0).any())             # the second lap has something to write
    assert torch.equal(_bits(img), want)


def test_feed_forward_split_close_to_fp32():
    from kanvit import dense as D
    torch.manual_seed(2)
    l1, l2 = torch.nn.Linear(64, 256).to(DEV), torch.nn.Linear(256, 64).to(DEV)
    x = torch.randn(2048, 64, device=DEV, requires_grad=True)
    dy = torch.randn(2048, 64, device=DEV)
    res = {}
    for mode in ("fp32", "bf16x3"):
        D.FF_MODE = mode
        try:
            x.grad = None
            l1.zero_grad()
            l2.zero_grad()
            y = D.feed_forward(x, l1, l2)
            y.backward(dy)
            res[mode] = [y.detach().clone(), l2.weight.grad.clone(), l2.bias.grad.clone(), x.grad.clone(), l1.weight.grad.clone()]
        finally:
            D.FF_MODE = "fp32"
    errs = [float((a - b).abs().max()) / float(a.abs().max()) for a, b in zip(res["fp32"], res["bf16x3"])]
    assert errs[0] > 0                                  # the split path really ran
    assert max(errs[:3]) < 3e-5, errs                   # y, dW2, db2
    assert max(errs[3:]) < 5e-2, errs                   # dx, dW1: ReLU-mask flips where a pre-activation is ~ 0


def test_model_with_split_feed_forward_within_parity_budget():
    from kanvit import dense as D
    from model import VisionTransformer
    torch.manual_seed(3)
    m = VisionTransformer((3, 32, 32), n_patches=4, n_blocks=4, d_hidden=64, n_heads=8, out_d=100, type="cheby").to(DEV)
    x = torch.randn(16, 3, 32, 32, device=DEV)
    with torch.no_grad():
        a = m(x)
        D.FF_MODE = "bf16x3"
        try:
            b = m(x)
        finally:
            D.FF_MODE = "fp32"
    assert 0 < float((a - b).abs().max()) < 1e-4
