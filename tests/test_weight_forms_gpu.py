"""Every weight-gradient form plan_layer_bwd_weight (csrc/kan_layer.hip) can name that no other file names, run and
named: one forward and backward through the Python modules at the smallest shape that takes the branch.  Each case asserts

  * the exact set of kan_bwd_weight*, kan_tiny_bwd_weight* and kan_slab_reduce* kernels the backward launched
    (tests/_util.record_kernels), as literals.  They are what the library of the commit BEFORE the plan existed launches: this file
    was run on the GPU against that library (tools/build_variant.sh parent, KANVIT_LIB) with these literals and passed, so a plan
    that names another form fails here by name (profiles/weight_plan_forms.md);
  * every parameter gradient (and y, dx where the call has them) against the float64 oracle with the suite's bounds
    (tests/test_launch_shapes_gpu.py: _check_fp32 / _check_bf16, called);
  * for fp32, a second run that is bitwise equal.

Already named elsewhere and not repeated: the B-spline 12-tile 16-row kernel and the ViT-B LDS-DMA launch
(tests/test_launch_shapes_gpu.py), FastKAN's 16-row kernel, the one-slab tiny kernel, the one-column-tile ChebyKAN kernel and the
LDS-tile bf16 kernel (tests/test_layer_forms_gpu.py)."""
import contextlib

import pytest
import torch

from oracle import kan_oracle as ko
from tests._util import record_kernels
from tests import test_launch_shapes_gpu as shapes
from tests import test_layer_forms_gpu as forms
from tests.test_launch_shapes_gpu import _Err

pytestmark = pytest.mark.gpu
DEV = "cuda"
WEIGHT_KERNELS = ("kan_bwd_weight", "kan_tiny_bwd_weight", "kan_slab_reduce")


def _weight_kernels(names):
    return {n for n in names if n.startswith(WEIGHT_KERNELS)}


def _kanlinear(i, o):
    from models.effkan import KANLinear
    return KANLinear(i, o)             # the constructor's grid: uniform cubic knots


# id -> (layer factory, rows, bf16, the weight-gradient kernels of one backward)
LAYER_CASES = {
    # three 128-row slabs (M = 100 in test_layer_forms_gpu.py is the one-slab case)
    "cheby-8x8-tiny-three-slabs": (lambda: forms._cheby(8, 8, 4), 300, False, {
        "kan_tiny_bwd_weight_kernel<1, 8>", "kan_slab_reduce_kernel"}),
    # 96 wave units x 11 >= 4 * 256, so three column tiles per wave stay; one group and fp32, so the register ring and not LDS-DMA
    "cheby-768x384-three-tiles": (lambda: forms._cheby(768, 384, 4), 704, False, {
        "kan_bwd_weight_reg_kernel<1, 5, 3, false, 5, false>", "kan_slab_reduce_kernel"}),
    # the 16-row kernel with four 16-column tiles per wave
    "kanlinear-64x64-reg16": (lambda: _kanlinear(64, 64), 300, False, {
        "kan_bwd_weight_reg16_kernel<2, 9, 3, 4>", "kan_slab_reduce_kernel"}),
    # two 16-column tiles divide by neither 12 nor 4: the exact 32-row kernel, two windows of five basis slots
    "kanlinear-64x32-exact-32-row": (lambda: _kanlinear(64, 32), 300, False, {
        "kan_bwd_weight_reg_kernel<2, 9, 2, false, 5, false>", "kan_slab_reduce_kernel"}),
    # B-splines under the bf16 flag: the same two windows on the bf16 matrix cores
    "bf16-kanlinear-64x64": (lambda: _kanlinear(64, 64), 300, True, {
        "kan_bwd_weight_reg_kernel<2, 9, 2, true, 5, false>", "kan_slab_reduce_kernel"}),
    # one row below the register kernels' threshold: the LDS-tile kernel, two 128-row splits
    "cheby-64x64-M255-tile": (lambda: forms._cheby(64, 64, 4), 255, False, {
        "kan_bwd_weight_kernel<1, 1, false>", "kan_slab_reduce_kernel"}),
    # at the threshold: the register kernel (one column tile per wave: the launch cannot fill the chip)
    "cheby-64x64-M256-register": (lambda: forms._cheby(64, 64, 4), 256, False, {
        "kan_bwd_weight_reg_kernel<1, 5, 1, false, 5, false>", "kan_slab_reduce_kernel"}),
}


@pytest.mark.parametrize("case", list(LAYER_CASES))
def test_weight_form_runs_named_and_matches_fp64_oracle(case, monkeypatch):
    make, m, bf16, expected = LAYER_CASES[case]
    torch.manual_seed(700 + len(case))
    layer = make().to(DEV)
    cfg = layer.kan_cfg()
    x = torch.randn(m, cfg.I)
    w = torch.randn(m, cfg.O)
    y, dx, grads, names = forms._run(layer, x, w, bf16, record=True)
    names = _weight_kernels(names)
    print(f"\n{case}: {sorted(names)}")
    monkeypatch.setattr(shapes, "_oracle", lambda layer_, _h, *a, **kw: forms._oracle(layer_, *a, **kw))      # the single-layer oracle
    if bf16:
        worst = shapes._check_bf16(case, layer, None, x, w, y, dx, grads)
    else:
        y2, dx2, grads2, _ = forms._run(layer, x, w, bf16)
        assert torch.equal(y, y2) and torch.equal(dx, dx2), (case, "fp32 results not reproducible")
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), (case, k, "fp32 gradient not reproducible")
        worst = shapes._check_fp32(case, layer, None, x, w, y, dx, grads)
    print(f"  worst {max(worst.items(), key=lambda kv: kv[1])}")
    assert names == expected, (case, sorted(names ^ expected))


def test_lds_dma_form_and_its_misaligned_fallback(monkeypatch):
    """One head's q|k|v (groups = 3) at M = 300 under KANVIT_BW_DMA_FORCE: the LDS-DMA kernel; the same call with the rows of x four
    bytes off the 16-byte grid (a contiguous view one float into a buffer: row stride still 64 floats) runs the register ring under the
    same plan -- same slab count, same workspace.  (kanvit.ops copies a column-offset view such as xfull[:, 1:] to a fresh aligned
    tensor, so that view never reaches the library misaligned.)  Both against the oracle, bitwise reproducible, and within 1e-5 of
    the KANVIT_BW_NO_DMA run."""
    from attention import MSA
    from kanvit import _lib, grouped
    torch.manual_seed(64)
    m, d = 300, 64
    msa = MSA(d, 1, type="cheby").to(DEV)
    x = torch.randn(m, d)
    w = torch.randn(m, 3 * d)
    flat = torch.empty(m * d + 4, device=DEV)
    views = {"aligned": flat[:m * d].view(m, d), "misaligned": flat[1:1 + m * d].view(m, d)}
    assert views["aligned"].data_ptr() % 16 == 0 and views["misaligned"].data_ptr() % 16 == 4 and views["misaligned"].is_contiguous()

    def run(view, record=False):
        msa.zero_grad(set_to_none=True)
        xg = view.copy_(x).detach().requires_grad_(True)
        assert xg.data_ptr() == view.data_ptr()
        with record_kernels() if record else contextlib.nullcontext(set()) as names:
            y = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, xg)
            (y * w.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().cpu() for k, p in msa.named_parameters() if p.grad is not None}
        return y.detach().cpu(), xg.grad.detach().cpu(), grads, _weight_kernels(names)

    monkeypatch.delenv("KANVIT_BW_NO_DMA", raising=False)
    monkeypatch.setenv("KANVIT_BW_DMA_FORCE", "1")
    _lib.reload_config()
    try:
        assert "bw_dma_force=1" in _lib.active_config()
        res = {k: run(v, record=True) for k, v in views.items()}
        again = {k: run(v) for k, v in views.items()}
        monkeypatch.setenv("KANVIT_BW_NO_DMA", "1")
        _lib.reload_config()
        ring = {k: run(v, record=True) for k, v in views.items()}
    finally:
        monkeypatch.delenv("KANVIT_BW_DMA_FORCE", raising=False)
        monkeypatch.delenv("KANVIT_BW_NO_DMA", raising=False)
        _lib.reload_config()
    for k, (y, dx, grads, names) in res.items():
        print(f"\nq|k|v M={m} {k}: {sorted(names)}; KANVIT_BW_NO_DMA: {sorted(ring[k][3])}")
        assert torch.equal(y, again[k][0]) and torch.equal(dx, again[k][1]), (k, "fp32 results not reproducible")
        for key in grads:
            assert torch.equal(grads[key], again[k][2][key]), (k, key, "fp32 gradient not reproducible")
            r = ring[k][2][key]
            assert float((grads[key] - r).abs().max()) / float(r.abs().max()) < 1e-5, (k, key)
        worst = shapes._check_fp32("cheby", msa, 1, x, w, y, dx, grads)
        print(f"  worst {max(worst.items(), key=lambda kv: kv[1])}")
    reg = {"kan_bwd_weight_reg_kernel<1, 5, 3, false, 5, false>", "kan_slab_reduce_kernel"}
    assert res["aligned"][3] == {"kan_bwd_weight_dma_kernel<1, 5, 3, false>", "kan_slab_reduce_kernel"}, sorted(res["aligned"][3])
    assert res["misaligned"][3] == reg, sorted(res["misaligned"][3])
    assert ring["aligned"][3] == reg and ring["misaligned"][3] == reg, (sorted(ring["aligned"][3]), sorted(ring["misaligned"][3]))


# id -> (family, d_hidden, bf16, the weight-gradient kernels of one backward of the patch embedding)
PATCH_CASES = {
    # the gathering kernel: x rows from the images, dY rows from the token-sequence gradient
    "cheby-patch-gather": ("cheby", 64, False, {
        "kan_bwd_weight_reg_kernel<1, 5, 1, false, 5, true>", "kan_slab_reduce_kernel"}),
    # bf16 mode keeps the patch matrix: the non-gather kernel on the bf16 matrix cores
    "bf16-cheby-patch-matrix": ("cheby", 64, True, {
        "kan_bwd_weight_reg_kernel<1, 5, 1, true, 5, false>", "kan_slab_reduce_kernel"}),
    # SineKAN at grid 28: the weight pass and its x * cos twin (KANVIT_FLAG_SINE_DFREQ: d loss / d freq), both gathering
    "sine-patch-gather-dfreq": ("sine", 128, False, {
        "kan_bwd_weight_reg_kernel<4, 28, 4, false, 4, true>", "kan_bwd_weight_reg_kernel<6, 28, 4, false, 4, true>",
        "kan_slab_reduce_kernel"}),
}


@pytest.mark.parametrize("case", list(PATCH_CASES))
def test_patch_embedding_weight_form_runs_named_and_matches_fp64_oracle(case, monkeypatch):
    """The patch embedding of a VisionTransformer: one 32 x 32 channel, 4 patches per side (I = 64), 19 images (M = 304)."""
    from model import VisionTransformer
    fam, d, bf16, expected = PATCH_CASES[case]
    chw, npatch, b = (1, 32, 32), 4, 19
    torch.manual_seed(900 + len(case))
    vit = VisionTransformer(chw, n_patches=npatch, n_blocks=1, d_hidden=d, n_heads=2, out_d=10, type=fam).to(DEV)
    layer = vit.linear_mapper
    images = torch.randn(b, *chw)
    wgt = torch.randn(b, npatch * npatch + 1, d)

    def run(record=False):
        vit.zero_grad(set_to_none=True)
        with record_kernels() if record else contextlib.nullcontext(set()) as names:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
                tok = vit._embed(images.to(DEV))
            (tok.float() * wgt.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().cpu() for k, p in layer.named_parameters() if p.grad is not None}
        return tok.detach().float().cpu(), grads, _weight_kernels(names)

    tok, grads, names = run(record=True)
    print(f"\n{case}: {sorted(names)}")
    # the layer's own rows: the patch matrix, the loss weights of the patch tokens, y = tokens - position embedding (in float64)
    x = ko.patchify(images.double(), npatch).reshape(-1, layer.kan_cfg().I).float()
    w = wgt[:, 1:, :].reshape(-1, d)
    y = (tok[:, 1:, :].double() - vit.pos_embeddings[1:npatch * npatch + 1].cpu().double()).reshape(-1, d)

    def oracle(layer_, _h, x_, w_, got_y, _got_dx, rounded):
        ey, _, gp = forms._oracle(layer_, x_, w_, got_y, torch.zeros_like(x_), rounded)
        return ey, _Err(), gp          # the images are data: the patch embedding has no input gradient to compare

    monkeypatch.setattr(shapes, "_oracle", oracle)
    if bf16:
        worst = shapes._check_bf16(fam, layer, None, x, w, y, None, grads)
    else:
        tok2, grads2, _ = run()
        assert torch.equal(tok, tok2), (case, "fp32 results not reproducible")
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), (case, k, "fp32 gradient not reproducible")
        worst = shapes._check_fp32(fam, layer, None, x, w, y, None, grads)
    print(f"  worst {max(worst.items(), key=lambda kv: kv[1])}")
    assert names == expected, (case, sorted(names ^ expected))
