"""Every kernel form that plan_layer_fwd / plan_layer_bwd_input (csrc/kan_layer.hip) choose for aligned, contiguous operands, run and
named: one single layer per form, through the Python modules (kanvit.ops.kan_layer underneath), at the smallest shape that takes
the branch.  Each case asserts

  * the exact set of kan_* kernels the forward and the backward launched (tests/_util.record_kernels), as literals.  They are what
    the library of the commit BEFORE the plans existed launches: this file was run on the GPU against that library
    (tools/build_variant.sh parent, KANVIT_LIB) with these literals and passed, so a plan that chooses another form fails here by
    name.  The forward and input-gradient names are the ones the plans' issue listed (none differed); the weight-gradient, weight
    repack and slab-reduction kernels of each case are listed too, because the set is exact (profiles/layer_plan_forms.md);
  * y, dx and every parameter gradient against the float64 oracle, with the suite's bounds (fp32: FWD / TOL; bf16: TIGHT against
    the bf16-operand oracle and LOOSE against the unrounded one -- tests/test_launch_shapes_gpu.py, whose _check_fp32 / _check_bf16 are called);
  * for fp32, a second run that is bitwise equal.

The shared-basis q|k|v form (row tiles x x_group_mod >= 256) and its launch tail already run at M = 2758 in
tests/test_launch_shapes_gpu.py::test_forced_tail_ragged_launch and are not repeated.  The weight-gradient forms that no case here
reaches (plan_layer_bwd_weight) are run and named in tests/test_weight_forms_gpu.py."""
import contextlib

import pytest
import torch

from oracle import kan_oracle as ko
from tests._util import record_kernels
from tests import test_launch_shapes_gpu as shapes
from tests.test_launch_shapes_gpu import CHUNK, _Err, _params64

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cheby(i, o, degree):
    from models.cheby import ChebyKANLayer
    return ChebyKANLayer(i, o, degree)


def _kanlinear_perturbed(i, o):
    """efficient-KAN with knots that are no longer g0 + j*h (still ascending): the general B-spline evaluation of the LDS-tile kernels"""
    from models.effkan import KANLinear
    layer = KANLinear(i, o)
    with torch.no_grad():
        nk = layer.grid.shape[1]
        layer.grid.add_(0.03 * torch.sin(torch.arange(nk, dtype=layer.grid.dtype))[None, :] * (1 + torch.arange(i, dtype=layer.grid.dtype)[:, None] % 3))
    return layer


def _fastkan(i, o):
    from models.fastkan import FastKANLayer
    layer = FastKANLayer(i, o)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():          # randomised, so a wrong gamma / beta index shows
        layer.layernorm.weight.copy_(1.0 + 0.3 * torch.randn(layer.layernorm.weight.shape, generator=g))
        layer.layernorm.bias.copy_(0.2 * torch.randn(layer.layernorm.bias.shape, generator=g))
    return layer


def _sine(i, o, grid):
    from models.sinekan import SineKANLayer
    return SineKANLayer(i, o, grid_size=grid)


# id -> (layer factory, rows, bf16, the kan_* kernels of one forward + backward: forward, input gradient, weight gradient and their helpers)
CASES = {
    # one column tile per work-group (the launch cannot fill the chip), compile-time basis size
    "cheby-64x64-deg4": (lambda: _cheby(64, 64, 4), 300, False, {
        "kan_fwd_reg_kernel<1, 1, 1, 4, 5, false>",
        "kan_bwd_input_reg_kernel<1, 5, 5, false>",
        "kan_bwd_weight_reg_kernel<1, 5, 1, false, 5, false>",
        "kan_slab_reduce_kernel"}),
    # run-time basis size in the register forward; no register input gradient for GP = 4
    "cheby-64x64-deg3": (lambda: _cheby(64, 64, 3), 300, False, {
        "kan_fwd_reg_kernel<1, 1, 1, 4, 0, false>",
        "kan_bwd_input_kernel<1, 3, false, false>",
        "kan_bwd_weight_kernel<1, 1, false>",
        "kan_slab_reduce_kernel"}),
    # I % 8 != 0: two features per lane half, run-time loop
    "cheby-36x64-deg4": (lambda: _cheby(36, 64, 4), 300, False, {
        "kan_fwd_reg_kernel<1, 1, 1, 2, 0, false>",
        "kan_bwd_input_kernel<1, 3, false, false>",
        "kan_bwd_weight_kernel<1, 1, false>",
        "kan_slab_reduce_kernel"}),
    # O = 48 is no whole number of column tiles: the LDS-tile kernels, predicated
    "cheby-64x48-deg4": (lambda: _cheby(64, 48, 4), 300, False, {
        "kan_fwd_kernel<1, 2, 1, false>",
        "kan_bwd_input_kernel<1, 3, false, false>",
        "kan_bwd_weight_kernel<1, 1, false>",
        "kan_slab_reduce_kernel"}),
    # the vector-pipe kernels
    "cheby-8x8-deg4-tiny": (lambda: _cheby(8, 8, 4), 100, False, {
        "kan_tiny_fwd_kernel<1, 8>",
        "kan_tiny_bwd_input_kernel<1, 8, 8>",
        "kan_tiny_bwd_weight_kernel<1, 8>"}),
    # non-uniform knots: LDS-tile kernels, fast variant
    "kanlinear-64x64-perturbed-knots": (lambda: _kanlinear_perturbed(64, 64), 300, False, {
        "kan_fwd_kernel<2, 2, 1, true>",
        "kan_bwd_input_kernel<2, 3, false, false>",
        "kan_bwd_weight_kernel<2, 1, false>",
        "kan_slab_reduce_kernel"}),
    # the fused-LayerNorm route: register kernels or nothing
    "fastkan-64x64-fused-ln": (lambda: _fastkan(64, 64), 300, False, {
        "kan_fwd_reg_kernel<3, 1, 1, 4, 9, false>",
        "kan_bwd_input_reg_kernel<3, 9, 5, false>",
        "kan_bwd_weight_reg16_kernel<3, 9, 9, 4>",
        "kan_slab_reduce_kernel",
        "kan_ln_bwd_kernel<1, 1>"}),
    # bf16 register forward, dY-resident input gradient
    "bf16-cheby-64x64": (lambda: _cheby(64, 64, 4), 300, True, {
        "kan_pack_w_fwd_reg_kernel",
        "kan_fwd_reg_bf16_kernel<1, 5, 2, 1, 8, false>",
        "kan_pack_w_bwd_reg_kernel",
        "kan_bwd_input_res_bf16_kernel<1, 5, 5, 1, false>",
        "kan_bwd_weight_reg_kernel<1, 5, 1, true, 5, false>",
        "kan_slab_reduce_kernel"}),
    # M >= 4096: the W-stationary forward
    "bf16-cheby-64x64-M4224": (lambda: _cheby(64, 64, 4), 4224, True, {
        "kan_pack_w_fwd_reg_kernel",
        "kan_fwd_ws_bf16_kernel<1, 5, 2, 1, 8, 4, true>",
        "kan_pack_w_bwd_reg_kernel",
        "kan_bwd_input_res_bf16_kernel<1, 5, 5, 1, false>",
        "kan_bwd_weight_reg_kernel<1, 5, 1, true, 5, false>",
        "kan_slab_reduce_kernel"}),
    # O = 32: the streaming bf16 input gradient
    "bf16-cheby-64x32": (lambda: _cheby(64, 32, 4), 300, True, {
        "kan_pack_w_fwd_reg_kernel",
        "kan_fwd_reg_bf16_kernel<1, 5, 1, 1, 8, false>",
        "kan_pack_w_bwd_reg_kernel",
        "kan_bwd_input_reg_bf16_kernel<1, 5, 5, false>",
        "kan_bwd_weight_reg_kernel<1, 5, 1, true, 5, false>",
        "kan_slab_reduce_kernel"}),
    # one wide layer: the 64-column chunks as a SHARED launch
    "bf16-cheby-64x128-wide": (lambda: _cheby(64, 128, 4), 300, True, {
        "kan_pack_w_fwd_reg_kernel",
        "kan_fwd_reg_bf16_kernel<1, 5, 4, 1, 8, false>",
        "kan_pack_w_bwd_reg_kernel",
        "kan_bwd_input_reg_bf16_kernel<1, 5, 5, true>",
        "kan_bwd_weight_reg_kernel<1, 5, 1, true, 5, false>",
        "kan_slab_reduce_kernel"}),
    # no bf16 register kernel for GP = 4: the LDS-tile bf16 kernels
    "bf16-cheby-64x64-deg3": (lambda: _cheby(64, 64, 3), 300, True, {
        "kan_pack_w_fwd_kernel",
        "kan_fwd_bf16_kernel<1, 2, 1>",
        "kan_pack_w_bwd_kernel",
        "kan_bwd_input_kernel<1, 3, false, true>",
        "kan_bwd_weight_kernel<1, 1, true>",
        "kan_slab_reduce_kernel"}),
    # SineKAN's per-head basis size
    "bf16-sine-64x64-grid4": (lambda: _sine(64, 64, 4), 300, True, {
        "kan_pack_w_fwd_reg_kernel",
        "kan_fwd_reg_bf16_kernel<4, 4, 2, 1, 8, false>",
        "kan_pack_w_bwd_reg_kernel",
        "kan_bwd_input_reg_bf16_kernel<4, 4, 4, false>",
        "kan_bwd_weight_reg_kernel<4, 4, 2, true, 4, false>",
        "kan_slab_reduce_kernel"}),
}


def _run(layer, x, w, bf16, record=False):
    layer.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    with record_kernels() if record else contextlib.nullcontext(set()) as names:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            y = layer(xg)
        (y.float() * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in layer.named_parameters() if p.grad is not None}
    return y.detach().float().cpu(), xg.grad.detach().cpu(), grads, {n for n in names if n.startswith("kan_")}


def _oracle(layer, x, w, got_y, got_dx, rounded):
    """float64 oracle on row chunks (loss sum(y * w): parameter gradients add up over the chunks)"""
    params = _params64(layer)
    ey, edx = _Err(), _Err()
    for r0 in range(0, x.shape[0], CHUNK):
        xd = x[r0:r0 + CHUNK].double().requires_grad_(True)
        with ko.operand_rounding(ko.bf16_round) if rounded else contextlib.nullcontext():
            y = ko.layer_forward(params, "", xd)
        (y * w[r0:r0 + CHUNK].double()).sum().backward()
        ey.add(got_y[r0:r0 + CHUNK], y.detach())
        edx.add(got_dx[r0:r0 + CHUNK], xd.grad)
    return ey, edx, {k: v.grad for k, v in params.items() if v.grad is not None}


@pytest.mark.parametrize("case", list(CASES))
def test_layer_form_runs_named_and_matches_fp64_oracle(case, monkeypatch):
    make, m, bf16, expected = CASES[case]
    torch.manual_seed(500 + len(case))
    layer = make().to(DEV)
    cfg = layer.kan_cfg()
    x = torch.randn(m, cfg.I)
    w = torch.randn(m, cfg.O)
    if "fused-ln" in case:
        from kanvit import ops
        assert ops.ln_fusable(cfg, m), "this shape is meant to take the fused-LayerNorm route"
    y, dx, grads, names = _run(layer, x, w, bf16, record=True)
    print(f"\n{case}: {sorted(names)}")
    # the suite's bounds, from the file that defines them: its two checks call its module-level _oracle(module, heads, ...), which is the
    # q|k|v oracle there and the single-layer one here
    monkeypatch.setattr(shapes, "_oracle", lambda layer_, _h, *a, **kw: _oracle(layer_, *a, **kw))
    fam = "sine" if "sine" in case else case
    if bf16:
        worst = shapes._check_bf16(fam, layer, None, x, w, y, dx, grads)
    else:
        y2, dx2, grads2, _ = _run(layer, x, w, bf16)
        assert torch.equal(y, y2) and torch.equal(dx, dx2), (case, "fp32 results not reproducible")
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), (case, k, "fp32 gradient not reproducible")
        worst = shapes._check_fp32(fam, layer, None, x, w, y, dx, grads)
    print(f"  worst {max(worst.items(), key=lambda kv: kv[1])}")
    assert names == expected, (case, sorted(names ^ expected))
