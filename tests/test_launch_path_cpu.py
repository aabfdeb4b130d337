"""The Python launch path of kanvit.ops / kanvit.dense without a GPU and without a library launch: the one scratch allocator rounds
up, its rounding-down predecessor is gone from the sources, and the two spline-fit wrappers that share one body still refuse bad
operands in their own names."""
import os

import pytest
import torch

from kanvit import ops

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kan-vit_amd", "kanvit")


@pytest.mark.parametrize("n", [0, 1, 5, 16, 18])
def test_workspace_rounds_up_and_has_a_floor(n):
    ws = ops._workspace(n, "cpu")
    nbytes = ws.numel() * ws.element_size()
    assert nbytes >= n and nbytes >= 16
    assert ws.dtype == torch.float32 and ws.device.type == "cpu"


@pytest.mark.parametrize("name", ["ops.py", "dense.py"])
def test_no_rounding_down_allocation_left(name):
    with open(os.path.join(PKG, name)) as f:
        assert "nbytes // 4" not in f.read()


I, O, NB, ORDER = 5, 4, 8, 3                              # grid_size 5 + spline_order 3
NK = NB + ORDER + 1
CFG = ops.LayerCfg(family=ops.BSPLINE, I=I, O=O, G=NB, spline_order=ORDER)


def _fit(name, x=None, w_old=None, cfg=CFG, old=None, new=None):
    """Call ops.bspline_refit / ops.bspline_regrid (old basis 8 -> new basis 8) with well-formed operands except those given."""
    x = torch.zeros(6, I) if x is None else x
    w_old = torch.zeros(1, I * NB, O) if w_old is None else w_old
    old = torch.zeros(1, I * NK) if old is None else old
    new = torch.zeros(1, I, NK) if new is None else new
    if name == "bspline_refit":
        return ops.bspline_refit(x, w_old, cfg, old, new)
    return ops.bspline_regrid(x, w_old, cfg, NB, old, new)


@pytest.fixture
def any_device(monkeypatch):
    """The operand checks that follow the device test are reached with CPU tensors: the device test is switched off, and every
    case below is refused before anything would be launched."""
    monkeypatch.setattr(ops, "_require_gpu_f32", lambda name, t: None)


@pytest.mark.parametrize("name", ["bspline_refit", "bspline_regrid"])
def test_spline_fit_refuses_other_families(name):
    with pytest.raises(NotImplementedError) as e:                 # precedes the device test: plain CPU tensors
        _fit(name, cfg=ops.LayerCfg(family=ops.CHEBY, I=I, O=O, G=NB))
    assert str(e.value) == f"{name}: family cheby has no knot table to refit (bspline only)"


@pytest.mark.parametrize("name", ["bspline_refit", "bspline_regrid"])
def test_spline_fit_keeps_the_device_test(name):
    with pytest.raises(ops.KanvitError, match="x is on cpu"):
        _fit(name)


@pytest.mark.parametrize("name", ["bspline_refit", "bspline_regrid"])
def test_spline_fit_refuses_bad_x(name, any_device):
    with pytest.raises(ops.KanvitError) as e:
        _fit(name, x=torch.zeros(2, 3, I))
    assert str(e.value) == f"{name}: x must be 2-D, got (2, 3, {I})"
    with pytest.raises(ops.KanvitError) as e:
        _fit(name, x=torch.zeros(6, I - 1))
    assert str(e.value) == f"{name}: x has {I - 1} columns, expected {I}"


def test_refit_refuses_bad_weights_and_knots(any_device):
    with pytest.raises(ops.KanvitError) as e:
        _fit("bspline_refit", w_old=torch.zeros(1, I * NB + 1, O))
    assert str(e.value) == f"bspline_refit: packed weight shape (1, {I * NB + 1}, {O}) != (1, {I * NB}, {O})"
    both = f"do not hold [1][{I}*{NK}] / [1][{I}][{NK}]"
    with pytest.raises(ops.KanvitError) as e:
        _fit("bspline_refit", old=torch.zeros(1, I * NK - 1))
    assert str(e.value) == f"bspline_refit: knot tables (1, {I * NK - 1}) / (1, {I}, {NK}) " + both
    with pytest.raises(ops.KanvitError) as e:
        _fit("bspline_refit", new=torch.zeros(1, I, NK - 1))
    assert str(e.value) == f"bspline_refit: knot tables (1, {I * NK}) / (1, {I}, {NK - 1}) " + both


def test_regrid_refuses_bad_weights_and_knots(any_device):
    with pytest.raises(ops.KanvitError) as e:
        _fit("bspline_regrid", w_old=torch.zeros(1, I * NB + 1, O))
    assert str(e.value) == f"bspline_regrid: old packed weight shape (1, {I * NB + 1}, {O}) != (1, {I * NB}, {O}) (old nb={NB})"
    with pytest.raises(ops.KanvitError) as e:
        _fit("bspline_regrid", old=torch.zeros(2, I * NK))                    # one table per group
    assert str(e.value) == f"bspline_regrid: old knot table (2, {I * NK}) does not hold [1][{I}*{NK}]"
    with pytest.raises(ops.KanvitError) as e:
        _fit("bspline_regrid", old=torch.zeros(1, I * NK - 1))
    assert str(e.value) == f"bspline_regrid: old knot table (1, {I * NK - 1}) does not hold [1][{I}*{NK}]"
    with pytest.raises(ops.KanvitError) as e:
        _fit("bspline_regrid", new=torch.zeros(1, I, NK - 1))
    assert str(e.value) == f"bspline_regrid: new knot table (1, {I}, {NK - 1}) != [1][{I}][{NK}]"
