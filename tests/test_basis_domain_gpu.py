"""Every restatement of the KAN basis families in csrc/kan_basis.h -- basis_fwd / basis_bwd (LDS-tile kernels), BasisGen and
BasisDGen (register and tiny kernels, fp32 and bf16), BasisGenP (weight gradient, windowed for G = 28), basis_bwd_sine_reg, the
private copies of the edge-L1 and refit kernels -- over its whole argument range: x bit-exactly on a knot and one ulp beside it,
outside the grid, saturated tanh, sine arguments to +-250, trained frequencies (one 0, one negative), base activations to
+-100, grids other than [-1, 1] / 5, a NaN row.  Inputs and float64 closed-form references: tests/_basis_domain.py.

The calls are kanvit.ops.kan_layer on packed operands.  Forward and input gradient use feature-diagonal weights
(w[i*GP + j][o] = delta(i, o) c[o][j], 0.5 <= |c| <= 1): y[m, o] and dx[m, i] are then univariate functions of one x, and a
failure prints that x.  The weight gradient and SineKAN's d loss / d freq (both routes) use dense random weights and dy.  Every
case asserts the kernel family that ran (tests/_util.record_kernels) by name stem and leading family template argument; the
exact literal sets stay with tests/test_layer_forms_gpu.py and tests/test_weight_forms_gpu.py, whose shapes these are.

Bounds are the suite's: fp32 forward max|err| < 2e-5 max(1, max|ref|), fp32 gradients max|err| / max|ref| < 1e-4
(tests/test_layers_gpu.py); bf16 TIGHT = 2e-3 against the operand-rounded reference and > 0 against the unrounded one
(tests/test_bf16_oracle_gpu.py).  No point of a sweep is left out of a comparison; entries whose x is >= 999 in magnitude (the
base column is O(|x|) there, up to 1e30) are held to the same bound against THEIR largest reference entry instead of hiding the
rest of the matrix behind it.  The only exclusion is the poisoned row of the NaN test."""
import contextlib
import re
from dataclasses import replace

import pytest
import torch

from tests import _basis_domain as bd
from tests._util import record_kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD, TOL, TIGHT = 2e-5, 1e-4, 2e-3
M = 300
FAM = {"cheby": 1, "bspline": 2, "rbf": 3, "sine": 4, "fourier": 5}
SINE_DF = 6           # the weight-gradient kernels' x cos(x f + p) operand (d loss / d freq through a weight pass)

REG = ("kan_fwd_reg", "kan_bwd_input_reg")
TILE = ("kan_fwd", "kan_bwd_input")
TINY = ("kan_tiny_fwd", "kan_tiny_bwd_input")
NO_REG = {"KANVIT_NO_REG": "1"}


@contextlib.contextmanager
def _switches(env, monkeypatch):
    from kanvit import _lib
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _lib.reload_config()
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
        _lib.reload_config()


def _ran(names, stem, fam, act=False, bf16=None):
    """A recorded kernel `<stem>[_act]_kernel<fam, ...>` (bf16: the last template argument of the LDS-tile kernels)."""
    pat = re.compile(r"^%s%s_kernel<%d,.*%s>$" % (re.escape(stem), "_act" if act else "", fam, {None: "", True: "true", False: "false"}[bf16]))
    return any(pat.match(n) for n in names)


def _worst_point(got, ref, x, cls):
    """The x whose entry is worst in the class that fails, for the assertion message."""
    d = (got.double() - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    out = []
    for sel in (cls, ~cls):
        if bool(sel.any()):
            k = int(torch.where(sel, d, torch.full_like(d, -1.0)).argmax())
            out.append("x=%r err=%.3e ref=%.6e" % (float(x.flatten()[k]), float(d.flatten()[k]), float(ref.flatten()[k])))
    return "; ".join(out)


def _run(name, i, o, weights, bf16=False, x_grad=True, base=True):
    """One forward + backward of ops.kan_layer on the layer's input set.  Returns the operands, the float64 references and what the
    GPU computed."""
    from kanvit import ops
    layer = bd.make_layer(name, i, o)
    p = bd.params_of(layer)
    x, u, _, _ = bd.input_set(name, layer, M)
    if not base:                # the layer without its base column (what KANLinear.b_splines launches): y is the spline path alone
        p = {**p, "act": None, "GP": p["G"]}
    gp = p["GP"]
    if weights == "diag":
        w3 = bd.diag_weights(i, gp, o)
        dy = (0.5 + 0.5 * torch.rand(M, o, generator=torch.Generator().manual_seed(7))) * (1 - 2 * (torch.arange(o) % 2))
    else:
        g = torch.Generator().manual_seed(11)
        w3 = torch.randn(i, gp, o, generator=g) / (i * gp) ** 0.5
        dy = torch.randn(M, o, generator=g)
    layer = layer.to(DEV)
    cfg = layer.kan_cfg() if base else replace(layer.kan_cfg(), has_base=0, base_act=0)
    _, bp, _ = layer.kan_pack()
    sine = p["family"] == "sine"
    w = w3.reshape(1, i * gp, o).to(DEV).requires_grad_(weights == "dense")
    bpar = None if bp is None else bp.detach().reshape(1, -1).clone().requires_grad_(sine and weights == "dense")
    xg = x.to(DEV).requires_grad_(x_grad)
    ug = None if u is None else u.to(DEV).requires_grad_(x_grad)
    with record_kernels() as names:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            y = ops.kan_layer(xg, w, cfg, u=ug, bparams=bpar)
        (y.float() * dy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = {"y": y.detach().float().cpu(), "dx": xg.grad.cpu() if x_grad else None, "du": ug.grad.cpu() if ug is not None and x_grad else None,
           "dw": w.grad.cpu().reshape(i, gp, o) if w.grad is not None else None,
           "dfreq": bpar.grad.cpu()[0, :p["G"]] if bpar is not None and bpar.grad is not None else None}
    return {"p": p, "x": x, "u": u, "w3": w3, "dy": dy, "cfg": cfg, "got": got, "names": {n for n in names if n.startswith("kan_")}}


def _check(tag, r, bf16=False):
    """y, dx, du, dW and d freq of a run against the float64 closed forms; returns {quantity: share of its bound used}."""
    p, x, u, got = r["p"], r["x"], r["u"], r["got"]
    phi, dphi, dphi_u, dphi_f = bd.basis(p, x, u)
    rnd = (lambda t: t.float().to(torch.bfloat16).double()) if bf16 else None
    y, dx, du, dw, dl = bd.contract(phi, dphi, r["w3"], r["dy"], dphi_u, rnd)
    xcls = bd.huge(x)
    if u is not None:
        xcls = xcls | bd.huge(u)
    o = y.shape[1]
    diag = got["dw"] is None
    ycls = xcls[:, :o] if diag and o <= x.shape[1] else xcls.any(1, keepdim=True).expand(-1, o)
    used = {}
    if bf16:
        used["y"] = bd.rel_err(got["y"], y, ycls, floor=1e-30) / TIGHT
        y_e = bd.contract(phi, dphi, r["w3"], r["dy"], dphi_u)[0]
        assert bd.fwd_err(got["y"], y_e, ycls) > 0, (tag, "the bf16 result equals the unrounded reference: the bf16 kernel did not run")
    else:
        used["y"] = bd.fwd_err(got["y"], y, ycls) / FWD
    gtol = TIGHT if bf16 else TOL
    floor = 1e-30 if bf16 else 1e-3
    if got["dx"] is not None:
        used["dx"] = bd.rel_err(got["dx"], dx, xcls, floor) / gtol
    if got["du"] is not None:
        used["du"] = bd.rel_err(got["du"], du, xcls, floor) / gtol
    if got["dw"] is not None:
        wcls = torch.zeros(dw.shape, dtype=torch.bool)
        if p.get("act") is not None:
            wcls[:, -1, :] = True                               # the base column, whose operand is O(|x|), apart from the basis columns
        used["dw"] = bd.rel_err(got["dw"], dw, wcls, floor) / gtol
    if got["dfreq"] is not None:
        used["dfreq"] = bd.rel_err(got["dfreq"], (dl * dphi_f).sum((0, 1)), None, floor) / gtol
    print(f"\n{tag}: {sorted(r['names'])}\n  share of the bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    for k, v in used.items():
        where = ""
        if k == "y" and diag and o <= x.shape[1]:
            where = _worst_point(got["y"], y, x[:, :o], ycls)
        elif k == "dx":
            where = _worst_point(got["dx"], dx, x, xcls)
        elif k == "du":
            where = _worst_point(got["du"], du, u, xcls)
        assert v < 1.0, (tag, k, v, where)
    return used


# ---- forward and input gradient: feature-diagonal weights -------------------------------------------------------------------------
# id -> (layer of tests/_basis_domain.LAYERS, I, O, switches, (forward stem, input-gradient stem))
DIAG = {
    # register kernels: BasisGen / BasisDGen with a compile-time basis size
    "reg/cheby-deg4": ("cheby-deg4", 64, 64, {}, REG),
    "reg/bspline": ("bspline[-1,1]/5", 64, 64, {}, REG),
    "reg/rbf": ("rbf", 64, 64, {}, REG),
    "reg/sine-grid4": ("sine-grid4", 64, 64, {}, REG),                     # basis_bwd_sine_reg's twin in the register input gradient
    "reg/sine-grid4-trained": ("sine-grid4-trained", 64, 64, {}, REG),
    "reg/sine-grid28-first": ("sine-grid28-first", 64, 64, {}, REG),
    "reg/sine-grid28-first-trained": ("sine-grid28-first-trained", 64, 64, {}, REG),
    "reg/fourier-G28": ("fourier-G28", 64, 64, {}, REG),
    # run-time basis size in the register forward, no register input gradient for these GP
    "reg-rt/cheby-deg3": ("cheby-deg3", 64, 64, {}, ("kan_fwd_reg", "kan_bwd_input")),
    "reg-rt/fourier-G3": ("fourier-G3", 64, 64, {}, ("kan_fwd_reg", "kan_bwd_input")),
    # LDS-tile kernels: basis_fwd / basis_bwd (and basis_bwd_sine_reg for SINE with G <= 32)
    "tile/cheby-deg4-64x48": ("cheby-deg4", 64, 48, {}, TILE),
    "tile/bspline-64x48": ("bspline[-1,1]/5", 64, 48, {}, TILE),
    "tile/cheby-deg4": ("cheby-deg4", 64, 64, NO_REG, TILE),
    "tile/bspline": ("bspline[-1,1]/5", 64, 64, NO_REG, TILE),
    "tile/rbf": ("rbf", 64, 64, NO_REG, TILE),
    "tile/sine-grid4-trained": ("sine-grid4-trained", 64, 64, NO_REG, TILE),
    "tile/sine-grid28-first-trained": ("sine-grid28-first-trained", 64, 64, NO_REG, TILE),
    "tile/fourier-G3": ("fourier-G3", 64, 64, NO_REG, TILE),
    "tile/fourier-G28": ("fourier-G28", 64, 64, NO_REG, TILE),
    # tiny kernels: BasisGen / BasisDGen with a run-time basis size on the vector pipe
    "tiny/cheby-deg4": ("cheby-deg4", 8, 8, {}, TINY),
    "tiny/bspline": ("bspline[-1,1]/5", 8, 8, {}, TINY),
    "tiny/fourier-G3": ("fourier-G3", 8, 8, {}, TINY),
}
DIAG.update({"act/" + n: (n, 64, 64, {}, REG) for n in bd.LAYERS if n[n.find("-") + 1:] in bd.ACTS})      # the base column to +-100
DIAG.update({"act-tile/" + n: (n, 64, 64, NO_REG, TILE) for n in ("bspline-gelu_tanh", "rbf-gelu")})


@pytest.mark.parametrize("case", list(DIAG))
def test_forward_and_input_gradient_over_the_whole_argument_range(case, monkeypatch):
    name, i, o, env, (fwd, bwi) = DIAG[case]
    with _switches(env, monkeypatch):
        r = _run(name, i, o, "diag")
    _check(case, r)
    fam, act = FAM[r["p"]["family"]], case.startswith("act") and not name.endswith("silu")      # SiLU: the kernels without _act_
    assert _ran(r["names"], fwd, fam, act), (case, "forward", sorted(r["names"]))
    assert _ran(r["names"], bwi, fam, act), (case, "input gradient", sorted(r["names"]))


# ---- B-spline grids: which evaluation ran (models/effkan.py _grid_facts), one bound for both ---------------------------------------
# id -> (layer, closed form?, switches, (forward stem, input-gradient stem))
# (the register input gradient exists for the 8 + 1 columns of grid_size = 5 only)
GRIDS = {bd.grid_name(g): (bd.grid_name(g), g[0] < 100, {}, ("kan_fwd_reg" if g[0] < 100 else "kan_fwd",
                                                             "kan_bwd_input_reg" if g[2] == 5 and g[0] < 100 else "kan_bwd_input"))
         for g in bd.BSPLINE_GRIDS}
GRIDS.update({
    "perturbed-knots": ("bspline-perturbed", False, {}, TILE),                   # kv_bspline_fixed<12, 3>
    "order-2": ("bspline-order2", False, {}, TILE),                             # kv_bspline_rt
    "tile/bspline[-1,1]/3": ("bspline[-1,1]/3", True, NO_REG, TILE),            # the closed form inside basis_fwd / basis_bwd
    "tile/bspline[-1,1]/30": ("bspline[-1,1]/30", True, NO_REG, TILE),
})


# The same grids without the base column.  With it y is silu(x) c + splines: on a grid at x ~ 1000 one float32 ulp of y is 6e-5 and
# the forward bound 2e-2, so only dx can see a basis error of 1e-4 there; without it y is the four live bases alone, O(1).
GRIDS.update({"no-base/" + bd.grid_name(g): (bd.grid_name(g), g[0] < 100, {}, ("kan_fwd_reg" if g[0] < 100 else "kan_fwd", "kan_bwd_input"))
              for g in bd.BSPLINE_GRIDS})


@pytest.mark.parametrize("case", list(GRIDS))
def test_bspline_grids_take_the_evaluation_that_meets_the_bound(case, monkeypatch):
    from kanvit import _lib
    name, closed_form, env, (fwd, bwi) = GRIDS[case]
    with _switches(env, monkeypatch):
        r = _run(name, 64, 64, "diag", base=not case.startswith("no-base"))
    assert bool(r["cfg"].flags & _lib.FLAG_UNIFORM_KNOTS) == closed_form, (case, "closed form" if closed_form else "Cox-de Boor", "expected")
    print(f"\n{case}: {'closed form' if closed_form else 'Cox-de Boor'}")
    _check(case, r)
    assert _ran(r["names"], fwd, 2), (case, "forward", sorted(r["names"]))
    assert _ran(r["names"], bwi, 2), (case, "input gradient", sorted(r["names"]))


# ---- weight gradient and d loss / d freq: dense weights ------------------------------------------------------------------------------
# id -> (layer, I, O, switches, weight-gradient stem)
DENSE = {
    "reg/cheby-deg4": ("cheby-deg4", 64, 64, {}, "kan_bwd_weight_reg"),
    "reg16/bspline": ("bspline[-1,1]/5", 64, 64, {}, "kan_bwd_weight_reg16"),
    "reg-two-windows/bspline-64x32": ("bspline[-1,1]/5", 64, 32, {}, "kan_bwd_weight_reg"),      # BasisGenP with compile-time window starts
    "reg16/rbf": ("rbf", 64, 64, {}, "kan_bwd_weight_reg16"),
    "reg/sine-grid4-trained": ("sine-grid4-trained", 64, 64, {}, "kan_bwd_weight_reg"),
    "reg-windows/sine-grid28-first-trained": ("sine-grid28-first-trained", 64, 128, {}, "kan_bwd_weight_reg"),      # windowed starts, G = 28
    "reg-windows/fourier-G28": ("fourier-G28", 64, 128, {}, "kan_bwd_weight_reg"),
    "tile/cheby-deg4": ("cheby-deg4", 64, 64, NO_REG, "kan_bwd_weight"),
    "tile/bspline": ("bspline[-1,1]/5", 64, 64, NO_REG, "kan_bwd_weight"),
    "tile/bspline-perturbed": ("bspline-perturbed", 64, 64, {}, "kan_bwd_weight"),
    "tile/bspline[1000,1001]/5": ("bspline[1000,1001]/5", 64, 64, {}, "kan_bwd_weight"),
    "tile/rbf": ("rbf", 64, 64, NO_REG, "kan_bwd_weight"),
    "tile/sine-grid4-trained": ("sine-grid4-trained", 64, 64, NO_REG, "kan_bwd_weight"),
    "tile/fourier-G3": ("fourier-G3", 64, 64, {}, "kan_bwd_weight"),
    "tiny/cheby-deg4": ("cheby-deg4", 8, 8, {}, "kan_tiny_bwd_weight"),
    "tiny/bspline": ("bspline[-1,1]/5", 8, 8, {}, "kan_tiny_bwd_weight"),
    "tiny/fourier-G3": ("fourier-G3", 8, 8, {}, "kan_tiny_bwd_weight"),
}


@pytest.mark.parametrize("case", list(DENSE))
def test_weight_gradient_over_the_whole_argument_range(case, monkeypatch):
    name, i, o, env, bww = DENSE[case]
    with _switches(env, monkeypatch):
        r = _run(name, i, o, "dense")
        fam = FAM[r["p"]["family"]]
        used = _check(case, r)
        assert _ran(r["names"], bww, fam), (case, "weight gradient", sorted(r["names"]))
        if fam == FAM["sine"]:
            # with dx wanted, d freq comes out of the input-gradient kernel; when nobody needs dx it is a weight-gradient pass over
            # x cos(x f + p) wherever the register weight-gradient kernel runs (ops._kan_backward)
            assert "dfreq" in used and not _ran(r["names"], bww, SINE_DF), (case, sorted(r["names"]))
            r2 = _run(name, i, o, "dense", x_grad=False)
            used2 = _check(case + " (x needs no gradient)", r2)
            assert "dfreq" in used2 and _ran(r2["names"], bww, SINE_DF) == (not env), (case, "d freq route", sorted(r2["names"]))


# ---- one bf16 register case per family --------------------------------------------------------------------------------------------------
BF16 = {
    "cheby-deg4": ("kan_fwd_reg_bf16", "kan_bwd_input_res_bf16"),
    "bspline[-1,1]/5": ("kan_fwd_reg_bf16", "kan_bwd_input_res_bf16"),
    "rbf": ("kan_fwd_reg_bf16", "kan_bwd_input_res_bf16"),
    "sine-grid4-trained": ("kan_fwd_reg_bf16", "kan_bwd_input_reg_bf16"),
    "fourier-G28": ("kan_fwd_reg_bf16", "kan_bwd_input"),          # no bf16 register input gradient for FOURIER: the LDS-tile one, bf16 contraction
}


@pytest.mark.parametrize("name", list(BF16))
def test_bf16_register_kernels_over_the_whole_argument_range(name):
    fwd, bwi = BF16[name]
    r = _run(name, 64, 64, "diag", bf16=True)
    _check("bf16/" + name, r, bf16=True)
    fam = FAM[r["p"]["family"]]
    assert _ran(r["names"], fwd, fam), (name, "forward", sorted(r["names"]))
    assert _ran(r["names"], bwi, fam, bf16=True if bwi == "kan_bwd_input" else None), (name, "input gradient", sorted(r["names"]))


# ---- a NaN in one row stays in that row ---------------------------------------------------------------------------------------------------
def _default_layer(kind, i, o):
    from models.cheby import ChebyKANLayer
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    from models.nfkan import NaiveFourierKANLayer
    from models.sinekan import SineKANLayer
    torch.manual_seed(99)
    return {"cheby": lambda: ChebyKANLayer(i, o, 4), "efficientkan": lambda: KANLinear(i, o), "fast": lambda: FastKANLayer(i, o),
            "sine": lambda: SineKANLayer(i, o), "fourier": lambda: NaiveFourierKANLayer(i, o, gridsize=5)}[kind]()


@pytest.mark.parametrize("shape", [(64, 64), (64, 48)], ids=["register-64x64", "tile-64x48"])
@pytest.mark.parametrize("kind", ["cheby", "efficientkan", "fast", "sine", "fourier"])
def test_a_nan_poisons_its_own_row_only(kind, shape):
    """One NaN in one row of x (a middle row tile, so that first and last tiles hold clean rows only): that row of y is all NaN,
    every other row of y and dx is bitwise what the clean run gives.  Non-finite inputs are plain data to these kernels."""
    i, o = shape
    layer = _default_layer(kind, i, o).to(DEV)
    g = torch.Generator().manual_seed(5)
    x = 1.5 * torch.randn(M, i, generator=g)
    dy = torch.randn(M, o, generator=g).to(DEV)
    row, col = 137, 21

    def run(xin, record=False):
        xg = xin.to(DEV).requires_grad_(True)
        with record_kernels() if record else contextlib.nullcontext(set()) as names:
            y = layer(xg)
            (y * dy).sum().backward()
        torch.cuda.synchronize()
        return y.detach().cpu(), xg.grad.cpu(), {n for n in names if n.startswith("kan_")}

    y0, dx0, names = run(x, record=True)
    xp = x.clone()
    xp[row, col] = float("nan")
    y1, dx1, _ = run(xp)
    print(f"\n{kind} {i}x{o}: {sorted(names)}")
    # (SineKAN's default grid_size = 5 gives a parameter row of 5 * 65 floats, off the 16-byte grid the register forward prefetches
    # phases on: the LDS-tile forward at both shapes, the register input gradient at 64 x 64)
    stem = "kan_fwd_reg" if o == 64 and kind != "sine" else "kan_fwd"
    fam = {"cheby": 1, "efficientkan": 2, "fast": 3, "sine": 4, "fourier": 5}[kind]
    assert _ran(names, stem, fam), (kind, shape, sorted(names))
    if kind == "sine":
        assert _ran(names, "kan_bwd_input_reg" if o == 64 else "kan_bwd_input", fam), (kind, shape, sorted(names))
    assert torch.isfinite(y0).all() and torch.isfinite(dx0).all()
    assert bool(torch.isnan(y1[row]).all()), (kind, shape, "the poisoned row of y", y1[row])
    keep = torch.arange(M) != row
    assert torch.equal(y1[keep].view(torch.int32), y0[keep].view(torch.int32)), (kind, shape, "y of the clean rows changed")
    assert torch.equal(dx1[keep].view(torch.int32), dx0[keep].view(torch.int32)), (kind, shape, "dx of the clean rows changed")


# ---- the private copies of the B-spline evaluation: edge-L1 and refit kernels, on the knot-edge set ---------------------------------
@pytest.mark.parametrize("name", ["bspline[-1,1]/5", "bspline-perturbed"], ids=["closed-form", "cox-de-boor"])
def test_edge_l1_on_the_knot_edge_set(name):
    """ops.edge_l1 forward and backward (csrc/kan_edge_l1.hip evaluates the bases itself) on x bit-exactly on every knot, one ulp
    beside it and outside the grid.  Reference and bound are the edge-L1 tests' (tests/test_edge_l1_gpu.py: ref_phi in float64
    with autograd, max|err| <= 2e-6 + 1e-4 max|ref|), without their mask of sign-fragile samples: the spline weights are positive
    here, so every edge function is >= 0 and |phi| has no kink inside the grid; outside it phi and its derivative are both 0."""
    from dataclasses import replace
    from kanvit import _lib, ops
    from tests.test_edge_l1_gpu import assert_close_masked, f64_state, ref_phi
    i = o = 64
    layer = bd.make_layer(name, i, o)
    with torch.no_grad():
        layer.spline_weight.copy_(0.5 + 0.5 * torch.rand(layer.spline_weight.shape, generator=torch.Generator().manual_seed(3)))
        layer.spline_scaler.fill_(1.0)
    x, _, _, _ = bd.input_set(name, layer, M)
    gA = torch.rand(o, i, generator=torch.Generator().manual_seed(4)) + 0.5
    sd = f64_state(layer)
    x64 = x.double().requires_grad_()
    phi, _ = ref_phi(sd, "", x64)                                                       # [m, o, i]
    A_ref = phi.abs().mean(0)
    (A_ref * gA.double()).sum().backward()
    layer = layer.to(DEV)
    cfg = replace(layer.kan_cfg(), has_base=0, base_act=0)
    assert bool(cfg.flags & _lib.FLAG_UNIFORM_KNOTS) == (name == "bspline[-1,1]/5")
    w = layer.scaled_spline_weight.detach().permute(1, 2, 0).reshape(1, -1, o).clone().requires_grad_()
    xg = x.to(DEV).requires_grad_()
    with record_kernels() as names:
        A = ops.edge_l1(xg, w, cfg, layer.grid.reshape(1, -1))[0].t()                  # [o, i]
        (A * gA.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    print(f"\nedge_l1 {name}: {sorted(n for n in names if n.startswith('kan_'))}")
    assert _ran(names, "kan_edge_l1_fwd", 2) and _ran(names, "kan_edge_l1_bwd", 2), sorted(names)
    assert_close_masked(name + " A", A, A_ref)
    assert_close_masked(name + " dx", xg.grad, x64.grad)
    dw_ref = sd["spline_weight"].grad.permute(1, 2, 0).reshape(1, -1, o)              # spline_scaler is 1: the packed weight IS spline_weight
    assert_close_masked(name + " dw", w.grad, dw_ref)


def test_refit_gram_on_the_knot_edge_sets():
    """kanvit_bspline_refit_gram (csrc/kan_bspline_refit.hip evaluates the bases itself: the closed form for the OLD table, Cox-de
    Boor for the new one): N = Bnew^T Bnew and C = Bnew^T Bold in float64 on rows that lie bit-exactly on every knot of BOTH tables
    and one ulp beside them, against the float64 bases tests/_update_grid_ref.py uses (oracle bspline_bases).  Bound: the suite's
    gradient bound, max|err| / max|ref| < 1e-4 (both are sums of products over the rows)."""
    import ctypes as C
    from dataclasses import replace
    from kanvit import _lib, ops
    from oracle import kan_oracle as ko
    i = o = 64
    old_l, new_l = bd.make_layer("bspline[-1,1]/5", i, o), bd.make_layer("bspline-perturbed", i, o)
    x = torch.cat([bd.input_set("bspline[-1,1]/5", old_l, M)[0], bd.input_set("bspline-perturbed", new_l, M)[0]])
    nb, order = 8, 3
    bo = ko.bspline_bases(x.double(), old_l.grid.double(), order)
    bn = ko.bspline_bases(x.double(), new_l.grid.double(), order)
    n_ref, c_ref = torch.einsum("mij,mik->ijk", bn, bn), torch.einsum("mij,mik->ijk", bn, bo)
    old_l = old_l.to(DEV)
    cfg = replace(old_l.kan_cfg(), has_base=0, base_act=0)
    assert cfg.flags & _lib.FLAG_UNIFORM_KNOTS
    xg, old_k, new_k = x.to(DEV), old_l.grid.reshape(1, -1).contiguous(), new_l.grid.to(DEV).unsqueeze(0).contiguous()
    d = ops._desc(cfg, x.shape[0], i, 0, o, old_k.shape[1])
    gram_n = torch.empty(1, i, nb, nb, device=DEV, dtype=torch.float64)
    gram_c = torch.empty(1, i, nb, nb, device=DEV, dtype=torch.float64)
    L = _lib.lib()
    nbytes = int(L.kanvit_bspline_refit_workspace(C.byref(d)))
    ws = ops._workspace(nbytes, xg.device)
    with record_kernels() as names:
        ops.check(L.kanvit_bspline_refit_gram(C.byref(d), ops._ptr(xg), ops._ptr(old_k), ops._ptr(new_k), ops._ptr(gram_n), ops._ptr(gram_c),
                                              ops._ptr(ws), C.c_size_t(nbytes), ops._stream()), "kanvit_bspline_refit_gram")
    torch.cuda.synchronize()
    assert any(n.startswith("kan_bspline_refit_gram_kernel") for n in names), sorted(names)
    en, ec = bd.rel_err(gram_n[0].cpu(), n_ref), bd.rel_err(gram_c[0].cpu(), c_ref)
    print(f"\nrefit gram: N {en:.3e}, C {ec:.3e} (bound {TOL:.0e})")
    assert en < TOL and ec < TOL, (en, ec)
