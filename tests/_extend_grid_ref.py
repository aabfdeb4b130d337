"""Float64 restatement of KANLinear.extend_grid (grid extension: the layer moves to another grid_size and keeps its function),
shared by tests/test_extend_grid_cpu.py and tests/test_extend_grid_gpu.py.  There is no reference implementation of this
feature, so the restatement is the yardstick; it is built on tests/_update_grid_ref.py (new_knots, pivot_ratios, forward64) and
oracle.kan_oracle.bspline_bases, in this project's own words: evaluate the layer's per-edge spline output on the OLD knots with
the nb_old old coefficients, and fit it on new_knots(x, new_grid_size, ...) by a float64 lstsq per feature.  A feature whose fit
on x does not exist (smallest Cholesky pivot ratio of its Gram matrix not above TAU) is fitted instead on
KANLinear.fallback_samples of its old knots, evaluated on the CPU, with its knots from new_knots of those samples."""
import torch

from oracle import kan_oracle as ko
from tests import _update_grid_ref as ug

TAU = ug.TAU


def scaled_weight(sd):
    w = sd["spline_weight"].double()
    return w * sd["spline_scaler"].double().unsqueeze(-1) if "spline_scaler" in sd else w


def fit(rows, sd, new_grid_size, order, grid_eps=0.02, margin=0.01):
    """(knots [in, nk_new], spline_weight [out, in, nb_new], pivot ratios [in]): the least-squares fit, on the samples rows[M, in],
    of the old layer's per-edge spline output by a spline on new_knots(rows, new_grid_size)."""
    r64 = rows.double()
    target = torch.einsum("mik,oik->imo", ko.bspline_bases(r64, sd["grid"].double(), order), scaled_weight(sd))     # [in, M, out]
    knots = ug.new_knots(rows, new_grid_size, order, grid_eps, margin)
    design = ko.bspline_bases(r64, knots, order).permute(1, 0, 2)                                                 # [in, M, nb_new]
    coeff = torch.linalg.lstsq(design, target).solution                                           # [in, nb_new, out]
    return knots, coeff.permute(2, 0, 1).contiguous(), ug.pivot_ratios(rows, knots, order)


def extend(x, sd, new_grid_size, order, grid_eps=0.02, margin=0.01, samples=256):
    """(knots [in, nk_new], spline_weight [out, in, nb_new], live [in] bool, pivot ratios on x [in], on the fallback samples [in])
    after extend_grid(x, new_grid_size) of the layer with (CPU) state dict sd, in float64.  live[i] is False where feature i took
    the fallback fit."""
    from models.effkan import KANLinear
    k_x, w_x, piv_x = fit(x, sd, new_grid_size, order, grid_eps, margin)
    rows = KANLinear.fallback_samples(sd["grid"], order, samples)
    k_f, w_f, piv_f = fit(rows, sd, new_grid_size, order, grid_eps, margin)
    live = piv_x > TAU
    return (torch.where(live[:, None], k_x, k_f), torch.where(live[None, :, None], w_x, w_f), live, piv_x, piv_f)


def fit_residual(x, sd, knots, spline_weight, order):
    """Normwise residual of the least-squares fit on the rows of x: the old layer's spline path (scaled weights, no base term)
    against the spline with the fitted coefficients on the new knots.  It is what the extension does NOT preserve: the new
    quantile knots do not nest the old ones, and a sample outside the old grid sees an old spline cut to zero."""
    x64 = x.double()
    old = torch.einsum("mik,oik->mo", ko.bspline_bases(x64, sd["grid"].double(), order), scaled_weight(sd))
    new = torch.einsum("mik,oik->mo", ko.bspline_bases(x64, knots.double(), order), spline_weight.double())
    return float((new - old).norm() / old.norm())
