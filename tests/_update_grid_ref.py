"""Float64 restatement of KANLinear.update_grid (models/effkan.py:189-242), shared by the CPU and GPU tests of the fused refit
(tests/test_update_grid_cpu.py pins it against the reference's goldens; tests/test_update_grid_gpu.py then uses it on shapes
that have no goldens).  Written in this project's own words: sort every channel, pick grid_size + 1 evenly spaced order
statistics, blend them with a uniform grid over the sample range, extend by spline_order uniform steps on each side; evaluate
the layer's per-edge spline output on the old knots (oracle.kan_oracle.bspline_bases) and fit it on the new ones by a float64
lstsq per feature."""
import torch

from oracle import kan_oracle as ko

TAU = 1e-5            # KANVIT_BSPLINE_REFIT_TAU (include/kanvit.h)


def rel(a, b):
    """Normwise relative error ||a - b|| / ||b||."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def grid_err(g, ref):
    """max |g - ref| / (1 + |ref|): the grid bound is 1e-6 of that."""
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    return float(((g - ref).abs() / (1.0 + ref.abs())).max())


def new_knots(x, grid_size, order, grid_eps, margin=0.01):
    """[in, grid_size + 2*order + 1] float64 knots for the rows x[M, in]."""
    xs = torch.sort(x.double(), dim=0).values
    m = xs.shape[0]
    picks = torch.linspace(0, m - 1, grid_size + 1, dtype=torch.int64)       # the index rule is the reference's (truncation)
    quantiles = xs[picks]
    lo, hi = xs[0], xs[-1]
    step = (hi - lo + 2.0 * margin) / grid_size
    ramp = torch.arange(grid_size + 1, dtype=torch.float64).unsqueeze(1)
    inner = grid_eps * (lo - margin + ramp * step) + (1.0 - grid_eps) * quantiles
    before = inner[0] - step * torch.arange(order, 0, -1, dtype=torch.float64).unsqueeze(1)
    after = inner[-1] + step * torch.arange(1, order + 1, dtype=torch.float64).unsqueeze(1)
    return torch.cat([before, inner, after], dim=0).t().contiguous()


def pivot_ratios(x, knots, order):
    """[in]: per feature the smallest Cholesky pivot of N = Bnew^T Bnew over its largest diagonal entry (0 where the
    factorisation breaks down) -- the quantity the solve kernel holds against TAU."""
    b = ko.bspline_bases(x.double(), knots.double(), order)                 # [M, in, nb]
    n = torch.einsum("mij,mik->ijk", b, b)
    out = []
    for ni in n:
        a = ni.clone()
        dmax = float(a.diagonal().max())
        worst = float("inf")
        for k in range(a.shape[0]):
            d = float(a[k, k])
            worst = min(worst, d / dmax if dmax > 0 else 0.0)
            if not d > 0:
                worst = 0.0
                break
            col = a[k + 1:, k] / d
            a[k + 1:, k + 1:] -= torch.outer(col, a[k + 1:, k])
        out.append(max(worst, 0.0))
    return torch.tensor(out, dtype=torch.float64)


def refit(x, sd, grid_size, order, grid_eps=0.02, margin=0.01):
    """(knots [in, nk], spline_weight [out, in, nb]) after update_grid(x) of the layer with (CPU) state dict sd, in float64."""
    x64 = x.double()
    scaled = sd["spline_weight"].double()
    if "spline_scaler" in sd:
        scaled = scaled * sd["spline_scaler"].double().unsqueeze(-1)
    target = torch.einsum("mik,oik->imo", ko.bspline_bases(x64, sd["grid"].double(), order), scaled)       # [in, M, out]
    knots = new_knots(x, grid_size, order, grid_eps, margin)
    design = ko.bspline_bases(x64, knots, order).permute(1, 0, 2)                                          # [in, M, nb]
    coeff = torch.linalg.lstsq(design, target).solution                                                    # [in, nb, out]
    return knots, coeff.permute(2, 0, 1).contiguous()


def forward64(x, sd, knots, spline_weight, order):
    """The layer's float64 forward (SiLU base) with the given knots and spline weights."""
    scaler = sd["spline_scaler"].double() if "spline_scaler" in sd else None
    return ko.kanlinear_forward(x.double(), sd["base_weight"].double(), spline_weight.double(), scaler, knots.double(), order)
