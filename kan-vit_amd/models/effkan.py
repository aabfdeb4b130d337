"""KANLinear (efficient-KAN B-spline layer) -- drop-in for models/effkan.py:8-264 (family BSPLINE).

Forward / backward run in the fused kernel: Cox-de Boor bases on the per-feature knot buffer
``grid`` (half-open order-0 intervals, models/effkan.py:115), the base path (``base_activation``: SiLU by
default, or one of ops.SUPPORTED_BASE_ACTIVATIONS, read on every forward) and both
contractions in one pass.  Construction-time host logic (knot vector, the least-squares
initialisation of ``spline_weight``) is plain torch, as in the reference.  ``update_grid`` computes the new
knots with the reference's torch expressions and refits the weights in the fused Gram-matrix kernels
(kanvit.ops.bspline_refit); ``extend_grid`` carries the layer to another ``grid_size`` the same way
(kanvit.ops.bspline_regrid, section 4.15)."""
import math
from dataclasses import replace

import torch
import torch.nn.functional as F

from kanvit import _lib, grouped, ops
from kanvit.prune import EdgePruning


_GRID_FACTS = {}      # (ids, versions, data_ptrs of the knot buffers) -> (uniform, all_equal, the knot buffers)


def _grid_facts(layers):
    """Are the knot buffers uniform (g0 + j*h, the only layout the reference ever builds, models/effkan.py:44-53) and
    identical across `layers`?  Checked once per set of buffers (needs a host sync) and cached on their version
    counters, so an in-place change of any grid is noticed."""
    key = tuple((id(m), m.grid._version, m.grid.data_ptr()) for m in layers)
    hit = _GRID_FACTS.get(key)
    # An entry keeps its knot tensors: a buffer replaced by `.to()` / `.cpu().cuda()` starts again at version 0 and may get a
    # freed buffer's address, and since update_grid a replaced buffer need not hold what the old one held.
    if hit is not None and any(t is not m.grid for t, m in zip(hit[2], layers)):
        hit = None
    if hit is None:
        g0 = layers[0].grid
        row = g0[0].double()
        step = (row[-1] - row[0]) / (row.numel() - 1)              # the kernel derives h the same way
        ideal = row[0] + step * torch.arange(row.numel(), device=row.device, dtype=torch.float64)
        # The closed form evaluates the IDEAL grid row[0] + j*step, the Cox-de Boor kernels the stored knots: a knot that sits d off
        # its ideal place moves the bases by up to ~0.65 d / step.  So the deviation is bounded RELATIVE TO THE SPACING (4e-6 of it:
        # an eighth of the 2e-5 forward bound), and so is half a float32 ulp of the largest knot, which is what rounding makes of d on
        # a table far from 0 for its spacing: grid_range [1000, 1001] / 5 stores knots 2.2e-4 of a spacing off and takes the
        # Cox-de Boor kernels, grids within a few tens of spacings of 0 keep the closed form (profiles/basis_domain.md).
        tol = 4e-6 * float(step)
        off = max(float((row - ideal).abs().max()), float(row.abs().max()) * 2.0 ** -24)
        uniform = bool(float(step) > 0 and off <= tol and bool((g0 == g0[0:1]).all()))
        equal = all(m.grid.shape == g0.shape and bool((m.grid == g0).all()) for m in layers[1:])
        if len(_GRID_FACTS) > 256:
            _GRID_FACTS.clear()
        hit = _GRID_FACTS[key] = (uniform and layers[0].spline_order == 3, equal, tuple(m.grid for m in layers))
    return hit[:2]


class KANLinear(EdgePruning, grouped.KanLayer, torch.nn.Module):
    def __init__(self, in_features, out_features, grid_size=5, spline_order=3, scale_noise=0.1, scale_base=1.0,
                 scale_spline=1.0, enable_standalone_scale_spline=True, base_activation=torch.nn.SiLU, grid_eps=0.02,
                 grid_range=[-1, 1]):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.grid_size = grid_size
        self.spline_order = spline_order

        # uniform knots, spline_order extra on each side (models/effkan.py:44-53)
        h = (grid_range[1] - grid_range[0]) / grid_size
        knots = torch.arange(-spline_order, grid_size + spline_order + 1) * h + grid_range[0]
        self.register_buffer("grid", knots.expand(in_features, -1).contiguous())

        n_basis = grid_size + spline_order
        self.base_weight = torch.nn.Parameter(torch.Tensor(out_features, in_features))
        self.spline_weight = torch.nn.Parameter(torch.Tensor(out_features, in_features, n_basis))
        if enable_standalone_scale_spline:
            self.spline_scaler = torch.nn.Parameter(torch.Tensor(out_features, in_features))

        self.scale_noise = scale_noise
        self.scale_base = scale_base
        self.scale_spline = scale_spline
        self.enable_standalone_scale_spline = enable_standalone_scale_spline
        self.base_activation = base_activation()
        ops.base_act_of(self.base_activation)          # refuse what the kernels do not implement (NotImplementedError)
        self.grid_eps = grid_eps
        self.reset_parameters()

    # ---- construction-time host logic (models/effkan.py:74-97,134-164) ----
    def reset_parameters(self):
        torch.nn.init.kaiming_uniform_(self.base_weight, a=math.sqrt(5) * self.scale_base)
        with torch.no_grad():
            noise = (torch.rand(self.grid_size + 1, self.in_features, self.out_features) - 0.5) \
                * self.scale_noise / self.grid_size
            scale = 1.0 if self.enable_standalone_scale_spline else self.scale_spline
            pts = self.grid.T[self.spline_order: -self.spline_order]
            self.spline_weight.data.copy_(scale * self.curve2coeff(pts, noise))
            if self.enable_standalone_scale_spline:
                torch.nn.init.kaiming_uniform_(self.spline_scaler, a=math.sqrt(5) * self.scale_spline)

    def b_splines(self, x: torch.Tensor):
        """(batch, in) -> (batch, in, grid_size + spline_order) bases.  Host-side torch version used
        by the initialiser; on a GPU tensor it calls the kernel through an identity contraction."""
        assert x.dim() == 2 and x.size(1) == self.in_features
        if x.is_cuda:
            nb = self.grid_size + self.spline_order
            cfg = ops.LayerCfg(family=ops.BSPLINE, I=1, O=nb, G=nb, groups=self.in_features,
                               x_group_mod=self.in_features, spline_order=self.spline_order, has_base=0)
            eye = torch.eye(nb, device=x.device).expand(self.in_features, nb, nb).contiguous()
            return ops.kan_layer(x, eye, cfg, bparams=self.grid).view(x.size(0), self.in_features, nb)
        g = self.grid
        xe = x.unsqueeze(-1)
        b = ((xe >= g[:, :-1]) & (xe < g[:, 1:])).to(x.dtype)
        for k in range(1, self.spline_order + 1):
            left = (xe - g[:, : -(k + 1)]) / (g[:, k:-1] - g[:, : -(k + 1)])
            right = (g[:, k + 1:] - xe) / (g[:, k + 1:] - g[:, 1:-k])
            b = left * b[:, :, :-1] + right * b[:, :, 1:]
        return b.contiguous()

    def curve2coeff(self, x: torch.Tensor, y: torch.Tensor):
        """Least-squares spline coefficients interpolating y (batch, in, out) at x (batch, in)."""
        assert x.dim() == 2 and x.size(1) == self.in_features
        assert y.size() == (x.size(0), self.in_features, self.out_features)
        a = self.b_splines(x).transpose(0, 1)
        sol = torch.linalg.lstsq(a, y.transpose(0, 1)).solution
        return sol.permute(2, 0, 1).contiguous()

    @property
    def scaled_spline_weight(self):
        if self.enable_standalone_scale_spline:
            return self.spline_weight * self.spline_scaler.unsqueeze(-1)
        return self.spline_weight

    # ---- fused-kernel protocol ----
    def kan_cfg(self, layers=None):
        uniform, equal = _grid_facts(layers if layers is not None else [self])
        flags = (_lib.FLAG_UNIFORM_KNOTS if uniform and equal else 0) | (_lib.FLAG_SHARED_BPARAMS if equal and layers is not None else 0)
        return ops.LayerCfg(family=ops.BSPLINE, I=self.in_features, O=self.out_features,
                            G=self.grid_size + self.spline_order, spline_order=self.spline_order, has_base=1, flags=flags,
                            base_act=ops.base_act_of(self.base_activation))

    def kan_pack(self):
        # [O, I, nb] (scaled) and base [O, I] -> [I, nb+1, O] -> [I*(nb+1), O]; base column last
        w = torch.cat([self.scaled_spline_weight.permute(1, 2, 0), self.base_weight.t().unsqueeze(1)], dim=1)
        return w.reshape(-1, self.out_features), self.grid.reshape(-1), None

    @staticmethod
    def kan_pack_grouped(layers):
        l0 = layers[0]
        sw = grouped.stack_params([m.spline_weight for m in layers])                  # [g, O, I, nb]
        if l0.enable_standalone_scale_spline:
            sw = sw * grouped.stack_params([m.spline_scaler for m in layers]).unsqueeze(-1)
        bw = grouped.stack_params([m.base_weight for m in layers])                    # [g, O, I]
        w = torch.cat([sw.permute(0, 2, 3, 1), bw.permute(0, 2, 1).unsqueeze(2)], dim=2)   # [g, I, nb+1, O]
        g, i, nb1, o = w.shape
        return w.reshape(g, i * nb1, o), torch.stack([m.grid.reshape(-1) for m in layers]), None

    def kan_base_act(self):
        return ops.base_act_of(self.base_activation)

    def forward(self, x: torch.Tensor):
        assert x.size(-1) == self.in_features
        y = grouped.run_single(self, x.reshape(-1, self.in_features))
        return y.reshape(*x.shape[:-1], self.out_features)

    @staticmethod
    def adapted_grid(x: torch.Tensor, grid_size, spline_order, grid_eps, margin=0.01):
        """[in, grid_size + 2*spline_order + 1]: the knots update_grid moves to -- per channel the blend of the sample quantiles
        and a uniform grid over the sample range, extended by spline_order uniform steps on each side.  The arithmetic of
        models/effkan.py:204-238 operation for operation (same dtypes, same order of the float operations, the same truncating
        int64 linspace for the sample indices), in torch on x's device, so the knots are the reference's up to contraction."""
        xs = x.sort(dim=0).values                                       # every channel on its own
        lo, hi = xs[0], xs[-1]
        picks = torch.linspace(0, x.size(0) - 1, grid_size + 1, dtype=torch.int64, device=x.device)
        step = (hi - lo + 2 * margin) / grid_size
        ramp = torch.arange(grid_size + 1, dtype=torch.float32, device=x.device).unsqueeze(1)
        inner = grid_eps * (ramp * step + lo - margin) + (1 - grid_eps) * xs[picks]
        away = torch.arange(1, spline_order + 1, device=x.device).unsqueeze(1)
        knots = torch.cat([inner[:1] - step * away.flip(0), inner, inner[-1:] + step * away], dim=0)
        return knots.t().contiguous()

    @torch.no_grad()
    def update_grid(self, x: torch.Tensor, margin=0.01):
        """Move the knots to where the rows of x (batch, in) lie and refit spline_weight so that the layer computes the same
        function on them (models/effkan.py:189-242), with the reference's quirk kept: the fit target is scaled_spline_weight, the
        result goes into spline_weight, spline_scaler stays.  The refit runs in the fused Gram-matrix kernels
        (ops.bspline_refit): no (batch, in, out) tensor, no lstsq.  A feature whose fit does not exist (a constant column,
        fewer distinct samples than basis functions) keeps its knots and weights, i.e. its function; the reference's answer
        there depends on the LAPACK driver.  Returns the number of features kept unchanged, a 0-d device tensor (the reference
        returns None)."""
        assert x.dim() == 2 and x.size(1) == self.in_features
        x = x.float()
        new_grid = self.adapted_grid(x, self.grid_size, self.spline_order, self.grid_eps, margin)
        cfg, w_old, old = self.regrid_operands(self.grid_size)
        w_new, ok = ops.bspline_refit(x, w_old, cfg, old, new_grid.unsqueeze(0))
        self.apply_refit(new_grid, w_new[0], ok[0])
        return (~ok).sum()

    def apply_refit(self, new_grid, w_new, ok):
        """Take the refitted knots [in, nk] and packed weights [in*nb, out] for the features with ok[in] set."""
        nb = self.grid_size + self.spline_order
        sw = w_new.view(self.in_features, nb, self.out_features).permute(2, 0, 1)
        self.grid.copy_(torch.where(ok[:, None], new_grid, self.grid))
        self.spline_weight.data.copy_(torch.where(ok[None, :, None], sw, self.spline_weight))

    MAX_BASIS = 24            # basis functions per feature the refit kernels hold in registers (include/kanvit.h)
    FALLBACK_SAMPLES = 256    # one row band of the Gram kernel

    @staticmethod
    def span_samples(lo: torch.Tensor, hi: torch.Tensor, P):
        """[P, in]: P evenly spaced samples from lo[in] to hi[in], both ends included."""
        t = torch.arange(P, dtype=torch.float32, device=lo.device).unsqueeze(1) / (P - 1)
        return lo.unsqueeze(0) + (hi - lo).unsqueeze(0) * t

    @staticmethod
    def fallback_samples(old_grid: torch.Tensor, spline_order, P):
        """[P, in]: the synthetic rows extend_grid refits a feature on when its fit on the real rows does not exist -- P evenly
        spaced samples across the inner span [knots[order], knots[-order-1]] of the feature's old knots [in, nk], the range its
        function was defined on.  Plain torch on old_grid's device."""
        return KANLinear.span_samples(old_grid[:, spline_order], old_grid[:, -spline_order - 1], P)

    @staticmethod
    def check_extension(grid_size, spline_order):
        nb = grid_size + spline_order
        if grid_size < 1 or nb > KANLinear.MAX_BASIS:
            raise ops.KanvitError(f"extend_grid: grid_size={grid_size} with spline_order={spline_order} gives grid_size + spline_order = "
                                  f"{nb} basis functions per feature; supported: grid_size >= 1 and at most {KANLinear.MAX_BASIS}")

    @torch.no_grad()
    def extend_grid(self, x: torch.Tensor, grid_size, margin=0.01):
        """Grid extension (pykan's refine): move the layer to `grid_size` intervals -- finer or coarser -- and initialise the new
        coefficients so that every edge keeps the function it has learnt, wherever the rows of x (batch, in) sample it.  The new
        knots are adapted_grid(x, grid_size, ...), the reference's knot rule at the new size; the new spline_weight is the
        least-squares fit of the old spline on them, from the fused Gram-matrix kernels with a rectangular cross matrix
        (ops.bspline_regrid).  update_grid's quirk is kept: the fit target is scaled_spline_weight, the
        result goes into spline_weight, spline_scaler stays.  `grid` becomes a new [in, nk_new] buffer, `spline_weight` a NEW
        Parameter [out, in, nb_new] (an optimizer holding the old one must be told), `grid_size` is updated.
        A feature whose fit on x does not exist (a constant column, too few distinct samples) cannot keep its old knots and
        weights, as it does in update_grid: their shapes change.  It is refitted on FALLBACK_SAMPLES evenly spaced synthetic
        samples across its old grid's inner span (fallback_samples) and takes its knots from adapted_grid of those, so it keeps its
        function over the range it was defined on.  Both fits always run and are combined on the device: no host sync.
        Returns the number of features that took the fallback (0-d device tensor)."""
        assert x.dim() == 2 and x.size(1) == self.in_features
        self.check_extension(grid_size, self.spline_order)
        x = x.float()
        cfg, w_old, old = self.regrid_operands(grid_size)
        new_grid = self.adapted_grid(x, grid_size, self.spline_order, self.grid_eps, margin)
        w_new, ok = ops.bspline_regrid(x, w_old, cfg, self.grid_size + self.spline_order, old, new_grid.unsqueeze(0))
        xf = self.fallback_samples(self.grid, self.spline_order, self.FALLBACK_SAMPLES)
        fb_grid = self.adapted_grid(xf, grid_size, self.spline_order, self.grid_eps, margin)
        w_fb, _ = ops.bspline_regrid(xf, w_old, cfg, self.grid_size + self.spline_order, old, fb_grid.unsqueeze(0))
        self.apply_regrid(grid_size, new_grid, w_new[0], fb_grid, w_fb[0], ok[0])
        return (~ok).sum()

    def regrid_operands(self, grid_size):
        """(cfg of the layer at `grid_size`, packed old spline weights [1, in*nb_old, out], old knots [1, in*nk_old])."""
        cfg = replace(self.kan_cfg(), has_base=0, base_act=0, G=grid_size + self.spline_order)
        w_old = self.scaled_spline_weight.permute(1, 2, 0).reshape(1, -1, self.out_features)
        return cfg, w_old, self.grid.reshape(1, -1)

    def apply_regrid(self, grid_size, new_grid, w_new, fb_grid, w_fb, ok):
        """Become a layer of `grid_size` intervals: knots [in, nk_new] and packed weights [in*nb_new, out] from the fit on the
        real rows where ok[in] is set, from the fit on the fallback samples elsewhere."""
        nb = grid_size + self.spline_order
        pick = torch.where(ok[:, None, None], w_new.view(self.in_features, nb, self.out_features),
                           w_fb.view(self.in_features, nb, self.out_features))
        self.resize_grid(grid_size, torch.where(ok[:, None], new_grid, fb_grid), pick.permute(2, 0, 1).contiguous())

    def resize_grid(self, grid_size, grid, spline_weight):
        """Replace the knot buffer and the spline_weight Parameter by tensors of another grid size."""
        self.grid = grid                                    # a registered buffer: assignment replaces it (_grid_facts sees a new tensor)
        self.spline_weight = torch.nn.Parameter(spline_weight, requires_grad=self.spline_weight.requires_grad)
        self.grid_size = grid_size

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """A checkpoint saved after extend_grid loads into a layer built at another grid_size: when the incoming grid [in, nk] and
        spline_weight [out, in, nb] agree with each other and with this layer's spline_order (nk = gs + 2*order + 1,
        nb = gs + order for one gs >= 1) and features, the layer adopts that grid size first.  Anything else fails as it always did."""
        g, w = state_dict.get(prefix + "grid"), state_dict.get(prefix + "spline_weight")
        if torch.is_tensor(g) and torch.is_tensor(w) and g.dim() == 2 and w.dim() == 3:
            gs = w.shape[2] - self.spline_order
            if (gs >= 1 and gs != self.grid_size and g.shape[1] == gs + 2 * self.spline_order + 1 and g.shape[0] == self.in_features
                    and tuple(w.shape[:2]) == (self.out_features, self.in_features)):
                self.resize_grid(gs, torch.zeros(g.shape, dtype=self.grid.dtype, device=self.grid.device),
                                 torch.empty(w.shape, dtype=self.spline_weight.dtype, device=self.spline_weight.device))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def edge_activation_l1(self, x: torch.Tensor, include_base=False):
        """[out, in]: the mean over the samples of |phi_{o,i}(x[.., i])|, the per-edge activation magnitude the KAN paper
        regularises and prunes by -- which the reference says it cannot form behind F.linear (models/effkan.py:244-264).  The
        fused kernel reduces over the samples as it generates the basis; the (batch, in, out) tensor never exists.  Without
        the base it is the spline path (scaled_spline_weight), with it the full edge function.  x: any leading dimensions."""
        assert x.size(-1) == self.in_features
        x2d = x if x.dim() == 2 else x.reshape(-1, self.in_features)
        cfg = self.kan_cfg()
        if include_base:
            w, bp, _ = self.kan_pack()
        else:
            cfg = replace(cfg, has_base=0, base_act=0)
            w, bp = self.scaled_spline_weight.permute(1, 2, 0).reshape(-1, self.out_features), self.grid.reshape(-1)
        return ops.edge_l1(x2d, w.unsqueeze(0), cfg, bp.unsqueeze(0))[0].t()

    # ---- edge pruning (kanvit/prune.py: prune_edges, edge_masked, restore_edge_mask) ----
    def _edge_dims(self):
        return self.in_features, self.out_features

    def _edge_tensors(self):
        # spline_scaler stays as it is: its gradient through a zero spline_weight is zero
        return [(self.spline_weight, self.spline_weight.shape[2]), (self.base_weight, 1)]

    def _edge_scores(self, x):
        return self.edge_activation_l1(x, include_base=True)

    def regularization_loss(self, regularize_activation=1.0, regularize_entropy=1.0, x=None, include_base=False):
        """Without x: the L1 / entropy surrogate on the spline weights (models/effkan.py:244-264); parameter-only math.
        With x: the same two terms on the sample-based edge_activation_l1(x, include_base), the paper's regulariser."""
        if x is not None:
            return ops.l1_entropy_loss(self.edge_activation_l1(x, include_base), regularize_activation, regularize_entropy)
        l1 = self.spline_weight.abs().mean(-1)
        total = l1.sum()
        p = l1 / total
        return regularize_activation * total - regularize_entropy * torch.sum(p * p.log())
