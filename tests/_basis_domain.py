"""Input sets and float64 references for the KAN basis generators over their whole argument range (no GPU needed).

csrc/kan_basis.h states every basis family several times (LDS-tile, register forward, register input gradient, weight gradient,
tiny kernels, private copies in the edge-L1 and refit kernels).  The places where such restatements can disagree are not where
randn * 1.5 falls: x exactly on a knot or one ulp beside it, x outside the grid, saturated tanh, large sine arguments, trained
frequencies, base activations far from 0.  This module builds those inputs and the closed-form value AND derivative of every
family's univariate functions, generic in the dtype: float64 is the reference, float32 the plain-torch restatement that
tests/test_basis_domain_cpu.py holds against it (half of each fp32 bound), so the ranges below are ones plain float32 meets.

The formulas are written from oracle/kan_oracle.py and the definitions: T_n by the three-term recurrence with T_n' = n U_{n-1}
(never autograd through acos, which is NaN at saturated tanh), Cox-de Boor with the derivative of its last level, Gaussians,
sin / cos.  SineKAN is evaluated at the FLOAT32 argument fl(fl(x f) + p), which the reference and the kernels both form.

Input sets: a flat float32 vector -- the special values, each REPLICAS times, then a dense sweep -- scattered over [M, I] so that
every special value lands in 8 different feature columns and in both the first and the last row tile (placement_ok checks)."""
import math

import torch

BM = 128              # row tile of the MFMA kernels; the tiny kernels tile by 256 (a last tile by both counts is used)
REPLICAS = 8          # copies of every special value: 8 columns, alternating first / last row tile
HUGE = 999.0          # |x| at and above this is judged as a class of its own (the base column is O(|x|) there)

# ---- the final input ranges (profiles/basis_domain.md) -------------------------------------------------------------------------
CHEBY_SWEEP = 12.0                        # dense sweep of tanh's argument
CHEBY_SPECIALS = [0.0, 1e-20, 1e-40, 9.0, 20.0, 44.0, 45.0, 89.0, 1e4, math.inf]      # each with both signs
SINE_ARG = 250.0                          # the sweep takes |x f + p| to about this (kv_sin documents |arg| <= 256)
FOURIER_RANGE = {3: 40.0, 28: 4.0}        # |x| by grid size: float32 k x loses 0.5 ulp(k |x|) in the restatement itself
RBF_U = 150.0                             # the spline-path input, centres in [-2, 2]
RBF_X = 2.0                               # the base column's input next to that sweep of u
BASE_SWEEP = 100.0                        # the base column's input
BSPLINE_FAR = [1e3, 1e30]                 # each with both signs

ACTS = ("silu", "gelu", "gelu_tanh", "relu", "tanh", "identity")       # KANVIT_BASE_* 0 .. 5


# ---- scattering ----------------------------------------------------------------------------------------------------------------
def last_tile_start(m):
    return max(BM * ((m - 1) // BM), 256 * ((m - 1) // 256))


def scatter(specials, lo, hi, m, i, seed=0):
    """(x[m, i] float32, src[m, i] int64): special value k sits where src == k (REPLICAS places: columns (k + r * (i // 8)) % i,
    r even in the first row tile, r odd in the last), the other slots (src == -1) hold a dense sweep of [lo, hi] in an order
    fixed by `seed`."""
    assert i >= REPLICAS and m > BM
    specials = torch.as_tensor(specials, dtype=torch.float32).flatten()
    x = torch.zeros(m, i, dtype=torch.float32)
    src = torch.full((m, i), -1, dtype=torch.int64)
    tiles = ((0, BM), (last_tile_start(m), m))
    for k in range(specials.numel()):
        for r in range(REPLICAS):
            r0, r1 = tiles[r % 2]
            col = (k + r * (i // REPLICAS)) % i
            row = r0 + (5 * k + 3 * r) % (r1 - r0)
            for _ in range(r1 - r0):
                if src[row, col] < 0:
                    break
                row = r0 + (row - r0 + 1) % (r1 - r0)
            assert src[row, col] < 0, "no free slot: too many special values for this shape"
            src[row, col] = k
            x[row, col] = specials[k]
    free = src < 0
    n = int(free.sum())
    sweep = torch.linspace(lo, hi, n, dtype=torch.float64).float()
    x[free] = sweep[torch.randperm(n, generator=torch.Generator().manual_seed(seed))]
    return x, src


def placement_ok(x, src, specials):
    """Every special value is in the matrix bit for bit, in >= 8 feature columns, and in both the first and the last row tile."""
    specials = torch.as_tensor(specials, dtype=torch.float32)
    if specials.dim() == 1:                        # one table for every feature
        specials = specials.unsqueeze(0)
    m, i = x.shape
    cols = torch.arange(i).expand(m, i)
    want = specials[cols.clamp(max=specials.shape[0] - 1), src.clamp(min=0)]
    placed = src >= 0
    if not torch.equal(x[placed].view(torch.int32), want[placed].view(torch.int32)):
        return False
    t1 = last_tile_start(m)
    for k in range(specials.shape[1]):
        rows, cs = torch.nonzero(src == k, as_tuple=True)
        if cs.unique().numel() < 8 or not bool((rows < BM).any()) or not bool((rows >= t1).any()):
            return False
    return True


def with_signs(values):
    out = []
    for v in values:
        out += [v, -v]
    return out


def cheby_inputs(m, i, seed=1):
    sp = with_signs(CHEBY_SPECIALS)
    x, src = scatter(sp, -CHEBY_SWEEP, CHEBY_SWEEP, m, i, seed)
    return x, src, sp


def bspline_specials(grid):
    """[I, n] float32: per feature every knot, its float32 neighbours on both sides, the interval midpoints, a point just outside
    each end, and +-1e3, +-1e30.  Built from the layer's stored float32 knot buffer grid[I, nk]."""
    g = grid.detach().cpu().float()
    inf = torch.full_like(g, math.inf)
    h0, h1 = g[:, 1:2] - g[:, 0:1], g[:, -1:] - g[:, -2:-1]
    far = torch.tensor(with_signs(BSPLINE_FAR), dtype=torch.float32).expand(g.shape[0], -1)
    return torch.cat([g, torch.nextafter(g, inf), torch.nextafter(g, -inf), 0.5 * (g[:, :-1] + g[:, 1:]),
                      g[:, 0:1] - 0.25 * h0, g[:, -1:] + 0.25 * h1, far], dim=1)


def bspline_inputs(grid, m, seed=2):
    """x[m, I] for the knot table grid[I, nk] (every feature gets ITS knots), src, the specials table [I, n]; the sweep reaches
    one spacing beyond both ends."""
    g = grid.detach().cpu().float()
    sp = bspline_specials(g)
    lo = float((g[:, 0] - (g[:, 1] - g[:, 0])).min())
    hi = float((g[:, -1] + (g[:, -1] - g[:, -2])).max())
    x, src = scatter(sp[0], lo, hi, m, g.shape[0], seed)
    cols = torch.arange(g.shape[0]).expand(m, -1)
    x = torch.where(src >= 0, sp[cols, src.clamp(min=0)], x)
    return x, src, sp


def sine_inputs(freq, phase, m, seed=3):
    """x[m, I] sweeping +-(SINE_ARG - max|phase|) / max|freq|: the largest |x f + p| is about SINE_ARG."""
    f, p = freq.detach().cpu().float().flatten(), phase.detach().cpu().float().reshape(-1, freq.numel())
    xmax = (SINE_ARG - float(p.abs().max())) / float(f.abs().max())
    assert xmax > 1.0
    sp = with_signs([0.0, xmax])
    x, src = scatter(sp, -xmax, xmax, m, p.shape[0], seed)
    return x, src, sp


def fourier_inputs(g, m, i, seed=4):
    r = FOURIER_RANGE[g]
    sp = with_signs([0.0, r, math.pi, 0.5 * math.pi])
    x, src = scatter(sp, -r, r, m, i, seed)
    return x, src, sp


def rbf_inputs(centres, m, i, seed=5):
    """(x, u, src, specials): u sweeps +-RBF_U and holds the centres themselves and the clamp points of the two-anchor recurrence's
    argument; x (the base column's input) sweeps +-RBF_X independently, so that y stays O(1) and resolves the Gaussians (the base
    column's own +-BASE_SWEEP is the set of the layers named after an activation)."""
    c = centres.detach().cpu().float().flatten()
    h = float(c[-1] - c[0]) / (c.numel() - 1)
    sp = c.tolist() + with_signs([RBF_U]) + [float(c[0]) - 20.0 * h, float(c[0]) + 30.0 * h, float(c[0]) - 7.35 * h, float(c[0]) + 14.4 * h]
    u, src = scatter(sp, -RBF_U, RBF_U, m, i, seed)
    x, _ = scatter(with_signs([0.0, RBF_X]), -RBF_X, RBF_X, m, i, seed + 100)
    return x, u, src, sp


def base_inputs(m, i, seed=6):
    sp = with_signs([0.0, 1e-3, 1.0, 10.0, 20.0, BASE_SWEEP])
    x, src = scatter(sp, -BASE_SWEEP, BASE_SWEEP, m, i, seed)
    return x, src, sp


def huge(x):
    return ~(x.abs() < HUGE)


# ---- closed-form values and derivatives (dtype generic) -----------------------------------------------------------------------
def act(name, x):
    """(value, derivative) of a base activation; the derivatives are torch's backward formulas (relu: 0 at x = 0)."""
    if name == "silu":
        s = torch.sigmoid(x)
        return x * s, s * (1 + x * (1 - s))
    if name == "gelu":
        cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
        return x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if name == "gelu_tanh":
        k = math.sqrt(2.0 / math.pi)
        t = torch.tanh(k * (x + 0.044715 * x ** 3))
        return 0.5 * x * (1 + t), 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k * (1 + 3 * 0.044715 * x * x)
    if name == "relu":
        return torch.relu(x), (x > 0).to(x.dtype)
    if name == "tanh":
        t = torch.tanh(x)
        return t, 1 - t * t
    assert name == "identity"
    return x, torch.ones_like(x)


def cheby(x, n):
    """T_0 .. T_{n-1} of tanh x and d/dx: T_j' = j U_{j-1}, times sech^2."""
    t = torch.tanh(x)
    s2 = 1 - t * t
    T, U = [torch.ones_like(t), t], [torch.ones_like(t), 2 * t]
    for _ in range(2, n):
        T.append(2 * t * T[-1] - T[-2])
        U.append(2 * t * U[-1] - U[-2])
    d = [torch.zeros_like(t)] + [j * U[j - 1] * s2 for j in range(1, n)]
    return torch.stack(T[:n], -1), torch.stack(d[:n], -1)


def bspline(x, grid, order):
    """Cox-de Boor on grid[I, nk] (half-open order-0 intervals) and the derivative of its last level,
    B_{j,p}' = p (B_{j,p-1} / (t_{j+p} - t_j) - B_{j+1,p-1} / (t_{j+p+1} - t_{j+1}))."""
    g = grid.to(x.dtype)
    xe = x.unsqueeze(-1)
    b = ((xe >= g[:, :-1]) & (xe < g[:, 1:])).to(x.dtype)
    if order == 0:
        return b, torch.zeros_like(b)
    for k in range(1, order):
        b = (xe - g[:, :-(k + 1)]) / (g[:, k:-1] - g[:, :-(k + 1)]) * b[:, :, :-1] \
            + (g[:, k + 1:] - xe) / (g[:, k + 1:] - g[:, 1:-k]) * b[:, :, 1:]
    p = order
    il = 1 / (g[:, p:-1] - g[:, :-(p + 1)])
    ir = 1 / (g[:, p + 1:] - g[:, 1:-p])
    return (xe - g[:, :-(p + 1)]) * il * b[:, :, :-1] + (g[:, p + 1:] - xe) * ir * b[:, :, 1:], p * (b[:, :, :-1] * il - b[:, :, 1:] * ir)


def basis(p, x, u=None, dtype=torch.float64):
    """(phi[M, I, GP], dphi/dx[M, I, GP], dphi/du[M, I, GP] | None, dphi/dfreq[M, I, GP] | None) of the family described by p
    (see the *_params helpers) at x[M, I] (RBF: the spline path reads u[M, I]), computed in `dtype` from the float32 inputs."""
    fam = p["family"]
    x32 = x.float()
    xv = x32.to(dtype)
    if fam == "cheby":
        return (*cheby(xv, p["G"]), None, None)
    if fam == "fourier":
        k = torch.arange(1, p["G"] + 1, dtype=dtype)
        ang = xv.unsqueeze(-1) * k
        c, s = torch.cos(ang), torch.sin(ang)
        return torch.cat([c, s], -1), torch.cat([-k * s, k * c], -1), None, None
    if fam == "sine":
        f32, p32 = p["freq"].float().reshape(1, 1, -1), p["phase"].float().reshape(1, x.shape[1], -1)
        arg = (x32.unsqueeze(-1) * f32 + p32).to(dtype)              # two float32 roundings: fl(fl(x f) + p)
        c = torch.cos(arg)
        return torch.sin(arg), f32.to(dtype) * c, None, xv.unsqueeze(-1) * c
    base = None
    if p.get("act") is not None:
        bv, bd = act(p["act"], xv)
        base = (bv.unsqueeze(-1), bd.unsqueeze(-1))
    if fam == "bspline":
        v, d = bspline(xv, p["grid"], p["order"])
        if base is not None:
            v, d = torch.cat([v, base[0]], -1), torch.cat([d, base[1]], -1)
        return v, d, None, None
    assert fam == "rbf"
    uv = (x32 if u is None else u.float()).to(dtype)
    z = (uv.unsqueeze(-1) - p["centres"].to(dtype)) / p["h"]
    v = torch.exp(-z * z)
    du = v * (-2 * z / p["h"])
    dx = torch.zeros_like(v)
    if base is not None:
        v, du, dx = torch.cat([v, base[0]], -1), torch.cat([du, torch.zeros_like(base[1])], -1), torch.cat([dx, base[1]], -1)
    return v, dx, du, None


def diag_weights(i, gp, o, seed=0):
    """w3[I, GP, O] float32 with w3[i, j, o] = delta(i, o) c[o][j], 0.5 <= |c| <= 1: y[m, o] and dx[m, i] become univariate
    functions of one x, so a failure names the x value."""
    g = torch.Generator().manual_seed(1000 + seed)
    n = min(i, o)
    c = (0.5 + 0.5 * torch.rand(n, gp, generator=g)) * (torch.randint(0, 2, (n, gp), generator=g) * 2 - 1)
    w3 = torch.zeros(i, gp, o, dtype=torch.float32)
    idx = torch.arange(n)
    w3[idx, :, idx] = c
    return w3


def contract(phi, dphi, w3, dy, dphi_u=None, rnd=None):
    """float64 (y[M, O], dx[M, I], du[M, I] | None, dW[I, GP, O], dPhi[M, I, GP]) of y = Phi W for the loss sum(y * dy).  rnd: the
    operand rounding of the bf16 kernels (both operands of each of the three products; the basis derivative stays unrounded)."""
    r = (lambda t: t) if rnd is None else rnd
    w3, dy = w3.double(), dy.double()
    y = torch.einsum("mik,iko->mo", r(phi), r(w3))
    dphi_loss = torch.einsum("mo,iko->mik", r(dy), r(w3))
    dx = (dphi_loss * dphi).sum(-1)
    du = None if dphi_u is None else (dphi_loss * dphi_u).sum(-1)
    dw = torch.einsum("mik,mo->iko", r(phi), r(dy))
    return y, dx, du, dw, dphi_loss


def fwd_err(got, ref, cls):
    """max over the two magnitude classes of max|err| / max(1, max|ref|), each class held against its OWN largest reference
    entry (every entry is in exactly one class, so none is masked and none hides behind a 1e30 elsewhere in the matrix)."""
    worst = 0.0
    for sel in (cls, ~cls):
        if bool(sel.any()):
            d, r = (got.double() - ref)[sel], ref[sel]
            e = float(d.abs().max()) / max(1.0, float(r.abs().max()))
            worst = max(worst, e if math.isfinite(e) else math.inf)
    return worst


def rel_err(got, ref, cls=None, floor=1e-3):
    """tests/_util.rel_err, max|err| / max(max|ref|, floor), per magnitude class when `cls` is given."""
    if cls is None:
        cls = torch.zeros(ref.shape, dtype=torch.bool)
    worst = 0.0
    for sel in (cls, ~cls):
        if bool(sel.any()):
            d, r = (got.double() - ref)[sel], ref[sel]
            e = float(d.abs().max()) / max(float(r.abs().max()), floor)
            worst = max(worst, e if math.isfinite(e) else math.inf)
    return worst


# ---- the layers and their input sets ---------------------------------------------------------------------------------------------
BSPLINE_GRIDS = [(-1, 1, 5), (0, 1, 5), (-3, 5, 5), (-1, 1, 3), (-1, 1, 12), (-1, 1, 30), (100, 101, 5), (1000, 1001, 5)]
CLOSED_FORM_GRIDS = [(-1, 1, 5), (0, 1, 5), (-3, 5, 5), (-8, 8, 5), (0, 255, 5), (-1, 1, 12)]      # _grid_facts must keep answering "uniform"


def grid_name(g):
    return "bspline[%g,%g]/%d" % g


LAYERS = (["cheby-deg4", "cheby-deg3", "sine-grid4", "sine-grid4-trained", "sine-grid28-first", "sine-grid28-first-trained",
           "fourier-G3", "fourier-G28", "rbf", "bspline-perturbed", "bspline-order2"]
          + [grid_name(g) for g in BSPLINE_GRIDS] + ["bspline-" + a for a in ACTS] + ["rbf-" + a for a in ACTS])


def _act_module(name):
    nn = torch.nn
    return {"silu": nn.SiLU, "gelu": nn.GELU, "gelu_tanh": lambda: nn.GELU(approximate="tanh"), "relu": nn.ReLU, "tanh": nn.Tanh,
            "identity": nn.Identity}[name]


def make_layer(name, i, o):
    """The CPU module behind a name of LAYERS (parameters as constructed, fixed seed; "-trained": freq * (1 + 0.3 randn) with one
    entry 0 and one negative)."""
    from models.cheby import ChebyKANLayer
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    from models.nfkan import NaiveFourierKANLayer
    from models.sinekan import SineKANLayer
    torch.manual_seed(4321)
    if name.startswith("cheby"):
        return ChebyKANLayer(i, o, int(name[-1]))
    if name.startswith("sine"):
        layer = SineKANLayer(i, o, grid_size=28, is_first=True) if "grid28" in name else SineKANLayer(i, o, grid_size=4)
        if name.endswith("trained"):
            with torch.no_grad():
                layer.freq.mul_(1 + 0.3 * torch.randn(layer.freq.shape))
                layer.freq[..., 1] = 0.0
                layer.freq[..., 2] = -layer.freq[..., 2].abs()
        return layer
    if name.startswith("fourier"):
        return NaiveFourierKANLayer(i, o, gridsize=int(name.split("G")[1]))
    if name.startswith("rbf"):
        return FastKANLayer(i, o, base_activation=_act_module(name[4:] or "silu")())
    if name == "bspline-perturbed":          # tests/test_layer_forms_gpu.py's layer: knots no longer g0 + j h, per feature
        from tests.test_layer_forms_gpu import _kanlinear_perturbed
        return _kanlinear_perturbed(i, o)
    if name == "bspline-order2":
        return KANLinear(i, o, grid_size=5, spline_order=2)
    if name.startswith("bspline-"):
        return KANLinear(i, o, base_activation=_act_module(name[8:]))
    a, b, n = next(g for g in BSPLINE_GRIDS + CLOSED_FORM_GRIDS if grid_name(g) == name)
    return KANLinear(i, o, grid_size=n, grid_range=[a, b])


def act_name(fn):
    from kanvit import ops
    return ACTS[ops.base_act_of(fn)]


def params_of(layer):
    """The family description basis() reads, from a module's buffers and parameters (CPU float32 tensors)."""
    kind = type(layer).__name__
    if kind == "ChebyKANLayer":
        return {"family": "cheby", "I": layer.inputdim, "G": layer.degree + 1, "GP": layer.degree + 1}
    if kind == "NaiveFourierKANLayer":
        return {"family": "fourier", "I": layer.inputdim, "G": layer.gridsize, "GP": 2 * layer.gridsize}
    if kind == "SineKANLayer":
        return {"family": "sine", "I": layer.input_dim, "G": layer.grid_size, "GP": layer.grid_size,
                "freq": layer.freq.detach().cpu().reshape(-1), "phase": layer.phase.detach().cpu().reshape(layer.input_dim, -1)}
    if kind == "KANLinear":
        nb = layer.grid_size + layer.spline_order
        return {"family": "bspline", "I": layer.in_features, "G": nb, "GP": nb + 1, "grid": layer.grid.detach().cpu(),
                "order": layer.spline_order, "act": act_name(layer.base_activation)}
    assert kind == "FastKANLayer"
    return {"family": "rbf", "I": layer.input_dim, "G": layer.num_grids, "GP": layer.num_grids + 1,
            "centres": layer.rbf.grid.detach().cpu(), "h": float(layer.rbf.denominator), "act": act_name(layer.base_activation)}


def input_set(name, layer, m):
    """(x[m, I], u[m, I] | None, src, specials) for a layer of LAYERS: the family's set, or the base column's +-BASE_SWEEP for the
    layers named after an activation."""
    p = params_of(layer)
    fam, i = p["family"], p["I"]
    if name[name.find("-") + 1:] in ACTS:
        x, src, sp = base_inputs(m, i)
        return x, (x.clone() if fam == "rbf" else None), src, sp
    if fam == "cheby":
        x, src, sp = cheby_inputs(m, i)
        return x, None, src, sp
    if fam == "fourier":
        x, src, sp = fourier_inputs(p["G"], m, i)
        return x, None, src, sp
    if fam == "sine":
        x, src, sp = sine_inputs(p["freq"], p["phase"], m)
        return x, None, src, sp
    if fam == "bspline":
        x, src, sp = bspline_inputs(p["grid"], m)
        return x, None, src, sp
    return rbf_inputs(p["centres"], m, i)
