"""Float64 statements of the fused small feed-forward (csrc/ff_small.hip) and the integer-lattice inputs on which its fp32
arithmetic is exact.  Shared by tests/test_ff_ref_cpu.py (the closed forms against autograd, the lattice precondition) and
tests/test_ff_walk_gpu.py (the kernels against the closed forms).  Plain torch, any device.

    FF       y = relu(x W1^T + b1) W2^T + b2                          x[M][D], W1[F][D], W2[D][F]      (model.py:25-29)
    LN + FF  the same on x = (s - mean) * rstd * gamma + beta          with the row statistics GIVEN, as the backward kernel gets
                                                                       them; ds is the LayerNorm backward through those statistics

The ReLU passes the gradient where the pre-activation is > 0 (threshold_backward on the saved output): a pre-activation of
exactly +0 or -0 is dead.

Lattice inputs.  Every operand is a small integer (rstd a power of two), so every product and every partial sum of every
contraction is a multiple of a power of two q (the sum's quantum) and no larger than S = sum |terms|.  While S / q < 2^24 all of
them are fp32 numbers: the result does not depend on the summation order, on fused multiply-adds or on how the rows are split
over tiles, work-groups and partial buffers, and equals the float64 result bit for bit.  lattice_margin() evaluates S / q for
every sum the kernels form; the exact tests assert it, so that a wrong recipe fails as a precondition and not as a kernel."""
import torch

D, F = 64, 256
EXACT_LIMIT = float(2 ** 24)
DEAD_ZERO, DEAD_NEGZERO, DEAD_BIAS, ALIVE_BIAS = 5, 6, 7, 8      # hidden units with a pinned ReLU state (lattice_weights)


# ------------------------------------------------------------------------------------------------
# closed forms
# ------------------------------------------------------------------------------------------------
def ff_forward64(x, w1, b1, w2, b2):
    x, w1, b1, w2, b2 = (t.double() for t in (x, w1, b1, w2, b2))
    return torch.relu(x @ w1.t() + b1) @ w2.t() + b2


def ff_backward64(x, w1, b1, w2, dy):
    """dict(pre, h, dhm, dx, dw1, db1, dw2, db2) of loss = sum(FF(x) * dy); dhm is the masked hidden gradient [M][F]."""
    x, w1, b1, w2, dy = (t.double() for t in (x, w1, b1, w2, dy))
    pre = x @ w1.t() + b1
    h = torch.relu(pre)
    dhm = (dy @ w2) * (pre > 0)
    return {"pre": pre, "h": h, "dhm": dhm, "dx": dhm @ w1, "dw1": dhm.t() @ x, "db1": dhm.sum(0), "dw2": dy.t() @ h, "db2": dy.sum(0)}


def ln_apply64(s, mean, rstd, gamma, beta):
    xh = (s.double() - mean.double()[:, None]) * rstd.double()[:, None]
    return xh, xh * gamma.double() + beta.double()


def lnff_backward64(s, mean, rstd, gamma, beta, w1, b1, w2, dy, ds_in=None):
    """ff_backward64 on x = LN(s; mean, rstd) plus xh, x, v (= d loss / d LN output), ds, dgamma, dbeta."""
    xh, x = ln_apply64(s, mean, rstd, gamma, beta)
    out = ff_backward64(x, w1, b1, w2, dy)
    v = out.pop("dx")
    gy = v * gamma.double()
    ds = rstd.double()[:, None] * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    if ds_in is not None:
        ds = ds + ds_in.double()
    out.update(xh=xh, x=x, v=v, ds=ds, dgamma=(v * xh).sum(0), dbeta=v.sum(0))
    return out


def relu_kink_rows(x, w1, b1):
    """Rows of x with a pre-activation so close to the ReLU kink that fp32 arithmetic cannot tell its sign: |pre| <= gamma * S with
    S = |x| |W1|^T + |b1| and gamma = (D + 8) u -- the standard bound (D + 1) u S of an fp32 dot product of D terms plus a bias in
    any order, and 7 u more for an x that is itself a rounded LayerNorm output.  There the mask of the float64 reference and the
    mask of a correct fp32 kernel may differ, and with it a whole gradient row: at 65536 rows (1.7e7 pre-activations with a density
    of about 0.7 per unit at zero) a few hundred elements are that close, and one or two of them do flip.  A test on random data
    gives such rows a zero dy, which makes their gradient independent of the mask, and says how many there were."""
    x, w1, b1 = x.double(), w1.double(), b1.double()
    pre = x @ w1.t() + b1
    s = x.abs() @ w1.abs().t() + b1.abs()
    return (pre.abs() <= (D + 8) * 2.0 ** -24 * s).any(1)


def row_stats64(s, eps):
    s = s.double()
    return s.mean(1), (s.var(1, unbiased=False) + eps).rsqrt()


# ------------------------------------------------------------------------------------------------
# lattice inputs (CPU, fp32)
# ------------------------------------------------------------------------------------------------
def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def lattice_weights(g):
    """W1, W2 in {-1, 0, 1} with half of the entries zeroed; b1, b2 in [-3, 3].  Units DEAD_ZERO / DEAD_NEGZERO: W1 row 0 and
    b1 = +0.0 / -0.0 (pre-activation exactly zero in every row); DEAD_BIAS: b1 = -100; ALIVE_BIAS: b1 = +100."""
    w1 = _ints(g, -1, 1, F, D) * (torch.rand(F, D, generator=g) < 0.5)
    w2 = _ints(g, -1, 1, D, F) * (torch.rand(D, F, generator=g) < 0.5)
    b1, b2 = _ints(g, -3, 3, F), _ints(g, -3, 3, D)
    w1[DEAD_ZERO] = 0.0
    w1[DEAD_NEGZERO] = 0.0
    b1[DEAD_ZERO], b1[DEAD_NEGZERO], b1[DEAD_BIAS], b1[ALIVE_BIAS] = 0.0, -0.0, -100.0, 100.0
    return w1, b1, w2, b2


def lattice_ff(M, seed=0):
    """Inputs of kanvit_ff_small_fwd / _bwd: x in {-2..2}, dy in {-1, 0, 1}."""
    g = torch.Generator().manual_seed(1000 + seed)
    w1, b1, w2, b2 = lattice_weights(g)
    return {"x": _ints(g, -2, 2, M, D), "w1": w1, "b1": b1, "w2": w2, "b2": b2, "dy": _ints(g, -1, 1, M, D)}


def lattice_ln(M, seed=0):
    """Inputs of kanvit_lnff_small_bwd with synthetic row statistics: mean in {-3..3}, rstd in {0.5, 1, 2}, s = mean + {-2..2},
    gamma in {-1, 0, 1} (columns 0..3: 0, 2, -2, 1), beta in {-2..2}, ds_in in {-4..4}."""
    g = torch.Generator().manual_seed(2000 + seed)
    w1, b1, w2, b2 = lattice_weights(g)
    mean = _ints(g, -3, 3, M)
    rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (M,), generator=g)]
    gamma = _ints(g, -1, 1, D)
    gamma[:4] = torch.tensor([0.0, 2.0, -2.0, 1.0])
    return {"s": mean[:, None] + _ints(g, -2, 2, M, D), "mean": mean, "rstd": rstd, "gamma": gamma, "beta": _ints(g, -2, 2, D),
            "w1": w1, "b1": b1, "w2": w2, "b2": b2, "dy": _ints(g, -1, 1, M, D), "ds_in": _ints(g, -4, 4, M, D)}


# ------------------------------------------------------------------------------------------------
# the exactness precondition
# ------------------------------------------------------------------------------------------------
def quantum(t):
    """The largest power of two that divides every entry of t (float64 arithmetic; 1.0 for an all-zero tensor)."""
    t = t.double().flatten()
    t = t[t != 0]
    if t.numel() == 0:
        return 1.0
    assert torch.isfinite(t).all()
    m, e = torch.frexp(t)                                     # t = m * 2^e, 0.5 <= |m| < 1: m * 2^53 is an integer
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()                                 # lowest set bit
    return float((low * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 53).double())).min())


def _ratio(abs_sums, *quanta):
    q = min(quanta)
    return float(abs_sums.max()) / q


def _matsum(a, b, bias=None):
    """max S / q of the contraction a @ b (+ bias): S = |a| @ |b| (+ |bias|), q = q(a) q(b) (or q(bias) if that is finer)."""
    s = a.abs() @ b.abs()
    qs = [quantum(a) * quantum(b)]
    if bias is not None:
        s = s + bias.abs()
        qs.append(quantum(bias))
    return _ratio(s, *qs)


def lattice_margin(c, ln, with_ds_in=True, forward_only=False):
    """{sum name: max S / q} over every sum the kernels form on the inputs c (lattice_ff / lattice_ln).  Exact in fp32 while
    every value is below EXACT_LIMIT."""
    c = {k: v.double() for k, v in c.items()}
    out = {}
    if ln:
        r = lnff_backward64(c["s"], c["mean"], c["rstd"], c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["dy"],
                            c["ds_in"] if with_ds_in else None)
        xh, x, g = r["xh"], r["x"], c["gamma"]
        d = c["s"] - c["mean"][:, None]
        out["s-mean"] = _ratio(c["s"].abs() + c["mean"].abs()[:, None], quantum(c["s"]), quantum(c["mean"]))
        out["xhat"] = _ratio(d.abs() * c["rstd"][:, None], quantum(d) * quantum(c["rstd"]))
        out["ln"] = _ratio((xh * g).abs() + c["beta"].abs(), quantum(xh) * quantum(g), quantum(c["beta"]))
    else:
        r = ff_backward64(c["x"], c["w1"], c["b1"], c["w2"], c["dy"])
        x = c["x"]
    out["pre"] = _matsum(x, c["w1"].t(), c["b1"])
    out["y"] = _matsum(r["h"], c["w2"].t(), c["b2"])
    if forward_only:
        return out
    out["dh"] = _matsum(c["dy"], c["w2"])
    out["dx"] = _matsum(r["dhm"], c["w1"])
    out["dw1"] = _matsum(r["dhm"].t(), x)
    out["dw2"] = _matsum(c["dy"].t(), r["h"])
    out["db1"] = _ratio(r["dhm"].abs().sum(0), quantum(r["dhm"]))
    out["db2"] = _ratio(c["dy"].abs().sum(0), quantum(c["dy"]))
    if ln:
        v, rs = r["v"], c["rstd"][:, None]
        gy = v * g
        q_gy, q_t2 = quantum(v) * quantum(g), quantum(v) * quantum(g) * quantum(xh)
        t1, t2 = gy.sum(1, keepdim=True), (gy * xh).sum(1, keepdim=True)
        out["v*gamma"] = _ratio(gy.abs(), q_gy)
        out["t1"] = _ratio(gy.abs().sum(1), q_gy)
        out["t2"] = _ratio((gy * xh).abs().sum(1), q_t2)
        q_in = min(q_gy, q_gy / D, q_t2 * quantum(xh) / D)                   # gy - t1 / D - xh * t2 / D
        inner = gy.abs() + t1.abs() / D + (xh * t2).abs() / D
        out["xhat*t2"] = _ratio((xh * t2).abs(), q_t2 * quantum(xh))
        out["ds-inner"] = _ratio(inner, q_in)
        q_ds = q_in * quantum(c["rstd"])
        out["ds"] = _ratio(inner * rs + (c["ds_in"].abs() if with_ds_in else 0.0), q_ds, quantum(c["ds_in"]) if with_ds_in else q_ds)
        out["dgamma"] = _ratio((v * xh).abs().sum(0), quantum(v) * quantum(xh))
        out["dbeta"] = _ratio(v.abs().sum(0), quantum(v))
    return out


def relu_state(c, ln):
    """(fraction of pre-activations exactly 0, > 0, < 0; the pre-activation matrix) of the lattice inputs c."""
    x = ln_apply64(c["s"], c["mean"], c["rstd"], c["gamma"], c["beta"])[1] if ln else c["x"].double()
    pre = x @ c["w1"].double().t() + c["b1"].double()
    n = pre.numel()
    return float((pre == 0).sum()) / n, float((pre > 0).sum()) / n, float((pre < 0).sum()) / n, pre


def assert_lattice(c, ln, with_ds_in=True, forward_only=False):
    """The precondition of an exact test: every sum exact in fp32, enough ReLU ties / alive / dead units, and the four pinned
    hidden units in the state their bias is meant to give them.  Returns the margins."""
    for k, v in c.items():
        assert v.dtype == torch.float32 and torch.isfinite(v).all(), k
    m = lattice_margin(c, ln, with_ds_in, forward_only)
    worst = max(m, key=m.get)
    assert m[worst] < EXACT_LIMIT, f"lattice precondition: sum '{worst}' has S / q = {m[worst]:.3e} >= 2^24, fp32 is not exact on these inputs"
    ties, alive, dead, pre = relu_state(c, ln)
    assert ties >= 0.02 and alive >= 0.25 and dead >= 0.25, f"lattice precondition: ties {ties:.3f}, alive {alive:.3f}, dead {dead:.3f}"
    assert (pre[:, DEAD_ZERO] == 0).all() and (pre[:, DEAD_NEGZERO] == 0).all(), "lattice precondition: units 5 / 6 are not exact ties"
    assert (pre[:, DEAD_BIAS] < 0).all() and (pre[:, ALIVE_BIAS] > 0).all(), "lattice precondition: units 7 / 8 are not always dead / alive"
    return m


def to_f32_exact(t64):
    """A float64 reference of a lattice case as fp32; it has to be an fp32 number already."""
    t32 = t64.float()
    assert torch.equal(t32.double(), t64), "the float64 reference is not representable in fp32"
    return t32
