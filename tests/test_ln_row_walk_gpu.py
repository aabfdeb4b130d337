"""The persistent row walkers of csrc/addln.hip past their grid caps: addln_fwd_kernel / addln_bwd_kernel (ln_grid: 512 work-groups
of 8 waves, one row per wave and pass) and kan_ln_bwd_kernel (ln_kan_grid: 2048 / x_group_mod work-groups of 4 waves).  Above the
cap a wave loops over several rows and carries its per-lane dgamma / dbeta sums from row to row; the last pass is ragged (some
waves have a row, others do not).  Every training step of the benchmark runs the kernels that way, the other suites stop below
the caps.

 (1) kanvit_addln_fwd_ex / _bwd_ex through the C ABI at the smallest row counts that cross the cap, one per register form
     (NV = 1..4), with / without delta and dres;
 (2) kanvit_layer_ln_bwd with a hand-made descriptor and synthetic gradients, one case per kan_ln_bwd_kernel<NCH, NS>
     instantiation, multi-pass and ragged, plus dx = NULL, padded leading dimensions (NaN in the padding), run-to-run bits, and a
     single-pass case of the forms no other test reaches;
 (3) smaller addln edges through ops.add_layernorm: widths either side of the NV boundaries, eps other than 1e-5, constant rows
     (variance 0), and a mean that is large against the spread (the two-pass variance must not cancel).

References are float64 torch on the GPU from the same fp32 inputs.  The backward references take the fp32 (mean, rstd) the kernel
reads, widened to double, and evaluate dx / dgamma / dbeta in closed form: the backward arithmetic alone is under test.
Bounds: 2e-5 * max(1, max|ref|) elementwise (tests/test_addln_gpu.py); column sums 2e-6 * max(1, max_c sum_m |term|), the bound
tests/test_ff_epilogue_gpu.py uses for ordered fp32 column sums of the same hierarchical shape."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
U = 2.0 ** -24                     # fp32 unit roundoff


def _close(got, want, what):
    err = float((got.double() - want).abs().max())
    bound = 2e-5 * max(1.0, float(want.abs().max()))
    assert err < bound, f"{what}: max error {err:.3e}, bound {bound:.3e}"


def _colsum_close(got, want, terms_abs, what):
    """Ordered fp32 column sums: every column within 2e-6 * max(1, max_c sum_m |term|)."""
    err = float((got.double().flatten() - want.flatten()).abs().max())
    bound = 2e-6 * max(1.0, float(terms_abs.sum(0).max()))
    assert err <= bound, f"{what}: max column error {err:.3e}, bound {bound:.3e}"


# ------------------------------------------------------------------------------------------------
# (1) addln forward / backward, several rows per wave
# ------------------------------------------------------------------------------------------------
def _addln_fwd(x, delta, gamma, beta, eps=EPS):
    from kanvit import _lib, ops
    L = _lib.lib()
    M, D = x.shape
    xsum = torch.empty_like(x) if delta is not None else None
    y = torch.empty_like(x)
    mean = torch.empty(M, device=DEV)
    rstd = torch.empty(M, device=DEV)
    _lib.check(L.kanvit_addln_fwd_ex(M, D, eps, ops._ptr(x), ops._ptr(delta), 0, ops._ptr(gamma), ops._ptr(beta), ops._ptr(xsum),
                                     ops._ptr(y), 0, ops._ptr(mean), ops._ptr(rstd), ops._stream()), "kanvit_addln_fwd_ex")
    return (xsum if delta is not None else x), y, mean, rstd


def _addln_bwd(s, gamma, mean, rstd, dy, dres):
    from kanvit import _lib, ops
    L = _lib.lib()
    M, D = s.shape
    dx = torch.empty_like(s)
    dg = torch.empty(D, device=DEV)
    db = torch.empty(D, device=DEV)
    nb = int(L.kanvit_addln_bwd_workspace(M, D))
    ws = ops._workspace(nb, s.device)
    _lib.check(L.kanvit_addln_bwd_ex(M, D, ops._ptr(s), ops._ptr(gamma), ops._ptr(mean), ops._ptr(rstd), ops._ptr(dy), 0, ops._ptr(dres),
                                     ops._ptr(dx), None, ops._ptr(dg), ops._ptr(db), ops._ptr(ws), C.c_size_t(nb), ops._stream()),
               "kanvit_addln_bwd_ex")
    return dx, dg, db


def _assert_addln_walk(M, D):
    from kanvit import _lib
    nb = int(_lib.lib().kanvit_addln_bwd_workspace(M, D))
    assert nb == 4 * 512 * 2 * D and M > 4096, \
        f"the addln grid cap moved (workspace {nb} bytes for M={M}, D={D}): re-choose M so that a wave takes more than one row"


# (M, D): one wave takes a second row | NV = 2, ragged third pass | NV = 3 (ViT-B width), ragged fourth pass | NV = 4, LDS at 64 KiB
WALK_SHAPES = [(4097, 64), (8200, 384), (12293, 768), (8197, 1024)]


@pytest.mark.parametrize("M,D", WALK_SHAPES)
@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("with_delta", [True, False])
def test_addln_multi_row_walk(M, D, with_delta, with_dres):
    _assert_addln_walk(M, D)
    torch.manual_seed(M + D)
    gamma = torch.randn(D, device=DEV) * 0.5 + 1.0
    beta = torch.randn(D, device=DEV) * 0.3
    x = torch.randn(M, D, device=DEV) * 2.0 + 0.7
    delta = torch.randn(M, D, device=DEV) if with_delta else None
    dy = torch.randn(M, D, device=DEV)
    dres = torch.randn(M, D, device=DEV) if with_dres else None

    s, y, mean, rstd = _addln_fwd(x, delta, gamma, beta)
    s64 = x.double() + delta.double() if with_delta else x.double()
    mu64 = s64.mean(1, keepdim=True)
    rs64 = (s64.var(1, unbiased=False, keepdim=True) + EPS).rsqrt()
    _close(s, s64, "xsum")
    _close(y, (s64 - mu64) * rs64 * gamma.double() + beta.double(), "y")
    _close(mean, mu64[:, 0], "mean")
    _close(rstd, rs64[:, 0], "rstd")
    del s64, mu64, rs64

    # backward on the kernel's own xsum / mean / rstd, the reference on the same values widened to double
    dx, dg, db = _addln_bwd(s, gamma, mean, rstd, dy, dres)
    dy64 = dy.double()
    xh = (s.double() - mean.double()[:, None]) * rstd.double()[:, None]
    gy = dy64 * gamma.double()
    want_dx = rstd.double()[:, None] * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    if with_dres:
        want_dx += dres.double()
    _close(dx, want_dx, "dx")
    del want_dx, gy
    t = dy64 * xh
    _colsum_close(dg, t.sum(0), t.abs(), "dgamma")
    _colsum_close(db, dy64.sum(0), dy64.abs(), "dbeta")

    dx2, dg2, db2 = _addln_bwd(s, gamma, mean, rstd, dy, dres)
    assert torch.equal(dg, dg2) and torch.equal(db, db2)          # ordered partials: bitwise run to run
    assert torch.equal(dx, dx2)


def test_addln_multi_row_walk_bf16_boundary():
    """bf16 delta, bf16 y and a bf16 gradient on y at (8200, 384): the relations of test_addln_gpu.py's
    test_bf16_tensors_at_the_boundary against the all-fp32 route, with every wave walking two or three rows."""
    from kanvit.ops import add_layernorm
    M, D = 8200, 384
    _assert_addln_walk(M, D)
    torch.manual_seed(M + D)
    norm = torch.nn.LayerNorm(D).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(D) * 0.5 + 1.0)
        norm.bias.copy_(torch.randn(D) * 0.3)
    x = (torch.randn(M, D, device=DEV) * 2.0 + 0.7).requires_grad_(True)
    delta = torch.randn(M, D, device=DEV).bfloat16().requires_grad_(True)
    ws = torch.randn(M, D, device=DEV)
    wy = torch.randn(M, D, device=DEV).bfloat16()

    s, y = add_layernorm(x, delta, norm, y_bf16=True)
    assert y.dtype == torch.bfloat16 and s.dtype == torch.float32
    torch.autograd.backward([s, y], [ws, wy])
    assert delta.grad.dtype == torch.bfloat16
    dg, db = norm.weight.grad.clone(), norm.bias.grad.clone()

    x2 = x.detach().clone().requires_grad_(True)
    d2 = delta.detach().float().requires_grad_(True)
    s2, y2 = add_layernorm(x2, d2, norm)
    norm.zero_grad()
    torch.autograd.backward([s2, y2], [ws, wy.float()])
    assert torch.equal(s, s2)
    assert torch.equal(y, y2.bfloat16())
    assert torch.equal(x.grad, x2.grad)                      # same arithmetic: bf16 -> fp32 widening is exact
    assert torch.equal(delta.grad, d2.grad.bfloat16())
    assert torch.equal(dg, norm.weight.grad) and torch.equal(db, norm.bias.grad)


# ------------------------------------------------------------------------------------------------
# (2) kanvit_layer_ln_bwd, every kan_ln_bwd_kernel<NCH, NS> instantiation
# ------------------------------------------------------------------------------------------------
G = 8


def _lpr_log2(I):
    k = 3
    while (1 << k) < I // 4 and k < 6:
        k += 1
    return k


def _rows_per_wg(I):
    return 4 * (64 >> _lpr_log2(I))


class _LnKanCase:
    """Inputs of one kanvit_layer_ln_bwd call.  pad = (extra ldx, extra ldu, extra bparam_stride): the padding holds NaN."""

    def __init__(self, M, I, xmod, groups, pad=(0, 0, 0), seed=0):
        from kanvit import _lib
        self.M, self.I, self.xmod, self.groups, self.ns = M, I, xmod, groups, groups // xmod
        self.wx, self.wu = xmod * I, groups * I
        self.ldx, self.ldu, self.bps = self.wx + pad[0], self.wu + pad[1], G + 2 * I + pad[2]
        g = torch.Generator(device=DEV).manual_seed(1000 * I + groups + seed)
        nan = float("nan")
        self.x = torch.full((M, self.ldx), nan, device=DEV)
        self.x[:, :self.wx] = torch.randn(M, self.wx, device=DEV, generator=g) * 1.5 + 0.3
        self.du = torch.full((M, self.ldu), nan, device=DEV)
        self.du[:, :self.wu] = torch.randn(M, self.wu, device=DEV, generator=g)
        self.dx0 = torch.full((M, self.ldx), nan, device=DEV)
        self.dx0[:, :self.wx] = torch.randn(M, self.wx, device=DEV, generator=g)
        self.bp = torch.full((groups, self.bps), nan, device=DEV)              # [centres | gamma | beta | padding]
        self.bp[:, :G] = torch.linspace(-2.0, 2.0, G, device=DEV)
        self.bp[:, G:G + I] = 1.0 + 0.3 * torch.randn(groups, I, device=DEV, generator=g)
        self.bp[:, G + I:G + 2 * I] = 0.2 * torch.randn(groups, I, device=DEV, generator=g)
        x3 = self.x[:, :self.wx].view(M, xmod, I).double()
        self.stats = torch.stack([x3.mean(-1), (x3.var(-1, unbiased=False) + EPS).rsqrt()], dim=-1).float().contiguous()
        self.desc = _lib.LayerDesc(family=_lib.RBF, groups=groups, x_group_mod=xmod, I=I, O=I, G=G, has_base=1, rbf_inv_h=1.75,
                                   flags=_lib.FLAG_FUSED_LN | _lib.FLAG_UNIFORM_KNOTS, M=M, ldx=self.ldx, ldu=self.ldu, ldy=groups * I,
                                   bparam_stride=self.bps, ln_eps=EPS)

    def assert_walk(self):
        from kanvit import _lib
        cap = 2048 // self.xmod
        nb = int(_lib.lib().kanvit_layer_ln_bwd_workspace(C.byref(self.desc)))
        assert nb == 4 * cap * 2 * self.groups * self.I and self.M > cap * _rows_per_wg(self.I), \
            (f"the kan_ln grid cap moved (workspace {nb} bytes for M={self.M}, I={self.I}, x_group_mod={self.xmod}): "
             "re-choose M so that the kernel makes at least two passes")

    def run(self, with_dx=True):
        from kanvit import _lib, ops
        L = _lib.lib()
        dx = self.dx0.clone() if with_dx else None
        dgb = torch.empty(2, self.groups, self.I, device=DEV)
        nb = int(L.kanvit_layer_ln_bwd_workspace(C.byref(self.desc)))
        ws = ops._workspace(nb, self.x.device)
        _lib.check(L.kanvit_layer_ln_bwd(C.byref(self.desc), ops._ptr(self.x), ops._ptr(self.stats), ops._ptr(self.bp), ops._ptr(self.du),
                                         ops._ptr(dx), ops._ptr(dgb[0]), ops._ptr(dgb[1]), ops._ptr(ws), C.c_size_t(nb), ops._stream()),
                   "kanvit_layer_ln_bwd")
        return dx, dgb[0], dgb[1]

    def check(self, dx, dg, db):
        M, I, xmod, ns = self.M, self.I, self.xmod, self.ns
        st = self.stats.double()
        mu, rs = st[..., 0:1], st[..., 1:2]                                           # [M, xmod, 1]
        xhat = (self.x[:, :self.wx].view(M, xmod, I).double() - mu) * rs              # [M, xmod, I]
        du = self.du[:, :self.wu].view(M, ns, xmod, I).double()                      # group g = s * xmod + gx
        gamma = self.bp[:, G:G + I].view(ns, xmod, I).double()
        if dx is not None:
            dxh = (du * gamma).sum(1)
            want = self.dx0[:, :self.wx].view(M, xmod, I).double() + rs * (dxh - dxh.mean(-1, keepdim=True)
                                                                           - xhat * (dxh * xhat).mean(-1, keepdim=True))
            _close(dx[:, :self.wx], want.reshape(M, self.wx), "dx")
            assert torch.isnan(dx[:, self.wx:]).all()                                # the padding of dx is never written
            del dxh, want
        t = du * xhat[:, None]
        _colsum_close(dg, t.sum(0), t.abs().reshape(M, -1), "dgamma")
        _colsum_close(db, du.sum(0), du.abs().reshape(M, -1), "dbeta")


# (I, x_group_mod, groups, M): M = the smallest row count with at least two passes and a ragged last one
LN_KAN_WALK = [
    pytest.param(32, 1, 1, 65569, id="1x1-lpr8"),
    pytest.param(64, 1, 1, 32851, id="1x1-lpr16"),
    pytest.param(96, 1, 1, 16395, id="1x1-lpr32-idle-lanes"),
    pytest.param(320, 1, 1, 8197, id="2x1"),
    pytest.param(768, 1, 1, 16413, id="3x1-patch-embedding-three-passes"),
    pytest.param(1024, 1, 1, 8197, id="4x1"),
    pytest.param(64, 6, 18, 10965, id="1x3-qkv-three-passes"),
    pytest.param(320, 2, 6, 4103, id="2x3"),
]


@pytest.mark.parametrize("I,xmod,groups,M", LN_KAN_WALK)
def test_kan_ln_bwd_multi_pass(I, xmod, groups, M):
    case = _LnKanCase(M, I, xmod, groups)
    case.assert_walk()
    case.check(*case.run())


def test_kan_ln_bwd_multi_pass_without_dx():
    """dx = NULL (x needs no gradient): dgamma and dbeta alone."""
    case = _LnKanCase(10965, 64, 6, 18, seed=1)
    case.assert_walk()
    dx, dg, db = case.run(with_dx=False)
    assert dx is None
    case.check(None, dg, db)


def test_kan_ln_bwd_multi_pass_padded_leading_dimensions():
    """ldx, ldu and bparam_stride above their minimum, NaN in the padding: a read of it poisons the result."""
    case = _LnKanCase(4103, 320, 2, 6, pad=(12, 8, 4), seed=2)
    case.assert_walk()
    dx, dg, db = case.run()
    assert torch.isfinite(dg).all() and torch.isfinite(db).all() and torch.isfinite(dx[:, :case.wx]).all()
    case.check(dx, dg, db)


def test_kan_ln_bwd_multi_pass_bitwise_run_to_run():
    case = _LnKanCase(16395, 96, 1, 1, seed=3)
    case.assert_walk()
    a, b = case.run(), case.run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    case.check(*a)


@pytest.mark.parametrize("I,xmod,groups", [pytest.param(320, 1, 1, id="2x1"), pytest.param(1024, 1, 1, id="4x1"),
                                           pytest.param(320, 2, 6, id="2x3")])
def test_kan_ln_bwd_single_pass_of_the_otherwise_unreached_forms(I, xmod, groups):
    """M = 300: one pass.  Tells a failure of the instantiation from a failure of the row walk."""
    from kanvit import _lib
    case = _LnKanCase(300, I, xmod, groups, seed=4)
    nb = int(_lib.lib().kanvit_layer_ln_bwd_workspace(C.byref(case.desc)))
    assert nb == 4 * 75 * 2 * groups * I                      # 300 rows / 4 per work-group: below the cap
    case.check(*case.run())


# ------------------------------------------------------------------------------------------------
# (3) smaller addln edges, through ops.add_layernorm at M = 37
# ------------------------------------------------------------------------------------------------
def _norm(D, eps=EPS, seed=0):
    torch.manual_seed(seed + D)
    norm = torch.nn.LayerNorm(D, eps=eps).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(D) * 0.5 + 1.0)
        norm.bias.copy_(torch.randn(D) * 0.3)
    return norm


def _fp64_add_layernorm(x, delta, norm, ws, wy):
    """[s, y, dx, dgamma, dbeta, (ddelta)] of loss = sum(s * ws) + sum(y * wy) in float64 (ws None: the y term alone)."""
    D = x.shape[-1]
    n64 = torch.nn.LayerNorm(D, eps=norm.eps).double().to(DEV)
    n64.load_state_dict({k: v.double() for k, v in norm.state_dict().items()})
    x64 = x.detach().double().requires_grad_(True)
    d64 = delta.detach().double().requires_grad_(True) if delta is not None else None
    s64 = x64 + d64 if delta is not None else x64
    y64 = n64(s64)
    loss = (y64 * wy.double()).sum()
    if ws is not None:
        loss = loss + (s64 * ws.double()).sum()
    loss.backward()
    out = [s64.detach(), y64.detach(), x64.grad, n64.weight.grad, n64.bias.grad]
    if delta is not None:
        out.append(d64.grad)
    return out


def _run_add_layernorm(x, delta, norm, ws, wy):
    from kanvit.ops import add_layernorm
    norm.zero_grad()
    xg = x.detach().clone().requires_grad_(True)
    dg = delta.detach().clone().requires_grad_(True) if delta is not None else None
    s, y = add_layernorm(xg, dg, norm)
    loss = (y * wy).sum()
    if ws is not None:
        loss = loss + (s * ws).sum()
    loss.backward()
    out = [s.detach(), y.detach(), xg.grad, norm.weight.grad.clone(), norm.bias.grad.clone()]
    if delta is not None:
        out.append(dg.grad)
    return out


NAMES = ["s", "y", "dx", "dgamma", "dbeta", "ddelta"]


@pytest.mark.parametrize("D", [256, 512, 516, 772])
@pytest.mark.parametrize("with_delta", [True, False])
def test_width_either_side_of_a_register_form_boundary(D, with_delta):
    """D = 256 | 512 fill NV = 1 | 2 exactly; 516 and 772 put one float4 of one lane into the next form's last vector."""
    M = 37
    norm = _norm(D)
    x = torch.randn(M, D, device=DEV) * 2.0 + 0.7
    delta = torch.randn(M, D, device=DEV) if with_delta else None
    ws, wy = torch.randn(M, D, device=DEV), torch.randn(M, D, device=DEV)
    got = _run_add_layernorm(x, delta, norm, ws, wy)
    want = _fp64_add_layernorm(x, delta, norm, ws, wy)
    for n, g, w in zip(NAMES, got, want):
        _close(g, w, n)


@pytest.mark.parametrize("eps", [1e-3, 1e-6])
def test_non_default_eps(eps):
    """Per-row standard deviation 1e-2 (variance 1e-4): eps = 1e-3 dominates the variance, 1e-6 is 1 % of it.  A kernel that
    ignored the argument (1e-5) is off by a factor 3 in rstd at the first and by 4 % at the second."""
    M, D = 37, 64
    norm = _norm(D, eps=eps)
    x = torch.randn(M, D, device=DEV) * 1e-2 + 0.05 * torch.randn(M, 1, device=DEV)
    ws, wy = torch.randn(M, D, device=DEV), torch.randn(M, D, device=DEV)
    got = _run_add_layernorm(x, None, norm, ws, wy)
    want = _fp64_add_layernorm(x, None, norm, ws, wy)
    for n, g, w in zip(NAMES, got, want):
        _close(g, w, n)
    _, _, _, rstd = _addln_fwd(x, None, norm.weight.detach(), norm.bias.detach(), eps=eps)
    _close(rstd, (x.double().var(1, unbiased=False) + eps).rsqrt(), "rstd")


@pytest.mark.parametrize("D", [64, 768])
def test_constant_rows(D):
    """Every row is one repeated value c (row 0: zero): the variance is 0, rstd = 1 / sqrt(eps), y = beta.

    fp32 bounds.  The kernel's row mean is c after at most three roundings (the per-lane sum of up to 4 float4, the product with
    the rounded 1 / D, its rounding; the xor tree only doubles): |mean - c| <= 4u|c| with u = 2^-24, so
    |y - beta| <= 4u |c| rstd |gamma| + u |beta| (all exact for D a power of two).  rstd, relative: eps rounded to fp32 (u / 2),
    rsqrtf within 1 ulp (2u), the store (u), and the residual variance (4u c)^2 against eps (8 u^2 c^2 / eps, about u at |c| = 5)."""
    M = 37
    norm = _norm(D)
    torch.manual_seed(D)
    c = torch.randn(M, 1, device=DEV) * 2.0
    c[0] = 0.0
    x = c.expand(M, D).contiguous()
    wy = torch.randn(M, D, device=DEV)
    got = _run_add_layernorm(x, None, norm, None, wy)
    want = _fp64_add_layernorm(x, None, norm, None, wy)
    rs = 1.0 / math.sqrt(EPS)
    gmax, bmax, cmax = float(norm.weight.detach().abs().max()), float(norm.bias.detach().abs().max()), float(c.abs().max())
    err = float((got[1].double() - norm.bias.detach().double()).abs().max())
    assert err <= 4 * U * cmax * rs * gmax + U * bmax, err
    _, _, mean, rstd = _addln_fwd(x, None, norm.weight.detach(), norm.bias.detach())
    assert float((rstd.double() - rs).abs().max()) <= (3.5 * U + 8 * U * U * cmax * cmax / EPS) * rs
    assert float((mean.double() - c[:, 0].double()).abs().max()) <= 4 * U * cmax
    assert torch.isfinite(got[2]).all()
    _close(got[2], want[2], "dx")
    _close(got[4], want[4], "dbeta")


def test_large_mean_two_pass_variance_does_not_cancel(capsys):
    """x = 100 + randn at D = 768: mean^2 is 1e4 times the variance.  No fixed tolerance: the fp32 floor of this input is set by
    the rounding of the mean, so the kernel is held to 4x the error of torch's own fp32 layer_norm (forward and autograd
    backward) against the float64 reference -- both are fp32 two-pass / Welford algorithms, the factor covers a different
    summation order and nothing more.  A one-pass E[x^2] - E[x]^2 variance would be out by about two orders of magnitude."""
    M, D = 37, 768
    norm = _norm(D)
    torch.manual_seed(5)
    x = 100.0 + torch.randn(M, D, device=DEV)
    wy = torch.randn(M, D, device=DEV)
    got = _run_add_layernorm(x, None, norm, None, wy)
    want = _fp64_add_layernorm(x, None, norm, None, wy)
    xt = x.clone().requires_grad_(True)
    yt = torch.nn.functional.layer_norm(xt, (D,), norm.weight.detach(), norm.bias.detach(), norm.eps)
    dxt, = torch.autograd.grad(yt, xt, wy)
    err = lambda a, b: float((a.double() - b).abs().max())
    ey, edx = err(got[1], want[1]), err(got[2], want[2])
    ty, tdx = err(yt.detach(), want[1]), err(dxt, want[2])
    with capsys.disabled():
        print(f"\nlarge mean (x = 100 + randn, D = 768): max|y - y64| kernel {ey:.3e} torch-fp32 {ty:.3e}; "
              f"max|dx - dx64| kernel {edx:.3e} torch-fp32 {tdx:.3e}")
    assert ey <= 4 * ty, (ey, ty)
    assert edx <= 4 * tdx, (edx, tdx)
