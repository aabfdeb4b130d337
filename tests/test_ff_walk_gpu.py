"""The persistent tile walkers of csrc/ff_small.hip (kanvit_ff_small_fwd / _bwd, kanvit_lnff_small_fwd / _bwd) past their grid caps,
the LayerNorm fused in front of them at its edges, and kanvit_split3_bf16 (csrc/ff_epilogue.hip) against its definition.

 (A) Exact: integer-lattice inputs (tests/_ff_ref.py) on which every fp32 product and partial sum of the kernels is exact, so y,
     dx / ds, dW1, db1, dW2, db2, dgamma and dbeta equal the float64 closed form BIT FOR BIT whatever the tile walk: one
     work-group walking all 25 tiles (KANVIT_FF_GRID=1), an uneven walk (=7: 4,4,4,4,3,3,3), a cap above the tile count (=64) and
     the default cap of 256 work-groups crossed by two tiles (M = 8229).  ReLU ties at +0 / -0 and always-dead / always-alive
     hidden units pin the `pre > 0` rule.  Workspace size, no write past it, run-to-run bits.  No tolerance in this section.
 (B) kanvit_lnff_small_fwd computes its own row statistics, so it is held to float64 within the project's bounds (2e-5 * max(1,
     max|ref|) elementwise, 1e-4 normwise for parameter gradients, 2e-6 * max(1, max_c sum_m |term|) for ordered column sums) at
     M = 32805 and 65536 rows (the forward walks), bitwise row independence of a walked launch against launches on row slices,
     LayerNorm edges at M = 37 (constant rows, eps other than 1e-5, a mean large against the spread, gamma with zero and negative
     entries), the TransformerBlock route under another grid, and what the entry points refuse without a launch.
 (C) kanvit_split3_bf16 bitwise against hi = bf16(v), lo = bf16(v - hi): every fused form, mask rows with special values, a padded
     mask, a shape whose grid-stride loop takes a second step, refusals.

References are float64 torch from the same fp32 inputs; the backward references of (B) take the kernel's own fp32 s / mean / rstd
widened to double, as tests/test_ln_row_walk_gpu.py does.  At tens of thousands of random rows a few pre-activations are closer to
zero than fp32 can resolve and their ReLU mask is not defined at that precision: those rows get dy = 0 (_ff_ref.relu_kink_rows).
Measured errors, and what the file found: profiles/ff_walk_tests.md."""
import contextlib
import ctypes as C
import functools
import math

import pytest
import torch

from tests import _ff_ref as R
from tests._util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, F = R.D, R.F
EPS = 1e-5
U = 2.0 ** -24                               # fp32 unit roundoff
PART = 2 * F * D + F + 3 * D                 # floats of one work-group's partial: dW1 | dW2^T | db1 | db2 | dgamma | dbeta
EINVAL, ENOMEM = -22, -12
NAN = float("nan")
W_KEYS = ("w1", "b1", "w2", "b2")


# ------------------------------------------------------------------------------------------------
# the four entry points through ctypes
# ------------------------------------------------------------------------------------------------
def _L():
    from kanvit import _lib
    return _lib.lib()


def _p(t):
    from kanvit import ops
    return t if t is None or isinstance(t, C.c_void_p) else ops._ptr(t)


def _off(t, nbytes=4):
    return C.c_void_p(t.data_ptr() + nbytes)


def _stream():
    from kanvit import ops
    return ops._stream()


def _rc_ff_fwd(M, x, w1, b1, w2, b2, y):
    return _L().kanvit_ff_small_fwd(M, D, F, *map(_p, (x, w1, b1, w2, b2, y)), _stream())


def _rc_ff_bwd(M, x, w1, b1, w2, dy, dx, dw1, db1, dw2, db2, ws, nb):
    return _L().kanvit_ff_small_bwd(M, D, F, *map(_p, (x, w1, b1, w2, dy, dx, dw1, db1, dw2, db2, ws)), C.c_size_t(nb), _stream())


def _rc_ln_fwd(M, eps, x, delta, gamma, beta, w1, b1, w2, b2, s, mean, rstd, y):
    return _L().kanvit_lnff_small_fwd(M, D, F, eps, *map(_p, (x, delta, gamma, beta, w1, b1, w2, b2, s, mean, rstd, y)), _stream())


def _rc_ln_bwd(M, s, mean, rstd, gamma, beta, w1, b1, w2, dy, ds_in, ds, dgamma, dbeta, dw1, db1, dw2, db2, ws, nb):
    return _L().kanvit_lnff_small_bwd(M, D, F, *map(_p, (s, mean, rstd, gamma, beta, w1, b1, w2, dy, ds_in, ds, dgamma, dbeta, dw1, db1, dw2,
                                                         db2, ws)), C.c_size_t(nb), _stream())


def _check(rc, what):
    from kanvit import _lib
    _lib.check(rc, what)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _ws_bytes(M):
    return int(_L().kanvit_ff_small_bwd_workspace(M, D, F))


def _guarded_workspace(M):
    """Exactly the bytes the library asks for, as the front of a larger NaN-filled buffer: (workspace, bytes, the elements behind)."""
    nb = _ws_bytes(M)
    assert nb % 16 == 0
    buf = _nan(nb // 4 + 4096)
    return buf[:nb // 4], nb, buf[nb // 4:]


def _param_outs():
    return {"dw1": _nan(F, D), "db1": _nan(F), "dw2": _nan(D, F), "db2": _nan(D)}


def ff_fwd(c):
    M = c["x"].shape[0]
    y = _nan(M, D)
    _check(_rc_ff_fwd(M, c["x"], c["w1"], c["b1"], c["w2"], c["b2"], y), "kanvit_ff_small_fwd")
    return y


def ff_bwd(c):
    M = c["x"].shape[0]
    o = {"dx": _nan(M, D), **_param_outs()}
    ws, nb, behind = _guarded_workspace(M)
    _check(_rc_ff_bwd(M, c["x"], c["w1"], c["b1"], c["w2"], c["dy"], o["dx"], o["dw1"], o["db1"], o["dw2"], o["db2"], ws, nb), "kanvit_ff_small_bwd")
    assert torch.isnan(behind).all(), "kanvit_ff_small_bwd wrote past the workspace it asked for"
    return o


def ln_fwd(c, eps=EPS, rows=None):
    """(s, mean, rstd, y) of kanvit_lnff_small_fwd on c's x / delta (rows = (a, b): on that row slice alone)."""
    a, b = rows or (0, c["x"].shape[0])
    x, delta = c["x"][a:b], (None if c.get("delta") is None else c["delta"][a:b])
    M = b - a
    s, mean, rstd, y = _nan(M, D), _nan(M), _nan(M), _nan(M, D)
    _check(_rc_ln_fwd(M, eps, x, delta, c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["b2"], s, mean, rstd, y), "kanvit_lnff_small_fwd")
    return s, mean, rstd, y


def ln_bwd(c, with_ds_in=True, rows=None):
    a, b = rows or (0, c["s"].shape[0])
    M = b - a
    o = {"ds": _nan(M, D), "dgamma": _nan(D), "dbeta": _nan(D), **_param_outs()}
    ws, nb, behind = _guarded_workspace(M)
    _check(_rc_ln_bwd(M, c["s"][a:b], c["mean"][a:b], c["rstd"][a:b], c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["dy"][a:b],
                      c["ds_in"][a:b] if with_ds_in else None, o["ds"], o["dgamma"], o["dbeta"], o["dw1"], o["db1"], o["dw2"], o["db2"], ws, nb),
           "kanvit_lnff_small_bwd")
    assert torch.isnan(behind).all(), "kanvit_lnff_small_bwd wrote past the workspace it asked for"
    return o


@contextlib.contextmanager
def _ff_grid(monkeypatch, k):
    """KANVIT_FF_GRID=k for the block (None: the default), checked in the configuration string the library echoes."""
    from kanvit import _lib
    if k is not None:
        monkeypatch.setenv("KANVIT_FF_GRID", str(k))
    try:
        assert f" ff_grid={k or 0} " in " " + _lib.reload_config() + " "
        yield
    finally:
        monkeypatch.delenv("KANVIT_FF_GRID", raising=False)
        assert " ff_grid=0 " in " " + _lib.reload_config() + " "


def _close(got, want, what, log=None):
    err = float((got.double() - want).abs().max())
    bound = 2e-5 * max(1.0, float(want.abs().max()))
    if log is not None:
        log.append(f"{what} {err:.2e}/{bound:.2e}")
    assert err < bound, f"{what}: max error {err:.3e}, bound {bound:.3e}"


def _colsum_close(got, want, terms_abs, what, log=None):
    """Ordered fp32 column sums: every column within 2e-6 * max(1, max_c sum_m |term|)."""
    err = float((got.double().flatten() - want.flatten()).abs().max())
    bound = 2e-6 * max(1.0, float(terms_abs.sum(0).max()))
    if log is not None:
        log.append(f"colsum {what} {err:.2e}/{bound:.2e}")
    assert err <= bound, f"{what}: max column error {err:.3e}, bound {bound:.3e}"


def _say(capsys, text):
    with capsys.disabled():
        print("\n" + text)


# ------------------------------------------------------------------------------------------------
# (A) exact: lattice inputs, bitwise against float64
# ------------------------------------------------------------------------------------------------
FF_NAMES = ("dx", "dw1", "db1", "dw2", "db2")
LN_NAMES = ("ds", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2")


@functools.lru_cache(maxsize=None)
def _exact_case(variant, M):
    """(inputs on the GPU, fp32 references, float64 intermediates) of one lattice case; the precondition is asserted here."""
    ln = variant != "ff"
    c = R.lattice_ln(M) if ln else R.lattice_ff(M)
    R.assert_lattice(c, ln, with_ds_in=variant == "ln+ds_in")
    if ln:
        r = R.lnff_backward64(c["s"], c["mean"], c["rstd"], c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["dy"],
                              c["ds_in"] if variant == "ln+ds_in" else None)
        xin = r["x"]
    else:
        r = R.ff_backward64(c["x"], c["w1"], c["b1"], c["w2"], c["dy"])
        xin = c["x"].double()
    want = {n: R.to_f32_exact(r[n]).to(DEV) for n in (LN_NAMES if ln else FF_NAMES)}
    # hidden unit ALIVE_BIAS without any mask: its gradients are those of a linear unit
    dh = c["dy"].double() @ c["w2"].double()[:, R.ALIVE_BIAS]
    alive = {"dw1": R.to_f32_exact(dh @ xin).to(DEV), "db1": R.to_f32_exact(dh.sum()).to(DEV),
             "dw2": R.to_f32_exact(c["dy"].double().t() @ r["pre"][:, R.ALIVE_BIAS]).to(DEV)}
    return {k: v.to(DEV) for k, v in c.items()}, want, alive


# (M, KANVIT_FF_GRID): one work-group walks all 25 tiles (the last has 9 rows) | uneven walk 4,4,4,4,3,3,3 | cap above the tile
# count: 25 work-groups, no walk | 258 tiles on the default 256 work-groups: two take a second tile, the last tile has 5 rows
EXACT_WALKS = [pytest.param(777, 1, id="777-grid1"), pytest.param(777, 7, id="777-grid7"), pytest.param(777, 64, id="777-grid64"),
               pytest.param(8229, None, id="8229-default")]


@pytest.mark.parametrize("M,grid", EXACT_WALKS)
@pytest.mark.parametrize("variant", ["ff", "ln", "ln+ds_in"])
def test_backward_on_lattice_data_is_exact(variant, M, grid, monkeypatch):
    c, want, alive = _exact_case(variant, M)
    tiles = (M + 31) // 32
    run = (lambda: ff_bwd(c)) if variant == "ff" else (lambda: ln_bwd(c, with_ds_in=variant == "ln+ds_in"))
    with _ff_grid(monkeypatch, grid):
        nb = _ws_bytes(M)
        if grid is None:
            assert nb == 4 * 256 * PART and tiles > 256, \
                f"the cap moved (workspace {nb} bytes for M={M}): re-choose M so that a work-group of the default grid takes a second tile"
        else:
            assert nb == 4 * min(tiles, grid) * PART
        got, again = run(), run()
    for n, w in want.items():
        assert torch.equal(got[n], w), f"{n}: {int((got[n] != w).sum())} of {w.numel()} elements differ from the float64 result"
        assert torch.equal(got[n], again[n]), f"{n}: not bitwise equal run to run"
    # the `pre > 0` rule of threshold_backward: a pre-activation of +0 (unit 5), of 0 + -0 (unit 6) and a negative one (unit 7)
    # pass nothing; unit 8 is alive in every row and gets the unmasked gradient
    for u in (R.DEAD_ZERO, R.DEAD_NEGZERO, R.DEAD_BIAS):
        assert not got["dw1"][u].any() and not got["db1"][u].any() and not got["dw2"][:, u].any(), f"hidden unit {u} must get no gradient"
    u = R.ALIVE_BIAS
    assert torch.equal(got["dw1"][u], alive["dw1"]) and torch.equal(got["db1"][u], alive["db1"]) and torch.equal(got["dw2"][:, u], alive["dw2"])


@pytest.mark.parametrize("M", [777, 32805])
def test_forward_on_lattice_data_is_exact(M):
    """M = 32805: 1026 tiles on the forward's 1024 work-groups (two take a second tile), the last tile has 5 rows."""
    c = R.lattice_ff(M)
    R.assert_lattice(c, False, forward_only=True)
    want = R.to_f32_exact(R.ff_forward64(c["x"], c["w1"], c["b1"], c["w2"], c["b2"])).to(DEV)
    c = {k: v.to(DEV) for k, v in c.items()}
    y = ff_fwd(c)
    assert torch.equal(y, want), f"{int((y != want).sum())} of {want.numel()} elements differ from the float64 result"
    assert torch.equal(y, ff_fwd(c))


# ------------------------------------------------------------------------------------------------
# (B) kanvit_lnff_small_fwd / _bwd on random data
# ------------------------------------------------------------------------------------------------
def _weights(seed):
    torch.manual_seed(seed)
    lin1, lin2 = torch.nn.Linear(D, F), torch.nn.Linear(F, D)
    return {"w1": lin1.weight, "b1": lin1.bias, "w2": lin2.weight, "b2": lin2.bias,
            "gamma": 1.0 + 0.3 * torch.randn(D), "beta": 0.2 * torch.randn(D)}


@functools.lru_cache(maxsize=None)
def _random_case(M, seed=0):
    c = {k: v.detach().to(DEV) for k, v in _weights(seed).items()}
    g = torch.Generator(device=DEV).manual_seed(M + seed)
    c["x"] = torch.randn(M, D, device=DEV, generator=g) * 1.5 + 0.3
    for k in ("delta", "dy", "ds_in"):
        c[k] = torch.randn(M, D, device=DEV, generator=g)
    return c


def _check_random_lnff(M, with_delta, with_ds_in, capsys):
    c = dict(_random_case(M))
    if not with_delta:
        c["delta"] = None
    log = []
    s, mean, rstd, y = ln_fwd(c)
    assert torch.equal(s, c["x"] + c["delta"] if with_delta else c["x"]), "s is not the fp32 x + delta"
    s64 = c["x"].double() + c["delta"].double() if with_delta else c["x"].double()
    mu64, rs64 = R.row_stats64(s64, EPS)
    _close(mean, mu64, "mean", log)
    _close(rstd, rs64, "rstd", log)
    _close(y, R.ff_forward64(R.ln_apply64(s64, mu64, rs64, c["gamma"], c["beta"])[1], *(c[k] for k in W_KEYS)), "y", log)
    del s64
    # backward on the kernel's own s / mean / rstd, the reference on the same values widened to double.  Rows with a pre-activation
    # that fp32 cannot tell from zero get dy = 0: their ReLU mask is not defined at this precision (_ff_ref.relu_kink_rows)
    kink = R.relu_kink_rows(R.ln_apply64(s, mean, rstd, c["gamma"], c["beta"])[1], c["w1"], c["b1"])
    assert int(kink.sum()) < 0.02 * M, int(kink.sum())
    log.append(f"{int(kink.sum())} rows at the ReLU kink")
    dy = c["dy"].clone()
    dy[kink] = 0.0
    c.update(s=s, mean=mean, rstd=rstd, dy=dy)
    got = ln_bwd(c, with_ds_in)
    r = R.lnff_backward64(s, mean, rstd, c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["dy"], c["ds_in"] if with_ds_in else None)
    _close(got["ds"], r["ds"], "ds", log)
    for n in LN_NAMES[1:]:
        e = rel_err(got[n], r[n])
        log.append(f"rel {n} {e:.2e}")
        assert e < 1e-4, (n, e)
    _colsum_close(got["dgamma"], r["dgamma"], (r["v"] * r["xh"]).abs(), "dgamma", log)
    _colsum_close(got["dbeta"], r["dbeta"], r["v"].abs(), "dbeta", log)
    _colsum_close(got["db1"], r["db1"], r["dhm"].abs(), "db1", log)
    _colsum_close(got["db2"], r["db2"], c["dy"].double().abs(), "db2", log)
    _say(capsys, f"lnff M={M} delta={with_delta} ds_in={with_ds_in} (error/bound): " + ", ".join(log))


@pytest.mark.parametrize("with_delta", [True, False])
@pytest.mark.parametrize("M", [32805, 65536])
def test_lnff_forward_and_backward_walk(M, with_delta, capsys):
    """32805 rows: 1026 tiles, two forward work-groups take a second one and the last tile has 5 rows.  65536 rows =
    kanvit_ff_small_max_rows(): every forward work-group takes exactly two tiles, every backward work-group eight."""
    assert M <= int(_L().kanvit_ff_small_max_rows()) == 65536 and (M + 31) // 32 > 1024
    assert _ws_bytes(M) == 4 * 256 * PART, "the cap moved: re-choose M"
    _check_random_lnff(M, with_delta, True, capsys)


def test_lnff_backward_walk_without_ds_in(capsys):
    assert _ws_bytes(8229) == 4 * 256 * PART, "the cap moved: re-choose M"
    _check_random_lnff(8229, True, False, capsys)


def test_forward_rows_do_not_depend_on_the_walk():
    """Rows of a walked launch (1026 tiles on 1024 work-groups) against the same rows from launches of their own: the first tile,
    three tiles in the middle, the last two tiles (the second-step tiles of work-groups 0 and 1) with the partial one."""
    M = 32805
    c = _random_case(M)
    full = ln_fwd(c)
    for a, b in ((0, 32), (16000, 16096), (32768, M)):
        part = ln_fwd(c, rows=(a, b))
        for name, f, p in zip(("s", "mean", "rstd", "y"), full, part):
            assert torch.equal(f[a:b], p), f"{name} of rows [{a}, {b}) depends on the launch they are computed in"


def test_backward_rows_do_not_depend_on_the_walk(monkeypatch):
    M = 777
    c = dict(_random_case(M))
    c["s"], c["mean"], c["rstd"], _ = ln_fwd(c)
    with _ff_grid(monkeypatch, 7):
        assert _ws_bytes(M) == 4 * 7 * PART
        full = ln_bwd(c)["ds"]
        for a, b in ((0, 32), (320, 416), (736, M)):
            assert torch.equal(full[a:b], ln_bwd(c, rows=(a, b))["ds"]), f"ds of rows [{a}, {b}) depends on the launch they are computed in"


# ---- LayerNorm edges at M = 37, through dense.ln_feed_forward and the C ABI ----
ME = 37


def _mods(eps=EPS, seed=0):
    torch.manual_seed(seed)
    norm, lin1, lin2 = torch.nn.LayerNorm(D, eps=eps), torch.nn.Linear(D, F), torch.nn.Linear(F, D)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(D) * 0.5 + 1.0)
        norm.bias.copy_(torch.randn(D) * 0.3)
    return norm.to(DEV), lin1.to(DEV), lin2.to(DEV)


def _abi_case(x, mods):
    norm, lin1, lin2 = mods
    return {"x": x, "delta": None, "gamma": norm.weight.detach(), "beta": norm.bias.detach(), "w1": lin1.weight.detach(),
            "b1": lin1.bias.detach(), "w2": lin2.weight.detach(), "b2": lin2.bias.detach()}


def _run_module(x, mods, ws, wy):
    """[s, y, ds, dgamma, dbeta] of loss = sum(s * ws) + sum(y * wy) through dense.ln_feed_forward."""
    from kanvit import dense
    norm, lin1, lin2 = mods
    for m in mods:
        m.zero_grad()
    xg = x.detach().clone().requires_grad_(True)
    s, y = dense.ln_feed_forward(xg, None, norm, lin1, lin2)
    ((s * ws).sum() + (y * wy).sum()).backward()
    return [s.detach(), y.detach(), xg.grad, norm.weight.grad.clone(), norm.bias.grad.clone()]


def _fp64_module(x, mods, ws, wy):
    norm, lin1, lin2 = mods
    x64 = x.detach().double().requires_grad_(True)
    g, b = norm.weight.detach().double().requires_grad_(True), norm.bias.detach().double().requires_grad_(True)
    h = torch.nn.functional.layer_norm(x64, (D,), g, b, norm.eps)
    y = torch.relu(h @ lin1.weight.detach().double().t() + lin1.bias.detach().double()) @ lin2.weight.detach().double().t() + lin2.bias.detach().double()
    ((x64 * ws.double()).sum() + (y * wy.double()).sum()).backward()
    return [x64.detach(), y.detach(), x64.grad, g.grad, b.grad, h.detach()]


def _fused_route_is_on(x, mods):
    from kanvit import _lib, dense
    return not _lib.py_switches()["no_lnff"] and dense._ff_small_ok(x.reshape(-1, D), mods[1], mods[2])


def test_constant_rows():
    """Every row is one repeated value c (row 0: zero): the variance is 0, rstd = 1 / sqrt(eps), LN(s) = beta and y = FF(beta).
    Bounds of tests/test_ln_row_walk_gpu.py's test_constant_rows.  With rstd = 316 an error of the mean of a few ulp of c is
    1e-4 .. 5e-4 of the LayerNorm output, far outside the feed-forward's 2e-5: the row sums have to be exact here (pairwise)."""
    mods = _mods(seed=1)
    torch.manual_seed(D)
    c = torch.randn(ME, 1, device=DEV) * 2.0
    c[0] = 0.0
    x = c.expand(ME, D).contiguous()
    cmax, rs = float(c.abs().max()), 1.0 / math.sqrt(EPS)
    case = _abi_case(x, mods)
    s, mean, rstd, y = ln_fwd(case)
    assert torch.equal(s, x)
    assert float((mean.double() - c[:, 0].double()).abs().max()) <= 4 * U * cmax
    assert float((rstd.double() - rs).abs().max()) <= (3.5 * U + 8 * U * U * cmax * cmax / EPS) * rs
    y_beta = R.ff_forward64(case["beta"][None, :], *(case[k] for k in W_KEYS)).expand(ME, D)
    _close(y, y_beta, "y against FF(beta)")
    assert _fused_route_is_on(x, mods)
    ws, wy = torch.randn(ME, D, device=DEV), torch.randn(ME, D, device=DEV)
    got, want = _run_module(x, mods, ws, wy), _fp64_module(x, mods, ws, wy)
    _close(got[1], y_beta, "module y against FF(beta)")
    assert torch.isfinite(got[2]).all()
    _close(got[2], want[2], "ds")
    _close(got[4], want[4], "dbeta")


@pytest.mark.parametrize("eps", [1e-3, 1e-6])
def test_non_default_eps(eps):
    """Row spread 1e-2 (variance 1e-4): eps = 1e-3 dominates the variance, 1e-6 is 1 % of it; a kernel that ignored the argument
    (1e-5) is off by a factor 3 in rstd at the first and by 4 % at the second.  Through the module the eps is norm.eps."""
    mods = _mods(eps=eps, seed=2)
    torch.manual_seed(3)
    x = torch.randn(ME, D, device=DEV) * 1e-2 + 0.05 * torch.randn(ME, 1, device=DEV)
    ws, wy = torch.randn(ME, D, device=DEV), torch.randn(ME, D, device=DEV)
    assert _fused_route_is_on(x, mods)
    got, want = _run_module(x, mods, ws, wy), _fp64_module(x, mods, ws, wy)
    for n, g, w in zip(("s", "y", "ds", "dgamma", "dbeta"), got, want):
        _close(g, w, n)
    _, mean, rstd, y = ln_fwd(_abi_case(x, mods), eps=eps)
    mu64, rs64 = R.row_stats64(x, eps)
    _close(rstd, rs64, "rstd")
    _close(mean, mu64, "mean")
    _close(y, want[1], "y")
    assert float((rs64 - R.row_stats64(x, EPS)[1]).abs().max()) > 100 * 2e-5 * float(rs64.max())      # the default eps would not pass


def test_large_mean_two_pass_variance_does_not_cancel(capsys, monkeypatch):
    """s = 100 + randn: mean^2 is 1e4 times the variance.  No fixed tolerance: the fp32 floor of this input is set by the rounding
    of the mean, so mean, rstd and the LayerNorm output are held to 4x the error of torch's own fp32 native_layer_norm against the
    float64 reference, y and ds to 4x the error of the unfused fp32 route (KANVIT_NO_LNFF=1: add_layernorm + feed_forward) -- the
    argument and the factor of tests/test_ln_row_walk_gpu.py.  The fused kernel does not write its LayerNorm output; it is
    rebuilt as the backward kernel rebuilds it, (s - mean) * rstd * gamma + beta in fp32 from the stored statistics."""
    from kanvit import _lib
    mods = _mods(seed=4)
    torch.manual_seed(5)
    x = 100.0 + torch.randn(ME, D, device=DEV)
    ws, wy = torch.randn(ME, D, device=DEV), torch.randn(ME, D, device=DEV)
    want = _fp64_module(x, mods, ws, wy)
    mu64, rs64 = R.row_stats64(x, EPS)
    err = lambda a, b: float((a.double() - b).abs().max())
    gamma, beta = mods[0].weight.detach(), mods[0].bias.detach()
    _, mean, rstd, _ = ln_fwd(_abi_case(x, mods))
    h_k = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    h_t, mean_t, rstd_t = torch.native_layer_norm(x, (D,), gamma, beta, EPS)
    assert _fused_route_is_on(x, mods)
    got = _run_module(x, mods, ws, wy)
    monkeypatch.setenv("KANVIT_NO_LNFF", "1")
    try:
        assert "py_no_lnff=1" in _lib.reload_config()
        plain = _run_module(x, mods, ws, wy)
    finally:
        monkeypatch.delenv("KANVIT_NO_LNFF")
        assert "py_no_lnff=0" in _lib.reload_config()
    pairs = {"mean": (err(mean, mu64), err(mean_t.flatten(), mu64)), "rstd": (err(rstd, rs64), err(rstd_t.flatten(), rs64)),
             "ln": (err(h_k, want[5]), err(h_t, want[5])), "y": (err(got[1], want[1]), err(plain[1], want[1])),
             "ds": (err(got[2], want[2]), err(plain[2], want[2]))}
    _say(capsys, "large mean (s = 100 + randn, D = 64), max error against float64, fused kernel | fp32 yardstick (torch native_layer_norm "
                 "for mean, rstd, ln; the unfused route for y, ds): " + ", ".join(f"{k} {a:.3e} | {b:.3e}" for k, (a, b) in pairs.items()))
    for k, (a, b) in pairs.items():
        assert a <= 4 * b, (k, a, b)


def test_gamma_with_zero_and_negative_entries():
    mods = _mods(seed=6)
    with torch.no_grad():
        mods[0].weight[:6] = torch.tensor([0.0, -1.5, 2.0, -0.5, 0.0, -0.0], device=DEV)
    torch.manual_seed(7)
    x = torch.randn(ME, D, device=DEV) * 2.0 + 0.7
    ws, wy = torch.randn(ME, D, device=DEV), torch.randn(ME, D, device=DEV)
    assert _fused_route_is_on(x, mods)
    got, want = _run_module(x, mods, ws, wy), _fp64_module(x, mods, ws, wy)
    for n, g, w in zip(("s", "y", "ds"), got, want):
        _close(g, w, n)
    for n, g, w in zip(("dgamma", "dbeta"), got[3:], want[3:]):
        assert rel_err(g, w) < 1e-4, (n, rel_err(g, w))
    _, _, _, y = ln_fwd(_abi_case(x, mods))
    _close(y, want[1], "y")


def test_block_under_another_grid_matches_the_default_one(monkeypatch):
    """TransformerBlock on (8, 50, 64): 400 rows = 13 tiles, under KANVIT_FF_GRID=3 a walk of 5, 4, 4 tiles.  Rows do not depend
    on the walk (bitwise output and input gradient); the parameter gradients are sums in another order."""
    from kanvit import ops
    from model import TransformerBlock
    torch.manual_seed(1)
    blk = TransformerBlock(64, 2, feedforward_dim=256, attn_type="cheby").to(DEV)
    x = torch.randn(8, 50, 64, device=DEV)

    def run():
        blk.zero_grad()
        xg = x.clone().requires_grad_(True)
        ops.timer = ops.KernelTimer()
        try:
            y = blk(xg)
            y.square().sum().backward()
            tags = set(ops.timer.records)
        finally:
            ops.timer = None
        assert "ff_small_fwd" in tags and "ff_small_bwd" in tags
        return y.detach(), xg.grad, [p.grad.clone() for p in blk.parameters()]

    y0, gx0, gp0 = run()
    with _ff_grid(monkeypatch, 3):
        assert _ws_bytes(400) == 4 * 3 * PART
        y1, gx1, gp1 = run()
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    for (name, _), a, b in zip(blk.named_parameters(), gp0, gp1):
        assert rel_err(b, a) < 2e-5, (name, rel_err(b, a))


# ---- refusals: no launch ----
def _refusal_args():
    c = dict(_random_case(ME + 3))           # 40 rows of inputs; the calls use the first 37 (room for the + 4 byte pointers)
    c["s"], c["mean"], c["rstd"], c["y"] = ln_fwd(c)
    o = {"dx": _nan(ME + 3, D), "dgamma": _nan(D), "dbeta": _nan(D), **_param_outs()}
    ws, nb, _ = _guarded_workspace(ME)
    return c, o, ws, nb


def _refused(rc, code, text):
    msg = _L().kanvit_last_error() or b""
    assert rc == code and text.encode() in msg, (rc, msg)


def test_misaligned_pointers_are_refused():
    c, o, ws, nb = _refusal_args()
    al = "16-byte aligned"
    ff_b = lambda **k: _rc_ff_bwd(ME, k.get("x", c["x"]), c["w1"], c["b1"], c["w2"], k.get("dy", c["dy"]), o["dx"], o["dw1"], o["db1"], o["dw2"],
                                  o["db2"], k.get("ws", ws), nb)
    ln_b = lambda **k: _rc_ln_bwd(ME, k.get("s", c["s"]), c["mean"], c["rstd"], c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], k.get("dy", c["dy"]),
                                  k.get("ds_in", c["ds_in"]), o["dx"], o["dgamma"], o["dbeta"], o["dw1"], o["db1"], o["dw2"], o["db2"], k.get("ws", ws), nb)
    ln_f = lambda **k: _rc_ln_fwd(ME, EPS, k.get("x", c["x"]), c["delta"], c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["b2"],
                                  k.get("s", c["s"]), c["mean"], c["rstd"], c["y"])
    _refused(_rc_ff_fwd(ME, _off(c["x"]), c["w1"], c["b1"], c["w2"], c["b2"], c["y"]), EINVAL, al)
    _refused(ff_b(x=_off(c["x"])), EINVAL, al)
    _refused(ff_b(dy=_off(c["dy"])), EINVAL, al)
    _refused(ff_b(ws=_off(ws)), EINVAL, al)
    _refused(ln_f(x=_off(c["x"])), EINVAL, al)
    _refused(ln_f(s=_off(c["s"])), EINVAL, al)
    _refused(ln_b(s=_off(c["s"])), EINVAL, al)
    _refused(ln_b(dy=_off(c["dy"])), EINVAL, al)
    _refused(ln_b(ds_in=_off(c["ds_in"])), EINVAL, al)
    _refused(ln_b(ws=_off(ws)), EINVAL, al)
    torch.cuda.synchronize()
    for k, t in o.items():
        assert torch.isnan(t).all(), f"{k} was written by a refused call"
    assert ff_b() == 0 and ln_b() == 0                      # the same arguments, aligned, are accepted
    torch.cuda.synchronize()


def test_short_or_missing_workspace_is_refused():
    c, o, ws, nb = _refusal_args()
    for w, n in ((ws, nb - 1), (None, nb), (None, 0)):
        _refused(_rc_ff_bwd(ME, c["x"], c["w1"], c["b1"], c["w2"], c["dy"], o["dx"], o["dw1"], o["db1"], o["dw2"], o["db2"], w, n), ENOMEM, "workspace")
        _refused(_rc_ln_bwd(ME, c["s"], c["mean"], c["rstd"], c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["dy"], c["ds_in"], o["dx"],
                            o["dgamma"], o["dbeta"], o["dw1"], o["db1"], o["dw2"], o["db2"], w, n), ENOMEM, "workspace")
    torch.cuda.synchronize()
    for k, t in o.items():
        assert torch.isnan(t).all(), f"{k} was written by a refused call"


def test_more_rows_than_the_path_takes_are_refused():
    """Refused on the row count alone, before any pointer is looked at (the pointers are NULL: nothing could be launched)."""
    M = int(_L().kanvit_ff_small_max_rows()) + 1
    n = [None] * 20
    _refused(_rc_ff_fwd(M, *n[:6]), EINVAL, "outside")
    _refused(_rc_ff_bwd(M, *n[:11], 0), EINVAL, "outside")
    _refused(_rc_ln_fwd(M, EPS, *n[:12]), EINVAL, "outside")
    _refused(_rc_ln_bwd(M, *n[:18], 0), EINVAL, "outside")
    assert _ws_bytes(M - 1) == 4 * 256 * PART


def test_lnff_backward_of_no_rows_zeroes_the_parameter_gradients():
    o = {"dgamma": _nan(D), "dbeta": _nan(D), **_param_outs()}
    n = [None] * 11
    assert _rc_ln_bwd(0, *n[:10], None, o["dgamma"], o["dbeta"], o["dw1"], o["db1"], o["dw2"], o["db2"], None, 0) == 0
    torch.cuda.synchronize()
    for k, t in o.items():
        assert not t.any() and torch.isfinite(t).all(), k


# ------------------------------------------------------------------------------------------------
# (C) kanvit_split3_bf16, bitwise against its definition
# ------------------------------------------------------------------------------------------------
def _rc_split3(M, K, x, bias, relu, mask, mask_ld, out, pattern):
    return _L().kanvit_split3_bf16(M, K, _p(x), _p(bias), int(relu), _p(mask), mask_ld, _p(out), pattern, _stream())


def _split3(x, pattern, bias=None, relu=False, mask=None, mask_ld=0):
    M, K = x.shape
    out = torch.full((M, 3 * K), NAN, device=DEV, dtype=torch.bfloat16)
    _check(_rc_split3(M, K, x, bias, relu, mask, mask_ld, out, pattern), "kanvit_split3_bf16")
    return out


def _split3_ref(x, pattern, bias=None, relu=False, mask=None):
    v = x if bias is None else x + bias
    if relu:
        v = torch.relu(v)
    if mask is not None:
        v = torch.where(mask.float() > 0, v, torch.zeros_like(v))
    hi = v.bfloat16()
    lo = (v - hi.float()).bfloat16()
    return torch.cat([hi, hi, lo] if pattern == 0 else [hi, lo, hi], dim=1)


def _same_bits(got, want):
    g, w = got.view(torch.int16), want.view(torch.int16)
    assert torch.equal(g, w), f"{int((g != w).sum())} of {w.numel()} bf16 elements differ"


def _scaled(g, *shape):
    """Finite, no -0.0, |value| in [1e-3, 1e3]: log-spaced column scales times [0.5, 1.5), random sign."""
    K = shape[-1]
    mag = torch.logspace(-2.6, 2.6, K, device=DEV) * (0.5 + torch.rand(*shape, device=DEV, generator=g))
    sign = torch.where(torch.rand(*shape, device=DEV, generator=g) < 0.5, -1.0, 1.0)
    v = mag * sign
    assert torch.isfinite(v).all() and float(v.abs().min()) >= 1e-3 and float(v.abs().max()) <= 1e3
    return v


@pytest.mark.parametrize("form", ["plain", "bias", "bias+relu", "mask", "bias+mask"])
@pytest.mark.parametrize("pattern", [0, 1])
def test_split3_forms_bitwise(pattern, form):
    from kanvit import dense
    M, K = 37, 64
    g = torch.Generator(device=DEV).manual_seed(10 + pattern)
    x, b, a = _scaled(g, M, K), _scaled(g, K), _scaled(g, M, K)
    bias = b if "bias" in form else None
    relu = "relu" in form
    # the mask is the hi part of a split image, as the backward pass gives it: mask_ld = 3K
    act = _split3(a, 0, bias=b, relu=True)
    _same_bits(act, _split3_ref(a, 0, bias=b, relu=True))
    mask = act[:, :K] if "mask" in form else None
    assert mask is None or (mask.stride(0) == 3 * K and 0.2 < float((mask.float() > 0).float().mean()) < 0.8)
    want = _split3_ref(x, pattern, bias, relu, mask)
    _same_bits(_split3(x, pattern, bias, relu, mask, 3 * K if mask is not None else 0), want)
    _same_bits(dense._split3(x, pattern, bias=bias, relu=relu, mask=mask), want)          # the wrapper passes the same leading dimension


def test_split3_mask_with_special_values_and_padding():
    """A bf16 mask with mask_ld = K + 8 whose padding is NaN; one row starts NaN, -0.0, +0.0, -inf, +inf, 2^-120: `mask > 0` keeps
    the last two only."""
    M, K = 37, 64
    g = torch.Generator(device=DEV).manual_seed(12)
    x, b = _scaled(g, M, K), _scaled(g, K)
    mbuf = torch.full((M, K + 8), NAN, device=DEV, dtype=torch.bfloat16)
    mbuf[:, :K] = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    mbuf[3, :6] = torch.tensor([NAN, -0.0, 0.0, -math.inf, math.inf, 2.0 ** -120], device=DEV).bfloat16()
    mask = mbuf[:, :K]
    assert float(mask[3, 5]) == 2.0 ** -120
    for pattern in (0, 1):
        got = _split3(x, pattern, bias=b, mask=mask, mask_ld=K + 8)
        _same_bits(got, _split3_ref(x, pattern, bias=b, mask=mask))
        hi = got[3, :6].float()
        assert not hi[:4].any() and hi[4] != 0 and hi[5] != 0
        assert torch.equal(got[3, 4:6], (x[3, 4:6] + b[4:6]).bfloat16())


def test_split3_grid_stride_second_step():
    """(4099, 2048): 1 049 344 threads of work on the cap of 4096 work-groups x 256 threads: the first three work-groups take a
    second step of the grid-stride loop."""
    M, K = 4099, 2048
    assert M * (K // 8) - 4096 * 256 == 3 * 256
    g = torch.Generator(device=DEV).manual_seed(13)
    x, b = _scaled(g, M, K), _scaled(g, K)
    _same_bits(_split3(x, 1, bias=b, relu=True), _split3_ref(x, 1, bias=b, relu=True))


def test_split3_refusals():
    x, out = torch.randn(8, 64, device=DEV), torch.full((8, 3 * 64 + 8), NAN, device=DEV, dtype=torch.bfloat16)
    mask = torch.ones(8, 3 * 64 + 8, device=DEV, dtype=torch.bfloat16)
    _refused(_rc_split3(8, 12, x, None, 0, None, 0, out, 0), EINVAL, "multiple of 8")
    _refused(_rc_split3(8, 64, x, None, 0, mask, 3 * 64 + 4, out, 0), EINVAL, "mask_ld a multiple of 8")
    _refused(_rc_split3(8, 64, x, None, 0, None, 0, _off(out), 0), EINVAL, "16-byte aligned")
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
