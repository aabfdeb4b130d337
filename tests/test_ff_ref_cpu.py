"""tests/_ff_ref.py, the reference of tests/test_ff_walk_gpu.py, checked without a GPU: its closed-form float64 backward of the
feed-forward (and of LayerNorm + feed-forward with given row statistics) against float64 torch autograd, on random and on lattice
data, and the exactness precondition of the lattice generators for every case the exact GPU tests run."""
import pytest
import torch

from tests import _ff_ref as R

D, F = R.D, R.F
NAMES_FF = ("dx", "dw1", "db1", "dw2", "db2")
NAMES_LN = ("ds", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2")


def _random_ff(M, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"x": r(M, D), "w1": r(F, D) / 8, "b1": r(F) / 8, "w2": r(D, F) / 16, "b2": r(D) / 16, "dy": r(M, D)}


def _autograd_ff(c):
    p = {k: c[k].double().requires_grad_(True) for k in ("x", "w1", "b1", "w2", "b2")}
    y = torch.relu(p["x"] @ p["w1"].t() + p["b1"]) @ p["w2"].t() + p["b2"]
    (y * c["dy"].double()).sum().backward()
    return y.detach(), {"dx": p["x"].grad, "dw1": p["w1"].grad, "db1": p["b1"].grad, "dw2": p["w2"].grad, "db2": p["b2"].grad}


def _autograd_ln(c, with_ds_in):
    """LayerNorm with GIVEN statistics as an autograd graph: the values of mean and rstd are the given ones, their derivatives
    those of the row mean and of (var + eps)^-1/2 at these values -- d mean / d s_j = 1 / D, d rstd / d s_j = -rstd^3 (s_j - mean) / D."""
    p = {k: c[k].double().requires_grad_(True) for k in ("s", "gamma", "beta", "w1", "b1", "w2", "b2")}
    s, mu0, r0 = p["s"], c["mean"].double()[:, None], c["rstd"].double()[:, None]
    lin = s - s.detach()                                             # value 0, derivative 1
    mu = mu0 + lin.mean(1, keepdim=True)
    rs = r0 - r0 ** 3 * ((s.detach() - mu0) * lin).mean(1, keepdim=True)
    x = (s - mu) * rs * p["gamma"] + p["beta"]
    y = torch.relu(x @ p["w1"].t() + p["b1"]) @ p["w2"].t() + p["b2"]
    loss = (y * c["dy"].double()).sum()
    if with_ds_in:
        loss = loss + (s * c["ds_in"].double()).sum()
    loss.backward()
    return y.detach(), {"ds": s.grad, "dgamma": p["gamma"].grad, "dbeta": p["beta"].grad, "dw1": p["w1"].grad, "db1": p["b1"].grad,
                        "dw2": p["w2"].grad, "db2": p["b2"].grad}


def _same(got, want, name, exact):
    if exact:
        assert torch.equal(got, want), name
    else:
        err = float((got - want).abs().max())
        assert err <= 1e-12 * max(1.0, float(want.abs().max())), (name, err)


@pytest.mark.parametrize("data", ["random", "lattice"])
def test_ff_closed_form_against_autograd(data):
    c = _random_ff(77, 1) if data == "random" else R.lattice_ff(777)
    y, want = _autograd_ff(c)
    got = R.ff_backward64(c["x"], c["w1"], c["b1"], c["w2"], c["dy"])
    _same(R.ff_forward64(c["x"], c["w1"], c["b1"], c["w2"], c["b2"]), y, "y", data == "lattice")
    for n in NAMES_FF:
        _same(got[n], want[n], n, data == "lattice")      # lattice data: float64 is exact too, whatever the order


@pytest.mark.parametrize("with_ds_in", [True, False])
@pytest.mark.parametrize("data", ["random", "lattice"])
def test_lnff_closed_form_against_autograd(data, with_ds_in):
    if data == "random":
        c = _random_ff(77, 2)
        g = torch.Generator().manual_seed(3)
        c["s"] = c.pop("x") * 2.0 + 0.7
        c["mean"], c["rstd"] = (t.float() for t in R.row_stats64(c["s"], 1e-5))
        c["gamma"], c["beta"] = 1.0 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
        c["ds_in"] = torch.randn(77, D, generator=g)
    else:
        c = R.lattice_ln(777)
    y, want = _autograd_ln(c, with_ds_in)
    got = R.lnff_backward64(c["s"], c["mean"], c["rstd"], c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["dy"], c["ds_in"] if with_ds_in else None)
    _same(R.ff_forward64(got["x"], c["w1"], c["b1"], c["w2"], c["b2"]), y, "y", data == "lattice")
    for n in NAMES_LN:
        _same(got[n], want[n], n, data == "lattice")


def test_lnff_closed_form_against_layer_norm_autograd():
    """With the row's own statistics the closed form is the gradient of torch's layer_norm followed by the feed-forward."""
    c = _random_ff(77, 4)
    s = (c.pop("x") * 2.0 + 0.7).double().requires_grad_(True)
    gamma, beta = (1.0 + 0.3 * torch.randn(D)).double().requires_grad_(True), (0.2 * torch.randn(D)).double().requires_grad_(True)
    p = {k: c[k].double().requires_grad_(True) for k in ("w1", "b1", "w2", "b2")}
    x = torch.nn.functional.layer_norm(s, (D,), gamma, beta, 1e-5)
    y = torch.relu(x @ p["w1"].t() + p["b1"]) @ p["w2"].t() + p["b2"]
    (y * c["dy"].double()).sum().backward()
    mean, rstd = R.row_stats64(s.detach(), 1e-5)
    got = R.lnff_backward64(s.detach(), mean, rstd, gamma.detach(), beta.detach(), c["w1"], c["b1"], c["w2"], c["dy"])
    want = {"ds": s.grad, "dgamma": gamma.grad, "dbeta": beta.grad, "dw1": p["w1"].grad, "db1": p["b1"].grad, "dw2": p["w2"].grad, "db2": p["b2"].grad}
    for n in NAMES_LN:
        err = float((got[n] - want[n]).abs().max())
        assert err <= 1e-10 * max(1.0, float(want[n].abs().max())), (n, err)


def test_relu_kink_rows_cover_every_sign_an_fp32_evaluation_gets_wrong():
    c = _random_ff(30000, 5)
    pre32 = c["x"] @ c["w1"].t() + c["b1"]
    pre64 = c["x"].double() @ c["w1"].double().t() + c["b1"].double()
    kink = R.relu_kink_rows(c["x"], c["w1"], c["b1"])
    wrong = ((pre32 > 0) != (pre64 > 0)).any(1)
    assert not (wrong & ~kink).any()
    assert 0 < int(kink.sum()) < 0.02 * 30000
    x = torch.ones(2, D)
    w1 = torch.zeros(F, D)
    w1[:, 0], w1[3, 1] = 1.0, -1.0                    # unit 3: pre = x0 - x1 = 0 in row 0
    x[1, 1] = 0.5
    assert R.relu_kink_rows(x, w1, torch.ones(F)).tolist() == [False, False]
    assert R.relu_kink_rows(x, w1, torch.zeros(F)).tolist() == [True, False]


def test_quantum():
    assert R.quantum(torch.tensor([3.0, -6.0, 0.0])) == 1.0
    assert R.quantum(torch.tensor([4.0, 12.0])) == 4.0
    assert R.quantum(torch.tensor([0.75, 2.0])) == 0.25
    assert R.quantum(torch.tensor([-0.0, 0.0])) == 1.0
    assert R.quantum(torch.tensor([2.0 ** -23 + 1.0])) == 2.0 ** -23
    assert R.quantum(torch.tensor([2.0 ** -40 + 1.0], dtype=torch.float64)) == 2.0 ** -40


# every exact case of tests/test_ff_walk_gpu.py
@pytest.mark.parametrize("M", [777, 8229])
@pytest.mark.parametrize("variant", ["ff", "ln", "ln-no-ds_in"])
def test_lattice_precondition_of_the_backward_cases(M, variant, capsys):
    ln = variant != "ff"
    c = R.lattice_ln(M) if ln else R.lattice_ff(M)
    m = R.assert_lattice(c, ln, with_ds_in=variant == "ln")
    ties, alive, dead, _ = R.relu_state(c, ln)
    with capsys.disabled():
        worst = max(m, key=m.get)
        print(f"\nlattice {variant} M={M}: worst S/q {m[worst]:.3e} ({worst}) of 2^24 = {R.EXACT_LIMIT:.3e}; ties {ties:.3f} alive {alive:.3f} dead {dead:.3f}")
    assert {"pre", "y", "dh", "dx", "dw1", "dw2", "db1", "db2"} <= set(m)
    if ln:
        assert {"t1", "t2", "ds", "dgamma", "dbeta"} <= set(m)


@pytest.mark.parametrize("M", [777, 32805])
def test_lattice_precondition_of_the_forward_cases(M):
    m = R.assert_lattice(R.lattice_ff(M), False, forward_only=True)
    assert set(m) == {"pre", "y"}


def test_precondition_refuses_inputs_that_are_not_exact():
    c = R.lattice_ff(777)
    c["x"] = c["x"] + 2.0 ** -20                      # 21 more bits below the integers: the sums no longer fit 24 bits
    with pytest.raises(AssertionError, match="lattice precondition"):
        R.assert_lattice(c, False)
    c = R.lattice_ff(777)
    c["b1"][R.ALIVE_BIAS] = 1.0                       # unit 8 no longer always alive
    with pytest.raises(AssertionError, match="lattice precondition"):
        R.assert_lattice(c, False)


def test_lattice_references_are_fp32_numbers():
    c = R.lattice_ln(777)
    r = R.lnff_backward64(c["s"], c["mean"], c["rstd"], c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["dy"], c["ds_in"])
    for n in NAMES_LN:
        R.to_f32_exact(r[n])
    with pytest.raises(AssertionError):
        R.to_f32_exact(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    pre = R.relu_state(c, True)[3]
    for u in (R.DEAD_ZERO, R.DEAD_NEGZERO, R.DEAD_BIAS):
        assert not r["dw1"][u].any() and r["db1"][u] == 0 and not r["dw2"][:, u].any()
    assert r["dw1"][R.ALIVE_BIAS].any() and (pre[:, R.ALIVE_BIAS] > 0).all()
