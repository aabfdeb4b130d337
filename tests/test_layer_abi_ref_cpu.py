"""tests/_layer_abi_ref.py (the float64 reference of the C ABI's own formula on PACKED operands) pinned to the reference-pinned
oracle (oracle/kan_oracle.py, which works on module state dicts), through every module's own kan_cfg() / kan_pack():

  * forward: _layer_abi_ref.forward on the packed operands == ko.layer_forward on the state dict, float64, 1e-12 relative;
  * gradients: the helper's dx (+ du chained through the caller's LayerNorm for FastKAN), and its packed dw / SINE d freq mapped
    back through the packing by autograd, == the oracle's input and parameter gradients.

So a packing whose column order differs from include/kanvit.h, or a `phi` whose column order does, fails here without a GPU.  (Checked
once by hand: swapping two columns in ChebyKANLayer.kan_pack, and calling the FOURIER branch of phi for SINE, both fail.)"""
import copy
import functools
from dataclasses import replace

import pytest
import torch
import torch.nn.functional as F

from oracle import kan_oracle as ko
from tests import _layer_abi_ref as ref

RTOL = 1e-12
ACT = {0: F.silu, 1: F.gelu, 2: functools.partial(F.gelu, approximate="tanh"), 3: F.relu, 4: torch.tanh, 5: lambda x: x}


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _cheby():
    from models.cheby import ChebyKANLayer
    return ChebyKANLayer(12, 10, 4)


def _kanlinear(perturbed=False, act=torch.nn.SiLU):
    from models.effkan import KANLinear
    layer = KANLinear(12, 10, base_activation=act)
    if perturbed:          # knots that are no longer g0 + j*h (still ascending), a different table per feature
        with torch.no_grad():
            nk = layer.grid.shape[1]
            layer.grid.add_(0.03 * torch.sin(torch.arange(nk, dtype=layer.grid.dtype))[None, :] * (1 + torch.arange(12, dtype=layer.grid.dtype)[:, None] % 3))
    return layer


def _fastkan(act=F.silu):
    from models.fastkan import FastKANLayer
    layer = FastKANLayer(12, 10, base_activation=act)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        layer.layernorm.weight.copy_(1.0 + 0.3 * torch.randn(layer.layernorm.weight.shape, generator=g))
        layer.layernorm.bias.copy_(0.2 * torch.randn(layer.layernorm.bias.shape, generator=g))
    return layer


def _sine():
    from models.sinekan import SineKANLayer
    return SineKANLayer(12, 10, grid_size=5)


def _fourier():
    from models.nfkan import NaiveFourierKANLayer
    return NaiveFourierKANLayer(12, 10, gridsize=6)


LAYERS = {
    "cheby": _cheby,
    "kanlinear-uniform-silu": _kanlinear,
    "kanlinear-perturbed-silu": lambda: _kanlinear(perturbed=True),
    "kanlinear-uniform-gelu": lambda: _kanlinear(act=torch.nn.GELU),
    "kanlinear-perturbed-tanh": lambda: _kanlinear(perturbed=True, act=torch.nn.Tanh),
    "fastkan-silu": _fastkan,
    "fastkan-relu": lambda: _fastkan(F.relu),
    "sine": _sine,
    "fourier": _fourier,
}


def _oracle_layer(layer64, prefix, sd, x):
    """ko.layer_forward, with the base column of a non-SiLU efficient-KAN / FastKAN layer formed by torch's own activation (the
    oracle hard-codes SiLU, the reference's default): as tests/test_base_activation_gpu.py::_ref_layer."""
    from kanvit import ops
    code = ops.base_activation_code(getattr(layer64, "base_activation", F.silu))
    if code == 0 or not getattr(layer64, "use_base_update", True):
        return ko.layer_forward(sd, prefix, x)
    g = lambda n: sd[prefix + n]
    if ko.layer_kind(sd, prefix) == "efficientkan":
        y = ko.kanlinear_forward(x, torch.zeros_like(g("base_weight")), g("spline_weight"), sd.get(prefix + "spline_scaler"), g("grid"))
        return y + ACT[code](x) @ g("base_weight").t()
    y = ko.fastkan_forward(x, g("layernorm.weight"), g("layernorm.bias"), g("rbf.grid"), g("spline_linear.weight"), None, None)
    return y + ACT[code](x) @ g("base_linear.weight").t() + g("base_linear.bias")


def _double(module):
    """A float64 copy whose parameters are fresh autograd leaves; the state dict the oracle reads shares them."""
    m = copy.deepcopy(module).double()
    sd = dict(m.named_parameters())
    sd.update(dict(m.named_buffers()))
    return m, sd


def _compare_grads(params, got, want):
    for (n, p), a, b in zip(params, got, want):
        if b is None:
            assert a is None or float(a.abs().max()) == 0.0, n
            continue
        assert a is not None and _rel(a, b) < RTOL, (n, _rel(a, b))


@pytest.mark.parametrize("name", list(LAYERS))
def test_packed_formula_equals_the_oracle_single_layer(name):
    torch.manual_seed(300 + len(name))
    layer = LAYERS[name]()
    cfg = layer.kan_cfg()
    m64, sd = _double(layer)
    M = 37
    x = (torch.randn(M, cfg.I, dtype=torch.float64) * 0.8).requires_grad_(True)
    dy = torch.randn(M, cfg.O, dtype=torch.float64)
    # the oracle on the state dict
    yo = _oracle_layer(m64, "", sd, x).reshape(M, cfg.O)
    params = [(n, p) for n, p in m64.named_parameters() if p.requires_grad]
    go = torch.autograd.grad((yo * dy).sum(), [x] + [p for _, p in params], allow_unused=True)
    # the ABI formula on the packed operands
    w, bp, bias = m64.kan_pack()
    u = m64.kan_u(x)
    y = ref.forward(cfg, x, u, w.unsqueeze(0), None if bp is None else bp.reshape(1, -1), None if bias is None else bias.reshape(1, -1))
    assert y.shape == (M, cfg.O)
    assert _rel(y, yo) < RTOL, _rel(y, yo)
    # autograd through the helper and back through the packing (and, for FastKAN, the caller's LayerNorm)
    g = torch.autograd.grad((y * dy).sum(), [x] + [p for _, p in params], allow_unused=True, retain_graph=True)
    assert _rel(g[0], go[0]) < RTOL, _rel(g[0], go[0])
    _compare_grads(params, g[1:], go[1:])
    # reference(): dx / du / dw / dfreq as the entry points return them, chained back by hand
    r = ref.reference(cfg, x, u, w.unsqueeze(0), None if bp is None else bp.reshape(1, -1), None if bias is None else bias.reshape(1, -1), dy)
    assert torch.equal(r["y"], y.detach())
    outs, gouts = [w], [r["dw"][0]]
    if cfg.family == ref.SINE:
        outs.append(bp)
        gouts.append(torch.cat([r["dfreq"][0], torch.zeros(cfg.I * cfg.G, dtype=torch.float64)]))
    if u is not None:
        outs.append(u)
        gouts.append(r["du"])
    back = torch.autograd.grad(outs, [x] + [p for _, p in params], grad_outputs=gouts, allow_unused=True)
    dx = r["dx"] + (back[0] if back[0] is not None else 0.0)
    assert _rel(dx, go[0]) < RTOL, _rel(dx, go[0])
    skip = {"base_linear.bias", "bias"}          # the bias gradient is the caller's column sum of dy, not an entry point's result
    _compare_grads([(n, p) for n, p in params if n not in skip], [b for (n, _), b in zip(params, back[1:]) if n not in skip],
                   [b for (n, _), b in zip(params, go[1:]) if n not in skip])


@pytest.mark.parametrize("kind", ["cheby", "efficientkan", "fast", "sine", "vanilla"])
def test_packed_formula_equals_the_oracle_qkv(kind):
    """The per-head q|k|v of an MSA: groups = 3*H, x_group_mod = H, group index proj*H + head, through kan_pack_grouped."""
    from attention import MSA
    from kanvit import grouped
    torch.manual_seed(17 + len(kind))
    H, dh, M = 2, 8, 29
    msa = MSA(H * dh, H, type=kind)
    layers = list(msa.q_mappings) + list(msa.k_mappings) + list(msa.v_mappings)
    cfg = replace(grouped.as_kan(layers[0]).kan_cfg(layers), groups=3 * H, x_group_mod=H)
    m64, sd = _double(msa)
    l64 = list(m64.q_mappings) + list(m64.k_mappings) + list(m64.v_mappings)
    x = (torch.randn(M, H * dh, dtype=torch.float64) * 0.8).requires_grad_(True)
    dy = torch.randn(M, 3 * H * dh, dtype=torch.float64)
    yo = torch.cat([ko.layer_forward(sd, f"{p}_mappings.{h}.", x[:, h * dh:(h + 1) * dh]).reshape(M, dh)
                    for p in ("q", "k", "v") for h in range(H)], dim=1)
    params = [(n, p) for n, p in m64.named_parameters() if p.requires_grad]
    go = torch.autograd.grad((yo * dy).sum(), [x] + [p for _, p in params], allow_unused=True)
    if kind == "vanilla":
        w = torch.stack([m.weight.t() for m in l64])
        bp, bias = None, torch.stack([m.bias for m in l64])
    else:
        w, bp, bias = type(l64[0]).kan_pack_grouped(l64)
    u = type(grouped.as_kan(l64[0])).kan_u_grouped(l64, x, H)
    y = ref.forward(cfg, x, u, w, bp, bias)
    assert _rel(y, yo) < RTOL, _rel(y, yo)
    g = torch.autograd.grad((y * dy).sum(), [x] + [p for _, p in params], allow_unused=True)
    assert _rel(g[0], go[0]) < RTOL, _rel(g[0], go[0])
    _compare_grads(params, g[1:], go[1:])


def test_operand_rounding_reaches_the_contraction():
    """Under ko.operand_rounding the helper is the bf16-operand reference: it equals the rounded oracle (same rounding points),
    and differs from the unrounded one by bf16's rounding error."""
    torch.manual_seed(5)
    layer = _cheby()
    cfg = layer.kan_cfg()
    m64, sd = _double(layer)
    x = torch.randn(33, cfg.I, dtype=torch.float64)
    dy = torch.randn(33, cfg.O, dtype=torch.float64)
    w, _, _ = m64.kan_pack()
    r = ref.reference(cfg, x, None, w.unsqueeze(0), None, None, dy, rounded=True)
    e = ref.reference(cfg, x, None, w.unsqueeze(0), None, None, dy)
    xo = x.clone().requires_grad_(True)
    with ko.operand_rounding(ko.bf16_round):
        yo = ko.layer_forward(sd, "", xo)
    (yo * dy).sum().backward()
    assert _rel(r["y"], yo.detach()) < RTOL and _rel(r["dx"], xo.grad) < RTOL
    assert 1e-4 < _rel(r["y"], e["y"]) < 2e-2 and 1e-4 < _rel(r["dw"], e["dw"]) < 2e-2


@pytest.mark.parametrize("code", range(6))
def test_base_activations_against_torch(code):
    x = torch.linspace(-4, 4, 801, dtype=torch.float64)
    assert _rel(ref.base_activation(code, x), ACT[code](x)) < 1e-14
