"""Float64 reference of the formula include/kanvit.h states for kanvit_layer_fwd / _bwd_input / _bwd_weight, on PACKED operands.

oracle/kan_oracle.py works on module state dicts; the C ABI works on what the modules' kan_pack() hands it:
    y[m, g*O + o] = bias[g][o] + sum_i sum_j phi_j(x[m, (g % x_group_mod)*I + i]) * w[g][i*GP + j][o]
`phi` generates the [M, I, GP] basis tensor of one group in the column order the header documents, `forward` contracts it
through ko._mm -- so ko.operand_rounding turns it into the bf16-operand reference with the rounding points
tests/test_bf16_oracle_gpu.py documents (basis values and packed weights rounded in the forward product, dY and W^T in the
input-gradient product, Phi and dY in the weight-gradient product) -- and `reference` adds the gradients the two backward entry
points return: dx / du by autograd, dw = Phi^T dY, and for SINE d loss / d freq (what the caller gets from dparam.sum(0)).

tests/test_layer_abi_ref_cpu.py pins this file to the reference-pinned oracle through every module's own packing."""
import math

import torch

from oracle import kan_oracle as ko

LINEAR, CHEBY, BSPLINE, RBF, SINE, FOURIER = range(6)                       # KANVIT_* families
BASE_SILU, BASE_GELU, BASE_GELU_TANH, BASE_RELU, BASE_TANH, BASE_IDENTITY = range(6)      # KANVIT_BASE_*


def base_activation(code, x):
    """The base column of BSPLINE / RBF: KANVIT_BASE_* applied to the layer's raw input."""
    if code == BASE_SILU:
        return x * torch.sigmoid(x)
    if code == BASE_GELU:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if code == BASE_GELU_TANH:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    if code == BASE_RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))                   # derivative 0 at x = 0
    if code == BASE_TANH:
        return torch.tanh(x)
    if code == BASE_IDENTITY:
        return x
    raise ValueError(f"unknown base activation {code}")


def phi(family, x, u, bparams, cfg):
    """[M, I, GP]: the generated columns of ONE group.  x [M, I] is the group's slice of the layer input, u [M, I] its
    spline-path input (RBF; None = x), bparams the group's 1-D basis parameters (None for the parameter-free families), cfg
    anything with the fields of kanvit_layer_desc (ops.LayerCfg)."""
    M, I = x.shape
    G = cfg.G
    if family == LINEAR:
        return x.unsqueeze(-1)
    if family == CHEBY:                              # j = degree: T_j(tanh x) by the three-term recurrence
        t = torch.tanh(x)
        cols = [torch.ones_like(t), t][:G]
        for _ in range(2, G):
            cols.append(2.0 * t * cols[-1] - cols[-2])
        return torch.stack(cols, dim=-1)
    if family == BSPLINE:                            # j = basis 0..G-1, then the base column
        nk = G + cfg.spline_order + 1
        out = ko.bspline_bases(x, bparams[:I * nk].reshape(I, nk), cfg.spline_order)
        assert out.shape[-1] == G
    elif family == RBF:                              # j = centre 0..G-1, then the base column
        us = x if u is None else u
        out = torch.exp(-(((us.unsqueeze(-1) - bparams[:G]) * cfg.rbf_inv_h) ** 2))
    elif family == SINE:                             # j = g: sin(x f_g + p_ig), bparams = freq[G] then phase[I][G]
        return torch.sin(x.unsqueeze(-1) * bparams[:G] + bparams[G:G + I * G].reshape(I, G))
    elif family == FOURIER:                          # j = c*G + (k-1): the cos block, then the sin block
        ang = x.unsqueeze(-1) * torch.arange(1, G + 1, dtype=x.dtype)
        return torch.cat([torch.cos(ang), torch.sin(ang)], dim=-1)
    else:
        raise ValueError(f"unknown family {family}")
    if cfg.has_base:
        out = torch.cat([out, base_activation(cfg.base_act, x).unsqueeze(-1)], dim=-1)
    return out


def forward(cfg, x, u, w, bparams, bias):
    """y [M, groups*O] of the header's formula.  x [M, x_group_mod*I], u [M, groups*I] or None, w [groups, I*GP, O],
    bparams [groups, stride] or None, bias [groups, O] or None; the contraction runs through ko._mm."""
    M, I = x.shape[0], cfg.I
    ys = []
    for g in range(cfg.groups):
        c = g % cfg.x_group_mod
        p = phi(cfg.family, x[:, c * I:(c + 1) * I], None if u is None else u[:, g * I:(g + 1) * I],
                None if bparams is None else bparams[g], cfg)
        assert p.shape == (M, I, cfg.GP), (tuple(p.shape), (M, I, cfg.GP))
        y = ko._mm(p.reshape(M, I * cfg.GP), w[g])
        ys.append(y if bias is None else y + bias[g])
    return torch.cat(ys, dim=1)


def reference(cfg, x, u, w, bparams, bias, dy, rounded=False):
    """{"y", "dx", "du", "dw", "dfreq"} in float64 (du only with u, dfreq only for SINE) for the loss sum(y * dy); `rounded`
    evaluates under ko.operand_rounding(ko.bf16_round).  As the ABI: RBF's dx is the base-path gradient alone when u is passed."""
    d = lambda t: None if t is None else t.detach().double()
    xd, ud, wd, bpd, bd = d(x).requires_grad_(True), d(u), d(w).requires_grad_(True), d(bparams), d(bias)
    if ud is not None:
        ud.requires_grad_(True)
    if cfg.family == SINE:
        bpd.requires_grad_(True)
    if rounded:
        with ko.operand_rounding(ko.bf16_round):
            y = forward(cfg, xd, ud, wd, bpd, bd)
            (y * d(dy)).sum().backward()
    else:
        y = forward(cfg, xd, ud, wd, bpd, bd)
        (y * d(dy)).sum().backward()
    out = {"y": y.detach(), "dx": xd.grad if xd.grad is not None else torch.zeros_like(xd), "dw": wd.grad}
    if ud is not None:
        out["du"] = ud.grad
    if cfg.family == SINE:
        out["dfreq"] = bpd.grad[:, :cfg.G]
    return out
