"""Launch helpers: one fused kernel per KAN layer, or ONE kernel for every head's q, k and v
mapping of an MSA block (3*H independent layers that share the rows of x) -- and the protocol a layer
module speaks to take part, `KanLayer`.  Every layer class of models/*.py inherits it; `as_kan` presents an
nn.Linear through it.  The packing is O(|W|) plumbing; every flop of the layer itself runs in the HIP kernel.

    kan_cfg(layers=None) -> ops.LayerCfg (groups = 1).  `layers`: the sibling layers of a grouped launch, for the families
                  whose flags depend on all of them (the efficient-KAN knot tables, the FastKAN centres); others ignore it.
    kan_pack()    -> (w[K, O], bparams[stride] | None, bias[O] | None), built with differentiable torch ops from the
                  module's reference-layout parameters, so autograd scatters the packed-weight gradient back to
                  cheby_coeffs / spline_weight / ... itself.  Row k = i*GP + j, a base column last (include/kanvit.h).
                  bparams None: the family has no basis parameters; bias None: no bias.
    kan_pack_grouped(layers)  (static) -> (w[g, K, O], bparams[g, stride] | None, bias[g, O] | None): kan_pack() of every
                  layer, stacked with a handful of launches (stack_params).  A family that is never grouped (FourierKAN:
                  patch embedding only) keeps the default, NotImplementedError.
    kan_u(x2d)    -> u[M, I], the separate input of the spline path (FastKAN: LayerNorm(x)), or None: the basis reads x.
    kan_u_grouped(layers, x2d, n_heads)  (static) -> u[M, g*I], column block g = proj*H + head, or None as above.
    kan_ln()      -> the nn.LayerNorm the kernels may form u with themselves (ops.kan_layer_ln), or None: no such LayerNorm
                  (or it is switched off: FastKANLayer.forward(time_benchmark=True)).
    kan_base_act() -> the kernels' code of the layer's base activation (ops.base_act_of), or None: no live base path.
                  One grouped launch has ONE base activation.

Adding a family: DESIGN.md section 2, "Adding a KAN family".
"""
from __future__ import annotations

from dataclasses import replace
from typing import Sequence

import torch
import torch.nn.functional as F

from . import ops


class _StackParams(torch.autograd.Function):
    """torch.stack over per-head parameters whose backward costs ONE kernel.

    Stock stack hands autograd 3*H strided slices of the packed-weight gradient; AccumulateGrad then clones each one
    (432 five-microsecond copies per ViT-B step).  Here the incoming gradient is made contiguous once and the per-parameter
    gradients are its unbound slices: contiguous, uniquely referenced, so AccumulateGrad adopts them without a copy."""

    @staticmethod
    def forward(ctx, *tensors):
        return torch.stack(tensors)

    @staticmethod
    def backward(ctx, grad):
        return grad.contiguous().unbind(0)


class _StackPermuted(torch.autograd.Function):
    """torch.stack over per-head parameters WITH a layout permutation, one kernel each way: forward stacks permuted VIEWS (torch.cat's
    strided-input path writes the packed layout directly -- stack followed by permute + reshape was a cat launch and a copy launch per
    block), backward makes the incoming gradient contiguous in the parameters' own layout once and hands out its unbound slices."""

    @staticmethod
    def forward(ctx, perm, *tensors):
        ctx.inv = tuple(sorted(range(len(perm)), key=lambda a: perm[a]))
        return torch.stack([t.permute(*perm) for t in tensors])

    @staticmethod
    def backward(ctx, grad):
        inv = (0,) + tuple(1 + a for a in ctx.inv)
        return (None,) + grad.permute(*inv).contiguous().unbind(0)


def stack_params(tensors: Sequence[torch.Tensor], perm: Sequence[int] = None) -> torch.Tensor:
    """torch.stack(tensors) -- of tensors.permute(perm) when perm is given -- whose backward costs one kernel (see above)."""
    tensors = list(tensors)
    if perm is not None:
        if any(t.requires_grad for t in tensors) and torch.is_grad_enabled():
            return _StackPermuted.apply(tuple(perm), *tensors)
        return torch.stack([t.permute(*perm) for t in tensors])
    if any(t.requires_grad for t in tensors) and torch.is_grad_enabled():
        return _StackParams.apply(*tensors)
    return torch.stack(tensors)


class KanLayer:
    """The layer-to-kernel protocol (module docstring).  A family states kan_cfg and kan_pack, kan_pack_grouped where it serves as
    per-head q|k|v mapping; the defaults below are a layer that reads x alone, has no LayerNorm to fuse and no base path."""

    def kan_cfg(self, layers=None) -> ops.LayerCfg:
        raise NotImplementedError

    def kan_pack(self):
        raise NotImplementedError

    @staticmethod
    def kan_pack_grouped(layers):
        raise NotImplementedError(f"{type(layers[0]).__name__} has no grouped packing: it is not a per-head q|k|v mapping")

    def kan_u(self, x2d):
        return None

    @staticmethod
    def kan_u_grouped(layers, x2d, n_heads):
        return None

    def kan_ln(self):
        return None

    def kan_base_act(self):
        return None


class LinearKan(KanLayer):
    """An nn.Linear (the vanilla q|k|v mapping) seen through the protocol: family LINEAR, nn.Linear keeps its weight as [O, I]."""

    def __init__(self, lin: torch.nn.Linear):
        self.lin = lin

    def kan_cfg(self, layers=None):
        return ops.LayerCfg(family=ops.LINEAR, I=self.lin.in_features, O=self.lin.out_features, G=1)

    def kan_pack(self):
        return self.lin.weight.t(), None, self.lin.bias

    @staticmethod
    def kan_pack_grouped(layers):
        w = stack_params([m.lin.weight for m in layers], perm=(1, 0))      # [g, I, O]
        return w, None, None if layers[0].lin.bias is None else stack_params([m.lin.bias for m in layers])


def as_kan(m) -> KanLayer:
    """m itself, or the adapter of an nn.Linear."""
    return LinearKan(m) if isinstance(m, torch.nn.Linear) else m


def run_single(layer, x2d: torch.Tensor) -> torch.Tensor:
    """y[M, O] for one layer on a 2-D input."""
    layer = as_kan(layer)
    cfg, (w, bp, bias) = layer.kan_cfg(), layer.kan_pack()
    ln = layer.kan_ln()
    if ln is not None and ops.ln_fusable(cfg, x2d.shape[0]):      # FastKAN: the LayerNorm of the spline path is formed inside the kernels
        return ops.kan_layer_ln(x2d, w.unsqueeze(0), cfg, torch.cat([bp, ln.weight, ln.bias]).unsqueeze(0),
                                None if bias is None else bias.reshape(1, -1), ln.eps)
    return ops.kan_layer(x2d, w.unsqueeze(0), cfg, u=layer.kan_u(x2d),
                         bparams=None if bp is None else bp.unsqueeze(0),
                         bias=None if bias is None else bias.reshape(1, -1))


def run_qkv(q_layers: Sequence, k_layers: Sequence, v_layers: Sequence, x2d: torch.Tensor) -> torch.Tensor:
    """x2d[M, H*dh] -> qkv[M, 3*H*dh]; column block g = proj*H + head holds layer g's output.

    Equivalent to the reference's per-sample, per-head loop (attention.py:188-197) because every
    layer acts row-wise."""
    return run_projections([q_layers, k_layers, v_layers], x2d)


def pack_projections(projections: Sequence[Sequence]):
    """(cfg, w, bparams, bias) of ONE grouped launch over P projections of H per-head layers each: groups = P*H, x_group_mod = H,
    group g = proj*H + head.  Pure packing (differentiable torch ops on the layers' parameters), no launch."""
    H = len(projections[0])
    assert all(len(p) == H for p in projections), "every projection has one layer per head"
    return _pack_layers([as_kan(m) for p in projections for m in p], H)


def _pack_layers(layers: Sequence[KanLayer], H: int):
    cfg = replace(layers[0].kan_cfg(layers), groups=len(layers), x_group_mod=H)
    # kan_pack_grouped packs ALL P*H layers with one stack + one layout transform (a handful of launches) instead of a
    # permute-copy per head (3*H launches forward and again backward: 880 tiny kernels per ViT-B step).
    return (cfg,) + tuple(type(layers[0]).kan_pack_grouped(layers))


def run_projections(projections: Sequence[Sequence], x2d: torch.Tensor, tag: str = None) -> torch.Tensor:
    """x2d[M, H*dh] -> y[M, P*H*dh] for P projections (lists of H per-head layers: [q, k, v], [k, v], [q], ...) in ONE grouped
    launch; column block g = proj*H + head holds layer g's output.  `tag` names the launch for the kernel timer (kanvit.ops.kan_layer);
    the q|k|v launch of run_qkv keeps the default "qkv"."""
    H = len(projections[0])
    assert all(len(p) == H for p in projections), "every projection has one layer per head"
    layers = [as_kan(m) for p in projections for m in p]
    # one grouped launch has ONE base activation (kanvit_layer_desc.base_act): layers whose activations differ (swapped after
    # construction) run one launch each, on their own head's columns
    if len({m.kan_base_act() for m in layers} - {None}) > 1:
        dh = x2d.shape[1] // H
        return torch.cat([run_single(m, x2d[:, (g % H) * dh:(g % H + 1) * dh]) for g, m in enumerate(layers)], dim=1)
    cfg, w, bp, bias = _pack_layers(layers, H)
    lns = [m.kan_ln() for m in layers]
    if lns[0] is not None and ops.ln_fusable(cfg, x2d.shape[0]):
        gamma = stack_params([ln.weight for ln in lns])
        beta = stack_params([ln.bias for ln in lns])
        return ops.kan_layer_ln(x2d, w, cfg, torch.cat([bp, gamma, beta], dim=1), bias, lns[0].eps, tag=tag)
    u = type(layers[0]).kan_u_grouped(layers, x2d, H)
    return ops.kan_layer(x2d, w, cfg, u=u, bparams=bp, bias=bias, tag=tag)
