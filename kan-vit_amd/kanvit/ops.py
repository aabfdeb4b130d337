"""torch.autograd wrappers around the kanvit C ABI (include/kanvit.h).

PyTorch is plumbing here: it owns device memory, the current HIP stream and the autograd tape.
All arithmetic of the hot path (basis evaluation, contractions, attention) runs in the HIP
kernels of libkanvit.so.  There is no fallback: CPU tensors or a missing library raise.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import BSPLINE, CHEBY, FOURIER, LINEAR, RBF, SINE, AttnDesc, KanvitError, LayerDesc, check  # noqa: F401


@dataclass(frozen=True)
class LayerCfg:
    """Static description of one (grouped) fused KAN layer launch; mirrors kanvit_layer_desc."""
    family: int
    I: int
    O: int
    G: int
    groups: int = 1
    x_group_mod: int = 1
    spline_order: int = 0
    has_base: int = 0
    rbf_inv_h: float = 0.0
    flags: int = 0          # _lib.FLAG_BF16_MFMA: contract on the bf16 matrix cores (set under bf16 autocast)
    ln_eps: float = 0.0     # _lib.FLAG_FUSED_LN (FastKAN): epsilon of the LayerNorm formed inside the kernels
    base_act: int = 0       # BSPLINE / RBF with has_base: activation of the base column (_lib.BASE_*; 0 = SiLU)

    @property
    def GP(self) -> int:
        return {LINEAR: 1, CHEBY: self.G, BSPLINE: self.G + self.has_base, RBF: self.G + self.has_base,
                SINE: self.G, FOURIER: 2 * self.G}[self.family]

    @property
    def K(self) -> int:
        return self.I * self.GP


class KernelTimer:
    """Optional in-stream timing of the C-ABI launches (bench.py's roofline leg): a pair of events
    recorded on the launch stream brackets each call, so the measured interval is that launch's
    kernels only.  Disabled (None) by default; costs nothing then."""

    def __init__(self):
        self.records = {}          # tag -> list of (start, end, flops, bytes)

    def add(self, tag, start, end, flops, nbytes):
        self.records.setdefault(tag, []).append((start, end, flops, nbytes))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for tag, recs in self.records.items():
            ms = [s.elapsed_time(e) for s, e, _, _ in recs]
            out[tag] = {"launches": len(recs), "total_ms": sum(ms), "avg_ms": sum(ms) / len(ms),
                        "flops": recs[0][2], "bytes": recs[0][3]}
        return out


timer: Optional[KernelTimer] = None


class _timed:
    def __init__(self, tag, flops=0, nbytes=0):
        self.tag, self.flops, self.nbytes = tag, flops, nbytes

    def __enter__(self):
        if timer is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if timer is not None:
            self.e.record()
            timer.add(self.tag, self.s, self.e, self.flops, self.nbytes)
        return False


def _layer_cost(cfg: "LayerCfg", M: int, kind: str):
    """Algorithmic flops / HBM bytes of one launch (SURVEY.md section 8d formulas, fp32)."""
    flops = 2 * M * cfg.K * cfg.O * cfg.groups
    xb, yb, wb = M * cfg.x_group_mod * cfg.I, M * cfg.groups * cfg.O, cfg.groups * cfg.K * cfg.O
    nbytes = 4 * {"fwd": xb + yb + wb, "bwd_input": 2 * xb + yb + wb, "bwd_weight": xb + yb + wb}[kind]
    return flops, nbytes


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_gpu_f32(name: str, t: Optional[torch.Tensor]):
    if t is None:
        return
    if not t.is_cuda:
        raise KanvitError(f"{name} is on {t.device}: the kanvit ops run only on an AMD GPU (no CPU fallback)")
    if t.dtype != torch.float32:
        raise KanvitError(f"{name} has dtype {t.dtype}; the kanvit kernels compute in float32")


SUPPORTED_BASE_ACTIVATIONS = ("nn.SiLU(), F.silu; nn.GELU(), F.gelu; nn.GELU(approximate='tanh'), "
                              "functools.partial(F.gelu, approximate='tanh'); nn.ReLU(), F.relu, torch.relu; "
                              "nn.Tanh(), torch.tanh, F.tanh; nn.Identity()")


def base_activation_code(fn) -> Optional[int]:
    """The kernels' code (_lib.BASE_*) for a base activation of KANLinear / FastKANLayer -- a module instance or a callable,
    as the reference applies it (models/effkan.py:178, models/fastkan.py:74) -- or None when the kernels do not implement
    it.  In-place variants are refused: the reference evaluates the B-splines of the already-activated x after them."""
    import functools
    import torch.nn.functional as F
    nn = torch.nn
    if isinstance(fn, functools.partial):
        if fn.args or not (fn.func is F.gelu or fn.func is torch._C._nn.gelu):
            return None
        if set(fn.keywords) - {"approximate"}:
            return None
        a = fn.keywords.get("approximate", "none")
        return {"none": _lib.BASE_GELU, "tanh": _lib.BASE_GELU_TANH}.get(a)
    if isinstance(fn, nn.Module):
        t = type(fn)
        if t is nn.SiLU:
            return None if fn.inplace else _lib.BASE_SILU
        if t is nn.GELU:
            return {"none": _lib.BASE_GELU, "tanh": _lib.BASE_GELU_TANH}.get(fn.approximate)
        if t is nn.ReLU:
            return None if fn.inplace else _lib.BASE_RELU
        if t is nn.Tanh:
            return _lib.BASE_TANH
        if t is nn.Identity:
            return _lib.BASE_IDENTITY
        return None
    if fn is F.silu:
        return _lib.BASE_SILU
    if fn is F.gelu or fn is torch._C._nn.gelu:
        return _lib.BASE_GELU
    if fn is F.relu or fn is torch.relu:
        return _lib.BASE_RELU
    if fn is torch.tanh or fn is F.tanh:
        return _lib.BASE_TANH
    return None


def base_act_of(fn) -> int:
    """base_activation_code(fn), or NotImplementedError naming the supported set."""
    code = base_activation_code(fn)
    if code is None:
        raise NotImplementedError(f"base_activation {fn!r} is not implemented by the fused kernels; supported: "
                                  f"{SUPPORTED_BASE_ACTIVATIONS}")
    return code


def _desc(cfg: LayerCfg, M: int, ldx: int, ldu: int, ldy: int, bp_stride: int) -> LayerDesc:
    return LayerDesc(cfg.family, cfg.groups, cfg.x_group_mod, cfg.I, cfg.O, cfg.G, cfg.spline_order, cfg.has_base,
                     cfg.rbf_inv_h, cfg.flags, M, ldx, ldu, ldy, bp_stride, cfg.ln_eps, cfg.base_act)


def _workspace(nbytes: int, device):
    """Caller-owned scratch for a C-ABI call (16-byte aligned by the torch allocator)."""
    return torch.empty(max((nbytes + 3) // 4, 4), device=device, dtype=torch.float32)


_NO_SCRATCH = (lambda: 0,)      # a workspace "query" that answers 0 without asking the library (the fp32 patch forward)


def _launch(fn, label, device, *args, query=None, null_ws=False, tag=None, cost=(0, 0)):
    """One C-ABI launch on `device` and its current stream: fn(*args, [workspace, bytes,] stream), checked under `label`.

    query = (workspace function, *its arguments): the entry point takes scratch -- the bytes are queried, allocated through
    _workspace and passed as `workspace, c_size_t(bytes)` in front of the stream; null_ws passes NULL when the query answers 0
    (entry points that refuse NULL always get an allocation).  tag: bracket the call with the kernel timer under that name and
    `cost` = (flops, bytes); a callable tag is given the queried bytes.  No host synchronisation; HIP-graph capturable."""
    with torch.cuda.device(device):
        if query is None:
            tail = (_stream(),)
        else:
            nbytes = int(query[0](*query[1:]))
            ws = None if null_ws and not nbytes else _workspace(nbytes, device)
            tail = (_ptr(ws), C.c_size_t(nbytes), _stream())
        if tag is None or timer is None:
            check(fn(*args, *tail), label)
        else:
            with _timed(tag(nbytes) if callable(tag) else tag, *cost):
                check(fn(*args, *tail), label)


_fwd_f32 = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_bwd = torch.amp.custom_bwd(device_type="cuda")
# Under torch.autocast (bench.py --amp bf16: the stock FF GEMMs run on the bf16 matrix cores) the kanvit ops
# keep computing in fp32: inputs are cast to fp32 at the boundary and autocast is off inside.


def _bf16_tag(tag: str, flags: int) -> str:
    return tag + "_bf16" if flags & _lib.FLAG_BF16_MFMA else tag


def _kan_forward(cfg: LayerCfg, x, u, w, bparams, bias, tag, fused_ln=False):
    """The kanvit_layer_fwd launch of _KanLayerFn and _KanLayerLnFn: (y, x, u, w, bparams, bias), the operands as the kernel read
    them (contiguous).  fused_ln: bparams is [centres | gamma | beta] and the u slot carries the [M, x_group_mod, 2] statistics
    the kernel writes, returned as u."""
    for n, t in (("x", x), ("u", u), ("w", w), ("bparams", bparams), ("bias", bias)):
        _require_gpu_f32(n, t)
    x, u, w, bparams, bias = (None if t is None else t.contiguous() for t in (x, u, w, bparams, bias))
    M, ldx = x.shape
    if ldx != cfg.x_group_mod * cfg.I:
        raise KanvitError(f"x has {ldx} columns, expected x_group_mod*I = {cfg.x_group_mod * cfg.I}")
    if tuple(w.shape) != (cfg.groups, cfg.K, cfg.O):
        raise KanvitError(f"packed weight shape {tuple(w.shape)} != {(cfg.groups, cfg.K, cfg.O)}")
    if fused_ln:
        if tuple(bparams.shape) != (cfg.groups, cfg.G + 2 * cfg.I):
            raise KanvitError(f"bparams shape {tuple(bparams.shape)} != {(cfg.groups, cfg.G + 2 * cfg.I)} (centres | gamma | beta)")
        u = torch.empty(M, cfg.x_group_mod, 2, device=x.device, dtype=torch.float32)
    elif u is not None and tuple(u.shape) != (M, cfg.groups * cfg.I):
        raise KanvitError(f"u shape {tuple(u.shape)} != {(M, cfg.groups * cfg.I)}")
    y = torch.empty(M, cfg.groups * cfg.O, device=x.device, dtype=torch.float32)
    d = _desc(cfg, M, ldx, cfg.groups * cfg.I, cfg.groups * cfg.O, 0 if bparams is None else bparams.shape[1])
    L = _lib.lib()
    _launch(L.kanvit_layer_fwd, "kanvit_layer_fwd", x.device, C.byref(d), _ptr(x), _ptr(u), _ptr(w), _ptr(bparams), _ptr(bias), _ptr(y),
            query=(L.kanvit_layer_fwd_workspace, C.byref(d)), null_ws=True,
            tag=_bf16_tag(_tag_prefix(cfg, tag) + "_fwd", cfg.flags), cost=_layer_cost(cfg, M, "fwd"))
    return y, x, u, w, bparams, bias


class _KanLayerFn(torch.autograd.Function):
    """y[M, groups*O] = fused_kan(x[M, x_group_mod*I], u, w[groups, K, O], bparams, bias)."""

    @staticmethod
    @_fwd_f32
    def forward(ctx, x, u, w, bparams, bias, cfg: LayerCfg, tag: Optional[str] = None):
        y, x, u, w, bparams, bias = _kan_forward(cfg, x, u, w, bparams, bias, tag)
        ctx.tag = tag
        ctx.cfg = cfg
        ctx.has_u = u is not None
        ctx.has_bp = bparams is not None
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, u, w, bparams)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, dy):
        x, u, w, bparams = ctx.saved_tensors
        return _kan_backward(ctx.cfg, x, u if ctx.has_u else None, w, bparams, dy.float().contiguous(), ctx.needs_input_grad[:5],
                             ctx.has_u, ctx.has_bias, tag=ctx.tag) + (None, None)


def _tag_prefix(cfg: "LayerCfg", tag: Optional[str]) -> str:
    """The timer tag stem of a KAN launch: "qkv" for a grouped launch and "layer" for a single layer, unless the caller names
    its launch (bench.py takes a tag's flops and bytes from its first launch: launches of another shape need their own tag)."""
    return tag or ("qkv" if cfg.groups > 1 else "layer")


def _kan_backward(cfg: "LayerCfg", x, u, w, bparams, dy, needs, has_u, has_bias, patch=None, tag=None):
    """Gradients of one fused KAN launch w.r.t. (x, u, w, bparams, bias): the C-ABI input-gradient and weight-gradient calls.

    patch = (PatchDesc, M): x is the NCHW image batch and dy the token-sequence gradient [B, P + pre, O]; the weight-gradient
    kernels gather both (kanvit_patch_embed_bwd_weight: no patch matrix, no dY copy).  Only weight-side gradients then."""
    if patch is not None:
        pd, M = patch
        ldx = cfg.I
        assert not (needs[0] or needs[1]), "the patch form has no input gradient"
    else:
        pd = None
        M, ldx = x.shape
    need_x, need_u, need_w, need_bp, need_b = needs
    stem = _tag_prefix(cfg, tag)
    d = _desc(cfg, M, ldx, cfg.groups * cfg.I, cfg.groups * cfg.O, 0 if bparams is None else bparams.shape[1])
    L = _lib.lib()

    def weight_pass(desc, out, what):
        tag, cost = _bf16_tag(stem + what, cfg.flags), _layer_cost(cfg, M, "bwd_weight")
        if pd is not None:
            _launch(L.kanvit_patch_embed_bwd_weight, "kanvit_patch_embed_bwd_weight", x.device, C.byref(desc), C.byref(pd), _ptr(x),
                    _ptr(bparams), _ptr(dy), _ptr(out), query=(L.kanvit_patch_embed_bwd_weight_workspace, C.byref(desc), C.byref(pd)),
                    tag=tag, cost=cost)
        else:
            _launch(L.kanvit_layer_bwd_weight, "kanvit_layer_bwd_weight", x.device, C.byref(desc), _ptr(x), _ptr(u), _ptr(bparams),
                    _ptr(dy), _ptr(out), query=(L.kanvit_layer_bwd_weight_workspace, C.byref(desc)), tag=tag, cost=cost)

    dx = du = dw = dbp = db = None
    sine_freq = cfg.family == SINE and need_bp
    # SineKAN's trainable freq (models/sinekan.py:60): d loss / d freq_g = sum_{m,i} x cos(x f_g + p_ig) dPhi[m,i,g] falls out of the
    # input-gradient kernel.  When nobody needs the input gradient itself (the patch embedding: x is the image), the same sum is
    # sum_{i,o} w[(i,g),o] Q[(i,g),o] with Q = a weight-gradient pass over the operand x cos(.) (KANVIT_FLAG_SINE_DFREQ) -- the faster
    # of the two contractions at G = 28 (8.6 instead of 13.9 ms at ViT-B).
    freq_via_w = False
    if sine_freq and not need_x and (pd is not None or not _lib.py_switches()["no_dfreq_w"]):
        with torch.cuda.device(x.device):
            freq_via_w = bool(L.kanvit_layer_sine_dfreq_ok(C.byref(d)))
    if pd is not None and sine_freq and not freq_via_w:
        raise KanvitError("patch form: SineKAN's frequency gradient needs the register weight-gradient kernel")
    with torch.cuda.device(x.device):
        if need_x or (need_u and has_u) or (sine_freq and not freq_via_w):
            dx = torch.empty_like(x)
            du_buf = torch.empty(M, cfg.groups * cfg.I, device=x.device, dtype=torch.float32) if cfg.family == RBF else None
            dpart = None
            if cfg.family == SINE:
                tiles = int(L.kanvit_layer_dparam_tiles(C.byref(d)))
                dpart = torch.empty(tiles, cfg.groups, cfg.G, device=x.device, dtype=torch.float32)
            # the tag says bf16 when the launch takes scratch (only the bf16 input-gradient kernels do), not when the flag is set
            _launch(L.kanvit_layer_bwd_input, "kanvit_layer_bwd_input", x.device, C.byref(d), _ptr(x), _ptr(u), _ptr(w), _ptr(bparams),
                    _ptr(dy), _ptr(dx), _ptr(du_buf), _ptr(dpart), query=(L.kanvit_layer_bwd_input_workspace, C.byref(d)), null_ws=True,
                    tag=lambda nb_in: stem + "_bwd_input" + ("_bf16" if nb_in else ""), cost=_layer_cost(cfg, M, "bwd_input"))
            if cfg.family == RBF:
                if has_u:
                    du = du_buf
                else:   # u aliased x (no LayerNorm): fold the spline-path gradient back into dx
                    nshare = cfg.groups // cfg.x_group_mod
                    dx = dx + du_buf.view(M, nshare, cfg.x_group_mod * cfg.I).sum(1)
            if sine_freq:
                dbp = torch.zeros_like(bparams)
                dbp[:, :cfg.G] = dpart.sum(0)
        if need_w:
            dw = torch.empty_like(w)
            weight_pass(d, dw, "_bwd_weight")
        if freq_via_w:
            dq = LayerDesc(*[getattr(d, f) for f, _ in LayerDesc._fields_])
            dq.flags = cfg.flags | _lib.FLAG_SINE_DFREQ
            q = torch.empty_like(w)
            weight_pass(dq, q, "_bwd_freq")
            dbp = torch.zeros_like(bparams)
            dbp[:, :cfg.G] = q.mul_(w).view(cfg.groups, cfg.I, cfg.G, cfg.O).sum((1, 3))
        if need_b and has_bias:
            if pd is not None:
                db = dy[:, pd.prepend_rows:, :].sum((0, 1)).view(1, cfg.O)
            else:
                db = dy.view(M, cfg.groups, cfg.O).sum(0)
    return (dx if need_x else None), (du if need_u else None), dw, dbp, db


def ln_fusable(cfg: "LayerCfg", M: int) -> bool:
    """True when the register kernels can form FastKAN's LayerNorm themselves for this launch (kanvit_layer_ln_fusable)."""
    if cfg.family != RBF:
        return False
    d = _desc(_autocast_cfg(cfg), M, cfg.x_group_mod * cfg.I, cfg.groups * cfg.I, cfg.groups * cfg.O,
              cfg.G + 2 * cfg.I)
    return bool(_lib.lib().kanvit_layer_ln_fusable(C.byref(d)))


class _KanLayerLnFn(torch.autograd.Function):
    """FastKAN launch with the LayerNorm of the spline path formed IN the kernels (KANVIT_FLAG_FUSED_LN):
    y = spline(rbf(LN_g(x_slice))) + base(silu(x_slice)) for every group g, bparams[g] = [centres | gamma_g | beta_g].

    The forward kernel computes each row slice's (mean, rstd), normalises on the fly and writes the statistics [M, x_group_mod, 2];
    the [M, groups*I] normalised tensor u is never materialised (one write + three reads of it per step saved).  Backward: both
    gradient kernels rebuild u from x and the saved statistics; the input-gradient kernel still returns d loss / d u, from which
    the LayerNorm backward (d gamma, d beta, d x) is the standard closed form over the saved statistics (models/fastkan.py:68's
    nn.LayerNorm, biased variance)."""

    @staticmethod
    @_fwd_f32
    def forward(ctx, x, w, bparams, bias, cfg: LayerCfg, tag: Optional[str] = None):
        y, x, stats, w, bparams, bias = _kan_forward(cfg, x, None, w, bparams, bias, tag, fused_ln=True)
        ctx.tag = tag
        ctx.cfg = cfg
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, stats, w, bparams)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, dy):
        x, stats, w, bparams = ctx.saved_tensors
        cfg = ctx.cfg
        need_x, need_w, need_bp, need_b = ctx.needs_input_grad[:4]
        need_ln = need_x or need_bp
        dx, du, dw, _, db = _kan_backward(cfg, x, stats, w, bparams, dy.float().contiguous(),
                                          (need_ln, need_ln, need_w, False, need_b), True, ctx.has_bias, tag=ctx.tag)
        dbp = None
        if need_ln:
            # LayerNorm backward from du and the saved statistics: dx += ..., d gamma, d beta in one pass (kanvit_layer_ln_bwd)
            M, I, G = x.shape[0], cfg.I, cfg.G
            d = _desc(cfg, M, x.shape[1], cfg.groups * I, cfg.groups * cfg.O, bparams.shape[1])
            L = _lib.lib()
            dgb = torch.empty(2, cfg.groups, I, device=x.device, dtype=torch.float32)
            _launch(L.kanvit_layer_ln_bwd, "kanvit_layer_ln_bwd", x.device, C.byref(d), _ptr(x), _ptr(stats), _ptr(bparams), _ptr(du),
                    _ptr(dx if need_x else None), _ptr(dgb[0]), _ptr(dgb[1]), query=(L.kanvit_layer_ln_bwd_workspace, C.byref(d)),
                    tag="ln_bwd", cost=(0, 4 * M * (cfg.groups * I + (3 if need_x else 1) * cfg.x_group_mod * I)))
            if need_bp:
                dbp = torch.cat([torch.zeros(cfg.groups, G, device=x.device, dtype=torch.float32), dgb[0], dgb[1]], dim=1)
        return (dx if need_x else None), dw, dbp, db, None, None


def kan_layer_ln(x: torch.Tensor, w: torch.Tensor, cfg: LayerCfg, bparams: torch.Tensor, bias: Optional[torch.Tensor],
                 eps: float, tag: Optional[str] = None) -> torch.Tensor:
    """kan_layer() for FastKAN with the LayerNorm fused (call only when ln_fusable(cfg, M)); bparams = [centres | gamma | beta]."""
    f = cfg.flags | _lib.FLAG_FUSED_LN | _autocast_flags()
    return _KanLayerLnFn.apply(x, w, bparams, bias, replace(cfg, flags=f, ln_eps=float(eps)), tag)


def patchify(images: torch.Tensor, n_patches: int) -> torch.Tensor:
    """(B, C, H, W) -> (B, n^2, C*ph*pw): patches row-major, each flattened in (C, ph, pw) order (model.py:111-126)."""
    b, c, h, w = images.shape
    ph, pw = h // n_patches, w // n_patches
    return images.reshape(b, c, n_patches, ph, n_patches, pw).permute(0, 2, 4, 1, 3, 5).reshape(b, n_patches * n_patches, c * ph * pw)


class _PatchEmbedFn(torch.autograd.Function):
    """images[B, C, H, W] -> tokens[B, P + 1, O] = [cls + pos[0]; layer(patch(b, p)) + pos[1 + p]] in ONE launch (SURVEY.md
    section 8(f)2): the kernel gathers its rows from the NCHW images (no [B, P, I] staging tensor), adds the position
    embedding in its epilogue and writes the class-token rows; with KANVIT_FLAG_BF16_MFMA in cfg.flags (bf16 autocast) the
    bf16 register-form forward does the same.  Backward: the layer's weight gradient (and SineKAN's frequency pass) gathers
    its x rows from the saved images and its dY rows from the token-sequence gradient (kanvit_patch_embed_bwd_weight) -- no
    transient patch matrix, no copy of dY without the class-token rows; layers the gathering kernels do not cover
    (kanvit_patch_embed_bwd_weight_ok) rebuild a transient patch matrix.  d cls = sum_b dy[b, 0]."""

    @staticmethod
    @_fwd_f32
    def forward(ctx, images, w, bparams, bias, cls, pos, cfg: LayerCfg, n_patches: int):
        for n, t in (("images", images), ("w", w), ("bparams", bparams), ("bias", bias), ("cls", cls), ("pos", pos)):
            _require_gpu_f32(n, t)
        images = images.contiguous()
        w = w.contiguous()
        B, Cc, H, W = images.shape
        P = n_patches * n_patches
        y = torch.empty(B, P + 1, cfg.O, device=images.device, dtype=torch.float32)
        d = _desc(cfg, B * P, cfg.I, cfg.I, cfg.O, 0 if bparams is None else bparams.shape[1])
        pd = _lib.PatchDesc(Cc, H, W, n_patches, 1, 0)
        bp = None if bparams is None else bparams.contiguous()
        bs = None if bias is None else bias.contiguous()
        cl, po = cls.contiguous(), pos.contiguous()
        L = _lib.lib()
        # only the bf16 forward takes scratch: the query is made under the flag alone
        _launch(L.kanvit_patch_embed_fwd_ws, "kanvit_patch_embed_fwd", images.device, C.byref(d), C.byref(pd), _ptr(images), _ptr(w), _ptr(bp),
                _ptr(bs), _ptr(cl), _ptr(po), _ptr(y), null_ws=True,
                query=(L.kanvit_layer_fwd_workspace, C.byref(d)) if cfg.flags & _lib.FLAG_BF16_MFMA else _NO_SCRATCH,
                tag=_bf16_tag("layer_fwd", cfg.flags), cost=_layer_cost(cfg, B * P, "fwd"))
        ctx.cfg, ctx.n_patches = cfg, n_patches
        ctx.has_bp, ctx.has_bias = bparams is not None, bias is not None
        ctx.save_for_backward(images, w, bp)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, dy):
        images, w, bparams = ctx.saved_tensors
        cfg, P = ctx.cfg, ctx.n_patches ** 2
        dy = dy.float().contiguous()
        B, Cc, H, W = images.shape
        dcls = dy[:, 0, :].sum(0) if ctx.needs_input_grad[4] else None
        needs = (False, False, ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bp, ctx.needs_input_grad[3] and ctx.has_bias)
        pd = _lib.PatchDesc(Cc, H, W, ctx.n_patches, 1, 0)
        d = _desc(cfg, B * P, cfg.I, cfg.I, cfg.O, 0 if bparams is None else bparams.shape[1])
        with torch.cuda.device(images.device):
            gather = bool(_lib.lib().kanvit_patch_embed_bwd_weight_ok(C.byref(d), C.byref(pd))) and not _lib.py_switches()["no_patch_bw"]
        if cfg.family == SINE and _lib.py_switches()["no_dfreq_w"]:
            gather = False          # d loss / d freq through the input-gradient kernel needs the patch matrix
        if gather:
            _, _, dw, dbp, db = _kan_backward(cfg, images, None, w, bparams, dy, needs, False, ctx.has_bias, patch=(pd, B * P))
        else:
            x = patchify(images, ctx.n_patches).reshape(-1, cfg.I)                 # transient
            dyt = dy[:, 1:, :].reshape(-1, cfg.O)                                  # transient (contiguous patch-token rows)
            _, _, dw, dbp, db = _kan_backward(cfg, x, None, w, bparams, dyt, needs, False, ctx.has_bias)
        return None, dw, dbp, db, dcls, None, None, None


def patch_embed(images, w, cfg: LayerCfg, bparams, bias, cls, pos, n_patches: int) -> torch.Tensor:
    """Fused patch embedding (see _PatchEmbedFn); w is the packed weight [1, K, O], cls [O], pos [P + 1, O].  Raises
    KanvitError for shapes the fused kernel does not cover (the caller falls back to patchify + kan_layer).  Under bf16
    autocast the contraction runs on the bf16 matrix cores (KANVIT_FLAG_BF16_MFMA), as kan_layer() does."""
    return _PatchEmbedFn.apply(images, w, bparams, bias, cls, pos, _autocast_cfg(cfg), n_patches)


def kan_layer(x: torch.Tensor, w: torch.Tensor, cfg: LayerCfg, u: Optional[torch.Tensor] = None,
              bparams: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, tag: Optional[str] = None) -> torch.Tensor:
    """Fused basis + contraction for `cfg.groups` layers sharing the rows of x (see include/kanvit.h).  `tag` names the launch
    for the kernel timer ("<tag>_fwd", "<tag>_bwd_input", ...; default "qkv" for a grouped launch, "layer" for a single layer).

    Under ``torch.autocast('cuda', dtype=torch.bfloat16)`` the contraction is allowed onto the bf16 matrix cores
    (KANVIT_FLAG_BF16_MFMA); without autocast it is always the exact fp32 path."""
    return _KanLayerFn.apply(x, u, w, bparams, bias, _autocast_cfg(cfg), tag)


# ------------------------------------------------------------------------------------------------
# per-edge mean absolute activation (the KAN paper's regulariser; csrc/kan_edge_l1.hip)
# ------------------------------------------------------------------------------------------------
EDGE_L1_FAMILIES = (BSPLINE, CHEBY, RBF)


def _edge_l1_desc(cfg: LayerCfg, x: torch.Tensor, bparams) -> LayerDesc:
    M, cols = x.shape
    two = cfg.family == RBF and cfg.has_base                 # [u | x]: the base column reads the raw input, ldu columns to the right
    want = cfg.x_group_mod * cfg.I * (2 if two else 1)
    if cols != want:
        raise KanvitError(f"edge_l1: x has {cols} columns, expected {want}" + (" ([u | x] for RBF with the base column)" if two else ""))
    ldx = max(x.stride(0), cols) if M > 1 else cols
    return _desc(cfg, M, ldx, cfg.x_group_mod * cfg.I if two else 0, cfg.groups * cfg.O, 0 if bparams is None else bparams.shape[1])


class _EdgeL1Fn(torch.autograd.Function):
    """A[groups, I, O] = mean over the rows of |phi_{g,i,o}(x)|; gradients to x and to the packed weights."""

    @staticmethod
    @_fwd_f32
    def forward(ctx, x, w, bparams, cfg: LayerCfg):
        for n, t in (("x", x), ("w", w), ("bparams", bparams)):
            _require_gpu_f32(n, t)
        if x.dim() != 2:
            raise KanvitError(f"edge_l1: x must be 2-D, got {tuple(x.shape)}")
        if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):      # a column slice of a wider matrix is read in place
            x = x.contiguous()                                                       # (ldx), any other layout is copied
        w = w.contiguous()
        bparams = None if bparams is None else bparams.contiguous()
        if tuple(w.shape) != (cfg.groups, cfg.K, cfg.O):
            raise KanvitError(f"packed weight shape {tuple(w.shape)} != {(cfg.groups, cfg.K, cfg.O)}")
        d = _edge_l1_desc(cfg, x, bparams)
        L = _lib.lib()
        A = torch.empty(cfg.groups, cfg.I, cfg.O, device=x.device, dtype=torch.float32)
        _launch(L.kanvit_edge_l1_fwd, "kanvit_edge_l1_fwd", x.device, C.byref(d), _ptr(x), _ptr(w), _ptr(bparams), _ptr(A),
                query=(L.kanvit_edge_l1_fwd_workspace, C.byref(d)), tag="edge_l1_fwd",
                cost=(2 * x.shape[0] * cfg.K * cfg.O * cfg.groups, 4 * (x.numel() + w.numel() + A.numel())))
        ctx.cfg = cfg
        ctx.save_for_backward(x, w, bparams)
        return A

    @staticmethod
    @_bwd
    def backward(ctx, gA):
        x, w, bparams = ctx.saved_tensors
        cfg = ctx.cfg
        gA = gA.float().contiguous()
        d = _edge_l1_desc(cfg, x, bparams)
        L = _lib.lib()
        dw = torch.empty_like(w)
        # dx in x's own row stride (the descriptor has one ldx); NULL when nobody asks for it: the kernel then skips the derivatives
        dx = torch.empty_strided(x.shape, (d.ldx, 1), device=x.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        _launch(L.kanvit_edge_l1_bwd, "kanvit_edge_l1_bwd", x.device, C.byref(d), _ptr(x), _ptr(w), _ptr(bparams), _ptr(gA), _ptr(dw), _ptr(dx),
                query=(L.kanvit_edge_l1_bwd_workspace, C.byref(d)), tag="edge_l1_bwd",
                cost=((6 if dx is not None else 4) * x.shape[0] * cfg.K * cfg.O * cfg.groups,
                      4 * ((1 if dx is None else 2) * x.numel() + 2 * w.numel() + gA.numel())))
        return dx, dw, None, None


def edge_l1(x2d: torch.Tensor, w_packed: torch.Tensor, cfg: LayerCfg, bparams: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A[groups, I, O] = mean_m |phi_{g,i,o}(x2d[m, (g % x_group_mod)*I + i])|, the mean absolute activation of every edge of
    `cfg.groups` KAN layers sharing the rows of x2d (kanvit_edge_l1_*; include/kanvit.h): the quantity the KAN paper's L1 and
    entropy regulariser is built from, computed without the (rows, in, out) activation tensor.  w_packed [groups, K, O] and
    bparams as for kan_layer(); families BSPLINE, CHEBY and RBF.  RBF takes the LayerNorm'ed input; with cfg.has_base its
    x2d is [u | x] (the base column reads the raw input).  Differentiable w.r.t. x2d and w_packed; always exact fp32, also
    under autocast (the statistic has no bf16 mode); deterministic; no host synchronisation (HIP-graph capturable)."""
    if cfg.family not in EDGE_L1_FAMILIES:
        raise NotImplementedError(f"edge_l1: family {_lib.FAMILY_NAMES[cfg.family]} is not supported (supported: bspline, cheby, rbf)")
    keep = _lib.FLAG_UNIFORM_KNOTS | _lib.FLAG_SHARED_BPARAMS
    if cfg.flags & ~keep:
        cfg = replace(cfg, flags=cfg.flags & keep)
    return _EdgeL1Fn.apply(x2d, w_packed, bparams, cfg)


def l1_entropy_loss(l1: torch.Tensor, regularize_activation: float = 1.0, regularize_entropy: float = 1.0) -> torch.Tensor:
    """The two regularisation terms of models/effkan.py:258-264 on per-edge magnitudes l1[..., out, in]: for every layer (the
    leading dimensions) activation * sum(l1) - entropy * sum(p log p) with p = l1 / sum(l1); summed over the layers.  An edge
    whose magnitude is exactly 0 (every sample outside the knot range) contributes the limit 0 to the entropy term."""
    total = l1.sum((-2, -1), keepdim=True)
    p = l1 / total
    per_layer = regularize_activation * total.squeeze(-1).squeeze(-1) - regularize_entropy * torch.special.xlogy(p, p).sum((-2, -1))
    return per_layer.sum()


# ------------------------------------------------------------------------------------------------
# B-spline refit to a new knot table (KANLinear.update_grid; csrc/kan_bspline_refit.hip)
# ------------------------------------------------------------------------------------------------
def _bspline_fit(who: str, x2d, w_old_packed, cfg: LayerCfg, old_G: int, old_knots, new_knots, keep_old: bool):
    """The body of bspline_refit (old_G = cfg.G, keep_old: a flagged feature's rows of w_new are the old ones) and of
    bspline_regrid (rows of zeros): validation under the caller's name `who`, then the kanvit_<who>_gram and _solve launches."""
    if cfg.family != BSPLINE:
        raise NotImplementedError(f"{who}: family {_lib.FAMILY_NAMES[cfg.family]} has no knot table to refit (bspline only)")
    cfg = replace(cfg, flags=cfg.flags & (_lib.FLAG_UNIFORM_KNOTS | _lib.FLAG_SHARED_BPARAMS))
    for n, t in (("x", x2d), ("w_old", w_old_packed), ("old_knots", old_knots), ("new_knots", new_knots)):
        _require_gpu_f32(n, t)
    x = x2d
    if x.dim() != 2:
        raise KanvitError(f"{who}: x must be 2-D, got {tuple(x.shape)}")
    if x.shape[1] != cfg.x_group_mod * cfg.I:
        raise KanvitError(f"{who}: x has {x.shape[1]} columns, expected {cfg.x_group_mod * cfg.I}")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):      # a column slice of a wider matrix is read in place
        x = x.contiguous()
    M = x.shape[0]
    ldx = max(x.stride(0), x.shape[1]) if M > 1 else x.shape[1]
    nb, nk = cfg.G, cfg.G + cfg.spline_order + 1
    nbo, nko = old_G, old_G + cfg.spline_order + 1
    w_old = w_old_packed.contiguous()
    if tuple(w_old.shape) != (cfg.groups, cfg.I * nbo, cfg.O):
        raise KanvitError(f"{who}: packed weight shape {tuple(w_old.shape)} != {(cfg.groups, cfg.I * nbo, cfg.O)}" if keep_old else
                          f"{who}: old packed weight shape {tuple(w_old.shape)} != {(cfg.groups, cfg.I * nbo, cfg.O)} (old nb={nbo})")
    old_msg = "{}: old knot table {} does not hold [{}][{}*{}]"
    if not keep_old and (old_knots.dim() < 1 or old_knots.shape[0] != cfg.groups):
        raise KanvitError(old_msg.format(who, tuple(old_knots.shape), cfg.groups, cfg.I, nko))
    old_knots = old_knots.reshape(cfg.groups, -1).contiguous()
    new_knots = new_knots.contiguous()
    bad_old, bad_new = old_knots.shape[1] < cfg.I * nko, tuple(new_knots.shape) != (cfg.x_group_mod, cfg.I, nk)
    if keep_old and (bad_old or bad_new):
        raise KanvitError(f"{who}: knot tables {tuple(old_knots.shape)} / {tuple(new_knots.shape)} do not hold "
                          f"[{cfg.groups}][{cfg.I}*{nk}] / [{cfg.x_group_mod}][{cfg.I}][{nk}]")
    if bad_old:
        raise KanvitError(old_msg.format(who, tuple(old_knots.shape), cfg.groups, cfg.I, nko))
    if bad_new:
        raise KanvitError(f"{who}: new knot table {tuple(new_knots.shape)} != [{cfg.x_group_mod}][{cfg.I}][{nk}]")
    d = _desc(cfg, M, ldx, 0, cfg.groups * cfg.O, old_knots.shape[1])
    L = _lib.lib()
    dev = x.device
    lead = (C.byref(d),) if keep_old else (C.byref(d), C.c_int(old_G))         # the regrid entry points take the old basis size
    gram_n = torch.empty(cfg.x_group_mod, cfg.I, nb, nb, device=dev, dtype=torch.float64)
    gram_c = torch.empty(cfg.groups, cfg.I, nb, nbo, device=dev, dtype=torch.float64)
    # the rows of a flagged feature are not written: they stay the old ones, or zero where the old rows have another shape
    w_new = w_old.clone() if keep_old else torch.zeros(cfg.groups, cfg.I * nb, cfg.O, device=dev, dtype=torch.float32)
    ok = torch.empty(cfg.x_group_mod, cfg.I, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev), _timed(who, 2 * M * cfg.I * nb * (cfg.groups * nbo + cfg.x_group_mod * nb),
                                        4 * (x.numel() + w_old.numel() + w_new.numel())):
        _launch(getattr(L, f"kanvit_{who}_gram"), f"kanvit_{who}_gram", dev, *lead, _ptr(x), _ptr(old_knots), _ptr(new_knots), _ptr(gram_n),
                _ptr(gram_c), query=(getattr(L, f"kanvit_{who}_workspace"), *lead))
        _launch(getattr(L, f"kanvit_{who}_solve"), f"kanvit_{who}_solve", dev, *lead, _ptr(gram_n), _ptr(gram_c), _ptr(w_old), _ptr(w_new),
                _ptr(ok))
    return w_new, ok.bool()


@torch.no_grad()
def bspline_refit(x2d: torch.Tensor, w_old_packed: torch.Tensor, cfg: LayerCfg, old_knots: torch.Tensor,
                  new_knots: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(w_new_packed [groups, I*nb, O], ok [x_group_mod, I] bool): the spline weights of `cfg.groups` B-spline layers refitted
    from old_knots [groups, I*nk] to new_knots [x_group_mod, I, nk] (one table per x slice) on the rows of x2d, so that every
    edge computes the function it computed before wherever the rows sample it -- what models/effkan.py:189-242 obtains from a
    (rows, in, out) tensor and lstsq, here from two nb x nb Gram matrices per feature (kanvit_bspline_refit_*; include/kanvit.h).
    cfg: family BSPLINE, G = nb = grid_size + spline_order, has_base = 0; w_old_packed as edge_l1's weights without the base
    column.  ok is False for a feature whose fit does not exist (constant column, fewer distinct samples than nb, ...): its rows
    of w_new_packed are w_old_packed's.  Exact fp32 / float64 also under autocast, deterministic, no autograd, no host
    synchronisation (HIP-graph capturable); workspace and matrices come from the torch allocator."""
    return _bspline_fit("bspline_refit", x2d, w_old_packed, cfg, cfg.G, old_knots, new_knots, keep_old=True)


@torch.no_grad()
def bspline_regrid(x2d: torch.Tensor, w_old_packed: torch.Tensor, cfg_new: LayerCfg, old_G: int, old_knots: torch.Tensor,
                   new_knots: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(w_new_packed [groups, I*nb_new, O], ok [x_group_mod, I] bool): bspline_refit onto a basis of another size, the numerical
    half of KANLinear.extend_grid (kanvit_bspline_regrid_*; include/kanvit.h).  cfg_new describes the NEW layers (family BSPLINE,
    G = nb_new = new grid_size + spline_order, has_base = 0), old_G = nb_old the old ones, the spline order is common;
    w_old_packed [groups, I*nb_old, O], old_knots [groups, I*nk_old], new_knots [x_group_mod, I, nk_new].  The cross matrix of
    the normal equations is rectangular, nb_new x nb_old; everything else is bspline_refit's.  ok is False for a feature whose
    fit does not exist; its rows of w_new_packed are ZERO (there are no old rows of the new shape to keep).  Exact fp32 /
    float64 also under autocast, deterministic, no autograd, no host synchronisation."""
    return _bspline_fit("bspline_regrid", x2d, w_old_packed, cfg_new, int(old_G), old_knots, new_knots, keep_old=False)


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
_attn_flags = 0     # set by attention()/attention_packed() from the ambient autocast state (the Functions run with autocast off)


def _attn_build_desc(q, k, v, o, causal: bool, scale: float, flags: int, self_attention: bool) -> AttnDesc:
    """kanvit_attn_desc of q, o [B, H, Nq, D] and k, v [B, H, Nk, D] (self-attention: Nk = Nq), after the shape and stride checks."""
    B, H, Nq, D = q.shape
    Nk = Nq if self_attention else k.shape[2]
    for n, t, L in (("q", q, Nq), ("k", k, Nk), ("v", v, Nk), ("o", o, Nq)):
        if t.dim() != 4 or tuple(t.shape) != (B, H, L, D):
            if not self_attention:
                raise KanvitError(f"attention: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, o {tuple(o.shape)} do not agree")
            # kanvit_attn_desc carries ONE sequence length: a shorter k/v would be read out of bounds, a longer one silently
            # truncated.  The reference's FlashAttentionFunction accepts q_len != k_len (utils.py:150-160); this path does not.
            raise KanvitError(f"attention: {n} has shape {tuple(t.shape)}, expected {(B, H, L, D)} "
                              "(self-attention only: q, k, v and o must agree in batch, heads, length and head size)")
        if t.stride(3) != 1:
            raise KanvitError(f"{n}: innermost dimension must be contiguous")
    return AttnDesc(B, H, Nq, D, int(bool(causal)), float(scale), int(flags), 0,
                    q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
                    v.stride(0), v.stride(1), v.stride(2), o.stride(0), o.stride(1), o.stride(2))


def _attn_desc(q, k, v, o, causal: bool, scale: float, flags: int = 0) -> AttnDesc:
    return _attn_build_desc(q, k, v, o, causal, scale, flags, True)


def _attn_fits_one_workgroup(N: int, D: int) -> bool:
    """The ViT kernels of csrc/attention.hip hold one head in a work-group's LDS (check_desc's bound: N <= 224 at D = 64, 256 at
    D <= 32) and take D <= 64 (KANVIT_ATTN_MAX_D); longer sequences (e.g. 384 x 384 images at patch 16: N = 577) and wider heads
    (64 < D <= 128, e.g. ViT-H/14: D = 80) take the chunked general kernels (csrc/attention_x.hip).  The forward and the backward
    both route by this one predicate."""
    if D > 64:
        return False
    ks, npad = (32 if D <= 32 else 64) + 1, (N + 31) // 32 * 32
    return N <= 256 and 4 * (2 * npad * ks + 2 * npad + 4 * 32 * ks) <= 160 * 1024


def _attn_x_flags(flags: int, D: int) -> int:
    """The flags a head routed to the general kernels takes: their bf16 twins cover D <= 64 (KANVIT_ATTN_MAX_D); wider heads run
    exact fp32 with or without autocast.  The forward and the backward of one head derive the same flags, as they must (lse
    of one mode is not valid input to the other's backward)."""
    return flags & _lib.FLAG_BF16_MFMA if D <= 64 else 0


def _attn_takes_general_kernels(q, k) -> bool:
    """The one routing decision of a self-attention head, for its forward and its backward alike."""
    return q.dim() == 4 and tuple(k.shape) == tuple(q.shape) and not _attn_fits_one_workgroup(q.shape[2], q.shape[3])


def _attn_fwd(q, k, v, o, causal, scale, flags=0):
    if _attn_takes_general_kernels(q, k):
        return _attn_x_fwd(q, k, v, o, None, causal, scale, flags=_attn_x_flags(flags, q.shape[3]))
    B, H, N, D = q.shape
    lse = torch.empty(B, H, N, device=q.device, dtype=torch.float32)
    d = _attn_desc(q, k, v, o, causal, scale, flags)
    _launch(_lib.lib().kanvit_attn_fwd, "kanvit_attn_fwd", q.device, C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse),
            tag=_bf16_tag("attn_fwd", flags), cost=(4 * B * H * N * N * D, 4 * 4 * B * H * N * D))
    return lse


def _attn_backward(name, descs, q, k, v, o, lse, do, dq, dk, dv, tag, cost):
    """The backward launch of either attention path: entry point `name` and its workspace query `name`_workspace, both led by
    the descriptor(s) `descs`."""
    if (do.stride() != o.stride()) or dq.stride() != q.stride() or dk.stride() != k.stride() or dv.stride() != v.stride():
        raise KanvitError("attention backward: gradient layouts must match their forward tensors")
    L = _lib.lib()
    lead = tuple(C.byref(t) for t in descs)
    _launch(getattr(L, name), name, q.device, *lead, _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), _ptr(do), _ptr(dq), _ptr(dk), _ptr(dv),
            query=(getattr(L, name + "_workspace"), *lead), tag=tag, cost=cost)


def _attn_bwd(q, k, v, o, lse, do, dq, dk, dv, causal, scale, flags=0):
    if _attn_takes_general_kernels(q, k):
        return _attn_x_bwd(q, k, v, o, lse, do, dq, dk, dv, None, causal, scale, flags=_attn_x_flags(flags, q.shape[3]))
    d = _attn_desc(q, k, v, o, causal, scale, flags)
    B, H, N, D = q.shape
    # algorithmic work of a recompute backward: 5 products (S, dP, dV, dK, dQ) = 2.5x the forward; the two-kernel bf16 path
    # executes 7 (S and dP twice), the fp32 dS-spill path exactly 5
    _attn_backward("kanvit_attn_bwd", (d,), q, k, v, o, lse, do, dq, dk, dv, _bf16_tag("attn_bwd", flags),
                   (10 * B * H * N * N * D, 4 * 9 * B * H * N * D))


def _attn_ext(Nk: int, mask) -> "_lib.AttnExt":
    """kanvit_attn_ext of Nk keys and a mask that is None or torch.bool on the device, expanded to [B, H, Nq, Nk]."""
    if mask is None:
        return _lib.AttnExt(Nk, 0, None, 0, 0, 0, 0)
    return _lib.AttnExt(Nk, 0, mask.data_ptr(), mask.stride(0), mask.stride(1), mask.stride(2), mask.stride(3))


def _attn_x_desc(q, k, v, o, mask, causal: bool, scale: float, flags: int = 0):
    """Descriptor pair of the general attention kernels (kanvit_attn_x_*): q, o [B, H, Nq, D]; k, v [B, H, Nk, D]; mask None or a
    torch.bool tensor already expanded (views, no copy) to [B, H, Nq, Nk]."""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        _require_gpu_f32(n, t)
    d = _attn_build_desc(q, k, v, o, causal, scale, flags, False)
    B, H, Nq, Nk = d.B, d.H, d.N, k.shape[2]
    if mask is not None and (mask.dtype != torch.bool or not mask.is_cuda or tuple(mask.shape) != (B, H, Nq, Nk)):
        raise KanvitError(f"attention mask: need a torch.bool GPU tensor expanded to {(B, H, Nq, Nk)}, got {mask.dtype} {tuple(mask.shape)}")
    return d, _attn_ext(Nk, mask)


def _attn_x_fwd(q, k, v, o, mask, causal, scale, flags=0):
    """flags = _lib.FLAG_BF16_MFMA runs the bf16 matrix-core twins (D <= 64); the backward must then take the same flags."""
    B, H, Nq, D = q.shape
    lse = torch.empty(B, H, Nq, device=q.device, dtype=torch.float32)
    d, e = _attn_x_desc(q, k, v, o, mask, causal, scale, flags)
    Nk = k.shape[2]
    _launch(_lib.lib().kanvit_attn_x_fwd, "kanvit_attn_x_fwd", q.device, C.byref(d), C.byref(e), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse),
            tag=_bf16_tag("attn_x_fwd", flags), cost=(4 * B * H * Nq * Nk * D, 4 * 2 * B * H * (Nq + Nk) * D))
    return lse


def _attn_x_bwd(q, k, v, o, lse, do, dq, dk, dv, mask, causal, scale, flags=0):
    d, e = _attn_x_desc(q, k, v, o, mask, causal, scale, flags)
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    _attn_backward("kanvit_attn_x_bwd", (d, e), q, k, v, o, lse, do, dq, dk, dv, _bf16_tag("attn_x_bwd", flags),
                   (14 * B * H * Nq * Nk * D, 4 * 4 * B * H * (Nq + Nk) * D))


class _AttnPackedFn(torch.autograd.Function):
    """qkv[B, N, 3, H, D] (the layout the grouped q|k|v KAN launch writes) -> o[B, N, H*D]."""

    @staticmethod
    @_fwd_f32
    def forward(ctx, qkv, causal: bool, scale: float, flags: int = 0):
        _require_gpu_f32("qkv", qkv)
        qkv = qkv.contiguous()
        B, N, three, H, D = qkv.shape
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o = torch.empty(B, N, H, D, device=qkv.device, dtype=torch.float32)
        lse = _attn_fwd(q, k, v, o.permute(0, 2, 1, 3), causal, scale, flags)
        ctx.save_for_backward(qkv, o, lse)
        ctx.causal, ctx.scale, ctx.flags = causal, scale, flags
        return o.view(B, N, H * D)

    @staticmethod
    @_bwd
    def backward(ctx, do):
        do = do.float()
        qkv, o, lse = ctx.saved_tensors
        B, N, _, H, D = qkv.shape
        do = do.contiguous().view(B, N, H, D)
        dqkv = torch.empty_like(qkv)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        _attn_bwd(q, k, v, o.permute(0, 2, 1, 3), lse, do.permute(0, 2, 1, 3), dq, dk, dv, ctx.causal, ctx.scale, ctx.flags)
        return dqkv, None, None, None


class _AttnFn(torch.autograd.Function):
    """Separate q, k, v of shape (B, H, N, D) with arbitrary outer strides -> o (B, H, N, D)."""

    @staticmethod
    @_fwd_f32
    def forward(ctx, q, k, v, causal: bool, scale: float, flags: int = 0):
        for n, t in (("q", q), ("k", k), ("v", v)):
            _require_gpu_f32(n, t)
        q, k, v = (t if t.stride(3) == 1 else t.contiguous() for t in (q, k, v))
        o = torch.empty(q.shape, device=q.device, dtype=torch.float32)
        lse = _attn_fwd(q, k, v, o, causal, scale, flags)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal, ctx.scale, ctx.flags = causal, scale, flags
        return o

    @staticmethod
    @_bwd
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        do = do.float().contiguous()
        dq, dk, dv = (torch.empty_strided(t.shape, t.stride(), device=t.device, dtype=t.dtype) for t in (q, k, v))
        _attn_bwd(q, k, v, o, lse, do, dq, dk, dv, ctx.causal, ctx.scale, ctx.flags)
        return dq, dk, dv, None, None, None


def _autocast_flags() -> int:
    """bf16 autocast allows the products onto the bf16 matrix cores; otherwise the exact fp32 kernels run."""
    on = torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16
    return _lib.FLAG_BF16_MFMA if on else 0


def _autocast_cfg(cfg: LayerCfg) -> LayerCfg:
    """cfg with the flag of _autocast_flags() added."""
    f = cfg.flags | _autocast_flags()
    return cfg if f == cfg.flags else replace(cfg, flags=f)


def attention_packed(qkv: torch.Tensor, causal: bool = False, scale: Optional[float] = None) -> torch.Tensor:
    """Self-attention on qkv[B, N, 3, H, D] -> o[B, N, H*D].  D even and <= 128.  Heads of D <= 64 that fit one work-group run the
    ViT kernels, longer sequences the chunked general kernels; under bf16 autocast both run on the bf16 matrix cores
    (KANVIT_FLAG_BF16_MFMA).  Heads wider than 64 run the exact-fp32 general kernels, with or without autocast (the general
    kernels' bf16 twins cover D <= 64)."""
    return _AttnPackedFn.apply(qkv, causal, qkv.shape[-1] ** -0.5 if scale is None else scale, _autocast_flags())


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False,
              scale: Optional[float] = None) -> torch.Tensor:
    """Self-attention on q, k, v of shape (B, H, N, D); routing and autocast behaviour as attention_packed()."""
    return _AttnFn.apply(q, k, v, causal, q.shape[-1] ** -0.5 if scale is None else scale, _autocast_flags())


class _AttnQ1Fn(torch.autograd.Function):
    """q0[B, H, D] and kv[B, N, 2, H, D] (the layout the grouped k|v KAN launch writes) -> o[B, H, D]: one query per head
    (kanvit_attn_q1_*).  The probabilities p[B, H, N] are the forward's second output inside the library and all the backward
    needs besides o; dk and dv are written into one packed tensor of kv's layout, which the KAN backward reads as it is."""

    @staticmethod
    @_fwd_f32
    def forward(ctx, q0, kv, scale: float):
        _require_gpu_f32("q0", q0)
        _require_gpu_f32("kv", kv)
        if kv.dim() != 5 or kv.shape[2] != 2 or q0.dim() != 3 or (q0.shape[0], q0.shape[1], q0.shape[2]) != (kv.shape[0], kv.shape[3], kv.shape[4]):
            raise KanvitError(f"attention_q1: q0 {tuple(q0.shape)} and kv {tuple(kv.shape)} are not [B, H, D] and [B, N, 2, H, D]")
        q0, kv = q0.contiguous(), kv.contiguous()
        B, N, _, H, D = kv.shape
        o = torch.empty(B, H, D, device=kv.device, dtype=torch.float32)
        p = torch.empty(B, H, N, device=kv.device, dtype=torch.float32)
        d, e = _attn_q1_desc(q0, kv, o, scale)
        # 2 flops per element of k and of v; k and v are read once, o and p are small
        _launch(_lib.lib().kanvit_attn_q1_fwd, "kanvit_attn_q1_fwd", kv.device, C.byref(d), C.byref(e), _ptr(q0), _ptr(kv[:, :, 0]),
                _ptr(kv[:, :, 1]), _ptr(o), _ptr(p), tag="attn_q1_fwd", cost=(4 * B * H * N * D, 4 * B * H * (2 * N * D + N + 2 * D)))
        ctx.save_for_backward(q0, kv, o, p)
        ctx.scale = scale
        return o

    @staticmethod
    @_bwd
    def backward(ctx, do):
        q0, kv, o, p = ctx.saved_tensors
        do = do.float().contiguous()
        B, N, _, H, D = kv.shape
        dq = torch.empty_like(q0)
        dkv = torch.empty_like(kv)
        d, e = _attn_q1_desc(q0, kv, o, ctx.scale)
        _launch(_lib.lib().kanvit_attn_q1_bwd, "kanvit_attn_q1_bwd", kv.device, C.byref(d), C.byref(e), _ptr(q0), _ptr(kv[:, :, 0]),
                _ptr(kv[:, :, 1]), _ptr(o), _ptr(p), _ptr(do), _ptr(dq), _ptr(dkv[:, :, 0]), _ptr(dkv[:, :, 1]),
                tag="attn_q1_bwd", cost=(8 * B * H * N * D, 4 * B * H * (4 * N * D + N + 4 * D)))
        return dq, dkv, None


def _attn_q1_desc(q0, kv, o, scale: float):
    """Descriptor pair of kanvit_attn_q1_*: contiguous q0, o [B, H, D] and the k / v halves of a contiguous kv[B, N, 2, H, D]."""
    B, N, _, H, D = kv.shape
    k = kv[:, :, 0]                  # [B, N, H, D]
    d = AttnDesc(B, H, 1, D, 0, float(scale), 0, 0, q0.stride(0), q0.stride(1), 0, k.stride(0), k.stride(2), k.stride(1),
                 k.stride(0), k.stride(2), k.stride(1), o.stride(0), o.stride(1), 0)
    return d, _attn_ext(N, None)


def attention_q1(q0: torch.Tensor, kv: torch.Tensor, scale: Optional[float] = None) -> torch.Tensor:
    """softmax(scale q0 k^T) v for ONE query per (sample, head): q0 [B, H, D] against kv [B, N, 2, H, D], the packed output of a
    grouped k|v launch (k = kv[:, :, 0], v = kv[:, :, 1], read in place) -> o [B, H, D].  What the last block of a ViT needs: its
    head reads the class token only.  D even and <= 128, any N >= 1; scale defaults to D ** -0.5.  Differentiable w.r.t. q0 and
    kv (the gradient of kv comes back packed).  One mode: exact fp32, also under autocast (inputs are cast to float32);
    bitwise reproducible; no host synchronisation.  B = 0 gives an empty result without a launch."""
    return _AttnQ1Fn.apply(q0, kv, kv.shape[-1] ** -0.5 if scale is None else float(scale))


def expand_attention_mask(mask: Optional[torch.Tensor], q: torch.Tensor, k: torch.Tensor) -> Optional[torch.Tensor]:
    """The mask forms utils.FlashAttentionFunction accepts -- a [B, Nk] key-padding mask ('b n -> b 1 1 n', utils.py:156-157) or
    anything broadcastable to [B, H, Nq, Nk], True = attend -- as a torch.bool view expanded to [B, H, Nq, Nk] (no copy)."""
    if mask is None:
        return None
    if mask.dim() == 2:
        mask = mask[:, None, None, :]
    return mask.to(device=q.device, dtype=torch.bool).expand(q.shape[0], q.shape[1], q.shape[2], k.shape[2])


def _attn_probs(q, k, mask, causal, scale, rows):
    for n, t in (("q", q), ("k", k)):
        _require_gpu_f32(n, t)
        if t.dim() != 4:
            raise KanvitError(f"attention_probs: {n} has shape {tuple(t.shape)}, expected [B, H, length, D]")
    B, H, Nq, D = q.shape
    if tuple(k.shape[:2]) != (B, H) or k.shape[3] != D:
        raise KanvitError(f"attention_probs: q {tuple(q.shape)} and k {tuple(k.shape)} do not agree in batch, heads and head size")
    Nk = k.shape[2]
    q, k = (t if t.stride(3) == 1 else t.contiguous() for t in (q, k))
    mask = expand_attention_mask(mask, q, k)
    scale = D ** -0.5 if scale is None else scale
    rows = Nq if rows is None else int(rows)
    if not 1 <= rows <= Nq:
        raise KanvitError(f"attention_probs: rows={rows} must be in [1, {Nq}]")
    if B == 0:
        return torch.empty(B, H, rows, Nk, device=q.device, dtype=torch.float32)
    d = AttnDesc(B, H, Nq, D, int(bool(causal)), float(scale), 0, 0, q.stride(0), q.stride(1), q.stride(2),
                 k.stride(0), k.stride(1), k.stride(2), 0, 0, 0, 0, 0, 0)
    e = _attn_ext(Nk, mask)     # expand_attention_mask: torch.bool on q's device, [B, H, Nq, Nk]
    p = torch.empty(B, H, rows, Nk, device=q.device, dtype=torch.float32)
    # three sweeps of the q.k products (max, sum, store); the map itself is the traffic
    _launch(_lib.lib().kanvit_attn_probs, "kanvit_attn_probs", q.device, C.byref(d), C.byref(e), _ptr(q), _ptr(k), _ptr(p), p.stride(0),
            p.stride(1), p.stride(2), rows, tag="attn_probs", cost=(6 * B * H * rows * Nk * D, 4 * B * H * (rows * Nk + rows * D + Nk * D)))
    return p


@torch.no_grad()
def attention_probs(q: torch.Tensor, k: torch.Tensor, mask: Optional[torch.Tensor] = None, causal: bool = False,
                    scale: Optional[float] = None, rows: Optional[int] = None) -> torch.Tensor:
    """softmax(scale * q k^T) of q [B, H, Nq, D] and k [B, H, Nk, D] -> [B, H, R, Nk] float32: the attention probabilities the
    fused kernels never materialise (kanvit_attn_probs; attention maps and rollout).  `rows` = R keeps the first R queries only
    (default Nq; 1 = the class-token row).  `mask`: a [B, Nk] key-padding mask or anything broadcastable to [B, H, Nq, Nk],
    True = attend; `causal` needs Nk <= Nq.  Domain and dead-position semantics are FlashAttentionFunction's: D even and <= 128,
    any lengths, a dead position is exactly 0 and a query with no live key gives an all-zero row.  scale defaults to D ** -0.5.
    The map is a diagnostic and is NOT differentiable: it is computed under torch.no_grad() and comes back without history.
    One mode, fp32 with compensated dot products, also under autocast (inputs of another dtype are cast to float32).  No host synchronisation."""
    with torch.autocast("cuda", enabled=False):
        q, k = (t.float() if t.is_cuda and t.is_floating_point() else t for t in (q, k))
        return _attn_probs(q, k, mask, causal, scale, rows)


@torch.no_grad()
def attention_probs_packed(qkv: torch.Tensor, causal: bool = False, scale: Optional[float] = None,
                           rows: Optional[int] = None) -> torch.Tensor:
    """attention_probs of the q and k slices of qkv[B, N, 3, H, D] (the layout the grouped q|k|v launch writes), read in place ->
    [B, H, R, N] float32.  Bit for bit attention_probs on contiguous copies of q and k.  Not differentiable; exact fp32 also
    under autocast."""
    with torch.autocast("cuda", enabled=False):
        if qkv.is_cuda and qkv.is_floating_point():
            qkv = qkv.float()
        _require_gpu_f32("qkv", qkv)
        if qkv.dim() != 5 or qkv.shape[2] != 3:
            raise KanvitError(f"attention_probs_packed: qkv has shape {tuple(qkv.shape)}, expected [B, N, 3, H, D]")
        qkv = qkv.contiguous()
        q, k = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(2))
        return _attn_probs(q, k, None, causal, scale, rows)


# ------------------------------------------------------------------------------------------------
# residual add + LayerNorm (TransformerBlock assembly, reference model.py:31-37)
# ------------------------------------------------------------------------------------------------
class _AddLayerNormFn(torch.autograd.Function):
    """(x, delta | None, gamma, beta) -> (s = x + delta, LayerNorm(s)) in one pass; backward in one pass + a tiny reduce.

    The residual stream (x, s, their gradients) is fp32.  Under torch.autocast(bfloat16) the tensors that come from / go to the
    feed-forward GEMMs may be bf16 and are read / written as they are (kanvit_addln_*_ex) instead of through cast kernels:
    `delta` (the previous block's feed-forward output), `y` when `y_bf16` (the feed-forward's input), the gradient arriving
    on y, and the gradient returned for a bf16 delta (a second, rounded copy of dx written by the same pass)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, delta, gamma, beta, eps, y_bf16):
        if not x.is_cuda:
            raise KanvitError(f"x is on {x.device}: the kanvit ops run only on an AMD GPU (no CPU fallback)")
        L = _lib.lib()
        D = x.shape[-1]
        x2 = x.float().contiguous().view(-1, D)
        d2 = None
        if delta is not None:
            d2 = (delta if delta.dtype in (torch.float32, torch.bfloat16) else delta.float()).contiguous().view(-1, D)
        M = x2.shape[0]
        y = torch.empty(M, D, device=x.device, dtype=torch.bfloat16 if y_bf16 else torch.float32)
        s = torch.empty_like(x2) if d2 is not None else x2
        mean = torch.empty(M, device=x.device, dtype=torch.float32)
        rstd = torch.empty(M, device=x.device, dtype=torch.float32)
        g, b = gamma.float().contiguous(), beta.float().contiguous()
        _launch(L.kanvit_addln_fwd_ex, "kanvit_addln_fwd", x.device, M, D, float(eps), _ptr(x2), _ptr(d2),
                int(d2 is not None and d2.dtype == torch.bfloat16), _ptr(g), _ptr(b), _ptr(s) if d2 is not None else None, _ptr(y),
                int(bool(y_bf16)), _ptr(mean), _ptr(rstd))
        ctx.save_for_backward(s, g, mean, rstd)
        ctx.delta_dtype = None if d2 is None else d2.dtype
        ctx.shape = x.shape
        return s.view(x.shape), y.view(x.shape)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gs, gy):
        s, g, mean, rstd = ctx.saved_tensors
        L = _lib.lib()
        M, D = s.shape
        if gy is None:
            gy2 = torch.zeros_like(s)
        else:
            gy2 = gy.contiguous().view(M, D)
            if gy2.dtype != torch.bfloat16:
                gy2 = gy2.float()
        gs2 = None if gs is None else gs.contiguous().view(M, D).float()
        dx = torch.empty_like(s)
        dxb = torch.empty(M, D, device=s.device, dtype=torch.bfloat16) if ctx.delta_dtype == torch.bfloat16 else None
        dg = torch.empty(D, device=s.device, dtype=torch.float32)
        db = torch.empty(D, device=s.device, dtype=torch.float32)
        _launch(L.kanvit_addln_bwd_ex, "kanvit_addln_bwd", s.device, M, D, _ptr(s), _ptr(g), _ptr(mean), _ptr(rstd), _ptr(gy2),
                int(gy2.dtype == torch.bfloat16), _ptr(gs2), _ptr(dx), _ptr(dxb), _ptr(dg), _ptr(db), query=(L.kanvit_addln_bwd_workspace, M, D))
        dx = dx.view(ctx.shape)
        dd = None if ctx.delta_dtype is None else (dxb.view(ctx.shape) if dxb is not None else dx)
        return dx, dd, dg, db, None, None


class _AddLayerNormScaledFn(torch.autograd.Function):
    """(x, delta, row_scale[B], gamma, beta) -> (s = x + row_scale[sample] * delta, LayerNorm(s)): _AddLayerNormFn with the per-sample
    scale of stochastic depth inside the same pass (kanvit_addln_sd_*).  Rows r * N .. r * N + N - 1 belong to sample r.  The gradient
    of delta, row_scale * dx, is a tensor of its own written by the backward pass (fp32, or bf16 for a bf16 delta); row_scale gets none."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, delta, row_scale, rows_per_sample, gamma, beta, eps, y_bf16):
        if not x.is_cuda:
            raise KanvitError(f"x is on {x.device}: the kanvit ops run only on an AMD GPU (no CPU fallback)")
        _require_gpu_f32("row_scale", row_scale)
        L = _lib.lib()
        D = x.shape[-1]
        x2 = x.float().contiguous().view(-1, D)
        d2 = (delta if delta.dtype in (torch.float32, torch.bfloat16) else delta.float()).contiguous().view(-1, D)
        M, N = x2.shape[0], int(rows_per_sample)
        sc = row_scale.contiguous().view(-1)
        if d2.shape != x2.shape or N < 1 or M % N or sc.numel() * N != M:
            raise KanvitError(f"add_layernorm(row_scale): x has {M} rows, delta {tuple(delta.shape)}, {sc.numel()} scales x {N} rows per sample")
        y = torch.empty(M, D, device=x.device, dtype=torch.bfloat16 if y_bf16 else torch.float32)
        s = torch.empty_like(x2)
        mean = torch.empty(M, device=x.device, dtype=torch.float32)
        rstd = torch.empty(M, device=x.device, dtype=torch.float32)
        g, b = gamma.float().contiguous(), beta.float().contiguous()
        _launch(L.kanvit_addln_sd_fwd, "kanvit_addln_sd_fwd", x.device, M, D, float(eps), _ptr(x2), _ptr(d2), int(d2.dtype == torch.bfloat16),
                _ptr(g), _ptr(b), _ptr(s), _ptr(y), int(bool(y_bf16)), _ptr(mean), _ptr(rstd), _ptr(sc), N)
        ctx.save_for_backward(s, g, mean, rstd, sc)
        ctx.delta_dtype = d2.dtype
        ctx.n = N
        ctx.shape = x.shape
        return s.view(x.shape), y.view(x.shape)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gs, gy):
        s, g, mean, rstd, sc = ctx.saved_tensors
        L = _lib.lib()
        M, D = s.shape
        if gy is None:
            gy2 = torch.zeros_like(s)
        else:
            gy2 = gy.contiguous().view(M, D)
            if gy2.dtype != torch.bfloat16:
                gy2 = gy2.float()
        gs2 = None if gs is None else gs.contiguous().view(M, D).float()
        dx = torch.empty_like(s)
        dd = torch.empty(M, D, device=s.device, dtype=ctx.delta_dtype)
        dg = torch.empty(D, device=s.device, dtype=torch.float32)
        db = torch.empty(D, device=s.device, dtype=torch.float32)
        _launch(L.kanvit_addln_sd_bwd, "kanvit_addln_sd_bwd", s.device, M, D, _ptr(s), _ptr(g), _ptr(mean), _ptr(rstd), _ptr(gy2),
                int(gy2.dtype == torch.bfloat16), _ptr(gs2), _ptr(dx), _ptr(dd), int(dd.dtype == torch.bfloat16), _ptr(dg), _ptr(db),
                _ptr(sc), ctx.n, query=(L.kanvit_addln_bwd_workspace, M, D))
        return dx.view(ctx.shape), dd.view(ctx.shape), None, None, dg, db, None, None


def add_layernorm(x: torch.Tensor, delta: Optional[torch.Tensor], norm: torch.nn.LayerNorm, y_bf16: bool = False,
                  row_scale: Optional[torch.Tensor] = None, rows_per_sample: Optional[int] = None):
    """(x + delta, norm(x + delta)) -- delta None gives (x, norm(x)).  Shapes the kernel does not cover (last dim not a
    multiple of 4 or > 1024, non-affine norms) take the stock ops; like every kanvit op it needs CUDA tensors.
    y_bf16: write norm(...) as bfloat16 (the caller feeds it to bf16 GEMMs under autocast: no cast pass in between).
    row_scale (float32 [B], stochastic depth: depth_scales): s = x + row_scale[sample] * delta in the same pass, sample = row //
    rows_per_sample; x is [B, N, d] (rows_per_sample = N) or 2-D with rows_per_sample given.  None is the unscaled path."""
    D = x.shape[-1]
    if row_scale is not None:
        if delta is None:
            raise ValueError("add_layernorm: row_scale scales delta, and delta is None")
        if x.dim() == 3 and rows_per_sample in (None, x.shape[1]):
            rows_per_sample = x.shape[1]
        elif x.dim() != 2 or rows_per_sample is None:
            raise ValueError(f"add_layernorm(row_scale): x is [B, N, d], or 2-D with rows_per_sample; got {tuple(x.shape)}, rows_per_sample={rows_per_sample}")
    if norm.weight is None or norm.bias is None or len(norm.normalized_shape) != 1 or D % 4 or D > 1024 or D < 4:
        if row_scale is not None:
            delta = (row_scale.repeat_interleave(int(rows_per_sample)).view(*x.shape[:-1], 1) * delta).to(delta.dtype)
        s = x if delta is None else x + delta
        return s, norm(s)
    if row_scale is not None:
        return _AddLayerNormScaledFn.apply(x, delta, row_scale, int(rows_per_sample), norm.weight, norm.bias, norm.eps, bool(y_bf16))
    return _AddLayerNormFn.apply(x, delta, norm.weight, norm.bias, norm.eps, bool(y_bf16))


def depth_scales(B: int, keep, seed: int, counter: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The stochastic-depth scales of one forward: float32 [n_branch, B], entry (j, b) = 1 / keep[j] if sample b keeps branch j, else 0
    (kanvit_depth_scales; the hash and the threshold are stated in include/kanvit.h, depth_keep below restates them on the CPU).
    keep: a sequence of n_branch <= 64 probabilities in (0, 1] -- host values, baked into the launch; seed: any integer (taken mod
    2^64); counter: a one-element int64 tensor on the device, read and then incremented by the launch, so consecutive calls -- and
    replays of a captured call -- draw different masks without RNG state and without anything from the host.  One launch, capturable."""
    keep = [float(k) for k in keep]
    n = len(keep)
    if not torch.is_tensor(counter) or not counter.is_cuda or counter.dtype != torch.int64 or counter.numel() != 1:
        raise KanvitError("depth_scales: counter is a one-element int64 tensor on the GPU")
    B = int(B)
    if out is None:
        out = torch.empty(n, max(B, 0), device=counter.device, dtype=torch.float32)
    elif not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (n, B) or not out.is_contiguous():
        raise KanvitError(f"depth_scales: out is a contiguous float32 [{n}, {B}] tensor on the GPU")
    host = (C.c_float * max(n, 1))(*keep)
    _launch(_lib.lib().kanvit_depth_scales, "kanvit_depth_scales", counter.device, B, n, C.cast(host, C.c_void_p),
            C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _ptr(counter), _ptr(out))
    return out


def depth_keep(B: int, keep, seed: int, counter: int) -> torch.Tensor:
    """depth_scales restated in Python integers and NumPy float32 on the CPU (the tests compare the kernel with it bit for bit):
    h = mix(mix(mix(seed) + counter) + (j << 32) + b); kept iff (h >> 40) < round(keep_j * 2^24); scale float32(1) / float32(keep_j)."""
    import numpy as np
    from .data import _mix
    m64 = 0xFFFFFFFFFFFFFFFF
    base = _mix((_mix(int(seed) & m64) + int(counter)) & m64)
    out = np.zeros((len(keep), int(B)), dtype=np.float32)
    for j, k in enumerate(keep):
        k32 = np.float32(k)
        if not 0.0 < float(k32) <= 1.0:
            raise ValueError(f"depth_keep: keep[{j}]={k} is outside (0, 1]")
        thr = int(np.rint(np.float64(k32) * 16777216.0))
        inv = np.float32(1.0) / k32
        for b in range(int(B)):
            if (_mix((base + (j << 32) + b) & m64) >> 40) < thr:
                out[j, b] = inv
    return torch.from_numpy(out)


def _patch_keep_domain(who: str, B: int, P: int, K: int):
    if B < 0 or not 1 <= K <= P <= _lib.PATCH_KEEP_MAX_P:
        raise KanvitOperandError(f"{who}: B={B}, P={P}, K={K}: B >= 0 and 1 <= K <= P <= {_lib.PATCH_KEEP_MAX_P} (one sample's keys live in LDS)")


def patch_keep(B: int, P: int, K: int, seed: int, counter: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PatchDropout's keep table of one forward: int32 [B, K], row b the K kept patch numbers of sample b out of P, ascending
    (kanvit_patch_keep; the hash is stated in include/kanvit.h, patch_keep_ref below restates it on the CPU).  seed: any integer (taken
    mod 2^64); counter: a one-element int64 tensor on the device with a value below 2^48, read by the launch and then incremented by
    it, so consecutive calls -- and replays of a captured call -- draw different sets without RNG state and without anything from the
    host.  One launch, capturable.  B = 0 gives an empty table and leaves the counter alone."""
    B, P, K = int(B), int(P), int(K)
    _patch_keep_domain("patch_keep", B, P, K)
    if not torch.is_tensor(counter) or counter.numel() != 1:
        raise KanvitOperandError("patch_keep: counter is a one-element int64 tensor on the GPU")
    _require_tensor("patch_keep", "counter", counter, torch.int64)
    if out is None:
        out = torch.empty(B, K, device=counter.device, dtype=torch.int32)
    else:
        _require_tensor("patch_keep", "out", out, torch.int32, shape=(B, K), device=counter.device)
    _launch(_lib.lib().kanvit_patch_keep, "kanvit_patch_keep", counter.device, B, P, K, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
            _ptr(counter), _ptr(out))
    return out


def patch_keep_ref(B: int, P: int, K: int, seed: int, counter: int) -> torch.Tensor:
    """patch_keep restated in Python integers on the CPU (the tests compare the kernel with it bit for bit): base = mix(mix(seed ^
    TAG) + counter), key(b, p) = mix(base + (b << 32) + p); row b is the K patches with the smallest (key, p), in ascending patch order."""
    from .data import _mix
    B, P, K = int(B), int(P), int(K)
    _patch_keep_domain("patch_keep_ref", B, P, K)
    m64 = 0xFFFFFFFFFFFFFFFF
    base = _mix((_mix((int(seed) & m64) ^ _lib.PATCH_KEEP_TAG) + int(counter)) & m64)
    out = torch.empty(B, K, dtype=torch.int32)
    for b in range(B):
        keys = [(_mix((base + (b << 32) + p) & m64), p) for p in range(P)]
        out[b] = torch.tensor(sorted(p for _, p in sorted(keys)[:K]), dtype=torch.int32)
    return out


def patch_gather(images: torch.Tensor, idx: torch.Tensor, n_patches: int) -> torch.Tensor:
    """patchify(images, n_patches) restricted to the patches idx names: float32 [B * K, C*ph*pw], row b*K + j = patch idx[b, j] of image b
    flattened in (C, ph, pw) order (kanvit_patch_gather: a copy of the kept patches only, straight out of NCHW -- no [B, P, I] matrix).
    images: float32 [B, C, H, W] on the GPU, contiguous, at any 4-byte address; idx: int32 [B, K] on the same GPU with entries in [0,
    n_patches^2) -- in any order, repeats allowed, not checked on the device.  No gradient reaches the images: they are data."""
    if not torch.is_tensor(images) or images.dim() != 4:
        raise KanvitOperandError("patch_gather: images is a float32 [B, C, H, W] tensor on the GPU")
    _require_tensor("patch_gather", "images", images, torch.float32)
    B, Cc, H, W = images.shape
    n = int(n_patches)
    if n < 1 or H % n or W % n:
        raise KanvitOperandError(f"patch_gather: n_patches={n} must divide H={H} and W={W}")
    if not torch.is_tensor(idx) or idx.dim() != 2 or idx.shape[0] != B or not 1 <= idx.shape[1] <= n * n:
        raise KanvitOperandError(f"patch_gather: idx is an int32 [B={B}, K] tensor with 1 <= K <= {n * n}")
    _require_tensor("patch_gather", "idx", idx, torch.int32, device=images.device)
    K, I = idx.shape[1], Cc * (H // n) * (W // n)
    rows = torch.empty(B * K, I, device=images.device, dtype=torch.float32)
    pd = _lib.PatchDesc(Cc, H, W, n, 0, 0)
    _launch(_lib.lib().kanvit_patch_gather, "kanvit_patch_gather", images.device, C.byref(pd), B, K, _ptr(idx), _ptr(images), _ptr(rows), I)
    return rows


class _AssembleTokensFn(torch.autograd.Function):
    """tokens [B*K, O] (or [B, K, O]), cls, pos, idx [B, K] -> [B, K + 1, O] = [cls + pos[0]; tokens[b, j] + pos[1 + idx[b, j]]] in one
    launch; backward: d tokens = the gradient without its class rows (a copy), d cls = sum_b dout[b, 0] in a fixed order."""

    @staticmethod
    @_fwd_f32
    def forward(ctx, tokens, cls, pos, idx):
        who = "assemble_tokens"
        for name, t in (("tokens", tokens), ("cls", cls), ("pos", pos), ("idx", idx)):
            if not torch.is_tensor(t):
                raise KanvitOperandError(f"{who}: {name} is a tensor on the GPU")
        if idx.dim() != 2 or idx.shape[1] < 1:
            raise KanvitOperandError(f"{who}: idx is an int32 [B, K] tensor with K >= 1, got shape {tuple(idx.shape)}")
        B, K = idx.shape
        _require_tensor(who, "tokens", tokens, torch.float32, contiguous=False)
        O = tokens.shape[-1]
        if tuple(tokens.shape) not in ((B * K, O), (B, K, O)):
            raise KanvitOperandError(f"{who}: tokens has shape {tuple(tokens.shape)}, expected ({B * K}, O) or ({B}, {K}, O)")
        _require_tensor(who, "idx", idx, torch.int32, device=tokens.device)
        _require_tensor(who, "cls", cls, torch.float32, device=tokens.device, contiguous=False)
        _require_tensor(who, "pos", pos, torch.float32, device=tokens.device, contiguous=False)
        if cls.numel() != O or pos.dim() != 2 or pos.shape[1] != O:
            raise KanvitOperandError(f"{who}: cls has {cls.numel()} elements and pos shape {tuple(pos.shape)}, expected {O} and (P + 1, {O})")
        t2 = tokens.reshape(B * K, O)
        if B * K and (t2.stride(1) != 1 or t2.stride(0) < O):      # a matrix with padded rows is read in place
            t2 = t2.contiguous()
        out = torch.empty(B, K + 1, O, device=tokens.device, dtype=torch.float32)
        _launch(_lib.lib().kanvit_tokens_assemble_fwd, "kanvit_tokens_assemble_fwd", tokens.device, B, K, O, _ptr(t2), max(t2.stride(0), O),
                _ptr(cls.reshape(-1).contiguous()), _ptr(pos.contiguous()), _ptr(idx), _ptr(out))
        ctx.tokens_shape, ctx.cls_shape = tuple(tokens.shape), tuple(cls.shape)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, dout):
        dout = dout.float().contiguous()
        B, N, O = dout.shape
        dtokens = torch.empty(B * (N - 1), O, device=dout.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        dcls = torch.empty(O, device=dout.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        if dtokens is not None or dcls is not None:
            _launch(_lib.lib().kanvit_tokens_assemble_bwd, "kanvit_tokens_assemble_bwd", dout.device, B, N - 1, O, _ptr(dout), _ptr(dtokens),
                    _ptr(dcls))
        return (None if dtokens is None else dtokens.view(ctx.tokens_shape), None if dcls is None else dcls.view(ctx.cls_shape), None, None)


def assemble_tokens(tokens: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """The token sequence of a PatchDropout forward: float32 [B, K + 1, O] with row 0 = cls + pos[0] and row 1 + j = tokens[b*K + j] +
    pos[1 + idx[b, j]] -- the position embedding of the ORIGINAL patch positions, one fp32 add per element (bit for bit torch's cat +
    indexed add).  tokens: float32 [B*K, O] (the row stride may exceed O) or [B, K, O]; cls: O elements; pos: [P + 1, O]; idx: int32
    [B, K] as patch_keep writes it.  Gradients for tokens (a copy of the patch rows) and cls (a fixed-order sum: reproducible)."""
    return _AssembleTokensFn.apply(tokens, cls, pos, idx)


class _RestoreTokensFn(torch.autograd.Function):
    """y [B, K + 1, O], mask_token, pos [P + 1, O], idx [B, K] -> [B, P + 1, O]: the kept tokens back at their patch positions, the mask
    token at the dropped ones, the position rows of all positions, in one launch; backward: d y = the rows the kept tokens went to (a
    copy), d mask_token = the sum of the dropped rows in a fixed tree."""

    @staticmethod
    @_fwd_f32
    def forward(ctx, y, mask_token, pos, idx):
        who = "restore_tokens"
        for name, t in (("y", y), ("mask_token", mask_token), ("pos", pos), ("idx", idx)):
            if not torch.is_tensor(t):
                raise KanvitOperandError(f"{who}: {name} is a tensor on the GPU")
        if idx.dim() != 2 or y.dim() != 3 or pos.dim() != 2:
            raise KanvitOperandError(f"{who}: y is [B, K + 1, O], pos [P + 1, O] and idx [B, K]; got shapes {tuple(y.shape)}, {tuple(pos.shape)}, "
                                     f"{tuple(idx.shape)}")
        B, K = idx.shape
        O, P = y.shape[-1], pos.shape[0] - 1
        if not 1 <= K < P <= _lib.PATCH_KEEP_MAX_P:
            raise KanvitOperandError(f"{who}: K={K} kept of P={P} patches: 1 <= K < P <= {_lib.PATCH_KEEP_MAX_P} (idx is patch_keep's table)")
        _require_tensor(who, "y", y, torch.float32, shape=(B, K + 1, O), contiguous=False, error=KanvitOperandError)
        _require_tensor(who, "idx", idx, torch.int32, device=y.device, error=KanvitOperandError)
        _require_tensor(who, "mask_token", mask_token, torch.float32, device=y.device, contiguous=False, error=KanvitOperandError)
        _require_tensor(who, "pos", pos, torch.float32, shape=(P + 1, O), device=y.device, contiguous=False, error=KanvitOperandError)
        if mask_token.numel() != O:
            raise KanvitOperandError(f"{who}: mask_token has {mask_token.numel()} elements, expected O = {O}")
        out = torch.empty(B, P + 1, O, device=y.device, dtype=torch.float32)
        _launch(_lib.lib().kanvit_tokens_restore_fwd, "kanvit_tokens_restore_fwd", y.device, B, P, K, O, _ptr(y.contiguous()),
                _ptr(mask_token.reshape(-1).contiguous()), _ptr(pos.contiguous()), _ptr(idx), _ptr(out), tag="restore_tokens",
                cost=(0, 4 * O * (B * (2 * P + K + 3) + P + 2)))
        ctx.save_for_backward(idx)
        ctx.mask_shape = tuple(mask_token.shape)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, dout):
        idx, = ctx.saved_tensors
        dout = dout.float().contiguous()
        (B, N, O), K = dout.shape, idx.shape[1]
        dy = torch.empty(B, K + 1, O, device=dout.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        dmask = torch.empty(O, device=dout.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        if dy is not None or dmask is not None:
            _launch(_lib.lib().kanvit_tokens_restore_bwd, "kanvit_tokens_restore_bwd", dout.device, B, N - 1, K, O, _ptr(dout), _ptr(idx),
                    _ptr(dy), _ptr(dmask), tag="restore_tokens_bwd", cost=(0, 4 * O * (B * (N + K + 1) + 1)))
        return dy, None if dmask is None else dmask.view(ctx.mask_shape), None, None


def restore_tokens(y: torch.Tensor, mask_token: torch.Tensor, pos: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """The decoder's sequence of a masked autoencoder: float32 [B, P + 1, O] with row 0 = y[b, 0] + pos[0] and row 1 + p = y[b, 1 + j] +
    pos[1 + p] where p = idx[b, j], mask_token + pos[1 + p] at every dropped p -- one fp32 add per element (bit for bit torch's repeat
    + cat + gather + add).  y: float32 [B, K + 1, O], the encoder's K + 1 rows after the decoder's input projection; mask_token: O
    elements; pos: [P + 1, O]; idx: int32 [B, K] as patch_keep writes it (rows strictly ascending: a precondition, not checked on the
    device), 1 <= K < P.  Gradients for y (a copy of its rows) and mask_token (a sum over the B (P - K) dropped rows in a tree that (B,
    P, K) fix: reproducible)."""
    return _RestoreTokensFn.apply(y, mask_token, pos, idx)


# ---------------------------------------------------------------------------------------------------------------------------
# the training loop's off-model kernels, from here to the end of the file: one operand check
# ---------------------------------------------------------------------------------------------------------------------------
class KanvitOperandError(KanvitError, ValueError):
    """A refused operand of erase_u8's own (erase, noise) or a refused RandAugment table: a KanvitError like every refusal here, and
    the ValueError a caller of a table-taking function expects."""


def _require_tensor(who: str, name: str, t: torch.Tensor, dtype, shape=None, device=None, contiguous: bool = True, hint: str = "",
                    error=KanvitError):
    """The one place the ops below test an operand: on a GPU (`device`: on that one; None: any), of `dtype` (one, or a tuple to choose
    from; `hint` is added to that refusal), contiguous, and of `shape` where one is given.  A refusal raises `error`."""
    if not t.is_cuda:
        raise error(f"{who}: {name} is on {t.device}: the kanvit ops run only on an AMD GPU (no CPU fallback)")
    if device is not None and t.device != device:
        raise error(f"{who}: {name} is on {t.device}, expected {device}")
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if t.dtype not in dtypes:
        raise error(f"{who}: {name} has dtype {t.dtype}, expected {' or '.join(str(d) for d in dtypes)}{hint}")
    if contiguous and not t.is_contiguous():
        raise error(f"{who}: {name} with shape {tuple(t.shape)} and strides {tuple(t.stride())} is not contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise error(f"{who}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")


# ---------------------------------------------------------------------------------------------------------------------------
# batches from a GPU-resident uint8 dataset (kanvit/data.py; csrc/batch_u8.hip)
# ---------------------------------------------------------------------------------------------------------------------------
_BATCH_TABLES = (("crop", torch.int32, (5,)), ("partner", torch.int64, ()), ("weight", torch.float32, ()), ("box", torch.int32, (4,)),
                 ("erase", torch.int32, (4,)))


def _batch_operands(who: str, images, labels, idx, lut, out, name: str, pair, **tables):
    """What augment_u8 / mix_u8 / resample_u8 / erase_u8 share, checked: the sizes (N, B, H, W, C), `pair` (an int or two; `name` is "pad", or
    "out_size": the output then has that size instead of the images') as two ints, and the tensors the launch writes: `out` (the
    caller's, or a new one), y where labels are given, y2 and w where the mix tables are.  tables: crop / partner / weight / box /
    erase, each or None."""
    _require_tensor(who, "images", images, torch.uint8)
    if images.dim() not in (3, 4):
        raise KanvitError(f"{who}: images has shape {tuple(images.shape)}, expected [N, H, W, C] or [N, H, W]")
    dev = images.device
    N, H, W = (int(v) for v in images.shape[:3])
    Cn = int(images.shape[3]) if images.dim() == 4 else 1
    try:
        pair = (int(pair), int(pair)) if isinstance(pair, int) else (int(pair[0]), int(pair[1]))
    except (TypeError, IndexError):
        raise KanvitError(f"{who}: {name}={pair!r} is an int or a pair of ints") from None
    OH, OW = pair if name == "out_size" else (H, W)
    _require_tensor(who, "idx", idx, torch.int64, None, dev)
    if idx.dim() != 1:
        raise KanvitError(f"{who}: idx has shape {tuple(idx.shape)}, expected [B]")
    B = int(idx.shape[0])
    if labels is not None:
        _require_tensor(who, "labels", labels, torch.int64, (N,), dev)
    _require_tensor(who, "lut", lut, torch.float32, (Cn, 256), dev)
    for table, dt, tail in _BATCH_TABLES:
        if tables.get(table) is not None:
            _require_tensor(who, table, tables[table], dt, (N,) + tail, dev, error=KanvitOperandError if table == "erase" else KanvitError)
    if out is None:
        out = torch.empty((B, Cn, max(OH, 0), max(OW, 0)), device=dev, dtype=torch.float32)
    else:
        _require_tensor(who, "out", out, torch.float32, (B, Cn, OH, OW), dev)
    mixing = tables.get("partner") is not None
    y = torch.empty((B,), device=dev, dtype=torch.int64) if labels is not None else None
    y2 = torch.empty((B,), device=dev, dtype=torch.int64) if mixing else None
    w = torch.empty((B,), device=dev, dtype=torch.float32) if mixing else None
    return (N, B, H, W, Cn), pair, (out, y, y2, w)


def augment_u8(images: torch.Tensor, labels: Optional[torch.Tensor], idx: torch.Tensor, lut: torch.Tensor, pad=0, flip: bool = False,
               seed: int = 0, epoch: int = 0, return_params: bool = False, out: Optional[torch.Tensor] = None):
    """One batch out of a dataset that stays on the device as uint8: gather images[idx], random crop out of the zero-padded image,
    random horizontal flip, ToTensor + Normalize through `lut` (data.make_lut), in one launch on the current stream (the reference's
    transforms, train.py:100-118; semantics and the per-sample hash: include/kanvit.h).

    images uint8 [N, H, W, C] or [N, H, W]; labels int64 [N] or None; idx int64 [B], every entry in [0, N) -- the CALLER checks that
    (data.GpuDataset does, on the CPU, before the list goes to the device); lut float32 [C, 256]; pad an int or (pad_y, pad_x).
    Returns x float32 [B, C, H, W] (and y int64 [B] when labels are given, and params int32 [B, 3] = (dy, dx, flip) with
    return_params).  `out`: write into this contiguous [B, C, H, W] float32 tensor instead of allocating one."""
    sizes, pads, (out, y, _, _) = _batch_operands("augment_u8", images, labels, idx, lut, out, "pad", pad)
    params = torch.empty((sizes[1], 3), device=images.device, dtype=torch.int32) if return_params else None
    _launch(_lib.lib().kanvit_augment_u8, "kanvit_augment_u8", images.device, _ptr(images), _ptr(labels), _ptr(idx), _ptr(lut), _ptr(out), _ptr(y),
            _ptr(params), *sizes, *pads, int(bool(flip)), int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1))
    res = (out,) + ((y,) if labels is not None else ()) + ((params,) if return_params else ())
    return res[0] if len(res) == 1 else res


def mix_u8(images: torch.Tensor, labels: torch.Tensor, idx: torch.Tensor, lut: torch.Tensor, partner: torch.Tensor, weight: torch.Tensor,
           box: torch.Tensor, pad=0, flip: bool = False, seed: int = 0, epoch: int = 0, out: Optional[torch.Tensor] = None):
    """augment_u8 with Mixup / CutMix in the same launch (semantics: include/kanvit.h).  partner int64 [N], weight float32 [N] and box
    int32 [N, 4] = (y0, y1, x0, x1) are the epoch's table (data.mix_table) on the device, indexed by the DATASET index: sample s =
    idx[b] is blended with (Mixup, empty box) or gets the box of (CutMix) sample partner[s] under that sample's own crop and flip;
    partner -1 leaves it as augment_u8 gives it.  Every partner lies in [-1, N): the CALLER checks that before the upload, as for idx.
    Returns (x float32 [B, C, H, W], y int64 [B] = labels[s], y2 int64 [B] = the partner's label (y where not mixed), w float32 [B] =
    weight[s])."""
    for name, t in (("labels", labels), ("partner", partner), ("weight", weight), ("box", box)):
        if t is None:
            raise KanvitError(f"mix_u8: {name} is None")
    sizes, pads, (out, y, y2, w) = _batch_operands("mix_u8", images, labels, idx, lut, out, "pad", pad, partner=partner, weight=weight, box=box)
    _launch(_lib.lib().kanvit_mix_u8, "kanvit_mix_u8", images.device, _ptr(images), _ptr(labels), _ptr(idx), _ptr(lut), _ptr(partner),
            _ptr(weight), _ptr(box), _ptr(out), _ptr(y), _ptr(y2), _ptr(w), *sizes, *pads, int(bool(flip)),
            int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1), tag="mix_u8", cost=(0, out.numel() * 6))
    return out, y, y2, w


def resample_u8(images: torch.Tensor, labels: Optional[torch.Tensor], idx: torch.Tensor, lut: torch.Tensor, out_size, crop: Optional[torch.Tensor] = None,
                partner: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None, box: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None):
    """augment_u8 / mix_u8 at an output size of their own, in one launch: the bilinear resize (half-pixel centres, no antialiasing) of
    a per-sample box of the zero-padded, possibly flipped image to out_size = (OH, OW) (semantics and the fixed fp32 operation sequence:
    include/kanvit.h).  crop int32 [N, 5] = (y0, x0, bh, bw, flip) is the epoch's table (data.crop_table) on the device, indexed by the
    DATASET index; None is the whole image, unflipped, for every sample.  partner / weight / box are mix_u8's tables, all three or
    none, with box in OUTPUT coordinates; the partner is resampled under its own crop row.  Every idx and partner lies inside the
    dataset: the CALLER checks that before the upload.
    Returns (x float32 [B, C, OH, OW], y int64 [B]) -- x alone when labels is None -- or (x, y, y2, w) with the mix tables."""
    tables = (partner, weight, box)
    mixing = any(t is not None for t in tables)
    if mixing and any(t is None for t in tables):
        raise KanvitError("resample_u8: partner, weight and box come together (all three or none)")
    if mixing and labels is None:
        raise KanvitError("resample_u8: labels is None: the mix tables yield (x, y, y2, w)")
    sizes, size, (out, y, y2, w) = _batch_operands("resample_u8", images, labels, idx, lut, out, "out_size", out_size, crop=crop, partner=partner,
                                                   weight=weight, box=box)
    _launch(_lib.lib().kanvit_resample_u8, "kanvit_resample_u8", images.device, _ptr(images), _ptr(labels), _ptr(idx), _ptr(lut), _ptr(crop),
            _ptr(partner), _ptr(weight), _ptr(box), _ptr(out), _ptr(y), _ptr(y2), _ptr(w), *sizes, *size,
            tag="resample_u8", cost=(0, out.numel() * 4))
    if mixing:
        return out, y, y2, w
    return (out, y) if labels is not None else out


def erase_u8(images: torch.Tensor, labels: Optional[torch.Tensor], idx: torch.Tensor, lut: torch.Tensor, out_size, crop: Optional[torch.Tensor] = None,
             partner: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None, box: Optional[torch.Tensor] = None,
             erase: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, noise_key: int = 0, out: Optional[torch.Tensor] = None):
    """resample_u8 with Random Erasing in the same launch (semantics: include/kanvit.h).  erase int32 [N, 4] = (y0, y1, x0, x1), half
    open, in OUTPUT coordinates, is the epoch's table (data.erase_table) on the device, indexed by the DATASET index: inside its box
    sample s = idx[b] is replaced by a fill before it is mixed, and its partner is erased under the partner's own row before it is
    pasted or blended in.  noise float32 [T], T a power of two in 2..65536 (data.normal_table), makes the fill noise[top bits of a
    hash of (noise_key, s, c, y, x)] (timm's "pixel"; noise_key: data.erase_noise_key); None makes it 0, the normalised mean
    ("const").  Everything else, and what is returned, is resample_u8's; erase=None IS resample_u8 (noise must then be None)."""
    tables = (partner, weight, box)
    mixing = any(t is not None for t in tables)
    if mixing and any(t is None for t in tables):
        raise KanvitError("erase_u8: partner, weight and box come together (all three or none)")
    if mixing and labels is None:
        raise KanvitError("erase_u8: labels is None: the mix tables yield (x, y, y2, w)")
    if noise is not None and erase is None:
        raise KanvitOperandError("erase_u8: noise without erase: the noise fills the erase boxes")
    sizes, size, (out, y, y2, w) = _batch_operands("erase_u8", images, labels, idx, lut, out, "out_size", out_size, crop=crop, partner=partner,
                                                   weight=weight, box=box, erase=erase)
    T = 0
    if noise is not None:
        _require_tensor("erase_u8", "noise", noise, torch.float32, None, images.device, error=KanvitOperandError)
        T = int(noise.numel())
        if noise.dim() != 1 or T < 2 or T > 65536 or T & (T - 1):
            raise KanvitOperandError(f"erase_u8: noise has shape {tuple(noise.shape)}, expected [T], T a power of two in 2..65536")
    _launch(_lib.lib().kanvit_erase_u8, "kanvit_erase_u8", images.device, _ptr(images), _ptr(labels), _ptr(idx), _ptr(lut), _ptr(crop),
            _ptr(partner), _ptr(weight), _ptr(box), _ptr(out), _ptr(y), _ptr(y2), _ptr(w), *sizes, *size, _ptr(erase), _ptr(noise), T,
            int(noise_key) & (2 ** 64 - 1), tag="erase_u8", cost=(0, out.numel() * 4))
    if mixing:
        return out, y, y2, w
    return (out, y) if labels is not None else out


# ---------------------------------------------------------------------------------------------------------------------------
# RandAugment: one uint8 -> uint8 pass over the dataset per epoch (kanvit/data.py: randaug_table; csrc/randaug.hip)
# ---------------------------------------------------------------------------------------------------------------------------
_RA_FACTOR_OPS = (_lib.RA_BRIGHTNESS, _lib.RA_COLOR, _lib.RA_CONTRAST, _lib.RA_SHARPNESS)
# (op, parameter, lowest, highest) of every parameter include/kanvit.h gives a range; AFFINE takes any int32
_RA_RANGES = ((_lib.RA_POSTERIZE, 0, 0, 8), (_lib.RA_SOLARIZE, 0, 0, 256), (_lib.RA_SOLARIZE_ADD, 0, 0, 255), (_lib.RA_SOLARIZE_ADD, 1, 0, 256),
              *((op, 0, 0, 2 * 65536) for op in _RA_FACTOR_OPS))


def randaug_check_table(table: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    """The check of a RandAugment table on the CPU, BEFORE it is uploaded (data.GpuDataset.batches runs it once per epoch): int32
    [N, K, 8] with 1 <= K <= 4 (and N == n where n is given), every op code one of the twelve of include/kanvit.h and every parameter
    inside the range stated there.  The kernel would turn a row outside them into the identity; here it is a KanvitOperandError (a
    ValueError) that names the first such row.  Returns the table."""
    if not isinstance(table, torch.Tensor) or table.is_cuda or table.dtype != torch.int32 or table.dim() != 3 or table.shape[2] != 8 or \
            not 1 <= table.shape[1] <= _lib.RA_MAX_OPS or (n is not None and table.shape[0] != n):
        what = f"{table.dtype} {tuple(table.shape)} on {table.device}" if isinstance(table, torch.Tensor) else repr(type(table))
        raise KanvitOperandError(f"randaug_check_table: the table is {what}, expected int32 [{'N' if n is None else n}, K, 8] on the CPU, "
                                 f"1 <= K <= {_lib.RA_MAX_OPS}")
    op, p = table[:, :, 0], table[:, :, 1:]
    bad = (op < 0) | (op >= len(_lib.RA_OP_NAMES))
    for code, j, lo, hi in _RA_RANGES:
        bad |= (op == code) & ((p[:, :, j] < lo) | (p[:, :, j] > hi))
    if bool(bad.any()):
        s, k = (int(v) for v in bad.nonzero()[0])
        raise KanvitOperandError(f"randaug_check_table: row [{s}, {k}] = {table[s, k].tolist()} has an unknown op code or a parameter outside its range")
    return table


def randaugment_u8(images: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RandAugment over a whole uint8 dataset in one launch on the current stream (semantics, every op and its integer arithmetic:
    include/kanvit.h, kanvit_randaug_u8): sample s is images[s] passed through the K rows table[s] in order.

    images uint8 [N, H, W, C] or [N, H, W] (C = 1), 1 <= C <= 4 and H W C <= 24 576 bytes (the image lives in LDS; a larger one is
    refused); table int32 [N, K, 8] on the device, 1 <= K <= 4, row = (op, p0 .. p6) -- data.randaug_table draws one per epoch,
    randaug_check_table checks it before the upload; the kernel treats a row it does not know as the identity and never reaches outside
    the image.  `out`: write into this contiguous uint8 tensor of the images' shape -- NOT the images themselves, nor memory that
    overlaps them -- instead of allocating one.  Returns the augmented images; `images` is not changed."""
    who = "randaugment_u8"
    _require_tensor(who, "images", images, torch.uint8)
    if images.dim() not in (3, 4):
        raise KanvitError(f"{who}: images has shape {tuple(images.shape)}, expected [N, H, W, C] or [N, H, W]")
    N, H, W = (int(v) for v in images.shape[:3])
    Cn = int(images.shape[3]) if images.dim() == 4 else 1
    if not 1 <= Cn <= 4 or H < 1 or W < 1 or H * W * Cn > _lib.RA_MAX_BYTES:
        raise KanvitError(f"{who}: images of {H} x {W} x {Cn} = {H * W * Cn} bytes: 1 to 4 channels and at most {_lib.RA_MAX_BYTES} bytes "
                          "(the image and its copy live in LDS)")
    _require_tensor(who, "table", table, torch.int32, None, images.device)
    if table.dim() != 3 or table.shape[0] != N or not 1 <= table.shape[1] <= _lib.RA_MAX_OPS or table.shape[2] != 8:
        raise KanvitError(f"{who}: table has shape {tuple(table.shape)}, expected [{N}, K, 8], 1 <= K <= {_lib.RA_MAX_OPS}")
    if out is None:
        out = torch.empty_like(images)
    else:
        if out is images:
            raise KanvitError(f"{who}: out is images: an op reads more than the byte it writes; give a second buffer")
        _require_tensor(who, "out", out, torch.uint8, tuple(images.shape), images.device)
    _launch(_lib.lib().kanvit_randaug_u8, "kanvit_randaug_u8", images.device, _ptr(images), _ptr(out), _ptr(table), N, H, W, Cn,
            int(table.shape[1]), tag="randaug_u8", cost=(0, 2 * images.numel()))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# soft-target cross-entropy: loss and gradient in one pass over the logits (csrc/soft_ce.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def _logits_2d(who: str, logits: torch.Tensor, dtypes, hint: str = ""):
    """(B, C) of the logits soft_ce and metrics_update walk: on the GPU, of one of `dtypes`, [B >= 1, C >= 2], unit column stride."""
    _require_tensor(who, "logits", logits, dtypes, contiguous=False, hint=hint)
    if logits.dim() != 2:
        raise KanvitError(f"{who}: logits has shape {tuple(logits.shape)}, expected [B, C]")
    B, Cn = (int(v) for v in logits.shape)
    if B < 1 or Cn < 2:
        raise KanvitError(f"{who}: logits has shape {tuple(logits.shape)}: at least one row and two classes")
    if logits.stride(1) != 1 or logits.stride(0) < Cn:
        raise KanvitError(f"{who}: logits has strides {tuple(logits.stride())}: unit column stride and a row stride of at least C = {Cn}")
    return B, Cn


def soft_ce(logits: torch.Tensor, y: torch.Tensor, y2: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None,
            label_smoothing: float = 0.0):
    """The kernel call behind soft_cross_entropy, without autograd: (loss float32 [], loss_rows float32 [B], dlogits float32 [B, C]) for
    logits float32 [B, C] (unit column stride; a padded row stride is taken as it is), y int64 [B], and y2 int64 [B] with w float32 [B]
    or neither (semantics: include/kanvit.h).  One launch plus the one-work-group mean; no host synchronisation."""
    who = "soft_cross_entropy"
    B, Cn = _logits_2d(who, logits, torch.float32, hint=" (train.py hands the loss y_hat.float())")
    if (y2 is None) != (w is None):
        raise KanvitError(f"{who}: y2 and w come together")
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise KanvitError(f"{who}: label_smoothing={label_smoothing} must be in [0, 1)")
    for name, t, dt in (("y", y, torch.int64), ("y2", y2, torch.int64), ("w", w, torch.float32)):
        if t is not None:
            _require_tensor(who, name, t, dt, (B,), logits.device)
    out = torch.empty((B * Cn + B + 1,), device=logits.device, dtype=torch.float32)
    dlogits, loss_rows, loss = out[:B * Cn].view(B, Cn), out[B * Cn:B * Cn + B], out[B * Cn + B:].view(())
    _launch(_lib.lib().kanvit_soft_ce, "kanvit_soft_ce", logits.device, _ptr(logits), int(logits.stride(0)), _ptr(y), _ptr(y2), _ptr(w), B, Cn,
            C.c_float(float(label_smoothing)), _ptr(loss_rows), _ptr(dlogits), _ptr(loss), tag="soft_ce", cost=(0, B * Cn * 16))
    return loss, loss_rows, dlogits


class _SoftCeFn(torch.autograd.Function):
    @staticmethod
    @_fwd_f32
    def forward(ctx, logits, y, y2, w, label_smoothing):
        loss, _, dlogits = soft_ce(logits, y, y2, w, label_smoothing)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    @_bwd
    def backward(ctx, grad_output):
        dlogits, = ctx.saved_tensors
        return dlogits * grad_output, None, None, None, None


def soft_cross_entropy(logits: torch.Tensor, y: torch.Tensor, y2: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None,
                       label_smoothing: float = 0.0) -> torch.Tensor:
    """Mean cross-entropy of logits [B, C] against the soft targets t = (1 - eps) (w onehot(y) + (1 - w) onehot(y2)) + eps / C (eps =
    label_smoothing; y2 and w absent: plain or smoothed cross-entropy), as torch's cross_entropy with probability targets gives it.
    The forward launch computes the gradient (softmax - t) / B as well and keeps it: backward is one element-wise multiply by the
    upstream gradient, with no second pass over the logits.  A row with a label outside [0, C) contributes 0 to the sum (the divisor
    stays B) and gets a zero gradient."""
    return _SoftCeFn.apply(logits, y, y2, w, float(label_smoothing))


# ---------------------------------------------------------------------------------------------------------------------------
# masked-patch reconstruction loss of a masked autoencoder: targets out of NCHW, loss and gradient in one pass (csrc/mae.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def mae_loss_rows(pred: torch.Tensor, images: torch.Tensor, idx: torch.Tensor, n_patches: int, norm_pix: bool = True):
    """The kernel call behind mae_loss, without autograd: (loss float32 [], rows float32 [B, P], dpred float32 [B, P + 1, I]) for pred
    float32 [B, P + 1, I] contiguous (the class row in place: skipped), images float32 [B, C, H, W] contiguous at any 4-byte address
    and idx int32 [B, K] as patch_keep writes it (semantics: include/kanvit.h).  One launch plus the one-work-group mean; no host
    synchronisation."""
    who = "mae_loss"
    for name, t in (("pred", pred), ("images", images), ("idx", idx)):
        if not torch.is_tensor(t):
            raise KanvitOperandError(f"{who}: {name} is a tensor on the GPU")
    if images.dim() != 4 or pred.dim() != 3 or idx.dim() != 2:
        raise KanvitOperandError(f"{who}: pred is [B, P + 1, I], images [B, C, H, W] and idx [B, K]; got shapes {tuple(pred.shape)}, "
                                 f"{tuple(images.shape)}, {tuple(idx.shape)}")
    B, Cc, H, W = images.shape
    n = int(n_patches)
    if n < 1 or H % n or W % n:
        raise KanvitOperandError(f"{who}: n_patches={n} must divide H={H} and W={W}")
    P, I, K = n * n, Cc * (H // n) * (W // n), idx.shape[1]
    if B < 1 or not 1 <= K < P:
        raise KanvitOperandError(f"{who}: B={B}, K={K} kept of P={P} patches: B >= 1 and 1 <= K < P (at least one masked patch)")
    if I > _lib.MAE_MAX_I or (norm_pix and I < 2):
        raise KanvitOperandError(f"{who}: I={I} values per patch: {2 if norm_pix else 1}..{_lib.MAE_MAX_I} (a wave holds one patch in registers)")
    _require_tensor(who, "pred", pred, torch.float32, shape=(B, P + 1, I), hint=" (the caller hands the loss pred.float())", error=KanvitOperandError)
    _require_tensor(who, "images", images, torch.float32, device=pred.device, error=KanvitOperandError)
    _require_tensor(who, "idx", idx, torch.int32, shape=(B, K), device=pred.device, error=KanvitOperandError)
    out = torch.empty((B * (P + 1) * I + B * P + 1,), device=pred.device, dtype=torch.float32)
    dpred, rows, loss = out[:B * (P + 1) * I].view(B, P + 1, I), out[B * (P + 1) * I:-1].view(B, P), out[-1:].view(())
    pd = _lib.PatchDesc(Cc, H, W, n, 0, 0)
    _launch(_lib.lib().kanvit_mae_loss, "kanvit_mae_loss", pred.device, C.byref(pd), B, K, _ptr(idx), _ptr(images), _ptr(pred),
            1 if norm_pix else 0, _ptr(rows), _ptr(loss), _ptr(dpred), tag="mae_loss", cost=(0, 4 * I * B * (3 * P - 2 * K + 1)))
    return loss, rows, dpred


class _MaeLossFn(torch.autograd.Function):
    @staticmethod
    @_fwd_f32
    def forward(ctx, pred, images, idx, n_patches, norm_pix):
        loss, _, dpred = mae_loss_rows(pred, images, idx, n_patches, norm_pix)
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    @_bwd
    def backward(ctx, grad_output):
        dpred, = ctx.saved_tensors
        return dpred * grad_output, None, None, None, None


def mae_loss(pred: torch.Tensor, images: torch.Tensor, idx: torch.Tensor, n_patches: int, norm_pix: bool = True) -> torch.Tensor:
    """The masked autoencoder's reconstruction loss (He et al. 2022): the mean over the dropped patches of the mean squared error between
    pred[b, 1 + p] and the patch p of images[b], flattened in patchify's (C, ph, pw) order and, with norm_pix, normalised by its own mean
    and unbiased variance ((t - mean) / sqrt(var + 1e-6), MAE's norm_pix_loss).  pred: float32 [B, P + 1, I] contiguous, the decoder
    head's output with its class row still in place (skipped: no slice copy); images: float32 [B, C, H, W] contiguous -- data, no
    gradient; idx: int32 [B, K] as patch_keep writes it, the KEPT patches.  The forward launch reads every dropped patch once, straight
    from the images, computes the gradient 2 (pred - target) / (I B (P - K)) as well (+0 in the kept rows and the class row) and keeps
    it: backward is one element-wise multiply by the upstream gradient.  Returns the 0-d loss."""
    if torch.is_tensor(images) and images.requires_grad:
        raise KanvitOperandError("mae_loss: images that want a gradient are not supported: the targets are data")
    return _MaeLossFn.apply(pred, images, idx, int(n_patches), bool(norm_pix))


# ---------------------------------------------------------------------------------------------------------------------------
# epoch metrics on the device (kanvit/metrics.py; csrc/metrics.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def metrics_update(logits: torch.Tensor, labels: torch.Tensor, n0: int, probs_t: torch.Tensor, labels_out: torch.Tensor,
                   preds_out: torch.Tensor, confusion: torch.Tensor) -> None:
    """One step's rows into the epoch-metrics state, in one launch on the current stream (semantics: include/kanvit.h): the fp32
    softmax of logits [B, C] (float32 or bfloat16, unit column stride; a padded row stride is taken as it is) goes class-major to
    probs_t [C, cap] at columns n0 .. n0 + B - 1, labels (int64 [B]) and the first argmax to labels_out / preds_out (int32 [cap]),
    and confusion (int64 [C, C]) gains one count per row.  A row whose label is outside [0, C) is stored with label -1 and counted
    nowhere.  No host synchronisation."""
    who = "metrics_update"
    B, Cn = _logits_2d(who, logits, (torch.float32, torch.bfloat16))
    cap = int(probs_t.shape[1]) if probs_t.dim() == 2 else -1
    _require_tensor(who, "labels", labels, torch.int64, (B,), logits.device)
    _require_tensor(who, "probs_t", probs_t, torch.float32, (Cn, cap), logits.device)
    _require_tensor(who, "labels_out", labels_out, torch.int32, (cap,), logits.device)
    _require_tensor(who, "preds_out", preds_out, torch.int32, (cap,), logits.device)
    _require_tensor(who, "confusion", confusion, torch.int64, (Cn, Cn), logits.device)
    if n0 < 0 or n0 + B > cap:
        raise KanvitError(f"{who}: rows {n0} .. {n0 + B - 1} do not fit the capacity {cap}")
    _launch(_lib.lib().kanvit_metrics_update, "kanvit_metrics_update", logits.device, _ptr(logits), int(logits.dtype == torch.bfloat16),
            int(logits.stride(0)), _ptr(labels), B, Cn, int(n0), cap, _ptr(probs_t), _ptr(labels_out), _ptr(preds_out), _ptr(confusion),
            tag="metrics_update", cost=(0, B * Cn * (logits.element_size() + 4)))


def metrics_auc_pairs(probs_t: torch.Tensor, labels: torch.Tensor, n: int, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The Mann-Whitney pair counts of the one-vs-rest ROC-AUC over the first n slots of the epoch-metrics state: counts[c] =
    (gt_c, eq_c), int64 [C, 2] (include/kanvit.h), written into `counts` when given.  probs_t float32 [C, cap] class-major, labels
    int32 [cap] (-1 = a dropped row).  n * n compares in all; no host synchronisation."""
    who = "metrics_auc_pairs"
    _require_tensor(who, "probs_t", probs_t, torch.float32)
    if probs_t.dim() != 2:
        raise KanvitError(f"{who}: probs_t has shape {tuple(probs_t.shape)}, expected [C, cap]")
    Cn, cap = (int(v) for v in probs_t.shape)
    _require_tensor(who, "labels", labels, torch.int32, (cap,), probs_t.device)
    if counts is None:
        counts = torch.empty((Cn, 2), device=probs_t.device, dtype=torch.int64)
    _require_tensor(who, "counts", counts, torch.int64, (Cn, 2), probs_t.device)
    n = int(n)
    if n < 1 or n > cap or Cn < 2:
        raise KanvitError(f"{who}: n = {n} of capacity {cap}, C = {Cn}: at least one sample, at most the capacity, at least two classes")
    L = _lib.lib()
    _launch(L.kanvit_metrics_auc_pairs, "kanvit_metrics_auc_pairs", probs_t.device, _ptr(probs_t), _ptr(labels), n, Cn, cap, _ptr(counts),
            query=(L.kanvit_metrics_auc_pairs_workspace, n, Cn), tag="metrics_auc", cost=(0, 4 * n * Cn))
    return counts


# ---------------------------------------------------------------------------------------------------------------------------
# fused AdamW step: global-norm clipping, schedule table, weight EMA (kanvit/optim.py; csrc/optim.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def _optim_ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def optim_max_tensors() -> int:
    """Tensors one optimizer launch takes in its kernel arguments (KANVIT_OPTIM_MAX_TENSORS)."""
    return int(_lib.lib().kanvit_optim_max_tensors())


def optim_grad_sumsq(grads, partials: torch.Tensor) -> int:
    """The float64 partial sums of squares of the float32 tensors `grads` into partials (float64, one entry per chunk of
    _lib.OPTIM_CHUNK elements, tensor after tensor; semantics: include/kanvit.h): ceil(len(grads) / optim_max_tensors()) launches, no
    atomics, no host synchronisation.  Returns the number of partials written; optim_begin adds them up."""
    who = "optim_grad_sumsq"
    _require_tensor(who, "partials", partials, torch.float64, (partials.numel(),))
    grads = list(grads)
    for k, g in enumerate(grads):
        _require_tensor(who, f"grads[{k}]", g, torch.float32, None, partials.device)
    L, done, cap = _lib.lib(), 0, optim_max_tensors()
    for lo in range(0, len(grads), cap):
        part = grads[lo:lo + cap]
        numel = (C.c_int64 * len(part))(*[g.numel() for g in part])
        need = int(L.kanvit_optim_sumsq_workspace(len(part), numel)) // 8
        if done + need > partials.numel():
            raise KanvitError(f"{who}: partials holds {partials.numel()} entries, {done + need} needed so far")
        if need:
            _launch(L.kanvit_optim_sumsq, "kanvit_optim_sumsq", partials.device, len(part), _optim_ptrs(part), numel,
                    C.c_void_p(partials.data_ptr() + 8 * done), C.c_size_t(8 * need), tag="optim_sumsq", cost=(0, 4 * sum(g.numel() for g in part)))
        done += need
    return done


def optim_begin(partials: Optional[torch.Tensor], n_partials: int, max_norm: float, step: torch.Tensor, norm_coef: torch.Tensor) -> None:
    """Open an optimizer step in one one-work-group launch (include/kanvit.h): norm_coef (float32 [2]) = (global gradient norm from the
    first n_partials of optim_grad_sumsq's partials, clip coefficient min(1, max_norm / (norm + 1e-6)) evaluated in float64; max_norm
    <= 0: no clipping, the coefficient is 1), and step (int64 [1]) += 1.  partials = None: the norm is not taken (NaN)."""
    who = "optim_begin"
    _require_tensor(who, "step", step, torch.int64, (1,))
    _require_tensor(who, "norm_coef", norm_coef, torch.float32, (2,), step.device)
    if partials is not None:
        _require_tensor(who, "partials", partials, torch.float64, (partials.numel(),), step.device)
        if not 0 <= int(n_partials) <= partials.numel():
            raise KanvitError(f"{who}: n_partials = {n_partials} of {partials.numel()} entries")
    elif n_partials:
        raise KanvitError(f"{who}: n_partials = {n_partials} without partials")
    _launch(_lib.lib().kanvit_optim_begin, "kanvit_optim_begin", step.device, _ptr(partials), int(n_partials), C.c_double(float(max_norm)),
            _ptr(step), _ptr(norm_coef), tag="optim_begin")


def optim_adamw(params, grads, offsets, decay, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, ema: Optional[torch.Tensor],
                table: torch.Tensor, step: torch.Tensor, norm_coef: Optional[torch.Tensor], has_wd: bool, consts) -> None:
    """The fused AdamW update of the float32 tensors `params` from `grads` (include/kanvit.h states the fp32 sequence): tensor k's
    moments are exp_avg / exp_avg_sq [offsets[k] : offsets[k] + numel], its weight EMA the same slice of `ema` (None: no EMA), it is
    decayed where decay[k] and has_wd; the step's coefficients are row min(step, T) - 1 of table (float32 [T, 4]); norm_coef (float32
    [2], from optim_begin) scales the gradients by its clip coefficient, None: no clipping.  consts = (b1, 1 - b1, b2, 1 - b2, eps, d,
    1 - d), each already rounded to float32.  ceil(len(params) / optim_max_tensors()) launches; no host synchronisation."""
    who = "optim_adamw"
    params, grads = list(params), list(grads)
    if not (len(params) == len(grads) == len(offsets) == len(decay)):
        raise KanvitError(f"{who}: {len(params)} params, {len(grads)} grads, {len(offsets)} offsets, {len(decay)} decay flags")
    _require_tensor(who, "exp_avg", exp_avg, torch.float32, (exp_avg.numel(),))
    dev, S = exp_avg.device, exp_avg.numel()
    for name, t in (("exp_avg_sq", exp_avg_sq), ("ema", ema)):
        if t is not None:
            _require_tensor(who, name, t, torch.float32, (S,), dev)
    if table.dim() != 2 or table.shape[1] != 4 or table.shape[0] < 1:
        raise KanvitError(f"{who}: table has shape {tuple(table.shape)}, expected [T, 4]")
    _require_tensor(who, "table", table, torch.float32, None, dev)
    _require_tensor(who, "step", step, torch.int64, (1,), dev)
    if norm_coef is not None:
        _require_tensor(who, "norm_coef", norm_coef, torch.float32, (2,), dev)
    for k, (p, g) in enumerate(zip(params, grads)):
        _require_tensor(who, f"params[{k}]", p, torch.float32, None, dev)
        _require_tensor(who, f"grads[{k}]", g, torch.float32, None, dev)
        if g.numel() != p.numel():
            raise KanvitError(f"{who}: grads[{k}] has {g.numel()} elements, params[{k}] {p.numel()}")
    if len(consts) != 7:
        raise KanvitError(f"{who}: consts = (b1, 1 - b1, b2, 1 - b2, eps, d, 1 - d)")
    L, cap = _lib.lib(), optim_max_tensors()
    for lo in range(0, len(params), cap):
        ps, gs = params[lo:lo + cap], grads[lo:lo + cap]
        n = len(ps)
        moved = sum(p.numel() for p in ps)
        _launch(L.kanvit_optim_adamw, "kanvit_optim_adamw", dev, n, _optim_ptrs(ps), _optim_ptrs(gs), (C.c_int64 * n)(*offsets[lo:lo + cap]),
                (C.c_int64 * n)(*[p.numel() for p in ps]), (C.c_int32 * n)(*[int(bool(f)) for f in decay[lo:lo + cap]]), _ptr(exp_avg),
                _ptr(exp_avg_sq), _ptr(ema), S, _ptr(table), int(table.shape[0]), _ptr(step), _ptr(norm_coef), int(bool(has_wd)),
                *[C.c_float(float(c)) for c in consts], tag="optim_adamw", cost=(0, moved * (36 if ema is not None else 28)))


# ---------------------------------------------------------------------------------------------------------------------------
# KAN edge pruning: ranked edge masks, held at zero (csrc/edge_prune.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def _prune_mode(who: str, mode) -> int:
    if isinstance(mode, str):
        if mode not in _lib.PRUNE_MODES:
            raise KanvitError(f"{who}: mode {mode!r} is none of {', '.join(_lib.PRUNE_MODES)}")
        return _lib.PRUNE_MODES[mode]
    return int(mode)


def edge_select(A: torch.Tensor, mode, value) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mask, kept) of the score table A (float32 [groups, ...]: every group's E entries in edge_l1's flat order, e = i * O + o):
    mask is uint8 of A's shape, 1 = keep, and kept int64 [groups] counts its ones (kanvit_edge_select; the exact total order --
    key = bits & 0x7fffffff, ties by ascending e -- is stated in include/kanvit.h and restated by edge_select_ref below).  mode
    'count': `value` = n_prune, exactly the n_prune smallest entries of every group go (0 <= n_prune <= E - 1); 'abs': the entries
    below the threshold `value` go; 'rel': those below fmul(value, the group's maximum), 0 <= value <= 1.  One launch, one
    work-group per group, no host synchronisation; capturable; bitwise reproducible."""
    who = "edge_select"
    if A.dim() < 1:
        raise KanvitError(f"{who}: A is a float32 [groups, ...] tensor, got a 0-d one")
    _require_tensor(who, "A", A, torch.float32)
    m = _prune_mode(who, mode)
    groups = A.shape[0]
    mask = torch.empty(A.shape, dtype=torch.uint8, device=A.device)
    kept = torch.empty(groups, dtype=torch.int64, device=A.device)
    if groups == 0:
        return mask, kept
    E = A.numel() // groups
    count = m == _lib.PRUNE_COUNT
    _launch(_lib.lib().kanvit_edge_select, "kanvit_edge_select", A.device, _ptr(A), groups, E, m, C.c_float(0.0 if count else float(value)),
            int(value) if count else 0, _ptr(mask), _ptr(kept), tag="edge_select", cost=(0, groups * E * 5))
    return mask, kept


def _edge_keys(a):
    import numpy as np
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def edge_select_ref(A, mode, value):
    """edge_select restated in NumPy on the CPU (the tests compare the kernel with it bit for bit): A is an array-like
    [groups, ...]; 'count' is a STABLE argsort of the uint32 keys, whose first n_prune indices go."""
    import numpy as np
    a = np.ascontiguousarray(A.detach().cpu().numpy() if torch.is_tensor(A) else A, dtype=np.float32)
    groups = a.shape[0]
    keys = _edge_keys(a).reshape(groups, -1)
    E = keys.shape[1] if groups else 0
    m = _prune_mode("edge_select_ref", mode)
    mask = np.ones((groups, E), dtype=np.uint8)
    if m == _lib.PRUNE_COUNT:
        n = int(value)
        if not 0 <= n <= E - 1:
            raise KanvitError(f"edge_select_ref: n_prune={n} must be in 0..E-1={E - 1}")
        for g in range(groups):
            mask[g, np.argsort(keys[g], kind="stable")[:n]] = 0
    else:
        t = np.float32(value)
        if not (t >= 0 and np.isfinite(t)) or (m == _lib.PRUNE_REL and t > 1):
            raise KanvitError(f"edge_select_ref: threshold={value} out of range")
        for g in range(groups):
            if m == _lib.PRUNE_REL:
                tg = np.float32(t * keys[g].max().reshape(1).view(np.float32)[0])       # ONE fp32 rounding
            else:
                tg = t
            mask[g] = keys[g] >= _edge_keys(np.array([tg], dtype=np.float32))[0]
    return mask.reshape(a.shape), mask.sum(axis=1, dtype=np.int64)


def mask_max_tensors() -> int:
    """Tensors one kanvit_mask_rows launch takes in its kernel arguments (KANVIT_MASK_MAX_TENSORS)."""
    return int(_lib.lib().kanvit_mask_max_tensors())


def mask_rows(tensors, masks, runs) -> None:
    """In place, for every k: tensors[k] (float32, contiguous, numel = rows * runs[k]) keeps row r of runs[k] consecutive elements
    where masks[k].flatten()[r] != 0 and becomes +0.0 elsewhere (kanvit_mask_rows: a select -- kept elements keep their bits, a
    masked NaN, infinity or -0 becomes +0; mask_rows_ref restates it).  masks[k] is uint8 with rows entries; one mask may serve
    several tensors.  ceil(len(tensors) / mask_max_tensors()) launches; no host synchronisation; capturable."""
    who = "mask_rows"
    tensors, masks, runs = list(tensors), list(masks), [int(r) for r in runs]
    if not (len(tensors) == len(masks) == len(runs)):
        raise KanvitError(f"{who}: {len(tensors)} tensors, {len(masks)} masks, {len(runs)} runs")
    if not tensors:
        return
    dev = tensors[0].device
    for k, (x, m, r) in enumerate(zip(tensors, masks, runs)):
        _require_tensor(who, f"tensors[{k}]", x, torch.float32, None, dev)
        _require_tensor(who, f"masks[{k}]", m, torch.uint8, None, dev)
        if r < 1 or x.numel() != m.numel() * r:
            raise KanvitError(f"{who}: tensors[{k}] has {x.numel()} elements, masks[{k}] {m.numel()} rows of run {r}")
    L, cap = _lib.lib(), mask_max_tensors()
    for lo in range(0, len(tensors), cap):
        xs, ms, rs = tensors[lo:lo + cap], masks[lo:lo + cap], runs[lo:lo + cap]
        n = len(xs)
        moved = sum(m.numel() for m in ms) + 4 * sum(x.numel() for x in xs)
        _launch(L.kanvit_mask_rows, "kanvit_mask_rows", dev, n, _optim_ptrs(xs), (C.c_int64 * n)(*[x.numel() for x in xs]),
                (C.c_int64 * n)(*rs), _optim_ptrs(ms), tag="mask_rows", cost=(0, moved))


def mask_rows_ref(x, mask, run: int):
    """mask_rows restated in NumPy for ONE tensor: a new float32 array of x's shape (x array-like or a tensor), bit for bit."""
    import numpy as np
    a = np.array(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32, copy=True)
    m = np.asarray(mask.detach().cpu().numpy() if torch.is_tensor(mask) else mask).reshape(-1)
    rows = a.reshape(-1, int(run)) if a.size else a.reshape(0, int(run))
    rows.view(np.uint32)[m == 0] = 0
    return rows.reshape(a.shape)
