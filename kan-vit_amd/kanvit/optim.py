"""KanvitAdamW: the optimizer half of the DeiT / timm recipe in the project's own kernels (csrc/optim.hip, include/kanvit.h).

One step is: the gradients' sum of squares (only when clipping is on), one one-work-group launch that turns it into the global norm
and the clip coefficient and counts the step, and one multi-tensor update that clips, decays, runs AdamW with the step's learning
rate and moves the weight EMA -- one pass over the gradients for the norm, one pass over everything for the update, no host
synchronisation, capturable in a HIP graph.  Everything that depends on the step number comes from a table the host computes once in
float64 (step_table); the kernel's fp32 operations are a fixed, uncontracted sequence, so a NumPy float32 restatement of it equals
the device bit for bit (tests/_optim_ref.py).

The one difference from torch.optim.AdamW's bookkeeping: there is ONE step counter.  A parameter whose .grad is None is left alone --
weights, moments and EMA -- while the global step still advances, so its bias corrections follow the global step, not its own age.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Iterable, Optional

import numpy as np
import torch

from . import _lib, ops
from ._lib import KanvitError

SCHEDULES = ("constant", "cosine")


def step_table(total_steps: int, lr: float, betas=(0.9, 0.999), weight_decay: float = 0.0, warmup_steps: int = 0,
               schedule: str = "constant", min_lr: float = 0.0, ema_decay: float = 0.0) -> np.ndarray:
    """The per-step coefficients of KanvitAdamW, float32 [total_steps, 4], computed in float64 and rounded once: row t - 1 (the
    t-th step, t = 1 ..) is
        (1 - lr_t * weight_decay,  lr_t / (1 - beta1^t),  sqrt(1 - beta2^t),  1 - ema_decay^t)
    with lr_t = lr * t / warmup_steps for t <= warmup_steps (linear warm-up from lr / warmup_steps to lr), and after it lr
    ("constant") or min_lr + (lr - min_lr) (1 + cos(pi (t - warmup_steps) / (total_steps - warmup_steps))) / 2 ("cosine": from lr at
    the end of the warm-up to min_lr at the last step).  A step beyond the table uses its last row."""
    T, W = int(total_steps), int(warmup_steps)
    if T < 1:
        raise ValueError(f"total_steps={total_steps}: the table has at least one row")
    if not 0 <= W <= T:
        raise ValueError(f"warmup_steps={warmup_steps} must be in 0..total_steps={T}")
    if schedule not in SCHEDULES:
        raise ValueError(f"schedule={schedule!r}: expected one of {SCHEDULES}")
    b1, b2 = (float(b) for b in betas)
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"betas={betas} must be in [0, 1)")
    if not 0.0 <= float(ema_decay) < 1.0:
        raise ValueError(f"ema_decay={ema_decay} must be in [0, 1)")
    if not (float(lr) >= 0.0 and float(min_lr) >= 0.0 and float(weight_decay) >= 0.0):
        raise ValueError(f"lr={lr}, min_lr={min_lr}, weight_decay={weight_decay}: none is negative")
    t = np.arange(1, T + 1, dtype=np.float64)
    lr_t = np.full(T, float(lr), dtype=np.float64)
    if schedule == "cosine" and T > W:
        lr_t = float(min_lr) + (float(lr) - float(min_lr)) * 0.5 * (1.0 + np.cos(np.pi * (t - W) / (T - W)))
    if W > 0:
        lr_t = np.where(t <= W, float(lr) * t / W, lr_t)
    table = np.stack([1.0 - lr_t * float(weight_decay), lr_t / (1.0 - b1 ** t), np.sqrt(1.0 - b2 ** t), 1.0 - float(ema_decay) ** t], axis=1)
    return table.astype(np.float32)


def rounded_constants(betas, eps: float, ema_decay: float):
    """(b1, 1 - b1, b2, 1 - b2, eps, d, 1 - d) as the kernel takes them: each computed in float64 and rounded to float32 once."""
    b1, b2, d = float(betas[0]), float(betas[1]), float(ema_decay)
    return tuple(float(np.float32(c)) for c in (b1, 1.0 - b1, b2, 1.0 - b2, float(eps), d, 1.0 - d))


def default_decay_filter(p: torch.Tensor) -> bool:
    """timm's rule: only weight matrices are decayed.  A tensor that is a vector up to leading dimensions of size 1 is not: biases and
    LayerNorm parameters ([d]), the class token ([1, d]), the [1, out] biases and [1, 1, 1, G] frequencies of the Sine / Fourier layers."""
    return p.ndim > 1 and p.numel() != p.shape[-1]


class KanvitAdamW(torch.optim.Optimizer):
    """AdamW with global-norm gradient clipping, a learning-rate schedule and a weight EMA, fused into the kanvit optimizer kernels.

    params            an iterable of float32 CUDA tensors (one parameter group); those with requires_grad=False are left out
    lr, betas, eps, weight_decay   as torch.optim.AdamW (decoupled decay p *= 1 - lr_t * weight_decay).  lr, weight_decay and the schedule
                      arguments only build the table: once it exists (or with table=) the table alone drives the step, and the values
                      kept in param_groups are a record -- changing them changes nothing
    max_grad_norm     None: no clipping (grad_norm then reads NaN: the norm is not taken); a float: clip_grad_norm_'s rule over ALL the
                      gradients of the step; float("inf") takes the norm without ever clipping
    ema_decay         d > 0: e = d e + (1 - d) p after every update, e starting at ZERO and debiased on read (ema_weights):
                      weights = e / (1 - d^t), as Adam debiases its own moments
    table             a step_table (float32 [T, 4]), or total_steps with warmup_steps / schedule / min_lr to build one
    decay_filter      callable(p) -> bool: which tensors are decayed; default: default_decay_filter (matrices, not vectors or [1, d] rows).
                      Whether anything is decayed at all is read off the table: a first column of all ones skips the multiply

    All state lives in self.state["flat"]: exp_avg, exp_avg_sq, ema (with ema_decay > 0) -- flat float32 buffers in which parameter k
    owns the slice that starts at a multiple of four elements --, step (int64 [1]), norm_coef (float32 [2]: the last step's gradient
    norm and clip coefficient) and the float64 workspace of the norm.  A state of all zeros is exactly a fresh optimizer; the table is
    not state.  state_dict() / load_state_dict() carry it as they carry any optimizer's."""

    def __init__(self, params: Iterable[torch.Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = None, ema_decay: float = 0.0, table=None, total_steps: Optional[int] = None,
                 warmup_steps: int = 0, schedule: str = "constant", min_lr: float = 0.0,
                 decay_filter: Optional[Callable[[torch.Tensor], bool]] = None):
        params = list(params)
        if any(isinstance(p, dict) for p in params):
            raise KanvitError("KanvitAdamW: one parameter group (one table drives every tensor); choose what is decayed with decay_filter=")
        params = [p for p in params if p.requires_grad]
        if not params:
            raise KanvitError("KanvitAdamW: no parameter requires a gradient")
        for k, p in enumerate(params):
            ops._require_tensor("KanvitAdamW", f"params[{k}]", p, torch.float32, None, params[0].device)
        if (table is None) == (total_steps is None):
            raise KanvitError("KanvitAdamW: give table= (a step_table) or total_steps= (with warmup_steps, schedule, min_lr), one of them")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise KanvitError(f"KanvitAdamW: max_grad_norm={max_grad_norm} must be positive (None: no clipping)")
        if not 0.0 <= float(ema_decay) < 1.0:
            raise KanvitError(f"KanvitAdamW: ema_decay={ema_decay} must be in [0, 1)")
        if table is None:
            table = step_table(total_steps, lr, betas, weight_decay, warmup_steps, schedule, min_lr, ema_decay)
        table = torch.as_tensor(np.asarray(table) if not torch.is_tensor(table) else table)
        if table.dim() != 2 or table.shape[1] != 4 or table.shape[0] < 1 or table.dtype != torch.float32:
            raise KanvitError(f"KanvitAdamW: table has shape {tuple(table.shape)} and dtype {table.dtype}, expected float32 [T, 4] (step_table)")
        super().__init__(params, dict(lr=float(lr), betas=tuple(betas), eps=float(eps), weight_decay=float(weight_decay),
                                      max_grad_norm=None if max_grad_norm is None else float(max_grad_norm), ema_decay=float(ema_decay)))
        dev = params[0].device
        self.table = table.to(dev).contiguous()
        self._consts = rounded_constants(betas, eps, ema_decay)
        keep = decay_filter if decay_filter is not None else default_decay_filter
        self._decay = [bool(keep(p)) for p in params]
        self._has_wd = bool((table[:, 0] != 1.0).any())         # p * 1 is p: the skipped multiply changes no bit
        self._offsets, total = [], 0
        for p in params:
            self._offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        self._numel = max(total, 4)
        chunks = sum((p.numel() + _lib.OPTIM_CHUNK - 1) // _lib.OPTIM_CHUNK for p in params)
        flat = {"exp_avg": torch.zeros(self._numel, device=dev), "exp_avg_sq": torch.zeros(self._numel, device=dev),
                "step": torch.zeros(1, device=dev, dtype=torch.int64), "norm_coef": torch.zeros(2, device=dev)}
        if float(ema_decay) > 0.0:
            flat["ema"] = torch.zeros(self._numel, device=dev)
        if max_grad_norm is not None:
            flat["sumsq"] = torch.zeros(max(chunks, 1), device=dev, dtype=torch.float64)
        self.state["flat"] = flat

    def load_state_dict(self, state_dict):
        """As torch's, but the loaded values are copied INTO this optimizer's own buffers: a captured HIP graph keeps pointing at
        them, and two optimizers never share state through a state dict that was not deep-copied."""
        own = self.state["flat"]
        super().load_state_dict(state_dict)
        loaded = self.state.get("flat", {})
        if set(loaded) != set(own) or any(loaded[k].shape != own[k].shape or loaded[k].dtype != own[k].dtype for k in own):
            self.state["flat"] = own
            raise KanvitError(f"KanvitAdamW.load_state_dict: the state holds {sorted(loaded)}, this optimizer {sorted(own)}, or a buffer has "
                              "another size: build the optimizer over the same parameters with the same max_grad_norm / ema_decay choices")
        with torch.no_grad():
            for k in own:
                own[k].copy_(loaded[k])
        self.state["flat"] = own

    # -- the pieces of the state ---------------------------------------------------------------------------------------------
    @property
    def _params(self):
        return self.param_groups[0]["params"]

    @property
    def flat(self) -> dict:
        return self.state["flat"]

    @property
    def grad_norm(self) -> torch.Tensor:
        """The last step's global gradient norm, a device scalar (NaN without max_grad_norm: the norm is not taken)."""
        return self.flat["norm_coef"][0]

    @property
    def clip_coef(self) -> torch.Tensor:
        """The last step's clip coefficient min(1, max_grad_norm / (norm + 1e-6)), a device scalar (1 without clipping)."""
        return self.flat["norm_coef"][1]

    def _index(self, p) -> int:
        for k, q in enumerate(self._params):
            if q is p:
                return k
        raise KeyError("the tensor is not one of this optimizer's parameters")

    def _slice(self, name: str, k: int) -> torch.Tensor:
        p = self._params[k]
        return self.flat[name][self._offsets[k]:self._offsets[k] + p.numel()].view(p.shape)

    def moments(self, p):
        """(exp_avg, exp_avg_sq) of parameter p, as views into the flat state."""
        k = self._index(p)
        return self._slice("exp_avg", k), self._slice("exp_avg_sq", k)

    def decayed(self, p) -> bool:
        """Whether parameter p carries the decay flag (decay_filter's answer at construction)."""
        return self._decay[self._index(p)]

    def ema(self, p) -> torch.Tensor:
        """The raw (not yet debiased) EMA of parameter p, a view into the flat state."""
        if "ema" not in self.flat:
            raise KanvitError("KanvitAdamW: no weight EMA is kept (ema_decay=0)")
        return self._slice("ema", self._index(p))

    # -- the step ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        flat, group = self.flat, self.param_groups[0]
        live = [k for k, p in enumerate(self._params) if p.grad is not None]
        params = [self._params[k] for k in live]
        grads = [p.grad for p in params]
        clip = group["max_grad_norm"] is not None
        n_partials = ops.optim_grad_sumsq(grads, flat["sumsq"]) if clip else 0
        ops.optim_begin(flat["sumsq"] if clip else None, n_partials, group["max_grad_norm"] if clip else 0.0, flat["step"], flat["norm_coef"])
        ops.optim_adamw(params, grads, [self._offsets[k] for k in live], [self._decay[k] for k in live], flat["exp_avg"], flat["exp_avg_sq"],
                        flat.get("ema"), self.table, flat["step"], flat["norm_coef"] if clip else None, self._has_wd,
                        self._consts)
        return loss

    # -- the averaged weights --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def ema_debiased(self, k: int) -> torch.Tensor:
        """The debiased EMA of parameter k, e / (1 - d^t) with the divisor from the table's row of the current step; before the first
        step, the parameter itself.  No host synchronisation.  The divisor follows the ONE global step: a parameter that got no
        gradient on some steps was not averaged on those and reads low by that share, and a trainable parameter that NEVER gets a
        gradient keeps e = 0 and reads as zeros -- freeze such a parameter (requires_grad=False) so that the optimizer leaves it out."""
        t = self.flat["step"]
        row = self.table.index_select(0, t.clamp(1, self.table.shape[0]) - 1)[0]
        return torch.where(t > 0, self._slice("ema", k) / row[3], self._params[k])

    @contextlib.contextmanager
    def ema_weights(self, model: Optional[torch.nn.Module] = None):
        """Inside the block the parameters hold the debiased EMA weights; on exit they get their own values back, bit for bit.  `model`,
        when given, is checked: every parameter of it that requires a gradient must be one of this optimizer's."""
        if "ema" not in self.flat:
            raise KanvitError("KanvitAdamW.ema_weights: no weight EMA is kept (ema_decay=0)")
        if model is not None:
            mine = {id(p) for p in self._params}
            for name, p in model.named_parameters():
                if p.requires_grad and id(p) not in mine:
                    raise KanvitError(f"KanvitAdamW.ema_weights: {name} is not one of this optimizer's parameters")
        with torch.no_grad():
            saved = [p.detach().clone() for p in self._params]
            for k, p in enumerate(self._params):
                p.copy_(self.ema_debiased(k))
        try:
            yield self
        finally:
            with torch.no_grad():
                for p, s in zip(self._params, saved):
                    p.copy_(s)
