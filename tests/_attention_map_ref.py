"""float64 statement of the attention probabilities (tests/test_attention_map_gpu.py): softmax(q k^T * scale) with the dead
positions of oracle.kan_oracle.attention_dead (the mask forms and the causal rule of FlashAttentionFunction) set to 0 and a query
with no live key giving an all-zero row."""
import torch

from oracle import kan_oracle as ko


def attention_probs_ref(q, k, mask=None, causal=False, scale=None):
    """q [.., Nq, D], k [.., Nk, D] (any float dtype, any device) -> float64 [.., Nq, Nk] on the CPU."""
    q, k = q.detach().double().cpu(), k.detach().double().cpu()
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    s = (q @ k.transpose(-1, -2)) * scale
    dead = ko.attention_dead(q, k, causal, None if mask is None else mask.detach().cpu())
    if dead is None:
        return torch.softmax(s, dim=-1)
    s = s.masked_fill(dead, float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    e = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m)).masked_fill(dead, 0.0)
    l = e.sum(dim=-1, keepdim=True)
    return torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))


def rollout_ref(maps, head_fusion):
    """Attention rollout in float64, written out: A_l = fuse_h maps[l]; A~_l = (A_l + I) / rowsum; A~_L ... A~_1."""
    maps = maps.detach().double().cpu()
    fuse = {"mean": lambda a: a.mean(dim=1), "max": lambda a: a.max(dim=1).values, "min": lambda a: a.min(dim=1).values}[head_fusion]
    n = maps.shape[-1]
    out = torch.eye(n, dtype=torch.float64).expand(maps.shape[1], n, n)
    for block in maps:
        a = fuse(block) + torch.eye(n, dtype=torch.float64)
        out = (a / a.sum(dim=-1, keepdim=True)) @ out
    return out
