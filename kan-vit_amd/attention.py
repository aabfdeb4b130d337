"""MSA and FlashAttention -- drop-ins for the reference's attention.py:13-202.

MSA keeps the reference's parameter layout ({q,k,v}_mappings.<head>.<layer keys>) but replaces the
python loop over samples x heads (attention.py:188-202) by two kernel launches per block: one fused
KAN launch that evaluates all 3*H per-head mappings on the batch-folded rows, and one attention
launch over every (sample, head)."""
from dataclasses import replace

import torch
from torch import nn

from kanvit import grouped, ops
from kanvit.prune import EdgePruning
from models.cheby import ChebyKANLayer
from models.effkan import KANLinear
from models.fastkan import FastKANLayer
from models.sinekan import SineKANLayer
from utils import FlashAttentionFunction, default


class FlashAttention(nn.Module):
    """Bias-free q / kv / out projections around the attention core (attention.py:13-109).
    ``parallel`` / ``mixed_precision`` are dead or broken branches in the reference (SURVEY.md
    section 2) and are rejected here instead of being imitated."""

    def __init__(self, *, dim, heads=8, dim_head=64, causal=False, q_bucket_size=512, k_bucket_size=1024,
                 parallel=False, mixed_precision=False):
        super().__init__()
        if parallel or mixed_precision:
            raise NotImplementedError("parallel / mixed_precision are not part of the accelerated path; "
                                      "data parallelism is done per process (see train.py --dp)")
        self.heads = heads
        self.causal = causal
        self.parallel = parallel
        self.mixed_precision = mixed_precision
        inner = heads * dim_head
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_kv = nn.Linear(dim, inner * 2, bias=False)
        self.to_out = nn.Linear(inner, dim, bias=False)
        self.q_bucket_size = q_bucket_size
        self.k_bucket_size = k_bucket_size

    def forward(self, x, context=None, mask=None, q_bucket_size=None, k_bucket_size=None):
        qb = default(q_bucket_size, self.q_bucket_size)
        kb = default(k_bucket_size, self.k_bucket_size)
        h = self.heads
        context = default(context, x)
        q = self.to_q(x)
        k, v = self.to_kv(context).chunk(2, dim=-1)
        b, n, _ = q.shape
        # 'b n (h d) -> b h n d' as strided views; the kernel takes the strides as they are
        q, k, v = (t.view(b, t.shape[1], h, -1).permute(0, 2, 1, 3) for t in (q, k, v))
        out = FlashAttentionFunction.apply(q, k, v, mask, self.causal, qb, kb)
        return self.to_out(out.permute(0, 2, 1, 3).reshape(b, n, -1))

    @torch.no_grad()
    def attention_map(self, x, context=None, mask=None, rows=None):
        """[B, heads, R, k_len] float32: the attention probabilities of every head for the call forward(x, context, mask) -- the
        same projections and strided views, the module's `causal`, the mask forms forward accepts -- from kanvit.ops.attention_probs
        (the fused forward never forms them).  `rows` = R keeps the first R queries (default all; 1 = the first token's row).
        Not differentiable; the softmax is exact fp32 also under autocast."""
        h = self.heads
        context = default(context, x)
        q = self.to_q(x)
        k = self.to_kv(context).chunk(2, dim=-1)[0]
        b = q.shape[0]
        q, k = (t.view(b, t.shape[1], h, -1).permute(0, 2, 1, 3) for t in (q, k))
        return ops.attention_probs(q, k, mask=mask, causal=self.causal, rows=rows)


class MSA(torch.nn.Module):
    """Multi-head self-attention with one small (KAN or linear) mapping per head and per q/k/v,
    no output projection (attention.py:112-202)."""

    def __init__(self, d, n_heads=4, type: str = "vanilla"):
        super().__init__()
        self.d = d
        self.n_heads = n_heads
        self.type = type
        assert d % n_heads == 0
        dh = d // n_heads
        makers = {
            "vanilla": lambda: nn.Linear(dh, dh),
            "flash-attn": lambda: nn.Linear(dh, dh),
            "fourier": lambda: nn.Linear(dh, dh),                       # attention.py:136: Fourier is patch-embed only
            "efficientkan": lambda: KANLinear(dh, dh),
            "fast": lambda: FastKANLayer(dh, dh),
            "sine": lambda: SineKANLayer(dh, dh, grid_size=4),
            "cheby": lambda: ChebyKANLayer(dh, dh, 4),
        }
        if type not in makers:
            # the reference prints and carries on half-built (attention.py:174-176); raise instead
            raise ValueError(f"{type} invalid. Please use a different argument.")
        make = makers[type]
        self.q_mappings = nn.ModuleList([make() for _ in range(n_heads)])
        self.k_mappings = nn.ModuleList([make() for _ in range(n_heads)])
        self.v_mappings = nn.ModuleList([make() for _ in range(n_heads)])
        self.d_head = dh
        self.softmax = nn.Softmax(dim=-1)

    REGULARIZED_TYPES = ("efficientkan", "cheby", "fast")

    def _qkv_layers(self, who=None):
        """The 3*H per-head layers in the order of the grouped launch, q | k | v.  With `who` (update_grid / extend_grid) they must
        be KANLinear layers that agree in what one grouped refit shares."""
        layers = list(self.q_mappings) + list(self.k_mappings) + list(self.v_mappings)
        l0 = layers[0]
        if who is not None:
            if not isinstance(l0, KANLinear):
                raise NotImplementedError(f"{who}: MSA type '{self.type}' has no B-spline grid to {who.split('_')[0]} "
                                          "(only 'efficientkan' has)")
            for m in layers[1:]:
                assert (m.grid_size, m.spline_order, m.grid_eps, m.enable_standalone_scale_spline) == \
                    (l0.grid_size, l0.spline_order, l0.grid_eps, l0.enable_standalone_scale_spline), \
                    f"{who}: the per-head layers of one MSA must agree in grid_size, spline_order and grid_eps"
        return layers, l0

    def _refit_operands(self, layers):
        """(packed old spline weights [g, I*nb_old, O], old knots [g, I, nk_old]) of the grouped refit launches."""
        sw = torch.stack([m.scaled_spline_weight for m in layers])                       # [g, O, I, nb_old]
        g, o, i, nb = sw.shape
        return sw.permute(0, 2, 3, 1).reshape(g, i * nb, o), torch.stack([m.grid for m in layers])

    def edge_activation_l1(self, x, include_base=False):
        """[3, H, d_head(out), d_head(in)]: the mean absolute activation of every edge of the 3*H per-head q, k and v layers on
        the rows of x [..., d] (the quantity the KAN paper regularises), from ONE grouped launch of kanvit.ops.edge_l1 with the
        packing of grouped.run_qkv.  `include_base` adds the base term of the efficient-KAN / FastKAN edge functions."""
        layers, l0 = self._qkv_layers()
        if not isinstance(l0, EdgePruning):
            raise NotImplementedError(f"edge_activation_l1: per-head layers of type {type(l0).__name__} have no edge-activation "
                                      f"statistic; supported MSA types: {', '.join(self.REGULARIZED_TYPES)}")
        H, dh = self.n_heads, self.d_head
        x2d = x.reshape(-1, self.d)
        cfg = l0.kan_cfg(layers)
        w, bp, _ = type(l0).kan_pack_grouped(layers)
        base = bool(include_base) and cfg.has_base
        if base and len({m.kan_base_act() for m in layers}) > 1:
            raise NotImplementedError("edge_activation_l1(include_base=True): one grouped launch has one base activation")
        if cfg.has_base and not base:        # spline path only: drop the base column of the packed weights
            w = w.reshape(3 * H, dh, cfg.GP, dh)[:, :, :cfg.G].reshape(3 * H, dh * cfg.G, dh)
            cfg = replace(cfg, has_base=0, base_act=0)
        xin = type(l0).kan_u_grouped(layers, x2d, H)
        if xin is None:                      # the basis reads x: every group its head's columns
            xin = x2d
            cfg = replace(cfg, groups=3 * H, x_group_mod=H)
        else:                                # every layer has its own u (FastKAN's LayerNorm): u[M, 3*H*dh], one column block per group
            if base:
                xin = torch.cat([xin, x2d.to(xin.dtype).repeat(1, 3)], dim=1)
            cfg = replace(cfg, groups=3 * H, x_group_mod=3 * H)
        A = ops.edge_l1(xin, w, cfg, bp)                       # [3*H, in, out]
        return A.view(3, H, dh, dh).transpose(-1, -2)

    def regularization_loss(self, x, regularize_activation=1.0, regularize_entropy=1.0, include_base=False):
        """Sum over the 3*H per-head layers of the L1 and entropy terms (models/effkan.py:258-264) of their sample-based edge
        magnitudes on the rows of x -- one grouped launch (edge_activation_l1)."""
        return ops.l1_entropy_loss(self.edge_activation_l1(x, include_base), regularize_activation, regularize_entropy)

    @torch.no_grad()
    def prune_edges(self, x, fraction=None, threshold=None, relative=True):
        """prune_edges (kanvit/prune.py) for all 3*H per-head q, k and v layers on the rows of x [..., d]: ONE grouped
        edge_activation_l1 launch scores the whole edge functions (the base term included where the layers have one) and ONE
        ops.edge_select launch (groups = 3*H: every layer is ranked on its own) chooses; `fraction` / `threshold` apply per layer.
        Every layer ends bit for bit as its own prune_edges on its head's slice would leave it.  Types 'efficientkan', 'cheby' and
        'fast'; others, and mixed base activations, raise edge_activation_l1's NotImplementedError.  Returns the number of kept
        edges of the 3*H layers (0-d device tensor)."""
        from kanvit import prune
        layers, _ = self._qkv_layers()
        H, dh = self.n_heads, self.d_head
        A = self.edge_activation_l1(x, include_base=True)             # [3, H, out, in], a transposed view of edge_l1's [3*H, in, out]
        mode, value = prune.select_args(dh * dh, fraction, threshold, relative)
        sel, _ = ops.edge_select(A.transpose(-1, -2).reshape(3 * H, dh * dh), mode, value)
        triples = []
        for g, m in enumerate(layers):
            m._take_selection(sel[g].view(dh, dh))
            triples += m.edge_masked()
        prune.zero_masked(triples)
        return torch.stack([m.edge_mask for m in layers]).sum()

    def edge_masked(self):
        """The (parameter, mask, run) triples of the 3*H per-head layers (kanvit/prune.py); [] for types that are not pruned."""
        layers, l0 = self._qkv_layers()
        return [t for m in layers for t in m.edge_masked()] if isinstance(l0, EdgePruning) else []

    @torch.no_grad()
    def update_grid(self, x, margin=0.01):
        """KANLinear.update_grid for all 3*H per-head q, k and v layers on the rows of x [..., d], from ONE grouped refit launch
        (groups = 3*H, x_group_mod = H, packing as edge_activation_l1).  The q, k and v layers of a head read the same columns
        with the same constructor arguments, so they share their new knots: one table per head slice.  Every layer ends bit
        for bit as its own update_grid on its head's slice would leave it.  Returns the number of (head, feature) pairs kept
        unchanged (0-d device tensor).  type='efficientkan' only."""
        layers, l0 = self._qkv_layers("update_grid")
        H, dh = self.n_heads, self.d_head
        x2d = x.reshape(-1, self.d).float()
        new_grid = KANLinear.adapted_grid(x2d, l0.grid_size, l0.spline_order, l0.grid_eps, margin).view(H, dh, -1)
        cfg = replace(l0.kan_cfg(layers), has_base=0, base_act=0, groups=3 * H, x_group_mod=H)
        w_old, grids = self._refit_operands(layers)
        w_new, ok = ops.bspline_refit(x2d, w_old, cfg, grids.reshape(3 * H, -1), new_grid)
        for g, m in enumerate(layers):
            m.apply_refit(new_grid[g % H], w_new[g], ok[g % H])
        return (~ok).sum()

    @torch.no_grad()
    def extend_grid(self, x, grid_size, margin=0.01):
        """KANLinear.extend_grid for all 3*H per-head q, k and v layers on the rows of x [..., d]: every layer moves to
        `grid_size` intervals and keeps its function.  ONE grouped launch of ops.bspline_regrid (groups = 3*H, x_group_mod = H)
        for the fit on x and one for the fit on the fallback samples; the q, k and v layers of a head share their new knots, as in
        update_grid.  The fallback span of a head slice is the smallest low and the largest high among its three layers' old
        inner spans; when the three share their old span (they do unless they were loaded from differing checkpoints) every layer
        ends bit for bit as its own extend_grid on its head's slice would leave it.  Returns the number of (head, feature) pairs
        that took the fallback (0-d device tensor).  type='efficientkan' only."""
        layers, l0 = self._qkv_layers("extend_grid")
        KANLinear.check_extension(grid_size, l0.spline_order)
        H, dh, order = self.n_heads, self.d_head, l0.spline_order
        nb_old = l0.grid_size + order
        x2d = x.reshape(-1, self.d).float()
        cfg = replace(l0.kan_cfg(layers), has_base=0, base_act=0, groups=3 * H, x_group_mod=H, G=grid_size + order)
        w_old, grids = self._refit_operands(layers)
        old = grids.reshape(3 * H, -1)
        new_grid = KANLinear.adapted_grid(x2d, grid_size, order, l0.grid_eps, margin).view(H, dh, -1)
        w_new, ok = ops.bspline_regrid(x2d, w_old, cfg, nb_old, old, new_grid)
        lo = grids[:, :, order].view(3, H * dh).min(dim=0).values
        hi = grids[:, :, -order - 1].view(3, H * dh).max(dim=0).values
        xf = KANLinear.span_samples(lo, hi, KANLinear.FALLBACK_SAMPLES)                  # [P, d]
        fb_grid = KANLinear.adapted_grid(xf, grid_size, order, l0.grid_eps, margin).view(H, dh, -1)
        w_fb, _ = ops.bspline_regrid(xf, w_old, cfg, nb_old, old, fb_grid)
        for g, m in enumerate(layers):
            m.apply_regrid(grid_size, new_grid[g % H], w_new[g], fb_grid[g % H], w_fb[g], ok[g % H])
        return (~ok).sum()

    @torch.no_grad()
    def attention_map(self, x, rows=None):
        """[B, H, R, N] float32: softmax(q k^T / sqrt(d_head)) of every head on x [B, N, d] -- what a forward hook on
        `self.softmax` collects in the reference (attention.py:199; here that module is constructed but never called, so such a
        hook does not fire).  q and k come from the same grouped q|k|v launch as forward's (under bf16 autocast: the autocast
        launch's values); the softmax on top of them is exact fp32 (kanvit.ops.attention_probs_packed, forward's scale).
        `rows` = R keeps the first R queries (default N; 1 = the class-token row).  Every MSA type.  Not differentiable."""
        b, n, d = x.shape
        qkv = grouped.run_qkv(self.q_mappings, self.k_mappings, self.v_mappings, x.reshape(b * n, d))
        return ops.attention_probs_packed(qkv.view(b, n, 3, self.n_heads, self.d_head), causal=False,
                                          scale=1.0 / (self.d_head ** 0.5), rows=rows)

    def forward(self, sequences):
        b, n, d = sequences.shape
        qkv = grouped.run_qkv(self.q_mappings, self.k_mappings, self.v_mappings, sequences.reshape(b * n, d))
        return ops.attention_packed(qkv.view(b, n, 3, self.n_heads, self.d_head), causal=False,
                                    scale=1.0 / (self.d_head ** 0.5))

    def forward_cls(self, sequences):
        """forward(sequences)[:, 0] -> [B, d], the class-token row alone (the head of a ViT reads nothing else of its last block):
        the q layers run on the B class rows, the k and v layers on all rows (two grouped launches with their own timer tags), and
        every head attends with its one query (kanvit.ops.attention_q1: exact fp32, also under autocast)."""
        b, n, d = sequences.shape
        q0 = grouped.run_projections([self.q_mappings], sequences[:, 0], tag="qcls")
        kv = grouped.run_projections([self.k_mappings, self.v_mappings], sequences.reshape(b * n, d), tag="kv")
        o = ops.attention_q1(q0.view(b, self.n_heads, self.d_head), kv.view(b, n, 2, self.n_heads, self.d_head),
                             scale=1.0 / (self.d_head ** 0.5))
        return o.view(b, d)
