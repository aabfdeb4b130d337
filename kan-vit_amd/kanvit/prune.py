"""KAN edge pruning on the layer side: the mask every prunable layer carries, and what is done with it.

A pruned edge is a run of exact zeros in the parameters the tuned kernels already read, so no kernel and no launch of the forward
or backward changes; what keeps it at zero through training is that its gradient, its optimizer moments and its weight EMA are
zeroed as well (kanvit.ops.mask_rows; train.py prune_and_mask).  The mask is a non-persistent uint8 buffer `edge_mask`, created
on first use, stored once in the leading layout of the layer's masked tensors and rewritten IN PLACE: a captured step keeps
pointing at it, and state_dict() keys do not change -- restore_edge_mask rebuilds it from the zeros of a loaded checkpoint."""
import torch

from . import ops


def select_args(n_edges: int, fraction, threshold, relative):
    """prune_edges' arguments as (mode, value) of ops.edge_select: exactly one of fraction (n_prune = int(fraction * n_edges),
    capped at n_edges - 1) and threshold (relative to the layer's largest score, or absolute)."""
    if (fraction is None) == (threshold is None):
        raise ValueError("prune_edges: give exactly one of fraction= and threshold=")
    if fraction is not None:
        f = float(fraction)
        if not 0.0 <= f <= 1.0:
            raise ValueError(f"prune_edges: fraction {fraction} must be in [0, 1]")
        return "count", min(int(f * n_edges), n_edges - 1)
    t = float(threshold)
    if not 0.0 <= t < float("inf") or (relative and t > 1.0):
        raise ValueError(f"prune_edges: threshold {threshold} must be finite and >= 0" + (", and <= 1 with relative=True" if relative else ""))
    return ("rel" if relative else "abs"), t


def zero_masked(triples, of=None):
    """One ops.mask_rows over (tensor, mask, run) triples; `of` maps every triple's tensor to the tensors to mask in its place (a
    gradient, optimizer moments), None entries are passed over."""
    xs, ms, rs = [], [], []
    for p, m, r in triples:
        for t in ((p,) if of is None else of(p)):
            if t is not None:
                xs.append(t.detach()), ms.append(m), rs.append(r)
    ops.mask_rows(xs, ms, rs)


class EdgePruning:
    """Mixin of KANLinear, ChebyKANLayer and FastKANLayer.  A layer states its masked tensors and scores its edges; the rest is here."""

    _edge_mask_out_in = True        # the masked tensors lead with [out, in] (False: [in, out], the layout ops.edge_select writes)

    def _edge_dims(self):
        """(in, out)"""
        raise NotImplementedError

    def _edge_tensors(self):
        """[(parameter, run)]: every parameter an edge owns `run` consecutive elements of, in the mask's row order."""
        raise NotImplementedError

    def _edge_scores(self, x):
        """[out, in]: edge_activation_l1 of the WHOLE edge function (the base term included where the layer has one)."""
        raise NotImplementedError

    def regularization_loss(self, x, regularize_activation=1.0, regularize_entropy=1.0, include_base=False):
        """The L1 and entropy terms of models/effkan.py:258-264 on edge_activation_l1(x, include_base)."""
        return ops.l1_entropy_loss(self.edge_activation_l1(x, include_base), regularize_activation, regularize_entropy)

    def _edge_mask_buffer(self):
        if getattr(self, "edge_mask", None) is None:
            i, o = self._edge_dims()
            dev = self._edge_tensors()[0][0].device
            self.register_buffer("edge_mask", torch.ones((o, i) if self._edge_mask_out_in else (i, o), dtype=torch.uint8, device=dev),
                                 persistent=False)
        return self.edge_mask

    def edge_masked(self):
        """[(parameter, mask, run)]: parameter, seen as rows of `run` elements, is held at zero where mask (uint8, one entry per row)
        is 0.  Creates the all-ones mask on first use."""
        mask = self._edge_mask_buffer()
        return [(p, mask, run) for p, run in self._edge_tensors()]

    @torch.no_grad()
    def _take_selection(self, sel):
        """AND an ops.edge_select mask ([in, out]) into edge_mask, in place."""
        self._edge_mask_buffer().bitwise_and_(sel.t() if self._edge_mask_out_in else sel)

    @torch.no_grad()
    def prune_edges(self, x, fraction=None, threshold=None, relative=True):
        """Prune the layer's weakest edges by their mean absolute activation on the rows of x (edge_activation_l1 of the whole edge
        function): `fraction` prunes exactly int(fraction * in * out) edges (at most all but the strongest), `threshold` those
        scoring below it -- times the layer's largest score with relative=True.  Exactly one of the two.  Pruned edges score 0 and
        rank first, so pruning is cumulative: `fraction` is the share of ALL edges that ends up pruned.  The choice is exact and
        reproducible (ops.edge_select: ties go by index), stays on the device, is ANDed into `edge_mask`, and the masked runs of
        the parameters become +0 (ops.mask_rows).  Returns the number of kept edges (0-d device tensor)."""
        i, o = self._edge_dims()
        mode, value = select_args(i * o, fraction, threshold, relative)
        scores = self._edge_scores(x).t().contiguous()                  # [in, out]: edge_l1's own layout
        sel, _ = ops.edge_select(scores.view(1, i * o), mode, value)
        self._take_selection(sel.view(i, o))
        zero_masked(self.edge_masked())
        return self.edge_mask.sum()

    @torch.no_grad()
    def restore_edge_mask(self):
        """Rebuild edge_mask from exact zeros: an edge is pruned iff every masked tensor is all-zero on it -- what a pruned
        checkpoint loaded into a fresh model needs to keep training sparse.  Returns the number of kept edges (0-d device tensor)."""
        mask = self._edge_mask_buffer()
        alive = None
        for p, run in self._edge_tensors():
            a = (p.detach().reshape(mask.numel(), run) != 0).any(dim=1)
            alive = a if alive is None else alive | a
        mask.copy_(alive.view(mask.shape))
        return mask.sum()
