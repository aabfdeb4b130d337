"""Epoch metrics on the device: the four numbers train.py logs (accuracy, balanced accuracy, weighted F1, one-vs-rest weighted
ROC-AUC; the reference's utils.calculate_metrics, utils.py:13-47) from small integer tables instead of scikit-learn on host copies.

Every step, one kernel (ops.metrics_update) takes the softmax and the argmax of the step's logits, stores the probabilities
class-major and counts the row in the C x C confusion matrix.  At the end of the epoch the pair kernel (ops.metrics_auc_pairs) counts,
per class c, the (positive, negative) pairs whose positive has the greater / an equal p[., c]; C * C + 2 * C integers go to the host
in one copy and metrics_from_counts turns them into the four numbers with scikit-learn's conventions.  Integer sums: exact, and the
same whatever the order of the atomic adds or the batch sizes the epoch was fed in.

The pair counts cost n * n compares per epoch (n the samples of the epoch, whatever C is): right for CIFAR-sized epochs (50 000
samples: 2.5e9 compares), not for ImageNet-sized ones, which want a sort-based form that is not built here."""
import numpy as np
import torch

from . import ops
from ._lib import KanvitError


def metrics_from_counts(confusion, gt, eq):
    """(accuracy, balanced accuracy, weighted F1, weighted one-vs-rest ROC-AUC) as float64 from integer tables, host only:
    confusion [C, C] (rows = true class), gt / eq [C] the Mann-Whitney pair counts of every class against the rest.

    scikit-learn's conventions: balanced accuracy averages the recall over the classes that have support; the F1 of a class with
    2 tp + fp + fn = 0 is 0; F1 and AUC are weighted by the supports; the AUC is nan when any class has no positive or no negative
    (roc_auc_score raises there and utils.calculate_metrics answers nan; scikit-learn releases that only warn about an absent class
    and give it weight 0 answer a number instead -- this function stays with nan whatever scikit-learn is installed)."""
    cm = np.asarray(confusion)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or cm.dtype.kind not in "iu":
        raise ValueError(f"confusion is {cm.dtype} {cm.shape}, expected a square integer matrix")
    C = cm.shape[0]
    gt, eq = np.asarray(gt), np.asarray(eq)
    if gt.shape != (C,) or eq.shape != (C,) or gt.dtype.kind not in "iu" or eq.dtype.kind not in "iu":
        raise ValueError(f"gt {gt.dtype} {gt.shape}, eq {eq.dtype} {eq.shape}: expected integer vectors of length {C}")
    cm = cm.astype(np.int64)
    tp = np.diag(cm)
    support = cm.sum(axis=1)
    predicted = cm.sum(axis=0)
    n = int(support.sum())
    if n == 0:
        return float("nan"), float("nan"), float("nan"), float("nan")
    has = support > 0
    acc = float(tp.sum() / n)
    bal = float(np.mean(tp[has] / support[has]))
    denom = support + predicted                      # 2 tp + fp + fn
    f1_c = np.divide(2.0 * tp, denom, out=np.zeros(C, dtype=np.float64), where=denom > 0)
    f1 = float(np.sum(f1_c * support) / n)
    negatives = n - support
    if np.any(support == 0) or np.any(negatives == 0):
        auc = float("nan")
    else:
        # (2 gt + eq) stays an exact integer (below 2^63 for every n the pair kernel accepts); one rounding in the division
        auc_c = (2 * gt.astype(np.int64) + eq.astype(np.int64)) / (2.0 * support * negatives)
        auc = float(np.sum(auc_c * support) / n)
    return acc, bal, f1, auc


class EpochMetrics:
    """The state of one epoch's metrics on `device`: probabilities class-major [C, capacity], labels and predictions [capacity], the
    confusion matrix and the pair counts.  update() per step (one launch, no host synchronisation), compute() per epoch (the pair
    kernel and one copy to the host), reset() before the next epoch.  The host keeps the fill count."""

    def __init__(self, num_classes: int, capacity: int, device):
        C, cap = int(num_classes), int(capacity)
        if C < 2 or cap < 1:
            raise ValueError(f"EpochMetrics(num_classes={num_classes}, capacity={capacity}): at least two classes and one sample")
        device = torch.device(device)
        if device.type != "cuda":
            raise KanvitError(f"EpochMetrics on {device}: the kanvit ops run only on an AMD GPU (no CPU fallback)")
        self.num_classes, self.capacity, self.device = C, cap, device
        self.n = 0
        self._probs_t = torch.empty((C, cap), device=device, dtype=torch.float32)
        self._labels = torch.empty((cap,), device=device, dtype=torch.int32)
        self._preds = torch.empty((cap,), device=device, dtype=torch.int32)
        self._tables = torch.zeros((C * C + 2 * C,), device=device, dtype=torch.int64)      # confusion | counts: one copy to the host
        self.confusion = self._tables[:C * C].view(C, C)
        self.counts = self._tables[C * C:].view(C, 2)

    def update(self, logits: torch.Tensor, y: torch.Tensor) -> None:
        """Add the rows of one step: logits [B, C] float32 or bfloat16, y int64 [B]."""
        B = int(logits.shape[0])
        if self.n + B > self.capacity:
            raise KanvitError(f"EpochMetrics.update: {self.n} + {B} rows exceed the capacity {self.capacity}")
        ops.metrics_update(logits, y, self.n, self._probs_t, self._labels, self._preds, self.confusion)
        self.n += B

    def compute(self):
        """(accuracy, balanced accuracy, weighted F1, ROC-AUC) of the rows fed since the last reset()."""
        if self.n == 0:
            raise KanvitError("EpochMetrics.compute: no rows since the last reset()")
        ops.metrics_auc_pairs(self._probs_t, self._labels, self.n, counts=self.counts)
        C = self.num_classes
        host = self._tables.cpu().numpy()
        counts = host[C * C:].reshape(C, 2)
        return metrics_from_counts(host[:C * C].reshape(C, C), counts[:, 0], counts[:, 1])

    def reset(self) -> None:
        self.n = 0
        self._tables.zero_()

    def probs(self) -> torch.Tensor:
        """The stored probabilities as an [n, C] view (row i = sample i)."""
        return self._probs_t[:, :self.n].t()

    def labels(self) -> torch.Tensor:
        """int32 [n]; -1 marks a row whose label was outside [0, C)."""
        return self._labels[:self.n]

    def preds(self) -> torch.Tensor:
        return self._preds[:self.n]
