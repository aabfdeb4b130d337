"""numpy brute force for the epoch-metrics tests: the tables the kernels of csrc/metrics.hip count, straight from their definitions."""
import numpy as np


def confusion(y_true, y_pred, C):
    """cm[t][p] = number of samples with label t predicted p; labels outside [0, C) are dropped."""
    y_true, y_pred = np.asarray(y_true).astype(np.int64), np.asarray(y_pred).astype(np.int64)
    cm = np.zeros((C, C), dtype=np.int64)
    ok = (y_true >= 0) & (y_true < C)
    np.add.at(cm, (y_true[ok], y_pred[ok]), 1)
    return cm


def pair_counts(y_true, proba, C):
    """(gt, eq), int64 [C] each: over the pairs (i a sample of class c, j a sample of another class) the number with
    proba[i, c] > proba[j, c] and with proba[i, c] == proba[j, c], compared as float32.  Labels outside [0, C) are on neither side."""
    y_true = np.asarray(y_true).astype(np.int64)
    proba = np.asarray(proba, dtype=np.float32)
    gt, eq = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)
    ok = (y_true >= 0) & (y_true < C)
    for c in range(C):
        pos = proba[ok & (y_true == c), c]
        neg = proba[ok & (y_true != c), c]
        gt[c] = int((pos[:, None] > neg[None, :]).sum())
        eq[c] = int((pos[:, None] == neg[None, :]).sum())
    return gt, eq


def softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def first_argmax(z):
    return np.argmax(np.asarray(z, dtype=np.float64), axis=1)          # numpy: the first of equal maxima


def tie_logits(rng, B, C):
    """Logits in [-10, 10] quantised to multiples of 0.25 (exact in bfloat16 too).  Every even row has its maximum at two columns, so
    the argmax has a tie to resolve; every third row is a copy of the one before, so probabilities are equal across rows."""
    z = np.round(rng.uniform(-10, 10, (B, C)) * 4) / 4
    for i in range(0, B, 2):
        a = int(np.argmax(z[i]))
        b = (a + 1 + int(rng.integers(0, C - 1))) % C                  # any other column, before or after the maximum
        z[i, b] = z[i, a]
    for i in range(2, B, 3):
        z[i] = z[i - 1]
    return z.astype(np.float32)


HIST_LAP = 2048 * 256               # metrics_hist_kernel / metrics_scatter_kernel: at most 2048 work-groups of 256 threads, one sample each per lap


def past_cap_case(seed=0, C=3, head=900, tail=700):
    """(labels int64 [n], proba float32 [n, C]) with n = HIST_LAP + tail: past the first lap of the histogram and the scatter.  Every
    row is dropped (label -1) but `head` rows scattered over the first HIST_LAP and all `tail` rows behind them.  The valid rows hold
    tied probabilities (softmax64 of tie_logits); the dropped rows hold -1.0, below any probability, so a dropped row taken for a
    negative adds to gt."""
    rng = np.random.default_rng(seed)
    n = HIST_LAP + tail
    valid = np.concatenate([np.sort(rng.choice(HIST_LAP, head, replace=False)), np.arange(HIST_LAP, n)])
    y = np.full(n, -1, dtype=np.int64)
    y[valid] = rng.integers(0, C, valid.size)
    p = np.full((n, C), -1.0, dtype=np.float32)
    p[valid] = softmax64(tie_logits(rng, valid.size, C)).astype(np.float32)
    return y, p
