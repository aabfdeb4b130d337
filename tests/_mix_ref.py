"""NumPy restatements for the Mixup / CutMix batch kernel and the fused soft-target cross-entropy (csrc/batch_u8.hip: mix_u8_kernel;
csrc/soft_ce.hip: soft_ce_kernel).  The batch side builds on tests/_augment_ref.augment and states the kernel's arithmetic in float32, operation by
operation, so the comparison is bitwise; the loss side is float64, the common yardstick for the kernel and for torch's own fp32
cross_entropy."""
import numpy as np

from tests import _augment_ref as ar


def hand_table(N, H, W, seed=0):
    """A table for N >= 16 samples that holds, in rows 0..10: an unmixed row; Mixup with w = 0, 0.3 and 1; a sample partnered with
    itself (Mixup, and CutMix in row 10); a full-image CutMix box; a one-pixel box; a box touching two edges; an EMPTY box with a
    weight (which is Mixup by the kernel's rule).  The rest is drawn: a third unmixed, a third Mixup, a third CutMix with a random
    box.  CutMix weights are 1 - area / (H W) in float64, rounded to float32.  Returns (partner int64, weight float32, box int32)."""
    assert N >= 16
    rng = np.random.default_rng(seed)
    partner = np.full(N, -1, np.int64)
    weight = np.ones(N, np.float32)
    box = np.zeros((N, 4), np.int32)

    def cut(i, j, b):
        partner[i], box[i] = j, b
        weight[i] = np.float32(1.0 - (b[1] - b[0]) * (b[3] - b[2]) / float(H * W))

    def blend(i, j, w, b=(0, 0, 0, 0)):
        partner[i], weight[i], box[i] = j, np.float32(w), b

    blend(1, 5, 0.0)
    blend(2, 7, 0.3)
    blend(3, 9, 1.0)
    blend(4, 4, 0.3)                                    # itself, under the same crop: fmul(w, a) + fmul(1 - w, a), not a
    cut(5, 11, (0, H, 0, W))
    cut(6, 12, (H // 2, H // 2 + 1, W // 2, W // 2 + 1))     # one pixel, in the middle: image content under every crop up to pad 2
    cut(7, 13, (0, H // 2, W - 3, W))                   # the top and the right edge
    blend(8, 14, 0.3, (3, 3, 2, 5))                     # no rows: an empty box
    blend(9, 15, 0.625, (1, 4, W, W))                   # no columns either way
    cut(10, 10, (1, 3, 1, 4))
    for i in range(11, N):
        kind = rng.integers(0, 3)
        if kind == 1:
            blend(i, rng.integers(0, N), rng.random())
        elif kind == 2:
            y0, x0 = rng.integers(0, H), rng.integers(0, W)
            cut(i, rng.integers(0, N), (y0, rng.integers(y0 + 1, H + 1), x0, rng.integers(x0 + 1, W + 1)))
    return partner, weight, box


def augment_all(images, mean, std, pad, flip, seed, epoch):
    """tests/_augment_ref.augment of every sample of the dataset, float32 [N, C, H, W] (NumPy): the operands a and p of the mix."""
    return ar.augment(images, list(range(images.shape[0])), mean, std, pad, flip, seed, epoch).numpy()


def mix(aug, labels, idx, partner, weight, box):
    """The batch ops.mix_u8 must give for samples idx, from aug = augment_all(...): (x float32 [B, C, H, W], y, y2, w)."""
    labels = np.asarray(labels)
    x = np.empty((len(idx),) + aug.shape[1:], np.float32)
    y, y2, w = np.empty(len(idx), np.int64), np.empty(len(idx), np.int64), np.empty(len(idx), np.float32)
    for b, s in enumerate(idx):
        j = int(partner[s])
        a = aug[s]
        y[b], w[b] = labels[s], weight[s]
        y2[b] = labels[j] if j >= 0 else labels[s]
        if j < 0:
            x[b] = a
            continue
        p = aug[j]
        y0, y1, x0, x1 = (int(v) for v in box[s])
        if y0 < y1 and x0 < x1:
            x[b] = a
            x[b][:, y0:y1, x0:x1] = p[:, y0:y1, x0:x1]
        else:
            ws = np.float32(weight[s])
            w1 = np.float32(1) - ws                                  # one fp32 subtraction
            x[b] = (ws * a) + (w1 * p)                               # float32 arrays: a rounding per operation, no fma
    return x, y, y2, w


def soft_targets(C, y1, y2, w, eps):
    """t [B, C] in float64 and the mask of rows whose labels are all inside [0, C) (the others are all zero)."""
    y1 = np.asarray(y1)
    y2 = y1 if y2 is None else np.asarray(y2)
    w = np.ones(len(y1)) if w is None else np.asarray(w, np.float64)
    ok = (y1 >= 0) & (y1 < C) & (y2 >= 0) & (y2 < C)
    t = np.zeros((len(y1), C))
    r = np.nonzero(ok)[0]
    np.add.at(t, (r, y1[r]), w[r])
    np.add.at(t, (r, y2[r]), 1.0 - w[r])
    t = (1.0 - eps) * t + eps / C
    t[~ok] = 0.0
    return t, ok


def soft_ce(z, y1, y2=None, w=None, eps=0.0):
    """float64: (loss, loss_rows [B], dlogits [B, C]) of include/kanvit.h's kanvit_soft_ce for float32 logits z [B, C]."""
    z = np.asarray(z, np.float64)
    B, C = z.shape
    t, ok = soft_targets(C, y1, y2, w, eps)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    rows = np.where(ok, np.log(s[:, 0]) + (t * (m - z)).sum(1), 0.0)
    dz = np.where(ok[:, None], (e / s - t) / B, 0.0)
    return rows.sum() / B, rows, dz


def mean_rows_f32(rows, threads=256):
    """soft_ce_mean_kernel in NumPy float32: thread t adds rows t, t + 256, ... in order, then part[:o] += part[o:2o] for o = 128 .. 1,
    then one float32 division by float32(B).  Every operation rounds once, as the device's do (its division is the IEEE sequence)."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 1 and rows.size >= 1
    part = np.zeros(threads, np.float32)
    for lo in range(0, rows.size, threads):
        blk = rows[lo:lo + threads]
        part[:blk.size] = part[:blk.size] + blk
    o = threads // 2
    while o:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    out = part[0] / np.float32(rows.size)
    assert out.dtype == np.float32
    return out
