"""NumPy restatement of the Random Erasing form of the batch kernel (csrc/batch_u8.hip: erase_u8_kernel, the erasing form of resample_u8_kernel; the semantics
of include/kanvit.h: kanvit_erase_u8).  It builds on tests/_resample_ref.resample_all (every sample under its own crop row) and
tests/_mix_ref.mix (the three mixing rules in float32), which it imports and does not change: between the two it replaces each
sample's erase box by the fill -- zeros, or the noise table indexed by the top bits of a splitmix64 hash stated here on uint64
arrays -- so that the partner enters the mix erased under its own row.  Every step is a look-up or a float32 operation the kernel
also performs: the comparison is bitwise."""
import numpy as np

from tests import _mix_ref as mr
from tests import _resample_ref as rr

M64 = (1 << 64) - 1
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1


def mix_u64(z):
    """One splitmix64 step on a uint64 array (the dtype's arithmetic is mod 2^64)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise_plane(noise, key, s, chw):
    """fill(s, c, y, x) for every (c, y, x) of one sample: noise[h >> (64 - log2 T)], h = mix(mix(key + s) + ((c OH + y) OW + x))."""
    C, OH, OW = chw
    T = len(noise)
    assert T >= 2 and T & (T - 1) == 0
    base = mix_u64(np.array([(int(key) + int(s)) & M64], np.uint64))
    h = mix_u64(base + np.arange(C * OH * OW, dtype=np.uint64))
    return np.asarray(noise, np.float32)[(h >> np.uint64(64 - (T.bit_length() - 1))).astype(np.int64)].reshape(C, OH, OW)


def inside(row, OH, OW):
    """bool [OH, OW]: the pixels of the half-open box (y0, y1, x0, x1), by comparison in Python integers (any int32 entries)."""
    y0, y1, x0, x1 = (int(v) for v in row)
    ys, xs = np.arange(OH), np.arange(OW)
    return ((ys >= y0) & (ys < y1))[:, None] & ((xs >= x0) & (xs < x1))[None, :]


def erase_all(res, erase, noise=None, key=0):
    """a' for every sample of the dataset: res float32 [N, C, OH, OW] (resample_all) with sample s's box replaced by its fill."""
    out = np.array(res, np.float32, copy=True)
    N, C, OH, OW = out.shape
    for s in range(N):
        m = inside(erase[s], OH, OW)
        if m.any():
            fill = np.zeros((C, OH, OW), np.float32) if noise is None else noise_plane(noise, key, s, (C, OH, OW))
            out[s] = np.where(m[None], fill, out[s])
    return out


def batch(erased, pad_value, idx, labels=None, tables=None):
    """What ops.erase_u8 must return for samples idx, from erased = erase_all(...): (x, y), or (x, y, y2, w) with tables = (partner,
    weight, box); x alone without labels.  An idx outside [0, N) is padding (pad_value [C]: lut[c][0]) with label -1, weight 1; a
    partner outside [0, N) leaves the row unmixed."""
    N = erased.shape[0]
    idx = [int(i) for i in idx]
    ok = [0 <= i < N for i in idx]
    safe = [i if o else 0 for i, o in zip(idx, ok)]
    lab = np.zeros(N, np.int64) if labels is None else np.asarray(labels)
    if tables is None:
        x, y = erased[safe].copy(), lab[safe].copy()
        y2 = w = None
    else:
        partner = np.asarray(tables[0]).copy()
        partner[(partner < 0) | (partner >= N)] = -1
        x, y, y2, w = mr.mix(erased, lab, safe, partner, np.asarray(tables[1]), np.asarray(tables[2]))
    for b, o in enumerate(ok):
        if not o:
            x[b] = np.asarray(pad_value, np.float32)[:, None, None]
            y[b] = -1
            if tables is not None:
                y2[b], w[b] = -1, 1.0
    if labels is None:
        return x
    return (x, y) if tables is None else (x, y, y2, w)


def reference(images, mean, std, crop, out_hw, erase, noise=None, key=0):
    """resample_all, then erase_all: the per-sample operands a' of the mix."""
    return erase_all(rr.resample_all(images, mean, std, crop, out_hw), erase, noise, key)
