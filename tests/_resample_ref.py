"""NumPy float32 restatement of the resampling batch kernel (csrc/batch_u8.hip: resample_u8_kernel; the operation sequence of
include/kanvit.h), operation by operation so that the comparison is bitwise, on tests/_augment_ref's look-up arithmetic (byte / 255,
minus mean, over std, in fp32) and padding rule (a tap outside the image is the normalised zero); and a plain per-sample loop
restating kanvit.data.crop_table(mode="rrc") from columns it draws itself.  Mixing reuses tests/_mix_ref.mix, which takes any
per-sample array."""
import math

import numpy as np
import torch

from tests import _augment_ref as ar

F32 = np.float32
CROP_TABLE_KEY = 0x63726F705F74626C


def lut(mean, std):
    """[C, 256] float32: ToTensor and Normalize of every byte, as tests/_augment_ref.augment applies them."""
    mean = torch.as_tensor(mean, dtype=torch.float32).reshape(-1, 1)
    std = torch.as_tensor(std, dtype=torch.float32).reshape(-1, 1)
    return (torch.arange(256, dtype=torch.float32).div(255)[None, :] - mean).div(std).numpy()


def axis(n, outputs):
    """Taps and weights of one axis: n source pixels onto `outputs`.  Every line is one float32 operation."""
    scale = F32(n) / F32(outputs)
    o = np.arange(outputs, dtype=F32)
    src = np.maximum(scale * (o + F32(0.5)) - F32(0.5), F32(0))
    assert src.dtype == F32
    t0 = np.minimum(src.astype(np.int64), n - 1)
    t1 = np.minimum(t0 + 1, n - 1)
    w1 = src - t0.astype(F32)
    w0 = F32(1) - w1
    assert w0.dtype == F32 and w1.dtype == F32
    return t0, t1, w0, w1


def taps(image, table, row, rows, cols):
    """t(r, u) for box-local rows `rows` and columns `cols` of one HWC uint8 image under crop row (y0, x0, bh, bw, flip):
    float32 [C, len(rows), len(cols)]."""
    H, W, C = image.shape
    y0, x0, _, _, fl = (int(v) for v in row)
    sy, sx = y0 + rows, x0 + cols
    oky, okx = (sy >= 0) & (sy < H), (sx >= 0) & (sx < W)
    fx = np.where(fl != 0, W - 1 - sx, sx)
    byte = image[np.clip(sy, 0, H - 1)[:, None], np.clip(fx, 0, W - 1)[None, :], :].astype(np.int64)      # [R, U, C]
    byte = np.where((oky[:, None] & okx[None, :])[..., None], byte, 0)
    return np.stack([table[c][byte[..., c]] for c in range(C)])


def resample_one(image, table, row, out_hw):
    """float32 [C, OH, OW]: the kernel's value for one image (HWC uint8, NumPy) under one crop row."""
    OH, OW = out_hw
    C = image.shape[2]
    bh, bw = int(row[2]), int(row[3])
    if bh < 1 or bw < 1:                                    # an empty box: padding, no arithmetic
        return np.broadcast_to(table[:C, 0][:, None, None], (C, OH, OW)).astype(F32).copy()
    r0, r1, wy0, wy1 = axis(bh, OH)
    u0, u1, wx0, wx1 = axis(bw, OW)
    t00, t01 = taps(image, table, row, r0, u0), taps(image, table, row, r0, u1)
    t10, t11 = taps(image, table, row, r1, u0), taps(image, table, row, r1, u1)
    top = (wx0 * t00) + (wx1 * t01)                         # float32 arrays: one rounding per operation, no fma
    bot = (wx0 * t10) + (wx1 * t11)
    out = (wy0[:, None] * top) + (wy1[:, None] * bot)
    assert out.dtype == F32
    return out


def resample_all(images, mean, std, crop, out_hw):
    """Every sample of the dataset under its own crop row (crop None: the whole image, unflipped): float32 [N, C, OH, OW]."""
    images = np.asarray(images)
    if images.ndim == 3:
        images = images[..., None]
    N, H, W, C = images.shape
    table = lut(mean, std)
    rows = np.tile(np.array([0, 0, H, W, 0]), (N, 1)) if crop is None else np.asarray(crop)
    return np.stack([resample_one(images[s], table, rows[s], out_hw) for s in range(N)])


def pad_rows(seed, epoch, n, hw, pad, flip=True):
    """crop_table(mode="pad") from tests/_augment_ref.params."""
    pad_y, pad_x = (pad, pad) if isinstance(pad, int) else pad
    return np.array([[dy - pad_y, dx - pad_x, hw[0], hw[1], fl] for dy, dx, fl in ar.params(seed, epoch, range(n), pad_y, pad_x, flip)], np.int32)


def rrc_rows(n, epoch, seed, hw, flip=True, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), with_fallback=False):
    """crop_table(mode="rrc") as a per-sample loop (torchvision's RandomResizedCrop.get_params) over columns drawn here: one PCG64
    generator seeded from (seed, epoch) under the crop table's key; ten area fractions, ten ratio fractions, row, column, flip.
    with_fallback: also the mask of the rows in which none of the ten attempts fitted."""
    H, W = hw
    g = np.random.Generator(np.random.PCG64(ar.mix(ar.mix((ar.mix(seed & ar.M64) + epoch) & ar.M64) ^ CROP_TABLE_KEY)))
    fa = [g.random(n) for _ in range(10)]
    fr = [g.random(n) for _ in range(10)]
    uy, ux, uf = g.random(n), g.random(n), g.random(n)
    rows, fell_back = [], []
    for s in range(n):
        box = None
        for k in range(10):
            area = H * W * (scale[0] + (scale[1] - scale[0]) * fa[k][s])
            r = math.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * fr[k][s])
            w, h = int(round(math.sqrt(area * r))), int(round(math.sqrt(area / r)))
            if 1 <= w <= W and 1 <= h <= H:
                box = (int(math.floor(uy[s] * (H - h + 1))), int(math.floor(ux[s] * (W - w + 1))), h, w)
                break
        fell_back.append(box is None)
        if box is None:
            h, w = H, W
            if W / H < ratio[0]:
                h = min(max(int(round(W / ratio[0])), 1), H)
            elif W / H > ratio[1]:
                w = min(max(int(round(H * ratio[1])), 1), W)
            box = ((H - h) // 2, (W - w) // 2, h, w)
        rows.append([*box, int(uf[s] < 0.5) if flip else 0])
    return (np.array(rows, np.int32), np.array(fell_back)) if with_fallback else np.array(rows, np.int32)
