"""NumPy integer restatement of the RandAugment epoch pass (csrc/randaug.hip: randaug_u8_kernel; the semantics of include/kanvit.h:
kanvit_randaug_u8).  It is the definition the kernel is held to: every op is integer arithmetic on int64 arrays, `>>` is NumPy's
arithmetic shift and `//` is only ever applied to non-negative operands, so the comparison with the kernel is bitwise.  Images are
uint8 [H, W, C]; a table row is (op, p0 .. p6) in Python integers."""
import numpy as np

IDENTITY, AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, AFFINE = range(12)
N_OPS = 12
Q16 = 65536
MAX_BYTES = 24576                       # KANVIT_RA_MAX_BYTES: the largest H W C the kernel takes


def blend(d, v, f):
    """clamp((d 65536 + f (v - d) + 32768) >> 16) on int64 arrays, f in Q16."""
    d, v = np.asarray(d, np.int64), np.asarray(v, np.int64)
    return np.clip((d * Q16 + int(f) * (v - d) + 32768) >> 16, 0, 255)


def grey(img):
    """PIL's L of an image with at least three channels: (19595 R + 38470 G + 7471 B + 32768) >> 16, int64 [H, W]."""
    v = img.astype(np.int64)
    return (19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 32768) >> 16


def row_is_valid(row):
    """The parameter ranges of include/kanvit.h; a row outside them is the identity."""
    op, p = int(row[0]), [int(v) for v in row[1:8]]
    if not 0 <= op < N_OPS:
        return False
    if op == POSTERIZE:
        return 0 <= p[0] <= 8
    if op == SOLARIZE:
        return 0 <= p[0] <= 256
    if op == SOLARIZE_ADD:
        return 0 <= p[0] <= 255 and 0 <= p[1] <= 256
    if op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS):
        return 0 <= p[0] <= 2 * Q16
    return True


def autocontrast(img):
    v = img.astype(np.int64)
    out = v.copy()
    for c in range(v.shape[2]):
        lo, hi = int(v[..., c].min()), int(v[..., c].max())
        if hi > lo:
            out[..., c] = ((v[..., c] - lo) * 255) // (hi - lo)
    return out


def equalize(img):
    v = img.astype(np.int64)
    out = v.copy()
    for c in range(v.shape[2]):
        h = np.bincount(v[..., c].ravel(), minlength=256).astype(np.int64)
        nz = np.flatnonzero(h)
        step = (int(h.sum()) - int(h[nz[-1]])) // 255
        if len(nz) <= 1 or step == 0:
            continue
        before = np.concatenate([[0], np.cumsum(h)[:-1]])          # sum of h[j], j < i
        lut = np.minimum((step // 2 + before) // step, 255)
        out[..., c] = lut[v[..., c]]
    return out


def color(img, f):
    v = img.astype(np.int64)
    if v.shape[2] < 3:
        return v
    out = v.copy()
    out[..., :3] = blend(grey(img)[..., None], v[..., :3], f)
    return out


def contrast(img, f):
    v = img.astype(np.int64)
    H, W, C = v.shape
    g = grey(img) if C >= 3 else v[..., 0]
    m = (int(g.sum()) + (H * W) // 2) // (H * W)
    return blend(m, v, f)


def sharpness(img, f):
    v = img.astype(np.int64)
    H, W, _ = v.shape
    sm = v.copy()
    if H >= 3 and W >= 3:
        s = sum(v[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))     # nine taps
        sm[1:-1, 1:-1] = (s + 4 * v[1:-1, 1:-1] + 6) // 13
    return blend(sm, v, f)


def affine(img, p):
    """Inverse map, nearest neighbour: xs = (p0 (2x+1) + p1 (2y+1) + 2 p2) >> 17, ys likewise from p3, p4, p5; fill from p6."""
    H, W, C = img.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    xs = (p[0] * (2 * x + 1) + p[1] * (2 * y + 1) + 2 * p[2]) >> 17
    ys = (p[3] * (2 * x + 1) + p[4] * (2 * y + 1) + 2 * p[5]) >> 17
    inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    fill = np.array([(p[6] >> (8 * c)) & 255 for c in range(C)], np.int64)
    src = img.astype(np.int64)[np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)]
    return np.where(inside[..., None], src, fill[None, None, :])


def apply_op(img, row):
    """One table row on one uint8 [H, W, C] image -> uint8 [H, W, C]."""
    if not row_is_valid(row):
        return img.copy()
    op, p = int(row[0]), [int(v) for v in row[1:8]]
    v = img.astype(np.int64)
    if op in (IDENTITY,):
        out = v
    elif op == AUTOCONTRAST:
        out = autocontrast(img)
    elif op == EQUALIZE:
        out = equalize(img)
    elif op == INVERT:
        out = 255 - v
    elif op == POSTERIZE:
        out = v & ~(0xFF >> p[0])
    elif op == SOLARIZE:
        out = np.where(v < p[0], v, 255 - v)
    elif op == SOLARIZE_ADD:
        out = np.where(v < p[1], np.minimum(v + p[0], 255), v)
    elif op == BRIGHTNESS:
        out = blend(0, v, p[0])
    elif op == COLOR:
        out = color(img, p[0])
    elif op == CONTRAST:
        out = contrast(img, p[0])
    elif op == SHARPNESS:
        out = sharpness(img, p[0])
    else:
        out = affine(img, p)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def randaugment(images, table):
    """The whole pass: images uint8 [N, H, W, C] or [N, H, W], table int [N, K, 8] -> uint8 of the images' shape; sample s is images[s]
    through its K rows in order."""
    images, table = np.asarray(images), np.asarray(table)
    x = images[..., None] if images.ndim == 3 else images
    out = np.empty_like(x)
    for s in range(x.shape[0]):
        img = x[s]
        for row in table[s]:
            img = apply_op(img, row)
        out[s] = img
    return out.reshape(images.shape)


def row(op, *p):
    """(op, p0 .. p6) with the parameters not given 0."""
    return [op, *p, *([0] * (7 - len(p)))]
