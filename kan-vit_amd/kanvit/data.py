"""Training and evaluation batches from a dataset that stays on the GPU as uint8.

CIFAR-100's training set is 154 MB as uint8 and MNIST's 47 MB: they fit in HBM thousands of times over.  GpuDataset keeps the images
(NHWC, as the arrays come) and the labels on the device and produces every batch with ONE kernel (ops.augment_u8, csrc/batch_u8.hip):
gather by index, random crop out of the zero-padded image, random horizontal flip, ToTensor and Normalize -- the reference's
transforms (train.py:100-118) without its DataLoader workers, its PIL round trip, its host-to-device copy per batch, and without
torchvision.  Per batch the device reads B*H*W*C bytes and writes 4*B*C*H*W.

The crop offsets and the flip of a sample are a pure function of (seed, epoch, sample index) (include/kanvit.h), and the epoch's
order is a permutation drawn from a CPU generator seeded by (seed, epoch): a run is reproducible across batch sizes and
data-parallel layouts, and needs no RNG state on the device.

Mixup and CutMix ride on the same pass: mix_table draws one table per epoch from (seed, epoch), indexed by dataset index, and
batches(mix=...) hands it to ops.mix_u8, which blends or pastes the partner under the partner's own crop and flip -- a sample's pixels
and soft targets stay a function of (seed, epoch, sample index).

Another output size and RandomResizedCrop ride on it too: GpuDataset(out_size=..., crop="rrc") produces every batch with
ops.resample_u8, the bilinear resize of a per-sample box named by crop_table -- again one table per epoch drawn from (seed, epoch) and
indexed by dataset index.  With the stored size and the padded crop nothing changes.

Random Erasing rides on it as well: GpuDataset(erase=...) produces every batch with ops.erase_u8, which replaces a per-sample box
named by erase_table -- one more table per epoch drawn from (seed, epoch) and indexed by dataset index -- by zeros or by
standard-normal noise (normal_table, looked up through a hash of (seed, epoch, sample, channel, pixel)) before the sample is mixed,
and erases the partner under the partner's own box.

RandAugment does not ride on the batch kernel: GpuDataset(randaug=...) keeps a second uint8 buffer of the dataset's size, and once
per epoch ONE launch (ops.randaugment_u8, csrc/randaug.hip) writes every image into it through the two ops randaug_table names for
it -- a table per epoch drawn from (seed, epoch), indexed by dataset index, integer parameters only.  Every batch kernel above then
reads that buffer in place of the stored images and works unchanged; a Mixup / CutMix partner comes augmented under its own rows.
The ops run at the stored resolution, BEFORE the crop, the flip and the resize (timm runs them after RandomResizedCrop).

The file format is an .npz: x_train uint8 [N, H, W, C] (or [N, H, W] for one channel), y_train of any integer type, optionally
x_test / y_test, optionally mean / std ([C], on the 0-1 scale; computed from x_train when absent).  tools/cifar_to_npz.py writes
one from an unpacked CIFAR python-pickle directory.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import ops

_M64 = (1 << 64) - 1


def _mix(z: int) -> int:
    """One splitmix64 step (the `mix` of include/kanvit.h) in Python integers."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def rank_seed(seed: int, rank: int = 0, world: int = 1) -> int:
    """The seed of a rank's own hashes (drop-path masks, patch-dropout keep sets): `seed` itself on one rank; with more, the rank
    is mixed in, or every rank would draw the same positions of its shard."""
    return seed if world == 1 else _mix(_mix(seed) + rank)


def make_lut(mean, std) -> torch.Tensor:
    """[C, 256] float32 on the CPU: the normalised value of every byte per channel, with the reference's own operations (ToTensor's
    byte / 255, then Normalize's (v - mean) / std, all in fp32: train.py:100-118).  Built on the CPU on purpose: a device divide by a
    scalar may multiply by the reciprocal, which is 1 ulp away, and the table is what makes the kernel's output bitwise."""
    mean = torch.as_tensor(mean, dtype=torch.float32, device="cpu").reshape(-1)
    std = torch.as_tensor(std, dtype=torch.float32, device="cpu").reshape(-1)
    if mean.numel() != std.numel() or not 1 <= mean.numel() <= 4:
        raise ValueError(f"make_lut: mean has {mean.numel()} and std {std.numel()} entries; one per channel, 1 to 4 channels")
    if not bool((std > 0).all()):
        raise ValueError("make_lut: std must be positive")
    v = torch.arange(256, dtype=torch.float32).div(255)
    return (v[None, :] - mean[:, None]).div(std[:, None]).contiguous()


def epoch_indices(n: int, epoch: int, seed: int, rank: int = 0, world: int = 1, shuffle: bool = True, device="cpu") -> torch.Tensor:
    """The sample indices `rank` of `world` visits in `epoch`, int64 on `device`.  With `shuffle` the order is a torch.randperm from a
    CPU generator seeded by (seed, epoch) -- the same permutation on every rank and on every device; it is padded by wrapping round
    to a multiple of `world` (as DistributedSampler does: every rank takes the same number of steps, which the collectives need),
    and the rank takes every world-th entry from its own."""
    if n < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"epoch_indices: n={n}, rank={rank}, world={world}")
    if shuffle:
        g = torch.Generator(device="cpu")
        g.manual_seed(_mix((_mix(int(seed) & _M64) + int(epoch)) & _M64) >> 1)
        perm = torch.randperm(n, generator=g)
    else:
        perm = torch.arange(n)
    total = -(-n // world) * world
    if total > n:
        perm = perm.repeat(-(-total // n))[:total]
    return perm[rank::world].contiguous().to(device)


class MixTable(NamedTuple):
    """One epoch's Mixup / CutMix decisions, CPU tensors indexed by the DATASET index: partner int64 [n] (-1: not mixed), weight
    float32 [n] (of the sample's own label; 1 where not mixed), box int32 [n, 4] = (y0, y1, x0, x1), half open, output coordinates
    (empty -- all zero -- for Mixup and unmixed rows)."""
    partner: torch.Tensor
    weight: torch.Tensor
    box: torch.Tensor


_MIX_TABLE_KEY = 0x6D69785F7461626C     # "mix_tabl": keeps the table's generator apart from the permutation's


def mix_table(n: int, epoch: int, seed: int, hw, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0,
              switch_prob: float = 0.5) -> MixTable:
    """The Mixup / CutMix table of `epoch` for a dataset of n images of size hw = (H, W) (the recipe of DeiT / timm's Mixup, per
    sample).  Every draw comes from ONE CPU generator (NumPy's PCG64) seeded by (seed, epoch), and all n rows are drawn, in index
    order: the table depends on nothing else -- not on the batch size, the rank or the world size -- so what ops.mix_u8 makes of
    sample i is a function of (seed, epoch, i) like the crop and the flip.

    With probability `prob` a sample is mixed, with a partner uniform over [0, n) (it may draw itself).  CutMix is chosen with
    probability `switch_prob` when both alphas are positive, otherwise the mode whose alpha is positive; lam ~ Beta(alpha, alpha).
    Mixup: weight = float32(lam), empty box.  CutMix is timm's rand_bbox: r = sqrt(1 - lam), a box of int(H r) x int(W r) around a
    centre uniform in [0, H) x [0, W), clipped to the image; weight = 1 - area / (H W), in float64, rounded to float32; a box clipped
    to nothing leaves the row unmixed.  Both alphas 0 is a ValueError (not a table of -1)."""
    H, W = int(hw[0]), int(hw[1])
    ma, ca = float(mixup_alpha), float(cutmix_alpha)
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"mix_table: n={n}, hw={tuple(hw)}")
    if ma < 0 or ca < 0 or not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
        raise ValueError(f"mix_table: mixup_alpha={ma}, cutmix_alpha={ca}, prob={prob}, switch_prob={switch_prob}: alphas are not "
                         "negative and probabilities lie in [0, 1]")
    if ma == 0 and ca == 0:
        raise ValueError("mix_table: mixup_alpha and cutmix_alpha are both 0: nothing to mix (leave `mix` out instead)")
    g = np.random.Generator(np.random.PCG64(_mix(_mix((_mix(int(seed) & _M64) + int(epoch)) & _M64) ^ _MIX_TABLE_KEY)))
    mixed = g.random(n) < prob                       # each column is drawn for all n rows, in index order, whatever the flags
    switch = g.random(n) < switch_prob
    partner = g.integers(0, n, n)
    lam_mix = g.beta(ma, ma, n) if ma > 0 else np.zeros(n)
    lam_cut = g.beta(ca, ca, n) if ca > 0 else np.zeros(n)
    cy, cx = g.integers(0, H, n), g.integers(0, W, n)
    cut = switch if (ma > 0 and ca > 0) else np.full(n, ca > 0)
    r = np.sqrt(1.0 - lam_cut)
    ch, cw = (H * r).astype(np.int64), (W * r).astype(np.int64)
    y0, y1 = np.clip(cy - ch // 2, 0, H), np.clip(cy + ch // 2, 0, H)
    x0, x1 = np.clip(cx - cw // 2, 0, W), np.clip(cx + cw // 2, 0, W)
    area = (y1 - y0) * (x1 - x0)
    mixed &= ~cut | (area > 0)
    cut &= mixed
    weight = np.where(cut, 1.0 - area / float(H * W), np.where(mixed, lam_mix, 1.0)).astype(np.float32)
    box = np.where(cut[:, None], np.stack([y0, y1, x0, x1], 1), 0).astype(np.int32)
    return MixTable(torch.from_numpy(np.where(mixed, partner, -1).astype(np.int64)), torch.from_numpy(weight), torch.from_numpy(box))


_CROP_TABLE_KEY = 0x63726F705F74626C    # "crop_tbl": the crop table's generator, apart from the permutation's and the mix table's
_RRC_ATTEMPTS = 10                      # torchvision's RandomResizedCrop.get_params tries ten boxes before it falls back


def _mix_u64(z: np.ndarray) -> np.ndarray:
    """_mix on a uint64 array (arithmetic mod 2^64 is what the dtype does)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def crop_table(n: int, epoch: int, seed: int, hw, mode: str, pad=(0, 0), flip: bool = True, scale=(0.08, 1.0),
               ratio=(3.0 / 4.0, 4.0 / 3.0)) -> torch.Tensor:
    """The crop table of `epoch` for ops.resample_u8: int32 [n, 5] on the CPU, row s = (y0, x0, bh, bw, flip) for DATASET index s -- a
    box of bh x bw source pixels at (y0, x0) in the coordinates of the possibly flipped, zero-padded image of size hw = (H, W).  Like
    mix_table it is a function of its arguments alone: not of the batch size, the rank or the world size.

    mode "pad": ops.augment_u8's crop.  (dy, dx, fl) are the per-sample hash of include/kanvit.h (mix(mix(mix(seed) + epoch) + s),
    here on a uint64 array) and the row is (dy - pad_y, dx - pad_x, H, W, fl); `scale` and `ratio` are not used.

    mode "rrc": torchvision's RandomResizedCrop.get_params; `pad` is not used.  The draws come from ONE NumPy PCG64 generator seeded
    by (seed, epoch) under a key of its own; every column is a g.random(n) in float64 for all n rows in index order: ten area
    fractions a_k (area = H W (lo + (hi - lo) a_k) over `scale`), then ten ratios r_k = exp(log lo + (log hi - log lo) u_k) over
    `ratio`, then one row position, one column position and one flip (u < 0.5).  Attempt k gives w = rint(sqrt(area r)),
    h = rint(sqrt(area / r)); the first with 1 <= w <= W and 1 <= h <= H is taken and placed at floor(u (H - h + 1)),
    floor(u (W - w + 1)).  If none fits: the centred whole image clipped to the ratio bounds (W / H below ratio[0]: w = W,
    h = rint(W / ratio[0]); above ratio[1]: h = H, w = rint(H ratio[1])).  Every box lies inside the image.

    flip=False zeroes the flip column.  Bad arguments are a ValueError."""
    H, W = int(hw[0]), int(hw[1])
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"crop_table: n={n}, hw={tuple(hw)}")
    if mode not in ("pad", "rrc"):
        raise ValueError(f"crop_table: mode '{mode}' is 'pad' or 'rrc'")
    base = _mix((_mix(int(seed) & _M64) + int(epoch)) & _M64)
    if mode == "pad":
        pad_y, pad_x = (int(pad), int(pad)) if isinstance(pad, int) else (int(pad[0]), int(pad[1]))
        if not 0 <= pad_y <= H or not 0 <= pad_x <= W:
            raise ValueError(f"crop_table: pad=({pad_y}, {pad_x}) must be in 0..H={H}, 0..W={W}")
        h = _mix_u64(np.uint64(base) + np.arange(n, dtype=np.uint64))
        m20 = np.uint64(0xFFFFF)
        dy = ((h & m20) % np.uint64(2 * pad_y + 1)).astype(np.int64)
        dx = (((h >> np.uint64(20)) & m20) % np.uint64(2 * pad_x + 1)).astype(np.int64)
        fl = ((h >> np.uint64(40)) & np.uint64(1)).astype(np.int64)
        rows = np.stack([dy - pad_y, dx - pad_x, np.full(n, H), np.full(n, W), fl if flip else np.zeros(n, np.int64)], 1)
        return torch.from_numpy(rows.astype(np.int32))
    s_lo, s_hi, r_lo, r_hi = float(scale[0]), float(scale[1]), float(ratio[0]), float(ratio[1])
    if not 0 < s_lo <= s_hi or not 0 < r_lo <= r_hi or not all(np.isfinite([s_hi, r_hi])):
        raise ValueError(f"crop_table: scale={tuple(scale)} and ratio={tuple(ratio)} are (lo, hi) with 0 < lo <= hi")
    g = np.random.Generator(np.random.PCG64(_mix(base ^ _CROP_TABLE_KEY)))
    area = [H * W * (s_lo + (s_hi - s_lo) * g.random(n)) for _ in range(_RRC_ATTEMPTS)]
    rat = [np.exp(np.log(r_lo) + (np.log(r_hi) - np.log(r_lo)) * g.random(n)) for _ in range(_RRC_ATTEMPTS)]
    uy, ux, fl = g.random(n), g.random(n), g.random(n) < 0.5
    bh, bw = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for a, r in zip(area, rat):
        w, h = np.rint(np.sqrt(a * r)).astype(np.int64), np.rint(np.sqrt(a / r)).astype(np.int64)
        take = (bh == 0) & (w >= 1) & (w <= W) & (h >= 1) & (h <= H)
        bh, bw = np.where(take, h, bh), np.where(take, w, bw)
    found = bh > 0
    y0 = np.floor(uy * (H - bh + 1)).astype(np.int64)
    x0 = np.floor(ux * (W - bw + 1)).astype(np.int64)
    fh, fw = H, W                                   # the fallback: one box for the whole table
    if W / H < r_lo:
        fh = min(max(int(np.rint(W / r_lo)), 1), H)
    elif W / H > r_hi:
        fw = min(max(int(np.rint(H * r_hi)), 1), W)
    rows = np.stack([np.where(found, y0, (H - fh) // 2), np.where(found, x0, (W - fw) // 2), np.where(found, bh, fh),
                     np.where(found, bw, fw), fl.astype(np.int64) if flip else np.zeros(n, np.int64)], 1)
    return torch.from_numpy(rows.astype(np.int32))


_ERASE_TABLE_KEY = 0x65726173655F7462   # "erase_tb": the erase table's generator, apart from the other tables'
_ERASE_NOISE_KEY = 0x65726173655F6E7A   # "erase_nz": the key of the noise hash
_ERASE_ATTEMPTS = 10                    # torchvision's RandomErasing.get_params tries ten boxes before it gives up


def erase_table(n: int, epoch: int, seed: int, hw, prob: float = 0.25, scale=(0.02, 1.0 / 3.0), ratio=(0.3, 1.0 / 0.3)) -> torch.Tensor:
    """The Random Erasing table of `epoch` for ops.erase_u8: int32 [n, 4] on the CPU, row s = (y0, y1, x0, x1), half open, for DATASET
    index s, in the coordinates of the OUTPUT of size hw = (OH, OW) (torchvision's RandomErasing.get_params / timm's RandomErasing,
    per sample).  Like mix_table and crop_table it is a function of its arguments alone: not of the batch size, the rank or the world
    size.

    The draws come from ONE NumPy PCG64 generator seeded by (seed, epoch) under a key of its own; every column is a g.random(n) in
    float64 for all n rows in index order, whatever the flags: one u_p, ten area fractions a_k (area = OH OW (lo + (hi - lo) a_k) over
    `scale`), ten ratios r_k = exp(log lo + (log hi - log lo) u_k) over `ratio`, one row position, one column position.  A row is
    erased iff u_p < prob and an attempt fits: attempt k gives h = rint(sqrt(area r)), w = rint(sqrt(area / r)); the first with
    1 <= h < OH and 1 <= w < OW is taken and placed at floor(u (OH - h + 1)), floor(u (OW - w + 1)).  Every other row is all zero
    (nothing is erased: torchvision's no-op).  Bad arguments are a ValueError."""
    OH, OW = int(hw[0]), int(hw[1])
    if n < 1 or OH < 1 or OW < 1:
        raise ValueError(f"erase_table: n={n}, hw={tuple(hw)}")
    prob = float(prob)
    s_lo, s_hi, r_lo, r_hi = float(scale[0]), float(scale[1]), float(ratio[0]), float(ratio[1])
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"erase_table: prob={prob} is not a probability")
    if not 0 < s_lo <= s_hi <= 1 or not 0 < r_lo <= r_hi or not np.isfinite(r_hi):
        raise ValueError(f"erase_table: scale={tuple(scale)} and ratio={tuple(ratio)} are (lo, hi) with 0 < lo <= hi, and scale's hi is at most 1")
    base = _mix((_mix(int(seed) & _M64) + int(epoch)) & _M64)
    g = np.random.Generator(np.random.PCG64(_mix(base ^ _ERASE_TABLE_KEY)))
    chosen = g.random(n) < prob
    area = [OH * OW * (s_lo + (s_hi - s_lo) * g.random(n)) for _ in range(_ERASE_ATTEMPTS)]
    rat = [np.exp(np.log(r_lo) + (np.log(r_hi) - np.log(r_lo)) * g.random(n)) for _ in range(_ERASE_ATTEMPTS)]
    uy, ux = g.random(n), g.random(n)
    bh, bw = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for a, r in zip(area, rat):
        h, w = np.rint(np.sqrt(a * r)).astype(np.int64), np.rint(np.sqrt(a / r)).astype(np.int64)
        take = (bh == 0) & (h >= 1) & (h < OH) & (w >= 1) & (w < OW)
        bh, bw = np.where(take, h, bh), np.where(take, w, bw)
    y0 = np.floor(uy * (OH - bh + 1)).astype(np.int64)
    x0 = np.floor(ux * (OW - bw + 1)).astype(np.int64)
    erased = chosen & (bh > 0)
    rows = np.where(erased[:, None], np.stack([y0, y0 + bh, x0, x0 + bw], 1), 0)
    return torch.from_numpy(rows.astype(np.int32))


def normal_table(T: int = 4096) -> torch.Tensor:
    """The noise table of ops.erase_u8's "pixel" fill: float32 [T] on the CPU, entry k the standard-normal quantile at (k + 0.5) / T
    (statistics.NormalDist().inv_cdf in float64, rounded once).  A uniform index into it is a standard-normal draw quantised to T
    levels: increasing, antisymmetric (t[k] == -t[T - 1 - k]), std 0.99984 and largest value 3.668 at T = 4096.  T is a power of two
    in 2..65536, so that the top bits of a hash index it."""
    from statistics import NormalDist
    T = int(T)
    if T < 2 or T > 65536 or T & (T - 1):
        raise ValueError(f"normal_table: T={T} is a power of two in 2..65536")
    inv = NormalDist().inv_cdf
    return torch.from_numpy(np.array([inv((k + 0.5) / T) for k in range(T)], np.float64).astype(np.float32))


def erase_noise_key(seed: int, epoch: int) -> int:
    """The noise_key of ops.erase_u8 for (seed, epoch): the hash chain of the tables, under a key of its own."""
    return _mix(_mix((_mix(int(seed) & _M64) + int(epoch)) & _M64) ^ _ERASE_NOISE_KEY)


def _erase_config(erase) -> dict:
    """GpuDataset's `erase` argument, checked: prob, scale, ratio as erase_table takes them and mode "pixel" or "const"."""
    cfg = dict(prob=0.25, scale=(0.02, 1.0 / 3.0), ratio=(0.3, 1.0 / 0.3), mode="pixel")
    if not isinstance(erase, dict) or not set(erase) <= set(cfg):
        raise ValueError(f"GpuDataset: erase={erase!r} is a dict with keys out of {sorted(cfg)}")
    cfg.update(erase)
    if cfg["mode"] not in ("pixel", "const"):
        raise ValueError(f"GpuDataset: erase mode '{cfg['mode']}' is 'pixel' or 'const'")
    cfg["scale"], cfg["ratio"] = tuple(cfg["scale"]), tuple(cfg["ratio"])
    erase_table(1, 0, 0, (2, 2), cfg["prob"], cfg["scale"], cfg["ratio"])        # its argument checks, once, before any epoch
    return cfg


_RANDAUG_TABLE_KEY = 0x72616E646175675F  # "randaug_": the RandAugment table's counters, apart from the other tables' generators
_RANDAUG_DRAWS = 4                      # hashed draws per slot: the op, whether it is kept, the magnitude, the sign
# timm's "increasing" set (rand-...-inc1), in its order; Rotate .. TranslateY are AFFINE rows, the rest map to a code each
RANDAUG_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
               "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY")
_RA_CODES = dict(Identity=0, AutoContrast=1, Equalize=2, Invert=3, Posterize=4, Solarize=5, SolarizeAdd=6, Brightness=7, Color=8, Contrast=9,
                 Sharpness=10, Rotate=11, ShearX=11, ShearY=11, TranslateX=11, TranslateY=11)


def _q16(v) -> np.ndarray:
    """value * 65536 rounded to the nearest integer, inside int32."""
    return np.clip(np.rint(np.asarray(v, np.float64) * 65536.0), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def _randaug_rows(name: str, level: np.ndarray, sign: np.ndarray, H: int, W: int, fill: int) -> np.ndarray:
    """The rows (op, p0 .. p6) of op `name` at level = m / 10 in [0, 1] and sign = +-1, int64 [len(level), 8]: the magnitude rules of
    randaug_table's docstring, in float64, rounded to integers here -- the kernel sees integers only."""
    rows = np.zeros((len(level), 8), np.int64)
    rows[:, 0] = _RA_CODES[name]
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        rows[:, 1] = _q16(np.maximum(0.1, 1.0 + sign * 0.9 * level))
    elif name == "Posterize":
        rows[:, 1] = 4 - (4.0 * level).astype(np.int64)
    elif name == "Solarize":
        rows[:, 1] = 256 - (256.0 * level).astype(np.int64)
    elif name == "SolarizeAdd":
        rows[:, 1], rows[:, 2] = np.minimum(128, (110.0 * level).astype(np.int64)), 128
    elif _RA_CODES[name] == 11:
        # the inverse map source = A (output - centre) + centre + t, in half-pixel-centre coordinates: centre = (W / 2, H / 2)
        one, zero = np.ones_like(level), np.zeros_like(level)
        a, b, d, e, tx, ty = one, zero, zero, one, zero, zero
        if name == "Rotate":                        # PIL's Image.rotate(angle): the matrix of -angle
            t = -np.radians(sign * 30.0 * level)
            a, b, d, e = np.cos(t), np.sin(t), -np.sin(t), np.cos(t)
        elif name == "ShearX":
            b = sign * 0.3 * level
        elif name == "ShearY":
            d = sign * 0.3 * level
        elif name == "TranslateX":
            tx = sign * 0.45 * level * W
        else:
            ty = sign * 0.45 * level * H
        cx, cy = W / 2.0, H / 2.0
        rows[:, 1], rows[:, 2], rows[:, 3] = _q16(a), _q16(b), _q16(cx - a * cx - b * cy + tx)
        rows[:, 4], rows[:, 5], rows[:, 6] = _q16(d), _q16(e), _q16(cy - d * cx - e * cy + ty)
        rows[:, 7] = fill
    return rows


def randaug_table(n: int, epoch: int, seed: int, hw, n_ops: int = 2, magnitude: float = 9.0, mstd: float = 0.5, prob: float = 0.5,
                  fill=(128, 128, 128), ops=None) -> torch.Tensor:
    """The RandAugment table of `epoch` for ops.randaugment_u8: int32 [n, n_ops, 8] on the CPU, rows (op, p0 .. p6) of include/kanvit.h
    for DATASET index s, for stored images of size hw = (H, W) (timm's rand-m{magnitude}-mstd{mstd}-inc1 with n_ops ops per sample,
    each applied with probability `prob`).  Like the other tables it is a function of its arguments alone -- not of the batch size,
    the rank or the world size -- and it is drawn by counters, not by a generator: draw d of slot k of sample s is
    mix(mix(base + s) + 4 k + d), base = mix(mix(mix(seed) + epoch) ^ key), all mod 2^64 (the vectorised splitmix64 of crop_table's "pad"
    rows), so row s does not depend on n either: the table of n samples is the head of the table of any larger n.

    Per slot: d = 0 picks the op, floor(u len(ops)) with u the top 53 bits as a fraction; d = 1 keeps it iff u < prob, otherwise the
    row is IDENTITY (all zero); d = 2 draws the magnitude m = clip(magnitude + mstd z, 0, 10), z = normal_table(4096)[top 12 bits] (the
    inverse normal CDF on a hashed uniform, quantised); d = 3 gives the sign (top bit set: -1) of the signed ops.  With level = m / 10:
      Rotate                       +-30 degrees * level                        ShearX / ShearY   +-0.3 * level
      TranslateX / TranslateY      +-0.45 * level of the width / height        AutoContrast, Equalize, Invert: no magnitude
      Brightness / Color / Contrast / Sharpness     factor f = max(0.1, 1 +- 0.9 * level)
      Posterize    bits = 4 - int(4 level)          Solarize   threshold = 256 - int(256 level)
      SolarizeAdd  add = min(128, int(110 level)), threshold = 128
    modelled on timm's _LEVEL functions; they are this project's definition.  Rotation, shear and translation are AFFINE rows: the
    inverse matrix about the image centre in Q16, the fill byte of channel c is fill[c] (an int, or a sequence whose last entry serves
    the channels beyond it).  All trigonometry and rounding happens here in float64.

    ops: the names to pick from, default RANDAUG_OPS (timm's fifteen "increasing" ops; "Identity" may be listed too).  Bad arguments
    are a ValueError."""
    H, W = int(hw[0]), int(hw[1])
    n_ops, magnitude, mstd, prob = int(n_ops), float(magnitude), float(mstd), float(prob)
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"randaug_table: n={n}, hw={tuple(hw)}")
    if not 1 <= n_ops <= 4:
        raise ValueError(f"randaug_table: n_ops={n_ops} is in 1..4")
    if not 0.0 <= magnitude <= 10.0 or not 0.0 <= mstd < float("inf") or not 0.0 <= prob <= 1.0:
        raise ValueError(f"randaug_table: magnitude={magnitude} is in [0, 10], mstd={mstd} is finite and not negative, prob={prob} is a probability")
    names = RANDAUG_OPS if ops is None else tuple(ops)
    if not names or any(name not in _RA_CODES for name in names):
        raise ValueError(f"randaug_table: ops={names!r} is a non-empty list of names out of {sorted(_RA_CODES)}")
    try:
        fills = [int(fill)] if isinstance(fill, (int, np.integer)) else [int(v) for v in fill]
    except (TypeError, ValueError):
        fills = []
    if not 1 <= len(fills) <= 4 or any(not 0 <= v <= 255 for v in fills):
        raise ValueError(f"randaug_table: fill={fill!r} is a byte, or one to four bytes (one per channel)")
    fills += [fills[-1]] * (4 - len(fills))
    packed = int(np.array([fills[0] | fills[1] << 8 | fills[2] << 16 | fills[3] << 24], np.uint32).view(np.int32)[0])
    base = _mix(_mix((_mix(int(seed) & _M64) + int(epoch)) & _M64) ^ _RANDAUG_TABLE_KEY)
    sample = _mix_u64(np.uint64(base) + np.arange(n, dtype=np.uint64))
    h = _mix_u64(sample[:, None] + np.arange(n_ops * _RANDAUG_DRAWS, dtype=np.uint64)[None, :]).reshape(n, n_ops, _RANDAUG_DRAWS)
    u = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    pick = np.minimum((u[..., 0] * len(names)).astype(np.int64), len(names) - 1)
    keep = u[..., 1] < prob
    z = normal_table(4096).numpy().astype(np.float64)[(h[..., 2] >> np.uint64(52)).astype(np.int64)]
    level = np.clip(magnitude + mstd * z, 0.0, 10.0) / 10.0
    sign = np.where((h[..., 3] >> np.uint64(63)).astype(bool), -1.0, 1.0)
    rows = np.zeros((n, n_ops, 8), np.int64)
    for j, name in enumerate(names):
        m = keep & (pick == j)
        rows[m] = _randaug_rows(name, level[m], sign[m], H, W, packed)
    return torch.from_numpy(rows.astype(np.int32))


def _randaug_config(randaug) -> dict:
    """GpuDataset's `randaug` argument, checked: n_ops, magnitude, mstd, prob, fill and ops as randaug_table takes them."""
    cfg = dict(n_ops=2, magnitude=9.0, mstd=0.5, prob=0.5, fill=(128, 128, 128), ops=None)
    if not isinstance(randaug, dict) or not set(randaug) <= set(cfg):
        raise ValueError(f"GpuDataset: randaug={randaug!r} is a dict with keys out of {sorted(cfg)}")
    cfg.update(randaug)
    randaug_table(1, 0, 0, (2, 2), **cfg)            # its argument checks, once, before any epoch
    return cfg


def _fail(path, key, what):
    raise ValueError(f"{path}: '{key}' {what}")


def load_npz(path) -> dict:
    """Read and validate the .npz layout of this module; a wrong dtype or shape is a ValueError that names the key."""
    with np.load(path, allow_pickle=False) as f:
        blob = {k: f[k] for k in f.files}
    if "x_train" not in blob or "y_train" not in blob:
        _fail(path, "x_train" if "x_train" not in blob else "y_train", "is missing")
    xt = blob["x_train"]
    for split in ("train", "test"):
        xk, yk = f"x_{split}", f"y_{split}"
        if (xk in blob) != (yk in blob):
            _fail(path, yk if xk in blob else xk, f"is missing ('{xk if xk in blob else yk}' is present)")
        if xk not in blob:
            continue
        x, y = blob[xk], blob[yk]
        if x.dtype != np.uint8:
            _fail(path, xk, f"has dtype {x.dtype}, expected uint8")
        if x.ndim not in (3, 4) or x.shape[0] < 1 or min(x.shape) < 1 or (x.ndim == 4 and x.shape[3] > 4):
            _fail(path, xk, f"has shape {x.shape}, expected [N, H, W, C] with 1 to 4 channels, or [N, H, W]")
        if x.shape[1:] != xt.shape[1:]:
            _fail(path, xk, f"has image shape {x.shape[1:]}, x_train has {xt.shape[1:]}")
        if not np.issubdtype(y.dtype, np.integer):
            _fail(path, yk, f"has dtype {y.dtype}, expected an integer type")
        if y.shape != (x.shape[0],):
            _fail(path, yk, f"has shape {y.shape}, expected ({x.shape[0]},) as '{xk}' has that many images")
        if int(y.min()) < 0:
            _fail(path, yk, "has a negative label")
    C = xt.shape[3] if xt.ndim == 4 else 1
    if ("mean" in blob) != ("std" in blob):
        _fail(path, "std" if "mean" in blob else "mean", "is missing (mean and std come together)")
    for k in ("mean", "std"):
        if k in blob:
            v = blob[k]
            if not np.issubdtype(v.dtype, np.floating) or v.shape != (C,):
                _fail(path, k, f"has dtype {v.dtype} and shape {v.shape}, expected floating point, shape ({C},)")
    if "std" in blob and not (blob["std"] > 0).all():
        _fail(path, "std", "must be positive")
    return blob


def channel_stats(x: np.ndarray):
    """Per-channel mean and std of uint8 images on the 0-1 scale, in float64 on the CPU, rounded to fp32."""
    v = x.reshape(x.shape[0], x.shape[1], x.shape[2], -1).astype(np.float64) / 255.0
    mean, std = v.mean(axis=(0, 1, 2)), v.std(axis=(0, 1, 2))
    return mean.astype(np.float32), std.astype(np.float32)


class Batches:
    """One configured pass over a GpuDataset as a re-iterable with a length (what an evaluation loop wants from a loader)."""

    def __init__(self, dataset, batch_size, epoch=0, seed=0, rank=0, world=1, shuffle=True):
        self.dataset, self.kw = dataset, dict(batch_size=batch_size, epoch=epoch, seed=seed, rank=rank, world=world, shuffle=shuffle)

    def __iter__(self):
        return self.dataset.batches(**self.kw)

    def __len__(self):
        return self.dataset.n_batches(self.kw["batch_size"], self.kw["world"])


class GpuDataset:
    """Images (uint8, NHWC) and labels (int64) resident on `device`; batches() yields normalised, augmented float32 NCHW batches."""

    def __init__(self, images, labels, mean, std, device, pad=0, flip=False, out_size=None, crop="pad", rrc_scale=(0.08, 1.0),
                 rrc_ratio=(3.0 / 4.0, 4.0 / 3.0), erase=None, randaug=None):
        """out_size (an int or (OH, OW)): the size of the batches, resized from the stored images by ops.resample_u8; None: the stored
        size.  crop: "pad" (the random crop out of the zero-padded image, `pad` and `flip`) or "rrc" (RandomResizedCrop over rrc_scale /
        rrc_ratio, with `flip`; `pad` is then unused).  With the stored size and crop="pad" nothing changes: ops.augment_u8 / ops.mix_u8.
        erase: Random Erasing -- a dict of prob, scale, ratio (erase_table's; defaults 0.25, (0.02, 1/3), (0.3, 1/0.3)) and mode
        ("pixel": standard-normal noise per value, the default; "const": zeros, the normalised mean).  Every batch then comes from
        ops.erase_u8, at any size; None (default): nothing changes.
        randaug: RandAugment -- a dict of n_ops, magnitude, mstd, prob, fill, ops (randaug_table's; defaults 2, 9, 0.5, 0.5, (128, 128,
        128), timm's "increasing" ops).  The dataset then holds ONE second uint8 buffer of the images' size, allocated here;
        batches() fills it once per epoch with ops.randaugment_u8 and every batch kernel reads it in place of the images (so two
        epochs of one dataset are not iterated at the same time).  The images are at most 24 576 bytes each.  None (default): nothing
        is allocated or launched and the batch kernels read the images themselves."""
        images = torch.as_tensor(images)
        labels = torch.as_tensor(labels)
        if images.dtype != torch.uint8 or images.dim() not in (3, 4):
            raise ValueError(f"GpuDataset: images have dtype {images.dtype} and shape {tuple(images.shape)}, expected uint8 [N, H, W, C] or [N, H, W]")
        if labels.dtype.is_floating_point or labels.dtype == torch.bool or tuple(labels.shape) != (images.shape[0],):
            raise ValueError(f"GpuDataset: labels have dtype {labels.dtype} and shape {tuple(labels.shape)}, expected integers, [{images.shape[0]}]")
        self.lut_cpu = make_lut(mean, std)
        self.chw = (int(images.shape[3]) if images.dim() == 4 else 1, int(images.shape[1]), int(images.shape[2]))
        if self.lut_cpu.shape[0] != self.chw[0]:
            raise ValueError(f"GpuDataset: mean/std have {self.lut_cpu.shape[0]} entries, the images {self.chw[0]} channels")
        self.pad = (int(pad), int(pad)) if isinstance(pad, int) else (int(pad[0]), int(pad[1]))
        self.flip = bool(flip)
        if crop not in ("pad", "rrc"):
            raise ValueError(f"GpuDataset: crop '{crop}' is 'pad' or 'rrc'")
        self.crop, self.rrc_scale, self.rrc_ratio = crop, tuple(rrc_scale), tuple(rrc_ratio)
        self.out_hw = self.chw[1:] if out_size is None else \
            (int(out_size), int(out_size)) if isinstance(out_size, int) else (int(out_size[0]), int(out_size[1]))
        if min(self.out_hw) < 1:
            raise ValueError(f"GpuDataset: out_size={out_size} must be positive")
        self.erase = None if erase is None else _erase_config(erase)
        self.randaug = None if randaug is None else _randaug_config(randaug)
        if self.randaug is not None and self.chw[0] * self.chw[1] * self.chw[2] > ops._lib.RA_MAX_BYTES:
            raise ops.KanvitError(f"GpuDataset: randaug takes images of at most {ops._lib.RA_MAX_BYTES} bytes (they live in LDS); these are "
                                  f"{self.chw[1]} x {self.chw[2]} x {self.chw[0]}")
        self.resample = crop != "pad" or self.out_hw != self.chw[1:] or self.erase is not None      # False: augment_u8 / mix_u8
        self.device = torch.device(device)
        self.images = images.contiguous().to(self.device)
        self.labels = labels.to(torch.int64).contiguous().to(self.device)
        self.lut = self.lut_cpu.to(self.device)
        self.noise = normal_table().to(self.device) if self.erase is not None and self.erase["mode"] == "pixel" else None
        self.randaug_buffer = torch.empty_like(self.images) if self.randaug is not None else None

    @classmethod
    def from_npz(cls, path, split, device, pad=0, flip=False, **resample):
        """The `split` ('train' or 'test') of an .npz in this module's layout; mean / std from the file, else from x_train."""
        if split not in ("train", "test"):
            raise ValueError(f"GpuDataset.from_npz: split '{split}' is 'train' or 'test'")
        return cls.from_arrays(load_npz(path), path, split, device, pad=pad, flip=flip, **resample)

    @classmethod
    def from_arrays(cls, blob, path, split, device, pad=0, flip=False, **resample):
        """`resample`: out_size, crop, rrc_scale, rrc_ratio, erase, randaug, as the constructor takes them."""
        if f"x_{split}" not in blob:
            _fail(path, f"x_{split}", "is missing")
        mean, std = (blob["mean"], blob["std"]) if "mean" in blob else channel_stats(blob["x_train"])
        return cls(torch.from_numpy(blob[f"x_{split}"]), torch.from_numpy(blob[f"y_{split}"].astype(np.int64)), mean.astype(np.float32),
                   std.astype(np.float32), device, pad=pad, flip=flip, **resample)

    def __len__(self):
        return int(self.images.shape[0])

    def n_batches(self, batch_size, world=1):
        return -(-(-(-len(self) // world)) // batch_size)

    def loader(self, batch_size, epoch=0, seed=0, rank=0, world=1, shuffle=True):
        return Batches(self, batch_size, epoch, seed, rank, world, shuffle)

    def batches(self, batch_size, epoch, seed, rank=0, world=1, shuffle=True, mix=None):
        """Generator of (x, y) device tensors for one epoch: x float32 [b, C, H, W], y int64 [b]; the last batch is short (a DataLoader
        with drop_last=False).  The index list is checked against [0, N) on the CPU and goes to the device once per epoch.

        mix: the keyword arguments of mix_table after hw (mixup_alpha, cutmix_alpha, prob, switch_prob) as a dict -- Mixup / CutMix.
        The epoch's table is drawn and checked on the CPU and uploaded once, next to the index list, and every batch is one
        ops.mix_u8 launch yielding (x, y, y2, w): y2 int64 [b] the partner's label (y where the sample is not mixed), w float32 [b]
        the weight of y.  Without `mix` nothing changes: (x, y) through ops.augment_u8.

        A dataset with an out_size of its own or crop="rrc" yields x float32 [b, C, OH, OW] from one ops.resample_u8 launch per batch
        instead: the epoch's crop table (crop_table) is drawn, checked and uploaded once, like the mix table, which is then drawn
        at hw = out_size; the evaluation transform (crop="pad", pad 0, no flip) passes no table at all.

        A dataset with `erase` goes the same way through ops.erase_u8: the epoch's erase table (erase_table at hw = out_size) is drawn,
        checked and uploaded once like the others; the noise table went to the device with the dataset.

        A dataset with `randaug` first draws, checks and uploads the epoch's RandAugment table (randaug_table) and runs
        ops.randaugment_u8 over the WHOLE dataset into its second buffer -- on every rank, because a partner can be any index -- and
        the launches above read that buffer in place of the images."""
        if batch_size < 1:
            raise ValueError(f"GpuDataset.batches: batch_size={batch_size}")
        idx = epoch_indices(len(self), epoch, seed, rank, world, shuffle)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError(f"GpuDataset.batches: an index outside [0, {len(self)})")
        idx = idx.to(self.device)
        images = self._epoch_images(epoch, seed)
        if self.resample:
            yield from self._resampled(images, idx, batch_size, epoch, seed, mix)
            return
        if mix is None:
            for i in range(0, idx.numel(), batch_size):
                yield ops.augment_u8(images, self.labels, idx[i:i + batch_size], self.lut, self.pad, self.flip, seed, epoch)
            return
        partner, weight, box = self._mix_tables(epoch, seed, self.chw[1:], mix)
        for i in range(0, idx.numel(), batch_size):
            yield ops.mix_u8(images, self.labels, idx[i:i + batch_size], self.lut, partner, weight, box, self.pad, self.flip, seed, epoch)

    def _epoch_images(self, epoch, seed):
        """The images the epoch's batch kernels read: the stored ones, or with `randaug` the second buffer after this epoch's pass."""
        if self.randaug is None:
            return self.images
        table = randaug_table(len(self), epoch, seed, self.chw[1:], **self.randaug)
        table = ops.randaug_check_table(table, len(self)).contiguous().to(self.device)
        return ops.randaugment_u8(self.images, table, out=self.randaug_buffer)

    def _mix_tables(self, epoch, seed, hw, mix):
        """The epoch's mix table at output size hw, checked on the CPU, on the device."""
        table = mix_table(len(self), epoch, seed, hw, **mix)
        if tuple(table.partner.shape) != (len(self),) or int(table.partner.min()) < -1 or int(table.partner.max()) >= len(self):
            raise IndexError(f"GpuDataset.batches: the mix table names a partner outside [-1, {len(self)}) or is not of length {len(self)}")
        return tuple(t.contiguous().to(self.device) for t in table)

    def _resampled(self, images, idx, batch_size, epoch, seed, mix):
        """batches() through ops.resample_u8, or ops.erase_u8 with `erase`: (x, y), or (x, y, y2, w) with `mix`."""
        n, crop = len(self), None
        if self.crop != "pad" or self.pad != (0, 0) or self.flip:
            crop = crop_table(n, epoch, seed, self.chw[1:], self.crop, pad=self.pad, flip=self.flip, scale=self.rrc_scale, ratio=self.rrc_ratio)
            if tuple(crop.shape) != (n, 5) or crop.dtype != torch.int32 or int(crop[:, 2:4].min()) < 1:
                raise ValueError(f"GpuDataset.batches: the crop table is not int32 [{n}, 5] or holds an empty box")
            crop = crop.contiguous().to(self.device)
        tables = self._mix_tables(epoch, seed, self.out_hw, mix) if mix is not None else ()
        if self.erase is None:
            for i in range(0, idx.numel(), batch_size):
                yield ops.resample_u8(images, self.labels, idx[i:i + batch_size], self.lut, self.out_hw, crop, *tables)
            return
        erase = erase_table(n, epoch, seed, self.out_hw, self.erase["prob"], self.erase["scale"], self.erase["ratio"])
        if tuple(erase.shape) != (n, 4) or erase.dtype != torch.int32:
            raise ValueError(f"GpuDataset.batches: the erase table is not int32 [{n}, 4]")
        erase, key = erase.contiguous().to(self.device), erase_noise_key(seed, epoch)
        for i in range(0, idx.numel(), batch_size):
            yield ops.erase_u8(images, self.labels, idx[i:i + batch_size], self.lut, self.out_hw, crop, *tables, erase=erase,
                               noise=self.noise, noise_key=key)
