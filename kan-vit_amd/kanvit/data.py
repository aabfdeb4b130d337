"""Training and evaluation batches from a dataset that stays on the GPU as uint8.

CIFAR-100's training set is 154 MB as uint8 and MNIST's 47 MB: they fit in HBM thousands of times over.  GpuDataset keeps the images
(NHWC, as the arrays come) and the labels on the device and produces every batch with ONE kernel (ops.augment_u8, csrc/augment.hip):
gather by index, random crop out of the zero-padded image, random horizontal flip, ToTensor and Normalize -- the reference's
transforms (train.py:100-118) without its DataLoader workers, its PIL round trip, its host-to-device copy per batch, and without
torchvision.  Per batch the device reads B*H*W*C bytes and writes 4*B*C*H*W.

The crop offsets and the flip of a sample are a pure function of (seed, epoch, sample index) (include/kanvit.h), and the epoch's
order is a permutation drawn from a CPU generator seeded by (seed, epoch): a run is reproducible across batch sizes and
data-parallel layouts, and needs no RNG state on the device.

Mixup and CutMix ride on the same pass: mix_table draws one table per epoch from (seed, epoch), indexed by dataset index, and
batches(mix=...) hands it to ops.mix_u8, which blends or pastes the partner under the partner's own crop and flip -- a sample's pixels
and soft targets stay a function of (seed, epoch, sample index).

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

    def __init__(self, images, labels, mean, std, device, pad=0, flip=False):
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
        self.device = torch.device(device)
        self.images = images.contiguous().to(self.device)
        self.labels = labels.to(torch.int64).contiguous().to(self.device)
        self.lut = self.lut_cpu.to(self.device)

    @classmethod
    def from_npz(cls, path, split, device, pad=0, flip=False):
        """The `split` ('train' or 'test') of an .npz in this module's layout; mean / std from the file, else from x_train."""
        if split not in ("train", "test"):
            raise ValueError(f"GpuDataset.from_npz: split '{split}' is 'train' or 'test'")
        return cls.from_arrays(load_npz(path), path, split, device, pad=pad, flip=flip)

    @classmethod
    def from_arrays(cls, blob, path, split, device, pad=0, flip=False):
        if f"x_{split}" not in blob:
            _fail(path, f"x_{split}", "is missing")
        mean, std = (blob["mean"], blob["std"]) if "mean" in blob else channel_stats(blob["x_train"])
        return cls(torch.from_numpy(blob[f"x_{split}"]), torch.from_numpy(blob[f"y_{split}"].astype(np.int64)), mean.astype(np.float32),
                   std.astype(np.float32), device, pad=pad, flip=flip)

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
        the weight of y.  Without `mix` nothing changes: (x, y) through ops.augment_u8."""
        if batch_size < 1:
            raise ValueError(f"GpuDataset.batches: batch_size={batch_size}")
        idx = epoch_indices(len(self), epoch, seed, rank, world, shuffle)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError(f"GpuDataset.batches: an index outside [0, {len(self)})")
        idx = idx.to(self.device)
        if mix is None:
            for i in range(0, idx.numel(), batch_size):
                yield ops.augment_u8(self.images, self.labels, idx[i:i + batch_size], self.lut, self.pad, self.flip, seed, epoch)
            return
        table = mix_table(len(self), epoch, seed, self.chw[1:], **mix)
        if tuple(table.partner.shape) != (len(self),) or int(table.partner.min()) < -1 or int(table.partner.max()) >= len(self):
            raise IndexError(f"GpuDataset.batches: the mix table names a partner outside [-1, {len(self)}) or is not of length {len(self)}")
        partner, weight, box = (t.contiguous().to(self.device) for t in table)
        for i in range(0, idx.numel(), batch_size):
            yield ops.mix_u8(self.images, self.labels, idx[i:i + batch_size], self.lut, partner, weight, box, self.pad, self.flip, seed, epoch)
