"""Reference for the GPU-resident data path (kanvit/data.py, csrc/batch_u8.hip): the per-sample hash of include/kanvit.h in Python
integers, and the reference's transform order (train.py:100-118: RandomHorizontalFlip, RandomCrop(size, padding) with zero padding
on the uint8 image, ToTensor, Normalize) in CPU torch with the parameters the hash gives."""
import torch
import torch.nn.functional as F

M64 = (1 << 64) - 1


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_params(seed, epoch, idx, pad_y, pad_x, flip_enabled=True):
    h = mix((mix((mix(seed & M64) + epoch) & M64) + idx) & M64)
    return ((h & 0xFFFFF) % (2 * pad_y + 1), ((h >> 20) & 0xFFFFF) % (2 * pad_x + 1), (h >> 40) & 1 if flip_enabled else 0)


def params(seed, epoch, indices, pad_y, pad_x, flip_enabled=True):
    return [sample_params(seed, epoch, int(i), pad_y, pad_x, flip_enabled) for i in indices]


def augment(images, idx, mean, std, pad, flip, seed, epoch):
    """images uint8 [N, H, W, C] or [N, H, W] (CPU), idx a list of ints -> float32 [B, C, H, W]."""
    pad_y, pad_x = (pad, pad) if isinstance(pad, int) else pad
    if images.dim() == 3:
        images = images[..., None]
    N, H, W, C = images.shape
    mean = torch.as_tensor(mean, dtype=torch.float32).reshape(C, 1, 1)
    std = torch.as_tensor(std, dtype=torch.float32).reshape(C, 1, 1)
    out = torch.empty(len(idx), C, H, W, dtype=torch.float32)
    for b, i in enumerate(idx):
        dy, dx, fl = sample_params(seed, epoch, int(i), pad_y, pad_x, flip)
        u8 = images[int(i)].permute(2, 0, 1)                        # CHW, uint8
        if fl:
            u8 = u8.flip(-1)
        u8 = F.pad(u8, (pad_x, pad_x, pad_y, pad_y))                # zeros, on the uint8 image
        u8 = u8[:, dy:dy + H, dx:dx + W]
        out[b] = (u8.float().div(255) - mean).div(std)
    return out
