"""Fixture loading helpers shared by the CPU and GPU tests."""
import contextlib
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_npz(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def bf16_bits_to_f32(a):
    return torch.from_numpy(a.astype(np.int32) << 16).view(torch.float32).reshape(a.shape).clone()


def state_dict_from(blob, prefix=""):
    """Rebuild a torch state dict from '<prefix>sd.<key>' / '<prefix>sdbf16.<key>' entries."""
    sd = {}
    for k, v in blob.items():
        if k.startswith(prefix + "sd."):
            sd[k[len(prefix) + 3:]] = torch.from_numpy(np.array(v))
        elif k.startswith(prefix + "sdbf16."):
            sd[k[len(prefix) + 7:]] = bf16_bits_to_f32(v)
    return sd


def grads_from(blob, prefix=""):
    return {k[len(prefix) + 5:]: torch.from_numpy(np.array(v)) for k, v in blob.items() if k.startswith(prefix + "grad.")}


def T(a):
    return torch.from_numpy(np.array(a))


def max_err(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max())


def rel_err(a, b, floor=1e-3):
    """max |a-b| / max(max|b|, floor): scale-aware error for gradient tensors.  The
    floor keeps tensors that are mathematically zero (e.g. the key-bias gradient of
    softmax attention, which is shift invariant) from being compared noise-to-noise."""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def close(a, b, rtol=1e-4, atol=2e-6):
    """max|a-b| <= atol + rtol*max|b| -- for tensors that may be mathematically zero."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) <= atol + rtol * float(b.abs().max())


def kernel_name(raw):
    """A device kernel's profiler name as `name<args>`: no `void`, no namespace, no parameter list
    ('void (anonymous namespace)::kan_fwd_reg_kernel<1, 2, 3, 4, 5, true>(LayerArgs)' -> 'kan_fwd_reg_kernel<1, 2, 3, 4, 5, true>')."""
    s = raw.strip()
    if s.startswith("void "):
        s = s[5:]
    s = s.replace("(anonymous namespace)::", "")
    depth, cut, ns = 0, len(s), 0
    for i, c in enumerate(s):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            cut = i
            break
        elif c == ":" and depth == 0 and s[i + 1:i + 2] == ":":
            ns = i + 2
    return s[ns:cut].strip()


@contextlib.contextmanager
def record_kernels():
    """with record_kernels() as names: ...  -- `names` becomes the set of device kernels launched inside the block, normalised by
    kernel_name().  torch.profiler (device activity) sees every launch on the device, the library's hipLaunchKernelGGL ones included.
    A block that records no device kernel at all raises: the recorder is not working, and a form assertion built on it would
    be meaningless."""
    from torch.profiler import ProfilerActivity, profile
    names = set()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA], acc_events=True) as prof:
        yield names
        torch.cuda.synchronize()
    for e in prof.events():
        if e.device_type != torch.autograd.DeviceType.CPU:
            names.add(kernel_name(e.name))
    assert names, "torch.profiler recorded no device kernel"
