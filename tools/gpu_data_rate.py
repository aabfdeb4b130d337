"""What the GPU-resident data path (kanvit/data.py, csrc/batch_u8.hip) delivers, on the GPU, for train.py's default geometry
(32x32x3 images, batch 128, random crop with padding 4, random flip) on a generated dataset of CIFAR's size (50 000 images):

  (a) GpuDataset.batches alone: images/s of whole epochs (host loop, allocation and launch included; device events around each
      epoch), and of the kernel alone (back-to-back launches into one output buffer);
  (b) train.py's step time with --data-npz against --synthetic (the existing synthetic stream: the ceiling), same commit, same
      process, runs alternated; the first epoch of every run (graph capture, first launches) is left out.

    python tools/gpu_data_rate.py [--out profiles/gpu_data_rate.md] [--reps 3] [--epochs 4] [--model-type cheby]

Needs the GPU: there is no CPU fall-back and no figure without a run."""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-vit_amd"))

N, H, W, C, BATCH, PAD = 50000, 32, 32, 3, 128, 4
MEAN, STD = [0.5071, 0.4867, 0.4408], [0.2675, 0.2565, 0.2761]


def stream_rate(ds, reps):
    """Whole epochs of GpuDataset.batches, nothing consuming them: ms per epoch, one figure per repetition."""
    out = []
    for rep in range(reps + 1):                                 # the first epoch is the warm-up
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        n = 0
        for x, y in ds.batches(BATCH, rep, 0):
            n += len(y)
        t1.record()
        t1.synchronize()
        assert n == N
        if rep:
            out.append(t0.elapsed_time(t1))
    return out


def kernel_rate(ds, reps, launches=400):
    """The kernel alone: `launches` back-to-back calls on one batch of indices into one output buffer; microseconds per launch."""
    from kanvit import data, ops
    idx = data.epoch_indices(N, 0, 0)[:BATCH].to(ds.device)
    buf = torch.empty(BATCH, C, H, W, device=ds.device)
    out = []
    for rep in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            ops.augment_u8(ds.images, ds.labels, idx, ds.lut, ds.pad, ds.flip, 0, rep, out=buf)
        t1.record()
        t1.synchronize()
        if rep:
            out.append(1e3 * t0.elapsed_time(t1) / launches)
    return out


def train_step_ms(argv, epochs):
    """One train.main run; ms per step of every epoch after the first."""
    import train
    hist = train.main(train.parse(argv + ["--epochs", str(epochs)]))
    steps = len(hist["losses"]) // epochs
    return [1e3 * s / steps for s in hist["epoch_seconds"][1:]], steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpu_data_rate.md"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--model-type", default="cheby")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_data_rate.py measures on the GPU; none is visible")
    from kanvit import data
    rng = np.random.default_rng(0)
    arrays = dict(x_train=rng.integers(0, 256, (N, H, W, C), dtype=np.uint8), y_train=rng.integers(0, 100, N).astype(np.int64),
                  mean=np.array(MEAN, np.float32), std=np.array(STD, np.float32))
    ds = data.GpuDataset(arrays["x_train"], arrays["y_train"], MEAN, STD, "cuda:0", pad=PAD, flip=True)
    epoch_ms = stream_rate(ds, a.reps)
    launch_us = kernel_rate(ds, a.reps)
    del ds
    steps_per_epoch = -(-N // BATCH)
    common = ["--model-type", a.model_type, "--graph", "--no-step-metrics"]
    synth, npz = [], []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cifar_sized.npz")
        np.savez(path, **arrays)
        for rep in range(a.reps):                               # alternated: other work shares the host
            s, n_s = train_step_ms(common + ["--synthetic", "--steps-per-epoch", str(steps_per_epoch), "--log-dir", os.path.join(tmp, f"s{rep}")], a.epochs)
            d, n_d = train_step_ms(common + ["--data-npz", path, "--log-dir", os.path.join(tmp, f"d{rep}")], a.epochs)
            assert n_s == n_d == steps_per_epoch
            synth += s
            npz += d
    med = statistics.median
    bytes_in, bytes_out = BATCH * H * W * C + BATCH * 8 * 2, BATCH * C * H * W * 4 + BATCH * 8
    ratio = med(npz) / med(synth)
    lines = [
        "# GPU-resident data path: what it delivers (`tools/gpu_data_rate.py`)",
        "",
        f"Device: {torch.cuda.get_device_name(0)}. Generated dataset of CIFAR's size: {N} images {H}x{W}x{C} uint8, batch {BATCH}, "
        f"random crop with padding {PAD}, random flip. Medians over {a.reps} repetitions, every single figure listed; device events (a) and "
        "a host clock around an epoch that ends in its one synchronise (b).",
        "",
        "## (a) `GpuDataset.batches` alone",
        "",
        "| what | per unit | images/s | repetitions |",
        "|---|---|---|---|",
        f"| whole epochs ({steps_per_epoch} batches: host loop, allocation, launch) | {med(epoch_ms):.2f} ms / epoch | "
        f"{N / med(epoch_ms) * 1e3:,.0f} | {', '.join(f'{v:.2f}' for v in epoch_ms)} ms |",
        f"| the kernel alone (400 back-to-back launches, one output buffer) | {med(launch_us):.2f} us / launch | "
        f"{BATCH / med(launch_us) * 1e6:,.0f} | {', '.join(f'{v:.2f}' for v in launch_us)} us |",
        "",
        f"Per batch the kernel reads {bytes_in / 1e6:.3f} MB (images, indices, labels) and writes {bytes_out / 1e6:.3f} MB: "
        f"{(bytes_in + bytes_out) / med(launch_us) / 1e3:.1f} GB/s over the back-to-back launch time, which at this size is launch cost, not bandwidth.",
        "",
        f"## (b) `train.py --model-type {a.model_type} --graph --no-step-metrics`, default geometry, {steps_per_epoch} steps per epoch",
        "",
        "| stream | ms / step (median) | images/s | every epoch after the first, ms / step |",
        "|---|---|---|---|",
        f"| `--synthetic` (the ceiling) | {med(synth):.4f} | {BATCH / med(synth) * 1e3:,.0f} | {', '.join(f'{v:.4f}' for v in synth)} |",
        f"| `--data-npz` | {med(npz):.4f} | {BATCH / med(npz) * 1e3:,.0f} | {', '.join(f'{v:.4f}' for v in npz)} |",
        "",
        f"Ratio `--data-npz` / `--synthetic`: **{ratio:.4f}** ({(ratio - 1) * 100:+.2f} %). Expectation from the byte counts (about 2 MB of traffic and one "
        "launch per step): a few percent at most. This is an expectation, not a gate. Both streams produce a batch with device "
        "kernels and copy it into the captured step's buffers; the last batch of the `--data-npz` epoch is short (80 images) and runs eagerly.",
        "",
        "The torchvision path (`cifar_loaders`: PIL transforms in 8 workers, a pinned copy per batch) was not measured: torchvision is not installed.",
        "",
    ]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
