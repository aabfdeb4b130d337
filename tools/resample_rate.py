"""What the resize / RandomResizedCrop form of the batch kernel costs, on the GPU:

  (a) ops.resample_u8 at B = 128, 32x32x3 -> 224x224 on a generated dataset of CIFAR's size: with the pad-4 crop table, with the
      RandomResizedCrop table, with that table plus the Mixup / CutMix tables of --mixup 0.8 --cutmix 1.0, and with no table (the
      evaluation transform) -- against
        the two-pass way: ops.augment_u8 followed by F.interpolate(..., size=224, mode="bilinear") on the GPU;
        for per-sample boxes, stock torch: the normalised images, F.affine_grid from per-sample matrices and F.grid_sample;
        the store floor: the 4 B C S S bytes every form must write, at the 6.1 TB/s plain stores reach (MI355X_MICROARCH);
      and at the identity size (32x32 -> 32x32, pad table) against ops.augment_u8 itself.
      Device time per call of a replayed graph that holds --launches of them.
  (b) one train.py step at the ViT-B/16 geometry (--n-patches 14 --d-hidden 768 --n-heads 12 --n-blocks 12, batch 128, ChebyKAN):
      --data-npz FILE --resize 224 on stored 32x32 images against --synthetic --image-size 224, `epoch_seconds` / steps of every
      epoch after the first, one process per run, the variants alternated.

    python tools/resample_rate.py [--out profiles/resample_u8.md] [--reps 5] [--launches 50] [--epochs 3] [--steps 20] [--skip-train]

Needs the GPU: there is no CPU fall-back and no figure without a run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-vit_amd"))

N, CLASSES, BATCH = 50000, 100, 128
H, W, CH, PAD, S = 32, 32, 3, 4, 224
MEAN, STD = [0.5071, 0.4867, 0.4408], [0.2675, 0.2565, 0.2761]
STORE_TBS = 6.1                     # plain dword-per-lane stores, chip-wide (the microarchitecture notes give 6.0-6.2)
VITB = ["--model-type", "cheby", "--n-patches", "14", "--d-hidden", "768", "--n-heads", "12", "--n-blocks", "12", "--batch-size", str(BATCH),
        "--no-step-metrics"]
CHILD = ("import sys, json; sys.path.insert(0, 'kan-vit_amd'); import train; h = train.main(train.parse(sys.argv[1:])); "
         "print('EPOCH_SECONDS ' + json.dumps(h['epoch_seconds']))")


def replayed_us(fn, launches, reps):
    """Device microseconds per call of fn(i) when `launches` of them are captured in one graph and replayed: no host between them."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(0)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(launches):
            fn(i)
    out = []
    for rep in range(reps + 1):                                     # the first replay is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        if rep:
            out.append(1e3 * e0.elapsed_time(e1) / launches)
    return out


def train_run(argv, timeout=900):
    """One train.py process; returns its epoch_seconds after the first epoch."""
    r = subprocess.run([sys.executable, "-c", CHILD, *argv], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"train.py ended with {r.returncode}; no further run is started:\n{r.stdout[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("EPOCH_SECONDS ")][-1]
    return json.loads(line.split(" ", 1)[1])[1:]


def fmt(vs, scale=1.0, digits=2):
    return ", ".join(f"{v * scale:.{digits}f}" for v in vs)


def affine_matrices(crop, hw):
    """[n, 2, 3] float32: the F.affine_grid matrices (align_corners=False) that map the output square onto each crop row's box."""
    Hs, Ws = hw
    y0, x0, bh, bw, fl = (crop[:, k].double() for k in range(5))
    sx = (bw / Ws) * (1 - 2 * fl)                                   # a flipped box runs right to left in the stored image
    cx = (2 * x0 + bw) / Ws - 1
    cx = torch.where(fl > 0, -cx, cx)
    theta = torch.zeros(crop.shape[0], 2, 3, dtype=torch.float64)
    theta[:, 0, 0], theta[:, 0, 2] = sx, cx
    theta[:, 1, 1], theta[:, 1, 2] = bh / Hs, (2 * y0 + bh) / Hs - 1
    return theta.float()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_u8.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="steps per epoch of part (b)")
    ap.add_argument("--skip-train", action="store_true", help="part (a) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/resample_rate.py measures on the GPU; none is visible")
    import torch.nn.functional as F
    from kanvit import data, ops
    dev, med = torch.device("cuda:0"), statistics.median
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (N, H, W, CH), dtype=np.uint8)
    labels = rng.integers(0, CLASSES, N).astype(np.int64)
    ds = data.GpuDataset(torch.from_numpy(images), torch.from_numpy(labels), MEAN, STD, dev, pad=PAD, flip=True)
    idx = data.epoch_indices(N, 0, 0).to(dev)
    pad_cpu, rrc_cpu = data.crop_table(N, 0, 0, (H, W), "pad", pad=PAD), data.crop_table(N, 0, 0, (H, W), "rrc")
    pad_t, rrc_t = pad_cpu.to(dev), rrc_cpu.to(dev)
    mix = data.mix_table(N, 0, 0, (S, S), mixup_alpha=0.8, cutmix_alpha=1.0)
    mixed_rows, cut_rows = int((mix.partner >= 0).sum()), int((mix.box[:, 1] > mix.box[:, 0]).sum())
    mix_t = [t.to(dev) for t in mix]
    theta = affine_matrices(rrc_cpu, (H, W)).to(dev)
    out = torch.empty((BATCH, CH, S, S), device=dev)
    small = torch.empty((BATCH, CH, H, W), device=dev)
    steps = N // BATCH

    def batch(i):
        return idx[(i % steps) * BATCH:(i % steps + 1) * BATCH]

    def two_pass(i):
        x, _ = ops.augment_u8(ds.images, ds.labels, batch(i), ds.lut, PAD, True, 0, 0, out=small)
        return F.interpolate(x, size=(S, S), mode="bilinear", align_corners=False)

    def grid_sampled(i):
        b = batch(i)
        x, _ = ops.augment_u8(ds.images, ds.labels, b, ds.lut, 0, False, 0, 0, out=small)      # normalise only
        grid = F.affine_grid(theta[b], (BATCH, CH, S, S), align_corners=False)
        return F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False)

    # how far what the stock routes compute is from the kernel's output: shown once, so that the timings compare like with like
    b0 = batch(0)
    ours = ops.resample_u8(ds.images, ds.labels, b0, ds.lut, (S, S), rrc_t)[0]
    diff_grid = float((grid_sampled(0) - ours).abs().max())
    diff_two = float((two_pass(0) - ops.resample_u8(ds.images, ds.labels, b0, ds.lut, (S, S), pad_t)[0]).abs().max())

    cases = [
        ("`resample_u8`, pad-4 table", lambda i: ops.resample_u8(ds.images, ds.labels, batch(i), ds.lut, (S, S), pad_t, out=out)),
        ("`resample_u8`, RandomResizedCrop table", lambda i: ops.resample_u8(ds.images, ds.labels, batch(i), ds.lut, (S, S), rrc_t, out=out)),
        ("`resample_u8`, RandomResizedCrop + Mixup / CutMix tables", lambda i: ops.resample_u8(ds.images, ds.labels, batch(i), ds.lut, (S, S), rrc_t, *mix_t, out=out)),
        ("`resample_u8`, no table (evaluation)", lambda i: ops.resample_u8(ds.images, ds.labels, batch(i), ds.lut, (S, S), None, out=out)),
        ("`augment_u8` + `F.interpolate` (two passes)", two_pass),
        ("`augment_u8` (pad 0) + `F.affine_grid` + `F.grid_sample`", grid_sampled),
    ]
    us = {name: replayed_us(fn, a.launches, a.reps) for name, fn in cases}
    us_id = replayed_us(lambda i: ops.resample_u8(ds.images, ds.labels, batch(i), ds.lut, (H, W), pad_t, out=small), a.launches, a.reps)
    us_aug = replayed_us(lambda i: ops.augment_u8(ds.images, ds.labels, batch(i), ds.lut, PAD, True, 0, 0, out=small), a.launches, a.reps)
    px = BATCH * CH * S * S
    floor_us = 4 * px / (STORE_TBS * 1e6)
    lines = [
        "# Bilinear resize and RandomResizedCrop in the batch kernel (`tools/resample_rate.py`)",
        "",
        f"Device: {torch.cuda.get_device_name(0)}. Device time per call from a replayed graph of {a.launches} calls, median of {a.reps} replays "
        "after one warm-up replay, every figure listed.",
        "",
        f"## (a) `ops.resample_u8`: B = {BATCH}, {H}x{W}x{CH} -> {S}x{S}, N = {N}",
        "",
        f"Every form stores {4 * px / 1e6:.2f} MB; at the {STORE_TBS} TB/s of plain stores that is {floor_us:.1f} us, the store floor. The batch's "
        f"source pixels are {BATCH * H * W * CH / 1e3:.0f} KB. The mix table is `mix_table(N, 0, 0, ({S}, {S}), mixup_alpha=0.8, cutmix_alpha=1.0)`: "
        f"{mixed_rows} of {N} rows mixed, {cut_rows} of them CutMix. What the stock routes compute, on the first batch: two passes (pad table) "
        f"max |difference| {diff_two:.2e} -- the same resize up to rounding; `grid_sample` (RandomResizedCrop table) {diff_grid:.2e} -- the same "
        "sampling points, but its taps are clamped to the image, not to the box, so pixels within half a source pixel of a box edge differ.",
        "",
        "| call | us / call | every replay | stores, GB/s | x store floor |",
        "|---|---|---|---|---|",
    ]
    for name, _ in cases:
        m = med(us[name])
        lines.append(f"| {name} | {m:.2f} | {fmt(us[name])} | {4 * px / m / 1e3:.0f} | {m / floor_us:.2f} |")
    first = med(us[cases[0][0]])
    lines += [
        "",
        f"Two passes / `resample_u8` (pad table): {med(us[cases[4][0]]) / first:.2f}. `grid_sample` route / `resample_u8` (RandomResizedCrop "
        f"table): {med(us[cases[5][0]]) / med(us[cases[1][0]]):.2f}. Not a gate.",
        "",
        f"At the identity size ({H}x{W} -> {H}x{W}, pad table; what `crop=\"rrc\"` without `out_size` launches): `resample_u8` "
        f"{med(us_id):.2f} us ({fmt(us_id)}), `augment_u8` {med(us_aug):.2f} us ({fmt(us_aug)}).",
        "",
    ]
    del ds, out, small
    torch.cuda.empty_cache()
    if a.skip_train:
        lines += ["## (b) `train.py`: not measured (`--skip-train`)", ""]
    else:
        n_img = BATCH * a.steps
        rows = {"--data-npz --resize 224": [], "--synthetic --image-size 224": []}
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "small.npz")
            np.savez(path, x_train=images[:n_img], y_train=labels[:n_img], mean=np.array(MEAN, np.float32), std=np.array(STD, np.float32))
            argv = {"--data-npz --resize 224": ["--data-npz", path, "--resize", str(S)],
                    "--synthetic --image-size 224": ["--synthetic", "--image-size", str(S), "--steps-per-epoch", str(a.steps)]}
            for rep in range(2):                                    # alternated, the second round in the opposite order
                for name in (list(rows) if rep == 0 else list(rows)[::-1]):
                    rows[name].append(train_run([*VITB, "--epochs", str(a.epochs), "--log-dir", os.path.join(tmp, f"log{rep}{len(name)}"), *argv[name]]))
        lines += [
            f"## (b) One `train.py` step, ViT-B/16 ChebyKAN (`{' '.join(VITB)}`), {a.steps} steps per epoch",
            "",
            "`epoch_seconds` (host clock around work that ends in the epoch's one synchronise) over the steps, for every epoch after the "
            f"first; two runs per variant, one process each, alternated: run 1 in the order of the table, run 2 in the opposite order. The "
            f"`--data-npz` file holds {n_img} stored {H}x{W} images.",
            "",
            "| variant | median, ms / step | run 1, ms / step | run 2, ms / step |",
            "|---|---|---|---|",
        ]
        for name in rows:
            both = rows[name][0] + rows[name][1]
            lines.append(f"| `{name}` | {med(both) * 1e3 / a.steps:.2f} | {fmt(rows[name][0], 1e3 / a.steps)} | {fmt(rows[name][1], 1e3 / a.steps)} |")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
