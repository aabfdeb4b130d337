"""What Mixup / CutMix in the batch kernel and the fused soft-target loss cost, on the GPU:

  (a) ops.mix_u8 against ops.augment_u8 at B = 128, 32x32x3, pad 4, flip, on a generated dataset of CIFAR's size -- with the table of
      --mixup 0.8 --cutmix 1.0 (up to twice the bytes read for the same stores) and with an all-unmixed table (the table reads alone);
  (b) ops.soft_cross_entropy forward + backward against the torch launches it replaces at 128 x 100: plain cross-entropy, and Mixup
      pairs with label smoothing (where stock torch also builds the dense [B, C] target from two one-hots);
      both (a) and (b) as device time per call of a replayed graph that holds --launches of them;
  (c) train.py --graph --data-npz at the default geometry, `epoch_seconds` of every epoch after the first: with
      --mixup 0.8 --cutmix 1.0 --label-smoothing 0.1, without them, and (--parent DIR: a checkout of the parent commit, built) the
      parent's train.py -- one process per run, the variants alternated.

    python tools/batch_mix_rate.py [--out profiles/batch_mix.md] [--reps 5] [--launches 200] [--epochs 3] [--parent DIR] [--skip-train]

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

N, C, BATCH = 50000, 100, 128
H, W, CH, PAD = 32, 32, 3, 4
MEAN, STD = [0.5071, 0.4867, 0.4408], [0.2675, 0.2565, 0.2761]
MIX_FLAGS = ["--mixup", "0.8", "--cutmix", "1.0", "--label-smoothing", "0.1"]
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


def train_run(tree, argv, timeout=600):
    """One train.py process in `tree` (this checkout or the parent's); returns its epoch_seconds after the first epoch."""
    r = subprocess.run([sys.executable, "-c", CHILD, *argv], cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"train.py in {tree} ended with {r.returncode}; no further run is started:\n{r.stdout[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("EPOCH_SECONDS ")][-1]
    return json.loads(line.split(" ", 1)[1])[1:]


def fmt(vs, scale=1.0, digits=2):
    return ", ".join(f"{v * scale:.{digits}f}" for v in vs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_mix.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--model-type", default="cheby")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for part (c)")
    ap.add_argument("--skip-train", action="store_true", help="parts (a) and (b) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/batch_mix_rate.py measures on the GPU; none is visible")
    import torch.nn.functional as F
    from kanvit import data, ops
    dev, med = torch.device("cuda:0"), statistics.median
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (N, H, W, CH), dtype=np.uint8)
    labels = rng.integers(0, C, N).astype(np.int64)
    ds = data.GpuDataset(torch.from_numpy(images), torch.from_numpy(labels), MEAN, STD, dev, pad=PAD, flip=True)
    idx = data.epoch_indices(N, 0, 0).to(dev)
    table = data.mix_table(N, 0, 0, (H, W), mixup_alpha=0.8, cutmix_alpha=1.0)
    mixed_rows, cut_rows = int((table.partner >= 0).sum()), int((table.box[:, 1] > table.box[:, 0]).sum())
    on_dev = [t.to(dev) for t in table]
    none = [torch.full((N,), -1, dtype=torch.int64, device=dev), torch.ones(N, device=dev), torch.zeros((N, 4), dtype=torch.int32, device=dev)]
    out = torch.empty((BATCH, CH, H, W), device=dev)
    steps = N // BATCH

    def batch(i):
        return idx[(i % steps) * BATCH:(i % steps + 1) * BATCH]

    us_aug = replayed_us(lambda i: ops.augment_u8(ds.images, ds.labels, batch(i), ds.lut, PAD, True, 0, 0, out=out), a.launches, a.reps)
    us_mix = replayed_us(lambda i: ops.mix_u8(ds.images, ds.labels, batch(i), ds.lut, *on_dev, pad=PAD, flip=True, out=out), a.launches, a.reps)
    us_none = replayed_us(lambda i: ops.mix_u8(ds.images, ds.labels, batch(i), ds.lut, *none, pad=PAD, flip=True, out=out), a.launches, a.reps)

    g = torch.Generator(device=dev).manual_seed(0)
    z = (2.0 * torch.randn(BATCH, C, device=dev, generator=g)).requires_grad_(True)
    y1, y2 = torch.randint(0, C, (BATCH,), device=dev, generator=g), torch.randint(0, C, (BATCH,), device=dev, generator=g)
    w = torch.rand(BATCH, device=dev, generator=g)
    kept = []

    def torch_plain(i):
        kept.append(torch.autograd.grad(F.cross_entropy(z, y1), z))

    def fused_plain(i):
        kept.append(torch.autograd.grad(ops.soft_cross_entropy(z, y1), z))

    def torch_soft(i):
        target = w[:, None] * F.one_hot(y1, C) + (1 - w[:, None]) * F.one_hot(y2, C)
        kept.append(torch.autograd.grad(F.cross_entropy(z, target, label_smoothing=0.1), z))

    def fused_soft(i):
        kept.append(torch.autograd.grad(ops.soft_cross_entropy(z, y1, y2, w, 0.1), z))

    loss_us = {}
    for name, fn in (("torch_plain", torch_plain), ("fused_plain", fused_plain), ("torch_soft", torch_soft), ("fused_soft", fused_soft),
                     ("fused_plain_again", fused_plain), ("torch_plain_again", torch_plain)):       # the plain pair twice, in either order
        loss_us[name] = replayed_us(fn, a.launches, a.reps)
        kept.clear()
    px = BATCH * CH * H * W
    lines = [
        "# Mixup / CutMix in the batch kernel and the fused soft-target loss (`tools/batch_mix_rate.py`)",
        "",
        f"Device: {torch.cuda.get_device_name(0)}. Device time per call from a replayed graph of {a.launches} calls, median of {a.reps} replays "
        "after one warm-up replay, every figure listed.",
        "",
        f"## (a) `ops.mix_u8` against `ops.augment_u8`: B = {BATCH}, {H}x{W}x{CH}, pad {PAD}, flip, N = {N}",
        "",
        f"The table is `mix_table(N, 0, 0, ({H}, {W}), mixup_alpha=0.8, cutmix_alpha=1.0)`: {mixed_rows} of {N} rows mixed, {cut_rows} of them "
        f"CutMix. Every call stores {4 * px / 1e6:.2f} MB; `augment_u8` reads {px / 1e6:.2f} MB of pixels, `mix_u8` up to twice that.",
        "",
        "| call | us / call | every replay | stores, GB/s |",
        "|---|---|---|---|",
        f"| `augment_u8` | {med(us_aug):.2f} | {fmt(us_aug)} | {4 * px / med(us_aug) / 1e3:.0f} |",
        f"| `mix_u8`, Mixup + CutMix table | {med(us_mix):.2f} | {fmt(us_mix)} | {4 * px / med(us_mix) / 1e3:.0f} |",
        f"| `mix_u8`, all rows unmixed | {med(us_none):.2f} | {fmt(us_none)} | {4 * px / med(us_none) / 1e3:.0f} |",
        "",
        f"Ratio `mix_u8` / `augment_u8`: {med(us_mix) / med(us_aug):.2f} with the table, {med(us_none) / med(us_aug):.2f} unmixed. Not a gate.",
        "",
        f"## (b) Loss forward + backward at {BATCH} x {C}: `ops.soft_cross_entropy` against the torch launches it replaces",
        "",
        "Each call is the loss and `torch.autograd.grad` of it with respect to the logits. The torch soft form also builds the dense "
        "[B, C] target from two one-hots, as a training loop without the kernel would.",
        "",
        "| case | torch, us / call | every replay | fused, us / call | every replay | torch / fused |",
        "|---|---|---|---|---|---|",
        f"| plain cross-entropy | {med(loss_us['torch_plain']):.2f} | {fmt(loss_us['torch_plain'])} | {med(loss_us['fused_plain']):.2f} | "
        f"{fmt(loss_us['fused_plain'])} | {med(loss_us['torch_plain']) / med(loss_us['fused_plain']):.2f} |",
        f"| plain, other order | {med(loss_us['torch_plain_again']):.2f} | {fmt(loss_us['torch_plain_again'])} | {med(loss_us['fused_plain_again']):.2f} | "
        f"{fmt(loss_us['fused_plain_again'])} | {med(loss_us['torch_plain_again']) / med(loss_us['fused_plain_again']):.2f} |",
        f"| Mixup pairs + smoothing 0.1 | {med(loss_us['torch_soft']):.2f} | {fmt(loss_us['torch_soft'])} | {med(loss_us['fused_soft']):.2f} | "
        f"{fmt(loss_us['fused_soft'])} | {med(loss_us['torch_soft']) / med(loss_us['fused_soft']):.2f} |",
        "",
    ]
    del ds, kept
    torch.cuda.empty_cache()
    if a.skip_train:
        lines += ["## (c) `train.py`: not measured (`--skip-train`)", ""]
    else:
        variants = [("with the three flags", ROOT, MIX_FLAGS), ("without them", ROOT, [])]
        if a.parent:
            variants.append(("parent commit", os.path.abspath(a.parent), []))
        rows = {name: [] for name, _, _ in variants}
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "cifar_sized.npz")
            np.savez(path, x_train=images, y_train=labels, mean=np.array(MEAN, np.float32), std=np.array(STD, np.float32))
            for rep in range(2):                                    # alternated, the second round in the opposite order: other work
                for name, tree, flags in (variants if rep == 0 else variants[::-1]):         # shares the host, and a run's place in the order shows
                    rows[name].append(train_run(tree, ["--model-type", a.model_type, "--graph", "--no-step-metrics", "--data-npz", path, "--epochs", str(a.epochs),
                                                       "--log-dir", os.path.join(tmp, f"log{rep}{len(flags)}{tree == ROOT}"), *flags]))
        lines += [
            f"## (c) `train.py --model-type {a.model_type} --graph --no-step-metrics --data-npz`, default geometry, {-(-N // BATCH)} steps per epoch",
            "",
            f"`epoch_seconds` (host clock around work that ends in the epoch's one synchronise) of every epoch after the first; two runs per "
            f"variant, one process each, alternated: run 1 in the order of the table, run 2 in the opposite order. The flags are "
            f"`{' '.join(MIX_FLAGS)}`.",
            "",
            "| variant | median, ms | run 1, ms | run 2, ms |",
            "|---|---|---|---|",
        ]
        for name, _, _ in variants:
            both = rows[name][0] + rows[name][1]
            lines.append(f"| {name} | {med(both) * 1e3:.1f} | {fmt(rows[name][0], 1e3, 1)} | {fmt(rows[name][1], 1e3, 1)} |")
        lines.append("")
        if a.parent:
            lo, hi = min(rows["parent commit"][0] + rows["parent commit"][1]), max(rows["parent commit"][0] + rows["parent commit"][1])
            m = med(rows["without them"][0] + rows["without them"][1])
            lines += [f"The parent's epochs span {lo * 1e3:.1f} .. {hi * 1e3:.1f} ms; the no-flag median is {m * 1e3:.1f} ms: "
                      f"{'inside' if lo <= m <= hi else 'OUTSIDE'} that spread (it runs the same code).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
