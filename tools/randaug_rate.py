"""What the RandAugment epoch pass costs, on the GPU:

  (a) device time of one ops.randaugment_u8 launch over a generated dataset of CIFAR's size (N = 50 000, 32x32x3): the default policy
      (data.randaug_table's defaults), a table of IDENTITY rows alone -- the copy cost of the same kernel -- a plain device copy of the
      same bytes, and every op of the policy alone (one row per sample, applied to every sample), which names the op a slow pass is
      owed to.  Every case is captured once as a graph of --launches calls; the graphs are replayed in turn, round after round, so that
      all cases share whatever else the machine is doing.  Beside it the host time of drawing, checking and uploading the table.
  (c) one --graph --data-npz epoch at train.py's default geometry: with --randaug, without it, and without it from the parent
      commit's tree; `epoch_seconds` of every epoch after the first, one process per run, the variants alternated.

    python tools/randaug_rate.py [--out profiles/randaug_u8.md] [--parent DIR] [--reps 7] [--launches 10] [--epochs 3] [--skip-train]

--parent: a checkout of the parent commit with its kan-vit_amd/kanvit/libkanvit.so built; without it the parent's row says
"not measured".  Needs the GPU: there is no CPU fall-back and no figure without a run."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-vit_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from erase_rate import alternated_us, train_run                    # noqa: E402  (the same replay scheme and child process)
from resample_rate import BATCH, CH, CLASSES, MEAN, STD, H, N, W, fmt     # noqa: E402  (the same dataset and geometry)

HBM_TBS = 6.3                       # the byte floor's rate: a read and a write of every byte


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randaug_u8.md"))
    ap.add_argument("--parent", dest="parent_tree", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--skip-train", action="store_true", help="part (a) only")
    a = ap.parse_args()
    a.parent_tree = os.path.abspath(a.parent_tree) if a.parent_tree else None
    if not torch.cuda.is_available():
        raise SystemExit("tools/randaug_rate.py measures on the GPU; none is visible")
    from kanvit import data, ops
    dev, med = torch.device("cuda:0"), statistics.median
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (N, H, W, CH), dtype=np.uint8)
    labels = rng.integers(0, CLASSES, N).astype(np.int64)
    x = torch.from_numpy(images).to(dev)
    out = torch.empty_like(x)

    host = {"`randaug_table`": [], "`randaug_check_table`": [], "upload": []}
    for epoch in range(5):
        t0 = time.perf_counter()
        table = data.randaug_table(N, epoch, 0, (H, W))
        t1 = time.perf_counter()
        ops.randaug_check_table(table, N)
        t2 = time.perf_counter()
        table.contiguous().to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        for name, v in zip(host, (t1 - t0, t2 - t1, t3 - t2)):
            host[name].append(1e3 * v)

    def tab(**kw):
        return data.randaug_table(N, 0, 0, (H, W), **kw).to(dev)

    policy = tab()
    share = float((policy[:, :, 0] != 0).double().mean())
    tables = [("default policy (2 ops, prob 0.5, m 9, mstd 0.5)", policy), ("IDENTITY rows alone (the kernel's copy)", torch.zeros_like(policy)),
              ("default policy, 4 ops per sample", tab(n_ops=4))]
    tables += [(f"`{name}` alone, on every sample", tab(n_ops=1, prob=1.0, ops=[name])) for name in data.RANDAUG_OPS]
    cases = [(name, (lambda t: lambda i: ops.randaugment_u8(x, t, out=out))(t)) for name, t in tables]
    cases.insert(2, ("`out.copy_(images)` (a device copy of the same bytes)", lambda i: out.copy_(x)))
    us = alternated_us(cases, a.launches, a.reps)
    nbytes = 2 * x.numel()
    floor_us = nbytes / (HBM_TBS * 1e6)
    lines = [
        "# RandAugment as one uint8 -> uint8 pass per epoch (`tools/randaug_rate.py`)",
        "",
        f"Device: {torch.cuda.get_device_name(0)}. Device time per call from a replayed graph of {a.launches} calls. The cases are captured once and "
        f"replayed in turn, {a.reps} rounds after one warm-up round; the median, the range and every round are listed.",
        "",
        f"## (a) `ops.randaugment_u8` over N = {N} images of {H}x{W}x{CH}",
        "",
        f"Every case reads {x.numel() / 1e6:.1f} MB and writes as many: at {HBM_TBS} TB/s that is {floor_us:.1f} us, the byte floor. The default policy's "
        f"table holds an op in {100 * share:.1f} % of its slots; the rows \"alone\" apply one op of the policy to every sample (one row per sample, "
        "magnitude 9, mstd 0.5).",
        "",
        "| case | us / call | min .. max | every round | x byte floor |", "|---|---|---|---|---|",
    ]
    for name, _ in cases:
        v = us[name]
        lines.append(f"| {name} | {med(v):.1f} | {min(v):.1f} .. {max(v):.1f} | {fmt(v, digits=1)} | {med(v) / floor_us:.2f} |")
    lines += ["", f"Host time per epoch at N = {N}, five epochs, ms: " + "; ".join(f"{name} {med(v):.1f} ({min(v):.1f} .. {max(v):.1f})" for name, v in host.items())
              + ".  It is spent before the epoch's first batch, outside the captured step.", ""]
    del x, out
    torch.cuda.empty_cache()
    if a.skip_train:
        lines += ["## (c) `train.py`: not measured (`--skip-train`)", ""]
    else:
        with tempfile.TemporaryDirectory() as tmp:
            full = os.path.join(tmp, "full.npz")
            np.savez(full, x_train=images, y_train=labels, mean=np.array(MEAN, np.float32), std=np.array(STD, np.float32))
            graph = ["--model-type", "cheby", "--batch-size", str(BATCH), "--no-step-metrics", "--graph", "--epochs", str(a.epochs), "--data-npz", full]
            runs = [("`--graph --randaug`", ROOT, [*graph, "--randaug"]), ("`--graph`", ROOT, graph)]
            if a.parent_tree:
                runs.append(("`--graph`, the parent commit", a.parent_tree, graph))
            rows = {name: [] for name, _, _ in runs}
            for rep in range(2):                                    # alternated, the second round in the opposite order
                for k, (name, cwd, argv) in enumerate(runs if rep == 0 else runs[::-1]):
                    rows[name].append(train_run([*argv, "--log-dir", os.path.join(tmp, f"c{rep}{k}")], cwd))
        n_steps = -(-N // BATCH)
        lines += [
            f"## (c) One `--graph --data-npz` epoch at `train.py`'s default geometry ({N} stored {H}x{W} images, batch {BATCH}, {n_steps} steps)",
            "",
            "`epoch_seconds` (host clock around work that ends in the epoch's one synchronise) of every epoch after the first; two runs per "
            "variant, one process each, alternated: run 1 in the order of the table, run 2 in the opposite order.  With the flag an epoch "
            "draws, checks and uploads its table and launches the pass once, then reads the second buffer; without it nothing is launched "
            "or allocated and the batch kernels read the stored images.",
            "",
            "| variant | median, s / epoch | min .. max | run 1, s / epoch | run 2, s / epoch |",
            "|---|---|---|---|---|",
        ]
        for name in rows:
            every = rows[name][0] + rows[name][1]
            lines.append(f"| {name} | {med(every):.3f} | {min(every):.3f} .. {max(every):.3f} | {fmt(rows[name][0], digits=3)} | {fmt(rows[name][1], digits=3)} |")
        if not a.parent_tree:
            lines.append("| `--graph`, the parent commit | not measured | | | |")
        lines.append("")
    lines += ["The effect of RandAugment on the accuracy of a long run was not measured.  Counters were not collected.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
