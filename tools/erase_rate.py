"""What Random Erasing in the batch kernel costs, on the GPU:

  (a) device time per call of ops.erase_u8 at B = 128, 32x32x3 -> 224x224 and at the stored size 32x32, on a generated dataset of
      CIFAR's size under the pad-4 crop table: both fills at prob 0.25 (the recipe's default) and 1.0 -- against ops.resample_u8 from
      the same build, ops.resample_u8 from a build of the parent commit (--parent), the stock composition (ops.resample_u8, then
      torch.where over a box mask with a torch.randn of the batch) and, at the stored size, ops.augment_u8 / ops.mix_u8.  Every case
      is captured once as a graph of --launches calls; the graphs are replayed in turn, round after round, so that all cases share
      whatever else the machine is doing.
  (b) one train.py step at the ViT-B/16 geometry (batch 128, ChebyKAN), --data-npz FILE --resize 224: with --random-erasing 0.25,
      without it, and without it from the parent commit's tree; `epoch_seconds` / steps of every epoch after the first, one process
      per run, the variants alternated.
  (c) one --graph --data-npz epoch at train.py's default geometry (stored size, pad-4 crop), with and without the flag.

    python tools/erase_rate.py [--out profiles/erase_u8.md] [--parent DIR] [--reps 7] [--launches 50] [--epochs 3] [--steps 20] [--skip-train]

--parent: a checkout of the parent commit with its kan-vit_amd/kanvit/libkanvit.so built; without it the parent's rows say
"not measured".  Needs the GPU: there is no CPU fall-back and no figure without a run."""
import argparse
import ctypes
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from resample_rate import BATCH, CH, CHILD, CLASSES, MEAN, STD, VITB, H, N, PAD, S, W, fmt     # noqa: E402  (the same dataset and geometry)

GRAPH_STEP_MS = 1.16                # the --graph step at train.py's default geometry (profiles/batch_mix.md)


def alternated_us(cases, launches, reps):
    """{name: [device microseconds per call, one per round]}: every fn(i) of `cases` is captured as a graph of `launches` calls, then
    the graphs are replayed one after the other, `reps` rounds after one warm-up round."""
    graphs = {}
    for name, fn in cases:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn(0)
        torch.cuda.current_stream().wait_stream(side)
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for i in range(launches):
                fn(i)
    out = {name: [] for name, _ in cases}
    for rep in range(reps + 1):                                     # the first round is the warm-up
        for name, _ in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[name].replay()
            e1.record()
            e1.synchronize()
            if rep:
                out[name].append(1e3 * e0.elapsed_time(e1) / launches)
    return out


def train_run(argv, cwd, timeout=900):
    """One train.py process in the tree `cwd`; returns its epoch_seconds after the first epoch."""
    print(f"train.py in {cwd}: {' '.join(argv[-6:])}", file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, "-c", CHILD, *argv], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"train.py ended with {r.returncode}; no further run is started:\n{r.stdout[-2000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("EPOCH_SECONDS ")][-1]
    return json.loads(line.split(" ", 1)[1])[1:]


def parent_resample(tree):
    """ops.resample_u8's launch through the parent commit's library: fn(images, labels, idx, lut, crop, out, y) on the current stream."""
    from kanvit import _lib
    handle = ctypes.CDLL(os.path.join(tree, "kan-vit_amd", "kanvit", "libkanvit.so"))
    fn = handle.kanvit_resample_u8
    fn.restype, fn.argtypes = _lib.SYMBOLS["kanvit_resample_u8"]

    def call(images, labels, idx, lut, crop, out, y):
        n, h, w, c = images.shape
        rc = fn(images.data_ptr(), labels.data_ptr(), idx.data_ptr(), lut.data_ptr(), crop.data_ptr(), None, None, None, out.data_ptr(), y.data_ptr(),
                None, None, n, idx.shape[0], h, w, c, out.shape[2], out.shape[3], torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise SystemExit(f"the parent's kanvit_resample_u8 returned {rc}")
    return call


def code_objects(lines, parent_tree):
    """The resample_u8_kernel instantiations' metadata from the built libraries (tools/kernel_meta.py): this build's, and beside the
    non-erasing ones the parent's."""
    from kernel_meta import demangled_short, kernels

    def rows(lib):
        return {demangled_short(n): (k[".vgpr_count"], k[".sgpr_count"], k[".vgpr_spill_count"], k[".sgpr_spill_count"], k[".private_segment_fixed_size"],
                                     k[".group_segment_fixed_size"]) for n, k in kernels(lib).items() if "resample_u8_kernel" in n or "erase_u8_kernel" in n}
    mine = rows(os.path.join(ROOT, "kan-vit_amd", "kanvit", "libkanvit.so"))
    old = rows(os.path.join(parent_tree, "kan-vit_amd", "kanvit", "libkanvit.so")) if parent_tree else {}
    lines += ["## Code objects (`tools/kernel_meta.py`): VGPRs, SGPRs, VGPR spills, SGPR spills, scratch bytes, LDS bytes", "",
              "`resample_u8_kernel<VEC, MIX>` and `erase_u8_kernel<VEC, MIX>` are the non-erasing and the erasing form of one body.", "",
              "| kernel | this build | the parent's build |", "|---|---|---|"]
    for name in sorted(mine):
        twin = old.get(name, "not measured") if name.startswith("resample") else "--"
        lines.append(f"| `{name}` | {', '.join(map(str, mine[name]))} | {twin if isinstance(twin, str) else ', '.join(map(str, twin))} |")
    lines.append("")
    return all(mine[n] == old.get(n) for n in mine if n.startswith("resample")) if old else None


def table(lines, us, names, floor_us=None):
    med = statistics.median
    lines += ["| call | us / call | min .. max | every round |" + (" x store floor |" if floor_us else ""), "|---|---|---|---|" + ("---|" if floor_us else "")]
    for name in names:
        v = us[name]
        lines.append(f"| {name} | {med(v):.2f} | {min(v):.2f} .. {max(v):.2f} | {fmt(v)} |" + (f" {med(v) / floor_us:.2f} |" if floor_us else ""))
    lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "erase_u8.md"))
    ap.add_argument("--parent", dest="parent_tree", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="steps per epoch of part (b)")
    ap.add_argument("--skip-train", action="store_true", help="part (a) only")
    a = ap.parse_args()
    a.parent_tree = os.path.abspath(a.parent_tree) if a.parent_tree else None
    if not torch.cuda.is_available():
        raise SystemExit("tools/erase_rate.py measures on the GPU; none is visible")
    from kanvit import data, ops
    dev, med = torch.device("cuda:0"), statistics.median
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (N, H, W, CH), dtype=np.uint8)
    labels = rng.integers(0, CLASSES, N).astype(np.int64)
    ds = data.GpuDataset(torch.from_numpy(images), torch.from_numpy(labels), MEAN, STD, dev, pad=PAD, flip=True)
    idx = data.epoch_indices(N, 0, 0).to(dev)
    pad_t = data.crop_table(N, 0, 0, (H, W), "pad", pad=PAD).to(dev)
    noise, key = data.normal_table().to(dev), data.erase_noise_key(0, 0)
    steps = N // BATCH
    parent = parent_resample(a.parent_tree) if a.parent_tree else None
    lines = [
        "# Random Erasing in the batch kernel (`tools/erase_rate.py`)",
        "",
        f"Device: {torch.cuda.get_device_name(0)}. Device time per call from a replayed graph of {a.launches} calls. The cases of a table are "
        f"captured once and replayed in turn, {a.reps} rounds after one warm-up round; the median, the range and every round are listed. The "
        "`resample_u8` of this build is replayed from two graphs, before and after the parent's build: what separates those two is not the kernel.",
        "",
    ]

    def batch(i):
        return idx[(i % steps) * BATCH:(i % steps + 1) * BATCH]

    def section(size, title):
        out = torch.empty((BATCH, CH, *size), device=dev)
        y = torch.empty((BATCH,), device=dev, dtype=torch.int64)
        erase = {p: data.erase_table(N, 0, 0, size, prob=p) for p in (0.25, 1.0)}
        share = {p: float(((t[:, 1] - t[:, 0]) * (t[:, 3] - t[:, 2])).double().mean()) / (size[0] * size[1]) for p, t in erase.items()}
        erase = {p: t.to(dev) for p, t in erase.items()}
        ys, xs = torch.arange(size[0], device=dev), torch.arange(size[1], device=dev)
        mix = [t.to(dev) for t in data.mix_table(N, 0, 0, size, mixup_alpha=0.8, cutmix_alpha=1.0)]

        def stock(i):
            b = batch(i)
            x, _ = ops.resample_u8(ds.images, ds.labels, b, ds.lut, size, pad_t, out=out)
            e = erase[0.25][b]
            rows = (ys[None, :] >= e[:, 0:1]) & (ys[None, :] < e[:, 1:2])
            cols = (xs[None, :] >= e[:, 2:3]) & (xs[None, :] < e[:, 3:4])
            return torch.where((rows[:, :, None] & cols[:, None, :])[:, None], torch.randn_like(x), x)

        def erased(p, pixel, tables=()):
            return lambda i: ops.erase_u8(ds.images, ds.labels, batch(i), ds.lut, size, pad_t, *tables, erase=erase[p], noise=noise if pixel else None,
                                          noise_key=key, out=out)

        cases = [("`resample_u8` (this build)", lambda i: ops.resample_u8(ds.images, ds.labels, batch(i), ds.lut, size, pad_t, out=out))]
        if parent:
            cases.append(("`resample_u8` (parent's build)", lambda i: parent(ds.images, ds.labels, batch(i), ds.lut, pad_t, out, y)))
            cases.append(("`resample_u8` (this build, again)", cases[0][1]))       # the same kernel at another place in the round
        cases += [("`erase_u8`, const, prob 0.25", erased(0.25, False)), ("`erase_u8`, pixel, prob 0.25", erased(0.25, True)),
                  ("`erase_u8`, const, prob 1.0", erased(1.0, False)), ("`erase_u8`, pixel, prob 1.0", erased(1.0, True)),
                  ("`erase_u8`, no erase table", lambda i: ops.erase_u8(ds.images, ds.labels, batch(i), ds.lut, size, pad_t, out=out)),
                  ("`resample_u8` + `torch.where(mask, torch.randn_like(x), x)` (stock, prob 0.25)", stock),
                  ("`resample_u8`, Mixup / CutMix tables", lambda i: ops.resample_u8(ds.images, ds.labels, batch(i), ds.lut, size, pad_t, *mix, out=out)),
                  ("`erase_u8`, pixel, prob 0.25, Mixup / CutMix tables", erased(0.25, True, mix))]
        if size == (H, W):
            cases += [("`augment_u8`", lambda i: ops.augment_u8(ds.images, ds.labels, batch(i), ds.lut, PAD, True, 0, 0, out=out)),
                      ("`mix_u8`", lambda i: ops.mix_u8(ds.images, ds.labels, batch(i), ds.lut, *mix, PAD, True, 0, 0, out=out))]
        if parent:                                                  # the two builds compute the same batch
            ops.resample_u8(ds.images, ds.labels, batch(0), ds.lut, size, pad_t, out=out)
            mine = out.clone()
            parent(ds.images, ds.labels, batch(0), ds.lut, pad_t, out, y)
            if not torch.equal(mine, out):
                raise SystemExit("resample_u8 of this build and of the parent's differ")
        us = alternated_us(cases, a.launches, a.reps)
        px = BATCH * CH * size[0] * size[1]
        floor_us = 4 * px / 6.1e6
        lines.extend([
            f"## {title}: B = {BATCH}, {H}x{W}x{CH} -> {size[0]}x{size[1]}, N = {N}, pad-{PAD} crop table",
            "",
            f"Every form stores {4 * px / 1e6:.2f} MB; at the 6.1 TB/s of plain stores that is {floor_us:.2f} us, the store floor. `erase_table` at prob 0.25 "
            f"erases {100 * share[0.25]:.2f} % of all pixels, at prob 1.0 {100 * share[1.0]:.2f} %.",
            "",
        ])
        table(lines, us, [n for n, _ in cases], floor_us)
        return us

    us_big = section((S, S), "(a1) the model's size")
    us_small = section((H, W), "(a2) the stored size")
    own, aug = med(us_small["`erase_u8`, pixel, prob 0.25"]), med(us_small["`augment_u8`"])
    lines += [
        f"At the stored size Random Erasing leaves `augment_u8` ({aug:.2f} us) for `erase_u8` ({own:.2f} us): {own - aug:+.2f} us per step, "
        f"{100 * (own - aug) / (1e3 * GRAPH_STEP_MS):.2f} % of the {GRAPH_STEP_MS} ms `--graph` step of `profiles/batch_mix.md`; with Mixup / CutMix, `mix_u8` "
        f"({med(us_small['`mix_u8`']):.2f} us) for `erase_u8` with the mix tables ({med(us_small['`erase_u8`, pixel, prob 0.25, Mixup / CutMix tables']):.2f} us).",
        "",
    ]
    if parent:
        new, old = us_big["`resample_u8` (this build)"], us_big["`resample_u8` (parent's build)"]
        lines += [f"The untouched path at 224x224: this build {med(new):.2f} us ({min(new):.2f} .. {max(new):.2f}), the parent's {med(old):.2f} us "
                  f"({min(old):.2f} .. {max(old):.2f}).", ""]
    same = code_objects(lines, a.parent_tree)
    if same is not None:
        lines += [f"The non-erasing instantiations' metadata {'equals' if same else 'DIFFERS FROM'} the parent's.", ""]
    del ds
    torch.cuda.empty_cache()
    if a.skip_train:
        lines += ["## (b), (c) `train.py`: not measured (`--skip-train`)", ""]
    else:
        n_img = BATCH * a.steps
        with tempfile.TemporaryDirectory() as tmp:
            small, full = os.path.join(tmp, "small.npz"), os.path.join(tmp, "full.npz")
            stats = dict(mean=np.array(MEAN, np.float32), std=np.array(STD, np.float32))
            np.savez(small, x_train=images[:n_img], y_train=labels[:n_img], **stats)
            np.savez(full, x_train=images, y_train=labels, **stats)
            vitb = [*VITB, "--epochs", str(a.epochs), "--data-npz", small, "--resize", str(S)]
            runs = [("`--resize 224 --random-erasing 0.25`", ROOT, [*vitb, "--random-erasing", "0.25"]), ("`--resize 224`", ROOT, vitb)]
            if a.parent_tree:
                runs.append(("`--resize 224`, the parent commit", a.parent_tree, vitb))
            rows = {name: [] for name, _, _ in runs}
            for rep in range(2):                                    # alternated, the second round in the opposite order
                for k, (name, cwd, argv) in enumerate(runs if rep == 0 else runs[::-1]):
                    rows[name].append(train_run([*argv, "--log-dir", os.path.join(tmp, f"b{rep}{k}")], cwd))
            lines += [
                f"## (b) One `train.py` step, ViT-B/16 ChebyKAN (`{' '.join(VITB)}`), `--data-npz FILE`, {a.steps} steps per epoch",
                "",
                "`epoch_seconds` (host clock around work that ends in the epoch's one synchronise) over the steps, for every epoch after the "
                f"first; two runs per variant, one process each, alternated: run 1 in the order of the table, run 2 in the opposite order. The "
                f"file holds {n_img} stored {H}x{W} images.",
                "",
                "| variant | median, ms / step | run 1, ms / step | run 2, ms / step |",
                "|---|---|---|---|",
            ]
            for name in rows:
                lines.append(f"| {name} | {med(rows[name][0] + rows[name][1]) * 1e3 / a.steps:.2f} | {fmt(rows[name][0], 1e3 / a.steps)} | {fmt(rows[name][1], 1e3 / a.steps)} |")
            graph = ["--model-type", "cheby", "--batch-size", str(BATCH), "--no-step-metrics", "--graph", "--epochs", str(a.epochs), "--data-npz", full]
            runs = [("`--graph --random-erasing 0.25`", [*graph, "--random-erasing", "0.25"]), ("`--graph`", graph)]
            rows = {name: [] for name, _ in runs}
            for rep in range(2):
                for k, (name, argv) in enumerate(runs if rep == 0 else runs[::-1]):
                    rows[name].append(train_run([*argv, "--log-dir", os.path.join(tmp, f"c{rep}{k}")], ROOT))
            n_steps = -(-N // BATCH)
            lines += [
                "",
                f"## (c) One `--graph --data-npz` epoch at `train.py`'s default geometry ({N} stored {H}x{W} images, batch {BATCH}, {n_steps} steps)",
                "",
                "As (b): `epoch_seconds` of every epoch after the first, two alternated runs per variant. Without the flag a batch is one "
                "`augment_u8` launch, with it one `erase_u8` launch under the pad-4 crop table.",
                "",
                "| variant | median, s / epoch | median, ms / step | run 1, s / epoch | run 2, s / epoch |",
                "|---|---|---|---|---|",
            ]
            for name in rows:
                m = med(rows[name][0] + rows[name][1])
                lines.append(f"| {name} | {m:.3f} | {m * 1e3 / n_steps:.3f} | {fmt(rows[name][0], digits=3)} | {fmt(rows[name][1], digits=3)} |")
            lines.append("")
    lines += ["The effect of Random Erasing on the accuracy of a long run was not measured.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
