"""What the epoch metrics cost, on the GPU, at CIFAR-100's size (N = 50 000 samples, C = 100 classes, batch 128), both ways:

  default           train.py's lists: per step argmax + softmax appended, at the end of the epoch three concatenations, the [N, C]
                    copy to the host and scikit-learn (utils.calculate_metrics);
  --device-metrics  kanvit/metrics.py: one kernel per step, at the end the pair-counting pass and one copy of C*C + 2*C integers.

  (a) on generated logits: the time from "last step issued" (host clock, nothing synchronised before it) to "four numbers on the
      host", median of --reps runs after a warm-up -- each path on its own, then the two alternated in either order; plus the device
      time of a whole epoch's per-step accumulation (device events) and the largest difference between the two paths' numbers;
  (b) train.py --graph --data-npz at the default geometry on a generated dataset of CIFAR's size, both ways, runs alternated:
      history["epoch_seconds"] (the epoch up to its one synchronise: the per-step accumulation is inside, the end-of-epoch metrics
      are not) and history["metrics_seconds"] (the end-of-epoch metrics), every epoch after the first.

    python tools/epoch_metrics_rate.py [--out profiles/epoch_metrics.md] [--reps 5] [--epochs 3] [--model-type cheby] [--skip-train]

Needs the GPU: there is no CPU fall-back and no figure without a run."""
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

N, C, BATCH = 50000, 100, 128
H, W, CH = 32, 32, 3
MEAN, STD = [0.5071, 0.4867, 0.4408], [0.2675, 0.2565, 0.2761]


def default_epoch(zs, ys):
    """train.py's default path on ready logits.  Returns (seconds from the last step issued to the numbers, device ms of the steps' part,
    the numbers)."""
    from utils import calculate_metrics
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    yl, preds, probs = [], [], []
    e0.record()
    for z, y in zip(zs, ys):
        yl.append(y)
        preds.append(z.argmax(dim=1))
        probs.append(torch.softmax(z.float(), dim=1))
    e1.record()
    t0 = time.perf_counter()
    out = calculate_metrics(torch.cat(yl).cpu().numpy(), torch.cat(preds).cpu().numpy(), torch.cat(probs).cpu().numpy(), num_classes=C)
    dt = time.perf_counter() - t0
    return dt, e0.elapsed_time(e1), out


def device_epoch(zs, ys, em):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    em.reset()
    e0.record()
    for z, y in zip(zs, ys):
        em.update(z, y)
    e1.record()
    t0 = time.perf_counter()
    out = em.compute()
    dt = time.perf_counter() - t0
    return dt, e0.elapsed_time(e1), out


def replayed_us(fn, launches=200, reps=5):
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


def train_epochs(argv, epochs):
    import train
    hist = train.main(train.parse(argv + ["--epochs", str(epochs)]))
    return hist["epoch_seconds"][1:], hist["metrics_seconds"][1:], hist["train_metrics"][-1]


def fmt(vs, scale=1.0, digits=2):
    return ", ".join(f"{v * scale:.{digits}f}" for v in vs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_metrics.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--model-type", default="cheby")
    ap.add_argument("--skip-train", action="store_true", help="part (a) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/epoch_metrics_rate.py measures on the GPU; none is visible")
    from kanvit import ops
    from kanvit.metrics import EpochMetrics
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    logits = 2.0 * torch.randn(N, C, device=dev, generator=g)
    labels = torch.randint(0, C, (N,), device=dev, generator=g)
    logits[torch.arange(N, device=dev), labels] += 1.5              # a classifier that has learnt something: AUC away from 0.5
    zs, ys = list(logits.split(BATCH)), list(labels.split(BATCH))
    em = EpochMetrics(C, N, dev)
    med = statistics.median
    paths = {"default": lambda: default_epoch(zs, ys), "device": lambda: device_epoch(zs, ys, em)}
    alone, step_ms, numbers = {}, {}, {}
    for name, run in paths.items():                                 # each path on its own: one warm-up, then the repetitions
        run()
        res = [run() for _ in range(a.reps)]
        alone[name], step_ms[name], numbers[name] = [r[0] for r in res], [r[1] for r in res], res[-1][2]
    mixed = {}
    for order in (("device", "default"), ("default", "device")):    # and alternated, in either order
        got = {n: [] for n in order}
        for _ in range(a.reps):
            for n in order:
                got[n].append(paths[n]()[0])
        mixed[order] = got
    diff = [abs(x - y) for x, y in zip(numbers["default"], numbers["device"])]
    em.reset()
    kept = []
    us_device = replayed_us(lambda i: ops.metrics_update(zs[0], ys[0], i * BATCH, em._probs_t, em._labels, em._preds, em.confusion), reps=a.reps)
    us_default = replayed_us(lambda i: kept.append((zs[0].argmax(dim=1), torch.softmax(zs[0].float(), dim=1))), reps=a.reps)
    em.reset()
    steps = len(zs)
    lines = [
        "# Epoch metrics: lists + scikit-learn against the device tables (`tools/epoch_metrics_rate.py`)",
        "",
        f"Device: {torch.cuda.get_device_name(0)}. N = {N} samples, C = {C} classes, {steps} steps of {BATCH} rows (the last one short), generated "
        f"fp32 logits. Medians of {a.reps} runs after one warm-up, every single figure listed.",
        "",
        "## (a) From \"last step issued\" to \"four numbers on the host\" (host clock)",
        "",
        "| arrangement | default: lists + `calculate_metrics` | `--device-metrics` |",
        "|---|---|---|",
        f"| each on its own | **{med(alone['default']) * 1e3:.1f} ms** ({fmt(alone['default'], 1e3, 1)}) | **{med(alone['device']) * 1e3:.2f} ms** ({fmt(alone['device'], 1e3)}) |",
    ]
    for order, got in mixed.items():
        lines.append(f"| alternated, {order[0]} first | {med(got['default']) * 1e3:.1f} ms ({fmt(got['default'], 1e3, 1)}) | "
                     f"{med(got['device']) * 1e3:.2f} ms ({fmt(got['device'], 1e3)}) |")
    lines += [
        "",
        f"Ratio of the medians, each on its own: {med(alone['default']) / med(alone['device']):.0f}x. The device figure holds the draining of "
        f"the queued update kernels, the counting pass, the pair kernel ({N}^2 = {N * N / 1e9:.1f}e9 compares) and one copy of "
        f"{C * C + 2 * C} integers; the default figure holds three concatenations, a {N * C * 4 / 1e6:.0f} MB copy and scikit-learn on one CPU thread.",
        "",
        "The per-step part. Issued back to back with nothing else queued (device events around the whole epoch's accumulation) it is bound by "
        "the host's issue rate, not by the kernels; captured 200 at a time in a graph and replayed it is device time:",
        "",
        "| path | issued from the host, ms / epoch | us / step | replayed graph, us / step |",
        "|---|---|---|---|",
        f"| default (argmax + softmax per step) | {med(step_ms['default']):.2f} ({fmt(step_ms['default'])}) | {med(step_ms['default']) / steps * 1e3:.1f} | "
        f"{med(us_default):.2f} ({fmt(us_default)}) |",
        f"| `--device-metrics` (one kernel per step) | {med(step_ms['device']):.2f} ({fmt(step_ms['device'])}) | {med(step_ms['device']) / steps * 1e3:.1f} | "
        f"{med(us_device):.2f} ({fmt(us_device)}) |",
        "",
        f"The four numbers, default: {', '.join(f'{v:.12f}' for v in numbers['default'])}; device: {', '.join(f'{v:.12f}' for v in numbers['device'])}; "
        f"largest difference {max(diff):.2e} (the two softmaxes differ in the last place; the three confusion-matrix numbers are exact).",
        "",
    ]
    if a.skip_train:
        lines += ["## (b) `train.py`: not measured (`--skip-train`)", ""]
    else:
        rng = np.random.default_rng(0)
        arrays = dict(x_train=rng.integers(0, 256, (N, H, W, CH), dtype=np.uint8), y_train=rng.integers(0, C, N).astype(np.int64),
                      mean=np.array(MEAN, np.float32), std=np.array(STD, np.float32))
        rows = {"default": ([], []), "device": ([], [])}
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "cifar_sized.npz")
            np.savez(path, **arrays)
            common = ["--model-type", a.model_type, "--graph", "--data-npz", path]
            for rep in range(2):                                    # alternated: other work shares the host
                for name, flag in (("default", []), ("device", ["--device-metrics"])):
                    es, ms, _ = train_epochs(common + flag + ["--log-dir", os.path.join(tmp, f"{name}{rep}")], a.epochs)
                    rows[name][0].extend(es)
                    rows[name][1].extend(ms)
        lines += [
            f"## (b) `train.py --model-type {a.model_type} --graph --data-npz`, default geometry, {steps} steps per epoch",
            "",
            "Every epoch after the first of two runs each way, alternated. `epoch_seconds` ends in the epoch's one synchronise: the per-step "
            "accumulation is inside it, the end-of-epoch metrics are not; `metrics_seconds` is the end-of-epoch part.",
            "",
            "| path | `epoch_seconds` median | every epoch | `metrics_seconds` median | every epoch |",
            "|---|---|---|---|---|",
        ]
        for name, label in (("default", "default"), ("device", "`--device-metrics`")):
            es, ms = rows[name]
            lines.append(f"| {label} | {med(es) * 1e3:.1f} ms | {fmt(es, 1e3, 1)} | {med(ms) * 1e3:.2f} ms | {fmt(ms, 1e3)} |")
        lines += [
            "",
            f"Epoch plus metrics, medians: default {(med(rows['default'][0]) + med(rows['default'][1])) * 1e3:.1f} ms, "
            f"`--device-metrics` {(med(rows['device'][0]) + med(rows['device'][1])) * 1e3:.1f} ms.",
            "",
        ]
    lines += ["The cost of the pair counts grows as N^2; a sort-based form for ImageNet-sized epochs is not built.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
