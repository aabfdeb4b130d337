"""What stochastic depth inside the fused residual add + LayerNorm costs, on the GPU:

  (1) kanvit_addln_sd_fwd / _bwd against kanvit_addln_fwd_ex / _bwd_ex at the ViT-B/16 launch shape (M = 128 x 197 rows, D = 768), and
      against the stock composition around the unscaled kernels (bernoulli_, divide, broadcast multiply forward; broadcast multiply
      backward) -- device time per call of a replayed graph that holds --launches calls; all variants replayed in turn, round after
      round, in one process; the byte floor at 6.3 TB/s beside each;
  (2) one ViT-B/16 ChebyKAN train.py step at batch 128 on the synthetic stream: with --drop-path 0.1, without, and (--parent DIR: a
      built checkout of the parent commit) the parent's train.py;
  (3) train.py --graph --data-npz at the default (small) geometry, `epoch_seconds` of every epoch after the first: with --drop-path 0.1
      (which leaves the one-launch LN2 + feed-forward), without, and the parent;
      (2) and (3): one process per run, the variants alternated, the second round in the opposite order.

    python tools/drop_path_rate.py [--out profiles/drop_path.md] [--reps 7] [--launches 20] [--parent DIR] [--skip-train]

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_mix_rate import fmt, train_run  # noqa: E402

B, NTOK, D = 128, 197, 768
KEEP = 0.9
VITB = ["--model-type", "cheby", "--synthetic", "--image-size", "224", "--n-patches", "14", "--n-blocks", "12", "--d-hidden", "768", "--n-heads", "12",
        "--batch-size", "128", "--no-step-metrics"]
N, C, H, W, CH = 50000, 100, 32, 32, 3


def captured(fn, launches):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(launches):
            fn()
    return graph


def replay_us(graph, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drop_path.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8, help="ViT-B steps per epoch in part (2)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for parts (2) and (3)")
    ap.add_argument("--skip-train", action="store_true", help="part (1) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/drop_path_rate.py measures on the GPU; none is visible")
    from kanvit import _lib, ops
    from kanvit.ops import _launch, _ptr
    L, dev, med = _lib.lib(), torch.device("cuda:0"), statistics.median
    M = B * NTOK
    g = torch.Generator(device=dev).manual_seed(0)
    x, delta, dy, dres = (torch.randn(M, D, device=dev, generator=g) for _ in range(4))
    gamma, beta = torch.rand(D, device=dev, generator=g) + 0.5, torch.randn(D, device=dev, generator=g)
    s, y, dx, dd, scaled = (torch.empty(M, D, device=dev) for _ in range(5))
    mean, rstd, dg, db = torch.empty(M, device=dev), torch.empty(M, device=dev), torch.empty(D, device=dev), torch.empty(D, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    scale = ops.depth_scales(B, [KEEP], 0, counter)[0].contiguous()
    mask = torch.empty(B, 1, 1, device=dev)
    ws = (L.kanvit_addln_bwd_workspace, M, D)

    def fwd():
        _launch(L.kanvit_addln_fwd_ex, "fwd", dev, M, D, 1e-5, _ptr(x), _ptr(delta), 0, _ptr(gamma), _ptr(beta), _ptr(s), _ptr(y), 0, _ptr(mean), _ptr(rstd))

    def fwd_sd():
        _launch(L.kanvit_addln_sd_fwd, "sd_fwd", dev, M, D, 1e-5, _ptr(x), _ptr(delta), 0, _ptr(gamma), _ptr(beta), _ptr(s), _ptr(y), 0, _ptr(mean),
                _ptr(rstd), _ptr(scale), NTOK)

    def fwd_stock():
        mask.bernoulli_(KEEP)
        mask.div_(KEEP)
        torch.mul(delta.view(B, NTOK, D), mask, out=scaled.view(B, NTOK, D))
        _launch(L.kanvit_addln_fwd_ex, "fwd", dev, M, D, 1e-5, _ptr(x), _ptr(scaled), 0, _ptr(gamma), _ptr(beta), _ptr(s), _ptr(y), 0, _ptr(mean), _ptr(rstd))

    def bwd():
        _launch(L.kanvit_addln_bwd_ex, "bwd", dev, M, D, _ptr(s), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dy), 0, _ptr(dres), _ptr(dx), None, _ptr(dg),
                _ptr(db), query=ws)

    def bwd_sd():
        _launch(L.kanvit_addln_sd_bwd, "sd_bwd", dev, M, D, _ptr(s), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dy), 0, _ptr(dres), _ptr(dx), _ptr(dd), 0,
                _ptr(dg), _ptr(db), _ptr(scale), NTOK, query=ws)

    def bwd_stock():
        bwd()
        torch.mul(dx.view(B, NTOK, D), mask, out=dd.view(B, NTOK, D))

    arr = 4 * M * D                                                 # bytes of one [M, D] fp32 tensor
    variants = {                                                    # name -> (call, [M, D] tensors the algorithm has to move)
        "forward, `kanvit_addln_fwd_ex`": (fwd, 4),                 # x, delta in; s, y out
        "forward, `kanvit_addln_sd_fwd`": (fwd_sd, 4),
        "forward, stock: `bernoulli_`, `div_`, `mul`, `kanvit_addln_fwd_ex`": (fwd_stock, 4),
        "backward, `kanvit_addln_bwd_ex` (+ reduce)": (bwd, 4),     # s, dy, dres in; dx out
        "backward, `kanvit_addln_sd_bwd` (+ reduce)": (bwd_sd, 5),  # ... and ddelta out
        "backward, stock: `kanvit_addln_bwd_ex` (+ reduce), `mul`": (bwd_stock, 5),
    }
    fwd()                                                           # mean / rstd / s exist before any backward runs
    graphs = {k: captured(fn, a.launches) for k, (fn, _) in variants.items()}
    times, order = {k: [] for k in variants}, list(variants)
    for rep in range(a.reps + 1):                                   # interleaved; the first round is the warm-up
        for k in (order if rep % 2 == 0 else order[::-1]):
            t = replay_us(graphs[k], a.launches)
            if rep:
                times[k].append(t)
    lines = [
        "# Stochastic depth in the fused residual add + LayerNorm (`tools/drop_path_rate.py`)",
        "",
        f"Device: {torch.cuda.get_device_name(0)}.",
        "",
        f"## (1) M = {B} x {NTOK} = {M} rows, D = {D}, fp32, keep = {KEEP}",
        "",
        f"Device time per call from a replayed graph of {a.launches} calls; the graphs are replayed in turn, {a.reps} rounds after one warm-up round, "
        "the order reversed every other round; every figure listed. The floor is the [M, D] tensors the algorithm moves at 6.3 TB/s (the "
        "stock compositions move two more through their multiply, which the floor does not count).",
        "",
        "| variant | us / call | every round | byte floor, us | floor / measured |",
        "|---|---|---|---|---|",
    ]
    for k, (_, n) in variants.items():
        floor = 1e6 * n * arr / 6.3e12
        lines.append(f"| {k} | {med(times[k]):.1f} | {fmt(times[k], 1.0, 1)} | {floor:.1f} | {floor / med(times[k]):.2f} |")
    f0, f1, f2, b0, b1, b2 = (times[k] for k in order)
    lines += ["",
              f"Forward: scaled / unscaled = {med(f1) / med(f0):.3f} (unscaled rounds span {min(f0):.1f} .. {max(f0):.1f} us); scaled / stock = {med(f1) / med(f2):.2f}.",
              f"Backward: scaled / unscaled = {med(b1) / med(b0):.3f} (one more [M, D] store: 5 / 4 = 1.25 by bytes); scaled / stock = {med(b1) / med(b2):.2f}.", ""]
    del graphs
    torch.cuda.empty_cache()
    if a.skip_train:
        lines += ["## (2), (3) `train.py`: not measured (`--skip-train`)", ""]
    else:
        flag = ["--drop-path", "0.1"]
        runs = [("`--drop-path 0.1`", ROOT, flag), ("without", ROOT, [])]
        if a.parent:
            runs.append(("parent commit", os.path.abspath(a.parent), []))
        rng = np.random.default_rng(0)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "cifar_sized.npz")
            np.savez(path, x_train=rng.integers(0, 256, (N, H, W, CH), dtype=np.uint8), y_train=rng.integers(0, C, N).astype(np.int64))
            parts = [(f"## (2) ViT-B/16 ChebyKAN, batch 128, synthetic stream: ms per step ({a.steps} steps per epoch)",
                      [*VITB, "--steps-per-epoch", str(a.steps), "--epochs", str(a.epochs)], 1e3 / a.steps),
                     (f"## (3) `train.py --model-type cheby --graph --no-step-metrics --data-npz`, default geometry: ms per epoch of {-(-N // 128)} steps",
                      ["--model-type", "cheby", "--graph", "--no-step-metrics", "--data-npz", path, "--epochs", str(a.epochs)], 1e3)]
            for title, argv, unit in parts:
                rows = {name: [] for name, _, _ in runs}
                for rep in range(2):
                    for name, tree, flags in (runs if rep == 0 else runs[::-1]):
                        rows[name].append(train_run(tree, [*argv, "--log-dir", os.path.join(tmp, f"log{len(title)}{rep}{len(flags)}{tree == ROOT}"), *flags]))
                lines += [title, "",
                          "`epoch_seconds` (host clock around work that ends in the epoch's one synchronise) of every epoch after the first; two runs per "
                          "variant, one process each, alternated: run 1 in the order of the table, run 2 in the opposite order.", "",
                          "| variant | median | run 1 | run 2 |", "|---|---|---|---|"]
                for name, _, _ in runs:
                    both = rows[name][0] + rows[name][1]
                    lines.append(f"| {name} | {med(both) * unit:.2f} | {fmt(rows[name][0], unit, 2)} | {fmt(rows[name][1], unit, 2)} |")
                base = rows["parent commit" if a.parent else "without"]
                lo, hi = min(base[0] + base[1]), max(base[0] + base[1])
                for name in ("`--drop-path 0.1`", "without") if a.parent else ("`--drop-path 0.1`",):
                    m = med(rows[name][0] + rows[name][1])
                    lines += ["", f"{name}: median {m * unit:.2f} against the {'parent' if a.parent else 'plain'} run's {lo * unit:.2f} .. {hi * unit:.2f}: "
                                  f"{'inside' if lo <= m <= hi else ('below' if m < lo else 'ABOVE')} that spread ({(m / med(base[0] + base[1]) - 1) * 100:+.2f} %)."]
                lines.append("")
    lines += ["The effect of stochastic depth on the accuracy of a long run was not measured.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
