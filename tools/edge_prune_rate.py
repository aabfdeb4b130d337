"""What KAN edge pruning (csrc/edge_prune.hip, train.py --prune) costs, on the GPU:

  (1) kanvit_mask_rows on the masked gradient set of ViT-B/16 ChebyKAN and of ViT-B/16 efficient-KAN (the shapes, no model is built),
      half of the edges masked and none masked, against the stock composition of the same effect -- torch._foreach_mul_ with the
      masks expanded to the gradients' shapes, float32 -- each captured in a graph and replayed in turn; beside them the bytes the
      kernel moves (the mask bytes and the zeros it writes) and the bytes of a read-modify-write, at 6.3 TB/s;
  (2) kanvit_edge_select at groups = 36, E = 4096 and groups = 1, E = 589 824, COUNT (half pruned) and REL (0.5), against a
      torch.sort-based selection (stable sort + scatter; amax + compare for REL);
  (3) train.py: one ViT-B/16 ChebyKAN epoch at batch 128 with --resize 224 and one --graph --data-npz epoch at the default geometry,
      `epoch_seconds` after the first epoch, with --prune active, idle (a step never reached: masks all ones), without the flag, and
      (--parent DIR: a built checkout of the parent commit) on the parent -- one process per run, alternated, the second round reversed.

    python tools/edge_prune_rate.py [--out profiles/edge_prune.md] [--reps 7] [--launches 20] [--epochs 3] [--parent DIR] [--skip-train]

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

from batch_mix_rate import fmt, replayed_us, train_run  # noqa: E402

D, HEADS, BLOCKS, PATCH_IN = 768, 12, 12, 768            # ViT-B/16: 16 x 16 x 3 = 768 inputs per patch, 36 per-head layers per block
DH = D // HEADS
# (tensor shape, run, mask shape) of every masked tensor, per model type
SETS = {
    "ChebyKAN": [((PATCH_IN, D, 5), 5, (PATCH_IN, D))] + [((DH, DH, 5), 5, (DH, DH))] * (3 * HEADS * BLOCKS),
    "efficient-KAN": [((D, PATCH_IN, 8), 8, (D, PATCH_IN)), ((D, PATCH_IN), 1, (D, PATCH_IN))]
                     + [((DH, DH, 8), 8, (DH, DH)), ((DH, DH), 1, (DH, DH))] * (3 * HEADS * BLOCKS),
}
RATE = 6.3e12
N_SMALL, N_FULL, C = 2560, 50000, 100


def mask_rows_part(a, lines):
    from kanvit import ops
    dev, med = torch.device("cuda:0"), statistics.median
    g = torch.Generator(device=dev).manual_seed(0)
    for name, spec in SETS.items():
        numel = sum(int(np.prod(s)) for s, _, _ in spec)
        lines += [f"### {name}: {len(spec)} tensors, {numel / 1e6:.2f} M floats, {-(-len(spec) // ops.mask_max_tensors())} launch(es) per call", "",
                  "| masked share | variant | us / call | every round | bytes moved at 6.3 TB/s, us | read-modify-write at 6.3 TB/s, us |", "|---|---|---|---|---|---|"]
        for share in (0.5, 0.0):
            grads = [torch.randn(s, device=dev, generator=g) for s, _, _ in spec]
            runs = [r for _, r, _ in spec]
            masks = []
            for k, (s, r, ms) in enumerate(spec):               # efficient-KAN: spline_weight and base_weight of a layer share their mask
                if r == 1 and k and spec[k - 1][2] == ms:
                    masks.append(masks[-1])
                else:
                    masks.append((torch.rand(ms, device=dev, generator=g) >= share).to(torch.uint8))
            wide = [m.float().reshape(m.shape + (1,) * (len(s) - m.dim())).expand(s).contiguous() for m, (s, _, _) in zip(masks, spec)]
            own = sum({id(m): m.numel() for m in masks}.values()) + 4 * sum(int((m == 0).sum()) * r for m, r in zip(masks, runs))
            rmw = 8 * numel + sum(m.numel() for m in masks)
            fns = {"`ops.mask_rows`": lambda i: ops.mask_rows(grads, masks, runs), "`torch._foreach_mul_`, expanded float masks": lambda i: torch._foreach_mul_(grads, wide)}
            times = {k: replayed_us(fn, a.launches, a.reps) for k, fn in fns.items()}
            for k, t in times.items():
                lines.append(f"| {share:.0%} | {k} | {med(t):.1f} | {fmt(t, 1.0, 1)} | {1e6 * own / RATE:.1f} | {1e6 * rmw / RATE:.1f} |")
            del grads, masks, wide
        lines.append("")


def select_part(a, lines):
    from kanvit import ops
    dev, med = torch.device("cuda:0"), statistics.median
    g = torch.Generator(device=dev).manual_seed(1)
    lines += ["| groups x E | mode | variant | us / call | every round |", "|---|---|---|---|---|"]
    for groups, E in ((36, 4096), (1, 589824)):
        A = torch.rand(groups, E, device=dev, generator=g)
        n = E // 2

        def sort_count(i):
            order = torch.sort(A, dim=1, stable=True).indices
            mask = torch.ones(groups, E, dtype=torch.uint8, device=dev)
            mask.scatter_(1, order[:, :n], 0)
            return mask, mask.sum(dim=1)

        def torch_rel(i):
            mask = (A >= 0.5 * A.amax(dim=1, keepdim=True)).to(torch.uint8)
            return mask, mask.sum(dim=1)
        assert torch.equal(sort_count(0)[0], ops.edge_select(A, "count", n)[0]) and torch.equal(torch_rel(0)[0], ops.edge_select(A, "rel", 0.5)[0])
        for mode, value, stock, label in (("count", n, sort_count, "`torch.sort(stable)` + scatter"), ("rel", 0.5, torch_rel, "`amax` + compare")):
            for k, fn in (("`ops.edge_select`", lambda i: ops.edge_select(A, mode, value)), (label, stock)):
                t = replayed_us(fn, a.launches, a.reps)
                lines.append(f"| {groups} x {E} | {mode} | {k} | {med(t):.1f} | {fmt(t, 1.0, 1)} |")
    lines.append("")


def train_part(a, lines):
    med = statistics.median
    rng = np.random.default_rng(0)
    cases = [("ViT-B/16 ChebyKAN, batch 128, `--resize 224`", N_SMALL,
              ["--model-type", "cheby", "--n-blocks", "12", "--d-hidden", "768", "--n-heads", "12", "--n-patches", "14", "--resize", "224", "--no-step-metrics"]),
             ("default geometry, `--graph`", N_FULL, ["--model-type", "cheby", "--graph", "--no-step-metrics"])]
    with tempfile.TemporaryDirectory() as tmp:
        for title, n, flags in cases:
            path = os.path.join(tmp, f"images{n}.npz")
            np.savez(path, x_train=rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8), y_train=rng.integers(0, C, n).astype(np.int64))
            runs = [("`--prune 2:0.5` (active)", ROOT, ["--prune", "2:0.5"]), ("`--prune 1000000:0.5` (idle: masks all ones)", ROOT, ["--prune", "1000000:0.5"]),
                    ("without the flag", ROOT, [])]
            if a.parent:
                runs.append(("parent commit", os.path.abspath(a.parent), []))
            rows = {name: [] for name, _, _ in runs}
            for rep in range(2):
                for k, (name, tree, extra) in enumerate(runs if rep == 0 else runs[::-1]):
                    rows[name].append(train_run(tree, [*flags, "--data-npz", path, "--epochs", str(a.epochs), "--log-dir", os.path.join(tmp, f"log{n}{rep}{k}"), *extra]))
                    print(f"[{title}] run {rep + 1}, {name}: {fmt(rows[name][-1], 1e3, 1)} ms", flush=True)
            lines += [f"### `train.py --data-npz`, {title}: {-(-n // 128)} steps per epoch", "",
                      "| variant | median epoch, ms | ms / step | run 1, ms | run 2, ms |", "|---|---|---|---|---|"]
            for name, _, _ in runs:
                both = rows[name][0] + rows[name][1]
                lines.append(f"| {name} | {med(both) * 1e3:.1f} | {med(both) * 1e3 / -(-n // 128):.3f} | {fmt(rows[name][0], 1e3, 1)} | {fmt(rows[name][1], 1e3, 1)} |")
            base = rows["parent commit" if a.parent else "without the flag"]
            lo, hi = min(base[0] + base[1]), max(base[0] + base[1])
            m = med(rows["without the flag"][0] + rows["without the flag"][1])
            lines += ["", f"The {'parent' if a.parent else 'unflagged'} run's epochs span {lo * 1e3:.1f} .. {hi * 1e3:.1f} ms; the median without the flag is "
                          f"{m * 1e3:.1f} ms: {'inside' if lo <= m <= hi else ('below' if m < lo else 'ABOVE')} that spread.", ""]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_prune.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20, help="calls per replayed graph")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for part (3)")
    ap.add_argument("--skip-train", action="store_true", help="parts (1) and (2) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/edge_prune_rate.py measures on the GPU; none is visible")
    lines = ["# KAN edge pruning (`tools/edge_prune_rate.py`)", "", f"Device: {torch.cuda.get_device_name(0)}.", "",
             f"Parts (1) and (2): device time per call from a replayed graph of {a.launches} calls, {a.reps} replays after one warm-up replay, every figure "
             "listed. The effect of a long pruned run on accuracy was not measured.", "",
             "## (1) `kanvit_mask_rows` on the masked gradient sets of ViT-B/16", ""]
    mask_rows_part(a, lines)
    print("\n".join(lines), flush=True)
    lines += ["## (2) `kanvit_edge_select` (one work-group per group)", ""]
    select_part(a, lines)
    torch.cuda.empty_cache()
    if a.skip_train:
        lines += ["## (3) `train.py`: not measured (`--skip-train`)", ""]
    else:
        lines += ["## (3) `train.py` epochs", "",
                  "`epoch_seconds` (host clock around work that ends in the epoch's one synchronise) of every epoch after the first; two runs per variant, one "
                  "process each, alternated: run 1 in the order of the table, run 2 in the opposite order.", ""]
        train_part(a, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
