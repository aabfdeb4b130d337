"""What the fused AdamW step (kanvit/optim.py: KanvitAdamW) costs, on the GPU:

  (1) the ViT-B/16 ChebyKAN parameter set, device time per optimizer step on fixed gradients -- the four variants captured in one graph
      each and replayed in turn, round after round, in one process:
        (a) stock Adam(fused=True), the default train step's optimizer;
        (b) the stock composition of the recipe: clip_grad_norm_(foreach), AdamW(fused=True) with a tensor lr, foreach lerp_ for the EMA;
        (c) KanvitAdamW with the same options (clipping, weight decay, EMA);
        (d) KanvitAdamW bare;
      and beside them the byte floor at 6.3 TB/s (28 B per parameter, 36 B with the EMA, 4 B more for the norm pass);
  (2) train.py --graph --data-npz at the default geometry, `epoch_seconds` of every epoch after the first: --optimizer kanvit-adamw
      bare, the default run, and (--parent DIR: a checkout of the parent commit, built) the parent's default run -- one process per
      run, the variants alternated, the second round in the opposite order.

    python tools/optim_step_rate.py [--out profiles/optim_step.md] [--reps 7] [--steps 10] [--epochs 3] [--parent DIR] [--skip-train]

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

VITB = dict(chw=(3, 224, 224), n_patches=14, n_blocks=12, d_hidden=768, n_heads=12, out_d=100, type="cheby")
LR, WD, CLIP, EMA = 1e-3, 0.05, 1.0, 0.9998
N, C, H, W, CH = 50000, 100, 32, 32, 3


def byte_floor_seconds(numel, ema, clip, bytes_per_second=6.3e12):
    """What the step's traffic costs at the achievable HBM rate: 28 B per parameter (p, g, m, v read; p, m, v written), 36 B with
    the EMA, plus 4 B for the norm pass."""
    return numel * ((36 if ema else 28) + (4 if clip else 0)) / bytes_per_second


def captured(step, steps):
    """A graph of `steps` calls of step() (after one throw-away call on a side stream, which creates lazy state)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(steps):
            step()
    return graph


def replay_ms(graph, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10, help="optimizer steps per replayed graph")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--model-type", default="cheby")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for part (2)")
    ap.add_argument("--skip-train", action="store_true", help="part (1) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_step_rate.py measures on the GPU; none is visible")
    from kanvit.optim import KanvitAdamW
    from model import VisionTransformer
    dev, med = torch.device("cuda:0"), statistics.median
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in VisionTransformer(VITB["chw"], n_patches=VITB["n_patches"], n_blocks=VITB["n_blocks"], d_hidden=VITB["d_hidden"],
                                                        n_heads=VITB["n_heads"], out_d=VITB["out_d"], type=VITB["type"]).parameters() if p.requires_grad]
    numel = sum(int(np.prod(s)) for s in shapes)
    g = torch.Generator(device=dev).manual_seed(0)

    def fresh():
        ps = [torch.nn.Parameter(0.02 * torch.randn(s, device=dev, generator=g)) for s in shapes]
        for p in ps:
            p.grad = 1e-3 * torch.randn(p.shape, device=dev, generator=g)
        return ps

    variants = {}
    pa = fresh()
    oa = torch.optim.Adam(pa, lr=LR, fused=True, capturable=True)
    variants["(a) stock `Adam(fused=True)`"] = (oa.step, False, False)
    pb = fresh()
    ob = torch.optim.AdamW(pb, lr=torch.tensor(LR, device=dev), weight_decay=WD, fused=True, capturable=True)
    eb = [p.detach().clone() for p in pb]

    def stock_recipe():
        torch.nn.utils.clip_grad_norm_(pb, CLIP, foreach=True)
        ob.step()
        torch._foreach_lerp_(eb, [p.detach() for p in pb], 1.0 - EMA)
    variants["(b) stock `clip_grad_norm_` + `AdamW(fused=True)` + foreach EMA"] = (stock_recipe, True, True)
    pc = fresh()
    oc = KanvitAdamW(pc, lr=LR, weight_decay=WD, max_grad_norm=CLIP, ema_decay=EMA, total_steps=1000, warmup_steps=10, schedule="cosine")
    variants["(c) `KanvitAdamW`, clipping + decay + schedule + EMA"] = (oc.step, True, True)
    pd = fresh()
    od = KanvitAdamW(pd, lr=LR, total_steps=1000)
    variants["(d) `KanvitAdamW` bare"] = (od.step, False, False)
    graphs = {name: captured(fn, a.steps) for name, (fn, _, _) in variants.items()}
    times = {name: [] for name in variants}
    order = list(variants)
    for rep in range(a.reps + 1):                                   # interleaved: every round replays all four; the first is the warm-up
        for name in (order if rep % 2 == 0 else order[::-1]):
            t = replay_ms(graphs[name], a.steps)
            if rep:
                times[name].append(t)
    from kanvit import ops
    per = -(-len(shapes) // ops.optim_max_tensors())
    lines = [
        "# The fused AdamW step (`tools/optim_step_rate.py`)",
        "",
        f"Device: {torch.cuda.get_device_name(0)}.",
        "",
        f"## (1) ViT-B/16 ChebyKAN parameter set: {len(shapes)} tensors, {numel / 1e6:.1f} M parameters, fixed gradients",
        "",
        f"Device time per optimizer step from a replayed graph of {a.steps} steps; the four graphs are replayed in turn, {a.reps} rounds after one "
        f"warm-up round, the order reversed every other round; every figure listed. `KanvitAdamW` issues {per} update launch(es) per step "
        f"({len(shapes)} tensors, {ops.optim_max_tensors()} per launch), one begin launch, and {per} more for the norm when clipping. The floor is "
        "the step's bytes at 6.3 TB/s.",
        "",
        "| variant | ms / step | every round | byte floor, ms | floor / measured |",
        "|---|---|---|---|---|",
    ]
    for name, (_, ema, clip) in variants.items():
        floor = 1e3 * byte_floor_seconds(numel, ema, clip)
        lines.append(f"| {name} | {med(times[name]):.3f} | {fmt(times[name], 1.0, 3)} | {floor:.3f} | {floor / med(times[name]):.2f} |")
    ta, tb, tc, td = (times[k] for k in order)
    lines += ["",
              f"(c) / (b) = {med(tc) / med(tb):.2f}: the fused recipe step is {'below' if med(tc) < med(tb) else 'NOT below'} the stock composition.",
              f"(d) = {med(td):.3f} ms against (a) spanning {min(ta):.3f} .. {max(ta):.3f} ms: "
              f"{'inside' if min(ta) <= med(td) <= max(ta) else ('below' if med(td) < min(ta) else 'ABOVE')} its run-to-run spread.", ""]
    del graphs, variants, pa, pb, pc, pd, oa, ob, oc, od, eb
    torch.cuda.empty_cache()
    if a.skip_train:
        lines += ["## (2) `train.py`: not measured (`--skip-train`)", ""]
    else:
        runs = [("`--optimizer kanvit-adamw`", ROOT, ["--optimizer", "kanvit-adamw"]), ("default (`adam`)", ROOT, [])]
        if a.parent:
            runs.append(("parent commit", os.path.abspath(a.parent), []))
        rows = {name: [] for name, _, _ in runs}
        rng = np.random.default_rng(0)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "cifar_sized.npz")
            np.savez(path, x_train=rng.integers(0, 256, (N, H, W, CH), dtype=np.uint8), y_train=rng.integers(0, C, N).astype(np.int64))
            for rep in range(2):
                for name, tree, flags in (runs if rep == 0 else runs[::-1]):
                    rows[name].append(train_run(tree, ["--model-type", a.model_type, "--graph", "--no-step-metrics", "--data-npz", path, "--epochs", str(a.epochs),
                                                       "--log-dir", os.path.join(tmp, f"log{rep}{len(flags)}{tree == ROOT}"), *flags]))
        lines += [
            f"## (2) `train.py --model-type {a.model_type} --graph --no-step-metrics --data-npz`, default geometry, {-(-N // 128)} steps per epoch",
            "",
            "`epoch_seconds` (host clock around work that ends in the epoch's one synchronise) of every epoch after the first; two runs per "
            "variant, one process each, alternated: run 1 in the order of the table, run 2 in the opposite order.",
            "",
            "| variant | median, ms | run 1, ms | run 2, ms |",
            "|---|---|---|---|",
        ]
        for name, _, _ in runs:
            both = rows[name][0] + rows[name][1]
            lines.append(f"| {name} | {med(both) * 1e3:.1f} | {fmt(rows[name][0], 1e3, 1)} | {fmt(rows[name][1], 1e3, 1)} |")
        base = rows["parent commit" if a.parent else "default (`adam`)"]
        lo, hi = min(base[0] + base[1]), max(base[0] + base[1])
        m = med(rows["`--optimizer kanvit-adamw`"][0] + rows["`--optimizer kanvit-adamw`"][1])
        lines += ["", f"The {'parent' if a.parent else 'default'} run's epochs span {lo * 1e3:.1f} .. {hi * 1e3:.1f} ms; the kanvit-adamw median is "
                      f"{m * 1e3:.1f} ms: {'inside' if lo <= m <= hi else ('below' if m < lo else 'ABOVE')} that spread.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
