"""What PatchDropout's front costs and what it saves, on the GPU:

  (1) kanvit_patch_keep, kanvit_patch_gather, kanvit_tokens_assemble_fwd / _bwd at the ViT-B/16 launch shape (B = 128 images of 3 x 224
      x 224, P = 196 patches of I = 768, d = 768) for K = 98 and 147 kept patches, each against its stock composition (rand + argsort;
      patchify + gather; cat + indexed position add; slice copy + sum) -- device time per call of a replayed graph that holds --launches
      calls; all variants replayed in turn, round after round, in one process; the byte floor at 6.3 TB/s beside each;
  (2) one ViT-B/16 ChebyKAN train.py step at batch 128 on the synthetic stream with --patch-dropout 0 (the flag absent), 0.25 and 0.5,
      and (--parent DIR: a built checkout of the parent commit) the parent's train.py;
  (3) train.py --graph --data-npz at the default (small) geometry, `epoch_seconds` of every epoch after the first: with --patch-dropout
      0.5, without, and the parent;
      (2) and (3): one process per run, the variants alternated, the second round in the opposite order.

    python tools/patch_dropout_rate.py [--out profiles/patch_dropout.md] [--reps 7] [--launches 20] [--parent DIR] [--skip-train]

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
from drop_path_rate import VITB, captured, replay_us  # noqa: E402

B, CH, SIDE, NP, D = 128, 3, 224, 14, 768
P, I = NP * NP, CH * (SIDE // NP) ** 2
KS = (98, 147)                                        # --patch-dropout 0.5 and 0.25
N, CLASSES, H, W = 50000, 100, 32, 32
BW = 6.3e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_dropout.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8, help="ViT-B steps per epoch in part (2)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for parts (2) and (3)")
    ap.add_argument("--skip-train", action="store_true", help="part (1) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/patch_dropout_rate.py measures on the GPU; none is visible")
    from kanvit import _lib, ops
    from kanvit.ops import _launch, _ptr
    L, dev, med = _lib.lib(), torch.device("cuda:0"), statistics.median
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randn(B, CH, SIDE, SIDE, device=dev, generator=g)
    cls, pos = torch.randn(1, D, device=dev, generator=g), torch.randn(P + 1, D, device=dev, generator=g)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    pd = _lib.PatchDesc(CH, SIDE, SIDE, NP, 0, 0)
    import ctypes as C
    variants = {}                                     # name -> (call, bytes the algorithm has to move, or None)
    keep_alive = []
    for K in KS:
        idx = ops.patch_keep(B, P, K, 0, counter)
        idx64 = idx.long()
        rows = torch.empty(B * K, I, device=dev)
        tokens, dtokens = torch.randn(B * K, D, device=dev, generator=g), torch.empty(B * K, D, device=dev)
        out, dout, dcls = torch.empty(B, K + 1, D, device=dev), torch.randn(B, K + 1, D, device=dev, generator=g), torch.empty(D, device=dev)
        keep_alive += [idx, idx64, rows, tokens, dtokens, out, dout, dcls]

        def keep(K=K, idx=idx):
            _launch(L.kanvit_patch_keep, "keep", dev, B, P, K, C.c_uint64(0), _ptr(counter), _ptr(idx))

        def keep_stock(K=K):
            return torch.rand(B, P, device=dev).argsort(dim=1)[:, :K]

        def gather(K=K, idx=idx, rows=rows):
            _launch(L.kanvit_patch_gather, "gather", dev, C.byref(pd), B, K, _ptr(idx), _ptr(images), _ptr(rows), I)

        def gather_stock(K=K, idx64=idx64):
            return torch.gather(ops.patchify(images, NP), 1, idx64.unsqueeze(-1).expand(B, K, I))

        def assemble(K=K, idx=idx, tokens=tokens, out=out):
            _launch(L.kanvit_tokens_assemble_fwd, "assemble", dev, B, K, D, _ptr(tokens), D, _ptr(cls), _ptr(pos), _ptr(idx), _ptr(out))

        def assemble_stock(K=K, idx64=idx64, tokens=tokens):
            where = torch.cat((torch.zeros(B, 1, dtype=torch.int64, device=dev), 1 + idx64), dim=1)
            return torch.cat((cls.unsqueeze(0).expand(B, -1, -1), tokens.view(B, K, D)), dim=1) + pos[where]

        def assemble_bwd(K=K, dout=dout, dtokens=dtokens, dcls=dcls):
            _launch(L.kanvit_tokens_assemble_bwd, "assemble_bwd", dev, B, K, D, _ptr(dout), _ptr(dtokens), _ptr(dcls))

        def assemble_bwd_stock(K=K, dout=dout):
            return dout[:, 1:, :].reshape(B * K, D), dout[:, 0, :].sum(0)

        row = 4 * B * K                               # bytes of one fp32 column over the kept rows
        variants.update({
            f"K = {K}: `kanvit_patch_keep`": (keep, None),
            f"K = {K}: stock `rand`, `argsort`, slice": (keep_stock, None),
            f"K = {K}: `kanvit_patch_gather`": (gather, 2 * row * I + row),                         # kept patches in, rows out, idx
            f"K = {K}: stock `patchify`, `gather`": (gather_stock, 2 * row * I + row),
            f"K = {K}: `kanvit_tokens_assemble_fwd`": (assemble, row * D + 4 * B * (K + 1) * D + 4 * (P + 1) * D + row),
            f"K = {K}: stock `cat`, indexed `pos` add": (assemble_stock, row * D + 4 * B * (K + 1) * D + 4 * (P + 1) * D + row),
            f"K = {K}: `kanvit_tokens_assemble_bwd`": (assemble_bwd, 4 * B * (K + 1) * D + row * D),
            f"K = {K}: stock slice copy, `sum(0)`": (assemble_bwd_stock, 4 * B * (K + 1) * D + row * D),
        })
    graphs = {k: captured(fn, a.launches) for k, (fn, _) in variants.items()}
    times, order = {k: [] for k in variants}, list(variants)
    for rep in range(a.reps + 1):                                   # interleaved; the first round is the warm-up
        for k in (order if rep % 2 == 0 else order[::-1]):
            t = replay_us(graphs[k], a.launches)
            if rep:
                times[k].append(t)
    lines = [
        "# PatchDropout: the keep table, the gather and the sequence assembly (`tools/patch_dropout_rate.py`)",
        "",
        f"Device: {torch.cuda.get_device_name(0)}.",
        "",
        f"## (1) B = {B} images of {CH} x {SIDE} x {SIDE}, P = {P} patches of I = {I}, d = {D}, fp32",
        "",
        f"Device time per call from a replayed graph of {a.launches} calls; the graphs are replayed in turn, {a.reps} rounds after one warm-up round, "
        "the order reversed every other round; every figure listed. The floor is the bytes the algorithm has to move (the kept rows in and "
        "out, the index table, the position table once) at 6.3 TB/s; the stock compositions move more (the full patch matrix, the "
        "concatenated sequence twice), which the floor does not count. The keep table moves next to nothing: it has no byte floor.",
        "",
        "| variant | us / call | every round | byte floor, us | floor / measured |",
        "|---|---|---|---|---|",
    ]
    for k, (_, nbytes) in variants.items():
        floor = None if nbytes is None else 1e6 * nbytes / BW
        lines.append(f"| {k} | {med(times[k]):.1f} | {fmt(times[k], 1.0, 1)} | {'-' if floor is None else f'{floor:.1f}'} | "
                     f"{'-' if floor is None else f'{floor / med(times[k]):.2f}'} |")
    lines.append("")
    for K in KS:
        ks = [k for k in order if k.startswith(f"K = {K}:")]
        for ours, stock, what in ((ks[0], ks[1], "keep table"), (ks[2], ks[3], "gather"), (ks[4], ks[5], "assemble forward"), (ks[6], ks[7], "assemble backward")):
            r = med(times[ours]) / med(times[stock])
            lines.append(f"K = {K}, {what}: kernel / stock = {r:.2f} ({'no slower' if r <= 1.0 else 'SLOWER'} than the stock composition; "
                         f"stock rounds span {min(times[stock]):.1f} .. {max(times[stock]):.1f} us).")
    lines.append("")
    del graphs
    torch.cuda.empty_cache()
    print("\n".join(lines), flush=True)
    if a.skip_train:
        lines += ["## (2), (3) `train.py`: not measured (`--skip-train`)", ""]
    else:
        rng = np.random.default_rng(0)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "cifar_sized.npz")
            np.savez(path, x_train=rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8), y_train=rng.integers(0, CLASSES, N).astype(np.int64))
            vitb = [("`--patch-dropout 0.5` (N = 99)", ROOT, ["--patch-dropout", "0.5"]), ("`--patch-dropout 0.25` (N = 148)", ROOT, ["--patch-dropout", "0.25"]),
                    ("`--patch-dropout 0` (N = 197)", ROOT, [])]
            small = [("`--patch-dropout 0.5` (9 tokens)", ROOT, ["--patch-dropout", "0.5"]), ("without (17 tokens)", ROOT, [])]
            if a.parent:
                vitb.append(("parent commit", os.path.abspath(a.parent), []))
                small.append(("parent commit", os.path.abspath(a.parent), []))
            parts = [(f"## (2) ViT-B/16 ChebyKAN, batch 128, synthetic stream: ms per step ({a.steps} steps per epoch)", vitb,
                      [*VITB, "--steps-per-epoch", str(a.steps), "--epochs", str(a.epochs)], 1e3 / a.steps),
                     (f"## (3) `train.py --model-type cheby --graph --no-step-metrics --data-npz`, default geometry: ms per epoch of {-(-N // 128)} steps", small,
                      ["--model-type", "cheby", "--graph", "--no-step-metrics", "--data-npz", path, "--epochs", str(a.epochs)], 1e3)]
            for title, runs, argv, unit in parts:
                rows = {name: [] for name, _, _ in runs}
                for rep in range(2):
                    for name, tree, flags in (runs if rep == 0 else runs[::-1]):
                        rows[name].append(train_run(tree, [*argv, "--log-dir", os.path.join(tmp, f"log{len(title)}{rep}{len(name)}{tree == ROOT}"), *flags]))
                        print(f"{title[:6]} run {rep + 1} {name}: {fmt(rows[name][-1], unit, 2)}", flush=True)
                block = [title, "",
                         "`epoch_seconds` (host clock around work that ends in the epoch's one synchronise) of every epoch after the first; two runs per "
                         "variant, one process each, alternated: run 1 in the order of the table, run 2 in the opposite order.", "",
                         "| variant | median | run 1 | run 2 | median / rate 0 |", "|---|---|---|---|---|"]
                zero = med(rows[runs[len(runs) - (2 if a.parent else 1)][0]][0] + rows[runs[len(runs) - (2 if a.parent else 1)][0]][1])
                for name, _, _ in runs:
                    both = rows[name][0] + rows[name][1]
                    block.append(f"| {name} | {med(both) * unit:.2f} | {fmt(rows[name][0], unit, 2)} | {fmt(rows[name][1], unit, 2)} | {med(both) / zero:.3f} |")
                if a.parent:
                    base = rows["parent commit"]
                    lo, hi = min(base[0] + base[1]), max(base[0] + base[1])
                    name = runs[-2][0]
                    m = med(rows[name][0] + rows[name][1])
                    block += ["", f"{name}: median {m * unit:.2f} against the parent run's {lo * unit:.2f} .. {hi * unit:.2f}: "
                                  f"{'inside' if lo <= m <= hi else ('below' if m < lo else 'ABOVE')} that spread ({(m / med(base[0] + base[1]) - 1) * 100:+.2f} %)."]
                block.append("")
                lines += block
                print("\n".join(block), flush=True)
    lines += ["The effect of PatchDropout on the accuracy of a long run was not measured.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
