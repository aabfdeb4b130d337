"""What the masked-autoencoder kernels cost, on the GPU:

  (1) kanvit_tokens_restore_fwd / _bwd and kanvit_mae_loss at the ViT-B/16 pretraining shape (B = 128 images of 3 x 224 x 224, P = 196
      patches of I = 768, K = 49 kept, decoder width O = 384), each against the stock torch composition it replaces -- the ones of
      tests/_mae_ref.py: repeat + cat + argsort + gather + add and the ops of its backward; patchify + mean + var + normalise + squared
      error + masked mean, forward and backward -- device time per call of a replayed graph that holds --launches calls; all variants
      replayed in turn, round after round, in one process; the byte floor at 6.3 TB/s beside each;
  (2) one ViT-B/16 ChebyKAN train.py step at batch 128 on the synthetic stream: --pretrain mae (mask ratio 0.75, decoder 2 x 384), the
      supervised step, --patch-dropout 0.75, and (--parent DIR: a built checkout of the parent commit) the parent's supervised step;
      one process per run, the variants alternated, the second round in the opposite order.

    python tools/mae_rate.py [--out profiles/mae.md] [--reps 7] [--launches 20] [--parent DIR] [--skip-train]

Needs the GPU: there is no CPU fall-back and no figure without a run."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "kan-vit_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_mix_rate import fmt, train_run  # noqa: E402
from drop_path_rate import VITB, captured, replay_us  # noqa: E402

B, CH, SIDE, NP, K, O = 128, 3, 224, 14, 49, 384
P, I = NP * NP, CH * (SIDE // NP) ** 2
BW = 6.3e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mae.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8, help="ViT-B steps per epoch in part (2)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for part (2)")
    ap.add_argument("--skip-train", action="store_true", help="part (1) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mae_rate.py measures on the GPU; none is visible")
    from kanvit import _lib, ops
    from kanvit.ops import _launch, _ptr
    from tests import _mae_ref as ref
    L, dev, med = _lib.lib(), torch.device("cuda:0"), statistics.median
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randn(B, CH, SIDE, SIDE, device=dev, generator=g)
    idx = ops.patch_keep(B, P, K, 0, torch.zeros(1, dtype=torch.int64, device=dev))
    y, mask, pos = (torch.randn(*s, device=dev, generator=g) for s in ((B, K + 1, O), (1, O), (P + 1, O)))
    out, dout = torch.empty(B, P + 1, O, device=dev), torch.randn(B, P + 1, O, device=dev, generator=g)
    dy, dmask = torch.empty(B, K + 1, O, device=dev), torch.empty(O, device=dev)
    pred = torch.randn(B, P + 1, I, device=dev, generator=g)
    rows, loss, dpred = torch.empty(B, P, device=dev), torch.empty((), device=dev), torch.empty(B, P + 1, I, device=dev)
    pd = _lib.PatchDesc(CH, SIDE, SIDE, NP, 0, 0)
    pred_leaf = pred.clone().requires_grad_(True)

    def restore():
        _launch(L.kanvit_tokens_restore_fwd, "restore", dev, B, P, K, O, _ptr(y), _ptr(mask), _ptr(pos), _ptr(idx), _ptr(out))

    def restore_stock():
        return ref.restore_torch(y, mask, pos, idx)

    def restore_bwd():
        _launch(L.kanvit_tokens_restore_bwd, "restore_bwd", dev, B, P, K, O, _ptr(dout), _ptr(idx), _ptr(dy), _ptr(dmask))

    def restore_bwd_stock():
        return ref.restore_bwd_torch(dout, idx)

    def mae_loss():
        _launch(L.kanvit_mae_loss, "mae_loss", dev, C.byref(pd), B, K, _ptr(idx), _ptr(images), _ptr(pred), 1, _ptr(rows), _ptr(loss), _ptr(dpred))

    def mae_loss_stock():
        value, _ = ref.mae_loss_composition(pred_leaf, images, idx, NP, True)
        return value, torch.autograd.grad(value, pred_leaf)

    seq, kept, dropped = 4 * B * (P + 1) * O, 4 * B * (K + 1) * O, 4 * B * (P - K)
    variants = {                                          # name -> (call, bytes the algorithm has to move)
        "`kanvit_tokens_restore_fwd`": (restore, kept + seq + 4 * (P + 2) * O + 4 * B * K),              # y in, out, pos and mask once, idx
        "stock `repeat`, `cat`, `argsort`, `gather`, add": (restore_stock, kept + seq + 4 * (P + 2) * O + 4 * B * K),
        "`kanvit_tokens_restore_bwd`": (restore_bwd, seq + kept + 4 * B * K),                            # dout in, dy out, idx
        "stock `scatter_add`, slices, `cat`, `sum` (that composition's backward)": (restore_bwd_stock, seq + kept + 4 * B * K),
        "`kanvit_mae_loss` (loss and `dpred`)": (mae_loss, dropped * I * 2 + seq // O * I + 4 * B * K),  # dropped patches and rows in, all of dpred out
        "stock `patchify`, `mean`, `var`, ..., forward and backward": (mae_loss_stock, dropped * I * 2 + seq // O * I + 4 * B * K),
    }
    graphs = {k: captured(fn, a.launches) for k, (fn, _) in variants.items()}
    times, order = {k: [] for k in variants}, list(variants)
    for rep in range(a.reps + 1):                                   # interleaved; the first round is the warm-up
        for k in (order if rep % 2 == 0 else order[::-1]):
            t = replay_us(graphs[k], a.launches)
            if rep:
                times[k].append(t)
    lines = [
        "# MAE pretraining: token restore and the masked-patch loss (`tools/mae_rate.py`)",
        "",
        f"Device: {torch.cuda.get_device_name(0)}.",
        "",
        f"## (1) B = {B} images of {CH} x {SIDE} x {SIDE}, P = {P} patches of I = {I}, K = {K} kept, decoder width O = {O}, fp32",
        "",
        f"Device time per call from a replayed graph of {a.launches} calls; the graphs are replayed in turn, {a.reps} rounds after one warm-up round, "
        "the order reversed every other round; every figure listed. The stock compositions are the ones of `tests/_mae_ref.py`, timed the same "
        "way in the same process. The floor is the bytes the algorithm has to move at 6.3 TB/s (restore: the kept rows in, the sequence out, "
        "the position table once; its backward: the sequence in, the kept rows out; the loss: the dropped patches and their prediction rows in, "
        "all of `dpred` out); the stock compositions move more, which the floor does not count.",
        "",
        "| variant | us / call | every round | byte floor, us | floor / measured |",
        "|---|---|---|---|---|",
    ]
    for k, (_, nbytes) in variants.items():
        floor = 1e6 * nbytes / BW
        lines.append(f"| {k} | {med(times[k]):.1f} | {fmt(times[k], 1.0, 1)} | {floor:.1f} | {floor / med(times[k]):.2f} |")
    lines.append("")
    for ours, stock, what in ((order[0], order[1], "restore forward"), (order[2], order[3], "restore backward"), (order[4], order[5], "loss")):
        r = med(times[ours]) / med(times[stock])
        lines.append(f"{what}: kernel / stock = {r:.2f} ({'no slower' if r <= 1.0 else 'SLOWER'} than the stock composition; "
                     f"stock rounds span {min(times[stock]):.1f} .. {max(times[stock]):.1f} us).")
    lines.append("")
    del graphs
    torch.cuda.empty_cache()
    print("\n".join(lines), flush=True)
    if a.skip_train:
        lines += ["## (2) `train.py`: not measured (`--skip-train`)", ""]
    else:
        with tempfile.TemporaryDirectory() as tmp:
            runs = [("`--pretrain mae --mask-ratio 0.75 --decoder-dim 384 --decoder-blocks 2` (encoder on 50 tokens)", ROOT,
                     ["--pretrain", "mae", "--mask-ratio", "0.75", "--decoder-dim", "384", "--decoder-blocks", "2"]),
                    ("`--patch-dropout 0.75` (50 tokens)", ROOT, ["--patch-dropout", "0.75"]),
                    ("supervised (197 tokens)", ROOT, [])]
            if a.parent:
                runs.append(("parent commit, supervised", os.path.abspath(a.parent), []))
            argv = [*VITB, "--steps-per-epoch", str(a.steps), "--epochs", str(a.epochs)]
            got = {name: [] for name, _, _ in runs}
            for rep in range(2):
                for name, tree, flags in (runs if rep == 0 else runs[::-1]):
                    got[name].append(train_run(tree, [*argv, "--log-dir", os.path.join(tmp, f"log{rep}{len(name)}{tree == ROOT}"), *flags]))
                    print(f"(2) run {rep + 1} {name}: {fmt(got[name][-1], 1e3 / a.steps, 2)}", flush=True)
            unit = 1e3 / a.steps
            zero = med(got["supervised (197 tokens)"][0] + got["supervised (197 tokens)"][1])
            block = [f"## (2) ViT-B/16 ChebyKAN, batch 128, synthetic stream: ms per step ({a.steps} steps per epoch)", "",
                     "`epoch_seconds` (host clock around work that ends in the epoch's one synchronise) of every epoch after the first; two runs per "
                     "variant, one process each, alternated: run 1 in the order of the table, run 2 in the opposite order. No bound applies.", "",
                     "| variant | median | run 1 | run 2 | median / supervised |", "|---|---|---|---|---|"]
            for name, _, _ in runs:
                both = got[name][0] + got[name][1]
                block.append(f"| {name} | {med(both) * unit:.2f} | {fmt(got[name][0], unit, 2)} | {fmt(got[name][1], unit, 2)} | {med(both) / zero:.3f} |")
            block.append("")
            lines += block
            print("\n".join(block), flush=True)
    lines += ["The effect of pretraining on the accuracy of a fine-tuned run was not measured.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
