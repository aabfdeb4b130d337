#!/usr/bin/env python3
"""Record what the kernel timer (kanvit.ops.timer, and through it bench.py's roofline leg) sees of a fixed set of small runs:
for every case the timer tags in order of first appearance, each with its number of launches and the flops and bytes of its
first launch.  No time is measured or kept.

    python tools/launch_ledger.py [--out tests/golden/launch_ledger.json]

tests/test_launch_ledger_gpu.py runs the same cases (CASES, run_case) and requires the committed ledger back, entry for entry:
a change to the Python launch path that renames a tag, drops or adds a launch, reorders first appearances or alters a cost
formula shows there.  Record the fixture on the commit whose behaviour is to be kept.  Needs the GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "kan-vit_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MODEL_TYPES = ("cheby", "efficientkan", "fast", "sine", "fourier", "vanilla")
SMALL = dict(chw=(1, 28, 28), n_patches=7, n_blocks=2, d_hidden=64, n_heads=2, out_d=10)
TINY_HEADS = dict(chw=(3, 32, 32), n_patches=4, n_blocks=2, d_hidden=64, n_heads=8, out_d=10)      # d_head = 8
# d = 128 has no fused small feed-forward, so the last block runs its class-token tail (model.py) in fp32
CLS_TAIL = dict(chw=(1, 28, 28), n_patches=7, n_blocks=2, d_hidden=128, n_heads=2, out_d=10)
BATCH = 8


def _model(geom, kind, dev):
    from model import VisionTransformer
    torch.manual_seed(0)
    return VisionTransformer(geom["chw"], n_patches=geom["n_patches"], n_blocks=geom["n_blocks"], d_hidden=geom["d_hidden"],
                             n_heads=geom["n_heads"], out_d=geom["out_d"], type=kind).to(dev)


def _train_step(geom, kind, dev, bf16):
    m = _model(geom, kind, dev)
    x = torch.rand(BATCH, *geom["chw"], device=dev)
    y = (torch.arange(BATCH) % geom["out_d"]).to(dev)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        loss = F.cross_entropy(m(x).float(), y)
    loss.backward()


def _msa_and_input(dev):
    msa = _model(SMALL, "efficientkan", dev).blocks[0].attn
    torch.manual_seed(1)
    return msa, torch.rand(BATCH, 50, 64, device=dev) * 2 - 1


def _msa_ops(dev):
    msa, x = _msa_and_input(dev)
    msa.regularization_loss(x).backward()
    msa.update_grid(x)
    msa.extend_grid(x, 7)
    msa.attention_map(x, rows=1)


def _attention_general(dev):
    from kanvit import ops
    torch.manual_seed(2)
    q, k, v = (torch.randn(1, 2, 300, 64, device=dev, requires_grad=True) for _ in range(3))
    ops.attention(q, k, v).sum().backward()


def _cases():
    cases = {}
    for kind in MODEL_TYPES:
        for bf16 in (False, True):
            cases[f"model_{kind}_{'bf16' if bf16 else 'fp32'}"] = lambda dev, k=kind, b=bf16: _train_step(SMALL, k, dev, b)
    cases["model_cheby_dhead8_fp32"] = lambda dev: _train_step(TINY_HEADS, "cheby", dev, False)
    for bf16 in (False, True):
        cases[f"model_cheby_d128_{'bf16' if bf16 else 'fp32'}"] = lambda dev, b=bf16: _train_step(CLS_TAIL, "cheby", dev, b)
    cases["msa_efficientkan_ops"] = _msa_ops
    cases["attention_general_300x64"] = _attention_general
    return cases


CASES = _cases()


def run_case(name, dev="cuda:0"):
    """[[tag, launches, flops, bytes], ...] of one case, tags in order of first appearance."""
    from kanvit import ops
    assert ops.timer is None, "another kernel timer is active"
    ops.timer = ops.KernelTimer()
    try:
        CASES[name](torch.device(dev))
        torch.cuda.synchronize()
        return [[tag, len(recs), int(recs[0][2]), int(recs[0][3])] for tag, recs in ops.timer.records.items()]
    finally:
        ops.timer = None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON ledger here (default: print it)")
    args = ap.parse_args()
    ledger = {name: run_case(name) for name in CASES}
    text = json.dumps(ledger, indent=1) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(f"{len(ledger)} cases, {sum(len(v) for v in ledger.values())} tags -> {args.out}")
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
