"""Compile the HIP sources in ../csrc into kanvit/libkanvit.so for gfx950 (MI355X).

hipcc cross-compiles without a GPU, so this runs in the build container; the .so is
git-ignored but travels to the GPU box with the working tree snapshot.

    python kan-vit_amd/kanvit/build.py [--force]
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "csrc")
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include")
LIB = os.path.join(HERE, "libkanvit.so")
# the fused KAN layer kernels are one translation unit per kernel generation (kan_layer_common.h): parallel compiles, and a
# rebuild costs only the kernel that changed.  22 units (tests/test_attention_map_cpu.py counts them): the feed-forward's two small
# helper passes, kanvit_relu_bwd_bias and kanvit_split3_bf16, share ff_epilogue.hip; the training loop's off-model kernels are one
# unit per family (batch_u8, soft_ce, metrics, optim).  The data family has two files: batch_u8.hip includes randaug.hip (the
# per-epoch RandAugment pass) at its end, so the two compile as one unit and randaug.hip is a dependency below, not a source.
# In the same way addln.hip includes patch_drop.hip (PatchDropout: the keep table shares kanvit_depth_scales' hash step), and
# optim.hip includes edge_prune.hip (KAN edge pruning: kanvit_mask_rows follows the optimizer's multi-tensor chunking), and
# soft_ce.hip includes mae.hip (MAE pretraining: the masked-patch loss shares the ordered row sum of the cross-entropy's mean).
SOURCES = ["kan_tile.hip", "kan_fwd_reg.hip", "kan_fwd_reg_bf16.hip", "kan_bwd_input_reg.hip", "kan_bwd_input_reg_bf16.hip",
           "kan_bwd_weight_reg.hip", "kan_bwd_weight_dma.hip", "kan_layer.hip", "attention.hip", "attention16.hip", "attention_x.hip", "attention_probs.hip", "addln.hip", "ff_small.hip", "ff_epilogue.hip", "kan_tiny.hip", "kan_edge_l1.hip",
           "kan_bspline_refit.hip", "batch_u8.hip", "soft_ce.hip", "metrics.hip", "optim.hip"]
HEADERS = ["kan_basis.h", "kanvit_common.h", "kan_layer_common.h", "attention_common.h", "randaug.hip", "patch_drop.hip", "edge_prune.hip", "mae.hip", os.path.join(INCLUDE, "kanvit.h")]
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=on", "-fno-finite-math-only", "-fvisibility=hidden"]


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [h if os.path.isabs(h) else os.path.join(CSRC, h) for h in HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    """(Re)build libkanvit.so when a source is newer than it. Returns the library path."""
    if not force and not _stale():
        return LIB
    objs = []
    procs = []
    for s in SOURCES:
        o = os.path.join(HERE, s.replace(".hip", ".o"))
        cmd = [_hipcc(), *FLAGS, "-I", INCLUDE, "-c", os.path.join(CSRC, s), "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(o)
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {s}:\n{out}")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB + ".tmp"]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}")
    os.replace(LIB + ".tmp", LIB)
    for o in objs:
        os.remove(o)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
