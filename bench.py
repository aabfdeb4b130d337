#!/usr/bin/env python3
"""bench.py -- images/s of a full ViKANformer train step on N MI355X (one process per GPU).

    python bench.py                                   # N=1, default workload, finishes in ~1-2 min
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A step = forward + CrossEntropy + zero_grad + backward (+ gradient all-reduce when N > 1) +
Adam.step on one synthetic batch that is already resident in HBM (train.py:31-40 of the
reference).  Weak scaling: the per-GPU batch is fixed, value = N * batch * K / t.

With --dump-outputs DIR rank 0 also writes what the last timed step computed (dump_outputs below) as float32 .npy files; the
inputs and the initial weights are seeded, so two builds run with the same arguments can be compared output for output.

Rank 0 prints ONE JSON line.  Besides the driver's contract it carries
  roofline      the dominant hand-written kernel: algorithmic flops divided
                by its average launch time measured live with events on the launch stream
  kernels       the same for every C-ABI launch class (extra, for DESIGN.md tables)
  cpu_baseline  the CPU oracle in reference-faithful mode (per-sample x per-head python loop,
                attention.py:188-202) timed on this box's host cores on a bounded sample
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "kan-vit_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

WORKLOADS = {
    # BASELINE.json metric: "images/sec (train step) KAN-ViT 224x224"; target workload of north_star
    "vitb16-224-cheby": dict(chw=(3, 224, 224), n_patches=14, n_blocks=12, d=768, heads=12, out_d=100, type="cheby", batch=128),
    "vits16-224-cheby": dict(chw=(3, 224, 224), n_patches=14, n_blocks=12, d=384, heads=6, out_d=100, type="cheby", batch=256),
    "vits16-224-fast": dict(chw=(3, 224, 224), n_patches=14, n_blocks=12, d=384, heads=6, out_d=100, type="fast", batch=256),
    "vitb16-224-efficientkan": dict(chw=(3, 224, 224), n_patches=14, n_blocks=12, d=768, heads=12, out_d=100, type="efficientkan", batch=128),
    "vitb16-224-sine": dict(chw=(3, 224, 224), n_patches=14, n_blocks=12, d=768, heads=12, out_d=100, type="sine", batch=128),
    "vitb16-224-fourier": dict(chw=(3, 224, 224), n_patches=14, n_blocks=12, d=768, heads=12, out_d=100, type="fourier", batch=128),
    # BASELINE.json configs[4]: "SineKAN + FourierKAN ViT-B mixed blocks" -- blocks alternate sine / fourier (model.split_types)
    "vitb16-224-sine+fourier": dict(chw=(3, 224, 224), n_patches=14, n_blocks=12, d=768, heads=12, out_d=100, type="sine,fourier", batch=128),
    # BASELINE.json configs[1]: MNIST-shaped defaults of model.py:49
    "mnist-cheby-tiny": dict(chw=(1, 28, 28), n_patches=7, n_blocks=4, d=64, heads=2, out_d=10, type="cheby", batch=128),
    # train.py:18-20 geometry
    "cifar-cheby-default": dict(chw=(3, 32, 32), n_patches=4, n_blocks=8, d=64, heads=8, out_d=100, type="cheby", batch=128),
}
PEAK_FP32_MFMA_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
PEAK_BF16_MFMA_TFLOPS = 2500.0    # same table, dense bf16 (never the 2:1-sparsity figure)
PEAK_HBM_GBS = 8000.0


class _StdoutToStderr:
    """RCCL prints a version banner on the C-level stdout when the first communicator is created; the
    contract is ONE JSON line on stdout, so fd 1 points at stderr while the process group comes up."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` with N > 1 and no RANK in the environment: start the N ranks ourselves -- one CHILD process
    per GPU under torch.distributed.run, exactly the command line the docstring gives -- BEFORE this process has made any GPU
    call (it never does: it only relays), pass rank 0's single JSON line through to stdout and return the launcher's exit
    code.  No exec: a process that may have touched the GPU must not be replaced on this pool."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: RCCL across processes needs it on this host driver
    # --standalone: the launcher's own c10d rendezvous on a port IT binds (endpoint port 0) -- nothing is probed and released
    # here for another process to take in between; --local-addr keeps every address on 127.0.0.1 (the hostname may not resolve)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           f"--nproc-per-node={n}", os.path.abspath(__file__)] + sys.argv[1:]
    print("bench.py: launching " + " ".join(cmd), file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = None
    for out in proc.stdout:                                     # stderr of the ranks is inherited (progress, warnings)
        t = out.strip()
        if t.startswith("{") and '"metric"' in t:
            line = t
        elif t:
            print(t, file=sys.stderr, flush=True)
    rc = proc.wait()
    if line is not None:
        print(line, flush=True)
    if rc == 0 and line is None:
        print("bench.py: the ranks exited 0 without a result line", file=sys.stderr)
        rc = 1
    return rc


def host_cores():
    """CPU cores this process may really use: affinity mask, cgroup quota, and the GPU box's per-GPU
    share (16).  os.cpu_count() reports all 256 host threads and oversubscribes torch ~16x."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except Exception:
        pass
    return int(os.environ.get("KANVIT_CPU_THREADS", min(n, 16)))


def cpu_baseline(model, wl, target_s=15.0):
    """Reference-faithful CPU train step (oracle/kan_oracle.py, the checker -- never the product)."""
    from oracle import kan_oracle as ko
    ko.REFERENCE_OP_SEQUENCE = True          # the reference's own op sequences for ChebyKAN / SineKAN (calibrated: profiles/r02_cpu_baseline_calibration.json)
    torch.set_num_threads(host_cores())
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    n_patches, heads, t = wl["n_patches"], wl["heads"], wl["type"]

    def step(n):
        g = torch.Generator().manual_seed(7)
        x = torch.randn(n, *wl["chw"], generator=g)
        y = torch.randint(0, wl["out_d"], (n,), generator=g)
        t0 = time.perf_counter()
        ko.train_steps(sd, x, y, n_patches, heads, t, steps=1, faithful_loop=True)
        return time.perf_counter() - t0

    t1 = step(1)                                    # warm-up + calibration
    n = int(max(1, min(wl["batch"], target_s / max(t1, 1e-3))))
    tn = step(n)
    return {"value": round(n / tn, 3), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"1 train step (fwd+loss+bwd+Adam) on {n} images of {wl['chw']}, reference-style "
                      f"per-sample x per-head loop, after a 1-image warm-up step ({t1:.2f} s)"}


PMC_TRAFFIC_FILES = ("r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json")     # newest first


def _pmc_traffic(tag, workload, batch):
    """HBM bytes per launch of launch class `tag` from the COMMITTED rocprofv3 --pmc passes of this workload (FETCH_SIZE and
    WRITE_SIZE are collected in separate runs; (2*FETCH + WRITE) KiB per the guide's gfx950 rule).  It is a recorded
    measurement of the same kernels, not a measurement of this run: `traffic_source` in the line says so."""
    for fn in PMC_TRAFFIC_FILES:
        try:
            pmc = json.load(open(os.path.join(ROOT, "profiles", fn)))
            rec = pmc["kernels"].get(tag)
            if pmc["workload"] == workload and pmc["per_gpu_batch"] == batch and rec and rec.get("write_kib") is not None:
                return (2 * rec["fetch_kib"] + rec["write_kib"]) * 1024, f"profiles/{fn} (separate --pmc passes of this workload, recorded)"
        except Exception:
            pass
    return None, None


def _roof(tag, k, workload, batch):
    ai = k["alg_flops"] / k["alg_bytes"]
    mfma_peak = PEAK_BF16_MFMA_TFLOPS if tag.endswith("_bf16") else PEAK_FP32_MFMA_TFLOPS
    mfma_bound = ai > mfma_peak * 1e3 / PEAK_HBM_GBS                   # ridge: 19.7 flop/B fp32 pipe, 312 bf16 pipe
    if mfma_bound:
        roof = {"bound": "mfma", "achieved": k["TFLOP/s"], "peak": mfma_peak, "unit": "TFLOP/s",
                "frac": round(k["TFLOP/s"] / mfma_peak, 4)}
    else:
        roof = {"bound": "hbm", "achieved": k["GB/s"], "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": round(k["GB/s"] / PEAK_HBM_GBS, 4)}
    roof["traffic"], src = _pmc_traffic(tag, workload, batch)
    if src:
        roof["traffic_source"] = src
    roof.update({"kernel": tag, "avg_launch_ms": k["avg_ms"], "ms_per_step": k["ms_per_step"],
                 "arith_intensity_flop_per_byte": round(ai, 1), "hbm_GB/s": k["GB/s"], "hbm_frac": round(k["GB/s"] / PEAK_HBM_GBS, 4)})
    return roof


def roofline_report(kern, steps, workload, batch):
    """Per-op table + `roofline`: the hand-written op with the largest time per step over ALL launch classes (KAN layers and
    attention alike) + `roofline_kan`: the same for the dominant fused KAN basis+contraction op (north_star's target kernel)."""
    res = {}
    kernels = {}
    for tag, r in kern.items():
        tf = r["flops"] / (r["avg_ms"] * 1e-3) / 1e12
        gb = r["bytes"] / (r["avg_ms"] * 1e-3) / 1e9
        kernels[tag] = {"launches_per_step": r["launches"] / steps, "avg_ms": round(r["avg_ms"], 4),
                        "ms_per_step": round(r["total_ms"] / steps, 3), "TFLOP/s": round(tf, 2),
                        "GB/s": round(gb, 1), "alg_flops": r["flops"], "alg_bytes": r["bytes"]}
    if not kernels:
        return res
    dom = max(kernels, key=lambda t: kernels[t]["ms_per_step"])
    res["roofline"] = _roof(dom, kernels[dom], workload, batch)
    kan = [t for t in kernels if t.startswith(("qkv", "layer"))]
    if kan:
        dk = max(kan, key=lambda t: kernels[t]["ms_per_step"])
        res["roofline_kan"] = _roof(dk, kernels[dk], workload, batch)
    res["kernels"] = kernels
    res["custom_kernel_ms_per_step"] = round(sum(v["ms_per_step"] for v in kernels.values()), 3)
    return res


DUMP_SAMPLE = 1 << 22        # elements per sampled array: 16 MB of float32 each, well inside the 64 MB budget of a dump


def dump_outputs(out_dir, model, logits, loss):
    """--dump-outputs: what the last timed step handed its caller, as float32 .npy files, so that two builds can be compared
    output for output.  logits.npy and loss.npy are whole; grads.npy and params.npy (the weights after the Adam update) are the
    trainable parameters flattened in named_parameters() order, whole when they fit in DUMP_SAMPLE elements and otherwise the
    same DUMP_SAMPLE sorted positions drawn by a fixed seed (they depend only on the parameter count, so on the workload)."""
    import numpy as np
    params = [p for p in model.parameters() if p.requires_grad]
    flat_p = torch.cat([p.detach().reshape(-1) for p in params])
    flat_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1) for p in params])
    if flat_p.numel() > DUMP_SAMPLE:
        idx = torch.randint(0, flat_p.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
        idx = idx.to(flat_p.device)
        flat_p, flat_g = flat_p[idx], flat_g[idx]
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"logits": logits, "loss": loss.reshape(1), "grads": flat_g, "params": flat_p}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a.detach().float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="vitb16-224-cheby", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: the workload's)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timer", action="store_true")
    ap.add_argument("--no-amp-leg", action="store_true", help="skip the secondary measurements (bf16 autocast, bf16x3 feed-forward) of the default run")
    ap.add_argument("--no-tuned-gemms", action="store_true",
                    help="library-default kernel selection for the stock GEMMs instead of the recorded TunableOp results (kanvit/tuned.py)")
    ap.add_argument("--ff", choices=["fp32", "bf16x3"], default="fp32",
                    help="feed-forward GEMMs: stock fp32 (default, the parity path) or three-term bf16 split products (~5e-6 relative)")
    ap.add_argument("--bucket-mib", type=float, default=64.0)
    ap.add_argument("--amp", choices=["off", "bf16"], default="off",
                    help="bf16 autocast for the stock dense ops (FF GEMMs); the kanvit kernels stay fp32 at their boundary")
    ap.add_argument("--graph", choices=["auto", "on", "off"], default="auto",
                    help="capture the whole train step in a HIP graph (auto: single GPU and a launch-bound workload)")
    ap.add_argument("--rendezvous-only", action="store_true",
                    help="(test hook) bring the process group up, all-reduce one number, print a stub line and exit: exercises the "
                         "self-launch / relay path without a GPU (KANVIT_DIST_BACKEND=gloo)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed (logits, loss, sampled gradients and updated "
                         "weights) as DIR/<name>.npy; rank 0 only")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(args.gpus))                    # plain `python bench.py --gpus N`: spawn the ranks, relay the line
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        args.gpus = world                                   # under a launcher the launcher's world size is the truth
    import torch.distributed as dist
    if args.rendezvous_only:
        dist.init_process_group(os.environ.get("KANVIT_DIST_BACKEND", "gloo"))
        t = torch.ones(1)
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"metric": "rendezvous-only", "n_gpus": world, "sum_of_ones": float(t)}), flush=True)
        dist.destroy_process_group()
        return
    # Rehearsal hooks for a ONE-GPU box (not used by the driver): KANVIT_SHARE_GPU=1 maps every rank to cuda:0 and
    # KANVIT_DIST_BACKEND=gloo swaps the transport, so the N > 1 control flow of this file (reducer hooks, barriers, max over
    # ranks, one line from rank 0) can be exercised where RCCL cannot (it refuses two ranks on one device).
    if os.environ.get("KANVIT_SHARE_GPU") == "1":
        local = 0
    backend = os.environ.get("KANVIT_DIST_BACKEND", "nccl")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    force_dp = os.environ.get("KANVIT_FORCE_DP") == "1" and "RANK" in os.environ   # 1-rank rehearsal of the RCCL path
    if world > 1 or force_dp:
        with _StdoutToStderr():
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=dev)
            else:
                dist.init_process_group(backend)
            dist.all_reduce(torch.zeros(1, device=dev))          # forces communicator creation (and its banner) now
            torch.cuda.synchronize()

    from kanvit import _lib as klib
    from kanvit import dense as kdense
    from kanvit import dp as kdp
    from kanvit import ops
    from model import VisionTransformer
    kdense.FF_MODE = args.ff
    from kanvit import tuned as ktuned
    tuned_ok = (not args.no_tuned_gemms) and not os.environ.get("PYTORCH_TUNABLEOP_ENABLED") and ktuned.enable_tuned_gemms()

    wl = dict(WORKLOADS[args.workload])
    if args.batch:
        wl["batch"] = args.batch
    torch.manual_seed(0)
    model = VisionTransformer(wl["chw"], wl["n_patches"], wl["n_blocks"], wl["d"], wl["heads"], wl["out_d"],
                              type=wl["type"]).to(dev)
    kdp.broadcast_parameters(model)
    use_graph = args.graph == "on" or (args.graph == "auto" and world == 1 and not force_dp and wl["d"] <= 128)
    # fused=True: the same Adam update (train.py:33 uses optim.Adam) as one multi-tensor kernel per chunk instead of ~8
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=use_graph, fused=True)
    reducer = kdp.GradReducer(model.parameters(), bucket_mib=args.bucket_mib, always_reduce=force_dp,
                              timing=True) if (world > 1 or force_dp) else None
    crit = torch.nn.CrossEntropyLoss()
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    x = torch.randn(wl["batch"], *wl["chw"], device=dev, generator=g)
    y = torch.randint(0, wl["out_d"], (wl["batch"],), device=dev, generator=g)

    amp_on = [args.amp == "bf16"]
    last = {}       # the last step's logits for --dump-outputs, detached: a kept autograd graph would carry its AccumulateGrad
                    # nodes, bound to the stream of that step, into the next step (the side-stream warm-up, the graph capture)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp_on[0]):
            logits = model(x)
            loss = crit(logits, y)
        last["logits"] = logits.detach()
        if reducer is not None:
            reducer.zero_grad()
            reducer.scale_loss(loss).backward()        # sums over ranks become means inside the collective / the loss: no pass over the buckets
            reducer.finish()
        else:
            opt.zero_grad()
            loss.backward()
        opt.step()
        return loss

    def fence():
        torch.cuda.synchronize()
        if world > 1 or force_dp:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    kern = {}
    if use_graph:
        # Launch-bound geometries (MNIST-tiny, train.py defaults): ~1 ms of kernels behind ~5-14 ms of launches.
        # Capture forward + loss + backward + Adam once and replay it: HIP graphs instead of a tracing compiler.
        # Per-kernel event timing cannot run inside a capture, so the roofline leg times 3 eager steps first.
        if not args.no_kernel_timer:
            ops.timer = ops.KernelTimer()
            for _ in range(3):
                step()
            kern = ops.timer.summary()
            for r in kern.values():
                r["launches"] = r["launches"] * args.steps / 3.0
                r["total_ms"] = r["total_ms"] * args.steps / 3.0
            ops.timer = None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        opt.zero_grad(set_to_none=True)
        last.clear()                                        # freed here, not inside the capture
        with torch.cuda.graph(graph):
            static_loss = step()
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            graph.replay()
        fence()
        dt = time.perf_counter() - t0
        loss = static_loss
    else:
        if not args.no_kernel_timer:
            ops.timer = ops.KernelTimer()
        if reducer is not None:
            reducer.reset_timing()
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step()
        fence()
        dt = time.perf_counter() - t0
        kern = ops.timer.summary() if ops.timer is not None else {}
        ops.timer = None
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1 or force_dp:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax)
    final_loss = float(loss.detach())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, model, last["logits"], loss)

    if rank == 0:
        ms = 1e3 * dt / args.steps
        out = {
            "metric": "images/sec (train step) KAN-ViT 224x224" if "224" in args.workload else "images/sec (train step)",
            "value": round(world * wl["batch"] * args.steps / dt, 2), "unit": "images/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": ("f32" if args.ff == "fp32" else "f32 (feed-forward GEMMs as three-term bf16 split products, f32 accumulate)") if args.amp == "off"
                     else "bf16 autocast (stock GEMMs) + f32 kanvit kernels", "data": "synthetic",
            "config": {"workload": args.workload, "model_type": wl["type"], "image": list(wl["chw"]),
                       "n_patches": wl["n_patches"], "n_blocks": wl["n_blocks"], "d_hidden": wl["d"],
                       "n_heads": wl["heads"], "per_gpu_batch": wl["batch"], "global_batch": world * wl["batch"],
                       "parallelism": f"dp{world}", "rccl_ranks": (dist.get_world_size() if dist.is_initialized() and backend == "nccl" else 0),
                       "dist_backend": (backend if dist.is_initialized() else None),
                       "optimizer": "Adam(lr=1e-3, fused)", "hip_graph": bool(use_graph), "tuned_gemm_selection": bool(tuned_ok),
                       "kanvit_switches": klib.active_config(), "loss_after": round(final_loss, 4)},
        }
        out.update(roofline_report(kern, args.steps, args.workload, wl["batch"]))
        if reducer is not None:
            # gradient exchange of rank 0 over the timed steps: all-reduce time on the stream the collectives are issued from,
            # the part of it backward did not hide (what the compute stream waited in finish()), bucket count and bytes
            out["comm"] = reducer.comm_summary()
        if world == 1 and args.amp == "off" and not use_graph and not force_dp and not args.no_amp_leg:
            # Secondary measurement, same run: the same step with the stock GEMMs under bf16 autocast and the kanvit kernels on
            # the bf16 matrix cores (BASELINE configs[2]/[4] name bf16 for the 224x224 streams).  `value` above is the fp32 path.
            amp_on[0] = True
            for _ in range(2):
                step()
            if not args.no_kernel_timer:
                ops.timer = ops.KernelTimer()
            asteps = max(3, args.steps // 2)
            fence()
            t0 = time.perf_counter()
            for _ in range(asteps):
                aloss = step()
            fence()
            adt = time.perf_counter() - t0
            akern = ops.timer.summary() if ops.timer is not None else {}
            ops.timer = None
            amp_on[0] = False
            leg = {"value": round(wl["batch"] * asteps / adt, 2), "unit": "images/s", "steps": asteps, "warmup": 2,
                   "ms_per_step": round(1e3 * adt / asteps, 3), "dtype": "bf16 autocast (stock GEMMs) + kanvit kernels on bf16 MFMA, f32 I/O and accumulate",
                   "loss_after": round(float(aloss.detach()), 4)}
            leg.update(roofline_report(akern, asteps, args.workload, wl["batch"]))
            out["amp_bf16"] = leg
            if args.ff == "fp32":
                # Third measurement, same run: fp32 everywhere except that the feed-forward GEMMs are formed as three-term
                # bf16 split products on the bf16 matrix cores (kanvit/dense.py; ~5e-6 relative, inside the 1e-4 parity budget
                # but not bit-faithful fp32 products, hence not the headline).
                kdense.FF_MODE = "bf16x3"
                for _ in range(2):
                    step()
                fence()
                t0 = time.perf_counter()
                for _ in range(asteps):
                    sloss = step()
                fence()
                sdt = time.perf_counter() - t0
                kdense.FF_MODE = "fp32"
                out["ff_bf16x3"] = {"value": round(wl["batch"] * asteps / sdt, 2), "unit": "images/s", "steps": asteps, "warmup": 2,
                                    "ms_per_step": round(1e3 * sdt / asteps, 3),
                                    "dtype": "f32 kanvit kernels + feed-forward GEMMs as three-term bf16 split products (f32 accumulate)",
                                    "loss_after": round(float(sloss.detach()), 4)}
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(model, wl)
        print(json.dumps(out), flush=True)
    if world > 1 or force_dp:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
