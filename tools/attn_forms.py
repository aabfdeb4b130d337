"""Which kernel form the one-work-group attention entry points (csrc/attention.hip: plan_attn_fwd / plan_attn_bwd) choose, over a
fixed table of shapes, precisions, KANVIT_ATTN_* switches and pointer alignments: one forward and one backward per row, after
printing the row's label and kanvit_attn_bwd_workspace.  Two builds of the library choose the same forms when their outputs and the
ordered attn* kernel names, grids and LDS sizes of their kernel traces agree:
    python tools/attn_forms.py --workspace-only                 (host only: no GPU needed)
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/attn_forms.py
    KANVIT_LIB=<other build> timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir2> -- python tools/attn_forms.py
    python tools/attn_forms.py --diff <dir> <dir2>             (compares the two traces)"""
import csv
import ctypes as C
import glob
import os
import re
import sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'kan-vit_amd'))

B, H = 2, 3
SHAPES = [(n, d) for n in (17, 32, 33, 64, 65, 96, 129, 197, 204, 208, 224) for d in (8, 16, 32, 64)] + [(256, 32)]
SWITCHES = ["", "KANVIT_ATTN_V1", "KANVIT_ATTN_V2", "KANVIT_ATTN_V3", "KANVIT_ATTN_V4", "KANVIT_ATTN_NO_DS", "KANVIT_NO_BF16"]


def rows():
    for sw in SWITCHES:
        for n, d in SHAPES:
            for causal in (0, 1):
                for flags in (0, 1):            # 1 = KANVIT_FLAG_BF16_MFMA
                    if sw == "KANVIT_NO_BF16" and not flags:
                        continue
                    for off in (0, 1):          # q and dq one float past a 16-byte boundary
                        yield sw, n, d, causal, flags, off


def trace_launches(directory, pattern=r"\battn(16)?_\w+_kernel"):
    """(kernel name, grid, LDS bytes) of the launches of a rocprofv3 --kernel-trace run whose kernel name matches `pattern`, in launch order."""
    out = []
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        recs = [r for r in csv.DictReader(open(path)) if re.search(pattern, r["Kernel_Name"])]
        recs.sort(key=lambda r: int(r["Start_Timestamp"]))
        grid = [c for c in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z") if recs and c in recs[0]] or ["Grid_Size"]
        out += [(r["Kernel_Name"], " x ".join(r[c] for c in grid), r["LDS_Block_Size"]) for r in recs]
    return out


def diff_traces(directories, what="attn*", **kw):
    """Compare the ordered launches of two traces; the exit status (0 = equal and not empty)."""
    a, b = (trace_launches(p, **kw) for p in directories[:2])
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    for i, x, y in bad[:20]:
        print(f"launch {i}: {x} != {y}")
    print(f"{len(a)} and {len(b)} {what} launches, {len(bad)} differ")
    return 1 if bad or len(a) != len(b) or not a else 0


def main():
    if "--diff" in sys.argv:
        sys.exit(diff_traces(sys.argv[sys.argv.index("--diff") + 1:]))
    host_only = "--workspace-only" in sys.argv
    from kanvit import _lib
    L = _lib.lib()
    if not host_only:
        import torch
        torch.manual_seed(0)
        nmax = max(B * H * n * d for n, d in SHAPES) + 4
        bufs = {name: torch.randn(nmax, device="cuda") for name in ("q", "k", "v", "o", "do", "dq", "dk", "dv")}
        lse = torch.empty(B * H * 256, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    current, count = None, 0
    for sw, n, d, causal, flags, off in rows():
        if sw != current:
            for name in SWITCHES[1:]:
                os.environ.pop(name, None)
            if sw:
                os.environ[sw] = "1"
            _lib.reload_config()
            current = sw
        s = (H * n * d, n * d, d)
        desc = _lib.AttnDesc(B, H, n, d, causal, d ** -0.5, flags, 0, *s, *s, *s, *s)
        nbytes = int(L.kanvit_attn_bwd_workspace(C.byref(desc)))
        print(f"{sw or 'default'} N={n} D={d} causal={causal} bf16={flags} offset={off} workspace={nbytes}", flush=True)
        count += 1
        if host_only:
            continue
        p = {name: t.data_ptr() + (4 * off if name in ("q", "dq") else 0) for name, t in bufs.items()}
        ws = torch.empty(max(nbytes // 4, 1), device="cuda")
        _lib.check(L.kanvit_attn_fwd(C.byref(desc), p["q"], p["k"], p["v"], p["o"], lse.data_ptr(), stream), "kanvit_attn_fwd")
        _lib.check(L.kanvit_attn_bwd(C.byref(desc), p["q"], p["k"], p["v"], p["o"], lse.data_ptr(), p["do"], p["dq"], p["dk"], p["dv"],
                                     ws.data_ptr(), C.c_size_t(nbytes), stream), "kanvit_attn_bwd")
    if not host_only:
        torch.cuda.synchronize()
    print(f"{count} rows")


if __name__ == "__main__":
    main()
