"""Which kernel form the fused KAN layer entry points (csrc/kan_layer.hip: plan_layer_fwd / plan_layer_bwd_input /
plan_layer_bwd_weight) choose, over a fixed table of layer descriptors and KANVIT_* switches.  Every row prints its label and every
host-visible answer -- the three layer workspace queries, kanvit_layer_ln_fusable, kanvit_layer_sine_dfreq_ok and, where a patch
geometry applies, kanvit_patch_embed_bwd_weight_ok / _workspace -- and then runs one forward, one input gradient and one weight
gradient through the C ABI on aligned buffers; a SINE row with dfreq_ok a second weight gradient under KANVIT_FLAG_SINE_DFREQ, a row
with patch_bw_ok one kanvit_patch_embed_bwd_weight.  Every return code is printed.  Two builds of the library choose the same forms when their outputs and the ordered kan_* kernel names, grids and LDS sizes
of their kernel traces agree:
    python tools/layer_forms.py --host-only                     (no GPU needed)
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/layer_forms.py
    KANVIT_LIB=<other build> timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir2> -- python tools/layer_forms.py
    python tools/layer_forms.py --diff <dir> <dir2>             (compares the two traces)"""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'kan-vit_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_forms import diff_traces

LINEAR, CHEBY, BSPLINE, RBF, SINE, FOURIER = range(6)
BF16, UNIFORM, SHARED, FUSED_LN, SINE_DFREQ = 1, 2, 4, 8, 16
# label, family, G, spline_order, has_base, flags, base_act: basis sizes with and without a compile-time register kernel
BASES = [("linear", LINEAR, 1, 0, 0, 0, 0), ("cheby5", CHEBY, 5, 0, 0, 0, 0), ("cheby4", CHEBY, 4, 0, 0, 0, 0),
         ("sine4", SINE, 4, 0, 0, 0, 0), ("sine5", SINE, 5, 0, 0, 0, 0), ("sine28", SINE, 28, 0, 0, 0, 0), ("fourier28", FOURIER, 28, 0, 0, 0, 0),
         ("bspline-uniform", BSPLINE, 8, 3, 1, UNIFORM, 0), ("bspline-uniform-shared", BSPLINE, 8, 3, 1, UNIFORM | SHARED, 0),
         ("bspline-knots", BSPLINE, 8, 3, 1, 0, 0), ("bspline-uniform-gelu", BSPLINE, 8, 3, 1, UNIFORM, 1),
         ("fastkan-uniform", RBF, 8, 0, 1, UNIFORM, 0), ("fastkan-knots", RBF, 8, 0, 1, 0, 0), ("fastkan-uniform-tanh", RBF, 8, 0, 1, UNIFORM, 4)]
INS, OUTS = (8, 36, 64, 256), (8, 16, 32, 48, 64, 128, 384)
GROUPS = ((1, 1), (3, 1), (36, 12))
ROWS = (64, 100, 300, 1000, 2758, 4224)
SWITCHES = ["", "KANVIT_NO_REG=1", "KANVIT_NO_BF16=1", "KANVIT_NO_TINY=1", "KANVIT_NO_PIPE=1", "KANVIT_NO_WS=1", "KANVIT_NO_FAST=1",
            "KANVIT_BI_NO_RES=1", "KANVIT_TAIL=0", "KANVIT_TAIL=5", "KANVIT_WS_NO_STRIP=1", "KANVIT_BF16_NSH=1", "KANVIT_BF16_IC=8",
            # the weight gradient's (plan_layer_bwd_weight)
            "KANVIT_NO_REG_BW=1", "KANVIT_BW_NO_T16=1", "KANVIT_BW_NO_DMA=1", "KANVIT_BW_DMA_FORCE=1", "KANVIT_BSPLINE_BW_BF16=1",
            "KANVIT_BSPLINE_BW_BF16=2"]
THIN = 29               # one row in THIN under every non-default switch: a prime above len(SWITCHES), so every switch keeps its own residue
PATCHES = {8: (2, 4, 4, 2), 36: (1, 12, 12, 2), 64: (1, 32, 32, 4), 256: (1, 64, 64, 4)}      # I -> (C, H, W, patches per side)
WORK_CAP = 1.5e11       # multiply-adds of a row: the largest combinations are dropped (every value of every dimension stays)


def gp_of(fam, G, has_base):
    return {LINEAR: 1, CHEBY: G, BSPLINE: G + has_base, RBF: G + has_base, SINE: G, FOURIER: 2 * G}[fam]


def rows():
    """(switch, label, descriptor fields).  The full product is thinned deterministically: a third of it under the default switches,
    one row in THIN under each of the others."""
    for si, sw in enumerate(SWITCHES):
        idx = 0
        for label, fam, G, order, hb, flags, act in BASES:
            for I in INS:
                for O in OUTS:
                    for groups, xmod in GROUPS:
                        for M in ROWS:
                            for bf in (0, BF16):
                                idx += 1
                                if (idx % 3) if si == 0 else (idx % THIN != si):
                                    continue
                                if float(M) * groups * I * gp_of(fam, G, hb) * O > WORK_CAP:
                                    continue
                                yield sw, label, dict(family=fam, groups=groups, x_group_mod=xmod, I=I, O=O, G=G, spline_order=order, has_base=hb,
                                                      flags=flags | bf, M=M, base_act=act)


def bparam_stride(f):
    I, G = f["I"], f["G"]
    return {BSPLINE: I * (G + f["spline_order"] + 1), RBF: G + 2 * I, SINE: G * (1 + I)}.get(f["family"], 0)


def make_desc(_lib, f):
    return _lib.LayerDesc(f["family"], f["groups"], f["x_group_mod"], f["I"], f["O"], f["G"], f["spline_order"], f["has_base"], 1.5, f["flags"], f["M"],
                          f["x_group_mod"] * f["I"], f["groups"] * f["I"], f["groups"] * f["O"], bparam_stride(f), 1e-5, f["base_act"])


def bparams_for(torch, f):
    """Valid basis parameters of one group, repeated per group: ascending knots (perturbed unless UNIFORM_KNOTS), centres, frequencies."""
    I, G, fam = f["I"], f["G"], f["family"]
    if fam == BSPLINE:
        nk = G + f["spline_order"] + 1
        k = torch.linspace(-2.2, 2.2, nk)
        if not f["flags"] & UNIFORM:
            k = k + 0.05 * torch.sin(torch.arange(nk, dtype=torch.float32))
        one = k.repeat(I)
    elif fam == RBF:
        one = torch.cat([torch.linspace(-2.0, 2.0, G), torch.ones(I), torch.zeros(I)])
    elif fam == SINE:
        one = torch.cat([torch.linspace(0.5, 2.0, G), 0.1 * torch.arange(I * G, dtype=torch.float32) % 3.0])
    else:
        return None
    return one.repeat(f["groups"]).cuda()


def main():
    if "--diff" in sys.argv:
        sys.exit(diff_traces(sys.argv[sys.argv.index("--diff") + 1:], what="kan_*", pattern=r"\bkan_\w+_kernel"))
    host_only = "--host-only" in sys.argv
    from kanvit import _lib
    L = _lib.lib()
    table = list(rows())
    if not host_only:
        import torch
        torch.manual_seed(0)
        size = lambda fn: max(fn(f) for _, _, f in table)
        x = torch.randn(size(lambda f: f["M"] * f["x_group_mod"] * f["I"]), device="cuda")
        u = torch.randn(size(lambda f: f["M"] * max(f["groups"] * f["I"], 2 * f["x_group_mod"])), device="cuda")
        w = 0.05 * torch.randn(size(lambda f: f["groups"] * f["I"] * gp_of(f["family"], f["G"], f["has_base"]) * f["O"]), device="cuda")
        ny = size(lambda f: f["M"] * f["groups"] * f["O"])
        y, dy = torch.empty(ny, device="cuda"), torch.randn(ny, device="cuda")
        dx, du = torch.empty_like(x), torch.empty_like(u)
        bias = torch.zeros(size(lambda f: f["groups"] * f["O"]), device="cuda")
        dparam = torch.empty(size(lambda f: ((f["M"] + 127) // 128) * f["groups"] * f["G"]), device="cuda")
        dy_seq = torch.randn(ny + ny // 4 + 64, device="cuda")      # the patch form's dY: one class-token row per image on top
        dw = torch.empty_like(w)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    names = sorted({s.split("=")[0] for sw in SWITCHES for s in sw.split() if s})
    current, count = None, 0
    for sw, label, f in table:
        if sw != current:
            for name in names:
                os.environ.pop(name, None)
            for s in sw.split():
                os.environ[s.split("=")[0]] = s.split("=")[1]
            _lib.reload_config()
            current = sw
        desc = make_desc(_lib, f)
        ln = 0
        if f["family"] == RBF and L.kanvit_layer_ln_fusable(C.byref(desc)):      # FUSED_LN where valid: the fused route replaces the plain one
            ln = 1
        out = [f"{sw or 'default'} {label} I={f['I']} O={f['O']} groups={f['groups']}/{f['x_group_mod']} M={f['M']} bf16={f['flags'] & BF16}",
               f"ln_fusable={ln}"]
        if ln:
            f = dict(f, flags=f["flags"] | FUSED_LN)
            desc = make_desc(_lib, f)
        nf, nb = int(L.kanvit_layer_fwd_workspace(C.byref(desc))), int(L.kanvit_layer_bwd_input_workspace(C.byref(desc)))
        nw, dfreq = int(L.kanvit_layer_bwd_weight_workspace(C.byref(desc))), L.kanvit_layer_sine_dfreq_ok(C.byref(desc))
        out += [f"fwd_ws={nf}", f"bwd_input_ws={nb}", f"bwd_weight_ws={nw}", f"dfreq_ok={dfreq}"]
        pd, npw = None, 0
        if f["groups"] == 1 and f["family"] != RBF and f["M"] % PATCHES[f["I"]][3] ** 2 == 0:
            pd = _lib.PatchDesc(*PATCHES[f["I"]], 1, 0)
            pok, npw = L.kanvit_patch_embed_bwd_weight_ok(C.byref(desc), C.byref(pd)), int(L.kanvit_patch_embed_bwd_weight_workspace(C.byref(desc), C.byref(pd)))
            out += [f"patch_bw_ok={pok}", f"patch_bw_ws={npw}"]
            pd = pd if pok else None
        count += 1
        if not host_only:
            bp = bparams_for(torch, f)
            ws = torch.empty(max(nf, nb, nw, npw, 16) // 4 + 4, device="cuda")
            pu = u.data_ptr() if f["family"] == RBF else None
            rf = L.kanvit_layer_fwd(C.byref(desc), x.data_ptr(), pu, w.data_ptr(), bp.data_ptr() if bp is not None else None, bias.data_ptr(),
                                    y.data_ptr(), ws.data_ptr(), C.c_size_t(nf), stream)
            rb = L.kanvit_layer_bwd_input(C.byref(desc), x.data_ptr(), pu, w.data_ptr(), bp.data_ptr() if bp is not None else None, dy.data_ptr(),
                                          dx.data_ptr(), du.data_ptr() if pu and not ln else None,
                                          dparam.data_ptr() if f["family"] == SINE else None, ws.data_ptr(), C.c_size_t(nb), stream)
            pbp = bp.data_ptr() if bp is not None else None
            rw = L.kanvit_layer_bwd_weight(C.byref(desc), x.data_ptr(), pu, pbp, dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), C.c_size_t(nw), stream)
            out.append(f"fwd={rf} bwd_input={rb} bwd_weight={rw}")
            if f["family"] == SINE and dfreq:
                dq = make_desc(_lib, dict(f, flags=f["flags"] | SINE_DFREQ))
                out.append(f"bwd_weight_dfreq={L.kanvit_layer_bwd_weight(C.byref(dq), x.data_ptr(), pu, pbp, dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), C.c_size_t(nw), stream)}")
            if pd is not None:      # x as the image batch (M / P images of I pixels), dY with the class-token rows
                out.append(f"patch_bw={L.kanvit_patch_embed_bwd_weight(C.byref(desc), C.byref(pd), x.data_ptr(), pbp, dy_seq.data_ptr(), dw.data_ptr(), ws.data_ptr(), C.c_size_t(npw), stream)}")
        print(" ".join(out), flush=True)
    if not host_only:
        torch.cuda.synchronize()
    print(f"{count} rows")


if __name__ == "__main__":
    main()
