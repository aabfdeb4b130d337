"""kanvit_layer_fwd / kanvit_layer_bwd_input / kanvit_layer_bwd_weight on padded and misaligned operands, through ctypes.

The Python ops make every tensor contiguous and pass the minimal row strides, and the torch allocator hands out 16-byte aligned
blocks, so through the modules the three host plans (csrc/kan_layer.hip) only ever see packed, aligned operands.  The C ABI
(include/kanvit.h) promises more: 4-byte aligned pointers, any ld at least the documented minimum.  Here every operand is a
[rows, width] view with row stride ld that starts GUARD + shift floats into its own flat, 16-byte aligned device buffer:

  * input buffers hold NaN outside the view, output buffers (y, dx, du, dw, dparam) a finite sentinel everywhere;
  * after every call each buffer must be bitwise unchanged outside its view -- the padding columns between rows included -- and
    the view of an output must hold no NaN (a read outside an input view surfaces as one);
  * every case runs twice on fresh buffers and must be bitwise repeatable (the ABI: deterministic, no atomics);
  * y, dx, du, dw and SINE's summed dparam are compared with the float64 formula of the header (tests/_layer_abi_ref.py, pinned
    to the oracle by tests/test_layer_abi_ref_cpu.py) at the suite's bounds (tests/test_launch_shapes_gpu.py), chosen per entry
    point by the kernels it launched: exact fp32 kernels FWD / TOL (also under the bf16 flag, where a layout moves the call to
    them), bf16 kernels TIGHT against the bf16-operand reference and LOOSE against the unrounded one;
  * the kan_* kernels each entry point launched (tests/_util.record_kernels, first run) are asserted as literals (FORMS: recorded on
    the MI355X, listed beside the plans' predictions in profiles/layer_strided_forms.md), and an entry point that launched the
    kernels it launches for `packed` must return bitwise what it returns for `packed` -- always so for `pad4`: a stride is pure
    addressing.

Layouts: packed (what ops passes) | pad4 (every ld and bparam_stride + 4 floats) | pad1:<ldx|ldu|ldy|bp> (that stride + 1) |
shift:<operand> (that operand's base one float past a 16-byte boundary) | shift:all (every operand shifted, every ld + 1) |
nobias (bias = NULL).  Descriptors and packed operands come from the modules (kan_cfg, kan_pack, ops._desc).  Families without a
bias parameter get a random one: the formula of the ABI has it for every family.

Three more groups follow the layout cases.  F's weight gradient under KANVIT_BW_DMA_FORCE: the LDS-DMA form for packed / pad4 and
the register ring for every layout that takes x or dy off the 16-byte grid or a stride off the 4-float grid.  KANVIT_FLAG_FUSED_LN,
which has register kernels only: the calls a register kernel serves as they are (aligned; the forward with x shifted; the weight
gradient with x, dy shifted) with numbers, statistics, guards and names, and the calls that are refused (KANVIT_EINVAL: y in the
forward, x / dx / dy in the input gradient, the statistics buffer off the 8-byte grid).  A bf16 workspace off the 16-byte grid is
KANVIT_ENOMEM.  Refused calls launch nothing and leave every output buffer bitwise untouched."""
import ctypes as C
import functools
from dataclasses import replace

import pytest
import torch

from tests import _layer_abi_ref as ref
from tests._util import record_kernels
from tests.test_launch_shapes_gpu import FWD, LOOSE, TIGHT, TOL, _Err

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64            # floats before and after every view (a multiple of 4: the guard does not move the 16-byte alignment)
SENTINEL = -24680.5   # output buffers before the run
EINVAL, ENOMEM = -22, -12
ENTRIES = ("fwd", "bwd_input", "bwd_weight")


# ---- operands between guards ------------------------------------------------------------------------------------------------
class Operand:
    """A [rows, width] view with row stride ld at element GUARD + shift of its own flat buffer: NaN elsewhere for an input
    (`data` given), SENTINEL everywhere for an output."""

    def __init__(self, rows, width, ld, shift, data=None):
        assert ld >= width and shift >= 0
        n = GUARD + shift + (rows - 1) * ld + width + GUARD
        self.buf = torch.full((n,), float("nan") if data is not None else SENTINEL, device=DEV, dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf.as_strided((rows, width), (ld, 1), GUARD + shift)
        if data is not None:
            self.view.copy_(data.reshape(rows, width))
        self.before = self.buf.clone()
        self.ptr = C.c_void_p(self.view.data_ptr())
        assert self.view.data_ptr() % 16 == 4 * (shift % 4)

    def outside_unchanged(self):
        """every element of the buffer outside the view is bitwise what it was"""
        now = self.buf.clone()
        now.as_strided(self.view.shape, self.view.stride(), self.view.storage_offset()).copy_(
            self.before.as_strided(self.view.shape, self.view.stride(), self.view.storage_offset()))
        return torch.equal(now.view(torch.int32), self.before.view(torch.int32))

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))

    def result(self):
        return self.view.detach().cpu().clone()


# ---- layers -----------------------------------------------------------------------------------------------------------------
def _cheby(i, o):
    from models.cheby import ChebyKANLayer
    return ChebyKANLayer(i, o, 4)


def _kanlinear():
    from models.effkan import KANLinear
    return KANLinear(64, 64)


def _fastkan():
    from tests.test_layer_forms_gpu import _fastkan as make
    return make(64, 64)


def _sine():
    from models.sinekan import SineKANLayer
    return SineKANLayer(64, 64, grid_size=4)


def _msa_cheby(d, h):
    from attention import MSA
    return MSA(d, h, type="cheby")


ALL_A = ("packed", "pad4", "pad1:ldx", "pad1:ldy", "shift:x", "shift:w", "shift:bias", "shift:y", "shift:dy", "shift:dx",
         "shift:dw", "shift:all")
# id -> (factory, rows, layouts, precisions)
LAYERS = {
    "A": (lambda: _cheby(64, 64), 300, ALL_A, ("fp32", "bf16")),
    "B": (_kanlinear, 300, ("packed", "pad4", "pad1:ldx", "pad1:ldy", "pad1:bp", "shift:all", "shift:bparams"), ("fp32",)),
    "C": (_fastkan, 300, ("packed", "pad4", "pad1:ldu", "shift:u", "shift:du", "shift:all"), ("fp32",)),
    "D": (_sine, 300, ("packed", "pad4", "pad1:bp", "shift:bparams", "shift:all"), ("fp32",)),
    "E": (lambda: _cheby(8, 8), 100, ("packed", "pad1:ldx", "pad1:ldy", "shift:all"), ("fp32",)),
    "E'": (lambda: _msa_cheby(16, 2), 100, ("packed", "pad1:ldx", "pad1:ldy", "shift:all"), ("fp32",)),
    "F": (lambda: _msa_cheby(128, 2), 300, ("packed", "pad4", "pad1:ldx", "pad1:ldy", "shift:x", "shift:dy", "shift:all"), ("fp32", "bf16")),
    "G": (lambda: _cheby(36, 48), 300, ("packed", "pad1:ldy", "shift:all", "nobias"), ("fp32",)),
}
CASES = [(k, p, l) for k, (_, _, layouts, precs) in LAYERS.items() for p in precs for l in layouts]


@functools.lru_cache(maxsize=None)
def problem(key, bf16):
    """Descriptor, packed operands (float32, host) and the float64 references of one layer: built once, shared, never written to."""
    from attention import MSA
    from kanvit import _lib
    make, m, _, _ = LAYERS[key]
    torch.manual_seed(4000 + 17 * ord(key[0]) + len(key))
    mod = make()
    with torch.no_grad():
        if isinstance(mod, MSA):
            layers = list(mod.q_mappings) + list(mod.k_mappings) + list(mod.v_mappings)
            cfg = replace(layers[0].kan_cfg(), groups=3 * mod.n_heads, x_group_mod=mod.n_heads)
            w, bp, bias = type(layers[0]).kan_pack_grouped(layers)
            kan_u, ln = (lambda x_: type(layers[0]).kan_u_grouped(layers, x_, mod.n_heads)), None
        else:
            cfg = mod.kan_cfg()
            w, bp, bias = mod.kan_pack()
            w, bp, bias = w.unsqueeze(0), None if bp is None else bp.reshape(1, -1), None if bias is None else bias.reshape(1, -1)
            kan_u, ln = mod.kan_u, mod.kan_ln()
        if bf16:
            cfg = replace(cfg, flags=cfg.flags | _lib.FLAG_BF16_MFMA)
        x = torch.randn(m, cfg.x_group_mod * cfg.I)
        u = kan_u(x)
        if bias is None:
            bias = 0.5 * torch.randn(cfg.groups, cfg.O)
        dy = torch.randn(m, cfg.groups * cfg.O)
        ops_ = {"x": x, "u": u, "w": w.contiguous().float(), "bparams": None if bp is None else bp.contiguous().float(),
                "bias": bias.contiguous().float(), "dy": dy}
        if ln is not None:                         # FastKAN: (gamma, beta, eps) of the LayerNorm that produced u, for the fused route
            ops_["ln"] = (ln.weight.detach().clone(), ln.bias.detach().clone(), ln.eps)
    refs = {}
    for nb in (True, False):                       # with the bias, and for the `nobias` layout without
        b_ = ops_["bias"] if nb else None
        refs[nb] = {"exact": ref.reference(cfg, x, u, ops_["w"], ops_["bparams"], b_, dy)}
        if bf16:
            refs[nb]["rounded"] = ref.reference(cfg, x, u, ops_["w"], ops_["bparams"], b_, dy, rounded=True)
    return cfg, m, ops_, refs


def _layout(cfg, ops_, layout):
    """(ld dict, shift dict, bias or None) of a layout name"""
    ld = {"ldx": cfg.x_group_mod * cfg.I, "ldu": cfg.groups * cfg.I, "ldy": cfg.groups * cfg.O,
          "bp": 0 if ops_["bparams"] is None else ops_["bparams"].shape[1]}
    names = ("x", "u", "w", "bparams", "bias", "y", "dy", "dx", "du", "dw", "dparam")
    shift = dict.fromkeys(names, 0)
    kind, _, arg = layout.partition(":")
    if kind == "pad4":
        ld = {k: v + 4 if v else 0 for k, v in ld.items()}
    elif kind == "pad1":
        assert ld[arg], (layout, "no such operand in this layer")
        ld[arg] += 1
    elif kind == "shift" and arg == "all":
        ld = {k: v + 1 if v else 0 for k, v in ld.items()}
        shift = dict.fromkeys(names, 1)
    elif kind == "shift":
        assert arg in shift, layout
        shift[arg] = 1
    else:
        assert kind in ("packed", "nobias"), layout
    return ld, shift, kind != "nobias"


def _desc(cfg, m, ld):
    from kanvit import ops
    return ops._desc(cfg, m, ld["ldx"], ld["ldu"], ld["ldy"], ld["bp"])


def _workspace(nbytes, shift_bytes=0):
    """(tensor kept alive, pointer, size): a 16-byte aligned workspace, or one `shift_bytes` off"""
    if not nbytes:
        return None, None, 0
    t = torch.empty(nbytes // 4 + 8, device=DEV, dtype=torch.float32)
    assert t.data_ptr() % 16 == 0
    return t, C.c_void_p(t.data_ptr() + shift_bytes), nbytes


def run_entry(entry, cfg, m, ops_, layout, record):
    """One call of one entry point on fresh guarded buffers: {output name: host tensor}, the kan_* kernels it launched (first
    run only).  Asserts the return code, the guards and that the outputs hold no NaN."""
    from kanvit import _lib
    L = _lib.lib()
    ld, sh, with_bias = _layout(cfg, ops_, layout)
    d = _desc(cfg, m, ld)
    G, K = cfg.groups, cfg.K
    has_u, has_bp = ops_["u"] is not None, ops_["bparams"] is not None
    inp = {"x": Operand(m, cfg.x_group_mod * cfg.I, ld["ldx"], sh["x"], ops_["x"])}
    if has_u:
        inp["u"] = Operand(m, G * cfg.I, ld["ldu"], sh["u"], ops_["u"])
    if has_bp:
        inp["bparams"] = Operand(G, ops_["bparams"].shape[1], ld["bp"], sh["bparams"], ops_["bparams"])
    if entry != "bwd_weight":
        inp["w"] = Operand(G * K, cfg.O, cfg.O, sh["w"], ops_["w"])
    if entry == "fwd" and with_bias:
        inp["bias"] = Operand(1, G * cfg.O, G * cfg.O, sh["bias"], ops_["bias"])
    if entry != "fwd":
        inp["dy"] = Operand(m, G * cfg.O, ld["ldy"], sh["dy"], ops_["dy"])
    out = {}
    p = lambda name: (inp.get(name) or out.get(name)).ptr if (name in inp or name in out) else None
    with torch.cuda.device(0):
        if entry == "fwd":
            out["y"] = Operand(m, G * cfg.O, ld["ldy"], sh["y"])
            keep, ws, nb = _workspace(int(L.kanvit_layer_fwd_workspace(C.byref(d))))
            call = lambda: L.kanvit_layer_fwd(C.byref(d), p("x"), p("u"), p("w"), p("bparams"), p("bias"), p("y"), ws, C.c_size_t(nb), None)
        elif entry == "bwd_input":
            out["dx"] = Operand(m, cfg.x_group_mod * cfg.I, ld["ldx"], sh["dx"])
            if cfg.family == ref.RBF:
                out["du"] = Operand(m, G * cfg.I, ld["ldu"], sh["du"])
            if cfg.family == ref.SINE:
                out["dparam"] = Operand(int(L.kanvit_layer_dparam_tiles(C.byref(d))) * G, cfg.G, cfg.G, sh["dparam"])
            keep, ws, nb = _workspace(int(L.kanvit_layer_bwd_input_workspace(C.byref(d))))
            call = lambda: L.kanvit_layer_bwd_input(C.byref(d), p("x"), p("u"), p("w"), p("bparams"), p("dy"), p("dx"), p("du"),
                                                    p("dparam"), ws, C.c_size_t(nb), None)
        else:
            out["dw"] = Operand(G * K, cfg.O, cfg.O, sh["dw"])
            keep, ws, nb = _workspace(int(L.kanvit_layer_bwd_weight_workspace(C.byref(d))))
            call = lambda: L.kanvit_layer_bwd_weight(C.byref(d), p("x"), p("u"), p("bparams"), p("dy"), p("dw"), ws, C.c_size_t(nb), None)
        torch.cuda.synchronize()
        names = set()
        if record:
            with record_kernels() as names:
                rc = call()
        else:
            rc = call()
        torch.cuda.synchronize()
    assert rc == 0, (entry, layout, rc, L.kanvit_last_error().decode())
    for name, o in {**inp, **out}.items():
        assert o.outside_unchanged(), (entry, layout, name, "written outside its view")
    res = {name: o.result() for name, o in out.items()}
    for name, t in res.items():
        assert not torch.isnan(t).any(), (entry, layout, name, "NaN in the result: something outside an input view was read")
    del keep
    return res, {n for n in names if n.startswith("kan_")}


@functools.lru_cache(maxsize=None)
def run_case(key, prec, layout):
    """All three entry points, twice (bitwise repeatable); results and kernel names of the first run."""
    cfg, m, ops_, _ = problem(key, prec == "bf16")
    results, names = {}, {}
    for entry in ENTRIES:
        r1, names[entry] = run_entry(entry, cfg, m, ops_, layout, record=True)
        r2, _ = run_entry(entry, cfg, m, ops_, layout, record=False)
        for k in r1:
            assert torch.equal(r1[k].view(torch.int32), r2[k].view(torch.int32)), (key, prec, layout, entry, k, "not repeatable")
        results.update(r1)
    return results, names


def _errors(cfg, got, want):
    """{output: _Err} of one case against one reference; dparam is summed over its row tiles first (as the caller does)"""
    errs = {}
    for k in ("y", "dx", "du", "dw"):
        if k in got:
            errs[k] = _Err().add(got[k].reshape(want[k].shape), want[k])
    if "dparam" in got:
        errs["dfreq"] = _Err().add(got["dparam"].double().reshape(-1, cfg.groups, cfg.G).sum(0), want["dfreq"])
    return errs


OUTPUTS = {"fwd": ("y",), "bwd_input": ("dx", "du", "dfreq"), "bwd_weight": ("dw",)}
# position of the template argument that says "contracts on the bf16 matrix cores" in the kernels that have an exact twin of the same name
BF_ARG = {"kan_bwd_input_kernel": 3, "kan_bwd_weight_kernel": 2, "kan_bwd_weight_reg_kernel": 3, "kan_bwd_weight_dma_kernel": 3}


def ran_bf16(names):
    """whether a set of recorded kan_* kernels contracted on the bf16 matrix cores: a *_bf16_* kernel, or BF = true of the others"""
    for n in names:
        base, _, args = n.partition("<")
        if "bf16" in base or (base in BF_ARG and args.rstrip(">").split(", ")[BF_ARG[base]] == "true"):
            return True
    return False


def check_entry(what, cfg, entry, got, refs, names):
    """One entry point's outputs against the float64 helper, at the bounds of the kernels that ran (`names`): the exact fp32 kernels
    at FWD / TOL -- also under the bf16 flag, which allows bf16 and does not require it --, the bf16 ones at TIGHT against the
    bf16-operand reference and LOOSE against the unrounded one (and not closer to it than bf16 rounding leaves them)."""
    ee = {k: e for k, e in _errors(cfg, got, refs["exact"]).items() if k in OUTPUTS[entry]}
    assert ee, (what, entry)
    if not ran_bf16(names):
        print(what, entry, "exact", {k: "%.3g" % (e.fwd() if k == "y" else e.maxrel(1e-3)) for k, e in ee.items()})
        for k, e in ee.items():
            if k == "y":
                assert e.fwd() < FWD, (what, k, e.fwd())
            else:
                assert e.maxrel(1e-3) < TOL, (what, k, e.maxrel(1e-3))
        return
    er = _errors(cfg, got, refs["rounded"])
    print(what, entry, "bf16 maxrel", {k: "%.3g" % er[k].maxrel() for k in ee}, "fro", {k: "%.3g" % e.fro() for k, e in ee.items()})
    for k, e in ee.items():
        assert er[k].maxrel() < TIGHT, (what, k, er[k].maxrel())
        assert 1e-5 < e.fro() < LOOSE, (what, k, e.fro())


def check_numbers(key, prec, layout, got, names):
    cfg, _, _, refs = problem(key, prec == "bf16")
    for entry in ENTRIES:
        check_entry((key, prec, layout), cfg, entry, got, refs[layout != "nobias"], names[entry])
    if prec == "bf16" and layout in ("packed", "pad4"):
        assert all(ran_bf16(names[e]) for e in ENTRIES), (key, layout, "an aligned call under the bf16 flag ran exact kernels")


# ---- the kan_* kernels every (layer, precision, entry point) launches, by layout: recorded on the MI355X ---------------------
# FORMS[(layer, precision)][entry] = [(kernel names, layouts that launch exactly them), ...]
FORMS = {
    ("A", "fp32"): {
        "fwd": [
            ({"kan_fwd_reg_kernel<1, 1, 1, 4, 5, false>"},
             ("packed", "pad4", "shift:dy", "shift:dx", "shift:dw",)),
            ({"kan_fwd_reg_kernel<1, 1, 1, 2, 0, false>"},
             ("pad1:ldx", "shift:x",)),
            ({"kan_fwd_kernel<1, 2, 1, false>"},
             ("pad1:ldy", "shift:w", "shift:bias", "shift:y", "shift:all",)),
        ],
        "bwd_input": [
            ({"kan_bwd_input_reg_kernel<1, 5, 5, false>"},
             ("packed", "pad4", "shift:bias", "shift:y", "shift:dw",)),
            ({"kan_bwd_input_kernel<1, 3, false, false>"},
             ("pad1:ldx", "pad1:ldy", "shift:x", "shift:w", "shift:dy", "shift:dx", "shift:all",)),
        ],
        "bwd_weight": [
            ({"kan_bwd_weight_reg_kernel<1, 5, 1, false, 5, false>", "kan_slab_reduce_kernel"},
             ("packed", "pad4", "pad1:ldx", "pad1:ldy", "shift:x", "shift:w", "shift:bias", "shift:y", "shift:dy", "shift:dx", "shift:dw", "shift:all",)),
        ],
    },
    ("A", "bf16"): {
        "fwd": [
            ({"kan_fwd_reg_bf16_kernel<1, 5, 2, 1, 8, false>", "kan_pack_w_fwd_reg_kernel"},
             ("packed", "pad4", "shift:w", "shift:dy", "shift:dx", "shift:dw",)),
            ({"kan_fwd_bf16_kernel<1, 2, 1>", "kan_pack_w_fwd_kernel"},
             ("pad1:ldx", "shift:x",)),
            ({"kan_fwd_kernel<1, 2, 1, false>"},
             ("pad1:ldy", "shift:bias", "shift:y", "shift:all",)),
        ],
        "bwd_input": [
            ({"kan_bwd_input_res_bf16_kernel<1, 5, 5, 1, false>", "kan_pack_w_bwd_reg_kernel"},
             ("packed", "pad4", "shift:w", "shift:bias", "shift:y", "shift:dw",)),
            ({"kan_bwd_input_kernel<1, 3, false, true>", "kan_pack_w_bwd_kernel"},
             ("pad1:ldx", "shift:x", "shift:dx",)),
            ({"kan_bwd_input_kernel<1, 3, false, false>"},
             ("pad1:ldy", "shift:dy", "shift:all",)),
        ],
        "bwd_weight": [
            ({"kan_bwd_weight_reg_kernel<1, 5, 1, true, 5, false>", "kan_slab_reduce_kernel"},
             ("packed", "pad4", "pad1:ldx", "pad1:ldy", "shift:x", "shift:w", "shift:bias", "shift:y", "shift:dy", "shift:dx", "shift:dw", "shift:all",)),
        ],
    },
    ("B", "fp32"): {
        "fwd": [
            ({"kan_fwd_reg_kernel<2, 1, 1, 4, 9, false>"},
             ("packed", "pad4", "pad1:bp", "shift:bparams",)),
            ({"kan_fwd_reg_kernel<2, 1, 1, 2, 9, false>"},
             ("pad1:ldx",)),
            ({"kan_fwd_kernel<2, 2, 1, false>"},
             ("pad1:ldy", "shift:all",)),
        ],
        "bwd_input": [
            ({"kan_bwd_input_reg_kernel<2, 9, 5, false>"},
             ("packed", "pad4", "pad1:bp", "shift:bparams",)),
            ({"kan_bwd_input_kernel<2, 3, false, false>"},
             ("pad1:ldx", "pad1:ldy", "shift:all",)),
        ],
        "bwd_weight": [
            ({"kan_bwd_weight_reg16_kernel<2, 9, 3, 4>", "kan_slab_reduce_kernel"},
             ("packed", "pad4", "pad1:ldx", "pad1:ldy", "pad1:bp", "shift:all", "shift:bparams",)),
        ],
    },
    ("C", "fp32"): {
        "fwd": [
            ({"kan_fwd_reg_kernel<3, 1, 1, 4, 9, false>"},
             ("packed", "pad4", "shift:du",)),
            ({"kan_fwd_reg_kernel<3, 1, 1, 2, 9, false>"},
             ("pad1:ldu", "shift:u",)),
            ({"kan_fwd_kernel<3, 2, 1, false>"},
             ("shift:all",)),
        ],
        "bwd_input": [
            ({"kan_bwd_input_reg_kernel<3, 9, 5, false>"},
             ("packed", "pad4", "pad1:ldu", "shift:u", "shift:du",)),
            ({"kan_bwd_input_kernel<3, 3, false, false>"},
             ("shift:all",)),
        ],
        "bwd_weight": [
            ({"kan_bwd_weight_reg16_kernel<3, 9, 9, 4>", "kan_slab_reduce_kernel"},
             ("packed", "pad4", "pad1:ldu", "shift:u", "shift:du", "shift:all",)),
        ],
    },
    ("D", "fp32"): {
        "fwd": [
            ({"kan_fwd_reg_kernel<4, 1, 1, 4, 4, false>"},
             ("packed", "pad4",)),
            ({"kan_fwd_kernel<4, 2, 1, true>"},
             ("pad1:bp", "shift:bparams",)),
            ({"kan_fwd_kernel<4, 2, 1, false>"},
             ("shift:all",)),
        ],
        "bwd_input": [
            ({"kan_bwd_input_reg_kernel<4, 4, 4, false>"},
             ("packed", "pad4", "pad1:bp", "shift:bparams",)),
            ({"kan_bwd_input_kernel<4, 3, false, false>"},
             ("shift:all",)),
        ],
        "bwd_weight": [
            ({"kan_bwd_weight_reg_kernel<4, 4, 2, false, 4, false>", "kan_slab_reduce_kernel"},
             ("packed", "pad4", "pad1:bp", "shift:bparams", "shift:all",)),
        ],
    },
    ("E", "fp32"): {
        "fwd": [
            ({"kan_tiny_fwd_kernel<1, 8>"},
             ("packed", "pad1:ldx", "pad1:ldy", "shift:all",)),
        ],
        "bwd_input": [
            ({"kan_tiny_bwd_input_kernel<1, 8, 8>"},
             ("packed", "pad1:ldx", "pad1:ldy", "shift:all",)),
        ],
        "bwd_weight": [
            ({"kan_tiny_bwd_weight_kernel<1, 8>"},
             ("packed", "pad1:ldx", "pad1:ldy", "shift:all",)),
        ],
    },
    ("E'", "fp32"): {
        "fwd": [
            ({"kan_tiny_fwd_kernel<1, 8>"},
             ("packed", "pad1:ldx", "pad1:ldy", "shift:all",)),
        ],
        "bwd_input": [
            ({"kan_tiny_bwd_input_kernel<1, 8, 8>"},
             ("packed", "pad1:ldx", "pad1:ldy", "shift:all",)),
        ],
        "bwd_weight": [
            ({"kan_tiny_bwd_weight_kernel<1, 8>"},
             ("packed", "pad1:ldx", "pad1:ldy", "shift:all",)),
        ],
    },
    ("F", "fp32"): {
        "fwd": [
            ({"kan_fwd_reg_kernel<1, 1, 1, 4, 5, false>"},
             ("packed", "pad4", "shift:dy",)),
            ({"kan_fwd_reg_kernel<1, 1, 1, 2, 0, false>"},
             ("pad1:ldx", "shift:x",)),
            ({"kan_fwd_kernel<1, 2, 3, false>"},
             ("pad1:ldy", "shift:all",)),
        ],
        "bwd_input": [
            ({"kan_bwd_input_reg_kernel<1, 5, 5, true>"},
             ("packed", "pad4",)),
            ({"kan_bwd_input_kernel<1, 3, true, false>"},
             ("pad1:ldx", "pad1:ldy", "shift:x", "shift:dy", "shift:all",)),
        ],
        "bwd_weight": [
            ({"kan_bwd_weight_reg_kernel<1, 5, 1, false, 5, false>", "kan_slab_reduce_kernel"},
             ("packed", "pad4", "pad1:ldx", "pad1:ldy", "shift:x", "shift:dy", "shift:all",)),
        ],
    },
    ("F", "bf16"): {
        "fwd": [
            ({"kan_fwd_reg_bf16_kernel<1, 5, 2, 3, 8, false>", "kan_pack_w_fwd_reg_kernel"},
             ("packed", "pad4", "shift:dy",)),
            ({"kan_fwd_bf16_kernel<1, 2, 3>", "kan_pack_w_fwd_kernel"},
             ("pad1:ldx", "shift:x",)),
            ({"kan_fwd_kernel<1, 2, 3, false>"},
             ("pad1:ldy", "shift:all",)),
        ],
        "bwd_input": [
            ({"kan_bwd_input_res_bf16_kernel<1, 5, 5, 3, true>", "kan_pack_w_bwd_reg_kernel"},
             ("packed", "pad4",)),
            ({"kan_bwd_input_kernel<1, 3, true, true>", "kan_pack_w_bwd_kernel"},
             ("pad1:ldx", "shift:x",)),
            ({"kan_bwd_input_kernel<1, 3, true, false>"},
             ("pad1:ldy", "shift:dy", "shift:all",)),
        ],
        "bwd_weight": [
            ({"kan_bwd_weight_reg_kernel<1, 5, 1, true, 5, false>", "kan_slab_reduce_kernel"},
             ("packed", "pad4", "pad1:ldx", "pad1:ldy", "shift:x", "shift:dy", "shift:all",)),
        ],
    },
    ("G", "fp32"): {
        "fwd": [
            ({"kan_fwd_kernel<1, 2, 1, false>"},
             ("packed", "pad1:ldy", "shift:all", "nobias",)),
        ],
        "bwd_input": [
            ({"kan_bwd_input_kernel<1, 3, false, false>"},
             ("packed", "pad1:ldy", "shift:all", "nobias",)),
        ],
        "bwd_weight": [
            ({"kan_bwd_weight_kernel<1, 1, false>", "kan_slab_reduce_kernel"},
             ("packed", "pad1:ldy", "shift:all", "nobias",)),
        ],
    },
}


def expected_names(key, prec, entry, layout):
    for names, layouts in FORMS[(key, prec)][entry]:
        if layout in layouts:
            return names
    raise KeyError((key, prec, entry, layout))


@pytest.mark.parametrize("key,prec,layout", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_layer_entry_points_on_guarded_strided_operands(key, prec, layout):
    got, names = run_case(key, prec, layout)
    print("\n", key, prec, layout, {e: sorted(n) for e, n in names.items()})
    check_numbers(key, prec, layout, got, names)
    if layout not in ("packed", "nobias"):
        pgot, pnames = run_case(key, prec, "packed")
        outs = {**OUTPUTS, "bwd_input": ("dx", "du", "dparam")}
        for entry in ENTRIES:
            if layout == "pad4":
                assert names[entry] == pnames[entry], (key, prec, entry, "pad4 took other kernels than packed", sorted(names[entry] ^ pnames[entry]))
            if names[entry] == pnames[entry]:
                for k in outs[entry]:
                    if k in got:
                        assert torch.equal(got[k].view(torch.int32), pgot[k].view(torch.int32)), (key, prec, layout, k, "same kernels as packed, other bits")
    for entry in ENTRIES:
        want = expected_names(key, prec, entry, layout)
        assert names[entry] == want, (key, prec, layout, entry, sorted(names[entry] ^ want))


# ---- the LDS-DMA weight gradient and what it falls back to ------------------------------------------------------------------------
# At 300 rows plan_bwd_weight_reg gives a ChebyKAN launch one column tile per wave and the LDS-DMA form (three tiles) is never
# planned.  KANVIT_BW_DMA_FORCE (the parity switch of tests/test_layers_gpu.py) keeps three tiles and lifts the fill test, so F's
# packed / pad4 calls take the DMA kernel, whose 16-byte pieces need x and dy on the 16-byte grid (kan_layer.hip: al.x | al.dy) and
# ldx, ldy % 4 == 0 (plan_bwd_weight_reg); every other layout must fall back to the register ring, which reads one float at a time.
DMA_LAYOUTS = LAYERS["F"][2]
DMA_FORMS = {
    "fp32": [({"kan_bwd_weight_dma_kernel<1, 5, 3, false>", "kan_slab_reduce_kernel"}, ("packed", "pad4")),
             ({"kan_bwd_weight_reg_kernel<1, 5, 3, false, 5, false>", "kan_slab_reduce_kernel"},
              ("pad1:ldx", "pad1:ldy", "shift:x", "shift:dy", "shift:all"))],
    "bf16": [({"kan_bwd_weight_dma_kernel<1, 5, 3, true>", "kan_slab_reduce_kernel"}, ("packed", "pad4")),
             ({"kan_bwd_weight_reg_kernel<1, 5, 3, true, 5, false>", "kan_slab_reduce_kernel"},
              ("pad1:ldx", "pad1:ldy", "shift:x", "shift:dy", "shift:all"))],
}


def run_dma_leg(prec, layout):
    """F's weight gradient under KANVIT_BW_DMA_FORCE=1, twice: (dw, kernel names)"""
    import os
    from kanvit import _lib
    cfg, m, ops_, _ = problem("F", prec == "bf16")
    old = os.environ.get("KANVIT_BW_DMA_FORCE")
    os.environ["KANVIT_BW_DMA_FORCE"] = "1"
    os.environ.pop("KANVIT_BW_NO_DMA", None)
    try:
        assert "bw_dma_force=1" in _lib.reload_config()
        r1, names = run_entry("bwd_weight", cfg, m, ops_, layout, record=True)
        r2, _ = run_entry("bwd_weight", cfg, m, ops_, layout, record=False)
    finally:
        if old is None:
            os.environ.pop("KANVIT_BW_DMA_FORCE", None)
        else:
            os.environ["KANVIT_BW_DMA_FORCE"] = old
        _lib.reload_config()
    assert torch.equal(r1["dw"].view(torch.int32), r2["dw"].view(torch.int32)), (prec, layout, "not repeatable")
    return r1, names


@pytest.mark.parametrize("layout", DMA_LAYOUTS)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_lds_dma_weight_gradient_and_its_fallbacks(prec, layout):
    cfg, _, _, refs = problem("F", prec == "bf16")
    got, names = run_dma_leg(prec, layout)
    print("\n", "F dma", prec, layout, sorted(names))
    check_entry(("F dma", prec, layout), cfg, "bwd_weight", got, refs[True], names)
    want = next(n for n, layouts in DMA_FORMS[prec] if layout in layouts)
    assert names == want, (prec, layout, sorted(names ^ want))
    if layout == "pad4":
        assert torch.equal(got["dw"].view(torch.int32), run_dma_leg(prec, "packed")[0]["dw"].view(torch.int32)), (prec, "pad4 is not bitwise packed")


# ---- KANVIT_FLAG_FUSED_LN: register kernels or nothing ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused_ln_problem():
    """Layer C with KANVIT_FLAG_FUSED_LN: the same module's centres, weights, gamma, beta and x; bparams = [centres | gamma | beta],
    the u slot carries the statistics.  The float64 reference forms u = LayerNorm(x) itself, and (mean, rstd) per row."""
    from kanvit import _lib
    cfg0, m, ops_, _ = problem("C", False)
    gamma, beta, eps = ops_["ln"]
    cfg = replace(cfg0, flags=cfg0.flags | _lib.FLAG_FUSED_LN, ln_eps=eps)
    bp = torch.cat([ops_["bparams"][0], gamma, beta]).reshape(1, -1)
    x64 = ops_["x"].double()
    mean = x64.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x64.var(dim=1, unbiased=False, keepdim=True) + eps)
    u64 = (x64 - mean) * rstd * gamma.double() + beta.double()
    want = ref.reference(cfg0, ops_["x"], u64, ops_["w"], ops_["bparams"], ops_["bias"], ops_["dy"])
    want["stats"] = torch.cat([mean, rstd], dim=1)
    return cfg, m, {**ops_, "bparams": bp, "u": None}, want


def _fused_ln_call(entry, shifted, stats_shift=0, record=False):
    """One FUSED_LN call with the `shifted` operands one float off the 16-byte grid and the statistics buffer `stats_shift` floats
    off the 8-byte grid: (return code, message, every output buffer untouched, the operands, kan_* kernels when recorded)"""
    from kanvit import _lib
    L = _lib.lib()
    cfg, m, ops_, want = fused_ln_problem()
    ld = {"ldx": cfg.I, "ldu": cfg.I, "ldy": cfg.O, "bp": ops_["bparams"].shape[1]}
    d = _desc(cfg, m, ld)
    assert L.kanvit_layer_ln_fusable(C.byref(d)) == 1
    s = lambda n: 1 if n in shifted else 0
    o = {"x": Operand(m, cfg.I, cfg.I, s("x"), ops_["x"]), "w": Operand(cfg.K, cfg.O, cfg.O, 0, ops_["w"]),
         "bparams": Operand(1, ld["bp"], ld["bp"], 0, ops_["bparams"]), "bias": Operand(1, cfg.O, cfg.O, 0, ops_["bias"]),
         "dy": Operand(m, cfg.O, cfg.O, s("dy"), ops_["dy"]),
         # the statistics: written by the forward (an output there), read by the gradients (the row's float64 values, rounded)
         "stats": Operand(m, 2, 2, stats_shift, None if entry == "fwd" else want["stats"].float()),
         "y": Operand(m, cfg.O, cfg.O, s("y")), "dx": Operand(m, cfg.I, cfg.I, s("dx")), "du": Operand(m, cfg.I, cfg.I, 0),
         "dw": Operand(cfg.K, cfg.O, cfg.O, 0)}
    with torch.cuda.device(0):
        if entry == "fwd":
            call = lambda: L.kanvit_layer_fwd(C.byref(d), o["x"].ptr, o["stats"].ptr, o["w"].ptr, o["bparams"].ptr, o["bias"].ptr, o["y"].ptr,
                                              None, C.c_size_t(0), None)
        elif entry == "bwd_input":
            call = lambda: L.kanvit_layer_bwd_input(C.byref(d), o["x"].ptr, o["stats"].ptr, o["w"].ptr, o["bparams"].ptr, o["dy"].ptr, o["dx"].ptr,
                                                    o["du"].ptr, None, None, C.c_size_t(0), None)
        else:
            keep, ws, nb = _workspace(int(L.kanvit_layer_bwd_weight_workspace(C.byref(d))))
            call = lambda: L.kanvit_layer_bwd_weight(C.byref(d), o["x"].ptr, o["stats"].ptr, o["bparams"].ptr, o["dy"].ptr, o["dw"].ptr, ws,
                                                     C.c_size_t(nb), None)
        torch.cuda.synchronize()
        names = set()
        if record:
            with record_kernels() as names:
                rc = call()
        else:
            rc = call()
        torch.cuda.synchronize()
    msg = L.kanvit_last_error().decode()
    outs = ["y", "dx", "du", "dw"] + (["stats"] if entry == "fwd" else [])
    return rc, msg, all(o[k].untouched() for k in outs), o, {n for n in names if n.startswith("kan_")}


# what the fused route serves: (entry point, operands off the 16-byte grid) -> the kan_* kernels it launches
FUSED_LN_SERVED = {
    ("fwd", ()): {"kan_fwd_reg_kernel<3, 1, 1, 4, 9, false>"},
    ("fwd", ("x",)): {"kan_fwd_reg_kernel<3, 1, 1, 2, 9, false>"},          # plan_fwd_reg steps down to two single-float x loads per lane
    ("bwd_input", ()): {"kan_bwd_input_reg_kernel<3, 9, 5, false>"},
    ("bwd_weight", ()): {"kan_bwd_weight_reg16_kernel<3, 9, 9, 4>", "kan_slab_reduce_kernel"},
    ("bwd_weight", ("x",)): {"kan_bwd_weight_reg16_kernel<3, 9, 9, 4>", "kan_slab_reduce_kernel"},      # reads x and dY one float at a time
    ("bwd_weight", ("dy",)): {"kan_bwd_weight_reg16_kernel<3, 9, 9, 4>", "kan_slab_reduce_kernel"},
    ("bwd_weight", ("x", "dy")): {"kan_bwd_weight_reg16_kernel<3, 9, 9, 4>", "kan_slab_reduce_kernel"},
}


@pytest.mark.parametrize("entry,shifted", list(FUSED_LN_SERVED), ids=["%s-%s" % (e, "+".join(sh) or "aligned") for e, sh in FUSED_LN_SERVED])
def test_fused_ln_served_calls(entry, shifted):
    """The FUSED_LN calls the plans accept -- aligned, and the misaligned ones a register kernel takes as they are: results against
    the float64 helper with u = LayerNorm(x) formed in float64, the written statistics against (mean, rstd), guards, kernel names,
    bitwise repeatable, and the misaligned weight gradient bitwise the aligned one (same kernel, same order of the sums)."""
    cfg, m, _, want = fused_ln_problem()
    rc, msg, _, o, names = _fused_ln_call(entry, shifted, record=True)
    assert rc == 0, (entry, shifted, rc, msg)
    rc2, _, _, o2, _ = _fused_ln_call(entry, shifted)
    assert rc2 == 0
    written = {"fwd": ("y", "stats"), "bwd_input": ("dx", "du"), "bwd_weight": ("dw",)}[entry]
    for k, op in o.items():
        assert op.outside_unchanged(), (entry, shifted, k, "written outside its view")
        if k in ("y", "dx", "du", "dw", "stats") and k not in written:
            assert op.untouched(), (entry, shifted, k, "an output of another entry point was written")
    got = {k: o[k].result() for k in written}
    for k in written:
        assert not torch.isnan(got[k]).any(), (entry, shifted, k)
        assert torch.equal(got[k].view(torch.int32), o2[k].result().view(torch.int32)), (entry, shifted, k, "not repeatable")
    print("\n", "fused-ln", entry, shifted, sorted(names))
    check_entry(("fused-ln", entry, shifted), cfg, entry, {k: v for k, v in got.items() if k != "stats"}, {"exact": want}, names)
    if entry == "fwd":
        # two-pass fp32 mean / variance over 64 features: rounding of a few 2^-24 of the largest entry, far inside the gradient bound
        e = _Err().add(got["stats"], want["stats"])
        assert e.maxrel(1e-3) < TOL, (entry, shifted, "stats", e.maxrel(1e-3))
    assert names == FUSED_LN_SERVED[(entry, shifted)], (entry, shifted, sorted(names ^ FUSED_LN_SERVED[(entry, shifted)]))
    if entry == "bwd_weight" and shifted:
        base = _fused_ln_call(entry, ())[3]["dw"].result()
        assert torch.equal(got["dw"].view(torch.int32), base.view(torch.int32)), (entry, shifted, "same kernel as aligned, other bits")


@pytest.mark.parametrize("entry,operand", [("fwd", "y"), ("bwd_input", "x"), ("bwd_input", "dy"), ("bwd_input", "dx")])
def test_fused_ln_refuses_a_misaligned_operand(entry, operand):
    """where no register kernel takes the operand as it is (the forward's float4 y rows, the input gradient's 16-byte x / dx / dy rows)"""
    rc, msg, untouched, _, _ = _fused_ln_call(entry, (operand,))
    assert rc == EINVAL and "alignment" in msg, (entry, operand, rc, msg)
    assert untouched, (entry, operand, "an output buffer was written by a refused call")


@pytest.mark.parametrize("entry", ENTRIES)
def test_fused_ln_refuses_a_misaligned_statistics_buffer(entry):
    rc, msg, untouched, _, _ = _fused_ln_call(entry, (), stats_shift=1)
    assert rc == EINVAL and "statistics" in msg, (entry, rc, msg)
    assert untouched, (entry, "an output buffer was written by a refused call")


@pytest.mark.parametrize("entry", ["fwd", "bwd_input"])
def test_bf16_refuses_a_misaligned_workspace(entry):
    from kanvit import _lib
    L = _lib.lib()
    cfg, m, ops_, _ = problem("A", True)
    ld, _, _ = _layout(cfg, ops_, "packed")
    d = _desc(cfg, m, ld)
    x = Operand(m, cfg.I, cfg.I, 0, ops_["x"])
    w = Operand(cfg.K, cfg.O, cfg.O, 0, ops_["w"])
    bias = Operand(1, cfg.O, cfg.O, 0, ops_["bias"])
    dy = Operand(m, cfg.O, cfg.O, 0, ops_["dy"])
    y, dx = Operand(m, cfg.O, cfg.O, 0), Operand(m, cfg.I, cfg.I, 0)
    with torch.cuda.device(0):
        if entry == "fwd":
            nbytes = int(L.kanvit_layer_fwd_workspace(C.byref(d)))
            assert nbytes > 0
            keep, ws, nb = _workspace(nbytes, shift_bytes=4)
            rc = L.kanvit_layer_fwd(C.byref(d), x.ptr, None, w.ptr, None, bias.ptr, y.ptr, ws, C.c_size_t(nb), None)
        else:
            nbytes = int(L.kanvit_layer_bwd_input_workspace(C.byref(d)))
            assert nbytes > 0
            keep, ws, nb = _workspace(nbytes, shift_bytes=4)
            rc = L.kanvit_layer_bwd_input(C.byref(d), x.ptr, None, w.ptr, None, dy.ptr, dx.ptr, None, None, ws, C.c_size_t(nb), None)
        torch.cuda.synchronize()
    msg = L.kanvit_last_error().decode()
    assert rc == ENOMEM and "16-byte" in msg, (entry, rc, msg)
    assert y.untouched() and dx.untouched(), (entry, "an output buffer was written by a refused call")
