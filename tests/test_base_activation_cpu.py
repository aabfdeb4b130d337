"""Base activations of KANLinear / FastKANLayer other than SiLU, on the host: which callables the port recognises, the refusals
(at construction and at the forward after an attribute swap), the descriptor field that carries the code, the library's own
validation of it, and the resources of the *_act_* kernels that evaluate it (tools/kernel_meta.py: no GPU needed)."""
import ctypes as C
import functools
import importlib.util
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from kanvit import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RECOGNISED = [
    (nn.SiLU(), 0), (F.silu, 0),
    (nn.GELU(), 1), (F.gelu, 1), (functools.partial(F.gelu, approximate="none"), 1),
    (nn.GELU(approximate="tanh"), 2), (functools.partial(F.gelu, approximate="tanh"), 2),
    (nn.ReLU(), 3), (F.relu, 3), (torch.relu, 3),
    (nn.Tanh(), 4), (torch.tanh, 4), (F.tanh, 4),
    (nn.Identity(), 5),
]
REFUSED = [nn.ReLU(inplace=True), nn.SiLU(inplace=True), lambda x: x * 2, torch.sigmoid, nn.Sigmoid(), nn.GELU,
           functools.partial(F.gelu, approximate="tanh", inplace=True), nn.LeakyReLU()]


def _case_id(f):
    """A test id that is the same in every process: the repr of a plain function carries its address."""
    return re.sub(r" at 0x[0-9a-f]+>", ">", repr(f)[:40])


@pytest.mark.parametrize("fn,code", RECOGNISED, ids=[_case_id(f) for f, _ in RECOGNISED])
def test_recognised(fn, code):
    assert ops.base_activation_code(fn) == code
    assert _lib.BASE_NAMES[code] in ("silu", "gelu", "gelu-tanh", "relu", "tanh", "identity")


@pytest.mark.parametrize("fn", REFUSED, ids=[_case_id(f) for f in REFUSED])
def test_refused(fn):
    assert ops.base_activation_code(fn) is None
    with pytest.raises(NotImplementedError, match="supported"):
        ops.base_act_of(fn)


def test_construction_accepts_the_supported_set():
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    for cls, code in ((nn.SiLU, 0), (nn.GELU, 1), (nn.ReLU, 3), (nn.Tanh, 4), (nn.Identity, 5)):
        m = KANLinear(5, 3, base_activation=cls)
        assert m.kan_cfg().base_act == code
    for fn, code in ((F.silu, 0), (F.gelu, 1), (functools.partial(F.gelu, approximate="tanh"), 2), (F.relu, 3),
                     (torch.tanh, 4), (nn.Identity(), 5)):
        m = FastKANLayer(5, 3, base_activation=fn)
        assert m.kan_cfg().base_act == code
    # no base path: nothing to evaluate, code 0 whatever the argument
    assert FastKANLayer(5, 3, use_base_update=False, base_activation=torch.sigmoid).kan_cfg().base_act == 0


def test_state_dict_keys_unchanged():
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    assert set(KANLinear(4, 3, base_activation=nn.GELU).state_dict()) == set(KANLinear(4, 3).state_dict())
    assert set(FastKANLayer(4, 3, base_activation=nn.Identity()).state_dict()) == set(FastKANLayer(4, 3).state_dict())


def test_refusal_at_construction_and_after_a_swap():
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    with pytest.raises(NotImplementedError):
        KANLinear(4, 3, base_activation=nn.Sigmoid)
    with pytest.raises(NotImplementedError):
        FastKANLayer(4, 3, base_activation=lambda x: x)
    a, b = KANLinear(4, 3), FastKANLayer(4, 3)
    a.base_activation = nn.ReLU(inplace=True)
    b.base_activation = torch.sigmoid
    x = torch.randn(2, 4)
    with pytest.raises(NotImplementedError):            # refused before any launch (the CPU tensor would be refused later)
        a(x)
    with pytest.raises(NotImplementedError):
        b(x)


def test_descriptor_field_at_the_old_offset():
    d = _lib.LayerDesc
    assert [f for f, _ in d._fields_][-1] == "base_act"
    assert d.base_act.offset == d.ln_eps.offset + 4 == 84            # where `reserved` was
    assert C.sizeof(d) == 88
    assert ops._desc(ops.LayerCfg(family=ops.RBF, I=4, O=4, G=8, has_base=1, base_act=3), 1, 4, 4, 4, 8).base_act == 3


def test_header_defines():
    h = open(os.path.join(ROOT, "include", "kanvit.h")).read()
    names = ["SILU", "GELU", "GELU_TANH", "RELU", "TANH", "IDENTITY"]
    for code, n in enumerate(names):
        assert re.search(rf"#define KANVIT_BASE_{n} {code}\b", h), n
        assert getattr(_lib, f"BASE_{n}") == code
    assert "int32_t base_act;" in h and "int32_t reserved;\n} kanvit_layer_desc;" not in h
    assert re.search(r"#define KANVIT_ABI_VERSION 7\b", h)


def _desc(family, base_act, has_base=1):
    cfg = ops.LayerCfg(family=family, I=4, O=4, G=8 if family == ops.RBF else 5, spline_order=3 if family == ops.BSPLINE else 0,
                       has_base=has_base if family in (ops.BSPLINE, ops.RBF) else 0, base_act=base_act)
    stride = {ops.BSPLINE: 4 * 12, ops.RBF: 8}.get(family, 0)
    return ops._desc(cfg, 16, 4, 4, 4, stride)


@pytest.mark.parametrize("family,code,has_base", [(ops.BSPLINE, -1, 1), (ops.BSPLINE, 6, 1), (ops.RBF, 6, 1), (ops.RBF, -1, 1),
                                                  (ops.BSPLINE, 1, 0), (ops.RBF, 3, 0), (ops.CHEBY, 1, 0), (ops.SINE, 5, 0)])
def test_library_refuses_bad_codes(family, code, has_base):
    lib = _lib.lib()
    d = _desc(family, code, has_base)
    p = C.c_void_p(16)                      # never dereferenced: validation runs first
    rc = lib.kanvit_layer_fwd(C.byref(d), p, None, p, p, None, p, None, 0, None)
    assert rc == -22, rc
    msg = _lib.last_error() if hasattr(_lib, "last_error") else lib.kanvit_last_error().decode()
    assert "activation" in msg, msg
    assert lib.kanvit_layer_ln_fusable(C.byref(d)) == 0


def _meta():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    return {km.demangled_short(n): k for n, k in km.kernels(_lib.LIB_PATH).items()}


# The two *_act_* kernels that spill more than their SiLU kernel, which already spills (the bf16 32-row weight gradients: the
# activation's switch adds live state to a body that is at its register limit), with the bound each is held to:
# (VGPR spills, scratch bytes); DESIGN.md section 4.8c and profiles/r05_base_activation.md give their measured cost.
SPILL_EXCEPTIONS = {"kan_bwd_weight_reg_act_kernel<2, 9, 3, 1, 5, 0>": (61, 248), "kan_bwd_weight_reg_act_kernel<3, 9, 2, 1, 9, 0>": (4, 20)}


def test_act_kernels_resources():
    """Every *_act_* kernel is a BSPLINE (2) / RBF (3) instantiation of a form that exists with SiLU.  Where the SiLU kernel uses no
    scratch, the twin uses none and spills nothing; where it does (the LDS-tile B-spline kernels: the general recursion's local
    arrays; two bf16 weight-gradient kernels), the twin uses no more than it -- except SPILL_EXCEPTIONS, held to their recorded
    bounds.  The resident bf16 input gradient (explicit vmcnt waits: scratch would corrupt its counting) and the other register
    forms of the reference's shapes use none at all."""
    ks = _meta()
    act = {n: k for n, k in ks.items() if "_act_kernel" in n}
    assert len(act) > 50
    for n, k in act.items():
        silu = n.replace("_act_kernel", "_kernel")
        assert silu in ks, n
        assert re.search(r"<([23]),", n), n
        base = ks[silu]
        spill, scratch = k[".vgpr_spill_count"], k[".private_segment_fixed_size"]
        if n.startswith(("kan_bwd_input_res_bf16_act_kernel", "kan_fwd_reg_act_kernel", "kan_bwd_input_reg_act_kernel",
                         "kan_fwd_reg_bf16_act_kernel", "kan_bwd_input_reg_bf16_act_kernel", "kan_tiny_")):
            assert scratch == 0 and spill == 0, (n, spill, scratch)
        elif base[".private_segment_fixed_size"] == 0:
            assert scratch == 0 and spill == 0, (n, spill, scratch)
        elif n in SPILL_EXCEPTIONS:
            assert spill <= SPILL_EXCEPTIONS[n][0] and scratch <= SPILL_EXCEPTIONS[n][1], (n, spill, scratch)
        else:
            assert spill <= base[".vgpr_spill_count"] and scratch <= base[".private_segment_fixed_size"], (n, spill, scratch)
    # the families without a base column have no twin
    assert not [n for n in act if re.search(r"<[0145],", n)]
