"""CPU-only checks of the fused B-spline refit behind KANLinear.update_grid (kanvit_bspline_refit_*, csrc/kan_bspline_refit.hip):
the exports, the pure host functions (supported descriptors, workspace sizes), the refusals by name, the code-object resources
of the new kernels, train.py's flag default, and the float64 restatement of update_grid (tests/_update_grid_ref.py) against the
reference's own results (tests/golden/update_grid.npz) -- the restatement the GPU tests use on shapes without goldens."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from tests import _update_grid_ref as ug
from tests._util import T, bf16_bits_to_f32, load_npz, state_dict_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REFIT_SYMBOLS = {"kanvit_bspline_refit_supported", "kanvit_bspline_refit_workspace", "kanvit_bspline_refit_gram",
                 "kanvit_bspline_refit_solve"}


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def desc(**kw):
    """The grouped refit of a ViT-B block's per-head KANLinear q|k|v layers: 12 heads x 3, 64 -> 64, grid 5, order 3."""
    from kanvit import _lib
    base = dict(family=_lib.BSPLINE, groups=36, x_group_mod=12, I=64, O=64, G=8, spline_order=3, has_base=0, rbf_inv_h=0.0,
                flags=_lib.FLAG_UNIFORM_KNOTS, M=25216, ldx=768, ldu=0, ldy=36 * 64, bparam_stride=64 * 12, ln_eps=0.0, base_act=0)
    base.update(kw)
    return _lib.LayerDesc(**base)


def test_exports_equal_the_headers_set(lib):
    from kanvit import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kanvit.h")).read(), flags=re.S)
    declared = {n for n in re.findall(r"\b(kanvit_[a-z0-9_]+)\s*\(", header) if "refit" in n}
    assert declared == REFIT_SYMBOLS
    assert {n for n in _lib.SYMBOLS if "refit" in n} == REFIT_SYMBOLS
    for name in REFIT_SYMBOLS:
        assert hasattr(raw, name), name
    assert lib.kanvit_abi_version() == 7
    from kanvit import ops
    assert callable(ops.bspline_refit)


def test_supported_and_workspace_are_host_functions_of_the_descriptor(lib):
    from kanvit import _lib
    ok = lambda d: lib.kanvit_bspline_refit_supported(C.byref(d))
    ws = lambda d: lib.kanvit_bspline_refit_workspace(C.byref(d))
    assert ok(desc()) == 1
    assert ok(desc(flags=0)) == 1                                              # non-uniform old knots: Cox-de Boor for both bases
    assert ok(desc(spline_order=2, G=10, bparam_stride=64 * 13, flags=0)) == 1  # grid 8, order 2
    assert ok(desc(spline_order=1, G=9, bparam_stride=64 * 11, flags=0)) == 1
    assert ok(desc(G=24, bparam_stride=64 * 28, flags=0)) == 1
    assert ok(desc(G=25, bparam_stride=64 * 29, flags=0)) == 0                 # more basis functions than the kernels hold in registers
    assert ok(desc(has_base=1)) == 0                                           # the spline weights alone
    assert ok(desc(flags=_lib.FLAG_BF16_MFMA | _lib.FLAG_UNIFORM_KNOTS)) == 0
    assert ok(desc(ldx=700)) == 0
    assert lib.kanvit_bspline_refit_supported(None) == 0
    for fam in (_lib.LINEAR, _lib.CHEBY, _lib.RBF, _lib.SINE, _lib.FOURIER):
        assert ok(desc(family=fam, flags=0)) == 0 and ws(desc(family=fam, flags=0)) == 0
    # workspace = row bands x (the N slab of every x slice + the C slab of every group), fp32; the bands are the edge-L1 statistic's
    for kw in (dict(), dict(M=1100, groups=1, x_group_mod=1, I=17, O=5, ldx=23, bparam_stride=17 * 12), dict(M=1), dict(M=257),
               dict(M=400, groups=1, x_group_mod=1, I=5, O=70, G=15, ldx=5, bparam_stride=5 * 19, flags=0)):
        d = desc(**kw)
        bands = lib.kanvit_edge_l1_row_bands(C.byref(d))
        assert bands >= 1
        assert ws(d) == bands * 4 * (d.x_group_mod + d.groups) * d.I * d.G * d.G, kw
    assert lib.kanvit_edge_l1_row_bands(C.byref(desc(M=1100))) >= 3
    assert ws(desc(M=0)) == 0
    assert ws(desc(G=25, bparam_stride=64 * 29, flags=0)) == 0


@pytest.mark.parametrize("call", ["gram", "solve"])
def test_refusals_name_the_family_or_the_limit(lib, call):
    from kanvit import _lib

    def run(d):
        if call == "gram":
            return lib.kanvit_bspline_refit_gram(C.byref(d), None, None, None, None, None, None, 0, None)
        return lib.kanvit_bspline_refit_solve(C.byref(d), None, None, None, None, None, None)

    cases = [(desc(family=_lib.LINEAR, flags=0), b"LINEAR"), (desc(family=_lib.CHEBY, flags=0), b"CHEBY"),
             (desc(family=_lib.RBF, flags=0), b"RBF"), (desc(family=_lib.SINE, flags=0), b"SINE"),
             (desc(family=_lib.FOURIER, flags=0), b"FOURIER"),
             (desc(G=25, bparam_stride=64 * 29, flags=0), b"nb=25"),
             (desc(flags=_lib.FLAG_BF16_MFMA), b"KANVIT_FLAG_BF16_MFMA"),
             (desc(has_base=1), b"has_base")]
    for d, word in cases:
        assert run(d) == -22, word
        assert word in lib.kanvit_last_error(), (word, lib.kanvit_last_error())
    # a supported descriptor with null device pointers is refused before anything is launched
    assert run(desc()) == -22
    assert b"null" in lib.kanvit_last_error()
    if call == "gram":                                     # ... and so is a workspace that is missing or too small
        buf = (C.c_double * 64)()
        p = C.cast(buf, C.c_void_p)
        assert lib.kanvit_bspline_refit_gram(C.byref(desc()), p, p, p, p, p, None, 0, None) == -12
        assert b"workspace" in lib.kanvit_last_error()
        assert lib.kanvit_bspline_refit_gram(C.byref(desc()), p, p, p, p, p, p, 64, None) == -12
        assert lib.kanvit_bspline_refit_gram(C.byref(desc(M=0)), None, None, None, p, p, None, 0, None) == 0      # no rows: nothing to launch


def test_refit_kernels_use_no_scratch_and_spill_no_vgpr(lib):
    pytest.importorskip("msgpack")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    from kanvit import _lib
    ks = {n: k for n, k in kernel_meta.kernels(_lib.LIB_PATH).items() if "refit" in n}
    assert len(ks) >= 4, sorted(ks)                       # the Gram kernel at 8 and 24 slots, the reduce, the solve
    for part in ("refit_gram", "refit_reduce", "refit_solve"):
        assert any(part in n for n in ks), part
    for n, k in ks.items():
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0, (n, k[".vgpr_spill_count"])


def test_train_flag_defaults_to_never():
    import train
    assert train.parse([]).grid_update_every == 0
    assert train.parse(["--grid-update-every", "5"]).grid_update_every == 5


def test_update_grid_has_no_cpu_fallback():
    from kanvit import ops
    from models.effkan import KANLinear
    with pytest.raises(ops.KanvitError):
        KANLinear(4, 3).update_grid(torch.randn(50, 4))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_float64_restatement_against_the_references_goldens(tag):
    """The reference's fp32 lstsq is itself 3e-7 to 7e-7 away from a float64 one; the restatement is held to 1e-5 normwise on the
    weights and 1e-6 (1 + |g|) on the knots."""
    blob = load_npz("update_grid.npz")
    m, i, o, gs, order = (int(v) for v in blob[f"{tag}.cfg"])
    x = bf16_bits_to_f32(blob[f"{tag}.x"])
    sd = state_dict_from(blob, tag + ".")
    assert tuple(x.shape) == (m, i) and tuple(sd["spline_weight"].shape) == (o, i, gs + order)
    knots, weight = ug.refit(x, sd, gs, order)
    ge, we = ug.grid_err(knots, T(blob[f"{tag}.grid_after"])), ug.rel(weight, T(blob[f"{tag}.spline_weight_after"]))
    piv = float(ug.pivot_ratios(x, knots, order).min())
    print(f"{tag}: grid err {ge:.3e} (bound 1e-6), weight err {we:.3e} (bound 1e-5), smallest pivot ratio {piv:.3e}")
    assert ge <= 1e-6, ge
    assert we <= 1e-5, we
    assert piv >= 10 * ug.TAU, piv
    # the reference's own forward before and after the update, against the float64 forward on the same knots and weights
    rows = slice(None, None, 2)
    y0 = ug.forward64(x, sd, sd["grid"], sd["spline_weight"], order)[rows]
    y1 = ug.forward64(x, sd, knots, weight, order)[rows]
    assert ug.rel(y0, T(blob[f"{tag}.y_before"])) <= 1e-5
    assert ug.rel(y1, T(blob[f"{tag}.y_after"])) <= 1e-5
