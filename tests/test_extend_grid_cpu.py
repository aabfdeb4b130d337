"""CPU-only checks of grid extension (KANLinear.extend_grid; kanvit_bspline_regrid_*, csrc/kan_bspline_refit.hip): the exports, the
pure host functions (supported descriptors, workspace sizes) of the descriptor and old_G, the refusals by name, the code-object
resources of the kernels that serve it, the float64 restatement (tests/_extend_grid_ref.py) against the update_grid one at an
unchanged size, train.py's flag, the missing CPU fallback and the checkpoint rule of KANLinear."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from tests import _extend_grid_ref as eg
from tests import _update_grid_ref as ug

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REGRID_SYMBOLS = {"kanvit_bspline_regrid_supported", "kanvit_bspline_regrid_workspace", "kanvit_bspline_regrid_gram",
                  "kanvit_bspline_regrid_solve"}


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def desc(**kw):
    """The grouped extension of a ViT-B block's per-head KANLinear q|k|v layers to grid 10: 12 heads x 3, 64 -> 64, order 3, G =
    nb_new = 13; bparam_stride is the stride of the OLD knot tables (grid 5: nk_old = 12)."""
    from kanvit import _lib
    base = dict(family=_lib.BSPLINE, groups=36, x_group_mod=12, I=64, O=64, G=13, spline_order=3, has_base=0, rbf_inv_h=0.0,
                flags=_lib.FLAG_UNIFORM_KNOTS, M=25216, ldx=768, ldu=0, ldy=36 * 64, bparam_stride=64 * 12, ln_eps=0.0, base_act=0)
    base.update(kw)
    return _lib.LayerDesc(**base)


def test_exports(lib):
    from kanvit import _lib, ops
    raw = C.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kanvit.h")).read(), flags=re.S)
    declared = {n for n in re.findall(r"\b(kanvit_[a-z0-9_]+)\s*\(", header) if "regrid" in n}
    assert declared == REGRID_SYMBOLS
    assert {n for n in _lib.SYMBOLS if "regrid" in n} == REGRID_SYMBOLS
    for name in REGRID_SYMBOLS:
        assert hasattr(raw, name), name
    assert lib.kanvit_abi_version() == 7
    assert callable(ops.bspline_regrid)


def test_supported_and_workspace_are_host_functions_of_the_descriptor_and_old_g(lib):
    from kanvit import _lib
    ok = lambda d, og: lib.kanvit_bspline_regrid_supported(C.byref(d), og)
    ws = lambda d, og: lib.kanvit_bspline_regrid_workspace(C.byref(d), og)
    assert ok(desc(), 8) == 1
    assert ok(desc(flags=0), 8) == 1                                               # non-uniform old knots
    assert ok(desc(G=8, bparam_stride=64 * 17), 13) == 1                           # coarsening 10 -> 5
    assert ok(desc(G=8), 8) == 1                                                   # the same size is a regrid too
    assert ok(desc(G=24), 8) == 1                                                  # new = 24
    assert ok(desc(G=25), 8) == 0
    assert ok(desc(G=13, bparam_stride=64 * 28, flags=0), 24) == 1                 # old = 24
    assert ok(desc(G=13, bparam_stride=64 * 29, flags=0), 25) == 0
    assert ok(desc(spline_order=2, G=14, bparam_stride=64 * 13, flags=0), 10) == 1  # grid 8 -> 12, order 2
    assert ok(desc(spline_order=1, G=17, bparam_stride=64 * 11, flags=0), 9) == 1   # grid 8 -> 16, order 1
    assert ok(desc(bparam_stride=64 * 12), 13) == 0                                # the stride does not hold the old tables (nk_old = 17)
    assert ok(desc(), 3) == 0                                                      # old side without a grid interval (order 3)
    assert ok(desc(), 0) == 0
    assert ok(desc(has_base=1), 8) == 0
    assert ok(desc(flags=_lib.FLAG_BF16_MFMA | _lib.FLAG_UNIFORM_KNOTS), 8) == 0
    assert ok(desc(ldx=700), 8) == 0
    assert lib.kanvit_bspline_regrid_supported(None, 8) == 0
    for fam in (_lib.LINEAR, _lib.CHEBY, _lib.RBF, _lib.SINE, _lib.FOURIER):
        assert ok(desc(family=fam, flags=0), 8) == 0 and ws(desc(family=fam, flags=0), 8) == 0
    # workspace = row bands x (the square N slab of every x slice + the rectangular C slab of every group), fp32
    for kw, og in ((dict(), 8), (dict(M=1100, groups=1, x_group_mod=1, I=17, O=5, ldx=23, bparam_stride=17 * 12), 8), (dict(M=1), 8),
                   (dict(M=257, G=6), 8), (dict(M=400, groups=1, x_group_mod=1, I=6, O=70, G=23, ldx=6, bparam_stride=6 * 17, flags=0), 13),
                   (dict(M=300, groups=1, x_group_mod=1, I=6, O=7, G=8, ldx=6, bparam_stride=6 * 17, flags=0), 13)):
        d = desc(**kw)
        bands = lib.kanvit_edge_l1_row_bands(C.byref(desc(G=8, M=d.M)))       # a function of M alone, asked of a grid-5 layer
        assert bands >= 1
        assert ws(d, og) == bands * 4 * (d.x_group_mod * d.I * d.G * d.G + d.groups * d.I * d.G * og), (kw, og)
    assert lib.kanvit_edge_l1_row_bands(C.byref(desc(G=8, M=1100))) >= 3
    assert ws(desc(M=0), 8) == 0
    assert ws(desc(G=25), 8) == 0 and ws(desc(bparam_stride=64 * 29), 25) == 0


@pytest.mark.parametrize("call", ["gram", "solve"])
def test_refusals_name_the_family_the_flag_or_the_side_over_the_limit(lib, call):
    from kanvit import _lib

    def run(d, og=8):
        if call == "gram":
            return lib.kanvit_bspline_regrid_gram(C.byref(d), og, None, None, None, None, None, None, 0, None)
        return lib.kanvit_bspline_regrid_solve(C.byref(d), og, None, None, None, None, None, None)

    cases = [(desc(family=_lib.LINEAR, flags=0), 8, b"LINEAR"), (desc(family=_lib.CHEBY, flags=0), 8, b"CHEBY"),
             (desc(family=_lib.RBF, flags=0), 8, b"RBF"), (desc(family=_lib.SINE, flags=0), 8, b"SINE"),
             (desc(family=_lib.FOURIER, flags=0), 8, b"FOURIER"),
             (desc(G=25), 8, b"new nb=25"),
             (desc(bparam_stride=64 * 29), 25, b"old nb=25"),
             (desc(spline_order=20, G=23, bparam_stride=64 * 44, flags=0), 23, b"new G=23"),      # 44 knots on the new side first
             (desc(spline_order=17, G=22, bparam_stride=64 * 42, flags=0), 24, b"old G=24"),      # new side 40 knots, old side 42
             (desc(flags=_lib.FLAG_BF16_MFMA), 8, b"KANVIT_FLAG_BF16_MFMA"),
             (desc(has_base=1), 8, b"has_base")]
    for d, og, word in cases:
        assert run(d, og) == -22, word
        assert word in lib.kanvit_last_error(), (word, lib.kanvit_last_error())
    # a supported descriptor with null device pointers is refused before anything is launched
    assert run(desc()) == -22
    assert b"null" in lib.kanvit_last_error()
    if call == "gram":                                     # ... and so is a workspace that is missing or too small
        buf = (C.c_double * 64)()
        p = C.cast(buf, C.c_void_p)
        assert lib.kanvit_bspline_regrid_gram(C.byref(desc()), 8, p, p, p, p, p, None, 0, None) == -12
        assert b"workspace" in lib.kanvit_last_error()
        assert lib.kanvit_bspline_regrid_gram(C.byref(desc()), 8, p, p, p, p, p, p, 64, None) == -12
        assert lib.kanvit_bspline_regrid_gram(C.byref(desc(M=0)), 8, None, None, None, p, p, None, 0, None) == 0    # no rows: nothing to launch


def test_the_kernels_use_no_scratch_and_spill_no_vgpr(lib):
    """The extension runs in the refit's kernels, generalised to two basis sizes: the Gram kernel once per pair of slot counts
    (old and new side 8 or 24 each), the reduce kernel, the solve kernel."""
    pytest.importorskip("msgpack")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    from kanvit import _lib
    ks = {kernel_meta.demangled_short(n): k for n, k in kernel_meta.kernels(_lib.LIB_PATH).items() if "refit" in n or "regrid" in n}
    for form in ("<8, 8>", "<8, 24>", "<24, 8>", "<24, 24>"):
        assert "kan_bspline_refit_gram_kernel" + form in ks, (form, sorted(ks))
    for part in ("refit_reduce", "refit_solve"):
        assert any(part in n for n in ks), part
    for n, k in ks.items():
        print(f"{n}: vgpr {k['.vgpr_count']} sgpr {k['.sgpr_count']} static lds {k['.group_segment_fixed_size']}")
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0, (n, k[".vgpr_spill_count"])


def _layer(i, o, grid_size, order, seed):
    from models.effkan import KANLinear
    torch.manual_seed(seed)
    layer = KANLinear(i, o, grid_size=grid_size, spline_order=order)
    with torch.no_grad():
        layer.spline_weight.uniform_(-0.5, 0.5)
    return layer


@pytest.mark.parametrize("grid_size, order", [(5, 3), (8, 2)])
def test_restatement_at_an_unchanged_size_is_the_update_grid_restatement(grid_size, order):
    layer = _layer(6, 4, grid_size, order, 40)
    torch.manual_seed(41)
    x = torch.randn(300, 6)
    sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    knots, weight, live, piv, _ = eg.extend(x, sd, grid_size, order, layer.grid_eps)
    ref_knots, ref_weight = ug.refit(x, sd, grid_size, order, layer.grid_eps)
    assert bool(live.all()) and float(piv.min()) >= 10 * eg.TAU
    assert float((knots - ref_knots).abs().max()) <= 1e-12
    assert float((weight - ref_weight).abs().max()) <= 1e-12 * float(ref_weight.abs().max())


def test_restatement_changes_the_shapes_and_falls_back_on_a_constant_column():
    layer = _layer(5, 3, 5, 3, 42)
    torch.manual_seed(43)
    x = torch.randn(200, 5)
    x[:, 1] = 0.25
    sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    knots, weight, live, piv, piv_fb = eg.extend(x, sd, 10, 3)
    assert tuple(knots.shape) == (5, 17) and tuple(weight.shape) == (3, 5, 13)
    assert live.tolist() == [True, False, True, True, True]
    assert float(piv[1]) <= 0.1 * eg.TAU and float(piv_fb.min()) >= 10 * eg.TAU
    assert torch.isfinite(knots).all() and torch.isfinite(weight).all()
    # the fallback feature keeps its function over the old grid's inner span: fitted on evenly spaced samples of [-1, 1]
    assert -1.1 < float(knots[1, 3]) < -0.9 and 0.9 < float(knots[1, -4]) < 1.1


def test_fallback_samples_span_the_old_inner_grid():
    from models.effkan import KANLinear
    layer = _layer(3, 2, 5, 3, 44)
    rows = KANLinear.fallback_samples(layer.grid, 3, 256)
    assert tuple(rows.shape) == (256, 3)
    assert torch.equal(rows[0], layer.grid[:, 3]) and torch.allclose(rows[-1], layer.grid[:, -4], atol=1e-6)
    assert bool((rows[1:] > rows[:-1]).all())


def test_train_flag_defaults_to_never_and_parses_step_size_pairs():
    import train
    assert not train.parse([]).grid_extend
    assert train.parse(["--grid-extend", "3:10,6:20"]).grid_extend == {3: 10, 6: 20}
    assert train.parse(["--grid-extend", "4:8"]).grid_extend == {4: 8}
    for bad in ("3", "3:x", "0:5", "3:10,3:12"):
        with pytest.raises(SystemExit, match="--grid-extend"):
            train.parse(["--grid-extend", bad])


def test_extend_grid_has_no_cpu_fallback():
    from kanvit import ops
    from models.effkan import KANLinear
    with pytest.raises(ops.KanvitError):
        KANLinear(4, 3).extend_grid(torch.randn(50, 4), 10)


def test_a_size_over_the_limit_is_refused_by_name_before_anything_runs():
    from kanvit import ops
    from models.effkan import KANLinear
    layer = KANLinear(4, 3)
    with pytest.raises(ops.KanvitError, match="grid_size \\+ spline_order = 25"):
        layer.extend_grid(torch.randn(50, 4), 22)
    assert layer.grid_size == 5 and tuple(layer.spline_weight.shape) == (3, 4, 8)


def test_checkpoint_of_a_resized_layer_loads_into_a_default_layer():
    from models.effkan import KANLinear
    torch.manual_seed(45)
    layer = KANLinear(4, 3)
    with torch.no_grad():                                  # resized by hand to grid 10: grid [in, 17], spline_weight [out, in, 13]
        layer.resize_grid(10, torch.linspace(-1.6, 1.6, 17).expand(4, -1).contiguous(), torch.randn(3, 4, 13))
    sd = layer.state_dict()
    fresh = KANLinear(4, 3)
    assert fresh.grid_size == 5
    fresh.load_state_dict(sd)
    assert fresh.grid_size == 10 and tuple(fresh.grid.shape) == (4, 17) and tuple(fresh.spline_weight.shape) == (3, 4, 13)
    assert isinstance(fresh.spline_weight, torch.nn.Parameter) and fresh.spline_weight.requires_grad
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[k]), k
    x = torch.rand(7, 4) * 2 - 1
    assert torch.equal(fresh.b_splines(x), layer.b_splines(x)) and fresh.b_splines(x).shape[-1] == 13
    # an inconsistent pair still fails: grid of grid size 10, spline_weight of grid size 12
    bad = dict(sd)
    bad["spline_weight"] = torch.randn(3, 4, 15)
    with pytest.raises(RuntimeError, match="size mismatch"):
        KANLinear(4, 3).load_state_dict(bad)
    bad = dict(sd)                                         # ... and so does another spline order's pair
    with pytest.raises(RuntimeError, match="size mismatch"):
        KANLinear(4, 3, spline_order=2).load_state_dict(bad)
