"""CPU-only checks of the per-edge mean-absolute-activation statistic (kanvit_edge_l1_*, csrc/kan_edge_l1.hip): the exports,
the pure host functions (supported families / flags, row bands, workspace sizes), the refusals by name, the code-object
resources of the new kernels, and that KANLinear.regularization_loss() without x is still the reference's formula."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDGE_SYMBOLS = ("kanvit_edge_l1_supported", "kanvit_edge_l1_row_bands", "kanvit_edge_l1_fwd_workspace", "kanvit_edge_l1_fwd",
                "kanvit_edge_l1_bwd_workspace", "kanvit_edge_l1_bwd")
BAND_M = 1100          # the row count of the multi-band GPU test (tests/test_edge_l1_gpu.py)


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def desc(**kw):
    """The default KANLinear q|k|v launch of a ViT-B block: 12 heads x (q, k, v), 64 -> 64, grid 5, order 3, base column."""
    from kanvit import _lib
    base = dict(family=_lib.BSPLINE, groups=36, x_group_mod=12, I=64, O=64, G=8, spline_order=3, has_base=1, rbf_inv_h=0.0,
                flags=_lib.FLAG_UNIFORM_KNOTS | _lib.FLAG_SHARED_BPARAMS, M=25216, ldx=768, ldu=0, ldy=36 * 64, bparam_stride=64 * 12,
                ln_eps=0.0, base_act=0)
    base.update(kw)
    return _lib.LayerDesc(**base)


def test_every_new_symbol_is_exported(lib):
    from kanvit import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "kanvit.h")).read()
    for name in EDGE_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name
    assert lib.kanvit_abi_version() == 7
    from kanvit import ops
    assert callable(ops.edge_l1) and callable(ops.l1_entropy_loss)


def test_supported_is_a_host_function_of_the_descriptor(lib):
    from kanvit import _lib
    ok = lambda d: lib.kanvit_edge_l1_supported(C.byref(d))
    assert ok(desc()) == 1                                                    # default KANLinear q|k|v
    assert ok(desc(flags=0)) == 1                                             # non-uniform grid: Cox-de Boor path
    assert ok(desc(spline_order=2, G=9, bparam_stride=64 * 12, flags=0)) == 1  # grid 7, order 2
    assert ok(desc(has_base=0)) == 1
    assert ok(desc(base_act=_lib.BASE_GELU)) == 1
    assert ok(desc(family=_lib.CHEBY, G=5, has_base=0, flags=0, bparam_stride=0)) == 1
    assert ok(desc(family=_lib.RBF, G=8, has_base=0, flags=0, rbf_inv_h=1.75, bparam_stride=8)) == 1
    assert ok(desc(family=_lib.SINE, G=4, has_base=0, flags=0, bparam_stride=4 * 65)) == 0
    assert ok(desc(family=_lib.FOURIER, G=4, has_base=0, flags=0)) == 0
    assert ok(desc(family=_lib.LINEAR, G=1, has_base=0, flags=0)) == 0
    assert ok(desc(family=_lib.RBF, G=8, rbf_inv_h=1.75, bparam_stride=8 + 128, flags=_lib.FLAG_FUSED_LN | _lib.FLAG_UNIFORM_KNOTS)) == 0
    assert ok(desc(flags=_lib.FLAG_BF16_MFMA | _lib.FLAG_UNIFORM_KNOTS)) == 0
    assert ok(desc(G=30, bparam_stride=64 * 34)) == 0                         # more generated columns than the kernels hold in registers
    assert lib.kanvit_edge_l1_supported(None) == 0


@pytest.mark.parametrize("call", ["fwd", "bwd"])
def test_refusals_name_the_family_or_flag(lib, call):
    from kanvit import _lib

    def run(d):
        if call == "fwd":
            return lib.kanvit_edge_l1_fwd(C.byref(d), None, None, None, None, None, 0, None)
        return lib.kanvit_edge_l1_bwd(C.byref(d), None, None, None, None, None, None, None, 0, None)

    cases = [(desc(family=_lib.SINE, G=4, has_base=0, flags=0, bparam_stride=4 * 65), b"SINE"),
             (desc(family=_lib.FOURIER, G=4, has_base=0, flags=0), b"FOURIER"),
             (desc(family=_lib.LINEAR, G=1, has_base=0, flags=0), b"LINEAR"),
             (desc(family=_lib.RBF, G=8, rbf_inv_h=1.75, bparam_stride=8 + 128, flags=_lib.FLAG_FUSED_LN), b"KANVIT_FLAG_FUSED_LN"),
             (desc(flags=_lib.FLAG_BF16_MFMA | _lib.FLAG_UNIFORM_KNOTS), b"KANVIT_FLAG_BF16_MFMA")]
    for d, word in cases:
        assert run(d) == -22, word
        assert word in lib.kanvit_last_error(), (word, lib.kanvit_last_error())
    # a supported descriptor with null device pointers is refused before anything is launched
    assert run(desc()) == -22
    assert b"null" in lib.kanvit_last_error()


def test_row_bands_and_workspace_arithmetic(lib):
    from kanvit import _lib
    for kw in (dict(), dict(M=BAND_M, groups=1, x_group_mod=1, I=32, O=32, ldx=32, bparam_stride=32 * 12),
               dict(family=_lib.CHEBY, G=5, has_base=0, flags=0, bparam_stride=0, M=4097), dict(M=1), dict(M=257)):
        d = desc(**kw)
        bands = lib.kanvit_edge_l1_row_bands(C.byref(d))
        gp = d.G + d.has_base if d.family != _lib.CHEBY else d.G
        slab_f = 4 * d.groups * d.I * d.O
        slab_b = slab_f * gp
        assert bands >= 1
        assert lib.kanvit_edge_l1_fwd_workspace(C.byref(d)) == bands * slab_f
        assert lib.kanvit_edge_l1_bwd_workspace(C.byref(d)) == bands * slab_b
        # the split is a function of M alone: a group computes the same whatever else is in the launch
        assert lib.kanvit_edge_l1_row_bands(C.byref(desc(**{**kw, "groups": d.x_group_mod}))) == bands
    assert lib.kanvit_edge_l1_row_bands(C.byref(desc(M=BAND_M))) >= 3
    assert lib.kanvit_edge_l1_row_bands(C.byref(desc(M=1))) == 1
    assert lib.kanvit_edge_l1_row_bands(C.byref(desc(M=0))) == 0
    assert lib.kanvit_edge_l1_fwd_workspace(C.byref(desc(M=0))) == 0
    assert lib.kanvit_edge_l1_row_bands(C.byref(desc(family=_lib.SINE, G=4, has_base=0, flags=0, bparam_stride=4 * 65))) == 0
    # the workspace is bounded: the band count saturates
    assert lib.kanvit_edge_l1_row_bands(C.byref(desc(M=1 << 22))) == lib.kanvit_edge_l1_row_bands(C.byref(desc(M=1 << 23)))


def test_new_kernels_use_no_scratch_and_spill_no_vgpr(lib):
    pytest.importorskip("msgpack")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    from kanvit import _lib
    ks = {n: k for n, k in kernel_meta.kernels(_lib.LIB_PATH).items() if "edge_l1" in n}
    assert len(ks) >= 3, sorted(ks)                       # forward, backward, reduce (each family / size an instantiation)
    assert any("edge_l1_fwd" in n for n in ks) and any("edge_l1_bwd" in n for n in ks) and any("edge_l1_reduce" in n for n in ks)
    for n, k in ks.items():
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0, (n, k[".vgpr_spill_count"])


def test_regularization_loss_without_x_is_the_reference_formula():
    from models.effkan import KANLinear
    torch.manual_seed(3)
    layer = KANLinear(7, 5)
    with torch.no_grad():
        layer.spline_weight.uniform_(-0.5, 0.5)
    for ra, re_ in ((1.0, 1.0), (0.3, 2.0)):
        got = layer.regularization_loss(ra, re_)
        l1 = layer.spline_weight.abs().mean(-1)          # models/effkan.py:258-264
        p = l1 / l1.sum()
        want = ra * l1.sum() - re_ * torch.sum(p * p.log())
        assert torch.equal(got, want)
    assert torch.equal(layer.regularization_loss(), layer.regularization_loss(x=None, include_base=True))


def test_edge_activation_has_no_cpu_fallback():
    from kanvit import ops
    from models.effkan import KANLinear
    layer = KANLinear(4, 3)
    with pytest.raises(ops.KanvitError):
        layer.edge_activation_l1(torch.randn(5, 4))
    with pytest.raises(ops.KanvitError):
        layer.regularization_loss(x=torch.randn(5, 4))


def test_train_flags_default_to_the_plain_step():
    import train
    a = train.parse([])
    assert a.reg_lambda == 0.0 and a.reg_activation == 1.0 and a.reg_entropy == 1.0
    a = train.parse(["--reg-lambda", "0.01", "--reg-entropy", "2"])
    assert a.reg_lambda == 0.01 and a.reg_entropy == 2.0
