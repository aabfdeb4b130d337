"""CPU checks of the general attention kernels' wider head domain (64 < D <= 128, csrc/attention_x.hip): the boundary accepts
D up to KANVIT_ATTN_X_MAX_D (even), the one-head-per-work-group ViT kernels still stop at KANVIT_ATTN_MAX_D, the Python routing
sends wide heads to the general kernels, and the new kernel forms compile without scratch or VGPR spills."""
import ctypes
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def _x_calls(lib, D):
    from kanvit import _lib
    a = _lib.AttnDesc(B=2, H=3, N=40, D=D, scale=0.125)
    e = _lib.AttnExt(Nk=50)
    rc_f = lib.kanvit_attn_x_fwd(ctypes.byref(a), ctypes.byref(e), None, None, None, None, None, None)
    err_f = lib.kanvit_last_error()
    rc_b = lib.kanvit_attn_x_bwd(ctypes.byref(a), ctypes.byref(e), None, None, None, None, None, None, None, None, None, None, 0, None)
    err_b = lib.kanvit_last_error()
    return (rc_f, err_f), (rc_b, err_b)


@pytest.mark.parametrize("D", [66, 80, 96, 98, 128])
def test_general_attention_accepts_heads_up_to_128(lib, D):
    """With null tensors the call fails on the null check, i.e. after the head size passed."""
    for rc, err in _x_calls(lib, D):
        assert rc == -22 and b"null" in err and b"D=" not in err, err


@pytest.mark.parametrize("D", [127, 129, 130, 256])
def test_general_attention_refuses_odd_or_wider_heads(lib, D):
    for rc, err in _x_calls(lib, D):
        assert rc == -22 and b"D=%d must be even and <= 128" % D in err, err


def test_vit_attention_kernels_keep_their_64_limit(lib):
    from kanvit import _lib
    assert lib.kanvit_abi_version() == 7
    a = _lib.AttnDesc(B=2, H=3, N=40, D=128, scale=0.125)
    assert lib.kanvit_attn_fwd(ctypes.byref(a), None, None, None, None, None, None) == -22
    assert b"null" not in lib.kanvit_last_error()
    assert lib.kanvit_attn_bwd(ctypes.byref(a), None, None, None, None, None, None, None, None, None, None, 0, None) == -22
    assert b"null" not in lib.kanvit_last_error()


def test_header_bounds():
    src = open(os.path.join(ROOT, "include", "kanvit.h")).read()
    assert "#define KANVIT_ATTN_MAX_D 64" in src and "#define KANVIT_ATTN_X_MAX_D 128" in src


@pytest.mark.parametrize("n,d,fits", [(197, 64, True), (224, 64, True), (225, 64, False), (256, 32, True), (17, 66, False),
                                      (17, 80, False), (197, 128, False), (1, 128, False)])
def test_routing_predicate_sends_wide_heads_to_the_general_kernels(n, d, fits):
    from kanvit import ops
    assert ops._attn_fits_one_workgroup(n, d) is fits


def test_routing_predicate_agrees_with_the_library(lib):
    """ops._attn_fits_one_workgroup is a copy of check_desc's bounds (csrc/attention.hip): it holds exactly where kanvit_attn_fwd
    with null tensors gets as far as its null check instead of refusing the size or the LDS need."""
    from kanvit import _lib, ops
    for D in range(2, 65, 2):
        for N in range(1, 301):
            a = _lib.AttnDesc(B=2, H=3, N=N, D=D, scale=0.125)
            assert lib.kanvit_attn_fwd(ctypes.byref(a), None, None, None, None, None, None) == -22
            assert ops._attn_fits_one_workgroup(N, D) is (b"null q/k/v/o" in lib.kanvit_last_error()), (N, D, lib.kanvit_last_error())


def test_wide_general_kernels_use_no_scratch_and_spill_no_vgprs(lib):
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    from kanvit import build
    ks = {km.demangled_short(n): k for n, k in km.kernels(build.LIB).items()}
    for kern in ("attn_x_fwd_kernel", "attn_x_bwd_kv_kernel", "attn_x_bwd_q_kernel"):
        for dt in (1, 2, 3, 4):
            name = f"{kern}<{dt}>"
            assert name in ks, name
            assert ks[name][".private_segment_fixed_size"] == 0 and ks[name][".vgpr_spill_count"] == 0, name
        for dt in (3, 4):                                    # one wave per SIMD: a 256-thread work-group
            assert ks[f"{kern}<{dt}>"][".max_flat_workgroup_size"] == 256
