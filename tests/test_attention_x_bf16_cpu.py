"""CPU checks of the general attention kernels' bf16 mode (csrc/attention_x.hip): kanvit_attn_x_fwd / _bwd accept
KANVIT_FLAG_BF16_MFMA for heads of D <= 64 and refuse it, by name, for wider heads (no silent fp32 fallback); the bf16 twins of
the forward, dK/dV and dQ kernels exist for DT = 1, 2 and compile without scratch or VGPR spills; the Python routing passes the
flag to them only for D <= 64."""
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


def _x_calls(lib, D, flags):
    from kanvit import _lib
    a = _lib.AttnDesc(B=2, H=3, N=300, D=D, scale=0.125, flags=flags)
    e = _lib.AttnExt(Nk=300)
    rc_f = lib.kanvit_attn_x_fwd(ctypes.byref(a), ctypes.byref(e), None, None, None, None, None, None)
    err_f = lib.kanvit_last_error()
    rc_b = lib.kanvit_attn_x_bwd(ctypes.byref(a), ctypes.byref(e), None, None, None, None, None, None, None, None, None, None, 0, None)
    err_b = lib.kanvit_last_error()
    return (rc_f, err_f), (rc_b, err_b)


@pytest.mark.parametrize("D", [2, 16, 40, 64])
def test_general_attention_accepts_the_bf16_flag_up_to_64(lib, D):
    """With null tensors the call fails on the null check, i.e. after the flag passed."""
    from kanvit import _lib
    for rc, err in _x_calls(lib, D, _lib.FLAG_BF16_MFMA):
        assert rc == -22 and b"null" in err and b"BF16" not in err, err


@pytest.mark.parametrize("D", [66, 80, 128])
def test_general_attention_refuses_the_bf16_flag_for_wide_heads(lib, D):
    from kanvit import _lib
    for rc, err in _x_calls(lib, D, _lib.FLAG_BF16_MFMA):
        assert rc == -22 and b"KANVIT_FLAG_BF16_MFMA" in err and b"D=%d" % D in err and b"null" not in err, err
    for rc, err in _x_calls(lib, D, 0):                      # without the flag the same head passes to the null check
        assert rc == -22 and b"null" in err, err


def test_abi_version_unchanged(lib):
    assert lib.kanvit_abi_version() == 7


def test_bf16_twins_use_no_scratch_and_spill_no_vgprs(lib):
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    from kanvit import build
    ks = {km.demangled_short(n): k for n, k in km.kernels(build.LIB).items()}
    for kern in ("attn_x_fwd_bf16_kernel", "attn_x_bwd_kv_bf16_kernel", "attn_x_bwd_q_bf16_kernel"):
        for dt in (1, 2):
            name = f"{kern}<{dt}>"
            assert name in ks, name
            assert ks[name][".private_segment_fixed_size"] == 0 and ks[name][".vgpr_spill_count"] == 0, name
        assert f"{kern}<3>" not in ks and f"{kern}<4>" not in ks        # no bf16 form for D > 64


@pytest.mark.parametrize("flags,D,want", [(1, 64, 1), (1, 2, 1), (1, 66, 0), (1, 128, 0), (0, 64, 0), (0, 128, 0)])
def test_routing_passes_the_flag_only_where_a_twin_exists(flags, D, want):
    from kanvit import ops
    assert ops._attn_x_flags(flags, D) == want
