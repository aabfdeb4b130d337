"""kanvit_attn_bwd_workspace (host only): the one output of plan_attn_bwd (csrc/attention.hip) that is visible without a GPU.
bytes = ceil16(4 B H N) [rowsum(dO*O)] + e B H NP NP [the dS hand-off], NP = N rounded up to 32 keys, e = 0 where the chosen
backward hands no dS over (causal, head sizes other than 32 / 64, exact D = 64 at N = 193..208 whose default is the one-kernel
16-row backward, KANVIT_ATTN_NO_DS), 4 for the fp32 dS and 2 for the bf16 one.  The literal byte counts below were worked out
from that formula by hand; the test also evaluates the formula, so a typo in either shows."""
import ctypes as C

import pytest

B, H = 2, 3
EXACT, BF16 = 0, 1
FP32_DS, BF16_DS, NO_DS = 4, 2, 0

# (N, D, bf16 flag, causal, element size of the dS hand-off, bytes)
CASES = [
    (192, 64, EXACT, 0, FP32_DS, 889344),
    (192, 64, BF16, 0, BF16_DS, 446976),
    (193, 64, EXACT, 0, NO_DS, 4640),
    (197, 64, EXACT, 0, NO_DS, 4736),
    (204, 64, EXACT, 0, NO_DS, 4896),
    (205, 64, EXACT, 0, NO_DS, 4928),          # outside the 16-row kernels, still no dS (kv2 + q2 run)
    (208, 64, EXACT, 0, NO_DS, 4992),
    (209, 64, EXACT, 0, FP32_DS, 1209248),
    (197, 64, BF16, 0, BF16_DS, 606848),       # reserved although the one-kernel bf16 backward leaves it unused
    (208, 64, BF16, 0, BF16_DS, 607104),
    (224, 64, EXACT, 0, FP32_DS, 1209600),
    (100, 64, EXACT, 0, FP32_DS, 395616),
    (50, 32, EXACT, 0, FP32_DS, 99504),
    (50, 32, BF16, 0, BF16_DS, 50352),
    (225, 32, EXACT, 0, FP32_DS, 1578272),
    (256, 32, BF16, 0, BF16_DS, 792576),
    (100, 48, EXACT, 0, NO_DS, 2400),
    (100, 48, BF16, 0, NO_DS, 2400),
    (17, 8, EXACT, 0, NO_DS, 416),
    (17, 8, BF16, 0, NO_DS, 416),
]
SWITCHES = ("KANVIT_ATTN_V1", "KANVIT_ATTN_V2", "KANVIT_ATTN_V3", "KANVIT_ATTN_V4", "KANVIT_ATTN_NO_DS", "KANVIT_NO_BF16", "KANVIT_ATTN_GRID")


def formula(n, e, b=B, h=H):
    npad = (n + 31) // 32 * 32
    return (4 * b * h * n + 15) // 16 * 16 + e * b * h * npad * npad


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


@pytest.fixture
def default_switches(lib, monkeypatch):
    """Every attention switch unset for the test, and the library's configuration re-read before and after it."""
    from kanvit import _lib
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    _lib.reload_config()
    try:
        yield monkeypatch
    finally:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        _lib.reload_config()


def workspace(lib, n, d, flags, causal, b=B, h=H):
    from kanvit import _lib
    s = (h * n * d, n * d, d)
    desc = _lib.AttnDesc(b, h, n, d, causal, d ** -0.5, flags, 0, *s, *s, *s, *s)
    return int(lib.kanvit_attn_bwd_workspace(C.byref(desc)))


@pytest.mark.parametrize("n,d,flags,causal,e,nbytes", CASES)
def test_workspace_bytes(lib, default_switches, n, d, flags, causal, e, nbytes):
    assert formula(n, e) == nbytes
    assert workspace(lib, n, d, flags, causal) == nbytes


@pytest.mark.parametrize("n,d,flags", sorted({(n, d, f) for n, d, f, _, _, _ in CASES}))
def test_causal_reserves_rowsums_only(lib, default_switches, n, d, flags):
    assert workspace(lib, n, d, flags, 1) == formula(n, NO_DS)


def test_second_form_switch_hands_fp32_ds_over_at_197(lib, default_switches):
    """KANVIT_ATTN_V2 switches the one-kernel 16-row backward off: exact (197, 64) then runs kv2 with the fp32 dS hand-off."""
    from kanvit import _lib
    assert formula(197, FP32_DS) == 1208960
    default_switches.setenv("KANVIT_ATTN_V2", "1")
    assert "attn_v2=1" in _lib.reload_config()
    assert workspace(lib, 197, 64, EXACT, 0) == 1208960


@pytest.mark.parametrize("n,d,flags", sorted({(n, d, f) for n, d, f, _, _, _ in CASES}))
def test_no_ds_switch_reserves_rowsums_only(lib, default_switches, n, d, flags):
    from kanvit import _lib
    default_switches.setenv("KANVIT_ATTN_NO_DS", "1")
    assert "attn_no_ds=1" in _lib.reload_config()
    assert workspace(lib, n, d, flags, 0) == formula(n, NO_DS)


def test_other_batch_and_head_counts_follow_the_formula(lib, default_switches):
    for b, h in ((1, 1), (5, 7), (0, 3)):
        assert workspace(lib, 100, 64, EXACT, 0, b, h) == formula(100, FP32_DS, b, h)
        assert workspace(lib, 50, 32, BF16, 0, b, h) == formula(50, BF16_DS, b, h)
