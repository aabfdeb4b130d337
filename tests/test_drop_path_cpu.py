"""Stochastic depth without a GPU: the three C entry points are declared, exported and listed with their signatures; their host-side
refusals by error code and message; the Python restatement of the keep decisions (ops.depth_keep); VisionTransformer.set_drop_path;
train.py's flags."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from kanvit import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
_P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_float * 256)()
    return C.cast(buf, _P), buf          # the pointer and what keeps it alive


def _keep(*values):
    arr = (C.c_float * len(values))(*values)
    return C.cast(arr, _P), arr


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_listed(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kanvit.h")).read(), flags=re.S)
    want = {
        "kanvit_depth_scales": (C.c_int, [C.c_int64, C.c_int, _P, C.c_uint64, _P, _P, _P]),
        "kanvit_addln_sd_fwd": (C.c_int, [C.c_int64, C.c_int, C.c_float, _P, _P, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int64, _P]),
        "kanvit_addln_sd_bwd": (C.c_int, [C.c_int64, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int64, _P,
                                          C.c_size_t, _P]),
    }
    raw = C.CDLL(_lib.LIB_PATH)
    for name, sig in want.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in kanvit.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert _lib.SYMBOLS[name] == sig, name
        assert not any(family in name for family in ("optim", "metrics", "refit", "regrid", "_q1_"))
    assert lib.kanvit_abi_version() == 7                       # additive
    assert "#define KANVIT_DEPTH_MAX_BRANCHES 64" in header and _lib.DEPTH_MAX_BRANCHES == 64


def test_depth_scales_refuses_on_the_host(lib, p):
    ptr, _ = p
    k65, hold = _keep(*([0.5] * 65))
    assert lib.kanvit_depth_scales(4, 65, k65, 0, ptr, ptr, None) == EINVAL
    assert b"kanvit_depth_scales" in lib.kanvit_last_error() and b"n_branch=65" in lib.kanvit_last_error()
    assert lib.kanvit_depth_scales(4, 0, k65, 0, ptr, ptr, None) == EINVAL
    for bad in (0.0, 1.5, -0.25, float("nan")):
        k, hold = _keep(0.5, bad)
        assert lib.kanvit_depth_scales(4, 2, k, 0, ptr, ptr, None) == EINVAL
        assert b"keep[1]" in lib.kanvit_last_error() and b"(0, 1]" in lib.kanvit_last_error()
    k, hold = _keep(0.5)
    assert lib.kanvit_depth_scales(-1, 1, k, 0, ptr, ptr, None) == EINVAL
    assert b"B=-1" in lib.kanvit_last_error()
    assert lib.kanvit_depth_scales(4, 1, None, 0, ptr, ptr, None) == EINVAL
    assert lib.kanvit_depth_scales(4, 1, k, 0, None, ptr, None) == EINVAL
    assert b"null" in lib.kanvit_last_error()


def test_scaled_addln_refuses_on_the_host(lib, p):
    ptr, _ = p

    def fwd(M, D, rps, delta=ptr, scale=ptr):
        return lib.kanvit_addln_sd_fwd(M, D, 1e-5, ptr, delta, 0, ptr, ptr, ptr, ptr, 0, ptr, ptr, scale, rps, None)

    def bwd(M, D, rps, dx=ptr, dd=ptr, scale=ptr):
        return lib.kanvit_addln_sd_bwd(M, D, ptr, ptr, ptr, ptr, ptr, 0, None, dx, dd, 0, ptr, ptr, scale, rps, ptr, 1 << 20, None)

    for call, who in ((fwd, b"kanvit_addln_sd_fwd"), (bwd, b"kanvit_addln_sd_bwd")):
        assert call(4, 64, 0) == EINVAL                         # rows_per_sample = 0
        assert who in lib.kanvit_last_error() and b"rows_per_sample=0" in lib.kanvit_last_error()
        assert call(4, 64, 3) == EINVAL                         # M % N != 0
        assert who in lib.kanvit_last_error() and b"rows_per_sample=3" in lib.kanvit_last_error()
        assert call(4, 10, 2) == EINVAL                         # D = 10
        assert who in lib.kanvit_last_error() and b"D=10" in lib.kanvit_last_error()
        assert call(4, 64, 2, scale=None) == EINVAL
        assert b"null" in lib.kanvit_last_error()
    assert fwd(4, 64, 2, delta=None) == EINVAL and b"null" in lib.kanvit_last_error()
    assert bwd(4, 64, 2, dd=None) == EINVAL and b"null" in lib.kanvit_last_error()
    hold = (C.c_float * 256)()
    other = C.cast(hold, _P)
    assert bwd(4, 64, 2, dx=other, dd=other) == EINVAL and b"two buffers" in lib.kanvit_last_error()
    assert fwd(4, 64, 2, scale=C.c_void_p(ptr.value + 2)) == EINVAL and b"aligned" in lib.kanvit_last_error()
    assert fwd(0, 64, 2) == 0                                   # no rows: nothing to do, nothing launched


def test_python_wrappers_refuse_without_a_gpu():
    norm = torch.nn.LayerNorm(8)
    x, d = torch.randn(2, 3, 8), torch.randn(2, 3, 8)
    with pytest.raises(ValueError):
        ops.add_layernorm(x, None, norm, row_scale=torch.ones(2))          # nothing to scale
    with pytest.raises(ValueError):
        ops.add_layernorm(x.view(6, 8), d.view(6, 8), norm, row_scale=torch.ones(2))      # 2-D without rows_per_sample
    with pytest.raises(_lib.KanvitError):
        ops.add_layernorm(x, d, norm, row_scale=torch.ones(2))             # CPU tensors: no fallback
    with pytest.raises(_lib.KanvitError):
        ops.depth_scales(4, [0.5], 0, torch.zeros(1, dtype=torch.int64))
    # a width the kernel does not cover takes the stock composition, like the unscaled call
    norm10 = torch.nn.LayerNorm(10)
    x, d, sc = torch.randn(2, 3, 10), torch.randn(2, 3, 10), torch.tensor([0.0, 2.0])
    s, y = ops.add_layernorm(x, d, norm10, row_scale=sc)
    assert torch.equal(s, x + sc[:, None, None] * d) and torch.equal(y, norm10(s))
    s2, _ = ops.add_layernorm(x.view(6, 10), d.view(6, 10), norm10, row_scale=sc, rows_per_sample=3)
    assert torch.equal(s2.view(2, 3, 10), s)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_keep_one_always_keeps_with_scale_one():
    t = ops.depth_keep(257, [1.0, 1.0], seed=5, counter=9)
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 257) and bool((t == 1.0).all())


@pytest.mark.parametrize("keep", [0.9, 0.5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_kept_fraction_and_scale(keep, seed):
    B = 4096
    t = ops.depth_keep(B, [keep], seed, 0)[0]
    frac = float((t != 0).double().mean())
    print(f"keep {keep} seed {seed}: kept {frac:.4f}")
    assert abs(frac - keep) <= 4.0 * math.sqrt(keep * (1.0 - keep) / B)
    inv = np.float32(1.0) / np.float32(keep)
    assert set(np.unique(t.numpy()).tolist()) == {0.0, float(inv)}


def test_rows_of_different_branches_counters_and_seeds_differ():
    a = ops.depth_keep(512, [0.5, 0.5], 0, 0)
    assert not torch.equal(a[0], a[1])
    assert not torch.equal(a, ops.depth_keep(512, [0.5, 0.5], 0, 1))
    assert not torch.equal(a, ops.depth_keep(512, [0.5, 0.5], 1, 0))
    assert torch.equal(a, ops.depth_keep(512, [0.5, 0.5], 0, 0))
    assert torch.equal(a[:, :100], ops.depth_keep(100, [0.5, 0.5], 0, 0))            # a function of the position, not of B
    assert torch.equal(a, ops.depth_keep(512, [0.5, 0.5], 1 << 64, 0))               # the seed is taken mod 2^64
    with pytest.raises(ValueError):
        ops.depth_keep(4, [0.0], 0, 0)


# ---- the model --------------------------------------------------------------------------------------------------------------------
def _vit(n_blocks, kind="vanilla"):
    from model import VisionTransformer
    return VisionTransformer((3, 32, 32), 4, n_blocks, 64, 4, 10, type=kind)


def test_linear_and_constant_rates():
    assert _vit(1).set_drop_path(0.2) == [0.2]
    assert _vit(2).set_drop_path(0.2) == [0.0, 0.2]
    rates = _vit(12).set_drop_path(0.1)
    assert rates == pytest.approx([0.1 * l / 11 for l in range(12)], abs=1e-15) and rates[0] == 0.0 and rates[-1] == 0.1
    m = _vit(3)
    assert m.set_drop_path(0.3, schedule="constant") == [0.3, 0.3, 0.3]
    assert m._drop_path[0] == [0.7] * 6 and m.drop_path_rates == [0.3, 0.3, 0.3]      # both branches of a block share its rate
    for bad in (dict(rate=1.0), dict(rate=-0.1), dict(rate=0.1, schedule="cosine")):
        with pytest.raises(ValueError):
            m.set_drop_path(**bad)


def test_state_dict_is_unchanged_and_rate_zero_restores():
    m = _vit(2, "cheby")
    keys = list(m.state_dict().keys())
    m.set_drop_path(0.5, seed=3)
    assert list(m.state_dict().keys()) == keys
    assert m.drop_path_counter.dtype == torch.int64 and m.drop_path_counter.numel() == 1
    assert "drop_path_counter" in dict(m.named_buffers())
    m.set_drop_path(0.0)
    assert m._drop_path is None and not hasattr(m, "drop_path_counter") and m.drop_path_rates == []
    assert list(m.state_dict().keys()) == keys
    m.load_state_dict(_vit(2, "cheby").state_dict(), strict=True)


def test_rate_zero_takes_the_old_path(monkeypatch):
    """With the rate back at 0 the forward asks for no scales and hands add_layernorm no scale row."""
    import model
    seen = []

    def fake_add_layernorm(x, delta, norm, y_bf16=False, **kw):
        seen.append(kw)
        s = x if delta is None else x + delta
        return s, norm(s)

    def boom(*a, **k):
        raise AssertionError("depth_scales must not run at rate 0 or in eval()")

    table = torch.arange(4, dtype=torch.float32).unsqueeze(1).expand(4, 2).contiguous()      # row j of the fake scales is all j
    asked = []

    def fake_depth_scales(B, keep, seed, counter, out=None):
        asked.append((B, list(keep), seed))
        return table

    # the model on the CPU with the GPU ops replaced by their stock compositions: only the routing is under test
    monkeypatch.setattr(model, "add_layernorm", fake_add_layernorm)
    monkeypatch.setattr(model, "ff_small_supported", lambda d, f: False)
    monkeypatch.setattr(model, "feed_forward", lambda h, l1, l2: l2(torch.relu(l1(h))))
    m = _vit(2)
    for blk in m.blocks:
        blk.attn = torch.nn.Identity()
    x = torch.randn(2, 3, 32, 32)

    monkeypatch.setattr(model.ops, "depth_scales", fake_depth_scales)
    m.set_drop_path(0.5, seed=3)
    m.train()
    m(x)
    assert asked == [(2, [1.0, 1.0, 0.5, 0.5], 3)]                     # one call per forward; block 0 at rate 0, block 1 at 0.5
    # block 0: nothing pending, then its attention (branch 0); block 1: block 0's feed-forward (branch 1), its attention (branch 2)
    assert [None if kw["row_scale"] is None else float(kw["row_scale"][0]) for kw in seen] == [None, 0.0, 1.0, 2.0]

    monkeypatch.setattr(model.ops, "depth_scales", boom)
    del seen[:]
    m.eval()
    want = m(x)
    assert len(seen) == 4 and all(kw == {"row_scale": None} for kw in seen)             # eval(): the unscaled calls
    del seen[:]
    m.train()
    m.set_drop_path(0.0)
    got = m(x)
    assert len(seen) == 4 and all(kw == {"row_scale": None} for kw in seen)
    assert torch.equal(got, want)


def test_flash_attn_is_refused():
    m = _vit(2, "flash-attn")
    with pytest.raises(NotImplementedError):
        m.set_drop_path(0.1)
    assert m.set_drop_path(0.0) == []


# ---- train.py -----------------------------------------------------------------------------------------------------------------------
def test_train_flags():
    import train
    a = train.parse([])
    assert a.drop_path == 0.0 and a.drop_path_schedule == "linear"
    b = train.parse(["--drop-path", "0.1", "--drop-path-schedule", "constant"])
    assert b.drop_path == 0.1 and b.drop_path_schedule == "constant"
    for bad in (["--drop-path", "1.0"], ["--drop-path", "-0.1"], ["--drop-path-schedule", "cosine"]):
        with pytest.raises(SystemExit):
            train.parse(bad)
