"""PatchDropout without a GPU: the Python restatement of the keep table (ops.patch_keep_ref), VisionTransformer.set_patch_dropout, the
host-side refusals of the four C entry points by error code and message, and train.py's flag."""
import ctypes as C
import math
import os
import re

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
    base = C.addressof(buf)
    base += (-base) % 16
    return C.c_void_p(base), buf          # a 16-byte aligned pointer and what keeps it alive


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_listed(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kanvit.h")).read(), flags=re.S)
    want = {
        "kanvit_patch_keep": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_uint64, _P, _P, _P]),
        "kanvit_patch_gather": (C.c_int, [C.POINTER(_lib.PatchDesc), C.c_int64, C.c_int, _P, _P, _P, C.c_int64, _P]),
        "kanvit_tokens_assemble_fwd": (C.c_int, [C.c_int64, C.c_int, C.c_int, _P, C.c_int64, _P, _P, _P, _P, _P]),
        "kanvit_tokens_assemble_bwd": (C.c_int, [C.c_int64, C.c_int, C.c_int, _P, _P, _P, _P]),
    }
    raw = C.CDLL(_lib.LIB_PATH)
    for name, sig in want.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in kanvit.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert _lib.SYMBOLS[name] == sig, name
    assert lib.kanvit_abi_version() == 7                       # additive
    assert "#define KANVIT_PATCH_KEEP_MAX_P 1024" in header and _lib.PATCH_KEEP_MAX_P == 1024
    tag = re.search(r"#define KANVIT_PATCH_KEEP_TAG (0x[0-9A-Fa-f]+)ull", header)
    assert tag and int(tag.group(1), 16) == _lib.PATCH_KEEP_TAG
    from kanvit import build
    assert "patch_drop.hip" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "patch_drop.hip"))
    assert open(os.path.join(build.CSRC, "addln.hip")).read().rstrip().endswith('#include "patch_drop.hip"')


def test_patch_keep_refuses_on_the_host(lib, p):
    ptr, _ = p
    for P, K in ((16, 17), (16, 0), (16, -1), (1025, 8), (0, 0)):
        assert lib.kanvit_patch_keep(4, P, K, 0, ptr, ptr, None) == EINVAL, (P, K)
        assert b"kanvit_patch_keep" in lib.kanvit_last_error()
    assert lib.kanvit_patch_keep(4, 1025, 8, 0, ptr, ptr, None) == EINVAL and b"P=1025" in lib.kanvit_last_error()
    assert lib.kanvit_patch_keep(4, 16, 17, 0, ptr, ptr, None) == EINVAL and b"K=17" in lib.kanvit_last_error()
    assert lib.kanvit_patch_keep(-1, 16, 8, 0, ptr, ptr, None) == EINVAL and b"B=-1" in lib.kanvit_last_error()
    assert lib.kanvit_patch_keep(4, 16, 8, 0, None, ptr, None) == EINVAL and b"null" in lib.kanvit_last_error()
    assert lib.kanvit_patch_keep(4, 16, 8, 0, ptr, None, None) == EINVAL and b"null" in lib.kanvit_last_error()
    assert lib.kanvit_patch_keep(4, 16, 8, 0, C.c_void_p(ptr.value + 4), ptr, None) == EINVAL and b"aligned" in lib.kanvit_last_error()
    assert lib.kanvit_patch_keep(4, 16, 8, 0, ptr, C.c_void_p(ptr.value + 2), None) == EINVAL and b"aligned" in lib.kanvit_last_error()
    counter = (C.c_uint64 * 1)(7)
    assert lib.kanvit_patch_keep(0, 16, 8, 0, C.cast(counter, _P), None, None) == 0          # no samples: nothing launched,
    assert counter[0] == 7                                                                   # the counter is not touched


def test_patch_gather_refuses_on_the_host(lib, p):
    ptr, _ = p
    pd = _lib.PatchDesc(3, 32, 32, 4, 0, 0)          # P = 16, I = 192

    def call(B=2, K=8, idx=ptr, images=ptr, rows=ptr, ldr=192, desc=pd):
        return lib.kanvit_patch_gather(None if desc is None else C.byref(desc), B, K, idx, images, rows, ldr, None)

    for kw, word in ((dict(K=17), b"K=17"), (dict(K=0), b"K=0"), (dict(B=-1), b"B=-1"), (dict(ldr=191), b"ldr=191"), (dict(idx=None), b"null"),
                     (dict(images=None), b"null"), (dict(rows=None), b"null"), (dict(desc=None), b"null"),
                     (dict(images=C.c_void_p(ptr.value + 2)), b"aligned"), (dict(rows=C.c_void_p(ptr.value + 1)), b"aligned"),
                     (dict(idx=C.c_void_p(ptr.value + 2)), b"aligned"), (dict(desc=_lib.PatchDesc(3, 32, 30, 4, 0, 0)), b"n_patches=4")):
        assert call(**kw) == EINVAL, kw
        assert b"kanvit_patch_gather" in lib.kanvit_last_error() and word in lib.kanvit_last_error(), (kw, lib.kanvit_last_error())
    assert call(B=0, idx=None, images=None, rows=None) == 0


def test_tokens_assemble_refuses_on_the_host(lib, p):
    ptr, _ = p

    def fwd(B=2, K=8, O=64, tokens=ptr, ldt=64, cls=ptr, pos=ptr, idx=ptr, out=ptr):
        return lib.kanvit_tokens_assemble_fwd(B, K, O, tokens, ldt, cls, pos, idx, out, None)

    for kw, word in ((dict(K=0), b"K=0"), (dict(O=0), b"O=0"), (dict(B=-1), b"B=-1"), (dict(ldt=63), b"ldt=63"), (dict(cls=None), b"null"),
                     (dict(pos=None), b"null"), (dict(tokens=None), b"null"), (dict(idx=None), b"null"), (dict(out=None), b"null"),
                     (dict(B=0, cls=None), b"null"), (dict(tokens=C.c_void_p(ptr.value + 2)), b"aligned"),
                     (dict(out=C.c_void_p(ptr.value + 3)), b"aligned"), (dict(B=1 << 30, K=8), b"2^31")):
        assert fwd(**kw) == EINVAL, kw
        assert b"kanvit_tokens_assemble_fwd" in lib.kanvit_last_error() and word in lib.kanvit_last_error(), (kw, lib.kanvit_last_error())
    assert fwd(B=0, tokens=None, idx=None, out=None) == 0

    def bwd(B=2, K=8, O=64, dout=ptr, dtokens=ptr, dcls=ptr):
        return lib.kanvit_tokens_assemble_bwd(B, K, O, dout, dtokens, dcls, None)

    for kw, word in ((dict(K=0), b"K=0"), (dict(O=-4), b"O=-4"), (dict(B=-1), b"B=-1"), (dict(dout=None), b"null"),
                     (dict(dtokens=None, dcls=None), b"null"), (dict(dcls=C.c_void_p(ptr.value + 2)), b"aligned")):
        assert bwd(**kw) == EINVAL, kw
        assert b"kanvit_tokens_assemble_bwd" in lib.kanvit_last_error() and word in lib.kanvit_last_error(), (kw, lib.kanvit_last_error())


def test_python_wrappers_refuse_without_a_gpu():
    counter = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(_lib.KanvitError):
        ops.patch_keep(4, 16, 8, 0, counter)                                   # CPU tensors: no fallback
    for P, K in ((16, 17), (16, 0), (1025, 8)):
        with pytest.raises(ops.KanvitOperandError):
            ops.patch_keep(4, P, K, 0, counter)
        with pytest.raises(ops.KanvitOperandError):
            ops.patch_keep_ref(4, P, K, 0, 0)
    idx = torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(_lib.KanvitError):
        ops.patch_gather(torch.zeros(2, 3, 32, 32), idx, 4)
    with pytest.raises(_lib.KanvitError):
        ops.assemble_tokens(torch.zeros(16, 64), torch.zeros(64), torch.zeros(17, 64), idx)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,K", [(1, 1, 1), (3, 16, 8), (5, 49, 13), (2, 196, 98), (2, 1024, 1), (1, 1024, 1023)])
def test_rows_are_k_distinct_ascending_patches(B, P, K):
    t = ops.patch_keep_ref(B, P, K, seed=11, counter=3)
    assert t.dtype == torch.int32 and tuple(t.shape) == (B, K)
    assert int(t.min()) >= 0 and int(t.max()) < P
    assert bool((t[:, 1:] > t[:, :-1]).all())                          # strictly ascending: distinct as well


def test_keeping_everything_is_arange():
    assert torch.equal(ops.patch_keep_ref(3, 49, 49, 5, 9), torch.arange(49, dtype=torch.int32).expand(3, 49))


def test_seeds_counters_and_batch_sizes():
    a = ops.patch_keep_ref(16, 49, 24, 0, 0)
    assert torch.equal(a, ops.patch_keep_ref(16, 49, 24, 0, 0))
    assert not torch.equal(a, ops.patch_keep_ref(16, 49, 24, 1, 0))
    assert not torch.equal(a, ops.patch_keep_ref(16, 49, 24, 0, 1))
    assert not torch.equal(a[0], a[1])
    assert torch.equal(a[:5], ops.patch_keep_ref(5, 49, 24, 0, 0))                  # a function of the sample's position, not of B
    assert torch.equal(a, ops.patch_keep_ref(16, 49, 24, 1 << 64, 0))               # the seed is taken mod 2^64
    assert tuple(ops.patch_keep_ref(0, 49, 24, 0, 0).shape) == (0, 24)


def test_the_stream_is_apart_from_drop_paths():
    """The tag in the seed: without it, base would be depth_keep's mix(mix(seed) + c) and the two features would share their hashes."""
    from kanvit.data import _mix
    m64 = (1 << 64) - 1
    seed, c, P, K = 7, 2, 16, 8
    base = _mix((_mix(seed ^ _lib.PATCH_KEEP_TAG) + c) & m64)
    keys = sorted((_mix((base + (1 << 32) + p) & m64), p) for p in range(P))
    assert ops.patch_keep_ref(2, P, K, seed, c)[1].tolist() == sorted(p for _, p in keys[:K])
    untagged = _mix((_mix(seed) + c) & m64)
    assert base != untagged


def test_keep_frequencies_and_pairs():
    B, P, K = 4096, 16, 8
    t = ops.patch_keep_ref(B, P, K, seed=1, counter=0).long()
    kept = torch.zeros(B, P, dtype=torch.float64).scatter_(1, t, 1.0)
    freq = kept.mean(0)
    bound = 5.0 * math.sqrt(0.25 / B)
    print("keep frequency per patch:", [round(float(f), 4) for f in freq], "bound 0.5 +-", round(bound, 4))
    assert bool(((freq - 0.5).abs() <= bound).all())
    together = kept.T @ kept                                            # [P, P]: samples that keep both
    off = together[~torch.eye(P, dtype=torch.bool)]
    assert float(off.max()) < float(kept.sum(0).min())                  # no two patches are always kept together
    assert float(off.min()) > 0


# ---- the model --------------------------------------------------------------------------------------------------------------------
def _vit(chw=(3, 32, 32), n=4, kind="vanilla"):
    from model import VisionTransformer
    return VisionTransformer(chw, n, 2, 64, 4, 10, type=kind)


def test_set_patch_dropout_returns_timms_k():
    assert _vit((1, 28, 28), 14).set_patch_dropout(0.5) == 98           # P = 196
    assert _vit((1, 28, 28), 14).set_patch_dropout(0.25) == 147
    assert _vit().set_patch_dropout(0.9) == 1                           # P = 16: int(1.6) = 1
    m = _vit()
    assert m.set_patch_dropout(0.5, seed=9) == 8 and m._patch_dropout == (8, 9)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            m.set_patch_dropout(bad)
    big = _vit((1, 33, 33), 33)                                         # P = 1089
    with pytest.raises(NotImplementedError):
        big.set_patch_dropout(0.5)
    assert big.set_patch_dropout(0.0) == 1089


def test_state_dict_is_unchanged_and_rate_zero_restores():
    m = _vit(kind="cheby")
    keys = list(m.state_dict().keys())
    m.set_patch_dropout(0.5, seed=3)
    assert list(m.state_dict().keys()) == keys
    assert m.patch_dropout_counter.dtype == torch.int64 and m.patch_dropout_counter.numel() == 1
    assert "patch_dropout_counter" in dict(m.named_buffers())
    m.patch_dropout_counter.fill_(5)
    m.set_patch_dropout(0.25)
    assert int(m.patch_dropout_counter) == 0                            # setting it again starts the walk again
    assert m.set_patch_dropout(0.0) == 16
    assert m._patch_dropout is None and not hasattr(m, "patch_dropout_counter")
    assert m.set_patch_dropout(1e-18) == 16 and m._patch_dropout is None         # 1 - rate rounds to 1: K == P is rate 0
    assert list(m.state_dict().keys()) == keys
    m.load_state_dict(_vit(kind="cheby").state_dict(), strict=True)


def test_a_cpu_model_and_eval_run_what_they_always_ran(monkeypatch):
    import model

    def boom(*a, **k):
        raise AssertionError("patch_keep must not run in eval(), at rate 0 or on a CPU model")

    def fake_add_layernorm(x, delta, norm, y_bf16=False, **kw):
        s = x if delta is None else x + delta
        return s, norm(s)

    # the model on the CPU with the GPU ops replaced by their stock compositions: only the routing is under test
    monkeypatch.setattr(model.ops, "patch_keep", boom)
    monkeypatch.setattr(model, "add_layernorm", fake_add_layernorm)
    monkeypatch.setattr(model, "ff_small_supported", lambda d, f: False)
    monkeypatch.setattr(model, "feed_forward", lambda h, l1, l2: l2(torch.relu(l1(h))))
    torch.manual_seed(0)
    m = _vit()
    for blk in m.blocks:
        blk.attn = torch.nn.Identity()
    x = torch.randn(2, 3, 32, 32)
    want = m.eval()(x)
    assert m.set_patch_dropout(0.5, seed=3) == 8
    assert torch.equal(m.eval()(x), want)
    assert torch.equal(m.train()(x), want)                              # a CPU model: the full sequence
    assert int(m.patch_dropout_counter) == 0
    assert tuple(m._embed(x).shape) == (2, 17, 64)


# ---- train.py -----------------------------------------------------------------------------------------------------------------------
def test_train_flag():
    import train
    assert train.parse([]).patch_dropout == 0.0
    assert train.parse(["--patch-dropout", "0.25"]).patch_dropout == 0.25
    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit) as e:
            train.parse(["--patch-dropout", bad])
        assert "--patch-dropout" in str(e.value)
