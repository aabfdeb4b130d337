"""CPU-only checks of the attention-map surface: the kanvit_attn_probs export and its refusals, the code-object metadata of its
kernel, the no-CPU-fallback rule, and VisionTransformer.rollout (pure torch) against a float64 statement."""
import ctypes
import os

import pytest
import torch

from tests._attention_map_ref import rollout_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def test_export_and_abi_version(lib):
    from kanvit import _lib
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "kanvit_attn_probs")
    P = ctypes.c_void_p
    assert lib.kanvit_attn_probs.restype is ctypes.c_int
    assert lib.kanvit_attn_probs.argtypes == [ctypes.POINTER(_lib.AttnDesc), ctypes.POINTER(_lib.AttnExt), P, P, P, ctypes.c_int64,
                                              ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, P]
    assert lib.kanvit_abi_version() == 7
    from kanvit import build
    assert "attention_probs.hip" in build.SOURCES and len(build.SOURCES) == 22


def _call(lib, d=None, e=None, q=8, k=8, p=8, stride_q=None, rows=1, **kw):
    """kanvit_attn_probs on a valid B=1, H=1, N=4, Nk=6, D=8 description with the keywords changed; the pointers are never
    dereferenced by a refused call (non-null dummies)."""
    from kanvit import _lib
    desc = dict(B=1, H=1, N=4, D=8, causal=0, scale=0.5, flags=0, q_stride_b=32, q_stride_h=32, q_stride_n=8,
                k_stride_b=48, k_stride_h=48, k_stride_n=8)
    ext = dict(Nk=6)
    for key, v in kw.items():
        (ext if key == "Nk" else desc)[key] = v
    dd = _lib.AttnDesc(**desc) if d is None else d
    ee = _lib.AttnExt(**ext) if e is None else e
    sq = ext["Nk"] if stride_q is None else stride_q
    return lib.kanvit_attn_probs(None if d is False else ctypes.byref(dd), None if e is False else ctypes.byref(ee), q or None, k or None,
                                 p or None, 24, 24, sq, rows, None)


REFUSALS = [
    (dict(d=False), b"null"), (dict(e=False), b"null"), (dict(q=0), b"null"), (dict(k=0), b"null"), (dict(p=0), b"null"),
    (dict(D=7), b"D=7"), (dict(D=130), b"D=130"), (dict(scale=0.0), b"scale"), (dict(scale=-1.0), b"scale"),
    (dict(rows=0), b"rows=0"), (dict(rows=5), b"rows=5"), (dict(stride_q=5), b"p_stride_q=5"),
    (dict(B=0), b"B=0"), (dict(H=0), b"H=0"), (dict(N=0), b"N=0"), (dict(Nk=0, stride_q=6), b"Nk=0"),
    (dict(causal=1), b"causal"),                       # Nk = 6 > N = 4
    (dict(flags=1), b"KANVIT_FLAG_BF16_MFMA"), (dict(flags=2), b"flags=2"),
]


@pytest.mark.parametrize("kw,needle", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in REFUSALS])
def test_refusals_return_einval_and_name_the_argument(lib, kw, needle):
    assert _call(lib, **kw) == -22
    msg = lib.kanvit_last_error()
    assert msg.startswith(b"kanvit_attn_probs") and needle in msg, msg


def test_causal_refusal_is_worded_as_the_general_forward_words_it(lib):
    from kanvit import _lib
    assert _call(lib, causal=1) == -22
    mine = lib.kanvit_last_error().split(b":", 1)[1]
    d = _lib.AttnDesc(B=1, H=1, N=4, D=8, causal=1, scale=0.5)
    e = _lib.AttnExt(Nk=6)
    assert lib.kanvit_attn_x_fwd(ctypes.byref(d), ctypes.byref(e), 8, 8, 8, 8, None, None) == -22
    assert lib.kanvit_last_error().split(b":", 1)[1] == mine


def test_ops_refuse_cpu_tensors():
    from kanvit import ops
    q, k = torch.zeros(1, 1, 4, 8), torch.zeros(1, 1, 6, 8)
    with pytest.raises(ops.KanvitError):
        ops.attention_probs(q, k)
    with pytest.raises(ops.KanvitError):
        ops.attention_probs_packed(torch.zeros(1, 4, 3, 1, 8))


def test_kernel_uses_no_scratch_and_spills_no_vgpr(lib):
    """The code object's own metadata (tools/kernel_meta.py: no GPU, no ROCm tool), as tests/test_abi_cpu.py reads it."""
    pytest.importorskip("msgpack")
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    from kanvit import build
    ks = km.kernels(build.LIB)
    mine = [n for n in ks if "attn_probs" in n]              # the symbol, mangled or not
    assert len(mine) >= 1
    for n in mine:
        assert ks[n][".private_segment_fixed_size"] == 0 and ks[n][".vgpr_spill_count"] == 0, (n, ks[n])


def _random_maps(L, B, H, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(2.0 * torch.randn(L, B, H, N, N, generator=g), dim=-1)


@pytest.mark.parametrize("fusion", ["mean", "max", "min"])
def test_rollout_against_float64_statement(fusion):
    """fp32 products of non-negative rows that sum to 1: n_blocks * N * 2^-23 (the bound of the GPU model test)."""
    from model import VisionTransformer
    maps = _random_maps(3, 2, 4, 9, 5)
    got = VisionTransformer.rollout(maps, fusion)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 9, 9)
    ref = rollout_ref(maps, fusion)
    bound = 3 * 9 * 2.0 ** -23
    assert float((got.double() - ref).abs().max()) <= bound
    assert float((got.double().sum(-1) - 1).abs().max()) <= bound


@pytest.mark.parametrize("fusion", ["mean", "max", "min"])
def test_rollout_closed_forms(fusion):
    """Uniform maps: A~ = (J/N + I)/2 with J the all-ones matrix, and (J/N)^2 = J/N, so A~^L = 2^-L I + (1 - 2^-L) J/N.
    Identity maps: A~ = I and the rollout is I."""
    from model import VisionTransformer
    L, B, H, N = 3, 2, 2, 6
    uni = torch.full((L, B, H, N, N), 1.0 / N)
    want = 2.0 ** -L * torch.eye(N, dtype=torch.float64) + (1 - 2.0 ** -L) / N
    got = VisionTransformer.rollout(uni, fusion)
    assert float((got.double() - want).abs().max()) <= L * N * 2.0 ** -23
    eye = torch.eye(N).expand(L, B, H, N, N)
    assert torch.equal(VisionTransformer.rollout(eye, fusion), torch.eye(N).expand(B, N, N))


def test_rollout_refuses_partial_maps_and_unknown_fusion():
    from model import VisionTransformer
    with pytest.raises(ValueError, match="full"):
        VisionTransformer.rollout(torch.rand(2, 1, 2, 1, 5))
    with pytest.raises(ValueError, match="head_fusion"):
        VisionTransformer.rollout(_random_maps(1, 1, 1, 4, 0), "median")
