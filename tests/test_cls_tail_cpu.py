"""CPU-only checks around the class-token tail: the single-query attention entry points are declared, exported and bound; the
switch that restores the every-row path is reported last by active_config(); and the generalised grouped packing gives run_qkv
the weights it always had."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q1_SYMBOLS = {"kanvit_attn_q1_fwd", "kanvit_attn_q1_bwd"}


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def test_q1_symbols_are_declared_exported_and_bound(lib):
    from kanvit import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kanvit.h")).read(), flags=re.S)
    declared = {n for n in re.findall(r"\b(kanvit_[a-z0-9_]+)\s*\(", header) if "_q1_" in n}
    assert declared == Q1_SYMBOLS
    assert {n for n in _lib.SYMBOLS if "_q1_" in n} == Q1_SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in Q1_SYMBOLS:
        assert hasattr(raw, name), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert len(_lib.SYMBOLS["kanvit_attn_q1_fwd"][1]) == 8 and len(_lib.SYMBOLS["kanvit_attn_q1_bwd"][1]) == 12


def test_q1_refusals_are_host_side(lib):
    """The descriptor checks run before anything touches the device: they answer without a GPU, with -22 and a message."""
    from kanvit import _lib

    def call(**kw):
        f = dict(B=2, H=2, N=1, D=64, causal=0, scale=0.125, flags=0)
        f.update(kw)
        d = _lib.AttnDesc(**f)
        e = _lib.AttnExt(Nk=9)
        return lib.kanvit_attn_q1_fwd(ctypes.byref(d), ctypes.byref(e), None, None, None, None, None, None)

    for kw, text in ((dict(D=3), b"D=3 must be even"), (dict(D=130), b"D=130 must be even and <= 128"), (dict(N=2), b"ONE query"),
                     (dict(causal=1), b"causal"), (dict(flags=1), b"flags=1"), (dict(), b"null q/k/v/o/p")):
        assert call(**kw) == -22, kw
        assert text in lib.kanvit_last_error(), (kw, lib.kanvit_last_error())
    assert call(B=0) == 0                                    # an empty batch returns before anything is looked at or launched


def test_no_cls_tail_is_the_last_python_switch(lib, monkeypatch):
    from kanvit import _lib
    monkeypatch.delenv("KANVIT_NO_CLS_TAIL", raising=False)
    monkeypatch.delenv("KANVIT_LIB", raising=False)
    try:
        cfg = _lib.reload_config()
        assert cfg.endswith(" py_no_cls_tail=0")
        assert re.findall(r"py_\w+(?==)", cfg)[-1] == "py_no_cls_tail"
        assert "no_cls_tail" in _lib.py_switches.__doc__ and "KANVIT_NO_CLS_TAIL" in _lib.py_switches.__doc__
        monkeypatch.setenv("KANVIT_NO_CLS_TAIL", "1")
        assert _lib.reload_config().endswith(" py_no_cls_tail=1")
        assert _lib.py_switches()["no_cls_tail"] == 1
    finally:
        monkeypatch.undo()
        _lib.reload_config()


def test_run_qkv_packing_is_the_generalised_packing(lib):
    """run_qkv packs through pack_projections([q, k, v]): for a cheby MSA that is kan_pack_grouped over q + k + v in head order
    (groups = 3H, x_group_mod = H), and the k|v and q packings of the class-token path are its slices.  CPU tensors, no launch."""
    from attention import MSA
    from kanvit import grouped
    from models.cheby import ChebyKANLayer
    torch.manual_seed(3)
    msa = MSA(64, 2, type="cheby")
    layers = list(msa.q_mappings) + list(msa.k_mappings) + list(msa.v_mappings)
    want, _, _ = ChebyKANLayer.kan_pack_grouped(layers)
    cfg, w, bp, bias = grouped.pack_projections([msa.q_mappings, msa.k_mappings, msa.v_mappings])
    assert (cfg.groups, cfg.x_group_mod, cfg.I, cfg.O, cfg.G) == (6, 2, 32, 32, 5) and bp is None and bias is None
    assert torch.equal(w, want)
    cfg_kv, w_kv, _, _ = grouped.pack_projections([msa.k_mappings, msa.v_mappings])
    cfg_q, w_q, _, _ = grouped.pack_projections([msa.q_mappings])
    assert (cfg_kv.groups, cfg_kv.x_group_mod, cfg_q.groups, cfg_q.x_group_mod) == (4, 2, 2, 2)
    assert torch.equal(w_q, want[:2]) and torch.equal(w_kv, want[2:])
    # the packed weight stays a differentiable function of the layers' own parameters
    w.sum().backward()
    assert all(m.cheby_coeffs.grad is not None for m in layers)
