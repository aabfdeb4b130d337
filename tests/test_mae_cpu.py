"""Masked-autoencoder pretraining without a GPU: the three C entry points' declarations and host-side refusals, MaskedAutoencoder's
construction, the float32 restatement of the loss against its float64 one (the yardstick of tests/test_mae_gpu.py checked on its own),
and train.py's flags, refusals and encoder hand-over."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from kanvit import _lib, ops
from tests import _mae_ref as ref

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
    return C.c_void_p(base), buf          # a 16-byte aligned pointer and what keeps it alive; never dereferenced


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_listed(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kanvit.h")).read(), flags=re.S)
    want = {
        "kanvit_tokens_restore_fwd": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
        "kanvit_tokens_restore_bwd": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
        "kanvit_mae_loss": (C.c_int, [C.POINTER(_lib.PatchDesc), C.c_int64, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, _P]),
    }
    raw = C.CDLL(_lib.LIB_PATH)
    for name, sig in want.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in kanvit.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert _lib.SYMBOLS[name] == sig, name
    assert lib.kanvit_abi_version() == 7                       # additive
    cap = re.search(r"#define KANVIT_MAE_MAX_I (\d+)", header)
    assert cap and int(cap.group(1)) == _lib.MAE_MAX_I >= 3072          # a 32 x 32 x 3 patch fits
    from kanvit import build
    assert "mae.hip" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "mae.hip"))
    assert open(os.path.join(build.CSRC, "soft_ce.hip")).read().rstrip().endswith('#include "mae.hip"')
    assert open(os.path.join(build.CSRC, "addln.hip")).read().rstrip().endswith('#include "patch_drop.hip"')
    assert len(build.SOURCES) == 22 and "mae.hip" not in build.SOURCES


def test_restore_refuses_on_the_host(lib, p):
    ptr, _ = p
    off4, off2 = C.c_void_p(ptr.value + 4), C.c_void_p(ptr.value + 2)

    def fwd(B=2, P=16, K=4, O=64, y=ptr, mask=ptr, pos=ptr, idx=ptr, out=ptr):
        return lib.kanvit_tokens_restore_fwd(B, P, K, O, y, mask, pos, idx, out, None)

    for kw, word in ((dict(K=16), b"K=16"), (dict(K=0), b"K=0"), (dict(K=17), b"K=17"), (dict(P=1025, K=8), b"P=1025"), (dict(O=0), b"O=0"),
                     (dict(B=-1), b"B=-1"), (dict(B=1 << 30), b"2^31"), (dict(y=None), b"null"), (dict(mask=None), b"null"),
                     (dict(pos=None), b"null"), (dict(idx=None), b"null"), (dict(out=None), b"null"), (dict(B=0, mask=None), b"null"),
                     (dict(y=off2), b"aligned"), (dict(out=C.c_void_p(ptr.value + 3)), b"aligned"), (dict(idx=off2), b"aligned")):
        assert fwd(**kw) == EINVAL, kw
        assert b"kanvit_tokens_restore_fwd" in lib.kanvit_last_error() and word in lib.kanvit_last_error(), (kw, lib.kanvit_last_error())
    assert fwd(B=0, y=None, idx=None, out=None) == 0            # no samples: nothing launched
    assert off4.value % 16 == 4                                  # a 4-byte aligned pointer is inside the domain (the general form takes it)

    def bwd(B=2, P=16, K=4, O=64, dout=ptr, idx=ptr, dy=ptr, dmask=ptr):
        return lib.kanvit_tokens_restore_bwd(B, P, K, O, dout, idx, dy, dmask, None)

    for kw, word in ((dict(K=16), b"K=16"), (dict(K=0), b"K=0"), (dict(P=1025, K=8), b"P=1025"), (dict(O=-4), b"O=-4"), (dict(B=-1), b"B=-1"),
                     (dict(dout=None), b"null"), (dict(idx=None), b"null"), (dict(dy=None, dmask=None), b"null"),
                     (dict(dmask=off2), b"aligned"), (dict(dy=off2), b"aligned"), (dict(dout=C.c_void_p(ptr.value + 1)), b"aligned")):
        assert bwd(**kw) == EINVAL, kw
        assert b"kanvit_tokens_restore_bwd" in lib.kanvit_last_error() and word in lib.kanvit_last_error(), (kw, lib.kanvit_last_error())


def test_mae_loss_refuses_on_the_host(lib, p):
    ptr, _ = p
    pd = _lib.PatchDesc(3, 32, 32, 4, 0, 0)          # P = 16, I = 192
    off2 = C.c_void_p(ptr.value + 2)

    def call(B=2, K=4, idx=ptr, images=ptr, pred=ptr, norm_pix=1, rows=ptr, loss=ptr, dpred=ptr, desc=pd):
        return lib.kanvit_mae_loss(None if desc is None else C.byref(desc), B, K, idx, images, pred, norm_pix, rows, loss, dpred, None)

    cap = _lib.MAE_MAX_I
    too_wide = _lib.PatchDesc(cap // 64 + 1, 16, 16, 2, 0, 0)           # I = 64 (C_max + 1) = cap + 64
    for kw, word in ((dict(K=16), b"K=16"), (dict(K=0), b"K=0"), (dict(K=17), b"K=17"), (dict(B=0), b"B=0"), (dict(B=-1), b"B=-1"),
                     (dict(desc=too_wide, K=1), f"I={cap + 64}".encode()), (dict(desc=_lib.PatchDesc(1, 4, 4, 4, 0, 0)), b"I=1"),
                     (dict(desc=_lib.PatchDesc(3, 32, 30, 4, 0, 0)), b"n_patches=4"), (dict(desc=None), b"null"),
                     (dict(idx=None), b"null"), (dict(images=None), b"null"), (dict(pred=None), b"null"), (dict(rows=None), b"null"),
                     (dict(loss=None), b"null"), (dict(dpred=None), b"null"), (dict(images=off2), b"aligned"), (dict(pred=off2), b"aligned"),
                     (dict(dpred=C.c_void_p(ptr.value + 1)), b"aligned"), (dict(rows=off2), b"aligned"), (dict(idx=off2), b"aligned")):
        assert call(**kw) == EINVAL, kw
        assert b"kanvit_mae_loss" in lib.kanvit_last_error() and word in lib.kanvit_last_error(), (kw, lib.kanvit_last_error())
    # I = 1 is refused because of norm_pix alone: without it the next refusal in line answers (a null pointer), not the size
    assert call(desc=_lib.PatchDesc(1, 4, 4, 4, 0, 0), norm_pix=0, idx=None) == EINVAL and b"null" in lib.kanvit_last_error()
    assert call(desc=_lib.PatchDesc(cap // 64, 16, 16, 2, 0, 0), K=1, idx=None) == EINVAL and b"null" in lib.kanvit_last_error()      # I = cap fits


def test_python_wrappers_refuse_without_a_gpu():
    idx = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(_lib.KanvitError, match="no CPU fallback"):
        ops.restore_tokens(torch.zeros(2, 5, 64), torch.zeros(1, 64), torch.zeros(17, 64), idx)
    with pytest.raises(_lib.KanvitError, match="no CPU fallback"):
        ops.mae_loss(torch.zeros(2, 17, 192), torch.zeros(2, 3, 32, 32), idx, 4)
    with pytest.raises(ops.KanvitOperandError, match="K=16"):
        ops.restore_tokens(torch.zeros(2, 17, 64), torch.zeros(64), torch.zeros(17, 64), torch.zeros(2, 16, dtype=torch.int32))
    with pytest.raises(ops.KanvitOperandError, match="K=16"):
        ops.mae_loss(torch.zeros(2, 17, 192), torch.zeros(2, 3, 32, 32), torch.zeros(2, 16, dtype=torch.int32), 4)
    with pytest.raises(ops.KanvitOperandError, match="I=1 "):
        ops.mae_loss(torch.zeros(2, 17, 1), torch.zeros(2, 1, 4, 4), idx, 4)


# ---- the module -------------------------------------------------------------------------------------------------------------------
def _vit(chw=(3, 32, 32), n=4, kind="vanilla", d=64, heads=2):
    from model import VisionTransformer
    return VisionTransformer(chw, n, 2, d, heads, 10, type=kind)


def test_construction_and_state_dict_keys():
    from mae import MaskedAutoencoder
    enc = _vit(kind="cheby")
    bare = list(enc.state_dict().keys())
    m = MaskedAutoencoder(enc, decoder_blocks=1, seed=5)
    keys = list(m.state_dict().keys())
    assert [k[len("encoder."):] for k in keys if k.startswith("encoder.")] == bare
    assert m.encoder is enc and list(enc.state_dict().keys()) == bare          # the encoder is used as it is
    rest = {k for k in keys if not k.startswith("encoder.")}
    block = {k for k in rest if k.startswith("decoder_blocks.0.")}
    assert rest - block == {"enc_norm.weight", "enc_norm.bias", "decoder_embed.weight", "decoder_embed.bias", "mask_token",
                            "decoder_norm.weight", "decoder_norm.bias", "decoder_pred.weight", "decoder_pred.bias"}
    from model import TransformerBlock
    assert {k[len("decoder_blocks.0."):] for k in block} == set(TransformerBlock(32, 2, 128).state_dict().keys())
    buffers = dict(m.named_buffers())
    assert "mask_counter" not in keys and buffers["mask_counter"].dtype == torch.int64 and buffers["mask_counter"].numel() == 1
    assert "decoder_pos" not in keys and tuple(buffers["decoder_pos"].shape) == (17, 32)
    assert torch.equal(buffers["decoder_pos"], enc.positional_embeddings(17, 32))
    assert tuple(m.mask_token.shape) == (1, 32) and m.decoder_dim == 32 and m.seed == 5
    assert m.decoder_embed.in_features == 64 and m.decoder_pred.out_features == enc.input_d == 192
    assert len(MaskedAutoencoder(_vit(), decoder_blocks=2).decoder_blocks) == 2          # the default


def test_widths_heads_and_the_kept_count():
    from mae import MaskedAutoencoder
    assert MaskedAutoencoder(_vit(d=192, heads=3)).decoder_dim == 96                       # d_hidden // 2
    assert MaskedAutoencoder(_vit(d=60, heads=6)).decoder_dim == 36                        # max(32, 30) rounded up to a multiple of 6
    assert MaskedAutoencoder(_vit(), decoder_dim=48, decoder_heads=4).decoder_blocks[0].attn.n_heads == 4
    with pytest.raises(ValueError, match="multiple"):
        MaskedAutoencoder(_vit(), decoder_dim=50, decoder_heads=4)
    assert MaskedAutoencoder(_vit(), decoder_type="cheby", decoder_blocks=1).decoder_blocks[0].attn is not None
    # K = max(1, int(P * (1 - ratio))): timm's rule, set_patch_dropout's
    for chw, n, ratio in (((1, 28, 28), 14, 0.75), ((1, 28, 28), 14, 0.5), ((3, 32, 32), 4, 0.75), ((3, 32, 32), 4, 0.9), ((3, 32, 32), 4, 0.99)):
        m = MaskedAutoencoder(_vit(chw, n), mask_ratio=ratio)
        assert m.n_keep == _vit(chw, n).set_patch_dropout(ratio) == max(1, int(n * n * (1.0 - ratio))), (n, ratio)
    assert MaskedAutoencoder(_vit((1, 28, 28), 14)).n_keep == 49                          # the default ratio 0.75
    for ratio in (0.0, 1e-18):                                                             # K == P: nothing to reconstruct
        with pytest.raises(ValueError, match="keeps all"):
            MaskedAutoencoder(_vit(), mask_ratio=ratio)
    for ratio in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            MaskedAutoencoder(_vit(), mask_ratio=ratio)
    with pytest.raises(NotImplementedError, match="flash-attn"):
        MaskedAutoencoder(_vit(kind="flash-attn"))
    with pytest.raises(TypeError):
        MaskedAutoencoder(torch.nn.Linear(2, 2))
    with pytest.raises(NotImplementedError, match="patches"):
        MaskedAutoencoder(_vit((1, 33, 33), 33))                                           # P = 1089


def test_a_cpu_model_or_cpu_images_are_refused():
    from mae import MaskedAutoencoder
    m = MaskedAutoencoder(_vit())
    with pytest.raises(_lib.KanvitError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 32, 32))
    with pytest.raises(_lib.KanvitError):
        m(torch.zeros(2, 3, 32))
    assert int(m.mask_counter) == 0


def test_unpatchify_inverts_patchify():
    from mae import MaskedAutoencoder
    m = MaskedAutoencoder(_vit((3, 8, 12), 2))
    x = torch.randn(3, 3, 8, 12)
    assert torch.equal(m.unpatchify(m.encoder.patchify(x, 2)), x)
    assert np.array_equal(ref.patchify(x.numpy(), 2), m.encoder.patchify(x, 2).numpy())


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(3, 8, 8, 4), (3, 16, 16, 4), (1, 28, 28, 4), (3, 32, 32, 2), (3, 64, 64, 2)]


@pytest.mark.parametrize("norm_pix", [True, False])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float32_restatement_agrees_with_float64(shape, norm_pix):
    """The two precisions of one restatement: every entry within the first-order bound of an fp32 evaluation of its formula -- for rows,
    a sum of I squares of differences whose operands carry a few ulp each: (I + 16) ulp of the value; for dpred, 16 ulp of the largest
    |pred| + |target| (the subtraction's operands); the loss, a sum of B P such rows, (B P + I + 16) ulp."""
    c, h, w, n = shape
    B, P = 3, n * n
    rng = np.random.default_rng(h * 10 + c)
    images = rng.standard_normal((B, c, h, w)).astype(np.float32)
    I = c * (h // n) * (w // n)
    pred = rng.standard_normal((B, P + 1, I)).astype(np.float32)
    for K in sorted({1, P - 1, max(1, P // 4)}):
        idx = ref.keep_table(B, P, K)
        l64, r64, d64 = ref.mae_loss(pred, images, idx, n, norm_pix, np.float64)
        l32, r32, d32 = ref.mae_loss(pred, images, idx, n, norm_pix, np.float32)
        assert r32.dtype == np.float32 and d32.dtype == np.float32 and l32.dtype == np.float32
        u = 2.0 ** -24
        assert (np.abs(r32 - r64) <= (I + 16) * u * r64).all()
        assert np.abs(d32 - d64).max() <= 16 * u * 2.0 / (I * B * (P - K)) * (np.abs(pred).max() + 8.0)
        assert abs(float(l32) - l64) <= (B * P + I + 16) * u * l64
        kept = ref.kept_mask(idx, P)
        assert (r64[kept] == 0).all() and (r64[~kept] > 0).all() and not d64[:, 0].any() and not d64[:, 1:][kept].any()
        assert int((~kept).sum()) == B * (P - K)


def test_masked_mean_is_the_projects_row_mean_with_another_divisor():
    rows = np.random.default_rng(0).random(1000).astype(np.float32)
    a, b = ref.masked_mean_rows_f32(rows, rows.size), ref.mean_rows_f32(rows)
    assert a.view(np.uint32) == b.view(np.uint32)
    assert ref.masked_mean_rows_f32(rows.reshape(10, 100), 250) == ref.masked_mean_rows_f32(rows, 1000) * np.float32(4)


def test_restore_restatements_agree():
    B, P, K, O = 3, 16, 4, 6
    rng = np.random.default_rng(1)
    y, mask, pos = (rng.standard_normal(s).astype(np.float32) for s in ((B, K + 1, O), (O,), (P + 1, O)))
    idx = ref.keep_table(B, P, K)
    assert (idx[:, 1:] > idx[:, :-1]).all() and idx[0, 0] == 0 and idx[1, -1] == P - 1
    want = ref.restore(y, mask, pos, idx)
    got = ref.restore_torch(torch.from_numpy(y), torch.from_numpy(mask), torch.from_numpy(pos), torch.from_numpy(idx)).numpy()
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32))
    dy, dmask, dropped = ref.restore_bwd(want, idx)
    assert np.array_equal(dy[:, 0], want[:, 0]) and np.array_equal(dy[2, 1:], want[2, 1 + idx[2]]) and int(dropped.sum()) == B * (P - K)
    dy_t, dmask_t = ref.restore_bwd_torch(torch.from_numpy(want), torch.from_numpy(idx))
    assert np.array_equal(dy_t.numpy(), dy) and np.allclose(dmask_t.numpy(), dmask, rtol=1e-5)


# ---- train.py -----------------------------------------------------------------------------------------------------------------------
def test_flags_and_their_defaults():
    import train
    a = train.parse([])
    assert (a.pretrain, a.mask_ratio, a.decoder_dim, a.decoder_blocks, a.decoder_heads, a.decoder_type, a.no_norm_pix_loss, a.save_encoder,
            a.init_encoder) == (None, 0.75, 0, 2, 0, "vanilla", False, None, None)
    a = train.parse(["--pretrain", "mae", "--mask-ratio", "0.5", "--decoder-dim", "48", "--decoder-blocks", "1", "--decoder-heads", "4",
                     "--decoder-type", "cheby", "--no-norm-pix-loss", "--save-encoder", "e.pt", "--init-encoder", "i.pt"])
    assert (a.pretrain, a.mask_ratio, a.decoder_dim, a.decoder_blocks, a.decoder_heads, a.decoder_type, a.no_norm_pix_loss, a.save_encoder,
            a.init_encoder) == ("mae", 0.5, 48, 1, 4, "cheby", True, "e.pt", "i.pt")
    import types
    hand = train.complete(types.SimpleNamespace(pretrain="mae"))                 # a namespace built by hand reads like a parsed one
    assert hand.mask_ratio == 0.75 and hand.decoder_blocks == 2 and hand.save_encoder is None
    assert {"pretrain", "mask_ratio", "decoder_dim", "decoder_blocks", "decoder_heads", "decoder_type", "no_norm_pix_loss", "save_encoder",
            "init_encoder"} <= set(train.defaults())
    for bad in (["--mask-ratio", "1.0"], ["--mask-ratio", "0"], ["--decoder-blocks", "0"], ["--decoder-dim", "-1"], ["--pretrain", "simclr"]):
        with pytest.raises(SystemExit):
            train.parse(bad)


REFUSED = [["--mixup", "0.8", "--data-npz", "x.npz"], ["--cutmix", "1.0", "--data-npz", "x.npz"], ["--label-smoothing", "0.1"], ["--fused-loss"],
           ["--reg-lambda", "1e-3", "--model-type", "cheby"], ["--prune", "2:0.5", "--model-type", "cheby"],
           ["--grid-update-every", "2", "--model-type", "efficientkan"], ["--grid-extend", "2:8", "--model-type", "efficientkan"],
           ["--patch-dropout", "0.5"], ["--device-metrics"], ["--model-type", "flash-attn"], ["--decoder-type", "flash-attn"]]


@pytest.mark.parametrize("flags", REFUSED, ids=lambda f: f[0] + ("=" + f[1] if f[0] in ("--model-type", "--decoder-type") else ""))
def test_refused_combinations_stop_main_before_the_gpu(flags, monkeypatch):
    import train

    def boom(*a, **k):
        raise AssertionError("the run went on to the GPU")
    monkeypatch.setattr(train, "setup_distributed", boom)
    data = "--synthetic" if "--data-npz" not in flags else None
    argv = ["--pretrain", "mae", "--device", "cuda", *([data] if data else []), *flags]
    word = flags[0] if flags[0] != "--model-type" else "flash-attn"
    with pytest.raises(SystemExit) as e:
        train.main(train.parse(argv))
    assert "--pretrain" in str(e.value) or "--decoder-type" in str(e.value), str(e.value)
    assert word in str(e.value), str(e.value)
    if flags[0] not in ("--model-type", "--decoder-type"):                       # the same flags without --pretrain go on to the GPU
        with pytest.raises(AssertionError, match="went on to the GPU"):
            train.main(train.parse(argv[2:]))


def test_a_missing_encoder_file_stops_main_before_the_gpu(monkeypatch, tmp_path):
    import train
    monkeypatch.setattr(train, "setup_distributed", lambda a: (_ for _ in ()).throw(AssertionError("the run went on to the GPU")))
    with pytest.raises(SystemExit, match="--init-encoder"):
        train.main(train.parse(["--synthetic", "--device", "cuda", "--init-encoder", str(tmp_path / "none.pt")]))


def test_encoder_round_trip_on_cpu_tensors(tmp_path):
    """--save-encoder writes the VisionTransformer's state_dict -- of a MaskedAutoencoder, the encoder's alone; --init-encoder loads all of
    it but the head, refuses a file that does not fit by naming the keys, and rebuilds the edge masks of a pruned file from its zeros."""
    import train
    from mae import MaskedAutoencoder
    torch.manual_seed(0)
    enc = _vit(kind="cheby")
    lm = enc.linear_mapper
    for prm, run in lm._edge_tensors():                                          # prune edge 3 by hand: exact zeros, as prune_edges leaves them
        with torch.no_grad():
            prm.view(-1, run)[3] = 0
    path = str(tmp_path / "enc.pt")
    train.save_encoder(MaskedAutoencoder(enc), None, path, ema=False)
    saved = torch.load(path, weights_only=True)
    assert list(saved) == list(enc.state_dict()) and all(torch.equal(saved[k], v) for k, v in enc.state_dict().items())

    torch.manual_seed(1)
    fresh = _vit(kind="cheby")
    head = {k: v.clone() for k, v in fresh.state_dict().items() if k.startswith("mlp_head.")}
    assert not torch.equal(fresh.v_class, enc.v_class)
    train.load_encoder(fresh, path)
    for k, v in fresh.state_dict().items():
        if k.startswith("mlp_head."):
            assert torch.equal(v, head[k]), k                                       # the head is fresh
        else:
            assert torch.equal(v, saved[k]), k
    assert not torch.equal(fresh.state_dict()["mlp_head.1.weight"], saved["mlp_head.1.weight"])
    mask = fresh.linear_mapper.edge_mask.reshape(-1)
    assert int(mask[3]) == 0 and int(mask.sum()) == mask.numel() - 1                # the pruned edge is masked again

    torch.save(saved, str(tmp_path / "plain.pt"))
    train.save_encoder(enc, None, str(tmp_path / "bare.pt"), ema=False)             # a supervised run saves the model itself
    assert list(torch.load(str(tmp_path / "bare.pt"), weights_only=True)) == list(saved)
    for change, word in ((lambda s: s.update(stranger=torch.zeros(1)), "stranger"), (lambda s: s.pop("v_class"), "v_class"),
                         (lambda s: s.update(v_class=torch.zeros(1, 3)), "v_class")):
        bad = dict(saved)
        change(bad)
        torch.save(bad, str(tmp_path / "bad.pt"))
        with pytest.raises(SystemExit, match=word):
            train.load_encoder(_vit(kind="cheby"), str(tmp_path / "bad.pt"))
    with pytest.raises(SystemExit, match="linear_mapper"):                        # another model type: its keys are named
        train.load_encoder(_vit(kind="vanilla"), path)
    no_head = {k: v for k, v in saved.items() if not k.startswith("mlp_head.")}
    torch.save(no_head, str(tmp_path / "nohead.pt"))
    train.load_encoder(_vit(kind="cheby"), str(tmp_path / "nohead.pt"))          # the head is skipped either way
