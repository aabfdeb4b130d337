"""CPU-only checks of Mixup / CutMix and the fused soft-target loss (kanvit/data.py: mix_table; csrc/batch_u8.hip: kanvit_mix_u8; csrc/soft_ce.hip:
kanvit_soft_ce; train.py --mixup / --cutmix / --label-smoothing / --fused-loss): the per-epoch table and what it may depend on, the new
symbols and their host-side refusals, the resources of the new kernels, the wrappers without a GPU and the command-line flags."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = dict(mixup_alpha=0.8, cutmix_alpha=1.0)


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def test_table_depends_on_seed_and_epoch_and_on_nothing_about_the_batches():
    from kanvit import data
    t = data.mix_table(500, 3, 11, (32, 32), **BOTH)
    assert isinstance(t, data.MixTable)
    assert (t.partner.dtype, t.weight.dtype, t.box.dtype) == (torch.int64, torch.float32, torch.int32)
    assert tuple(t.partner.shape) == (500,) and tuple(t.weight.shape) == (500,) and tuple(t.box.shape) == (500, 4)
    assert all(v.device.type == "cpu" for v in t)
    assert _same(t, data.mix_table(500, 3, 11, (32, 32), **BOTH))
    assert not _same(t, data.mix_table(500, 4, 11, (32, 32), **BOTH)) and not _same(t, data.mix_table(500, 3, 12, (32, 32), **BOTH))
    # the signature has no batch size, rank or world size to depend on (tests/test_batch_mix_gpu.py checks the pixels across batch
    # sizes and ranks)
    import inspect
    assert list(inspect.signature(data.mix_table).parameters) == ["n", "epoch", "seed", "hw", "mixup_alpha", "cutmix_alpha", "prob", "switch_prob"]


@pytest.mark.parametrize("kw", [BOTH, dict(mixup_alpha=0.4), dict(cutmix_alpha=1.0), dict(cutmix_alpha=0.2, prob=0.5),
                                dict(mixup_alpha=1.0, cutmix_alpha=1.0, switch_prob=0.9, prob=0.7)])
@pytest.mark.parametrize("hw", [(32, 32), (8, 12), (1, 1)])
def test_table_rows_are_well_formed(kw, hw):
    from kanvit import data
    n, (H, W) = 2000, hw
    p, w, box = (v.numpy() for v in data.mix_table(n, 0, 5, hw, **kw))
    assert p.min() >= -1 and p.max() < n
    assert w.min() >= 0.0 and w.max() <= 1.0
    y0, y1, x0, x1 = box.T.astype(np.int64)
    assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= H).all() and (0 <= x0).all() and (x0 <= x1).all() and (x1 <= W).all()
    area = (y1 - y0) * (x1 - x0)
    unmixed, cut = p < 0, area > 0
    assert (w[unmixed] == 1.0).all() and (area[unmixed] == 0).all() and not (cut & unmixed).any()
    assert np.array_equal(w[cut], (1.0 - area[cut] / float(H * W)).astype(np.float32))          # exactly, from float64
    assert (box[~cut] == 0).all()                                       # Mixup and unmixed rows hold the empty box
    if kw.get("mixup_alpha", 0) == 0:
        assert (cut | unmixed).all()
    if kw.get("cutmix_alpha", 0) == 0:
        assert not cut.any() and len(np.unique(w[~unmixed])) > n // 2    # lam itself
    if kw.get("prob", 1.0) == 1.0 and kw.get("cutmix_alpha", 0) == 0:
        assert not unmixed.any()
    if "prob" in kw:                    # 2000 draws: 0.05 is over four standard deviations; CutMix boxes clipped to nothing add to the share
        assert unmixed.mean() > 1 - kw["prob"] - 0.05 and (unmixed & (area == 0)).sum() == unmixed.sum()
    if kw.get("switch_prob") == 0.9 and hw == (32, 32):
        assert 0.75 < cut[~unmixed].mean() <= 0.9 + 0.03                # a box clipped to nothing leaves the CutMix share
    if (~unmixed).sum() > 100:                                          # (1, 1) images leave CutMix next to no box
        assert len(set(p[~unmixed].tolist())) > (~unmixed).sum() // 4     # partners are spread over the dataset


def test_prob_zero_mixes_nothing_and_both_alphas_zero_is_refused():
    from kanvit import data
    t = data.mix_table(300, 0, 0, (8, 8), prob=0.0, **BOTH)
    assert (t.partner == -1).all() and (t.weight == 1).all() and not t.box.any()
    with pytest.raises(ValueError, match="both 0"):
        data.mix_table(300, 0, 0, (8, 8))
    for bad in (dict(mixup_alpha=-1.0), dict(mixup_alpha=1.0, prob=1.5), dict(cutmix_alpha=1.0, switch_prob=-0.1)):
        with pytest.raises(ValueError):
            data.mix_table(300, 0, 0, (8, 8), **bad)


def test_symbols_are_declared_exported_and_bound(lib):
    from kanvit import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kanvit.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kanvit_[a-z0-9_]+)\s*\(", src))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("kanvit_mix_u8", "kanvit_soft_ce"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
    P, I64, I, U64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64
    assert _lib.SYMBOLS["kanvit_mix_u8"] == (I, [P] * 11 + [I64, I64, I, I, I, I, I, I, U64, U64, P])
    assert _lib.SYMBOLS["kanvit_soft_ce"] == (I, [P, I64, P, P, P, I64, I, ctypes.c_float, P, P, P, P])
    assert lib.kanvit_abi_version() == 7


def test_mix_entry_point_validates_on_the_host(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(images=p, partner=p, weight=p, box=p, N=10, B=1, H=32, W=32, C=3, pad_y=4, pad_x=4, flip=1, labels=None, y_out=None):
        return lib.kanvit_mix_u8(images, labels, p, p, partner, weight, box, p, y_out, None, None, N, B, H, W, C, pad_y, pad_x, flip, 0, 0, None)

    for kw, word in ((dict(C=5), b"C=5"), (dict(pad_y=33), b"pad_y=33"), (dict(pad_x=33), b"pad_x=33"), (dict(N=0), b"N=0"),
                     (dict(B=-1), b"B=-1"), (dict(H=0), b"H=0"), (dict(flip=2), b"flip=2"), (dict(images=None), b"null images"),
                     (dict(partner=None), b"partner"), (dict(weight=None), b"weight"), (dict(box=None), b"box"),
                     (dict(y_out=p), b"without labels")):
        assert call(**kw) == -22, kw
        msg = lib.kanvit_last_error()
        assert b"kanvit_mix_u8" in msg and word in msg, (kw, msg)
    assert call(B=0) == 0                                            # an empty batch launches nothing: no device needed
    assert call(B=0, partner=None) == 0


def test_soft_ce_entry_point_validates_on_the_host(lib):
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(logits=p, ld=4, y1=p, y2=None, w=None, B=2, C=4, eps=0.1, rows=p, dz=p, loss=p):
        return lib.kanvit_soft_ce(logits, ld, y1, y2, w, B, C, eps, rows, dz, loss, None)

    for kw, word in ((dict(C=1), b"C=1"), (dict(B=0), b"B=0"), (dict(ld=3), b"ld=3"), (dict(eps=1.0), b"eps=1"), (dict(eps=-0.5), b"eps=-0.5"),
                     (dict(eps=float("nan")), b"eps="), (dict(logits=None), b"null"), (dict(y1=None), b"null"), (dict(rows=None), b"null"),
                     (dict(dz=None), b"null"), (dict(loss=None), b"null"), (dict(y2=p), b"y2 without w"), (dict(w=p), b"w without y2")):
        assert call(**kw) == -22, kw
        msg = lib.kanvit_last_error()
        assert b"kanvit_soft_ce" in msg and word in msg, (kw, msg)


def test_new_kernels_use_no_scratch_and_spill_nothing(lib):
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    from kanvit import build
    ks = {km.demangled_short(n): k for n, k in km.kernels(build.LIB).items()}
    mix = sorted(n for n in ks if n.startswith("mix_u8_kernel"))
    assert mix == ["mix_u8_kernel<1>", "mix_u8_kernel<4>"]                  # the scalar and the 16-byte store form
    loss = sorted((n for n in ks if "soft_ce_" in n), key=len)             # no template arguments: the names stay mangled
    assert len(loss) == 2 and "14soft_ce_kernelE" in loss[0] and "19soft_ce_mean_kernelE" in loss[1], loss
    for n in mix + loss:
        assert ks[n][".private_segment_fixed_size"] == 0 and ks[n][".vgpr_spill_count"] == 0 and ks[n][".sgpr_spill_count"] == 0, n
    for n in mix:
        assert ks[n][".group_segment_fixed_size"] == 4 * 1024               # the staged table, as augment_u8_kernel's
    assert ks[loss[0]][".group_segment_fixed_size"] == 0                    # one wave per row: shuffles only
    assert not [n for n in ks if "metrics" in n and ("mix" in n or "soft" in n)]


def test_wrappers_refuse_cpu_tensors():
    from kanvit import KanvitError, data, ops
    images, labels, idx = torch.zeros(4, 4, 4, 3, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    t = data.mix_table(4, 0, 0, (4, 4), mixup_alpha=1.0)
    with pytest.raises(KanvitError, match="no CPU fallback"):
        ops.mix_u8(images, labels, idx, data.make_lut([0.5] * 3, [0.2] * 3), *t)
    z, y = torch.zeros(4, 3, requires_grad=True), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(KanvitError, match="no CPU fallback"):
        ops.soft_cross_entropy(z, y)
    with pytest.raises(KanvitError, match="no CPU fallback"):
        ops.soft_cross_entropy(z, y, y, torch.ones(4), label_smoothing=0.1)


def test_command_line_flags(tmp_path):
    import train
    a = train.parse([])
    assert (a.mixup, a.cutmix, a.mix_prob, a.mix_switch_prob, a.label_smoothing, a.fused_loss) == (0.0, 0.0, 1.0, 0.5, 0.0, False)
    assert train.mix_config(a) is None
    b = train.parse(["--data-npz", "x.npz", "--mixup", "0.8", "--cutmix", "1.0", "--mix-prob", "0.9", "--mix-switch-prob", "0.25",
                     "--label-smoothing", "0.1", "--fused-loss"])
    assert train.mix_config(b) == dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.9, switch_prob=0.25)
    assert b.label_smoothing == 0.1 and b.fused_loss is True
    assert train.parse(["--synthetic", "--label-smoothing", "0.1"]).label_smoothing == 0.1      # the loss needs no dataset
    with pytest.raises(SystemExit, match="--data-npz"):
        train.parse(["--mixup", "0.8"])
    with pytest.raises(SystemExit, match="--data-npz"):
        train.parse(["--synthetic", "--cutmix", "1.0"])
    with pytest.raises(SystemExit, match="--no-augment"):
        train.parse(["--data-npz", "x.npz", "--cutmix", "1.0", "--no-augment"])
    for bad in (["--mixup", "-1"], ["--label-smoothing", "1.0"], ["--mix-prob", "1.5"], ["--mix-switch-prob", "-0.1"]):
        with pytest.raises(SystemExit, match=bad[0]):
            train.parse(["--data-npz", "x.npz", *bad])
    a.mixup = 0.8
    with pytest.raises(SystemExit, match="--data-npz"):
        train.main(a)                                                # also for a namespace that did not come through parse()
    src = open(os.path.join(ROOT, "kan-vit_amd", "train.py")).read()
    assert "majority label" in src[src.index("'--mixup'"):src.index("'--mix-prob'")]            # the metrics rule is in the flags' help
