"""CPU-only checks of the resampling batch kernel's surroundings (csrc/batch_u8.hip: kanvit_resample_u8; kanvit/data.py: crop_table;
train.py --resize / --random-resized-crop): the float32 restatement the GPU tests compare with, anchored to torch's own bilinear
interpolation; the per-epoch crop table and what it may depend on; the new symbols and their host-side refusals; the resources of
the new kernels; the wrapper without a GPU and the command-line flags."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _augment_ref as ar
from tests import _resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [0.5071], [0.2675]                      # CIFAR's channel 0 (train.py:101-104)


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def _image(H, W, seed):
    x = np.random.default_rng(seed).integers(0, 256, (1, H, W, 1), dtype=np.uint8)
    x.reshape(-1)[:2] = (0, 255)[:x.size]           # the table's ends occur whenever the image has two pixels
    return x


@pytest.mark.parametrize("src,dst", [((8, 8), (20, 20)), ((7, 9), (12, 10)), ((8, 8), (5, 5)), ((1, 1), (7, 7)), ((32, 32), (224, 224))])
def test_restatement_is_torchs_bilinear_interpolation(src, dst):
    """Whole-image boxes against F.interpolate(bilinear, align_corners=False) on the CPU.  Bound: 2^-20 max(bh, bw) (max lut - min lut)
    -- a few ulp of a source coordinate below max(bh, bw), times the largest step between neighbouring taps."""
    x = _image(*src, seed=src[0] * 100 + dst[0])
    table = rr.lut(MEAN, STD)
    got = rr.resample_all(x, MEAN, STD, None, dst)
    normalised = torch.from_numpy(table[0][x[..., 0].astype(np.int64)])[:, None]                 # [1, 1, H, W]
    want = torch.nn.functional.interpolate(normalised, size=dst, mode="bilinear", align_corners=False, antialias=False).numpy()
    bound = 2.0 ** -20 * max(src) * float(table.max() - table.min())
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"{src} -> {dst}: max |restatement - torch| = {err:.3e}, bound {bound:.3e}")
    assert got.shape == want.shape == (1, 1, *dst) and got.dtype == np.float32
    assert err <= bound


@pytest.mark.parametrize("hw", [(8, 8), (32, 32)])
def test_restatement_is_the_identity_at_the_stored_size(hw):
    x = _image(*hw, seed=hw[0])
    got = rr.resample_all(x, MEAN, STD, None, hw)
    want = rr.lut(MEAN, STD)[0][x[..., 0].astype(np.int64)][:, None]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("pad,flip", [((4, 4), True), ((3, 1), True), ((0, 0), True), ((2, 2), False)])
def test_pad_table_is_the_per_sample_hash(pad, flip):
    from kanvit import data
    n, hw = 300, (32, 24)
    t = data.crop_table(n, 3, 11, hw, "pad", pad=pad, flip=flip)
    assert t.dtype == torch.int32 and tuple(t.shape) == (n, 5) and t.device.type == "cpu"
    want = [[dy - pad[0], dx - pad[1], hw[0], hw[1], fl] for dy, dx, fl in ar.params(11, 3, range(n), pad[0], pad[1], flip)]
    assert t.tolist() == want
    assert np.array_equal(t.numpy(), rr.pad_rows(11, 3, n, hw, pad, flip))
    if flip and pad[0]:
        assert set(t[:, 4].tolist()) == {0, 1} and len(set(t[:, 0].tolist())) == 2 * pad[0] + 1
    assert np.array_equal(data.crop_table(n, 3, 11, hw, "pad", pad=2).numpy(), rr.pad_rows(11, 3, n, hw, 2))       # an int pads both axes


def test_rrc_table_is_the_loop_restatement_and_depends_on_seed_and_epoch_alone():
    from kanvit import data
    n, hw = 2000, (32, 32)
    t = data.crop_table(n, 3, 11, hw, "rrc")
    assert t.dtype == torch.int32 and tuple(t.shape) == (n, 5) and t.device.type == "cpu"
    assert np.array_equal(t.numpy(), rr.rrc_rows(n, 3, 11, hw))
    y0, x0, h, w, fl = t.numpy().T.astype(np.int64)
    assert (h >= 1).all() and (w >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all() and (y0 + h <= 32).all() and (x0 + w <= 32).all()
    assert set(fl.tolist()) == {0, 1} and 0.4 < fl.mean() < 0.6
    assert h.min() < 12 and h.max() > 28 and len(set(zip(h.tolist(), w.tolist()))) > 100       # the scale range is used
    assert torch.equal(t, data.crop_table(n, 3, 11, hw, "rrc"))
    assert not torch.equal(t, data.crop_table(n, 4, 11, hw, "rrc")) and not torch.equal(t, data.crop_table(n, 3, 12, hw, "rrc"))
    assert torch.equal(t[:500], data.crop_table(n, 3, 11, hw, "rrc", pad=(4, 4))[:500])        # `pad` is not used
    # the signature has no batch size, rank or world size to depend on
    assert list(inspect.signature(data.crop_table).parameters) == ["n", "epoch", "seed", "hw", "mode", "pad", "flip", "scale", "ratio"]
    other = data.crop_table(300, 0, 5, (7, 9), "rrc", scale=(0.3, 0.6), ratio=(0.5, 2.0))
    assert np.array_equal(other.numpy(), rr.rrc_rows(300, 0, 5, (7, 9), scale=(0.3, 0.6), ratio=(0.5, 2.0)))
    area = (other[:, 2] * other[:, 3]).double() / 63
    assert float(area.min()) > 0.2 and float(area.max()) < 0.75


def test_rrc_fallback_and_flip_column():
    from kanvit import data
    t = data.crop_table(400, 0, 0, (2, 64), "rrc")                  # no 3/4..4/3 box of >= 8 % fits two rows: every row falls back
    assert (t[:, :4] == torch.tensor([0, (64 - 3) // 2, 2, 3], dtype=torch.int32)).all()
    assert np.array_equal(t.numpy(), rr.rrc_rows(400, 0, 0, (2, 64)))
    tall = data.crop_table(50, 0, 0, (64, 2), "rrc")
    assert (tall[:, :4] == torch.tensor([(64 - 3) // 2, 0, 3, 2], dtype=torch.int32)).all()
    assert np.array_equal(tall.numpy(), rr.rrc_rows(50, 0, 0, (64, 2)))
    cifar = data.crop_table(50000, 0, 0, (32, 32), "rrc")           # a square image: one of ten attempts fits in every row
    rows, fell_back = rr.rrc_rows(50000, 0, 0, (32, 32), with_fallback=True)
    assert np.array_equal(cifar.numpy(), rows) and not fell_back.any()
    assert rr.rrc_rows(400, 0, 0, (2, 64), with_fallback=True)[1].all()
    assert not data.crop_table(400, 0, 0, (32, 32), "rrc", flip=False)[:, 4].any()
    flipped = data.crop_table(400, 0, 0, (32, 32), "rrc")
    assert flipped[:, 4].any() and torch.equal(data.crop_table(400, 0, 0, (32, 32), "rrc", flip=False)[:, :4], flipped[:, :4])


def test_crop_table_refuses_bad_arguments():
    from kanvit import data
    for bad in (dict(n=0), dict(hw=(0, 8)), dict(mode="center"), dict(mode="pad", pad=(9, 0)), dict(mode="pad", pad=(0, -1)),
                dict(scale=(0.0, 1.0)), dict(scale=(0.5, 0.2)), dict(ratio=(2.0, 1.0)), dict(ratio=(-1.0, 1.0))):
        kw = dict(n=10, epoch=0, seed=0, hw=(8, 8), mode="rrc")
        kw.update(bad)
        with pytest.raises(ValueError, match="crop_table"):
            data.crop_table(**kw)


def test_symbols_are_declared_exported_and_bound(lib):
    from kanvit import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kanvit.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kanvit_[a-z0-9_]+)\s*\(", src))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("kanvit_resample_u8", "kanvit_resample_u8_supported"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
    P, I64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _lib.SYMBOLS["kanvit_resample_u8_supported"] == (I, [I64, I, I, I, I, I])
    assert _lib.SYMBOLS["kanvit_resample_u8"] == (I, [P] * 12 + [I64, I64, I, I, I, I, I, P])
    assert lib.kanvit_abi_version() == 7


def test_entry_point_validates_on_the_host(lib):
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)

    def call(images=p, idx=p, lut=p, crop=None, partner=None, weight=None, box=None, out=p, labels=None, y_out=None, y2_out=None, w_out=None,
             N=10, B=1, H=32, W=32, C=3, OH=224, OW=224):
        return lib.kanvit_resample_u8(images, labels, idx, lut, crop, partner, weight, box, out, y_out, y2_out, w_out, N, B, H, W, C, OH, OW, None)

    for kw, word in ((dict(N=0), b"N=0"), (dict(C=5), b"C=5"), (dict(C=0), b"C=0"), (dict(H=0), b"H=0"), (dict(W=(1 << 20) + 1), b"W=1048577"),
                     (dict(OH=0), b"OH=0"), (dict(OW=-3), b"OW=-3"), (dict(OH=(1 << 20) + 1), b"OH=1048577"), (dict(B=-1), b"B=-1"),
                     (dict(images=None), b"null images"), (dict(idx=None), b"null"), (dict(lut=None), b"null"), (dict(out=None), b"null"),
                     (dict(partner=p), b"null weight"), (dict(weight=p, box=p), b"null partner"), (dict(partner=p, weight=p), b"null box"),
                     (dict(y2_out=p, labels=p), b"without the mix tables"), (dict(w_out=p), b"without the mix tables"),
                     (dict(y_out=p), b"without labels"), (dict(partner=p, weight=p, box=p, y2_out=p), b"without labels"),
                     (dict(out=odd), b"aligned"), (dict(crop=odd), b"aligned"), (dict(idx=odd), b"aligned")):
        assert call(**kw) == -22, kw
        msg = lib.kanvit_last_error()
        assert b"kanvit_resample_u8" in msg and word in msg, (kw, msg)
    assert call(B=0) == 0                                            # an empty batch launches nothing: no device needed
    assert call(B=0, images=None, partner=p) == 0


def test_supported_agrees_with_the_entry_point(lib):
    for shape in ((10, 32, 32, 3, 224, 224), (1, 1, 1, 1, 1, 1), (1, 1 << 20, 1 << 20, 4, 1 << 20, 1 << 20), (0, 32, 32, 3, 8, 8), (5, 32, 32, 5, 8, 8),
                  (5, 32, 32, 0, 8, 8), (5, 0, 32, 3, 8, 8), (5, 32, (1 << 20) + 1, 3, 8, 8), (5, 32, 32, 3, 0, 8), (5, 32, 32, 3, 8, (1 << 20) + 1)):
        N, H, W, C, OH, OW = shape
        ok = lib.kanvit_resample_u8_supported(*shape)
        rc = lib.kanvit_resample_u8(None, None, None, None, None, None, None, None, None, None, None, None, N, 0, H, W, C, OH, OW, None)
        assert ok == (1 if rc == 0 else 0) and rc in (0, -22), shape
    assert lib.kanvit_resample_u8_supported(10, 32, 32, 3, 224, 224) == 1 and lib.kanvit_resample_u8_supported(10, 32, 32, 3, 0, 224) == 0


def test_new_kernels_use_no_scratch_and_spill_nothing(lib):
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    from kanvit import build
    ks = {km.demangled_short(n): k for n, k in km.kernels(build.LIB).items()}
    res = sorted(n for n in ks if n.startswith("resample_u8_kernel"))
    # <VEC, MIX>: the scalar and the 16-byte store form, each without and with the mix tables
    assert res == ["resample_u8_kernel<1, 0>", "resample_u8_kernel<1, 1>", "resample_u8_kernel<4, 0>", "resample_u8_kernel<4, 1>"]
    for n in res:
        assert ks[n][".private_segment_fixed_size"] == 0 and ks[n][".vgpr_spill_count"] == 0 and ks[n][".sgpr_spill_count"] == 0, n
        assert ks[n][".group_segment_fixed_size"] == 4 * 1024               # the staged table, as augment_u8_kernel's
    assert sorted(n for n in ks if n.startswith("augment_u8_kernel")) == ["augment_u8_kernel<1>", "augment_u8_kernel<4>"]
    assert sorted(n for n in ks if n.startswith("mix_u8_kernel")) == ["mix_u8_kernel<1>", "mix_u8_kernel<4>"]


def test_wrapper_refuses_cpu_tensors():
    from kanvit import KanvitError, data, ops
    images, labels, idx = torch.zeros(4, 4, 4, 3, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    lut = data.make_lut([0.5] * 3, [0.2] * 3)
    with pytest.raises(KanvitError, match="no CPU fallback"):
        ops.resample_u8(images, labels, idx, lut, (8, 8))
    with pytest.raises(KanvitError, match="no CPU fallback"):
        ops.resample_u8(images, labels, idx, lut, 8, data.crop_table(4, 0, 0, (4, 4), "rrc"), *data.mix_table(4, 0, 0, (8, 8), mixup_alpha=1.0))
    with pytest.raises(KanvitError, match="come together"):
        ops.resample_u8(images, labels, idx, lut, 8, partner=torch.zeros(4, dtype=torch.int64))


def test_command_line_flags(tmp_path):
    import train
    a = train.parse([])
    assert (a.resize, a.random_resized_crop, tuple(a.rrc_scale), tuple(a.rrc_ratio)) == (0, False, (0.08, 1.0), (3 / 4, 4 / 3))
    b = train.parse(["--data-npz", "x.npz", "--resize", "224", "--random-resized-crop", "--rrc-scale", "0.25", "1", "--rrc-ratio", "0.5", "2",
                     "--mixup", "0.8", "--graph", "--device-metrics", "--amp", "bf16"])
    assert (b.resize, b.random_resized_crop, tuple(b.rrc_scale), tuple(b.rrc_ratio)) == (224, True, (0.25, 1.0), (0.5, 2.0))
    assert b.image_size == 32                                        # keeps its meaning: the file's size
    assert train.parse(["--data-npz", "x.npz", "--random-resized-crop"]).resize == 0
    for argv, word in ((["--resize", "224"], "--data-npz"), (["--synthetic", "--resize", "224"], "--data-npz"),
                       (["--random-resized-crop"], "--data-npz"), (["--synthetic", "--random-resized-crop"], "--data-npz"),
                       (["--data-npz", "x.npz", "--random-resized-crop", "--no-augment"], "--no-augment"),
                       (["--data-npz", "x.npz", "--resize", "-8"], "--resize"),
                       (["--data-npz", "x.npz", "--random-resized-crop", "--rrc-scale", "0.5", "0.2"], "--rrc-scale"),
                       (["--data-npz", "x.npz", "--random-resized-crop", "--rrc-scale", "0", "1"], "--rrc-scale"),
                       (["--data-npz", "x.npz", "--random-resized-crop", "--rrc-ratio", "2", "1"], "--rrc-ratio")):
        with pytest.raises(SystemExit, match=word):
            train.parse(argv)
    assert train.parse(["--data-npz", "x.npz", "--resize", "64", "--no-augment"]).no_augment      # a plain resize needs no augmentation
    # namespaces that did not come through parse()
    for change, word in ((dict(resize=224), "--data-npz"), (dict(random_resized_crop=True), "--data-npz"),
                         (dict(data_npz="x.npz", random_resized_crop=True, no_augment=True), "--no-augment"),
                         (dict(data_npz="x.npz", resize=-1), "--resize"), (dict(data_npz="x.npz", rrc_scale=(1.0, 0.5)), "--rrc-scale")):
        ns = train.parse([])
        for k, v in change.items():
            setattr(ns, k, v)
        with pytest.raises(SystemExit, match=word):
            train.main(ns)
    src = open(os.path.join(ROOT, "kan-vit_amd", "train.py")).read()
    assert "unused" in src[src.index("'--crop-padding'"):src.index("'--resize'")]                  # the help says what RandomResizedCrop replaces
