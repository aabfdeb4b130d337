"""RandAugment without a GPU: kanvit.data.randaug_table and the wrapper's table check, the NumPy restatement of tests/_randaug_ref.py
against Pillow (equal where Pillow's op is integer, within one level where Pillow computes in floating point and truncates) and
against arithmetic alone for AFFINE, the C-ABI surface and refusals of kanvit_randaug_u8 (dummy pointers: a refused call dereferences
nothing) and train.parse's flag rules.  The kernel's pixels are tests/test_randaug_gpu.py's."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _randaug_ref as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = ra.Q16
P = 0x10000         # a non-null dummy pointer, aligned to 16 bytes


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


# ---- randaug_table ------------------------------------------------------------------------------------------------------------
def test_randaug_table_is_a_function_of_its_arguments():
    from kanvit import data
    a = data.randaug_table(200, 3, 11, (32, 32))
    assert a.dtype == torch.int32 and tuple(a.shape) == (200, 2, 8) and a.device.type == "cpu"
    assert torch.equal(a, data.randaug_table(200, 3, 11, (32, 32)))
    assert not torch.equal(a, data.randaug_table(200, 4, 11, (32, 32)))             # another epoch
    assert not torch.equal(a, data.randaug_table(200, 3, 12, (32, 32)))             # another seed
    assert not torch.equal(data.randaug_table(200, 0, 0, (32, 32)), data.randaug_table(200, 1, 0, (32, 32)))
    # the scheme is indexed by s (counters, no generator): row s does not depend on n, so a shorter table is the head of a longer one
    assert torch.equal(data.randaug_table(100, 3, 11, (32, 32)), a[:100])
    for k in (1, 3, 4):
        assert tuple(data.randaug_table(50, 0, 0, (28, 28), n_ops=k).shape) == (50, k, 8)
    # slot k's draws do not depend on n_ops either, and a row's parameters do not depend on prob, only whether it is kept
    assert torch.equal(data.randaug_table(200, 3, 11, (32, 32), n_ops=4)[:, :2], a)
    full = data.randaug_table(200, 3, 11, (32, 32), prob=1.0)
    kept = a[:, :, 0] != 0
    assert 0 < int(kept.sum()) < 400 and torch.equal(a[kept], full[kept]) and not bool(a[~kept].any())
    assert bool((full[:, :, 0] != 0).all())


def test_every_drawn_row_passes_the_wrappers_check_and_a_bad_row_does_not():
    from kanvit import data, ops
    for hw, kw in (((32, 32), {}), ((28, 28), dict(n_ops=4, magnitude=10.0, mstd=3.0, prob=1.0)), ((7, 5), dict(magnitude=0.0, prob=1.0)),
                   ((1, 24576), dict(prob=1.0, fill=255)), ((64, 96), dict(prob=1.0, fill=(1, 2, 3, 200)))):
        t = data.randaug_table(3000, 1, 5, hw, **kw)
        assert ops.randaug_check_table(t, 3000) is t
        assert set(np.unique(t[:, :, 0].numpy())) <= set(range(12))
    assert len(np.unique(data.randaug_table(3000, 1, 5, (32, 32), prob=1.0)[:, :, 0].numpy())) == 11      # every code but IDENTITY
    good = data.randaug_table(10, 0, 0, (8, 8))
    for s, k, row, in ((0, 0, ra.row(12)), (3, 1, ra.row(-1)), (9, 1, ra.row(ra.POSTERIZE, 9)), (2, 0, ra.row(ra.SOLARIZE, 257)),
                       (2, 0, ra.row(ra.SOLARIZE_ADD, 256, 128)), (2, 0, ra.row(ra.SOLARIZE_ADD, 10, -1)), (5, 1, ra.row(ra.BRIGHTNESS, 2 * Q + 1)),
                       (5, 1, ra.row(ra.COLOR, -1)), (5, 1, ra.row(ra.CONTRAST, 2 * Q + 1)), (5, 1, ra.row(ra.SHARPNESS, -5))):
        bad = good.clone()
        bad[s, k] = torch.tensor(row, dtype=torch.int32)
        with pytest.raises(ValueError, match=rf"row \[{s}, {k}\]") as e:
            ops.randaug_check_table(bad)
        assert isinstance(e.value, ops.KanvitError) and not ra.row_is_valid(row)
    edge = good.clone()                              # the ends of every range, and AFFINE with any int32
    edge[:8, 0] = torch.tensor([ra.row(ra.POSTERIZE, 0), ra.row(ra.POSTERIZE, 8), ra.row(ra.SOLARIZE, 0), ra.row(ra.SOLARIZE, 256),
                                ra.row(ra.SOLARIZE_ADD, 255, 256), ra.row(ra.SHARPNESS, 2 * Q), ra.row(ra.COLOR, 0),
                                ra.row(ra.AFFINE, *([-2 ** 31] * 7))], dtype=torch.int32)
    ops.randaug_check_table(edge, 10)
    for wrong in (good.long(), good[:, :, :7], good.reshape(10, 16), torch.zeros((10, 5, 8), dtype=torch.int32), good.numpy()):
        with pytest.raises(ValueError, match="randaug_check_table"):
            ops.randaug_check_table(wrong)
    with pytest.raises(ValueError, match="randaug_check_table"):
        ops.randaug_check_table(good, 11)


def test_kept_share():
    """n = 20 000 slots, prob 0.5: the binomial sigma is 0.0035, so 0.5 +- 0.02 is 5.7 sigmas.  The default op list holds no IDENTITY,
    so a kept slot is a row whose op code is not 0."""
    from kanvit import data
    assert "Identity" not in data.RANDAUG_OPS and len(data.RANDAUG_OPS) == 15
    t = data.randaug_table(20000, 0, 0, (32, 32), n_ops=1, prob=0.5).numpy()
    assert abs((t[:, 0, 0] != 0).mean() - 0.5) <= 0.02
    assert not data.randaug_table(1000, 0, 0, (32, 32), prob=0.0).any()
    picks = np.bincount(data.randaug_table(30000, 2, 1, (32, 32), n_ops=1, prob=1.0, ops=["Invert", "Equalize", "Identity"])[:, 0, 0].numpy())
    assert picks.shape == (4,) and picks[1] == 0 and all(abs(picks[c] / 30000 - 1 / 3) < 0.02 for c in (0, 2, 3))      # 7 sigmas


def test_magnitude_rules():
    from kanvit import data

    def rows(name, magnitude, hw=(32, 32), **kw):
        return data.randaug_table(400, 0, 3, hw, n_ops=1, magnitude=magnitude, mstd=0.0, prob=1.0, ops=[name], **kw)[:, 0].numpy().astype(np.int64)

    for name, code in (("AutoContrast", 1), ("Equalize", 2), ("Invert", 3)):
        assert (rows(name, 9.0) == ra.row(code)).all()
    assert (rows("Posterize", 10.0) == ra.row(4, 0)).all() and (rows("Posterize", 0.0) == ra.row(4, 4)).all() and (rows("Posterize", 9.0) == ra.row(4, 1)).all()
    assert (rows("Solarize", 10.0) == ra.row(5, 0)).all() and (rows("Solarize", 0.0) == ra.row(5, 256)).all() and (rows("Solarize", 5.0) == ra.row(5, 128)).all()
    assert (rows("SolarizeAdd", 10.0) == ra.row(6, 110, 128)).all() and (rows("SolarizeAdd", 5.0) == ra.row(6, 55, 128)).all()
    for name, code in (("Brightness", 7), ("Color", 8), ("Contrast", 9), ("Sharpness", 10)):
        r = rows(name, 10.0)
        assert (r[:, 0] == code).all() and set(r[:, 1]) == {int(round(0.1 * Q)), int(round(1.9 * Q))} and not r[:, 2:].any()
        assert set(rows(name, 5.0)[:, 1]) == {int(round(0.55 * Q)), int(round(1.45 * Q))} and (rows(name, 0.0)[:, 1] == Q).all()
    fill = 1 | 2 << 8 | 3 << 16 | 3 << 24
    ident = ra.row(11, Q, 0, 0, 0, Q, 0, fill)
    for name in ("Rotate", "ShearX", "ShearY", "TranslateX", "TranslateY"):
        assert (rows(name, 0.0, fill=(1, 2, 3)) == ident).all()
    r = rows("TranslateX", 10.0, hw=(20, 40), fill=(1, 2, 3))
    assert set(map(tuple, r)) == {tuple(ra.row(11, Q, 0, s * 18 * Q, 0, Q, 0, fill)) for s in (1, -1)}          # 0.45 of the width, 40
    r = rows("TranslateY", 10.0, hw=(20, 40), fill=(1, 2, 3))
    assert set(map(tuple, r)) == {tuple(ra.row(11, Q, 0, 0, 0, Q, s * 9 * Q, fill)) for s in (1, -1)}
    r = rows("ShearX", 10.0, hw=(20, 40))
    assert set(map(tuple, r[:, 1:7])) == {(Q, s * 19661, -s * 196608, 0, Q, 0) for s in (1, -1)}              # about the centre: -0.3 cy = -3 pixels
    r = rows("ShearY", 10.0, hw=(20, 40))
    assert set(map(tuple, r[:, 1:7])) == {(Q, 0, 0, s * 19661, Q, -s * 393216) for s in (1, -1)}
    r = rows("Rotate", 10.0)                         # 30 degrees about (16, 16); the centre maps to itself
    c30, s30 = int(round(np.cos(np.pi / 6) * Q)), Q // 2
    assert set(map(tuple, r[:, [1, 2, 4, 5]])) == {(c30, -s * s30, s * s30, c30) for s in (1, -1)}
    for p in r:                                      # each entry is off by at most 1/2: 32 / 2 + 32 / 2 + 2 / 2
        assert abs(p[1] * 32 + p[2] * 32 + 2 * p[3] - 32 * Q) <= 33 and abs(p[4] * 32 + p[5] * 32 + 2 * p[6] - 32 * Q) <= 33
    spread = data.randaug_table(4000, 0, 3, (32, 32), n_ops=1, prob=1.0, ops=["Solarize"])[:, 0, 1].numpy()
    m = (256 - spread) / 25.6                        # the magnitude back from the threshold, to 0.04: mean 9, std 0.5, clipped at 10
    assert abs(m.mean() - 9.0) < 0.1 and abs(m.std() - 0.5) < 0.1 and m.max() <= 10.0


@pytest.mark.parametrize("kw", [dict(n=0), dict(hw=(0, 8)), dict(n_ops=0), dict(n_ops=5), dict(magnitude=-1.0), dict(magnitude=10.5), dict(mstd=-0.1),
                                dict(mstd=float("inf")), dict(prob=1.5), dict(ops=[]), dict(ops=["Rotate", "Blur"]), dict(fill=256), dict(fill=(1, 2, 3, 4, 5)),
                                dict(fill=()), dict(fill="grey")])
def test_randaug_table_refuses_bad_arguments(kw):
    from kanvit import data
    args = dict(n=10, epoch=0, seed=0, hw=(8, 8))
    args.update(kw)
    with pytest.raises(ValueError, match="randaug_table"):
        data.randaug_table(**args)


def test_gpu_dataset_randaug_argument_is_checked_before_any_upload():
    from kanvit import data, ops
    x, y = torch.zeros((4, 8, 8, 3), dtype=torch.uint8), torch.zeros(4, dtype=torch.int64)
    for bad, word in ((dict(n_ops=5), "n_ops"), (dict(prob=2.0), "prob"), (dict(count=2), "keys"), (9.0, "dict"), (dict(ops=["Blur"]), "ops")):
        with pytest.raises(ValueError, match=word):
            data.GpuDataset(x, y, [0.5] * 3, [0.25] * 3, "cuda:0", randaug=bad)
    big = torch.zeros((1, 64, 97, 4), dtype=torch.uint8)
    with pytest.raises(ops.KanvitError, match="24576"):
        data.GpuDataset(big, y[:1], [0.5] * 4, [0.25] * 4, "cuda:0", randaug={})


# ---- the restatement against Pillow ---------------------------------------------------------------------------------------------
def _test_images():
    """(name, uint8 [H, W, C]) at 32x32x3 and 28x28 'L': random, a narrow range (so autocontrast and equalize have work), constant."""
    g = np.random.default_rng(5)
    out = []
    for H, W, C in ((32, 32, 3), (28, 28, 1)):
        out.append((f"random{C}", g.integers(0, 256, (H, W, C), dtype=np.uint8)))
        out.append((f"narrow{C}", g.integers(40, 200, (H, W, C), dtype=np.uint8)))
        smooth = (np.add.outer(np.arange(H), np.arange(W))[..., None] * 3 + np.arange(C) * 20 + g.integers(0, 9, (H, W, C))).astype(np.uint8)
        out.append((f"ramp{C}", smooth))
        out.append((f"constant{C}", np.full((H, W, C), 77, np.uint8) + np.arange(C, dtype=np.uint8)))
    return out


def _pil(img):
    from PIL import Image
    return Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)         # "L" from [H, W], "RGB" from [H, W, 3]


def _arr(pil, like):
    return np.asarray(pil).reshape(like.shape)


FACTORS = (0, 6554, Q // 4, 40000, Q, 80000, 124518, 2 * Q)


def test_the_integer_ops_equal_pillows():
    pytest.importorskip("PIL")
    from PIL import ImageOps
    for name, img in _test_images():
        pil = _pil(img)
        assert np.array_equal(ra.apply_op(img, ra.row(ra.INVERT)), _arr(ImageOps.invert(pil), img)), name
        assert np.array_equal(ra.apply_op(img, ra.row(ra.EQUALIZE)), _arr(ImageOps.equalize(pil), img)), name
        for threshold in (0, 1, 77, 128, 200, 255, 256):
            assert np.array_equal(ra.apply_op(img, ra.row(ra.SOLARIZE, threshold)), _arr(ImageOps.solarize(pil, threshold), img)), (name, threshold)
        for bits in range(1, 9):
            assert np.array_equal(ra.apply_op(img, ra.row(ra.POSTERIZE, bits)), _arr(ImageOps.posterize(pil, bits), img)), (name, bits)
        assert not ra.apply_op(img, ra.row(ra.POSTERIZE, 0)).any()
        for add, threshold in ((0, 128), (55, 128), (110, 128), (128, 128), (255, 256), (30, 0)):
            lut = [min(255, i + add) if i < threshold else i for i in range(256)]             # timm's solarize_add
            want = _arr(pil.point(lut * (3 if img.shape[2] == 3 else 1)), img)
            assert np.array_equal(ra.apply_op(img, ra.row(ra.SOLARIZE_ADD, add, threshold)), want), (name, add, threshold)


def test_the_rounded_ops_are_within_one_level_of_pillows():
    """Pillow computes these in floating point and truncates; the restatement rounds in integers: two roundings of one real value."""
    pytest.importorskip("PIL")
    from PIL import ImageEnhance, ImageOps

    def close(a, b):
        return int(np.abs(a.astype(np.int64) - np.asarray(b).astype(np.int64)).max()) <= 1

    for name, img in _test_images():
        pil = _pil(img)
        assert close(ra.apply_op(img, ra.row(ra.AUTOCONTRAST)), _arr(ImageOps.autocontrast(pil), img)), name
        for op, enhance in ((ra.BRIGHTNESS, ImageEnhance.Brightness), (ra.COLOR, ImageEnhance.Color), (ra.CONTRAST, ImageEnhance.Contrast),
                            (ra.SHARPNESS, ImageEnhance.Sharpness)):
            for f in FACTORS:
                assert close(ra.apply_op(img, ra.row(op, f)), _arr(enhance(pil).enhance(f / Q), img)), (name, op, f)
    # and the ops do something: on the random RGB image every one of them changes pixels at f = 0 and at f = 2
    img = _test_images()[0][1]
    for op in (ra.BRIGHTNESS, ra.COLOR, ra.CONTRAST, ra.SHARPNESS):
        assert np.array_equal(ra.apply_op(img, ra.row(op, Q)), img)
        assert (ra.apply_op(img, ra.row(op, 0)) != img).mean() > 0.5 and (ra.apply_op(img, ra.row(op, 2 * Q)) != img).mean() > 0.5


def test_statistics_ops_on_degenerate_images():
    const = np.full((6, 5, 3), 9, np.uint8)
    for op in (ra.AUTOCONTRAST, ra.EQUALIZE):
        assert np.array_equal(ra.apply_op(const, ra.row(op)), const)
    assert np.array_equal(ra.apply_op(const, ra.row(ra.CONTRAST, 0)), const)         # the mean of a constant image is its value
    two = np.where(np.arange(36).reshape(6, 6, 1) % 3 == 0, 50, 180).astype(np.uint8)          # 12 pixels at 50, 24 at 180: step 0
    assert np.array_equal(ra.apply_op(two, ra.row(ra.EQUALIZE)), two)
    big = np.where(np.arange(32 * 32).reshape(32, 32, 1) % 4 == 0, 50, 180).astype(np.uint8)   # 256 at 50, 768 at 180: step 1
    assert sorted(np.unique(ra.apply_op(big, ra.row(ra.EQUALIZE)))) == [0, 255]
    assert sorted(np.unique(ra.apply_op(two, ra.row(ra.AUTOCONTRAST)))) == [0, 255]
    for bad in (ra.row(12), ra.row(-3), ra.row(ra.POSTERIZE, 9), ra.row(ra.SOLARIZE, -1), ra.row(ra.BRIGHTNESS, 2 * Q + 1)):
        assert np.array_equal(ra.apply_op(big, bad), big)
    thin = np.arange(2 * 9 * 3, dtype=np.uint8).reshape(2, 9, 3)                                # H < 3: no interior
    assert np.array_equal(ra.apply_op(thin, ra.row(ra.SHARPNESS, 0)), thin)


# ---- AFFINE, from arithmetic alone --------------------------------------------------------------------------------------------
FILL = 10 | 20 << 8 | 30 << 16 | 40 << 24


def test_affine():
    g = np.random.default_rng(2)
    for H, W, C in ((9, 9, 3), (8, 8, 1), (5, 12, 4)):
        img = g.integers(0, 256, (H, W, C), dtype=np.uint8)
        fill = np.array([10, 20, 30, 40], np.uint8)[:C]
        assert np.array_equal(ra.apply_op(img, ra.row(ra.AFFINE, Q, 0, 0, 0, Q, 0, FILL)), img)
        for tx, ty in ((2, 0), (-3, 1), (0, -4), (W, 0), (1 - W, H - 1)):                     # source = output + (tx, ty)
            want = np.empty_like(img)
            want[:] = fill
            ys, xs = np.arange(H) + ty, np.arange(W) + tx
            oy, ox = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            want[np.ix_(oy, ox)] = img[np.ix_(ys[oy], xs[ox])]
            assert np.array_equal(ra.apply_op(img, ra.row(ra.AFFINE, Q, 0, tx * Q, 0, Q, ty * Q, FILL)), want), (tx, ty)
        for far in (ra.row(ra.AFFINE, Q, 0, 10 * W * Q, 0, Q, 0, FILL), ra.row(ra.AFFINE, Q, 0, 0, 0, Q, -H * Q, FILL),
                    ra.row(ra.AFFINE, 0, 0, -Q, 0, 0, 0, FILL), ra.row(ra.AFFINE, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 0, FILL)):
            assert np.array_equal(ra.apply_op(img, far), np.broadcast_to(fill, img.shape)), far
        if H == W:
            # a quarter turn about the centre: out[y, x] = img[x, n - 1 - y] is np.rot90.  With half-pixel centres every source
            # coordinate is an integer plus 1/2, so nothing is rounded: xs + 1/2 = n - (y + 1/2), ys + 1/2 = x + 1/2.
            n = H
            assert np.array_equal(ra.apply_op(img, ra.row(ra.AFFINE, 0, -Q, n * Q, Q, 0, 0, FILL)), np.rot90(img))
            assert np.array_equal(ra.apply_op(img, ra.row(ra.AFFINE, -Q, 0, n * Q, 0, -Q, n * Q, FILL)), img[::-1, ::-1])      # a half turn
    img = g.integers(0, 256, (4, 6, 1), dtype=np.uint8)                                         # an all-zero map reads pixel (0, 0)
    assert (ra.apply_op(img, ra.row(ra.AFFINE)) == img[0, 0, 0]).all()


def test_chained_rows_feed_each_other():
    g = np.random.default_rng(3)
    x = g.integers(0, 256, (3, 8, 8, 3), dtype=np.uint8)
    table = np.array([[ra.row(ra.INVERT), ra.row(ra.INVERT)], [ra.row(ra.IDENTITY), ra.row(ra.SOLARIZE, 100)],
                      [ra.row(ra.AFFINE, Q, 0, 3 * Q, 0, Q, 0, FILL), ra.row(ra.AUTOCONTRAST)]])
    out = ra.randaugment(x, table)
    assert np.array_equal(out[0], x[0]) and np.array_equal(out[1], ra.apply_op(x[1], table[1][1]))
    assert np.array_equal(out[2], ra.apply_op(ra.apply_op(x[2], table[2][0]), table[2][1])) and not np.array_equal(out[2], ra.apply_op(x[2], table[2][1]))
    assert np.array_equal(ra.randaugment(x[..., 0], table), ra.randaugment(x[..., :1], table)[..., 0])             # [N, H, W] is C = 1


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(lib):
    from kanvit import _lib, build
    header = open(os.path.join(ROOT, "include", "kanvit.h")).read()
    assert "int kanvit_randaug_u8(const uint8_t* src, uint8_t* dst, const int32_t* table, long long N, int H, int W, int C, int K, void* stream);" in header
    codes = {name: int(v) for name, v in re.findall(r"#define KANVIT_RA_(\w+) (\d+)", header)}
    assert codes.pop("MAX_OPS") == _lib.RA_MAX_OPS == 4 and codes.pop("MAX_BYTES") == _lib.RA_MAX_BYTES == ra.MAX_BYTES == 24576
    assert codes == {name.upper(): code for code, name in enumerate(_lib.RA_OP_NAMES)} and len(codes) == ra.N_OPS == 12
    assert all(getattr(_lib, "RA_" + name) == code == getattr(ra, name) for name, code in codes.items())
    Pt = ctypes.c_void_p
    assert _lib.SYMBOLS["kanvit_randaug_u8"] == (ctypes.c_int, [Pt, Pt, Pt, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, Pt])
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "kanvit_randaug_u8")
    assert lib.kanvit_randaug_u8.restype is ctypes.c_int and lib.kanvit_abi_version() == 7 and "#define KANVIT_ABI_VERSION 7" in header
    # randaug.hip is compiled inside the batch_u8 unit (its last line includes it), so it is a dependency of the build, not a source
    assert "randaug.hip" in build.HEADERS and "batch_u8.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "randaug.hip"))
    assert open(os.path.join(build.CSRC, "batch_u8.hip")).read().rstrip().endswith('#include "randaug.hip"')


VALID = dict(src=P, dst=P + 0x100000, table=P + 0x200000, N=10, H=32, W=32, C=3, K=2)
REFUSALS = [
    (dict(N=-1), "kanvit_randaug_u8: N=-1 is negative"),
    (dict(C=0), "kanvit_randaug_u8: C=0 must be in 1..4"),
    (dict(C=5), "kanvit_randaug_u8: C=5 must be in 1..4"),
    (dict(H=0), "kanvit_randaug_u8: H=0, W=32 must be positive"),
    (dict(W=-2), "kanvit_randaug_u8: H=32, W=-2 must be positive"),
    (dict(H=1, W=6145, C=4, N=1), "kanvit_randaug_u8: an image of H=1 x W=6145 x C=4 bytes exceeds 24576 (the image and its copy live in LDS)"),
    (dict(H=2 ** 20, W=2 ** 20, C=4, N=1), "kanvit_randaug_u8: an image of H=1048576 x W=1048576 x C=4 bytes exceeds 24576 (the image and its copy live in LDS)"),
    (dict(K=0), "kanvit_randaug_u8: K=0 must be in 1..4"),
    (dict(K=5), "kanvit_randaug_u8: K=5 must be in 1..4"),
    (dict(src=0), "kanvit_randaug_u8: null src/dst/table"),
    (dict(dst=0), "kanvit_randaug_u8: null src/dst/table"),
    (dict(table=0), "kanvit_randaug_u8: null src/dst/table"),
    (dict(dst=P), "kanvit_randaug_u8: src == dst (an op reads more than the byte it writes; give a second buffer)"),
    (dict(dst=P + 3072 * 10 - 1), "kanvit_randaug_u8: src and dst overlap"),
    (dict(src=P + 3072 * 10 - 1 + 0x100000), "kanvit_randaug_u8: src and dst overlap"),
    (dict(table=P + 0x200002), "kanvit_randaug_u8: table is not aligned to its element size"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=["-".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in REFUSALS])
def test_randaug_u8_refusal_code_and_message(lib, kw, message):
    args = dict(VALID, **kw)
    assert lib.kanvit_randaug_u8(*[(v or None) if k in ("src", "dst", "table") else v for k, v in args.items()], None) == -22
    assert lib.kanvit_last_error().decode() == message


def test_randaug_u8_empty_dataset_returns_0_with_every_pointer_null(lib):
    assert lib.kanvit_randaug_u8(None, None, None, 0, 32, 32, 3, 2, None) == 0
    assert lib.kanvit_randaug_u8(None, None, None, 0, 64, 96, 4, 4, None) == 0                 # exactly 24 576 bytes is a valid shape
    assert lib.kanvit_randaug_u8(None, None, None, 0, 64, 97, 4, 4, None) == -22


def test_wrapper_refuses_cpu_tensors():
    from kanvit import ops
    x, t = torch.zeros((4, 8, 8, 3), dtype=torch.uint8), torch.zeros((4, 2, 8), dtype=torch.int32)
    with pytest.raises(ops.KanvitError, match="no CPU fallback"):
        ops.randaugment_u8(x, t)


# ---- train.parse ----------------------------------------------------------------------------------------------------------------
def test_train_flags():
    import train
    off = train.parse(["--data-npz", "x.npz"])
    assert off.randaug is None and off.randaug_ops == 2 and off.randaug_mstd == 0.5 and off.randaug_prob == 0.5 and train.randaug_config(off) is None
    on = train.parse(["--data-npz", "x.npz", "--randaug"])
    assert on.randaug == 9.0 and train.randaug_config(on) == dict(n_ops=2, magnitude=9.0, mstd=0.5, prob=0.5)
    assert train.randaug_config(on, [0.5071, 0.4867, 0.4408])["fill"] == (129, 124, 112)
    tuned = train.parse(["--data-npz", "x.npz", "--randaug", "7", "--randaug-ops", "3", "--randaug-mstd", "0", "--randaug-prob", "1", "--graph",
                         "--mixup", "0.8", "--resize", "64", "--random-erasing", "0.25", "--device-metrics"])
    assert train.randaug_config(tuned) == dict(n_ops=3, magnitude=7.0, mstd=0.0, prob=1.0)
    assert train.parse(["--randaug", "--data-npz", "x.npz"]).randaug == 9.0                     # the optional value, then another flag
    refused = [(["--randaug"], "--data-npz"),
               (["--synthetic", "--randaug", "5"], "--data-npz"),
               (["--data-npz", "x.npz", "--randaug", "--no-augment"], "--no-augment"),
               (["--data-npz", "x.npz", "--randaug", "11"], "0..10"),
               (["--data-npz", "x.npz", "--randaug", "-1"], "0..10"),
               (["--data-npz", "x.npz", "--randaug", "--randaug-ops", "0"], "--randaug-ops"),
               (["--data-npz", "x.npz", "--randaug", "--randaug-ops", "5"], "--randaug-ops"),
               (["--data-npz", "x.npz", "--randaug", "--randaug-mstd", "-1"], "--randaug-mstd"),
               (["--data-npz", "x.npz", "--randaug", "--randaug-prob", "1.5"], "--randaug-prob")]
    for argv, word in refused:
        with pytest.raises(SystemExit, match=word):
            train.parse(argv)
    assert all(flag in train.__doc__ for flag in ("--randaug [M]", "--randaug-ops", "--randaug-mstd", "--randaug-prob"))
