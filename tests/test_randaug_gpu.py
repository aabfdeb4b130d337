"""ops.randaugment_u8 (csrc/randaug.hip: randaug_u8_kernel) on the GPU against the NumPy integer restatement of tests/_randaug_ref.py --
torch.equal throughout: every op is integer arithmetic.  The shapes are the smallest that reach each path: 32x32x3 and 28x28x1 (16-byte
loads and stores), 6x6x1 (4-byte), 7x5x3 (single bytes, fewer pixels than threads, the sharpness border dominates), 64x64x3 (three
16-byte chunks per thread), 64x96x4 (exactly the 24 576 bytes of the LDS limit), `out` and `src` off the 16-byte grid, one launch past
the grid cap; then GpuDataset(randaug=...) against the existing batch references applied to the restatement's images, and train.main
with --randaug."""
import numpy as np
import pytest
import torch

from tests import _augment_ref as ar
from tests import _erase_ref as er
from tests import _randaug_ref as ra

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, EPOCH = 3, 2
Q = ra.Q16
MEAN, STD = [0.5071, 0.4867, 0.4408, 0.45], [0.2675, 0.2565, 0.2761, 0.25]
MAX_GROUPS = 2048                               # RANDAUG_MAX_GROUPS: past that many images a work-group takes a second one
FILL = 10 | 20 << 8 | 30 << 16 | 200 << 24      # the fourth byte sets the sign bit of p6
FACTORS = (0, 6554, Q // 4, 40000, Q, 80000, 124518, 2 * Q)
SHAPES = [(32, 32, 3), (28, 28, 1), (6, 6, 1), (7, 5, 3), (64, 64, 3)]
_cache = {}


def _images(n, H, W, C, seed):
    """uint8 [n, H, W, C] with something for every statistic: full-range noise, a narrow range, a ramp, four grey levels, and one
    constant image; the extremes 0 and 255 are present."""
    key = ("img", n, H, W, C, seed)
    if key not in _cache:
        g = np.random.default_rng(seed)
        x = g.integers(0, 256, (n, H, W, C), dtype=np.uint8)
        x[1::4] = g.integers(40, 200, x[1::4].shape, dtype=np.uint8)
        ramp = (np.add.outer(np.arange(H), np.arange(W))[None, :, :, None] * 3 + np.arange(C) * 20) % 256
        x[2::4] = (ramp + g.integers(0, 9, x[2::4].shape)).astype(np.uint8)
        x[3::4] = np.array([7, 90, 91, 250], np.uint8)[g.integers(0, 4, x[3::4].shape)]
        if n > 4:
            x[4] = 77
        x.reshape(-1)[:3] = [0, 255, 1]
        _cache[key] = x
    return _cache[key]


def _affine_rows(n, H, W):
    """Per-sample inverse maps about the centre: rotations, shears, translations, a zoom, a flip, one wholly outside, one identity."""
    rows = []
    for s in range(n):
        t = np.radians(15.0 * s - 50.0)
        kind = s % 6
        a, b, d, e, tx, ty = ((np.cos(t), np.sin(t), -np.sin(t), np.cos(t), 0, 0), (1, 0.3 * (s - 5) / 5, 0, 1, 0, 0), (1, 0, -0.25, 1, 0, 0),
                              (1, 0, 0, 1, 0.3 * W * (1 if s % 4 else -1), -0.2 * H), (0.6, 0, 0, 1.7, 0.5, 0), (-1, 0, 0, 1, 0, 0))[kind]
        cx, cy = W / 2, H / 2
        rows.append(ra.row(ra.AFFINE, *(int(np.rint(v * Q)) for v in (a, b, cx - a * cx - b * cy + tx, d, e, cy - d * cx - e * cy + ty)), FILL))
    rows[0] = ra.row(ra.AFFINE, Q, 0, 0, 0, Q, 0, FILL)
    rows[1] = ra.row(ra.AFFINE, Q, 0, 10 * W * Q, 0, Q, 0, FILL)
    return rows


def _op_rows(op, n, H, W):
    """[n, 1, 8]: op alone, with a different parameter for every sample."""
    if op == ra.POSTERIZE:
        rows = [ra.row(op, s % 9) for s in range(n)]
    elif op == ra.SOLARIZE:
        rows = [ra.row(op, (0, 1, 77, 128, 200, 255, 256)[s % 7]) for s in range(n)]
    elif op == ra.SOLARIZE_ADD:
        rows = [ra.row(op, (0, 55, 110, 128, 255)[s % 5], (128, 0, 256, 90)[s % 4]) for s in range(n)]
    elif op in (ra.BRIGHTNESS, ra.COLOR, ra.CONTRAST, ra.SHARPNESS):
        rows = [ra.row(op, FACTORS[(s + s // 8) % 8]) for s in range(n)]
    elif op == ra.AFFINE:
        rows = _affine_rows(n, H, W)
    else:
        rows = [ra.row(op)] * n
    return np.array(rows, np.int64).reshape(n, 1, 8)


def _run(x, table, out=None):
    from kanvit import ops
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    before = xd.clone()
    got = ops.randaugment_u8(xd, torch.as_tensor(np.asarray(table), dtype=torch.int32).contiguous().to(DEV), out=out)
    assert torch.equal(xd, before)                   # src is unchanged
    return got


def _same(got, x, table):
    return torch.equal(got.cpu(), torch.from_numpy(ra.randaugment(x, table)))


# ---- every op alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_every_op_alone(shape):
    H, W, C = shape
    n = 16
    x = _images(n, H, W, C, 11)
    for op in range(ra.N_OPS):
        table = _op_rows(op, n, H, W)
        got = _run(x, table)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, H, W, C)
        assert _same(got, x, table), ra.row(op)
        if C == 1:                                   # [N, H, W] is C = 1
            flat = _run(x[..., 0], table)
            assert tuple(flat.shape) == (n, H, W) and torch.equal(flat, got[..., 0]), op
    # the ops do something here: each of them changes at least one image (COLOR needs three channels, and EQUALIZE 255 pixels
    # beside the last bin's: below that its step is 0)
    for op in range(1, ra.N_OPS):
        if (op == ra.COLOR and C < 3) or (op == ra.EQUALIZE and H * W < 300):
            continue
        table = _op_rows(op, n, H, W)
        assert not np.array_equal(ra.randaugment(x, table), x), op


def test_the_image_that_fills_lds():
    """64 x 96 x 4 = 24 576 bytes exactly: both buffers, four histograms and the scratch are 53 312 bytes of LDS.  C = 4: COLOR passes
    the fourth channel through, the others treat it like any channel."""
    x = _images(2, 64, 96, 4, 5)
    assert x[0].size == ra.MAX_BYTES
    for rows in ([ra.row(ra.EQUALIZE)], [ra.row(ra.SHARPNESS, 2 * Q)], [ra.row(ra.COLOR, 0)], [ra.row(ra.AFFINE, 60000, 20000, 9 * Q, -20000, 60000, 5 * Q, FILL)],
                 [ra.row(ra.EQUALIZE), ra.row(ra.SHARPNESS, 0), ra.row(ra.COLOR, 124518), ra.row(ra.AUTOCONTRAST)]):
        table = np.array([rows, rows[::-1]], np.int64)
        got = _run(x, table)
        assert _same(got, x, table), rows
    colored = _run(x, np.array([[ra.row(ra.COLOR, 0)]] * 2)).cpu().numpy()
    assert np.array_equal(colored[..., 3], x[..., 3]) and not np.array_equal(colored[..., :3], x[..., :3])


def test_a_larger_image_is_refused():
    from kanvit import ops
    x = torch.zeros((1, 1, 6145, 4), dtype=torch.uint8, device=DEV)                 # 24 580 bytes
    t = torch.zeros((1, 1, 8), dtype=torch.int32, device=DEV)
    with pytest.raises(ops.KanvitError, match="24576"):
        ops.randaugment_u8(x, t)
    with pytest.raises(ops.KanvitError, match="24576"):
        ops.randaugment_u8(torch.zeros((2, 128, 128, 3), dtype=torch.uint8, device=DEV), t.expand(2, 1, 8).contiguous())
    assert tuple(ops.randaugment_u8(torch.zeros((1, 1, 6144, 4), dtype=torch.uint8, device=DEV), t).shape) == (1, 1, 6144, 4)


def test_edge_parameters():
    n, (H, W, C) = 24, (32, 32, 3)
    x = _images(n, H, W, C, 23).copy()
    x[5] = np.where(np.arange(H * W).reshape(H, W, 1) % 4 == 0, 50, 180)            # exactly two grey levels, 256 and 768 pixels: step 1
    x[6] = np.where(np.arange(H * W).reshape(H, W, 1) % 3 == 0, 50, 180)            # 342 and 682 pixels: step 1 as well, another table
    x[7, :, :, 1] = 200                              # one constant channel among two that are not
    rows = [ra.row(ra.POSTERIZE, 0), ra.row(ra.POSTERIZE, 8), ra.row(ra.SOLARIZE, 0), ra.row(ra.SOLARIZE, 256),
            *(ra.row(op, f) for op in (ra.BRIGHTNESS, ra.COLOR, ra.CONTRAST, ra.SHARPNESS) for f in (0, 2 * Q)),
            ra.row(ra.AFFINE, Q, 0, 10 * W * Q, 0, Q, 0, FILL), ra.row(ra.AFFINE, *([-2 ** 31] * 7)), ra.row(ra.AFFINE, *([2 ** 31 - 1] * 7)),
            # unknown op codes and parameters outside their range: the identity
            ra.row(12), ra.row(-1), ra.row(2 ** 31 - 1), ra.row(-2 ** 31), ra.row(ra.POSTERIZE, 9), ra.row(ra.POSTERIZE, -1), ra.row(ra.SOLARIZE, 257),
            ra.row(ra.SOLARIZE_ADD, 256, 128), ra.row(ra.SOLARIZE_ADD, 10, 257), ra.row(ra.BRIGHTNESS, 2 * Q + 1), ra.row(ra.COLOR, -1),
            ra.row(ra.CONTRAST, 2 ** 31 - 1), ra.row(ra.SHARPNESS, -2 ** 31)]
    for r in rows:
        table = np.array([[r]] * n, np.int64)
        got = _run(x, table)
        assert _same(got, x, table), r
        if not ra.row_is_valid(r):
            assert torch.equal(got.cpu(), torch.from_numpy(x)), r
    for op in (ra.AUTOCONTRAST, ra.EQUALIZE, ra.CONTRAST):
        got = _run(x, np.array([[ra.row(op, 0)]] * n)).cpu().numpy()
        assert np.array_equal(got[4], x[4]), op                                      # the constant image
    eq = _run(x, np.array([[ra.row(ra.EQUALIZE)]] * n)).cpu().numpy()
    assert sorted(np.unique(eq[5])) == [0, 255] and np.array_equal(eq, ra.randaugment(x, np.array([[ra.row(ra.EQUALIZE)]] * n)))
    outside = _run(x, np.array([[rows[12]]] * n)).cpu().numpy()
    assert np.array_equal(outside, np.broadcast_to(np.array([10, 20, 30], np.uint8), x.shape))


@pytest.mark.parametrize("K", [2, 3, 4])
def test_chains_read_the_previous_ops_output(K):
    """Mixed per-sample ops.  A statistics op follows an AFFINE (its fill enters the histogram) and a SHARPNESS follows an EQUALIZE
    (the neighbours it reads are equalised ones): the result differs from the same op applied to src."""
    from kanvit import data
    for H, W, C in ((32, 32, 3), (7, 5, 3), (28, 28, 1)):
        n = 20
        x = _images(n, H, W, C, 31 + K)
        table = data.randaug_table(n, EPOCH, SEED, (H, W), n_ops=K, prob=0.8, fill=(10, 20, 30)).numpy().astype(np.int64)
        shift = ra.row(ra.AFFINE, Q, 0, (W // 2) * Q, 0, Q, 0, FILL)
        table[0, :2] = [shift, ra.row(ra.AUTOCONTRAST)]
        table[1, :2] = [ra.row(ra.EQUALIZE), ra.row(ra.SHARPNESS, 0)]
        table[2, :2] = [shift, ra.row(ra.CONTRAST, 0)]
        table[3] = [ra.row(ra.INVERT)] * K                                           # K inversions
        table[4] = [ra.row(ra.IDENTITY)] * K                                         # nothing at all
        table[5] = [ra.row(ra.IDENTITY)] * (K - 1) + [ra.row(ra.EQUALIZE)]
        table[6] = [ra.row(ra.SOLARIZE, 100)] + [ra.row(ra.IDENTITY)] * (K - 1)    # an op, then identities up to the store
        table[7] = [ra.row(ra.SHARPNESS, 2 * Q), ra.row(99)] + [ra.row(ra.SHARPNESS, 2 * Q)] * (K - 2)          # an unknown code in the middle
        got = _run(x, table)
        assert _same(got, x, table), (H, W, C)
        want = got.cpu().numpy()
        assert np.array_equal(want[3], x[3] if K % 2 == 0 else 255 - x[3]) and np.array_equal(want[4], x[4])
        if K == 2 and (H, W) == (32, 32):
            for s in (0, 1, 2):
                assert not np.array_equal(want[s], ra.apply_op(x[s], table[s][1])), s   # not the second op on src


def test_more_images_than_work_groups():
    """N = the grid cap + 3: the first three work-groups take a second image."""
    from kanvit import data
    n = MAX_GROUPS + 3
    x = _images(n, 8, 8, 1, 41)
    table = data.randaug_table(n, EPOCH, SEED, (8, 8), prob=1.0, fill=77).numpy()
    table[-1] = [ra.row(ra.INVERT), ra.row(ra.POSTERIZE, 3)]
    got = _run(x, table)
    assert _same(got, x, table)
    assert torch.equal(got[-1].cpu(), torch.from_numpy((255 - x[-1]) & 0xE0))


def test_out_is_honoured_at_every_alignment():
    from kanvit import ops
    n, (H, W, C) = 6, (32, 32, 3)
    x = _images(n, H, W, C, 51)
    table = np.array([[ra.row(ra.SHARPNESS, 2 * Q), ra.row(ra.EQUALIZE)], [ra.row(ra.AFFINE, 60000, 20000, 0, -20000, 60000, 0, FILL), ra.row(ra.COLOR, 0)]] * 3)
    want = torch.from_numpy(ra.randaugment(x, table))
    for offset in (0, 16, 4, 1, 3):                  # 16-byte, 4-byte and single-byte stores
        buf = torch.full((x.size + 32,), 0xAB, dtype=torch.uint8, device=DEV)
        out = buf[offset:offset + x.size].view(n, H, W, C)
        assert out.data_ptr() % 16 == offset % 16
        got = _run(x, table, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(got.cpu(), want), offset
        assert bool((buf[:offset] == 0xAB).all()) and bool((buf[offset + x.size:] == 0xAB).all()), offset        # nothing outside it
    xd, td = torch.from_numpy(x).to(DEV), torch.as_tensor(table, dtype=torch.int32).to(DEV)
    src = torch.zeros(x.size + 4, dtype=torch.uint8, device=DEV)[1:1 + x.size].view(n, H, W, C).copy_(xd)        # src off the 16-byte grid too
    assert src.data_ptr() % 4 == 1 and torch.equal(ops.randaugment_u8(src, td).cpu(), want)
    for bad, word in ((dict(out=xd), "out is images"), (dict(out=torch.empty((n, H, W, C), dtype=torch.int8, device=DEV)), "out has dtype"),
                      (dict(out=torch.empty((n, H, W), dtype=torch.uint8, device=DEV)), "out has shape"), (dict(out=torch.empty_like(xd).cpu()), "out is on cpu")):
        with pytest.raises(ops.KanvitError, match=word):
            ops.randaugment_u8(xd, td, **bad)
    with pytest.raises(ops.KanvitError, match="overlap"):
        big = torch.zeros(2 * x.size, dtype=torch.uint8, device=DEV)
        ops.randaugment_u8(big[:x.size].view(n, H, W, C), td, out=big[16:16 + x.size].view(n, H, W, C))
    for bad, word in ((td.long(), "table has dtype"), (td[:, :, :7].contiguous(), "table has shape"), (td[:5], "table has shape"), (td.cpu(), "table is on cpu"),
                      (torch.zeros((n, 5, 8), dtype=torch.int32, device=DEV), "table has shape")):
        with pytest.raises(ops.KanvitError, match=word):
            ops.randaugment_u8(xd, bad)


# ---- GpuDataset(randaug=...) ----------------------------------------------------------------------------------------------------
N_DS = 40
RANDAUG = dict(n_ops=2, magnitude=9.0, mstd=0.5, prob=0.7, fill=(129, 124, 112))
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5)


def _ds():
    if "ds" not in _cache:
        images = torch.from_numpy(_images(N_DS, 8, 8, 3, 8))
        _cache["ds"] = (images, (torch.arange(N_DS) * 5 + 1) % 11)
    return _cache["ds"]


def _augmented(epoch, seed):
    """The restatement's augmented copy of the dataset for one epoch (uint8 [N, 8, 8, 3], NumPy), from the table data.py documents."""
    from kanvit import data
    key = ("aug", epoch, seed)
    if key not in _cache:
        _cache[key] = ra.randaugment(_ds()[0].numpy(), data.randaug_table(N_DS, epoch, seed, (8, 8), **RANDAUG).numpy())
    return _cache[key]


def test_gpu_dataset_padded_crop_reads_the_augmented_copy():
    from kanvit import data
    images, labels = _ds()
    gd = data.GpuDataset(images, labels, MEAN[:3], STD[:3], DEV, pad=2, flip=True, randaug=RANDAUG)
    assert not gd.resample and gd.randaug_buffer is not None and gd.randaug_buffer.shape == gd.images.shape
    assert gd.randaug_buffer.dtype == torch.uint8 and gd.randaug_buffer.data_ptr() != gd.images.data_ptr()
    aug = _augmented(EPOCH, SEED)
    assert 5 < int((aug != images.numpy()).any(axis=(1, 2, 3)).sum()) < N_DS         # the epoch changes some samples and leaves some
    by_sample = {}
    for bs in (4, 7):
        order = data.epoch_indices(N_DS, EPOCH, SEED).tolist()
        fed = list(gd.batches(bs, EPOCH, SEED))
        assert sum(b[0].shape[0] for b in fed) == N_DS
        x, y = torch.cat([b[0] for b in fed]).cpu(), torch.cat([b[1] for b in fed]).cpu()
        assert torch.equal(x, ar.augment(torch.from_numpy(aug), order, MEAN[:3], STD[:3], 2, True, SEED, EPOCH)) and torch.equal(y, labels[order])
        by_sample[bs] = dict(zip(order, x))
    assert all(torch.equal(by_sample[4][s], by_sample[7][s]) for s in range(N_DS))  # the same sample, the same pixels
    assert torch.equal(gd.images.cpu(), images)                                      # the stored images are never written
    assert torch.equal(gd.randaug_buffer.cpu(), torch.from_numpy(aug))
    other = torch.cat([b[0] for b in gd.batches(7, EPOCH + 1, SEED)]).cpu()          # another epoch: another table, the same buffer
    order = data.epoch_indices(N_DS, EPOCH + 1, SEED).tolist()
    assert torch.equal(other, ar.augment(torch.from_numpy(_augmented(EPOCH + 1, SEED)), order, MEAN[:3], STD[:3], 2, True, SEED, EPOCH + 1))
    halves = {}
    for rank in (0, 1):                              # every rank augments the whole dataset
        order = data.epoch_indices(N_DS, EPOCH, SEED, rank, 2).tolist()
        halves.update(zip(order, torch.cat([b[0] for b in gd.batches(7, EPOCH, SEED, rank, 2)]).cpu()))
    assert all(torch.equal(halves[s], by_sample[7][s]) for s in range(N_DS))


def test_gpu_dataset_resize_erase_and_mixup_read_the_augmented_copy():
    """out_size, Random Erasing and Mixup / CutMix together: the existing references applied to the restatement's images.  The partner
    is gathered from the same copy, so it appears under its own randaug rows."""
    from kanvit import data
    images, labels = _ds()
    out = (16, 16)
    gd = data.GpuDataset(images, labels, MEAN[:3], STD[:3], DEV, pad=2, flip=True, out_size=out, erase=dict(prob=0.5, mode="pixel"), randaug=RANDAUG)
    aug = _augmented(EPOCH, SEED)
    crop = data.crop_table(N_DS, EPOCH, SEED, (8, 8), "pad", pad=2, flip=True).numpy()
    erase = data.erase_table(N_DS, EPOCH, SEED, out, prob=0.5).numpy()
    want = er.reference(aug, MEAN[:3], STD[:3], crop, out, erase, data.normal_table(4096).numpy(), data.erase_noise_key(SEED, EPOCH))
    tables = tuple(t.numpy() for t in data.mix_table(N_DS, EPOCH, SEED, out, **MIX))
    order = data.epoch_indices(N_DS, EPOCH, SEED).tolist()
    pad_value = data.make_lut(MEAN[:3], STD[:3])[:, 0].numpy()
    fed = list(gd.batches(16, EPOCH, SEED, mix=MIX))
    assert [b[0].shape[0] for b in fed] == [16, 16, 8] and all(len(b) == 4 for b in fed)
    for i, b in enumerate(fed):
        ref = er.batch(want, pad_value, order[16 * i:16 * i + 16], labels, tables)
        assert all(torch.equal(g.cpu(), torch.from_numpy(np.asarray(w))) for g, w in zip(b, ref)), i
    plain = er.reference(images.numpy(), MEAN[:3], STD[:3], crop, out, erase, data.normal_table(4096).numpy(), data.erase_noise_key(SEED, EPOCH))
    assert not np.array_equal(want, plain)


def test_gpu_dataset_without_randaug_is_the_parents():
    from kanvit import data, ops
    images, labels = _ds()
    gd = data.GpuDataset(images, labels, MEAN[:3], STD[:3], DEV, pad=2, flip=True)
    assert gd.randaug is None and gd.randaug_buffer is None
    assert gd._epoch_images(EPOCH, SEED) is gd.images                                # the batch ops get the stored images themselves
    order = data.epoch_indices(N_DS, EPOCH, SEED)
    fed = list(gd.batches(16, EPOCH, SEED))
    for i, (x, y) in enumerate(fed):
        idx = order[16 * i:16 * i + 16]
        px, py = ops.augment_u8(gd.images, gd.labels, idx.to(DEV), gd.lut, 2, True, SEED, EPOCH)
        assert torch.equal(x, px) and torch.equal(y, py)
        assert torch.equal(x.cpu(), ar.augment(images, idx.tolist(), MEAN[:3], STD[:3], 2, True, SEED, EPOCH))


# ---- train.main -------------------------------------------------------------------------------------------------------------------
TRAIN = ["--model-type", "cheby", "--n-patches", "2", "--n-blocks", "2", "--n-heads", "2", "--d-hidden", "64", "--out-d", "4",
         "--batch-size", "32", "--crop-padding", "2", "--no-tuned-gemms", "--epochs", "1"]       # the geometry of tests/test_gpu_data_gpu.py


@pytest.fixture(scope="module")
def npz_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("npz") / "tiny.npz")
    x = _images(80, 8, 8, 3, 8)
    np.savez(path, x_train=x[:64], y_train=(np.arange(64) % 4).astype(np.uint8), x_test=x[64:], y_test=(np.arange(16) % 4).astype(np.uint8))
    return path


def test_train_main_with_randaug(npz_file, tmp_path):
    import train
    runs = {}
    for name, extra in (("a", ["--randaug", "--graph"]), ("b", ["--randaug", "--graph"]), ("plain", ["--graph"]), ("eager", ["--randaug"])):
        runs[name] = train.main(train.parse([*TRAIN, "--data-npz", npz_file, *extra, "--log-dir", str(tmp_path / name)]))["losses"]
    assert len(runs["a"]) == 2 and all(np.isfinite(runs["a"]))                       # two steps of 32 out of 64 images
    assert runs["a"] == runs["b"] and runs["a"] != runs["plain"] and runs["a"] == runs["eager"]


def test_train_main_feeds_the_datasets_batches_and_leaves_the_test_split_alone(npz_file, tmp_path):
    import train
    from kanvit import data
    args = train.parse([*TRAIN, "--data-npz", npz_file, "--randaug", "7", "--randaug-ops", "3", "--randaug-prob", "0.9", "--log-dir", str(tmp_path / "a")])
    train_set, test_set = train.npz_datasets(args, torch.device(DEV))
    mean = data.channel_stats(np.load(npz_file)["x_train"])[0]
    assert train_set.randaug == dict(n_ops=3, magnitude=7.0, mstd=0.5, prob=0.9, fill=tuple(int(round(255 * float(m))) for m in mean), ops=None)
    assert test_set.randaug is None and test_set.randaug_buffer is None
    plain_args = train.parse([*TRAIN, "--data-npz", npz_file, "--log-dir", str(tmp_path / "p")])
    plain_train, plain_test = train.npz_datasets(plain_args, torch.device(DEV))
    assert plain_train.randaug is None and plain_train.randaug_buffer is None
    for (x, y), (px, py) in zip(test_set.loader(32, shuffle=False), plain_test.loader(32, shuffle=False)):
        assert torch.equal(x, px) and torch.equal(y, py)
    run = train.main(args)
    fed = list(train_set.batches(32, 0, args.seed))
    synthetic = train.parse([*TRAIN, "--synthetic", "--image-size", "8", "--log-dir", str(tmp_path / "b")])
    assert train.main(synthetic, batches=fed)["losses"] == run["losses"]
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(fed, plain_train.batches(32, 0, args.seed)))


def test_train_refuses_randaug_without_its_dataset():
    import train
    with pytest.raises(SystemExit, match="--randaug augments a second copy of the GPU-resident dataset once per epoch; give --data-npz"):
        train.parse([*TRAIN, "--randaug"])
    with pytest.raises(SystemExit, match="--randaug is an augmentation; it is not combined with --no-augment"):
        train.parse([*TRAIN, "--data-npz", "x.npz", "--randaug", "--no-augment"])
