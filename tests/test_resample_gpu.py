"""ops.resample_u8 (csrc/batch_u8.hip: resample_u8_kernel) on the GPU against the float32 restatement of tests/_resample_ref.py --
BITWISE: the kernel's fp32 operation sequence is fixed and never contracted, and NumPy's float32 operations repeat it.  The shapes
are the smallest that reach each form and edge: 8x8x3 -> 20x20 (16-byte stores, boxes over every edge), 7x9x1 -> 12x10 (the scalar
form), a hand-made table of degenerate boxes, a downscale, the identity size against ops.augment_u8 / ops.mix_u8, mixing with the
partner under its own crop row, and one batch past the grid cap.  Then GpuDataset and train.main with --resize."""
import re

import numpy as np
import pytest
import torch

from tests import _mix_ref as mr
from tests import _resample_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, SEED, EPOCH = 40, 3, 2
MEAN, STD = [0.5071, 0.4867, 0.4408, 0.45], [0.2675, 0.2565, 0.2761, 0.25]
GRID_ITEMS = 2048 * 256                         # the launch's cap: 2048 work-groups of 256 work items
_cache = {}


def _images(n, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, H, W, C), dtype=torch.uint8, generator=g)
    x.view(-1)[:3] = torch.tensor([0, 255, 1], dtype=torch.uint8)
    return x[..., 0].contiguous() if C == 1 else x


def _case(shape, out_hw, pad):
    """Dataset, pad-mode crop table, device copies and the restatement of every sample, computed once and left unchanged."""
    key = (shape, out_hw, pad)
    if key not in _cache:
        from kanvit import data
        H, W, C = shape
        images, labels = _images(N, H, W, C, 100 * H + 10 * W + C), (torch.arange(N) * 5 + 1) % 11
        crop = data.crop_table(N, EPOCH, SEED, (H, W), "pad", pad=pad, flip=True)
        _cache[key] = dict(images=images, labels=labels, crop=crop, C=C,
                           want=torch.from_numpy(rr.resample_all(images.numpy(), MEAN[:C], STD[:C], crop.numpy(), out_hw)),
                           dev=dict(images=images.to(DEV), labels=labels.to(DEV), lut=data.make_lut(MEAN[:C], STD[:C]).to(DEV), crop=crop.to(DEV)))
    return _cache[key]


def _run(c, idx, out_hw, crop="own", tables=(), labels=True, out=None):
    from kanvit import ops
    d = c["dev"]
    return ops.resample_u8(d["images"], d["labels"] if labels else None, torch.as_tensor(idx, dtype=torch.int64).to(DEV), d["lut"], out_hw,
                           d["crop"] if isinstance(crop, str) else crop, *tables, out=out)


def test_padded_crops_upsampled_with_16_byte_stores():
    """40 images of 8x8x3 -> 20x20 under the pad-2 table: boxes reach over every edge, so padding taps are blended with image taps."""
    c = _case((8, 8, 3), (20, 20), (2, 2))
    rows = c["crop"].numpy()
    assert {-2, 2} <= set(rows[:, 0].tolist()) and {-2, 2} <= set(rows[:, 1].tolist()) and set(rows[:, 4].tolist()) == {0, 1}
    idx = list(range(N))
    x, y = _run(c, idx, (20, 20))
    assert x.shape == (N, 3, 20, 20) and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0
    assert torch.equal(x.cpu(), c["want"])
    assert torch.equal(y.cpu(), c["labels"])
    assert torch.equal(_run(c, idx, (20, 20), labels=False).cpu(), c["want"])        # without labels: x alone


def test_one_channel_odd_width_takes_the_scalar_form():
    c = _case((7, 9, 1), (12, 10), (3, 2))
    assert c["images"].dim() == 3
    x, _ = _run(c, list(range(N)), (12, 10))
    assert x.shape == (N, 1, 12, 10) and torch.equal(x.cpu(), c["want"])


HAND = [(3, 4, 1, 1, 0),            # 0: one pixel
        (2, 1, 1, 5, 0),            # 1: one row
        (1, 6, 6, 1, 1),            # 2: one column, flipped
        (0, 0, 8, 8, 0),            # 3: the whole image
        (-20, 3, 12, 12, 0),        # 4: wholly outside, at the output's own size: the second weights are 0, so lut[c][0] exactly
        (9, 9, 5, 7, 1),            # 5: wholly outside, resized
        (5, -3, 6, 6, 0),           # 6: half outside
        (1, 2, 5, 4, 0),            # 7 and 8: twins, unflipped and flipped
        (1, 2, 5, 4, 1),
        (2, 2, 0, 4, 0),            # 9: no rows: padding, nothing is read
        (2, 2, 3, 0, 1),            # 10: no columns
        (-1, -1, 10, 10, 1)]        # 11: the image with a one-pixel frame of padding


def test_hand_made_boxes():
    from kanvit import data
    images, C, out = _images(len(HAND), 8, 8, 3, 7), 3, (12, 12)
    table = np.array(HAND, np.int32)
    want = rr.resample_all(images.numpy(), MEAN[:C], STD[:C], table, out)
    c = dict(dev=dict(images=images.to(DEV), labels=None, lut=data.make_lut(MEAN[:C], STD[:C]).to(DEV), crop=torch.from_numpy(table).to(DEV)))
    x = _run(c, list(range(len(HAND))), out, labels=False).cpu()
    assert torch.equal(x, torch.from_numpy(want))
    pad = data.make_lut(MEAN[:C], STD[:C])[:, 0]
    for row in (4, 9, 10):
        assert torch.equal(x[row], pad[:, None, None].expand(3, 12, 12)), row
    one = rr.lut(MEAN[:C], STD[:C])[np.arange(3), images[0, 3, 4].numpy()][:, None, None]      # row 0: one tap under every weight pair
    assert np.abs(want[0] - one).max() <= 6 * np.spacing(np.abs(one).max())       # 1 - w, two products' sums: six roundings of 2^-24
    assert not torch.equal(x[7], x[8])
    mirrored = rr.resample_all(images.numpy()[:, :, ::-1], MEAN[:C], STD[:C], np.array([(1, 2, 5, 4, 0)] * len(HAND), np.int32), out)
    assert np.array_equal(want[8], mirrored[8])                     # the flipped twin is the unflipped box of the mirrored image


@pytest.mark.parametrize("out", [(5, 5), (6, 8)])
def test_downscale(out):
    """No antialiasing: taps are skipped.  Both heights end in a short group of rows (a work item is four rows): 5 = 4 + 1 in the scalar
    form, 6 = 4 + 2 with 16-byte stores."""
    c = _case((8, 8, 3), out, (2, 2))
    x, _ = _run(c, list(range(N)), out)
    assert x.shape == (N, 3, *out) and torch.equal(x.cpu(), c["want"])


def test_no_table_is_the_whole_image_unflipped():
    c = _case((8, 8, 3), (20, 20), (2, 2))
    idx = list(range(N))
    whole = torch.tensor([[0, 0, 8, 8, 0]] * N, dtype=torch.int32, device=DEV)
    x = _run(c, idx, (20, 20), crop=None)[0]
    assert torch.equal(x, _run(c, idx, (20, 20), crop=whole)[0])
    assert torch.equal(x.cpu(), torch.from_numpy(rr.resample_all(c["images"].numpy(), MEAN[:3], STD[:3], None, (20, 20))))
    assert not torch.equal(x.cpu(), c["want"])


@pytest.mark.parametrize("shape,pad", [((8, 8, 3), (2, 2)), ((7, 9, 1), (3, 2))])
def test_identity_size_is_augment_u8_bitwise(shape, pad):
    from kanvit import ops
    H, W, _ = shape
    c = _case(shape, (H, W), pad)
    d, idx = c["dev"], torch.arange(N - 1, -1, -1, device=DEV)
    x, y = _run(c, idx, (H, W))
    ax, ay = ops.augment_u8(d["images"], d["labels"], idx, d["lut"], pad, True, SEED, EPOCH)
    assert torch.equal(x, ax) and torch.equal(y, ay)
    assert torch.equal(x.cpu(), c["want"].flip(0))


def test_identity_size_with_mix_tables_is_mix_u8_bitwise():
    from kanvit import ops
    pad = (2, 2)
    c = _case((8, 8, 3), (8, 8), pad)
    d, idx = c["dev"], torch.arange(N, device=DEV)
    tables = [torch.from_numpy(t).to(DEV) for t in mr.hand_table(N, 8, 8, seed=16)]
    got = _run(c, idx, (8, 8), tables=tables)
    want = ops.mix_u8(d["images"], d["labels"], idx, d["lut"], *tables, pad=pad, flip=True, seed=SEED, epoch=EPOCH)
    assert len(got) == 4 and all(torch.equal(g, w) for g, w in zip(got, want))
    assert bool((got[2] != got[1]).any()) and bool(((got[3] > 0) & (got[3] < 1)).any())


def test_mixing_takes_the_partner_under_its_own_crop_row():
    """8x8x3 -> 20x20 against tests/_mix_ref.mix over the resampled-all array.  The hand table's rows: Mixup at w = 0, 0.3, 1, a
    sample partnered with itself, a full box, a one-pixel box, and the box (0, 10, 17, 20), which starts inside the four-pixel store
    group 16..19."""
    c = _case((8, 8, 3), (20, 20), (2, 2))
    table = mr.hand_table(N, 20, 20, seed=40)
    assert table[0][4] == 4 and tuple(table[2][7]) == (0, 10, 17, 20) and table[2][7][2] % 4 != 0
    rng = np.random.default_rng(1)
    idx = np.concatenate([rng.permutation(N), rng.permutation(N)[:9]]).tolist()
    x, y, y2, w = _run(c, idx, (20, 20), tables=[torch.from_numpy(t).to(DEV) for t in table])
    want = mr.mix(c["want"].numpy(), c["labels"].numpy(), idx, *table)
    assert torch.equal(x.cpu(), torch.from_numpy(want[0]))
    assert np.array_equal(y.cpu().numpy(), want[1]) and np.array_equal(y2.cpu().numpy(), want[2])
    assert np.array_equal(w.cpu().numpy().view(np.uint32), want[3].view(np.uint32))
    plain = c["want"].numpy()
    j = int(table[0][5])                                            # row 5: the full box -- the partner's own crop, not the sample's
    assert np.array_equal(want[0][idx.index(5)], plain[j]) and not np.array_equal(plain[j], plain[5])


def test_batch_past_the_grid_cap_wraps_the_stride_loop():
    """A work item is 4 rows by 4 columns, so B = 56, C = 3 at 224x224 is 526 848 items against the 524 288 of a full grid: the last
    items -- the end of the last sample's last plane -- are reached through the carried (b, c, og, xg) digits.  The restatement is
    computed for the first and the last two samples; every sample is compared with its own one-sample batch (a launch far below the
    cap, the kind the tests above hold against the restatement)."""
    B, out = 56, (224, 224)
    assert B * 3 * (224 // 4) * (224 // 4) > GRID_ITEMS
    c = _case((8, 8, 3), (20, 20), (2, 2))
    idx = (list(range(N)) + list(range(N)))[3:3 + B]
    x, y = _run(c, idx, out)
    assert torch.equal(y.cpu(), c["labels"][idx])
    ends = [0, B - 2, B - 1]
    want = rr.resample_all(c["images"].numpy()[[idx[b] for b in ends]], MEAN[:3], STD[:3], c["crop"].numpy()[[idx[b] for b in ends]], out)
    assert torch.equal(x[ends].cpu(), torch.from_numpy(want))
    for b in range(B):
        assert torch.equal(x[b:b + 1], _run(c, idx[b:b + 1], out)[0]), b


def test_pixels_do_not_depend_on_the_batch_or_the_position():
    c = _case((8, 8, 3), (20, 20), (2, 2))
    tables = [torch.from_numpy(t).to(DEV) for t in mr.hand_table(N, 20, 20, seed=40)]
    for tb in ((), tables):
        whole = _run(c, list(range(N)), (20, 20), tables=tb)[0]
        for idx in ([2], [5, 2, 6, 0, 7], [7, 7, 36, 2], list(range(N - 1, -1, -1))):
            assert torch.equal(_run(c, idx, (20, 20), tables=tb)[0], whole[idx])
    x, y = _run(c, [], (20, 20))
    assert x.shape == (0, 3, 20, 20) and y.shape == (0,)
    assert all(t.shape[0] == 0 for t in _run(c, [], (20, 20), tables=tables))


def test_output_off_the_16_byte_grid_takes_the_scalar_form():
    c = _case((8, 8, 3), (20, 20), (2, 2))
    n = 9 * 3 * 20 * 20
    buf = torch.full((n + 5,), float("nan"), device=DEV)
    view = buf[1:n + 1].view(9, 3, 20, 20)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got = _run(c, list(range(9)), (20, 20), labels=False, out=view)
    assert got.data_ptr() == view.data_ptr()
    assert torch.equal(view.cpu(), c["want"][:9])
    rest = buf.cpu()
    assert torch.isnan(rest[0]) and torch.isnan(rest[n + 1:]).all()         # nothing written outside the view


def test_wrapper_checks_its_operands():
    from kanvit import KanvitError
    c = _case((8, 8, 3), (20, 20), (2, 2))
    d = c["dev"]
    p, w, box = (torch.from_numpy(t).to(DEV) for t in mr.hand_table(N, 20, 20, seed=40))
    with pytest.raises(KanvitError, match="crop"):
        _run(c, [0], (20, 20), crop=d["crop"].long())
    with pytest.raises(KanvitError, match="crop"):
        _run(c, [0], (20, 20), crop=d["crop"][:, :4].contiguous())
    with pytest.raises(KanvitError, match="contiguous"):
        _run(c, [0], (20, 20), crop=d["crop"].t().contiguous().t())
    with pytest.raises(KanvitError, match="come together"):
        _run(c, [0], (20, 20), tables=(p, w))
    with pytest.raises(KanvitError, match="weight"):
        _run(c, [0], (20, 20), tables=(p, w[:5], box))
    with pytest.raises(KanvitError, match="labels"):
        _run(c, [0], (20, 20), tables=(p, w, box), labels=False)
    with pytest.raises(KanvitError, match="OH=0"):
        _run(c, [0], (0, 20))
    with pytest.raises(KanvitError, match="out_size"):
        _run(c, [0], None)
    with pytest.raises(KanvitError, match="out has shape"):
        _run(c, [0], (20, 20), out=torch.empty(1, 3, 20, 24, device=DEV))
    with pytest.raises(KanvitError, match="cpu"):
        _run(c, [0], (20, 20), crop=c["crop"])


def test_dataset_with_random_resized_crops():
    """GpuDataset(out_size=(20, 20), crop="rrc"): an epoch covers the dataset, the batches are the restatement fed crop_table, another
    epoch differs; with out_size=None and crop="pad" the dataset yields what it yields today."""
    from kanvit import data
    images, labels = _images(50, 8, 8, 3, 6), torch.arange(50)
    ds = data.GpuDataset(images, labels, MEAN[:3], STD[:3], DEV, pad=2, flip=True, out_size=(20, 20), crop="rrc")
    assert ds.resample and ds.out_hw == (20, 20) and ds.chw == (3, 8, 8)
    got = list(ds.batches(16, epoch=3, seed=11))
    assert [len(y) for _, y in got] == [16, 16, 16, 2]
    ys = torch.cat([y for _, y in got]).cpu()
    assert torch.equal(ys, data.epoch_indices(50, 3, 11)) and sorted(ys.tolist()) == list(range(50))
    table = data.crop_table(50, 3, 11, (8, 8), "rrc")
    want = torch.from_numpy(rr.resample_all(images.numpy(), MEAN[:3], STD[:3], table.numpy(), (20, 20)))
    x = torch.cat([x for x, _ in got]).cpu()
    assert x.shape == (50, 3, 20, 20) and torch.equal(x, want[ys])
    other = torch.cat([b[0] for b in ds.batches(16, epoch=4, seed=11)]).cpu()
    assert not torch.equal(other[torch.argsort(data.epoch_indices(50, 4, 11))], want)
    halves = [list(ds.batches(16, epoch=3, seed=11, rank=r, world=2)) for r in range(2)]
    x2 = torch.stack([torch.cat([b[0] for b in h]) for h in halves], 1).reshape(50, 3, 20, 20).cpu()
    assert torch.equal(x2, want[ys])                                # two ranks: the same pixels per sample
    mixed = list(ds.batches(16, epoch=3, seed=11, mix=dict(mixup_alpha=0.8, cutmix_alpha=1.0)))
    mt = data.mix_table(50, 3, 11, (20, 20), mixup_alpha=0.8, cutmix_alpha=1.0)          # drawn at the output size
    mw = mr.mix(want.numpy(), labels.numpy(), ys.tolist(), *(t.numpy() for t in mt))
    assert all(len(b) == 4 for b in mixed) and torch.equal(torch.cat([b[0] for b in mixed]).cpu(), torch.from_numpy(mw[0]))
    assert np.array_equal(torch.cat([b[2] for b in mixed]).cpu().numpy(), mw[2])
    # the evaluation transform at another size passes no table; at the stored size with crop="pad" nothing changes
    ev = data.GpuDataset(images, labels, MEAN[:3], STD[:3], DEV, out_size=20)
    ex = torch.cat([b[0] for b in ev.batches(16, 0, 0, shuffle=False)]).cpu()
    assert torch.equal(ex, torch.from_numpy(rr.resample_all(images.numpy(), MEAN[:3], STD[:3], None, (20, 20))))
    today = data.GpuDataset(images, labels, MEAN[:3], STD[:3], DEV, pad=2, flip=True)
    same = data.GpuDataset(images, labels, MEAN[:3], STD[:3], DEV, pad=2, flip=True, out_size=(8, 8), crop="pad")
    assert not today.resample and not same.resample
    from tests import _augment_ref as ar
    a = torch.cat([b[0] for b in same.batches(16, 3, 11)]).cpu()
    assert torch.equal(a, ar.augment(images, ys.tolist(), MEAN[:3], STD[:3], 2, True, 11, 3))
    assert torch.equal(a, torch.cat([b[0] for b in today.batches(16, 3, 11)]).cpu())


TRAIN = ["--model-type", "cheby", "--n-patches", "2", "--n-blocks", "2", "--n-heads", "2", "--d-hidden", "64", "--out-d", "4",
         "--batch-size", "16", "--crop-padding", "2", "--no-tuned-gemms"]             # the geometry of tests/test_gpu_data_gpu.py
RESIZE = ["--resize", "16"]
RECIPE = ["--random-resized-crop", "--mixup", "0.8", "--cutmix", "1.0"]


@pytest.fixture(scope="module")
def npz_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("npz") / "tiny.npz")
    np.savez(path, x_train=_images(40, 8, 8, 3, 8).numpy(), y_train=(np.arange(40) % 4).astype(np.uint8),
             x_test=_images(12, 8, 8, 3, 9).numpy(), y_test=(np.arange(12) % 4).astype(np.int16))
    return path


@pytest.fixture(scope="module")
def resized_run(npz_file, tmp_path_factory):
    """train.main --data-npz --resize 16, eager: 2 epochs x (16, 16, 8).  Run once, shared by the tests below."""
    import train
    return train.main(train.parse([*TRAIN, *RESIZE, "--data-npz", npz_file, "--epochs", "2", "--log-dir", str(tmp_path_factory.mktemp("logs"))]))


def test_train_main_with_resize_adds_nothing_but_the_stream(npz_file, resized_run, tmp_path):
    import train
    from kanvit import data
    assert len(resized_run["losses"]) == 6 and all(np.isfinite(resized_run["losses"]))
    ds = data.GpuDataset.from_npz(npz_file, "train", DEV, pad=2, flip=True, out_size=(16, 16))
    fed = [b for epoch in range(2) for b in ds.batches(16, epoch, 0)]
    assert [tuple(x.shape) for x, _ in fed] == [(16, 3, 16, 16), (16, 3, 16, 16), (8, 3, 16, 16)] * 2
    args = train.parse([*TRAIN, "--synthetic", "--image-size", "16", "--epochs", "1", "--log-dir", str(tmp_path / "b")])
    assert train.main(args, batches=fed)["losses"] == resized_run["losses"]


def test_train_main_with_resize_replayed_from_a_graph(npz_file, resized_run, tmp_path):
    import train
    graphed = train.main(train.parse([*TRAIN, *RESIZE, "--data-npz", npz_file, "--epochs", "2", "--graph", "--log-dir", str(tmp_path / "c")]))
    assert graphed["losses"] == resized_run["losses"]


def test_train_main_with_the_recipe(npz_file, resized_run, tmp_path):
    """--random-resized-crop --mixup --cutmix at --resize 16: the losses are those of train.main fed the dataset's own (x, y, y2, w)
    batches (--fused-loss there: the soft-target loss a mixed run takes)."""
    import train
    from kanvit import data
    run = train.main(train.parse([*TRAIN, *RESIZE, *RECIPE, "--data-npz", npz_file, "--epochs", "1", "--log-dir", str(tmp_path / "r")]))
    assert len(run["losses"]) == 3 and all(np.isfinite(run["losses"])) and run["losses"] != resized_run["losses"][:3]
    ds = data.GpuDataset.from_npz(npz_file, "train", DEV, pad=2, flip=True, out_size=(16, 16), crop="rrc")
    fed = list(ds.batches(16, 0, 0, mix=dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5)))
    assert all(len(b) == 4 and tuple(b[0].shape[1:]) == (3, 16, 16) for b in fed)
    args = train.parse([*TRAIN, "--synthetic", "--image-size", "16", "--fused-loss", "--epochs", "1", "--log-dir", str(tmp_path / "s")])
    assert train.main(args, batches=fed)["losses"] == run["losses"]


def test_train_main_with_resize_evaluates_the_test_split_at_the_models_size(npz_file, resized_run):
    from kanvit import data
    text = open(resized_run["metrics_file"]).read()
    m = re.search(r"Phase: Test\n  Loss: (\d+\.\d{4})\n  Accuracy: \d\.\d{4}\n", text)
    assert m and "Epoch: 2, Phase: Train" in text, text
    test = data.GpuDataset.from_npz(npz_file, "test", DEV, out_size=(16, 16))
    model = resized_run["model"].eval()
    with torch.no_grad():
        batches = list(test.batches(16, 0, 0, shuffle=False))
        per_batch = [torch.nn.functional.cross_entropy(model(x), y) for x, y in batches]
    assert [tuple(x.shape) for x, _ in batches] == [(12, 3, 16, 16)]
    assert abs(float(torch.stack(per_batch).mean()) - float(m.group(1))) < 1e-4
