"""GPU tests of the GPU-resident data path: ops.augment_u8 (csrc/batch_u8.hip) against the CPU transform of tests/_augment_ref.py --
BITWISE, since the kernel only looks values up in a table the host built with the reference's operations -- at the smallest shapes
that reach each form and edge; GpuDataset.batches; and train.main --data-npz against train.main fed the same batches."""
import re

import numpy as np
import pytest
import torch

from tests import _augment_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CIFAR_MEAN, CIFAR_STD = [0.5071, 0.4867, 0.4408], [0.2675, 0.2565, 0.2761]            # train.py:101-104


def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    x.view(-1)[:3] = torch.tensor([0, 255, 1], dtype=torch.uint8)            # the table's ends occur whatever the draw
    return x


def _run(images, labels, idx, mean, std, pad, flip, seed, epoch, **kw):
    from kanvit import data, ops
    lut = data.make_lut(mean, std).to(DEV)
    return ops.augment_u8(images.to(DEV), None if labels is None else labels.to(DEV), torch.as_tensor(idx, dtype=torch.int64).to(DEV), lut,
                          pad, flip, seed, epoch, **kw)


@pytest.fixture(scope="module")
def cifar_case():
    """32x32x3, pad 4, indices 0..129 at seed 0, epoch 0: every offset and both flips (tests/test_gpu_data_cpu.py), 16-byte stores,
    more than one work-group (130 * 3 * 32 * 8 work items of four pixels over 256-thread groups).  The reference is computed once."""
    images, labels = _images((130, 32, 32, 3), 1), (torch.arange(130) * 7) % 100
    idx = list(range(130))
    want = ar.augment(images, idx, CIFAR_MEAN, CIFAR_STD, 4, True, 0, 0)
    x, y, p = _run(images, labels, idx, CIFAR_MEAN, CIFAR_STD, 4, True, 0, 0, return_params=True)
    return dict(images=images, labels=labels, idx=idx, want=want, x=x.cpu(), y=y.cpu(), p=p.cpu())


def test_cifar_shape_is_bitwise_the_cpu_transform(cifar_case):
    c = cifar_case
    assert c["x"].shape == (130, 3, 32, 32) and c["x"].dtype == torch.float32
    assert torch.equal(c["x"], c["want"])
    assert torch.equal(c["y"], c["labels"][c["idx"]])
    want_p = ar.params(0, 0, c["idx"], 4, 4)
    assert c["p"].dtype == torch.int32 and c["p"].tolist() == [list(q) for q in want_p]
    assert {q[0] for q in want_p} == set(range(9)) and {q[1] for q in want_p} == set(range(9)) and {q[2] for q in want_p} == {0, 1}


def test_odd_one_channel_shape_takes_the_scalar_form():
    """7x9, one channel as an [N, H, W] array, pad 3: W % 4 != 0.  The five samples include a crop at an extreme offset on both axes,
    where only a corner of the image is left."""
    N = 64
    images = _images((N, 7, 9), 2)
    par = ar.params(5, 1, range(N), 3, 3)
    corner = [i for i, q in enumerate(par) if q[0] in (0, 6) and q[1] in (0, 6)]
    assert corner, "no corner crop among the 64 samples: pick another seed"
    idx = [corner[0], 0, 63, 17, corner[-1]]
    x, p = _run(images, None, idx, [0.1307], [0.3081], 3, True, 5, 1, return_params=True)
    assert x.shape == (5, 1, 7, 9)
    assert torch.equal(x.cpu(), ar.augment(images, idx, [0.1307], [0.3081], 3, True, 5, 1))
    assert p.cpu().tolist() == [list(par[i]) for i in idx]


def test_padding_as_large_as_the_image():
    """6x8x4 with pad = (H, W): offsets up to twice the image, rows and whole samples that are padding only."""
    images = _images((9, 6, 8, 4), 3)
    mean, std = [0.5, 0.4, 0.3, 0.2], [0.2, 0.25, 0.3, 0.35]
    idx = [8, 0, 4]
    x, p = _run(images, None, idx, mean, std, (6, 8), True, 0, 0, return_params=True)
    want = ar.augment(images, idx, mean, std, (6, 8), True, 0, 0)
    assert torch.equal(x.cpu(), want)
    assert p.cpu().tolist() == [list(q) for q in ar.params(0, 0, idx, 6, 8)]
    assert any(q[0] != 6 for q in ar.params(0, 0, idx, 6, 8))              # some rows are all padding


@pytest.mark.parametrize("shape", [(6, 32, 32, 3), (5, 7, 9)])
def test_evaluation_transform_is_the_normalised_image(shape):
    from kanvit import data
    images = _images(shape, 4)
    C = shape[3] if len(shape) == 4 else 1
    mean, std = CIFAR_MEAN[:C], CIFAR_STD[:C]
    idx = list(range(shape[0]))
    x, p = _run(images, None, idx, mean, std, 0, False, 3, 9, return_params=True)
    u8 = images.reshape(*shape[:3], C).permute(0, 3, 1, 2)
    want = (u8.float().div(255) - torch.tensor(mean).reshape(1, C, 1, 1)).div(torch.tensor(std).reshape(1, C, 1, 1))
    assert torch.equal(x.cpu(), want)
    lut = data.make_lut(mean, std)
    assert torch.equal(x.cpu(), torch.stack([lut[c][u8[:, c].long()] for c in range(C)], 1))
    assert not p.cpu().any()


def test_single_and_empty_batches(cifar_case):
    c = cifar_case
    x, y = _run(c["images"], c["labels"], [57], CIFAR_MEAN, CIFAR_STD, 4, True, 0, 0)
    assert torch.equal(x.cpu(), c["want"][57:58]) and y.cpu().tolist() == [int(c["labels"][57])]
    x, y, p = _run(c["images"], c["labels"], [], CIFAR_MEAN, CIFAR_STD, 4, True, 0, 0, return_params=True)
    assert x.shape == (0, 3, 32, 32) and y.shape == (0,) and p.shape == (0, 3)


def test_repeats_descending_order_and_position_independence(cifar_case):
    c = cifar_case
    idx = [129, 129, 100, 57, 57, 3, 0]
    x, y = _run(c["images"], c["labels"], idx, CIFAR_MEAN, CIFAR_STD, 4, True, 0, 0)
    assert torch.equal(x.cpu(), c["want"][idx]) and torch.equal(y.cpu(), c["labels"][idx])
    # sample 57: alone (above), inside the batch of 130 at position 57, here at positions 3 and 4
    assert torch.equal(x[3].cpu(), c["x"][57]) and torch.equal(x[4].cpu(), c["x"][57])


def test_another_epoch_and_another_seed_change_the_batch(cifar_case):
    c = cifar_case
    for seed, epoch in ((0, 1), (1, 0)):
        x = _run(c["images"], None, c["idx"], CIFAR_MEAN, CIFAR_STD, 4, True, seed, epoch)
        assert not torch.equal(x.cpu(), c["want"])
        assert torch.equal(x.cpu(), ar.augment(c["images"], c["idx"], CIFAR_MEAN, CIFAR_STD, 4, True, seed, epoch))


def test_output_off_the_16_byte_grid_takes_the_scalar_form(cifar_case):
    c = cifar_case
    idx = c["idx"][:9]
    n = 9 * 3 * 32 * 32
    buf = torch.full((n + 5,), float("nan"), device=DEV)
    view = buf[1:n + 1].view(9, 3, 32, 32)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got = _run(c["images"], None, idx, CIFAR_MEAN, CIFAR_STD, 4, True, 0, 0, out=view)
    assert got.data_ptr() == view.data_ptr()
    assert torch.equal(view.cpu(), c["want"][:9])
    rest = buf.cpu()
    assert torch.isnan(rest[0]) and torch.isnan(rest[n + 1:]).all()         # nothing written outside the view


GRID_ITEMS = 2048 * 256             # BATCH_MAX_GROUPS work-groups of 256 threads: past that many work items a thread takes a second one
# name -> ((H, W, C), B, pixels per work item, out= one element off the 16-byte grid)
LAP_CASES = {"vec 8x8x3": ((8, 8, 3), 11000, 4, False), "vec 8x12x4": ((8, 12, 4), 5500, 4, False),
             "scalar 6x6x1": ((6, 6, 1), 14600, 1, False), "scalar by alignment 8x8x3": ((8, 8, 3), 2750, 1, True)}


@pytest.mark.parametrize("name", list(LAP_CASES))
def test_batch_past_the_grid_cap_wraps_the_stride_loop(name):
    """More work items than a full grid has threads: the end of the batch -- pixels, and the labels and parameters of its last samples,
    which the thread of a sample's first item writes -- comes from a thread's second lap.  40 stored samples, repeated in a shuffled
    order; the transform of a sample does not depend on its place, so the reference is the 40 transforms, gathered."""
    (H, W, C), B, vec, off = LAP_CASES[name]
    per_sample = H * C * (W // vec)
    assert B * per_sample > GRID_ITEMS and (B - 1) * per_sample >= GRID_ITEMS           # the last sample lies in the second lap whole
    assert (vec == 4) == (W % 4 == 0 and not off)
    N, seed, epoch, pad = 40, 3, 2, (2, 2)
    images, labels = _images((N, H, W, C) if C > 1 else (N, H, W), 8), (torch.arange(N) * 7) % 100
    mean, std = [0.5, 0.4, 0.3, 0.2][:C], [0.2, 0.25, 0.3, 0.35][:C]
    rng = np.random.default_rng(B)
    idx = torch.from_numpy(np.concatenate([rng.permutation(N) for _ in range(-(-B // N))])[:B])
    n = B * C * H * W
    buf = torch.full((n + 5,), float("nan"), device=DEV)
    view = buf[off:n + off].view(B, C, H, W)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    x, y, p = _run(images, labels, idx, mean, std, pad, True, seed, epoch, return_params=True, out=view)
    assert x.data_ptr() == view.data_ptr()
    got, rest = view.cpu(), buf.cpu()
    assert not torch.isnan(got).any()
    assert torch.isnan(rest[:off]).all() and torch.isnan(rest[n + off:]).all()           # nothing written outside the view
    assert torch.equal(got, ar.augment(images, list(range(N)), mean, std, pad, True, seed, epoch)[idx])
    assert torch.equal(y.cpu(), labels[idx])
    par = torch.tensor(ar.params(seed, epoch, range(N), *pad), dtype=torch.int32)
    assert p.dtype == torch.int32 and torch.equal(p.cpu(), par[idx])
    assert len({tuple(q) for q in par.tolist()}) > 10                               # the parameters tell the samples apart


def test_wrapper_checks_its_operands(cifar_case):
    from kanvit import KanvitError, data, ops
    images = cifar_case["images"][:4].to(DEV)
    lut = data.make_lut(CIFAR_MEAN, CIFAR_STD).to(DEV)
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(KanvitError, match="dtype"):
        ops.augment_u8(images.float(), None, idx, lut)
    with pytest.raises(KanvitError, match="dtype"):
        ops.augment_u8(images, None, idx.int(), lut)
    with pytest.raises(KanvitError, match="contiguous"):
        ops.augment_u8(images.permute(0, 2, 1, 3), None, idx, lut)
    with pytest.raises(KanvitError, match="lut"):
        ops.augment_u8(images, None, idx, lut[:2])
    with pytest.raises(KanvitError, match="labels"):
        ops.augment_u8(images, torch.zeros(3, dtype=torch.int64, device=DEV), idx, lut)
    with pytest.raises(KanvitError, match="pad_y"):
        ops.augment_u8(images, None, idx, lut, pad=33)
    with pytest.raises(KanvitError, match="cpu"):
        ops.augment_u8(images, None, idx.cpu(), lut)


def test_dataset_batches_cover_an_epoch():
    """50 samples at batch 16: 16, 16, 16, 2; labels = sample indices, so every batch names the samples it holds."""
    from kanvit import data
    images, labels = _images((50, 8, 8, 3), 6), torch.arange(50)
    ds = data.GpuDataset(images, labels, CIFAR_MEAN, CIFAR_STD, DEV, pad=2, flip=True)
    assert len(ds) == 50 and ds.n_batches(16) == 4 and ds.chw == (3, 8, 8)
    got = list(ds.batches(16, epoch=3, seed=11))
    assert [len(y) for _, y in got] == [16, 16, 16, 2] and all(x.is_cuda and y.is_cuda for x, y in got)
    ys = torch.cat([y for _, y in got]).cpu()
    assert torch.equal(ys, data.epoch_indices(50, 3, 11)) and sorted(ys.tolist()) == list(range(50))
    want = ar.augment(images, ys.tolist(), CIFAR_MEAN, CIFAR_STD, 2, True, 11, 3)
    assert torch.equal(torch.cat([x for x, _ in got]).cpu(), want)
    # two ranks: equal step counts, the same samples between them, each sample the same pixels as in the one-rank epoch
    halves = [list(ds.batches(16, epoch=3, seed=11, rank=r, world=2)) for r in range(2)]
    assert [[len(y) for _, y in h] for h in halves] == [[16, 9], [16, 9]]
    y2 = torch.stack([torch.cat([y for _, y in h]) for h in halves], 1).reshape(-1).cpu()
    assert torch.equal(y2, ys)
    x2 = torch.stack([torch.cat([x for x, _ in h]) for h in halves], 1).reshape(50, 3, 8, 8).cpu()
    assert torch.equal(x2, want)
    assert len(ds.loader(16, shuffle=False)) == 4
    assert torch.equal(torch.cat([y for _, y in ds.loader(16, shuffle=False)]).cpu(), labels)


def test_dataset_refuses_an_index_outside_it(monkeypatch):
    from kanvit import data
    ds = data.GpuDataset(_images((5, 8, 8, 3), 7), torch.arange(5), CIFAR_MEAN, CIFAR_STD, DEV)
    monkeypatch.setattr(data, "epoch_indices", lambda *a, **k: torch.tensor([0, 5]))
    with pytest.raises(IndexError):
        next(ds.batches(2, 0, 0))


TRAIN = ["--model-type", "cheby", "--n-patches", "2", "--n-blocks", "2", "--n-heads", "2", "--d-hidden", "64", "--out-d", "4",
         "--batch-size", "16", "--crop-padding", "2", "--no-tuned-gemms"]


@pytest.fixture(scope="module")
def npz_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("npz") / "tiny.npz")
    np.savez(path, x_train=_images((40, 8, 8, 3), 8).numpy(), y_train=(np.arange(40) % 4).astype(np.uint8),
             x_test=_images((12, 8, 8, 3), 9).numpy(), y_test=(np.arange(12) % 4).astype(np.int16))
    return path


@pytest.fixture(scope="module")
def npz_run(npz_file, tmp_path_factory):
    """train.main --data-npz, eager: 2 epochs x (16, 16, 8).  Run once, shared by the tests below."""
    import train
    return train.main(train.parse([*TRAIN, "--data-npz", npz_file, "--epochs", "2", "--log-dir", str(tmp_path_factory.mktemp("logs"))]))


def test_train_main_on_an_npz_adds_nothing_but_the_stream(npz_file, npz_run, tmp_path):
    """Six finite losses, equal as Python floats to those of train.main fed the very batches GpuDataset.batches yields for the two
    epochs (one epoch of six steps there: `batches` is the whole stream)."""
    import train
    from kanvit import data
    assert len(npz_run["losses"]) == 6 and all(np.isfinite(npz_run["losses"]))
    ds = data.GpuDataset.from_npz(npz_file, "train", DEV, pad=2, flip=True)
    fed = [b for epoch in range(2) for b in ds.batches(16, epoch, 0)]
    assert [len(y) for _, y in fed] == [16, 16, 8, 16, 16, 8]
    args = train.parse([*TRAIN, "--synthetic", "--image-size", "8", "--epochs", "1", "--log-dir", str(tmp_path / "b")])
    assert train.main(args, batches=fed)["losses"] == npz_run["losses"]


def test_train_main_on_an_npz_replayed_from_a_graph(npz_file, npz_run, tmp_path):
    """--graph copies each full batch into the captured step's buffers (the short third batch of an epoch runs eagerly)."""
    import train
    graphed = train.main(train.parse([*TRAIN, "--data-npz", npz_file, "--epochs", "2", "--graph", "--log-dir", str(tmp_path / "c")]))
    assert graphed["losses"] == npz_run["losses"]


def test_train_main_on_an_npz_evaluates_the_test_split(npz_file, npz_run):
    """The test block is written from x_test: the evaluation transform in the file's order, the logged loss the mean of its batch losses."""
    from kanvit import data
    text = open(npz_run["metrics_file"]).read()
    m = re.search(r"Phase: Test\n  Loss: (\d+\.\d{4})\n  Accuracy: \d\.\d{4}\n", text)
    assert m and "Epoch: 2, Phase: Train" in text, text
    test = data.GpuDataset.from_npz(npz_file, "test", DEV)
    model = npz_run["model"].eval()
    with torch.no_grad():
        per_batch = [torch.nn.functional.cross_entropy(model(x), y) for x, y in test.batches(16, 0, 0, shuffle=False)]
    assert len(per_batch) == 1 and abs(float(torch.stack(per_batch).mean()) - float(m.group(1))) < 1e-4


def test_train_main_refuses_an_npz_the_flags_contradict(npz_file, tmp_path):
    import train
    for extra in (["--image-size", "16"], ["--in-chans", "1"], ["--out-d", "3"], ["--crop-padding", "9"]):      # a later flag overrides TRAIN's
        with pytest.raises(SystemExit, match=extra[0]):
            train.main(train.parse([*TRAIN, *extra, "--data-npz", npz_file, "--epochs", "1", "--log-dir", str(tmp_path / "l")]))
