"""CPU-only checks of the GPU-resident data path (kanvit/data.py, csrc/batch_u8.hip, train.py --data-npz): the per-sample hash
against its check vectors, the coverage of offsets the GPU parity test relies on, the look-up table against the reference's
operations, the epoch's index lists, host-side validation of the entry point, the .npz layout and the new command-line flags."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import _augment_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIFAR_MEAN, CIFAR_STD = [0.5071, 0.4867, 0.4408], [0.2675, 0.2565, 0.2761]            # train.py:101-104


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def test_hash_check_vectors():
    assert ar.sample_params(0, 0, 0, 4, 4) == (8, 1, 1)
    assert ar.sample_params(0, 0, 1, 4, 4) == (3, 5, 1)
    assert ar.sample_params(0, 1, 0, 4, 4) == (8, 7, 0)
    assert ar.sample_params(0, 0, 0, 4, 4, flip_enabled=False) == (8, 1, 0)
    from kanvit import data
    assert data._mix(12345) == ar.mix(12345)                       # the module's own copy seeds the epoch's permutation


def test_hash_statistics_over_a_cifar_sized_epoch():
    p = ar.params(0, 0, range(50000), 4, 4)
    counts = np.bincount([q[0] for q in p], minlength=9)
    assert len(counts) == 9 and counts.min() >= 5451 and counts.max() <= 5655, counts
    assert sum(q[2] for q in p) == 25021


def test_first_130_samples_reach_every_offset_and_both_flips():
    """What the 32x32x3 GPU parity case relies on: indices 0..129 at seed 0, epoch 0, pad 4."""
    p = ar.params(0, 0, range(130), 4, 4)
    assert {q[0] for q in p} == set(range(9)) and {q[1] for q in p} == set(range(9)) and {q[2] for q in p} == {0, 1}
    assert sum(q[2] for q in p) == 56


def test_parameters_of_an_index_do_not_depend_on_the_others():
    alone = ar.params(3, 2, [77], 4, 4)[0]
    assert ar.params(3, 2, [5, 77, 9], 4, 4)[1] == alone and ar.params(3, 2, list(range(100)), 4, 4)[77] == alone
    assert ar.params(3, 3, [77], 4, 4)[0] != alone or ar.params(4, 2, [77], 4, 4)[0] != alone


def test_make_lut_is_the_reference_operations_on_every_byte():
    from kanvit import data
    lut = data.make_lut(CIFAR_MEAN, CIFAR_STD)
    assert lut.shape == (3, 256) and lut.dtype == torch.float32 and lut.device.type == "cpu" and lut.is_contiguous()
    mean, std = torch.tensor(CIFAR_MEAN, dtype=torch.float32), torch.tensor(CIFAR_STD, dtype=torch.float32)
    for c in range(3):
        assert torch.equal(lut[c], (torch.arange(256, dtype=torch.float32).div(255) - mean[c]).div(std[c]))
    # ... and the whole-image form of the reference: ToTensor (uint8 -> float / 255) then Normalize, on an image holding every byte
    img = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).expand(1, 16, 16, 3)
    want = ar.augment(img, [0], CIFAR_MEAN, CIFAR_STD, 0, False, 0, 0)[0]
    assert torch.equal(lut.reshape(3, 16, 16), want)
    one = data.make_lut([0.1307], [0.3081])
    assert one.shape == (1, 256)
    with pytest.raises(ValueError):
        data.make_lut([0.5, 0.5], [0.2])
    with pytest.raises(ValueError):
        data.make_lut([0.5], [0.0])


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_epoch_indices_cover_the_dataset_with_equal_shares(world):
    from kanvit import data
    n = 50
    lists = [data.epoch_indices(n, 0, 0, rank, world) for rank in range(world)]
    assert all(l.dtype == torch.int64 and l.dim() == 1 for l in lists)
    assert len({len(l) for l in lists}) == 1
    joined = torch.cat(lists)
    assert set(joined.tolist()) == set(range(n))
    assert 0 <= len(joined) - n <= world - 1
    again = [data.epoch_indices(n, 0, 0, rank, world) for rank in range(world)]
    assert all(torch.equal(a, b) for a, b in zip(lists, again))
    other = [data.epoch_indices(n, 1, 0, rank, world) for rank in range(world)]
    assert not all(torch.equal(a, b) for a, b in zip(lists, other))
    assert not torch.equal(data.epoch_indices(n, 0, 1, 0, world), lists[0])        # another seed, another order
    # every rank draws from ONE permutation: interleaving the ranks' lists gives it back, wrapped round at the end
    perm = data.epoch_indices(n, 0, 0)
    inter = torch.stack(lists, 1).reshape(-1)
    assert torch.equal(inter[:n], perm) and torch.equal(inter[n:], perm[:len(inter) - n])
    plain = torch.cat([data.epoch_indices(n, 0, 0, rank, world, shuffle=False) for rank in range(world)])
    assert torch.equal(data.epoch_indices(n, 5, 0, shuffle=False), torch.arange(n)) and set(plain.tolist()) == set(range(n))


def test_entry_point_validates_on_the_host(lib):
    ok = lib.kanvit_augment_u8_supported
    assert ok(50000, 32, 32, 3, 4, 4) == 1 and ok(1, 1, 1, 1, 0, 0) == 1 and ok(10, 6, 8, 4, 6, 8) == 1
    assert ok(10, 32, 32, 5, 4, 4) == 0 and ok(10, 32, 32, 0, 4, 4) == 0
    assert ok(10, 32, 32, 3, 33, 4) == 0 and ok(10, 32, 32, 3, 4, 33) == 0 and ok(10, 32, 32, 3, -1, 0) == 0
    assert ok(0, 32, 32, 3, 4, 4) == 0 and ok(10, 0, 32, 3, 0, 0) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(N=10, B=1, H=32, W=32, C=3, pad_y=4, pad_x=4, flip=1):
        return lib.kanvit_augment_u8(p, None, p, p, p, None, None, N, B, H, W, C, pad_y, pad_x, flip, 0, 0, None)

    for kw, word in ((dict(C=5), b"C=5"), (dict(pad_y=33), b"pad_y=33"), (dict(pad_x=33), b"pad_x=33"), (dict(N=0), b"N=0"),
                     (dict(B=-1), b"B=-1"), (dict(H=0), b"H=0"), (dict(flip=2), b"flip=2")):
        assert call(**kw) == -22, kw
        msg = lib.kanvit_last_error()
        assert b"kanvit_augment_u8" in msg and word in msg, (kw, msg)
    assert call(B=0) == 0                                            # an empty batch launches nothing: no device needed
    assert lib.kanvit_augment_u8(None, None, p, p, p, None, None, 10, 1, 32, 32, 3, 4, 4, 1, 0, 0, None) == -22
    assert b"null" in lib.kanvit_last_error()
    assert lib.kanvit_abi_version() == 7


def test_symbols_are_bound():
    from kanvit import _lib
    assert "kanvit_augment_u8" in _lib.SYMBOLS and "kanvit_augment_u8_supported" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["kanvit_augment_u8"][1]) == 18


def test_wrapper_refuses_cpu_tensors():
    from kanvit import KanvitError, data, ops
    with pytest.raises(KanvitError):
        ops.augment_u8(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), None, torch.zeros(1, dtype=torch.int64), data.make_lut(CIFAR_MEAN, CIFAR_STD))


def test_new_command_line_flags():
    import train
    a = train.parse([])
    assert a.data_npz is None and a.no_augment is False and a.crop_padding == 4
    b = train.parse(["--data-npz", "x.npz", "--no-augment", "--crop-padding", "2"])
    assert (b.data_npz, b.no_augment, b.crop_padding) == ("x.npz", True, 2)
    with pytest.raises(SystemExit):
        train.parse(["--synthetic", "--data-npz", "x.npz"])
    with pytest.raises(SystemExit):
        train.parse(["--data-npz", "x.npz", "--crop-padding", "-1"])
    a.synthetic, a.data_npz = True, "x.npz"
    with pytest.raises(SystemExit, match="--synthetic and --data-npz"):
        train.main(a)                                                # also for a namespace that did not come through parse()


def _good(n=6, h=4, w=4, c=3):
    rng = np.random.default_rng(0)
    return dict(x_train=rng.integers(0, 256, (n, h, w, c), dtype=np.uint8), y_train=np.arange(n, dtype=np.int32) % 3)


def test_npz_layout_is_validated_with_the_key_named(tmp_path):
    from kanvit import data
    path = str(tmp_path / "d.npz")
    good = _good()
    np.savez(path, **good, x_test=good["x_train"][:2], y_test=good["y_train"][:2].astype(np.uint8),
             mean=np.array([0.5, 0.4, 0.3], np.float32), std=np.array([0.2, 0.2, 0.2], np.float32))
    blob = data.load_npz(path)
    assert set(blob) == {"x_train", "y_train", "x_test", "y_test", "mean", "std"}
    np.savez(path, x_train=good["x_train"][..., 0], y_train=good["y_train"])         # [N, H, W]: one channel, no test split, no statistics
    assert data.load_npz(path)["x_train"].ndim == 3
    bad = [
        (dict(good, x_train=good["x_train"].astype(np.float32)), "x_train"),
        (dict(good, x_train=good["x_train"].reshape(6, -1)), "x_train"),
        (dict(good, x_train=np.zeros((6, 4, 4, 5), np.uint8)), "x_train"),
        (dict(good, y_train=good["y_train"].astype(np.float32)), "y_train"),
        (dict(good, y_train=good["y_train"][:5]), "y_train"),
        (dict(good, y_train=-good["y_train"] - 1), "y_train"),
        (dict(x_train=good["x_train"]), "y_train"),
        (dict(y_train=good["y_train"]), "x_train"),
        (dict(good, x_test=good["x_train"][:2]), "y_test"),
        (dict(good, x_test=good["x_train"][:2, :3], y_test=good["y_train"][:2]), "x_test"),
        (dict(good, x_test=good["x_train"][:2], y_test=good["y_train"][:3]), "y_test"),
        (dict(good, mean=np.zeros(2, np.float32), std=np.ones(2, np.float32)), "mean"),
        (dict(good, mean=np.zeros(3, np.float32), std=np.ones(3, np.int32)), "std"),
        (dict(good, mean=np.zeros(3, np.float32)), "std"),
        (dict(good, mean=np.zeros(3, np.float32), std=np.zeros(3, np.float32)), "std"),
    ]
    for arrays, key in bad:
        np.savez(path, **arrays)
        with pytest.raises(ValueError, match=f"'{key}'"):
            data.load_npz(path)


def test_channel_statistics_when_the_file_has_none():
    from kanvit import data
    x = _good()["x_train"]
    mean, std = data.channel_stats(x)
    v = x.astype(np.float64) / 255
    assert mean.dtype == np.float32 and np.array_equal(mean, v.mean((0, 1, 2)).astype(np.float32))
    assert np.array_equal(std, v.std((0, 1, 2)).astype(np.float32))
    m1, _ = data.channel_stats(x[..., 0])
    assert m1.shape == (1,) and m1[0] == mean[0]


def test_cifar_converter_reads_an_unpacked_directory(tmp_path):
    """tools/cifar_to_npz.py on a generated directory in the CIFAR-100 python-pickle layout (channel-planar rows, b'fine_labels')."""
    import pickle
    spec = importlib.util.spec_from_file_location("cifar_to_npz", os.path.join(ROOT, "tools", "cifar_to_npz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(1)
    src = tmp_path / "cifar-100-python"
    src.mkdir()
    rows = {}
    for name, n in (("train", 7), ("test", 3)):
        rows[name] = (rng.integers(0, 256, (n, 3072), dtype=np.uint8), [int(v) for v in rng.integers(0, 100, n)])
        with open(src / name, "wb") as f:
            pickle.dump({b"data": rows[name][0], b"fine_labels": rows[name][1], b"coarse_labels": [0] * n}, f)
    out = str(tmp_path / "c100.npz")
    mod.main([str(src), out])
    from kanvit import data
    blob = data.load_npz(out)
    assert blob["x_train"].shape == (7, 32, 32, 3) and blob["x_test"].shape == (3, 32, 32, 3)
    assert np.array_equal(blob["x_train"][2, 5, 9], rows["train"][0][2].reshape(3, 32, 32)[:, 5, 9])
    assert blob["y_train"].tolist() == rows["train"][1] and blob["y_test"].tolist() == rows["test"][1]
    assert np.array_equal(blob["mean"], np.array(CIFAR_MEAN, np.float32)) and np.array_equal(blob["std"], np.array(CIFAR_STD, np.float32))
    assert os.path.getsize(out) < 64 << 10


def test_new_kernels_use_no_scratch(lib):
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    from kanvit import build
    ks = {km.demangled_short(n): k for n, k in km.kernels(build.LIB).items()}
    mine = sorted(n for n in ks if n.startswith("augment_u8_kernel"))
    assert mine == ["augment_u8_kernel<1>", "augment_u8_kernel<4>"]         # the scalar and the 16-byte store form
    for n in mine:
        assert ks[n][".private_segment_fixed_size"] == 0 and ks[n][".vgpr_spill_count"] == 0 and ks[n][".sgpr_spill_count"] == 0, n
        assert ks[n][".group_segment_fixed_size"] == 4 * 1024               # the table: up to 4 channels x 1 KB
