"""Random Erasing without a GPU: kanvit.data.erase_table / normal_table / erase_noise_key, the C-ABI refusals of kanvit_erase_u8 (null
device pointers, as tests/test_batch_u8_abi_cpu.py calls the older entries: a refused call dereferences nothing) and train.parse's flag
rules.  The pixels are tests/test_erase_gpu.py's."""
import numpy as np
import pytest
import torch

from tests import _erase_ref as er

P = 0x1000          # a non-null dummy pointer, aligned to 16 bytes
POINTERS = ("images", "labels", "idx", "lut", "crop", "partner", "weight", "box", "out", "y_out", "y2_out", "w_out", "erase", "noise")
# a valid call of kanvit_erase_u8 in the order of its C arguments (the stream, last, is null)
VALID = dict(images=P, labels=P, idx=P, lut=P, crop=P, partner=P, weight=P, box=P, out=P, y_out=P, y2_out=P, w_out=P, N=3, B=2, H=4, W=4, C=1,
             OH=8, OW=8, erase=P, noise=P, noise_len=4096, noise_key=7)


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


# ---- erase_table ------------------------------------------------------------------------------------------------------------
def test_erase_table_is_a_function_of_its_arguments():
    from kanvit import data
    a = data.erase_table(500, 3, 11, (16, 20), prob=0.5)
    assert a.dtype == torch.int32 and tuple(a.shape) == (500, 4) and a.device.type == "cpu"
    assert torch.equal(a, data.erase_table(500, 3, 11, (16, 20), prob=0.5))
    assert not torch.equal(a, data.erase_table(500, 4, 11, (16, 20), prob=0.5))             # another epoch
    assert not torch.equal(a, data.erase_table(500, 3, 12, (16, 20), prob=0.5))             # another seed
    assert not torch.equal(data.erase_table(500, 0, 0, (16, 20), prob=0.5), data.erase_table(500, 1, 0, (16, 20), prob=0.5))
    # every column is drawn for all n rows whatever the flags: a row's geometry does not depend on prob, only whether it is kept
    b = data.erase_table(500, 3, 11, (16, 20), prob=1.0)
    kept = (a != 0).any(1)
    assert 0 < int(kept.sum()) < 500 and torch.equal(a[kept], b[kept])


@pytest.mark.parametrize("hw", [(5, 7), (8, 8), (12, 20), (32, 32), (224, 224)])
def test_erase_table_rows_are_boxes_inside_the_output_or_all_zero(hw):
    from kanvit import data
    OH, OW = hw
    t = data.erase_table(20000, 1, 5, hw, prob=0.6).numpy().astype(np.int64)
    y0, y1, x0, x1 = t.T
    erased = (t != 0).any(1)
    e = t[erased]
    assert 0 < len(e) < len(t)
    assert (0 <= e[:, 0]).all() and (e[:, 0] < e[:, 1]).all() and (e[:, 1] <= OH).all()
    assert (0 <= e[:, 2]).all() and (e[:, 2] < e[:, 3]).all() and (e[:, 3] <= OW).all()
    assert (e[:, 1] - e[:, 0] < OH).all() and (e[:, 3] - e[:, 2] < OW).all()
    assert (t[~erased] == 0).all()
    assert abs(erased.mean() - 0.6) < 0.02               # five binomial sigmas at n = 20000 are 0.017


def test_erase_table_probabilities():
    from kanvit import data
    assert not data.erase_table(1000, 0, 0, (32, 32), prob=0.0).any()
    full = data.erase_table(100000, 0, 0, (32, 32), prob=1.0).numpy().astype(np.int64)
    assert ((full[:, 1] > full[:, 0]) & (full[:, 3] > full[:, 2])).all()                    # every row finds a box within ten attempts
    area = ((full[:, 1] - full[:, 0]) * (full[:, 3] - full[:, 2])).mean() / (32 * 32)
    assert 0.16 < area < 0.19                            # the box rule's mean erased area is 17-18 % of the image
    quarter = data.erase_table(100000, 0, 0, (32, 32)).numpy()                              # the default prob, 0.25
    assert abs((quarter != 0).any(1).mean() - 0.25) < 0.01                                  # five binomial sigmas are 0.007


def test_erase_table_restated_row_by_row():
    """The box rule as a per-sample loop over columns drawn here, in the order erase_table documents."""
    import math
    from kanvit import data
    from tests import _augment_ref as ar
    n, epoch, seed, (OH, OW), prob, scale, ratio = 300, 2, 9, (12, 20), 0.7, (0.02, 1 / 3), (0.3, 1 / 0.3)
    g = np.random.Generator(np.random.PCG64(ar.mix(ar.mix((ar.mix(seed) + epoch) & ar.M64) ^ 0x65726173655F7462)))
    up, fa, fr = g.random(n), [g.random(n) for _ in range(10)], [g.random(n) for _ in range(10)]
    uy, ux = g.random(n), g.random(n)
    rows = np.zeros((n, 4), np.int32)
    for s in range(n):
        if not up[s] < prob:
            continue
        for k in range(10):
            area = OH * OW * (scale[0] + (scale[1] - scale[0]) * fa[k][s])
            r = math.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * fr[k][s])
            h, w = int(round(math.sqrt(area * r))), int(round(math.sqrt(area / r)))
            if 1 <= h < OH and 1 <= w < OW:
                y0, x0 = int(math.floor(uy[s] * (OH - h + 1))), int(math.floor(ux[s] * (OW - w + 1)))
                rows[s] = (y0, y0 + h, x0, x0 + w)
                break
    assert np.array_equal(data.erase_table(n, epoch, seed, (OH, OW), prob, scale, ratio).numpy(), rows)


@pytest.mark.parametrize("kw", [dict(n=0), dict(hw=(0, 8)), dict(prob=-0.1), dict(prob=1.5), dict(scale=(0.0, 0.3)), dict(scale=(0.4, 0.3)),
                                dict(scale=(0.1, 1.5)), dict(ratio=(0.0, 3.0)), dict(ratio=(3.0, 0.3)), dict(ratio=(0.3, float("inf")))])
def test_erase_table_refuses_bad_arguments(kw):
    from kanvit import data
    args = dict(n=10, epoch=0, seed=0, hw=(8, 8))
    args.update(kw)
    with pytest.raises(ValueError, match="erase_table"):
        data.erase_table(**args)


# ---- normal_table, erase_noise_key --------------------------------------------------------------------------------------------
def test_normal_table():
    from statistics import NormalDist
    from kanvit import data
    t = data.normal_table(4096)
    assert t.dtype == torch.float32 and tuple(t.shape) == (4096,) and torch.equal(t, data.normal_table())
    v = t.numpy()
    assert (v[1:] > v[:-1]).all()
    assert np.array_equal(v, -v[::-1])
    assert abs(v.astype(np.float64).std() - 1.0) < 1e-3 and abs(v.astype(np.float64).mean()) == 0.0
    assert abs(float(v.max()) - 3.668) < 1e-3
    assert v[2048] == np.float32(NormalDist().inv_cdf(2048.5 / 4096))
    assert tuple(data.normal_table(2).shape) == (2,) and tuple(data.normal_table(65536).shape) == (65536,)
    for bad in (0, 1, 3, 4095, 131072):
        with pytest.raises(ValueError, match="normal_table"):
            data.normal_table(bad)


def test_erase_noise_key_and_the_restated_hash():
    from kanvit import data
    from tests import _augment_ref as ar
    k = data.erase_noise_key(3, 2)
    assert k == ar.mix(ar.mix((ar.mix(3) + 2) & ar.M64) ^ 0x65726173655F6E7A) and 0 <= k < 2 ** 64
    assert len({data.erase_noise_key(s, e) for s in range(3) for e in range(3)}) == 9
    # the uint64-array hash of tests/_erase_ref is the Python-integer one, element by element, wrap-around included
    noise = np.arange(16, dtype=np.float32)
    key, s, (C, OH, OW) = 2 ** 64 - 2, 5, (2, 3, 5)
    plane = er.noise_plane(noise, key, s, (C, OH, OW))
    base = ar.mix((key + s) & ar.M64)
    for c, y, x in ((0, 0, 0), (1, 2, 4), (0, 1, 3)):
        assert plane[c, y, x] == noise[ar.mix((base + (c * OH + y) * OW + x) & ar.M64) >> 60]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def _call(lib, **kw):
    assert set(kw) <= set(VALID)
    args = dict(VALID, **kw)
    return lib.kanvit_erase_u8(*[(v or None) if k in POINTERS else v for k, v in args.items()], None)


def test_erase_u8_supported(lib):
    ok = lib.kanvit_erase_u8_supported
    assert ok(3, 4, 4, 1, 8, 8, 0) == 1 and ok(3, 4, 4, 1, 8, 8, 2) == 1 and ok(3, 4, 4, 4, 8, 8, 65536) == 1
    for noise_len in (1, 3, 6, -4, 131072):
        assert ok(3, 4, 4, 1, 8, 8, noise_len) == 0
    assert ok(0, 4, 4, 1, 8, 8, 0) == 0 and ok(3, 4, 4, 5, 8, 8, 0) == 0 and ok(3, 4, 4, 1, 0, 8, 0) == 0 and ok(3, 0, 4, 1, 8, 8, 0) == 0


REFUSALS = [
    # kanvit_resample_u8's, under the new entry's name
    (dict(N=0), "kanvit_erase_u8: N=0: the dataset holds at least one image"),
    (dict(C=5), "kanvit_erase_u8: C=5 must be in 1..4 (the look-up table is staged as C x 1 KB)"),
    (dict(OH=0), "kanvit_erase_u8: OH=0, OW=8 must be in 1..2^20"),
    (dict(B=-1), "kanvit_erase_u8: B=-1 is negative"),
    (dict(out=0), "kanvit_erase_u8: null images/idx/lut/out"),
    (dict(labels=0), "kanvit_erase_u8: y_out / y2_out without labels"),
    (dict(out=P + 2), "kanvit_erase_u8: a pointer is not aligned to its element size"),
    (dict(weight=0), "kanvit_erase_u8: null weight (the three mix tables partner/weight/box come together or not at all)"),
    (dict(partner=0, weight=0, box=0), "kanvit_erase_u8: y2_out / w_out without the mix tables"),
    # its own
    (dict(noise_len=3), "kanvit_erase_u8: noise_len=3 must be a power of two in 2..65536 (or 0 with a null noise: the fill is 0)"),
    (dict(noise_len=1), "kanvit_erase_u8: noise_len=1 must be a power of two in 2..65536 (or 0 with a null noise: the fill is 0)"),
    (dict(noise_len=131072), "kanvit_erase_u8: noise_len=131072 must be a power of two in 2..65536 (or 0 with a null noise: the fill is 0)"),
    (dict(erase=0), "kanvit_erase_u8: noise without erase (the noise fills the erase boxes)"),
    (dict(noise=0), "kanvit_erase_u8: noise_len=4096 with a null noise (a table and its length come together; both absent: the fill is 0)"),
    (dict(noise_len=0), "kanvit_erase_u8: noise_len=0 with a noise (a table and its length come together; both absent: the fill is 0)"),
    (dict(erase=P + 2), "kanvit_erase_u8: erase / noise is not aligned to its element size"),
    (dict(noise=P + 1), "kanvit_erase_u8: erase / noise is not aligned to its element size"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=["-".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in REFUSALS])
def test_erase_u8_refusal_code_and_message(lib, kw, message):
    assert _call(lib, **kw) == -22
    assert lib.kanvit_last_error().decode() == message


def test_erase_u8_empty_batch_returns_0_with_every_pointer_null(lib):
    assert _call(lib, B=0, noise_len=0, **{k: 0 for k in POINTERS}) == 0


# ---- train.parse ----------------------------------------------------------------------------------------------------------------
def test_train_flags():
    import train
    off = train.parse(["--data-npz", "x.npz"])
    assert off.random_erasing == 0.0 and off.erase_mode == "pixel" and train.erase_config(off) is None
    assert tuple(off.erase_scale) == (0.02, 1.0 / 3.0) and tuple(off.erase_ratio) == (0.3, 1.0 / 0.3)
    zero = train.parse(["--data-npz", "x.npz", "--random-erasing", "0"])
    assert vars(zero) == vars(off)                       # P = 0 is the old configuration
    assert vars(train.parse(["--synthetic", "--random-erasing", "0"])) == vars(train.parse(["--synthetic"]))
    on = train.parse(["--data-npz", "x.npz", "--random-erasing", "0.25", "--erase-mode", "const", "--erase-scale", "0.1", "0.2", "--erase-ratio", "0.5", "2"])
    assert train.erase_config(on) == dict(prob=0.25, scale=(0.1, 0.2), ratio=(0.5, 2.0), mode="const")
    assert train.erase_config(train.parse(["--data-npz", "x.npz", "--random-erasing", "1"]))["mode"] == "pixel"
    refused = [(["--random-erasing", "0.5"], "--data-npz"),
               (["--synthetic", "--random-erasing", "0.5"], "--data-npz"),
               (["--data-npz", "x.npz", "--random-erasing", "0.5", "--no-augment"], "--no-augment"),
               (["--data-npz", "x.npz", "--random-erasing", "1.5"], "probability"),
               (["--data-npz", "x.npz", "--random-erasing", "-0.1"], "probability"),
               (["--data-npz", "x.npz", "--erase-scale", "0", "0.3"], "--erase-scale"),
               (["--data-npz", "x.npz", "--erase-scale", "0.4", "0.3"], "--erase-scale"),
               (["--data-npz", "x.npz", "--erase-scale", "0.1", "1.5"], "at most 1"),
               (["--data-npz", "x.npz", "--erase-ratio", "0", "3"], "--erase-ratio"),
               (["--data-npz", "x.npz", "--erase-ratio", "3", "0.3"], "--erase-ratio"),
               (["--data-npz", "x.npz", "--erase-mode", "rand"], None)]
    for argv, word in refused:
        with pytest.raises(SystemExit, match=word):
            train.parse(argv)
    assert "--random-erasing" in train.__doc__ and "--erase-mode" in train.__doc__


def test_gpu_dataset_erase_argument_is_checked_before_any_upload():
    from kanvit import data
    x, y = torch.zeros((4, 8, 8, 3), dtype=torch.uint8), torch.zeros(4, dtype=torch.int64)
    for bad, word in ((dict(mode="rand"), "mode"), (dict(prob=2.0), "prob"), (dict(count=2), "keys"), (0.25, "dict"), (dict(scale=(0.5, 2.0)), "scale")):
        with pytest.raises(ValueError, match=word):
            data.GpuDataset(x, y, [0.5] * 3, [0.25] * 3, "cuda:0", erase=bad)
