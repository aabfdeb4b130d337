"""ops.erase_u8 (csrc/batch_u8.hip: erase_u8_kernel, the erasing form of resample_u8_kernel) on the GPU against the NumPy restatement of tests/_erase_ref.py --
BITWISE throughout: the fill is a look-up, the resize and the blend are the float32 sequences tests/_resample_ref.py and
tests/_mix_ref.py already restate.  The shapes are the smallest that reach each path: 8x8x3 at the identity size with box edges inside
a 4-wide vector and on a 4-row item boundary, the scalar store form, the window path (8x8 -> 22x32), the tap path (downscale), mixing
with the partner erased under its own row, indices outside the dataset, one batch past the grid cap; then GpuDataset(erase=...) and
train.main with --random-erasing."""
import numpy as np
import pytest
import torch

from tests import _erase_ref as er
from tests import _resample_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, EPOCH = 3, 2
KEY = 0xFEDCBA9876543210                        # a noise key with the top bit set: key + s is a 64-bit sum
MEAN, STD = [0.5071, 0.4867, 0.4408, 0.45], [0.2675, 0.2565, 0.2761, 0.25]
GRID_ITEMS = 2048 * 256                         # the launch's cap: 2048 work-groups of 256 work items
IMIN, IMAX = er.IMIN, er.IMAX
_cache = {}


def _images(n, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, H, W, C), dtype=torch.uint8, generator=g)
    x.view(-1)[:3] = torch.tensor([0, 255, 1], dtype=torch.uint8)
    return x[..., 0].contiguous() if C == 1 else x


def _noise():
    if "noise" not in _cache:
        from kanvit import data
        t = data.normal_table(4096)
        _cache["noise"] = (t.numpy(), t.to(DEV))
    return _cache["noise"]


def _dataset(n, shape, seed):
    """Images, labels and their device copies, made once per (n, shape, seed)."""
    key = ("ds", n, shape, seed)
    if key not in _cache:
        from kanvit import data
        H, W, C = shape
        images, labels = _images(n, H, W, C, seed), (torch.arange(n) * 5 + 1) % 11
        lut = data.make_lut(MEAN[:C], STD[:C])
        _cache[key] = dict(images=images, labels=labels, C=C, pad=lut[:, 0].numpy(), dev=dict(images=images.to(DEV), labels=labels.to(DEV), lut=lut.to(DEV)))
    return _cache[key]


def _dev(table, dtype=None):
    return None if table is None else torch.as_tensor(np.asarray(table), dtype=dtype).contiguous().to(DEV)


def _run(ds, idx, out_hw, crop=None, tables=None, erase=None, mode="const", key=KEY, labels=True, out=None):
    from kanvit import ops
    d = ds["dev"]
    t = (None, None, None) if tables is None else (_dev(tables[0], torch.int64), _dev(tables[1], torch.float32), _dev(tables[2], torch.int32))
    return ops.erase_u8(d["images"], d["labels"] if labels else None, torch.as_tensor(idx, dtype=torch.int64).to(DEV), d["lut"], out_hw,
                        _dev(crop, torch.int32), *t, erase=_dev(erase, torch.int32), noise=_noise()[1] if mode == "pixel" else None, noise_key=key, out=out)


def _want(ds, crop, out_hw, erase, mode, key=KEY):
    """a' of every sample of the dataset (NumPy float32 [N, C, OH, OW])."""
    C = ds["C"]
    return er.reference(ds["images"].numpy(), MEAN[:C], STD[:C], None if crop is None else np.asarray(crop), out_hw, np.asarray(erase),
                        _noise()[0] if mode == "pixel" else None, key)


def _same(got, want):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    return all(torch.equal(g.cpu(), torch.from_numpy(np.asarray(w))) for g, w in zip(got, want))


def _pad_table(n, hw, pad):
    from kanvit import data
    return data.crop_table(n, EPOCH, SEED, hw, "pad", pad=pad, flip=True).numpy()


# left edges at x = 1, 2, 3, 5 and right edges at 6, 7: inside a 4-wide vector; rows 4 and 8 are item boundaries (RES_ROWS = 4)
HAND = [(2, 6, 1, 6),                   # 0: top and bottom inside the two items, left edge at 1, right at 6
        (0, 4, 2, 7),                   # 1: exactly the first item's rows
        (4, 8, 3, 7),                   # 2: exactly the second item's rows
        (1, 7, 5, 6),                   # 3: one column
        (3, 5, 0, 8),                   # 4: whole vectors, rows across the item boundary
        (0, 8, 0, 8),                   # 5: the whole image
        (0, 0, 0, 0),                   # 6: all zero
        (6, 2, 1, 7),                   # 7: inverted rows
        (1, 7, 6, 2),                   # 8: inverted columns
        (-3, 100, -3, 100),             # 9: reaching outside on every side: the whole image
        (-3, 5, 2, 100),                # 10: reaching outside on two
        (IMIN, IMAX, IMIN, IMAX),       # 11: the whole image again
        (IMAX, IMIN, 0, 8),             # 12: nothing
        (3, IMAX, IMIN, 4),             # 13
        (IMIN, 3, 5, IMAX),             # 14
        (8, 12, 0, 8)]                  # 15: below the image: nothing
WHOLE, NOTHING = (5, 9, 11), (6, 7, 8, 12, 15)


@pytest.mark.parametrize("mode", ["const", "pixel"])
def test_hand_made_boxes_at_the_identity_size(mode):
    n = len(HAND)
    ds = _dataset(n, (8, 8, 3), 7)
    crop, erase = _pad_table(n, (8, 8), 2), np.array(HAND, np.int32)
    x, y = _run(ds, range(n), (8, 8), crop, erase=erase, mode=mode)
    assert x.data_ptr() % 16 == 0                        # the 16-byte store form
    want = _want(ds, crop, (8, 8), erase, mode)
    assert _same((x, y), er.batch(want, ds["pad"], range(n), ds["labels"]))
    plain = rr.resample_all(ds["images"].numpy(), MEAN[:3], STD[:3], crop, (8, 8))
    x = x.cpu().numpy()
    for s in NOTHING:
        assert np.array_equal(x[s], plain[s]), s
    for s in WHOLE:
        fill = er.noise_plane(_noise()[0], KEY, s, (3, 8, 8)) if mode == "pixel" else np.zeros((3, 8, 8), np.float32)
        assert np.array_equal(x[s], fill), s
    assert np.array_equal(x[0][:, 2:6, 1:6], want[0][:, 2:6, 1:6]) and np.array_equal(x[0][:, :2], plain[0][:, :2])
    assert np.array_equal(x[0][:, 2:6, :1], plain[0][:, 2:6, :1]) and np.array_equal(x[0][:, 2:6, 6:], plain[0][:, 2:6, 6:])
    assert (x[0][:, 2:6, 1:6] != plain[0][:, 2:6, 1:6]).any()


@pytest.mark.parametrize("mode", ["const", "pixel"])
def test_scalar_store_form(mode):
    """7x9x1 -> 7x9: an odd width; and 8x8x3 -> 8x8 into a view 4 bytes off the 16-byte grid."""
    from kanvit import data
    n = 12
    ds = _dataset(n, (7, 9, 1), 791)
    crop, erase = _pad_table(n, (7, 9), (3, 2)), data.erase_table(n, EPOCH, SEED, (7, 9), prob=1.0).numpy()
    erase[0], erase[1] = (0, 7, 0, 9), (2, 5, 8, 9)      # the whole image; the last column
    x, y = _run(ds, range(n), (7, 9), crop, erase=erase, mode=mode)
    assert x.shape == (n, 1, 7, 9)
    assert _same((x, y), er.batch(_want(ds, crop, (7, 9), erase, mode), ds["pad"], range(n), ds["labels"]))
    n = len(HAND)
    ds = _dataset(n, (8, 8, 3), 7)
    crop, erase = _pad_table(n, (8, 8), 2), np.array(HAND, np.int32)
    buf = torch.empty(n * 3 * 8 * 8 + 4, device=DEV)
    out = buf[1:1 + n * 3 * 8 * 8].view(n, 3, 8, 8)
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4
    x, y = _run(ds, range(n), (8, 8), crop, erase=erase, mode=mode, out=out)
    assert x.data_ptr() == out.data_ptr()
    assert _same((x, y), er.batch(_want(ds, crop, (8, 8), erase, mode), ds["pad"], range(n), ds["labels"]))


@pytest.mark.parametrize("rows,mode", [("pad", "const"), ("pad", "pixel"), ("rrc", "pixel")])
def test_upsampling_through_the_window_path(rows, mode):
    """8x8 -> 22x32: a magnification of 4 along x, so every vector goes through the windows; 22 = 5 * 4 + 2 rows."""
    from kanvit import data
    n, out = 24, (22, 32)
    ds = _dataset(n, (8, 8, 3), 88)
    crop = _pad_table(n, (8, 8), 2) if rows == "pad" else data.crop_table(n, EPOCH, SEED, (8, 8), "rrc", scale=(0.25, 1.0)).numpy()
    erase = data.erase_table(n, EPOCH, SEED, out, prob=1.0).numpy()
    erase[:4] = [(0, 22, 0, 32), (20, 22, 30, 32), (3, 9, 5, 27), (0, 0, 0, 0)]
    x, y = _run(ds, range(n), out, crop, erase=erase, mode=mode)
    assert _same((x, y), er.batch(_want(ds, crop, out, erase, mode), ds["pad"], range(n), ds["labels"]))


@pytest.mark.parametrize("out", [(5, 5), (6, 8)])
def test_downscale_through_the_tap_path(out):
    from kanvit import data
    n = 24
    ds = _dataset(n, (8, 8, 3), 88)
    crop = _pad_table(n, (8, 8), 2)
    erase = data.erase_table(n, EPOCH, SEED, out, prob=1.0).numpy()
    assert ((erase[:, 1] > erase[:, 0]) & (erase[:, 3] > erase[:, 2])).sum() >= n // 2
    for mode in ("const", "pixel"):
        x, y = _run(ds, range(n), out, crop, erase=erase, mode=mode)
        assert _same((x, y), er.batch(_want(ds, crop, out, erase, mode), ds["pad"], range(n), ds["labels"])), mode


def _mix_tables(H, W):
    """N = 6: 0 unmixed; 1 CutMix with 2, whose erase box overlaps the cut; 2 Mixup with 3, both erased; 3 Mixup with itself; 4 a
    partner outside the dataset; 5 CutMix with itself."""
    partner = np.array([-1, 2, 3, 3, 6, 5], np.int64)
    weight = np.array([1.0, 0.5625, 0.3, 0.625, 0.25, 0.75], np.float32)
    box = np.array([(0, 0, 0, 0), (2, 10, 2, 10), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (1, 7, 3, 9)], np.int32)
    erase = np.array([(2, 9, 3, 10), (0, 6, 0, 6), (4, 12, 5, 11), (3, 8, 1, 7), (5, 11, 2, 6), (0, 4, 0, 12)], np.int32)
    assert H == 12 and W == 12
    return (partner, weight, box), erase


@pytest.mark.parametrize("mode", ["const", "pixel"])
def test_mixing_takes_the_partner_erased_under_its_own_row(mode):
    n, out = 6, (12, 12)
    ds = _dataset(n, (8, 8, 3), 66)
    crop = _pad_table(n, (8, 8), 2)
    tables, erase = _mix_tables(*out)
    got = _run(ds, range(n), out, crop, tables, erase, mode)
    want = _want(ds, crop, out, erase, mode)
    assert _same(got, er.batch(want, ds["pad"], range(n), ds["labels"], tables))
    x, y, y2, w = (t.cpu().numpy() for t in got)
    plain = rr.resample_all(ds["images"].numpy(), MEAN[:3], STD[:3], crop, out)
    fill = [er.noise_plane(_noise()[0], KEY, s, (3, 12, 12)) if mode == "pixel" else np.zeros((3, 12, 12), np.float32) for s in range(n)]
    assert np.array_equal(x[0], want[0]) and np.array_equal(x[0][:, 2:9, 3:10], fill[0][:, 2:9, 3:10])          # unmixed, erased
    # 1: inside the cut (2..10 x 2..10) the partner shows -- its fill where ITS box (4..12 x 5..11) lies, its pixels elsewhere;
    # outside the cut the sample's own fill (0..6 x 0..6) and its own pixels
    assert np.array_equal(x[1][:, 4:10, 5:10], fill[2][:, 4:10, 5:10]) and np.array_equal(x[1][:, 2:4, 2:10], plain[2][:, 2:4, 2:10])
    assert np.array_equal(x[1][:, 0:2, 0:6], fill[1][:, 0:2, 0:6]) and np.array_equal(x[1][:, 2:6, 0:2], fill[1][:, 2:6, 0:2])
    assert np.array_equal(x[1][:, 10:, :], plain[1][:, 10:, :])
    # 2: Mixup of two erased samples: where both boxes lie (4..8 x 5..7) the float32 blend of the two fills
    ws = np.float32(0.3)
    both = (ws * fill[2][:, 4:8, 5:7]) + ((np.float32(1) - ws) * fill[3][:, 4:8, 5:7])
    assert both.dtype == np.float32 and np.array_equal(x[2][:, 4:8, 5:7], both)
    if mode == "pixel":
        assert (both != fill[2][:, 4:8, 5:7]).any() and (both != fill[3][:, 4:8, 5:7]).any()
    assert y2[4] == y[4] and y2[1] == ds["labels"][2] and w[4] == np.float32(0.25)      # a partner outside [0, N): unmixed ...
    assert np.array_equal(x[4], want[4]) and np.array_equal(x[4][:, 5:11, 2:6], fill[4][:, 5:11, 2:6])         # ... but erased
    assert np.array_equal(x[5], want[5])                 # CutMix with itself: a' either way


def test_no_erase_table_is_resample_u8():
    from kanvit import ops
    n, out = 6, (12, 12)
    ds = _dataset(n, (8, 8, 3), 66)
    d = ds["dev"]
    crop = _pad_table(n, (8, 8), 2)
    tables, _ = _mix_tables(*out)
    idx = torch.arange(n, device=DEV)
    dev_tables = (_dev(tables[0], torch.int64), _dev(tables[1], torch.float32), _dev(tables[2], torch.int32))
    for t in ((), dev_tables):
        got = _run(ds, range(n), out, crop, tables if t else None, erase=None)
        ref = ops.resample_u8(d["images"], d["labels"], idx, d["lut"], out, _dev(crop, torch.int32), *t)
        assert len(got) == len(ref) == (4 if t else 2) and all(torch.equal(a, b) for a, b in zip(got, ref))
    nothing = np.zeros((n, 4), np.int32)                 # and a table that erases nothing changes nothing
    assert torch.equal(_run(ds, range(n), out, crop, erase=nothing, mode="pixel")[0], ops.resample_u8(d["images"], d["labels"], idx, d["lut"], out, _dev(crop, torch.int32))[0])


@pytest.mark.parametrize("mixing", [False, True])
def test_idx_outside_the_dataset_is_padding_whatever_the_erase_row(mixing):
    n, out = 6, (12, 12)
    ds = _dataset(n, (8, 8, 3), 66)
    crop = _pad_table(n, (8, 8), 2)
    tables, _ = _mix_tables(*out)
    erase = np.array([(0, 12, 0, 12)] * n, np.int32)     # the whole image, at every index
    idx = [-1, 0, n, 2, -2 ** 40, 2 ** 40]
    got = _run(ds, idx, out, crop, tables if mixing else None, erase, "pixel")
    assert _same(got, er.batch(_want(ds, crop, out, erase, "pixel"), ds["pad"], idx, ds["labels"], tables if mixing else None))
    x, y = got[0].cpu(), got[1].cpu()
    pad = torch.from_numpy(ds["pad"])[:, None, None].expand(3, 12, 12)
    for b in (0, 2, 4, 5):
        assert torch.equal(x[b], pad) and int(y[b]) == -1, b
    assert not torch.equal(x[1], pad) and int(y[1]) == int(ds["labels"][0])


@pytest.mark.parametrize("mode", ["const", "pixel"])
def test_a_samples_pixels_do_not_depend_on_the_batching(mode):
    n, out = 6, (12, 12)
    ds = _dataset(n, (8, 8, 3), 66)
    crop = _pad_table(n, (8, 8), 2)
    _, erase = _mix_tables(*out)
    alone = _run(ds, [2], out, crop, erase=erase, mode=mode)[0]
    many = _run(ds, [5, 0, 2, 1, 2, 4, 3], out, crop, erase=erase, mode=mode)[0]
    assert torch.equal(many[2], alone[0]) and torch.equal(many[4], alone[0])
    # as the partner of sample 1 under a cut box that covers the image, sample 2 comes out as it does on its own
    tables = (np.array([-1, 2, -1, -1, -1, -1], np.int64), np.array([1, 0, 1, 1, 1, 1], np.float32), np.array([(0, 0, 0, 0), (0, 12, 0, 12)] + [(0, 0, 0, 0)] * 4, np.int32))
    pasted = _run(ds, [1], out, crop, tables, erase, mode)[0]
    assert torch.equal(pasted[0], alone[0])
    assert torch.equal(alone.cpu(), torch.from_numpy(_want(ds, crop, out, erase, mode)[2:3]))


def test_one_batch_past_the_grid_cap():
    """4 stored images, 48 batch entries at 256x256: 48 * 3 * 64 * 64 work items, so threads walk on to a second item."""
    from kanvit import data
    n, B, out = 4, 48, (256, 256)
    assert B * 3 * (out[0] // 4) * (out[1] // 4) > GRID_ITEMS
    ds = _dataset(n, (8, 8, 3), 4)
    crop = _pad_table(n, (8, 8), 2)
    erase = data.erase_table(n, EPOCH, SEED, out, prob=1.0).numpy()
    erase[3] = (100, 101, 0, 256)                        # one whole row
    idx = [(7 * b + b // 5) % n for b in range(B)]
    x, y = _run(ds, idx, out, crop, erase=erase, mode="pixel")
    want = torch.from_numpy(_want(ds, crop, out, erase, "pixel")).to(DEV)
    assert torch.equal(x, want[torch.tensor(idx, device=DEV)])
    assert torch.equal(y.cpu(), ds["labels"][idx])


def test_noise_statistics():
    """One whole-image erase at 64x64x3: 12 288 looked-up values.  Five sigmas of their mean are 0.045 and of their std 0.032."""
    ds = _dataset(4, (8, 8, 3), 4)
    erase = np.array([(0, 64, 0, 64)] * 4, np.int32)
    x = _run(ds, [0, 1], (64, 64), None, erase=erase, mode="pixel")[0].cpu().double()
    for b in range(2):
        assert abs(float(x[b].mean())) <= 0.05 and abs(float(x[b].std()) - 1.0) <= 0.05, b
    planes = [x[0, 0], x[0, 1], x[0, 2], x[1, 0], x[1, 1], x[1, 2]]
    for i in range(6):
        for j in range(i + 1, 6):
            a, b = planes[i].flatten(), planes[j].flatten()
            assert float((a == b).double().mean()) < 0.01          # 4096 levels: equal values by chance are 1 in thousands
            assert abs(float(torch.corrcoef(torch.stack([a, b]))[0, 1])) < 0.08       # 1 / sqrt(4096) = 0.016: five sigmas
    assert set(np.unique(x[0].numpy().astype(np.float32))) <= set(_noise()[0].tolist())


def test_replayed_from_a_graph():
    from kanvit import ops
    n, out = 6, (12, 12)
    ds = _dataset(n, (8, 8, 3), 66)
    d = ds["dev"]
    tables, erase = _mix_tables(*out)
    args = (d["images"], d["labels"], torch.arange(n, device=DEV), d["lut"], out, _dev(_pad_table(n, (8, 8), 2), torch.int32),
            _dev(tables[0], torch.int64), _dev(tables[1], torch.float32), _dev(tables[2], torch.int32))
    kw = dict(erase=_dev(erase, torch.int32), noise=_noise()[1], noise_key=KEY)      # every operand is on the device before the capture
    eager = ops.erase_u8(*args, **kw)                    # loads the library outside the capture
    static = torch.zeros_like(eager[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = ops.erase_u8(*args, **kw, out=static)
    static.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert held[0].data_ptr() == static.data_ptr() and all(torch.equal(a, b) for a, b in zip(held, eager))


def test_wrapper_refuses_wrong_operands():
    from kanvit import ops
    from kanvit.ops import KanvitError
    n = 6
    ds = _dataset(n, (8, 8, 3), 66)
    d = ds["dev"]
    idx = torch.arange(n, device=DEV)
    erase, noise = torch.zeros((n, 4), dtype=torch.int32, device=DEV), _noise()[1]

    def call(**kw):
        return ops.erase_u8(d["images"], d["labels"], idx, d["lut"], (8, 8), **kw)

    for kw, word in ((dict(erase=erase.long()), "erase has dtype"), (dict(erase=erase[:, :3].contiguous()), "erase has shape"),
                     (dict(erase=erase[:5]), "erase has shape"), (dict(erase=erase.cpu()), "erase is on cpu"),
                     (dict(erase=torch.zeros((n, 8), dtype=torch.int32, device=DEV)[:, ::2]), "not contiguous"),
                     (dict(erase=erase, noise=noise.double()), "noise has dtype"), (dict(erase=erase, noise=noise[:4095]), "noise has shape"),
                     (dict(erase=erase, noise=noise[:1]), "noise has shape"), (dict(erase=erase, noise=noise.view(64, 64)), "noise has shape"),
                     (dict(erase=erase, noise=noise.cpu()), "noise is on cpu"), (dict(noise=noise), "noise without erase")):
        with pytest.raises(ValueError, match=word) as e:
            call(**kw)
        assert isinstance(e.value, KanvitError)
    with pytest.raises(KanvitError, match="come together"):
        call(erase=erase, partner=torch.zeros(n, dtype=torch.int64, device=DEV))
    assert torch.equal(call(erase=erase, noise=noise[:2].contiguous())[0], call()[0])       # the shortest table is accepted


# ---- GpuDataset(erase=...) ------------------------------------------------------------------------------------------------------
N_DS, OUT_DS, ERASE_DS = 40, (16, 16), dict(prob=0.5)
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5)


def _gpu_dataset(mode):
    from kanvit import data
    ds = _dataset(N_DS, (8, 8, 3), 8)
    return ds, data.GpuDataset(ds["images"], ds["labels"], MEAN[:3], STD[:3], DEV, pad=2, flip=True, out_size=OUT_DS, erase=dict(ERASE_DS, mode=mode))


def _epoch_reference(ds, mode, epoch, seed):
    """a' of all N_DS samples for one epoch, from the tables data.py documents (tests/test_erase_cpu.py and tests/test_resample_cpu.py
    restate those)."""
    from kanvit import data
    key = ("epoch", mode, epoch, seed)
    if key not in _cache:
        crop = data.crop_table(N_DS, epoch, seed, (8, 8), "pad", pad=2, flip=True).numpy()
        erase = data.erase_table(N_DS, epoch, seed, OUT_DS, prob=0.5).numpy()
        _cache[key] = _want(ds, crop, OUT_DS, erase, mode, data.erase_noise_key(seed, epoch))
    return _cache[key]


@pytest.mark.parametrize("mode,mixing", [("pixel", False), ("pixel", True), ("const", True)])
def test_gpu_dataset_epoch_equals_the_restatement(mode, mixing):
    from kanvit import data
    ds, gd = _gpu_dataset(mode)
    assert gd.resample and (gd.noise is not None) == (mode == "pixel")
    order = data.epoch_indices(N_DS, EPOCH, SEED).tolist()
    tables = tuple(t.numpy() for t in data.mix_table(N_DS, EPOCH, SEED, OUT_DS, **MIX)) if mixing else None
    fed = list(gd.batches(16, EPOCH, SEED, mix=MIX if mixing else None))
    assert [b[0].shape[0] for b in fed] == [16, 16, 8] and all(len(b) == (4 if mixing else 2) for b in fed)
    want = _epoch_reference(ds, mode, EPOCH, SEED)
    for i, b in enumerate(fed):
        assert _same(b, er.batch(want, ds["pad"], order[16 * i:16 * i + 16], ds["labels"], tables)), i
    erased = (data.erase_table(N_DS, EPOCH, SEED, OUT_DS, prob=0.5) != 0).any(1)
    assert 5 < int(erased.sum()) < 35                    # the epoch erases some samples and leaves some


def test_gpu_dataset_epochs_differ_and_ranks_agree():
    from kanvit import data
    ds, gd = _gpu_dataset("pixel")

    def by_sample(epoch, rank, world):
        order = data.epoch_indices(N_DS, epoch, SEED, rank, world).tolist()
        x = torch.cat([b[0] for b in gd.batches(16, epoch, SEED, rank, world)]).cpu()
        return dict(zip(order, x))

    e0, e1 = by_sample(0, 0, 1), by_sample(1, 0, 1)
    assert sorted(e0) == list(range(N_DS)) and any(not torch.equal(e0[s], e1[s]) for s in e0)
    halves = {**by_sample(0, 0, 2), **by_sample(0, 1, 2)}
    assert sorted(halves) == list(range(N_DS)) and all(torch.equal(halves[s], e0[s]) for s in e0)
    want = _epoch_reference(ds, "pixel", 0, SEED)
    assert all(torch.equal(e0[s], torch.from_numpy(want[s])) for s in e0)


def test_gpu_dataset_at_the_stored_size_goes_through_erase_u8():
    """No out_size and the padded crop: with `erase` the batches come from ops.erase_u8 under crop_table(mode="pad") rows."""
    from kanvit import data
    ds = _dataset(N_DS, (8, 8, 3), 8)
    gd = data.GpuDataset(ds["images"], ds["labels"], MEAN[:3], STD[:3], DEV, pad=2, flip=True, erase=dict(prob=1.0, mode="const"))
    plain = data.GpuDataset(ds["images"], ds["labels"], MEAN[:3], STD[:3], DEV, pad=2, flip=True)
    assert gd.resample and not plain.resample and plain.erase is None and plain.noise is None
    erase = data.erase_table(N_DS, 0, SEED, (8, 8), prob=1.0).numpy()
    order = data.epoch_indices(N_DS, 0, SEED).tolist()
    for i, ((x, y), (px, py)) in enumerate(zip(gd.batches(16, 0, SEED), plain.batches(16, 0, SEED))):
        assert torch.equal(y, py)
        for b, s in enumerate(order[16 * i:16 * i + 16]):
            m = torch.from_numpy(er.inside(erase[s], 8, 8)).to(DEV)
            assert bool(m.any()) and torch.equal(x[b], torch.where(m[None], torch.zeros((), device=DEV), px[b])), (i, b)


# ---- train.main -------------------------------------------------------------------------------------------------------------------
TRAIN = ["--model-type", "cheby", "--n-patches", "2", "--n-blocks", "2", "--n-heads", "2", "--d-hidden", "64", "--out-d", "4",
         "--batch-size", "16", "--crop-padding", "2", "--no-tuned-gemms", "--epochs", "1"]       # the geometry of tests/test_gpu_data_gpu.py
RECIPE = ["--mixup", "0.8", "--cutmix", "1.0", "--resize", "16"]


@pytest.fixture(scope="module")
def npz_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("npz") / "tiny.npz")
    np.savez(path, x_train=_images(40, 8, 8, 3, 8).numpy(), y_train=(np.arange(40) % 4).astype(np.uint8))
    return path


@pytest.mark.parametrize("mode", ["pixel", "const"])
@pytest.mark.parametrize("recipe", [False, True], ids=["plain", "recipe"])
def test_train_main_eager_and_replayed_from_a_graph(npz_file, tmp_path, mode, recipe):
    import train
    argv = [*TRAIN, *(RECIPE if recipe else []), "--data-npz", npz_file, "--random-erasing", "0.5", "--erase-mode", mode]
    eager = train.main(train.parse([*argv, "--log-dir", str(tmp_path / "e")]))
    assert len(eager["losses"]) == 3 and all(np.isfinite(eager["losses"]))
    graphed = train.main(train.parse([*argv, "--graph", "--log-dir", str(tmp_path / "g")]))
    assert graphed["losses"] == eager["losses"]


def test_train_main_feeds_the_datasets_batches(npz_file, tmp_path):
    import train
    from kanvit import data
    run = train.main(train.parse([*TRAIN, "--data-npz", npz_file, "--random-erasing", "0.5", "--log-dir", str(tmp_path / "a")]))
    gd = data.GpuDataset.from_npz(npz_file, "train", DEV, pad=2, flip=True, erase=dict(prob=0.5, mode="pixel"))
    fed = list(gd.batches(16, 0, 0))
    args = train.parse([*TRAIN, "--synthetic", "--image-size", "8", "--log-dir", str(tmp_path / "b")])
    assert train.main(args, batches=fed)["losses"] == run["losses"]
    unerased = list(data.GpuDataset.from_npz(npz_file, "train", DEV, pad=2, flip=True).batches(16, 0, 0))
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(fed, unerased))


def test_train_random_erasing_0_changes_nothing(npz_file, tmp_path):
    import train
    streams = []
    for extra in ([], ["--random-erasing", "0"]):
        args = train.parse([*TRAIN, *RECIPE, "--data-npz", npz_file, *extra, "--log-dir", str(tmp_path / f"l{len(extra)}")])
        train_set, _ = train.npz_datasets(args, torch.device(DEV), want_test=False)
        assert train_set.erase is None and train_set.noise is None
        streams.append(list(train_set.batches(16, 0, args.seed, mix=train.mix_config(args))))
    assert len(streams[0]) == len(streams[1]) == 3
    assert all(torch.equal(a, b) for x, y in zip(*streams) for a, b in zip(x, y))
    plain = train.npz_datasets(train.parse([*TRAIN, "--data-npz", npz_file, "--random-erasing", "0", "--log-dir", str(tmp_path / "p")]), torch.device(DEV), False)[0]
    assert not plain.resample                            # ops.augment_u8, call for call
