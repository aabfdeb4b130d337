"""ops.mix_u8 (csrc/batch_u8.hip: mix_u8_kernel) on the GPU against the float32 restatement of tests/_mix_ref.py -- BITWISE: CutMix
only looks values up, and Mixup is three roundings the compiler may not contract, which NumPy's float32 operations repeat.  A
hand-built table holds every kind of row (tests/_mix_ref.hand_table); the shapes cover both store forms (W = 8, 12: 16 bytes per lane;
W = 6: the scalar form) and every channel count the table is staged for on both sides of three channels."""
import numpy as np
import pytest
import torch

from tests import _mix_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, SEED, EPOCH = 37, 3, 2
MEAN, STD = [0.5071, 0.4867, 0.4408, 0.45], [0.2675, 0.2565, 0.2761, 0.25]
SHAPES = [(8, 8, 3), (6, 6, 1), (8, 12, 4)]
BATCHES = {1: [2], 5: [5, 2, 6, 0, 7]}          # B = 64 > N: drawn, every sample at least once (below)
_cache = {}


def _images(H, W, C):
    g = torch.Generator().manual_seed(100 * H + 10 * W + C)
    x = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, generator=g)
    x.view(-1)[:3] = torch.tensor([0, 255, 1], dtype=torch.uint8)
    return x[..., 0].contiguous() if C == 1 else x


def _case(shape, pad, flip):
    """Dataset, table, device copies and the reference operands of one (shape, pad, flip), computed once and left unchanged."""
    key = (shape, pad, flip)
    if key not in _cache:
        from kanvit import data
        H, W, C = shape
        images, labels = _images(H, W, C), (torch.arange(N) * 5 + 1) % 11
        table = mr.hand_table(N, H, W, seed=H + W)
        _cache[key] = dict(images=images, labels=labels, table=table, aug=mr.augment_all(images, MEAN[:C], STD[:C], pad, flip, SEED, EPOCH),
                           dev=dict(images=images.to(DEV), labels=labels.to(DEV), lut=data.make_lut(MEAN[:C], STD[:C]).to(DEV),
                                    table=[torch.from_numpy(t).to(DEV) for t in table]))
    return _cache[key]


def _idx(B):
    if B in BATCHES:
        return BATCHES[B]
    rng = np.random.default_rng(B)
    return np.concatenate([rng.permutation(N), rng.permutation(N)[:B - N]]).tolist()


def _run(c, idx, pad, flip, table=None, seed=SEED, epoch=EPOCH, out=None):
    from kanvit import ops
    d = c["dev"]
    return ops.mix_u8(d["images"], d["labels"], torch.tensor(idx, dtype=torch.int64, device=DEV), d["lut"], *(table or d["table"]),
                      pad=pad, flip=flip, seed=seed, epoch=epoch, out=out)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("pad", [(0, 0), (2, 2), (3, 1)])
@pytest.mark.parametrize("shape", SHAPES)
def test_batch_is_bitwise_the_restatement(shape, pad, flip, B):
    c, idx = _case(shape, pad, flip), _idx(B)
    x, y, y2, w = _run(c, idx, pad, flip)
    H, W, C = shape
    assert x.shape == (B, C, H, W) and x.dtype == torch.float32 and y.dtype == y2.dtype == torch.int64 and w.dtype == torch.float32
    want_x, want_y, want_y2, want_w = mr.mix(c["aug"], c["labels"].numpy(), idx, *c["table"])
    assert np.array_equal(_bits(x), want_x.view(np.uint32))
    assert np.array_equal(y.cpu().numpy(), want_y) and np.array_equal(y2.cpu().numpy(), want_y2)
    assert np.array_equal(_bits(w), want_w.view(np.uint32))
    if B == 64:
        assert set(idx) == set(range(N))                            # every kind of row of the hand-built table was there


GRID_ITEMS = 2048 * 256             # BATCH_MAX_GROUPS work-groups of 256 threads: past that many work items a thread takes a second one
# name -> ((H, W, C), B, pixels per work item, out= one element off the 16-byte grid)
LAP_CASES = {"vec 8x8x3": ((8, 8, 3), 11000, 4, False), "vec 8x12x4": ((8, 12, 4), 5500, 4, False),
             "scalar 6x6x1": ((6, 6, 1), 14600, 1, False), "scalar by alignment 8x8x3": ((8, 8, 3), 2750, 1, True)}


def _lap_idx(B):
    """The N samples repeated in a shuffled order, ending on a whole permutation."""
    rng = np.random.default_rng(B)
    return np.concatenate([rng.permutation(N) for _ in range(-(-B // N))])[-B:]


def _kinds(c, samples):
    """The kinds of table row among `samples`: unmixed, Mixup (a partner and an empty box), CutMix."""
    partner, _, box = c["table"]
    area = (box[:, 1] - box[:, 0]).clip(0) * (box[:, 3] - box[:, 2]).clip(0)
    return {"unmixed" if partner[s] < 0 else "cutmix" if area[s] > 0 else "mixup" for s in samples}


@pytest.mark.parametrize("name", list(LAP_CASES))
def test_batch_past_the_grid_cap_wraps_the_stride_loop(name):
    """More work items than a full grid has threads: the end of the batch -- pixels, and y, y2 and w of its last samples, which the
    thread of a sample's first item writes -- comes from a thread's second lap, and that lap holds unmixed, Mixup and CutMix rows.  A
    sample's output does not depend on its place, so the reference is the restatement of the N samples, gathered."""
    (H, W, C), B, vec, off = LAP_CASES[name]
    per_sample = H * C * (W // vec)
    assert B * per_sample > GRID_ITEMS and (vec == 4) == (W % 4 == 0 and not off)
    pad, flip = (2, 2), True
    c, idx = _case((H, W, C), pad, flip), _lap_idx(B)
    second_lap = idx[-(-GRID_ITEMS // per_sample):]                 # the samples that lie in the second lap whole
    assert len(second_lap) >= 16 and _kinds(c, second_lap) == {"unmixed", "mixup", "cutmix"}
    n = B * C * H * W
    buf = torch.full((n + 5,), float("nan"), device=DEV)
    view = buf[off:n + off].view(B, C, H, W)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    x, y, y2, w = _run(c, idx.tolist(), pad, flip, out=view)
    assert x.data_ptr() == view.data_ptr()
    got, rest = view.cpu().numpy(), buf.cpu()
    assert not np.isnan(got).any()
    assert torch.isnan(rest[:off]).all() and torch.isnan(rest[n + off:]).all()           # nothing written outside the view
    want_x, want_y, want_y2, want_w = mr.mix(c["aug"], c["labels"].numpy(), list(range(N)), *c["table"])
    assert np.array_equal(got.view(np.uint32), want_x[idx].view(np.uint32))
    assert np.array_equal(y.cpu().numpy(), want_y[idx]) and np.array_equal(y2.cpu().numpy(), want_y2[idx])
    assert np.array_equal(_bits(w), want_w[idx].view(np.uint32))
    assert (want_y[idx] != want_y2[idx]).any() and len(set(want_w[second_lap].tolist())) > 3


def test_the_table_holds_every_kind_of_row_and_mixing_changes_them():
    """What the parity test relies on: the kinds are present, and a mixed row differs from the unmixed one (the restatement is no
    identity) except where it must not -- Mixup with w = 1, and a sample cut with itself."""
    c = _case((8, 8, 3), (2, 2), True)
    partner, weight, box = c["table"]
    area = (box[:, 1] - box[:, 0]).clip(0) * (box[:, 3] - box[:, 2]).clip(0)
    assert (partner < 0).sum() >= 3 and ((partner >= 0) & (area == 0)).sum() >= 6 and (area > 0).sum() >= 6
    assert {0.0, 1.0, float(np.float32(0.3))} <= set(weight[(partner >= 0) & (area == 0)].tolist())
    assert partner[4] == 4 and partner[10] == 10 and area[5] == 64 and area[6] == 1 and tuple(box[8]) == (3, 3, 2, 5)
    plain = c["aug"]
    mixed, _, _, _ = mr.mix(plain, c["labels"].numpy(), list(range(N)), *c["table"])
    same = [i for i in range(N) if np.array_equal(mixed[i], plain[i])]
    assert set(same) >= {0, 3, 10} and {1, 2, 5, 6, 7, 8, 9} & set(same) == set()
    assert np.array_equal(mixed[1], 0 * plain[1] + plain[5]) and np.array_equal(mixed[5], plain[11])


def test_pixels_do_not_depend_on_the_batch_or_the_position():
    shape, pad, flip = (8, 12, 4), (3, 1), True
    c = _case(shape, pad, flip)
    whole = _run(c, list(range(N)), pad, flip)[0]
    for idx in ([2], [5, 2, 6, 0, 7], [7, 7, 36, 2], _idx(64)):
        x = _run(c, idx, pad, flip)[0]
        assert torch.equal(x, whole[idx])
    other = _run(c, list(range(N)), pad, flip, epoch=EPOCH + 1)[0]
    assert not torch.equal(other, whole)


@pytest.mark.parametrize("shape", SHAPES)
def test_an_unmixed_table_gives_augment_u8_bitwise(shape):
    from kanvit import ops
    pad, flip = (2, 2), True
    c = _case(shape, pad, flip)
    d = c["dev"]
    none = [torch.full((N,), -1, dtype=torch.int64, device=DEV), torch.ones(N, device=DEV), torch.zeros((N, 4), dtype=torch.int32, device=DEV)]
    idx = _idx(64)
    x, y, y2, w = _run(c, idx, pad, flip, table=none)
    ax, ay = ops.augment_u8(d["images"], d["labels"], torch.tensor(idx, device=DEV), d["lut"], pad, flip, SEED, EPOCH)
    assert torch.equal(x, ax) and torch.equal(y, ay) and torch.equal(y2, ay) and bool((w == 1).all())


def test_dataset_batches_with_a_mix_configuration():
    """GpuDataset.batches(mix=...): one table per epoch from data.mix_table, (x, y, y2, w) per batch; a sample's pixels and targets are
    the same at another batch size and when the epoch is split over two ranks."""
    from kanvit import data
    H, W, C = 8, 8, 3
    images, labels = _images(H, W, C), torch.arange(N)
    ds = data.GpuDataset(images, labels, MEAN[:C], STD[:C], DEV, pad=2, flip=True)
    mix = dict(mixup_alpha=0.8, cutmix_alpha=1.0)
    table = data.mix_table(N, 1, 9, (H, W), **mix)
    assert (table.partner >= 0).sum() > N // 2
    got = list(ds.batches(16, epoch=1, seed=9, mix=mix))
    assert [len(b[1]) for b in got] == [16, 16, 5] and all(len(b) == 4 for b in got)
    x, y, y2, w = (torch.cat([b[k] for b in got]).cpu() for k in range(4))
    assert torch.equal(y, data.epoch_indices(N, 1, 9))
    aug = mr.augment_all(images, MEAN[:C], STD[:C], 2, True, 9, 1)
    want = mr.mix(aug, labels.numpy(), y.tolist(), *(t.numpy() for t in table))
    assert np.array_equal(_bits(x), want[0].view(np.uint32)) and np.array_equal(y2.numpy(), want[2]) and np.array_equal(w.numpy(), want[3])
    by_sample = {int(s): (x[i], int(y2[i]), float(w[i])) for i, s in enumerate(y)}
    again = [b for r in range(2) for b in ds.batches(7, epoch=1, seed=9, rank=r, world=2, mix=mix)]
    seen = set()
    for bx, by, by2, bw in again:
        for i, s in enumerate(by.tolist()):
            px, p2, pw = by_sample[s]
            assert torch.equal(bx[i].cpu(), px) and int(by2[i]) == p2 and float(bw[i]) == pw
            seen.add(s)
    assert seen == set(range(N))
    assert all(len(b) == 2 for b in ds.batches(16, epoch=1, seed=9))            # without `mix`: today's pairs


def test_wrapper_checks_its_operands():
    from kanvit import KanvitError
    c = _case((8, 8, 3), (2, 2), True)
    p, w, box = c["dev"]["table"]
    with pytest.raises(KanvitError, match="partner"):
        _run(c, [0], 0, False, table=[p.int(), w, box])
    with pytest.raises(KanvitError, match="weight"):
        _run(c, [0], 0, False, table=[p, w[:5], box])
    with pytest.raises(KanvitError, match="box"):
        _run(c, [0], 0, False, table=[p, w, box.reshape(-1)])
    with pytest.raises(KanvitError, match="pad_y"):
        _run(c, [0], 33, False)
    x, y, y2, w_out = _run(c, [], 0, False)
    assert x.shape == (0, 3, 8, 8) and y.shape == y2.shape == w_out.shape == (0,)
