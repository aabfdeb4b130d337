"""ops.soft_cross_entropy (csrc/soft_ce.hip: soft_ce_kernel) on the GPU against the float64 restatement of tests/_mix_ref.py.

The bound is relative to torch's own fp32 cross_entropy on the same device and the same inputs (probability targets plus
label_smoothing, forward and backward), measured against the same float64 values: with e_t its largest error of a case, the kernel may
be off by 2 e_t + 4 ulp of the value for the losses and by 2 e_t + 2^-22 for the gradient (entries in [-1, 1]); the factor 2 is the
room for a different, equally valid order of the sums.

e_t is taken per case (one shape, input kind, eps and target kind): the largest absolute error over the rows for `loss_rows` and over
the entries for the gradient; the ulp term is that of each row's own value.  Every case prints its figures before it asserts; DESIGN.md
section 4.20 has the measured table per shape and input (all 252 cases inside their bounds: at 130 x 1000 with standard-normal logits
the mean loss is off by 4.8e-7 against torch's 9.6e-7 and the gradient by 4.6e-10 against 4.2e-10)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _mix_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (257, 5, 5): one row in the mean kernel's second lap; (1000, 3, 4): four laps and a padded row stride
SHAPES = [(1, 2, 2), (5, 3, 3), (17, 100, 100), (130, 1000, 1000), (4, 1025, 1032), (257, 5, 5), (1000, 3, 4)]
MEAN_THREADS = 256                   # soft_ce_mean_kernel: one work-group, thread t adds rows t, t + 256, ...
assert any(s[0] == MEAN_THREADS + 1 for s in SHAPES) and any(s[0] > 3 * MEAN_THREADS and s[2] > s[1] for s in SHAPES)
INPUTS = ["normal", "pm80", "equal-row"]
TARGETS = ["plain", "w0", "w1", "w037", "same-label", "bad-label"]


def _logits(B, C, ld, kind, seed=0):
    """float32 [B, C] as a view with row stride ld of a device buffer whose padding holds NaN (never read)."""
    g = torch.Generator().manual_seed(1000 * B + C + seed)
    z = torch.randn(B, C, generator=g)
    if kind == "pm80":
        z = z * (80.0 / float(z.abs().max()))
    elif kind == "equal-row":
        z[B // 2] = 1.5
    buf = torch.full((B, ld), float("nan"))
    buf[:, :C] = z
    return buf.to(DEV)[:, :C], z.numpy()


def _targets(B, C, kind, seed=0):
    rng = np.random.default_rng(B * 7 + C + seed)
    y1, y2 = rng.integers(0, C, B), rng.integers(0, C, B)
    w = {"plain": None, "w0": 0.0, "w1": 1.0, "w037": 0.37, "same-label": 0.37, "bad-label": 0.37}[kind]
    if kind == "plain":
        return y1, None, None
    if kind == "same-label":
        y2 = y1.copy()
    if kind == "bad-label":
        (y1 if B % 2 else y2)[B - 1] = C if B % 3 else -1           # y1 or y2, just past the end or negative, by the shape
    return y1, y2, np.full(B, w, np.float32)


def _torch_ce(z, y1, y2, w, eps):
    """torch's fp32 answer on the device: (loss, rows, gradient of the mean).  A row with a label outside [0, C) has no torch form: its
    labels are clamped, and the row is masked out of the rows, of the sum (divisor B) and so of the gradient -- in fp32, by torch."""
    B, C = z.shape
    _, ok = mr.soft_targets(C, y1, y2, w, eps)
    a = torch.from_numpy(np.clip(y1, 0, C - 1)).to(DEV)
    zt = z.detach().clone().contiguous().requires_grad_(True)
    if y2 is None:
        target = F.one_hot(a, C).float()
    else:
        b, wt = torch.from_numpy(np.clip(y2, 0, C - 1)).to(DEV), torch.from_numpy(w).to(DEV)[:, None]
        target = wt * F.one_hot(a, C).float() + (1 - wt) * F.one_hot(b, C).float()
    rows = F.cross_entropy(zt, target, label_smoothing=eps, reduction="none")
    if ok.all():
        loss = F.cross_entropy(zt, target, label_smoothing=eps)
    else:
        rows = rows * torch.from_numpy(ok).to(DEV)
        loss = rows.sum() / B
    loss.backward()
    return float(loss.detach()), rows.detach().cpu().numpy().astype(np.float64), zt.grad.cpu().numpy().astype(np.float64)


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def _device_args(y1, y2, w):
    t = lambda v: None if v is None else torch.from_numpy(v).to(DEV)       # noqa: E731
    return t(y1), t(y2), t(w)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient_within_twice_torchs_own_error(shape, kind):
    from kanvit import ops
    B, C, ld = shape
    z, z_host = _logits(B, C, ld, kind)
    assert z.stride(0) == ld
    for eps in (0.0, 0.1):
        for tk in TARGETS:
            y1, y2, w = _targets(B, C, tk)
            want_loss, want_rows, want_dz = mr.soft_ce(z_host, y1, y2, w, eps)
            t_loss, t_rows, t_dz = _torch_ce(z, y1, y2, w, eps)
            loss, rows, dz = ops.soft_ce(z, *_device_args(y1, y2, w), label_smoothing=eps)
            assert dz.shape == (B, C) and dz.is_contiguous() and rows.shape == (B,) and loss.shape == ()
            loss, rows, dz = float(loss), rows.cpu().numpy().astype(np.float64), dz.cpu().numpy().astype(np.float64)
            e_loss, e_rows, e_dz = abs(t_loss - want_loss), np.abs(t_rows - want_rows).max(), np.abs(t_dz - want_dz).max()
            k_loss, k_rows, k_dz = abs(loss - want_loss), np.abs(rows - want_rows), np.abs(dz - want_dz).max()
            print(f"{shape} {kind} eps={eps} {tk}: loss {want_loss:.6g} torch {e_loss:.2e} kernel {k_loss:.2e} | rows torch {e_rows:.2e} "
                  f"kernel {k_rows.max():.2e} | grad torch {e_dz:.2e} kernel {k_dz:.2e}")
            assert k_loss <= 2 * e_loss + 4 * _ulp(want_loss), (eps, tk, k_loss, e_loss)
            assert (k_rows <= 2 * e_rows + 4 * _ulp(want_rows)).all(), (eps, tk, k_rows.max(), e_rows)
            assert k_dz <= 2 * e_dz + 2.0 ** -22, (eps, tk, k_dz, e_dz)
            if tk == "bad-label":
                assert rows[B - 1] == 0.0 and not dz[B - 1].any()


@pytest.mark.parametrize("B", [1, 130, 256, 257, 1000])
def test_mean_equals_the_restatement_of_its_own_rows_bitwise(B):
    """The second kernel given its input: `loss` is mr.mean_rows_f32 of the returned `loss_rows`, bit for bit, below, at and past one
    lap of 256 rows.  With "bad-label" the last row has a bad label: it counts 0 and the divisor stays B (at B = 257 that row is the
    whole second lap, so the same batch runs with every label good as well)."""
    from kanvit import ops
    C = 5
    z, _ = _logits(B, C, C + 1, "normal", seed=11)
    for tk in ("bad-label", "w037"):
        y1, y2, w = _targets(B, C, tk, seed=11)
        loss, rows, _ = ops.soft_ce(z, *_device_args(y1, y2, w), label_smoothing=0.1)
        loss, rows = loss.cpu().numpy(), rows.cpu().numpy()
        bad = tk == "bad-label"
        assert rows.dtype == np.float32 and rows.shape == (B,) and (rows[:B - 1] > 0.0).all() and (rows[B - 1] == 0.0) == bad
        want = mr.mean_rows_f32(rows)
        assert np.array_equal(loss.view(np.uint32), want.view(np.uint32)), (B, tk, float(loss), float(want))
        if B > MEAN_THREADS and (not bad or B > MEAN_THREADS + 1):       # what a walk that stops after its first lap would return
            first_lap = mr.mean_rows_f32(rows[:MEAN_THREADS]) * np.float32(MEAN_THREADS) / np.float32(B)
            assert rows[MEAN_THREADS:].sum() > 0.0 and first_lap != want, (B, tk)
        if bad and B > 1:                                # the bad row is in the divisor: the mean of the good rows alone is another number
            assert mr.mean_rows_f32(rows[:B - 1]) != want


@pytest.fixture(scope="module")
def big():
    """The 130 x 1000 case with Mixup pairs and smoothing, run once."""
    from kanvit import ops
    B, C, ld = 130, 1000, 1000
    z, _ = _logits(B, C, ld, "normal", seed=5)
    y1, y2, w = _device_args(*_targets(B, C, "w037", seed=5))
    w = torch.rand(B, generator=torch.Generator().manual_seed(3)).to(DEV)
    out = ops.soft_ce(z, y1, y2, w, label_smoothing=0.1)
    return dict(z=z, y1=y1, y2=y2, w=w, out=[t.clone() for t in out])


def test_two_runs_give_the_same_bits(big):
    from kanvit import ops
    again = ops.soft_ce(big["z"], big["y1"], big["y2"], big["w"], label_smoothing=0.1)
    assert all(torch.equal(a, b) for a, b in zip(again, big["out"]))


@pytest.mark.parametrize("r", [0, 63, 129])
def test_a_row_alone_gives_the_bits_it_gives_inside_the_batch(big, r):
    """The row's loss bitwise; its gradient bitwise up to the documented factor: inside the batch it is the row's own (softmax - t)
    times fp32(1 / 130), alone (B = 1) times 1."""
    from kanvit import ops
    loss, rows, dz = ops.soft_ce(big["z"][r:r + 1], big["y1"][r:r + 1], big["y2"][r:r + 1], big["w"][r:r + 1], label_smoothing=0.1)
    assert torch.equal(rows[0], big["out"][1][r]) and torch.equal(loss, rows[0])
    inv = np.float32(1) / np.float32(130)
    assert np.array_equal((dz[0].cpu().numpy() * inv).view(np.uint32), big["out"][2][r].cpu().numpy().view(np.uint32))


def test_autograd_scales_the_stored_gradient(big):
    from kanvit import ops
    z = big["z"].detach().clone().requires_grad_(True)
    loss = ops.soft_cross_entropy(z, big["y1"], big["y2"], big["w"], label_smoothing=0.1)
    assert torch.equal(loss.detach(), big["out"][0])
    (0.5 * loss).backward()
    assert torch.equal(z.grad, 0.5 * big["out"][2])
    plain = ops.soft_cross_entropy(z.detach(), big["y1"])
    assert abs(float(plain) - float(F.cross_entropy(z.detach(), big["y1"]))) < 1e-5


def test_wrapper_checks_its_operands(big):
    from kanvit import KanvitError, ops
    z, y = big["z"], big["y1"]
    with pytest.raises(KanvitError, match="come together"):
        ops.soft_cross_entropy(z, y, big["y2"])
    with pytest.raises(KanvitError, match="dtype"):
        ops.soft_cross_entropy(z.bfloat16(), y)
    with pytest.raises(KanvitError, match="strides"):
        ops.soft_cross_entropy(z.t(), y[:1000].repeat(2)[:1000])
    with pytest.raises(KanvitError, match="shape"):
        ops.soft_cross_entropy(z, y[:5])
    with pytest.raises(KanvitError, match="label_smoothing"):
        ops.soft_cross_entropy(z, y, label_smoothing=1.0)
