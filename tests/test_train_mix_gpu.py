"""train.main with --mixup / --cutmix / --label-smoothing / --fused-loss on a generated .npz of 48 images (8x8x3, 5 classes): one epoch
of three 16-sample steps on a one-block model.  Eager and --graph agree, a sample's pixels do not depend on --batch-size, the fused
plain loss is the default run's within the bound of tests/test_soft_ce_gpu.py, and the device metrics count every row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAIN = ["--model-type", "cheby", "--n-patches", "2", "--n-blocks", "1", "--d-hidden", "16", "--n-heads", "2", "--out-d", "5",
         "--batch-size", "16", "--crop-padding", "2", "--no-tuned-gemms", "--epochs", "1"]
MIX = ["--mixup", "0.8", "--cutmix", "1.0", "--label-smoothing", "0.1"]


@pytest.fixture(scope="module")
def npz_file(tmp_path_factory):
    rng = np.random.default_rng(48)
    path = str(tmp_path_factory.mktemp("npz") / "mix.npz")
    np.savez(path, x_train=rng.integers(0, 256, (48, 8, 8, 3), dtype=np.uint8), y_train=(np.arange(48) % 5).astype(np.int64))
    return path


def _main(npz_file, log_dir, *flags):
    import train
    return train.main(train.parse([*TRAIN, "--data-npz", npz_file, "--log-dir", str(log_dir), *flags]))


@pytest.fixture(scope="module")
def mixed_run(npz_file, tmp_path_factory):
    return _main(npz_file, tmp_path_factory.mktemp("eager"), *MIX)


@pytest.fixture(scope="module")
def default_run(npz_file, tmp_path_factory):
    return _main(npz_file, tmp_path_factory.mktemp("default"))


def test_eager_and_graph_give_equal_losses(npz_file, mixed_run, default_run, tmp_path):
    assert len(mixed_run["losses"]) == 3 and all(np.isfinite(mixed_run["losses"]))
    assert mixed_run["losses"] != default_run["losses"]                      # the flags did something
    graphed = _main(npz_file, tmp_path / "g", *MIX, "--graph")
    assert graphed["losses"] == mixed_run["losses"]
    assert len(mixed_run["train_metrics"]) == 1                             # the host lists took the majority labels


def _first_step(npz_file, mix):
    """The first batch of the run (seed 0, epoch 0) and the logits the freshly initialised model gives it: train.main seeds torch,
    then builds the model, and nothing in between draws from torch's generator."""
    from kanvit import data
    from model import VisionTransformer
    ds = data.GpuDataset.from_npz(npz_file, "train", DEV, pad=2, flip=True)
    batch = next(ds.batches(16, 0, 0, mix=mix))
    torch.manual_seed(0)
    model = VisionTransformer((3, 8, 8), n_patches=2, n_blocks=1, d_hidden=16, n_heads=2, out_d=5, type="cheby").to(DEV)
    with torch.no_grad():
        return batch, model(batch[0]).float()


def _ulp(v):
    return float(np.spacing(np.float32(abs(v))))


def test_first_loss_is_the_soft_loss_of_the_first_mixed_batch(npz_file, mixed_run):
    """Against the float64 restatement on the first step's logits, with torch's probability-target cross_entropy on the same logits
    as the yardstick e_t: the bound of tests/test_soft_ce_gpu.py, 2 e_t + 4 ulp."""
    import train
    from tests import _mix_ref as mr
    (x, y, y2, w), z = _first_step(npz_file, train.mix_config(train.parse([*TRAIN, "--data-npz", npz_file, *MIX])))
    assert bool((y2 != y).any()) and bool(((w > 0) & (w < 1)).any())
    want = mr.soft_ce(z.cpu().numpy(), y.cpu().numpy(), y2.cpu().numpy(), w.cpu().numpy(), 0.1)[0]
    onehot = torch.nn.functional.one_hot
    target = w[:, None] * onehot(y, 5) + (1 - w[:, None]) * onehot(y2, 5)
    e_t = abs(float(torch.nn.functional.cross_entropy(z, target, label_smoothing=0.1)) - want)
    print(f"first mixed loss: logged {mixed_run['losses'][0]!r} float64 {want!r} torch error {e_t:.2e}")
    assert abs(mixed_run["losses"][0] - want) <= 2 * e_t + 4 * _ulp(want)


def test_a_samples_pixels_do_not_depend_on_the_batch_size(npz_file):
    import train
    from kanvit import data
    mix = train.mix_config(train.parse([*TRAIN, "--data-npz", npz_file, *MIX]))
    ds = data.GpuDataset.from_npz(npz_file, "train", DEV, pad=2, flip=True)
    runs = []
    for batch in (16, 12):
        got = list(ds.batches(batch, 0, 0, mix=mix))
        x, y2, w = (torch.cat([b[k] for b in got]) for k in (0, 2, 3))
        runs.append((x, y2, w))
    assert all(torch.equal(a, b) for a, b in zip(*runs))                       # the same order (seed, epoch), the same pixels and targets
    plain = torch.cat([b[0] for b in ds.batches(16, 0, 0)])
    assert not torch.equal(plain, runs[0][0])


def test_fused_plain_loss_is_the_default_runs_first_loss(npz_file, default_run, tmp_path):
    """--fused-loss alone: the first step sees the same parameters and the same batch as the default run.  Both logged losses against
    the float64 cross-entropy of that step's logits: the default run's error is e_t, the fused one stays within 2 e_t + 4 ulp."""
    from tests import _mix_ref as mr
    fused = _main(npz_file, tmp_path / "f", "--fused-loss")
    (x, y), z = _first_step(npz_file, None)
    want = mr.soft_ce(z.cpu().numpy(), y.cpu().numpy())[0]
    e_t = abs(default_run["losses"][0] - want)
    print(f"first-step loss: fused {fused['losses'][0]!r} default {default_run['losses'][0]!r} float64 {want!r}")
    assert e_t <= 16 * _ulp(want)                                           # the logits are the run's: torch's own loss is about there
    assert abs(fused["losses"][0] - want) <= 2 * e_t + 4 * _ulp(want)
    assert len(fused["losses"]) == 3 and all(np.isfinite(fused["losses"]))


def test_device_metrics_count_every_row(npz_file, tmp_path):
    run = _main(npz_file, tmp_path / "m", *MIX, "--device-metrics", "--epochs", "2")        # a second epoch: another table, the state reset
    em = run["epoch_metrics"]
    assert em.n == 48 and int(em.confusion.sum()) == 48 and len(run["losses"]) == 6
    assert len(run["train_metrics"]) == 2 and all(0.0 <= v <= 1.0 for m in run["train_metrics"] for v in m[:3])
