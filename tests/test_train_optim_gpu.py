"""train.main with --optimizer kanvit-adamw and every recipe flag on a generated .npz of 48 images (8x8x3, 5 classes): one epoch of three
16-sample steps on a one-block model, as tests/test_train_mix_gpu.py runs it.  Eager and --graph agree, the recipe changes the
trajectory from the second step on, --ema-decay evaluates on the averaged weights, and the last gradient norm is reported."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TRAIN = ["--model-type", "cheby", "--n-patches", "2", "--n-blocks", "1", "--d-hidden", "16", "--n-heads", "2", "--out-d", "5",
         "--batch-size", "16", "--crop-padding", "2", "--no-tuned-gemms", "--epochs", "1"]
RECIPE = ["--optimizer", "kanvit-adamw", "--weight-decay", "0.05", "--clip-grad-norm", "0.5", "--warmup-steps", "2", "--lr-schedule", "cosine",
          "--min-lr", "1e-5", "--ema-decay", "0.9"]


@pytest.fixture(scope="module")
def npz_file(tmp_path_factory):
    rng = np.random.default_rng(48)
    path = str(tmp_path_factory.mktemp("npz") / "optim.npz")
    np.savez(path, x_train=rng.integers(0, 256, (48, 8, 8, 3), dtype=np.uint8), y_train=(np.arange(48) % 5).astype(np.int64),
             x_test=rng.integers(0, 256, (16, 8, 8, 3), dtype=np.uint8), y_test=(np.arange(16) % 5).astype(np.int64))
    return path


def _main(npz_file, log_dir, *flags):
    import train
    return train.main(train.parse([*TRAIN, "--data-npz", npz_file, "--log-dir", str(log_dir), *flags]))


@pytest.fixture(scope="module")
def recipe_run(npz_file, tmp_path_factory):
    return _main(npz_file, tmp_path_factory.mktemp("eager"), *RECIPE)


def test_eager_and_graph_give_equal_losses(npz_file, recipe_run, tmp_path):
    assert len(recipe_run["losses"]) == 3 and all(np.isfinite(recipe_run["losses"]))
    graphed = _main(npz_file, tmp_path / "g", *RECIPE, "--graph")
    assert graphed["losses"] == recipe_run["losses"]
    assert graphed["grad_norm"] == recipe_run["grad_norm"]


def test_the_recipe_changes_the_trajectory_from_the_second_step(npz_file, recipe_run, tmp_path):
    default = _main(npz_file, tmp_path / "d")
    assert "grad_norm" not in default and "ema_eval" not in default          # the default run's history gains no key
    assert default["losses"][0] == recipe_run["losses"][0]                   # the same weights see the same first batch
    assert all(a != b for a, b in zip(default["losses"][1:], recipe_run["losses"][1:]))


def test_ema_evaluation_and_gradient_norm_are_reported(recipe_run):
    from kanvit.optim import KanvitAdamW
    assert recipe_run["ema_eval"] is True
    acc, bal, f1, auc = recipe_run["test_metrics"]
    assert 0.0 <= acc <= 1.0 and 0.0 <= bal <= 1.0 and 0.0 <= f1 <= 1.0
    assert np.isfinite(recipe_run["grad_norm"]) and recipe_run["grad_norm"] > 0.0
    opt = recipe_run["optimizer"]
    assert isinstance(opt, KanvitAdamW) and int(opt.flat["step"]) == 3 and opt.table.shape == (3, 4)
    assert 0.0 < float(opt.clip_coef) <= 1.0


def test_composes_with_bf16_and_the_regulariser(npz_file, tmp_path):
    run = _main(npz_file, tmp_path / "b", *RECIPE, "--amp", "bf16", "--reg-lambda", "0.01", "--mixup", "0.8", "--label-smoothing", "0.1")
    assert len(run["losses"]) == 3 and all(np.isfinite(run["losses"])) and np.isfinite(run["grad_norm"])
