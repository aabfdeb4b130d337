"""The device epoch metrics on the GPU (csrc/metrics.hip: kanvit_metrics_update, kanvit_metrics_auc_pairs; kanvit/metrics.py;
train.py --device-metrics) against the numpy brute force of tests/_metrics_ref.py, scikit-learn and the default metrics path."""
import re

import numpy as np
import pytest
import torch

from tests import _metrics_ref as mr
from tests._util import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _state(C, cap):
    return (torch.full((C, cap), -7.0, device=DEV), torch.full((cap,), -9, device=DEV, dtype=torch.int32),
            torch.full((cap,), -9, device=DEV, dtype=torch.int32), torch.zeros((C, C), device=DEV, dtype=torch.int64))


def _logits(B, C, seed, dtype, quantised):
    rng = np.random.default_rng(seed)
    z = mr.tie_logits(rng, B, C) if quantised else rng.uniform(-10, 10, (B, C)).astype(np.float32)
    t = torch.from_numpy(z).to(dtype)                    # bf16: round first; the kernel widens what it is given exactly
    return t, t.float().numpy()


# (B, C) as the kernel meets them: one row, fewer rows than a tile, several work-groups (128 and 70 rows: the second with a short last
# tile), C below / at / above one 64-class chunk and far above it; n0 and cap cover a start inside a tile and an exact fit
UPDATE_CASES = [(1, 2, 0, 1), (5, 3, 3, 11), (4, 10, 0, 4), (128, 100, 3, 131), (70, 65, 0, 96), (3, 1000, 3, 6)]


@pytest.mark.parametrize("B,C,n0,cap", UPDATE_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("quantised,padded", [(False, False), (True, False), (False, True)])
def test_update_kernel_against_numpy(B, C, n0, cap, dtype, quantised, padded):
    """Labels, predictions (first index among equal maxima) and the confusion matrix exactly; probabilities within relative
    (C + 32) * 2^-23 of the float64 softmax for logits in [-10, 10].  With u = 2^-24: the fp32 sum of C positive terms gives (C - 1) u
    in any order, exp 2 ulp = 4 u, the rounding of the argument |z - max| u <= 20 u; that total, (C + 23) u, doubled (numerator and
    denominator, the division) stays below the bound.  Slots outside n0 .. n0 + B - 1 keep what they held."""
    from kanvit import ops
    t, z = _logits(B, C, 100 * B + C, dtype, quantised)
    if padded:
        wide = torch.full((B, C + 5), float("nan"), dtype=dtype)
        wide[:, :C] = t
        zt = wide.to(DEV)[:, :C]
        assert zt.stride(0) == C + 5
    else:
        zt = t.to(DEV)
    y = np.random.default_rng(B).integers(0, C, B)
    probs_t, lab, pred, cm = _state(C, cap)
    ops.metrics_update(zt, torch.from_numpy(y).to(DEV), n0, probs_t, lab, pred, cm)
    want_pred = mr.first_argmax(z)
    if quantised:
        assert (np.sort(z, axis=1)[:, -1] == np.sort(z, axis=1)[:, -2]).any()        # some row does have a tied maximum
    sl = slice(n0, n0 + B)
    assert np.array_equal(lab.cpu().numpy()[sl], y) and np.array_equal(pred.cpu().numpy()[sl], want_pred)
    assert np.array_equal(cm.cpu().numpy(), mr.confusion(y, want_pred, C))
    got = probs_t.cpu().numpy().astype(np.float64)
    want = mr.softmax64(z)
    rel = np.abs(got[:, sl].T - want) / want
    print(f"B={B} C={C} {dtype} max rel err {rel.max():.3e} bound {(C + 32) * 2.0 ** -23:.3e}")
    assert rel.max() <= (C + 32) * 2.0 ** -23
    keep = np.ones(cap, dtype=bool)
    keep[sl] = False
    assert (got[:, keep] == -7.0).all() and (lab.cpu().numpy()[keep] == -9).all() and (pred.cpu().numpy()[keep] == -9).all()


def test_update_drops_rows_with_labels_outside_the_classes():
    """Rows with label C and label -1: stored label -1, no confusion count, and the pair counts as if the rows were absent."""
    from kanvit import ops
    B, C = 40, 5
    t, z = _logits(B, C, 7, torch.float32, True)
    y = np.random.default_rng(3).integers(0, C, B)
    y[[0, 17, 33]] = C
    y[[5, 39]] = -1
    probs_t, lab, pred, cm = _state(C, B)
    ops.metrics_update(t.to(DEV), torch.from_numpy(y).to(DEV), 0, probs_t, lab, pred, cm)
    ok = (y >= 0) & (y < C)
    assert np.array_equal(lab.cpu().numpy(), np.where(ok, y, -1))
    assert np.array_equal(pred.cpu().numpy(), mr.first_argmax(z))
    assert np.array_equal(cm.cpu().numpy(), mr.confusion(y[ok], mr.first_argmax(z)[ok], C))
    counts = ops.metrics_auc_pairs(probs_t, lab, B).cpu().numpy()
    p = probs_t.cpu().numpy().T
    gt, eq = mr.pair_counts(y[ok], p[ok], C)
    assert np.array_equal(counts[:, 0], gt) and np.array_equal(counts[:, 1], eq)


def _pairs(y, p, C, cap=None):
    """Run the pair kernel on given float32 probabilities [n, C] and labels; the state is laid out as the update kernel leaves it."""
    from kanvit import ops
    n = len(y)
    cap = cap or n
    probs_t = torch.full((C, cap), float("nan"), device=DEV)
    probs_t[:, :n] = torch.from_numpy(np.ascontiguousarray(p.T))
    lab = torch.full((cap,), 0, device=DEV, dtype=torch.int32)
    lab[:n] = torch.from_numpy(np.asarray(y).astype(np.int32))
    counts = torch.full((C, 2), 12345, device=DEV, dtype=torch.int64)              # the call zeroes them itself
    out = ops.metrics_auc_pairs(probs_t, lab, n, counts=counts)
    assert out is counts
    return counts.cpu().numpy()


def _tied_probs(n, C, seed):
    z = mr.tie_logits(np.random.default_rng(seed), n, C)
    return mr.softmax64(z).astype(np.float32)


def test_pair_counts_on_the_golden_probabilities():
    from kanvit.metrics import metrics_from_counts
    m = load_npz("metrics.npz")
    y, p = m["cm.y_true"], m["cm.proba"].astype(np.float32)
    counts = _pairs(y, p, 100, cap=307)
    gt, eq = mr.pair_counts(y, p, 100)
    assert np.array_equal(counts[:, 0], gt) and np.array_equal(counts[:, 1], eq)
    got = metrics_from_counts(mr.confusion(y, m["cm.y_pred"], 100), counts[:, 0], counts[:, 1])
    assert np.abs(np.array(got) - m["cm.out"]).max() <= 1e-12, (got, m["cm.out"])


@pytest.mark.parametrize("case", ["n1", "n2c2", "n1030c3", "n2500c2", "empty_class"])
def test_pair_counts_equal_the_brute_force_exactly(case):
    """One sample; the smallest pair; more than one tile of 1024 samples with every class on both sides; 2100 positives of one class
    (three LDS chunks of 1024, n no multiple of any tile) with ties; a class without samples (counts 0)."""
    rng = np.random.default_rng(11)
    if case == "n1":
        y, p, C = np.array([1]), np.array([[0.25, 0.75]], np.float32), 2
    elif case == "n2c2":
        y, p, C = np.array([0, 1]), np.array([[0.75, 0.25], [0.75, 0.25]], np.float32), 2
    elif case == "n1030c3":
        y, p, C = rng.integers(0, 3, 1030), _tied_probs(1030, 3, 5), 3
    elif case == "n2500c2":
        y, p, C = rng.permutation(np.array([1] * 2100 + [0] * 400)), _tied_probs(2500, 2, 6), 2
    else:
        y, p, C = rng.integers(0, 3, 333) * 2, _tied_probs(333, 6, 8), 6             # classes 1, 3, 5 never occur
    counts = _pairs(y, p, C)
    gt, eq = mr.pair_counts(y, p, C)
    assert np.array_equal(counts[:, 0], gt) and np.array_equal(counts[:, 1], eq), (counts, gt, eq)
    if case == "n1":
        assert not counts.any()
    if case == "n2c2":
        assert counts.tolist() == [[0, 1], [0, 1]]
    if case in ("n1030c3", "n2500c2"):
        assert eq.sum() > 0 and gt.sum() > 0
    if case == "empty_class":
        assert not counts[1::2].any() and counts[::2, 0].all()


SCAN_THREADS = 256                  # metrics_scan_kernel: one work-group, ceil(C / 256) consecutive classes per thread


@pytest.mark.parametrize("case", ["c257", "c300_every_third_empty"])
def test_pair_counts_with_more_than_one_class_per_scan_thread(case):
    """C = 257: two classes per thread, thread 128 owns class 256 alone and threads 129..255 own a range that starts past C.
    C = 300: the same with every third class empty, so offsets repeat inside a thread's range."""
    rng = np.random.default_rng(12)
    if case == "c257":
        C, n = 257, 1500
        y = rng.integers(0, C, n)
        y[[3, 700, 1499]] = 256
    else:
        C, n = 300, 2000
        k = rng.integers(0, 200, n)
        y = k + k // 2                                               # 0, 1, 3, 4, 6, 7, ...: classes 2, 5, 8, ... never occur
    per = (C + SCAN_THREADS - 1) // SCAN_THREADS
    assert per >= 2 and (C - 1) // per < SCAN_THREADS - 1              # some thread's range starts past C
    p = _tied_probs(n, C, 13)
    counts = _pairs(y, p, C)
    gt, eq = mr.pair_counts(y, p, C)
    assert np.array_equal(counts[:, 0], gt) and np.array_equal(counts[:, 1], eq)
    assert eq.sum() > 0 and gt.sum() > 0
    if case == "c257":
        assert (y == 256).sum() >= 3 and counts[256, 0] > 0 and (C - 1) % per == 0 and C - 1 + per > C       # class 256: alone in its range
    else:
        assert not counts[2::3].any() and counts[0::3, 0].all() and counts[1::3, 0].all()


def test_epoch_metrics_at_a_thousand_classes_equal_the_brute_force_tables():
    """C = 1000 (four classes per scan thread), 3000 rows fed in batches of 128 as bfloat16: the update kernel and the pair kernel
    together at an ImageNet-sized head.  The tables are exact integers; compute() is metrics_from_counts of the brute-force tables."""
    from kanvit.metrics import EpochMetrics, metrics_from_counts
    C, n, B = 1000, 3000, 128
    assert (C + SCAN_THREADS - 1) // SCAN_THREADS >= 2
    rng = np.random.default_rng(14)
    t, z = _logits(n, C, 15, torch.bfloat16, True)
    y = rng.permutation(np.arange(n) % C)                            # every class has positives: the AUC is a number
    zt, yt = t.to(DEV), torch.from_numpy(y).to(DEV)
    em = EpochMetrics(C, n, DEV)
    for at in range(0, n, B):
        em.update(zt[at:at + B], yt[at:at + B])
    got = em.compute()
    pred, p = em.preds().cpu().numpy(), em.probs().cpu().numpy()
    assert np.array_equal(em.labels().cpu().numpy(), y) and np.array_equal(pred, mr.first_argmax(z))
    cm = mr.confusion(y, pred, C)
    gt, eq = mr.pair_counts(y, p, C)
    counts = em.counts.cpu().numpy()
    assert np.array_equal(em.confusion.cpu().numpy(), cm)
    assert np.array_equal(counts[:, 0], gt) and np.array_equal(counts[:, 1], eq) and eq.sum() > 0 and gt.all()
    assert got == metrics_from_counts(cm, gt, eq) and all(np.isfinite(got))


def test_pair_counts_past_the_histogram_and_scatter_cap():
    """n = 2048 * 256 + 700 samples, more than one lap of the histogram and the scatter, of which about 1600 are valid: 900 scattered
    over the first lap and the 700 of the second (tests/_metrics_ref.past_cap_case; tests/test_epoch_metrics_cpu.py checks that the
    first lap alone counts differently in every class)."""
    y, p = mr.past_cap_case()
    n, C = len(y), 3
    assert n > mr.HIST_LAP == 2048 * 256 and (y[mr.HIST_LAP:] >= 0).all() and (y[:mr.HIST_LAP] >= 0).any()
    counts = _pairs(y, p, C)
    gt, eq = mr.pair_counts(y, p, C)
    assert np.array_equal(counts[:, 0], gt) and np.array_equal(counts[:, 1], eq), (counts, gt, eq)
    assert (eq > 0).all() and (gt > 0).all()


@pytest.fixture(scope="module")
def fed():
    """161 rows, 9 classes, with ties, fed to EpochMetrics in one batch and in batches of 7, 1, 120 and 33; computed once."""
    from kanvit.metrics import EpochMetrics
    rng = np.random.default_rng(21)
    z = torch.from_numpy(mr.tie_logits(rng, 161, 9)).to(DEV)
    y = torch.from_numpy(rng.integers(0, 9, 161)).to(DEV)
    runs = []
    for sizes in ((161,), (7, 1, 120, 33), (161,)):
        em = EpochMetrics(9, 161, DEV)
        at = 0
        for b in sizes:
            em.update(z[at:at + b], y[at:at + b])
            at += b
        out = em.compute()
        runs.append((em, out, em.probs().cpu().clone(), em.labels().cpu().clone(), em.preds().cpu().clone(), em.confusion.cpu().clone(),
                     em.counts.cpu().clone()))
    return z, y, runs


def test_epoch_metrics_do_not_depend_on_the_batch_sizes_or_the_run(fed):
    _, _, runs = fed
    for other in runs[1:]:
        assert other[1] == runs[0][1]                                # the four floats, bitwise
        for a, b in zip(other[2:], runs[0][2:]):
            assert torch.equal(a, b)
    assert runs[0][2].shape == (161, 9)


def test_epoch_metrics_equal_scikit_learn(fed):
    from utils import calculate_metrics
    _, y, runs = fed
    em, out = runs[1][0], runs[1][1]
    want = calculate_metrics(em.labels().long().cpu().numpy(), em.preds().cpu().numpy(), em.probs().cpu().numpy(), num_classes=9)      # one_hot wants int64
    assert np.abs(np.array(out) - np.array(want)).max() <= 1e-12, (out, want)
    assert np.array_equal(em.labels().cpu().numpy(), y.cpu().numpy())


def test_epoch_metrics_reset_clears_and_a_full_state_refuses(fed):
    from kanvit import KanvitError
    from kanvit.metrics import EpochMetrics
    from utils import calculate_metrics
    z, y, _ = fed
    em = EpochMetrics(9, 60, DEV)
    em.update(z[100:160], y[100:160])
    with pytest.raises(KanvitError, match="capacity"):
        em.update(z[:1], y[:1])                                      # full: refused on the host, nothing launched
    assert em.n == 60 and int(em.confusion.sum()) == 60
    em.reset()
    assert em.n == 0 and not em.confusion.any() and not em.counts.any() and em.probs().shape == (0, 9) and em.labels().numel() == 0
    with pytest.raises(KanvitError):
        em.compute()
    em.update(z[:50], y[:50])
    first = em.compute()
    want = calculate_metrics(y[:50].cpu().numpy(), em.preds().cpu().numpy(), em.probs().cpu().numpy(), num_classes=9)
    assert np.abs(np.array(first) - np.array(want)).max() <= 1e-12
    assert em.compute() == first                                     # computing twice counts nothing twice


TRAIN_GEOM = ["--synthetic", "--in-chans", "1", "--image-size", "28", "--n-patches", "7", "--n-blocks", "1", "--n-heads", "2",
              "--d-hidden", "64", "--out-d", "3", "--batch-size", "16", "--model-type", "cheby", "--epochs", "1", "--no-tuned-gemms"]


@pytest.mark.parametrize("graph", [False, True])
def test_train_main_device_metrics_equal_the_default_path(graph, tmp_path):
    """Three fixed batches of 16, three classes, one block: the same losses, and the four metrics of the epoch equal to the lists +
    scikit-learn path -- the three confusion-matrix numbers within 1e-12, the AUC within 1e-9 (the two softmaxes differ in the last
    place; a flipped near-tie would show as a multiple of 0.5 / (P (N - P)) >= 4e-4)."""
    import train
    from model import VisionTransformer
    torch.manual_seed(5)
    init = {k: v.clone() for k, v in VisionTransformer((1, 28, 28), 7, 1, 64, 2, 3, type="cheby").state_dict().items()}
    batches = [(torch.rand(16, 1, 28, 28), torch.randint(0, 3, (16,))) for _ in range(3)]
    hists = []
    for flag in ((), ("--device-metrics",)):
        args = train.parse([*TRAIN_GEOM, "--log-dir", str(tmp_path / f"logs{len(hists)}"), *flag, *(("--graph",) if graph else ())])
        hists.append(train.main(args, batches=batches, init_state=init))
    host, dev = hists
    assert host["losses"] == dev["losses"] and len(dev["losses"]) == 3
    assert len(host["train_metrics"]) == 1 and len(dev["train_metrics"]) == 1
    assert "epoch_metrics" in dev and "epoch_metrics" not in host and dev["epoch_metrics"].n == 48
    a, b = np.array(host["train_metrics"][0]), np.array(dev["train_metrics"][0])
    print("host", a, "device", b)
    assert np.isfinite(a).all()
    assert np.abs(a[:3] - b[:3]).max() <= 1e-12 and abs(a[3] - b[3]) <= 1e-9, (a, b)
    for h in hists:
        text = open(h["metrics_file"]).read()
        assert re.fullmatch(r"Epoch: 1, Phase: Train\n  Loss: \d+\.\d{4}\n  Accuracy: \d\.\d{4}\n  Balanced Accuracy: \d\.\d{4}\n"
                            r"  F1 Score: \d\.\d{4}\n  ROC AUC: (nan|\d\.\d{4})\n\n", text), text


def test_train_main_device_metrics_cover_the_test_pass(tmp_path):
    """--data-npz with a test split (24 images, 3 classes, batches of 16 and 8): the test block's four numbers with --device-metrics
    equal the default path's, as the epoch's do; bf16 autocast feeds the update kernel bfloat16 logits."""
    import train
    rng = np.random.default_rng(4)
    path = str(tmp_path / "tiny.npz")
    np.savez(path, x_train=rng.integers(0, 256, (40, 8, 8, 3), dtype=np.uint8), y_train=(np.arange(40) % 3).astype(np.uint8),
             x_test=rng.integers(0, 256, (24, 8, 8, 3), dtype=np.uint8), y_test=(np.arange(24) % 3).astype(np.uint8))
    geom = ["--model-type", "cheby", "--n-patches", "2", "--n-blocks", "1", "--n-heads", "2", "--d-hidden", "64", "--out-d", "3",
            "--batch-size", "16", "--crop-padding", "2", "--no-tuned-gemms", "--epochs", "1", "--data-npz", path]
    for amp in ("off", "bf16"):
        hists = [train.main(train.parse([*geom, "--amp", amp, *flag, "--log-dir", str(tmp_path / f"{amp}{len(flag)}")]))
                 for flag in ((), ("--device-metrics",))]
        assert hists[0]["losses"] == hists[1]["losses"]
        for key in ("test_metrics", "train_metrics"):
            a, b = np.array(hists[0][key]).reshape(-1), np.array(hists[1][key]).reshape(-1)
            print(amp, key, a, b)
            assert np.isfinite(a).all() and np.abs(a[:3] - b[:3]).max() <= 1e-12 and abs(a[3] - b[3]) <= 1e-9, (amp, key, a, b)
        text = open(hists[1]["metrics_file"]).read()
        assert re.search(r"Phase: Test\n  Loss: \d+\.\d{4}\n  Accuracy: \d\.\d{4}\n  Balanced Accuracy: \d\.\d{4}\n  F1 Score: \d\.\d{4}\n"
                         r"  ROC AUC: \d\.\d{4}\n\n", text), text
