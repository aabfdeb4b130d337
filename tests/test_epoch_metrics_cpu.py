"""CPU-only checks of the device epoch metrics (kanvit/metrics.py, csrc/metrics.hip, train.py --device-metrics): the host formulas
on brute-force tables against the reference's own calculate_metrics output and against scikit-learn, the new symbols and their
argument lists, the host-side refusals of both entry points, and the new command-line flag."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import _metrics_ref as mr
from tests._util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRIC_SYMBOLS = {"kanvit_metrics_update", "kanvit_metrics_auc_pairs", "kanvit_metrics_auc_pairs_workspace"}


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def _from_tables(y_true, y_pred, proba, C):
    from kanvit.metrics import metrics_from_counts
    gt, eq = mr.pair_counts(y_true, proba, C)
    return metrics_from_counts(mr.confusion(y_true, y_pred, C), gt, eq)


def test_formulas_reproduce_the_reference_on_the_golden_input():
    m = load_npz("metrics.npz")
    got = _from_tables(m["cm.y_true"], m["cm.y_pred"], m["cm.proba"].astype(np.float32), 100)
    assert np.abs(np.array(got) - m["cm.out"]).max() <= 1e-12, (got, m["cm.out"])


def _tied_case(n, C, seed, drop_class=None):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, n)
    if drop_class is not None:
        y[y == drop_class] = (drop_class + 1) % C
    z = mr.tie_logits(rng, n, C)
    p = mr.softmax64(z).astype(np.float32)
    return y, mr.first_argmax(z), p


def test_formulas_equal_scikit_learn_on_a_case_with_ties():
    from utils import calculate_metrics
    y, pred, p = _tied_case(2000, 7, 1)
    gt, eq = mr.pair_counts(y, p, 7)
    assert eq.sum() > 0                                              # the ties are there
    want = calculate_metrics(y, pred, p, num_classes=7)
    got = _from_tables(y, pred, p, 7)
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12, (got, want)


def test_a_missing_class_gives_nan_auc_and_leaves_the_rest():
    from utils import calculate_metrics
    y, pred, p = _tied_case(500, 5, 2, drop_class=3)
    want = calculate_metrics(y, pred, p, num_classes=5)
    got = _from_tables(y, pred, p, 5)
    # scikit-learn's roc_auc_score raised for an absent class for years (calculate_metrics turns that into nan); recent releases
    # warn and average over the classes that are there.  metrics_from_counts keeps the one answer: nan.
    assert math.isnan(got[3]) and (math.isnan(want[3]) or 0.0 <= want[3] <= 1.0)
    assert np.abs(np.array(got[:3]) - np.array(want[:3])).max() <= 1e-12, (got, want)


def test_the_past_cap_case_has_valid_rows_on_both_sides_and_a_first_lap_that_counts_less():
    """What tests/test_epoch_metrics_gpu.py's past-the-cap case relies on: valid rows before and behind sample 2048 * 256, and pair
    counts over the first lap's rows alone that differ from the full ones in every class, so a histogram or a scatter that stops after
    its first lap cannot give the full counts.  The dropped rows hold -1.0, below every valid probability: one of them counted as a
    negative would add the class's positives to its gt."""
    y, p = mr.past_cap_case()
    lap, C = mr.HIST_LAP, 3
    assert lap == 2048 * 256 and len(y) == lap + 700 and p.shape == (len(y), C) and p.dtype == np.float32
    ok = y >= 0
    assert ok[:lap].sum() == 900 and ok[lap:].all() and set(y[ok].tolist()) == set(range(C)) and (y[~ok] == -1).all()
    assert (p[~ok] == -1.0).all() and (p[ok] > 0.0).all()
    gt, eq = mr.pair_counts(y, p, C)
    gt1, eq1 = mr.pair_counts(y[:lap], p[:lap], C)
    assert (gt != gt1).all() and (eq != eq1).all() and (eq > 0).all() and (gt1 > 0).all()


def test_from_counts_conventions_and_argument_checks():
    from kanvit.metrics import metrics_from_counts
    # class 2 is never true and never predicted: F1 term 0 with weight 0, no recall term, AUC nan
    cm = np.array([[3, 1, 0], [2, 4, 0], [0, 0, 0]])
    acc, bal, f1, auc = metrics_from_counts(cm, np.zeros(3, np.int64), np.zeros(3, np.int64))
    assert acc == 0.7 and bal == (3 / 4 + 4 / 6) / 2 and math.isnan(auc)
    assert abs(f1 - (4 * (6 / 9) + 6 * (8 / 11)) / 10) < 1e-15
    # two samples, two classes, the positive above the negative for both classes: AUC 1
    assert metrics_from_counts(np.eye(2, dtype=np.int64), np.array([1, 1]), np.array([0, 0])) == (1.0, 1.0, 1.0, 1.0)
    assert metrics_from_counts(np.eye(2, dtype=np.int64), np.array([0, 0]), np.array([1, 1]))[3] == 0.5
    with pytest.raises(ValueError):
        metrics_from_counts(np.eye(2), np.zeros(2, np.int64), np.zeros(2, np.int64))              # float tables are refused
    with pytest.raises(ValueError):
        metrics_from_counts(np.eye(2, dtype=np.int64), np.zeros(3, np.int64), np.zeros(2, np.int64))


def test_symbols_are_declared_and_bound_with_the_documented_arguments(lib):
    from kanvit import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kanvit.h")).read(), flags=re.S)
    assert {n for n in re.findall(r"\b(kanvit_[a-z0-9_]+)\s*\(", src) if "metrics" in n} == METRIC_SYMBOLS
    assert {n for n in _lib.SYMBOLS if "metrics" in n} == METRIC_SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in METRIC_SYMBOLS:
        assert hasattr(raw, name), name
    P, I64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _lib.SYMBOLS["kanvit_metrics_update"] == (I, [P, I, I64, P, I64, I, I64, I64, P, P, P, P, P])
    assert _lib.SYMBOLS["kanvit_metrics_auc_pairs_workspace"] == (ctypes.c_size_t, [I64, I])
    assert _lib.SYMBOLS["kanvit_metrics_auc_pairs"] == (I, [P, P, I64, I, I64, P, P, ctypes.c_size_t, P])
    assert lib.kanvit_abi_version() == 7


def test_update_validates_on_the_host(lib):
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(logits=p, bf16=0, ld=4, labels=p, B=2, C=4, n0=0, cap=8, probs=p, lo=p, po=p, cm=p):
        return lib.kanvit_metrics_update(logits, bf16, ld, labels, B, C, n0, cap, probs, lo, po, cm, None)

    for kw, word in ((dict(C=1), b"C=1"), (dict(B=0), b"B=0"), (dict(n0=7), b"n0=7"), (dict(B=9, cap=8), b"cap=8"), (dict(ld=3), b"ld=3"),
                     (dict(n0=-1), b"n0=-1"), (dict(bf16=2), b"logits_bf16=2"),
                     (dict(logits=None), b"null"), (dict(labels=None), b"null"), (dict(probs=None), b"null"), (dict(lo=None), b"null"),
                     (dict(po=None), b"null"), (dict(cm=None), b"null")):
        assert call(**kw) == -22, kw
        msg = lib.kanvit_last_error()
        assert b"kanvit_metrics_update" in msg and word in msg, (kw, msg)


def test_auc_pairs_validates_on_the_host(lib):
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.kanvit_metrics_auc_pairs_workspace
    assert need(50000, 100) == (3 * 100 + 1) * 4 + 12 + 50000 * 4            # three int32 tables + 1, rounded up to 16 bytes, one float per sample
    assert need(1, 2) == 32 + 4
    assert need(0, 2) == 0 and need(10, 1) == 0 and need((1 << 28) + 1, 2) == 0

    def call(probs=p, labels=p, n=4, C=2, cap=8, counts=p, ws=p, nbytes=1 << 20):
        return lib.kanvit_metrics_auc_pairs(probs, labels, n, C, cap, counts, ws, nbytes, None)

    for kw, word in ((dict(C=1), b"C=1"), (dict(n=0), b"n=0"), (dict(n=9), b"cap=8"), (dict(n=(1 << 28) + 1, cap=1 << 29), b"2^28"),
                     (dict(nbytes=8), b"workspace"), (dict(probs=None), b"null"), (dict(labels=None), b"null"),
                     (dict(counts=None), b"null"), (dict(ws=None), b"null")):
        assert call(**kw) == -22, kw
        msg = lib.kanvit_last_error()
        assert b"kanvit_metrics_auc_pairs" in msg and word in msg, (kw, msg)


def test_wrappers_refuse_cpu_tensors():
    from kanvit import KanvitError, ops
    from kanvit.metrics import EpochMetrics
    z, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    probs_t, li, cm = torch.zeros(3, 8), torch.zeros(8, dtype=torch.int32), torch.zeros(3, 3, dtype=torch.int64)
    with pytest.raises(KanvitError):
        ops.metrics_update(z, y, 0, probs_t, li, li.clone(), cm)
    with pytest.raises(KanvitError):
        ops.metrics_auc_pairs(probs_t, li, 4)
    with pytest.raises(KanvitError):
        EpochMetrics(3, 8, "cpu")


def test_device_metrics_flag_defaults_to_off():
    import train
    assert train.parse([]).device_metrics is False
    assert train.parse(["--device-metrics"]).device_metrics is True
