"""Without a GPU: the host restatements that the training-loop kernels' lap tests compare against bit for bit, and the properties of
the cases that make a dropped second lap visible (tests/test_soft_ce_gpu.py, tests/test_optim_gpu.py)."""
import numpy as np

from tests import _mix_ref as mr
from tests import _optim_ref as R


def test_mean_rows_restatement_is_exact_on_ones_and_within_its_bound_of_float64():
    """257 ones: every partial sum is a small integer, the mean is exactly 1.  Positive rows: n - 1 float32 additions and one division,
    each within 2^-24 relative, so the mean is within B * 2^-24 relative of the float64 mean of the same float32 rows."""
    one = mr.mean_rows_f32(np.ones(257, np.float32))
    assert one.dtype == np.float32 and one == np.float32(1.0)
    assert mr.mean_rows_f32(np.float32([3.5])) == np.float32(3.5)
    rng = np.random.default_rng(0)
    for B in (1, 2, 130, 256, 257, 1000, 5000):
        rows = rng.uniform(0.01, 12.0, B).astype(np.float32)
        got, want = float(mr.mean_rows_f32(rows)), float(rows.astype(np.float64).mean())
        assert abs(got - want) <= B * 2.0 ** -24 * want, (B, got, want)


def test_mean_rows_restatement_reaches_past_the_first_lap():
    rows = np.random.default_rng(1).uniform(0.5, 3.0, 257).astype(np.float32)
    first_lap = mr.mean_rows_f32(rows[:256]) * np.float32(256) / np.float32(257)         # the sum of the first 256 rows over B
    assert mr.mean_rows_f32(rows) != first_lap
    moved = rows.copy()
    moved[256] += np.float32(1.0)                                    # the one row of the second lap is in the sum
    assert mr.mean_rows_f32(moved) > mr.mean_rows_f32(rows)
    # the order is the kernel's: thread 0 adds rows 0 and 256 BEFORE the tree.  2^24 + 1 is not a float32: (2^24 + 1) + 1 = 2^24 + 1
    # rounds to 2^24 twice, whereas 2^24 + (1 + 1) is exact
    order = np.zeros(512, np.float32)                                # B = 512: the division is exact
    order[0], order[256], order[128] = 2.0 ** 24, 1.0, 1.0
    assert mr.mean_rows_f32(order) * np.float32(512) == np.float32(2.0 ** 24)
    order[256], order[128], order[64], order[192] = 0.0, 0.0, 1.0, 1.0          # the same three numbers, the two ones meeting in the tree first
    assert mr.mean_rows_f32(order) * np.float32(512) == np.float32(2.0 ** 24 + 2.0)


def test_the_optimizer_lap_case_is_what_it_claims():
    """R.LAP_NUMELS: more partials than the begin kernel's 256 threads, the large tensor behind 81 tiny ones, and on both steps a norm
    and a coefficient that the first 256 partials alone do not give."""
    numels = R.LAP_NUMELS
    assert len(numels) == 83 and numels[81] == 260 * R.CHUNK + 5 and numels[82] == 9 and 81 % 4 == 1
    for step in range(R.LAP_STEPS):
        parts = np.concatenate([R.sumsq_partials(g) for g in R.case_grads(numels, step, none=())])
        assert len(parts) == 81 + 261 + 1 > R.THREADS
        full = R.norm_and_coef(R.total_sumsq(parts), 0.5)
        lap0 = R.norm_and_coef(R.total_sumsq(parts[:R.THREADS]), 0.5)
        assert full[0] != lap0[0] and full[1] != lap0[1] and full[1] < 1.0, (step, full, lap0)
        assert full == R.norm_and_coef(R.grads_sumsq(R.case_grads(numels, step, none=())), 0.5)
