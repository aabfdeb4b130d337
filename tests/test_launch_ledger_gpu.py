"""What the kernel timer -- and through it bench.py's roofline leg -- sees of a fixed set of small runs must be what the recorded
ledger says (tests/golden/launch_ledger.json, written by tools/launch_ledger.py on the commit before the launches of kanvit.ops
and kanvit.dense moved into ops._launch): for every case the same timer tags in the same order of first appearance, each with
the same number of launches and the same flops and bytes, all integers.  No time is compared.

The cases (tools/launch_ledger.py): one forward + backward of the (1, 28, 28) / 7 patches / 2 blocks / d = 64 / 2 heads model at
batch 8 for every model type, in fp32 and under bf16 autocast (patch embedding, a normal block, the fused small feed-forward,
FastKAN's fused LayerNorm, SineKAN's frequency pass); the same for cheby with 8 heads of d_head = 8 (the tiny per-head kernels)
and at d = 128, where the last block runs its class-token tail; regularization_loss + backward, update_grid, extend_grid and
attention_map of an efficient-KAN MSA; ops.attention forward + backward at (1, 2, 300, 64) for the general kernels."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "launch_ledger.json")) as _f:
    GOLDEN = json.load(_f)


def _tool():
    spec = importlib.util.spec_from_file_location("launch_ledger", os.path.join(ROOT, "tools", "launch_ledger.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_covers_the_cases():
    """No GPU: the fixture and the tool name the same cases in the same order, and the fixture holds integers only."""
    assert list(GOLDEN) == list(_tool().CASES)
    for rows in GOLDEN.values():
        assert rows and all(isinstance(t, str) and all(type(v) is int for v in rest) and len(rest) == 3 for t, *rest in rows)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(GOLDEN))
def test_launch_ledger(case):
    got = _tool().run_case(case)
    assert got == GOLDEN[case], f"{case}: the timer saw\n{got}\nrecorded\n{GOLDEN[case]}"
