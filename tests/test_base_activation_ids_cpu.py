"""The four cases of tests/test_base_activation_cpu.py::test_recognised / test_refused whose test ids there are `repr(fn)` of a Python
function -- `<function relu at 0x...>` -- and so carry the function's memory address, which differs from process to process (address
space layout randomisation): the same checks under ids that name the callable instead."""
import pytest
import torch.nn.functional as F

from kanvit import _lib, ops

RECOGNISED = {"F.silu": (F.silu, 0), "F.relu": (F.relu, 3), "F.tanh": (F.tanh, 4)}


@pytest.mark.parametrize("name", sorted(RECOGNISED))
def test_recognised(name):
    fn, code = RECOGNISED[name]
    assert ops.base_activation_code(fn) == code
    assert _lib.BASE_NAMES[code] in ("silu", "gelu", "gelu-tanh", "relu", "tanh", "identity")


def test_refused_lambda():
    fn = lambda x: x * 2          # noqa: E731  (the callable under test)
    assert ops.base_activation_code(fn) is None
    with pytest.raises(NotImplementedError, match="supported"):
        ops.base_act_of(fn)
