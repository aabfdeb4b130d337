"""The operand refusals of the training-loop ops (kanvit/ops.py from augment_u8 on: ops._require_tensor and the two helpers built on it),
on the GPU: starting from a valid call at the smallest shapes, each tensor operand in turn is replaced by a CPU tensor, one of the wrong
dtype, a non-contiguous view and one of the wrong shape, and the KanvitError must name the function, the operand and the fault.  The
valid call itself runs once per function.  A refused call launches nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, H, W, B, OUT, CLASSES, CAP, NUMEL, STATE = 3, 4, 4, 2, 8, 3, 4, 5, 8

# function -> (the name its messages carry, its tensor operands).  "x[0]" is the first tensor of the list x.
OPERANDS = {
    "augment_u8": ("augment_u8", ["images", "labels", "idx", "lut", "out"]),
    "mix_u8": ("mix_u8", ["images", "labels", "idx", "lut", "partner", "weight", "box", "out"]),
    "resample_u8": ("resample_u8", ["images", "labels", "idx", "lut", "crop", "partner", "weight", "box", "out"]),
    "soft_ce": ("soft_cross_entropy", ["logits", "y", "y2", "w"]),           # the op behind soft_cross_entropy reports under that name
    "metrics_update": ("metrics_update", ["logits", "labels", "probs_t", "labels_out", "preds_out", "confusion"]),
    "metrics_auc_pairs": ("metrics_auc_pairs", ["probs_t", "labels", "counts"]),
    "optim_grad_sumsq": ("optim_grad_sumsq", ["grads[0]", "partials"]),
    "optim_begin": ("optim_begin", ["partials", "step", "norm_coef"]),
    "optim_adamw": ("optim_adamw", ["params[0]", "grads[0]", "exp_avg", "exp_avg_sq", "ema", "table", "step", "norm_coef"]),
}
FAULTS = {"cpu": "no CPU fallback", "dtype": "dtype", "noncontiguous": "contiguous", "shape": "shape"}


def _left_out(fn, name, fault):
    """The cells of the table that do not exist."""
    if fault == "noncontiguous" and name == "step":
        return True         # one element: every view of it is contiguous
    if fault == "noncontiguous" and name == "logits":
        return True         # logits may be a strided view (a padded row stride is taken as it is); tests/test_soft_ce_gpu.py has the strides rule
    if fault == "shape" and name in ("params[0]", "grads[0]"):
        return True         # the optimizer's parameter list takes tensors of any shape
    return False


CELLS = [(fn, name, fault) for fn, (_, names) in OPERANDS.items() for name in names for fault in FAULTS if not _left_out(fn, name, fault)]


def _valid():
    def t(shape, dtype, hi=None):
        g = torch.Generator().manual_seed(len(shape) + (hi or 0))
        x = torch.randint(0, hi, shape, generator=g).to(dtype) if hi else torch.rand(shape, generator=g).to(dtype)
        return x.to(DEV)

    batch = dict(images=t((N, H, W, 1), torch.uint8, 256), labels=t((N,), torch.int64, 10), idx=torch.tensor([0, 2], device=DEV), lut=t((1, 256), torch.float32))
    mix = dict(partner=torch.tensor([1, -1, 0], device=DEV), weight=t((N,), torch.float32), box=torch.zeros((N, 4), dtype=torch.int32, device=DEV))
    crop = torch.tensor([[0, 0, H, W, 0]] * N, dtype=torch.int32, device=DEV)
    logits = t((B, CLASSES), torch.float32)
    state = dict(exp_avg=torch.zeros(STATE, device=DEV), exp_avg_sq=torch.zeros(STATE, device=DEV), ema=torch.zeros(STATE, device=DEV))
    step, norm_coef, partials = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(2, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV)
    return {
        "augment_u8": dict(**batch, pad=1, flip=True, out=torch.empty((B, 1, H, W), device=DEV)),
        "mix_u8": dict(**batch, **mix, pad=1, flip=True, out=torch.empty((B, 1, H, W), device=DEV)),
        "resample_u8": dict(**batch, out_size=OUT, crop=crop, **mix, out=torch.empty((B, 1, OUT, OUT), device=DEV)),
        "soft_ce": dict(logits=logits, y=t((B,), torch.int64, CLASSES), y2=t((B,), torch.int64, CLASSES), w=t((B,), torch.float32), label_smoothing=0.1),
        "metrics_update": dict(logits=logits, labels=t((B,), torch.int64, CLASSES), n0=0, probs_t=torch.zeros((CLASSES, CAP), device=DEV),
                               labels_out=torch.zeros(CAP, dtype=torch.int32, device=DEV), preds_out=torch.zeros(CAP, dtype=torch.int32, device=DEV),
                               confusion=torch.zeros((CLASSES, CLASSES), dtype=torch.int64, device=DEV)),
        "metrics_auc_pairs": dict(probs_t=t((CLASSES, CAP), torch.float32), labels=t((CAP,), torch.int32, CLASSES), n=CAP,
                                  counts=torch.empty((CLASSES, 2), dtype=torch.int64, device=DEV)),
        "optim_grad_sumsq": dict(grads=[t((NUMEL,), torch.float32)], partials=partials),
        "optim_begin": dict(partials=partials, n_partials=1, max_norm=1.0, step=step, norm_coef=norm_coef),
        "optim_adamw": dict(params=[t((NUMEL,), torch.float32)], grads=[t((NUMEL,), torch.float32)], offsets=[0], decay=[True], **state,
                            table=torch.tensor([[0.99, 1e-3, 1.0, 0.0]], device=DEV), step=step, norm_coef=norm_coef, has_wd=True,
                            consts=(0.9, 0.1, 0.999, 0.001, 1e-8, 0.0, 1.0)),
    }


@pytest.fixture(scope="module")
def valid():
    """The valid call of every function, run once: the refusals below start from arguments the op accepts."""
    from kanvit import ops
    calls = _valid()
    for fn, kw in calls.items():
        getattr(ops, fn)(**kw)
    torch.cuda.synchronize()
    return calls


def _faulty(fn, name, fault, t):
    if fault == "cpu":
        return t.cpu()
    if fault == "dtype":
        return t.to({torch.uint8: torch.float32, torch.int64: torch.int32, torch.int32: torch.int64, torch.float32: torch.float16,
                     torch.float64: torch.float32}[t.dtype])
    if fault == "noncontiguous":
        v = t.new_zeros(tuple(t.shape) + (2,))[..., 0]
        assert v.shape == t.shape and not v.is_contiguous()
        return v
    if name in ("images", "logits") or (fn, name) == ("metrics_auc_pairs", "probs_t"):
        return t.reshape(-1)                                         # the rank is what these have to get right
    if name in ("idx", "partials", "exp_avg"):
        return t.reshape(1, -1)
    if (fn, name) == ("metrics_update", "probs_t"):
        return t.new_zeros((t.shape[0] + 1, t.shape[1]))             # [C, cap]: the capacity is read from it, the class count is not
    return t.new_zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 1,))


@pytest.mark.parametrize("fn,name,fault", CELLS, ids=["-".join(c) for c in CELLS])
def test_operand_refusal_names_function_operand_and_fault(valid, fn, name, fault):
    from kanvit import KanvitError, ops
    kw = dict(valid[fn])
    key = name.split("[")[0]
    if key == name:
        kw[key] = _faulty(fn, name, fault, kw[key])
    else:
        kw[key] = [_faulty(fn, name, fault, kw[key][0])]
    with pytest.raises(KanvitError) as e:
        getattr(ops, fn)(**kw)
    msg = str(e.value)
    assert OPERANDS[fn][0] in msg and name in msg and FAULTS[fault] in msg, msg
