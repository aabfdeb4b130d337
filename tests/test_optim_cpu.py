"""The fused AdamW step without a GPU: the schedule table against closed forms, the float32 restatement of the kernel's sequence
against torch.optim.AdamW, the precondition of the GPU tests' clip coefficients, the C ABI's host-side refusals, train.py's flags."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from kanvit import _lib, optim
from kanvit._lib import KanvitError
from tests import _optim_ref as R

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


# ---- step_table ---------------------------------------------------------------------------------------------------------------
def test_table_warmup_and_cosine_closed_forms():
    lr, lo, wd, b1, b2, d, T, W = 3e-3, 1e-5, 0.05, 0.9, 0.999, 0.9998, 1000, 100
    tab = optim.step_table(T, lr, (b1, b2), wd, W, "cosine", lo, d)
    assert tab.dtype == np.float32 and tab.shape == (T, 4)

    def lr_of(t):            # undo the bias correction in float64: the row is float32, so to 2^-23
        return float(tab[t - 1, 1]) * (1.0 - b1 ** t)
    rel = 2.0 ** -23
    assert lr_of(1) == pytest.approx(lr / W, rel=rel)                       # warm-up starts at lr / warmup_steps ...
    assert lr_of(W) == pytest.approx(lr, rel=rel)                           # ... and ends at lr
    assert lr_of(W // 2) == pytest.approx(lr * 0.5, rel=rel)
    assert lr_of((T + W) // 2) == pytest.approx(0.5 * (lr + lo), rel=rel)   # the cosine's mid point
    assert lr_of(T) == pytest.approx(lo, rel=rel)                           # and its last point
    assert all(lr_of(t) > lr_of(t + 1) for t in range(W, T))                # decreasing in between
    for t in (1, 2, W, T):
        lr_t = lr * t / W if t <= W else lo + (lr - lo) * 0.5 * (1.0 + math.cos(math.pi * (t - W) / (T - W)))
        want = np.array([1.0 - lr_t * wd, lr_t / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), 1.0 - d ** t]).astype(np.float32)
        assert np.array_equal(tab[t - 1], want), (t, tab[t - 1], want)


def test_table_bias_corrections_and_constant_schedule():
    tab = optim.step_table(200000, 1e-3, (0.9, 0.999), 0.0, 0, "constant", 0.0, 0.0)
    assert tab[0, 1] == np.float32(1e-3 / (1.0 - 0.9)) and tab[0, 2] == np.float32(math.sqrt(1.0 - 0.999))      # t = 1
    assert tab[-1, 1] == np.float32(1e-3) and tab[-1, 2] == np.float32(1.0)                                     # large t: no correction left
    assert np.all(tab[:, 0] == 1.0) and np.all(tab[:, 3] == 1.0)            # no decay; ema_decay = 0: 1 - 0^t = 1
    for bad in (dict(total_steps=0), dict(total_steps=4, warmup_steps=5), dict(total_steps=4, schedule="linear"), dict(total_steps=4, ema_decay=1.0)):
        with pytest.raises(ValueError):
            optim.step_table(**{"lr": 1e-3, **bad})


def test_rounded_constants_round_once_from_float64():
    c = optim.rounded_constants((0.9, 0.999), 1e-8, 0.9998)
    want = [np.float32(x) for x in (0.9, 1.0 - 0.9, 0.999, 1.0 - 0.999, 1e-8, 0.9998, 1.0 - 0.9998)]
    assert [np.float32(x) for x in c] == want
    assert np.float32(c[1]) != np.float32(1.0) - np.float32(0.9)            # not the float32 difference of rounded operands


# ---- the restatement against torch.optim.AdamW ----------------------------------------------------------------------------------
def test_restatement_tracks_torch_adamw_within_torchs_own_fp32_error():
    """Six steps with weight decay, warm-up and cosine on, gradients whose scale runs over 1e-7 .. 1e2.  Reference: torch.optim.AdamW in
    float64 with the step's learning rate set from the float64 schedule.  Yardstick e_t: torch's own float32 AdamW on the same inputs.
    Per step, in the max norm, the restatement's error is at most 2 e_t + u, u = one ulp of the largest parameter + lr * 2^-23 (the
    table's rows and the seven constants are each rounded once: a relative 2^-24 on the step).
    Measured (units of u, steps 1..6): restatement 1.21 / 1.52 / 2.25 / 2.52 / 3.16 / 3.72 and torch-fp32 the same to three digits: the
    largest error of both sits on the largest parameters, where it is the rounding of p itself and the two round alike."""
    steps, lr, lo, wd, betas, eps, W = 6, 1e-2, 1e-4, 0.05, (0.9, 0.999), 1e-8, 2
    rng = np.random.default_rng(6)
    n = 4096
    p0 = rng.standard_normal(n).astype(np.float32)
    scale = 10.0 ** rng.uniform(-7, 2, size=n)
    grads = [(rng.standard_normal(n) * scale).astype(np.float32) for _ in range(steps)]
    table = optim.step_table(steps, lr, betas, wd, W, "cosine", lo, 0.0)
    consts = optim.rounded_constants(betas, eps, 0.0)
    ref = R.Optimizer([p0], [True], table, consts)
    p64 = torch.nn.Parameter(torch.from_numpy(p0).double())
    p32 = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    o64 = torch.optim.AdamW([p64], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    o32 = torch.optim.AdamW([p32], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    for t in range(1, steps + 1):
        lr_t = lr * t / W if t <= W else lo + (lr - lo) * 0.5 * (1.0 + math.cos(math.pi * (t - W) / (steps - W)))
        for o, p, g in ((o64, p64, torch.from_numpy(grads[t - 1]).double()), (o32, p32, torch.from_numpy(grads[t - 1]))):
            o.param_groups[0]["lr"] = lr_t
            p.grad = g
            o.step()
        ref.step([grads[t - 1]])
        want = p64.detach().numpy()
        e_t = float(np.abs(p32.detach().numpy().astype(np.float64) - want).max())
        err = float(np.abs(ref.p[0].astype(np.float64) - want).max())
        u = float(np.spacing(np.float32(np.abs(want).max()))) + lr * 2.0 ** -23
        print(f"step {t}: restatement {err / u:.2f} u, torch-fp32 {e_t / u:.2f} u")
        assert err <= 2.0 * e_t + u, (t, err, e_t, u)


def test_restatement_asserts_float32_intermediates_and_skips_what_is_off():
    p, g = np.float32([1.0, -2.0]), np.float32([0.5, 0.25])
    z = np.zeros(2, np.float32)
    row, consts = np.float32([0.5, 0.1, 1.0, 1.0]), optim.rounded_constants((0.9, 0.999), 1e-8, 0.5)
    a = R.adamw_f32(p, g, z, z, z, row, consts, coef=np.float32(1.0))
    b = R.adamw_f32(p, g, z, z, z, row, consts, coef=None)
    assert all(x.dtype == np.float32 for x in a) and all(np.array_equal(x, y) for x, y in zip(a, b))        # coef = 1 is no clipping
    c = R.adamw_f32(p, g, z, z, None, row, consts, decay=False)
    d = R.adamw_f32(p, g, z, z, None, row, consts, has_wd=False)
    assert c[3] is None and np.array_equal(c[0], d[0]) and not np.array_equal(c[0], a[0])
    with pytest.raises(AssertionError):
        R._f32(np.zeros(2))                                                  # a float64 intermediate is caught


# ---- the clip coefficients the GPU tests compare bit for bit ----------------------------------------------------------------------
def test_clip_coefficients_do_not_depend_on_the_order_of_the_sum(lib):
    """For every synthetic clipping case of tests/test_optim_gpu.py (R.clip_cases: each with the gradient set that test really runs)
    and for its 1e25 case, the float64 sum of squares is taken sequentially, pairwise and in the device's order; all three must round
    to the same float32 norm and coefficient.  A case that fails here is replaced, not tolerated.  (The model cases check the same on
    their own gradients, inside the GPU test.)"""
    names = []
    for name, numels, max_norm, none, steps in R.clip_cases(lib.kanvit_optim_max_tensors()):
        names.append(name)
        for step in range(steps):
            got = R.coefficient_in_three_orders(R.case_grads(numels, step, none=none), max_norm)
            assert got[0] == got[1] == got[2], (name, step, got)
            if max_norm == 0.5:
                assert got[0][1] < 1.0, (name, step, got)                    # "clipping binds" means it
            else:
                assert got[0][1] == 1.0, (name, step, got)
    assert len(names) == len(set(names)) == sum(c[1] is not None for c in R.CONFIGS.values()) + 4
    n, value, max_norm = R.HUGE
    got = R.coefficient_in_three_orders([np.full(n, value, np.float32)], max_norm)
    assert got[0] == got[1] == got[2] and 0.0 < got[0][1] < 1.0, got


def test_norm_restatement_keeps_what_float32_would_overflow():
    n, value, max_norm = R.HUGE
    g = [np.full(n, value, np.float32)]
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(value) * np.float32(value))
    norm, coef = R.norm_and_coef(R.grads_sumsq(g), max_norm)
    assert np.isfinite(norm) and norm == np.float32(math.sqrt(5000.0) * float(np.float32(1e25))) and 0.0 < coef < 1e-25
    assert np.isnan(R.norm_and_coef(np.nan, 1.0)[1])                         # a NaN norm is a NaN coefficient, as torch's clamp leaves it


# ---- what the default filter decays ---------------------------------------------------------------------------------------------------
def undecayed_by_name(name):
    """The recipe's no-weight-decay set, by NAME: the class token, LayerNorm parameters (the head's is mlp_head.0), biases, SineKAN's
    frequencies, FastKAN's grid."""
    leaf = name.split(".")[-1]
    return name == "v_class" or "norm" in name or name.startswith("mlp_head.0.") or leaf in ("bias", "freq", "grid")


@pytest.mark.parametrize("kind", ["cheby", "efficientkan", "fast", "sine", "fourier", "vanilla"])
def test_default_filter_decays_the_weight_matrices_only(kind):
    from model import VisionTransformer
    model = VisionTransformer((3, 8, 8), 2, 1, 16, 2, 5, type=kind)
    flags = {name: optim.default_decay_filter(p) for name, p in model.named_parameters()}
    assert flags["v_class"] is False and model.v_class.ndim == 2             # a [1, d] row: ndim alone would decay it
    assert flags["blocks.0.norm1.weight"] is False and flags["mlp_head.1.bias"] is False
    assert flags["blocks.0.ff.0.weight"] is True and flags["mlp_head.1.weight"] is True
    for name, flag in flags.items():
        assert flag == (not undecayed_by_name(name)), (kind, name, tuple(dict(model.named_parameters())[name].shape))
    assert optim.default_decay_filter(torch.zeros(())) is False and optim.default_decay_filter(torch.zeros(1, 1, 1, 28)) is False


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
NEW = ("kanvit_optim_max_tensors", "kanvit_optim_sumsq_workspace", "kanvit_optim_sumsq", "kanvit_optim_begin", "kanvit_optim_adamw")


def test_symbols_are_declared_and_exported(lib):
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kanvit.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SYMBOLS and hasattr(raw, name), name
    P = C.c_void_p
    assert _lib.SYMBOLS["kanvit_optim_max_tensors"] == (C.c_int, [])
    assert _lib.SYMBOLS["kanvit_optim_sumsq_workspace"] == (C.c_size_t, [C.c_int, P])
    assert _lib.SYMBOLS["kanvit_optim_sumsq"] == (C.c_int, [C.c_int, P, P, P, C.c_size_t, P])
    assert _lib.SYMBOLS["kanvit_optim_begin"] == (C.c_int, [P, C.c_int64, C.c_double, P, P, P])
    assert _lib.SYMBOLS["kanvit_optim_adamw"] == (C.c_int, [C.c_int] + [P] * 8 + [C.c_int64, P, C.c_int64, P, P, C.c_int] + [C.c_float] * 7 + [P])
    assert [n for n in _lib.SYMBOLS if "optim" in n] == list(NEW)
    assert lib.kanvit_abi_version() == 7
    m = re.search(r"#define KANVIT_OPTIM_MAX_TENSORS (\d+)", header)
    assert int(m.group(1)) == lib.kanvit_optim_max_tensors() >= 32
    assert int(re.search(r"#define KANVIT_OPTIM_CHUNK (\d+)", header).group(1)) == _lib.OPTIM_CHUNK == R.CHUNK


def test_workspace_is_one_double_per_chunk(lib):
    def ws(*numels):
        return lib.kanvit_optim_sumsq_workspace(len(numels), (C.c_int64 * len(numels))(*numels))
    ch = _lib.OPTIM_CHUNK
    assert [ws(0), ws(1), ws(ch), ws(ch + 1), ws(2 * ch + 1)] == [0, 8, 8, 16, 24]
    assert ws(*R.EDGE_NUMELS) == 8 * sum((n + ch - 1) // ch for n in R.EDGE_NUMELS) and ws() == 0
    assert ws(4, -1) == 0 and lib.kanvit_optim_sumsq_workspace(2, None) == 0 and lib.kanvit_optim_sumsq_workspace(-1, None) == 0


def _refused(lib, rc, who, *words):
    msg = lib.kanvit_last_error().decode()
    assert rc == EINVAL and msg.startswith(who + ":") and all(w in msg for w in words), (rc, msg)


def _arr(ctype, *vals):
    return (ctype * len(vals))(*vals)


def test_sumsq_and_begin_refuse_on_the_host(lib):
    """None of these reaches a launch: they pass on a machine without a GPU.  The pointers are never dereferenced."""
    who, cap, fake = "kanvit_optim_sumsq", lib.kanvit_optim_max_tensors(), 0x1000
    one = _arr(C.c_int64, 8)
    _refused(lib, lib.kanvit_optim_sumsq(1, None, one, fake, 64, None), who, "null")
    _refused(lib, lib.kanvit_optim_sumsq(1, _arr(C.c_void_p, None), one, fake, 64, None), who, "tensor 0", "null")
    _refused(lib, lib.kanvit_optim_sumsq(1, _arr(C.c_void_p, fake), one, None, 64, None), who, "null workspace")
    _refused(lib, lib.kanvit_optim_sumsq(cap + 1, _arr(C.c_void_p, *[fake] * (cap + 1)), _arr(C.c_int64, *[8] * (cap + 1)), fake, 1 << 20, None),
             who, f"n={cap + 1}", str(cap))
    _refused(lib, lib.kanvit_optim_sumsq(-1, None, None, fake, 64, None), who, "n=-1")
    _refused(lib, lib.kanvit_optim_sumsq(1, _arr(C.c_void_p, fake), _arr(C.c_int64, -8), fake, 64, None), who, "numel=-8")
    _refused(lib, lib.kanvit_optim_sumsq(1, _arr(C.c_void_p, fake + 2), one, fake, 64, None), who, "tensor 0", "4 bytes")
    _refused(lib, lib.kanvit_optim_sumsq(2, _arr(C.c_void_p, fake, fake), _arr(C.c_int64, 8, _lib.OPTIM_CHUNK + 1), fake, 16, None), who,
             "16 bytes", "24 needed")
    _refused(lib, lib.kanvit_optim_sumsq(1, _arr(C.c_void_p, fake), one, fake + 4, 64, None), who, "8 bytes")
    assert lib.kanvit_optim_sumsq(0, None, None, None, 0, None) == 0                                  # nothing to do is no error
    assert lib.kanvit_optim_sumsq(1, _arr(C.c_void_p, None), _arr(C.c_int64, 0), None, 0, None) == 0  # a tensor without elements
    who = "kanvit_optim_begin"
    _refused(lib, lib.kanvit_optim_begin(None, 0, 0.0, None, fake, None), who, "null")
    _refused(lib, lib.kanvit_optim_begin(None, 0, 0.0, fake, None, None), who, "null")
    _refused(lib, lib.kanvit_optim_begin(None, 3, 0.0, fake, fake, None), who, "null partials")
    _refused(lib, lib.kanvit_optim_begin(fake, -1, 0.0, fake, fake, None), who, "n_partials=-1")
    _refused(lib, lib.kanvit_optim_begin(None, 0, 1.0, fake, fake, None), who, "max_norm")
    _refused(lib, lib.kanvit_optim_begin(fake, 1, float("nan"), fake, fake, None), who, "NaN")
    _refused(lib, lib.kanvit_optim_begin(fake + 4, 1, 1.0, fake, fake, None), who, "aligned")
    _refused(lib, lib.kanvit_optim_begin(fake, 1, 1.0, fake + 4, fake, None), who, "aligned")


def test_adamw_refuses_on_the_host(lib):
    who, cap, fake = "kanvit_optim_adamw", lib.kanvit_optim_max_tensors(), 0x1000
    f = [C.c_float(x) for x in optim.rounded_constants((0.9, 0.999), 1e-8, 0.0)]

    def call(n=1, params=(fake,), grads=(fake,), offsets=(0,), numel=(8,), decay=(1,), m=fake, v=fake, e=None, S=64, table=fake, rows=4,
             step=fake, nc=None):
        arr = [None if a is None else _arr(t, *a) for t, a in ((C.c_void_p, params), (C.c_void_p, grads), (C.c_int64, offsets),
                                                              (C.c_int64, numel), (C.c_int32, decay))]
        return lib.kanvit_optim_adamw(n, *arr, m, v, e, S, table, rows, step, nc, 1, *f, None)
    _refused(lib, call(m=None), who, "null")
    _refused(lib, call(table=None), who, "null")
    _refused(lib, call(step=None), who, "null")
    _refused(lib, call(params=None), who, "null")
    _refused(lib, call(decay=None), who, "null")
    _refused(lib, call(params=(None,)), who, "tensor 0", "null")
    _refused(lib, call(grads=(None,)), who, "tensor 0", "null")
    many = cap + 1
    _refused(lib, call(n=many, params=[fake] * many, grads=[fake] * many, offsets=[0] * many, numel=[1] * many, decay=[0] * many), who, f"n={many}")
    _refused(lib, call(numel=(-1,)), who, "numel=-1")
    _refused(lib, call(params=(fake + 1,)), who, "4 bytes")
    _refused(lib, call(grads=(fake + 2,)), who, "4 bytes")
    _refused(lib, call(offsets=(2,)), who, "multiple of 4")
    _refused(lib, call(offsets=(60,)), who, "offset=60", "numel=8")          # the slice ends past the state
    _refused(lib, call(offsets=(-4,)), who, "offset=-4")
    _refused(lib, call(m=fake + 4), who, "16 bytes")
    _refused(lib, call(e=fake + 8), who, "16 bytes")
    _refused(lib, call(rows=0), who, "table_rows=0")
    _refused(lib, call(step=fake + 4), who, "aligned")
    _refused(lib, call(nc=fake + 2), who, "aligned")
    assert call(n=0, params=None, grads=None, offsets=None, numel=None, decay=None) == 0
    assert call(params=(None,), grads=(None,), numel=(0,)) == 0             # only a tensor without elements: no launch


def test_cpu_tensors_are_refused_without_a_fallback():
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(KanvitError, match="no CPU fallback"):
        optim.KanvitAdamW([p], total_steps=3)
    from kanvit import ops
    with pytest.raises(KanvitError, match="no CPU fallback"):
        ops.optim_grad_sumsq([torch.zeros(3)], torch.zeros(1, dtype=torch.float64))
    with pytest.raises(KanvitError, match="no CPU fallback"):
        ops.optim_begin(None, 0, 0.0, torch.zeros(1, dtype=torch.int64), torch.zeros(2))
    with pytest.raises(KanvitError, match="no CPU fallback"):
        ops.optim_adamw([p], [torch.zeros(3)], [0], [True], torch.zeros(4), torch.zeros(4), None, torch.ones(1, 4), torch.zeros(1, dtype=torch.int64),
                        None, False, optim.rounded_constants((0.9, 0.999), 1e-8, 0.0))


# ---- train.py's flags ---------------------------------------------------------------------------------------------------------------
def test_train_defaults_and_refusals():
    import train
    args = train.parse([])
    assert args.optimizer == "adam" and args.weight_decay == 0.0 and args.clip_grad_norm == 0.0 and args.warmup_steps == 0
    assert args.lr_schedule == "constant" and args.min_lr == 0.0 and args.ema_decay == 0.0
    ok = train.parse(["--optimizer", "kanvit-adamw", "--weight-decay", "0.05", "--clip-grad-norm", "1", "--warmup-steps", "5",
                      "--lr-schedule", "cosine", "--min-lr", "1e-5", "--ema-decay", "0.999"])
    assert ok.optimizer == "kanvit-adamw" and ok.lr_schedule == "cosine"
    for flags in (["--weight-decay", "0.05"], ["--clip-grad-norm", "1"], ["--warmup-steps", "5"], ["--lr-schedule", "cosine"],
                  ["--min-lr", "1e-5"], ["--ema-decay", "0.99"]):
        with pytest.raises(SystemExit, match="kanvit-adamw"):
            train.parse(flags)                                               # a recipe flag without the optimizer is not silently ignored
    with pytest.raises(SystemExit, match="grid-extend"):
        train.parse(["--optimizer", "kanvit-adamw", "--model-type", "efficientkan", "--grid-extend", "3:10"])
    for flags in (["--ema-decay", "1.0"], ["--weight-decay", "-1"], ["--clip-grad-norm", "-1"], ["--warmup-steps", "-1"], ["--min-lr", "-1"]):
        with pytest.raises(SystemExit):
            train.parse(["--optimizer", "kanvit-adamw", *flags])
    import argparse
    by_hand = argparse.Namespace(synthetic=True, weight_decay=0.1)           # tests build namespaces by hand: every new flag has a default
    with pytest.raises(SystemExit, match="kanvit-adamw"):
        train.check_optimizer_args(by_hand)
    train.check_optimizer_args(argparse.Namespace(synthetic=True))
