"""Every kernel form that plan_attn_fwd / plan_attn_bwd (csrc/attention.hip) can fall back to, run and named.

The plans choose between seven forward and nine backward forms from N, D, causal, the bf16 flag, the KANVIT_ATTN_* switches, the
strides and the 16-byte alignment of three pointer groups.  Each case below places every operand in its own flat buffer as a
torch.as_strided view at a chosen element offset and chosen strides, between guard elements, runs one forward and one backward
through the library entry points and asserts
  * the set of attn* kernels that ran (torch.profiler), as literals: a case whose operands take another form than the one its row
    names fails, so the numbers below always belong to the named kernels;
  * o, lse, dq, dk, dv against the float64 oracle: exact mode at the suite's exact bounds (max|o - ref| < 1e-5, tests/_util.close for
    lse and the gradients), bf16 mode at TIGHT / LOOSE of tests/test_bf16_oracle_gpu.py::test_attention_bf16 against the oracle
    with the kernels' rounding points and the unrounded one;
  * every element of every buffer outside its view bitwise unchanged (output buffers hold a finite sentinel, input buffers NaN,
    so a read outside a view would also surface as a NaN result), the padding columns between rows included;
  * a second run on fresh buffers bitwise equal to the first.

The forward goes through kanvit_attn_fwd with ops._attn_desc's descriptor rather than ops._attn_fwd, because that helper allocates
lse itself and lse has to sit between guard elements here; the backward is ops._attn_bwd.

Rounding points of the bf16 forms (read from the kernels): every form contracts r(q) r(k)^T, r(dO) r(v)^T, r(P)^T r(dO), r(dS)^T r(q)
and r(dS) r(k) with P, dS formed in fp32 and rowsum(dO * o) unrounded.  The first-form forward (attn_fwd_kernel<.., true>) rounds the
NORMALISED probabilities, o = r(p / l) r(v); the second-form and 16-row forwards round p and divide afterwards.  `norm_first`
below follows the forward form that the case names."""
import ctypes as C
import functools

import pytest
import torch

from oracle import kan_oracle as ko
from tests._util import close, max_err, record_kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIGHT = 2e-3          # max |err| / max |ref| against the bf16-operand oracle (tests/test_bf16_oracle_gpu.py)
LOOSE = 1e-2          # ||err||_F / ||ref||_F against the unrounded oracle; test_attention_bf16 allows 1.5 * LOOSE (three chained bf16 products)
GUARD = 64            # floats before and after every view (a multiple of 4: the guard does not move the 16-byte alignment)
SENTINEL = -24680.5   # output buffers before the run
SWITCHES = ("KANVIT_ATTN_V1", "KANVIT_ATTN_V2", "KANVIT_ATTN_V3", "KANVIT_ATTN_V4", "KANVIT_ATTN_NO_DS", "KANVIT_ATTN_GRID")
INPUTS, OUTPUTS = ("q", "k", "v", "do"), ("o", "dq", "dk", "dv")
GROUP = {"q": "q", "dq": "q", "k": "k", "dk": "k", "v": "v", "dv": "v", "o": "o", "do": "o"}


# ---- kernel names of the forms (the names only: which form a case takes is written in the case lists) --------------------------
def _b(flag):
    return "true" if flag else "false"


def FIRST(dt, nkt, bf):
    return "attn_fwd_kernel<%d, %d, %s>" % (dt, nkt, _b(bf))


def SECOND(dt, nkt, bf):
    return "attn_fwd2_kernel<%d, %d, %s>" % (dt, nkt, _b(bf))


def THIRD(dt, nkt):
    return "attn_fwd3_kernel<%d, %d>" % (dt, nkt)


def FOURTH(nkt):
    return "attn_fwd4_kernel<2, %d>" % nkt


ROWS16 = "attn16_fwd_kernel<"          # a prefix: the tile count follows


def KV_Q(dt, bf):
    return {"attn_delta_kernel", "attn_bwd_kv_kernel<%d, %s>" % (dt, _b(bf)), "attn_bwd_q_kernel<%d, %s>" % (dt, _b(bf))}


def KV2_Q2(dt, bf):
    return {"attn_delta_kernel", "attn_bwd_kv2_kernel<%d, %s, false>" % (dt, _b(bf)), "attn_bwd_q2_kernel<%d, %s>" % (dt, _b(bf))}


def KV2DS_DQ(dt):
    return {"attn_delta_kernel", "attn_bwd_kv2_kernel<%d, false, true>" % dt, "attn_bwd_dq_kernel<%d>" % dt}


def KV2DS_DQ_BF16(dt, nkt):
    return {"attn_delta_kernel", "attn_bwd_kv2_kernel<%d, true, true>" % dt, "attn_bwd_dq_bf16_kernel<%d, %d>" % (dt, nkt)}


def KV3_DQ3(dt, nkt):
    return {"attn_bwd_kv3_kernel<%d, %d>" % (dt, nkt), "attn_bwd_dq3_kernel<%d, %d>" % (dt, nkt)}


def KV4_DQ3(nkt):
    return {"attn_bwd_kv4_kernel<2>", "attn_bwd_dq3_kernel<2, %d>" % nkt}


def ROWS16_BWD(bf):
    return {"attn16_bwd_kernel<%s>" % _b(bf)}


def assert_forms(names, fwd, bwd):
    """The recorded attn* kernels are exactly the forward `fwd` (a full name, or a prefix ending in '<') and the set `bwd`."""
    attn = {n for n in names if n.startswith("attn")}
    forward = attn - bwd
    assert bwd <= attn and len(forward) == 1, (sorted(attn), fwd, sorted(bwd))
    got = next(iter(forward))
    assert got.startswith(fwd) if fwd.endswith("<") else got == fwd, (sorted(attn), fwd, sorted(bwd))


# ---- problems and oracles ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(n, d, causal, bf16, b=2, h=3):
    """Inputs and the float64 reference of one (N, D, causal): computed once, shared, never written to.  Exact cases draw q, k, v
    as randn * 1.2 like the exact tests of test_attention_gpu.py; bf16 cases plain randn, the scale TIGHT and LOOSE were set for."""
    g = torch.Generator().manual_seed(100003 * n + 101 * d + 7 * causal + 3 * bf16 + b * h)
    amp = 1.0 if bf16 else 1.2
    q, k, v = (torch.randn(b, h, n, d, generator=g) * amp for _ in range(3))
    do = torch.randn(b, h, n, d, generator=g)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    o, lse = ko.attention_reference(qd, kd, vd, causal=bool(causal))
    o.backward(do.double())
    return {"q": q, "k": k, "v": v, "do": do, "ref": (o.detach(), lse.detach(), qd.grad, kd.grad, vd.grad)}


def _scores(q, k, causal, r):
    s = (r(q) @ r(k).transpose(-1, -2)) * q.shape[-1] ** -0.5
    if causal:
        n = q.shape[-2]
        s = s.masked_fill(torch.arange(n)[None, :] > torch.arange(n)[:, None], -float("inf"))
    return s


def rounded_forward(q, k, v, causal, norm_first, r=ko.bf16_round):
    s = _scores(q, k, causal, r)
    mx = s.amax(dim=-1, keepdim=True)
    p = torch.exp(s - mx)
    l = p.sum(dim=-1, keepdim=True)
    o = r(p / l) @ r(v) if norm_first else (r(p) @ r(v)) / l
    return o, (l.log() + mx).squeeze(-1)


def rounded_backward(q, k, v, o, lse, do, causal, r=ko.bf16_round):
    p = torch.exp(_scores(q, k, causal, r) - lse.unsqueeze(-1))          # exp(-inf) = 0 on the masked positions
    dp = r(do) @ r(v).transpose(-1, -2)
    delta = (do * o).sum(dim=-1, keepdim=True)
    ds = p * q.shape[-1] ** -0.5 * (dp - delta)
    return r(ds) @ r(k), r(ds).transpose(-1, -2) @ r(q), r(p).transpose(-1, -2) @ r(do)


@functools.lru_cache(maxsize=None)
def rounded_reference(n, d, causal, norm_first, b=2, h=3):
    pr = problem(n, d, causal, 1, b, h)
    q, k, v, do = (pr[name].double() for name in INPUTS)
    o, lse = rounded_forward(q, k, v, causal, norm_first)
    return (o, lse) + rounded_backward(q, k, v, o, lse, do, causal)


class _RoundedAttention(torch.autograd.Function):
    """The rounded oracle as an autograd node, for the test through the public op (gradients flow on into the sliced base)."""

    @staticmethod
    def forward(ctx, q, k, v, norm_first):
        o, lse = rounded_forward(q, k, v, False, norm_first)
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        return rounded_backward(q, k, v, o, lse, do, False) + (None,)


def fro(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def check_exact(got, ref, what):
    names = ("o", "lse", "dq", "dk", "dv")
    print(what, "exact", {n: "%.3g" % max_err(a, r) for n, a, r in zip(names, got, ref)})
    assert max_err(got[0], ref[0]) < 1e-5, (what, max_err(got[0], ref[0]))
    for name, a, r in zip(names[1:], got[1:], ref[1:]):
        assert close(a, r), (what, name, max_err(a, r), float(r.abs().max()))


def check_bf16(got, rounded, exact, what):
    names = ("o", "lse", "dq", "dk", "dv")
    print(what, "bf16 maxrel", {n: "%.3g" % maxrel(a, r) for n, a, r in zip(names, got, rounded)},
          "fro", {n: "%.3g" % fro(a, e) for n, a, e in zip(names, got, exact)})
    for name, a, r, e in zip(names, got, rounded, exact):
        assert maxrel(a, r) < TIGHT, (what, name, maxrel(a, r))
        assert fro(a, e) < 1.5 * LOOSE, (what, name, fro(a, e))
        if name != "lse":
            assert fro(a, e) > 1e-5, (what, name, fro(a, e))            # the bf16 kernels really ran


# ---- operands between guards ------------------------------------------------------------------------------------------------
class Operand:
    """A [B, H, N, D] (or [B, H, N]) view at element `GUARD + shift` of its own flat buffer, which is `fill` everywhere else."""

    def __init__(self, shape, strides, shift, fill, data=None):
        extent = sum((s - 1) * st for s, st in zip(shape, strides)) + 1
        self.buf = torch.full((GUARD + shift + extent + GUARD,), fill, device=DEV, dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.view = torch.as_strided(self.buf, shape, strides, GUARD + shift)
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=DEV)
        torch.as_strided(inside, shape, strides, GUARD + shift).fill_(True)
        self.outside = ~inside
        assert int(inside.sum()) == self.view.numel() and int(self.outside[:GUARD].sum()) == GUARD and int(self.outside[-GUARD:].sum()) == GUARD
        if data is not None:
            self.view.copy_(data)
        self.before = self.buf.clone()

    def bits(self):
        return self.buf.view(torch.int32)

    def untouched_outside(self):
        return bool((self.bits()[self.outside] == self.before.view(torch.int32)[self.outside]).all())

    def untouched(self):
        return torch.equal(self.bits(), self.before.view(torch.int32))


def layout_strides(b, h, n, d, row=None, head=None):
    sn = row or d
    sh = head or n * sn
    return (h * sh, sh, sn, 1)


def make_operands(pr, shape, shifts, row, head):
    b, h, n, d = shape
    st = layout_strides(b, h, n, d, row, head)
    ops_ = {name: Operand(shape, st, shifts.get(name, 0), float("nan"), pr[name].to(DEV)) for name in INPUTS}
    ops_.update({name: Operand(shape, st, shifts.get(name, 0), SENTINEL) for name in OUTPUTS})
    ops_["lse"] = Operand((b, h, n), (h * n, n, 1), 0, SENTINEL)
    for name, op in ops_.items():
        if name != "lse":
            assert op.view.data_ptr() % 16 == 4 * shifts.get(name, 0) % 16
    return ops_


def launch(t, causal, flags):
    """One forward + backward on the operand views.  The forward is ops._attn_fwd's call with lse placed by the caller."""
    from kanvit import _lib, ops
    v = {name: op.view for name, op in t.items()}
    assert not ops._attn_takes_general_kernels(v["q"], v["k"])
    scale = v["q"].shape[3] ** -0.5
    desc = ops._attn_desc(v["q"], v["k"], v["v"], v["o"], causal, scale, flags)
    with torch.cuda.device(v["q"].device):
        _lib.check(_lib.lib().kanvit_attn_fwd(C.byref(desc), ops._ptr(v["q"]), ops._ptr(v["k"]), ops._ptr(v["v"]), ops._ptr(v["o"]),
                                              ops._ptr(v["lse"]), ops._stream()), "kanvit_attn_fwd")
    ops._attn_bwd(v["q"], v["k"], v["v"], v["o"], v["lse"], v["do"], v["dq"], v["dk"], v["dv"], causal, scale, flags)
    torch.cuda.synchronize()


def run_case(n, d, causal, flags, bf16_numbers, shifts, row, head, fwd, bwd, b=2, h=3, recorded=True):
    """Runs the case twice on fresh guarded buffers; asserts names (first run), guards, NaN-freedom and bitwise repeatability.
    Returns the results (o, lse, dq, dk, dv) on the CPU."""
    pr = problem(n, d, causal, int(bf16_numbers), b, h)
    first = make_operands(pr, (b, h, n, d), shifts, row, head)
    if recorded:
        with record_kernels() as names:
            launch(first, causal, flags)
        assert_forms(names, fwd, bwd)
    else:
        launch(first, causal, flags)
    for name, op in first.items():
        if name in INPUTS:
            assert op.untouched(), "input buffer %s was written" % name
        else:
            assert op.untouched_outside(), "%s: an element outside the view was written" % name
            assert not bool(torch.isnan(op.view).any()), "%s holds NaN" % name
            assert not bool((op.view == SENTINEL).any()), "%s: an element of the view was not written" % name
    second = make_operands(pr, (b, h, n, d), shifts, row, head)
    launch(second, causal, flags)
    for name in OUTPUTS + ("lse",):
        assert torch.equal(first[name].bits(), second[name].bits()), "%s differs between two runs" % name
    return tuple(first[name].view.cpu() for name in ("o", "lse", "dq", "dk", "dv"))


def check_numbers(got, n, d, causal, bf16_numbers, fwd, what, b=2, h=3):
    if bf16_numbers:
        norm_first = fwd.startswith("attn_fwd_kernel<")
        check_bf16(got, rounded_reference(n, d, causal, norm_first, b, h), problem(n, d, causal, 1, b, h)["ref"], what)
    else:
        check_exact(got, problem(n, d, causal, 0, b, h)["ref"], what)


@pytest.fixture
def switches(monkeypatch):
    """set(name=value, ...) sets KANVIT_* switches and re-reads them; everything is unset and re-read again afterwards."""
    from kanvit import _lib
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    _lib.reload_config()

    def set_(**kv):
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in kv.items():
            monkeypatch.setenv(name, value)
        return _lib.reload_config()

    try:
        yield set_
    finally:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        _lib.reload_config()


Q1 = {"q": 1, "dq": 1}          # q and dq one float past a 16-byte boundary
K2 = {"k": 2, "dk": 2}          # k and dk two floats (8 bytes) past
DO1 = {"do": 1}
DK1 = {"dk": 1}
O1 = {"o": 1}

# (N, D, causal, bf16 flag, element shifts, row stride, head stride, forward, backward)
MISALIGNED = [
    # a. an operand of the row group (q, k, v, dO, dq, dk, dv) off a 16-byte boundary: first forms, scalar loads
    (50, 32, 0, 0, Q1, None, None, FIRST(1, 2, False), KV_Q(1, False)),
    (50, 32, 1, 1, Q1, None, None, FIRST(1, 2, True), KV_Q(1, True)),
    (197, 64, 0, 0, Q1, None, None, FIRST(2, 7, False), KV_Q(2, False)),
    (197, 64, 0, 1, Q1, None, None, FIRST(2, 7, True), KV_Q(2, True)),
    (197, 64, 1, 0, Q1, None, None, FIRST(2, 7, False), KV_Q(2, False)),
    (197, 64, 0, 0, K2, None, None, FIRST(2, 7, False), KV_Q(2, False)),
    (100, 64, 0, 0, DO1, None, None, ROWS16, KV_Q(2, False)),             # the forward does not see dO: its default form
    (100, 64, 0, 0, DK1, None, None, ROWS16, KV_Q(2, False)),
    (197, 64, 0, 1, DK1, None, None, ROWS16, KV_Q(2, True)),
    # b. o alone off the boundary (dO aligned, same strides): first-form forward, second-form backward behind attn_delta_kernel
    (50, 32, 0, 0, O1, None, None, FIRST(1, 2, False), KV2DS_DQ(1)),
    (50, 32, 1, 0, O1, None, None, FIRST(1, 2, False), KV2_Q2(1, False)),
    (50, 32, 0, 1, O1, None, None, FIRST(1, 2, True), KV2DS_DQ_BF16(1, 4)),
    (100, 64, 0, 0, O1, None, None, FIRST(2, 4, False), KV2DS_DQ(2)),
    (197, 64, 0, 0, O1, None, None, FIRST(2, 7, False), KV2_Q2(2, False)),      # N = 193..208 reserves no fp32 dS
    (197, 64, 0, 1, O1, None, None, FIRST(2, 7, True), KV2DS_DQ_BF16(2, 8)),    # the bf16 dS the default path reserves and never uses
    (197, 64, 1, 1, O1, None, None, FIRST(2, 7, True), KV2_Q2(2, True)),
    (224, 64, 0, 0, O1, None, None, FIRST(2, 7, False), KV2DS_DQ(2)),
    (224, 64, 0, 1, O1, None, None, FIRST(2, 7, True), KV2DS_DQ_BF16(2, 8)),
    # c. strides, base pointers aligned: a stride that is no multiple of four floats anywhere takes the first forms
    (100, 64, 0, 0, {}, 66, None, FIRST(2, 4, False), KV_Q(2, False)),
    (100, 64, 0, 0, {}, 64, 6402, FIRST(2, 4, False), KV_Q(2, False)),          # only the later heads are misaligned
    (100, 64, 0, 0, {}, 68, None, ROWS16, KV4_DQ3(4)),                          # padded rows that are still float4 rows
    (197, 64, 0, 1, {}, 68, None, ROWS16, ROWS16_BWD(True)),
]


def _id(c):
    n, d, causal, bf, shifts, row, head = c[:7]
    where = "+".join("%s%d" % kv for kv in sorted(shifts.items())) or "aligned"
    return "%dx%d%s%s-%s%s%s" % (n, d, "-causal" if causal else "", "-bf16" if bf else "", where,
                                 "-row%d" % row if row else "", "-head%d" % head if head else "")


@pytest.mark.parametrize("case", MISALIGNED, ids=_id)
def test_misaligned_and_strided_operands(case, switches):
    n, d, causal, bf, shifts, row, head, fwd, bwd = case
    got = run_case(n, d, causal, bf, bool(bf), shifts, row, head, fwd, bwd)
    check_numbers(got, n, d, causal, bool(bf), fwd, _id(case))


SECOND_FORMS = [
    # d. KANVIT_ATTN_V2=1: the exact second forms that no default shape reaches
    (17, 32, 0, 0, SECOND(1, 1, False), KV2DS_DQ(1)),
    (64, 64, 0, 0, SECOND(2, 2, False), KV2DS_DQ(2)),
    (100, 32, 0, 0, SECOND(1, 4, False), KV2DS_DQ(1)),
    (100, 32, 1, 0, SECOND(1, 4, False), KV2_Q2(1, False)),
    (197, 64, 0, 0, SECOND(2, 7, False), KV2DS_DQ(2)),
    (197, 64, 1, 0, SECOND(2, 7, False), KV2_Q2(2, False)),
    (224, 64, 0, 0, SECOND(2, 7, False), KV2DS_DQ(2)),
    (256, 32, 0, 0, FIRST(1, 8, False), KV2DS_DQ(1)),          # eight key tiles: the forward has no second form
]


@pytest.mark.parametrize("n,d,causal,bf,fwd,bwd", SECOND_FORMS)
def test_second_forms_behind_their_switch(n, d, causal, bf, fwd, bwd, switches):
    assert "attn_v2=1" in switches(KANVIT_ATTN_V2="1")
    got = run_case(n, d, causal, bf, bool(bf), {}, None, None, fwd, bwd)
    check_numbers(got, n, d, causal, bool(bf), fwd, "v2 %dx%d causal=%d" % (n, d, causal))


DEFAULT_FORMS = [
    # e. N = 225..256 (D <= 32 stays on the one-work-group kernels up to 256)
    (225, 32, 0, 0, FIRST(1, 8, False), KV3_DQ3(1, 8)),
    (256, 32, 0, 0, FIRST(1, 8, False), KV3_DQ3(1, 8)),
    (225, 32, 1, 0, FIRST(1, 8, False), KV2_Q2(1, False)),
    (250, 8, 0, 0, FIRST(1, 8, False), KV_Q(1, False)),
    (250, 8, 1, 0, FIRST(1, 8, False), KV_Q(1, False)),
    (225, 32, 0, 1, FIRST(1, 8, True), KV2DS_DQ_BF16(1, 8)),
    # f. around the 16-row / fourth / third boundaries at D = 64
    (200, 64, 1, 0, FOURTH(7), KV2_Q2(2, False)),
    (201, 64, 1, 0, THIRD(2, 7), KV2_Q2(2, False)),
    (205, 64, 0, 0, THIRD(2, 7), KV2_Q2(2, False)),
    (208, 64, 0, 0, THIRD(2, 7), KV2_Q2(2, False)),
    (208, 64, 0, 1, SECOND(2, 7, True), KV2DS_DQ_BF16(2, 8)),
    (209, 64, 0, 0, THIRD(2, 7), KV3_DQ3(2, 8)),
    # g. ragged head sizes: 32 < D < 64 and D no multiple of 4 on the two-tile first forms; the flag needs D % 16 == 0
    (100, 34, 0, 0, FIRST(2, 4, False), KV_Q(2, False)),
    (100, 62, 0, 0, FIRST(2, 4, False), KV_Q(2, False)),
    (100, 48, 0, 0, FIRST(2, 4, False), KV_Q(2, False)),
    (100, 48, 0, 1, FIRST(2, 4, True), KV_Q(2, True)),
    (100, 48, 1, 1, FIRST(2, 4, True), KV_Q(2, True)),
    (50, 16, 0, 1, FIRST(1, 2, True), KV_Q(1, True)),
    (50, 30, 0, 1, FIRST(1, 2, False), KV_Q(1, False)),        # the flag is refused (D % 16 != 0): exact kernels, exact bounds
]


@pytest.mark.parametrize("n,d,causal,bf,fwd,bwd", DEFAULT_FORMS)
def test_default_forms_at_aligned_operands(n, d, causal, bf, fwd, bwd, switches):
    bf16_numbers = bool(bf) and d % 16 == 0
    got = run_case(n, d, causal, bf, bf16_numbers, {}, None, None, fwd, bwd)
    check_numbers(got, n, d, causal, bf16_numbers, fwd, "default %dx%d causal=%d bf16=%d" % (n, d, causal, bf))


HEAD_WALKS = [
    # h. KANVIT_ATTN_GRID=2 on 7 heads: the persistent third forms walk 4 and 3 heads
    (20, 64, THIRD(2, 1), KV3_DQ3(2, 2)),
    (40, 32, THIRD(1, 2), KV3_DQ3(1, 2)),
    (64, 64, THIRD(2, 2), KV3_DQ3(2, 2)),
    (100, 32, THIRD(1, 4), KV3_DQ3(1, 4)),
]


@pytest.mark.parametrize("n,d,fwd,bwd", HEAD_WALKS)
def test_third_forms_walk_several_heads(n, d, fwd, bwd, switches):
    assert "attn_grid=2" in switches(KANVIT_ATTN_GRID="2")
    walked = run_case(n, d, 0, 0, False, {}, None, None, fwd, bwd, b=1, h=7)
    check_numbers(walked, n, d, 0, False, fwd, "walk %dx%d" % (n, d), b=1, h=7)
    assert "attn_grid=0" in switches()
    spread = run_case(n, d, 0, 0, False, {}, None, None, fwd, bwd, b=1, h=7, recorded=False)
    for name, a, c in zip(("o", "lse", "dq", "dk", "dv"), walked, spread):
        assert torch.equal(a, c), name          # a head's sums have one order, whichever work-group takes it


@pytest.mark.parametrize("n,d", [(100, 64), (50, 32)])
@pytest.mark.parametrize("amp", [False, True])
def test_public_op_on_column_slices(n, d, amp, switches):
    """i. ops.attention on q, k, v that are column slices of one [B, H, N, 3 D + 4] tensor starting at column 1: rows of 3 D + 4
    floats, one float past a 16-byte boundary -> the first forms, and gradients that land in the right columns of the base."""
    from kanvit import ops
    b, h = 2, 3
    dt = 1 if d <= 32 else 2
    nkt = (2, 4)[d == 64]
    g = torch.Generator().manual_seed(n + d)
    base0 = torch.randn(b, h, n, 3 * d + 4, generator=g) * (1.0 if amp else 1.2)
    do = torch.randn(b, h, n, d, generator=g)

    def slices(t):
        return tuple(t[..., 1 + i * d:1 + (i + 1) * d] for i in range(3))

    base = base0.to(DEV).requires_grad_(True)
    with record_kernels() as names:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            o = ops.attention(*slices(base))
        o.backward(do.to(DEV))
    assert_forms(names, FIRST(dt, nkt, amp), KV_Q(dt, amp))
    grad = base.grad.cpu()
    assert float(grad[..., 0].abs().max()) == 0.0 and float(grad[..., 3 * d + 1:].abs().max()) == 0.0
    assert not bool(torch.isnan(grad).any()) and not bool(torch.isnan(o).any())

    def reference(rounded):
        bd = base0.double().requires_grad_(True)
        od = _RoundedAttention.apply(*slices(bd), True) if rounded else ko.attention_reference(*slices(bd))[0]
        od.backward(do.double())
        return od.detach(), bd.grad

    o_e, g_e = reference(False)
    got = (o.detach().cpu(),) + slices(grad)
    if not amp:
        assert max_err(got[0], o_e) < 1e-5
        for a, r in zip(got[1:], slices(g_e)):
            assert close(a, r)
    else:
        o_t, g_t = reference(True)
        for name, a, r, e in zip(("o", "dq", "dk", "dv"), got, (o_t,) + slices(g_t), (o_e,) + slices(g_e)):
            assert maxrel(a, r) < TIGHT, (name, maxrel(a, r))
            assert 1e-5 < fro(a, e) < 1.5 * LOOSE, (name, fro(a, e))
