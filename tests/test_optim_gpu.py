"""KanvitAdamW on the GPU against the host restatement (tests/_optim_ref.py), bit for bit.

The tensor list is the smallest that can go wrong (R.EDGE_NUMELS: around one 16-byte group, one round of 256 lanes, one chunk, two
chunks, no element), with parameters that are views at a 4-byte offset, gradients at 4, 8 and 12 bytes, a gradient that is None on two
steps and mixed decay flags; MAX and MAX + 1 tiny tensors sit on both sides of the launch boundary."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import _optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MISALIGNED_PARAMS = (4, 8)          # of R.EDGE_NUMELS: 255 elements, and exactly one chunk (whole 16-byte groups on the 4-byte path)


def _optim():
    from kanvit import optim
    return optim


def _device_params(values, misalign):
    """Leaf tensors holding `values`; with misalign, those named above are views one element into their buffer."""
    out = []
    for k, v in enumerate(values):
        off = 1 if misalign and k in MISALIGNED_PARAMS else 0
        buf = torch.zeros(v.size + off, device=DEV)
        buf[off:] = torch.from_numpy(v).to(DEV)
        out.append(buf[off:].detach().requires_grad_())
        assert out[-1].data_ptr() % 16 == 4 * off or v.size == 0
    return out


def _set_grads(params, grads, misalign):
    """p.grad = the step's gradient, with misalign at k % 4 elements (0, 4, 8, 12 bytes) into its buffer; None stays None."""
    for k, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            p.grad = None
            continue
        off = k % 4 if misalign else 0
        buf = torch.zeros(g.size + off, device=DEV)
        buf[off:] = torch.from_numpy(g).to(DEV)
        p.grad = buf[off:]


def _make(name, numels, misalign=True, table_steps=R.STEPS, seed=0):
    optim = _optim()
    ema, max_norm, wd = R.CONFIGS[name]
    kw = R.case_table(ema, wd, table_steps)
    params = _device_params(R.case_params(numels, seed), misalign)
    decay = R.case_decay(numels)
    flags = {id(p): d for p, d in zip(params, decay)}
    opt = optim.KanvitAdamW(params, eps=1e-8, max_grad_norm=max_norm, decay_filter=lambda p: flags[id(p)], **kw)
    ref = R.Optimizer(R.case_params(numels, seed), decay, optim.step_table(**kw), optim.rounded_constants(kw["betas"], 1e-8, kw["ema_decay"]),
                      max_norm=max_norm, ema=ema, has_wd=wd != 0.0)
    return opt, params, ref


def _snapshot(opt, params):
    snap = {"p": [p.detach().cpu().numpy().copy() for p in params],
            "m": [opt.moments(p)[0].cpu().numpy().copy() for p in params], "v": [opt.moments(p)[1].cpu().numpy().copy() for p in params],
            "e": [opt.ema(p).cpu().numpy().copy() for p in params] if "ema" in opt.flat else None,
            "norm": opt.grad_norm.cpu().numpy().copy(), "coef": opt.clip_coef.cpu().numpy().copy(), "t": int(opt.flat["step"])}
    return snap


@functools.lru_cache(maxsize=None)
def _run(name, numels=tuple(R.EDGE_NUMELS), misalign=True, steps=R.STEPS, table_steps=R.STEPS, none=tuple(sorted(R.NONE_GRAD))):
    """`steps` steps of config `name` on the device and on the host: [(device snapshot, host optimizer state)] per step."""
    opt, params, ref = _make(name, list(numels), misalign, table_steps)
    out = []
    for s in range(steps):
        grads = R.case_grads(list(numels), s, none=set(none))
        _set_grads(params, grads, misalign)
        opt.step()
        ref.step(grads)
        out.append((_snapshot(opt, params), copy.deepcopy(ref)))
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_equals_host(run, what):
    for s, (dev, ref) in enumerate(run):
        assert dev["t"] == ref.t == s + 1
        for k in range(len(ref.p)):
            for key, host in (("p", ref.p), ("m", ref.m), ("v", ref.v), ("e", ref.e)):
                if host is not None:
                    assert _same(dev[key][k], host[k]), f"{what}: step {s}, tensor {k} ({host[k].size} elements), {key}"
        if ref.max_norm is not None:
            assert _same(dev["norm"], np.asarray(ref.norm)) and _same(dev["coef"], np.asarray(ref.coef)), (what, s, dev["norm"], ref.norm, dev["coef"], ref.coef)
        else:
            assert np.isnan(dev["norm"]) and dev["coef"] == 1.0


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_four_steps_equal_the_restatement_bitwise(name):
    run = _run(name)
    _assert_equals_host(run, name)
    ema, max_norm, wd = R.CONFIGS[name]
    coefs = [float(dev["coef"]) for dev, _ in run]
    assert all(c < 1.0 for c in coefs) if max_norm == 0.5 else all(c == 1.0 for c in coefs)
    assert (run[0][0]["e"] is not None) == ema
    first, none_steps = run[0][0], sorted(s for k, s in R.NONE_GRAD if k == 3)
    for s in none_steps:                      # no gradient: the tensor, its moments and its EMA stand still while the step advances
        for key in ("p", "m", "v") + (("e",) if ema else ()):
            assert _same(run[s][0][key][3], run[s - 1][0][key][3])
    assert not _same(run[none_steps[-1] + 1][0]["p"][3], run[none_steps[-1]][0]["p"][3])
    assert not _same(first["p"][8], R.case_params(R.EDGE_NUMELS)[8])


def test_a_step_past_the_table_uses_its_last_row():
    run = _run("ema_clip", table_steps=2)
    assert len(run[-1][1].table) == 2 and run[-1][1].t == 4
    _assert_equals_host(run, "short table")
    assert not _same(run[-1][0]["p"][8], _run("ema_clip")[-1][0]["p"][8])


def test_misaligned_launches_equal_aligned_ones_and_runs_repeat():
    mis, ali = _run("ema_clip"), _run("ema_clip", misalign=False)
    _run.cache_clear()
    again = _run("ema_clip")
    for s in range(R.STEPS):
        for other in (ali, again):
            for key in ("p", "m", "v", "e"):
                assert all(_same(a, b) for a, b in zip(mis[s][0][key], other[s][0][key])), (s, key)
            assert _same(mis[s][0]["norm"], other[s][0]["norm"]) and _same(mis[s][0]["coef"], other[s][0]["coef"])


@pytest.mark.parametrize("extra", [0, 1])
def test_tensor_counts_on_both_sides_of_the_launch_boundary(extra):
    from kanvit import ops
    n = ops.optim_max_tensors() + extra
    run = _run("ema_clip", numels=tuple(R.tiny_numels(n)), none=())
    assert len(run[0][1].p) == n
    _assert_equals_host(run, f"{n} tensors")


def _lap_partials(step):
    return np.concatenate([R.sumsq_partials(g) for g in R.case_grads(R.LAP_NUMELS, step, none=())])


def test_partials_past_the_begin_kernels_first_lap_over_two_launches():
    """R.LAP_NUMELS: 343 partials, so threads 0..86 of the begin kernel add a second one; 83 tensors, so the 261-chunk tensor sits in
    the second launch behind one tiny tensor and writes its partials from offset 80 of the workspace.  Misaligned, its gradient lies
    4 bytes off the 16-byte grid (the 4-byte path over 261 chunks); aligned, it takes the 16-byte path.  Both equal the host bit for bit."""
    from kanvit import ops
    numels, big = tuple(R.LAP_NUMELS), len(R.LAP_NUMELS) - 2
    assert len(numels) > ops.optim_max_tensors() and big >= ops.optim_max_tensors() and big % 4 == 1
    assert numels[big] > 256 * R.CHUNK
    mis = _run("ema_clip", numels=numels, steps=R.LAP_STEPS, none=())
    ali = _run("ema_clip", numels=numels, misalign=False, steps=R.LAP_STEPS, none=())
    _assert_equals_host(mis, "lap, misaligned")
    _assert_equals_host(ali, "lap, aligned")
    for s in range(R.LAP_STEPS):
        parts = _lap_partials(s)
        assert len(parts) == sum((n + R.CHUNK - 1) // R.CHUNK for n in numels) > R.THREADS
        full, lap0 = R.norm_and_coef(R.total_sumsq(parts), 0.5), R.norm_and_coef(R.total_sumsq(parts[:R.THREADS]), 0.5)
        assert full[0] != lap0[0] and full[1] != lap0[1], (s, full, lap0)      # a dropped second lap cannot hide
        assert _same(mis[s][0]["norm"], np.asarray(full[0])) and _same(mis[s][0]["coef"], np.asarray(full[1])) and full[1] < 1.0
        for key in ("p", "m", "v", "e"):
            assert all(_same(a, b) for a, b in zip(mis[s][0][key], ali[s][0][key])), (s, key)
        assert _same(mis[s][0]["norm"], ali[s][0]["norm"]) and _same(mis[s][0]["coef"], ali[s][0]["coef"])
    assert not _same(mis[0][0]["p"][big], R.case_params(R.LAP_NUMELS)[big])


def test_graph_replay_past_the_begin_kernels_first_lap_equals_the_eager_step():
    numels = R.LAP_NUMELS
    opt, params, _ = _make("ema_clip", numels)
    eager = _run("ema_clip", numels=tuple(numels), steps=R.LAP_STEPS, none=())
    assert len(_lap_partials(0)) > R.THREADS
    static = []
    for k, g in enumerate(R.case_grads(numels, 0, none=())):
        buf = torch.zeros(g.size + k % 4, device=DEV)
        static.append(buf[k % 4:])
        params[k].grad = static[-1]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                      # a throw-away step, as train.py's captured step takes one
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for p, v in zip(params, R.case_params(numels)):
            p.copy_(torch.from_numpy(v).to(DEV))
        for st in opt.state.values():                   # all zeros is a fresh optimizer
            for t in st.values():
                t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for buf, g in zip(static, R.case_grads(numels, 0, none=())):
        buf.copy_(torch.from_numpy(g).to(DEV))
    graph.replay()
    got = _snapshot(opt, params)
    for key in ("p", "m", "v", "e"):
        assert all(_same(a, b) for a, b in zip(got[key], eager[0][0][key])), key
    assert got["t"] == 1 and _same(got["norm"], eager[0][0]["norm"]) and _same(got["coef"], eager[0][0]["coef"])
    _assert_equals_host([(got, eager[0][1])], "lap, replayed")       # and the host, whatever the eager run gave


def test_huge_gradients_keep_a_finite_norm():
    """1e25 squared overflows float32; the float64 sum of squares does not, and the clipped step stays finite."""
    optim = _optim()
    n, value, max_norm = R.HUGE
    p = torch.ones(n, device=DEV, requires_grad=True)
    opt = optim.KanvitAdamW([p], lr=1e-2, max_grad_norm=max_norm, total_steps=2)
    g = np.full(n, value, np.float32)
    p.grad = torch.from_numpy(g).to(DEV)
    opt.step()
    norm, coef = R.norm_and_coef(R.grads_sumsq([g]), max_norm)
    assert np.isfinite(norm) and float(opt.grad_norm) == float(norm) and float(opt.clip_coef) == float(coef)
    assert bool(torch.isfinite(p).all()) and not bool((p == 1).any())


def test_graph_replays_equal_eager_steps_and_zeroed_state_is_fresh():
    numels = R.EDGE_NUMELS
    opt, params, _ = _make("ema_clip", numels)
    eager = _run("ema_clip", none=())
    static = []
    for k, g in enumerate(R.case_grads(numels, 0, none=())):
        buf = torch.zeros(g.size + k % 4, device=DEV)
        static.append(buf[k % 4:])
        params[k].grad = static[-1]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                      # a throw-away step, as train.py's captured step takes one
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for p, v in zip(params, R.case_params(numels)):
            p.copy_(torch.from_numpy(v).to(DEV))
        for st in opt.state.values():                   # all zeros is a fresh optimizer
            for t in st.values():
                t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    with torch.no_grad():                               # the capture itself computes nothing
        assert int(opt.flat["step"]) == 0
    for s in range(3):
        for buf, g in zip(static, R.case_grads(numels, s, none=())):
            buf.copy_(torch.from_numpy(g).to(DEV))
        graph.replay()
        got = _snapshot(opt, params)
        for key in ("p", "m", "v", "e"):
            assert all(_same(a, b) for a, b in zip(got[key], eager[s][0][key])), (s, key)
        assert got["t"] == s + 1 and _same(got["norm"], eager[s][0]["norm"])


def test_state_dict_round_trip_continues_bitwise():
    numels = R.EDGE_NUMELS
    whole = _run("ema_clip")
    opt, params, _ = _make("ema_clip", numels)
    for s in range(2):
        _set_grads(params, R.case_grads(numels, s), True)
        opt.step()
    saved = copy.deepcopy(opt.state_dict())
    assert set(saved["state"]) == {"flat"} and "table" not in saved["state"]["flat"]
    opt2, params2, _ = _make("ema_clip", numels, seed=1)                 # other weights, fresh state
    with torch.no_grad():
        for q, p in zip(params2, params):
            q.copy_(p)
    opt2.load_state_dict(saved)
    for s in range(2, R.STEPS):
        _set_grads(params2, R.case_grads(numels, s), True)
        opt2.step()
        got = _snapshot(opt2, params2)
        for key in ("p", "m", "v", "e"):
            assert all(_same(a, b) for a, b in zip(got[key], whole[s][0][key])), (s, key)


def test_ema_weights_swap_in_the_debiased_average_and_restore():
    numels = R.EDGE_NUMELS
    opt, params, ref = _make("ema_clip", numels)
    with opt.ema_weights():                             # before the first step the average is the weights themselves
        assert all(torch.equal(p.detach().cpu(), torch.from_numpy(v)) for p, v in zip(params, ref.p))
    for s in range(2):
        grads = R.case_grads(numels, s)
        _set_grads(params, grads, True)
        opt.step()
        ref.step(grads)
    before = [p.detach().clone() for p in params]
    with opt.ema_weights():
        for p, e, own in zip(params, ref.e, before):
            want = e / ref.table[ref.t - 1][3]                # one division: correctly rounded or, in a fast form, within 2 ulp
            assert want.dtype == np.float32 and bool(np.all(np.abs(p.detach().cpu().numpy() - want) <= 2 * np.spacing(np.abs(want))))
            assert p.numel() == 0 or not torch.equal(p.detach(), own)
    assert all(torch.equal(p.detach(), own) for p, own in zip(params, before))
    from kanvit import KanvitError
    with pytest.raises(KanvitError, match="ema_decay"):
        with _make("noema_clip", [4])[0].ema_weights():
            pass


# ---- a real model --------------------------------------------------------------------------------------------------------------------
def _model(kind):
    from model import VisionTransformer
    torch.manual_seed(3)
    return VisionTransformer((3, 8, 8), 2, 1, 16, 2, 5, type=kind).to(DEV)


def _backward(model, step):
    g = torch.Generator(device=DEV).manual_seed(100 + step)
    x = torch.randn(4, 3, 8, 8, device=DEV, generator=g)
    y = torch.randint(0, 5, (4,), device=DEV, generator=g)
    model.zero_grad(set_to_none=True)
    torch.nn.functional.cross_entropy(model(x), y).backward()


@pytest.mark.parametrize("kind", ["cheby", "efficientkan", "fast"])
def test_model_steps_equal_the_restatement_of_their_own_inputs(kind):
    """Three steps of a one-block model: after each, every parameter, moment and EMA equals the restatement applied to what that step
    read -- its own (p, g, m, v, e) and the norm of its own gradients; frozen parameters are untouched and own no state."""
    optim = _optim()
    model = _model(kind)
    frozen = [p for p in model.parameters() if not p.requires_grad]
    last = list(model.parameters())[-1]
    last.requires_grad_(False)                          # one more, frozen by hand (the head's bias)
    frozen.append(last)
    kept = [p.detach().clone() for p in frozen]
    kw = dict(total_steps=3, lr=1e-2, betas=(0.9, 0.999), weight_decay=0.05, warmup_steps=1, schedule="cosine", min_lr=1e-4, ema_decay=0.9)
    opt = optim.KanvitAdamW(model.parameters(), eps=1e-8, max_grad_norm=0.05, **kw)
    params = opt.param_groups[0]["params"]
    assert len(params) == sum(p.requires_grad for p in model.parameters()) and all(p.requires_grad for p in params)
    from tests.test_optim_cpu import undecayed_by_name
    names = {id(p): name for name, p in model.named_parameters()}
    decay = [not undecayed_by_name(names[id(p)]) for p in params]                    # by name, not by the filter's own rule
    assert [opt.decayed(p) for p in params] == decay and any(decay) and not all(decay)
    assert not opt.decayed(model.v_class) and opt.decayed(model.blocks[0].ff[0].weight) and not opt.decayed(model.blocks[0].norm1.weight)
    table, consts = optim.step_table(**kw), optim.rounded_constants(kw["betas"], 1e-8, 0.9)
    for s in range(3):
        _backward(model, s)
        assert all(p.grad is not None for p in params)
        was = [[t.detach().cpu().numpy().copy() for t in (p, p.grad, *opt.moments(p), opt.ema(p))] for p in params]
        opt.step()
        orders = R.coefficient_in_three_orders([w[1] for w in was], 0.05)             # sequential, pairwise, the device's order
        assert orders[0] == orders[1] == orders[2] and orders[2][1] < 1.0, (kind, s, orders)
        norm, coef = orders[2]
        assert _same(opt.grad_norm.cpu().numpy(), np.asarray(norm)) and _same(opt.clip_coef.cpu().numpy(), np.asarray(coef))
        for k, (p, (p0, g, m0, v0, e0)) in enumerate(zip(params, was)):
            want = R.adamw_f32(p0, g, m0, v0, e0, table[s], consts, coef, decay=decay[k])
            got = (p.detach(), *opt.moments(p), opt.ema(p))
            for key, a, b in zip("pmve", got, want):
                assert _same(a.cpu().numpy(), b.reshape(a.shape)), f"{kind}: step {s}, parameter {k} {tuple(p.shape)}, {key}"
        assert all(torch.equal(p.detach(), k) for p, k in zip(frozen, kept))


def test_gradients_in_reducer_buckets_give_the_same_bits():
    """GradReducer without a process group: finish() packs the gradients into its buckets and re-points every .grad at a view at an
    arbitrary 4-byte offset.  The step on those equals the step on the gradients where autograd left them."""
    from kanvit import dp
    optim = _optim()
    a, b = _model("cheby"), _model("cheby")
    kw = dict(total_steps=3, lr=1e-2, weight_decay=0.05, warmup_steps=1, schedule="cosine", max_grad_norm=0.05, ema_decay=0.9)
    oa, ob = optim.KanvitAdamW(a.parameters(), **kw), optim.KanvitAdamW(b.parameters(), **kw)
    reducer = dp.GradReducer(b.parameters())
    for s in range(3):
        _backward(a, s)
        reducer.zero_grad()
        for pa, pb in zip(a.parameters(), b.parameters()):
            pb.grad = None if pa.grad is None else pa.grad.clone()
        reducer.finish()
        views = {pb.grad.data_ptr() % 16 for pb in b.parameters() if pb.requires_grad}
        assert all(pb.grad._base is not None for pb in b.parameters() if pb.requires_grad)
        assert views - {0}, "no gradient view off a 16-byte boundary: the case does not test what it names"
        orders = R.coefficient_in_three_orders([pb.grad.cpu().numpy() for pb in b.parameters() if pb.requires_grad], 0.05)
        assert orders[0] == orders[1] == orders[2], (s, orders)
        oa.step()
        ob.step()
        assert _same(ob.grad_norm.cpu().numpy(), np.asarray(orders[2][0])) and _same(ob.clip_coef.cpu().numpy(), np.asarray(orders[2][1]))
        assert all(torch.equal(pa.detach(), pb.detach()) for pa, pb in zip(a.parameters(), b.parameters()))
        assert torch.equal(oa.flat["exp_avg_sq"], ob.flat["exp_avg_sq"]) and torch.equal(oa.flat["ema"], ob.flat["ema"])
        assert torch.equal(oa.flat["norm_coef"], ob.flat["norm_coef"])
