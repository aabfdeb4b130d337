"""Stochastic depth on the GPU: kanvit_depth_scales against its Python restatement (bitwise; the counter walk, also from a captured
graph), the scaled residual add + LayerNorm (kanvit_addln_sd_*) against fp64 torch and bitwise against the unscaled kernel, the bf16
boundary, and VisionTransformer.set_drop_path against the same model with the scale applied by a torch multiply in front of the
unscaled kernel, through train.py's captured step."""
import copy
import functools

import pytest
import torch

from tests._util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- depth_scales ---------------------------------------------------------------------------------------------------------------------
def _keeps(n):
    return [1.0 if j % 7 == 0 else 1.0 - 0.5 * (j + 1) / (n + 1) for j in range(n)]      # 1.0 among them: always kept, scale 1


@pytest.mark.parametrize("B,n_branch", [(1, 1), (5, 3), (128, 24), (300, 64)])
def test_depth_scales_equal_the_restatement_bitwise(B, n_branch):
    from kanvit import ops
    keep, seed, c = _keeps(n_branch), 12345 + B, 7
    counter = torch.full((1,), c, dtype=torch.int64, device=DEV)
    first = ops.depth_scales(B, keep, seed, counter)
    second = ops.depth_scales(B, keep, seed, counter, out=torch.empty(n_branch, B, device=DEV))
    assert first.dtype == torch.float32 and tuple(first.shape) == (n_branch, B)
    assert torch.equal(first.cpu(), ops.depth_keep(B, keep, seed, c))
    assert torch.equal(second.cpu(), ops.depth_keep(B, keep, seed, c + 1))
    assert int(counter) == c + 2
    assert bool((first[0] == 1.0).all())                             # keep = 1


def test_depth_scales_replayed_from_a_graph_walk_the_counter():
    from kanvit import ops
    B, keep, seed, c = 128, [0.9, 0.5, 0.75], 99, 41
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.empty(3, B, device=DEV)
    ops.depth_scales(B, keep, seed, counter, out=out)                # loads the library outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.depth_scales(B, keep, seed, counter, out=out)
    counter.fill_(c)
    for k in range(3):
        graph.replay()
        assert torch.equal(out.cpu(), ops.depth_keep(B, keep, seed, c + k)), k
    assert int(counter) == c + 3


# ---- add_layernorm(row_scale=...) ------------------------------------------------------------------------------------------------------
SHAPES = [(5, 3, 4), (3, 17, 64), (2, 197, 768), (4, 50, 260), (3, 11, 1024), (9, 500, 8)]
INV09 = float(torch.tensor(1.0) / torch.tensor(0.9))


def _scales(B):
    return torch.tensor([(0.0, INV09, 1.0)[b % 3] for b in range(B)], device=DEV)      # mixes 0, 1 / 0.9 and 1; sample 0 is dropped


def _norm(D):
    norm = torch.nn.LayerNorm(D).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(D) * 0.5 + 1.0)
        norm.bias.copy_(torch.randn(D) * 0.3)
    return norm


def _run(x, delta, norm, ws, wy, **kw):
    """s, y and the gradients (x, gamma, beta, delta) of add_layernorm on fresh leaves."""
    from kanvit.ops import add_layernorm
    x, delta = x.detach().clone().requires_grad_(True), delta.detach().clone().requires_grad_(True)
    norm.zero_grad()
    s, y = add_layernorm(x, delta, norm, **kw)
    torch.autograd.backward([s, y], [ws, wy])
    return s.detach(), y.detach(), x.grad, norm.weight.grad.clone(), norm.bias.grad.clone(), delta.grad


@pytest.mark.parametrize("B,N,D", SHAPES)
def test_scaled_add_layernorm_matches_fp64_torch(B, N, D):
    torch.manual_seed(B * 7 + N + D)
    norm = _norm(D)
    x = torch.randn(B, N, D, device=DEV) * 2.0 + 0.7
    delta = torch.randn(B, N, D, device=DEV)
    ws, wy = torch.randn(B, N, D, device=DEV), torch.randn(B, N, D, device=DEV)
    sc = _scales(B)
    got = _run(x, delta, norm, ws, wy, row_scale=sc)

    n64 = torch.nn.LayerNorm(D, eps=norm.eps).double().to(DEV)
    n64.load_state_dict({k: v.double() for k, v in norm.state_dict().items()})
    x64, d64 = x.double().requires_grad_(True), delta.double().requires_grad_(True)
    s64 = x64 + sc.double()[:, None, None] * d64
    y64 = n64(s64)
    ((s64 * ws.double()).sum() + (y64 * wy.double()).sum()).backward()
    want = [s64.detach(), y64.detach(), x64.grad, n64.weight.grad, n64.bias.grad, d64.grad]
    for name, g, w in zip(("s", "y", "dx", "dgamma", "dbeta", "ddelta"), got, want):
        scale = max(1.0, float(w.abs().max()))
        err = float((g.double() - w).abs().max())
        print(f"{(B, N, D)} {name}: {err:.2e} (bound {2e-5 * scale:.2e})")
        assert err < 2e-5 * scale, name

    s, dd = got[0], got[5]
    assert torch.equal(s, x + sc[:, None, None] * delta)             # two fp32 roundings, as torch computes it
    dropped = sc == 0
    assert bool(dropped.any())
    assert torch.equal(s[dropped], x[dropped])
    assert bool((dd[dropped] == 0).all())
    # the 2-D form with explicit rows per sample is the same launch
    got2 = _run(x.view(B * N, D), delta.view(B * N, D), norm, ws.view(B * N, D), wy.view(B * N, D), row_scale=sc, rows_per_sample=N)
    for a, b in zip(got, got2):
        assert torch.equal(a.reshape(b.shape), b)


@pytest.mark.parametrize("B,N,D", SHAPES)
def test_all_scales_one_is_the_unscaled_kernel_bitwise(B, N, D):
    torch.manual_seed(B + N * 3 + D)
    norm = _norm(D)
    x = torch.randn(B, N, D, device=DEV) * 2.0 + 0.7
    delta = torch.randn(B, N, D, device=DEV)
    ws, wy = torch.randn(B, N, D, device=DEV), torch.randn(B, N, D, device=DEV)
    s, y, dx, dg, db, dd = _run(x, delta, norm, ws, wy, row_scale=torch.ones(B, device=DEV))
    s0, y0, dx0, dg0, db0, dd0 = _run(x, delta, norm, ws, wy)
    for a, b in ((s, s0), (y, y0), (dx, dx0), (dg, dg0), (db, db0), (dd, dx), (dd0, dx0)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,N,D", [(7, 1, 8), (3, 43, 64), (2, 500, 384), (2, 1025, 768), (5, 1, 260)])
@pytest.mark.parametrize("delta_bf16,y_bf16", [(True, True), (True, False), (False, True)])
def test_bf16_tensors_at_the_boundary(B, N, D, delta_bf16, y_bf16):
    """As tests/test_addln_gpu.py's test of the same name: bf16 delta and / or bf16 y (and the bf16 gradient arriving on it) give, bit
    for bit, what the fp32 scaled kernel gives on the widened values; y is its result rounded to bf16, ddelta is round_bf16(scale * dx)."""
    torch.manual_seed(B + N + D)
    norm = _norm(D)
    x = torch.randn(B, N, D, device=DEV) * 2.0 + 0.7
    delta = torch.randn(B, N, D, device=DEV)
    delta = delta.bfloat16() if delta_bf16 else delta
    ws, wy = torch.randn(B, N, D, device=DEV), torch.randn(B, N, D, device=DEV)
    wy = wy.bfloat16() if y_bf16 else wy
    sc = _scales(B)
    s, y, dx, dg, db, dd = _run(x, delta, norm, ws, wy, y_bf16=y_bf16, row_scale=sc)
    assert y.dtype == (torch.bfloat16 if y_bf16 else torch.float32) and s.dtype == torch.float32 and dd.dtype == delta.dtype
    s2, y2, dx2, dg2, db2, dd2 = _run(x, delta.float(), norm, ws, wy.float(), row_scale=sc)
    assert torch.equal(s, s2)
    assert torch.equal(y, y2.bfloat16()) if y_bf16 else torch.equal(y, y2)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    assert torch.equal(dd2, sc[:, None, None] * dx2)
    assert torch.equal(dd, dd2.bfloat16()) if delta_bf16 else torch.equal(dd, dd2)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def _vit(kind, d=64, heads=4, seed=11):
    from model import VisionTransformer
    torch.manual_seed(seed)
    return VisionTransformer((3, 32, 32), 4, 3, d, heads, 10, type=kind).to(DEV)


def _batch(B=6):
    g = torch.Generator().manual_seed(5)
    return torch.randn(B, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 10, (B,), generator=g).to(DEV)


def _pass(m, x, labels):
    m.zero_grad()
    logits = m(x)
    torch.nn.functional.cross_entropy(logits, labels).backward()
    return logits.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


MODELS = [("cheby", 64, 4), ("vanilla", 64, 4), ("cheby", 384, 6)]      # two small geometries (the fallback route), one that takes the class-token tail


@pytest.mark.parametrize("kind,d,heads", MODELS)
def test_model_against_a_torch_multiply_in_front_of_the_unscaled_kernel(kind, d, heads, monkeypatch):
    import model
    from kanvit import ops
    from kanvit.dense import ff_small_supported
    assert ff_small_supported(d, 4 * d) == (d == 64)
    m = _vit(kind, d, heads).train()
    x, labels = _batch()
    m.set_drop_path(0.5, seed=3)
    logits, grads = _pass(m, x, labels)
    assert int(m.drop_path_counter) == 1

    # the same masks (counter back at 0), the scale applied by torch, the kernel that knows nothing of it
    table = ops.depth_keep(x.shape[0], m._drop_path[0], 3, 0).to(DEV)
    assert 0 < int((table == 0).sum()) < table.numel()
    used = []

    def stock(x_, d_, n_, y_bf16=False, row_scale=None):
        if row_scale is not None:
            used.append(row_scale)
            d_ = d_ * row_scale[:, None, None]
        return ops.add_layernorm(x_, d_, n_, y_bf16)

    monkeypatch.setattr(model, "add_layernorm", stock)
    monkeypatch.setattr(model.ops, "depth_scales", lambda B, keep, seed, counter, out=None: table)
    logits0, grads0 = _pass(m, x, labels)
    assert len(used) == (4 if d == 384 else 5)      # 3 blocks: 5 full-size adds; the tail's LN2 add and the last one take class rows
    print(f"{kind} d={d}: logits {rel_err(logits, logits0):.2e}, worst gradient {max(rel_err(grads[k], grads0[k]) for k in grads):.2e}")
    assert rel_err(logits, logits0) <= 1e-5
    assert set(grads) == set(grads0) and len(grads) > 10
    for k in grads:
        assert rel_err(grads[k], grads0[k]) <= 1e-5, (kind, k, rel_err(grads[k], grads0[k]))


@pytest.mark.parametrize("kind,d,heads", MODELS[:1] + MODELS[2:])
def test_eval_ignores_it_and_seeds_decide_the_masks(kind, d, heads):
    x, _ = _batch()
    plain = _vit(kind, d, heads)
    a, b, c = (copy.deepcopy(plain) for _ in range(3))
    a.set_drop_path(0.5, seed=3), b.set_drop_path(0.5, seed=3), c.set_drop_path(0.5, seed=4)
    with torch.no_grad():
        assert torch.equal(a.eval()(x), plain.eval()(x))
        assert int(a.drop_path_counter) == 0
        a.train(), b.train(), c.train(), plain.train()
        steps = [(a(x), b(x), c(x)) for _ in range(3)]
        assert all(torch.equal(ya, yb) for ya, yb, _ in steps)
        assert not any(torch.equal(ya, yc) for ya, _, yc in steps)
        assert not torch.equal(steps[0][0], steps[1][0])                 # the counter moves the masks from step to step
        assert not torch.equal(steps[0][0], plain(x))
        a.set_drop_path(0.0)
        assert torch.equal(a(x), plain(x))


def test_regularised_forward_keeps_working():
    x, _ = _batch()
    m = _vit("cheby").train()
    m.set_drop_path(0.5, seed=3)
    with torch.no_grad():
        logits, reg = m(x, return_regularization=True)
        m.drop_path_counter.zero_()
        assert torch.equal(logits, m(x)) and bool(torch.isfinite(reg))


def test_graphed_train_step_equals_the_eager_one(tmp_path):
    """train.py --graph: the throw-away step in front of the capture must not use up a mask (_GraphedStep puts the counter back)."""
    import train
    flags = ["--model-type", "cheby", "--epochs", "1", "--steps-per-epoch", "3", "--synthetic", "--no-step-metrics", "--n-blocks", "2",
             "--batch-size", "16", "--out-d", "10", "--drop-path", "0.5", "--seed", "7"]
    eager = train.main(train.parse([*flags, "--log-dir", str(tmp_path / "e")]))
    graphed = train.main(train.parse([*flags, "--graph", "--log-dir", str(tmp_path / "g")]))
    plain = train.main(train.parse([*flags[:-4], "--seed", "7", "--log-dir", str(tmp_path / "p")]))
    print("eager", eager["losses"], "graphed", graphed["losses"], "without", plain["losses"])
    assert len(eager["losses"]) == 3 and eager["losses"] == graphed["losses"]
    assert int(graphed["model"].drop_path_counter) == 3 and int(eager["model"].drop_path_counter) == 3
    assert eager["losses"] != plain["losses"]
