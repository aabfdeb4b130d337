"""GPU tests of grid extension: KANLinear.extend_grid as a fused Gram-matrix spline fit onto a basis of another size
(kanvit_bspline_regrid_*, csrc/kan_bspline_refit.hip) and everything built on it: ops.bspline_regrid, MSA.extend_grid (one grouped
launch per fit), VisionTransformer.extend_grid, checkpoints across grid sizes and train.py --grid-extend.

There is no reference implementation of this feature; the yardstick is the float64 restatement of tests/_extend_grid_ref.py
(which tests/test_extend_grid_cpu.py ties to the update_grid restatement at an unchanged size).  Bounds, the project's own from
tests/test_update_grid_gpu.py: knots within 1e-6 (1 + |g|); spline_weight within 1e-4 normwise per layer; the layer's forward on x
within 1e-4 normwise against the float64 forward with the restated knots and weights.  Every non-degenerate case first asserts,
from the restatement, that every feature's smallest Cholesky pivot ratio is at least 10 tau (tau = 1e-5, the solve kernel's
degeneracy threshold): a condition on the inputs.

The comparison is against the float64 FIT, not against the layer's output before the call: quantile knots do not nest the old
ones, so the new layer is the least-squares fit on the samples, not the identical function (fit residuals of 0.07 to 0.6
normwise on these inputs, most of it from samples outside the old grid, where the old spline is cut to zero)."""
import copy

import pytest
import torch

from tests import _extend_grid_ref as eg
from tests import _update_grid_ref as ug

pytestmark = pytest.mark.gpu

GRID_BOUND, WEIGHT_BOUND, FORWARD_BOUND = 1e-6, 1e-4, 1e-4


def cpu_state(layer):
    return {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}


def make_layer(i, o, grid_size=5, order=3, seed=0, standalone=True):
    from models.effkan import KANLinear
    torch.manual_seed(700 + seed)
    layer = KANLinear(i, o, grid_size=grid_size, spline_order=order, enable_standalone_scale_spline=standalone)
    with torch.no_grad():
        layer.spline_weight.uniform_(-0.5, 0.5)
    return layer


def check_against(tag, layer, x, knots, weight, y, features=None):
    """The three bounds for a GPU layer after its extension; `features`: the feature subset the knots and weights are compared on
    (the forward is always the whole layer's)."""
    g, w = layer.grid.detach().cpu(), layer.spline_weight.detach().cpu()
    assert tuple(g.shape) == tuple(knots.shape) and tuple(w.shape) == tuple(weight.shape)
    if features is not None:
        g, knots, w, weight = g[features], knots[features], w[:, features], weight[:, features]
    ge, we, fe = ug.grid_err(g, knots), ug.rel(w, weight), ug.rel(layer(x).detach().cpu(), y)
    print(f"{tag}: grid err {ge:.3e} (bound {GRID_BOUND:.0e})  weight err {we:.3e} (bound {WEIGHT_BOUND:.0e})  "
          f"forward err {fe:.3e} (bound {FORWARD_BOUND:.0e})")
    assert ge <= GRID_BOUND, (tag, ge)
    assert we <= WEIGHT_BOUND, (tag, we)
    assert fe <= FORWARD_BOUND, (tag, fe)
    assert torch.isfinite(layer.grid).all() and torch.isfinite(layer.spline_weight).all()


def restated_case(tag, layer, x, new_grid_size, xg=None):
    """extend_grid(x, new_grid_size) of `layer` on the GPU against the float64 restatement on the layer's state before the call."""
    sd = cpu_state(layer)
    order = layer.spline_order
    knots, weight, live, piv, _ = eg.extend(x, sd, new_grid_size, order, layer.grid_eps)
    print(f"{tag}: smallest pivot ratio {float(piv.min()):.3e}, float64 fit residual {eg.fit_residual(x, sd, knots, weight, order):.3f}")
    assert float(piv.min()) >= 10 * eg.TAU and bool(live.all()), (tag, piv)                 # a condition on the inputs
    layer = layer.cuda()
    xg = x.cuda() if xg is None else xg
    fell_back = layer.extend_grid(xg, new_grid_size)
    assert fell_back.dim() == 0 and fell_back.is_cuda and int(fell_back) == 0
    assert layer.grid_size == new_grid_size
    check_against(tag, layer, xg, knots, weight, ug.forward64(x, sd, knots, weight, order))
    return layer


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement: every pair of slot counts of the Gram kernel, every order, one and several bands
# ---------------------------------------------------------------------------------------------------------------------
CASES = {  # name: (M, I, O, old grid, new grid, order)
    "old 8 slots, new 24, uniform old knots": (512, 8, 8, 5, 10, 3),
    "three ragged bands, ragged I, strided x": (1100, 17, 5, 5, 10, 3),
    "both 24 slots (nb 13 -> 23), O > solve threads": (400, 6, 70, 10, 20, 3),
    "coarsening: old 24 slots, new 8": (300, 6, 7, 10, 5, 3),
    "both 8 slots": (257, 8, 8, 5, 3, 3),
    "order 2": (300, 6, 7, 8, 12, 2),
    "order 1": (300, 6, 7, 8, 16, 1),
    "one band": (64, 8, 8, 5, 10, 3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_restated_cases(name):
    from kanvit import _lib
    m, i, o, g_old, g_new, order = CASES[name]
    n = list(CASES).index(name) + 1
    layer = make_layer(i, o, grid_size=g_old, order=order, seed=n)
    torch.manual_seed(n)
    x = torch.randn(m, i)
    xg = None
    if "strided" in name:                                    # a column slice of a wider matrix, read in place
        wide = torch.zeros(m, i + 8)
        wide[:, 3:3 + i] = x
        xg = wide.cuda()[:, 3:3 + i]
        assert xg.stride(0) == i + 8 and not xg.is_contiguous()
    if order == 3:                                           # the old basis runs the closed form for uniform knots
        assert layer.cuda().kan_cfg().flags & _lib.FLAG_UNIFORM_KNOTS
        layer = layer.cpu()
    restated_case(f"{(m, i, o)} grid {g_old} -> {g_new} order {order} [{name}]", layer, x, g_new, xg)


def test_non_uniform_old_knots():
    """update_grid first, then extend_grid: the old basis of the extension runs the Cox-de Boor path.  The restatement is chained
    the same way (restated_case of the second step starts from the GPU layer's state after the first)."""
    from kanvit import _lib
    layer = make_layer(8, 8, seed=20).cuda()
    torch.manual_seed(20)
    x1, x2 = torch.randn(512, 8), 0.8 * torch.randn(512, 8) + 0.1
    sd = cpu_state(layer)
    knots, weight = ug.refit(x1, sd, 5, 3, layer.grid_eps)
    assert float(ug.pivot_ratios(x1, knots, 3).min()) >= 10 * ug.TAU
    layer.update_grid(x1.cuda())
    assert ug.grid_err(layer.grid, knots) <= GRID_BOUND and ug.rel(layer.spline_weight, weight) <= WEIGHT_BOUND
    assert not layer.kan_cfg().flags & _lib.FLAG_UNIFORM_KNOTS
    restated_case("(512, 8, 8) update_grid, then 5 -> 10", layer.cpu(), x2, 10)


def test_without_the_standalone_scaler():
    torch.manual_seed(21)
    layer = make_layer(8, 8, seed=21, standalone=False)
    assert not hasattr(layer, "spline_scaler")
    restated_case("(300, 8, 8) 5 -> 10, no spline_scaler", layer, torch.randn(300, 8), 10)


def test_same_size_agrees_with_update_grid():
    torch.manual_seed(22)
    a = make_layer(8, 8, seed=22).cuda()
    b = copy.deepcopy(a)
    x = torch.randn(512, 8).cuda()
    a.extend_grid(x, 5)
    b.update_grid(x)
    ge, we = ug.grid_err(a.grid, b.grid), ug.rel(a.spline_weight, b.spline_weight)
    fe = ug.rel(a(x), b(x))
    print(f"same size: grid err {ge:.3e}  weight err {we:.3e}  forward err {fe:.3e}")
    assert ge <= GRID_BOUND and we <= WEIGHT_BOUND and fe <= FORWARD_BOUND


def test_shapes_and_bookkeeping_after_the_call():
    from kanvit import _lib
    torch.manual_seed(23)
    layer = make_layer(8, 6, seed=23).cuda()
    x = torch.randn(300, 8).cuda()
    layer(x)
    assert layer.kan_cfg().flags & _lib.FLAG_UNIFORM_KNOTS
    old_weight, old_grid = layer.spline_weight, layer.grid
    scaler, base = layer.spline_scaler.detach().clone(), layer.base_weight.detach().clone()
    layer.extend_grid(x, 10)
    assert layer.grid_size == 10
    assert tuple(layer.grid.shape) == (8, 17) and layer.grid is not old_grid and "grid" in dict(layer.named_buffers())
    assert isinstance(layer.spline_weight, torch.nn.Parameter) and layer.spline_weight is not old_weight
    assert tuple(layer.spline_weight.shape) == (6, 8, 13) and layer.spline_weight.requires_grad and layer.spline_weight.is_leaf
    assert dict(layer.named_parameters())["spline_weight"] is layer.spline_weight
    assert torch.equal(layer.spline_scaler, scaler) and torch.equal(layer.base_weight, base)          # the scaler quirk is kept
    cfg = layer.kan_cfg()                                    # the replaced buffer is a new one to the grid-facts cache
    assert cfg.G == 13 and not cfg.flags & _lib.FLAG_UNIFORM_KNOTS
    assert tuple(layer.b_splines(x).shape) == (300, 8, 13)
    w, bp, _ = layer.kan_pack()
    assert tuple(w.shape) == (8 * 14, 6) and bp.numel() == 8 * 17
    xin = x.clone().requires_grad_()
    y = layer(xin)
    y.square().sum().backward()
    assert tuple(y.shape) == (300, 6) and torch.isfinite(y).all()
    assert tuple(layer.spline_weight.grad.shape) == (6, 8, 13)
    for p in list(layer.parameters()) + [xin]:
        assert p.grad is not None and torch.isfinite(p.grad).all()
    a = layer.edge_activation_l1(x)
    assert tuple(a.shape) == (6, 8) and torch.isfinite(a).all() and bool((a > 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# degenerate features stay defined: they are fitted on the fallback samples
# ---------------------------------------------------------------------------------------------------------------------
def test_constant_column_takes_the_fallback_fit():
    layer = make_layer(6, 4, seed=24)
    torch.manual_seed(24)
    x = torch.randn(200, 6)
    x[:, 2] = 0.3
    sd = cpu_state(layer)
    knots, weight, live, piv, piv_fb = eg.extend(x, sd, 10, 3, layer.grid_eps)
    good = [0, 1, 3, 4, 5]
    print("pivot ratios on x", piv.tolist(), "on the fallback samples", piv_fb.tolist())
    assert float(piv[good].min()) >= 10 * eg.TAU and float(piv[2]) <= 0.1 * eg.TAU and float(piv_fb.min()) >= 10 * eg.TAU
    assert live.tolist() == [True, True, False, True, True, True]
    layer = layer.cuda()
    fell_back = layer.extend_grid(x.cuda(), 10)
    assert fell_back.dim() == 0 and fell_back.is_cuda and int(fell_back) == 1
    y = ug.forward64(x, sd, knots, weight, 3)
    check_against("(200, 6, 4) 5 -> 10, live features", layer, x.cuda(), knots, weight, y, features=good)
    check_against("(200, 6, 4) 5 -> 10, constant column 2 on the fallback samples", layer, x.cuda(), knots, weight, y, features=[2])


def test_too_few_rows_every_feature_takes_the_fallback_fit():
    from models.effkan import KANLinear
    layer = make_layer(3, 3, seed=25)
    torch.manual_seed(25)
    x = torch.randn(4, 3)
    sd = cpu_state(layer)
    knots, weight, live, piv, piv_fb = eg.extend(x, sd, 10, 3, layer.grid_eps)
    assert not live.any() and float(piv.max()) <= 0.1 * eg.TAU and float(piv_fb.min()) >= 10 * eg.TAU
    layer = layer.cuda()
    fell_back = layer.extend_grid(x.cuda(), 10)
    assert int(fell_back) == 3
    # the layer is now the fit on the fallback samples: compare its forward on them (x itself lies partly outside that span)
    rows = KANLinear.fallback_samples(sd["grid"], 3, 256)
    check_against("(4, 3, 3) 5 -> 10, all on the fallback samples", layer, rows.cuda(), knots, weight, ug.forward64(rows, sd, knots, weight, 3))
    for v in layer.state_dict().values():
        assert torch.isfinite(v).all()
    assert torch.isfinite(layer(x.cuda())).all()


def test_no_rows_flags_everything_and_writes_zeros():
    from dataclasses import replace
    from kanvit import ops
    layer = make_layer(5, 4, seed=26).cuda()
    cfg = replace(layer.kan_cfg(), has_base=0, base_act=0, G=13)
    w_old = layer.scaled_spline_weight.detach().permute(1, 2, 0).reshape(1, -1, 4)
    new = torch.linspace(-1.6, 1.6, 17, device="cuda").expand(1, 5, -1).contiguous()
    w_new, ok = ops.bspline_regrid(torch.zeros(0, 5, device="cuda"), w_old, cfg, 8, layer.grid.reshape(1, -1), new)
    assert ok.dtype == torch.bool and tuple(ok.shape) == (1, 5) and not ok.any()
    assert tuple(w_new.shape) == (1, 5 * 13, 4) and not w_new.any()


def test_ops_validates_both_packings_and_both_knot_tables_by_name():
    from dataclasses import replace
    from kanvit import ops
    layer = make_layer(5, 4, seed=27).cuda()
    cfg = replace(layer.kan_cfg(), has_base=0, base_act=0, G=13)
    w_old = layer.scaled_spline_weight.detach().permute(1, 2, 0).reshape(1, -1, 4)
    old = layer.grid.reshape(1, -1)
    new = torch.linspace(-1.6, 1.6, 17, device="cuda").expand(1, 5, -1).contiguous()
    x = torch.randn(32, 5, device="cuda")
    with pytest.raises(ops.KanvitError, match="old packed weight"):
        ops.bspline_regrid(x, w_old, cfg, 9, old, new)
    with pytest.raises(ops.KanvitError, match="old knot table"):
        ops.bspline_regrid(x, w_old, cfg, 8, old[:, :-1], new)
    with pytest.raises(ops.KanvitError, match="new knot table"):
        ops.bspline_regrid(x, w_old, cfg, 8, old, new[:, :, :-1])
    with pytest.raises(ops.KanvitError, match="columns"):
        ops.bspline_regrid(x[:, :4], w_old, cfg, 8, old, new)
    with pytest.raises(NotImplementedError, match="cheby"):
        ops.bspline_regrid(x, w_old, ops.LayerCfg(family=ops.CHEBY, I=5, O=4, G=5), 8, old, new)
    with pytest.raises(ops.KanvitError, match="new nb=25"):
        ops.bspline_regrid(x, w_old, replace(cfg, G=25), 8, old, torch.zeros(1, 5, 29, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# determinism, autocast, grouping
# ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal_and_autocast_changes_nothing():
    torch.manual_seed(28)
    proto = make_layer(17, 5, seed=28).cuda()
    x = torch.randn(1100, 17).cuda()
    x[:, 4] = -0.2                                           # one feature on the fallback path
    runs = []
    for mode in ("plain", "plain", "autocast"):
        layer = copy.deepcopy(proto)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "autocast"):
            assert int(layer.extend_grid(x, 10)) == 1
        runs.append(layer)
    for other in runs[1:]:
        assert torch.equal(runs[0].grid, other.grid) and torch.equal(runs[0].spline_weight, other.spline_weight)
    assert tuple(runs[0].spline_weight.shape) == (5, 17, 13)


def test_msa_grouped_launch_equals_every_layer_alone(monkeypatch):
    from attention import MSA
    from kanvit import ops
    H, dh = 2, 16
    torch.manual_seed(29)
    msa = MSA(32, n_heads=H, type="efficientkan")
    with torch.no_grad():
        for n, p in msa.named_parameters():
            if "spline_weight" in n:
                p.uniform_(-0.5, 0.5)
    msa = msa.cuda()
    x = torch.randn(18, 17, 32).cuda()                       # 306 rows
    x[..., 5] = 0.1                                          # a feature of head 0 on the fallback path
    alone = copy.deepcopy(msa)
    calls = []
    real = ops.bspline_regrid

    def recorder(x2d, w, cfg, old_g, old, new):
        calls.append((cfg, old_g, x2d.shape[0]))
        return real(x2d, w, cfg, old_g, old, new)

    monkeypatch.setattr(ops, "bspline_regrid", recorder)
    fell_back = msa.extend_grid(x, 10)
    # ONE grouped launch over the 3*H layers for the fit on x, one for the fit on the 256 fallback samples
    assert [(c.groups, c.x_group_mod, c.G, g, m) for c, g, m in calls] == [(3 * H, H, 13, 8, 306), (3 * H, H, 13, 8, 256)]
    assert int(fell_back) == 1
    calls.clear()
    rows = x.reshape(-1, 32)
    layers = list(msa.q_mappings) + list(msa.k_mappings) + list(msa.v_mappings)
    singles = list(alone.q_mappings) + list(alone.k_mappings) + list(alone.v_mappings)
    for gi, (grouped, single) in enumerate(zip(layers, singles)):
        h = gi % H
        assert int(single.extend_grid(rows[:, h * dh:(h + 1) * dh], 10)) == (1 if h == 0 else 0)
        assert grouped.grid_size == 10 and tuple(grouped.spline_weight.shape) == (dh, dh, 13)
        assert torch.equal(grouped.grid, single.grid), gi
        assert torch.equal(grouped.spline_weight, single.spline_weight), gi
        assert torch.equal(grouped.spline_scaler, single.spline_scaler) and torch.equal(grouped.base_weight, single.base_weight)
    for h in range(H):                                       # q, k and v of a head share their knots
        assert torch.equal(msa.q_mappings[h].grid, msa.k_mappings[h].grid) and torch.equal(msa.q_mappings[h].grid, msa.v_mappings[h].grid)
    assert not torch.equal(msa.q_mappings[0].grid, msa.q_mappings[1].grid)
    y = msa(x)                                               # the grouped forward runs on the extended layers
    assert torch.isfinite(y).all()
    assert torch.isfinite(msa.edge_activation_l1(x)).all()


def test_msa_refuses_other_types_by_name():
    from attention import MSA
    msa = MSA(32, n_heads=2, type="cheby").cuda()
    with pytest.raises(NotImplementedError, match="cheby"):
        msa.extend_grid(torch.randn(2, 5, 32, device="cuda"), 10)


# ---------------------------------------------------------------------------------------------------------------------
# VisionTransformer.extend_grid, checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def _vit(kind, seed=30):
    from model import VisionTransformer
    torch.manual_seed(seed)
    return VisionTransformer((3, 32, 32), n_patches=4, n_blocks=2, d_hidden=64, n_heads=8, type=kind).cuda()


def test_vision_transformer_extends_every_kanlinear_and_its_checkpoint_loads_into_a_default_model():
    from models.effkan import KANLinear
    model = _vit("efficientkan")
    torch.manual_seed(31)
    images, labels = torch.randn(4, 3, 32, 32).cuda(), torch.randint(0, 10, (4,)).cuda()
    with torch.no_grad():
        model(images)                                        # the model has run: the fused-embedding decision is cached
    assert model._fused_embed is not None
    names = [n for n, _ in model.named_parameters()]
    fell_back = model.extend_grid(images, 10)
    assert fell_back.dim() == 0 and fell_back.is_cuda
    assert model._fused_embed is None
    assert [n for n, _ in model.named_parameters()] == names             # the replaced parameters keep their places
    layers = [m for m in model.modules() if isinstance(m, KANLinear)]
    assert len(layers) == 1 + 2 * 3 * 8
    for m in layers:
        assert m.grid_size == 10 and m.grid.shape[1] == 17 and m.spline_weight.shape[2] == 13
    logits = model(images)
    torch.nn.functional.cross_entropy(logits, labels).backward()
    assert torch.isfinite(logits).all()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    # checkpoint: a freshly constructed default model (grid_size 5 everywhere) adopts the sizes of the state dict
    fresh = _vit("efficientkan", seed=32)
    assert all(m.grid_size == 5 for m in fresh.modules() if isinstance(m, KANLinear))
    fresh.load_state_dict(model.state_dict())
    assert all(m.grid_size == 10 for m in fresh.modules() if isinstance(m, KANLinear))
    with torch.no_grad():
        assert torch.equal(fresh(images), model(images))


def test_vision_transformer_mixed_blocks_extend_only_the_efficient_kan_ones():
    model = _vit("efficientkan,cheby")
    torch.manual_seed(33)
    images = torch.randn(4, 3, 32, 32).cuda()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model.extend_grid(images, 10)
    for k, v in model.state_dict().items():
        if k.startswith("blocks.1."):
            assert torch.equal(v, before[k]), k              # the ChebyKAN block just runs
        elif k.endswith(".grid"):
            assert v.shape[1] == 17, k
        elif k.endswith("spline_weight"):
            assert v.shape[2] == 13, k
    assert torch.isfinite(model(images)).all()


def test_vision_transformer_without_a_kanlinear_raises():
    model = _vit("sine")
    with pytest.raises(NotImplementedError, match="KANLinear"):
        model.extend_grid(torch.randn(2, 3, 32, 32).cuda(), 10)


# ---------------------------------------------------------------------------------------------------------------------
# train.py --grid-extend
# ---------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _train(extra, tmp_path):
    """train.main on five fixed batches at train.py's default geometry with one block (cached per flag set)."""
    import train
    key = tuple(extra)
    if "init" not in _RUNS:               # one initial state for every run: KANLinear's least-squares initialisation is not bitwise reproducible
        from model import VisionTransformer
        torch.manual_seed(9)
        _RUNS["init"] = {k: v.clone() for k, v in VisionTransformer((3, 32, 32), 4, 1, 64, 8, 100, type="efficientkan").state_dict().items()}
    if key not in _RUNS:
        g = torch.Generator().manual_seed(7)
        batches = [(torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 100, (8,), generator=g)) for _ in range(5)]
        args = train.parse(["--model-type", "efficientkan", "--epochs", "1", "--n-blocks", "1", "--synthetic", "--no-step-metrics",
                            "--log-dir", str(tmp_path / f"logs{len(_RUNS)}")] + list(extra))
        _RUNS[key] = train.main(args, batches=batches, init_state=_RUNS["init"])
    return _RUNS[key]


def test_train_with_a_grid_extension(tmp_path):
    run = _train(["--grid-extend", "3:10"], tmp_path)
    plain = _train([], tmp_path)
    print("loss trajectories:", plain["losses"], run["losses"])
    assert len(run["losses"]) == 5 and all(v == v and abs(v) != float("inf") for v in run["losses"])
    assert run["losses"][:2] == plain["losses"][:2]          # the extension comes at the start of step 3
    model, opt = run["model"], run["optimizer"]
    params = dict(model.named_parameters())
    replaced = [n for n in params if n.endswith("spline_weight")]
    assert len(replaced) == 1 + 3 * 8
    for n in replaced:
        assert params[n].shape[-1] == 13, n
    for k, v in model.state_dict().items():
        if k.endswith(".grid"):
            assert v.shape[1] == 17 and torch.isfinite(v).all(), k
    held = {id(p) for group in opt.param_groups for p in group["params"]}
    assert held == {id(p) for p in params.values()}          # the optimizer holds exactly the model's parameters, the new ones included
    assert len(opt.state) == len(params)
    for n, p in params.items():
        steps = int(opt.state[p]["step"])
        assert steps == (3 if n in replaced else 5), (n, steps)          # steps 3, 4, 5 since the extension; all five otherwise
    assert int(opt.state[params["mlp_head.1.weight"]]["step"]) == 5


def test_train_extension_takes_the_place_of_an_update_due_on_the_same_step(tmp_path, monkeypatch):
    from model import VisionTransformer
    seen = []
    real_update, real_extend = VisionTransformer.update_grid, VisionTransformer.extend_grid
    monkeypatch.setattr(VisionTransformer, "update_grid", lambda self, x, *a: (seen.append("update"), real_update(self, x, *a))[1])
    monkeypatch.setattr(VisionTransformer, "extend_grid", lambda self, x, *a: (seen.append("extend"), real_extend(self, x, *a))[1])
    run = _train(["--grid-extend", "2:8", "--grid-update-every", "2"], tmp_path)
    assert seen == ["extend", "update"]                       # step 2: the extension alone; step 4: the update
    assert len(run["losses"]) == 5 and all(v == v and abs(v) != float("inf") for v in run["losses"])


@pytest.mark.parametrize("flag, word", [("--graph", "--graph"), ("--dp", "--dp")])
def test_train_refuses_graph_and_dp(flag, word):
    import train
    args = train.parse(["--model-type", "efficientkan", "--synthetic", "--grid-extend", "3:10", flag])
    with pytest.raises(SystemExit, match=f"--grid-extend is not combined with {word}"):
        train.main(args)


def test_train_refuses_model_types_without_a_kanlinear():
    import train
    args = train.parse(["--model-type", "cheby", "--synthetic", "--grid-extend", "3:10"])
    with pytest.raises(SystemExit, match="KANLinear"):
        train.main(args)
