"""GPU tests of KANLinear.update_grid as a fused Gram-matrix spline refit (kanvit_bspline_refit_*, csrc/kan_bspline_refit.hip) and
of everything built on it: ops.bspline_refit, MSA.update_grid (one grouped launch), VisionTransformer.update_grid and train.py
--grid-update-every.

References: the reference implementation's own results (tests/golden/update_grid.npz) and, on the shapes that have no goldens,
the float64 restatement of tests/_update_grid_ref.py, which tests/test_update_grid_cpu.py pins against those goldens.  Bounds,
after update_grid on the GPU: knots within 1e-6 (1 + |g|); spline_weight within 1e-4 normwise per layer; the layer's forward on
x within 1e-4 normwise.  Every non-degenerate case first asserts, from the restatement, that every feature's smallest Cholesky
pivot ratio is at least 10 tau (tau = 1e-5, the solve kernel's degeneracy threshold): a condition on the inputs."""
import copy

import pytest
import torch

from tests import _update_grid_ref as ug
from tests._util import T, bf16_bits_to_f32, load_npz, state_dict_from

pytestmark = pytest.mark.gpu

GRID_BOUND, WEIGHT_BOUND, FORWARD_BOUND = 1e-6, 1e-4, 1e-4


def cpu_state(layer):
    return {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}


def make_layer(i, o, grid_size=5, order=3, seed=0, standalone=True):
    from models.effkan import KANLinear
    torch.manual_seed(500 + seed)
    layer = KANLinear(i, o, grid_size=grid_size, spline_order=order, enable_standalone_scale_spline=standalone)
    with torch.no_grad():
        layer.spline_weight.uniform_(-0.5, 0.5)
    return layer


def check_against(tag, layer, x, knots, weight, y, features=None, rows=None):
    """The three bounds for a GPU layer after its update; `features`: the feature subset the knots and weights are compared on."""
    g, w = layer.grid.detach().cpu(), layer.spline_weight.detach().cpu()
    if features is not None:
        g, knots, w, weight = g[features], knots[features], w[:, features], weight[:, features]
    got_y = layer(x).detach().cpu()
    if rows is not None:
        got_y = got_y[rows]
    ge, we, fe = ug.grid_err(g, knots), ug.rel(w, weight), ug.rel(got_y, y)
    print(f"{tag}: grid err {ge:.3e} (bound {GRID_BOUND:.0e})  weight err {we:.3e} (bound {WEIGHT_BOUND:.0e})  "
          f"forward err {fe:.3e} (bound {FORWARD_BOUND:.0e})")
    assert ge <= GRID_BOUND, (tag, ge)
    assert we <= WEIGHT_BOUND, (tag, we)
    assert fe <= FORWARD_BOUND, (tag, fe)
    assert torch.isfinite(layer.grid).all() and torch.isfinite(layer.spline_weight).all()


def restated_case(tag, layer, x, xg=None):
    """update_grid(x) of `layer` on the GPU against the float64 restatement on the layer's state before the call."""
    sd = cpu_state(layer)
    gs, order = layer.grid_size, layer.spline_order
    knots, weight = ug.refit(x, sd, gs, order, layer.grid_eps)
    piv = float(ug.pivot_ratios(x, knots, order).min())
    print(f"{tag}: smallest pivot ratio {piv:.3e}")
    assert piv >= 10 * ug.TAU, (tag, piv)                   # a condition on the inputs
    layer = layer.cuda()
    xg = x.cuda() if xg is None else xg
    kept = layer.update_grid(xg)
    assert kept.dim() == 0 and kept.is_cuda and int(kept) == 0
    check_against(tag, layer, xg, knots, weight, ug.forward64(x, sd, knots, weight, order))
    return layer


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own results
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_goldens(tag):
    from kanvit import _lib
    from models.effkan import KANLinear
    blob = load_npz("update_grid.npz")
    m, i, o, gs, order = (int(v) for v in blob[f"{tag}.cfg"])
    x = bf16_bits_to_f32(blob[f"{tag}.x"]).cuda()
    layer = KANLinear(i, o, grid_size=gs, spline_order=order)
    layer.load_state_dict(state_dict_from(blob, tag + "."))
    layer = layer.cuda()
    rows = slice(None, None, 2)
    assert ug.rel(layer(x)[rows], T(blob[f"{tag}.y_before"])) <= FORWARD_BOUND
    uniform_before = bool(layer.kan_cfg().flags & _lib.FLAG_UNIFORM_KNOTS)
    kept = layer.update_grid(x)
    assert kept.dim() == 0 and kept.is_cuda and int(kept) == 0
    # grid.copy_ bumped the buffer's version: the next forward re-derives the knot flags and runs the general kernels
    assert uniform_before == (order == 3) and not layer.kan_cfg().flags & _lib.FLAG_UNIFORM_KNOTS
    check_against(f"golden {tag} {(m, i, o, gs, order)}", layer, x, T(blob[f"{tag}.grid_after"]), T(blob[f"{tag}.spline_weight_after"]),
                  T(blob[f"{tag}.y_after"]), rows=rows)


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement, ragged shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_three_bands_ragged_sizes_strided_input():
    layer = make_layer(17, 5, seed=1)
    torch.manual_seed(1)
    x = torch.randn(1100, 17)
    wide = torch.zeros(1100, 25)
    wide[:, 3:20] = x
    xg = wide.cuda()[:, 3:20]
    assert xg.stride(0) == 25 and not xg.is_contiguous()
    restated_case("(1100, 17, 5) strided", layer, x, xg)


def test_data_far_outside_the_initial_grid():
    torch.manual_seed(2)
    restated_case("(257, 8, 8) x ~ 3 randn + 0.5", make_layer(8, 8, seed=2), 3.0 * torch.randn(257, 8) + 0.5)


def test_one_band():
    torch.manual_seed(3)
    restated_case("(64, 8, 8)", make_layer(8, 8, seed=3), torch.randn(64, 8))


def test_wide_basis_and_wide_output():
    """grid_size 12, order 3: nb = 15, the 24-slot instantiation of the Gram kernel; O = 70: more output columns than the solve
    kernel has threads."""
    torch.manual_seed(4)
    restated_case("(400, 5, 70) grid 12", make_layer(5, 70, grid_size=12, seed=4), torch.randn(400, 5))


def test_order_1_grid_8():
    torch.manual_seed(5)
    restated_case("(300, 6, 7) grid 8 order 1", make_layer(6, 7, grid_size=8, order=1, seed=5), torch.randn(300, 6))


def test_second_update_starts_from_a_non_uniform_grid():
    from kanvit import _lib
    torch.manual_seed(6)
    layer = restated_case("(512, 8, 8) first", make_layer(8, 8, seed=6), torch.randn(512, 8))
    assert not layer.kan_cfg().flags & _lib.FLAG_UNIFORM_KNOTS          # the old basis of the next refit takes the general path
    x2 = 0.7 * torch.randn(512, 8) + 0.2
    restated_case("(512, 8, 8) second", layer.cpu(), x2)


def test_without_the_standalone_scaler():
    torch.manual_seed(7)
    layer = make_layer(8, 8, seed=7, standalone=False)
    assert not hasattr(layer, "spline_scaler")
    restated_case("(300, 8, 8) no spline_scaler", layer, torch.randn(300, 8))


def test_the_scaler_quirk_is_kept():
    """The fit target is scaled_spline_weight, the result goes into spline_weight, spline_scaler stays (models/effkan.py:196,241)."""
    torch.manual_seed(8)
    layer = make_layer(8, 8, seed=8).cuda()
    scaler = layer.spline_scaler.detach().clone()
    base = layer.base_weight.detach().clone()
    layer.update_grid(torch.randn(300, 8).cuda())
    assert torch.equal(layer.spline_scaler, scaler) and torch.equal(layer.base_weight, base)


# ---------------------------------------------------------------------------------------------------------------------
# degenerate features keep their function
# ---------------------------------------------------------------------------------------------------------------------
def test_constant_column_is_flagged_and_left_alone():
    layer = make_layer(6, 4, seed=9)
    torch.manual_seed(9)
    x = torch.randn(200, 6)
    x[:, 2] = 0.3
    sd = cpu_state(layer)
    knots, weight = ug.refit(x, sd, 5, 3, layer.grid_eps)
    good = [0, 1, 3, 4, 5]
    piv = ug.pivot_ratios(x, knots, 3)
    print("pivot ratios", piv.tolist())
    assert float(piv[good].min()) >= 10 * ug.TAU and float(piv[2]) <= 0.1 * ug.TAU
    layer = layer.cuda()
    kept = layer.update_grid(x.cuda())
    assert int(kept) == 1
    assert torch.equal(layer.grid[2].cpu(), sd["grid"][2]) and torch.equal(layer.spline_weight[:, 2].cpu(), sd["spline_weight"][:, 2])
    # the other features are independent of it (in the reference too): expected state = the restatement's there, the old one at 2
    knots[2], weight[:, 2] = sd["grid"][2].double(), sd["spline_weight"][:, 2].double()
    check_against("(200, 6, 4) column 2 constant", layer, x.cuda(), knots, weight, ug.forward64(x, sd, knots, weight, 3), features=good)


def test_fewer_rows_than_basis_functions():
    layer = make_layer(3, 3, seed=10)
    torch.manual_seed(10)
    x = torch.randn(4, 3)
    sd = cpu_state(layer)
    layer = layer.cuda()
    kept = layer.update_grid(x.cuda())
    assert int(kept) == 3
    for k, v in layer.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
        assert torch.isfinite(v).all()


def test_no_rows_flags_everything_and_launches_nothing():
    from dataclasses import replace
    from kanvit import ops
    layer = make_layer(5, 4, seed=11).cuda()
    cfg = replace(layer.kan_cfg(), has_base=0, base_act=0)
    w_old = layer.scaled_spline_weight.detach().permute(1, 2, 0).reshape(1, -1, 4)
    w_new, ok = ops.bspline_refit(torch.zeros(0, 5, device="cuda"), w_old, cfg, layer.grid.reshape(1, -1), layer.grid.unsqueeze(0) * 1.5)
    assert ok.dtype == torch.bool and tuple(ok.shape) == (1, 5) and not ok.any()
    assert torch.equal(w_new, w_old)


def test_other_families_are_refused_by_name():
    from kanvit import ops
    cfg = ops.LayerCfg(family=ops.CHEBY, I=4, O=4, G=5)
    z = torch.zeros(8, 4, device="cuda")
    with pytest.raises(NotImplementedError, match="cheby"):
        ops.bspline_refit(z, torch.zeros(1, 20, 4, device="cuda"), cfg, z, z)


# ---------------------------------------------------------------------------------------------------------------------
# determinism, autocast, grouping
# ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal_and_autocast_changes_nothing():
    torch.manual_seed(12)
    proto = make_layer(17, 5, seed=12).cuda()
    x = torch.randn(1100, 17).cuda()
    runs = []
    for mode in ("plain", "plain", "autocast"):
        layer = copy.deepcopy(proto)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "autocast"):
            layer.update_grid(x)
        runs.append(layer)
    for other in runs[1:]:
        assert torch.equal(runs[0].grid, other.grid) and torch.equal(runs[0].spline_weight, other.spline_weight)
    assert not torch.equal(runs[0].grid, proto.grid)


def test_msa_grouped_launch_equals_every_layer_alone(monkeypatch):
    from attention import MSA
    from kanvit import ops
    H, dh = 2, 16
    torch.manual_seed(13)
    msa = MSA(32, n_heads=H, type="efficientkan")
    with torch.no_grad():
        for n, p in msa.named_parameters():
            if "spline_weight" in n:
                p.uniform_(-0.5, 0.5)
    msa = msa.cuda()
    x = torch.randn(8, 17, 32).cuda()
    alone = copy.deepcopy(msa)
    calls = []
    real = ops.bspline_refit

    def recorder(x2d, w, cfg, old, new):
        calls.append(cfg)
        return real(x2d, w, cfg, old, new)

    monkeypatch.setattr(ops, "bspline_refit", recorder)
    kept = msa.update_grid(x)
    assert len(calls) == 1 and calls[0].groups == 3 * H and calls[0].x_group_mod == H      # ONE grouped launch over the 3*H layers
    assert int(kept) == 0
    rows = x.reshape(-1, 32)
    layers = list(msa.q_mappings) + list(msa.k_mappings) + list(msa.v_mappings)
    singles = list(alone.q_mappings) + list(alone.k_mappings) + list(alone.v_mappings)
    for gi, (grouped, single) in enumerate(zip(layers, singles)):
        h = gi % H
        before = single.grid.clone()
        single.update_grid(rows[:, h * dh:(h + 1) * dh])
        assert not torch.equal(single.grid, before)
        assert torch.equal(grouped.grid, single.grid), gi
        assert torch.equal(grouped.spline_weight, single.spline_weight), gi
        assert torch.equal(grouped.spline_scaler, single.spline_scaler) and torch.equal(grouped.base_weight, single.base_weight)
    for h in range(H):                                       # q, k and v of a head share their knots
        assert torch.equal(msa.q_mappings[h].grid, msa.k_mappings[h].grid) and torch.equal(msa.q_mappings[h].grid, msa.v_mappings[h].grid)
    assert not torch.equal(msa.q_mappings[0].grid, msa.q_mappings[1].grid)
    y = msa(x)                                               # the grouped forward runs on the per-head grids
    assert torch.isfinite(y).all()


def test_msa_refuses_other_types_by_name():
    from attention import MSA
    msa = MSA(32, n_heads=2, type="cheby").cuda()
    with pytest.raises(NotImplementedError, match="cheby"):
        msa.update_grid(torch.randn(2, 5, 32, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# VisionTransformer.update_grid
# ---------------------------------------------------------------------------------------------------------------------
def _vit(kind, seed=14):
    from model import VisionTransformer
    torch.manual_seed(seed)
    return VisionTransformer((3, 32, 32), n_patches=4, n_blocks=2, d_hidden=64, n_heads=8, type=kind).cuda()


def test_vision_transformer_equals_the_pieces_by_hand():
    model = _vit("efficientkan")
    torch.manual_seed(15)
    images, labels = torch.randn(8, 3, 32, 32).cuda(), torch.randint(0, 10, (8,)).cuda()
    with torch.no_grad():
        model(images)                                        # the model has run: the fused-embedding decision is cached
    assert model._fused_embed is not None
    hand = copy.deepcopy(model)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    kept = model.update_grid(images)
    assert kept.dim() == 0 and kept.is_cuda
    assert model._fused_embed is None
    with torch.no_grad():
        hand.linear_mapper.update_grid(hand.patchify(images, 4).reshape(-1, hand.input_d))
        hand._fused_embed = None
        out = hand._embed(images)
        hand.blocks[0].attn.update_grid(hand.blocks[0].norm1(out))
        out = hand.blocks[0](out)
        hand.blocks[1].attn.update_grid(hand.blocks[1].norm1(out))
    sd, sd_hand = model.state_dict(), hand.state_dict()
    moved = 0
    for k in sd:
        assert torch.equal(sd[k], sd_hand[k]), k
        if k.endswith(".grid"):
            moved += int(not torch.equal(sd[k], before[k]))
        elif not k.endswith("spline_weight"):
            assert torch.equal(sd[k], before[k]), k          # only knots and spline weights move
    assert moved == 1 + 2 * 3 * 8                            # the patch embedding and every per-head layer of both blocks
    logits = model(images)
    torch.nn.functional.cross_entropy(logits, labels).backward()
    assert torch.isfinite(logits).all()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_vision_transformer_mixed_blocks_update_only_the_efficient_kan_ones():
    model = _vit("efficientkan,cheby")
    torch.manual_seed(16)
    images = torch.randn(8, 3, 32, 32).cuda()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model.update_grid(images)
    for k, v in model.state_dict().items():
        changed = not torch.equal(v, before[k])
        if k.startswith("blocks.1."):
            assert not changed, k                            # the ChebyKAN block just runs
        elif k.endswith(".grid"):
            assert changed, k
    assert torch.isfinite(model(images)).all()


@pytest.mark.parametrize("kind", ["cheby", "vanilla"])
def test_vision_transformer_without_a_kanlinear_raises(kind):
    model = _vit(kind)
    with pytest.raises(NotImplementedError, match="KANLinear"):
        model.update_grid(torch.randn(2, 3, 32, 32).cuda())


# ---------------------------------------------------------------------------------------------------------------------
# train.py --grid-update-every
# ---------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _train(extra, tmp_path):
    """train.main on four fixed batches at train.py's default geometry with one block (cached per flag set)."""
    import train
    key = tuple(extra)
    if "init" not in _RUNS:               # one initial state for every run: KANLinear's least-squares initialisation is not bitwise reproducible
        from model import VisionTransformer
        torch.manual_seed(9)
        _RUNS["init"] = {k: v.clone() for k, v in VisionTransformer((3, 32, 32), 4, 1, 64, 8, 100, type="efficientkan").state_dict().items()}
    if key not in _RUNS:
        g = torch.Generator().manual_seed(7)
        batches = [(torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 100, (8,), generator=g)) for _ in range(4)]
        args = train.parse(["--model-type", "efficientkan", "--epochs", "1", "--n-blocks", "1", "--synthetic", "--no-step-metrics",
                            "--log-dir", str(tmp_path / f"logs{len(_RUNS)}")] + list(extra))
        _RUNS[key] = train.main(args, batches=batches, init_state=_RUNS["init"])
    return _RUNS[key]


def test_train_with_grid_updates(tmp_path):
    run = _train(["--grid-update-every", "2"], tmp_path)
    plain = _train([], tmp_path)
    print("loss trajectories:", plain["losses"], run["losses"])
    assert len(run["losses"]) == 4 and all(v == v and abs(v) != float("inf") for v in run["losses"])
    assert run["losses"][0] == plain["losses"][0]            # the first update comes before the second step
    grids = {k: v for k, v in run["model"].state_dict().items() if k.endswith(".grid")}
    assert len(grids) == 1 + 3 * 8
    for k, v in grids.items():
        assert not torch.equal(v.cpu(), _RUNS["init"][k]), k
        assert torch.isfinite(v).all()


def test_train_grid_update_every_zero_is_the_plain_step(tmp_path):
    plain, zero = _train([], tmp_path), _train(["--grid-update-every", "0"], tmp_path)
    assert len(plain["losses"]) == 4 and zero["losses"] == plain["losses"]
    for k, v in zero["model"].state_dict().items():
        if k.endswith(".grid"):
            assert torch.equal(v.cpu(), _RUNS["init"][k]), k


@pytest.mark.parametrize("flag, word", [("--graph", "--graph"), ("--dp", "--dp")])
def test_train_refuses_graph_and_dp(flag, word):
    import train
    args = train.parse(["--model-type", "efficientkan", "--synthetic", "--grid-update-every", "2", flag])
    with pytest.raises(SystemExit, match=f"--grid-update-every is not combined with {word}"):
        train.main(args)


def test_train_refuses_model_types_without_a_kanlinear():
    import train
    args = train.parse(["--model-type", "cheby", "--synthetic", "--grid-update-every", "2"])
    with pytest.raises(SystemExit, match="KANLinear"):
        train.main(args)
