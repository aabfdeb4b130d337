"""The layer-to-kernel protocol (kanvit/grouped.py: KanLayer, as_kan) and VisionTransformer's one model walk, without a GPU:

  * the grouped packing of an MSA's q|k|v layers is, slice by slice and gradient by gradient, every layer's own kan_pack();
  * every layer class answers the whole protocol, and only FastKAN has a u input, a LayerNorm to fuse and a grouped u;
  * _walk hands out every block with its real input, runs a block only after its consumer is done with it, never the last one."""
import pytest
import torch

KINDS = ["cheby", "efficientkan", "fast", "sine", "vanilla"]


def _layer_classes():
    from models.cheby import ChebyKANLayer
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    from models.nfkan import NaiveFourierKANLayer
    from models.sinekan import SineKANLayer
    return {"cheby": lambda: ChebyKANLayer(6, 5, 4), "efficientkan": lambda: KANLinear(6, 5), "fast": lambda: FastKANLayer(6, 5),
            "sine": lambda: SineKANLayer(6, 5, grid_size=4), "fourier": lambda: NaiveFourierKANLayer(6, 5, grid_size=3),
            "vanilla": lambda: torch.nn.Linear(6, 5)}


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


@pytest.mark.parametrize("kind", KINDS)
def test_grouped_packing_is_every_layers_own_packing(kind):
    from attention import MSA
    from kanvit import grouped
    torch.manual_seed(11 + len(kind))
    msa = MSA(32, 2, type=kind)
    cfg, w, bp, bias = grouped.pack_projections([msa.q_mappings, msa.k_mappings, msa.v_mappings])
    assert cfg.groups == 6 and cfg.x_group_mod == 2
    layers = [grouped.as_kan(m) for m in list(msa.q_mappings) + list(msa.k_mappings) + list(msa.v_mappings)]
    singles = [m.kan_pack() for m in layers]
    for g, (w1, bp1, bias1) in enumerate(singles):
        assert torch.equal(w[g], w1), (kind, g)
        assert _same(None if bp is None else bp[g], bp1), (kind, g)
        assert _same(None if bias is None else bias[g], None if bias1 is None else bias1.reshape(-1)), (kind, g)
    params = [p for p in msa.parameters() if p.requires_grad]
    got = torch.autograd.grad(w.sum(), params, allow_unused=True)
    want = torch.autograd.grad(sum(w1.sum() for w1, _, _ in singles), params, allow_unused=True)
    assert any(g is not None for g in want)
    for (name, _), a, b in zip(msa.named_parameters(), got, want):
        assert _same(a, b), (kind, name)


@pytest.mark.parametrize("kind", KINDS + ["fourier"])
def test_every_class_answers_the_whole_protocol(kind):
    from kanvit import grouped, ops
    layer = grouped.as_kan(_layer_classes()[kind]())
    assert isinstance(layer, grouped.KanLayer)
    a, b = layer.kan_cfg(), layer.kan_cfg([layer])
    assert isinstance(a, ops.LayerCfg) and isinstance(b, ops.LayerCfg) and (a.family, a.I, a.O, a.G) == (b.family, b.I, b.O, b.G)
    w, _, _ = layer.kan_pack()
    assert tuple(w.shape) == (a.I * a.GP, a.O)
    x = torch.randn(7, 6)
    if kind == "fast":
        assert torch.equal(layer.kan_u(x), layer.layernorm(x)) and layer.kan_ln() is layer.layernorm
        assert tuple(type(layer).kan_u_grouped([layer], x, 1).shape) == (7, 6)
    else:
        assert layer.kan_u(x) is None and layer.kan_ln() is None and type(layer).kan_u_grouped([layer], x, 1) is None
    assert (layer.kan_base_act() is None) == (kind not in ("efficientkan", "fast"))


def test_base_act_is_none_without_a_live_base_path():
    from kanvit import _lib
    from models.fastkan import FastKANLayer
    assert FastKANLayer(6, 5, use_base_update=False).kan_base_act() is None
    assert FastKANLayer(6, 5, base_activation=torch.relu).kan_base_act() == _lib.BASE_RELU


def test_fourier_has_no_grouped_packing():
    from models.nfkan import NaiveFourierKANLayer
    with pytest.raises(NotImplementedError, match="NaiveFourierKANLayer"):
        NaiveFourierKANLayer.kan_pack_grouped([NaiveFourierKANLayer(6, 5, grid_size=3)])


def test_time_benchmark_switches_the_layernorm_off_for_the_call_only(monkeypatch):
    from kanvit import grouped
    from models.fastkan import FastKANLayer
    layer = FastKANLayer(6, 5)
    seen = []

    def recorder(m, x2d):
        seen.append((m.kan_ln(), m.kan_u(x2d)))
        raise RuntimeError("stop here")

    monkeypatch.setattr(grouped, "run_single", recorder)
    x = torch.randn(3, 6)
    with pytest.raises(RuntimeError, match="stop here"):
        layer(x, time_benchmark=True)
    assert seen == [(None, None)]
    assert layer.kan_ln() is layer.layernorm and torch.equal(layer.kan_u(x), layer.layernorm(x))      # restored after the exception
    with pytest.raises(RuntimeError, match="stop here"):
        layer(x)
    assert seen[1][0] is layer.layernorm and torch.equal(seen[1][1], layer.layernorm(x))


# ---- VisionTransformer._walk ------------------------------------------------------------------------------------------------------------
class _Recording(torch.nn.Module):
    """A block stand-in: adds `step`, and logs that it ran."""

    def __init__(self, k, log):
        super().__init__()
        self.k, self.log, self.step = k, log, 1.0

    def forward(self, x):
        self.log.append(("run", self.k))
        return x + self.step


def _recording_vit():
    from model import VisionTransformer
    torch.manual_seed(0)
    m = VisionTransformer((1, 8, 8), n_patches=2, n_blocks=3, d_hidden=8, n_heads=2, out_d=3, type="vanilla")
    log = []
    m.blocks = torch.nn.ModuleList([_Recording(k, log) for k in range(3)])
    return m, log


def test_walk_yields_each_block_with_its_real_input_and_runs_it_afterwards():
    m, log = _recording_vit()
    images = torch.randn(2, 1, 8, 8)
    with torch.no_grad():
        first = m._embed(images)
        inputs = []
        for blk, x in m._walk(images):
            log.append(("see", blk.k))
            inputs.append(x)
            blk.step = 10.0 ** (blk.k + 1)            # a consumer that changes the block: the block's run must see it
    assert log == [("see", 0), ("run", 0), ("see", 1), ("run", 1), ("see", 2)]          # the last block is never run
    assert torch.equal(inputs[0], first)
    assert torch.equal(inputs[1], first + 10.0) and torch.equal(inputs[2], first + 10.0 + 100.0)


@pytest.mark.parametrize("who,args,verb", [("update_grid", (), "update"), ("extend_grid", (8,), "extend")])
def test_refits_refuse_a_model_without_kanlinear_before_anything_runs(who, args, verb, monkeypatch):
    m, log = _recording_vit()

    def boom(*a, **k):
        raise AssertionError("nothing may run before the refusal")

    monkeypatch.setattr(m, "_embed", boom)
    with pytest.raises(NotImplementedError, match=rf"{who}: model type\(s\) \['vanilla'\] have no KANLinear, the only layer "
                                                  rf"with a B-spline grid to {verb} \('efficientkan'\)"):
        getattr(m, who)(torch.randn(2, 1, 8, 8), *args)
    assert log == []
