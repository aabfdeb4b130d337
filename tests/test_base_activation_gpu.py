"""Base activations other than SiLU on the GPU: KANLinear / FastKANLayer against a float64 restatement (the oracle's layer with the
base path removed, plus act(x) Wb^T in float64), the q|k|v launches at the benchmark's row counts (same kernel forms as SiLU, the
*_act_* twins, forced tails bitwise equal to the untailed launch), the fused patch embedding, the tiny per-head kernels, an
attribute swap, mixed activations in one MSA and train.main eager against --graph.

Bounds are the suite's: fp32 forward 2e-5 of max(1, max |ref|), gradients 1e-4 relative (tests/test_headline_parity_gpu.py);
bf16 within 1e-2 normwise of the unrounded float64 result (tests/test_bf16_oracle_gpu.py's LOOSE)."""
import functools
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import kan_oracle as ko
import numpy as np

from tests._util import bf16_bits_to_f32, load_npz, record_kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD, TOL, LOOSE = 2e-5, 1e-4, 1e-2
CHUNK = 4096

ACTS = {   # name -> (module for KANLinear, callable for FastKANLayer, float64 reference)
    "silu": (nn.SiLU, F.silu, F.silu),
    "gelu": (nn.GELU, F.gelu, F.gelu),
    "gelu-tanh": (functools.partial(nn.GELU, approximate="tanh"), functools.partial(F.gelu, approximate="tanh"),
                  functools.partial(F.gelu, approximate="tanh")),
    "relu": (nn.ReLU, F.relu, F.relu),
    "tanh": (nn.Tanh, torch.tanh, torch.tanh),
    "identity": (nn.Identity, nn.Identity(), lambda x: x),
}
REF = {0: F.silu, 1: F.gelu, 2: functools.partial(F.gelu, approximate="tanh"), 3: F.relu, 4: torch.tanh, 5: lambda x: x}


def _code(layer):
    from kanvit import ops
    return ops.base_activation_code(layer.base_activation)


def _ref_layer(layer, x):
    """float64 forward of one KANLinear / FastKANLayer (parameters from the module, requires_grad) with its base activation."""
    from models.effkan import KANLinear
    p = {n: t.detach().cpu().double().requires_grad_(t.requires_grad) for n, t in layer.named_parameters()}
    act = REF[_code(layer)]
    if isinstance(layer, KANLinear):
        zero = torch.zeros_like(p["base_weight"])
        y = ko.kanlinear_forward(x, zero, p["spline_weight"], p.get("spline_scaler"), layer.grid.detach().cpu().double(),
                                 layer.spline_order)
        y = y + act(x) @ p["base_weight"].t()
    else:
        y = ko.fastkan_forward(x, p["layernorm.weight"], p["layernorm.bias"], p["rbf.grid"], p["spline_linear.weight"], None, None,
                               float(layer.rbf.denominator))
        y = y + act(x) @ p["base_linear.weight"].t() + p["base_linear.bias"]
    return y, p


def _rel(a, b, floor=1e-3):
    return float((a.double() - b).abs().max()) / max(float(b.abs().max()), floor)


def _fro(a, b):
    return float((a.double() - b).norm()) / max(float(b.norm()), 1e-30)


def _check_layer(layer, x, bf16=False):
    layer = layer.to(DEV)
    layer.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    w = torch.randn(*x.shape[:-1], layer.out_features if hasattr(layer, "out_features") else layer.output_dim)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        y = layer(xg)
    (y.float() * w.to(DEV)).sum().backward()
    x64 = x.double().requires_grad_(True)
    yr, p = _ref_layer(layer, x64)
    (yr * w.double()).sum().backward()
    got = {n: t.grad.cpu() for n, t in layer.named_parameters() if t.grad is not None}
    if bf16:
        assert _fro(y.detach().cpu(), yr.detach()) < LOOSE
        assert _fro(xg.grad.cpu(), x64.grad) < LOOSE
        for n, g in got.items():
            assert _fro(g, p[n].grad) < LOOSE, n
        return
    assert float((y.detach().cpu().double() - yr.detach()).abs().max()) / max(1.0, float(yr.abs().max())) < FWD
    assert _rel(xg.grad.cpu(), x64.grad) < TOL
    assert set(got) == {n for n, t in p.items() if t.grad is not None}
    for n, g in got.items():
        assert _rel(g, p[n].grad) < TOL, n


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("m", [1, 7, 129, 1000])
def test_kanlinear_vs_fp64(act, m):
    from models.effkan import KANLinear
    torch.manual_seed(m)
    layer = KANLinear(13, 7, base_activation=ACTS[act][0])
    _check_layer(layer, torch.randn(m, 13) * 1.5)
    # spline_order 2 and non-uniform knots: the LDS-tile kernels
    layer2 = KANLinear(40, 33, spline_order=2, base_activation=ACTS[act][0])      # wider than the tiny kernels take
    with torch.no_grad():
        layer2.grid.add_(torch.rand_like(layer2.grid) * 0.01)
        layer2.grid.copy_(layer2.grid.sort(dim=1).values)
    with record_kernels() as names:
        _check_layer(layer2, torch.randn(m, 3, 40))          # 3-D input
    sfx = "_kernel" if act == "silu" else "_act_kernel"
    for k in ("kan_fwd", "kan_bwd_input", "kan_bwd_weight"):
        assert any(n.startswith(k + sfx + "<2,") for n in names), (k + sfx, sorted(names))


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("m", [1, 7, 129, 1000])
def test_fastkan_vs_fp64(act, m):
    from models.fastkan import FastKANLayer
    torch.manual_seed(10 + m)
    _check_layer(FastKANLayer(11, 5, base_activation=ACTS[act][1]), torch.randn(m, 11))
    _check_layer(FastKANLayer(64, 64, base_activation=ACTS[act][1]), torch.randn(m, 2, 64))


@pytest.mark.parametrize("act", ["gelu", "relu", "tanh"])
def test_layers_bf16_autocast(act):
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    torch.manual_seed(3)
    _check_layer(KANLinear(64, 64, base_activation=ACTS[act][0]), torch.randn(2048, 64), bf16=True)
    _check_layer(FastKANLayer(64, 64, base_activation=ACTS[act][1]), torch.randn(2048, 64), bf16=True)


def _set_act(module, act):
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    for m in module.modules():
        if isinstance(m, KANLinear):
            m.base_activation = ACTS[act][0]()
        elif isinstance(m, FastKANLayer):
            m.base_activation = ACTS[act][1]


def _run_qkv(msa, x, w, bf16):
    from kanvit import grouped
    msa.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    with record_kernels() as names:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            y = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, xg)
        (y * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in msa.named_parameters() if p.grad is not None}
    return y.detach().cpu(), xg.grad.detach().cpu(), grads, {n for n in names if n.startswith("kan_")}


def _oracle_qkv(msa, h, x, w):
    """float64 q|k|v of every head on row chunks: (y, dx, parameter gradients by name)."""
    layers = [(f"{p}_mappings.{i}.", getattr(msa, f"{p}_mappings")[i]) for p in ("q", "k", "v") for i in range(h)]
    dh = x.shape[1] // h
    ys, dxs, grads = [], [], {}
    params = {}
    for r0 in range(0, x.shape[0], CHUNK):
        xd = x[r0:r0 + CHUNK].double().requires_grad_(True)
        outs = []
        for gi, (pre, layer) in enumerate(layers):
            y, p = _ref_layer(layer, xd[:, (gi % h) * dh:(gi % h + 1) * dh])
            params.setdefault(pre, []).append(p)
            outs.append(y)
        y = torch.cat(outs, dim=1)
        (y * w[r0:r0 + CHUNK].double()).sum().backward()
        ys.append(y.detach())
        dxs.append(xd.grad)
    for pre, plist in params.items():
        for n in plist[0]:
            if plist[0][n].grad is not None:
                grads[pre + n] = sum(p[n].grad for p in plist)
    return torch.cat(ys), torch.cat(dxs), grads


def _silu_names(names):
    return {n.replace("_act_kernel", "_kernel") for n in names}


BENCH = [("efficientkan", 768, 12, 128 * 197), ("fast", 384, 6, 256 * 197)]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fam,d,h,m", BENCH, ids=[c[0] for c in BENCH])
def test_bench_shape_qkv(fam, d, h, m, bf16):
    from attention import MSA
    torch.manual_seed(7 + d)
    msa = MSA(d, h, type=fam).to(DEV)
    x = torch.randn(m, d)
    w = torch.randn(m, 3 * d)
    _, _, _, silu_names = _run_qkv(msa, x, w, bf16)
    for act in ("gelu", "relu"):
        _set_act(msa, act)
        y, dx, grads, names = _run_qkv(msa, x, w, bf16)
        # same forms as SiLU, every B-spline / RBF kernel an *_act_* twin (none of them computes SiLU)
        assert _silu_names(names) == silu_names, (act, sorted(names), sorted(silu_names))
        fam_kernels = [n for n in names if re.search(r"<[23],", n)]
        assert fam_kernels and all("_act_kernel" in n for n in fam_kernels), sorted(names)
        yr, dxr, gr = _oracle_qkv(msa, h, x, w)
        if bf16:
            assert _fro(y, yr) < LOOSE and _fro(dx, dxr) < LOOSE, act
            for k, g in gr.items():
                assert _fro(grads[k], g) < LOOSE, (act, k)
        else:
            assert float((y.double() - yr).abs().max()) / max(1.0, float(yr.abs().max())) < FWD, act
            assert _rel(dx, dxr) < TOL, act
            for k, g in gr.items():
                assert _rel(grads[k], g) < TOL, (act, k)
            y2, dx2, grads2, _ = _run_qkv(msa, x, w, bf16)
            assert torch.equal(y, y2) and torch.equal(dx, dx2)
            assert all(torch.equal(grads[k], grads2[k]) for k in grads)


TAIL_FORMS = {   # a piece of the sub-divided launch tail that must run when KANVIT_TAIL = 6 (tests/test_launch_shapes_gpu.py)
    ("efficientkan", False): r"kan_fwd_reg_act_kernel<2, 2, 3, 2, 9, true>",
    ("efficientkan", True): r"kan_bwd_input_res_bf16_act_kernel<2, \d+, \d+, 3, true>",
}
# FastKAN's launches (NSH = 1 forward, no input-gradient tail at these shapes) have no tail pieces to force


@pytest.mark.parametrize("fam,bf16", list(TAIL_FORMS), ids=[f"{f}-{'bf16' if b else 'fp32'}" for f, b in TAIL_FORMS])
def test_forced_tail_bitwise(fam, bf16, monkeypatch):
    """KANVIT_TAIL = 6 cuts the last row tiles into pieces (efficient-KAN at the bench shape): the *_act_* pieces run, and the results
    are bitwise the untailed launch's."""
    from attention import MSA
    from kanvit import _lib
    torch.manual_seed(5)
    d, h, m = 768, 12, 128 * 197
    msa = MSA(d, h, type=fam).to(DEV)
    _set_act(msa, "gelu")
    x, w = torch.randn(m, d), torch.randn(m, 3 * d)
    runs = []
    try:
        for tail in ("0", "6"):
            monkeypatch.setenv("KANVIT_TAIL", tail)
            assert f"tail={tail}" in _lib.reload_config().split()
            runs.append(_run_qkv(msa, x, w, bf16))
    finally:
        monkeypatch.undo()
        _lib.reload_config()
    (y0, dx0, g0, n0), (y1, dx1, g1, n1) = runs
    assert any(re.fullmatch(TAIL_FORMS[(fam, bf16)], n) for n in n1), sorted(n1)
    assert all("_act_kernel" in n for n in n0 | n1 if re.search(r"<[23],", n)), sorted(n0 | n1)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    assert all(torch.equal(g0[k], g1[k]) for k in g0)


def test_patch_embed_gelu_vs_three_step():
    from model import VisionTransformer
    torch.manual_seed(11)
    vit = VisionTransformer((3, 224, 224), 14, 1, 128, 2, 10, "efficientkan").to(DEV)
    _set_act(vit, "gelu")
    x = torch.randn(4, 3, 224, 224, device=DEV)
    lm = vit.linear_mapper
    with record_kernels() as names:
        out = vit._embed_fused(x)
    assert out is not None, "the fused patch embedding did not run"
    assert any(n.startswith("kan_fwd_reg_act_kernel") for n in names), sorted(names)
    patches = vit.patchify(x, vit.n_patches)

    def three_step():
        tok = lm(patches).reshape(4, -1, vit.d_hidden)
        return torch.cat((vit.v_class.unsqueeze(0).expand(4, -1, -1), tok), 1) + vit.pos_embeddings[: patches.shape[1] + 1]

    ref = three_step()
    assert float((out - ref).abs().max()) / max(1.0, float(ref.abs().max())) < FWD
    g = torch.randn_like(out)
    vit.zero_grad(set_to_none=True)
    (vit._embed_fused(x) * g).sum().backward()
    fused = {k: p.grad.detach().cpu() for k, p in lm.named_parameters() if p.grad is not None}
    vit.zero_grad(set_to_none=True)
    (three_step() * g).sum().backward()
    steps = {k: p.grad.detach().cpu() for k, p in lm.named_parameters() if p.grad is not None}
    assert set(fused) == set(steps) and fused
    for k in fused:
        assert _rel(fused[k], steps[k].double()) < TOL, k


@pytest.mark.parametrize("fam", ["efficientkan", "fast"])
def test_tiny_kernels_train_geometry(fam):
    """train.py's defaults (d_hidden 64, 8 heads: 8-wide per-head layers) run the tiny per-head kernels."""
    from attention import MSA
    torch.manual_seed(2)
    msa = MSA(64, 8, type=fam).to(DEV)
    _set_act(msa, "gelu")
    x, w = torch.randn(1000, 64), torch.randn(1000, 192)
    y, dx, grads, names = _run_qkv(msa, x, w, False)
    fam_kernels = [n for n in names if re.search(r"<[23],", n)]
    assert fam_kernels and all("_act_kernel" in n for n in fam_kernels), sorted(names)
    if fam == "efficientkan":            # FastKAN's per-head LayerNorm keeps it on the general kernels
        assert any(n.startswith("kan_tiny_") for n in names), sorted(names)
    yr, dxr, gr = _oracle_qkv(msa, 8, x, w)
    assert float((y.double() - yr).abs().max()) / max(1.0, float(yr.abs().max())) < FWD
    assert _rel(dx, dxr) < TOL
    for k, g in gr.items():
        assert _rel(grads[k], g) < TOL, k


def test_attribute_swap_between_forwards():
    from model import VisionTransformer
    torch.manual_seed(4)
    vit = VisionTransformer((1, 28, 28), 7, 2, 64, 2, 10, "efficientkan").to(DEV)
    x = torch.rand(8, 1, 28, 28, device=DEV)
    y_silu = vit(x).detach()
    _set_act(vit, "gelu")
    y_gelu = vit(x).detach()
    _set_act(vit, "silu")
    assert torch.equal(vit(x).detach(), y_silu)
    assert float((y_gelu - y_silu).abs().max()) > 1e-4


def test_mixed_activations_in_one_msa():
    from attention import MSA
    torch.manual_seed(6)
    msa = MSA(96, 3, type="efficientkan").to(DEV)
    for i, act in enumerate(("gelu", "relu", "silu")):
        msa.q_mappings[i].base_activation = ACTS[act][0]()
    msa.k_mappings[1].base_activation = nn.Tanh()
    x, w = torch.randn(500, 96), torch.randn(500, 288)
    y, dx, grads, _ = _run_qkv(msa, x, w, False)
    yr, dxr, gr = _oracle_qkv(msa, 3, x, w)
    assert float((y.double() - yr).abs().max()) / max(1.0, float(yr.abs().max())) < FWD
    assert _rel(dx, dxr) < TOL
    for k, g in gr.items():
        assert _rel(grads[k], g) < TOL, k


@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_train_main_eager_equals_graph_bitwise(act, tmp_path):
    """train.main --base-activation gelu (SiLU as the control), in the geometry of tests/test_train_gpu.py: eager and --graph give
    bitwise the same losses and parameters, and a second run of each gives bitwise the first."""
    import train
    from model import VisionTransformer
    from models.effkan import KANLinear
    torch.manual_seed(9)
    init = {k: v.clone() for k, v in VisionTransformer((1, 28, 28), 7, 2, 64, 2, 10, type="efficientkan").state_dict().items()}
    x, y = torch.rand(4, 1, 28, 28), torch.arange(4) % 10
    runs = []
    for i, extra in enumerate(((), ("--graph",), (), ("--graph",))):
        args = train.parse(["--model-type", "efficientkan", "--base-activation", act, "--epochs", "1", "--steps-per-epoch", "3",
                            "--log-dir", str(tmp_path / f"l{i}"), "--no-tuned-gemms", "--synthetic", "--in-chans", "1",
                            "--image-size", "28", "--n-patches", "7", "--n-blocks", "2", "--n-heads", "2", "--d-hidden", "64",
                            "--out-d", "10", "--batch-size", "4", *extra])
        h = train.main(args, batches=[(x, y)] * 3, init_state=init)
        want = nn.GELU if act == "gelu" else nn.SiLU
        assert all(isinstance(m.base_activation, want) for m in h["model"].modules() if isinstance(m, KANLinear))
        runs.append((list(h["losses"]), {k: v.detach().cpu().clone() for k, v in h["model"].state_dict().items()}))
    for l, sd in runs[1:]:
        assert l == runs[0][0], [r[0] for r in runs]
        assert all(torch.equal(sd[k], runs[0][1][k]) for k in sd)


# ---- the reference's own outputs (tests/golden/base_act.npz, written by tests/golden/make_golden_act.py) ----
def _det_fill(shape, salt):
    """tests/golden/make_golden_act.py::det_fill: exact float32 values from integer arithmetic."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    return torch.from_numpy((((i * 7919 + salt * 104729) % 4093 - 2046) / 16384.0).astype(np.float32).reshape(shape))


def _fill(module):
    with torch.no_grad():
        for salt, (name, p) in enumerate(sorted(module.named_parameters())):
            if p.requires_grad:
                p.copy_(_det_fill(p.shape, salt))


def _t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["eff", "fast"])
@pytest.mark.parametrize("act", list(ACTS))
def test_layer_vs_reference(act, kind, bf16):
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    blob = load_npz("base_act.npz")
    tag = f"{kind}.{act}"
    layer = KANLinear(13, 7, base_activation=ACTS[act][0]) if kind == "eff" else FastKANLayer(11, 5, base_activation=ACTS[act][1])
    _fill(layer)
    layer = layer.to(DEV)
    x = bf16_bits_to_f32(blob[tag + ".x"]).to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        y = layer(x)
    (y.float() * torch.linspace(-1, 1, y.numel(), device=DEV).reshape(y.shape)).sum().backward()
    ref_y = _t(blob[tag + ".y"]).double()
    got = {"y": (y.detach().cpu(), ref_y), "grad_x": (x.grad.cpu(), _t(blob[tag + ".grad_x"]).double())}
    for n, p in layer.named_parameters():
        if p.grad is not None:
            got[n] = (p.grad.cpu(), _t(blob[f"{tag}.grad.{n}"]).double())
    assert set(got) - {"y", "grad_x"} == {k[len(tag) + 6:] for k in blob if k.startswith(tag + ".grad.")}
    for n, (a, b) in got.items():
        if bf16:
            assert _fro(a, b) < LOOSE, (n, _fro(a, b))
        elif n == "y":
            assert float((a.double() - b).abs().max()) / max(1.0, float(b.abs().max())) < FWD
        else:
            assert _rel(a, b) < TOL, (n, _rel(a, b))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("typ", ["efficientkan", "fast"])
def test_model_vs_reference(typ, bf16):
    """VisionTransformer with GELU swapped into every KAN layer after construction (as the reference allows) against the
    reference's logits, loss and parameter gradients; bf16 bounds as tests/test_bf16_oracle_gpu.py's model tests."""
    from model import VisionTransformer
    blob = load_npz("base_act.npz")
    p = f"vit.{typ}."
    torch.manual_seed(0)
    vit = VisionTransformer((1, 28, 28), 7, 2, 64, 2, 10, typ)
    _set_act(vit, "gelu")
    _fill(vit)
    vit = vit.to(DEV)
    x = bf16_bits_to_f32(blob[p + "x"]).to(DEV)
    labels = _t(blob[p + "labels"]).long().to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        logits = vit(x)
        loss = F.cross_entropy(logits.float(), labels)
    loss.backward()
    ref = _t(blob[p + "logits"]).double()
    if bf16:
        assert 1e-6 < _fro(logits.detach().float().cpu(), ref) < 2 * LOOSE, _fro(logits.detach().float().cpu(), ref)
        assert abs(float(loss) - float(blob[p + "loss"])) < 2 * LOOSE
    else:
        assert float((logits.detach().cpu().double() - ref).abs().max()) < 1e-4
        assert abs(float(loss) - float(blob[p + "loss"])) < 1e-5
    if bf16:             # as tests/test_bf16_oracle_gpu.py's model tests: logits and loss (the gradients are checked in fp32)
        return
    n = 0
    for name, prm in vit.named_parameters():
        if prm.grad is None:
            continue
        g = prm.grad.detach().cpu().reshape(-1)
        want = _t(blob[p + "grad." + name]).double()
        g = g if g.numel() <= 64 else g[::37]
        assert _rel(g, want) < TOL, (name, _rel(g, want))
        n += 1
    assert n == len([k for k in blob if k.startswith(p + "grad.")])
