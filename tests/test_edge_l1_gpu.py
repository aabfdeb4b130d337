"""GPU tests of the per-edge mean-absolute-activation statistic (kanvit_edge_l1_*, csrc/kan_edge_l1.hip) and everything built on
it: KANLinear / ChebyKANLayer / FastKANLayer.edge_activation_l1, the sample-based regularization_loss, MSA's grouped launch,
VisionTransformer.forward(return_regularization=True) and train.py --reg-lambda.

Reference: float64 torch written here (oracle.kan_oracle.bspline_bases for the B-spline bases): phi[m, o, i] by einsum, A =
|phi|.mean(0), the two loss terms, autograd for every gradient.  A and the loss are held to tests/_util.close at 1e-4.

sign(phi) is discontinuous, so a sample whose phi is a near-total cancellation may legitimately take the other sign in fp32.
A sample is FRAGILE when, in the float64 reference, |phi| <= 1e-5 * sum_j |Phi_j w_j| and that sum is non-zero.  Gradient
comparisons leave out the (i, o) pairs (weight gradients) and the (m, i) entries (input gradient) that contain a fragile sample
-- and every test asserts that the share left out is at most 2 % of pairs and 2 % of entries; everything else is held to the
same 1e-4 criterion.  FastKAN's kernel input is u = LayerNorm(x): its (m, i) entries are compared under that rule on d loss / d u
(read off the LayerNorm's output), and d loss / d x, in which the LayerNorm backward mixes the features of a row, on the rows
that hold no fragile sample; the share of rows that leaves out is printed and held to row_cap()."""
import pytest
import torch
import torch.nn.functional as F

from oracle import kan_oracle as ko
from tests._util import close

pytestmark = pytest.mark.gpu

FRAGILE = 1e-5
CAP = 0.02


def row_cap(m, samples_per_row):
    """Bound on the share of ROWS that hold a fragile sample (FastKAN's d loss / d x only).  A sample is fragile with probability
    about 2 * FRAGILE * f(0), f the density of phi / sum_j |Phi_j w_j| at 0, which is of order 1 for weights symmetric about 0:
    2e-5 per sample, so 2e-5 * samples_per_row per row.  Three times that expectation, plus one row (m is small)."""
    return 3 * 2 * FRAGILE * samples_per_row + 1.0 / m
ACTS = {"silu": (torch.nn.SiLU, F.silu), "gelu": (torch.nn.GELU, F.gelu),
        "gelu-tanh": (lambda: torch.nn.GELU(approximate="tanh"), lambda t: F.gelu(t, approximate="tanh")),
        "relu": (torch.nn.ReLU, F.relu), "tanh": (torch.nn.Tanh, torch.tanh), "identity": (torch.nn.Identity, lambda t: t)}


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def ref_phi(sd, prefix, x, include_base=False, act=F.silu, order=3, keep_u=None):
    """(phi, mag)[m, o, i] of the layer under `prefix` of a reference-layout state dict on rows x[m, i]: the edge functions
    and sum_j |Phi_j w_j| (the scale a cancellation is measured against)."""
    kind = ko.layer_kind(sd, prefix)
    g = lambda n: sd[prefix + n]
    if kind == "efficientkan":
        B = ko.bspline_bases(x, g("grid"), order)
        w = g("spline_weight") * g("spline_scaler").unsqueeze(-1) if prefix + "spline_scaler" in sd else g("spline_weight")
        phi = torch.einsum("mig,oig->moi", B, w)
        mag = torch.einsum("mig,oig->moi", B.abs(), w.abs())
        base_w = g("base_weight") if include_base else None
        xb = x
    elif kind == "cheby":
        t = torch.tanh(x)
        cols = [torch.ones_like(t), t]
        c = g("cheby_coeffs")
        for _ in range(2, c.shape[2]):
            cols.append(2.0 * t * cols[-1] - cols[-2])
        B = torch.stack(cols[:c.shape[2]], dim=-1)
        phi = torch.einsum("mid,iod->moi", B, c)
        mag = torch.einsum("mid,iod->moi", B.abs(), c.abs())
        base_w = None
    else:
        assert kind == "fast"
        grid = g("rbf.grid")
        h = (grid[-1] - grid[0]) / (grid.numel() - 1)
        u = F.layer_norm(x, (x.shape[-1],), g("layernorm.weight"), g("layernorm.bias"), 1e-5)
        if keep_u is not None:
            u.retain_grad()
            keep_u.append(u)
        B = torch.exp(-(((u.unsqueeze(-1) - grid) / h) ** 2))
        w = g("spline_linear.weight").view(-1, x.shape[-1], grid.numel())
        phi = torch.einsum("mig,oig->moi", B, w)
        mag = torch.einsum("mig,oig->moi", B.abs(), w.abs())
        base_w = g("base_linear.weight") if include_base and prefix + "base_linear.weight" in sd else None
        xb = x
    if base_w is not None:
        b = act(xb).unsqueeze(1) * base_w.unsqueeze(0)
        phi = phi + b
        mag = mag + b.abs()
    return phi, mag


def ref_loss(l1, ra=1.0, re_=1.0):
    total = l1.sum()
    p = l1 / total
    return ra * total - re_ * torch.special.xlogy(p, p).sum()


def fragile_of(phi, mag):
    return ((phi.abs() <= FRAGILE * mag) & (mag > 0)).detach()


def f64_state(module):
    sd = {}
    for k, v in module.state_dict().items():
        v = v.detach().cpu()
        sd[k] = v.double().clone().requires_grad_(not ko.is_buffer_key(k)) if v.is_floating_point() else v.clone()
    return sd


def weight_keep(sd, prefix, frag):
    """{parameter key: bool mask of the elements to compare} for the layer's own weights, from fragile[m, o, i]."""
    pair = ~frag.any(0)                                     # [o, i]
    kind = ko.layer_kind(sd, prefix)
    if kind == "efficientkan":
        out = {prefix + "spline_weight": pair.unsqueeze(-1).expand_as(sd[prefix + "spline_weight"]), prefix + "base_weight": pair}
        if prefix + "spline_scaler" in sd:
            out[prefix + "spline_scaler"] = pair
        return out, pair
    if kind == "cheby":
        return {prefix + "cheby_coeffs": pair.t().unsqueeze(-1).expand_as(sd[prefix + "cheby_coeffs"])}, pair
    o, i = pair.shape
    out = {prefix + "spline_linear.weight": pair.unsqueeze(-1).expand(o, i, sd[prefix + "rbf.grid"].numel()).reshape(o, -1)}
    if prefix + "base_linear.weight" in sd:
        out[prefix + "base_linear.weight"] = pair
    return out, pair


def assert_close_masked(name, got, want, keep=None):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if keep is not None:
        got, want = got[keep], want[keep]
    if want.numel() == 0:
        return
    err, bound = float((got - want).abs().max()), 2e-6 + 1e-4 * float(want.abs().max())
    print(f"{name}: max err {err:.3e} (bound {bound:.3e}, {want.numel()} elements)")
    assert close(got, want, rtol=1e-4), (name, err, bound)


# ---------------------------------------------------------------------------------------------------------------------
# single layers
# ---------------------------------------------------------------------------------------------------------------------
def make_layer(kind, i, o, seed, act="silu", grid_size=5, order=3, nonuniform=False):
    from models.cheby import ChebyKANLayer
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    torch.manual_seed(1000 + seed)
    if kind == "efficientkan":
        layer = KANLinear(i, o, grid_size=grid_size, spline_order=order, base_activation=ACTS[act][0])
        if nonuniform:                                      # strictly increasing knots with uneven, per-feature spacing
            steps = layer.grid[:, 1:] - layer.grid[:, :-1]
            steps = steps * (0.6 + 0.8 * torch.rand(steps.shape))
            layer.grid.copy_(torch.cat([layer.grid[:, :1], layer.grid[:, :1] + steps.cumsum(1)], dim=1))
    elif kind == "cheby":
        layer = ChebyKANLayer(i, o, 4)
    else:
        layer = FastKANLayer(i, o, base_activation=ACTS[act][1])
        with torch.no_grad():
            layer.layernorm.weight.add_(0.1 * torch.randn(i))
            layer.layernorm.bias.add_(0.1 * torch.randn(i))
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if "layernorm" not in n and "rbf" not in n and "bias" not in n:
                p.uniform_(-0.5, 0.5)
    return layer


def layer_case(kind, shape, seed, include_base=False, act="silu", grid_size=5, order=3, nonuniform=False, sliced=False):
    m, i, o = shape
    layer = make_layer(kind, i, o, seed, act, grid_size, order, nonuniform)
    torch.manual_seed(seed)
    x = 0.8 * torch.randn(m, i)
    # float64 reference
    sd = f64_state(layer)
    x64 = x.double().requires_grad_()
    u64 = []
    phi, mag = ref_phi(sd, "", x64, include_base, ACTS[act][1], order, keep_u=u64)
    A_ref = phi.abs().mean(0)
    loss_ref = ref_loss(A_ref, 0.7, 1.3)
    loss_ref.backward()
    frag = fragile_of(phi, mag)
    keep, pair = weight_keep(sd, "", frag)
    entry = ~frag.any(1)                                    # [m, i]
    assert 1.0 - float(pair.float().mean()) <= CAP, ("share of (i, o) pairs left out", 1.0 - float(pair.float().mean()))
    assert 1.0 - float(entry.float().mean()) <= CAP, ("share of (m, i) entries left out", 1.0 - float(entry.float().mean()))
    # GPU
    layer = layer.cuda()
    if sliced:                                              # x is a column slice of a wider matrix: ldx > I
        wide = torch.zeros(m, i + 5)
        wide[:, 3:3 + i] = x
        wide = wide.cuda().requires_grad_()
        xg, leaf = wide[:, 3:3 + i], wide
    else:
        xg = leaf = x.cuda().requires_grad_()
    kw = {} if kind == "cheby" else {"include_base": include_base}
    with torch.no_grad():
        A = layer.edge_activation_l1(xg, **kw)
    assert tuple(A.shape) == (o, i)
    ug = []
    if kind == "fast":
        layer.layernorm.register_forward_hook(lambda mod, inp, out: (out.retain_grad(), ug.append(out))[0])
    loss = layer.regularization_loss(0.7, 1.3, x=xg, **kw) if kind == "efficientkan" else layer.regularization_loss(xg, 0.7, 1.3, **kw)
    loss.backward()
    torch.cuda.synchronize()
    tag = f"{kind}{shape} seed {seed} base {include_base} {act}"
    assert_close_masked(tag + " A", A, A_ref)
    assert_close_masked(tag + " loss", loss, loss_ref)
    gx = leaf.grad[:, 3:3 + i] if sliced else leaf.grad
    if kind == "fast":
        assert_close_masked(tag + " du", ug[0].grad, u64[0].grad, entry)
        entry = entry.all(1, keepdim=True).expand(m, i)     # the LayerNorm backward spreads a row's du over the row
        rows_out = 1.0 - float(entry.float().mean())
        print(f"{tag}: share of rows left out of dx {rows_out:.4f} (cap {row_cap(m, i * o):.4f})")
        assert rows_out <= row_cap(m, i * o), (rows_out, row_cap(m, i * o))
    assert_close_masked(tag + " dx", gx, x64.grad, entry)
    if sliced:
        assert float(leaf.grad[:, :3].abs().max()) == 0.0 and float(leaf.grad[:, 3 + i:].abs().max()) == 0.0
    params = dict(layer.named_parameters())
    for k, mask in keep.items():
        if sd[k].grad is None:                              # the base weights without the base term
            assert params[k].grad is None or float(params[k].grad.abs().max()) == 0.0, k
            continue
        assert_close_masked(f"{tag} d{k}", params[k].grad, sd[k].grad, mask)


SHAPES = [(1, 3, 5), (33, 7, 10), (130, 64, 64), (257, 16, 48), (1100, 32, 32)]


@pytest.mark.parametrize("include_base", [False, True])
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_kanlinear_against_float64(shape, seed, include_base):
    layer_case("efficientkan", shape, seed, include_base)


def test_band_shape_has_three_ragged_bands():
    import ctypes as C
    from kanvit import _lib
    d = _lib.LayerDesc(family=_lib.BSPLINE, groups=1, x_group_mod=1, I=32, O=32, G=8, spline_order=3, has_base=0, flags=2, M=1100,
                       ldx=32, ldy=32, bparam_stride=32 * 12)
    bands = _lib.lib().kanvit_edge_l1_row_bands(C.byref(d))
    assert bands >= 3
    # every band but the last holds ceil(M / bands) rows rounded up to whole 64-row blocks
    rows_per_band = -(-(-(-1100 // bands)) // 64) * 64
    assert (bands - 1) * rows_per_band < 1100 <= bands * rows_per_band          # that many bands, none empty
    assert 1100 % rows_per_band != 0                                             # the last one is ragged


VSHAPES = [(33, 7, 10), (130, 64, 64)]


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("shape", VSHAPES)
def test_base_activations(shape, act):
    layer_case("efficientkan", shape, 0, include_base=True, act=act)


@pytest.mark.parametrize("include_base", [False, True])
@pytest.mark.parametrize("shape", VSHAPES)
def test_non_uniform_knots_take_the_general_path(shape, include_base):
    layer_case("efficientkan", shape, 0, include_base, nonuniform=True)


@pytest.mark.parametrize("include_base", [False, True])
@pytest.mark.parametrize("shape", VSHAPES)
def test_spline_order_2_grid_7(shape, include_base):
    layer_case("efficientkan", shape, 1, include_base, grid_size=7, order=2)


@pytest.mark.parametrize("nonuniform", [False, True])
def test_wide_basis_and_more_than_one_column_chunk(nonuniform):
    """grid_size 12: 15 bases + the base column = 16 generated columns, the 24-column instantiations; O = 70: two chunks of output
    columns, so dx is summed over chunks by read-modify-write; non-uniform knots: 18-float Cox-de Boor strips, the LDS opt-in."""
    layer_case("efficientkan", (33, 7, 70), 0, include_base=True, grid_size=12, nonuniform=nonuniform)


@pytest.mark.parametrize("shape", VSHAPES)
def test_column_slice_input(shape):
    layer_case("efficientkan", shape, 0, include_base=True, sliced=True)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", VSHAPES + [(1100, 32, 32)])
def test_chebykan(shape, seed):
    layer_case("cheby", shape, seed)


@pytest.mark.parametrize("include_base", [False, True])
@pytest.mark.parametrize("shape", VSHAPES)
def test_fastkan(shape, include_base):
    layer_case("fast", shape, 0, include_base)


def test_fastkan_other_base_activation():
    layer_case("fast", (33, 7, 10), 1, include_base=True, act="gelu")


# ---------------------------------------------------------------------------------------------------------------------
# determinism, the dx = NULL path, autocast, empty input
# ---------------------------------------------------------------------------------------------------------------------
def _run(layer, x, need_x=True, **kw):
    xg = x.clone().requires_grad_(need_x)
    layer.zero_grad(set_to_none=True)
    A = layer.edge_activation_l1(xg, **kw)
    (A * torch.linspace(0.5, 1.5, A.numel(), device=A.device).view_as(A)).sum().backward()
    return A.detach(), {k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None}, xg.grad


@pytest.mark.parametrize("kind", ["efficientkan", "cheby", "fast"])
def test_bitwise_reproducible_and_dx_null_path(kind):
    layer = make_layer(kind, 32, 32, 0).cuda()
    torch.manual_seed(0)
    x = (0.8 * torch.randn(1100, 32)).cuda()
    kw = {} if kind == "cheby" else {"include_base": True}
    A1, g1, dx1 = _run(layer, x, **kw)
    A2, g2, dx2 = _run(layer, x, **kw)
    assert torch.equal(A1, A2) and torch.equal(dx1, dx2)
    assert g1.keys() == g2.keys() and all(torch.equal(g1[k], g2[k]) for k in g1)
    if kind != "fast":                                      # FastKAN's LayerNorm parameters need dx of the kernel either way
        A3, g3, dx3 = _run(layer, x, need_x=False, **kw)
        assert dx3 is None and torch.equal(A1, A3)
        assert all(torch.equal(g1[k], g3[k]) for k in g1)


@pytest.mark.parametrize("kind", ["efficientkan", "cheby", "fast"])
def test_autocast_runs_the_exact_fp32_kernels(kind):
    layer = make_layer(kind, 16, 48, 1).cuda()
    torch.manual_seed(1)
    x = (0.8 * torch.randn(257, 16)).cuda()
    A1, g1, dx1 = _run(layer, x)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        A2, g2, dx2 = _run(layer, x)
    assert A2.dtype == torch.float32 and torch.equal(A1, A2) and torch.equal(dx1, dx2)
    assert all(torch.equal(g1[k], g2[k]) for k in g1)


def test_empty_input_gives_zeros():
    layer = make_layer("efficientkan", 7, 10, 0).cuda()
    x = torch.zeros(0, 7, device="cuda", requires_grad=True)
    A = layer.edge_activation_l1(x)
    A.sum().backward()
    assert float(A.abs().max()) == 0.0 and float(layer.spline_weight.grad.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# grouped launch (MSA)
# ---------------------------------------------------------------------------------------------------------------------
def _randomize(module, seed):
    torch.manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if any(s in n for s in ("spline_weight", "spline_scaler", "base_weight", "cheby_coeffs", "spline_linear.weight",
                                    "base_linear.weight")):
                p.uniform_(-0.5, 0.5)


@pytest.mark.parametrize("include_base", [False, True])
@pytest.mark.parametrize("kind", ["efficientkan", "cheby", "fast"])
def test_msa_grouped_launch(kind, include_base, monkeypatch):
    from dataclasses import replace
    from attention import MSA
    from kanvit import ops
    from models.fastkan import FastKANLayer
    H = 2
    msa = MSA(32, n_heads=H, type=kind)
    _randomize(msa, 5)
    torch.manual_seed(0)
    x = 0.8 * torch.randn(2, 17, 32)
    sd = f64_state(msa)
    x64 = x.double().requires_grad_()
    rows = x64.reshape(-1, 32)
    A_ref, loss_ref, keeps, pairs, entry, left = [], 0.0, {}, [], torch.ones(34, 32, dtype=torch.bool), []
    u64, u_entry = [], []
    for pi, proj in enumerate("qkv"):
        for h in range(H):
            prefix = f"{proj}_mappings.{h}."
            phi, mag = ref_phi(sd, prefix, rows[:, h * 16:(h + 1) * 16], include_base, keep_u=u64)
            l1 = phi.abs().mean(0)
            A_ref.append(l1)
            loss_ref = loss_ref + ref_loss(l1)
            frag = fragile_of(phi, mag)
            k, pair = weight_keep(sd, prefix, frag)
            keeps.update(k)
            pairs.append(pair)
            e = ~frag.any(1)
            left.append(1.0 - float(e.float().mean()))
            u_entry.append(e)
            entry[:, h * 16:(h + 1) * 16] &= e.all(1, keepdim=True).expand_as(e) if kind == "fast" else e
    loss_ref.backward()
    assert 1.0 - float(torch.stack(pairs).float().mean()) <= CAP
    assert max(left) <= CAP
    if kind == "fast":
        rows_out = 1.0 - float(entry.float().mean())
        print(f"msa fast: share of rows left out of dx {rows_out:.4f} (cap {row_cap(34, 3 * 16 * 16):.4f})")
        assert rows_out <= row_cap(34, 3 * 16 * 16)
    msa = msa.cuda()
    xg = x.cuda().requires_grad_()
    # record the grouped launch's operands, and FastKAN's grouped LayerNorm output u (the kernel's input)
    calls, ug = [], []
    real_edge_l1, real_u = ops.edge_l1, FastKANLayer.kan_u_grouped

    def edge_l1_recorder(x2d, w, cfg, bparams=None):
        calls.append((x2d.detach(), w.detach(), cfg, None if bparams is None else bparams.detach()))
        return real_edge_l1(x2d, w, cfg, bparams)

    def u_recorder(layers, x2d, n_heads):
        u = real_u(layers, x2d, n_heads)
        if u.requires_grad:
            u.retain_grad()
        ug.append(u)
        return u

    monkeypatch.setattr(ops, "edge_l1", edge_l1_recorder)
    monkeypatch.setattr(FastKANLayer, "kan_u_grouped", staticmethod(u_recorder))
    with torch.no_grad():
        A = msa.edge_activation_l1(xg, include_base)
    assert len(calls) == 1                                   # ONE grouped launch over the 3*H layers
    xin, wg, cfg, bpg = calls[0]
    assert cfg.groups == 3 * H and tuple(wg.shape)[0] == 3 * H
    assert tuple(A.shape) == (3, H, 16, 16)
    loss = msa.regularization_loss(xg, include_base=include_base)
    loss.backward()
    assert_close_masked(f"msa {kind} A", A.reshape(3 * H, 16, 16), torch.stack(A_ref))
    assert_close_masked(f"msa {kind} loss", loss, loss_ref)
    assert_close_masked(f"msa {kind} dx", xg.grad.reshape(-1, 32), x64.grad.reshape(-1, 32), entry)
    if kind == "fast":                                       # the kernel's own input gradient, under the (m, i) entry rule
        du_ref = torch.cat([u.grad for u in u64], dim=1)
        assert_close_masked("msa fast du", ug[-1].grad, du_ref, torch.cat(u_entry, dim=1))
    params = dict(msa.named_parameters())
    for k, mask in keeps.items():
        if sd[k].grad is not None:
            assert_close_masked(f"msa {kind} d{k}", params[k].grad, sd[k].grad, mask)
    # the grouped launch computes for every layer exactly what a launch of that layer alone computes
    with torch.no_grad():
        kw = {} if kind == "cheby" else {"include_base": include_base}
        layers = list(msa.q_mappings) + list(msa.k_mappings) + list(msa.v_mappings)
        xr = xg.detach().reshape(-1, 32)
        for gi, layer in enumerate(layers):
            h = gi % H
            single = layer.edge_activation_l1(xr[:, h * 16:(h + 1) * 16], **kw)
            if kind == "fast":              # torch forms the grouped and the single LayerNorm with different arithmetic: u differs in ulps
                assert close(single, A[gi // H, h], rtol=1e-5), (kind, gi)
            else:
                assert torch.equal(single, A[gi // H, h]), (kind, gi)
        if kind == "fast":
            # the same statement bit for bit at the kernel's own input: every group alone, on its column slice of the SAME u
            # (row stride > I), with the raw input next to it in the [u | x] layout when the base is on
            Ag = A.transpose(-1, -2).reshape(3 * H, 16, 16)                 # [group, in, out], as the kernel writes it
            n = 3 * H * 16
            for gi in range(3 * H):
                if cfg.has_base:
                    wide = torch.cat([xin[:, gi * 16:(gi + 1) * 16], xin[:, n + gi * 16:n + (gi + 1) * 16], xin[:, :5]], dim=1)
                    xs = wide[:, :32]
                else:
                    xs = xin[:, gi * 16:(gi + 1) * 16]
                assert xs.stride(0) > xs.shape[1]
                one = real_edge_l1(xs, wg[gi:gi + 1], replace(cfg, groups=1, x_group_mod=1), bpg[gi:gi + 1])
                assert torch.equal(one[0], Ag[gi]), ("fast", gi)


def test_msa_refuses_other_types_by_name():
    from attention import MSA
    msa = MSA(32, n_heads=2, type="sine").cuda()
    with pytest.raises(NotImplementedError, match="efficientkan, cheby, fast"):
        msa.edge_activation_l1(torch.randn(2, 5, 32, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# VisionTransformer.forward(return_regularization=True)
# ---------------------------------------------------------------------------------------------------------------------
def _vit_reference(sd, images, labels, n_patches, n_heads, lam):
    """float64 forward of oracle.kan_oracle.vit_forward's structure that also collects the regulariser; returns
    (logits, reg, total loss, {parameter key: keep mask}, share of pairs left out)."""
    d = sd["v_class"].shape[1]
    n_blocks = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    patches = ko.patchify(images.double(), n_patches)
    rows = patches.reshape(-1, patches.shape[-1])
    keeps, pairs = {}, []

    def layer_reg(prefix, r):
        phi, mag = ref_phi(sd, prefix, r)
        k, pair = weight_keep(sd, prefix, fragile_of(phi, mag))
        keeps.update(k)
        pairs.append(pair.reshape(-1))
        return ref_loss(phi.abs().mean(0))

    reg = layer_reg("linear_mapper.", rows)
    tok = ko.layer_forward(sd, "linear_mapper.", patches).reshape(patches.shape[0], patches.shape[1], d)
    tok = torch.cat([sd["v_class"].unsqueeze(0).expand(tok.shape[0], -1, -1), tok], dim=1)
    out = tok + ko.positional_embeddings(tok.shape[1], d).double()
    dh = d // n_heads
    for l in range(n_blocks):
        p = f"blocks.{l}."
        hN = F.layer_norm(out, (d,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-5)
        hr = hN.reshape(-1, d)
        for proj in "qkv":
            for h in range(n_heads):
                reg = reg + layer_reg(f"{p}attn.{proj}_mappings.{h}.", hr[:, h * dh:(h + 1) * dh])
        out = out + ko.msa_forward(sd, p + "attn.", hN, n_heads)
        hN = F.layer_norm(out, (d,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-5)
        out = out + F.linear(F.relu(F.linear(hN, sd[p + "ff.0.weight"], sd[p + "ff.0.bias"])), sd[p + "ff.2.weight"], sd[p + "ff.2.bias"])
    cls = F.layer_norm(out[:, 0], (d,), sd["mlp_head.0.weight"], sd["mlp_head.0.bias"], 1e-5)
    logits = F.linear(cls, sd["mlp_head.1.weight"], sd["mlp_head.1.bias"])
    total = F.cross_entropy(logits, labels) + lam * reg
    return logits, reg, total, keeps, 1.0 - float(torch.cat(pairs).float().mean())


@pytest.mark.parametrize("kind", ["efficientkan", "cheby", "fast"])
def test_vision_transformer_returns_the_regulariser(kind):
    from model import VisionTransformer
    torch.manual_seed(0)
    model = VisionTransformer((3, 32, 32), n_patches=4, n_blocks=2, d_hidden=64, n_heads=8, type=kind)
    torch.manual_seed(1)
    images, labels = 0.8 * torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,))
    sd = f64_state(model)
    logits_ref, reg_ref, total_ref, keeps, left_out = _vit_reference(sd, images, labels, 4, 8, 0.01)
    total_ref.backward()
    assert left_out <= CAP, left_out
    model = model.cuda()
    xg, yg = images.cuda(), labels.cuda()
    with torch.no_grad():
        plain = model(xg)
    logits, reg = model(xg, return_regularization=True)
    assert torch.equal(logits, plain)
    (F.cross_entropy(logits, yg) + 0.01 * reg).backward()
    assert_close_masked(f"vit {kind} logits", logits, logits_ref)
    assert_close_masked(f"vit {kind} reg", reg, reg_ref)
    for k, p in model.named_parameters():
        if sd[k].grad is None:
            continue
        assert p.grad is not None, k
        assert_close_masked(f"vit {kind} d{k}", p.grad, sd[k].grad, keeps.get(k))


def test_vision_transformer_refuses_other_types():
    from model import VisionTransformer
    model = VisionTransformer((3, 32, 32), n_patches=4, n_blocks=1, d_hidden=64, n_heads=8, type="sine").cuda()
    with pytest.raises(NotImplementedError, match="efficientkan, cheby, fast"):
        model(torch.randn(2, 3, 32, 32, device="cuda"), return_regularization=True)


# ---------------------------------------------------------------------------------------------------------------------
# train.py --reg-lambda
# ---------------------------------------------------------------------------------------------------------------------
_TRAJ = {}


def _train(extra, tmp_path):
    """CE loss trajectory of train.main on three fixed batches at train.py's default geometry (cached per flag set)."""
    import train
    key = tuple(extra)
    if "init" not in _TRAJ:           # one initial state for every run: KANLinear's least-squares initialisation is not bitwise reproducible
        from model import VisionTransformer
        torch.manual_seed(9)
        _TRAJ["init"] = {k: v.clone() for k, v in VisionTransformer((3, 32, 32), 4, 8, 64, 8, 100, type="efficientkan").state_dict().items()}
    if key not in _TRAJ:
        g = torch.Generator().manual_seed(7)
        batches = [(torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 100, (8,), generator=g)) for _ in range(3)]
        args = train.parse(["--model-type", "efficientkan", "--epochs", "1", "--synthetic", "--no-step-metrics",
                            "--log-dir", str(tmp_path / f"logs{len(_TRAJ)}")] + list(extra))
        _TRAJ[key] = train.main(args, batches=batches, init_state=_TRAJ["init"])["losses"]
    return _TRAJ[key]


def test_train_reg_lambda_zero_is_the_plain_step(tmp_path):
    plain, zero = _train([], tmp_path), _train(["--reg-lambda", "0"], tmp_path)
    assert len(plain) == 3 and zero == plain, (plain, zero)


def test_train_with_the_regulariser_eager_equals_graph(tmp_path):
    plain = _train([], tmp_path)
    eager = _train(["--reg-lambda", "0.01"], tmp_path)
    graph = _train(["--reg-lambda", "0.01", "--graph"], tmp_path)
    print("CE trajectories:", plain, eager, graph)
    assert len(eager) == 3 and all(v == v for v in eager)
    assert eager == graph                   # the regularised step replays from a HIP graph with the same trajectory
    assert eager[0] == plain[0] and eager[1:] != plain[1:]      # the logged loss is the CE term; the regulariser moves the weights


def test_train_with_the_regulariser_under_bf16_autocast(tmp_path):
    amp = _train(["--reg-lambda", "0.01", "--amp", "bf16"], tmp_path)
    eager = _train(["--reg-lambda", "0.01"], tmp_path)
    print("CE trajectories:", eager, amp)
    assert len(amp) == 3 and all(v == v for v in amp)
    assert all(abs(a - e) < 0.1 for a, e in zip(amp, eager)), (amp, eager)
