"""ChebyKAN's constant T0 column in the exact-fp32 register kernels (kan_fwd_reg.hip, kan_bwd_input_reg.hip, kan_bwd_weight_dma.hip).

T0(tanh x) = 1, so the forward adds b[o] = sum_i c[i, o, 0] once per output instead of contracting the T0 rows on the matrix
cores, the input gradient leaves the T0 slots out (dT0/dx = 0), and the weight gradient's T0 rows are one column sum of dY per
column, written to every feature.  Checked at the launch shapes of the benchmark (ViT-B/16, B = 128: 25 216 q|k|v rows, 25 088
patch rows) and at a ragged q|k|v launch with forced launch tails:
 (1) with c[:, :, 1:] = 0 every row of y is b, bitwise the same in every row and within fp32 rounding of the float64 sum;
 (2) dW[:, o, 0] is bitwise the same for every feature and within fp32 rounding of the float64 column sum of dY;
 (3) y, dx and dW agree with the general LDS-tile kernels (KANVIT_NO_REG / KANVIT_NO_REG_BW) and are bitwise reproducible."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 1e-5            # register form against the LDS-tile form: max |a - b| / max |b|


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


@contextlib.contextmanager
def _env(monkeypatch, **kv):
    from kanvit import _lib
    for k, v in kv.items():
        monkeypatch.setenv(k, v)
    try:
        _lib.reload_config()
        yield
    finally:
        monkeypatch.undo()
        _lib.reload_config()


def _qkv(msa, x, w):
    from kanvit import grouped
    msa.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    y = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, xg)
    (y * w).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), xg.grad.detach(), {k: p.grad.detach().clone() for k, p in msa.named_parameters() if p.grad is not None}


def _layers(msa):
    return [(f"{p}_mappings.{h}", m) for p in ("q", "k", "v") for h, m in enumerate(getattr(msa, f"{p}_mappings"))]


def _check_t0_rows(msa, w, grads):
    """dW[:, o, 0] of every q|k|v layer: the same bits for every feature, and the float64 column sum of its dY columns"""
    d = w.shape[1] // 3
    o = d // len(msa.q_mappings)
    for j, (name, _) in enumerate(_layers(msa)):
        g0 = grads[f"{name}.cheby_coeffs"][:, :, 0]
        assert torch.equal(g0, g0[:1].expand_as(g0)), name
        ref = w[:, j * o:(j + 1) * o].double().sum(0)
        assert _rel(g0[0], ref) < REL, name


QKV = [(128 * 197, 0), (14 * 197, 0), (14 * 197, 5)]      # bench rows; ragged 22-tile launch, untailed and with a 5-tile tail


@pytest.mark.parametrize("m,tail", QKV, ids=[f"M{m}-tail{t}" for m, t in QKV])
def test_qkv_t0_only_layer_is_its_column_constant(m, tail, monkeypatch):
    from attention import MSA
    torch.manual_seed(11 + m)
    msa = MSA(768, 12, type="cheby").to(DEV)
    with torch.no_grad():
        for _, lay in _layers(msa):
            lay.cheby_coeffs[:, :, 1:] = 0.0
    x = torch.randn(m, 768, device=DEV)
    w = torch.randn(m, 3 * 768, device=DEV)
    with _env(monkeypatch, KANVIT_TAIL=str(tail)) if tail else contextlib.nullcontext():
        y, _, grads = _qkv(msa, x, w)
    assert torch.equal(y, y[:1].expand_as(y))
    b = torch.cat([lay.cheby_coeffs[:, :, 0].double().sum(0) for _, lay in _layers(msa)])
    assert _rel(y[0], b) < REL
    _check_t0_rows(msa, w, grads)


@pytest.mark.parametrize("m,tail", QKV, ids=[f"M{m}-tail{t}" for m, t in QKV])
def test_qkv_register_kernels_match_lds_tile_kernels(m, tail, monkeypatch):
    from attention import MSA
    torch.manual_seed(23 + m)
    msa = MSA(768, 12, type="cheby").to(DEV)
    x = torch.randn(m, 768, device=DEV)
    w = torch.randn(m, 3 * 768, device=DEV)
    with _env(monkeypatch, KANVIT_TAIL=str(tail)) if tail else contextlib.nullcontext():
        y, dx, g = _qkv(msa, x, w)
        y2, dx2, g2 = _qkv(msa, x, w)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and all(torch.equal(g[k], g2[k]) for k in g)
    _check_t0_rows(msa, w, g)
    with _env(monkeypatch, KANVIT_NO_REG="1", KANVIT_NO_REG_BW="1"):
        yt, dxt, gt = _qkv(msa, x, w)
    assert _rel(y, yt) < REL and _rel(dx, dxt) < REL
    for k in g:
        assert _rel(g[k], gt[k]) < REL, k


def _vit():
    from model import VisionTransformer
    return VisionTransformer((3, 224, 224), 14, 1, 768, 12, 10, type="cheby").to(DEV)


def _embed(m, images, w, fused):
    m.zero_grad(set_to_none=True)
    m._fused_embed = None if fused else {False: False}
    out = m._embed_fused(images)
    if not fused:
        patches = m.patchify(images, m.n_patches)
        b, p, _ = patches.shape
        tok = m.linear_mapper(patches).reshape(b, p, m.d_hidden)
        out = torch.cat((m.v_class.unsqueeze(0).expand(b, -1, -1), tok), dim=1) + m.pos_embeddings[: p + 1]
    assert out is not None
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), m.linear_mapper.cheby_coeffs.grad.detach().clone()


def test_patch_embedding_t0_only_is_its_column_constant():
    torch.manual_seed(5)
    m = _vit()
    with torch.no_grad():
        m.linear_mapper.cheby_coeffs[:, :, 1:] = 0.0
        m.pos_embeddings.zero_()
    images = torch.rand(128, 3, 224, 224, device=DEV)
    w = torch.randn(128, 197, 768, device=DEV)
    tok, dw = _embed(m, images, w, fused=True)
    rows = tok[:, 1:].reshape(-1, 768)
    assert torch.equal(rows, rows[:1].expand_as(rows))
    assert _rel(rows[0], m.linear_mapper.cheby_coeffs[:, :, 0].double().sum(0)) < REL
    g0 = dw[:, :, 0]
    assert torch.equal(g0, g0[:1].expand_as(g0))
    assert _rel(g0[0], w[:, 1:].reshape(-1, 768).double().sum(0)) < REL


def test_patch_embedding_register_kernels_match_lds_tile_kernels(monkeypatch):
    torch.manual_seed(6)
    m = _vit()
    images = torch.rand(128, 3, 224, 224, device=DEV)
    w = torch.randn(128, 197, 768, device=DEV)
    tok, dw = _embed(m, images, w, fused=True)
    tok2, dw2 = _embed(m, images, w, fused=True)
    assert torch.equal(tok, tok2) and torch.equal(dw, dw2)
    g0 = dw[:, :, 0]
    assert torch.equal(g0, g0[:1].expand_as(g0))
    with _env(monkeypatch, KANVIT_NO_REG="1", KANVIT_NO_REG_BW="1"):
        tokt, dwt = _embed(m, images, w, fused=False)
    assert _rel(tok, tokt) < REL and _rel(dw, dwt) < REL
