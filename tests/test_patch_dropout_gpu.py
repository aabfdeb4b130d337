"""PatchDropout on the GPU: kanvit_patch_keep against its Python restatement (bitwise; the counter walk, also from a captured graph),
kanvit_patch_gather against torch.gather on the patch matrix and kanvit_tokens_assemble_* against cat + indexed add (bitwise; the
class-token gradient within the bound of any fp32 summation order and reproducible), VisionTransformer.set_patch_dropout against the
same model with the embedding restated in stock torch ops on patch_keep_ref's table, and train.py's captured step."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- patch_keep -----------------------------------------------------------------------------------------------------------------------
# one thread's worth, a partial wave, more samples than the launch has work-groups (128), every patch kept, the LDS cap at both ends of K
KEEP_SHAPES = [(1, 1, 1), (3, 16, 8), (5, 49, 13), (130, 196, 98), (4, 196, 196), (2, 1024, 1), (2, 1024, 1023)]
_ref_tables = {}


def _ref(B, P, K, seed, c):
    key = (B, P, K, seed, c)
    if key not in _ref_tables:
        from kanvit import ops
        _ref_tables[key] = ops.patch_keep_ref(B, P, K, seed, c)
    return _ref_tables[key]


@pytest.mark.parametrize("B,P,K", KEEP_SHAPES)
def test_patch_keep_equals_the_restatement_bitwise(B, P, K):
    from kanvit import ops
    seed, c = 12345 + B, 7
    counter = torch.full((1,), c, dtype=torch.int64, device=DEV)
    got = ops.patch_keep(B, P, K, seed, counter)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, K)
    assert int(counter) == c + 1                                     # bumped exactly once, the ticket bits back at zero
    assert torch.equal(got.cpu(), _ref(B, P, K, seed, c))
    if K == P:
        assert torch.equal(got.cpu(), torch.arange(P, dtype=torch.int32).expand(B, P))
    out = torch.empty(B, K, dtype=torch.int32, device=DEV)
    assert ops.patch_keep(B, P, K, seed, counter, out=out) is out and int(counter) == c + 2
    if B * P <= 1024:                                                # the next counter's table: once, on the small shapes
        assert torch.equal(out.cpu(), _ref(B, P, K, seed, c + 1))
    assert tuple(ops.patch_keep(0, P, K, seed, counter).shape) == (0, K) and int(counter) == c + 2      # B = 0 leaves the counter alone


def test_patch_keep_replayed_from_a_graph_walks_the_counter():
    from kanvit import ops
    B, P, K, seed, c = 130, 49, 24, 99, 7
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.empty(B, K, dtype=torch.int32, device=DEV)
    ops.patch_keep(B, P, K, seed, counter, out=out)                  # loads the library outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.patch_keep(B, P, K, seed, counter, out=out)
    counter.fill_(c)
    for k in range(3):
        graph.replay()
        assert torch.equal(out.cpu(), _ref(B, P, K, seed, c + k)), k
    assert int(counter) == c + 3


# ---- patch_gather ----------------------------------------------------------------------------------------------------------------------
# (2,3,30,42,6,17): 5 x 7 patches, I = 105, rows that are no 16-byte multiples (the scalar form); the others take float4
GATHER_SHAPES = [(2, 1, 28, 28, 7, 20), (3, 3, 32, 32, 4, 8), (2, 3, 30, 42, 6, 17), (2, 3, 224, 224, 14, 98)]


def _gather_ref(images, idx, n):
    from kanvit import ops
    patches = ops.patchify(images, n)
    return torch.gather(patches, 1, idx.long().unsqueeze(-1).expand(-1, -1, patches.shape[-1])).reshape(-1, patches.shape[-1])


@pytest.mark.parametrize("B,C,H,W,n,K", GATHER_SHAPES)
def test_patch_gather_equals_torch_gather_on_the_patch_matrix(B, C, H, W, n, K):
    from kanvit import ops
    g = torch.Generator().manual_seed(B + H + K)
    images = torch.randn(B, C, H, W, generator=g).to(DEV)
    P = n * n
    idx = torch.stack([torch.randperm(P, generator=g)[:K].sort().values for _ in range(B)]).int().to(DEV)
    rows = ops.patch_gather(images, idx, n)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (B * K, C * (H // n) * (W // n)) and not rows.requires_grad
    assert torch.equal(rows, _gather_ref(images, idx, n))
    # unsorted, with repeats: the kernel may not assume patch_keep's order
    wild = torch.randint(0, P, (B, K), generator=g).int().to(DEV)
    wild[:, -1] = wild[:, 0]
    assert torch.equal(ops.patch_gather(images, wild, n), _gather_ref(images, wild, n))
    # images one float past a 16-byte boundary: the scalar form on a geometry that otherwise takes float4
    buf = torch.empty(images.numel() + 1, device=DEV)
    view = buf[1:].view_as(images).copy_(images)
    assert view.data_ptr() % 16 == 4 and torch.equal(ops.patch_gather(view, idx, n), _gather_ref(images, idx, n))
    # every patch, in order: patchify
    everything = torch.arange(P, dtype=torch.int32, device=DEV).expand(B, P).contiguous()
    assert torch.equal(ops.patch_gather(images, everything, n), ops.patchify(images, n).reshape(B * P, -1))


# ---- assemble_tokens --------------------------------------------------------------------------------------------------------------------
# (2, 5, 30): a width that is no multiple of 4 (the scalar form); (130, 98, 768): more rows than one lap of the grid
ASSEMBLE_SHAPES = [(1, 1, 32), (3, 8, 64), (5, 13, 260), (2, 5, 30), (130, 98, 768)]


def _assemble_operands(B, K, O):
    g = torch.Generator().manual_seed(B * 3 + K + O)
    P = 2 * K + 3
    tokens = torch.randn(B * K, O, generator=g).to(DEV)
    cls, pos = torch.randn(1, O, generator=g).to(DEV), torch.randn(P + 1, O, generator=g).to(DEV)
    idx = torch.stack([torch.randperm(P, generator=g)[:K].sort().values for _ in range(B)]).int().to(DEV)
    return tokens, cls, pos, idx


def _assemble_ref(tokens, cls, pos, idx):
    B, K = idx.shape
    where = torch.cat((torch.zeros(B, 1, dtype=torch.int64, device=idx.device), 1 + idx.long()), dim=1)
    return torch.cat((cls.reshape(1, 1, -1).expand(B, -1, -1), tokens.reshape(B, K, -1)), dim=1) + pos[where]


@pytest.mark.parametrize("B,K,O", ASSEMBLE_SHAPES)
def test_assemble_tokens_forward_equals_cat_and_indexed_add(B, K, O):
    from kanvit import ops
    tokens, cls, pos, idx = _assemble_operands(B, K, O)
    want = _assemble_ref(tokens, cls, pos, idx)
    out = ops.assemble_tokens(tokens, cls, pos, idx)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, K + 1, O) and out.is_contiguous()
    assert torch.equal(out, want)
    assert torch.equal(ops.assemble_tokens(tokens.view(B, K, O), cls.reshape(-1), pos, idx), want)
    # a (B*K, O) matrix inside wider rows is read in place, vector-aligned (pad 4) and not (pad 3)
    for pad in (4, 3):
        wide = torch.zeros(B * K, O + pad, device=DEV)
        wide[:, :O] = tokens
        assert wide[:, :O].stride(0) == O + pad and torch.equal(ops.assemble_tokens(wide[:, :O], cls, pos, idx), want)


@pytest.mark.parametrize("B,K,O", ASSEMBLE_SHAPES)
def test_assemble_tokens_backward(B, K, O):
    from kanvit import ops
    tokens, cls, pos, idx = _assemble_operands(B, K, O)
    dout = torch.randn(B, K + 1, O, generator=torch.Generator().manual_seed(O)).to(DEV)
    runs = []
    for _ in range(2):
        t, c = tokens.clone().requires_grad_(True), cls.clone().requires_grad_(True)
        ops.assemble_tokens(t, c, pos, idx).backward(dout)
        runs.append((t.grad, c.grad))
    dtokens, dcls = runs[0]
    assert tuple(dtokens.shape) == (B * K, O) and tuple(dcls.shape) == (1, O)
    assert torch.equal(dtokens, dout[:, 1:, :].reshape(B * K, O))                  # bitwise the slice
    rows = dout[:, 0, :].double()
    err = (dcls.double().reshape(-1) - rows.sum(0)).abs()
    bound = B * 2.0 ** -24 * rows.abs().sum(0)                                      # any fp32 summation order of B terms
    print(f"{(B, K, O)}: worst dcls error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(runs[1][1], dcls) and torch.equal(runs[1][0], dtokens)       # bitwise the same from run to run
    # only one of the two gradients wanted
    t = tokens.clone().requires_grad_(True)
    ops.assemble_tokens(t, cls, pos, idx).backward(dout)
    assert torch.equal(t.grad, dtokens)
    c = cls.clone().requires_grad_(True)
    ops.assemble_tokens(tokens, c, pos, idx).backward(dout)
    assert torch.equal(c.grad, dcls)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
LOOSE = 1e-2          # tests/test_bf16_oracle_gpu.py: ||err||_F / ||ref||_F; model outputs are held to 2 * LOOSE there


def fro(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


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


def _restated_embed(seen):
    """VisionTransformer._embed_kept in stock torch ops on patch_keep_ref's table: patchify -> index -> linear_mapper -> cat -> + pos[...]."""
    def embed(self, images):
        from kanvit import ops
        K, seed = self._patch_dropout
        B, P = images.shape[0], self.n_patches ** 2
        idx = ops.patch_keep_ref(B, P, K, seed, int(self.patch_dropout_counter)).to(images.device).long()
        self.patch_dropout_counter.add_(1)
        rows = ops.patchify(images, self.n_patches)[torch.arange(B, device=images.device)[:, None], idx].reshape(B * K, -1)
        tokens = self.linear_mapper(rows).float().reshape(B, K, self.d_hidden)
        where = torch.cat((torch.zeros(B, 1, dtype=torch.int64, device=images.device), 1 + idx), dim=1)
        out = torch.cat((self.v_class.unsqueeze(0).expand(B, -1, -1), tokens), dim=1) + self.pos_embeddings[where]
        if out.requires_grad:
            out.register_hook(lambda g: seen.append(g.detach().clone()))
        return out, rows
    return embed


# the geometries of tests/test_drop_path_gpu.py: small ones (the fallback route) and one that takes the class-token tail
MODELS = [("cheby", 64, 4), ("efficientkan", 64, 4), ("fast", 64, 4), ("vanilla", 64, 4), ("cheby,efficientkan", 64, 4), ("cheby", 384, 6)]


@pytest.mark.parametrize("kind,d,heads", MODELS)
def test_model_against_the_embedding_restated_in_torch(kind, d, heads, monkeypatch):
    import model
    from kanvit.dense import ff_small_supported
    assert ff_small_supported(d, 4 * d) == (d == 64)
    m = _vit(kind, d, heads).train()
    x, labels = _batch()
    B = x.shape[0]
    K = m.set_patch_dropout(0.5, seed=3)
    assert K == 8
    shapes = []
    run = m.blocks[0].run
    m.blocks[0].run = lambda out, *a, **kw: (shapes.append(tuple(out.shape)), run(out, *a, **kw))[1]
    logits, grads = _pass(m, x, labels)
    assert shapes == [(B, K + 1, d)] and int(m.patch_dropout_counter) == 1

    m.patch_dropout_counter.zero_()                                    # the same keep sets
    douts = []
    monkeypatch.setattr(model.VisionTransformer, "_embed_kept", _restated_embed(douts))
    logits0, grads0 = _pass(m, x, labels)
    assert shapes[1:] == [(B, K + 1, d)] and len(douts) == 1
    assert torch.equal(logits, logits0)
    assert set(grads) == set(grads0) and len(grads) > 10
    for k in grads:
        if k != "v_class":
            assert torch.equal(grads[k], grads0[k]), (kind, k, float((grads[k] - grads0[k]).abs().max()))
    rows = douts[0][:, 0, :].double()
    bound = B * 2.0 ** -24 * rows.abs().sum(0)
    for g in (grads["v_class"], grads0["v_class"]):
        assert bool(((g.double().reshape(-1) - rows.sum(0)).abs() <= bound).all())


@pytest.mark.parametrize("kind,d,heads", [MODELS[0], MODELS[-1]])
def test_eval_ignores_it_and_seeds_decide_the_sets(kind, d, heads):
    x, _ = _batch()
    plain = _vit(kind, d, heads)
    a, b, c = (copy.deepcopy(plain) for _ in range(3))
    a.set_patch_dropout(0.5, seed=3), b.set_patch_dropout(0.5, seed=3), c.set_patch_dropout(0.5, seed=4)
    with torch.no_grad():
        assert torch.equal(a.eval()(x), plain.eval()(x))
        assert int(a.patch_dropout_counter) == 0
        assert tuple(a.attention_maps(x).shape[-2:]) == (17, 17)         # the helpers use the full sequence
        a.train(), b.train(), c.train(), plain.train()
        assert tuple(a.attention_maps(x).shape[-2:]) == (17, 17) and int(a.patch_dropout_counter) == 0
        steps = [(a(x), b(x), c(x)) for _ in range(3)]
        assert all(torch.equal(ya, yb) for ya, yb, _ in steps)
        assert not any(torch.equal(ya, yc) for ya, _, yc in steps)
        assert not torch.equal(steps[0][0], steps[1][0])                 # the counter moves the sets from step to step
        assert not torch.equal(steps[0][0], plain(x))
        a.patch_dropout_counter.zero_()
        assert torch.equal(a(x), steps[0][0])                            # the same seed with the counter put back
        a.set_patch_dropout(0.0)
        assert torch.equal(a(x), plain(x))


def test_images_that_want_a_gradient_take_the_torch_path():
    x, labels = _batch()
    m = _vit("cheby").train()
    K = m.set_patch_dropout(0.5, seed=3)
    logits = m(x)
    m.patch_dropout_counter.zero_()
    xg = x.clone().requires_grad_(True)
    logits_g = m(xg)
    assert torch.equal(logits_g, logits)
    torch.nn.functional.cross_entropy(logits_g, labels).backward()
    touched = (m.patchify(xg.grad, 4).abs().sum(-1) != 0).sum(1)         # per sample: patches with a gradient
    assert bool(torch.isfinite(xg.grad).all()) and bool((touched == K).all())


@pytest.mark.parametrize("kind", ["cheby", "flash-attn"])
def test_composition_with_drop_path_and_the_regulariser(kind):
    x, labels = _batch()
    m = _vit(kind).train()
    m.set_patch_dropout(0.5, seed=3)
    if kind == "cheby":
        m.set_drop_path(0.1, seed=3)
        logits, reg = m(x, return_regularization=True)
        loss = torch.nn.functional.cross_entropy(logits, labels) + 1e-3 * reg
    else:
        loss = torch.nn.functional.cross_entropy(m(x), labels)
    loss.backward()
    assert bool(torch.isfinite(loss))
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) > 5 and all(bool(torch.isfinite(g).all()) for g in grads)
    assert int(m.patch_dropout_counter) == 1


@pytest.mark.parametrize("kind", ["cheby", "vanilla"])
def test_bf16_autocast_step(kind, monkeypatch):
    """One step under bf16 autocast against the same step with the torch-restated embedding, at the bound tests/test_bf16_oracle_gpu.py
    applies to model outputs (2 * LOOSE in the Frobenius norm).  nn.Linear's bf16 tokens are widened before the sequence is assembled."""
    import model
    x, labels = _batch()
    m = _vit(kind).train()
    m.set_patch_dropout(0.5, seed=3)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits, grads = _pass(m, x, labels)
    m.patch_dropout_counter.zero_()
    monkeypatch.setattr(model.VisionTransformer, "_embed_kept", _restated_embed([]))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits0, grads0 = _pass(m, x, labels)
    print(f"{kind}: logits {fro(logits.float(), logits0.float()):.2e}, worst gradient {max(fro(grads[k], grads0[k]) for k in grads):.2e}")
    assert bool(torch.isfinite(logits).all()) and fro(logits.float(), logits0.float()) < 2 * LOOSE
    for k in grads:
        assert fro(grads[k], grads0[k]) < 2 * LOOSE, k


def test_graphed_train_step_equals_the_eager_one(tmp_path):
    """train.py --graph: the throw-away step in front of the capture must not use up a keep set (_GraphedStep puts the counter back), and
    every replay draws a new one."""
    import train
    flags = ["--model-type", "cheby", "--epochs", "1", "--steps-per-epoch", "3", "--synthetic", "--no-step-metrics", "--n-blocks", "2",
             "--batch-size", "16", "--out-d", "10", "--seed", "7"]
    eager = train.main(train.parse([*flags, "--patch-dropout", "0.5", "--log-dir", str(tmp_path / "e")]))
    graphed = train.main(train.parse([*flags, "--patch-dropout", "0.5", "--graph", "--log-dir", str(tmp_path / "g")]))
    plain = train.main(train.parse([*flags, "--log-dir", str(tmp_path / "p")]))
    print("eager", eager["losses"], "graphed", graphed["losses"], "without", plain["losses"])
    assert len(eager["losses"]) == 3 and eager["losses"] == graphed["losses"]
    assert int(graphed["model"].patch_dropout_counter) == 3 and int(eager["model"].patch_dropout_counter) == 3
    assert eager["losses"] != plain["losses"] and not hasattr(plain["model"], "patch_dropout_counter")
    we, wg = eager["model"].state_dict(), graphed["model"].state_dict()
    assert list(we) == list(wg) and all(torch.equal(we[k], wg[k]) for k in we)
