"""KAN edge pruning on the GPU: kanvit_edge_select and kanvit_mask_rows against their NumPy restatements (ops.edge_select_ref,
ops.mask_rows_ref), bitwise; prune_edges of the three layer types against the restatement applied to the layer's own scores and
against a deep copy zeroed by torch indexing; MSA.prune_edges against per-layer calls on head slices; VisionTransformer.prune_edges
against the walk written out by hand."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- edge_select -------------------------------------------------------------------------------------------------------------------
# E = 1 (the one edge stays), a partial wave, under one lap, and 2 * 4096 + 37: the index-ordered pass walks laps of
# _lib.EDGE_SELECT_LAP = 4096 entries (1024 threads x 4) and the radix passes laps of 1024 -- the last lap of both is partial
SELECT_E = [1, 35, 2400, 2 * 4096 + 37]
VALUE_SETS = ["uniform", "four", "zeros", "lowbyte", "highbyte", "denormal"]


def _values(kind, groups, E, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((groups, E), dtype=np.float32)
    if kind == "four":                  # E // 2 lands inside a tie class
        return rng.choice(np.array([0.25, 0.5, 1.0, 2.0], dtype=np.float32), (groups, E))
    if kind == "zeros":                 # the first n_prune indices go
        return np.zeros((groups, E), dtype=np.float32)
    if kind == "lowbyte":               # keys that differ in their lowest byte only: the first three radix passes see one bucket
        return (np.uint32(0x3F123400) | rng.integers(0, 256, (groups, E), dtype=np.uint32)).view(np.float32)
    if kind == "highbyte":              # ... in their highest byte only (the exponent stays below 0xFF: finite)
        return ((rng.integers(0, 0x7F, (groups, E), dtype=np.uint32) << np.uint32(24)) | np.uint32(0x00345678)).view(np.float32)
    if kind == "denormal":              # denormals mixed with zeros
        v = rng.integers(1, 0x00800000, (groups, E), dtype=np.uint32)
        v[rng.random((groups, E)) < 0.5] = 0
        return v.view(np.float32)
    raise ValueError(kind)


def _check_select(a_np, A, mode, value):
    from kanvit import ops
    mask, kept = ops.edge_select(A, mode, value)
    want_mask, want_kept = ops.edge_select_ref(a_np, mode, value)
    assert mask.dtype == torch.uint8 and mask.shape == A.shape and kept.dtype == torch.int64 and tuple(kept.shape) == (A.shape[0],)
    assert np.array_equal(mask.cpu().numpy(), want_mask), (mode, value, int((mask.cpu().numpy() != want_mask).sum()))
    assert np.array_equal(kept.cpu().numpy(), want_kept), (mode, value)
    return mask


@pytest.mark.parametrize("kind", VALUE_SETS)
@pytest.mark.parametrize("E", SELECT_E)
@pytest.mark.parametrize("groups", [1, 6])
def test_edge_select_equals_the_restatement_bitwise(groups, E, kind):
    a = _values(kind, groups, E, 1000 * groups + E)
    A = torch.from_numpy(a).to(DEV)
    for n in sorted({0, 1, E // 2, E - 1} & set(range(E))):
        mask = _check_select(a, A, "count", n)
        assert int((mask == 0).sum()) == groups * n
        if kind == "zeros":
            assert bool((mask.view(groups, E)[:, :n] == 0).all()) and bool((mask.view(groups, E)[:, n:] == 1).all())
    flat = np.sort(a.reshape(-1))
    inside = float(flat[flat.size // 2])                             # a threshold that cuts inside the value range (an entry: >= keeps it)
    for t in (inside, 0.0):
        _check_select(a, A, "abs", t)
    for t in (0.5, 0.037, 0.0, 1.0):
        mask = _check_select(a, A, "rel", t)
        assert bool((mask.view(groups, E).sum(dim=1) >= 1).all())    # the maximum always stays
    assert bool(_check_select(a, A, "rel", 0.0).all())


def test_edge_select_a_group_does_not_depend_on_its_neighbours():
    from kanvit import ops
    a = _values("four", 6, 2400, 5)
    A = torch.from_numpy(a).to(DEV)
    for mode, value in (("count", 1200), ("rel", 0.5), ("abs", 0.5)):
        together, kept = ops.edge_select(A, mode, value)
        alone, kept1 = ops.edge_select(A[3:4].clone(), mode, value)
        assert torch.equal(together[3:4], alone) and torch.equal(kept[3:4], kept1)
    mask, kept = ops.edge_select(A[:0], "count", 0)                  # no groups: no launch
    assert tuple(mask.shape) == (0, 2400) and tuple(kept.shape) == (0,)


def test_edge_select_replayed_from_a_graph():
    from kanvit import ops
    a = [_values(kind, 6, 2400, 11) for kind in ("uniform", "four")]
    A = torch.from_numpy(a[0]).to(DEV)
    ops.edge_select(A, "count", 700)                                 # loads the library outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mask, kept = ops.edge_select(A, "count", 700)
    for k in (0, 1):
        A.copy_(torch.from_numpy(a[k]))
        graph.replay()
        want_mask, want_kept = ops.edge_select_ref(a[k], "count", 700)
        assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(kept.cpu().numpy(), want_kept), k


def test_edge_select_refuses_what_the_header_refuses():
    from kanvit import ops
    A = torch.rand(2, 35, device=DEV)
    for mode, value in (("count", 35), ("count", -1), ("abs", -1.0), ("abs", float("nan")), ("rel", 1.5), ("median", 0.5)):
        with pytest.raises(ops.KanvitError):
            ops.edge_select(A, mode, value)
    with pytest.raises(ops.KanvitError):
        ops.edge_select(A.double(), "count", 3)
    with pytest.raises(ops.KanvitError):
        ops.edge_select(A.t(), "count", 3)


# ---- mask_rows ---------------------------------------------------------------------------------------------------------------------
def _mask_case(rows, run, seed, offset=0):
    """(buffer, the tensor inside it `offset` elements in, mask): random values with NaN, infinities and -0 sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    n = rows * run
    buf = torch.randn(n + offset + 8, generator=g)
    special = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0])
    at = torch.randint(0, max(n, 1) + offset + 8, (max(n // 7, 4),), generator=g)
    buf[at] = special[torch.randint(0, 4, at.shape, generator=g)]
    mask = (torch.rand(rows, generator=g) < 0.5).to(torch.uint8)
    buf = buf.to(DEV)
    return buf, buf[offset:offset + n], mask.to(DEV)


def _check_masked(buf, x, mask, run, before, offset):
    from kanvit import ops
    n = x.numel()
    want = torch.from_numpy(ops.mask_rows_ref(before[offset:offset + n], mask, run)).view(torch.int32)
    assert torch.equal(_bits(x).cpu(), want)
    outside = torch.cat([_bits(buf)[:offset], _bits(buf)[offset + n:]]).cpu()
    assert torch.equal(outside, torch.cat([before.view(torch.int32)[:offset], before.view(torch.int32)[offset + n:]]))


@pytest.mark.parametrize("offset", [0, 1])                            # 16-byte aligned: the 16-byte form; one element in: the 4-byte form
@pytest.mark.parametrize("run", [1, 5, 8, 9])
def test_mask_rows_equals_the_restatement_bitwise(run, offset):
    from kanvit import _lib, ops
    chunk = _lib.MASK_CHUNK                                           # 4096 elements per work-group
    # shorter than a chunk; the first multiple of run at or above chunk + run (a row straddles the chunk boundary unless run
    # divides the chunk); several chunks with a partial last one
    for k, rows in enumerate((37, -(-(chunk + run) // run), (3 * chunk + 100) // run + 1)):
        buf, x, mask = _mask_case(rows, run, 100 * run + k, offset)
        assert x.data_ptr() % 16 == 4 * offset
        before = buf.cpu().clone()
        ops.mask_rows([x], [mask], [run])
        _check_masked(buf, x, mask, run, before, offset)
        ops.mask_rows([x], [mask], [run])                             # idempotent
        _check_masked(buf, x, mask, run, before, offset)


def test_mask_rows_both_forms_give_the_same_bits():
    from kanvit import ops
    for run in (5, 8):
        rows = 20000 // run
        buf0, x0, mask = _mask_case(rows, run, 3, 0)
        buf1 = torch.empty(x0.numel() + 1, device=DEV)
        x1 = buf1[1:]
        x1.copy_(x0)
        ops.mask_rows([x0, x1], [mask, mask], [run, run])
        assert _same_bits(x0, x1)


def test_mask_rows_many_tensors_an_empty_one_and_a_shared_mask():
    from kanvit import ops
    cap = ops.mask_max_tensors()
    cases = [_mask_case(3 + k % 5, (1, 5, 8, 9)[k % 4], k) for k in range(cap + 1)]           # cap + 1 tensors: two launches
    empty = torch.empty(0, device=DEV), torch.empty(0, dtype=torch.uint8, device=DEV)
    shared = _mask_case(40, 5, 777)                                   # one mask over a run-5 and a run-12 tensor
    other = torch.randn(40 * 12, device=DEV)
    tensors = [c[1] for c in cases[:7]] + [empty[0]] + [c[1] for c in cases[7:]] + [shared[1], other]
    masks = [c[2] for c in cases[:7]] + [empty[1]] + [c[2] for c in cases[7:]] + [shared[2], shared[2]]
    runs = [(1, 5, 8, 9)[k % 4] for k in range(7)] + [5] + [(1, 5, 8, 9)[k % 4] for k in range(7, cap + 1)] + [5, 12]
    befores = [t.cpu().clone() for t in tensors]
    ops.mask_rows(tensors, masks, runs)
    for t, m, r, b in zip(tensors, masks, runs, befores):
        assert torch.equal(_bits(t).cpu(), torch.from_numpy(ops.mask_rows_ref(b, m, r)).view(torch.int32).reshape(t.shape))
    ops.mask_rows([], [], [])                                         # nothing to do
    with pytest.raises(ops.KanvitError):
        ops.mask_rows([other], [shared[2]], [5])                      # 480 elements are not 40 rows of 5


# ---- layers ------------------------------------------------------------------------------------------------------------------------
def _layer(kind, i, o):
    from models.cheby import ChebyKANLayer
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    torch.manual_seed(17 * i + o)
    return {"efficientkan": lambda: KANLinear(i, o), "cheby": lambda: ChebyKANLayer(i, o, 4), "fast": lambda: FastKANLayer(i, o)}[kind]()


def _zero_by_indexing(layer, mask):
    """The restatement of the zeroing: torch indexing on every masked tensor seen as rows of `run`."""
    with torch.no_grad():
        for p, run in layer._edge_tensors():
            p.view(mask.numel(), run)[mask.reshape(-1) == 0] = 0.0


@pytest.mark.parametrize("how", [dict(fraction=0.5), dict(threshold=0.3), dict(threshold="median", relative=False)],
                         ids=["fraction", "relative", "absolute"])
@pytest.mark.parametrize("i,o", [(5, 7), (16, 16)])
@pytest.mark.parametrize("kind", ["efficientkan", "cheby", "fast"])
def test_layer_prune_edges(kind, i, o, how):
    from kanvit import ops, prune
    layer = _layer(kind, i, o).to(DEV)
    x = torch.randn(64, i, generator=torch.Generator().manual_seed(5)).to(DEV)
    keys = list(layer.state_dict())
    with torch.no_grad():
        scores = layer._edge_scores(x)                                # [out, in]: the layer's own edge_activation_l1, the base included
    assert tuple(scores.shape) == (o, i)
    if how.get("threshold") == "median":                              # an absolute threshold that cuts inside the layer's own scores
        how = dict(how, threshold=float(scores.flatten().sort().values[i * o // 2]))
    mode, value = prune.select_args(i * o, how.get("fraction"), how.get("threshold"), how.get("relative", True))
    want, _ = ops.edge_select_ref(scores.t().contiguous().cpu().view(1, i * o), mode, value)
    want = torch.from_numpy(want).view(i, o)
    want = want if kind == "cheby" else want.t()                      # the mask lives in the masked tensors' leading layout
    twin = copy.deepcopy(layer)
    before = [p.detach().clone() for p, _ in layer._edge_tensors()]

    kept = layer.prune_edges(x, **how)
    assert kept.dim() == 0 and kept.is_cuda and int(kept) == int(want.sum())
    if "fraction" in how:
        assert int(kept) == i * o - int(how["fraction"] * i * o)
    assert 0 < int(kept) < i * o, "the case prunes something and keeps something"
    assert layer.edge_mask.dtype == torch.uint8 and torch.equal(layer.edge_mask.cpu(), want.contiguous())
    assert list(layer.state_dict()) == keys
    for (p, run), b in zip(layer._edge_tensors(), before):
        rows, dead = p.detach().view(-1, run), (layer.edge_mask.reshape(-1) == 0)
        assert bool((_bits(rows)[dead] == 0).all())                  # +0.0 exactly
        assert torch.equal(_bits(rows)[~dead], _bits(b.view(-1, run))[~dead])       # kept runs: the same bits
    _zero_by_indexing(twin, want.to(DEV))
    with torch.no_grad():
        assert _same_bits(layer(x), twin(x))

    first = layer.edge_mask.clone()
    kept2 = layer.prune_edges(x, fraction=0.75)                       # cumulative: pruned edges score 0 and rank first
    assert bool((layer.edge_mask <= first).all()) and int(kept2) == int(layer.edge_mask.sum())       # a superset is pruned
    # 0.75 is the share of ALL edges: a threshold that already pruned more leaves nothing to add
    assert int(kept2) == min(int(kept), i * o - int(0.75 * i * o))

    fresh = _layer(kind, i, o)
    fresh.load_state_dict(layer.state_dict())
    fresh = fresh.to(DEV)
    assert int(fresh.restore_edge_mask()) == int(kept2) and torch.equal(fresh.edge_mask, layer.edge_mask)


def test_prune_edges_argument_refusals():
    layer = _layer("cheby", 5, 7).to(DEV)
    x = torch.randn(8, 5, device=DEV)
    for bad in (dict(), dict(fraction=0.5, threshold=0.5), dict(fraction=1.5), dict(threshold=2.0)):
        with pytest.raises(ValueError):
            layer.prune_edges(x, **bad)
    assert int(layer.prune_edges(x, fraction=1.0)) == 1               # the strongest edge stays


# ---- MSA and the model -------------------------------------------------------------------------------------------------------------
def _state_bits_equal(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert _same_bits(sa[k], sb[k]), k


@pytest.mark.parametrize("how", [dict(fraction=0.5), dict(threshold=0.3)], ids=["fraction", "relative"])
@pytest.mark.parametrize("kind", ["efficientkan", "cheby", "fast"])
def test_msa_prune_edges_equals_the_per_layer_calls(kind, how):
    from attention import MSA
    torch.manual_seed(3)
    msa = MSA(16, 2, type=kind).to(DEV)
    twin = copy.deepcopy(msa)
    x = torch.randn(4, 16, 16, generator=torch.Generator().manual_seed(6)).to(DEV)
    kept = msa.prune_edges(x, **how)
    layers, twins = msa._qkv_layers()[0], twin._qkv_layers()[0]
    total = 0
    for g, m in enumerate(twins):
        h = g % 2
        total += int(m.prune_edges(x.reshape(-1, 16)[:, 8 * h:8 * h + 8].contiguous(), **how))
    assert kept.dim() == 0 and int(kept) == total
    if "fraction" in how:
        assert total == 6 * (64 - 32)
    for a, b in zip(layers, twins):
        assert torch.equal(a.edge_mask, b.edge_mask)
    _state_bits_equal(msa, twin)
    assert len(msa.edge_masked()) == sum(len(m.edge_masked()) for m in layers)


def test_msa_prune_edges_refuses_other_types():
    from attention import MSA
    x = torch.randn(2, 4, 16, device=DEV)
    for kind in ("sine", "vanilla"):
        with pytest.raises(NotImplementedError, match="supported MSA types"):
            MSA(16, 2, type=kind).to(DEV).prune_edges(x, fraction=0.5)
    msa = MSA(16, 2, type="efficientkan").to(DEV)
    msa.q_mappings[0].base_activation = torch.nn.GELU()
    with pytest.raises(NotImplementedError, match="one base activation"):
        msa.prune_edges(x, fraction=0.5)


@pytest.mark.parametrize("kind", ["efficientkan", "cheby", "fast"])
def test_vision_transformer_prune_edges_equals_the_walk_by_hand(kind):
    from model import VisionTransformer
    torch.manual_seed(4)
    model = VisionTransformer((3, 8, 8), n_patches=2, n_blocks=2, d_hidden=16, n_heads=2, out_d=10, type=kind).to(DEV)
    model.set_drop_path(0.2, seed=1)                                  # neither takes part in the walk, neither counter moves
    model.set_patch_dropout(0.5, seed=1)
    model.train()
    twin = copy.deepcopy(model)
    images = torch.randn(16, 3, 8, 8, generator=torch.Generator().manual_seed(8)).to(DEV)
    keys = list(model.state_dict())
    kept0, total0 = (int(v) for v in model.edge_sparsity())
    assert kept0 == total0 == 48 * 16 + 2 * 6 * 64
    got = model.prune_edges(images, fraction=0.5)
    assert int(model.drop_path_counter) == 0 and int(model.patch_dropout_counter) == 0

    with torch.no_grad():                                             # the walk, written out
        want = [(int(twin.linear_mapper.prune_edges(twin.patchify(images, 2).reshape(-1, 48), fraction=0.5)), 48 * 16)]
        out = twin._embed(images)
        for l, blk in enumerate(twin.blocks):
            want.append((int(blk.attn.prune_edges(blk.norm1(out), fraction=0.5)), 6 * 64))
            if l == 0:
                out = blk(out)
    assert [(int(k), int(t)) for k, t in got] == want and all(k.is_cuda and t.is_cuda for k, t in got)
    assert want == [(48 * 16 - int(0.5 * 48 * 16), 48 * 16)] + [(6 * 32, 6 * 64)] * 2
    _state_bits_equal(model, twin)
    assert list(model.state_dict()) == keys
    kept1, total1 = model.edge_sparsity()
    assert kept1.is_cuda and (int(kept1), int(total1)) == (sum(k for k, _ in want), total0)
    triples = model.edge_masked()
    assert len(triples) == len(twin.edge_masked()) and all(m.dtype == torch.uint8 and p.numel() == m.numel() * r for p, m, r in triples)

    fresh = VisionTransformer((3, 8, 8), n_patches=2, n_blocks=2, d_hidden=16, n_heads=2, out_d=10, type=kind)
    fresh.load_state_dict(model.state_dict())
    fresh = fresh.to(DEV)
    assert int(fresh.restore_edge_masks()) == int(kept1)
    for (_, a, _), (_, b, _) in zip(fresh.edge_masked(), triples):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["sine", "fourier", "vanilla"])
def test_vision_transformer_refuses_other_types_by_name(kind):
    from model import VisionTransformer
    model = VisionTransformer((3, 8, 8), n_patches=2, n_blocks=1, d_hidden=16, n_heads=2, out_d=10, type=kind).to(DEV)
    with pytest.raises(NotImplementedError, match=kind):
        model.prune_edges(torch.randn(2, 3, 8, 8, device=DEV), fraction=0.5)
    with pytest.raises(NotImplementedError, match=kind):
        model.edge_masked()
