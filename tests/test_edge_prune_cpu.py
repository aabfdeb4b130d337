"""CPU-only checks of KAN edge pruning: the properties of the NumPy restatements the GPU tests compare the kernels with, the two
entry points' refusals (before any device call), their exports, the code-object metadata of the two kernels, and --prune parsing."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRUNE_SYMBOLS = {"kanvit_edge_select", "kanvit_mask_max_tensors", "kanvit_mask_rows"}


@pytest.fixture(scope="module")
def lib():
    from kanvit import build
    build.build(verbose=False)
    from kanvit import _lib
    return _lib.lib()


def _keys(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def _value_sets(E, rng):
    yield "uniform", rng.random(E, dtype=np.float32)
    yield "four values", rng.choice(np.array([0.25, 0.5, 1.0, 2.0], dtype=np.float32), E)
    yield "zeros", np.zeros(E, dtype=np.float32)
    yield "signs and a NaN", np.concatenate([rng.standard_normal(E - 1).astype(np.float32), np.array([np.nan], dtype=np.float32)])


@pytest.mark.parametrize("E", [1, 2, 35, 600])
def test_count_restatement_prunes_exactly_the_n_smallest_pairs(E):
    from kanvit import ops
    rng = np.random.default_rng(E)
    for name, a in _value_sets(E, rng):
        keys = _keys(a).astype(np.int64)
        for n in sorted({0, 1, E // 2, E - 1} & set(range(E))):
            mask, kept = ops.edge_select_ref(a[None], "count", n)
            assert mask.dtype == np.uint8 and mask.shape == (1, E) and kept.dtype == np.int64
            assert int((mask == 0).sum()) == n and int(kept[0]) == E - n, (name, n)
            # every pruned (key, index) pair lies below every kept one in the total order
            pair = keys * E + np.arange(E)
            pruned, stay = pair[mask[0] == 0], pair[mask[0] == 1]
            assert pruned.size == 0 or pruned.max() < stay.min(), (name, n)
    with pytest.raises(ops.KanvitError):
        ops.edge_select_ref(np.zeros((1, E), dtype=np.float32), "count", E)        # the strongest edge always stays


def test_threshold_restatements():
    from kanvit import ops
    a = np.array([[3.0, 1.0, 1.0, 0.0, 1.5, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    mask, kept = ops.edge_select_ref(a, "rel", 1.0)                # threshold 1 keeps only the maxima (all of them: no tie-break)
    assert mask.tolist() == [[1, 0, 0, 0, 0, 1], [1, 1, 1, 1, 1, 1]] and kept.tolist() == [2, 6]
    mask, kept = ops.edge_select_ref(a, "rel", 0.5)                # t_g = 1.5: >= keeps the entry at the threshold
    assert mask.tolist() == [[1, 0, 0, 0, 1, 1], [1, 1, 1, 1, 1, 1]]
    mask, kept = ops.edge_select_ref(a, "abs", 1.0)
    assert mask.tolist() == [[1, 1, 1, 0, 1, 1], [0, 0, 0, 0, 0, 0]] and kept.tolist() == [5, 0]
    assert ops.edge_select_ref(a, "abs", 0.0)[0].all() and ops.edge_select_ref(a, "rel", 0.0)[0].all()
    # one fp32 rounding of threshold * max: 0.1f * 3.0f in float32, not in float64
    t = np.float32(np.float32(0.1) * np.float32(3.0))
    b = np.array([[3.0, t, np.nextafter(t, np.float32(0))]], dtype=np.float32)
    assert ops.edge_select_ref(b, "rel", 0.1)[0].tolist() == [[1, 1, 0]]
    # a group's answer does not depend on its neighbours
    assert (ops.edge_select_ref(a[1:], "rel", 0.5)[0] == ops.edge_select_ref(a, "rel", 0.5)[0][1:]).all()
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ops.KanvitError):
            ops.edge_select_ref(a, "abs", bad)
    with pytest.raises(ops.KanvitError):
        ops.edge_select_ref(a, "rel", 1.5)


def test_mask_rows_restatement_is_a_select():
    from kanvit import ops
    x = np.array([np.nan, -0.0, 1.0, -2.0, np.inf, 5.0, -np.inf, np.nan], dtype=np.float32)
    out = ops.mask_rows_ref(x, np.array([0, 1, 0, 1], dtype=np.uint8), 2)
    want = x.copy().view(np.uint32)
    want[[0, 1, 4, 5]] = 0                                         # +0.0, whatever was there; kept elements keep their bits (the NaN's too)
    assert (out.view(np.uint32) == want).all() and (x.view(np.uint32)[:2] != 0).any()      # a new array: x is untouched
    assert ops.mask_rows_ref(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint8), 3).shape == (0,)


def test_exports_and_signatures(lib):
    from kanvit import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kanvit.h")).read(), flags=re.S)
    declared = {n for n in re.findall(r"\b(kanvit_[a-z0-9_]+)\s*\(", header) if "edge_select" in n or "_mask_" in n}
    assert declared == PRUNE_SYMBOLS
    raw = C.CDLL(_lib.LIB_PATH)
    for name in PRUNE_SYMBOLS:
        assert hasattr(raw, name) and name in _lib.SYMBOLS, name
    P = C.c_void_p
    assert _lib.SYMBOLS["kanvit_edge_select"] == (C.c_int, [P, C.c_int64, C.c_int64, C.c_int, C.c_float, C.c_int64, P, P, P])
    assert _lib.SYMBOLS["kanvit_mask_rows"] == (C.c_int, [C.c_int, P, P, P, P, P])
    assert lib.kanvit_abi_version() == 7
    for macro, value in (("KANVIT_PRUNE_COUNT", _lib.PRUNE_COUNT), ("KANVIT_PRUNE_ABS", _lib.PRUNE_ABS), ("KANVIT_PRUNE_REL", _lib.PRUNE_REL),
                         ("KANVIT_EDGE_SELECT_LAP", _lib.EDGE_SELECT_LAP), ("KANVIT_MASK_CHUNK", _lib.MASK_CHUNK),
                         ("KANVIT_MASK_MAX_TENSORS", lib.kanvit_mask_max_tensors())):
        assert re.search(rf"#define {macro} {value}\b", header), macro


def test_entry_points_validate_arguments_without_a_gpu(lib):
    """KANVIT_EINVAL with a message, before any device call; the pointers of a refused call are never dereferenced."""
    from kanvit import _lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    select = lib.kanvit_edge_select
    cases = [(None, 1, 8, 0, 0.0, 1, p, p), (p, 1, 8, 0, 0.0, 1, None, p), (p, 1, 8, 0, 0.0, 1, p, None),      # null pointers
             (p, 1, 8, 3, 0.0, 1, p, p), (p, 1, 8, -1, 0.0, 1, p, p),                                         # unknown mode
             (p, 1, 0, 0, 0.0, 0, p, p), (p, -1, 8, 0, 0.0, 1, p, p),                                         # E < 1, groups < 0
             (p, 1, 8, 0, 0.0, 8, p, p), (p, 1, 8, 0, 0.0, -1, p, p), (p, 1, 1, 0, 0.0, 1, p, p),             # n_prune outside 0..E-1
             (p, 1, 8, 1, float("nan"), 0, p, p), (p, 1, 8, 1, -1.0, 0, p, p), (p, 1, 8, 1, float("inf"), 0, p, p),
             (p, 1, 8, 2, float("nan"), 0, p, p), (p, 1, 8, 2, -0.25, 0, p, p), (p, 1, 8, 2, 1.5, 0, p, p)]
    for args in cases:
        assert select(*args, None) == -22, args
        assert b"kanvit_edge_select" in lib.kanvit_last_error(), args
    assert select(p, 0, 8, 0, 0.0, 1, p, p, None) == 0               # no groups: nothing to launch
    assert select(p, 0, 8, 2, 1.0, 0, p, p, None) == 0

    rows = lib.kanvit_mask_rows
    cap = lib.kanvit_mask_max_tensors()
    assert cap == 80

    def call(n, tensors, numel, run, masks):
        arr = lambda v: None if v is None else (C.c_void_p * len(v))(*v)
        i64 = lambda v: None if v is None else (C.c_int64 * len(v))(*v)
        return rows(n, arr(tensors), i64(numel), i64(run), arr(masks), None)
    a = p.value
    bad = [(1, None, [8], [2], [a]), (1, [a], None, [2], [a]), (1, [a], [8], None, [a]), (1, [a], [8], [2], None),      # null arrays
           (1, [None], [8], [2], [a]), (1, [a], [8], [2], [None]),                                                 # null pointers
           (1, [a], [8], [0], [a]), (1, [a], [8], [-2], [a]), (1, [a], [8], [3], [a]), (1, [a], [-4], [2], [a]),      # run / numel
           (1, [a + 2], [8], [2], [a]),                                                                            # off 4-byte alignment
           (-1, [a], [8], [2], [a]), (cap + 1, [a] * (cap + 1), [8] * (cap + 1), [2] * (cap + 1), [a] * (cap + 1))]
    for args in bad:
        assert call(*args) == -22, args
        assert b"kanvit_mask_rows" in lib.kanvit_last_error(), args
    assert call(0, None, None, None, None) == 0                      # no tensors: nothing to launch
    assert call(2, [None, None], [0, 0], [5, 1], [None, None]) == 0  # tensors without elements get no work-group


def test_new_kernels_use_no_scratch_and_spill_no_vgpr(lib):
    pytest.importorskip("msgpack")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_meta
    finally:
        sys.path.pop(0)
    from kanvit import _lib
    ks = {n: k for n, k in kernel_meta.kernels(_lib.LIB_PATH).items() if "edge_select_kernel" in n or "mask_rows_kernel" in n}
    assert len(ks) == 2, sorted(ks)
    for n, k in ks.items():
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k[".vgpr_spill_count"] == 0, (n, k[".vgpr_spill_count"])


def test_ops_have_no_cpu_fallback():
    from kanvit import ops
    from models.cheby import ChebyKANLayer
    with pytest.raises(ops.KanvitError):
        ops.edge_select(torch.rand(1, 8), "count", 3)
    with pytest.raises(ops.KanvitError):
        ops.mask_rows([torch.rand(8)], [torch.ones(4, dtype=torch.uint8)], [2])
    with pytest.raises(ops.KanvitError):
        ChebyKANLayer(4, 3, 4).prune_edges(torch.randn(5, 4), fraction=0.5)


def test_prune_edges_takes_exactly_one_of_fraction_and_threshold():
    from kanvit import prune
    assert prune.select_args(35, 0.5, None, True) == ("count", 17)
    assert prune.select_args(35, 1.0, None, True) == ("count", 34)           # capped: the strongest edge stays
    assert prune.select_args(35, None, 0.25, True) == ("rel", 0.25) and prune.select_args(35, None, 2.5, False) == ("abs", 2.5)
    for bad in ((None, None, True), (0.5, 0.5, True), (1.5, None, True), (-0.1, None, True), (None, 1.5, True), (None, -1.0, False)):
        with pytest.raises(ValueError):
            prune.select_args(35, *bad)


def test_an_unpruned_layer_is_unchanged():
    from models.effkan import KANLinear
    layer = KANLinear(5, 7)
    keys = list(layer.state_dict())
    assert not hasattr(layer, "edge_mask")
    triples = layer.edge_masked()                                    # creates the all-ones mask
    assert [(tuple(p.shape), tuple(m.shape), r) for p, m, r in triples] == [((7, 5, 8), (7, 5), 8), ((7, 5), (7, 5), 1)]
    assert layer.edge_mask.dtype == torch.uint8 and bool(layer.edge_mask.all())
    assert list(layer.state_dict()) == keys                          # a non-persistent buffer
    with torch.no_grad():
        layer.spline_weight[2, 3] = 0
        layer.base_weight[2, 3] = 0
        layer.spline_weight[4, 1] = 0                                # the base term is alive: the edge is
    assert int(layer.restore_edge_mask()) == 34 and layer.edge_mask[2, 3] == 0 and layer.edge_mask[4, 1] == 1


def test_prune_flag_parsing_and_refusals():
    import train
    a = train.parse([])
    assert a.prune == {} and a.prune_mode == "fraction"
    a = train.parse(["--prune", "3:0.5, 6:0.75", "--prune-mode", "relative"])
    assert a.prune == {3: 0.5, 6: 0.75} and a.prune_mode == "relative"
    assert train.parse(["--prune", "2:7.5", "--prune-mode", "absolute"]).prune == {2: 7.5}
    plain, pruned = vars(train.parse(["--synthetic"])), vars(train.parse(["--synthetic", "--prune", "3:0.5"]))
    assert {k for k in pruned if pruned[k] != plain[k]} == {"prune"} and set(pruned) == set(plain)
    for text in ("3", "3:x", "a:0.5", "0:0.5", "3:-0.5", "3:nan", "3:inf", "3:0.5,3:0.6"):
        with pytest.raises(SystemExit, match="--prune"):
            train.parse(["--prune", text])
    for mode in ("fraction", "relative"):
        with pytest.raises(SystemExit, match="at most 1"):
            train.parse(["--prune", "3:1.5", "--prune-mode", mode])
    with pytest.raises(SystemExit, match="--prune is not combined with --dp: every rank would score its own shard"):
        train.parse(["--prune", "3:0.5", "--dp"])
    for kind in ("sine", "vanilla", "fourier", "cheby,sine"):
        with pytest.raises(SystemExit, match=f"--prune: model type\\(s\\) .*{kind.split(',')[-1]}.* have no edge-activation statistic"):
            train.main(train.parse(["--model-type", kind, "--synthetic", "--prune", "3:0.5"]))
