"""The input sets and references of tests/_basis_domain.py, checked without a GPU:

 (1) the plain-torch float32 restatement of every family's formulas (for B-splines KANLinear.b_splines' CPU branch) meets HALF of
     each fp32 bound of the GPU file against the float64 reference on every input set -- so the ranges in the helper are ones
     float32 arithmetic can meet at all, and the GPU kernels are held to bounds with room for their own rounding;
 (2) the knot-edge sets contain every stored knot and both of its float32 neighbours bit for bit, each in 8 feature columns and
     in the first and the last row tile;
 (3) _grid_facts still answers "uniform" for the ordinary grids (a fix of the closed form's admission test cannot simply switch
     the fast path off) and no longer does for grids shifted far from 0 relative to their spacing."""
import pytest
import torch

from tests import _basis_domain as bd

FWD = 2e-5            # tests/test_layers_gpu.py FWD_TOL: max|err| / max(1, max|ref|)
TOL = 1e-4            # tests/test_layers_gpu.py GRAD_TOL: max|err| / max|ref|
M, I = 300, 64


@pytest.mark.parametrize("name", bd.LAYERS)
def test_float32_restatement_meets_half_the_bounds(name):
    layer = bd.make_layer(name, I, I)
    p = bd.params_of(layer)
    x, u, _, _ = bd.input_set(name, layer, M)
    w3 = bd.diag_weights(I, p["GP"], I)
    dy = torch.ones(M, I)
    phi64, dphi64, du64, df64 = bd.basis(p, x, u, torch.float64)
    phi32, dphi32, du32, df32 = bd.basis(p, x, u, torch.float32)
    if p["family"] == "bspline":
        nb = p["G"]
        b = layer.b_splines(x)                                  # the restatement the issue names: the module's own CPU branch
        assert b.dtype == torch.float32 and b.shape == phi32[..., :nb].shape
        phi32 = torch.cat([b, phi32[..., nb:]], -1)
    y64, dx64, dU64, _, dl = bd.contract(phi64, dphi64, w3, dy, du64)
    y32, dx32, dU32, _, _ = bd.contract(phi32.double(), dphi32.double(), w3, dy, None if du32 is None else du32.double())
    cls = bd.huge(x)
    worst = {"y": bd.fwd_err(y32, y64, cls) / FWD, "dx": bd.rel_err(dx32, dx64, cls) / TOL}
    if dU64 is not None:
        worst["du"] = bd.rel_err(dU32, dU64) / TOL
    if df64 is not None:
        worst["dfreq"] = bd.rel_err((dl * df32.double()).sum((0, 1)), (dl * df64).sum((0, 1))) / TOL
    print(f"\n{name}: share of the fp32 bound used by plain float32: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert torch.isfinite(y64).all() and torch.isfinite(dx64).all()
    for k, v in worst.items():
        assert v < 0.5, (name, k, v)


@pytest.mark.parametrize("name", [n for n in bd.LAYERS if n.startswith("bspline")])
def test_knot_edge_sets_hold_every_knot_and_its_neighbours_bitwise(name):
    layer = bd.make_layer(name, I, I)
    x, _, src, sp = bd.input_set(name, layer, M)
    if name[8:] in bd.ACTS:                                     # the base column's sweep: no knots
        assert bd.placement_ok(x, src, sp)
        return
    g = layer.grid
    nk = g.shape[1]
    inf = torch.full_like(g, float("inf"))
    for off, want in ((0, g), (nk, torch.nextafter(g, inf)), (2 * nk, torch.nextafter(g, -inf))):
        assert torch.equal(sp[:, off:off + nk].view(torch.int32), want.view(torch.int32))
    assert bd.placement_ok(x, src, sp)
    want = torch.cat([g, torch.nextafter(g, inf), torch.nextafter(g, -inf)], dim=1)      # and read back from the matrix itself
    for k in range(3 * nk):
        rows, cols = torch.nonzero(src == k, as_tuple=True)
        assert rows.numel() >= 8 and torch.equal(x[rows, cols].view(torch.int32), want[cols, k].view(torch.int32)), (name, k)


@pytest.mark.parametrize("name", ["cheby-deg4", "sine-grid4-trained", "fourier-G28", "rbf", "rbf-gelu"])
def test_special_values_land_in_eight_columns_and_both_row_tiles(name):
    for i in (I, 8):
        layer = bd.make_layer(name, i, i)
        x, u, src, sp = bd.input_set(name, layer, M)
        assert bd.placement_ok(u if name == "rbf" else x, src, sp), (name, i)


def test_trained_frequencies_hold_a_zero_and_a_negative_entry():
    f = bd.make_layer("sine-grid28-first-trained", I, I).freq.detach().flatten()
    assert int((f == 0).sum()) == 1 and int((f < 0).sum()) >= 1 and float(f.abs().max()) > 20


@pytest.mark.parametrize("grid", bd.CLOSED_FORM_GRIDS)
def test_ordinary_grids_keep_the_closed_form(grid):
    from models.effkan import KANLinear, _grid_facts
    a, b, n = grid
    layer = KANLinear(8, 8, grid_size=n, grid_range=[a, b])
    assert _grid_facts([layer]) == (True, True), grid
    from kanvit import _lib
    assert layer.kan_cfg().flags & _lib.FLAG_UNIFORM_KNOTS


@pytest.mark.parametrize("grid", [(100, 101, 5), (1000, 1001, 5), (300, 301, 5)])
def test_grids_far_from_zero_for_their_spacing_take_cox_de_boor(grid):
    """The closed form evaluates the IDEAL uniform grid g0 + j h; the stored float32 knots of these tables sit up to 1.5e-4 of a
    spacing off it, which the bases feel as up to 1.4e-4 (profiles/basis_domain.md)."""
    from models.effkan import KANLinear, _grid_facts
    a, b, n = grid
    layer = KANLinear(8, 8, grid_size=n, grid_range=[a, b])
    assert _grid_facts([layer]) == (False, True), grid
