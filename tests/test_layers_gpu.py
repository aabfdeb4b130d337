"""GPU parity of the fused KAN layer kernels (through the C ABI) against
 (1) tensors produced by the real reference (tests/golden/layer_*.npz), and
 (2) the float64 CPU oracle on seeded inputs, including ragged / odd shapes and grouped launches.
Tolerance: BASELINE.json asks for 1e-4 (fp32); the asserts below are tighter."""
import pytest
import torch

from oracle import kan_oracle as ko
from tests._util import T, grads_from, load_npz, max_err, rel_err, state_dict_from

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMS = ["cheby", "efficientkan", "fast", "fourier", "sine"]
FWD_TOL = 2e-5
GRAD_TOL = 1e-4       # BASELINE.json north_star: within 1e-4 (normwise, relative to the largest reference entry)


def make_layer(fam, i, o, big):
    from models.cheby import ChebyKANLayer
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    from models.nfkan import NaiveFourierKANLayer
    from models.sinekan import SineKANLayer
    return {"cheby": lambda: ChebyKANLayer(i, o, 4), "efficientkan": lambda: KANLinear(i, o),
            "fast": lambda: FastKANLayer(i, o), "fourier": lambda: NaiveFourierKANLayer(i, o, 28 if big else 3),
            "sine": lambda: SineKANLayer(i, o, grid_size=28 if big else 4)}[fam]()


def run_gpu(layer, x):
    layer = layer.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    y = layer(xg)
    layer.zero_grad()
    y.square().sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), xg.grad.cpu(), {k: v.grad.cpu() for k, v in layer.named_parameters() if v.grad is not None}


@pytest.mark.parametrize("fam", FAMS)
def test_against_reference_fixtures(fam):
    blob = load_npz(f"layer_{fam}.npz")
    shapes = [((6, 4), 3, False), ((50, 32), 32, False), ((4, 49, 16), 64, True)]
    for c in range(int(blob["n_cases"])):
        shape, o, big = shapes[c // 3]
        p = f"c{c}."
        layer = make_layer(fam, shape[-1], o, big)
        layer.load_state_dict(state_dict_from(blob, p))
        y, gx, gp = run_gpu(layer, T(blob[p + "x"]))
        assert y.shape == T(blob[p + "y"]).shape, (fam, c)
        assert max_err(y, T(blob[p + "y"])) < FWD_TOL, (fam, c, max_err(y, T(blob[p + "y"])))
        assert rel_err(gx, T(blob[p + "grad_x"])) < GRAD_TOL, (fam, c, "grad_x")
        want = grads_from(blob, p)
        assert set(want) == set(gp), (fam, c, set(want) ^ set(gp))
        for k, g in want.items():
            assert rel_err(gp[k], g) < GRAD_TOL, (fam, c, k, rel_err(gp[k], g))


@pytest.mark.parametrize("fam", FAMS)
def test_known_answer_vectors(fam):
    blob = load_npz(f"layer_{fam}.npz")
    layer = make_layer(fam, 4, 3, False)
    layer.load_state_dict(state_dict_from(blob, "kat."))
    y, gx, _ = run_gpu(layer, T(blob["kat.x"]))
    assert max_err(y, T(blob["kat.y"])) < 2e-6
    assert max_err(gx, T(blob["kat.grad_x"])) < 2e-5


def oracle_run(layer, x):
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in layer.state_dict().items()}
    params = {k: v.clone().requires_grad_(not ko.is_buffer_key(k) and v.is_floating_point()) for k, v in sd.items()}
    xd = x.double().clone().requires_grad_(True)
    y = ko.layer_forward(params, "", xd)
    y.square().sum().backward()
    return y.detach(), xd.grad, {k: v.grad for k, v in params.items() if v.grad is not None}


SHAPES = [(1, 2, 1), (7, 5, 3), (127, 16, 64), (129, 64, 64), (1000, 33, 70), (300, 192, 64), (257, 8, 8), (513, 48, 200),
          (1100, 64, 64)]      # the last one: several ragged token slabs in the streaming weight-gradient kernel


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_oracle_ragged_shapes(fam, shape):
    m, i, o = shape
    torch.manual_seed(m * 131 + i)
    layer = make_layer(fam, i, o, big=(i <= 48))
    x = torch.randn(m, i) * (1.5 if fam != "cheby" else 1.0)
    y, gx, gp = run_gpu(layer, x)
    yo, gxo, gpo = oracle_run(layer, x)
    scale = max(1.0, float(yo.abs().max()))
    assert max_err(y, yo) < FWD_TOL * scale, (fam, shape, max_err(y, yo))
    assert rel_err(gx, gxo) < GRAD_TOL, (fam, shape, "grad_x", rel_err(gx, gxo))
    for k, g in gpo.items():
        assert rel_err(gp[k], g) < GRAD_TOL, (fam, shape, k, rel_err(gp[k], g))


@pytest.mark.parametrize("shape", [(7, 5, 3), (300, 192, 64), (513, 48, 200), (1100, 64, 64), (2048, 768, 96), (129, 64, 64)])
def test_sine_frequency_gradient_without_input_gradient(shape, monkeypatch):
    """x that needs no gradient (the patch embedding's input is the image): d loss / d freq comes from a second weight-gradient pass
    over the operand x cos(x f + p) (KANVIT_FLAG_SINE_DFREQ, ops._kan_backward) instead of the input-gradient kernel -- the same
    number within fp32 summation order, and within 1e-4 of the float64 oracle (models/sinekan.py:81-91, freq trainable :60)."""
    from kanvit import _lib, ops
    m, i, o = shape
    torch.manual_seed(m + i)
    layer = make_layer("sine", i, o, big=(i <= 48 or i == 768)).to(DEV)
    x = (torch.randn(m, i) * 1.5)
    _, _, gpo = oracle_run(layer, x)
    res = {}
    for name, env, needs_x in (("weight_pass", None, False), ("input_kernel", "1", False), ("with_dx", None, True)):
        if env:
            monkeypatch.setenv("KANVIT_NO_DFREQ_W", env)
        else:
            monkeypatch.delenv("KANVIT_NO_DFREQ_W", raising=False)
        _lib.reload_config()
        layer.zero_grad()
        xg = x.to(DEV).requires_grad_(needs_x)
        layer(xg).square().sum().backward()
        res[name] = {k: v.grad.clone().cpu() for k, v in layer.named_parameters() if v.grad is not None}
    monkeypatch.delenv("KANVIT_NO_DFREQ_W", raising=False)
    _lib.reload_config()
    for name, gp in res.items():
        assert set(gp) == set(gpo), (name, set(gp) ^ set(gpo))
        for k, g in gpo.items():
            assert rel_err(gp[k], g) < GRAD_TOL, (shape, name, k, rel_err(gp[k], g))
    # the two routes are different sums of the same products; amplitudes / bias do not depend on the route at all
    assert rel_err(res["weight_pass"]["freq"], res["input_kernel"]["freq"]) < 2e-5
    for k in ("amplitudes", "bias"):
        assert torch.equal(res["weight_pass"][k], res["input_kernel"][k]), k
    assert torch.equal(res["input_kernel"]["freq"], res["with_dx"]["freq"])      # same kernel whether or not dx is kept


def test_sine_dfreq_flag_is_refused_elsewhere():
    import ctypes as C
    from kanvit import _lib
    L = _lib.lib()
    d = _lib.LayerDesc(4, 1, 1, 64, 64, 4, 0, 0, 0.0, _lib.FLAG_SINE_DFREQ, 256, 64, 64, 64, 4 + 64 * 4, 0.0, 0)
    assert L.kanvit_layer_sine_dfreq_ok(C.byref(d)) == 1
    buf = torch.zeros(64 * 64 * 4 + 4096, device=DEV)
    p = C.c_void_p(buf.data_ptr())
    assert L.kanvit_layer_fwd(C.byref(d), p, None, p, p, None, p, None, 0, None) != 0 and b"bwd_weight flag" in L.kanvit_last_error()
    assert L.kanvit_layer_bwd_input(C.byref(d), p, None, p, p, p, p, None, p, None, 0, None) != 0 and b"bwd_weight flag" in L.kanvit_last_error()
    d2 = _lib.LayerDesc(1, 1, 1, 64, 64, 4, 0, 0, 0.0, _lib.FLAG_SINE_DFREQ, 256, 64, 64, 64, 0, 0.0, 0)
    assert L.kanvit_layer_sine_dfreq_ok(C.byref(d2)) == 0
    assert L.kanvit_layer_bwd_weight(C.byref(d2), p, None, None, p, p, None, 0, None) != 0 and b"SINE flag" in L.kanvit_last_error()


def test_non_default_spline_configuration():
    """grid_size / spline_order other than (5, 3) take the runtime-sized B-spline path."""
    from models.effkan import KANLinear
    torch.manual_seed(3)
    layer = KANLinear(10, 12, grid_size=7, spline_order=2, grid_range=[-1.5, 1.5])
    x = torch.randn(200, 10)
    y, gx, gp = run_gpu(layer, x)
    sd = {k: v.detach().cpu().double() for k, v in layer.state_dict().items()}
    params = {k: v.clone().requires_grad_(k != "grid") for k, v in sd.items()}
    xd = x.double().requires_grad_(True)
    yo = ko.kanlinear_forward(xd, params["base_weight"], params["spline_weight"], params["spline_scaler"],
                              params["grid"], 2)
    yo.square().sum().backward()
    assert max_err(y, yo) < FWD_TOL
    assert rel_err(gx, xd.grad) < GRAD_TOL
    assert rel_err(gp["spline_weight"], params["spline_weight"].grad) < GRAD_TOL


def test_empty_batch_and_determinism():
    layer = make_layer("cheby", 16, 8, False).to(DEV)
    assert layer(torch.empty(0, 16, device=DEV)).shape == (0, 8)
    x = torch.randn(777, 16, device=DEV, requires_grad=True)
    outs = []
    for _ in range(2):
        layer.zero_grad()
        x.grad = None
        layer(x).square().sum().backward()
        outs.append((x.grad.clone(), layer.cheby_coeffs.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])   # no atomics: bitwise


@pytest.mark.parametrize("fam", ["vanilla", "cheby", "efficientkan", "fast", "sine"])
@pytest.mark.parametrize("geom", [(2, 50, 64, 2), (3, 17, 64, 8), (2, 197, 128, 2)])
def test_grouped_qkv_equals_per_layer_oracle(fam, geom):
    """One launch for all heads' q|k|v == the reference's per-head layers applied one by one."""
    from attention import MSA
    from kanvit import grouped
    b, n, d, h = geom
    torch.manual_seed(5)
    msa = MSA(d, h, type=fam)
    x = torch.randn(b, n, d)
    sd = {k: (v.detach().double() if v.is_floating_point() else v) for k, v in msa.state_dict().items()}
    dh = d // h
    want = []
    for name in ("q", "k", "v"):
        for hh in range(h):
            want.append(ko.layer_forward(sd, f"{name}_mappings.{hh}.", x.double().reshape(b * n, d)[:, hh * dh:(hh + 1) * dh]))
    want = torch.cat(want, dim=1)
    msa = msa.to(DEV)
    got = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x.to(DEV).reshape(b * n, d)).cpu()
    assert max_err(got, want) < FWD_TOL * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("fam", ["vanilla", "cheby", "efficientkan", "fast", "sine"])
def test_bf16_mfma_forward_close_to_fp32(fam):
    """KANVIT_FLAG_BF16_MFMA (set under bf16 autocast): operands rounded to bf16, fp32 accumulate.  Loose
    tolerance against the exact path (bf16 configs are judged at ~1e-2 relative)."""
    from attention import MSA
    from kanvit import grouped
    torch.manual_seed(2)
    msa = MSA(256, 4, type=fam).to(DEV)
    x = torch.randn(4 * 197, 256, device=DEV)
    exact = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        fast = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x)
    assert fast.dtype == torch.float32
    err = float((fast - exact).abs().max()) / float(exact.abs().max())
    assert 0 < err < 2e-2, (fam, err)          # > 0: the bf16 kernel really ran


@pytest.mark.parametrize("fam", ["vanilla", "cheby", "efficientkan", "fast", "sine"])
@pytest.mark.parametrize("dh", [64, 32])
def test_bf16_mfma_gradients_close_to_fp32(fam, dh):
    from attention import MSA
    from kanvit import grouped
    torch.manual_seed(4)
    msa = MSA(4 * dh, 4, type=fam).to(DEV)
    x = torch.randn(4 * 197 + 5, 4 * dh, device=DEV, requires_grad=True)
    w = torch.randn(4 * 197 + 5, 12 * dh, device=DEV)

    def grads(amp):
        msa.zero_grad()
        x.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x)
        (y * w).sum().backward()
        return [x.grad.clone()] + [p.grad.clone() for p in msa.parameters() if p.grad is not None]

    for a, b in zip(grads(True), grads(False)):
        if float(b.abs().max()) > 1e-3:
            assert float((a - b).abs().max()) / float(b.abs().max()) < 3e-2, fam


@pytest.mark.parametrize("fam", ["vanilla", "cheby"])
def test_bf16_weight_stationary_forward_matches_tile_kernel(fam, monkeypatch):
    """M >= 4096 rows switches the bf16 q|k|v forward to the persistent W-stationary kernel (weights resident in LDS,
    flipped product, stores from accumulators).  Same bf16 operand rounding as the per-tile kernel, so the two must agree
    to fp32 accumulation-order noise; a ragged last row tile (M % 256 != 0) and the bias path (vanilla) are included."""
    from attention import MSA
    from kanvit import _lib, grouped
    torch.manual_seed(11)
    msa = MSA(256, 4, type=fam).to(DEV)
    x = torch.randn(4096 + 129, 256, device=DEV)
    exact = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ws = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x)
        monkeypatch.setenv("KANVIT_NO_WS", "1")
        _lib.reload_config()
        try:
            tile = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x)
        finally:
            monkeypatch.delenv("KANVIT_NO_WS")
            _lib.reload_config()
    scale = float(exact.abs().max())
    assert float((ws - tile).abs().max()) / scale < 1e-5, fam
    err = float((ws - exact).abs().max()) / scale
    assert 0 < err < 2e-2, (fam, err)


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("fam", ["cheby", "fast", "sine"])
def test_weight_gradient_kernels_agree_and_are_deterministic(fam, amp, monkeypatch):
    """The streaming register-form weight-gradient kernel and the LDS-tile kernel compute the same sums (same operand rounding,
    fp32 accumulation in a different order), and each is bitwise reproducible run to run (slabs + ordered reduce, no atomics)."""
    from attention import MSA
    from kanvit import _lib, grouped
    torch.manual_seed(4)
    msa = MSA(256, 4, type=fam).to(DEV)
    x = torch.randn(4 * 197 + 5, 256, device=DEV, requires_grad=True)
    w = torch.randn(4 * 197 + 5, 768, device=DEV)
    # FastKAN: both kernels must see the SAME normalised input u.  The LDS-tile kernel has no fused LayerNorm, and a u that
    # differs in its last bit flips bf16 roundings of basis values (a route difference, not a kernel one; the fused route is
    # covered by tests/test_fused_ln_gpu.py), so the comparison runs with the LayerNorm as a separate op on both sides.
    monkeypatch.setenv("KANVIT_NO_FUSED_LN", "1")
    _lib.reload_config()

    def grads():
        msa.zero_grad()
        x.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x)
        (y * w).sum().backward()
        return torch.cat([p.grad.flatten() for p in msa.parameters() if p.grad is not None]).clone()

    try:
        reg = [grads() for _ in range(3)]
        monkeypatch.setenv("KANVIT_NO_REG_BW", "1")
        _lib.reload_config()
        tile = [grads() for _ in range(2)]
    finally:
        monkeypatch.delenv("KANVIT_NO_REG_BW", raising=False)
        monkeypatch.delenv("KANVIT_NO_FUSED_LN")
        _lib.reload_config()
    assert all(torch.equal(reg[0], r) for r in reg[1:])
    assert torch.equal(tile[0], tile[1])
    # FastKAN: the register kernel forms the eight Gaussians by the two-anchor recurrence, the LDS-tile kernel by one exp per
    # centre (relative difference <= ~2e-6 in fp32); under bf16 such a difference flips roundings of single basis values
    tol = 2e-3 if (fam == "fast" and amp) else 1e-5
    assert float((reg[0] - tile[0]).abs().max()) / float(tile[0].abs().max()) < tol


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("rows", [4 * 197 + 5, 64, 2049, 3 * 1024])
def test_chebykan_weight_gradient_lds_dma_form(rows, amp, monkeypatch):
    """The LDS-DMA form of ChebyKAN's weight gradient (csrc/kan_bwd_weight_dma.hip: wave-private rings filled by global_load_lds,
    four row ranges per work-group summed through the LDS) against the register-ring form on the same launch: same operands and
    roundings, fp32 sums in another order.  KANVIT_BW_DMA_FORCE takes shapes that would not fill the chip through it: row ranges
    that end inside a 16-row block, waves without rows, a single block per wave.  Bitwise reproducible.  The x_off leg passes a
    sliced x whose rows do not start on 16-byte boundaries to the Python op: kanvit.ops makes every operand contiguous first, so
    the library sees an aligned copy and the leg checks that copy path against the register form.  A misaligned x that does
    reach the library is run in tests/test_layer_strided_gpu.py and tests/test_weight_forms_gpu.py."""
    from attention import MSA
    from kanvit import _lib, grouped
    torch.manual_seed(9)
    msa = MSA(256, 4, type="cheby").to(DEV)
    xfull = torch.randn(rows, 257, device=DEV)
    w = torch.randn(rows, 768, device=DEV)

    def grads(x):
        msa.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x)
        (y * w).sum().backward()
        return torch.cat([p.grad.flatten() for p in msa.parameters() if p.grad is not None]).clone()

    x = xfull[:, :256].contiguous()
    x_off = xfull[:, 1:]                           # a view 4 bytes off the 16-byte grid with row stride 257: ops copies it before the call
    monkeypatch.delenv("KANVIT_BW_NO_DMA", raising=False)      # (a run of the parity files with the round-4 forms switched off must not switch this one off)
    monkeypatch.setenv("KANVIT_BW_DMA_FORCE", "1")
    _lib.reload_config()
    try:
        assert "bw_dma_force=1" in _lib.active_config()
        dma = [grads(x) for _ in range(3)]
        off = grads(x_off)
        monkeypatch.setenv("KANVIT_BW_NO_DMA", "1")
        _lib.reload_config()
        ring = grads(x)
        ring_off = grads(x_off)
    finally:
        monkeypatch.delenv("KANVIT_BW_DMA_FORCE", raising=False)
        monkeypatch.delenv("KANVIT_BW_NO_DMA", raising=False)
        _lib.reload_config()
    assert all(torch.equal(dma[0], d) for d in dma[1:])
    scale = float(ring.abs().max())
    assert torch.isfinite(dma[0]).all() and float((dma[0] - ring).abs().max()) / scale < 1e-5
    if rows >= 256:
        assert not torch.equal(dma[0], ring)       # another order of the fp32 sums: the LDS-DMA kernel really ran (below 256 rows neither form applies)
    assert float((off - ring_off).abs().max()) / float(ring_off.abs().max()) < 1e-5


@pytest.mark.parametrize("fam", ["vanilla", "cheby", "efficientkan", "fast"])
@pytest.mark.parametrize("rows", [4 * 197 + 5, 128, 1])
def test_bf16_input_gradient_resident_form_is_bitwise_the_streaming_form(fam, rows, monkeypatch):
    """The dY-resident bf16 input gradient (a row tile's dY loaded once, W through an LDS-DMA ring of three step images) forms the same
    products in the same order as the streaming kernel it replaces on the per-head layers: dx (and FastKAN's du path) bit for bit."""
    from attention import MSA
    from kanvit import _lib, grouped
    torch.manual_seed(12)
    msa = MSA(256, 4, type=fam).to(DEV)
    x = torch.randn(rows, 256, device=DEV, requires_grad=True)
    w = torch.randn(rows, 768, device=DEV)

    def dx():
        msa.zero_grad()
        x.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x)
        (y * w).sum().backward()
        return x.grad.clone()

    monkeypatch.delenv("KANVIT_BI_NO_RES", raising=False)
    _lib.reload_config()
    res = [dx(), dx()]
    monkeypatch.setenv("KANVIT_BI_NO_RES", "1")
    _lib.reload_config()
    try:
        assert "bi_no_res=1" in _lib.active_config()
        stream = dx()
    finally:
        monkeypatch.delenv("KANVIT_BI_NO_RES")
        _lib.reload_config()
    assert torch.isfinite(res[0]).all() and torch.equal(res[0], res[1])
    assert torch.equal(res[0], stream), (fam, float((res[0] - stream).abs().max()))


def test_bspline_non_uniform_or_differing_grids_take_the_general_path():
    """The closed-form / shared-basis shortcuts are only taken when the knot buffers allow it."""
    from attention import MSA
    from kanvit import grouped
    from models.effkan import _grid_facts
    torch.manual_seed(6)
    msa = MSA(128, 2, type="efficientkan").to(DEV)
    layers = list(msa.q_mappings) + list(msa.k_mappings) + list(msa.v_mappings)
    assert _grid_facts(layers) == (True, True)
    x = torch.randn(300, 128, device=DEV)
    ref = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x).cpu()
    with torch.no_grad():
        msa.k_mappings[1].grid[:, 5] += 0.05           # one layer gets a non-uniform knot vector
    assert _grid_facts(layers) == (True, False)        # (layer 0 still uniform, but not all equal)
    got = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, x)
    sd = {k: v.detach().cpu().double() if v.is_floating_point() else v.cpu() for k, v in msa.state_dict().items()}
    want = []
    for name in ("q", "k", "v"):
        for hh in range(2):
            want.append(ko.layer_forward(sd, f"{name}_mappings.{hh}.", x.cpu().double()[:, hh * 64:(hh + 1) * 64]))
    want = torch.cat(want, dim=1)
    assert max_err(got.cpu(), want) < FWD_TOL * max(1.0, float(want.abs().max()))
    assert max_err(got.cpu()[:, :64 * 3], ref[:, :64 * 3]) < 1e-6        # untouched layers unchanged


@pytest.mark.parametrize("fam", ["vanilla", "cheby", "efficientkan"])
def test_tiny_head_kernels_against_oracle_and_general_path(fam, monkeypatch):
    """train.py's default geometry (d = 64, 8 heads -> per-head layers of 8 -> 8 features, M = 128 x 17 rows): the vector-pipe
    kernels of csrc/kan_tiny.hip.  Forward and every gradient against the fp64 oracle, and against the general (LDS-tile) kernels
    they replace (KANVIT_NO_TINY=1)."""
    from attention import MSA
    from kanvit import _lib, grouped
    from tests.test_headline_parity_gpu import _oracle_qkv
    torch.manual_seed(21)
    d, h, rows = 64, 8, 128 * 17
    msa = MSA(d, h, type=fam)
    x = torch.randn(rows, d)
    w = torch.randn(rows, 3 * d)
    yo, gxo, gpo = _oracle_qkv(msa, x, w, h)
    msa = msa.to(DEV)

    def run():
        msa.zero_grad()
        xg = x.to(DEV).requires_grad_(True)
        y = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, xg)
        (y * w.to(DEV)).sum().backward()
        return y.detach(), xg.grad, {k: v.grad.clone() for k, v in msa.named_parameters() if v.grad is not None}

    y, gx, gp = run()
    assert max_err(y.cpu(), yo) < 2e-5 * max(1.0, float(yo.abs().max()))
    assert rel_err(gx.cpu(), gxo) < GRAD_TOL
    assert set(gp) == set(gpo)
    for k, g in gpo.items():
        assert rel_err(gp[k].cpu(), g) < GRAD_TOL, (k, rel_err(gp[k].cpu(), g))
    y2, gx2, gp2 = run()
    assert torch.equal(y, y2) and torch.equal(gx, gx2) and all(torch.equal(gp[k], gp2[k]) for k in gp)      # deterministic
    monkeypatch.setenv("KANVIT_NO_TINY", "1")
    _lib.reload_config()
    try:
        y0, gx0, gp0 = run()
    finally:
        monkeypatch.delenv("KANVIT_NO_TINY")
        _lib.reload_config()
    assert rel_err(y, y0) < 1e-5 and rel_err(gx, gx0) < 1e-5
    for k in gp0:
        assert rel_err(gp[k], gp0[k]) < 1e-5, k


@pytest.mark.parametrize("fam", ["cheby", "efficientkan", "fourier"])
@pytest.mark.parametrize("shape", [(300, 5, 3), (64, 16, 16), (1000, 8, 8), (257, 16, 4), (90, 1, 12)])
def test_tiny_single_layers_against_oracle(fam, shape):
    """Single layers with I, O <= 16 and M >= 64 (odd sizes included) take the vector-pipe kernels of csrc/kan_tiny.hip."""
    m, i, o = shape
    torch.manual_seed(m + 7 * i + o)
    layer = make_layer(fam, i, o, big=False)
    x = torch.randn(m, i) * (1.5 if fam != "cheby" else 1.0)
    y, gx, gp = run_gpu(layer, x)
    yo, gxo, gpo = oracle_run(layer, x)
    assert max_err(y, yo) < FWD_TOL * max(1.0, float(yo.abs().max())), (fam, shape, max_err(y, yo))
    assert rel_err(gx, gxo) < GRAD_TOL, (fam, shape, "grad_x", rel_err(gx, gxo))
    for k, g in gpo.items():
        assert rel_err(gp[k], g) < GRAD_TOL, (fam, shape, k, rel_err(gp[k], g))
