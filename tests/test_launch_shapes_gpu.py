"""The grouped q|k|v launch at the row counts the BENCHMARK runs, against the float64 oracle.

The layer dispatch picks its kernel form from the launch size (kan_fwd_reg.hip try_fwd_reg, kan_bwd_input_reg*.hip,
kan_bwd_weight_*.hip, kan_layer_common.h kv_tail_first_tile): below about one round of the chip it takes one column tile per
wave, no shared-basis q|k|v (NSH = 1), no LDS-DMA weight gradient and no sub-divided launch tail.  The other parity files run a
few hundred to a few thousand rows, so the forms the headline workloads spend their time in are checked here:

 (1) bench shapes (B = 128 ViT-B, B = 256 ViT-S, and B = 100 for a ragged last row tile together with the automatic tail):
     the expected kernel forms ran (names as recorded by the profiles, profiles/r04_*_kernel_stats.md), y / dx / every
     parameter gradient against the oracle run on row chunks, fp32 results bitwise reproducible;
 (2) forced launch tails (KANVIT_TAIL = k) at a ragged 22-tile launch: against the oracle AND bitwise equal to the untailed
     launch, as the kernels promise (dx columns are independent; a tail piece keeps the k order of every output);
 (3) the NSH = 1 resident bf16 input gradient (one layer of 64 outputs) with a forced tail.

Bounds are the suite's: fp32 forward 2e-5 of the largest entry, gradients 1e-4 (tests/test_headline_parity_gpu.py); bf16 TIGHT
against the bf16-operand oracle and LOOSE against the unrounded one (tests/test_bf16_oracle_gpu.py)."""
import contextlib
import re

import pytest
import torch

from oracle import kan_oracle as ko
from tests._util import record_kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4            # fp32 gradients: max |err| / max |ref|
FWD = 2e-5            # fp32 forward: max |err| / max(1, max |ref|)
TIGHT = 2e-3          # bf16 against the bf16-operand oracle (max |err| / max |ref|)
LOOSE = 1e-2          # bf16 against the unrounded oracle (Frobenius)
CHUNK = 4096          # oracle rows per pass: bounded host memory; the loss is a sum over rows, so parameter gradients add up


class _Err:
    """max |a - b|, max |b|, sum (a - b)^2 and sum b^2 of one tensor, accumulated over row chunks."""

    def __init__(self):
        self.e = self.r = self.e2 = self.r2 = 0.0

    def add(self, got, ref):
        d = got.double() - ref
        self.e = max(self.e, float(d.abs().max()))
        self.r = max(self.r, float(ref.abs().max()))
        self.e2 += float(d.square().sum())
        self.r2 += float(ref.square().sum())
        return self

    def maxrel(self, floor=1e-30):
        return self.e / max(self.r, floor)

    def fwd(self):
        return self.e / max(1.0, self.r)

    def fro(self):
        return (self.e2 / max(self.r2, 1e-60)) ** 0.5


def _params64(module):
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in module.state_dict().items()}
    return {k: v.clone().requires_grad_(not ko.is_buffer_key(k) and v.is_floating_point()) for k, v in sd.items()}


def _oracle(msa, h, x, w, got_y, got_dx, rounded):
    """The float64 oracle of every head's q, k, v on row chunks of x, loss sum(y * w): the errors of got_y / got_dx, compared
    chunk by chunk, and the parameter gradients summed over the chunks (every row carries loss weight)."""
    params = _params64(msa)
    dh = x.shape[1] // h
    ey, edx = _Err(), _Err()
    for r0 in range(0, x.shape[0], CHUNK):
        xd = x[r0:r0 + CHUNK].double().requires_grad_(True)
        with ko.operand_rounding(ko.bf16_round) if rounded else contextlib.nullcontext():
            y = torch.cat([ko.layer_forward(params, f"{p}_mappings.{hh}.", xd[:, hh * dh:(hh + 1) * dh])
                           for p in ("q", "k", "v") for hh in range(h)], dim=1)
        (y * w[r0:r0 + CHUNK].double()).sum().backward()
        ey.add(got_y[r0:r0 + CHUNK], y.detach())
        edx.add(got_dx[r0:r0 + CHUNK], xd.grad)
        del y, xd
    return ey, edx, {k: v.grad for k, v in params.items() if v.grad is not None}


def _run(msa, x, w, bf16, record=False):
    """grouped.run_qkv forward + (y * w).sum().backward() on the GPU: y, dx, parameter gradients (host), launched kernels."""
    from kanvit import grouped
    msa.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    wg = w.to(DEV)
    with record_kernels() if record else contextlib.nullcontext(set()) as names:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            y = grouped.run_qkv(msa.q_mappings, msa.k_mappings, msa.v_mappings, xg)
        assert y.dtype == torch.float32
        (y * wg).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in msa.named_parameters() if p.grad is not None}
    return y.detach().cpu(), xg.grad.detach().cpu(), grads, names


def _assert_forms(names, forms, what):
    """every pattern in `forms` (a regular expression over normalised kernel names) matches a kernel that ran"""
    kan = sorted(n for n in names if n.startswith("kan_"))
    for f in forms:
        assert any(re.fullmatch(f, n) for n in names), (what, f, kan)


def _check_fp32(fam, msa, h, x, w, y, dx, grads):
    ey, edx, gp = _oracle(msa, h, x, w, y, dx, rounded=False)
    assert set(grads) == set(gp), set(grads) ^ set(gp)
    worst = {"y": ey.fwd(), "dx": edx.maxrel(1e-3)}
    for k, g in gp.items():
        worst[k] = _Err().add(grads[k], g).maxrel(1e-3)          # rel_err of tests/_util.py
    assert worst["y"] < FWD, (fam, "y", worst["y"])
    for k, v in worst.items():
        if k != "y":
            assert v < TOL, (fam, k, v)
    return worst


def _check_bf16(fam, msa, h, x, w, y, dx, grads):
    et, edt, gpt = _oracle(msa, h, x, w, y, dx, rounded=True)
    ee, ede, gpe = _oracle(msa, h, x, w, y, dx, rounded=False)
    assert set(grads) == set(gpt), set(grads) ^ set(gpt)
    # as tests/test_bf16_oracle_gpu.py: SineKAN's dx and d freq stay on the exact fp32 kernel under the bf16 flag
    exact_ok = fam == "sine"
    worst = {"y": et.maxrel(), "dx": min(edt.maxrel(), ede.maxrel()) if exact_ok else edt.maxrel()}
    for k, g in gpt.items():
        t = _Err().add(grads[k], g).maxrel()
        worst[k] = min(t, _Err().add(grads[k], gpe[k]).maxrel()) if (exact_ok and k.endswith("freq")) else t
    for k, v in worst.items():
        assert v < TIGHT, (fam, k, v)
    assert 1e-5 < ee.fro() < LOOSE, (fam, "y", ee.fro())
    assert ede.fro() < LOOSE, (fam, "dx", ede.fro())
    for k, g in gpe.items():
        f = _Err().add(grads[k], g).fro()
        assert f < (3 * LOOSE if k.endswith("freq") else LOOSE), (fam, k, f)
    return worst


# The kernel forms each case must reach.  fp32: the names profiles/r04_*_kernel_stats.md recorded for the q|k|v launches of the
# bench (the patch embedding's forms are the other entries of those files).  bf16 ChebyKAN: r04_vitb16_cheby_amp_bf16; the bf16
# efficient-KAN and FastKAN bench runs were not recorded, so the family and the parameters that make the form: the resident
# input gradient with NSH = 3 (SHARED for the B-spline basis, which q, k and v share; FastKAN's per-layer LayerNorm is not shared).
FWD_TAIL = {"cheby": r"kan_fwd_reg_kernel<1, 2, 3, 4, 5, true>", "efficientkan": r"kan_fwd_reg_kernel<2, 2, 3, 2, 9, true>"}
FORMS = {
    ("cheby", False): [FWD_TAIL["cheby"], r"kan_bwd_input_reg_kernel<1, 5, 5, true>", r"kan_bwd_weight_dma_kernel<1, 5, 3, false>"],
    ("cheby", True): [r"kan_fwd_ws_bf16_kernel<1, 5, 2, 3, 8, 4, true>", r"kan_bwd_input_res_bf16_kernel<1, 5, 5, 3, true>",
                      r"kan_bwd_weight_dma_kernel<1, 5, 3, true>"],
    ("efficientkan", False): [FWD_TAIL["efficientkan"], r"kan_bwd_input_reg_kernel<2, 9, 5, true>",
                              r"kan_bwd_weight_reg16_kernel<2, 9, 3, 12>"],
    ("efficientkan", True): [r"kan_bwd_input_res_bf16_kernel<2, \d+, \d+, 3, true>"],
    ("vanilla", False): [r"kan_fwd_reg_kernel<0, 2, 3, 4, 1, true>", r"kan_bwd_input_reg_kernel<0, 1, 2, true>",
                         r"kan_bwd_weight_reg_kernel<0, 1, 6, false, 1, false>"],
    ("sine", False): [r"kan_fwd_reg_kernel<4, 2, 1, 4, 4, false>", r"kan_bwd_input_reg_kernel<4, 4, 4, false>",
                      r"kan_bwd_weight_reg_kernel<4, 4, 2, false, 4, false>"],
    ("fast", False): [r"kan_fwd_reg_kernel<3, 2, 1, 4, 9, false>", r"kan_bwd_input_reg_kernel<3, 9, 5, false>",
                      r"kan_bwd_weight_reg16_kernel<3, 9, 9, 4>", r"kan_ln_bwd_kernel<.*>"],
    ("fast", True): [r"kan_bwd_input_res_bf16_kernel<3, \d+, \d+, 3, false>", r"kan_ln_bwd_kernel<.*>"],
}

BENCH = [  # (family, d, heads, rows, bf16)
    ("cheby", 768, 12, 128 * 197, False), ("cheby", 768, 12, 128 * 197, True),
    ("efficientkan", 768, 12, 128 * 197, False), ("efficientkan", 768, 12, 128 * 197, True),
    ("vanilla", 768, 12, 128 * 197, False),
    ("sine", 768, 12, 128 * 197, False),
    ("fast", 384, 6, 256 * 197, False), ("fast", 384, 6, 256 * 197, True),
    # B = 100: 154 row tiles, the last one 116 rows; the automatic tail covers it (tiles 144..153 of the forward)
    ("cheby", 768, 12, 100 * 197, False), ("cheby", 768, 12, 100 * 197, True),
]


@pytest.mark.parametrize("fam,d,h,m,bf16", BENCH, ids=[f"{c[0]}-M{c[3]}-{'bf16' if c[4] else 'fp32'}" for c in BENCH])
def test_bench_shape_qkv_vs_fp64_oracle(fam, d, h, m, bf16):
    from attention import MSA
    torch.manual_seed(1000 + m % 997 + d)
    msa = MSA(d, h, type=fam)
    x = torch.randn(m, d)
    w = torch.randn(m, 3 * d)
    msa = msa.to(DEV)
    y, dx, grads, names = _run(msa, x, w, bf16, record=True)
    if bf16:
        worst = _check_bf16(fam, msa, h, x, w, y, dx, grads)
    else:
        y2, dx2, grads2, _ = _run(msa, x, w, bf16)
        assert torch.equal(y, y2) and torch.equal(dx, dx2), (fam, m, "fp32 results not reproducible")
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), (fam, m, k, "fp32 gradient not reproducible")
        worst = _check_fp32(fam, msa, h, x, w, y, dx, grads)
    _assert_forms(names, FORMS[(fam, bf16)], (fam, m, bf16))
    print(f"\n{fam} M={m} {'bf16' if bf16 else 'fp32'}: kernels {sorted(n for n in names if n.startswith('kan_'))}"
          f"\n  worst {max(worst.items(), key=lambda kv: kv[1])}")


@contextlib.contextmanager
def _forced_tail(monkeypatch, k):
    """KANVIT_TAIL = k for the block (the library reads its switches at load; reload_config re-reads them)."""
    from kanvit import _lib
    monkeypatch.setenv("KANVIT_TAIL", str(k))
    try:
        cfg = _lib.reload_config()
        assert f"tail={k}" in cfg.split(), cfg
        yield
    finally:
        monkeypatch.undo()
        _lib.reload_config()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fam", ["cheby", "efficientkan", "fast"])
def test_forced_tail_ragged_launch(fam, bf16, monkeypatch):
    """MSA(768, 12) at M = 2758 (B = 14): 22 row tiles, the last one 70 rows, NSH = 3 in the fp32 forward (22 x 12 >= 256
    work-groups).  Tails of 1 (the ragged tile alone), 5 and 21 tiles (everything but tile 0): bitwise the untailed results,
    and within the oracle's bounds."""
    from attention import MSA
    torch.manual_seed(2758 + len(fam))
    m, d, h = 14 * 197, 768, 12
    msa = MSA(d, h, type=fam).to(DEV)
    x = torch.randn(m, d)
    w = torch.randn(m, 3 * d)
    with _forced_tail(monkeypatch, 0):
        y0, dx0, g0, names0 = _run(msa, x, w, bf16, record=True)
    if not bf16 and fam in FWD_TAIL:
        assert not any(re.fullmatch(FWD_TAIL[fam], n) for n in names0), (fam, "TAIL form ran with KANVIT_TAIL=0")
        assert any(re.fullmatch(FWD_TAIL[fam][:-5] + "false>", n) for n in names0), (fam, sorted(names0))
    for k in (1, 5, 21):
        with _forced_tail(monkeypatch, k):
            y, dx, grads, names = _run(msa, x, w, bf16, record=True)
        if not bf16 and fam in FWD_TAIL:
            _assert_forms(names, [FWD_TAIL[fam]], (fam, k))
        assert torch.equal(y, y0), (fam, bf16, k, "y", float((y - y0).abs().max()))
        assert torch.equal(dx, dx0), (fam, bf16, k, "dx", float((dx - dx0).abs().max()))
        for key in g0:
            assert torch.equal(grads[key], g0[key]), (fam, bf16, k, key)
    worst = (_check_bf16 if bf16 else _check_fp32)(fam, msa, h, x, w, y0, dx0, g0)
    print(f"\n{fam} M={m} {'bf16' if bf16 else 'fp32'} forced tails: worst {max(worst.items(), key=lambda kv: kv[1])}")


def test_forced_tail_nsh1_resident_bf16(monkeypatch):
    """One ChebyKAN layer of 64 outputs (groups = 1): the NSH = 1 resident bf16 input gradient, 8 feature chunks per row tile.
    M = 1000 rows = 8 tiles (the last 104 rows), KANVIT_TAIL = 3: three tiles cut into single-chunk pieces of one step each."""
    from models.cheby import ChebyKANLayer
    torch.manual_seed(64)
    layer = ChebyKANLayer(256, 64, 4).to(DEV)
    x = torch.randn(1000, 256)
    w = torch.randn(1000, 64)
    res = {}
    for k in (0, 3):
        with _forced_tail(monkeypatch, k):
            layer.zero_grad(set_to_none=True)
            xg = x.to(DEV).requires_grad_(True)
            with record_kernels() as names:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = layer(xg)
                (y * w.to(DEV)).sum().backward()
            _assert_forms(names, [r"kan_bwd_input_res_bf16_kernel<1, 5, 5, 1, false>"], k)
            res[k] = (y.detach().cpu(), xg.grad.cpu(), {n: p.grad.cpu() for n, p in layer.named_parameters()})
    (y, dx, g), (y0, dx0, g0) = res[3], res[0]
    assert torch.equal(y, y0) and torch.equal(dx, dx0), float((dx - dx0).abs().max())
    assert all(torch.equal(g[n], g0[n]) for n in g0)
    for rounded in (True, False):
        params = _params64(layer)
        xd = x.double().requires_grad_(True)
        with ko.operand_rounding(ko.bf16_round) if rounded else contextlib.nullcontext():
            yr = ko.layer_forward(params, "", xd)
        (yr * w.double()).sum().backward()
        errs = [_Err().add(y, yr.detach()), _Err().add(dx, xd.grad)] + [_Err().add(g[n], params[n].grad) for n in g]
        if rounded:
            assert max(e.maxrel() for e in errs) < TIGHT, [e.maxrel() for e in errs]
        else:
            assert 1e-5 < errs[0].fro() < LOOSE and all(e.fro() < LOOSE for e in errs), [e.fro() for e in errs]
