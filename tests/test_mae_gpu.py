"""Masked-autoencoder pretraining on the GPU: ops.restore_tokens and ops.mae_loss (csrc/mae.hip) against the restatements of
tests/_mae_ref.py, MaskedAutoencoder against a stock-torch forward from its own parameters, and train.py --pretrain mae.

Restore is one add per element and its backward copies: both bitwise.  The mask-token gradient is a sum of n = B (P - K) rows in a fixed
tree: bitwise from run to run, and within (n - 1) 2^-24 sum|x_i| of float64, the first-order bound of any fp32 order.

The loss is measured as tests/test_soft_ce_gpu.py measures its own: with e the error of the stock torch fp32 composition on the same
GPU against the same float64 values, the kernel may err by 2 e + 4 ulp of the value for rows and loss and by 2 e + 2^-22 of the largest
gradient entry for dpred.  Every case prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _mae_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROW_GRID, THREADS = 2048, 256        # csrc/mae.hip: MAE_ROW_GRID work-groups at most, MAE_THREADS / lanes-per-row rows each


def _dev(a, misaligned=False):
    """The array on the GPU; misaligned: at an address that is a multiple of 4 but not of 16 bytes (the general form's)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misaligned:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _restore_raw(y, mask, pos, idx, out):
    from kanvit import _lib, ops
    (B, K), P, O = idx.shape, pos.shape[0] - 1, y.shape[-1]
    ops._launch(_lib.lib().kanvit_tokens_restore_fwd, "kanvit_tokens_restore_fwd", y.device, B, P, K, O, ops._ptr(y), ops._ptr(mask), ops._ptr(pos),
                ops._ptr(idx), ops._ptr(out))
    return out


def _restore_bwd_raw(dout, idx, dy, dmask):
    from kanvit import _lib, ops
    (B, N, O), K = dout.shape, idx.shape[1]
    ops._launch(_lib.lib().kanvit_tokens_restore_bwd, "kanvit_tokens_restore_bwd", dout.device, B, N - 1, K, O, ops._ptr(dout), ops._ptr(idx),
                ops._ptr(dy), ops._ptr(dmask))


# (B, P, K, O, misaligned): a tail past float4 with one masked token; one kept token and an odd width; P at the cap; the general form
# at a 4-byte address; more rows than MAE_ROW_GRID work-groups of 256 one-lane rows take in one lap (O = 4: 8 MB)
RESTORE = [(3, 16, 4, 64, False), (3, 16, 15, 66, False), (2, 16, 1, 5, False), (1, 1024, 256, 8, False), (3, 16, 4, 64, True),
           (513, 1024, 2, 4, False)]
assert RESTORE[-1][0] * (RESTORE[-1][1] + 1) > ROW_GRID * THREADS


@pytest.fixture(scope="module")
def restore_cases():
    cases = {}
    for B, P, K, O, mis in RESTORE:
        rng = np.random.default_rng(B + P + K + O)
        y, mask, pos = (rng.standard_normal(s).astype(np.float32) for s in ((B, K + 1, O), (O,), (P + 1, O)))
        idx = ref.keep_table(B, P, K)
        assert (idx[:, 1:] > idx[:, :-1]).all() and (idx[:, 0] == 0).any() and (idx[:, -1] == P - 1).any()
        dout = rng.standard_normal((B, P + 1, O)).astype(np.float32)
        cases[(B, P, K, O, mis)] = dict(y=y, mask=mask, pos=pos, idx=idx, dout=dout, want=ref.restore(y, mask, pos, idx))
    return cases


@pytest.mark.parametrize("case", RESTORE, ids=lambda c: "x".join(map(str, c[:4])) + ("-4byte" if c[4] else ""))
def test_restore_forward_is_the_torch_composition_bitwise(case, restore_cases):
    from kanvit import ops
    B, P, K, O, mis = case
    c = restore_cases[case]
    y, mask, pos, idx = _dev(c["y"], mis), _dev(c["mask"]), _dev(c["pos"]), _dev(c["idx"])
    composed = ref.restore_torch(y, mask, pos, idx)
    if mis:
        out = _restore_raw(y, mask, pos, idx, _dev(np.zeros((B, P + 1, O), np.float32), True))
    else:
        out = ops.restore_tokens(y, mask.view(1, O), pos, idx)
        assert y.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert out.shape == (B, P + 1, O) and out.dtype == torch.float32
    assert np.array_equal(_bits(out), c["want"].view(np.uint32))
    assert np.array_equal(_bits(out), _bits(composed))


@pytest.mark.parametrize("case", RESTORE, ids=lambda c: "x".join(map(str, c[:4])) + ("-4byte" if c[4] else ""))
def test_restore_backward_copies_and_sums_in_a_fixed_tree(case, restore_cases):
    B, P, K, O, mis = case
    c = restore_cases[case]
    dout, idx = _dev(c["dout"], mis), _dev(c["idx"])
    want_dy, want_dmask, dropped = ref.restore_bwd(c["dout"], c["idx"])
    runs = []
    for _ in range(2):
        dy = _dev(np.full((B, K + 1, O), np.nan, np.float32), mis)
        dmask = torch.full((O,), float("nan"), device=DEV)
        _restore_bwd_raw(dout, idx, dy, dmask)
        runs.append((dy, dmask))
    (dy, dmask), (dy2, dmask2) = runs
    assert np.array_equal(_bits(dy), want_dy.view(np.uint32))
    assert np.array_equal(_bits(dmask), _bits(dmask2)) and np.array_equal(_bits(dy), _bits(dy2))
    n = B * (P - K)
    bound = (n - 1) * 2.0 ** -24 * (np.abs(c["dout"][:, 1:].astype(np.float64)) * dropped[:, :, None]).sum((0, 1))
    err = np.abs(dmask.cpu().numpy().astype(np.float64) - want_dmask)
    one_row = np.abs(c["dout"][:, 1:][dropped]).min(0)                       # what a missing or doubled row would cost at least
    print(f"{case}: dmask error {err.max():.2e}, bound {bound.min():.2e}..{bound.max():.2e}, smallest row entry {one_row.max():.2e}")
    assert (err <= bound).all()
    # either output alone: the other pointer NULL
    only_dy = _dev(np.full((B, K + 1, O), np.nan, np.float32), mis)
    _restore_bwd_raw(dout, idx, only_dy, None)
    only_dmask = torch.full((O,), float("nan"), device=DEV)
    _restore_bwd_raw(dout, idx, None, only_dmask)
    assert np.array_equal(_bits(only_dy), _bits(dy)) and np.array_equal(_bits(only_dmask), _bits(dmask))


def test_restore_autograd_and_operand_checks(restore_cases):
    from kanvit import KanvitError, ops
    case = RESTORE[1]
    B, P, K, O, _ = case
    c = restore_cases[case]
    y, mask = _dev(c["y"]).requires_grad_(True), _dev(c["mask"]).view(1, O).requires_grad_(True)
    pos, idx, dout = _dev(c["pos"]), _dev(c["idx"]), _dev(c["dout"])
    ops.restore_tokens(y, mask, pos, idx).backward(dout)
    y0, mask0 = _dev(c["y"]).requires_grad_(True), _dev(c["mask"]).view(1, O).requires_grad_(True)
    ref.restore_torch(y0, mask0, pos, idx).backward(dout)
    assert torch.equal(y.grad, y0.grad) and mask.grad.shape == (1, O)
    assert float((mask.grad - mask0.grad).abs().max()) <= 1e-5 * float(mask0.grad.abs().max())
    only_y = _dev(c["y"]).requires_grad_(True)
    ops.restore_tokens(only_y, mask.detach(), pos, idx).backward(dout)
    assert torch.equal(only_y.grad, y.grad)
    with pytest.raises(KanvitError, match="dtype"):
        ops.restore_tokens(y.detach(), mask.detach(), pos, idx.long())
    with pytest.raises(KanvitError, match="shape"):
        ops.restore_tokens(y.detach()[:, :-1], mask.detach(), pos, idx)
    with pytest.raises(KanvitError, match="mask_token"):
        ops.restore_tokens(y.detach(), mask.detach()[:, :-1], pos, idx)


# ---- the loss -------------------------------------------------------------------------------------------------------------------------
# (C, H, W, n_patches, B): I = 12 (less than a wave), 48, 49 (odd: 7-float patch lines at unaligned addresses), 768, 3072; the last case
# has more rows of pred than MAE_ROW_GRID work-groups of four rows take in one lap
LOSS = [(3, 8, 8, 4, 3), (3, 16, 16, 4, 3), (1, 28, 28, 4, 3), (3, 32, 32, 2, 3), (3, 64, 64, 2, 3), (3, 8, 8, 4, 500)]
assert LOSS[-1][4] * (LOSS[-1][3] ** 2 + 1) > ROW_GRID * 4


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def _loss_inputs(shape, K, misaligned):
    c, h, w, n, B = shape
    P, I = n * n, c * (h // n) * (w // n)
    rng = np.random.default_rng(h * 100 + c * 10 + K)
    images = rng.standard_normal((B, c, h, w)).astype(np.float32)
    pred = rng.standard_normal((B, P + 1, I)).astype(np.float32)
    idx = ref.keep_table(B, P, K)
    # a constant patch among the dropped ones of sample 0.  0.5: every partial sum of it is exact in fp32 and in float64, so the mean
    # is 0.5 and the normalised target 0 in every precision and order -- the reference's `that = 0` is the exact answer
    p0 = int(np.flatnonzero(~ref.kept_mask(idx, P)[0])[0])
    ph, pw = h // n, w // n
    images[0, :, (p0 // n) * ph:(p0 // n + 1) * ph, (p0 % n) * pw:(p0 % n + 1) * pw] = 0.5
    return images, pred, idx, p0


@pytest.mark.parametrize("misaligned", [False, True], ids=["16byte", "4byte"])
@pytest.mark.parametrize("norm_pix", [True, False], ids=["norm_pix", "raw"])
@pytest.mark.parametrize("shape", LOSS, ids=lambda s: "x".join(map(str, s)))
def test_loss_rows_and_gradient_within_twice_torchs_own_error(shape, norm_pix, misaligned):
    from kanvit import ops
    c, h, w, n, B = shape
    P, I = n * n, c * (h // n) * (w // n)
    for K in sorted({1, P - 1, max(1, P // 4)}):
        images_h, pred_h, idx_h, p0 = _loss_inputs(shape, K, misaligned)
        images, pred, idx = _dev(images_h, misaligned), _dev(pred_h), _dev(idx_h)
        want_loss, want_rows, want_d = ref.mae_loss(pred_h, images_h, idx_h, n, norm_pix, np.float64)
        t_loss, t_rows, t_d = (t.cpu().numpy().astype(np.float64) for t in ref.mae_loss_torch(pred, images, idx, n, norm_pix))
        loss, rows, d = ops.mae_loss_rows(pred, images, idx, n, norm_pix)
        loss2, rows2, d2 = ops.mae_loss_rows(pred, images, idx, n, norm_pix)
        assert rows.shape == (B, P) and d.shape == (B, P + 1, I) and loss.shape == () and d.is_contiguous()
        assert torch.equal(loss, loss2) and np.array_equal(_bits(rows), _bits(rows2)) and np.array_equal(_bits(d), _bits(d2))
        assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(rows).all()) and bool(torch.isfinite(loss))
        rows32, d32 = rows.cpu().numpy(), d.cpu().numpy()
        # the mean kernel given its input, bit for bit; kept rows and the class row are +0 (all bits clear)
        assert np.array_equal(_bits(loss), ref.masked_mean_rows_f32(rows32, B * (P - K)).view(np.uint32))
        kept = ref.kept_mask(idx_h, P)
        assert not rows32.view(np.uint32)[kept].any() and (rows32[~kept] > 0).all()
        assert not d32.view(np.uint32)[:, 0].any() and not d32.view(np.uint32)[:, 1:][kept].any()
        if norm_pix:                                     # the constant patch: target 0, so the gradient is 2 pred / (I B (P - K))
            assert np.allclose(d32[0, 1 + p0], pred_h[0, 1 + p0] * np.float32(2.0 / (I * B * (P - K))), rtol=1e-6, atol=0)
        loss, rows64, d64 = float(loss), rows32.astype(np.float64), d32.astype(np.float64)
        e_loss, e_rows, e_d = abs(float(t_loss) - want_loss), np.abs(t_rows - want_rows).max(), np.abs(t_d - want_d).max()
        k_loss, k_rows, k_d = abs(loss - want_loss), np.abs(rows64 - want_rows), np.abs(d64 - want_d).max()
        top = np.abs(want_d).max()
        print(f"{shape} norm_pix={norm_pix} K={K} {'4-byte' if misaligned else '16-byte'}: loss {want_loss:.6g} torch {e_loss:.2e} kernel "
              f"{k_loss:.2e} | rows torch {e_rows:.2e} kernel {k_rows.max():.2e} | dpred (largest {top:.2e}) torch {e_d:.2e} kernel {k_d:.2e}")
        assert k_loss <= 2 * e_loss + 4 * _ulp(want_loss), (K, k_loss, e_loss)
        assert (k_rows <= 2 * e_rows + 4 * _ulp(want_rows)).all(), (K, k_rows.max(), e_rows)
        assert k_d <= 2 * e_d + 2.0 ** -22 * top, (K, k_d, e_d)


def test_loss_autograd_scales_the_stored_gradient_and_checks_operands():
    from kanvit import KanvitError, ops
    shape = LOSS[1]
    n = shape[3]
    images_h, pred_h, idx_h, _ = _loss_inputs(shape, 4, False)
    images, idx = _dev(images_h), _dev(idx_h)
    pred = _dev(pred_h).requires_grad_(True)
    loss0, _, d0 = ops.mae_loss_rows(pred.detach(), images, idx, n, True)
    loss = ops.mae_loss(pred, images, idx, n)
    assert torch.equal(loss.detach(), loss0)
    (0.5 * loss).backward()
    assert torch.equal(pred.grad, 0.5 * d0)
    with pytest.raises(KanvitError, match="dtype"):
        ops.mae_loss(pred.detach().bfloat16(), images, idx, n)
    with pytest.raises(KanvitError, match="shape"):
        ops.mae_loss(pred.detach()[:, 1:], images, idx, n)
    with pytest.raises(KanvitError, match="contiguous"):
        ops.mae_loss(pred.detach(), images.transpose(2, 3), idx, n)
    with pytest.raises(KanvitError, match="gradient"):
        ops.mae_loss(pred.detach(), images.clone().requires_grad_(True), idx, n)


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def fro(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


PARITY = 1e-4                        # relative Frobenius error of losses and gradients against the restated model


def _mae(kind="vanilla", decoder_type="vanilla", seed=3, **kw):
    from mae import MaskedAutoencoder
    from model import VisionTransformer
    torch.manual_seed(0)
    enc = VisionTransformer((3, 32, 32), 4, 2, 64, 2, 10, type=kind)
    return MaskedAutoencoder(enc, mask_ratio=0.75, decoder_dim=32, decoder_blocks=1, decoder_type=decoder_type, seed=seed, **kw).to(DEV)


def _images(B=4):
    return torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(DEV)


@pytest.mark.parametrize("kind,decoder_type", [("vanilla", "vanilla"), ("cheby", "vanilla"), ("vanilla", "cheby")])
def test_module_loss_and_gradients_against_the_stock_torch_forward(kind, decoder_type):
    from kanvit import ops
    m, x = _mae(kind, decoder_type).train(), _images()
    B, P, K = 4, 16, m.n_keep
    assert K == 4
    loss, pred, idx = m(x, return_pred=True)
    assert pred.shape == (B, P, 192) and idx.shape == (B, K) and idx.dtype == torch.int32
    assert torch.equal(idx.cpu(), ops.patch_keep_ref(B, P, K, 3, 0)) and int(m.mask_counter) == 1
    loss.backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    want = ref.mae_forward_torch(m, x, idx)
    want.backward()
    grads0 = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert set(grads) == set(grads0) and "mask_token" in grads and not any(k.startswith("encoder.mlp_head") for k in grads)
    assert {k for k, _ in m.named_parameters()} - set(grads) == {k for k, _ in m.named_parameters() if k.startswith("encoder.mlp_head")}
    worst = max((fro(grads[k], grads0[k]), k) for k in grads if not (".k_mappings." in k and k.endswith(".bias")))
    print(f"{kind}/{decoder_type}: loss {float(loss):.6f} against {float(want):.6f}, worst gradient {worst[1]} {worst[0]:.2e}")
    assert abs(float(loss) - float(want)) <= PARITY * abs(float(want))
    for k in grads:
        if ".k_mappings." in k and k.endswith(".bias"):
            # a key bias shifts every score of a query by one constant, which softmax ignores: its gradient is mathematically zero and
            # both values are rounding noise, for which a relative norm says nothing.  The bound is taken relative to the gradient of
            # the same layer's weight instead: the bias gradient is zero to within the parity bound of the layer's real gradient
            scale = float(grads0[k[:-len("bias")] + "weight"].double().norm())
            assert float((grads[k].double() - grads0[k].double()).norm()) < PARITY * scale, k
            assert float(grads[k].double().norm()) < PARITY * scale, k
        else:
            assert fro(grads[k], grads0[k]) < PARITY, k


def test_a_new_mask_on_every_call_in_eval_too():
    from kanvit import ops
    m, x = _mae(seed=9), _images()
    with torch.no_grad():
        for step, mode in enumerate((m.train, m.eval, m.eval, m.train)):
            mode()
            _, _, idx = m(x, return_pred=True)
            assert torch.equal(idx.cpu(), ops.patch_keep_ref(4, 16, 4, 9, step)) and int(m.mask_counter) == step + 1
        a = m(x)
        m.mask_counter.fill_(4)
        assert torch.equal(m(x), a)                                    # the same counter: the same mask, the same bits
        assert not torch.equal(m(x), a)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = m.train()(x)
    loss.backward()
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss)) and bool(torch.isfinite(m.mask_token.grad).all())


def test_a_bare_vision_transformer_still_runs_its_own_patch_dropout():
    """_embed_kept without a table draws its own, as before: twice with equal counters gives equal bits, the sequence is the torch
    restatement's bit for bit, and a table handed in replaces the draw without moving the counter."""
    from kanvit import ops
    from model import VisionTransformer
    torch.manual_seed(0)
    m, x = VisionTransformer((3, 32, 32), 4, 2, 64, 2, 10, type="vanilla").to(DEV).train(), _images()
    K = m.set_patch_dropout(0.5, seed=3)
    with torch.no_grad():
        y1 = m(x)
        assert int(m.patch_dropout_counter) == 1
        m.patch_dropout_counter.zero_()
        assert torch.equal(m(x), y1)
        m.patch_dropout_counter.zero_()
        out, rows = m._embed_kept(x)
        idx = ops.patch_keep_ref(4, 16, K, 3, 0)
        out_t, rows_t = m._embed_kept_torch(x, idx)
        assert torch.equal(out, out_t) and torch.equal(rows, rows_t)
        out_i, _ = m._embed_kept(x, idx.to(DEV))
        assert torch.equal(out_i, out) and int(m.patch_dropout_counter) == 1
        other = ops.patch_keep_ref(4, 16, 3, 11, 0).to(DEV)             # another K than the one that is set: the table decides
        assert m._embed_kept(x, other)[0].shape == (4, 4, 64) and int(m.patch_dropout_counter) == 1


@pytest.mark.parametrize("norm_pix", [True, False])
def test_reconstruct_leaves_kept_patches_alone(norm_pix):
    m, x = _mae("cheby", norm_pix_loss=norm_pix).train(), _images()
    rec, idx = m.reconstruct(x)
    assert m.training and rec.shape == x.shape and int(m.mask_counter) == 1 and bool(torch.isfinite(rec).all())
    kept = torch.from_numpy(ref.kept_mask(idx.cpu().numpy(), 16)).to(DEV)
    a, b = m.encoder.patchify(rec, 4), m.encoder.patchify(x, 4)
    assert torch.equal(a[kept], b[kept])
    assert bool((a[~kept] != b[~kept]).any(dim=-1).all())


# ---- train.py -------------------------------------------------------------------------------------------------------------------------
FLAGS = ["--synthetic", "--pretrain", "mae", "--epochs", "1", "--steps-per-epoch", "6", "--model-type", "cheby", "--seed", "7"]


def test_graphed_pretraining_equals_eager_and_every_replay_draws_a_new_mask(tmp_path):
    import train
    eager = train.main(train.parse([*FLAGS, "--log-dir", str(tmp_path / "e")]))
    graphed = train.main(train.parse([*FLAGS, "--graph", "--log-dir", str(tmp_path / "g")]))
    print("eager", eager["losses"], "graphed", graphed["losses"])
    assert len(eager["losses"]) == 6 and eager["losses"] == graphed["losses"] and all(np.isfinite(eager["losses"]))
    assert int(eager["model"].mask_counter) == 6 and int(graphed["model"].mask_counter) == 6
    assert len(eager["epoch_loss"]) == 1 and not eager["train_metrics"] and "test_metrics" not in eager
    we, wg = eager["model"].state_dict(), graphed["model"].state_dict()
    assert list(we) == list(wg) and all(torch.equal(we[k], wg[k]) for k in we)
    # one batch six times with the weights held still (learning rate 0): only the mask can move the loss
    g = torch.Generator().manual_seed(1)
    batch = (torch.randn(128, 3, 32, 32, generator=g).to(DEV), torch.zeros(128, dtype=torch.int64, device=DEV))
    still = train.main(train.parse([*FLAGS, "--graph", "--learning-rate", "0", "--log-dir", str(tmp_path / "s")]), batches=[batch] * 6)
    print("one batch, fixed weights:", still["losses"])
    assert len(set(still["losses"])) == 6 and int(still["model"].mask_counter) == 6


def test_pretraining_under_bf16_autocast_runs(tmp_path):
    import train
    h = train.main(train.parse([*FLAGS, "--amp", "bf16", "--log-dir", str(tmp_path / "a")]))
    assert len(h["losses"]) == 6 and all(np.isfinite(h["losses"]))


def test_the_averaged_encoder_is_handed_to_a_supervised_run(tmp_path):
    import train
    path = str(tmp_path / "encoder.pt")
    pre = train.main(train.parse([*FLAGS, "--optimizer", "kanvit-adamw", "--ema-decay", "0.99", "--save-encoder", path, "--log-dir", str(tmp_path / "p")]))
    saved = torch.load(path, weights_only=True)
    enc = pre["model"].encoder
    assert list(saved) == list(enc.state_dict())
    with pre["optimizer"].ema_weights(pre["model"]):
        averaged = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    assert all(torch.equal(saved[k], averaged[k]) for k in saved)                  # the weights evaluate() would use,
    assert not torch.equal(saved["v_class"], enc.v_class.detach().cpu())           # not the raw ones
    head = enc.mlp_head[1].weight                                                  # frozen in pretraining: no gradient, no average, as initialised
    assert not head.requires_grad and torch.equal(saved["mlp_head.1.weight"], head.detach().cpu()) and bool(head.abs().sum() > 0)
    sup = ["--synthetic", "--epochs", "1", "--steps-per-epoch", "1", "--model-type", "cheby", "--seed", "7", "--learning-rate", "0", "--no-step-metrics"]
    loaded = train.main(train.parse([*sup, "--init-encoder", path, "--log-dir", str(tmp_path / "l")]))["model"].state_dict()
    fresh = train.main(train.parse([*sup, "--log-dir", str(tmp_path / "f")]))["model"].state_dict()
    assert list(loaded) == list(saved)
    for k in loaded:
        if k.startswith("mlp_head."):
            assert torch.equal(loaded[k], fresh[k]), k                             # the head is the fresh initialisation of the seed
        else:
            assert torch.equal(loaded[k].cpu(), saved[k]), k
    assert not torch.equal(loaded["v_class"], fresh["v_class"])
