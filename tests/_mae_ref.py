"""Restatements of the masked-autoencoder kernels (csrc/mae.hip) for the tests: NumPy in a chosen precision, the stock torch compositions
the kernels replace, and a stock-torch forward of a MaskedAutoencoder from the module's own parameters and a given keep table."""
import numpy as np
import torch

from tests._mix_ref import mean_rows_f32


# ---- keep tables ----------------------------------------------------------------------------------------------------------------------
def keep_table(B, P, K, seed=0):
    """A hand-built int32 [B, K] table, every row strictly ascending: row 0 keeps the first K patches (patch 0 among them), row 1 the
    last K (patch P - 1 among them), the others K random ones."""
    rng = np.random.default_rng(1000 * B + 10 * P + K + seed)
    rows = []
    for b in range(B):
        if b == 0:
            rows.append(np.arange(K))
        elif b == 1:
            rows.append(np.arange(P - K, P))
        else:
            rows.append(np.sort(rng.choice(P, K, replace=False)))
    if B == 1 and K >= 2:                                   # one sample only: both ends in it
        rows[0] = np.sort(np.concatenate(([0, P - 1], rng.choice(np.arange(1, P - 1), K - 2, replace=False))))
    return np.stack(rows).astype(np.int32)


def kept_mask(idx, P):
    """bool [B, P]: True where the patch is kept."""
    m = np.zeros((idx.shape[0], P), bool)
    np.put_along_axis(m, idx.astype(np.int64), True, axis=1)
    return m


# ---- restore --------------------------------------------------------------------------------------------------------------------------
def restore(y, mask_token, pos, idx):
    """out[b, 0] = y[b, 0] + pos[0]; out[b, 1 + p] = (y[b, 1 + j] if p == idx[b, j] else mask_token) + pos[1 + p], in the inputs' dtype:
    one add per element."""
    B, K = idx.shape
    P = pos.shape[0] - 1
    src = np.broadcast_to(mask_token.reshape(1, 1, -1), (B, P + 1, y.shape[-1])).copy()
    src[:, 0] = y[:, 0]
    for b in range(B):
        src[b, 1 + idx[b]] = y[b, 1:]
    return src + pos[None]


def restore_torch(y, mask_token, pos, idx):
    """The stock composition (He et al.'s decoder input): repeat + cat + argsort of the keep table + gather + add."""
    B, K = idx.shape
    P, O = pos.shape[0] - 1, y.shape[-1]
    noise = torch.ones(B, P, device=y.device).scatter_(1, idx.long(), 0.0)
    ids_restore = torch.argsort(torch.argsort(noise, dim=1, stable=True), dim=1)          # kept first, each group ascending
    x = torch.cat([y[:, 1:], mask_token.reshape(1, 1, O).repeat(B, P - K, 1)], dim=1)
    x = torch.gather(x, 1, ids_restore.unsqueeze(-1).expand(B, P, O))
    return torch.cat([y[:, :1], x], dim=1) + pos


def restore_bwd_torch(dout, idx):
    """The stock backward of restore_torch, (dy [B, K + 1, O], dmask [O]), as autograd runs it: gather's backward is an unordered
    scatter_add into zeros, cat's are slices, repeat's is a sum."""
    B, K = idx.shape
    P, O = dout.shape[1] - 1, dout.shape[-1]
    noise = torch.ones(B, P, device=dout.device).scatter_(1, idx.long(), 0.0)
    ids_restore = torch.argsort(torch.argsort(noise, dim=1, stable=True), dim=1)
    g = torch.zeros(B, P, O, device=dout.device).scatter_add_(1, ids_restore.unsqueeze(-1).expand(B, P, O), dout[:, 1:])
    return torch.cat([dout[:, :1], g[:, :K]], dim=1), g[:, K:].sum(dim=(0, 1))


def restore_bwd(dout, idx):
    """(dy [B, K + 1, O] in dout's dtype: copies; dmask [O] float64: the sum of the dropped rows)."""
    B, K = idx.shape
    P = dout.shape[1] - 1
    dy = np.empty((B, K + 1, dout.shape[-1]), dout.dtype)
    dy[:, 0] = dout[:, 0]
    for b in range(B):
        dy[b, 1:] = dout[b, 1 + idx[b]]
    dropped = ~kept_mask(idx, P)
    return dy, (dout[:, 1:].astype(np.float64) * dropped[:, :, None]).sum((0, 1)), dropped


# ---- the loss -------------------------------------------------------------------------------------------------------------------------
def patchify(images, n):
    """(B, C, H, W) -> (B, n^2, C*ph*pw): VisionTransformer.patchify in NumPy."""
    b, c, h, w = images.shape
    ph, pw = h // n, w // n
    return images.reshape(b, c, n, ph, n, pw).transpose(0, 2, 4, 1, 3, 5).reshape(b, n * n, c * ph * pw)


def masked_mean_rows_f32(rows, divisor, threads=256):
    """mae_mean_kernel in NumPy float32: soft_ce_mean_kernel's ordered sum of all entries of rows (tests/_mix_ref.py: mean_rows_f32 --
    thread t adds entries t, t + 256, ... in order, then part[:o] += part[o:2o] for o = 128 .. 1), then one float32 division by
    float32(divisor), the number of masked patches."""
    rows = np.asarray(rows).reshape(-1)
    assert rows.dtype == np.float32 and rows.size >= 1
    part = np.zeros(threads, np.float32)
    for lo in range(0, rows.size, threads):
        blk = rows[lo:lo + threads]
        part[:blk.size] = part[:blk.size] + blk
    o = threads // 2
    while o:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    out = part[0] / np.float32(divisor)
    assert out.dtype == np.float32
    return out


def mae_loss(pred, images, idx, n, norm_pix=True, dtype=np.float64):
    """(loss, rows [B, P], dpred [B, P + 1, I]) in `dtype`.  pred [B, P + 1, I] with its class row; for a dropped patch: the target
    normalised by its own mean and unbiased variance under norm_pix, rows = mean_i (pred - target)^2, dpred = 2 (pred - target) / (I B
    (P - K)); kept entries and the class row are 0; loss = sum(rows) / (B (P - K)) -- in float32 through masked_mean_rows_f32."""
    t = patchify(np.asarray(images), n).astype(dtype)
    z = np.asarray(pred).astype(dtype)[:, 1:]
    B, P, I = t.shape
    K = idx.shape[1]
    if norm_pix:
        mu = t.mean(-1, keepdims=True, dtype=dtype)
        var = ((t - mu) ** 2).sum(-1, keepdims=True, dtype=dtype) / dtype(I - 1)
        t = (t - mu) / np.sqrt(var + dtype(1e-6))
    dropped = ~kept_mask(idx, P)
    d = (z - t) * dropped[:, :, None]
    rows = ((d * d).sum(-1, dtype=dtype) / dtype(I)).astype(dtype)
    dpred = np.zeros((B, P + 1, I), dtype)
    dpred[:, 1:] = d * dtype(2.0 / (I * B * (P - K)))
    if dtype == np.float32:
        return masked_mean_rows_f32(rows, B * (P - K)), rows, dpred
    return rows.sum() / (B * (P - K)), rows, dpred


def mae_loss_composition(z, images, idx, n, norm_pix=True):
    """The stock fp32 forward, (loss, rows [B, P]), differentiable in z [B, P + 1, I]: patchify of the whole batch, mean, var, normalise,
    subtract, square, two means and a mask multiply (He et al.'s forward_loss)."""
    b, c, h, w = images.shape
    ph, pw = h // n, w // n
    target = images.reshape(b, c, n, ph, n, pw).permute(0, 2, 4, 1, 3, 5).reshape(b, n * n, c * ph * pw)
    if norm_pix:
        mean, var = target.mean(dim=-1, keepdim=True), target.var(dim=-1, keepdim=True)
        target = (target - mean) / (var + 1.0e-6) ** 0.5
    mask = torch.ones(b, n * n, device=z.device).scatter_(1, idx.long(), 0.0)              # 1 = dropped
    rows = ((z[:, 1:] - target) ** 2).mean(dim=-1) * mask
    return rows.sum() / mask.sum(), rows


def mae_loss_torch(pred, images, idx, n, norm_pix=True):
    """mae_loss_composition on pred's device, forward and backward.  Returns (loss, rows [B, P], dpred [B, P + 1, I])."""
    z = pred.detach().clone().requires_grad_(True)
    loss, rows = mae_loss_composition(z, images, idx, n, norm_pix)
    loss.backward()
    return loss.detach(), rows.detach(), z.grad


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def mae_forward_torch(mae, images, idx):
    """The loss of MaskedAutoencoder.forward for the keep table idx, from the module's own parameters with stock torch ops around the
    blocks: the torch-restated kept-patch embedding (VisionTransformer._embed_kept_torch), every block's plain forward, nn.LayerNorm,
    restore_torch and mae_loss_torch's composition -- no fused add + norm, no restore or loss kernel."""
    enc = mae.encoder
    x, _ = enc._embed_kept_torch(images, idx)
    for blk in enc.blocks:
        x = blk(x)
    y = mae.decoder_embed(mae.enc_norm(x))
    x = restore_torch(y.float(), mae.mask_token, mae.decoder_pos, idx)
    for blk in mae.decoder_blocks:
        x = blk(x)
    pred = mae.decoder_pred(mae.decoder_norm(x)).float()
    return mae_loss_composition(pred, images, idx, enc.n_patches, mae.norm_pix_loss)[0]


__all__ = ["keep_table", "kept_mask", "restore", "restore_torch", "restore_bwd", "restore_bwd_torch", "patchify", "masked_mean_rows_f32", "mae_loss",
           "mae_loss_composition", "mae_loss_torch", "mae_forward_torch", "mean_rows_f32"]
