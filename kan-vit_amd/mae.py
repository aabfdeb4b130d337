"""MaskedAutoencoder -- self-supervised pretraining of a VisionTransformer (He et al. 2022, "Masked Autoencoders Are Scalable Vision
Learners").  The reference has no such mode.  The encoder is a VisionTransformer used as it is: it embeds and runs only the K kept
patches of every sample plus the class token (PatchDropout's keep table, gather and assembly); a light decoder of the same
TransformerBlocks gets the full sequence back -- mask tokens at the dropped positions (kanvit.ops.restore_tokens) -- and predicts the
dropped patches' pixels, which the masked-patch loss (kanvit.ops.mae_loss) compares with the images directly.  The state_dict keys of
the encoder appear under `encoder.`: encoder.state_dict() is what a supervised run loads (train.py --save-encoder / --init-encoder)."""
import torch
import torch.nn as nn

from kanvit import _lib, ops
from kanvit.ops import add_layernorm
from model import _NO_DROP, TransformerBlock, VisionTransformer


class MaskedAutoencoder(nn.Module):
    def __init__(self, encoder, mask_ratio=0.75, decoder_dim=None, decoder_blocks=2, decoder_heads=None, decoder_type="vanilla",
                 norm_pix_loss=True, seed=0):
        """encoder: a VisionTransformer of any type but 'flash-attn' (whose bare attention modules have no pending residual to fold
        into a norm).  Every sample keeps K = max(1, int(P * (1 - mask_ratio))) of its P patches -- set_patch_dropout's rule; a ratio
        that keeps all P is refused.  decoder_dim: None = max(32, d_hidden // 2) rounded up to a multiple of the head count;
        decoder_heads: None = the encoder's; decoder_type: the attention type of the decoder blocks, any the TransformerBlock takes;
        norm_pix_loss: normalise every target patch by its own mean and variance.  seed: of the mask hash (under data parallelism a
        rank's own: kanvit.data.rank_seed)."""
        super().__init__()
        if not isinstance(encoder, VisionTransformer):
            raise TypeError(f"MaskedAutoencoder: encoder is a VisionTransformer, got {type(encoder).__name__}")
        if not all(isinstance(blk, TransformerBlock) for blk in encoder.blocks):
            raise NotImplementedError("MaskedAutoencoder: 'flash-attn' models stack bare FlashAttention modules (model.py:113-117), which "
                                      "the kept-token walk does not cover")
        mask_ratio = float(mask_ratio)
        if not 0.0 <= mask_ratio < 1.0:
            raise ValueError(f"MaskedAutoencoder: mask_ratio {mask_ratio} must be in [0, 1)")
        P = encoder.n_patches ** 2
        K = max(1, int(P * (1.0 - mask_ratio)))
        if K >= P:
            raise ValueError(f"MaskedAutoencoder: mask_ratio {mask_ratio} keeps all {P} patches: nothing is left to reconstruct")
        if P > _lib.PATCH_KEEP_MAX_P:
            raise NotImplementedError(f"MaskedAutoencoder: {P} patches per image; one patch_keep launch ranks {_lib.PATCH_KEEP_MAX_P}")
        if encoder.input_d > _lib.MAE_MAX_I:
            raise NotImplementedError(f"MaskedAutoencoder: {encoder.input_d} values per patch; the loss kernel holds {_lib.MAE_MAX_I}")
        heads = int(decoder_heads) if decoder_heads else encoder.n_heads
        dd = int(decoder_dim) if decoder_dim else -(-max(32, encoder.d_hidden // 2) // heads) * heads
        if heads < 1 or dd < 1 or dd % heads:
            raise ValueError(f"MaskedAutoencoder: decoder_dim {dd} is not a positive multiple of decoder_heads {heads}")
        self.encoder = encoder
        self.mask_ratio, self.n_keep, self.norm_pix_loss, self.seed = mask_ratio, K, bool(norm_pix_loss), int(seed)
        self.decoder_dim = dd
        d = encoder.d_hidden
        self.enc_norm = nn.LayerNorm(d)
        self.decoder_embed = nn.Linear(d, dd)
        self.mask_token = nn.Parameter(torch.zeros(1, dd))
        nn.init.normal_(self.mask_token, std=0.02)
        self.decoder_blocks = nn.ModuleList([TransformerBlock(dd, heads, feedforward_dim=4 * dd, attn_type=decoder_type)
                                             for _ in range(int(decoder_blocks))])
        self.decoder_norm = nn.LayerNorm(dd)
        self.decoder_pred = nn.Linear(dd, encoder.input_d)
        self.register_buffer("decoder_pos", encoder.positional_embeddings(P + 1, dd), persistent=False)
        # the mask hash's call counter, like patch_dropout_counter: on the device, stepped by the launch, not in state_dict()
        self.register_buffer("mask_counter", torch.zeros(1, dtype=torch.int64), persistent=False)

    def _encode(self, images, idx):
        """enc_norm of the encoder's stream on the K + 1 kept rows, [B, K + 1, d]: the kept-patch embedding with the given table, every
        block on every row (no class-token tail: the decoder reads all rows), the encoder's own drop-path if it is set, and the last
        block's pending residual add inside the norm pass."""
        enc = self.encoder
        out, _ = enc._embed_kept(images, idx)
        scales = None
        if enc._drop_path is not None and enc.training:
            scales = ops.depth_scales(out.shape[0], enc._drop_path[0], enc._drop_path[1], enc.drop_path_counter)
        pending = None
        for l, blk in enumerate(enc.blocks):
            drop = _NO_DROP if scales is None else (scales[2 * l - 1] if l else None, scales[2 * l], scales[2 * l + 1])
            out, pending = blk.run(out, pending, drop=drop)
        return add_layernorm(out, pending, self.enc_norm, row_scale=None if scales is None or pending is None else scales[-1])[1]

    def _decode(self, latent, idx):
        """The decoder head's output [B, P + 1, I] (the class row in place) from enc_norm's rows."""
        out = ops.restore_tokens(self.decoder_embed(latent), self.mask_token, self.decoder_pos, idx)
        pending = None
        for blk in self.decoder_blocks:
            out, pending = blk.run(out, pending)
        return self.decoder_pred(add_layernorm(out, pending, self.decoder_norm)[1])

    def forward(self, images, return_pred=False):
        """The reconstruction loss of one batch (0-d); with return_pred=True, (loss, the predicted patches [B, P, I], the keep table
        int32 [B, K]).  A new mask is drawn on every call, in train() and eval() alike (one ops.patch_keep launch, which steps
        mask_counter on the device: a captured step draws a new mask at every replay).  images: float32 [B, C, H, W] on the model's
        GPU; they are data and get no gradient."""
        enc = self.encoder
        if not torch.is_tensor(images) or images.dim() != 4:
            raise ops.KanvitOperandError("MaskedAutoencoder: images is a float32 [B, C, H, W] tensor on the GPU")
        ops._require_tensor("MaskedAutoencoder", "images", images, torch.float32, contiguous=False, error=ops.KanvitOperandError)
        if images.requires_grad:
            raise ops.KanvitOperandError("MaskedAutoencoder: images that want a gradient are not supported: the targets are data")
        images = images.contiguous()
        idx = ops.patch_keep(images.shape[0], enc.n_patches ** 2, self.n_keep, self.seed, self.mask_counter)
        pred = self._decode(self._encode(images, idx), idx)
        loss = ops.mae_loss(pred.float(), images, idx, enc.n_patches, self.norm_pix_loss)       # bf16 under autocast: the loss takes fp32
        if return_pred:
            return loss, pred[:, 1:], idx
        return loss

    def unpatchify(self, patches):
        """(B, P, C*ph*pw) -> (B, C, H, W): the inverse of VisionTransformer.patchify."""
        enc = self.encoder
        (c, h, w), n, (ph, pw) = enc.chw, enc.n_patches, enc.patch_size
        return patches.reshape(-1, n, n, c, ph, pw).permute(0, 3, 1, 4, 2, 5).reshape(-1, c, h, w)

    @torch.no_grad()
    def reconstruct(self, images):
        """(the image batch with the predicted patches pasted in at the dropped positions, the keep table): one eval() forward without
        gradients; under norm_pix_loss a prediction is brought back to pixel scale with its target patch's own mean and variance.
        Kept patches are the input's, unchanged.  Stock torch ops around the forward -- for looking at, not a hot path; leaves the
        training / eval mode as it finds it."""
        was_training = self.training
        self.eval()
        try:
            _, pred, idx = self(images, return_pred=True)
        finally:
            self.train(was_training)
        patches = self.encoder.patchify(images, self.encoder.n_patches)
        pred = pred.float()
        if self.norm_pix_loss:
            pred = pred * (patches.var(dim=-1, keepdim=True) + 1e-6).sqrt() + patches.mean(dim=-1, keepdim=True)
        kept = torch.zeros(patches.shape[:2], dtype=torch.bool, device=images.device).scatter_(1, idx.long(), True)
        return self.unpatchify(torch.where(kept.unsqueeze(-1), patches, pred)), idx
