"""VisionTransformer / TransformerBlock -- drop-ins for the reference's model.py:14-169.

Same constructor, same state_dict keys; the KAN patch embedding and the per-head KAN q/k/v
mappings + attention run in the HIP kernels (through models/*.py and attention.py).  The
feed-forward block and the LayerNorms are stock dense ops (hipBLASLt / MIOpen through torch) --
they are not KAN kernels."""
import torch
import torch.nn as nn

from attention import MSA, FlashAttention
from kanvit import _lib, ops
from kanvit.dense import feed_forward, ff_mode, ff_small_supported, ln_feed_forward
from kanvit.ops import add_layernorm
from kanvit.prune import EdgePruning
from models.cheby import ChebyKANLayer
from models.effkan import KANLinear
from models.fastkan import FastKANLayer
from models.nfkan import NaiveFourierKANLayer
from models.sinekan import SineKANLayer


_NO_DROP = (None, None, None)      # TransformerBlock.run / run_cls: the scale rows of stochastic depth, off


class TransformerBlock(nn.Module):
    """x + MSA(LN(x)), then x + FF(LN(x)) (model.py:31-37)."""

    def __init__(self, d_model, n_heads, feedforward_dim=128, attn_type="vanilla"):
        super().__init__()
        self.norm1 = nn.LayerNorm(d_model)
        self.attn = MSA(d_model, n_heads, type=attn_type)
        self.norm2 = nn.LayerNorm(d_model)
        self.ff = nn.Sequential(nn.Linear(d_model, feedforward_dim), nn.ReLU(inplace=True),
                                nn.Linear(feedforward_dim, d_model))

    def forward(self, x):
        x, f = self.run(x, None)
        return x + f

    @torch.no_grad()
    def attention_map(self, x, rows=None):
        """[B, H, R, N]: the attention probabilities of this block's heads on the stream x the block receives
        (MSA.attention_map of norm1(x))."""
        return self.attn.attention_map(self.norm1(x), rows)

    def run(self, x, pending, reg=None, drop=_NO_DROP):
        """The block with its residual adds fused into the LayerNorms (kanvit.ops.add_layernorm: one pass instead of an
        add kernel + a LayerNorm kernel forward, one pass instead of three + an add backward).  `pending` is the previous
        block's feed-forward output that has not been added to the stream yet (None for the first block); returns
        (stream after the attention add, this block's feed-forward output) -- same arithmetic as model.py:31-37:
            x = x + MSA(LN1(x));  x = x + FF(LN2(x)).
        reg (a dict of MSA.regularization_loss keywords, or None): also return, as a third value, the sample-based KAN
        regulariser of the per-head q|k|v layers on the rows they read, LN1(x) -- the tensor this forward already holds.
        drop (stochastic depth, VisionTransformer.set_drop_path; all None = off): (the [B] scale row of the branch `pending` is --
        the previous block's feed-forward -- or None, the [B] scale row of this block's attention branch, ...).  Each fused add takes
        the row of the branch it adds; the returned feed-forward output is unscaled, like `pending`."""
        x, h1 = add_layernorm(x, pending, self.norm1, row_scale=None if pending is None else drop[0])
        if reg is not None:
            return self._rest(x, h1, drop[1]) + (self.attn.regularization_loss(h1, **reg),)
        return self._rest(x, h1, drop[1])

    def _rest(self, x, h1, attn_scale):
        if attn_scale is None and x.dim() == 3 and ff_small_supported(self.ff[0].in_features, self.ff[0].out_features):
            # small geometries: residual add + LN2 + feed-forward in one launch; ln_feed_forward itself falls
            # back to add_layernorm + feed_forward for inputs the fused kernel refuses (dtype, autocast, row count)
            return ln_feed_forward(x, self.attn(h1), self.norm2, self.ff[0], self.ff[2])
        # under bf16 autocast the stock feed-forward GEMMs take bf16 operands: LN2 writes its output as bf16 directly, and the bf16
        # feed-forward output comes back into the next block's add_layernorm as it is (no cast passes in either direction)
        ybf = (x.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16 and ff_mode() != "bf16x3")
        # a scaled attention branch comes here also at the small geometries: the one-launch LN2 + feed-forward has no scaled form
        x, h2 = add_layernorm(x, self.attn(h1), self.norm2, y_bf16=ybf, row_scale=attn_scale)
        # Same three ops as self.ff (Linear -> ReLU(inplace) -> Linear, model.py:25-29), applied to the 2-D
        # (B*N, d) tensor: nn.Linear on 3-D input returns a VIEW, and an in-place ReLU on a view makes autograd
        # insert CopySlices (two full [B*N, 4d] copies per block in backward: 12 ms/step at ViT-B, B=128).
        # The two Linears go through kanvit.dense: stock GEMMs, but with the weight gradient split over tokens
        # (the unsplit library kernel fills 36 of 256 CUs: 2.2 ms -> 0.83 ms per call).
        b, n, d = x.shape
        return x, feed_forward(h2.reshape(b * n, d), self.ff[0], self.ff[2]).view(b, n, d)   # bias + ReLU in the GEMM epilogue


    def run_cls(self, x, pending, drop=_NO_DROP):
        """The class-token row [B, d] of x + MSA(LN1(x)) + FF(LN2(.)) after the pending add, i.e. forward(x + pending)[:, 0]:
        all the head of a ViT reads of its last block (model.py:166-169).  LN1 still runs on all rows (k and v need them); the
        q layers, the attention, the residual, LN2 and the feed-forward run on the B class rows only (MSA.forward_cls).  Under
        bf16 autocast the grouped q|k|v launch and the attention stay what they are in run() -- all rows, on the bf16 matrix
        cores, the rounding points the bf16 results are specified with -- and LN2 + feed-forward take the class rows.
        drop (stochastic depth; all None = off): run()'s pair and, third, the scale row of this block's feed-forward branch.  The
        pending add takes its row inside the fused pass; the two [B, d] class-row branches are scaled by a plain multiply."""
        x, h1 = add_layernorm(x, pending, self.norm1, row_scale=None if pending is None else drop[0])
        ybf = (x.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16)
        a0 = _FirstRow.apply(self.attn(h1)) if ybf else self.attn.forward_cls(h1)
        if drop[1] is not None:
            a0 = a0 * drop[1].unsqueeze(1)
        s, h2 = add_layernorm(_FirstRow.apply(x), a0, self.norm2, y_bf16=ybf and ff_mode() != "bf16x3")
        f = feed_forward(h2, self.ff[0], self.ff[2])
        return s + (f if drop[2] is None else f * drop[2].unsqueeze(1))


class _FirstRow(torch.autograd.Function):
    """t[:, 0] of t [B, N, d] whose backward is ONE padding launch (g in row 0, zeros below) -- the one full-size pass the
    gradient of the class row costs on its way back into the stream."""

    @staticmethod
    def forward(ctx, t):
        ctx.n = t.shape[1]
        return t[:, 0].contiguous()

    @staticmethod
    def backward(ctx, g):
        return torch.nn.functional.pad(g.unsqueeze(1), (0, 0, 0, ctx.n - 1))


class _ClsToken(torch.autograd.Function):
    """out[:, 0] + pending[:, 0] (model.py:166-169 reads only the class token; the last block's feed-forward output is still
    pending, TransformerBlock.run).  The two inputs receive the SAME gradient -- g in row 0, zeros elsewhere -- so backward builds
    it once, as ONE padding launch (the small geometries count launches)."""

    @staticmethod
    def forward(ctx, out, pending):
        ctx.shape = out.shape
        ctx.pdtype = pending.dtype
        return out[:, 0] + pending[:, 0]

    @staticmethod
    def backward(ctx, g):
        full = torch.nn.functional.pad(g.unsqueeze(1), (0, 0, 0, ctx.shape[1] - 1))      # [B, N, d]: g in row 0, zeros below
        return full, (full if ctx.pdtype == full.dtype else full.to(ctx.pdtype))      # a bf16 feed-forward output under autocast


def _patch_embedding(kind, in_dim, d):
    if kind in ("vanilla", "flash-attn"):
        return nn.Linear(in_dim, d)
    if kind == "efficientkan":
        return KANLinear(in_dim, d)
    if kind == "sine":
        return SineKANLayer(in_dim, d, grid_size=28)
    if kind == "fourier":
        return NaiveFourierKANLayer(in_dim, d, grid_size=28)     # works here; crashes in the reference (D4)
    if kind == "cheby":
        return ChebyKANLayer(in_dim, d, 4)
    if kind == "fast":
        return FastKANLayer(in_dim, d)
    raise ValueError(f"Unknown transformer type: {kind}")


def split_types(kind: str):
    """'sine' -> ['sine'];  'sine,fourier' (or 'sine+fourier') -> ['sine', 'fourier']: a per-block list of layer types.
    The reference takes ONE global string (model.py:67-80); the list form is the build-only extension of SURVEY.md section
    8(d) cfg5 / BASELINE.json configs[4] ("SineKAN + FourierKAN mixed blocks"): block l uses types[l % len(types)] for its
    per-head q|k|v mappings, the patch embedding uses types[0].  Parameter names and shapes per block are exactly those of the
    single-type model of that block's type, so a mixed model's state_dict is a block-wise splice of reference state_dicts."""
    kinds = [k.strip() for k in kind.replace("+", ",").split(",") if k.strip()]
    if not kinds:
        raise ValueError(f"Unknown transformer type: {kind}")
    if len(kinds) > 1 and any(k in ("flash-attn",) for k in kinds):
        raise ValueError("'flash-attn' stacks bare FlashAttention modules (model.py:113-117) and cannot be mixed per block")
    return kinds


def patch_embedding_type(model) -> str:
    """The layer type of a model's patch embedding (the first entry of its type list)."""
    lm = model.linear_mapper
    return {KANLinear: "efficientkan", ChebyKANLayer: "cheby", FastKANLayer: "fast", SineKANLayer: "sine",
            NaiveFourierKANLayer: "fourier"}.get(type(lm), "vanilla")


class VisionTransformer(nn.Module):
    def __init__(self, chw, n_patches=7, n_blocks=4, d_hidden=64, n_heads=2, out_d=10, type: str = "vanilla"):
        super().__init__()
        kinds = split_types(type)
        self.block_types = [kinds[l % len(kinds)] for l in range(n_blocks)]
        type = kinds[0]                      # the patch embedding (and the flash-attn switch) follow the first entry
        self.chw = chw
        self.n_patches = n_patches
        self.n_blocks = n_blocks
        self.n_heads = n_heads
        self.d_hidden = d_hidden
        assert chw[1] % n_patches == 0
        assert chw[2] % n_patches == 0
        self.patch_size = (chw[1] // n_patches, chw[2] // n_patches)
        self.input_d = int(chw[0] * self.patch_size[0] * self.patch_size[1])

        self.linear_mapper = _patch_embedding(type, self.input_d, d_hidden)
        self.v_class = nn.Parameter(torch.randn(1, d_hidden))
        self.register_buffer('pos_embeddings', self.positional_embeddings(n_patches ** 2 + 1, d_hidden),
                             persistent=False)
        if type == "flash-attn":
            self.blocks = nn.ModuleList([FlashAttention(dim=d_hidden, heads=n_heads) for _ in range(n_blocks)])
        else:
            self.blocks = nn.ModuleList([TransformerBlock(d_hidden, n_heads, feedforward_dim=4 * d_hidden,
                                                          attn_type=self.block_types[l]) for l in range(n_blocks)])
        self.mlp_head = nn.Sequential(nn.LayerNorm(d_hidden), nn.Linear(d_hidden, out_d))
        self._fused_embed = None       # None = not tried yet, else {bf16 autocast?: the fused patch-embedding kernel covers this model}
        self._drop_path = None         # set_drop_path: None = off, else (keep probabilities of the 2 * n_blocks branches, seed)
        self.drop_path_rates = []
        self._patch_dropout = None     # set_patch_dropout: None = off, else (K kept patches per sample, seed)

    def _set_counter(self, name, on):
        """The device call counter `name` of a hashed draw (set_drop_path, set_patch_dropout): a non-persistent int64 buffer, so
        state_dict() is unchanged.  on: create it, or zero the one there is; off: remove it."""
        if not on:
            if name in self._buffers:
                del self._buffers[name]
                self._non_persistent_buffers_set.discard(name)
        elif name not in self._buffers:
            self.register_buffer(name, torch.zeros(1, dtype=torch.int64, device=self.v_class.device), persistent=False)
        else:
            self._buffers[name].zero_()

    def set_patch_dropout(self, rate, seed=0):
        """PatchDropout (Liu et al. 2023; timm's patch_drop_rate): in train() mode on the GPU every sample keeps K = max(1, int(P *
        (1 - rate))) of its P patch tokens (timm's rule) plus the class token, so every block runs on K + 1 tokens; eval() sees all
        of them.  Set after construction, like set_drop_path; rate 0 (or a rate that keeps all P) removes it again.  The keep set
        comes from one kanvit.ops.patch_keep launch per forward -- a hash of (seed, a device call counter, sample, patch), no RNG
        state, so a captured step draws a new set at every replay; only the kept patches are gathered from the images and embedded
        (_embed_kept).  The counter is a non-persistent buffer: state_dict() is unchanged.  update_grid, extend_grid and the attention
        maps always use the full sequence.  Returns K."""
        rate = float(rate)
        if not 0.0 <= rate < 1.0:
            raise ValueError(f"set_patch_dropout: rate {rate} must be in [0, 1)")
        P = self.n_patches ** 2
        K = max(1, int(P * (1.0 - rate)))
        if rate == 0.0 or K == P:
            self._patch_dropout = None
            self._set_counter("patch_dropout_counter", False)
            return P
        if P > _lib.PATCH_KEEP_MAX_P:
            raise NotImplementedError(f"set_patch_dropout: {P} patches per image; one patch_keep launch ranks {_lib.PATCH_KEEP_MAX_P}")
        self._patch_dropout = (K, int(seed))
        self._set_counter("patch_dropout_counter", True)
        return K

    def set_drop_path(self, rate, seed=0, schedule="linear"):
        """Stochastic depth (DropPath, Huang et al. 2016, as the DeiT recipe uses it): in train() mode every residual branch of
        block l is dropped per sample with probability rates[l] and scaled by 1 / (1 - rates[l]) otherwise; rates[l] = rate * l /
        (L - 1) for schedule 'linear' (rate itself with L = 1), rate everywhere for 'constant'.  Set after construction, like a
        base activation (the constructor stays the reference's, whose model has no such option); rate 0 removes it again, and
        eval() ignores it.  The keep decisions come from one kanvit.ops.depth_scales launch per forward -- a hash of (seed, a
        device call counter, branch, position in the batch), no RNG state -- and ride as per-sample scales in the fused residual
        add + LayerNorm passes.  The counter is a non-persistent buffer: state_dict() is unchanged.  Returns the per-block rates."""
        if schedule not in ("linear", "constant"):
            raise ValueError(f"set_drop_path: schedule must be 'linear' or 'constant', got {schedule!r}")
        rate = float(rate)
        if not 0.0 <= rate < 1.0:
            raise ValueError(f"set_drop_path: rate {rate} must be in [0, 1)")
        if rate == 0.0:
            self._drop_path = None
            self.drop_path_rates = []
            self._set_counter("drop_path_counter", False)
            return self.drop_path_rates
        if not all(isinstance(blk, TransformerBlock) for blk in self.blocks):
            raise NotImplementedError("set_drop_path: 'flash-attn' models stack bare FlashAttention modules (model.py:113-117), which "
                                      "have no residual branches to drop")
        n = len(self.blocks)
        if 2 * n > _lib.DEPTH_MAX_BRANCHES:
            raise NotImplementedError(f"set_drop_path: {n} blocks have {2 * n} branches; one depth_scales launch takes {_lib.DEPTH_MAX_BRANCHES}")
        self.drop_path_rates = [rate if schedule == "constant" or n == 1 else rate * l / (n - 1) for l in range(n)]
        self._drop_path = ([1.0 - r for r in self.drop_path_rates for _ in range(2)], int(seed))      # branch 2l: attention, 2l + 1: feed-forward
        self._set_counter("drop_path_counter", True)
        return self.drop_path_rates

    def patchify(self, images, n_patches):
        """(B, C, H, W) -> (B, n_patches^2, C*ph*pw): patches row-major, each flattened in (C, ph, pw)
        order -- one strided view + copy instead of the reference's n_patches^2 slice copies
        (model.py:111-126)."""
        b, c, h, w = images.shape
        ph, pw = h // n_patches, w // n_patches
        t = images.reshape(b, c, n_patches, ph, n_patches, pw).permute(0, 2, 4, 1, 3, 5)
        return t.reshape(b, n_patches * n_patches, c * ph * pw)

    def positional_embeddings(self, seq_length, d):
        """pe[i, j] = sin(i / 10000^(j/d)) for even j, cos(...) for odd j, evaluated in float64 and
        stored as float32 (the values of model.py:128-140, without its O(N*d) python loop)."""
        i = torch.arange(seq_length, dtype=torch.float64).unsqueeze(1)
        j = torch.arange(d, dtype=torch.float64).unsqueeze(0)
        ang = i / torch.pow(torch.tensor(10000.0, dtype=torch.float64), j / d)
        even = (torch.arange(d) % 2 == 0).unsqueeze(0)
        return torch.where(even, torch.sin(ang), torch.cos(ang)).to(torch.float32)

    def _embed_fused(self, images):
        """patchify + patch-embedding KAN layer + class token + position embedding in ONE kernel launch (SURVEY.md section
        8(f)2; kanvit.ops.patch_embed), or None when the fused kernel does not cover this layer / geometry (then the
        three-step path below runs: same arithmetic).  Under bf16 autocast the same launch runs on the bf16 matrix cores."""
        lm = self.linear_mapper
        if isinstance(lm, nn.Linear) or lm.kan_ln() is not None:      # the kernel forms no LayerNorm: a layer whose basis reads u is not covered
            return None
        # the cached per-model decision is per arithmetic mode: the fp32 and the bf16 kernels tile the patch width differently
        mode = bool(torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16)
        if self._fused_embed is None:
            self._fused_embed = {}
        if self._fused_embed.get(mode) is False:
            return None
        # per-call conditions (they depend on the INPUT, so they never touch the cached per-model decision): the kernel wants
        # contiguous-able fp32 NCHW on the GPU at a 16-byte aligned address, and it produces no gradient for the images --
        # a caller that differentiates w.r.t. the input (saliency, adversarial examples) takes the three-step path below
        if (not images.is_cuda or images.dim() != 4 or images.dtype != torch.float32 or images.requires_grad
                or (images.is_contiguous() and images.data_ptr() % 16)):
            return None
        cfg = lm.kan_cfg()
        w, bp, bias = lm.kan_pack()
        try:
            out = ops.patch_embed(images, w.unsqueeze(0), cfg, None if bp is None else bp.unsqueeze(0),
                                  None if bias is None else bias.reshape(1, -1), self.v_class.reshape(-1),
                                  self.pos_embeddings[: self.n_patches ** 2 + 1], self.n_patches)
        except ops.KanvitError:
            if mode not in self._fused_embed:              # layer / geometry not covered: decided once, at the first forward of a mode
                self._fused_embed[mode] = False
                return None
            raise
        self._fused_embed[mode] = True
        return out

    def _embed(self, images, patches=None):
        """The token sequence the first block reads: patch embedding, class token, position embedding (model.py:144-152)."""
        out = self._embed_fused(images)
        if out is None:
            if patches is None:
                patches = self.patchify(images, self.n_patches)
            b, p, _ = patches.shape
            if isinstance(self.linear_mapper, nn.Linear):
                tokens = self.linear_mapper(patches)
            else:
                # ChebyKANLayer returns (B*P, d) like the reference's; restore (B, P, d)
                tokens = self.linear_mapper(patches).reshape(b, p, self.d_hidden)
            cls = self.v_class.unsqueeze(0).expand(b, -1, -1)
            out = torch.cat((cls, tokens), dim=1) + self.pos_embeddings[: p + 1]
        return out

    def _keeps_patches(self, images):
        """PatchDropout applies: set, train() mode, a batch on the GPU (a CPU model, eval() and rate 0 run what they always ran)."""
        return self._patch_dropout is not None and self.training and images.is_cuda

    def _embed_kept_torch(self, images, idx):
        """_embed_kept in stock torch ops, for images that want a gradient (and what the tests compare _embed_kept with): the full
        patch matrix, the rows idx ([B, K], any integer dtype) names, the embedding, cat and the position rows of the original
        patch numbers.  Returns (tokens [B, K + 1, d], the kept patch rows [B * K, I])."""
        b, k = idx.shape
        take = idx.to(device=images.device, dtype=torch.int64)
        patches = self.patchify(images, self.n_patches)
        rows = torch.gather(patches, 1, take.unsqueeze(-1).expand(b, k, patches.shape[-1])).reshape(b * k, self.input_d)
        tokens = self.linear_mapper(rows).float().reshape(b, k, self.d_hidden)
        cls = self.v_class.unsqueeze(0).expand(b, -1, -1)
        pos = self.pos_embeddings[: self.n_patches ** 2 + 1]
        return torch.cat((cls + pos[:1], tokens + pos[1 + take]), dim=1), rows

    def _embed_kept(self, images, idx=None):
        """The token sequence of a PatchDropout forward, [B, K + 1, d]: the keep table (ops.patch_keep bumps the device counter), the
        kept patches gathered out of the NCHW batch, the patch-embedding module on those B * K rows, whatever its type, and the
        sequence with the class token and the position embedding of the original positions (ops.assemble_tokens).  Also returns the
        gathered rows -- the rows the layer saw, which is what the regulariser is taken on.  idx (int32 [B, K], a keep table the caller
        drew: MaskedAutoencoder's) replaces the draw; set_patch_dropout need not be set then."""
        if idx is None:
            K, seed = self._patch_dropout
            idx = ops.patch_keep(images.shape[0], self.n_patches ** 2, K, seed, self.patch_dropout_counter)
        if images.requires_grad or images.dtype != torch.float32:
            return self._embed_kept_torch(images, idx)
        rows = ops.patch_gather(images.contiguous(), idx, self.n_patches)
        tokens = self.linear_mapper(rows)
        if tokens.dtype != torch.float32:               # nn.Linear under autocast: torch's cat with the fp32 class token promotes it too
            tokens = tokens.float()
        return ops.assemble_tokens(tokens, self.v_class, self.pos_embeddings[: self.n_patches ** 2 + 1], idx), rows

    def _walk(self, images):
        """(block, the block's real input) for every block, on the full sequence: embed, hand a block and its input to the consumer,
        run the block after the consumer returns -- so a consumer that changes the block is seen by its run, and later blocks read
        the activations of the already-changed earlier ones.  The last block is not run: nothing reads its output."""
        out = self._embed(images)
        for blk in self.blocks:
            yield blk, out
            if blk is not self.blocks[-1]:
                out = blk(out)

    def _refit_grids(self, who, images, refit):
        """The body of update_grid and extend_grid (`who`): refit(module, rows) -- the method of that name of a KANLinear or an MSA --
        on the patch embedding with the patch rows, then on every efficient-KAN block's MSA with norm1 of the block's input.  Returns
        the sum of what refit returns."""
        def has_grid(blk):
            return isinstance(blk, TransformerBlock) and isinstance(blk.attn.q_mappings[0], KANLinear)
        if not isinstance(self.linear_mapper, KANLinear) and not any(has_grid(blk) for blk in self.blocks):
            raise NotImplementedError(f"{who}: model type(s) {sorted(self.layer_types())} have no KANLinear, the only layer "
                                      f"with a B-spline grid to {who.split('_')[0]} ('efficientkan')")
        count = torch.zeros((), dtype=torch.int64, device=images.device)
        if isinstance(self.linear_mapper, KANLinear):
            count = count + refit(self.linear_mapper, self.patchify(images, self.n_patches).reshape(-1, self.input_d))
        # whether the fused patch embedding covers this model was decided for the old grid's flags and size
        self._fused_embed = None
        for blk, x in self._walk(images):
            if has_grid(blk):
                count = count + refit(blk.attn, blk.norm1(x))
        self._fused_embed = None
        return count

    @torch.no_grad()
    def update_grid(self, images, margin=0.01):
        """KANLinear.update_grid (models/effkan.py:189-242) for every efficient-KAN layer of the model on one image batch: the
        patch embedding on the patch rows, then block by block the per-head q|k|v layers on norm1 of the block's input
        (MSA.update_grid, one grouped launch per block).  A block runs after its own update, so later blocks adapt to the
        activations of the already-updated earlier ones.  Blocks of other types in a mixed model just run.  Afterwards the
        updated layers evaluate the general Cox-de Boor kernels instead of the uniform closed form.  Returns the number of
        features kept unchanged (0-d device tensor)."""
        return self._refit_grids("update_grid", images, lambda m, rows: m.update_grid(rows, margin))

    @torch.no_grad()
    def extend_grid(self, images, grid_size, margin=0.01):
        """KANLinear.extend_grid for every efficient-KAN layer of the model on one image batch (grid extension: train on a coarse
        grid, then move every layer to `grid_size` intervals with its function kept).  The walk is update_grid's: the patch
        embedding on the patch rows, then block by block the per-head q|k|v layers on norm1 of the block's input
        (MSA.extend_grid); a block runs after its own extension; blocks of other types in a mixed model just run.  Every
        spline_weight of an extended layer is a NEW Parameter: an optimizer holding the old ones must be told (train.py
        --grid-extend does).  Returns the number of features that took the fallback fit (0-d device tensor)."""
        for m in self.modules():                             # refuse a size a layer cannot take before any of them moves
            if isinstance(m, KANLinear):
                KANLinear.check_extension(grid_size, m.spline_order)
        return self._refit_grids("extend_grid", images, lambda m, rows: m.extend_grid(rows, grid_size, margin))

    def _prunable(self, who):
        """The modules edge pruning covers, in the walk's order (the patch embedding, then every block's MSA), or NotImplementedError
        naming the model types that have no edge statistic to prune by."""
        kinds = self.layer_types()
        if not kinds <= set(self.REGULARIZED_TYPES):
            raise NotImplementedError(f"{who}: model type(s) {sorted(kinds - set(self.REGULARIZED_TYPES))} have no edge-activation "
                                      f"statistic to prune by; supported: {', '.join(self.REGULARIZED_TYPES)}")
        return [self.linear_mapper] + [blk.attn for blk in self.blocks]

    @torch.no_grad()
    def prune_edges(self, images, fraction=None, threshold=None, relative=True):
        """prune_edges (kanvit/prune.py) for every KAN layer of the model on one image batch; `fraction` / `threshold` apply to
        every layer on its own.  The walk is update_grid's: the patch embedding on the patch rows, then block by block the
        per-head q|k|v layers on norm1 of the block's input (MSA.prune_edges: one scoring and one selection launch per block); a
        block runs after its own pruning, so later blocks are scored on the activations the pruned earlier ones produce.  The
        walk runs the plain blocks on the full sequence, whatever the mode: drop path (set_drop_path) drops no branch and
        PatchDropout (set_patch_dropout) no patch, and neither counter moves.  Model types efficientkan, cheby and fast.
        Returns [(kept, total)], 0-d device tensors, per pruned layer group: the patch embedding, then every block's 3*H layers."""
        self._prunable("prune_edges")
        kw = dict(fraction=fraction, threshold=threshold, relative=relative)

        def pair(kept, total):
            return kept, torch.full((), total, dtype=torch.int64, device=images.device)
        out = [pair(self.linear_mapper.prune_edges(self.patchify(images, self.n_patches).reshape(-1, self.input_d), **kw),
                    self.input_d * self.d_hidden)]
        for blk, x in self._walk(images):
            out.append(pair(blk.attn.prune_edges(blk.norm1(x), **kw), 3 * blk.attn.n_heads * blk.attn.d_head ** 2))
        return out

    def edge_masked(self):
        """The (parameter, mask, run) triples of every prunable layer (kanvit/prune.py); creates the all-ones masks on first use."""
        return [t for m in self._prunable("edge_masked") for t in m.edge_masked()]

    @torch.no_grad()
    def restore_edge_masks(self):
        """restore_edge_mask on every prunable layer: the masks of a pruned checkpoint, rebuilt from its exact zeros after
        load_state_dict.  Returns the number of kept edges (0-d device tensor)."""
        self._prunable("restore_edge_masks")
        return torch.stack([m.restore_edge_mask() for m in self.modules() if isinstance(m, EdgePruning)]).sum()

    def edge_sparsity(self):
        """(kept, total) edges over every prunable layer, 0-d device tensors; a layer never pruned counts as whole.  No host
        synchronisation."""
        masks = {id(m): m for _, m, _ in self.edge_masked()}.values()
        kept = torch.stack([m.sum() for m in masks]).sum()
        return kept, torch.full((), sum(m.numel() for m in masks), dtype=torch.int64, device=kept.device)

    @torch.no_grad()
    def attention_maps(self, images, rows=None):
        """[n_blocks, B, H, R, N] float32 (N = n_patches^2 + 1 tokens, the class token first): every head's attention
        probabilities in every block on one image batch -- TransformerBlock.attention_map (FlashAttention.attention_map for a
        'flash-attn' model) on each block's real input.  `rows` = R keeps the first R query rows (default N; 1 = the class-token
        row).  Runs without gradients and leaves the training / eval mode as it finds it.  The stacked result grows with
        n_blocks * B * H * N^2 (ViT-B at batch 128: 2.9 GB); attention_rollout holds one block's map at a time."""
        return torch.stack([blk.attention_map(x, rows=rows) for blk, x in self._walk(images)])

    @staticmethod
    def _rollout_factor(block_map, head_fusion):
        """(fuse_h A + I) / rowsum of one block's [B, H, N, N] map, float32 with autocast off."""
        if block_map.dim() != 4 or block_map.shape[-1] != block_map.shape[-2]:
            raise ValueError(f"rollout needs full attention maps [.., B, H, N, N] (rows=None), got a block of shape {tuple(block_map.shape)}")
        a = block_map.float()
        if head_fusion == "mean":
            a = a.mean(dim=1)
        elif head_fusion == "max":
            a = a.amax(dim=1)
        elif head_fusion == "min":
            a = a.amin(dim=1)
        else:
            raise ValueError(f"head_fusion must be 'mean', 'max' or 'min', got {head_fusion!r}")
        a = a + torch.eye(a.shape[-1], dtype=a.dtype, device=a.device)
        return a / a.sum(dim=-1, keepdim=True)

    @staticmethod
    def rollout(maps, head_fusion="mean"):
        """Attention rollout (Abnar & Zuidema 2020) of maps [n_blocks, B, H, N, N] -> [B, N, N]: with A_l = fuse_h maps[l]
        (head_fusion: 'mean', 'max' or 'min' over the heads) and A~_l = (A_l + I) / rowsum(A_l + I), the product
        A~_L ... A~_1.  Pure torch, any device; float32 products with autocast off.  Needs full maps (R == N)."""
        if maps.dim() != 5:
            raise ValueError(f"rollout needs maps [n_blocks, B, H, N, N], got shape {tuple(maps.shape)}")
        with torch.autocast(maps.device.type, enabled=False):
            out = None
            for block_map in maps:
                f = VisionTransformer._rollout_factor(block_map, head_fusion)
                out = f if out is None else f @ out
        return out

    @torch.no_grad()
    def attention_rollout(self, images, head_fusion="mean"):
        """rollout(attention_maps(images), head_fusion) -> [B, N, N] without the stacked maps: the same walk, carrying the running
        product and one block's map.  [:, 0, 1:] is the class token's saliency over the patches (cls_saliency)."""
        out = None
        for blk, x in self._walk(images):
            block_map = blk.attention_map(x)
            with torch.autocast(block_map.device.type, enabled=False):
                f = self._rollout_factor(block_map, head_fusion)
                out = f if out is None else f @ out
        return out

    def cls_saliency(self, rollout):
        """[B, N, N] rollout -> [B, n_patches, n_patches]: the class token's row over the patch grid."""
        return rollout[:, 0, 1:].reshape(-1, self.n_patches, self.n_patches)

    REGULARIZED_TYPES = MSA.REGULARIZED_TYPES

    def layer_types(self):
        """The KAN layer types of the model: its blocks' and its patch embedding's."""
        return set(self.block_types) | {patch_embedding_type(self)}

    def forward(self, images, return_regularization=False, regularize_activation=1.0, regularize_entropy=1.0):
        """logits; with return_regularization=True, (logits, reg): reg is the KAN paper's sample-based L1 + entropy regulariser
        (KANLinear.regularization_loss(x=...), MSA.regularization_loss) summed over the patch embedding, on the patch rows, and
        every block's per-head q|k|v layers, on norm1(x) -- computed on the tensors this forward holds anyway, by the fused
        edge-activation kernel (no second forward, no (rows, in, out) tensor).  Model types efficientkan, cheby and fast."""
        reg, reg_kw, patches = None, None, None
        # PatchDropout (set_patch_dropout), train() mode on the GPU only: the sequence is built from the kept patches
        out = None
        if self._keeps_patches(images):
            out, rows = self._embed_kept(images)
        if return_regularization:
            kinds = self.layer_types()
            if not kinds <= set(self.REGULARIZED_TYPES):
                raise NotImplementedError(f"return_regularization: model type(s) {sorted(kinds - set(self.REGULARIZED_TYPES))} have no "
                                          f"edge-activation regulariser; supported: {', '.join(self.REGULARIZED_TYPES)}")
            reg_kw = dict(regularize_activation=regularize_activation, regularize_entropy=regularize_entropy)
            # the fused patch embedding gathers from NCHW and never holds the patch matrix: build it once for the regulariser
            # (under PatchDropout the regulariser is taken on the kept rows, the rows the layer saw)
            if out is None:
                patches = self.patchify(images, self.n_patches)
                rows = patches.reshape(-1, self.input_d)
            reg = self.linear_mapper.regularization_loss(x=rows, **reg_kw)
        if out is None:
            out = self._embed(images, patches)
        pending = None
        # the head reads the class token only: the last block computes that row alone (TransformerBlock.run_cls), except for the
        # small geometries (launch-bound: they keep the one-launch LN2 + feed-forward) and when the regulariser is asked for
        last = self.blocks[-1] if len(self.blocks) else None
        cls_tail = (isinstance(last, TransformerBlock) and reg_kw is None and out.is_cuda and not _lib.py_switches()["no_cls_tail"]
                    and not ff_small_supported(last.ff[0].in_features, last.ff[0].out_features))
        # stochastic depth (set_drop_path), train() mode only: one launch draws every branch's per-sample scales, rows 2l (attention)
        # and 2l + 1 (feed-forward) of block l; the add that takes a branch in takes its row
        scales = None
        if self._drop_path is not None and self.training:
            scales = ops.depth_scales(out.shape[0], self._drop_path[0], self._drop_path[1], self.drop_path_counter)
        for l, blk in enumerate(self.blocks):
            drop = _NO_DROP if scales is None else (scales[2 * l - 1] if l else None, scales[2 * l], scales[2 * l + 1])
            if cls_tail and blk is last:
                return self.mlp_head(blk.run_cls(out, pending, drop))
            if isinstance(blk, TransformerBlock) and reg_kw is not None:
                out, pending, r = blk.run(out, pending, reg_kw, drop)
                reg = reg + r
            elif isinstance(blk, TransformerBlock):
                out, pending = blk.run(out, pending, drop=drop)
            else:                                     # 'flash-attn' models stack bare FlashAttention modules (model.py:113-117)
                out = blk(out)
        if pending is not None and scales is not None:    # the class rows of the stream and of the last, still pending branch
            out = _FirstRow.apply(out) + _FirstRow.apply(pending) * scales[-1].unsqueeze(1)
        elif pending is not None:
            out = _ClsToken.apply(out, pending)   # only the class token feeds the head (model.py:166-169)
        else:
            out = out[:, 0]
        if return_regularization:
            return self.mlp_head(out), reg
        return self.mlp_head(out)
