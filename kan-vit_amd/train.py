"""Training entry point -- drop-in for the reference's train.py (same flags and defaults,
train.py:87-97; same step order forward -> CE loss -> zero_grad -> backward -> Adam.step,
train.py:31-40), running on the MI355X kernels, with optional pure data parallelism:

    python train.py --model-type cheby                                 # 1 GPU, CIFAR-100 if torchvision + data exist
    python train.py --model-type cheby --synthetic --epochs 1          # synthetic stream, no dataset needed
    python train.py --model-type cheby --synthetic --graph             # the whole step replayed from one HIP graph
    python train.py --model-type fast --synthetic --amp bf16           # bf16 autocast + kanvit kernels on the bf16 matrix cores
    python train.py --model-type cheby --data-npz cifar100.npz         # real images from a GPU-resident uint8 dataset, no torchvision
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py --dp --synthetic ...

Additions over the reference (none changes a default; each flag's help text has the details, DESIGN.md the design):
    stream, geometry      --synthetic --steps-per-epoch --image-size --in-chans --n-patches --out-d --seed
    step and metrics      --dp --amp --graph --no-tuned-gemms --base-activation --no-step-metrics --device-metrics
    KAN layers            --reg-lambda --reg-activation --reg-entropy --grid-update-every --grid-extend STEP:SIZE[,...] --prune STEP:VALUE[,...] --prune-mode
    GPU-resident dataset  --data-npz --no-augment --crop-padding --resize S --random-resized-crop --rrc-scale --rrc-ratio --mixup --cutmix --mix-prob
                          --mix-switch-prob --random-erasing P --erase-mode --erase-scale --erase-ratio --randaug [M] --randaug-ops --randaug-mstd --randaug-prob
    loss, optimizer       --label-smoothing --fused-loss --optimizer kanvit-adamw --weight-decay --clip-grad-norm --warmup-steps --lr-schedule --min-lr --ema-decay
    regularisation        --drop-path RATE --drop-path-schedule --patch-dropout RATE
    pretraining           --pretrain mae --mask-ratio --decoder-dim --decoder-blocks --decoder-heads --decoder-type --no-norm-pix-loss
                          --save-encoder PATH --init-encoder PATH

`main(args, batches=None, init_state=None)` also serves the parity tests: `batches` (a list of (x, y) tensors) replaces
the data stream, `init_state` (a reference-layout state dict) replaces the random initialisation, and the returned dict
carries the per-step loss trajectory."""
import argparse
import contextlib
import functools
import logging
import os
import time
import types

import torch
from torch.optim import Adam

from kanvit import data as kdata, dp as kdp, ops as kops, prune as kprune, tuned
from kanvit.metrics import EpochMetrics
from kanvit.optim import KanvitAdamW
from mae import MaskedAutoencoder
from model import VisionTransformer, split_types
from utils import calculate_metrics, save_metrics, setup_logging


def synthetic_loader(n_steps, batch, chw, out_d, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    for _ in range(n_steps):
        yield (torch.randn(batch, *chw, device=device, generator=g),
               torch.randint(0, out_d, (batch,), device=device, generator=g))


def cifar_loaders(batch, rank, world):
    """CIFAR-100 with the reference's transforms (train.py:100-118); built ONCE.  Returns (train, test, sampler)."""
    from torchvision import transforms
    from torchvision.datasets import CIFAR100
    norm = transforms.Normalize(mean=[0.5071, 0.4867, 0.4408], std=[0.2675, 0.2565, 0.2761])
    tr = transforms.Compose([transforms.RandomHorizontalFlip(), transforms.RandomCrop(32, padding=4),
                             transforms.ToTensor(), norm])
    te = transforms.Compose([transforms.ToTensor(), norm])
    train = CIFAR100(root='./cifar100', train=True, download=True, transform=tr)
    test = CIFAR100(root='./cifar100', train=False, download=True, transform=te)
    sampler = torch.utils.data.distributed.DistributedSampler(train, world, rank, shuffle=True) if world > 1 else None
    mk = torch.utils.data.DataLoader
    return (mk(train, batch_size=batch, shuffle=sampler is None, sampler=sampler, num_workers=8, pin_memory=True),
            mk(test, batch_size=batch, shuffle=False, num_workers=8, pin_memory=True), sampler)


@functools.lru_cache(maxsize=None)
def defaults():
    """Every flag's default by attribute name, read from build_parser(): the one place where a default is written down."""
    return vars(build_parser().parse_args([]))


def complete(args):
    """Give `args` every attribute it lacks, at the parser's default: in place, so that a namespace built by hand (the tests build
    them) reads like one from parse().  It validates nothing.  main() and every helper that takes `args` call it first."""
    for name, default in defaults().items():
        vars(args).setdefault(name, default)
    return args


def check_args(args):
    """Everything parse() refuses.  main() calls it too, for namespaces that did not come through parse()."""
    complete(args)
    for flag, name in (("--drop-path", "drop_path"), ("--patch-dropout", "patch_dropout")):
        if not 0.0 <= float(getattr(args, name)) < 1.0:
            raise SystemExit(f"{flag} {float(getattr(args, name))} must be in [0, 1)")
    if not 0.0 < float(args.mask_ratio) < 1.0:
        raise SystemExit(f"--mask-ratio {float(args.mask_ratio)} must be in (0, 1)")
    for flag, name, least in (("--decoder-dim", "decoder_dim", 0), ("--decoder-blocks", "decoder_blocks", 1), ("--decoder-heads", "decoder_heads", 0)):
        if int(getattr(args, name)) < least:
            raise SystemExit(f"{flag} {getattr(args, name)} is below {least}")
    check_data_args(args)
    check_optimizer_args(args)
    check_prune_args(args)


def lo_hi(flag, pair):
    """(LO, HI) of a range flag as floats; refused unless 0 < LO <= HI < inf."""
    lo, hi = (float(v) for v in pair)
    if not 0 < lo <= hi or hi == float("inf"):
        raise SystemExit(f"{flag} {lo} {hi}: LO and HI are positive and LO is not above HI")
    return lo, hi


def check_data_args(args):
    """Contradictions among the data-source flags."""
    complete(args)
    if args.data_npz and args.synthetic:
        raise SystemExit("--synthetic and --data-npz name two data sources; give one")
    if args.crop_padding < 0:
        raise SystemExit(f"--crop-padding {args.crop_padding} is negative")
    mixup, cutmix = float(args.mixup), float(args.cutmix)
    if mixup < 0 or cutmix < 0:
        raise SystemExit(f"--mixup {mixup} / --cutmix {cutmix}: a Beta parameter is not negative")
    for flag, name in (("--mix-prob", "mix_prob"), ("--mix-switch-prob", "mix_switch_prob")):
        if not 0.0 <= float(getattr(args, name)) <= 1.0:
            raise SystemExit(f"{flag} {getattr(args, name)} is not a probability")
    if not 0.0 <= float(args.label_smoothing) < 1.0:
        raise SystemExit(f"--label-smoothing {args.label_smoothing} must be in [0, 1)")
    if mixup > 0 or cutmix > 0:
        if not args.data_npz:
            raise SystemExit("--mixup / --cutmix mix inside the kernel that reads the GPU-resident dataset; give --data-npz")
        if args.no_augment:
            raise SystemExit("--mixup / --cutmix are augmentations; they are not combined with --no-augment")
    resize, rrc = int(args.resize), bool(args.random_resized_crop)
    if resize < 0:
        raise SystemExit(f"--resize {resize} is negative (0: off)")
    if (resize > 0 or rrc) and not args.data_npz:
        raise SystemExit("--resize / --random-resized-crop resample inside the kernel that reads the GPU-resident dataset; give --data-npz")
    if rrc and args.no_augment:
        raise SystemExit("--random-resized-crop is an augmentation; it is not combined with --no-augment")
    lo_hi("--rrc-scale", args.rrc_scale)
    lo_hi("--rrc-ratio", args.rrc_ratio)
    p_erase = float(args.random_erasing)
    if not 0.0 <= p_erase <= 1.0:
        raise SystemExit(f"--random-erasing {p_erase} is not a probability")
    lo, hi = lo_hi("--erase-scale", args.erase_scale)
    if hi > 1:
        raise SystemExit(f"--erase-scale {lo} {hi}: HI is a fraction of the image, at most 1")
    lo_hi("--erase-ratio", args.erase_ratio)
    if p_erase > 0:
        if not args.data_npz:
            raise SystemExit("--random-erasing erases inside the kernel that reads the GPU-resident dataset; give --data-npz")
        if args.no_augment:
            raise SystemExit("--random-erasing is an augmentation; it is not combined with --no-augment")
    if args.randaug is not None and not 0.0 <= float(args.randaug) <= 10.0:
        raise SystemExit(f"--randaug {args.randaug}: the magnitude is in 0..10")
    if not 1 <= int(args.randaug_ops) <= 4:
        raise SystemExit(f"--randaug-ops {args.randaug_ops} must be in 1..4")
    if not 0.0 <= float(args.randaug_mstd) < float("inf"):
        raise SystemExit(f"--randaug-mstd {args.randaug_mstd} is negative or not finite")
    if not 0.0 <= float(args.randaug_prob) <= 1.0:
        raise SystemExit(f"--randaug-prob {args.randaug_prob} is not a probability")
    if args.randaug is not None:
        if not args.data_npz:
            raise SystemExit("--randaug augments a second copy of the GPU-resident dataset once per epoch; give --data-npz")
        if args.no_augment:
            raise SystemExit("--randaug is an augmentation; it is not combined with --no-augment")


RECIPE_FLAGS = (("--weight-decay", "weight_decay"), ("--clip-grad-norm", "clip_grad_norm"), ("--warmup-steps", "warmup_steps"),
                ("--lr-schedule", "lr_schedule"), ("--min-lr", "min_lr"), ("--ema-decay", "ema_decay"))


def check_optimizer_args(args):
    """Contradictions among the optimizer flags.  The recipe flags belong to --optimizer kanvit-adamw: given without it (away from
    their defaults) they are refused, not ignored."""
    complete(args)
    fused = args.optimizer == "kanvit-adamw"
    given = [flag for flag, name in RECIPE_FLAGS if getattr(args, name) != defaults()[name]]
    if given and not fused:
        raise SystemExit(f"{' / '.join(given)}: the recipe flags are implemented by --optimizer kanvit-adamw; the default Adam has none of them")
    if not fused:
        return
    if args.grid_extend:
        raise SystemExit("--grid-extend is not combined with --optimizer kanvit-adamw: its flat moment buffers cannot take the "
                         "parameters of a new shape that an extension creates")
    for flag, name in RECIPE_FLAGS:
        if name != "lr_schedule" and float(getattr(args, name)) < 0:
            raise SystemExit(f"{flag} {getattr(args, name)} is negative")
    if not float(args.ema_decay) < 1.0:
        raise SystemExit(f"--ema-decay {args.ema_decay} must be in [0, 1)")


def mix_config(args):
    """The `mix` argument of GpuDataset.batches from the flags, or None when neither --mixup nor --cutmix is given."""
    complete(args)
    mixup, cutmix = float(args.mixup), float(args.cutmix)
    if mixup <= 0 and cutmix <= 0:
        return None
    return dict(mixup_alpha=mixup, cutmix_alpha=cutmix, prob=float(args.mix_prob), switch_prob=float(args.mix_switch_prob))


def erase_config(args):
    """The `erase` argument of GpuDataset from the flags, or None when --random-erasing is 0."""
    complete(args)
    p_erase = float(args.random_erasing)
    if p_erase <= 0:
        return None
    return dict(prob=p_erase, scale=tuple(args.erase_scale), ratio=tuple(args.erase_ratio), mode=args.erase_mode)


def randaug_config(args, mean=None):
    """The `randaug` argument of GpuDataset from the flags, or None without --randaug.  mean: the dataset's per-channel mean on the 0-1
    scale; the geometric ops fill with round(255 mean) per channel."""
    complete(args)
    if args.randaug is None:
        return None
    cfg = dict(n_ops=int(args.randaug_ops), magnitude=float(args.randaug), mstd=float(args.randaug_mstd), prob=float(args.randaug_prob))
    if mean is not None:
        cfg["fill"] = tuple(min(max(int(round(255.0 * float(m))), 0), 255) for m in mean)
    return cfg


def npz_datasets(args, device, want_test=True):
    """--data-npz: (train, test or None) GpuDatasets.  --image-size / --in-chans left at their defaults follow the file (args is
    updated); given values that contradict it, labels that --out-d does not cover and non-square images are refused.  Only the rank
    that evaluates asks for the test split.  --resize S gives both splits out_size = (S, S) (--image-size stays the file's size) and
    --random-resized-crop gives the train split crop="rrc": their batches then come from ops.resample_u8.  --random-erasing gives the
    train split -- never the test split -- erase=...: its batches come from ops.erase_u8.  --randaug gives the train split -- never the
    test split -- randaug=...: a second buffer that ops.randaugment_u8 fills once per epoch and the batch kernels read."""
    complete(args)
    blob = kdata.load_npz(args.data_npz)
    x = blob["x_train"]
    c, h, w = (x.shape[3] if x.ndim == 4 else 1), x.shape[1], x.shape[2]
    if h != w:
        raise SystemExit(f"--data-npz {args.data_npz}: images are {h}x{w}; the model takes square images (--image-size)")
    for flag, name, have in (("--image-size", "image_size", h), ("--in-chans", "in_chans", c)):
        if getattr(args, name) == defaults()[name]:
            setattr(args, name, int(have))
        elif getattr(args, name) != have:
            raise SystemExit(f"{flag} {getattr(args, name)} contradicts --data-npz {args.data_npz}, whose images have {have}")
    top = max(int(blob[k].max()) for k in ("y_train", "y_test") if k in blob)
    if args.out_d <= top:
        raise SystemExit(f"--out-d {args.out_d} does not cover the labels of --data-npz {args.data_npz} (largest: {top})")
    augment = not args.no_augment
    if augment and args.crop_padding > h:
        raise SystemExit(f"--crop-padding {args.crop_padding} exceeds the image size {h}")
    resize = int(args.resize)
    out_size = (resize, resize) if resize > 0 else None          # --resize: both splits come out at the model's size
    mean = None
    if args.randaug is not None:                                 # the fill of its geometric ops: the dataset mean, as the datasets use it
        mean = blob["mean"] if "mean" in blob else kdata.channel_stats(x)[0]
    train = kdata.GpuDataset.from_arrays(blob, args.data_npz, "train", device, pad=args.crop_padding if augment else 0, flip=augment,
                                         out_size=out_size, crop="rrc" if args.random_resized_crop else "pad",
                                         rrc_scale=tuple(args.rrc_scale), rrc_ratio=tuple(args.rrc_ratio), erase=erase_config(args),
                                         randaug=randaug_config(args, mean))
    test = kdata.GpuDataset.from_arrays(blob, args.data_npz, "test", device, out_size=out_size) if want_test and "x_test" in blob else None
    return train, test


def hash_counters(model):
    """The device call counters of the model's hashed draws (drop_path_counter, patch_dropout_counter, a MaskedAutoencoder's
    mask_counter), wherever in the module tree they live."""
    return [b for name, b in model.named_buffers() if name.rsplit(".", 1)[-1].endswith("_counter")]


class _GraphedStep:
    """The whole train step (forward, loss, zero_grad, backward, Adam) captured once in a HIP graph and replayed per batch:
    the launch-bound geometries (train.py's own defaults: 64-wide model, 17 tokens) spend their time in ~1000 launches of
    microsecond kernels.  Batches are copied into static buffers; a batch of another shape (the last, short one) runs eagerly.

    Capturing needs lazily created state (optimizer moments, library workspaces) to exist, so one throw-away step runs on a
    side stream first; parameters are then restored, the Adam moments / step counters zeroed, which is exactly the state
    of a fresh optimizer, and the model's drop-path, patch-dropout and mask counters (--drop-path, --patch-dropout, --pretrain mae)
    put back -- the replayed trajectory equals the eager one."""

    def __init__(self, eager_step, model, optimizer, x, y, y2=None, w=None):
        self.eager = eager_step
        self.sx, self.sy = x.clone(), y.clone()
        self.pair = () if y2 is None else (y2.clone(), w.clone())      # Mixup / CutMix: static buffers like x and y
        saved = [p.detach().clone() for p in model.parameters()]
        # --drop-path / --patch-dropout / --pretrain mae: the throw-away step must not use up a mask or a keep set
        counters = hash_counters(model)
        counts = [c.clone() for c in counters]
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(side):
            eager_step(self.sx, self.sy, *self.pair)
        torch.cuda.current_stream(x.device).wait_stream(side)
        with torch.no_grad():
            for p, s in zip(model.parameters(), saved):
                if p.requires_grad:             # only what the throw-away step can have changed: rewriting FastKAN's frozen
                    p.copy_(s)                  # rbf.grid would bump its version and re-derive grid facts (host syncs) in capture
            for st in optimizer.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
            for c, count in zip(counters, counts):
                c.copy_(count)
        optimizer.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss, self.logits = eager_step(self.sx, self.sy, *self.pair)

    def __call__(self, x, y, y2=None, w=None):
        if x.shape != self.sx.shape:
            return self.eager(x, y, y2, w)
        self.sx.copy_(x, non_blocking=True)
        self.sy.copy_(y, non_blocking=True)
        if self.pair:
            self.pair[0].copy_(y2, non_blocking=True)
            self.pair[1].copy_(w, non_blocking=True)
        self.graph.replay()
        return self.loss, self.logits


def set_base_activation(model, model_type, name):
    """--base-activation: the base activation of every KANLinear ('efficientkan') or FastKANLayer ('fast') of the model, set
    after construction as the reference's layers allow (they read `base_activation` on every forward).  The constructors of
    VisionTransformer / MSA take no such argument, so their signatures stay the reference's."""
    import torch.nn.functional as F
    from models.effkan import KANLinear
    from models.fastkan import FastKANLayer
    if name == "silu":
        return
    modules = {"gelu": lambda: torch.nn.GELU(), "gelu-tanh": lambda: torch.nn.GELU(approximate="tanh"),
               "relu": lambda: torch.nn.ReLU(), "tanh": lambda: torch.nn.Tanh(), "identity": lambda: torch.nn.Identity()}
    functions = {"gelu": F.gelu, "gelu-tanh": functools.partial(F.gelu, approximate="tanh"), "relu": F.relu,
                 "tanh": torch.tanh, "identity": torch.nn.Identity()}
    if model_type not in ("efficientkan", "fast"):
        raise SystemExit(f"--base-activation {name}: only the 'efficientkan' and 'fast' model types have a base activation")
    for m in model.modules():
        if isinstance(m, KANLinear):
            m.base_activation = modules[name]()
        elif isinstance(m, FastKANLayer) and m.use_base_update:
            m.base_activation = functions[name]


def parse_grid_extend(text):
    """'3:10,6:20' -> {3: 10, 6: 20}: at the start of step 3 extend to grid size 10, at step 6 to 20."""
    plan = {}
    for item in filter(None, (t.strip() for t in (text or "").split(","))):
        try:
            step, size = (int(v) for v in item.split(":"))
        except ValueError:
            raise SystemExit(f"--grid-extend: '{item}' is not STEP:SIZE")
        if step < 1 or size < 1 or step in plan:
            raise SystemExit(f"--grid-extend: '{item}': STEP and SIZE are positive and a step is named once")
        plan[step] = size
    return plan


def extend_grid_and_swap(model, optimizer, x, grid_size):
    """model.extend_grid(x, grid_size), then hand the optimizer the Parameters the extension replaced (by name): they take the old
    ones' places in the param groups and start without state; every other parameter keeps its moments and its step count."""
    before = dict(model.named_parameters())
    model.extend_grid(x, grid_size)
    swap = {id(before[n]): (before[n], p) for n, p in model.named_parameters() if before[n] is not p}
    for group in optimizer.param_groups:
        group["params"] = [swap[id(p)][1] if id(p) in swap else p for p in group["params"]]
    for old, _ in swap.values():
        optimizer.state.pop(old, None)
    return len(swap)


PRUNE_MODES = ("fraction", "relative", "absolute")


def parse_prune(text):
    """'3:0.5,6:0.75' -> {3: 0.5, 6: 0.75}: at the start of step 3 prune with VALUE 0.5, at step 6 with 0.75 (--prune-mode says
    what VALUE is)."""
    plan = {}
    for item in filter(None, (t.strip() for t in (text or "").split(","))):
        try:
            step, value = item.split(":")
            step, value = int(step), float(value)
        except ValueError:
            raise SystemExit(f"--prune: '{item}' is not STEP:VALUE")
        if step < 1 or not 0.0 <= value < float("inf") or step in plan:
            raise SystemExit(f"--prune: '{item}': STEP is positive, VALUE is finite and not negative, and a step is named once")
        plan[step] = value
    return plan


def check_prune_args(args):
    """--prune against --prune-mode and --dp."""
    complete(args)
    if args.prune_mode not in PRUNE_MODES:
        raise SystemExit(f"--prune-mode {args.prune_mode} is none of {', '.join(PRUNE_MODES)}")
    if not args.prune:
        return
    if args.prune_mode != "absolute" and any(v > 1.0 for v in args.prune.values()):
        raise SystemExit(f"--prune: with --prune-mode {args.prune_mode} VALUE is a share, at most 1")
    if args.dp:
        raise SystemExit("--prune is not combined with --dp: every rank would score its own shard and the replicas "
                         "would diverge (a gathered scoring is not implemented)")


def prune_and_mask(model, optimizer, x, value, mode="fraction"):
    """model.prune_edges on the batch x (mode 'fraction': value is the share of every layer's edges that ends up pruned; 'relative' /
    'absolute': a threshold on the edge scores), then the masked runs of the optimizer's state become +0 as the parameters' just
    did (ops.mask_rows): KanvitAdamW's views moments(p) and ema(p), stock Adam's state[p]['exp_avg'] / ['exp_avg_sq'] where they
    exist.  With weight, moments and EMA at +0 and the gradient masked before every step, both optimizers leave a pruned entry at
    exactly 0.  Returns model.prune_edges' [(kept, total)]."""
    if mode == "fraction":
        counts = model.prune_edges(x, fraction=value)
    else:
        counts = model.prune_edges(x, threshold=value, relative=mode == "relative")
    if isinstance(optimizer, KanvitAdamW):
        mine = {id(p) for p in optimizer._params}
        has_ema = "ema" in optimizer.flat

        def state_of(p):
            if id(p) not in mine:
                return ()
            return optimizer.moments(p) + ((optimizer.ema(p),) if has_ema else ())
    else:
        def state_of(p):
            st = optimizer.state.get(p, {})
            return tuple(st.get(k) for k in ("exp_avg", "exp_avg_sq"))
    kprune.zero_masked(model.edge_masked(), of=state_of)
    return counts


PRETRAIN_REFUSED = (("--mixup", "mixup", "there are no labels to mix"), ("--cutmix", "cutmix", "there are no labels to mix"),
                    ("--label-smoothing", "label_smoothing", "there are no labels to smooth"),
                    ("--fused-loss", "fused_loss", "the loss is the reconstruction error, not a cross-entropy"),
                    ("--reg-lambda", "reg_lambda", "the kept-token walk takes no regulariser"),
                    ("--prune", "prune", "edge scoring walks the supervised model"),
                    ("--grid-update-every", "grid_update_every", "the grid refit walks the supervised model"),
                    ("--grid-extend", "grid_extend", "the grid refit walks the supervised model"),
                    ("--patch-dropout", "patch_dropout", "the mask is the patch dropout: --mask-ratio sets it"),
                    ("--device-metrics", "device_metrics", "there are no class metrics to count"))


def check_pretrain_args(args, kinds):
    """--pretrain mae against the flags of the supervised step, and --init-encoder against the file system."""
    if args.pretrain is not None:
        for flag, name, why in PRETRAIN_REFUSED:
            if getattr(args, name) != defaults()[name]:
                raise SystemExit(f"{flag} is not combined with --pretrain {args.pretrain}: {why}")
        if "flash-attn" in kinds:
            raise SystemExit(f"--pretrain {args.pretrain}: model type 'flash-attn' stacks bare attention modules, which the kept-token "
                             "walk does not cover")
        try:
            split_types(args.decoder_type)
        except ValueError as e:
            raise SystemExit(f"--decoder-type: {e}")
        if "flash-attn" in split_types(args.decoder_type) or len(split_types(args.decoder_type)) != 1:
            raise SystemExit(f"--decoder-type {args.decoder_type}: one attention type of a TransformerBlock, not 'flash-attn'")
    if args.init_encoder and not os.path.isfile(args.init_encoder):
        raise SystemExit(f"--init-encoder {args.init_encoder}: no such file")


def check_run_args(args):
    """What only a run refuses, not parse(): main() calls it after check_args, before anything touches the GPU or the process group."""
    regularized = VisionTransformer.REGULARIZED_TYPES
    kinds = split_types(args.model_type)
    check_pretrain_args(args, kinds)
    bad = sorted(set(kinds) - set(regularized))
    if args.prune and bad:
        raise SystemExit(f"--prune: model type(s) {', '.join(bad)} have no edge-activation statistic to prune by; "
                         f"supported: {', '.join(regularized)}")
    for flag, on, verb, noun, baked in (
            ("--grid-extend", bool(args.grid_extend), "extend", "extension",
             "the parameters, the grid sizes and the kernel forms the grids' flags selected, and an extension replaces all three"),
            ("--grid-update-every", int(args.grid_update_every) > 0, "update", "update",
             "the kernel forms the grids' flags selected, and a grid update changes them")):
        if not on:
            continue
        if args.graph:
            raise SystemExit(f"{flag} is not combined with --graph: the captured step bakes in {baked}")
        if args.dp:
            raise SystemExit(f"{flag} is not combined with --dp: every rank would fit its own shard and the replicas "
                             f"would diverge (a gathered {noun} is not implemented)")
        if "efficientkan" not in kinds:
            raise SystemExit(f"{flag}: model type '{args.model_type}' has no KANLinear, the only layer with a B-spline "
                             f"grid to {verb} ('efficientkan')")
    if args.dp:
        world = int(os.environ["WORLD_SIZE"])
        if args.batch_size % world:
            raise SystemExit(f"--batch-size {args.batch_size} is not divisible by the {world} ranks (equal shards keep the "
                             "all-reduced mean equal to the global-batch mean)")
        if args.graph:
            raise SystemExit("--graph captures a single-GPU step; it is not combined with --dp")
    elif torch.device(args.device).type != "cuda":
        raise SystemExit("this build runs the hot path on the MI355X only; --device must be a cuda device")
    # the model's layer types (VisionTransformer.layer_types): block l has kinds[l % len(kinds)], the patch embedding kinds[0]
    if float(args.reg_lambda) > 0 and not set(kinds[:max(args.n_blocks, 1)]) <= set(regularized):
        raise SystemExit(f"--reg-lambda: the edge-activation regulariser covers the model types {', '.join(regularized)}")


def setup_distributed(args):
    """(rank, world, device); with --dp the process group comes up here.  The kernels launch on the current device: it becomes `device`."""
    rank, world, local = 0, 1, 0
    if args.dp:
        import torch.distributed as dist
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        local = int(os.environ.get("LOCAL_RANK", rank))
        # rehearsal hooks for a ONE-GPU box (same as bench.py's; never set by a real launch): every rank on cuda:0, gloo transport
        if os.environ.get("KANVIT_SHARE_GPU") == "1":
            local = 0
        torch.cuda.set_device(local)
        backend = os.environ.get("KANVIT_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    device = torch.device(args.device if not args.dp else f"cuda:{local}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.set_device(device)
    return rank, world, device


def build_model(args, chw, rank, world, device, init_state=None):
    """The VisionTransformer of the flags on `device`, the same on every rank.  --drop-path's masks and --patch-dropout's keep sets are
    hashes of (seed, a device step counter, position in the rank's batch, ...), so under --dp each rank has a seed of its own."""
    model = VisionTransformer(chw, n_patches=args.n_patches, n_blocks=args.n_blocks, d_hidden=args.d_hidden,
                              n_heads=args.n_heads, out_d=args.out_d, type=args.model_type)
    set_base_activation(model, args.model_type, args.base_activation)
    for flag, rate, switch_on, more in (("--drop-path", args.drop_path, model.set_drop_path, dict(schedule=args.drop_path_schedule)),
                                        ("--patch-dropout", args.patch_dropout, model.set_patch_dropout, {})):
        try:
            if float(rate) > 0:
                switch_on(float(rate), seed=kdata.rank_seed(args.seed, rank, world), **more)
        except NotImplementedError as e:
            raise SystemExit(f"{flag}: {e}")
    if init_state is not None:
        model.load_state_dict(init_state)
    if args.init_encoder:
        load_encoder(model, args.init_encoder)
    if args.pretrain == "mae":
        try:
            model = MaskedAutoencoder(model, mask_ratio=float(args.mask_ratio), decoder_dim=int(args.decoder_dim) or None,
                                      decoder_blocks=int(args.decoder_blocks), decoder_heads=int(args.decoder_heads) or None,
                                      decoder_type=args.decoder_type, norm_pix_loss=not args.no_norm_pix_loss,
                                      seed=kdata.rank_seed(args.seed, rank, world))
        except (NotImplementedError, ValueError) as e:
            raise SystemExit(f"--pretrain mae: {e}")
        # the reconstruction loss never reaches the classifier head: frozen, the optimizers and the gradient reducer leave it out (a
        # trainable parameter without a gradient would read as zeros in kanvit-adamw's weight EMA and never fill its bucket under --dp)
        for p in model.encoder.mlp_head.parameters():
            p.requires_grad_(False)
    model = model.to(device)
    kdp.broadcast_parameters(model)
    return model


def encoder_of(model):
    """The VisionTransformer of a run's model: the model itself, or a MaskedAutoencoder's encoder."""
    return model.encoder if isinstance(model, MaskedAutoencoder) else model


def load_encoder(model, path):
    """--init-encoder: load a --save-encoder file (a VisionTransformer state_dict) into `model`.  mlp_head.* is skipped -- the head of a
    pretraining run never saw a gradient -- and everything else is strict: a key the file lacks, a key the model lacks or a shape that
    differs ends the run naming it.  The edge masks of a pruned file are rebuilt from its exact zeros, as for any loaded checkpoint."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(state, dict) or not all(torch.is_tensor(v) for v in state.values()):
        raise SystemExit(f"--init-encoder {path}: not a state_dict (a mapping of names to tensors)")
    own = model.state_dict()
    is_head = lambda k: k.startswith("mlp_head.")
    missing = sorted(k for k in own if not is_head(k) and k not in state)
    foreign = sorted(k for k in state if not is_head(k) and k not in own)
    shapes = sorted(k for k in state if not is_head(k) and k in own and tuple(state[k].shape) != tuple(own[k].shape))
    if missing or foreign or shapes:
        raise SystemExit(f"--init-encoder {path} does not fit the model: missing keys {missing}, unexpected keys {foreign}, "
                         f"shapes that differ {shapes}")
    model.load_state_dict({k: v for k, v in state.items() if not is_head(k)}, strict=False)
    if model.layer_types() <= set(model.REGULARIZED_TYPES):
        model.restore_edge_masks()


def save_encoder(model, optimizer, path, ema):
    """--save-encoder: the VisionTransformer's state_dict() to `path` (torch.save); with `ema` the averaged weights, the ones evaluate()
    would use."""
    with torch.no_grad(), (optimizer.ema_weights(model) if ema else contextlib.nullcontext()):
        state = {k: v.detach().to("cpu", copy=True) for k, v in encoder_of(model).state_dict().items()}
    torch.save(state, path)


def steps_per_epoch(args, batches, train_set, per_rank, world):
    """Steps every rank takes per epoch: the loop's count and, times --epochs, the length of kanvit-adamw's schedule."""
    if batches is not None:
        return len(batches)
    if train_set is not None:
        return train_set.n_batches(per_rank, world)
    if args.synthetic:
        return args.steps_per_epoch
    return -(-50000 // args.batch_size)         # CIFAR-100's train split as cifar_loaders serves it: len() of its train loader on every rank


def build_optimizer(args, model, per_epoch):
    if args.optimizer != "kanvit-adamw":
        # fused=True: same update rule as the reference's Adam, one multi-tensor kernel per parameter chunk instead of ~8 per step
        return Adam(model.parameters(), lr=args.learning_rate, fused=True, capturable=bool(args.graph))
    # --optimizer kanvit-adamw: clipping, decay, schedule and weight EMA in the project's own step (kanvit/optim.py); the schedule
    # spans the run, epochs x batches per epoch, and a step past it keeps the last row
    total = max(args.epochs * per_epoch, 1)
    return KanvitAdamW(model.parameters(), lr=args.learning_rate, weight_decay=float(args.weight_decay),
                       max_grad_norm=float(args.clip_grad_norm) or None, ema_decay=float(args.ema_decay), total_steps=total,
                       warmup_steps=min(int(args.warmup_steps), total), schedule=args.lr_schedule, min_lr=float(args.min_lr))


def build_step(args, model, optimizer, reducer, mixed):
    """The step that _GraphedStep captures: eager_step(x, y, y2=None, w=None) -> (CE loss, logits), both detached.  The loss is the
    reference's criterion, or with any of --mixup / --cutmix (`mixed`) / --label-smoothing / --fused-loss the fused soft-target
    cross-entropy (ops.soft_cross_entropy: loss and gradient in one launch).  --reg-lambda adds the KAN paper's sample-based
    regulariser of the same forward (exact fp32 also under --amp bf16) to what is differentiated; the returned (logged) loss stays
    the CE term, so trajectories with and without it compare.  --prune makes the gradients of pruned edges +0 between backward and
    the step (one ops.mask_rows call), so the optimizer keeps those entries at 0 and the clip norm is that of the gradients in use."""
    amp = args.amp == "bf16"
    label_smoothing = float(args.label_smoothing)
    soft_loss = mixed or label_smoothing > 0 or bool(args.fused_loss)
    reg_lambda = float(args.reg_lambda)
    reg_kw = dict(return_regularization=True, regularize_activation=float(args.reg_activation), regularize_entropy=float(args.reg_entropy))
    masking = bool(args.prune)
    criterion = torch.nn.CrossEntropyLoss()

    def pretrain_step(x, y, y2=None, w=None):
        """--pretrain mae: the same step around the reconstruction loss; the labels are ignored, and with no logits the second output is
        the loss again."""
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            loss = model(x)
        if reducer is not None:
            reducer.zero_grad()
            reducer.scale_loss(loss).backward()
            reducer.finish()
        else:
            optimizer.zero_grad()
            loss.backward()
        optimizer.step()
        return loss.detach(), loss.detach()
    if args.pretrain == "mae":
        return pretrain_step

    def eager_step(x, y, y2=None, w=None):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            if reg_lambda > 0:
                y_hat, reg = model(x, **reg_kw)
            else:
                y_hat = model(x)
            loss = kops.soft_cross_entropy(y_hat.float(), y, y2, w, label_smoothing) if soft_loss else criterion(y_hat.float(), y)
        total = loss + reg_lambda * reg.float() if reg_lambda > 0 else loss
        if reducer is not None:
            reducer.zero_grad()
            reducer.scale_loss(total).backward()    # mean over ranks inside the collective (RCCL AVG) or the loss: kanvit/dp.py
            reducer.finish()
        else:
            optimizer.zero_grad()
            total.backward()
        if masking:
            kprune.zero_masked(model.edge_masked(), of=lambda p: (p.grad,))
        optimizer.step()
        return loss.detach(), y_hat.detach()
    return eager_step


class Metrics:
    """(accuracy, balanced accuracy, F1, ROC AUC) of the (logits, labels) that update() saw since reset(): from host lists through
    utils.calculate_metrics, or, given `rows` (the most it will see), from the integer tables kanvit.metrics.EpochMetrics counts on the
    device (--device-metrics).  True once it saw anything."""

    def __init__(self, num_classes, device=None, rows=None):
        self.num_classes, self.seen = num_classes, []
        self.table = EpochMetrics(num_classes, max(rows, 1), device) if rows is not None else None

    def reset(self):
        self.seen = []
        if self.table is not None:
            self.table.reset()

    def update(self, logits, y):
        if self.table is not None:
            return self.table.update(logits, y)
        self.seen.append((y, logits.argmax(dim=1), torch.softmax(logits.float(), dim=1)))

    def __bool__(self):
        return bool(self.seen or (self.table is not None and self.table.n))

    def compute(self):
        if self.table is not None:
            return self.table.compute()
        ys, preds, probs = (torch.cat(column).cpu().numpy() for column in zip(*self.seen))
        return calculate_metrics(ys, preds, probs, num_classes=self.num_classes)


def run_epoch(run, epoch, loader, n_batches):
    """One epoch over `loader` with ONE host sync, the step losses' way to the host; rank 0's train metrics follow it.  run.step becomes a
    _GraphedStep at the first batch under --graph; run.n_steps counts the run's steps from 1, as --grid-extend and --prune name them."""
    args, model, optimizer, history, device = run.args, run.model, run.optimizer, run.history, run.device
    grid_extend, grid_every, prune_plan = args.grid_extend or {}, int(args.grid_update_every), args.prune or {}
    metrics = run.train_metrics
    step_losses = []
    if metrics is not None:
        metrics.reset()
    t_epoch = time.perf_counter()
    for x, y, *pair in loader:
        x, y = x.to(device, non_blocking=True), y.to(device, non_blocking=True)
        if args.graph and not isinstance(run.step, _GraphedStep):
            run.step = _GraphedStep(run.step, model, optimizer, x, y, *pair)
        run.n_steps = n_steps = run.n_steps + 1
        if n_steps in grid_extend:              # the extension refits on this batch too: an update due on the same step is skipped
            extend_grid_and_swap(model, optimizer, x, grid_extend[n_steps])
        elif grid_every > 0 and n_steps % grid_every == 0:
            model.update_grid(x)                # before the step, on the step's own batch; Adam's moments stay as they are
        if n_steps in prune_plan:               # before the step, on the step's own batch; parameters, moments and EMA of pruned edges -> 0
            prune_and_mask(model, optimizer, x, prune_plan[n_steps], args.prune_mode)
        loss, y_hat = run.step(x, y, *pair)
        if pair:                                # the metrics count a mixed sample against its majority label
            y = torch.where(pair[1] >= 0.5, y, pair[0])
        step_losses.append(loss.clone() if args.graph else loss)
        if metrics is not None:
            metrics.update(y_hat, y)            # eagerly after the step, also under --graph (y_hat is then the graph's output buffer)
    losses = torch.stack(step_losses) if step_losses else torch.zeros(0, device=device)
    if run.world > 1:                           # every rank's step loss is the mean over ITS shard; equal shards -> the mean
        torch.distributed.all_reduce(losses)            # of rank means is the global-batch mean the reference would log
        losses /= run.world
    if prune_plan:                              # --prune: the kept and total edge counts ride on the epoch's host sync
        edges = torch.stack(model.edge_sparsity())
    losses = losses.cpu()                       # the epoch's one host sync
    history["epoch_seconds"].append(time.perf_counter() - t_epoch)     # host clock around work that ends in that sync
    history["losses"] += [float(v) for v in losses]
    train_loss = float(losses.sum() / max(n_batches, 1))
    history["epoch_loss"].append(train_loss)
    if prune_plan:                              # two integers the device finished before the losses left it
        kept, total = (int(v) for v in edges.cpu())
        history.setdefault("edges", []).append((kept, total))
    if run.rank != 0:
        return
    logging.info(f"Epoch {epoch + 1}/{args.epochs}\n  Train Loss: {train_loss:.4f}")
    if prune_plan:
        logging.info(f"  Edges kept: {kept} of {total}")
    if metrics:
        t_metrics = time.perf_counter()         # host clock around work that ends with the four numbers on the host
        acc, bal, f1, auc = metrics.compute()
        history["train_metrics"].append((acc, bal, f1, auc))
        history["metrics_seconds"].append(time.perf_counter() - t_metrics)
        logging.info(f"  Train Accuracy: {acc:.4f}\n  Train Balanced Accuracy: {bal:.4f}\n"
                     f"  Train F1 Score: {f1:.4f}\n  Train ROC AUC: {auc:.4f}")
        if epoch == args.epochs - 1:
            save_metrics(run.metrics_file, epoch + 1, "Train", train_loss, acc, bal, f1, auc, flag=0)
            history["metrics_file"] = run.metrics_file


def evaluate(run, test_loader, per_rank):
    """The test pass (rank 0): the plain criterion, no drop-path, every patch, and with --ema-decay the averaged weights."""
    args, model, device, history = run.args, run.model, run.device, run.history
    ema = float(args.ema_decay) > 0             # --ema-decay (kanvit-adamw's alone): the test pass runs on the averaged weights
    criterion = torch.nn.CrossEntropyLoss()
    model.eval()
    if args.optimizer == "kanvit-adamw":
        history["ema_eval"] = ema
    with torch.no_grad(), (run.optimizer.ema_weights(model) if ema else contextlib.nullcontext()):
        tl = []
        metrics = Metrics(args.out_d, device, len(test_loader) * per_rank if args.device_metrics else None)
        for x, y in test_loader:
            x, y = x.to(device), y.to(device)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.amp == "bf16"):
                y_hat = model(x)
            tl.append(criterion(y_hat.float(), y))
            metrics.update(y_hat, y)
        test_loss = float(torch.stack(tl).sum() / len(test_loader))
        acc, bal, f1, auc = metrics.compute()
        history["test_metrics"] = (acc, bal, f1, auc)
        logging.info(f"Test Results:\n  Test Loss: {test_loss:.4f}\n  Test Accuracy: {acc:.4f}")
        save_metrics(run.metrics_file, args.epochs, "Test", test_loss, acc, bal, f1, auc, flag=1)


def main(args, batches=None, init_state=None):
    check_args(args)
    check_run_args(args)
    rank, world, device = setup_distributed(args)
    per_rank = args.batch_size // world if args.dp else args.batch_size
    torch.manual_seed(args.seed)
    train_set = test_set = None
    if batches is None and args.data_npz:
        train_set, test_set = npz_datasets(args, device, want_test=rank == 0)     # before the model: the geometry may come from the file
    size = int(args.resize) or args.image_size          # --resize S: --image-size stays the file's, the model sees S x S
    chw = (args.in_chans, size, size)
    model = build_model(args, chw, rank, world, device, init_state)
    mix = mix_config(args) if train_set is not None else None
    if not args.no_tuned_gemms:
        tuned.enable_tuned_gemms()          # recorded kernel selections for the stock FF GEMMs (no run-time tuning)
    n_batches = steps_per_epoch(args, batches, train_set, per_rank, world)
    optimizer = build_optimizer(args, model, n_batches)
    reducer = kdp.GradReducer(model.parameters()) if world > 1 else None
    metrics_file = setup_logging(args.log_dir) if rank == 0 else None
    logging.info(f"Using device: {device} ({torch.cuda.get_device_name(device)}), world {world}, amp {args.amp}, graph {bool(args.graph)}")
    if args.prune:
        model.edge_masked()     # --prune: the masks exist from the first step, all ones, and are rewritten in place -- a captured step keeps its one launch
    history = {"losses": [], "epoch_loss": [], "epoch_seconds": [], "train_metrics": [], "metrics_seconds": []}
    run = types.SimpleNamespace(args=args, rank=rank, world=world, device=device, model=model, optimizer=optimizer, history=history,
                                metrics_file=metrics_file, step=build_step(args, model, optimizer, reducer, mix is not None),
                                n_steps=0, train_metrics=None)          # what run_epoch and evaluate share
    train_loader = test_loader = sampler = None
    if train_set is not None:
        if test_set is not None:                # the evaluation transform: normalise only, in the file's order
            test_loader = test_set.loader(per_rank, shuffle=False)
    elif batches is None and not args.synthetic:
        train_loader, test_loader, sampler = cifar_loaders(per_rank, rank, world)
    model.train()
    for epoch in range(args.epochs):
        if batches is not None:
            loader = batches
        elif train_set is not None:             # order and augmentation are functions of (seed, epoch): the same on every rank
            loader = train_set.batches(per_rank, epoch, args.seed, rank, world, mix=mix)    # with mix: (x, y, y2, w), one table per epoch
        elif args.synthetic:
            loader = synthetic_loader(args.steps_per_epoch, per_rank, chw, args.out_d, device, args.seed + 1000 * epoch + rank)
        else:
            if sampler is not None:
                sampler.set_epoch(epoch)            # a different shuffle per epoch, the same on every rank
            loader = train_loader
        if epoch == 0 and rank == 0 and not args.no_step_metrics and args.pretrain is None:      # rank 0's shard; --device-metrics: sized here, once, reset per epoch
            rows =sum(int(b[1].shape[0]) for b in batches) if batches is not None else n_batches * per_rank
            run.train_metrics = Metrics(args.out_d, device, rows if args.device_metrics else None)
            if args.device_metrics:
                history["epoch_metrics"] = run.train_metrics.table
        run_epoch(run, epoch, loader, n_batches)

    if args.optimizer == "kanvit-adamw":
        history["grad_norm"] = float(optimizer.grad_norm)       # the last step's global norm (NaN without --clip-grad-norm: not taken)
    if test_loader is not None and rank == 0 and args.pretrain is None:      # --pretrain: no classifier to test
        evaluate(run, test_loader, per_rank)
    if args.save_encoder and rank == 0:
        save_encoder(model, optimizer, args.save_encoder, ema=float(args.ema_decay) > 0)
    if args.dp:
        torch.distributed.barrier()             # the other ranks wait for rank 0's evaluation before the group goes away
        torch.distributed.destroy_process_group()
    history.update(model=model, optimizer=optimizer)
    return history


def build_parser():
    p = argparse.ArgumentParser(description='Benchmark Vision Transformer on CIFAR-100')
    # the reference's flags, verbatim (train.py:87-97)
    p.add_argument('--epochs', type=int, default=20, help='number of epochs to train')
    p.add_argument('--batch-size', type=int, default=128, help='batch size for training')
    p.add_argument('--learning-rate', type=float, default=0.001, help='learning rate for optimizer')
    p.add_argument('--device', type=str, default='cuda' if torch.cuda.is_available() else 'cpu',
                   help='device to use for training (cuda/cpu)')
    p.add_argument('--model-type', type=str, default='vanilla', help='variant to run')
    p.add_argument('--n-blocks', type=int, default=8, help='number of transformer blocks')
    p.add_argument('--d-hidden', type=int, default=64, help='hidden dimension of transformer block')
    p.add_argument('--n-heads', type=int, default=8, help='number of attention heads')
    p.add_argument('--log-dir', type=str, default='logs', help='directory to store logs')
    # additions (defaults reproduce the geometry hard-coded at train.py:19)
    p.add_argument('--synthetic', action='store_true', help='synthetic image stream instead of CIFAR-100')
    p.add_argument('--steps-per-epoch', type=int, default=100, help='steps per epoch of the synthetic stream')
    p.add_argument('--image-size', type=int, default=32)
    p.add_argument('--in-chans', type=int, default=3)
    p.add_argument('--n-patches', type=int, default=4)
    p.add_argument('--out-d', type=int, default=100)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--dp', action='store_true', help='data parallel: one process per GPU (launch with torch.distributed.run)')
    p.add_argument('--no-step-metrics', action='store_true', help='skip per-step metric accumulation')
    p.add_argument('--device-metrics', action='store_true',
                   help='count the epoch metrics on the GPU (kanvit/metrics.py: confusion matrix and exact ROC-AUC pair counts; only '
                        'C*C + 2*C integers go to the host) instead of scikit-learn on host copies; the pair counts cost N^2 compares '
                        'per epoch, so this is for CIFAR-sized epochs; --no-step-metrics still switches the train metrics off')
    p.add_argument('--amp', choices=['off', 'bf16'], default='off',
                   help='bf16: autocast for the stock dense ops and the kanvit kernels on the bf16 matrix cores (fp32 I/O and '
                        'accumulation); off (default): the reference\'s fp32 arithmetic')
    p.add_argument('--graph', action='store_true', help='capture the whole train step in a HIP graph and replay it per batch')
    p.add_argument('--base-activation', choices=['silu', 'gelu', 'gelu-tanh', 'relu', 'tanh', 'identity'], default='silu',
                   help="base activation of every KANLinear / FastKANLayer ('efficientkan' and 'fast' model types)")
    p.add_argument('--reg-lambda', type=float, default=0.0,
                   help="weight of the KAN paper's sample-based L1 + entropy regulariser in the step's loss (CE + lambda * reg); "
                        "'efficientkan', 'cheby' and 'fast' model types; 0 (default): the plain step")
    p.add_argument('--reg-activation', type=float, default=1.0, help='weight of the L1 term inside the regulariser')
    p.add_argument('--reg-entropy', type=float, default=1.0, help='weight of the entropy term inside the regulariser')
    p.add_argument('--grid-update-every', type=int, default=0,
                   help="every N-th step, before the step, move the B-spline knots of every KANLinear to that step's batch and refit "
                        "the spline weights (VisionTransformer.update_grid; 'efficientkan' model types; not with --graph or --dp). "
                        "Adam's moments of spline_weight are left as they are, as upstream practice has it; 0 (default): never")
    p.add_argument('--grid-extend', type=parse_grid_extend, default={}, metavar='STEP:SIZE[,STEP:SIZE...]',
                   help="grid extension -- at the start of step STEP (counted from 1 over the whole run), on "
                        "that step's batch, move every KANLinear to SIZE grid intervals and fit the new spline coefficients so that "
                        "every edge keeps its function (VisionTransformer.extend_grid; 'efficientkan' model types; not with --graph "
                        "or --dp).  The replaced spline_weight parameters start with fresh Adam state, every other parameter keeps "
                        "its own; a --grid-update-every update due on the same step is skipped.  Default: never")
    p.add_argument('--prune', type=parse_prune, default={}, metavar='STEP:VALUE[,STEP:VALUE...]',
                   help="KAN edge pruning -- at the start of step STEP (counted from 1 over the whole run), on that step's batch, prune "
                        "the weakest edges of every KAN layer by their mean absolute activation (VisionTransformer.prune_edges; "
                        "'efficientkan', 'cheby' and 'fast' model types; not with --dp) and zero their optimizer state; from the first "
                        "step on, one masking launch between backward and the optimizer step keeps pruned edges at exactly 0, with "
                        "--graph too.  VALUE is what --prune-mode says.  Default: never")
    p.add_argument('--prune-mode', choices=list(PRUNE_MODES), default='fraction',
                   help="--prune: VALUE is the share of every layer's edges that ends up pruned (fraction, cumulative over the named "
                        "steps), or a threshold on the edge scores relative to the layer's largest (relative, 0..1), or absolute")
    p.add_argument('--no-tuned-gemms', action='store_true', help='library-default kernel selection for the stock GEMMs')
    p.add_argument('--data-npz', type=str, default=None, metavar='PATH',
                   help='train on this .npz (x_train uint8 [N,H,W,C] or [N,H,W], y_train; optional x_test, y_test, mean, std: '
                        'kanvit/data.py), kept on the GPU as uint8; every batch is one gather + crop + flip + normalise kernel. '
                        '--image-size and --in-chans follow the file when left at their defaults')
    p.add_argument('--no-augment', action='store_true', help='with --data-npz: normalise only (no random crop, no flip)')
    p.add_argument('--crop-padding', type=int, default=4,
                   help="with --data-npz: zero padding of the random crop, the reference's RandomCrop(32, padding=4); unused with "
                        "--random-resized-crop")
    p.add_argument('--resize', type=int, default=0, metavar='S',
                   help='with --data-npz: resize every batch to S x S inside the batch kernel (bilinear, half-pixel centres, no '
                        'antialiasing: meant for upsampling and mild downsampling; ops.resample_u8) and build the model at S x S; the '
                        'test split is resized too.  --image-size keeps its meaning, the size of the stored images.  0 (default): off')
    p.add_argument('--random-resized-crop', action='store_true',
                   help="with --data-npz: torchvision's RandomResizedCrop in place of the padded random crop (--crop-padding is then "
                        'unused; the flip stays), from a per-epoch table that is a function of (seed, epoch) alone (kanvit/data.py: '
                        'crop_table); the output size is --resize S, else the stored size')
    p.add_argument('--rrc-scale', type=float, nargs=2, default=(0.08, 1.0), metavar=('LO', 'HI'),
                   help='--random-resized-crop: the range of the box area as a fraction of the image')
    p.add_argument('--rrc-ratio', type=float, nargs=2, default=(3.0 / 4.0, 4.0 / 3.0), metavar=('LO', 'HI'),
                   help='--random-resized-crop: the range of the box aspect ratio (log-uniform)')
    p.add_argument('--random-erasing', type=float, default=0.0, metavar='P',
                   help="with --data-npz: Random Erasing (torchvision's RandomErasing / timm's, per sample, at the output size, after "
                        'normalisation, before Mixup / CutMix) inside the batch kernel -- with probability P a box from a per-epoch table, '
                        'a function of (seed, epoch) alone, is replaced (kanvit/data.py erase_table, ops.erase_u8); the train split only.  '
                        '0 (default): off')
    p.add_argument('--erase-mode', choices=('pixel', 'const'), default='pixel',
                   help="--random-erasing: 'pixel' fills the box with standard-normal noise per value (timm's pixel mode, DeiT's default), "
                        "'const' with zeros, the normalised dataset mean")
    p.add_argument('--erase-scale', type=float, nargs=2, default=(0.02, 1.0 / 3.0), metavar=('LO', 'HI'),
                   help='--random-erasing: the range of the box area as a fraction of the image')
    p.add_argument('--erase-ratio', type=float, nargs=2, default=(0.3, 1.0 / 0.3), metavar=('LO', 'HI'),
                   help='--random-erasing: the range of the box aspect ratio (log-uniform)')
    p.add_argument('--randaug', type=float, nargs='?', const=9.0, default=None, metavar='M',
                   help="with --data-npz: RandAugment (timm's rand-mM-mstd0.5-inc1; M defaults to 9) as one uint8 -> uint8 pass over the "
                        'whole train split per epoch, into a second GPU-resident copy that the batch kernel then reads (kanvit/data.py '
                        'randaug_table, ops.randaugment_u8): --randaug-ops ops per sample out of fifteen, from a per-epoch table that is a '
                        'function of (seed, epoch) alone, in integer arithmetic at the STORED size, before crop / flip / resize (timm '
                        'applies them after RandomResizedCrop); geometric ops fill with the dataset mean.  The train split only; images '
                        'of at most 24 576 bytes.  Default: off')
    p.add_argument('--randaug-ops', type=int, default=2, metavar='N', help='--randaug: ops per sample, 1 to 4')
    p.add_argument('--randaug-mstd', type=float, default=0.5, metavar='S',
                   help='--randaug: standard deviation of the per-op magnitude around M (clipped to 0..10)')
    p.add_argument('--randaug-prob', type=float, default=0.5, metavar='P', help='--randaug: probability that a drawn op is applied')
    p.add_argument('--mixup', type=float, default=0.0, metavar='ALPHA',
                   help='with --data-npz: Mixup -- blend every sample with a partner, lam ~ Beta(ALPHA, ALPHA), inside the batch kernel '
                        '(kanvit/data.py: mix_table, ops.mix_u8); the loss becomes the fused soft-target cross-entropy and the train '
                        'metrics count a mixed sample against its majority label (the one whose weight is at least 0.5).  0 (default): off')
    p.add_argument('--cutmix', type=float, default=0.0, metavar='ALPHA',
                   help="with --data-npz: CutMix -- paste a box of the partner, area ~ 1 - Beta(ALPHA, ALPHA) (timm's rand_bbox); the "
                        'same loss and the same majority-label rule for the train metrics as --mixup.  0 (default): off')
    p.add_argument('--mix-prob', type=float, default=1.0, metavar='P', help='probability that a sample is mixed at all (--mixup / --cutmix)')
    p.add_argument('--mix-switch-prob', type=float, default=0.5, metavar='P',
                   help='probability of CutMix for a mixed sample when both --mixup and --cutmix are given')
    p.add_argument('--label-smoothing', type=float, default=0.0, metavar='EPS',
                   help='label smoothing of the training loss, in [0, 1) (through the fused soft-target cross-entropy; the test loss '
                        'stays plain).  0 (default): off')
    p.add_argument('--fused-loss', action='store_true',
                   help='the fused cross-entropy kernel (ops.soft_cross_entropy: loss and gradient in one launch) also for the plain '
                        'training loss; opt-in, the default stays torch.nn.CrossEntropyLoss')
    p.add_argument('--optimizer', choices=['adam', 'kanvit-adamw'], default='adam',
                   help="adam (default): the reference's torch Adam at a constant learning rate.  kanvit-adamw: AdamW in the project's own "
                        'fused step (kanvit/optim.py) -- global-norm clipping, decoupled weight decay, warm-up / cosine schedule from a '
                        'device table and a weight EMA in one pass over the parameters; the flags below belong to it and are refused '
                        'without it; not with --grid-extend')
    p.add_argument('--weight-decay', type=float, default=0.0,
                   help='kanvit-adamw: decoupled weight decay of the weight matrices; biases, LayerNorm parameters, the class token and other '
                        'tensors that are vectors up to leading dimensions of size 1 are not decayed')
    p.add_argument('--clip-grad-norm', type=float, default=0.0, metavar='MAX',
                   help="kanvit-adamw: clip the global gradient norm to MAX (clip_grad_norm_'s rule); 0 (default): off")
    p.add_argument('--warmup-steps', type=int, default=0, help='kanvit-adamw: linear warm-up of the learning rate over this many steps')
    p.add_argument('--lr-schedule', choices=['constant', 'cosine'], default='constant',
                   help='kanvit-adamw: after the warm-up, a constant rate or cosine decay to --min-lr at the last step of the run')
    p.add_argument('--min-lr', type=float, default=0.0, help='kanvit-adamw: where --lr-schedule cosine ends')
    p.add_argument('--ema-decay', type=float, default=0.0, metavar='D',
                   help='kanvit-adamw: keep an exponential moving average of the weights (decay D, debiased) and run the test pass on it; '
                        '0 (default): off')
    p.add_argument('--drop-path', type=float, default=0.0, metavar='RATE',
                   help='stochastic depth (DropPath): in training, drop every residual branch per sample with a probability that grows '
                        'to RATE at the last block and scale the kept ones by 1 / (1 - p), inside the fused residual add + LayerNorm '
                        'passes (VisionTransformer.set_drop_path; masks from a hash of --seed and a device step counter, so --graph '
                        "works); not for 'flash-attn'; the test pass runs without it.  0 (default): off")
    p.add_argument('--drop-path-schedule', choices=['linear', 'constant'], default='linear',
                   help='--drop-path: the rate of block l of L is RATE * l / (L - 1) (linear, the DeiT / timm rule) or RATE in every block')
    p.add_argument('--patch-dropout', type=float, default=0.0, metavar='RATE',
                   help='PatchDropout: in training every sample keeps max(1, int(P * (1 - RATE))) of its P patch tokens (timm\'s rule) and '
                        'the class token, so a step costs roughly the kept fraction (VisionTransformer.set_patch_dropout; keep sets from a '
                        'hash of --seed and a device step counter, so --graph works); the test pass sees every patch.  0 (default): off')
    p.add_argument('--pretrain', choices=['mae'], default=None,
                   help='mae: masked-autoencoder pretraining (He et al. 2022; mae.py) -- the model of the flags becomes the encoder of a '
                        'MaskedAutoencoder, every sample keeps 1 - --mask-ratio of its patches (the kept-token path of --patch-dropout), a '
                        'light decoder reconstructs the dropped ones and the step differentiates the masked-patch loss (ops.restore_tokens, '
                        'ops.mae_loss); labels are ignored, train metrics and the test pass are off.  Works with --graph, --dp, --amp bf16 '
                        'and both optimizers; not with the label, regulariser, grid, pruning and --patch-dropout flags.  Default: off')
    p.add_argument('--mask-ratio', type=float, default=0.75, help='--pretrain mae: the share of patches dropped per sample')
    p.add_argument('--decoder-dim', type=int, default=0, help='--pretrain mae: width of the decoder; 0 (default): max(32, d_hidden / 2)')
    p.add_argument('--decoder-blocks', type=int, default=2, help='--pretrain mae: transformer blocks of the decoder')
    p.add_argument('--decoder-heads', type=int, default=0, help="--pretrain mae: heads of the decoder; 0 (default): the encoder's")
    p.add_argument('--decoder-type', type=str, default='vanilla', help='--pretrain mae: attention type of the decoder blocks (any --model-type but flash-attn)')
    p.add_argument('--no-norm-pix-loss', action='store_true',
                   help='--pretrain mae: compare with the raw pixels instead of every patch normalised by its own mean and variance')
    p.add_argument('--save-encoder', type=str, default=None, metavar='PATH',
                   help="after the last epoch, rank 0 writes the VisionTransformer's state_dict() to PATH (torch.save; under --pretrain the "
                        'encoder alone); with --ema-decay the averaged weights.  Not a resume facility: no optimizer state')
    p.add_argument('--init-encoder', type=str, default=None, metavar='PATH',
                   help='start from the weights of a --save-encoder file: everything but mlp_head.* (a pretrained head is untrained), strict; '
                        'then training runs as usual')
    return p


def parse(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    return args


if __name__ == "__main__":
    main(parse())
