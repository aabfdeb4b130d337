"""Host restatements of the optimizer kernels (include/kanvit.h, csrc/optim.hip) for tests/test_optim_*.py.

adamw_f32      the update as NumPy float32 operations, one rounding each, in the kernel's order: equals the device bit for bit.
sumsq_partials / total_sumsq / norm_and_coef    the float64 norm in the kernels' own order of additions, and clip_grad_norm_'s rule.
Optimizer      a whole KanvitAdamW on the host, built from the two: parameters, flat moments, EMA, one global step."""
import numpy as np

CHUNK, THREADS, VEC, ROUNDS = 4096, 256, 4, 4
F = np.float32


def _f32(*xs):
    for x in xs:
        assert isinstance(x, np.ndarray) and x.dtype == np.float32 or isinstance(x, np.float32), type(x)
    return xs[0] if len(xs) == 1 else xs


def adamw_f32(p, g, m, v, e, row, consts, coef=None, decay=True, has_wd=True):
    """One update of float32 arrays p, g, m, v (and e, or None) -> (p, m, v, e).  row = the table's float32 row, consts = the seven
    float32 constants (b1, 1 - b1, b2, 1 - b2, eps, d, 1 - d), coef = the float32 clip coefficient or None (no clipping)."""
    b1, ob1, b2, ob2, eps, d, od = (F(c) for c in consts)
    r0, r1, r2 = (F(r) for r in np.asarray(row, dtype=np.float32)[:3])
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        if coef is not None:
            g = _f32(g * F(coef))
        if decay and has_wd:
            p = _f32(p * r0)
        m = _f32(_f32(b1 * m) + _f32(ob1 * g))
        v = _f32(_f32(b2 * v) + _f32(_f32(ob2 * g) * g))
        den = _f32(_f32(_f32(np.sqrt(v)) / r2) + eps)
        p = _f32(p - _f32(r1 * _f32(m / den)))
        if e is not None:
            e = _f32(_f32(d * np.asarray(e, dtype=np.float32)) + _f32(od * p))
    return p, m, v, e


def sumsq_partials(g):
    """The float64 partials of one tensor, one per chunk of CHUNK elements: thread t of THREADS adds the squares of elements
    VEC (THREADS r + t) + k in the order r = 0.., k = 0.., then part[t] += part[t + o] for o = THREADS / 2, .., 1."""
    g = np.asarray(g, dtype=np.float32).reshape(-1).astype(np.float64)
    out = []
    for lo in range(0, g.size, CHUNK):
        sq = np.zeros(CHUNK, dtype=np.float64)
        sq[:min(CHUNK, g.size - lo)] = g[lo:lo + CHUNK] ** 2               # past the end: + 0.0
        sq = sq.reshape(ROUNDS, THREADS, VEC)
        part = np.zeros(THREADS, dtype=np.float64)
        for r in range(ROUNDS):
            for k in range(VEC):
                part = part + sq[r, :, k]
        o = THREADS // 2
        while o:
            part[:o] = part[:o] + part[o:2 * o]
            o //= 2
        out.append(part[0])
    return np.asarray(out, dtype=np.float64)


def total_sumsq(partials):
    """The begin kernel's sum: thread t adds partials t, t + THREADS, .. in order, then the same tree."""
    partials = np.asarray(partials, dtype=np.float64)
    part = np.zeros(THREADS, dtype=np.float64)
    for lo in range(0, partials.size, THREADS):
        blk = partials[lo:lo + THREADS]
        part[:blk.size] = part[:blk.size] + blk
    o = THREADS // 2
    while o:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    return part[0]


def norm_and_coef(S, max_norm):
    """(float32 norm, float32 coefficient) from the float64 sum of squares: clip_grad_norm_'s rule in float64, rounded once."""
    with np.errstate(all="ignore"):
        root = np.sqrt(np.float64(S))
        c = np.float64(max_norm) / (root + 1e-6)
        return F(root), F(1.0 if c > 1.0 else c)


def grads_sumsq(grads):
    """The device's float64 sum of squares of a list of gradient arrays (None entries are skipped, as the optimizer skips them)."""
    parts = [sumsq_partials(g) for g in grads if g is not None]
    return total_sumsq(np.concatenate(parts) if parts else np.zeros(0))


def sumsq_two_orders(grads):
    """The float64 sum of squares taken sequentially and pairwise (NumPy's own reduction): two orders the device's lies between."""
    flat = np.concatenate([np.asarray(g, dtype=np.float32).reshape(-1).astype(np.float64) ** 2 for g in grads if g is not None])
    seq = np.float64(0.0)
    for x in flat:
        seq = seq + x
    return seq, np.sum(flat)


# ---- the cases tests/test_optim_gpu.py runs; tests/test_optim_cpu.py checks their clip coefficients' precondition -----------------
STEPS = 4
# the smallest sizes that can go wrong: below / at / above one 16-byte group, one wave's round (256 lanes), one chunk, two chunks; no
# element at all
EDGE_NUMELS = [1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 0]
NONE_GRAD = {(3, 1), (3, 2)}        # (tensor, step): tensor 3 gets no gradient on steps 1 and 2
# name -> (ema, max_norm, weight decay): clipping that binds, that does not, that is off; no decay
CONFIGS = {"ema_clip": (True, 0.5, 0.05), "noema_clip": (False, 0.5, 0.05), "loose_clip": (True, 1e4, 0.05), "no_clip": (True, None, 0.05),
           "no_wd": (False, 0.5, 0.0), "inf_clip": (False, float("inf"), 0.05)}


def tiny_numels(n):
    return [(1, 2, 3, 5, 8)[k % 5] for k in range(n)]


# the begin kernel's second lap: 81 + 261 + 1 = 343 partials (threads 0..86 add two) over 83 tensors, so two launches; the second
# launch holds tiny tensor 80, the 261-chunk tensor (chunks from first[1] = 1, partials from offset 80 of the workspace) and a 9-element
# one.  Tensor 81 is the large one: 81 % 4 = 1 puts its misaligned gradient 4 bytes off the 16-byte grid
LAP_NUMELS = tiny_numels(81) + [260 * CHUNK + 5, 9]
LAP_STEPS = 2                       # the sequential float64 order is a Python loop over 1.07 M elements: about a second per step


def case_params(numels, seed=0):
    rng = np.random.default_rng([seed, len(numels)])
    return [rng.standard_normal(n).astype(np.float32) for n in numels]


def case_grads(numels, step, seed=0, none=NONE_GRAD):
    """The gradients of one step: normal draws scaled per tensor over 1e-4 .. 1e0 (so that moments, denominators and the sum of
    squares see several binades), None where `none` names (tensor, step)."""
    rng = np.random.default_rng([seed, step, len(numels), 7])
    out = []
    for k, n in enumerate(numels):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0)).astype(np.float32)
        out.append(None if (k, step) in none else g)
    return out


def case_decay(numels):
    return [k % 3 != 1 for k in range(len(numels))]


def case_table(ema, wd, steps=STEPS):
    """A step_table's arguments for the cases: warm-up over 2 steps, then cosine."""
    return dict(total_steps=steps, lr=1e-2, betas=(0.9, 0.999), weight_decay=wd, warmup_steps=2, schedule="cosine", min_lr=1e-4,
                ema_decay=0.9 if ema else 0.0)


HUGE = (5000, 1e25, 1.0)            # (numel, value, max_norm): squares that overflow float32


def clip_cases(max_tensors):
    """Every synthetic clipping case tests/test_optim_gpu.py runs, as (name, numels, max_norm, none, steps): the edge list under each
    clipping config with the None gradients, the edge list without them (graph replay against eager), MAX and MAX + 1 tiny tensors,
    the list whose partials take the begin kernel past its first lap."""
    for name, (_, max_norm, _) in CONFIGS.items():
        if max_norm is not None:
            yield f"{name}/edge", EDGE_NUMELS, max_norm, NONE_GRAD, STEPS
    max_norm = CONFIGS["ema_clip"][1]
    yield "ema_clip/edge, every gradient", EDGE_NUMELS, max_norm, frozenset(), STEPS
    for n in (max_tensors, max_tensors + 1):
        yield f"ema_clip/{n} tiny", tiny_numels(n), max_norm, frozenset(), STEPS
    yield "ema_clip/lap", LAP_NUMELS, max_norm, frozenset(), LAP_STEPS


def coefficient_in_three_orders(grads, max_norm):
    """[(norm, coef)] from the float64 sum of squares taken sequentially, pairwise and in the device's order."""
    seq, pair = sumsq_two_orders(grads)
    return [norm_and_coef(S, max_norm) for S in (seq, pair, grads_sumsq(grads))]


class Optimizer:
    """KanvitAdamW on the host: params is a list of float32 arrays (copied), decay the flags, table / consts as the device takes them."""

    def __init__(self, params, decay, table, consts, max_norm=None, ema=False, has_wd=True):
        self.p = [np.array(p, dtype=np.float32) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.e = [np.zeros_like(p) for p in self.p] if ema else None
        self.decay, self.table, self.consts = list(decay), np.asarray(table, dtype=np.float32), consts
        self.max_norm, self.has_wd, self.t = max_norm, has_wd, 0
        self.norm = self.coef = None

    def step(self, grads):
        self.t += 1
        row = self.table[min(self.t, len(self.table)) - 1]
        coef = None
        if self.max_norm is not None:
            self.norm, self.coef = norm_and_coef(grads_sumsq(grads), self.max_norm)
            coef = self.coef
        for k, g in enumerate(grads):
            if g is None:
                continue
            e = self.e[k] if self.e is not None else None
            self.p[k], self.m[k], self.v[k], e = adamw_f32(self.p[k], g, self.m[k], self.v[k], e, row, self.consts, coef, self.decay[k], self.has_wd)
            if self.e is not None:
                self.e[k] = e
