// Fused KAN layer kernels for gfx950 (MI355X): the C ABI entry points (include/kanvit.h), descriptor validation, kernel
// selection and the run-time switches.  The kernels themselves live in one translation unit per generation
// (kan_layer_common.h lists them); every family is
//     Y[M x O] = Phi(X)[M x K] . W[K x O],   K = I*GP,  Phi generated on the fly from X[M x I]
// so the three operations are GEMMs whose generated operand never exists in HBM:
//     fwd         Y    = Phi(X) . W
//     bwd_input   dPhi = dY . W^T, then dX = sum_j dPhi_j * phi_j'(X)
//     bwd_weight  dW   = Phi(X)^T . dY          (split over row ranges -> slabs -> ordered reduce)
// Which kernel runs is decided ONCE per call, on the host, by plan_layer_fwd / plan_layer_bwd_input / plan_layer_bwd_weight (below):
// tiny per-head layers (kan_tiny.hip) -> the bf16 forms under KANVIT_FLAG_BF16_MFMA -> the exact register-form kernels (the shapes
// the reference instantiates on its 224x224 path, KV_REG_BASES) -> the general LDS-tile kernels (every other shape).  Every entry point is: validate, build the arguments, plan, check the workspace against
// the plan, launch the plan's form.  The workspace queries, kanvit_layer_ln_fusable, kanvit_layer_sine_dfreq_ok and
// kanvit_patch_embed_bwd_weight_ok read the same plans.
#include "kan_layer_common.h"

extern "C" int kanvit_layer_ln_fusable(const kanvit_layer_desc* d);

namespace {

int validate(const kanvit_layer_desc* d, const char* who) {
    if (!d) return kv_fail(KANVIT_EINVAL, "%s: null descriptor", who);
    const int gp = gp_of(d);
    if (gp < 1) return kv_fail(KANVIT_EINVAL, "%s: unknown family %d or G=%d", who, d->family, d->G);
    if (gp > 80) return kv_fail(KANVIT_EINVAL, "%s: %d generated columns per feature exceeds the supported 80", who, gp);
    if (d->groups < 1 || d->x_group_mod < 1 || d->groups % d->x_group_mod != 0)
        return kv_fail(KANVIT_EINVAL, "%s: groups=%d must be a positive multiple of x_group_mod=%d", who, d->groups,
                       d->x_group_mod);
    if (d->groups > 65535) return kv_fail(KANVIT_EINVAL, "%s: groups=%d exceeds 65535", who, d->groups);
    if ((d->M + BM - 1) / BM > 65535) return kv_fail(KANVIT_EINVAL, "%s: M=%lld exceeds %d rows per launch", who,
                                                     (long long)d->M, 65535 * BM);
    if (d->I < 1 || d->O < 1 || d->M < 0) return kv_fail(KANVIT_EINVAL, "%s: bad sizes M=%lld I=%d O=%d", who,
                                                          (long long)d->M, d->I, d->O);
    if ((long long)d->I * gp > 0x7fffffffLL / 4) return kv_fail(KANVIT_EINVAL, "%s: K too large", who);
    if (d->ldx < (int64_t)d->x_group_mod * d->I) return kv_fail(KANVIT_EINVAL, "%s: ldx=%lld < x_group_mod*I", who,
                                                                 (long long)d->ldx);
    if (d->ldy < (int64_t)d->groups * d->O) return kv_fail(KANVIT_EINVAL, "%s: ldy=%lld < groups*O", who,
                                                            (long long)d->ldy);
    if (d->family == KANVIT_BSPLINE) {
        const int nk = d->G + d->spline_order + 1;
        if (d->spline_order < 0 || d->G < 1 || nk > KV_MAX_KNOTS)
            return kv_fail(KANVIT_EINVAL, "%s: bspline G=%d order=%d unsupported (knots %d > %d)", who, d->G,
                           d->spline_order, nk, KV_MAX_KNOTS);
        if (d->bparam_stride < (int64_t)d->I * nk) return kv_fail(KANVIT_EINVAL, "%s: bparam_stride too small", who);
    }
    if (d->family == KANVIT_RBF && d->bparam_stride < d->G) return kv_fail(KANVIT_EINVAL, "%s: bparam_stride too small", who);
    if (d->base_act < KANVIT_BASE_SILU || d->base_act > KANVIT_BASE_IDENTITY)
        return kv_fail(KANVIT_EINVAL, "%s: unknown base activation %d (KANVIT_BASE_SILU .. KANVIT_BASE_IDENTITY)", who, d->base_act);
    if (d->base_act != KANVIT_BASE_SILU && (d->family != KANVIT_BSPLINE && d->family != KANVIT_RBF))
        return kv_fail(KANVIT_EINVAL, "%s: base activation %d set for family %d (only BSPLINE and RBF have a base column)", who,
                       d->base_act, d->family);
    if (d->base_act != KANVIT_BASE_SILU && !d->has_base)
        return kv_fail(KANVIT_EINVAL, "%s: base activation %d set with has_base = 0", who, d->base_act);
    if ((d->flags & KANVIT_FLAG_SINE_DFREQ) && d->family != KANVIT_SINE)
        return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_SINE_DFREQ is a SINE flag", who);
    if (d->flags & KANVIT_FLAG_FUSED_LN) {
        if (d->family != KANVIT_RBF) return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_FUSED_LN is an RBF (FastKAN) flag", who);
        if (d->bparam_stride < (int64_t)d->G + 2 * (int64_t)d->I)
            return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_FUSED_LN needs bparams = [centres(G) | gamma(I) | beta(I)] per group", who);
        if (!kanvit_layer_ln_fusable(d)) return kv_fail(KANVIT_EINVAL, "%s: shape not covered by the register kernels that fuse the LayerNorm", who);
    }
    if (d->family == KANVIT_SINE && d->bparam_stride < (int64_t)d->G * (1 + d->I))
        return kv_fail(KANVIT_EINVAL, "%s: bparam_stride too small", who);
    return 0;
}

LayerArgs base_args(const kanvit_layer_desc* d) {
    LayerArgs a{};
    a.M = d->M;
    a.ldx = d->ldx;
    a.ldu = d->ldu;
    a.ldy = d->ldy;
    a.bp_stride = d->bparam_stride;
    a.I = d->I;
    a.O = d->O;
    a.groups = d->groups;
    a.xmod = d->x_group_mod;
    a.G = d->G;
    a.GP = gp_of(d);
    a.order = d->spline_order;
    a.nk = d->G + d->spline_order + 1;
    a.has_base = d->has_base;
    a.K = d->I * a.GP;
    a.rbf_inv_h = d->rbf_inv_h;
    a.flags = d->flags;
    a.ln = (d->family == KANVIT_RBF && (d->flags & KANVIT_FLAG_FUSED_LN)) ? 1 : 0;
    a.ln_eps = d->ln_eps;
    a.tail_y0 = 0x7fffffff;             // no sub-divided tail unless a launcher sets one (kv_tail_first_tile)
    a.base_act = d->base_act;           // validated: nonzero only for BSPLINE / RBF with the base column
    return a;
}

int needs_bparams(int family) { return family == KANVIT_BSPLINE || family == KANVIT_RBF || family == KANVIT_SINE; }

// the argument checks every host query shares (a query answers 0 for a descriptor it cannot read)
bool desc_ok(const kanvit_layer_desc* d) {
    return d && gp_of(d) >= 1 && d->groups >= 1 && d->x_group_mod >= 1 && d->I >= 1 && d->O >= 1;
}

LayerAlign layer_align(const void* x, const void* u, const void* w, const void* bp, const void* bias, const void* y, const void* dy,
                       const void* dx, const void* du) {
    return LayerAlign{(uintptr_t)x, (uintptr_t)u, (uintptr_t)w, (uintptr_t)bp, (uintptr_t)bias, (uintptr_t)y, (uintptr_t)dy, (uintptr_t)dx,
                      (uintptr_t)du, u ? 1 : 0};
}

bool is_ln(const kanvit_layer_desc* d) { return d->family == KANVIT_RBF && (d->flags & KANVIT_FLAG_FUSED_LN); }

// form = NONE: the call fails with KANVIT_EINVAL and the text `why` (a printf format taking the two integers)
template <typename P>
P plan_none(P p, const char* why, int a = 0, int b = 0) {
    p.form = {};          // *_NONE
    p.why = why;
    p.why_a = a;
    p.why_b = b;
    return p;
}

// exact fp32 register forward (kan_fwd_reg.hip): sets form = REG when the shape and the operands are covered
void plan_fwd_reg(const kanvit_layer_desc* d, const kanvit_patch_desc* pd, const LayerAlign& al, LayerFwdPlan& p) {
    const int fam = d->family, gp = gp_of(d);
    if (kv_config().no_reg || !kv_reg_family_ok(fam, d->flags, d->spline_order, d->G)) return;
    // (Measured and rejected, round 3: EIGHT column tiles per generated value for SineKAN's G = 28 patch embedding -- it halves the
    // sine evaluations per MFMA, 5.5 -> 2.9 VALU instructions, but its 114 KB of W per work-group leave one wave per SIMD:
    // 10.06 -> 10.49 ms.)
    int nt = d->O <= 32 ? 1 : (d->O <= 64 ? 2 : 4);
    if (d->O % (32 * nt)) return;
    const long long tiles = (d->M + BM - 1) / BM;
    const int nshare = d->groups / d->x_group_mod;
    // Launches that cannot fill the chip (the small geometries' patch embedding: 2048 rows x 64 columns = 16 work-groups of two column
    // tiles): a wave's MFMA chain IS the kernel time there, so one column tile per work-group -- twice (four times) the work-groups, half
    // (a quarter of) the chain each; the basis is re-evaluated per column tile, the k order of every output is unchanged (bitwise equal).
    if (nt > 1 && tiles * (long long)d->groups * (d->O / (32 * nt)) < N_CU) nt = 1;
    // q|k|v sharing one basis evaluation (NSH = 3) triples the MFMA chain of every wave; when the launch has fewer
    // work-groups than CUs (the small geometries: 50 row tiles x 2 heads) the chain length IS the kernel time, so each
    // projection gets its own work-groups there and re-evaluates the basis
    const bool share3 = kv_share_ok(fam, d->flags) && nshare == 3 && nt <= 2 && tiles * d->x_group_mod >= N_CU;
    const int nsh = share3 ? 3 : 1;
    if ((d->O & 3) || (d->ldy & 3) || ((al.y | al.w | al.bias) & 15)) return;
    if (fam == KANVIT_SINE && ((al.bp & 15) || (d->bparam_stride & 3))) return;      // the phase rows are prefetched as 16-byte vectors
    const long long ldx = pd ? d->I : d->ldx;                                         // the gather has no row stride
    const bool has_u = fam == KANVIT_RBF && al.has_u && !is_ln(d);                    // FUSED_LN: the u slot carries the statistics
    const int wrow = 32 * nt * nsh, wrs = 256 / (8 * nt);
    const RegBasis* rb = kv_config().no_pipe ? nullptr : kv_reg_basis(d);             // the pipelined compile-time-GP twins
    for (int ich = 4; ich >= 1; ich >>= 1) {
        const int ic = 2 * ich, kc = ic * gp;
        if (d->I % ic) continue;
        if (pd && (((pd->W / pd->n_patches) % ic) || (ich == 4 && (pd->W & 3)))) continue;     // a chunk is ic consecutive pixels of one line
        if (ich == 4 && ((ldx & 3) || (d->I & 3) || (al.x & 15) || (has_u && ((d->ldu & 3) || (al.u & 15))))) continue;
        if ((kc + wrs - 1) / wrs > (share3 ? 4 : 8)) continue;                   // W passes held in registers
        if ((long long)kc * d->O >= (1LL << 30)) continue;
        size_t lds = sizeof(float) * 2 * (size_t)kc * wrow;
        // floor (the size of the four transposition patches the epilogue had before the flipped product; it stores straight from
        // registers now): kept as a number, what still reads this area after the last chunk are the T0 column sums of the CHEBY
        // compile-time-GP kernels, 5 x (32 * NT * NSH) floats, which a one-feature-pair chunk of a narrow layer would not cover
        if (lds < sizeof(float) * 4 * 32 * 36) lds = sizeof(float) * 4 * 32 * 36;
        if (lds > 160 * 1024) continue;
        p.form = LAYER_FWD_REG;
        p.nt = nt;
        p.nsh = nsh;
        p.ich = ich;
        p.gpc = rb ? rb->fwd_gpc[ich == 4 ? 0 : (ich == 2 ? 1 : 2)] : 0;
        p.lds = lds;
        p.gx = (unsigned)((d->groups / nsh) * (d->O / (32 * nt)));
        p.gy = (unsigned)tiles;
        if (nsh == 3 && p.gpc > 0) {              // the launch tail (kv_tail_first_tile): the last row tiles run one projection per work-group
            const int t1 = kv_tail_first_tile(tiles, (int)p.gx);
            if (t1 < tiles) {
                p.tail_y0 = t1;
                p.gy = (unsigned)(t1 + 3 * (tiles - t1));
            }
        }
        return;
    }
}

// bf16 register forward (kan_fwd_reg_bf16.hip): the W-stationary persistent form when the whole weight image of a column set fits the
// LDS and there are enough row tiles (instantiated for I = 64 per group: 4 chunks of 16 features -- the per-head q|k|v launches of
// ViT-B/S; LINEAR and CHEBY: the families whose basis fragments fit the register file), else one work-group per row tile
void plan_fwd_reg_bf16_form(const kanvit_layer_desc* d, const kanvit_patch_desc* pd, LayerFwdPlan& p) {
    const FwdRegBf16Plan& r = p.rb;
    p.nt = r.nt;
    p.nsh = r.nsh;
    p.ich = r.ich;
    p.ws_bytes = r.ws_bytes;
    p.gx = (unsigned)((d->groups / r.nsh) * (d->O / (32 * r.nt)));
    p.gy = (unsigned)((d->M + BM - 1) / BM);
    p.lds = r.lds;
    p.form = pd ? LAYER_FWD_REG_BF16_PATCH : LAYER_FWD_REG_BF16;
    if (pd || r.ich != 8 || !(d->family == KANVIT_LINEAR || d->family == KANVIT_CHEBY)) return;
    const size_t wlds = (size_t)r.nch * r.vs * 2 * 32 * r.nt * r.nsh * 16 + sizeof(float) * 32 * r.nt * r.nsh;
    if (wlds > 150 * 1024 || r.nch != 4 || d->M < 4096 || p.gx > N_CU || kv_config().no_ws) return;
    const long long ntiles = (d->M + KV_WS_THREADS / 2 - 1) / (KV_WS_THREADS / 2);
    long long py = N_CU / p.gx;                   // one work-group per CU (the image fills the LDS)
    if (py > ntiles) py = ntiles;
    if (py < 1) py = 1;
    const size_t slds = wlds + sizeof(float) * (KV_WS_THREADS / 64) * 32 * 36;       // + the store strips (see the kernel), when they fit
    p.form = LAYER_FWD_WS_BF16;
    p.strip = (slds <= 160 * 1024 && !kv_config().ws_no_strip) ? 1 : 0;
    p.gy = (unsigned)py;
    p.lds = p.strip ? slds : wlds;
}

// general LDS-tile forward (kan_tile.hip): every shape whose chunk fits the LDS
LayerFwdPlan plan_fwd_tile(const kanvit_layer_desc* d, const LayerAlign& al, LayerFwdPlan p) {
    const int fam = d->family, gp = gp_of(d);
    p.nt = d->O <= 32 ? 1 : (d->O <= 64 ? 2 : 4);
    p.nsh = (kv_share_ok(fam, d->flags) && d->groups / d->x_group_mod == 3 && p.nt <= 2) ? 3 : 1;
    // largest feature chunk whose two operand buffers fit the 160 KiB LDS (cap 80 columns)
    int ic = 80 / gp;
    if (ic < 1) ic = 1;
    if (ic > d->I) ic = d->I;
    while (ic > 1 && kv_tile_fwd_lds(fam, ic, gp, p.nt, p.nsh) > 160 * 1024) --ic;
    if (kv_tile_fwd_lds(fam, ic, gp, p.nt, p.nsh) > 160 * 1024)
        return plan_none(p, "kanvit_layer_fwd: %d generated columns per feature with O=%d does not fit the LDS", gp, d->O);
    // fast path: power-of-two chunk dividing I, whole column tiles, 32-bit tile-local offsets, and 16-byte rows of w, bias and y (it
    // loads W and stores its output tile as float4 without a test of its own); anything else takes the predicated variant
    int icf = 1;
    while (icf * 2 <= ic) icf *= 2;
    p.fast = (icf >= 8) && (d->I % icf == 0) && (d->O % (32 * p.nt) == 0) && ((long long)BM * d->ldx < (1LL << 30)) &&
             ((long long)BM * d->ldy < (1LL << 30)) && ((long long)BM * d->ldu < (1LL << 30)) &&
             ((long long)d->I * gp * d->O < (1LL << 30)) && !(d->ldy & 3) && !((al.y | al.bias | al.w) & 15) && !kv_config().no_fast;
    p.ic = p.fast ? icf : ic;
    p.form = LAYER_FWD_TILE;
    p.gx = (unsigned)((d->groups / p.nsh) * ((d->O + 32 * p.nt - 1) / (32 * p.nt)));
    p.gy = (unsigned)((d->M + BM - 1) / BM);
    p.lds = kv_tile_fwd_lds(fam, p.ic, gp, p.nt, p.nsh);
    return p;
}

}  // namespace

// pd != nullptr: the fused patch embedding (register forms only; x is the image batch, validated 16-byte aligned by the entry point)
LayerFwdPlan plan_layer_fwd(const kanvit_layer_desc* d, const kanvit_patch_desc* pd, const LayerAlign& al) {
    LayerFwdPlan p{};
    p.tail_y0 = 0x7fffffff;
    const char* uncovered = "kanvit_patch_embed_fwd: shape not covered by the fused kernel (O %% 32, patch width %% chunk, basis size); "
                            "use patchify + kanvit_layer_fwd";
    if (d->flags & KANVIT_FLAG_BF16_MFMA) {
        p.rb = plan_fwd_reg_bf16(d);
        if (!pd) p.tb = plan_fwd_bf16(d);
        const size_t a1 = p.rb.ok ? p.rb.ws_bytes : 0, a2 = p.tb.ok ? p.tb.ws_bytes : 0;
        p.ws_max = a1 > a2 ? a1 : a2;
    }
    if (!pd && kv_tiny_ok(d)) {       // tiny per-head layers (I, O <= 16): vector-pipe kernels, csrc/kan_tiny.hip
        p.form = LAYER_FWD_TINY;
        return p;
    }
    if ((d->flags & KANVIT_FLAG_BF16_MFMA) && !kv_config().no_bf16) {
        const FwdRegBf16Plan& r = p.rb;
        if (pd) {
            // the register-form forward in its patch form (one wide layer: four column tiles per work-group; a lane's feature chunk
            // must be consecutive pixels of one image line); nothing else gathers
            const int pw = pd->W / pd->n_patches;
            if (!(r.ok && r.nt == 4 && r.nsh == 1 && d->family != KANVIT_RBF && d->family != KANVIT_LINEAR && pw % (2 * r.ich) == 0 &&
                  (r.ich < 4 || (pd->W & 3) == 0) && !((al.y | al.bias | al.bp) & 15)))
                return plan_none(p, uncovered);
            plan_fwd_reg_bf16_form(d, pd, p);
            return p;
        }
        if (r.ok && !((al.x | al.y | al.u | al.bias | al.bp) & 15)) {
            plan_fwd_reg_bf16_form(d, pd, p);
            return p;
        }
        // (its epilogue stores float4 rows of y and reads the bias as float4; a y or bias off the 16-byte grid runs exact)
        if (p.tb.ok && !is_ln(d) && !(d->ldy & 3) && !((al.y | al.bias) & 15)) {
            p.form = LAYER_FWD_TILE_BF16;
            p.nt = p.tb.nt;
            p.nsh = p.tb.nsh;
            p.ic = p.tb.ic;
            p.ws_bytes = p.tb.ws_bytes;
            p.gx = (unsigned)((d->groups / p.nsh) * (d->O / (32 * p.nt)));
            p.gy = (unsigned)((d->M + BM - 1) / BM);
            p.lds = p.tb.lds;
            return p;
        }
    }
    plan_fwd_reg(d, pd, al, p);
    if (p.form == LAYER_FWD_REG) return p;
    if (pd) return plan_none(p, uncovered);
    if (is_ln(d)) return plan_none(p, "kanvit_layer_fwd: KANVIT_FLAG_FUSED_LN needs the register kernel (alignment / shape)");
    return plan_fwd_tile(d, al, p);
}

LayerBwdInputPlan plan_layer_bwd_input(const kanvit_layer_desc* d, const LayerAlign& al) {
    LayerBwdInputPlan p{};
    p.tail_y0 = 0x7fffffff;
    const int fam = d->family, gp = gp_of(d), nshare = d->groups / d->x_group_mod;
    const long long tiles = (d->M + BM - 1) / BM;
    p.gp = gp;
    p.shared = (kv_share_ok(fam, d->flags) && nshare > 1) ? 1 : 0;
    p.gx = (unsigned)d->x_group_mod;
    p.gy = (unsigned)tiles;
    // KANVIT_FLAG_BF16_MFMA allows bf16, it does not require it: the layer widths the bf16 kernels are built for ...
    p.rb = plan_bwd_input_reg_bf16(d);
    const bool wide = d->groups == 1 && d->x_group_mod == 1 && d->O > 64 && d->O % 64 == 0 && d->O <= 64 * 64;      // register kernel only
    bool bf = (d->flags & KANVIT_FLAG_BF16_MFMA) && !kv_config().no_bf16 && (d->O == 16 || d->O == 32 || d->O == 64 || wide) && (d->ldy % 4 == 0);
    // ... and for SINE only the register one: the bf16 LDS-tile kernel measures SLOWER than the exact fp32 register kernel (0.81 vs
    // 0.38 ms on the ViT-B q|k|v launch)
    if (fam == KANVIT_SINE && !kv_config().no_reg && !p.rb.ok) bf = false;
    const int ic_bf = bf ? kv_tile_bwd_input_ic(fam, d->I, gp, d->G, nshare, d->O) : 0;
    if (bf) {
        const size_t reg_ws = p.rb.ok ? p.rb.ws_bytes : 0;
        const size_t lds_ws = ic_bf ? (size_t)d->groups * ((d->I + ic_bf - 1) / ic_bf) * (d->O / 8) * (32 * ((ic_bf * gp + 31) / 32)) * 16 : 0;
        p.ws_max = reg_ws > lds_ws ? reg_ws : lds_ws;
    }
    if (kv_tiny_ok(d)) {
        p.form = LAYER_BWI_TINY;
        return p;
    }
    bool wb = bf && !(al.dy & 15) && p.ws_max > 0;        // a bf16 form may run: the repacked weights go to the workspace
    p.ws_bytes = wb ? p.ws_max : 0;
    if (wb) {
        const BwdRegBf16Plan& r = p.rb;
        if (r.ok && !((al.x | al.dx | al.dy | al.u | al.du) & 15)) {
            p.kt = r.kt;
            p.ic = 2 * r.fph;
            p.nci = r.nci;
            p.lds = r.lds;
            if (r.vcols) {
                // one wide layer (the patch embedding: O = 384 / 768): its 64-column chunks are contracted one per step into the SAME
                // accumulators -- exactly the SHARED schedule with the chunks in the role of the groups that share x and the basis
                p.form = LAYER_BWI_REG_BF16_WIDE;
                p.shared = 1;
                p.gx = 1;
            } else if (fam != KANVIT_SINE && d->O == 64 && (nshare == 1 || nshare == 3) && !kv_config().bi_no_res) {
                p.form = LAYER_BWI_RES_BF16;      // the per-head layers: dY resident (see the kernel)
                p.nsh = nshare;
                if (r.nci > 1) p.tail_y0 = kv_tail_first_tile(tiles, d->x_group_mod);
                const long long t1 = p.tail_y0 < tiles ? p.tail_y0 : tiles;
                p.gy = (unsigned)(t1 + (long long)r.nci * (tiles - t1));
                p.lds = (size_t)3 * 4 * 2 * 32 * r.kt * 16 + sizeof(float) * 4 * 32 * (p.ic + 4);      // a ring of three W step images + four store strips
            } else {
                p.form = LAYER_BWI_REG_BF16;
            }
            return p;
        }
        // no LayerNorm fusion, no wide layers and no SINE in the LDS-tile bf16 kernel: the exact kernels run instead
        if (is_ln(d) || d->O > 64 || fam == KANVIT_SINE) wb = false;
    }
    // every form below addresses its tiles with 32-bit offsets
    if ((long long)BM * d->ldx >= (1LL << 30) || (long long)BM * d->ldy >= (1LL << 30) || (long long)BM * d->ldu >= (1LL << 30) ||
        (long long)d->I * gp * d->O >= (1LL << 30))
        return plan_none(p, "kanvit_layer_bwd_input: row strides / weight slab too large for 32-bit tile offsets");
    if (wb) {
        // the bf16 tile does not fit the LDS (no basis size of today's kernels: GP <= 80, O <= 64 always fits): the exact LDS-tile
        // kernel, NOT the register one -- what this route has always done once the workspace was claimed
        p.form = ic_bf ? LAYER_BWI_TILE_BF16 : LAYER_BWI_TILE;
        p.ic = ic_bf ? ic_bf : kv_tile_bwd_input_ic(fam, d->I, gp, d->G, nshare, 0);
        if (!p.ic) return plan_none(p, "kanvit_layer_bwd_input: tile does not fit the LDS");
    } else {
        // exact fp32 register kernel (kan_bwd_input_reg.hip): the table's basis sizes, whole chunks and column tiles, 16-byte rows
        const RegBasis* rb = kv_config().no_reg ? nullptr : kv_reg_basis(d);
        if (rb && rb->bwi_kt) {
            const int kt = rb->bwi_kt, fph = (16 * kt) / gp, ic = 2 * fph;
            if (!(d->I % ic || d->O % 32 || (d->ldx & 3) || (d->ldy & 3) || ((fph & 3) == 0 && (d->I & 3)) || ((al.x | al.dx | al.dy | al.w) & 15) ||
                  (long long)ic * gp * d->O >= (1LL << 30))) {
                const int kct = 32 * kv_bwi_kt(fam, gp, kt), hoff = (kct % 64 == 32) ? kct : kct + 32, ws2 = ((hoff + kct + 13) / 16) * 16 + 2;
                p.form = LAYER_BWI_REG;
                p.kt = kt;
                p.ic = ic;
                p.nci = d->I / ic;
                p.lds = sizeof(float) * (2 * 16 * ws2 + (fam == KANVIT_SINE ? (size_t)nshare * 4 * gp : 0));
                if (fam != KANVIT_SINE && p.nci > 1) p.tail_y0 = kv_tail_first_tile(tiles, d->x_group_mod);
                const long long t1 = p.tail_y0 < tiles ? p.tail_y0 : tiles;
                p.gy = (unsigned)(t1 + p.nci * (tiles - t1));
                return p;
            }
        }
        if (is_ln(d)) return plan_none(p, "kanvit_layer_bwd_input: KANVIT_FLAG_FUSED_LN needs the register kernel (alignment / shape)");
        p.form = LAYER_BWI_TILE;
        p.ic = kv_tile_bwd_input_ic(fam, d->I, gp, d->G, nshare, 0);
        if (!p.ic) return plan_none(p, "kanvit_layer_bwd_input: tile does not fit the LDS");
    }
    // general LDS-tile kernel (kan_tile.hip), exact or with the bf16 contraction
    p.kt = (p.ic * gp + 31) / 32;
    p.nci = (d->I + p.ic - 1) / p.ic;
    p.lds = kv_tile_bwd_input_lds(fam, p.ic, gp, d->G, nshare, p.form == LAYER_BWI_TILE_BF16 ? d->O : 0);
    return p;
}

static const char* const KV_PATCH_BWW_UNCOVERED =
    "kanvit_patch_embed_bwd_weight: layer / geometry not covered by the gathering weight-gradient kernels "
    "(kanvit_patch_embed_bwd_weight_ok); use patchify + kanvit_layer_bwd_weight";

// pd != nullptr: the patch embedding's gather (REG_PATCH or nothing).  Of the operands only the alignment of x and dy counts.
LayerBwdWeightPlan plan_layer_bwd_weight(const kanvit_layer_desc* d, const kanvit_patch_desc* pd, const LayerAlign& al) {
    LayerBwdWeightPlan p{};
    p.total = (long long)d->groups * d->I * gp_of(d) * d->O;
    auto slabs = [&p](int ws_slabs, int n, long long rows) {      // the partial slabs are the only workspace of every form
        p.slabs = n;
        p.rows_per_slab = rows;
        p.ws_bytes = ws_slabs > 1 ? sizeof(float) * (size_t)ws_slabs * (size_t)p.total : 0;
    };
    if (kv_tiny_ok(d)) {              // tiny per-head layers (I, O <= 16): csrc/kan_tiny.hip
        if (pd) return plan_none(p, KV_PATCH_BWW_UNCOVERED);
        // 128 rows (two staged chunks) per slab, at most 64 slabs: the chunks of a work-group run back to back behind a global-load latency
        // each, so few chunks per group beats few partials.  The rows are rounded to the kernel's 64-row chunks, which can lower the slab
        // count (M = 129: two slabs become one); the workspace stays what the query has always answered, the count BEFORE the rounding
        const int s = (int)((d->M + 127) / 128 < 64 ? (d->M + 127) / 128 : 64);      // >= 1: kv_tiny_ok has M >= 64
        const long long rows = ((d->M + s - 1) / s + 63) / 64 * 64;
        slabs(s, (int)((d->M + rows - 1) / rows), rows);
        p.form = LAYER_BWW_TINY;
        return p;
    }
    p.r = plan_bwd_weight_reg(d);
    if (p.r.ok) {                     // the register kernels (kan_bwd_weight_reg.hip, kan_bwd_weight_dma.hip)
        slabs(p.r.slabs, p.r.slabs, p.r.rows_per_slab);
        p.bf = p.r.bf;
        if (pd) {                     // exact fp32, one layer, a table row with the gather instantiation
            if (d->groups != 1 || p.r.bf || p.r.t16 || !kv_reg_basis(d)->bww_pg) return plan_none(p, KV_PATCH_BWW_UNCOVERED);
            p.form = LAYER_BWW_REG_PATCH;
        } else if (p.r.t16) {
            p.form = LAYER_BWW_REG16;
        } else {
            // DMA moves 16-byte pieces: the rows of x and dY must start on 16-byte boundaries (the strides and widths are multiples of
            // four floats in every DMA-sized plan).  Rows off that grid -- a view into the middle of a tensor -- run the register ring
            // under the SAME slab sizing: correct and slower, and the workspace does not depend on the pointers
            p.form = (p.r.dma && !((al.x | al.dy) & 15)) ? LAYER_BWW_DMA : LAYER_BWW_REG;
        }
        return p;
    }
    if (pd) return plan_none(p, KV_PATCH_BWW_UNCOVERED);
    // general LDS-tile kernel (kan_tile.hip), exact or with the bf16 contraction
    p.t = plan_bwd_weight(d);
    slabs(p.t.msplit, p.t.msplit, p.t.rows_per_split);
    p.bf = ((d->flags & KANVIT_FLAG_BF16_MFMA) && !kv_config().no_bf16) ? 1 : 0;
    if (is_ln(d)) return plan_none(p, "kanvit_layer_bwd_weight: KANVIT_FLAG_FUSED_LN needs the register kernel (shape)");
    if ((long long)BW_ROWS * d->ldy >= (1LL << 30)) return plan_none(p, "kanvit_layer_bwd_weight: ldy too large for 32-bit tile offsets");
    // (plan_bwd_weight's chunk keeps the MFMA tiles of a wave within its accumulators: KC <= 160 with three projections, <= 288 with one)
    const int kt = (p.t.ic * gp_of(d) + 31) / 32;
    p.lds = sizeof(float) * 2 * ((size_t)BW_ROWS * (p.t.ic | 1) * (d->family == KANVIT_RBF ? 2 : 1) + (size_t)BW_ROWS * 32 * BW_NT * p.t.nsh +
                                 (size_t)kt * 32 * BW_AS);
    if (p.lds > 160 * 1024) return plan_none(p, "kanvit_layer_bwd_weight: tile does not fit the LDS");
    p.form = p.bf ? LAYER_BWW_TILE_BF16 : LAYER_BWW_TILE;
    return p;
}

static KvTinyArgs tiny_args(const kanvit_layer_desc* d) {
    KvTinyArgs t{};
    t.M = d->M; t.ldx = d->ldx; t.ldy = d->ldy; t.bp_stride = d->bparam_stride;
    t.family = d->family; t.I = d->I; t.O = d->O; t.groups = d->groups; t.xmod = d->x_group_mod; t.G = d->G;
    t.GP = gp_of(d); t.K = d->I * t.GP; t.order = d->spline_order; t.nk = d->G + d->spline_order + 1;
    t.has_base = d->has_base; t.flags = d->flags; t.base_act = d->base_act;
    return t;
}

thread_local char g_kanvit_err[512] = "";

// ---- run-time switches: read once, reported, never consulted through getenv on the launch path ----
static KvConfig g_kv_config;
static int g_kv_config_state = 0;      // 0 = not loaded
static void kv_config_load() {
    KvConfig c{};
    auto flag = [](const char* n) { const char* v = getenv(n); return (v && *v && !(v[0] == '0' && !v[1])) ? 1 : 0; };
    auto num = [](const char* n) { const char* v = getenv(n); return v ? atoi(v) : 0; };
    c.no_reg = flag("KANVIT_NO_REG");
    c.no_reg_bw = flag("KANVIT_NO_REG_BW");
    c.bw_no_t16 = flag("KANVIT_BW_NO_T16");
    c.bw_no_dma = flag("KANVIT_BW_NO_DMA");
    c.bi_no_res = flag("KANVIT_BI_NO_RES");
    c.bw_dma_force = flag("KANVIT_BW_DMA_FORCE");
    c.ws_no_strip = flag("KANVIT_WS_NO_STRIP");
    c.no_fast = flag("KANVIT_NO_FAST");
    c.no_pipe = flag("KANVIT_NO_PIPE");
    c.no_ws = flag("KANVIT_NO_WS");
    c.no_bf16 = flag("KANVIT_NO_BF16");
    c.no_fused_ln = flag("KANVIT_NO_FUSED_LN");
    c.no_tiny = flag("KANVIT_NO_TINY");
    c.attn_v1 = flag("KANVIT_ATTN_V1");
    c.attn_v2 = flag("KANVIT_ATTN_V2");
    c.attn_v3 = flag("KANVIT_ATTN_V3");
    c.attn_v4 = flag("KANVIT_ATTN_V4");
    c.attn_no_ds = flag("KANVIT_ATTN_NO_DS");
    c.attn_grid = num("KANVIT_ATTN_GRID");
    c.ff_grid = num("KANVIT_FF_GRID");
    c.bf16_nsh = num("KANVIT_BF16_NSH");
    c.bf16_ic = num("KANVIT_BF16_IC");
    c.bs_bw_bf16 = num("KANVIT_BSPLINE_BW_BF16");
    c.tail = getenv("KANVIT_TAIL") ? atoi(getenv("KANVIT_TAIL")) : -1;
    snprintf(c.text, sizeof(c.text),
             "no_reg=%d no_reg_bw=%d bw_no_t16=%d no_fast=%d no_pipe=%d no_ws=%d no_bf16=%d no_fused_ln=%d no_tiny=%d attn_v1=%d attn_v2=%d attn_v3=%d attn_v4=%d attn_no_ds=%d attn_grid=%d bf16_nsh=%d bf16_ic=%d ff_grid=%d bs_bw_bf16=%d tail=%d bw_no_dma=%d bi_no_res=%d bw_dma_force=%d ws_no_strip=%d",
             c.no_reg, c.no_reg_bw, c.bw_no_t16, c.no_fast, c.no_pipe, c.no_ws, c.no_bf16, c.no_fused_ln, c.no_tiny, c.attn_v1, c.attn_v2, c.attn_v3, c.attn_v4, c.attn_no_ds, c.attn_grid, c.bf16_nsh, c.bf16_ic, c.ff_grid, c.bs_bw_bf16, c.tail, c.bw_no_dma, c.bi_no_res, c.bw_dma_force, c.ws_no_strip);
    g_kv_config = c;
    __atomic_store_n(&g_kv_config_state, 1, __ATOMIC_RELEASE);
}
const KvConfig& kv_config() {
    if (!__atomic_load_n(&g_kv_config_state, __ATOMIC_ACQUIRE)) kv_config_load();     // idempotent: a race loads the same values twice
    return g_kv_config;
}

extern "C" {

const char* kanvit_last_error(void) { return g_kanvit_err; }
const char* kanvit_config(void) { return kv_config().text; }
int kanvit_config_reload(void) {
    kv_config_load();
    return 0;
}
int kanvit_abi_version(void) { return KANVIT_ABI_VERSION; }
int kanvit_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return kv_fail(KANVIT_EDEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

size_t kanvit_layer_fwd_workspace(const kanvit_layer_desc* d) {
    if (!desc_ok(d) || !(d->flags & KANVIT_FLAG_BF16_MFMA)) return 0;
    return plan_layer_fwd(d, nullptr, LayerAlign{}).ws_max;
}

// the forms both forward entry points launch; `who` names the entry point in the workspace message
static int launch_layer_fwd(const kanvit_layer_desc* d, LayerArgs& a, const LayerFwdPlan& p, const char* who, void* workspace,
                            size_t workspace_bytes, hipStream_t st) {
    if (p.form == LAYER_FWD_NONE) return kv_fail(KANVIT_EINVAL, p.why, p.why_a, p.why_b);
    if (p.ws_bytes && (!workspace || workspace_bytes < p.ws_bytes || ((uintptr_t)workspace & 15)))
        return kv_fail(KANVIT_ENOMEM, "%s: workspace %zu bytes < required %zu (or not 16-byte aligned)", who, workspace_bytes, p.ws_bytes);
    a.tail_y0 = p.tail_y0;
    switch (p.form) {
        case LAYER_FWD_WS_BF16:
        case LAYER_FWD_REG_BF16:
        case LAYER_FWD_REG_BF16_PATCH: return kv_fwd_reg_bf16(d->family, a, p, workspace, st);
        case LAYER_FWD_TILE_BF16: return kv_tile_fwd_bf16(d->family, a, p, workspace, st);
        case LAYER_FWD_REG: return kv_fwd_reg(d->family, a, p, st);
        default: return kv_tile_fwd(d->family, a, p, st);
    }
}

int kanvit_layer_fwd(const kanvit_layer_desc* d, const float* x, const float* u, const float* w, const float* bparams,
                     const float* bias, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = validate(d, "kanvit_layer_fwd")) return rc;
    if (d->flags & KANVIT_FLAG_SINE_DFREQ) return kv_fail(KANVIT_EINVAL, "kanvit_layer_fwd: KANVIT_FLAG_SINE_DFREQ is a kanvit_layer_bwd_weight flag");
    if (d->M == 0) return 0;
    if (!x || !w || !y) return kv_fail(KANVIT_EINVAL, "kanvit_layer_fwd: null x/w/y");
    if (needs_bparams(d->family) && !bparams) return kv_fail(KANVIT_EINVAL, "kanvit_layer_fwd: family %d needs bparams", d->family);
    if (d->family == KANVIT_RBF && u && d->ldu < (int64_t)d->groups * d->I)
        return kv_fail(KANVIT_EINVAL, "kanvit_layer_fwd: ldu < groups*I");
    const LayerAlign al = layer_align(x, u, w, bparams, bias, y, nullptr, nullptr, nullptr);
    const LayerFwdPlan p = plan_layer_fwd(d, nullptr, al);
    if (p.form == LAYER_FWD_TINY) {
        KvTinyArgs t = tiny_args(d);
        t.x = x; t.w = w; t.bp = bparams; t.bias = bias; t.y = y;
        return kv_tiny_fwd(t, (hipStream_t)stream);
    }
    LayerArgs a = base_args(d);
    a.x = x;
    a.u = u;
    a.w = w;
    a.bp = bparams;
    a.bias = bias;
    a.y = y;
    a.vec = al.vec();
    if (a.ln) {                       // the u slot carries the statistics buffer [M][x_group_mod][2] (written here)
        if (!u || ((uintptr_t)u & 7)) return kv_fail(KANVIT_EINVAL, "kanvit_layer_fwd: KANVIT_FLAG_FUSED_LN needs the (8-byte aligned) statistics buffer in the u argument");
        a.stats = const_cast<float*>(u);
        a.u = nullptr;
    }
    return launch_layer_fwd(d, a, p, "kanvit_layer_fwd", workspace, workspace_bytes, (hipStream_t)stream);
}

/* 1 when the three register kernels that can form the FastKAN LayerNorm in-kernel cover this layer (pure host function): asks the
   three plans, for aligned operands, whether each would run a register form with the flag set */
int kanvit_layer_ln_fusable(const kanvit_layer_desc* d) {
    if (!desc_ok(d) || d->family != KANVIT_RBF || d->groups % d->x_group_mod) return 0;
    if (d->base_act < KANVIT_BASE_SILU || d->base_act > KANVIT_BASE_IDENTITY) return 0;      // every valid activation has the fused kernels
    if (d->M < 256) return 0;                              // fewer rows: the weight gradient's register kernel does not start, and the route is all three kernels or none
    {                                                      // kanvit_layer_ln_bwd's lane-group layout: one layer or q|k|v per x slice, a row of I features per lane group
        const int ns = d->groups / d->x_group_mod;
        if ((ns != 1 && ns != 3) || d->I > (ns == 3 ? 512 : 1024)) return 0;
    }
    if (kv_config().no_reg || kv_config().no_reg_bw || kv_config().no_fused_ln) return 0;      // the A/B switches that take a register kernel (or the route) away
    // Everything else is the plans' own and is no longer restated here: whole 32-feature / 32-column blocks and 16-byte rows (the
    // three register kernels), the forward's column tiling (32, 64, multiples of 128), the base column and FastKAN's 8-centre grid
    // (KV_REG_BASES), and the kernels' 32-bit offset bounds -- plan_bwd_weight_reg's rows-per-slab bound as before, and now also
    // plan_layer_bwd_input's tile-offset bound (row strides below 2^23 floats), which kanvit_layer_bwd_input has always refused.
    kanvit_layer_desc e = *d;
    e.flags |= KANVIT_FLAG_FUSED_LN;
    const bool bf = (d->flags & KANVIT_FLAG_BF16_MFMA) && !kv_config().no_bf16;
    if (plan_layer_fwd(&e, nullptr, LayerAlign{}).form != (bf ? LAYER_FWD_REG_BF16 : LAYER_FWD_REG)) return 0;
    const LayerBwdInputForm bi = plan_layer_bwd_input(&e, LayerAlign{}).form;
    if (bi != LAYER_BWI_REG && bi != LAYER_BWI_REG_BF16 && bi != LAYER_BWI_REG_BF16_WIDE && bi != LAYER_BWI_RES_BF16) return 0;
    return plan_layer_bwd_weight(&e, nullptr, LayerAlign{}).r.ok ? 1 : 0;
}

// ---- fused patch embedding (model.py:111-126 patchify, :144-152 class token + position embedding) ----
static int patch_validate(const kanvit_layer_desc* d, const kanvit_patch_desc* p, const char* who) {
    if (!p) return kv_fail(KANVIT_EINVAL, "%s: null patch descriptor", who);
    if (p->C < 1 || p->H < 1 || p->W < 1 || p->n_patches < 1 || p->H % p->n_patches || p->W % p->n_patches)
        return kv_fail(KANVIT_EINVAL, "%s: image %dx%dx%d is not divisible into %d x %d patches", who, p->C, p->H, p->W, p->n_patches,
                       p->n_patches);
    if (p->prepend_rows != 0 && p->prepend_rows != 1) return kv_fail(KANVIT_EINVAL, "%s: prepend_rows must be 0 or 1", who);
    const long long P = (long long)p->n_patches * p->n_patches, I = (long long)p->C * (p->H / p->n_patches) * (p->W / p->n_patches);
    if (d->groups != 1 || d->x_group_mod != 1) return kv_fail(KANVIT_EINVAL, "%s: one layer per launch (groups = 1)", who);
    if (d->I != I) return kv_fail(KANVIT_EINVAL, "%s: I=%d but a patch has %lld pixels", who, d->I, I);
    if (d->M % P) return kv_fail(KANVIT_EINVAL, "%s: M=%lld is not a whole number of images (%lld patches each)", who, (long long)d->M, P);
    if ((long long)p->C * p->H * p->W >= (1LL << 30)) return kv_fail(KANVIT_EINVAL, "%s: image too large for 32-bit offsets", who);
    if (d->family == KANVIT_RBF) return kv_fail(KANVIT_EINVAL, "%s: FastKAN needs its LayerNorm'ed input u (use kanvit_layer_fwd)", who);
    return 0;
}

static void patch_args(LayerArgs& a, const kanvit_patch_desc* p, const float* cls, const float* pos) {
    a.pg = 1;
    a.pg_C = p->C;
    a.pg_H = p->H;
    a.pg_W = p->W;
    a.pg_n = p->n_patches;
    a.pg_pre = p->prepend_rows;
    a.cls = cls;
    a.pos = pos;
    a.ldx = a.I;                         // unused by the gather; the value plan_fwd_reg tests in its place
}

int kanvit_patch_embed_fwd_ws(const kanvit_layer_desc* d, const kanvit_patch_desc* p, const float* images, const float* w,
                              const float* bparams, const float* bias, const float* cls, const float* pos, float* y,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = validate(d, "kanvit_patch_embed_fwd")) return rc;
    if (int rc = patch_validate(d, p, "kanvit_patch_embed_fwd")) return rc;
    if (d->M == 0) return 0;
    if (!images || !w || !y) return kv_fail(KANVIT_EINVAL, "kanvit_patch_embed_fwd: null images/w/y");
    if (needs_bparams(d->family) && !bparams) return kv_fail(KANVIT_EINVAL, "kanvit_patch_embed_fwd: family %d needs bparams", d->family);
    if (p->prepend_rows && !cls) return kv_fail(KANVIT_EINVAL, "kanvit_patch_embed_fwd: prepend_rows = 1 needs the class token");
    if (((uintptr_t)images | (uintptr_t)(cls ? cls : w) | (uintptr_t)(pos ? pos : w)) & 15)
        return kv_fail(KANVIT_EINVAL, "kanvit_patch_embed_fwd: images / cls / pos must be 16-byte aligned");
    LayerArgs a = base_args(d);
    a.x = images;
    a.w = w;
    a.bp = bparams;
    a.bias = bias;
    a.y = y;
    patch_args(a, p, cls, pos);
    // (an absent bias / bparams is tested as w: what this entry point has always done, so a misaligned w is refused only then)
    const LayerFwdPlan pl = plan_layer_fwd(d, p, layer_align(images, nullptr, w, bparams ? bparams : w, bias ? bias : w, y, nullptr, nullptr, nullptr));
    return launch_layer_fwd(d, a, pl, "kanvit_patch_embed_fwd", workspace, workspace_bytes, (hipStream_t)stream);
}

int kanvit_patch_embed_fwd(const kanvit_layer_desc* d, const kanvit_patch_desc* p, const float* images, const float* w,
                           const float* bparams, const float* bias, const float* cls, const float* pos, float* y, void* stream) {
    if (d && (d->flags & KANVIT_FLAG_BF16_MFMA) && !kv_config().no_bf16)
        return kv_fail(KANVIT_EINVAL, "kanvit_patch_embed_fwd: KANVIT_FLAG_BF16_MFMA needs a workspace (kanvit_patch_embed_fwd_ws)");
    return kanvit_patch_embed_fwd_ws(d, p, images, w, bparams, bias, cls, pos, y, nullptr, 0, stream);
}

// Weight gradient of the patch-embedding layer with the same gather: x rows from the NCHW images, dY rows from the token-sequence
// gradient [B][P + prepend_rows][ldy] (the class-token rows are stepped over) -- no transient patch matrix, no dY copy.
static bool patch_bwd_weight_geometry_ok(const kanvit_layer_desc* d, const kanvit_patch_desc* p) {
    if (!desc_ok(d) || !p || d->groups != 1 || d->x_group_mod != 1 || d->M < 1) return false;
    if (p->C < 1 || p->H < 1 || p->W < 1 || p->n_patches < 1 || p->H % p->n_patches || p->W % p->n_patches) return false;
    if (p->prepend_rows != 0 && p->prepend_rows != 1) return false;
    const long long P = (long long)p->n_patches * p->n_patches;
    if (d->I != (long long)p->C * (p->H / p->n_patches) * (p->W / p->n_patches) || d->M % P) return false;
    const long long B = d->M / P;
    // 32-bit element offsets from the image base / the dY base
    return B * p->C * p->H * p->W < (1LL << 31) && (d->M + B * p->prepend_rows + 1) * d->ldy < (1LL << 31);
}

int kanvit_patch_embed_bwd_weight_ok(const kanvit_layer_desc* d, const kanvit_patch_desc* p) {
    return patch_bwd_weight_geometry_ok(d, p) && plan_layer_bwd_weight(d, p, LayerAlign{}).form == LAYER_BWW_REG_PATCH;
}

size_t kanvit_patch_embed_bwd_weight_workspace(const kanvit_layer_desc* d, const kanvit_patch_desc* p) {
    if (!patch_bwd_weight_geometry_ok(d, p)) return 0;
    const LayerBwdWeightPlan pl = plan_layer_bwd_weight(d, p, LayerAlign{});
    return pl.form == LAYER_BWW_REG_PATCH ? pl.ws_bytes : 0;
}

// the forms both weight-gradient entry points launch, and the ordered sum of the partial slabs behind them
static int launch_layer_bwd_weight(const kanvit_layer_desc* d, LayerArgs& a, const LayerBwdWeightPlan& p, float* dw, void* workspace,
                                   hipStream_t st) {
    if (p.form == LAYER_BWW_NONE) return kv_fail(KANVIT_EINVAL, p.why, p.why_a, p.why_b);
    a.rows_per_split = p.rows_per_slab;
    a.msplit = p.slabs;
    a.slab = p.slabs > 1 ? (float*)workspace : dw;
    int rc;
    switch (p.form) {
        case LAYER_BWW_TINY: {
            KvTinyArgs t = tiny_args(d);
            t.x = a.x; t.bp = a.bp; t.dy = a.dy;
            t.slabs = p.slabs; t.rows_per_slab = p.rows_per_slab; t.slab = a.slab;
            rc = kv_tiny_bwd_weight(t, st);
            break;
        }
        case LAYER_BWW_DMA: rc = kv_bwd_weight_dma(a, p, st); break;
        case LAYER_BWW_REG16:
        case LAYER_BWW_REG:
        case LAYER_BWW_REG_PATCH: rc = kv_bwd_weight_reg(d->family, a, p, st); break;
        default:
            a.IC = p.t.ic;
            a.nchunks_n = p.t.nchunks_n;
            rc = kv_tile_bwd_weight(d->family, a, p, st);
    }
    if (rc || p.slabs <= 1) return rc;
    return kv_slab_reduce((const float*)workspace, dw, p.total, p.slabs, st);
}

int kanvit_patch_embed_bwd_weight(const kanvit_layer_desc* d, const kanvit_patch_desc* p, const float* images, const float* bparams,
                                  const float* dy, float* dw, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = validate(d, "kanvit_patch_embed_bwd_weight")) return rc;
    if (int rc = patch_validate(d, p, "kanvit_patch_embed_bwd_weight")) return rc;
    if (!dw) return kv_fail(KANVIT_EINVAL, "kanvit_patch_embed_bwd_weight: null dw");
    if (d->M == 0) {
        KV_HIP_CHECK(hipMemsetAsync(dw, 0, sizeof(float) * (size_t)d->I * gp_of(d) * d->O, (hipStream_t)stream));
        return 0;
    }
    if (!images || !dy) return kv_fail(KANVIT_EINVAL, "kanvit_patch_embed_bwd_weight: null images/dy");
    if (needs_bparams(d->family) && !bparams) return kv_fail(KANVIT_EINVAL, "kanvit_patch_embed_bwd_weight: family %d needs bparams", d->family);
    const LayerBwdWeightPlan pl = plan_layer_bwd_weight(d, p, layer_align(images, nullptr, nullptr, nullptr, nullptr, nullptr, dy, nullptr, nullptr));
    if ((d->flags & KANVIT_FLAG_SINE_DFREQ) && !pl.r.ok)     // as kanvit_layer_bwd_weight: never hand plain dW back as Q
        return kv_fail(KANVIT_EINVAL, "kanvit_patch_embed_bwd_weight: KANVIT_FLAG_SINE_DFREQ is not available for this layer (kanvit_layer_sine_dfreq_ok)");
    if (!patch_bwd_weight_geometry_ok(d, p) || pl.form != LAYER_BWW_REG_PATCH) return kv_fail(KANVIT_EINVAL, KV_PATCH_BWW_UNCOVERED);
    if (pl.ws_bytes > 0 && (!workspace || workspace_bytes < pl.ws_bytes))
        return kv_fail(KANVIT_ENOMEM, "kanvit_patch_embed_bwd_weight: workspace %zu bytes < required %zu", workspace_bytes, pl.ws_bytes);
    LayerArgs a = base_args(d);
    a.x = images;
    a.bp = bparams;
    a.dy = dy;
    patch_args(a, p, nullptr, nullptr);
    return launch_layer_bwd_weight(d, a, pl, dw, workspace, (hipStream_t)stream);
}

// 1 when a register weight-gradient kernel covers the layer: the forms that have the x * cos twin (KV_SINE_DF)
int kanvit_layer_sine_dfreq_ok(const kanvit_layer_desc* d) {
    if (!desc_ok(d) || d->family != KANVIT_SINE || d->M < 1) return 0;
    return plan_layer_bwd_weight(d, nullptr, LayerAlign{}).r.ok ? 1 : 0;
}

int64_t kanvit_layer_dparam_tiles(const kanvit_layer_desc* d) {
    if (!d || d->family != KANVIT_SINE) return 0;
    return (d->M + BM - 1) / BM;
}

size_t kanvit_layer_bwd_input_workspace(const kanvit_layer_desc* d) {
    if (!desc_ok(d)) return 0;
    return plan_layer_bwd_input(d, LayerAlign{}).ws_max;
}

int kanvit_layer_bwd_input(const kanvit_layer_desc* d, const float* x, const float* u, const float* w,
                           const float* bparams, const float* dy, float* dx, float* du, float* dparam, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (int rc = validate(d, "kanvit_layer_bwd_input")) return rc;
    if (d->M == 0) return 0;
    if (!x || !w || !dy || !dx) return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_input: null x/w/dy/dx");
    if (needs_bparams(d->family) && !bparams) return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_input: family %d needs bparams", d->family);
    if (d->family == KANVIT_SINE && !dparam) return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_input: SINE needs dparam");
    if (d->flags & KANVIT_FLAG_SINE_DFREQ) return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_input: KANVIT_FLAG_SINE_DFREQ is a kanvit_layer_bwd_weight flag");
    if (d->family == KANVIT_RBF && (u || du) && d->ldu < (int64_t)d->groups * d->I)
        return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_input: ldu < groups*I");
    if (d->family == KANVIT_SINE && (d->groups / d->x_group_mod) * 4 * d->G > 4096)
        return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_input: SINE G too large");
    const LayerAlign al = layer_align(x, u, w, bparams, nullptr, nullptr, dy, dx, du);
    const LayerBwdInputPlan p = plan_layer_bwd_input(d, al);
    hipStream_t st = (hipStream_t)stream;
    if (p.form == LAYER_BWI_TINY) {
        KvTinyArgs t = tiny_args(d);
        t.x = x; t.w = w; t.bp = bparams; t.dy = dy; t.dx = dx;
        return kv_tiny_bwd_input(t, st);
    }
    LayerArgs a = base_args(d);
    a.x = x;
    a.u = u;
    a.w = w;
    a.bp = bparams;
    a.dy = dy;
    a.dx = dx;
    a.du = du;
    a.dparam = dparam;
    a.vec = al.vec();
    if (a.ln) {                       // the kernels read a row's (mean, rstd) as one 8-byte pair
        if (!u || ((uintptr_t)u & 7)) return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_input: KANVIT_FLAG_FUSED_LN needs the (8-byte aligned) statistics buffer in the u argument");
        a.stats = const_cast<float*>(u);
        a.u = nullptr;
    }
    if (p.ws_bytes && (!workspace || workspace_bytes < p.ws_bytes || ((uintptr_t)workspace & 15)))
        return kv_fail(KANVIT_ENOMEM, "kanvit_layer_bwd_input: workspace %zu bytes < required %zu (or not 16-byte aligned)",
                       workspace_bytes, p.ws_bytes);
    a.tail_y0 = p.tail_y0;
    switch (p.form) {
        case LAYER_BWI_NONE: return kv_fail(KANVIT_EINVAL, p.why, p.why_a, p.why_b);
        case LAYER_BWI_RES_BF16:
        case LAYER_BWI_REG_BF16:
        case LAYER_BWI_REG_BF16_WIDE:
            a.wb2 = (const unsigned short*)workspace;      // the repacked weights
            return kv_bwd_input_reg_bf16(d->family, a, p, st);
        case LAYER_BWI_TILE_BF16:
            a.wb2 = (const unsigned short*)workspace;
            return kv_tile_bwd_input(d->family, a, p, st);
        case LAYER_BWI_REG: return kv_bwd_input_reg(d->family, a, p, st);
        default: return kv_tile_bwd_input(d->family, a, p, st);
    }
}

size_t kanvit_layer_bwd_weight_workspace(const kanvit_layer_desc* d) {
    if (!desc_ok(d)) return 0;
    return plan_layer_bwd_weight(d, nullptr, LayerAlign{}).ws_bytes;
}

int kanvit_layer_bwd_weight(const kanvit_layer_desc* d, const float* x, const float* u, const float* bparams,
                            const float* dy, float* dw, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = validate(d, "kanvit_layer_bwd_weight")) return rc;
    if (d->M == 0) {   // no rows: the gradient is exactly zero
        if (!dw) return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_weight: null dw");
        KV_HIP_CHECK(hipMemsetAsync(dw, 0, sizeof(float) * (size_t)d->groups * d->I * gp_of(d) * d->O, (hipStream_t)stream));
        return 0;
    }
    if (!x || !dy || !dw) return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_weight: null x/dy/dw");
    if (needs_bparams(d->family) && !bparams) return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_weight: family %d needs bparams", d->family);
    if (d->family == KANVIT_RBF && u && d->ldu < (int64_t)d->groups * d->I)
        return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_weight: ldu < groups*I");
    const LayerAlign al = layer_align(x, u, nullptr, bparams, nullptr, nullptr, dy, nullptr, nullptr);
    const LayerBwdWeightPlan p = plan_layer_bwd_weight(d, nullptr, al);
    if (p.ws_bytes > 0 && (!workspace || workspace_bytes < p.ws_bytes))
        return kv_fail(KANVIT_ENOMEM, "kanvit_layer_bwd_weight: workspace %zu bytes < required %zu", workspace_bytes, p.ws_bytes);
    if ((d->flags & KANVIT_FLAG_SINE_DFREQ) && !p.r.ok)
        return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_weight: KANVIT_FLAG_SINE_DFREQ needs the register weight-gradient kernel (shape)");
    LayerArgs a = base_args(d);
    a.x = x;
    a.u = u;
    a.bp = bparams;
    a.dy = dy;
    a.vec = al.vec();
    if (a.ln) {                       // the kernels read a row's (mean, rstd) as one 8-byte pair
        if (!u || ((uintptr_t)u & 7)) return kv_fail(KANVIT_EINVAL, "kanvit_layer_bwd_weight: KANVIT_FLAG_FUSED_LN needs the (8-byte aligned) statistics buffer in the u argument");
        a.stats = const_cast<float*>(u);
        a.u = nullptr;
    }
    return launch_layer_bwd_weight(d, a, p, dw, workspace, (hipStream_t)stream);
}

// ---- per-family named entry points ---------------------------------------------------------------
#define KV_DEFINE_FAMILY(name, FAMID)                                                                               \
    int kanvit_##name##_fwd(const kanvit_layer_desc* d, const float* x, const float* u, const float* w,            \
                            const float* bp, const float* bias, float* y, void* ws, size_t wsb, void* s) {         \
        if (!d || d->family != FAMID) return kv_fail(KANVIT_EINVAL, "kanvit_" #name "_fwd: descriptor family mismatch"); \
        return kanvit_layer_fwd(d, x, u, w, bp, bias, y, ws, wsb, s);                                               \
    }                                                                                                               \
    int kanvit_##name##_bwd_input(const kanvit_layer_desc* d, const float* x, const float* u, const float* w,      \
                                  const float* bp, const float* dy, float* dx, float* du, float* dp, void* ws,     \
                                  size_t wsb, void* s) {                                                            \
        if (!d || d->family != FAMID) return kv_fail(KANVIT_EINVAL, "kanvit_" #name "_bwd_input: descriptor family mismatch"); \
        return kanvit_layer_bwd_input(d, x, u, w, bp, dy, dx, du, dp, ws, wsb, s);                                  \
    }                                                                                                               \
    int kanvit_##name##_bwd_weight(const kanvit_layer_desc* d, const float* x, const float* u, const float* bp,    \
                                   const float* dy, float* dw, void* ws, size_t wsb, void* s) {                    \
        if (!d || d->family != FAMID) return kv_fail(KANVIT_EINVAL, "kanvit_" #name "_bwd_weight: descriptor family mismatch"); \
        return kanvit_layer_bwd_weight(d, x, u, bp, dy, dw, ws, wsb, s);                                            \
    }                                                                                                               \
    int kanvit_##name##_qkv_fwd(const kanvit_layer_desc* d, const float* x, const float* u, const float* w,        \
                                const float* bp, const float* bias, float* y, void* ws, size_t wsb, void* s) {     \
        if (!d || d->family != FAMID || d->groups != 3 * d->x_group_mod)                                            \
            return kv_fail(KANVIT_EINVAL, "kanvit_" #name "_qkv_fwd: need family match and groups == 3*x_group_mod"); \
        return kanvit_layer_fwd(d, x, u, w, bp, bias, y, ws, wsb, s);                                               \
    }                                                                                                               \
    int kanvit_##name##_qkv_bwd_input(const kanvit_layer_desc* d, const float* x, const float* u, const float* w,  \
                                      const float* bp, const float* dy, float* dx, float* du, float* dp, void* ws, \
                                      size_t wsb, void* s) {                                                        \
        if (!d || d->family != FAMID || d->groups != 3 * d->x_group_mod)                                            \
            return kv_fail(KANVIT_EINVAL, "kanvit_" #name "_qkv_bwd_input: need family match and groups == 3*x_group_mod"); \
        return kanvit_layer_bwd_input(d, x, u, w, bp, dy, dx, du, dp, ws, wsb, s);                                  \
    }                                                                                                               \
    int kanvit_##name##_qkv_bwd_weight(const kanvit_layer_desc* d, const float* x, const float* u, const float* bp, \
                                       const float* dy, float* dw, void* ws, size_t wsb, void* s) {                \
        if (!d || d->family != FAMID || d->groups != 3 * d->x_group_mod)                                            \
            return kv_fail(KANVIT_EINVAL, "kanvit_" #name "_qkv_bwd_weight: need family match and groups == 3*x_group_mod"); \
        return kanvit_layer_bwd_weight(d, x, u, bp, dy, dw, ws, wsb, s);                                            \
    }
KV_DEFINE_FAMILY(linear, KANVIT_LINEAR)
KV_DEFINE_FAMILY(cheby, KANVIT_CHEBY)
KV_DEFINE_FAMILY(bspline, KANVIT_BSPLINE)
KV_DEFINE_FAMILY(rbf, KANVIT_RBF)
KV_DEFINE_FAMILY(sine, KANVIT_SINE)
KV_DEFINE_FAMILY(fourier, KANVIT_FOURIER)

}  // extern "C"

