// Internal header of the fused KAN layer kernels (csrc/kan_*.hip): launch arguments, tile constants, the plan structs the
// host entry points (kan_layer.hip) share with the kernel translation units, and the functions that cross between them.
// One translation unit per kernel generation keeps a rebuild at the size of the kernel that changed:
//     kan_layer.hip               C ABI entry points, validation, run-time switches, plan_layer_fwd / _bwd_input / _bwd_weight
//     kan_tile.hip                general LDS-tile producer/consumer kernels (every shape; fp32 and bf16 contraction)
//     kan_fwd_reg.hip             register-form forward (fp32 exact; also the fused patch embedding)
//     kan_fwd_reg_bf16.hip        register-form and W-stationary forward on the bf16 matrix cores
//     kan_bwd_input_reg.hip       register-form input gradient (fp32 exact)
//     kan_bwd_input_reg_bf16.hip  register-form input gradient on the bf16 matrix cores
//     kan_bwd_weight_reg.hip      streaming register-form weight gradient + the ordered slab reduction
//     kan_bwd_weight_dma.hip      the same wave unit fed through an LDS-DMA ring (ChebyKAN, three column tiles per wave)
//     kan_tiny.hip                tiny per-head layers on the vector pipe (all three operations)
#pragma once
#include "kan_basis.h"

#include <type_traits>
#include "kanvit_common.h"

#include <stdlib.h>

constexpr int BM = 128;          // rows per block in fwd / bwd_input (4 consumer waves x 32 rows)
constexpr int NTHR = 512;        // 4 consumer (MFMA) waves + 4 producer (load / basis) waves
constexpr int NPROD = 256;       // producer threads
constexpr int AS = BM + 1;       // row stride of the K-major LDS tiles
constexpr int BIN_NC = 32;       // dY columns staged per step in bwd_input
constexpr int BW_ROWS = 32;      // rows staged per step in bwd_weight
constexpr int BW_AS = BW_ROWS + 1;
constexpr int BW_NT = 2;         // 64 output columns per bwd_weight block
constexpr int BW_TPW = 5;        // max 32x32 MFMA tiles per consumer wave in bwd_weight
constexpr int BW_KC_MAX = 288;   // (BW_TPW*4 tiles / BW_NT) * 32 = 320 >= 288
constexpr int N_CU = 256;

struct LayerArgs {
    const float* x;
    const float* u;
    const float* w;
    const float* bp;
    const float* bias;
    float* y;
    const float* dy;
    float* dx;
    float* du;
    float* dparam;
    float* slab;
    const unsigned short* wb;   // bf16 fragment-major repack of w (KANVIT_FLAG_BF16_MFMA)
    const unsigned short* wb2;  // bf16 repack for the input-gradient kernel: [g][chunk][O/8][KCT][8 n]
    long long M, ldx, ldu, ldy, bp_stride, rows_per_split;
    int I, O, groups, xmod, G, GP, order, nk, has_base, K, IC, msplit, nchunks_n;
    float rbf_inv_h;
    int flags;
    // patch gather (kanvit_patch_embed_*): x is an NCHW image batch, row m = (sample m / P, patch m % P), feature i = (c, iy, ix)
    // of the patch (model.py:111-126); y rows are shifted behind `pg_pre` prepended rows per sample (the class token), `pos`
    // ([P + pg_pre][O]) is added and the class-token row cls + pos[0] is written by the lanes that own a sample's first patch
    int pg, pg_C, pg_H, pg_W, pg_n, pg_pre;
    const float* cls;
    const float* pos;
    // KANVIT_FLAG_FUSED_LN (RBF): the spline-path input u = LayerNorm(x slice) * gamma + beta (models/fastkan.py:68) is formed
    // in the kernels; bparams of a group = [centres(G) | gamma(I) | beta(I)]; stats[M][xmod][2] = (mean, rstd) per row and x
    // slice, written by the forward kernel and read by the two backward kernels
    int vcols;            // bf16 input gradient of ONE wide layer (O = 64*v): the v column chunks run as "groups" sharing x, basis and chain rule
    int ln;
    float ln_eps;
    float* stats;
    // launch tail (kv_tail_tiles): row tiles >= tail_y0 are cut into smaller work-groups that sit at the END of the grid and
    // fill the wave slots the last whole work-groups leave idle (forward: one projection each; input gradient: one feature chunk each)
    int tail_y0;
    int base_act;         // BSPLINE / RBF: KANVIT_BASE_* of the base column; nonzero launches the *_act_* kernels (KV_ACT_LAUNCH)
    // KV_VEC_*: the operands the host found on the 16-byte grid (LayerAlign::vec()).  The LDS-tile kernels (kan_tile.hip) never see a
    // plan condition on a pointer, so their 16-byte loads of w / dY are taken only with the bit set (wave-uniform, next to full_n /
    // vec_n); without it they run the per-element branch they have for ragged columns.  The register kernels ignore it: the plans
    // send them aligned operands only.
    int vec;
};
constexpr int KV_VEC_W = 1, KV_VEC_DY = 2;

// Row tiles [T1, T) of a launch of T row tiles x P work-groups per tile (two resident work-groups per CU) that should run as
// sub-divided work-groups.  Measured on ViT-B (197 tiles x 12 heads = 9.23 work-groups per CU): a CU runs its work-groups in
// pairs and a last single one at twice the speed, so the launch takes as long as 10 per CU although 60 of the 256 CUs get a
// tenth; cutting the tiles beyond 9 per CU into thirds / halves spreads that remainder over all CUs.
inline int kv_tail_first_tile(long long tiles, int per_tile) {
    const int cfg = kv_config().tail;
    if (cfg == 0 || tiles < 2) return (int)tiles;
    if (cfg > 0) return (int)(tiles - (cfg < tiles ? cfg : tiles - 1));
    const long long wgs = tiles * per_tile;
    const long long per_cu = wgs / N_CU;                      // whole work-groups every CU gets
    if (per_cu < 4) return (int)tiles;                       // short launches: the pieces' fixed costs outweigh the tail
    // the remainder beyond per_cu per CU, plus a quarter of a work-group per CU: the dispatcher hands work-groups to whichever CU
    // frees a slot, and a reserve of small pieces at the end evens out what that leaves uneven (measured: the launch time is flat
    // between 8 and 16 tail tiles of 12 and rises below 5; the pieces cost ~20 % more than the whole they replace)
    const long long rest = wgs - per_cu * N_CU + N_CU / 4;
    long long t1 = (wgs - rest) / per_tile;
    if (t1 < tiles / 2) t1 = tiles / 2;
    return (int)t1;
}

__device__ __forceinline__ BasisArgs make_basis(const LayerArgs& a, int g) {
    BasisArgs b;
    b.G = a.G;
    b.GP = a.GP;
    b.order = a.order;
    b.nk = a.nk;
    b.has_base = a.has_base;
    b.inv_h = a.rbf_inv_h;
    b.bp = a.bp ? a.bp + (long long)g * a.bp_stride : nullptr;
    b.uniform = (a.flags & KANVIT_FLAG_UNIFORM_KNOTS) && a.order == 3;
    b.act = a.base_act;
    return b;
}

// LayerNorm statistics of one row of I features held by a lane pair: this lane sees ICH consecutive features of every
// chunk of 2*ICH (xh points at its first one), its partner lane (l ^ 32) the others.  Two passes (mean, then centred
// sum of squares: the accuracy of torch's Welford kernel), biased variance, rstd = rsqrt(var + eps) as nn.LayerNorm.
template <int ICH>
__device__ __forceinline__ void kv_ln_row_stats(const float* __restrict__ xh, int nch, int I, float eps, float& mean, float& rstd) {
    float s = 0.0f;
    for (int c = 0; c < nch; ++c)
#pragma unroll
        for (int e = 0; e < ICH; ++e) s += xh[c * 2 * ICH + e];
    s += __shfl_xor(s, 32);
    mean = s / (float)I;
    float q = 0.0f;
    for (int c = 0; c < nch; ++c)
#pragma unroll
        for (int e = 0; e < ICH; ++e) {
            const float d = xh[c * 2 * ICH + e] - mean;
            q = fmaf(d, d, q);
        }
    q += __shfl_xor(q, 32);
    rstd = rsqrtf(q / (float)I + eps);
}

// Patch rows that exist only as an NCHW image batch (kanvit_patch_embed_*; model.py:111-126): row m = (image m / P, patch
// m % P).  The weight-gradient kernels visit the rows of a slab in order, a few per step, so the walker keeps the position
// of ONE row -- element offset of the patch origin (channel 0) from the image base, element offset of the row's dY row
// from the dY base (dY has pg_pre extra rows per image in front of the patch tokens) -- and advances it row by row: adds and
// compares on wave-uniform values (the scalar unit), no division after init().  Feature i = (c, iy, ix) of a patch adds
// the lane constant kv_patch_feature_offset().
struct PatchWalk {
    int px, py, xoff, dyoff;
    int n, pw, line_wrap, img_wrap, ldy, pre_ldy;
    __device__ __forceinline__ void init(const LayerArgs& a, int m) {
        n = a.pg_n;
        const int P = n * n, ph = a.pg_H / n;
        pw = a.pg_W / n;
        const int smp = m / P, pidx = m - smp * P;
        py = pidx / n;
        px = pidx - py * n;
        xoff = (smp * a.pg_C * a.pg_H + py * ph) * a.pg_W + px * pw;
        ldy = (int)a.ldy;
        pre_ldy = a.pg_pre * ldy;
        dyoff = (m + (smp + 1) * a.pg_pre) * ldy;
        line_wrap = ph * a.pg_W - n * pw;                       // last patch of a patch row -> first patch of the next one
        img_wrap = (a.pg_C * a.pg_H - n * ph) * a.pg_W;         // last patch of an image -> first patch of the next image
    }
    __device__ __forceinline__ void step() {      // branch-free: compares and selects on wave-uniform values (s_cmp / s_cselect)
        ++px;
        const bool w1 = px == n;                  // past the last patch of a patch row
        px = w1 ? 0 : px;
        py += w1 ? 1 : 0;
        const bool w2 = py == n;                  // past the last patch row of an image
        py = w2 ? 0 : py;
        xoff += pw + (w1 ? line_wrap : 0) + (w2 ? img_wrap : 0);
        dyoff += ldy + (w2 ? pre_ldy : 0);
    }
};

__device__ __forceinline__ int kv_patch_feature_offset(const LayerArgs& a, int f) {
    const int ph = a.pg_H / a.pg_n, pw = a.pg_W / a.pg_n;
    const int c = f / (ph * pw), r = f - c * (ph * pw), iy = r / pw, ix = r - iy * pw;
    return (c * a.pg_H + iy) * a.pg_W + ix;
}

__device__ __forceinline__ int kv_pow2_ge(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned kv_pack_bf16(float lo, float hi) {
    bf16x2_t v = {(__bf16)lo, (__bf16)hi};        // hipcc -O3: one v_cvt_pk_bf16_f32 (round to nearest even)
    return __builtin_bit_cast(unsigned, v);
}


// ---------------------------------------------------------------------------------------------
// host side: what the translation units share
// ---------------------------------------------------------------------------------------------
// RBF in the register kernels: only FastKAN's own uniform 8-centre grid (kv_rbf8: two exp anchors + recurrence); the caller
// vouches with KANVIT_FLAG_UNIFORM_KNOTS, anything else takes the LDS-tile kernels (direct exp per centre)
inline bool kv_rbf_reg_ok(int flags, int G) { return (flags & KANVIT_FLAG_UNIFORM_KNOTS) && G == 8; }

// families that get shared-basis (NSH = 3 / SHARED) kernel instantiations ...
template <int FAM>
constexpr bool kv_shared_basis() { return FAM == KV_LINEAR || FAM == KV_CHEBY || FAM == KV_FOURIER || FAM == KV_BSPLINE; }
// ... and whether a given launch may use them: parameter-free families always, BSPLINE when the caller vouches that the
// groups sharing x also share the knot table (KANVIT_FLAG_SHARED_BPARAMS)
inline bool kv_share_ok(int family, int flags) {
    return family == KANVIT_LINEAR || family == KANVIT_CHEBY || family == KANVIT_FOURIER ||
           (family == KANVIT_BSPLINE && (flags & KANVIT_FLAG_SHARED_BPARAMS));
}


#define KV_FAMILY_SWITCH(fam, CALL)                                   \
    switch (fam) {                                                    \
        case KANVIT_LINEAR: return CALL(KV_LINEAR);                   \
        case KANVIT_CHEBY: return CALL(KV_CHEBY);                     \
        case KANVIT_BSPLINE: return CALL(KV_BSPLINE);                 \
        case KANVIT_RBF: return CALL(KV_RBF);                         \
        case KANVIT_SINE: return CALL(KV_SINE);                       \
        case KANVIT_FOURIER: return CALL(KV_FOURIER);                 \
        default: return kv_fail(KANVIT_EINVAL, "unknown family %d", fam); \
    }

// ---- the compile-time basis sizes of the register kernels: ONE table --------------------------------------------------
// Which (family, generated columns per feature GP) have register kernels built for exactly that basis size (the shapes the
// reference's call sites build), and with which template arguments.  The five kernel generations differ on purpose:
//   * the fp32 forward takes ANY basis size through its run-time-GP loop (GPC = 0); fwd_gpc only names the pipelined twins;
//   * the bf16 forward and both input gradients exist for the listed sizes only, and the bf16 input gradient has neither
//     SINE GP = 5 (the layer's default grid; attention.py:140 builds 4) nor FOURIER;
//   * the weight gradient reads nt / njc (plan_bwd_weight_reg; DESIGN.md 4.5a says why these), and bww_pg names the rows whose
//     32-row kernel is also instantiated in its patch-gather form (kv_bwd_weight_reg).
// kan_tiny.hip keeps its own list: a different kernel family (run-time basis size on the vector pipe).
struct RegBasis {
    int family, gp;
    int fwd_gpc[3];             // fp32 forward <.., ICH, GPC>: GPC of the ICH = 4 / 2 / 1 instantiation, 0 = run-time GP
    int fwd_bf16_ich;           // bf16 forward <GP, .., ICH>: features per lane half and chunk, 0 = no kernel
    int bwi_kt, bwi_bf16_kt;    // input gradient <GP, KT>: exact fp32 / bf16 matrix cores, 0 = no kernel
    int bww_nt, bww_njc;        // weight gradient: column tiles per wave unit, basis windows
    int bww_pg;                 // weight gradient: 1 = the patch-gather instantiation exists
};
constexpr RegBasis KV_REG_BASES[] = {
    {KANVIT_LINEAR, 1, {1, 0, 0}, 8, 2, 2, 6, 1, 0},
    {KANVIT_CHEBY, 5, {5, 0, 0}, 8, 5, 5, 3, 1, 1},
    {KANVIT_BSPLINE, 9, {9, 9, 0}, 8, 5, 5, 3, 2, 0},      // 8 uniform cubic bases + the base column; ICH = 2: eight features x 9 rows x three projections overflow the W staging registers
    {KANVIT_RBF, 9, {9, 9, 0}, 8, 5, 5, 2, 1, 0},          // FastKAN's 8 centres + the base column
    {KANVIT_SINE, 4, {4, 0, 0}, 8, 4, 4, 2, 1, 0},         // the per-head mappings (attention.py:140)
    {KANVIT_SINE, 5, {0, 0, 0}, 0, 5, 0, 2, 1, 0},         // the layer's default grid
    {KANVIT_SINE, 28, {0, 0, 28}, 1, 7, 7, 4, 7, 1},       // the G = 28 patch embedding (model.py:72)
    {KANVIT_FOURIER, 56, {0, 0, 56}, 1, 7, 0, 4, 14, 1},
};

// the families the register kernels evaluate at all: B-splines on uniform cubic knots, FastKAN's own grid (kv_rbf_reg_ok), every parameter-free one
inline bool kv_reg_family_ok(int family, int flags, int order, int G) {
    if (family == KANVIT_BSPLINE) return (flags & KANVIT_FLAG_UNIFORM_KNOTS) && order == 3;
    if (family == KANVIT_RBF) return kv_rbf_reg_ok(flags, G);
    return true;
}

// the table's row for a layer, nullptr when its basis size has no compile-time register kernel
inline const RegBasis* kv_reg_basis(int family, int gp, int has_base, int flags, int order, int G) {
    if (!kv_reg_family_ok(family, flags, order, G)) return nullptr;
    if ((family == KANVIT_BSPLINE || family == KANVIT_RBF) && !has_base) return nullptr;
    for (const RegBasis& r : KV_REG_BASES)
        if (r.family == family && r.gp == gp) return &r;
    return nullptr;
}
inline const RegBasis* kv_reg_basis(const kanvit_layer_desc* d) {
    return kv_reg_basis(d->family, gp_of(d), d->has_base, d->flags, d->spline_order, d->G);
}

// the weight-gradient instantiations <FAM, GP> that also exist in the patch-gather form (KV_SINE_DF is SINE's twin)
constexpr bool kv_bww_pg(int fam, int gp) {
    for (const RegBasis& r : KV_REG_BASES)
        if (r.family == (fam == KV_SINE_DF ? KV_SINE : fam) && r.gp == gp) return r.bww_pg != 0;
    return false;
}

// accumulators the fp32 register input gradient contracts: CHEBY leaves the T0 slots out (dT0/dx = 0), see kan_bwd_input_reg.hip
constexpr int kv_bwi_g0(int fam) { return fam == KV_CHEBY ? 1 : 0; }
constexpr int kv_bwi_kt(int fam, int gp, int kt) { return ((16 * kt) / gp * (gp - kv_bwi_g0(fam)) + 15) / 16; }

// ---- plans: pure host functions of the descriptor (the workspace queries and the launches must agree) ----
struct FwdRegBf16Plan {
    bool ok;
    int gp, nt, nsh, ich, vs, nch;
    size_t lds, ws_bytes;
};

struct FwdBf16Plan {
    bool ok;
    int ic, nt, nsh, kc, kcp, nch;
    size_t lds, ws_bytes;
};

struct BwdRegBf16Plan {
    bool ok;
    int gp, kt, fph, nci;
    int vcols;            // > 0: one wide layer (groups = 1, O = 64*vcols) contracted 64 columns at a time into the same accumulators
    size_t lds, ws_bytes;
};

// shape side of the LDS-tile weight gradient (kan_tile.hip): feature chunk, grid, row split
struct BwPlan {
    int ic, nfchunks, nchunks_n, msplit, nsh;
    long long rows_per_split;
};

// shape side of the register weight gradients (kan_bwd_weight_reg.hip, kan_bwd_weight_dma.hip): the wave-unit geometry
struct BwRegPlan {
    bool ok;
    int gp, nt, nfb, nos, tiles_per_bg, nbg, shared, slabs, njc;
    int t16;              // 1: the 16-row-tile kernel (nt = 16-column tiles per wave, nfb = 16-feature blocks)
    int bf;               // 1: the planned kernel contracts on the bf16 matrix cores (KANVIT_FLAG_BF16_MFMA allows it; the exact kernels ignore it)
    int dma;              // 1: sized for the LDS-DMA form (a work-group = four row ranges of one wave unit, slabs counts WORK-GROUP slabs)
    long long rows_per_slab;
};

// ---- the plan of a forward / input-gradient / weight-gradient call (kan_layer.hip: plan_layer_fwd, plan_layer_bwd_input, -------
// plan_layer_bwd_weight).  Pure functions of the descriptor, kv_config() and the alignment of the operands: the workspace queries,
// kanvit_layer_ln_fusable, kanvit_layer_sine_dfreq_ok, kanvit_patch_embed_bwd_weight_ok and the launchers read the same plan, and the
// launchers below cannot refuse (DESIGN.md section 4.5a, tables of forms).
enum LayerFwdForm { LAYER_FWD_NONE, LAYER_FWD_TINY, LAYER_FWD_WS_BF16, LAYER_FWD_REG_BF16, LAYER_FWD_REG_BF16_PATCH, LAYER_FWD_TILE_BF16,
                    LAYER_FWD_REG, LAYER_FWD_TILE };
enum LayerBwdInputForm { LAYER_BWI_NONE, LAYER_BWI_TINY, LAYER_BWI_RES_BF16, LAYER_BWI_REG_BF16, LAYER_BWI_REG_BF16_WIDE, LAYER_BWI_TILE_BF16,
                         LAYER_BWI_REG, LAYER_BWI_TILE };
enum LayerBwdWeightForm { LAYER_BWW_NONE, LAYER_BWW_TINY, LAYER_BWW_DMA, LAYER_BWW_REG16, LAYER_BWW_REG, LAYER_BWW_REG_PATCH, LAYER_BWW_TILE,
                          LAYER_BWW_TILE_BF16 };

// The operand pointers whose alignment the plans look at (null pointers as 0; all 0 = aligned, the workspace queries' case)
struct LayerAlign {
    uintptr_t x, u, w, bp, bias, y, dy, dx, du;
    int has_u;            // RBF: the call passes the spline-path input u (its row stride ldu counts only then)
    int vec() const { return ((w & 15) ? 0 : KV_VEC_W) | ((dy & 15) ? 0 : KV_VEC_DY); }      // LayerArgs::vec
};

struct LayerFwdPlan {
    LayerFwdForm form;
    const char* why;      // form == NONE: the call fails with KANVIT_EINVAL and this text (a printf format taking why_a, why_b)
    int why_a, why_b;
    int nt, nsh;          // 32-column tiles per work-group, groups sharing one basis evaluation (1 or 3)
    int ich, gpc;         // REG: features per lane half and chunk, compile-time basis size (0 = the run-time-GP kernel)
    int ic, fast;         // TILE: feature chunk, predicate-free variant
    int strip;            // WS_BF16: the store strips fit the LDS beside the weight image
    int tail_y0;          // REG with nsh = 3: first row tile of the sub-divided tail (kv_tail_first_tile), 0x7fffffff = none
    unsigned gx, gy;      // grid of the layer kernel (the repack kernels size themselves)
    size_t lds;           // its dynamic LDS bytes
    size_t ws_bytes;      // workspace this form needs
    size_t ws_max;        // kanvit_layer_fwd_workspace: the most any alignment outcome needs (KANVIT_NO_BF16 does not lower it)
    FwdRegBf16Plan rb;    // WS_BF16, REG_BF16, REG_BF16_PATCH
    FwdBf16Plan tb;       // TILE_BF16
};

struct LayerBwdInputPlan {
    LayerBwdInputForm form;
    const char* why;
    int why_a, why_b;
    int gp, kt;           // register forms: the <GP, KT> instantiation (the table's row); TILE forms: kt = 32-row k tiles of a chunk
    int shared;           // the groups that read one x slice are summed in the accumulators (one chain rule per slice)
    int nsh;              // RES_BF16: projections per head (1 or 3)
    int ic, nci;          // features per chunk, chunks
    int tail_y0;          // REG, RES_BF16: first row tile of the sub-divided tail, 0x7fffffff = none
    unsigned gx, gy;
    size_t lds;
    size_t ws_bytes;      // workspace the call must bring: ws_max whenever dy allows a bf16 form (one size for all of them: the query cannot see the pointers)
    size_t ws_max;        // kanvit_layer_bwd_input_workspace
    BwdRegBf16Plan rb;    // RES_BF16, REG_BF16, REG_BF16_WIDE
};

struct LayerBwdWeightPlan {
    LayerBwdWeightForm form;
    const char* why;
    int why_a, why_b;
    int bf;               // the form contracts on the bf16 matrix cores (DMA, REG, TILE_BF16)
    int slabs;            // row ranges whose partial dW go to the workspace and are summed in order (1: the kernel writes dw itself)
    long long rows_per_slab;
    long long total;      // floats of one slab: groups * K * O
    size_t lds;           // TILE forms: dynamic LDS bytes
    size_t ws_bytes;      // kanvit_layer_bwd_weight_workspace / kanvit_patch_embed_bwd_weight_workspace
    BwRegPlan r;          // r.ok: a register kernel covers the shape (DMA, REG16, REG, REG_PATCH run it; the patch entry may still refuse)
    BwPlan t;             // TILE, TILE_BF16
};

LayerFwdPlan plan_layer_fwd(const kanvit_layer_desc* d, const kanvit_patch_desc* pd, const LayerAlign& al);
LayerBwdInputPlan plan_layer_bwd_input(const kanvit_layer_desc* d, const LayerAlign& al);
LayerBwdWeightPlan plan_layer_bwd_weight(const kanvit_layer_desc* d, const kanvit_patch_desc* pd, const LayerAlign& al);

// LDS bytes of the LDS-tile kernels (kan_tile.hip) for a feature chunk of ic
inline size_t kv_tile_fwd_lds(int family, int ic, int gp, int nt, int nsh) {
    const int kcp = (ic * gp + 1) & ~1;
    const size_t xarea = 2 * (size_t)BM * (ic | 1) * (family == KANVIT_RBF ? 2 : 1);
    const size_t opnd = 2 * ((size_t)kcp * AS + (size_t)kcp * 32 * nt * nsh);
    const size_t otile = (size_t)BM * (32 * nt * nsh + 4);          // staged output tile (FAST epilogue) aliases the operands
    return sizeof(float) * (xarea + (opnd > otile ? opnd : otile));
}
constexpr int KV_WS_THREADS = 512;   // W-stationary bf16 forward: 8 waves (12 measured slower: 66 row tiles over 21 work-groups per head quantise to 79 %)

inline size_t kv_tile_bwd_input_lds(int family, int ic, int gp, int G, int nshare, int bf_O) {
    const int kct = 32 * ((ic * gp + 31) / 32);
    const size_t ops = bf_O ? ((size_t)BM * (bf_O + 8) / 2 + (size_t)(bf_O / 8) * kct * 4)
                            : ((size_t)BIN_NC * AS + (size_t)BIN_NC * (kct + 1));
    return sizeof(float) * ((size_t)BM * (ic | 1) * (family == KANVIT_RBF ? 8 : 4) + (family == KANVIT_SINE ? (size_t)nshare * 4 * G : 0) +
                            (size_t)kct * AS + 2 * ops);
}

// chunking of the LDS-tile input-gradient kernel: the largest feature chunk (cap 96 columns) that fits the LDS, 0 = none does
inline int kv_tile_bwd_input_ic(int family, int I, int gp, int G, int nshare, int bf_O) {
    int ic = 96 / gp;
    if (ic < 1) ic = 1;
    if (ic > I) ic = I;
    while (ic > 1 && kv_tile_bwd_input_lds(family, ic, gp, G, nshare, bf_O) > 160 * 1024) --ic;
    return kv_tile_bwd_input_lds(family, ic, gp, G, nshare, bf_O) > 160 * 1024 ? 0 : ic;
}

// ---- launchers: each runs the form its plan names, with the plan's numbers; none of them decides or refuses ----------
int kv_fwd_reg(int family, const LayerArgs& a, const LayerFwdPlan& p, hipStream_t st);                     // kan_fwd_reg.hip
int kv_fwd_reg_bf16(int family, LayerArgs& a, const LayerFwdPlan& p, void* ws, hipStream_t st);            // kan_fwd_reg_bf16.hip
int kv_tile_fwd(int family, LayerArgs& a, const LayerFwdPlan& p, hipStream_t st);                          // kan_tile.hip
int kv_tile_fwd_bf16(int family, LayerArgs& a, const LayerFwdPlan& p, void* ws, hipStream_t st);
int kv_bwd_input_reg(int family, const LayerArgs& a, const LayerBwdInputPlan& p, hipStream_t st);         // kan_bwd_input_reg.hip
int kv_bwd_input_reg_bf16(int family, LayerArgs& a, const LayerBwdInputPlan& p, hipStream_t st);          // kan_bwd_input_reg_bf16.hip
int kv_tile_bwd_input(int family, LayerArgs& a, const LayerBwdInputPlan& p, hipStream_t st);              // kan_tile.hip; TILE_BF16: a.wb2 = the workspace
// the shape side of the bf16 plans (no alignment): members of the layer plans
FwdRegBf16Plan plan_fwd_reg_bf16(const kanvit_layer_desc* d);
FwdBf16Plan plan_fwd_bf16(const kanvit_layer_desc* d);
BwdRegBf16Plan plan_bwd_input_reg_bf16(const kanvit_layer_desc* d);
// ---- weight gradient: the shape-side pieces (members r / t of the layer plan) and the launchers of its forms ----
BwPlan plan_bwd_weight(const kanvit_layer_desc* d);                                                       // kan_tile.hip
BwRegPlan plan_bwd_weight_reg(const kanvit_layer_desc* d);                                                // kan_bwd_weight_reg.hip
int kv_tile_bwd_weight(int family, const LayerArgs& a, const LayerBwdWeightPlan& p, hipStream_t st);      // TILE, TILE_BF16
int kv_bwd_weight_reg(int family, LayerArgs& a, const LayerBwdWeightPlan& p, hipStream_t st);             // REG16, REG, REG_PATCH
int kv_bwd_weight_dma(LayerArgs& a, const LayerBwdWeightPlan& p, hipStream_t st);                         // DMA; kan_bwd_weight_dma.hip
int kv_slab_reduce(const float* slab, float* dw, long long total, int slabs, hipStream_t st);
