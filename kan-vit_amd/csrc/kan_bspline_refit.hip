// Refit of a (grouped) B-spline KAN layer's coefficients to a new knot table -- the numerical half of KANLinear.update_grid
// (models/effkan.py:189-242) -- without the (rows, in, out) tensor the reference fits to.
// The reference evaluates the layer's spline output per edge on the OLD knots, y[m, i, o] = sum_k Bold_k(x[m, i]) w[o, i, k], and
// solves min || Bnew c - y || per (feature, output) by lstsq.  The target is itself a spline in the old basis, so the normal
// equations need two small per-feature matrices and no `out` dimension:
//     N[c][i][j][k] = sum_m Bnew_j(x[m, c*I + i]) * Bnew_k(x[m, c*I + i])        per x slice c (it depends on x and the new knots only)
//     C[g][i][j][k] = sum_m Bnew_j(x[m, c*I + i]) * Bold_k(x[m, c*I + i])        per group g, c = g % x_group_mod
//     w_new[g][i*nb + :][o] = N[c][i]^-1 * C[g][i] * w_old[g][i*nb + :][o]
// Gram kernel: grid (row bands, x_group_mod + groups); block y < x_group_mod forms N of slice y, block x_group_mod + g forms C of
// group g.  As in kan_edge_l1.hip a thread evaluates both basis vectors of one (row, feature) pair into an LDS tile (64 rows x 4
// features per tile; the general Cox-de Boor recursion in a per-thread LDS strip, no private array), then a WAVE owns one feature:
// lane (jl, kl) = (lane / 8, lane % 8) holds the entries (jl + 8a, kl + 8b) of that feature's matrix in registers for a whole row
// band (1 entry for nb <= 8, 9 for nb <= 24) and reads the tile back as broadcasts.  fp32 sums inside a band, COMPENSATED (the
// rounding error of every add and product is carried in a second fp32 register): a constant x column adds the same product in
// every row, and a plain fp32 running sum then drifts by up to rows/2 ulp, all in one direction -- more than the pivot threshold
// that has to recognise exactly that column as rank one.  A band writes its partial matrices to a slab of the workspace and the
// reduce kernel adds the slabs in band order IN FLOAT64: no atomics, bitwise reproducible.  The band split is kan_edge_l1.hip's function of M alone and every block serves one slice or one group, so a
// grouped launch computes for every group exactly what a launch of that group alone computes.
// Solve kernel: one work-group (one wave) per (group, feature): float64 Cholesky of N[c][i] in LDS, then one thread per output
// column forms C w_old and runs the two triangular solves in its LDS strip.  A feature whose matrix has a non-finite entry or a
// Cholesky pivot <= KANVIT_BSPLINE_REFIT_TAU * max_j N[j][j] is flagged in ok[c][i] and nothing is written for it.
// Dead rows and features are masked: their tile entries are zero, so they contribute exactly 0.
// The same kernels serve KANLinear.extend_grid (kanvit_bspline_regrid_*), the fit onto a basis of ANOTHER size:
// every kernel carries the old side's nb / nk (nbo, nko) next to the new side's, C is nb x nbo, and the Gram kernel is instantiated per
// pair of slot counts <NBN, NBO>.  The refit passes nbo = nb and runs exactly the arithmetic it ran with one size.
#include "kan_basis.h"
#include "kanvit_common.h"

namespace {

constexpr int RF_THR = 256;                  // threads per work-group of the Gram kernel = (row, feature) pairs per staged tile
constexpr int RF_FEAT = 4;                   // features per tile: one per wave
constexpr int RF_ROWS = RF_THR / RF_FEAT;    // rows per tile
constexpr int RF_MAX_NB = 24;                // basis functions per feature the register-resident matrix entries cover
constexpr int RF_BAND_ROWS = 256;            // the band split of kan_edge_l1.hip (el_rows_per_band), restated
constexpr int RF_MAX_BANDS = 32;
constexpr int RF_SOLVE_THR = 64;             // one wave: thread r owns row r of the Cholesky factor, then output columns
constexpr int RF_STRIP = 2 * RF_MAX_NB + 1;  // doubles per thread of the solve kernel: w_old[0 .. nbo) | right-hand side / solution

struct GramArgs {
    const float* x;
    const float* kold;     // [groups][old_stride], knots[I][nk] at the front
    const float* knew;     // [x_group_mod][I][nk]
    float* slab;           // [bands][ N: [x_group_mod][I][nb][nb] | C: [groups][I][nb][nbo] ]
    long long M, ldx, old_stride, rows_per_band, n_count, total;      // floats of the N part / of one band's slab
    int I, groups, xmod, nb, order, nk;                               // nb, nk: the NEW basis (the refit's only one)
    int nbo, nko;          // the OLD basis: nb, nk for the refit, old_G and old_G + order + 1 for the regrid
    int blk0;              // first blockIdx.y of this launch (a regrid with unequal slot counts launches N and C blocks apart)
    int uniform_old;       // KANVIT_FLAG_UNIFORM_KNOTS and order 3: closed-form cubic for the OLD basis
    int cbs;               // Cox-de Boor strip floats per thread
};

// B[0 .. NBT) of one (row, feature) pair into LDS (slots past nb and every slot of a dead pair: 0).  Same arithmetic as el_basis of
// kan_edge_l1.hip (half-open order-0 intervals, models/effkan.py:115); `tab` is the knot table [I][nk] of the slice / group.
template <int NBT>
__device__ __forceinline__ void rf_basis(const float* tab, int i, int nk, int ord, int nb, bool uniform, float xv, bool valid, float* B,
                                         float* cb) {
#pragma unroll
    for (int j = 0; j < NBT; ++j) B[j] = 0.0f;
    if (!valid) return;
    if (uniform) {                                         // order 3, uniform knots (caller's flag): 4 non-zero bases
        int j0;
        float bv[4], dv[4];
        if (kv_bspline_uniform(tab, nk, xv, j0, bv, dv, false)) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int idx = j0 - 3 + e;
                if (idx >= 0 && idx < nb) B[idx] = bv[e];
            }
        }
        return;
    }
    const float* kn = tab + (long long)i * nk;             // Cox-de Boor (models/effkan.py:99-132), any order, any knots
    const int n0 = nk - 1;
    for (int j = 0; j < n0; ++j) cb[j] = (xv >= kn[j] && xv < kn[j + 1]) ? 1.0f : 0.0f;
    for (int k = 1; k < ord; ++k)
        for (int j = 0; j < n0 - k; ++j) {
            const float l = __fdividef(xv - kn[j], kn[j + k] - kn[j]);
            const float r = __fdividef(kn[j + k + 1] - xv, kn[j + k + 1] - kn[j + 1]);
            cb[j] = l * cb[j] + r * cb[j + 1];
        }
    if (ord == 0) {
        for (int j = 0; j < nb; ++j) B[j] = cb[j];
    } else {
        for (int j = 0; j < nb; ++j) {
            const float il = __fdividef(1.0f, kn[j + ord] - kn[j]);
            const float ir = __fdividef(1.0f, kn[j + ord + 1] - kn[j + 1]);
            B[j] = (xv - kn[j]) * il * cb[j] + (kn[j + ord + 1] - xv) * ir * cb[j + 1];
        }
    }
}

// LDS: Bn_s[256][NBN] | Bo_s[256][NBO] | cb_s[256][cbs].  NBN / NBO: slots of the new / old basis vector (8 or 24).  With NBN == NBO a
// launch holds N blocks and C blocks (the refit, and a regrid whose sides take the same slot count); an instantiation with
// NBN != NBO serves C blocks only, and the N blocks of that regrid run in the <NBN, NBN> one.
template <int NBN, int NBO>
__global__ __launch_bounds__(RF_THR) void kan_bspline_refit_gram_kernel(const GramArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rf_smem[];
    constexpr int R = NBN / 8, RO = NBO / 8;
    float* Bn_s = rf_smem;
    float* Bo_s = Bn_s + RF_THR * NBN;
    float* cb_s = Bo_s + RF_THR * NBO;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int jl = lane >> 3, kl = lane & 7;
    const int sr = tid >> 2, sf = tid & (RF_FEAT - 1);     // the (row, feature) pair this thread stages
    const int blk = a.blk0 + (int)blockIdx.y;
    const bool is_n = NBN == NBO && blk < a.xmod;          // N of slice blk, else C of group blk - xmod
    const int g = is_n ? 0 : blk - a.xmod;
    const int c = is_n ? blk : g % a.xmod;
    const float* tnew = a.knew + (long long)c * a.I * a.nk;
    const float* told = a.kold + (long long)g * a.old_stride;
    const float* second_s = is_n ? Bn_s : Bo_s;            // N = Bnew^T Bnew: the second factor is the first tile again
    const long long m0 = (long long)blockIdx.x * a.rows_per_band;
    const long long m1 = (m0 + a.rows_per_band < a.M) ? m0 + a.rows_per_band : a.M;
    const int nb2 = is_n ? a.nb : a.nbo;                   // columns of this block's matrix
    float* Bnt = Bn_s + tid * NBN;
    float* Bot = Bo_s + tid * NBO;
    float* cbt = cb_s + tid * a.cbs;

    for (int f0 = 0; f0 < a.I; f0 += RF_FEAT) {
        float acc[R][RO], low[R][RO];
#pragma unroll
        for (int p = 0; p < R; ++p)
#pragma unroll
            for (int q = 0; q < RO; ++q) acc[p][q] = low[p][q] = 0.0f;
        const int si = f0 + sf;
        for (long long mt = m0; mt < m1; mt += RF_ROWS) {
            __syncthreads();                               // the previous tile has been consumed
            const long long m = mt + sr;
            const bool valid = m < m1 && si < a.I;
            const float xv = valid ? a.x[m * a.ldx + (long long)c * a.I + si] : 0.0f;
            rf_basis<NBN>(tnew, si, a.nk, a.order, a.nb, false, xv, valid, Bnt, cbt);
            if (!is_n) rf_basis<NBO>(told, si, a.nko, a.order, a.nbo, a.uniform_old != 0, xv, valid, Bot, cbt);
            __syncthreads();
#pragma unroll 4
            for (int r = 0; r < RF_ROWS; ++r) {            // in row order: the sum of a band is the same in every launch
                const int pr = r * RF_FEAT + wave;
                const float* bn = Bn_s + pr * NBN + jl;
                const float* bs = second_s + pr * NBO + kl;
                float vn[R], vs[RO];
#pragma unroll
                for (int p = 0; p < R; ++p) vn[p] = bn[8 * p];
#pragma unroll
                for (int q = 0; q < RO; ++q) vs[q] = bs[8 * q];
#pragma unroll
                for (int p = 0; p < R; ++p)
#pragma unroll
                    for (int q = 0; q < RO; ++q) {          // acc + low <- acc + low + vn*vs, the rounding errors kept (TwoSum, TwoProduct)
                        const float pr2 = __fmul_rn(vn[p], vs[q]);
                        const float s = __fadd_rn(acc[p][q], pr2);
                        const float bb = __fsub_rn(s, acc[p][q]);
                        low[p][q] += __fadd_rn(__fsub_rn(acc[p][q], __fsub_rn(s, bb)), __fsub_rn(pr2, bb)) + __builtin_fmaf(vn[p], vs[q], -pr2);
                        acc[p][q] = s;
                    }
            }
        }
        const int i = f0 + wave;
        if (i < a.I) {
            float* sp = a.slab + (long long)blockIdx.x * a.total +
                        (is_n ? ((long long)c * a.I + i) * a.nb * a.nb : a.n_count + ((long long)g * a.I + i) * a.nb * a.nbo);
#pragma unroll
            for (int p = 0; p < R; ++p)
#pragma unroll
                for (int q = 0; q < RO; ++q) {
                    const int j = jl + 8 * p, k = kl + 8 * q;
                    if (j < a.nb && k < nb2) sp[j * nb2 + k] = acc[p][q] + low[p][q];
                }
        }
    }
}

// out[e] = slab[0][e] + slab[1][e] + ... in float64, the bands in order; the first n_count elements are N, the rest C
__global__ __launch_bounds__(256) void kan_bspline_refit_reduce_kernel(const float* __restrict__ slab, double* __restrict__ N,
                                                                       double* __restrict__ Cm, long long n_count, long long total,
                                                                       int slabs) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    double s = 0.0;
    for (int b = 0; b < slabs; ++b) s += (double)slab[(long long)b * total + e];
    if (e < n_count) N[e] = s;
    else Cm[e - n_count] = s;
}

// grid (I, groups), one wave.  ok[c][i] was preset to 1; a failing work-group stores 0 (every group of a slice decides alike from
// N[c][i]; a non-finite C[g][i] of one group also clears the slice's flag).
__global__ __launch_bounds__(RF_SOLVE_THR) void kan_bspline_refit_solve_kernel(const double* __restrict__ N, const double* __restrict__ Cm,
                                                                               const float* __restrict__ w_old, float* __restrict__ w_new,
                                                                               unsigned char* __restrict__ ok, int I, int O, int xmod, int nb,
                                                                               int nbo, double tau) {
    __shared__ double L_s[RF_MAX_NB * RF_MAX_NB];
    __shared__ double C_s[RF_MAX_NB * RF_MAX_NB];
    __shared__ double v_s[RF_SOLVE_THR * RF_STRIP];
    __shared__ int bad_s;
    const int i = (int)blockIdx.x, g = (int)blockIdx.y, c = g % xmod, tid = threadIdx.x;
    const double* Np = N + ((long long)c * I + i) * nb * nb;
    const double* Cp = Cm + ((long long)g * I + i) * nb * nbo;            // nb x nbo: w_old has nbo coefficients per feature
    if (tid == 0) bad_s = 0;
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < nb * nb; e += RF_SOLVE_THR) {
        const double n = Np[e];
        L_s[e] = n;
        if (!(__builtin_fabs(n) <= 1.7976931348623157e308)) bad = true;
    }
    for (int e = tid; e < nb * nbo; e += RF_SOLVE_THR) {
        const double cc = Cp[e];
        C_s[e] = cc;
        if (!(__builtin_fabs(cc) <= 1.7976931348623157e308)) bad = true;
    }
    if (bad) bad_s = 1;
    __syncthreads();
    double dmax = 0.0;
    for (int j = 0; j < nb; ++j) dmax = L_s[j * nb + j] > dmax ? L_s[j * nb + j] : dmax;
    const double thr = tau * dmax;
    for (int k = 0; k < nb; ++k) {                         // Cholesky, column by column; thread r owns row r
        if (tid == k) {
            double d = L_s[k * nb + k];
            for (int p = 0; p < k; ++p) d -= L_s[k * nb + p] * L_s[k * nb + p];
            if (!(d > thr)) {                              // a NaN fails too
                bad_s = 1;
                d = 1.0;
            }
            L_s[k * nb + k] = __builtin_sqrt(d);
        }
        __syncthreads();
        if (tid > k && tid < nb) {
            double s = L_s[tid * nb + k];
            for (int p = 0; p < k; ++p) s -= L_s[tid * nb + p] * L_s[k * nb + p];
            L_s[tid * nb + k] = s / L_s[k * nb + k];
        }
        __syncthreads();
    }
    if (bad_s) {
        if (tid == 0) ok[(long long)c * I + i] = 0;
        return;
    }
    double* u = v_s + tid * RF_STRIP;                      // w_old[0 .. nbo) of this column
    double* v = u + nbo;                                   // right-hand side, then the solution
    const long long wb = ((long long)g * I + i) * nb, wbo = ((long long)g * I + i) * nbo;
    for (int o = tid; o < O; o += RF_SOLVE_THR) {
        for (int k = 0; k < nbo; ++k) u[k] = (double)w_old[(wbo + k) * O + o];
        for (int j = 0; j < nb; ++j) {
            double s = 0.0;
            for (int k = 0; k < nbo; ++k) s += C_s[j * nbo + k] * u[k];
            v[j] = s;
        }
        for (int j = 0; j < nb; ++j) {                     // L y = C w
            double s = v[j];
            for (int p = 0; p < j; ++p) s -= L_s[j * nb + p] * v[p];
            v[j] = s / L_s[j * nb + j];
        }
        for (int j = nb - 1; j >= 0; --j) {                // L^T z = y
            double s = v[j];
            for (int p = j + 1; p < nb; ++p) s -= L_s[p * nb + j] * v[p];
            v[j] = s / L_s[j * nb + j];
        }
        for (int j = 0; j < nb; ++j) w_new[(wb + j) * O + o] = (float)v[j];
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// old_G = 0: the refit, one basis size on both sides.  old_G != 0: the regrid; d->G describes the NEW basis, old_G the old one, and
// the messages name the side a size belongs to.
int rf_validate(const kanvit_layer_desc* d, const char* who, int old_G = 0) {
    const bool two = old_G != 0;
    const char* side = two ? "new " : "";
    if (!d) return kv_fail(KANVIT_EINVAL, "%s: null descriptor", who);
    switch (d->family) {
        case KANVIT_BSPLINE: break;
        case KANVIT_LINEAR: return kv_fail(KANVIT_EINVAL, "%s: family LINEAR has no knot table to refit (BSPLINE only)", who);
        case KANVIT_CHEBY: return kv_fail(KANVIT_EINVAL, "%s: family CHEBY has no knot table to refit (BSPLINE only)", who);
        case KANVIT_RBF: return kv_fail(KANVIT_EINVAL, "%s: family RBF is not covered by the spline refit (BSPLINE only)", who);
        case KANVIT_SINE: return kv_fail(KANVIT_EINVAL, "%s: family SINE has no knot table to refit (BSPLINE only)", who);
        case KANVIT_FOURIER: return kv_fail(KANVIT_EINVAL, "%s: family FOURIER has no knot table to refit (BSPLINE only)", who);
        default: return kv_fail(KANVIT_EINVAL, "%s: unknown family %d", who, d->family);
    }
    if (d->flags & KANVIT_FLAG_FUSED_LN) return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_FUSED_LN is an RBF flag", who);
    if (d->flags & KANVIT_FLAG_BF16_MFMA)
        return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_BF16_MFMA is not supported: the refit has no bf16 mode (clear the flag)", who);
    if (d->flags & KANVIT_FLAG_SINE_DFREQ) return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_SINE_DFREQ is a SINE flag", who);
    if (d->has_base || d->base_act)
        return kv_fail(KANVIT_EINVAL, "%s: has_base=%d base_act=%d: the refit takes the spline weights alone (has_base = 0)", who, d->has_base,
                       d->base_act);
    if (d->G < 1) return kv_fail(KANVIT_EINVAL, "%s: %sG=%d", who, side, d->G);
    if (d->G > RF_MAX_NB)
        return kv_fail(KANVIT_EINVAL, "%s: %snb=%d basis functions per feature exceeds the supported %d", who, side, d->G, RF_MAX_NB);
    int nk = d->G + d->spline_order + 1;
    if (d->spline_order < 0 || d->spline_order >= d->G || nk > KV_MAX_KNOTS)
        return kv_fail(KANVIT_EINVAL, "%s: bspline %sG=%d order=%d unsupported (knots %d > %d, or no grid interval)", who, side, d->G,
                       d->spline_order, nk, KV_MAX_KNOTS);
    if (two) {                                             // bparam_stride below is the stride of the OLD knot tables
        if (old_G < 1) return kv_fail(KANVIT_EINVAL, "%s: old G=%d", who, old_G);
        if (old_G > RF_MAX_NB)
            return kv_fail(KANVIT_EINVAL, "%s: old nb=%d basis functions per feature exceeds the supported %d", who, old_G, RF_MAX_NB);
        nk = old_G + d->spline_order + 1;
        if (d->spline_order >= old_G || nk > KV_MAX_KNOTS)
            return kv_fail(KANVIT_EINVAL, "%s: bspline old G=%d order=%d unsupported (knots %d > %d, or no grid interval)", who, old_G,
                           d->spline_order, nk, KV_MAX_KNOTS);
    }
    if (d->groups < 1 || d->x_group_mod < 1 || d->groups % d->x_group_mod != 0)
        return kv_fail(KANVIT_EINVAL, "%s: groups=%d must be a positive multiple of x_group_mod=%d", who, d->groups, d->x_group_mod);
    if ((long long)d->groups + d->x_group_mod > 65535) return kv_fail(KANVIT_EINVAL, "%s: groups=%d + x_group_mod=%d exceeds 65535", who, d->groups, d->x_group_mod);
    if (d->I < 1 || d->O < 1 || d->M < 0) return kv_fail(KANVIT_EINVAL, "%s: bad sizes M=%lld I=%d O=%d", who, (long long)d->M, d->I, d->O);
    if ((long long)d->I * (d->G > old_G ? d->G : old_G) * d->O > 0x7fffffffLL / 4) return kv_fail(KANVIT_EINVAL, "%s: layer too large", who);
    if (d->ldx < (int64_t)d->x_group_mod * d->I) return kv_fail(KANVIT_EINVAL, "%s: ldx=%lld < x_group_mod*I", who, (long long)d->ldx);
    if (d->bparam_stride < (int64_t)d->I * nk) return kv_fail(KANVIT_EINVAL, "%s: bparam_stride too small", who);
    return 0;
}

// kan_edge_l1.hip's el_rows_per_band / el_bands: a function of M alone
long long rf_rows_per_band(long long M) {
    long long nb = (M + RF_BAND_ROWS - 1) / RF_BAND_ROWS;
    if (nb > RF_MAX_BANDS) nb = RF_MAX_BANDS;
    if (nb < 1) nb = 1;
    return ((M + nb - 1) / nb + 63) / 64 * 64;
}
long long rf_bands(long long M) {
    if (M <= 0) return 0;
    const long long rpb = rf_rows_per_band(M);
    return (M + rpb - 1) / rpb;
}

// nbo: basis functions of the old side (d->G for the refit)
long long rf_n_count(const kanvit_layer_desc* d) { return (long long)d->x_group_mod * d->I * d->G * d->G; }
long long rf_c_count(const kanvit_layer_desc* d, int nbo) { return (long long)d->groups * d->I * d->G * nbo; }

bool rf_quiet_ok(const kanvit_layer_desc* d, int old_G = 0) {   // rf_validate without disturbing kanvit_last_error
    char saved[sizeof(g_kanvit_err)];
    __builtin_memcpy(saved, g_kanvit_err, sizeof(saved));
    const bool ok = rf_validate(d, "kanvit_bspline_refit", old_G) == 0;
    __builtin_memcpy(g_kanvit_err, saved, sizeof(saved));
    return ok;
}

size_t rf_workspace(const kanvit_layer_desc* d, int nbo) {
    return (size_t)rf_bands(d->M) * sizeof(float) * (size_t)(rf_n_count(d) + rf_c_count(d, nbo));
}

// blocks [blk0, blk0 + nblk) of the (x_group_mod + groups) N and C blocks
template <int NBN, int NBO>
int rf_launch_gram(GramArgs a, int blk0, int nblk, hipStream_t st) {
    const size_t lds = sizeof(float) * ((size_t)RF_THR * (NBN + NBO) + (size_t)RF_THR * a.cbs);
    const dim3 grid((unsigned)rf_bands(a.M), (unsigned)nblk);
    a.blk0 = blk0;
    if (lds > 64 * 1024) KV_ALLOW_LDS(lds, (kan_bspline_refit_gram_kernel<NBN, NBO>));
    hipLaunchKernelGGL((kan_bspline_refit_gram_kernel<NBN, NBO>), grid, dim3(RF_THR), lds, st, a);
    KV_LAUNCH_CHECK("kan_bspline_refit_gram_kernel");
    return 0;
}

// The Gram and reduce launches of both entry points.  nbo = d->G is the refit.
int rf_gram(const kanvit_layer_desc* d, int nbo, const float* x, const float* old_knots, const float* new_knots, double* N, double* C,
            void* workspace, hipStream_t st) {
    GramArgs a{};
    a.x = x;
    a.kold = old_knots;
    a.knew = new_knots;
    a.slab = (float*)workspace;
    a.M = d->M;
    a.ldx = d->ldx;
    a.old_stride = d->bparam_stride;
    a.rows_per_band = rf_rows_per_band(d->M);
    a.n_count = rf_n_count(d);
    a.total = a.n_count + rf_c_count(d, nbo);
    a.I = d->I;
    a.groups = d->groups;
    a.xmod = d->x_group_mod;
    a.nb = d->G;
    a.order = d->spline_order;
    a.nk = d->G + d->spline_order + 1;
    a.nbo = nbo;
    a.nko = nbo + d->spline_order + 1;
    a.uniform_old = ((d->flags & KANVIT_FLAG_UNIFORM_KNOTS) && d->spline_order == 3) ? 1 : 0;
    a.cbs = ((a.nk > a.nko ? a.nk : a.nko) - 1) | 1;        // odd strip length: the threads' strips start in different LDS banks
    const int all = a.xmod + a.groups;
    const bool n8 = a.nb <= 8, o8 = a.nbo <= 8;
    int rc;
    if (n8 && o8) rc = rf_launch_gram<8, 8>(a, 0, all, st);
    else if (!n8 && !o8) rc = rf_launch_gram<RF_MAX_NB, RF_MAX_NB>(a, 0, all, st);
    else if (n8) {                                          // slot counts differ: the N blocks in the square form, the C blocks apart
        rc = rf_launch_gram<8, 8>(a, 0, a.xmod, st);
        if (!rc) rc = rf_launch_gram<8, RF_MAX_NB>(a, a.xmod, a.groups, st);
    } else {
        rc = rf_launch_gram<RF_MAX_NB, RF_MAX_NB>(a, 0, a.xmod, st);
        if (!rc) rc = rf_launch_gram<RF_MAX_NB, 8>(a, a.xmod, a.groups, st);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(kan_bspline_refit_reduce_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, st, a.slab, N, C, a.n_count,
                       a.total, (int)rf_bands(d->M));
    KV_LAUNCH_CHECK("kan_bspline_refit_reduce_kernel");
    return 0;
}

int rf_solve(const kanvit_layer_desc* d, int nbo, const double* N, const double* C, const float* w_old, float* w_new, unsigned char* ok,
             hipStream_t st, const char* who) {
    const size_t ok_bytes = (size_t)d->x_group_mod * d->I;
    if (d->M == 0) {                                        // nothing was summed: no feature has a fit
        KV_HIP_CHECK(hipMemsetAsync(ok, 0, ok_bytes, st));
        return 0;
    }
    if (!N || !C || !w_old) return kv_fail(KANVIT_EINVAL, "%s: null N/C/w_old", who);
    KV_HIP_CHECK(hipMemsetAsync(ok, 1, ok_bytes, st));
    hipLaunchKernelGGL(kan_bspline_refit_solve_kernel, dim3((unsigned)d->I, (unsigned)d->groups), dim3(RF_SOLVE_THR), 0, st, N, C, w_old, w_new, ok,
                       d->I, d->O, d->x_group_mod, d->G, nbo, (double)KANVIT_BSPLINE_REFIT_TAU);
    KV_LAUNCH_CHECK("kan_bspline_refit_solve_kernel");
    return 0;
}

}  // namespace

extern "C" {

int kanvit_bspline_refit_supported(const kanvit_layer_desc* d) { return rf_quiet_ok(d) ? 1 : 0; }

size_t kanvit_bspline_refit_workspace(const kanvit_layer_desc* d) { return rf_quiet_ok(d) ? rf_workspace(d, d->G) : 0; }

int kanvit_bspline_refit_gram(const kanvit_layer_desc* d, const float* x, const float* old_knots, const float* new_knots, double* N, double* C,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = rf_validate(d, "kanvit_bspline_refit_gram")) return rc;
    if (!N || !C) return kv_fail(KANVIT_EINVAL, "kanvit_bspline_refit_gram: null N/C");
    if (d->M == 0) return 0;                                // no rows: nothing to sum (kanvit_bspline_refit_solve flags every feature)
    if (!x || !old_knots || !new_knots) return kv_fail(KANVIT_EINVAL, "kanvit_bspline_refit_gram: null x/old_knots/new_knots");
    const size_t need = rf_workspace(d, d->G);
    if (!workspace || workspace_bytes < need)
        return kv_fail(KANVIT_ENOMEM, "kanvit_bspline_refit_gram: workspace %zu bytes < required %zu", workspace_bytes, need);
    return rf_gram(d, d->G, x, old_knots, new_knots, N, C, workspace, (hipStream_t)stream);
}

int kanvit_bspline_refit_solve(const kanvit_layer_desc* d, const double* N, const double* C, const float* w_old, float* w_new, unsigned char* ok,
                               void* stream) {
    if (int rc = rf_validate(d, "kanvit_bspline_refit_solve")) return rc;
    if (!w_new || !ok) return kv_fail(KANVIT_EINVAL, "kanvit_bspline_refit_solve: null w_new/ok");
    return rf_solve(d, d->G, N, C, w_old, w_new, ok, (hipStream_t)stream, "kanvit_bspline_refit_solve");
}

// ---- the same fit onto a basis of another size (KANLinear.extend_grid): d->G is the new nb, old_G the old one ----
int kanvit_bspline_regrid_supported(const kanvit_layer_desc* d, int old_G) { return old_G != 0 && rf_quiet_ok(d, old_G) ? 1 : 0; }

size_t kanvit_bspline_regrid_workspace(const kanvit_layer_desc* d, int old_G) {
    return old_G != 0 && rf_quiet_ok(d, old_G) ? rf_workspace(d, old_G) : 0;
}

int kanvit_bspline_regrid_gram(const kanvit_layer_desc* d, int old_G, const float* x, const float* old_knots, const float* new_knots, double* N,
                               double* C, void* workspace, size_t workspace_bytes, void* stream) {
    if (old_G == 0) return kv_fail(KANVIT_EINVAL, "kanvit_bspline_regrid_gram: old G=0");
    if (int rc = rf_validate(d, "kanvit_bspline_regrid_gram", old_G)) return rc;
    if (!N || !C) return kv_fail(KANVIT_EINVAL, "kanvit_bspline_regrid_gram: null N/C");
    if (d->M == 0) return 0;
    if (!x || !old_knots || !new_knots) return kv_fail(KANVIT_EINVAL, "kanvit_bspline_regrid_gram: null x/old_knots/new_knots");
    const size_t need = rf_workspace(d, old_G);
    if (!workspace || workspace_bytes < need)
        return kv_fail(KANVIT_ENOMEM, "kanvit_bspline_regrid_gram: workspace %zu bytes < required %zu", workspace_bytes, need);
    return rf_gram(d, old_G, x, old_knots, new_knots, N, C, workspace, (hipStream_t)stream);
}

int kanvit_bspline_regrid_solve(const kanvit_layer_desc* d, int old_G, const double* N, const double* C, const float* w_old, float* w_new,
                                unsigned char* ok, void* stream) {
    if (old_G == 0) return kv_fail(KANVIT_EINVAL, "kanvit_bspline_regrid_solve: old G=0");
    if (int rc = rf_validate(d, "kanvit_bspline_regrid_solve", old_G)) return rc;
    if (!w_new || !ok) return kv_fail(KANVIT_EINVAL, "kanvit_bspline_regrid_solve: null w_new/ok");
    return rf_solve(d, old_G, N, C, w_old, w_new, ok, (hipStream_t)stream, "kanvit_bspline_regrid_solve");
}

}  // extern "C"
