// Per-edge mean absolute activation of a (grouped) KAN layer -- the quantity the KAN paper's regulariser is built from -- and
// its gradients, without the (rows, in, out) activation tensor:
//     phi[m, g, i, o] = sum_j Phi_j(x[m, (g % x_group_mod)*I + i]) * w[g][i*GP + j][o]
//     A[g][i][o]      = (1/M) sum_m |phi[m, g, i, o]|
// backward, given gA = d loss / d A:  s = sign(phi) * gA / M  (sign(0) = 0, as torch.abs differentiates),
//     dw[g][i*GP + j][o] = sum_m Phi_j(x) * s[m, i, o]
//     dx[m, c*I + i]     = sum_{g % x_group_mod == c} sum_j Phi_j'(x) * sum_o s[m, i, o] * w[g][i*GP + j][o]
// Kernel form: the contraction per (row, feature) is K = GP long (5 .. 10 for the layers the models build), so it runs on the
// VECTOR pipe.  A thread owns one edge (i, o): its GP weights live in registers for a whole row band, the basis values of a
// tile of (row, feature) pairs are evaluated once into LDS (one pair per thread) and read back as wave broadcasts, and the
// sums over the rows never leave the thread: GP FMAs + one add with an |.| source modifier per (row, edge) forward, 2 GP FMAs
// + a select backward (3 GP and a lane-group reduction over the output columns when dx is wanted).  The row range is cut
// into bands; a band writes its partial sums to a slab of the workspace and a second kernel adds the slabs in band order:
// no atomics, bitwise reproducible.  The band split depends on M alone, so a grouped launch computes for every group exactly
// what a launch of that group alone computes.
// Dead rows, features and columns are masked: their basis tile entries / weights are zero, so they contribute exactly 0.
#include "kan_basis.h"
#include "kanvit_common.h"

namespace {

constexpr int EL_THR = 256;          // threads per work-group = (row, feature) pairs per staged tile
constexpr int EL_MAX_GP = 24;        // generated columns per feature the register-resident weights cover
constexpr int EL_BAND_ROWS = 256;    // a band is at least this many rows ...
constexpr int EL_MAX_BANDS = 32;     // ... and there are at most this many (workspace = bands x result)

struct EdgeArgs {
    const float* x;
    const float* w;
    const float* bp;
    const float* ga;       // backward: d loss / d A [groups][I][O]
    float* slab;           // forward: [bands][groups][I][O]; backward: [bands][groups][I*GP][O]
    float* dx;             // backward, may be NULL
    long long M, ldx, bp_stride, rows_per_band, xb_off;
    int I, O, groups, xmod, G, GP, order, nk, has_base, flags, base_act;
    int ot_shift;          // a wave covers OT = 1 << ot_shift output columns (16, 32 or 64) of 64 / OT features
    int cbs;               // Cox-de Boor scratch floats per thread (general B-spline path), 0 otherwise
    float inv_m;
};

__device__ __forceinline__ BasisArgs el_basis_args(const EdgeArgs& a, int g) {
    BasisArgs b;
    b.G = a.G;
    b.GP = a.GP;
    b.order = a.order;
    b.nk = a.nk;
    b.has_base = a.has_base;
    b.inv_h = 0.0f;
    b.bp = a.bp ? a.bp + (long long)g * a.bp_stride : nullptr;
    b.uniform = (a.flags & KANVIT_FLAG_UNIFORM_KNOTS) && a.order == 3;
    b.act = a.base_act;
    return b;
}

// Values B[0 .. GPT) and, if der, derivatives D[0 .. GPT) of one (row, feature) pair into LDS (slots past GP and every slot
// of a dead pair: 0).  Same arithmetic as basis_fwd / basis_bwd of kan_basis.h; the general Cox-de Boor recursion runs in the
// thread's LDS strip cb[0 .. nk-1) instead of a private array (no scratch).  RBF: D holds d/du of the Gaussians and 0 in the
// base slot; the base column reads xb and its derivative is returned in dbase.
template <int FAM, int ACT, int GPT>
__device__ __forceinline__ void el_basis(const BasisArgs& b, float inv_h, float xv, float xb, int i, bool valid, bool der, float* B,
                                         float* D, float* cb, float& dbase) {
#pragma unroll
    for (int j = 0; j < GPT; ++j) B[j] = 0.0f;
    if (der) {
#pragma unroll
        for (int j = 0; j < GPT; ++j) D[j] = 0.0f;
    }
    dbase = 0.0f;
    if (!valid) return;
    if constexpr (FAM == KV_CHEBY) {
        const float t = kv_tanh(xv), sech2 = 1.0f - t * t;
        float p0 = 1.0f, p1 = t, u0 = 1.0f, u1 = 2.0f * t;      // T_{g-2}, T_{g-1}; U_{g-2}, U_{g-1}: dT_g/dt = g U_{g-1}
        B[0] = 1.0f;
        if (b.G > 1) {
            B[1] = t;
            if (der) D[1] = sech2;
        }
        for (int g = 2; g < b.G; ++g) {
            const float p2 = 2.0f * t * p1 - p0;
            B[g] = p2;
            if (der) D[g] = (float)g * u1 * sech2;
            const float u2 = 2.0f * t * u1 - u0;
            p0 = p1;
            p1 = p2;
            u0 = u1;
            u1 = u2;
        }
    } else if constexpr (FAM == KV_BSPLINE) {
        if (b.uniform) {                                   // order 3, uniform knots (host-checked): 4 non-zero bases
            int j0;
            float bv[4], dv[4];
            if (kv_bspline_uniform(b.bp, b.nk, xv, j0, bv, dv, der)) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int idx = j0 - 3 + e;
                    if (idx >= 0 && idx < b.G) {
                        B[idx] = bv[e];
                        if (der) D[idx] = dv[e];
                    }
                }
            }
        } else {                                           // Cox-de Boor (models/effkan.py:99-132), any order, any knots
            const float* kn = b.bp + (long long)i * b.nk;
            const int nb = b.nk - 1, ord = b.order;
            for (int j = 0; j < nb; ++j) cb[j] = (xv >= kn[j] && xv < kn[j + 1]) ? 1.0f : 0.0f;
            for (int k = 1; k < ord; ++k)
                for (int j = 0; j < nb - k; ++j) {
                    const float l = __fdividef(xv - kn[j], kn[j + k] - kn[j]);
                    const float r = __fdividef(kn[j + k + 1] - xv, kn[j + k + 1] - kn[j + 1]);
                    cb[j] = l * cb[j] + r * cb[j + 1];
                }
            if (ord == 0) {
                for (int j = 0; j < b.G; ++j) B[j] = cb[j];
            } else {
                for (int j = 0; j < b.G; ++j) {
                    const float il = __fdividef(1.0f, kn[j + ord] - kn[j]);
                    const float ir = __fdividef(1.0f, kn[j + ord + 1] - kn[j + 1]);
                    const float c0 = cb[j], c1 = cb[j + 1];
                    B[j] = (xv - kn[j]) * il * c0 + (kn[j + ord + 1] - xv) * ir * c1;
                    if (der) D[j] = (float)ord * (c0 * il - c1 * ir);
                }
            }
        }
        if (b.has_base) {
            B[b.G] = kv_base<ACT>(xv, b.act);
            if (der) D[b.G] = kv_dbase<ACT>(xv, b.act);
        }
    } else {                                               // RBF (models/fastkan.py:29-30)
        for (int g = 0; g < b.G; ++g) {
            const float d = (xv - b.bp[g]) * inv_h;
            const float e = __expf(-d * d);
            B[g] = e;
            if (der) D[g] = e * (-2.0f * d * inv_h);
        }
        if (b.has_base) {
            B[b.G] = kv_base<ACT>(xb, b.act);
            if (der) dbase = kv_dbase<ACT>(xb, b.act);
        }
    }
}

// Forward: grid (bands, groups).  Backward: grid (bands, x_group_mod); the work-group walks the groups that read its x slice,
// so the sums of dx over those groups (and over column chunks) are its own read-modify-writes, in a fixed order.
// LDS: B_s[256][GPT] | D_s[256][GPT] (backward) | q_s[256] | qb_s[256] | db_s[256] (backward) | cb_s[256][cbs]
template <int FAM, int ACT, int GPT, bool BWD>
__device__ __forceinline__ void el_body(const EdgeArgs& a, float inv_h) {
    extern __shared__ __attribute__((aligned(16))) float el_smem[];
    float* B_s = el_smem;
    float* D_s = B_s + EL_THR * GPT;
    float* q_s = D_s + (BWD ? EL_THR * GPT : 0);
    float* qb_s = q_s + (BWD ? EL_THR : 0);
    float* db_s = qb_s + (BWD ? EL_THR : 0);
    float* cb_s = db_s + (BWD ? EL_THR : 0);

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int OT = 1 << a.ot_shift, FW = 64 >> a.ot_shift, FP = 4 * FW, RT = EL_THR / FP;
    const int fp_shift = 8 - a.ot_shift;                   // FP = 256 / OT
    const int ol = lane & (OT - 1), fi = wave * FW + (lane >> a.ot_shift);
    const int sr = tid >> fp_shift, sf = tid & (FP - 1);   // the (row, feature) pair this thread stages
    const long long m0 = (long long)blockIdx.x * a.rows_per_band;
    const long long m1 = (m0 + a.rows_per_band < a.M) ? m0 + a.rows_per_band : a.M;
    const int ns = BWD ? a.groups / a.xmod : 1;
    const int c = BWD ? (int)blockIdx.y : (int)blockIdx.y % a.xmod;
    const bool want_dx = BWD && a.dx != nullptr;
    const bool rbf_base = (FAM == KV_RBF) && a.has_base;
    float* Bt = B_s + tid * GPT;
    float* Dt = D_s + tid * GPT;
    float* cbt = cb_s + tid * a.cbs;

    for (int p = 0; p < ns; ++p) {
        const int g = BWD ? p * a.xmod + c : (int)blockIdx.y;
        const BasisArgs b = el_basis_args(a, g);
        for (int oc = 0; oc < a.O; oc += OT) {
            const int o = oc + ol;
            for (int f0 = 0; f0 < a.I; f0 += FP) {
                const int i = f0 + fi;
                const bool act = o < a.O && i < a.I;
                float wr[GPT], dwr[GPT];
                const float* wp = a.w + (((long long)g * a.I + i) * a.GP) * a.O + o;
#pragma unroll
                for (int j = 0; j < GPT; ++j) {
                    wr[j] = (act && j < a.GP) ? wp[(long long)j * a.O] : 0.0f;
                    dwr[j] = 0.0f;
                }
                const float wbase = (rbf_base && act) ? wp[(long long)a.G * a.O] : 0.0f;
                const float ga = (BWD && act) ? a.ga[((long long)g * a.I + i) * a.O + o] * a.inv_m : 0.0f;
                float acc = 0.0f;
                const int si = f0 + sf;
                for (long long mt = m0; mt < m1; mt += RT) {
                    __syncthreads();                       // the previous tile has been consumed
                    const long long m = mt + sr;
                    const bool valid = m < m1 && si < a.I;
                    const long long xo = m * a.ldx + (long long)c * a.I + si;
                    const float xv = valid ? a.x[xo] : 0.0f;
                    const float xb = (valid && rbf_base) ? a.x[xo + a.xb_off] : xv;
                    float dbase;
                    el_basis<FAM, ACT, GPT>(b, inv_h, xv, xb, si, valid, want_dx, Bt, Dt, cbt, dbase);
                    if (want_dx && rbf_base) db_s[tid] = dbase;
                    __syncthreads();
                    for (int r = 0; r < RT; ++r) {
                        const int pr = r * FP + fi;
                        const float* Br = B_s + pr * GPT;
                        float phi = 0.0f;
#pragma unroll
                        for (int j = 0; j < GPT; ++j) phi = __builtin_fmaf(Br[j], wr[j], phi);
                        if constexpr (!BWD) {
                            acc += __builtin_fabsf(phi);
                        } else {
                            const float s = phi > 0.0f ? ga : (phi < 0.0f ? -ga : 0.0f);
#pragma unroll
                            for (int j = 0; j < GPT; ++j) dwr[j] = __builtin_fmaf(Br[j], s, dwr[j]);
                            if (want_dx) {
                                const float* Dr = D_s + pr * GPT;
                                float dphi = 0.0f;
#pragma unroll
                                for (int j = 0; j < GPT; ++j) dphi = __builtin_fmaf(Dr[j], wr[j], dphi);
                                float q = s * dphi;
                                float qb = rbf_base ? s * wbase * db_s[pr] : 0.0f;
                                for (int off = OT >> 1; off > 0; off >>= 1) {      // sum over the output columns of this feature
                                    q += __shfl_xor(q, off);
                                    if (FAM == KV_RBF) qb += __shfl_xor(qb, off);
                                }
                                if (ol == 0) {
                                    q_s[pr] = q;
                                    if (FAM == KV_RBF) qb_s[pr] = qb;
                                }
                            }
                        }
                    }
                    if (want_dx) {
                        __syncthreads();
                        if (valid) {                       // this thread owns dx of its staged pair for the whole launch
                            const bool first = p == 0 && oc == 0;
                            float* dp = a.dx + xo;
                            const float v = q_s[tid];
                            *dp = first ? v : *dp + v;
                            if (rbf_base) {
                                float* db = dp + a.xb_off;
                                const float vb = qb_s[tid];
                                *db = (first && a.xb_off != 0) ? vb : *db + vb;
                            }
                        }
                    }
                }
                if (act) {
                    if constexpr (!BWD) {
                        a.slab[(((long long)blockIdx.x * a.groups + g) * a.I + i) * a.O + o] = acc;
                    } else {
                        float* sp = a.slab + ((((long long)blockIdx.x * a.groups + g) * a.I + i) * a.GP) * a.O + o;
#pragma unroll
                        for (int j = 0; j < GPT; ++j)
                            if (j < a.GP) sp[(long long)j * a.O] = dwr[j];
                    }
                }
            }
        }
    }
}

template <int FAM, int ACT, int GPT>
__global__ __launch_bounds__(EL_THR) void kan_edge_l1_fwd_kernel(const EdgeArgs a, float inv_h) {
    el_body<FAM, ACT, GPT, false>(a, inv_h);
}
template <int FAM, int ACT, int GPT>
__global__ __launch_bounds__(EL_THR) void kan_edge_l1_bwd_kernel(const EdgeArgs a, float inv_h) {
    el_body<FAM, ACT, GPT, true>(a, inv_h);
}

// out[e] = scale * (slab[0][e] + slab[1][e] + ...): the bands in order
__global__ __launch_bounds__(256) void kan_edge_l1_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out, long long total,
                                                                 int slabs, float scale) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = 0.0f;
    for (int b = 0; b < slabs; ++b) s += slab[(long long)b * total + e];
    out[e] = s * scale;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int el_gp(const kanvit_layer_desc* d) {
    switch (d->family) {
        case KANVIT_CHEBY: return d->G;
        case KANVIT_BSPLINE:
        case KANVIT_RBF: return d->G + (d->has_base ? 1 : 0);
        default: return -1;
    }
}

int el_validate(const kanvit_layer_desc* d, const char* who) {
    if (!d) return kv_fail(KANVIT_EINVAL, "%s: null descriptor", who);
    switch (d->family) {
        case KANVIT_CHEBY:
        case KANVIT_BSPLINE:
        case KANVIT_RBF: break;
        case KANVIT_LINEAR: return kv_fail(KANVIT_EINVAL, "%s: family LINEAR has no edge-L1 statistic (BSPLINE, CHEBY and RBF do)", who);
        case KANVIT_SINE: return kv_fail(KANVIT_EINVAL, "%s: family SINE is not covered by the edge-L1 statistic (BSPLINE, CHEBY and RBF are)", who);
        case KANVIT_FOURIER: return kv_fail(KANVIT_EINVAL, "%s: family FOURIER is not covered by the edge-L1 statistic (BSPLINE, CHEBY and RBF are)", who);
        default: return kv_fail(KANVIT_EINVAL, "%s: unknown family %d", who, d->family);
    }
    if (d->flags & KANVIT_FLAG_FUSED_LN)
        return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_FUSED_LN is not supported (pass the LayerNorm'ed input)", who);
    if (d->flags & KANVIT_FLAG_BF16_MFMA)
        return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_BF16_MFMA is not supported: the statistic has no bf16 mode (clear the flag)", who);
    if (d->flags & KANVIT_FLAG_SINE_DFREQ) return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_SINE_DFREQ is a SINE flag", who);
    if (d->G < 1) return kv_fail(KANVIT_EINVAL, "%s: G=%d", who, d->G);
    const int gp = el_gp(d);
    if (gp > EL_MAX_GP)
        return kv_fail(KANVIT_EINVAL, "%s: %d generated columns per feature exceeds the supported %d", who, gp, EL_MAX_GP);
    if (d->groups < 1 || d->x_group_mod < 1 || d->groups % d->x_group_mod != 0)
        return kv_fail(KANVIT_EINVAL, "%s: groups=%d must be a positive multiple of x_group_mod=%d", who, d->groups, d->x_group_mod);
    if (d->groups > 65535) return kv_fail(KANVIT_EINVAL, "%s: groups=%d exceeds 65535", who, d->groups);
    if (d->I < 1 || d->O < 1 || d->M < 0) return kv_fail(KANVIT_EINVAL, "%s: bad sizes M=%lld I=%d O=%d", who, (long long)d->M, d->I, d->O);
    if ((long long)d->I * gp * d->O > 0x7fffffffLL / 4) return kv_fail(KANVIT_EINVAL, "%s: layer too large", who);
    const bool two_inputs = d->family == KANVIT_RBF && d->has_base;
    // the raw-input block may coincide with the spline block (ldu = 0) or lie clear of it; a partial overlap would make two
    // work-groups of the backward own one dx element
    if (two_inputs && d->ldu != 0 && d->ldu < (int64_t)d->x_group_mod * d->I)
        return kv_fail(KANVIT_EINVAL, "%s: ldu=%lld must be 0 or at least x_group_mod*I=%lld", who, (long long)d->ldu,
                       (long long)d->x_group_mod * d->I);
    if (d->ldx < (int64_t)d->x_group_mod * d->I + (two_inputs ? d->ldu : 0))
        return kv_fail(KANVIT_EINVAL, "%s: ldx=%lld < x_group_mod*I%s", who, (long long)d->ldx, two_inputs ? " + ldu" : "");
    if (d->family == KANVIT_BSPLINE) {
        const int nk = d->G + d->spline_order + 1;
        if (d->spline_order < 0 || nk > KV_MAX_KNOTS)
            return kv_fail(KANVIT_EINVAL, "%s: bspline G=%d order=%d unsupported (knots %d > %d)", who, d->G, d->spline_order, nk, KV_MAX_KNOTS);
        if (d->bparam_stride < (int64_t)d->I * nk) return kv_fail(KANVIT_EINVAL, "%s: bparam_stride too small", who);
    }
    if (d->family == KANVIT_RBF && d->bparam_stride < d->G) return kv_fail(KANVIT_EINVAL, "%s: bparam_stride too small", who);
    if (d->base_act < KANVIT_BASE_SILU || d->base_act > KANVIT_BASE_IDENTITY)
        return kv_fail(KANVIT_EINVAL, "%s: unknown base activation %d (KANVIT_BASE_SILU .. KANVIT_BASE_IDENTITY)", who, d->base_act);
    if (d->base_act != KANVIT_BASE_SILU && (d->family == KANVIT_CHEBY || !d->has_base))
        return kv_fail(KANVIT_EINVAL, "%s: base activation %d set for a layer without a base column", who, d->base_act);
    return 0;
}

// the band split is a function of M alone (a group's result does not depend on what else is in the launch)
long long el_rows_per_band(long long M) {
    long long nb = (M + EL_BAND_ROWS - 1) / EL_BAND_ROWS;
    if (nb > EL_MAX_BANDS) nb = EL_MAX_BANDS;
    if (nb < 1) nb = 1;
    return ((M + nb - 1) / nb + 63) / 64 * 64;
}
long long el_bands(long long M) {
    if (M <= 0) return 0;
    const long long rpb = el_rows_per_band(M);
    return (M + rpb - 1) / rpb;
}

EdgeArgs el_args(const kanvit_layer_desc* d) {
    EdgeArgs a{};
    a.M = d->M;
    a.ldx = d->ldx;
    a.bp_stride = d->bparam_stride;
    a.rows_per_band = el_rows_per_band(d->M);
    a.xb_off = (d->family == KANVIT_RBF && d->has_base) ? d->ldu : 0;
    a.I = d->I;
    a.O = d->O;
    a.groups = d->groups;
    a.xmod = d->x_group_mod;
    a.G = d->G;
    a.GP = el_gp(d);
    a.order = d->spline_order;
    a.nk = d->G + d->spline_order + 1;
    a.has_base = d->has_base ? 1 : 0;
    a.flags = d->flags;
    a.base_act = d->base_act;
    a.ot_shift = d->O <= 16 ? 4 : (d->O <= 32 ? 5 : 6);
    const bool general = d->family == KANVIT_BSPLINE && !((d->flags & KANVIT_FLAG_UNIFORM_KNOTS) && d->spline_order == 3);
    a.cbs = general ? ((a.nk - 1) | 1) : 0;                // odd strip length: the threads' strips start in different LDS banks
    a.inv_m = d->M > 0 ? 1.0f / (float)d->M : 0.0f;
    return a;
}

template <int FAM, int ACT, int GPT>
int el_launch_t(const EdgeArgs& a, float inv_h, bool bwd, hipStream_t st) {
    const size_t lds = sizeof(float) * ((size_t)EL_THR * GPT * (bwd ? 2 : 1) + (bwd ? 3 * EL_THR : 0) + (size_t)EL_THR * a.cbs);
    const dim3 grid((unsigned)el_bands(a.M), (unsigned)(bwd ? a.xmod : a.groups));
    if (bwd) {
        if (lds > 64 * 1024) KV_ALLOW_LDS(lds, (kan_edge_l1_bwd_kernel<FAM, ACT, GPT>));
        hipLaunchKernelGGL((kan_edge_l1_bwd_kernel<FAM, ACT, GPT>), grid, dim3(EL_THR), lds, st, a, inv_h);
        KV_LAUNCH_CHECK("kan_edge_l1_bwd_kernel");
    } else {
        if (lds > 64 * 1024) KV_ALLOW_LDS(lds, (kan_edge_l1_fwd_kernel<FAM, ACT, GPT>));
        hipLaunchKernelGGL((kan_edge_l1_fwd_kernel<FAM, ACT, GPT>), grid, dim3(EL_THR), lds, st, a, inv_h);
        KV_LAUNCH_CHECK("kan_edge_l1_fwd_kernel");
    }
    return 0;
}

template <int FAM, int ACT>
int el_launch_gp(const EdgeArgs& a, float inv_h, bool bwd, hipStream_t st) {
    if (a.GP <= 8) return el_launch_t<FAM, ACT, 8>(a, inv_h, bwd, st);
    if (a.GP <= 12) return el_launch_t<FAM, ACT, 12>(a, inv_h, bwd, st);
    return el_launch_t<FAM, ACT, EL_MAX_GP>(a, inv_h, bwd, st);
}

int el_launch(int family, const EdgeArgs& a, float inv_h, bool bwd, hipStream_t st) {
    switch (family) {
        case KANVIT_CHEBY: return el_launch_gp<KV_CHEBY, KV_ACT_SILU>(a, inv_h, bwd, st);
        case KANVIT_BSPLINE:
            return a.base_act ? el_launch_gp<KV_BSPLINE, KV_ACT_DYN>(a, inv_h, bwd, st) : el_launch_gp<KV_BSPLINE, KV_ACT_SILU>(a, inv_h, bwd, st);
        case KANVIT_RBF:
            return a.base_act ? el_launch_gp<KV_RBF, KV_ACT_DYN>(a, inv_h, bwd, st) : el_launch_gp<KV_RBF, KV_ACT_SILU>(a, inv_h, bwd, st);
        default: return kv_fail(KANVIT_EINVAL, "internal: edge-L1 dispatch (family %d)", family);
    }
}

int el_reduce(const float* slab, float* out, long long total, int slabs, float scale, hipStream_t st) {
    hipLaunchKernelGGL(kan_edge_l1_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, slab, out, total, slabs, scale);
    KV_LAUNCH_CHECK("kan_edge_l1_reduce_kernel");
    return 0;
}

size_t el_slab_bytes(const kanvit_layer_desc* d, bool bwd) {
    return sizeof(float) * (size_t)d->groups * d->I * (bwd ? (size_t)el_gp(d) : 1) * d->O;
}

bool el_quiet_ok(const kanvit_layer_desc* d) {              // el_validate without disturbing kanvit_last_error
    char saved[sizeof(g_kanvit_err)];
    __builtin_memcpy(saved, g_kanvit_err, sizeof(saved));
    const bool ok = el_validate(d, "kanvit_edge_l1") == 0;
    __builtin_memcpy(g_kanvit_err, saved, sizeof(saved));
    return ok;
}

}  // namespace

extern "C" {

int kanvit_edge_l1_supported(const kanvit_layer_desc* d) { return el_quiet_ok(d) ? 1 : 0; }

int64_t kanvit_edge_l1_row_bands(const kanvit_layer_desc* d) { return el_quiet_ok(d) ? el_bands(d->M) : 0; }

size_t kanvit_edge_l1_fwd_workspace(const kanvit_layer_desc* d) {
    return el_quiet_ok(d) ? (size_t)el_bands(d->M) * el_slab_bytes(d, false) : 0;
}

size_t kanvit_edge_l1_bwd_workspace(const kanvit_layer_desc* d) {
    return el_quiet_ok(d) ? (size_t)el_bands(d->M) * el_slab_bytes(d, true) : 0;
}

int kanvit_edge_l1_fwd(const kanvit_layer_desc* d, const float* x, const float* w, const float* bparams, float* A, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (int rc = el_validate(d, "kanvit_edge_l1_fwd")) return rc;
    if (!A) return kv_fail(KANVIT_EINVAL, "kanvit_edge_l1_fwd: null A");
    hipStream_t st = (hipStream_t)stream;
    if (d->M == 0) {
        KV_HIP_CHECK(hipMemsetAsync(A, 0, el_slab_bytes(d, false), st));
        return 0;
    }
    if (!x || !w) return kv_fail(KANVIT_EINVAL, "kanvit_edge_l1_fwd: null x/w");
    if (d->family != KANVIT_CHEBY && !bparams) return kv_fail(KANVIT_EINVAL, "kanvit_edge_l1_fwd: family %d needs bparams", d->family);
    const size_t need = kanvit_edge_l1_fwd_workspace(d);
    if (!workspace || workspace_bytes < need)
        return kv_fail(KANVIT_ENOMEM, "kanvit_edge_l1_fwd: workspace %zu bytes < required %zu", workspace_bytes, need);
    EdgeArgs a = el_args(d);
    a.x = x;
    a.w = w;
    a.bp = bparams;
    a.slab = (float*)workspace;
    if (int rc = el_launch(d->family, a, d->rbf_inv_h, false, st)) return rc;
    return el_reduce(a.slab, A, (long long)d->groups * d->I * d->O, (int)el_bands(d->M), a.inv_m, st);
}

int kanvit_edge_l1_bwd(const kanvit_layer_desc* d, const float* x, const float* w, const float* bparams, const float* gA, float* dw,
                       float* dx, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = el_validate(d, "kanvit_edge_l1_bwd")) return rc;
    if (!dw) return kv_fail(KANVIT_EINVAL, "kanvit_edge_l1_bwd: null dw");
    hipStream_t st = (hipStream_t)stream;
    if (d->M == 0) {                                        // no rows: dw is exactly zero and dx has no element
        KV_HIP_CHECK(hipMemsetAsync(dw, 0, el_slab_bytes(d, true), st));
        return 0;
    }
    if (!x || !w || !gA) return kv_fail(KANVIT_EINVAL, "kanvit_edge_l1_bwd: null x/w/gA");
    if (d->family != KANVIT_CHEBY && !bparams) return kv_fail(KANVIT_EINVAL, "kanvit_edge_l1_bwd: family %d needs bparams", d->family);
    const size_t need = kanvit_edge_l1_bwd_workspace(d);
    if (!workspace || workspace_bytes < need)
        return kv_fail(KANVIT_ENOMEM, "kanvit_edge_l1_bwd: workspace %zu bytes < required %zu", workspace_bytes, need);
    EdgeArgs a = el_args(d);
    a.x = x;
    a.w = w;
    a.bp = bparams;
    a.ga = gA;
    a.dx = dx;
    a.slab = (float*)workspace;
    if (int rc = el_launch(d->family, a, d->rbf_inv_h, true, st)) return rc;
    return el_reduce(a.slab, dw, (long long)d->groups * d->I * el_gp(d) * d->O, (int)el_bands(d->M), 1.0f, st);
}

}  // extern "C"
