// General attention core: independent query / key lengths and a boolean attend-mask (exact fp32).
//
// FlashAttentionFunction (utils.py:134-295) tiles over independent q / k lengths (utils.py:150-160, cross-attention through
// FlashAttention(context=...), attention.py:59-109) and takes a mask broadcastable to [b, h, q_len, k_len] (a [b, k_len]
// key-padding mask is viewed as [b, 1, 1, k_len], utils.py:156-157).  `causal` (key j > query i is dead, utils.py:178-190) is taken
// for k_len <= q_len only: with k_len > q_len the reference shifts the diagonal the wrong way (utils.py:169 SUBTRACTS qk_len_diff:
// query i sees keys j <= i - (k_len - q_len)), the first k_len - q_len queries have no visible key and its answer for them depends
// on the bucket sizes -- refused here (KANVIT_EINVAL) instead of imitated.  The ViT path never uses either (attention.hip's kernels: one length, no
// mask); these kernels cover the rest of the function's domain with the same tile orientation as attention.hip's first form:
//   forward       work-group = eight 32-query tiles of one (batch, head), one per wave; the keys are swept in LDS chunks of 128 rows
//                 (K, V images [128][KS]); S^T = K.Q^T with the key index in the accumulator register index -> softmax over the
//                 chunk in registers, running (max, sum) across chunks (utils.py:199-221) -> O^T = V^T.P^T from registers
//   backward      rowsum(dO*O) (attn_x_delta_kernel), then a key-stationary kernel (a wave owns a key tile: dK^T, dV^T in
//                 accumulators; Q, dO swept in LDS chunks) and a query-stationary one (dQ^T in accumulators; K, V swept in
//                 chunks): no atomics, bitwise reproducible
// ANY sequence length (the swept operand never has to fit the LDS): ops.attention also routes self-attention heads that do not fit
// the ViT kernels of attention.hip (N > 224 at D = 64, e.g. ViT-B/16 at 384 x 384: N = 577) here.
// A position is dead when key >= k_len, or causal and key > query, or the mask says so.  A query whose keys are ALL
// dead gets o = 0, lse = -FLT_MAX and zero gradients (the reference's clamp(min=EPSILON) row sum gives the same o = 0 and
// lse = log(1e-10) - FLT_MAX for a fully MASKED row).
// Head sizes: DT = ceil(D / 32) column tiles of 32 (x_load_tile zero-fills the columns >= D).  DT = 1, 2 (D <= 64) run eight waves,
// two per SIMD, each with its own 32-row staging tile in LDS.  DT = 3, 4 (D <= 96, <= 128) run four waves, one per SIMD, so that a
// lane may hold up to 512 registers (the dK/dV kernel keeps 4 x 16*DT values of K, V, dK, dV), and alias the staging tiles onto the
// chunk buffers (they are used only before the sweep and after it, across a barrier) to fit the 160 KiB of LDS at 128-row chunks.
// Limits (host-checked): D even and <= KANVIT_ATTN_X_MAX_D (128).
#include "kanvit_common.h"

#include <float.h>
#include <initializer_list>

namespace {

// Work-group shape of the DT form: 8 waves, two per SIMD (one LDS chunk of the swept operand serves eight 32-row tiles) up to D = 64;
// 4 waves, one per SIMD, with each wave's 32-row staging tile aliased onto the chunk buffers for D > 64.
template <int DT>
struct XShape {
    static constexpr int THR = DT <= 2 ? 512 : 256;
    static constexpr int W = THR / 64;
    static constexpr bool ALIAS = DT > 2;
};
constexpr float LOG2E_X = 1.4426950408889634f;

struct AttnXArgs {
    const float* q;
    const float* k;
    const float* v;
    const float* o;
    const float* lse_in;
    const float* d_o;
    const float* delta_in;
    const unsigned char* mask;      // nonzero = attend; element (b, h, i, j) at mask[b*msb + h*msh + i*msq + j*msk] (0 strides broadcast)
    float* out;
    float* lse;
    float* dq;
    float* dk;
    float* dv;
    float* delta;
    long long msb, msh, msq, msk;
    long long qsb, qsh, qsn, ksb, ksh, ksn, vsb, vsh, vsn, osb, osh, osn;
    int B, H, Nq, Nk, D, causal, nqt, nkt;
    int vec;          // rows are 16-byte aligned pieces (D % 4 == 0, strides % 4 == 0, aligned bases): tile fills use 16-byte loads
    float scale;
};

__device__ __forceinline__ bool x_dead(const AttnXArgs& a, const unsigned char* mrow_base, int qrow, int key) {
    if (key >= a.Nk || (a.causal && key > qrow)) return true;
    if (mrow_base) {
        const int qi = qrow < a.Nq ? qrow : a.Nq - 1;
        return mrow_base[(long long)qi * a.msq + (long long)key * a.msk] == 0;
    }
    return false;
}

// Dead positions of one 32x32 accumulator tile as a bit per accumulator register.  The mask bytes are read HERE, before the
// accumulators are touched: with the loads inside the select on the accumulator value, hipcc 7.2 reused the register holding the
// element for the loaded byte and every masked launch returned wrong numbers (an all-true mask changed the result).
// KEY_IN_REG: the register index runs over keys and the lane is the query (forward, dQ); else the register index runs over queries
// and the lane is the key (dK, dV).
template <bool KEY_IN_REG>
__device__ __forceinline__ unsigned x_dead_bits(const AttnXArgs& a, const unsigned char* mrow_base, int lane_index, int tile0, int hf) {
    unsigned bits = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int reg_index = tile0 + kv_acc_row(r, hf);
        const bool d = KEY_IN_REG ? x_dead(a, mrow_base, lane_index, reg_index) : x_dead(a, mrow_base, reg_index, lane_index);
        bits |= (d ? 1u : 0u) << r;
    }
    return bits;
}

// dst[rows][KS] <- src rows row0.. (row stride stride_n), zero beyond n_valid rows and D columns
template <int DT>
__device__ __forceinline__ void x_load_tile(float* __restrict__ dst, const float* __restrict__ src, long long stride_n, int row0,
                                            int rows, int n_valid, int D, int tid, int nthr, bool vec) {
    constexpr int W = 32 * DT, KS = W + 1;
    if (vec) {
        constexpr int W4 = W / 4;
        for (int idx = tid; idx < rows * W4; idx += nthr) {
            const int r = idx / W4, c = (idx - r * W4) * 4;
            const int n = row0 + r;
            f32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
            if (n < n_valid && c < D) t = *reinterpret_cast<const f32x4*>(src + (long long)n * stride_n + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[r * KS + c + e] = t[e];
        }
        return;
    }
    for (int idx = tid; idx < rows * W; idx += nthr) {
        const int r = idx / W, c = idx - r * W;
        const int n = row0 + r;
        dst[r * KS + c] = (n < n_valid && c < D) ? src[(long long)n * stride_n + c] : 0.0f;
    }
}

template <int DT>
__device__ __forceinline__ void x_store_tile(float* __restrict__ dstg, long long stride_n, int row0, int n_valid, int D,
                                             const float* __restrict__ T, int lane) {
    constexpr int KS = 32 * DT + 1;
    for (int idx = lane; idx < 32 * D; idx += 64) {
        const int r = idx / D, c = idx - r * D;
        const int n = row0 + r;
        if (n < n_valid) dstg[(long long)n * stride_n + c] = T[r * KS + c];
    }
}

constexpr int XCH = 4;            // tiles of 32 rows per LDS chunk of the swept operand (128 rows)

// forward: grid (B*H, ceil(q tiles / waves)); a wave owns a 32-query tile and sweeps the keys in chunks of XCH tiles with the running
// (max, sum) rescale of utils.py:199-221 -- in this orientation (O^T[d][query]: the query is the lane) the rescale of the partial
// output is one multiplication of the lane's accumulators by a lane-private factor
template <int DT>
__global__ __launch_bounds__(XShape<DT>::THR) void attn_x_fwd_kernel(const AttnXArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KS = 32 * DT + 1, CH = XCH * 32, XTHR = XShape<DT>::THR, XW = XShape<DT>::W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hf = lane >> 5;
    const int bh = blockIdx.x, bi = bh / a.H, hi = bh - bi * a.H;
    const int D = a.D, nkt = a.nkt;
    float* K_s = smem;
    float* V_s = K_s + CH * KS;
    float* Q_w = (XShape<DT>::ALIAS ? smem : V_s + CH * KS) + wave * 32 * KS;      // aliased: read before the first chunk fill's barrier

    const float* qb = a.q + bi * a.qsb + hi * a.qsh;
    const float* kb = a.k + bi * a.ksb + hi * a.ksh;
    const float* vb = a.v + bi * a.vsb + hi * a.vsh;
    float* ob = a.out + bi * a.osb + hi * a.osh;
    const unsigned char* mb = a.mask ? a.mask + bi * a.msb + hi * a.msh : nullptr;

    const float sc2 = a.scale * LOG2E_X;
    const int qt = blockIdx.y * XW + wave;       // tiles past nqt run on zero rows and store nothing
    const int qrow = qt * 32 + l31;
    x_load_tile<DT>(Q_w, qb, a.qsn, qt * 32, 32, (qt < a.nqt) ? a.Nq : 0, D, lane, 64, a.vec);
    __syncthreads();
    float qf[16 * DT];
#pragma unroll
    for (int s = 0; s < 16 * DT; ++s) qf[s] = Q_w[l31 * KS + 2 * s + hf];

    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.0f;
    float mrun = -INFINITY, lrun = 0.0f;         // running max (raw scores) and sum of this lane's query

    for (int kc = 0; kc < nkt; kc += XCH) {
        __syncthreads();                         // every wave is done with the previous chunk
        x_load_tile<DT>(K_s, kb, a.ksn, kc * 32, CH, a.Nk, D, tid, XTHR, a.vec);
        x_load_tile<DT>(V_s, vb, a.vsn, kc * 32, CH, a.Nk, D, tid, XTHR, a.vec);
        __syncthreads();
        f32x16 sacc[XCH];
        unsigned dbits[XCH];
#pragma unroll
        for (int j = 0; j < XCH; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[j][r] = 0.0f;
            dbits[j] = (kc + j < nkt) ? x_dead_bits<true>(a, mb, qrow, (kc + j) * 32, hf) : 0xffffu;
            if (kc + j < nkt) {
                const float* kp = K_s + (j * 32 + l31) * KS + hf;
#pragma unroll
                for (int s = 0; s < 16 * DT; ++s) sacc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * s], qf[s], sacc[j], 0, 0, 0);
            }
        }
        float mx = mrun;
#pragma unroll
        for (int j = 0; j < XCH; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float sv = ((dbits[j] >> r) & 1u) ? -INFINITY : sacc[j][r];
                sacc[j][r] = sv;
                mx = fmaxf(mx, sv);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mxs = (mx == -INFINITY) ? 0.0f : mx * sc2;
        const float corr = exp2f(mrun * sc2 - mxs);          // 0 while nothing was live before (mrun = -inf)
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < XCH; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = exp2f(sacc[j][r] * sc2 - mxs);
                sacc[j][r] = p;
                sum += p;
            }
        sum += __shfl_xor(sum, 32);
        lrun = lrun * corr + sum;
        mrun = mx;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= corr;
#pragma unroll
        for (int j = 0; j < XCH; ++j) {
            if (kc + j < nkt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float* vp = V_s + (j * 32 + kv_acc_row(r, hf)) * KS + l31;
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[dt * 32], sacc[j][r], oacc[dt], 0, 0, 0);
                }
            }
        }
    }
    const float inv = lrun > 0.0f ? 1.0f / lrun : 0.0f;      // every key dead: o = 0
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) Q_w[l31 * KS + dt * 32 + kv_acc_row(r, hf)] = oacc[dt][r] * inv;
    __syncthreads();
    if (qt < a.nqt) {
        x_store_tile<DT>(ob, a.osn, qt * 32, a.Nq, D, Q_w, lane);
        if (hf == 0 && qrow < a.Nq && a.lse) a.lse[(long long)bh * a.Nq + qrow] = lrun > 0.0f ? mrun * a.scale + logf(lrun) : -FLT_MAX;
    }
}

__global__ __launch_bounds__(256) void attn_x_delta_kernel(const AttnXArgs a) {
    const int sub = threadIdx.x & 15;
    const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const long long rows = (long long)a.B * a.H * a.Nq;
    float s = 0.0f;
    if (row < rows) {
        const int n = (int)(row % a.Nq);
        const long long bh = row / a.Nq;
        const int hi = (int)(bh % a.H);
        const long long bi = bh / a.H;
        const float* op = a.o + bi * a.osb + hi * a.osh + (long long)n * a.osn;
        const float* dp = a.d_o + bi * a.osb + hi * a.osh + (long long)n * a.osn;
        for (int c = sub; c < a.D; c += 16) s += op[c] * dp[c];
    }
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if (row < rows && sub == 0) a.delta[row] = s;
}

// dK, dV: key-stationary (utils.py:262-291).  grid (B*H, ceil(key tiles / waves)); a wave owns a 32-key tile (K, V fragments in registers,
// dK^T / dV^T in accumulators) and sweeps the queries in LDS chunks of XCH tiles.
template <int DT>
__global__ __launch_bounds__(XShape<DT>::THR) void attn_x_bwd_kv_kernel(const AttnXArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KS = 32 * DT + 1, CH = XCH * 32, XTHR = XShape<DT>::THR, XW = XShape<DT>::W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hf = lane >> 5;
    const int bh = blockIdx.x, bi = bh / a.H, hi = bh - bi * a.H;
    const int D = a.D;
    float* Q_s = smem;
    float* dO_s = Q_s + CH * KS;
    float* lse_s = dO_s + CH * KS;
    float* dl_s = lse_s + CH;
    float* T_w = (XShape<DT>::ALIAS ? smem : dl_s + CH) + wave * 32 * KS;          // aliased: in Q_s, used only outside the sweep

    const float* qb = a.q + bi * a.qsb + hi * a.qsh;
    const float* kb = a.k + bi * a.ksb + hi * a.ksh;
    const float* vb = a.v + bi * a.vsb + hi * a.vsh;
    const float* dob = a.d_o + bi * a.osb + hi * a.osh;
    float* dkb = a.dk + bi * a.ksb + hi * a.ksh;
    float* dvb = a.dv + bi * a.vsb + hi * a.vsh;
    const unsigned char* mb = a.mask ? a.mask + bi * a.msb + hi * a.msh : nullptr;
    const float sc2 = a.scale * LOG2E_X;

    const int jt = blockIdx.y * XW + wave;
    const int key = jt * 32 + l31;
    float kf[16 * DT], vf[16 * DT];
    x_load_tile<DT>(T_w, kb, a.ksn, jt * 32, 32, (jt < a.nkt) ? a.Nk : 0, D, lane, 64, a.vec);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16 * DT; ++s) kf[s] = T_w[l31 * KS + 2 * s + hf];
    __syncthreads();
    x_load_tile<DT>(T_w, vb, a.vsn, jt * 32, 32, (jt < a.nkt) ? a.Nk : 0, D, lane, 64, a.vec);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16 * DT; ++s) vf[s] = T_w[l31 * KS + 2 * s + hf];

    f32x16 dkacc[DT], dvacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            dkacc[dt][r] = 0.0f;
            dvacc[dt][r] = 0.0f;
        }
    for (int qc = 0; qc < a.nqt; qc += XCH) {
        __syncthreads();
        x_load_tile<DT>(Q_s, qb, a.qsn, qc * 32, CH, a.Nq, D, tid, XTHR, a.vec);
        x_load_tile<DT>(dO_s, dob, a.osn, qc * 32, CH, a.Nq, D, tid, XTHR, a.vec);
        for (int n = tid; n < CH; n += XTHR) {
            const int qn = qc * 32 + n;
            lse_s[n] = (qn < a.Nq) ? a.lse_in[(long long)bh * a.Nq + qn] * LOG2E_X : INFINITY;      // exp2(-inf) = 0 on pad rows
            dl_s[n] = (qn < a.Nq) ? a.delta_in[(long long)bh * a.Nq + qn] : 0.0f;
        }
        __syncthreads();
        for (int qq = 0; qq < XCH && qc + qq < a.nqt; ++qq) {
            f32x16 sacc, pacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[r] = 0.0f;
                pacc[r] = 0.0f;
            }
            const float* qp = Q_s + (qq * 32 + l31) * KS + hf;
            const float* dp = dO_s + (qq * 32 + l31) * KS + hf;
#pragma unroll
            for (int s = 0; s < 16 * DT; ++s) {
                sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(qp[2 * s], kf[s], sacc, 0, 0, 0);      // S[q][key]
                pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(dp[2 * s], vf[s], pacc, 0, 0, 0);      // dP[q][key]
            }
            const unsigned db = x_dead_bits<false>(a, mb, key, (qc + qq) * 32, hf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ql = qq * 32 + kv_acc_row(r, hf), qrow = qc * 32 + ql;
                float p = exp2f(sacc[r] * sc2 - lse_s[ql]);
                if (jt >= a.nkt || qrow >= a.Nq || ((db >> r) & 1u)) p = 0.0f;          // select, never multiply: exp2 may be inf on a dead row
                sacc[r] = p;
                pacc[r] = p == 0.0f ? 0.0f : p * a.scale * (pacc[r] - dl_s[ql]);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (qq * 32 + kv_acc_row(r, hf)) * KS + l31;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    dvacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(dO_s[row + dt * 32], sacc[r], dvacc[dt], 0, 0, 0);
                    dkacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Q_s[row + dt * 32], pacc[r], dkacc[dt], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) T_w[l31 * KS + dt * 32 + kv_acc_row(r, hf)] = dkacc[dt][r];
    __syncthreads();
    if (jt < a.nkt) x_store_tile<DT>(dkb, a.ksn, jt * 32, a.Nk, D, T_w, lane);
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) T_w[l31 * KS + dt * 32 + kv_acc_row(r, hf)] = dvacc[dt][r];
    __syncthreads();
    if (jt < a.nkt) x_store_tile<DT>(dvb, a.vsn, jt * 32, a.Nk, D, T_w, lane);
}

// dQ: query-stationary mirror of the forward kernel (grid (B*H, ceil(q tiles / waves)); keys swept in LDS chunks of XCH tiles)
template <int DT>
__global__ __launch_bounds__(XShape<DT>::THR) void attn_x_bwd_q_kernel(const AttnXArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KS = 32 * DT + 1, CH = XCH * 32, XTHR = XShape<DT>::THR, XW = XShape<DT>::W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hf = lane >> 5;
    const int bh = blockIdx.x, bi = bh / a.H, hi = bh - bi * a.H;
    const int D = a.D, nkt = a.nkt;
    float* K_s = smem;
    float* V_s = K_s + CH * KS;
    float* T_w = (XShape<DT>::ALIAS ? smem : V_s + CH * KS) + wave * 32 * KS;      // aliased: in K_s, used only outside the sweep

    const float* qb = a.q + bi * a.qsb + hi * a.qsh;
    const float* kb = a.k + bi * a.ksb + hi * a.ksh;
    const float* vb = a.v + bi * a.vsb + hi * a.vsh;
    const float* dob = a.d_o + bi * a.osb + hi * a.osh;
    float* dqb = a.dq + bi * a.qsb + hi * a.qsh;
    const unsigned char* mb = a.mask ? a.mask + bi * a.msb + hi * a.msh : nullptr;
    const float sc2 = a.scale * LOG2E_X;

    const int qt = blockIdx.y * XW + wave;
    const int qrow = qt * 32 + l31;
    const bool q_ok = (qt < a.nqt) && (qrow < a.Nq);
    float qf[16 * DT], dof[16 * DT];
    x_load_tile<DT>(T_w, qb, a.qsn, qt * 32, 32, (qt < a.nqt) ? a.Nq : 0, D, lane, 64, a.vec);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16 * DT; ++s) qf[s] = T_w[l31 * KS + 2 * s + hf];
    __syncthreads();
    x_load_tile<DT>(T_w, dob, a.osn, qt * 32, 32, (qt < a.nqt) ? a.Nq : 0, D, lane, 64, a.vec);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16 * DT; ++s) dof[s] = T_w[l31 * KS + 2 * s + hf];
    const float lse2 = q_ok ? a.lse_in[(long long)bh * a.Nq + qrow] * LOG2E_X : INFINITY;
    const float dl = q_ok ? a.delta_in[(long long)bh * a.Nq + qrow] : 0.0f;

    f32x16 dqacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dqacc[dt][r] = 0.0f;
    for (int kc = 0; kc < nkt; kc += XCH) {
        __syncthreads();
        x_load_tile<DT>(K_s, kb, a.ksn, kc * 32, CH, a.Nk, D, tid, XTHR, a.vec);
        x_load_tile<DT>(V_s, vb, a.vsn, kc * 32, CH, a.Nk, D, tid, XTHR, a.vec);
        __syncthreads();
        for (int j = 0; j < XCH && kc + j < nkt; ++j) {
            f32x16 sacc, pacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[r] = 0.0f;
                pacc[r] = 0.0f;
            }
            const float* kp = K_s + (j * 32 + l31) * KS + hf;
            const float* vp = V_s + (j * 32 + l31) * KS + hf;
#pragma unroll
            for (int s = 0; s < 16 * DT; ++s) {
                sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * s], qf[s], sacc, 0, 0, 0);      // S^T[key][q]
                pacc = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[2 * s], dof[s], pacc, 0, 0, 0);     // dP^T[key][q]
            }
            const unsigned db = x_dead_bits<true>(a, mb, qrow, (kc + j) * 32, hf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = exp2f(sacc[r] * sc2 - lse2);
                const bool dead = !q_ok || ((db >> r) & 1u);
                pacc[r] = dead ? 0.0f : p * a.scale * (pacc[r] - dl);                             // dS^T
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* kr = K_s + (j * 32 + kv_acc_row(r, hf)) * KS + l31;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) dqacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[dt * 32], pacc[r], dqacc[dt], 0, 0, 0);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) T_w[l31 * KS + dt * 32 + kv_acc_row(r, hf)] = dqacc[dt][r];
    __syncthreads();
    if (qt < a.nqt) x_store_tile<DT>(dqb, a.qsn, qt * 32, a.Nq, D, T_w, lane);
}

// ---- bf16 matrix-core twins (KANVIT_FLAG_BF16_MFMA, D <= 64): the fp32 kernels' tile orientation, chunked sweep, masks and
// running (max, sum), with every product on v_mfma_f32_32x32x16_bf16 and the rounding points of attention.hip's bf16 kernels
// (oracle/kan_oracle.py::_RoundedAttention):
//   forward   S^T = r(K).r(Q)^T; p = exp(scale S - max) in fp32, max = the row's maximum over ALL keys (a first sweep, see
//             attn_x_fwd_bf16_kernel); O^T accumulates r(V)^T.r(p) and is divided by the fp32 row sum at the end
//   backward  P = exp(scale S - lse) from the same rounded S; dP = r(dO).r(V)^T; dS = P scale (dP - delta), delta = rowsum(dO*O)
//             in fp32 (attn_x_delta_kernel); dV = r(P)^T.r(dO), dK = r(dS)^T.r(Q), dQ = r(dS).r(K)
// The swept operand lives in the LDS AS bf16, converted once per chunk by the work-group instead of once per wave: a row image
// [CH][RB] (RB = 32*DT + 8: the A fragment of a lane's row is one ds_read_b128) for the products over d, and a transposed image
// [32*DT][TB] (TB = CH + 8) with the 32 rows of each tile in accumulator slot order (kv_key_slot) for the products whose k index
// is the accumulator's register index (the score tile packed to bf16 by kv_acc8 is the B operand; cdna guide section 3).  The
// stationary operand (a wave's own 32 rows) is read from global straight into bf16 fragments, and the results are stored straight
// from the accumulators (register 4q + e of O^T is column dt*32 + 8q + 4hf + e of the lane's row): no staging tile.
// LDS per work-group (DT = 2): forward 35 KiB (K rows, V^T), dK/dV 71 KiB (Q, dO rows and transposes, lse, delta), dQ 53 KiB
// (K, V rows, K^T).  Operand idioms as in attention.hip (kv_pk, kv_pack8, kv_acc8, kv_key_slot).
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned kv_pk(float lo, float hi) {
    bf16x2_t v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ bf16x8_t kv_pack8(const float (&f)[8]) {
    const u32x4 u = {kv_pk(f[0], f[1]), kv_pk(f[2], f[3]), kv_pk(f[4], f[5]), kv_pk(f[6], f[7])};
    return __builtin_bit_cast(bf16x8_t, u);
}
__device__ __forceinline__ bf16x8_t kv_acc8(const f32x16& a, int s) {
    const u32x4 u = {kv_pk(a[8 * s], a[8 * s + 1]), kv_pk(a[8 * s + 2], a[8 * s + 3]), kv_pk(a[8 * s + 4], a[8 * s + 5]),
                     kv_pk(a[8 * s + 6], a[8 * s + 7])};
    return __builtin_bit_cast(bf16x8_t, u);
}
__device__ __forceinline__ int kv_key_slot(int ko) {      // slot of row offset ko (0..31) inside its tile of a transposed image
    const int w = ko & 15;
    return (ko & 16) + 8 * ((w >> 2) & 1) + 4 * (w >> 3) + (w & 3);
}

template <int DT>
struct XbShape {
    static constexpr int RB = 32 * DT + 8;         // bf16 row image stride (elements)
    static constexpr int TB = XCH * 32 + 8;        // bf16 transposed image stride (elements)
    static constexpr int ROWS = XCH * 32 * RB;     // elements of a row image
    static constexpr int TRANS = 32 * DT * TB;     // elements of a transposed image
};

// columns c..c+7 of one fp32 row rounded to bf16 (zero at columns >= D, everywhere unless ok): a wave's own rows
__device__ __forceinline__ bf16x8_t xb_grow8(const float* __restrict__ p, int c, int D, bool ok, bool vec) {
    float f[8];
    if (vec) {
        f32x4 u0 = {0.0f, 0.0f, 0.0f, 0.0f}, u1 = u0;
        if (ok && c < D) u0 = *reinterpret_cast<const f32x4*>(p + c);
        if (ok && c + 4 < D) u1 = *reinterpret_cast<const f32x4*>(p + c + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[e] = u0[e];
            f[4 + e] = u1[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (ok && c + e < D) ? p[c + e] : 0.0f;
    }
    return kv_pack8(f);
}

// rows row0 .. row0 + CH - 1 of src -> the bf16 row image (ROWS) and / or transposed image (TRANS) of a chunk; zero beyond n_valid
// rows and D columns.  A thread converts a row PAIR (2m, 2m + 1) x 4 columns: the pair is one 32-bit word of the transposed image.
template <int DT, int NTHR, bool ROWS, bool TRANS>
__device__ __forceinline__ void xb_fill(unsigned short* __restrict__ rimg, unsigned short* __restrict__ timg, const float* __restrict__ src,
                                        long long stride_n, int row0, int n_valid, int D, int tid, bool vec) {
    constexpr int W4 = 8 * DT, ITEMS = XCH * 16 * W4, RB = XbShape<DT>::RB, TB = XbShape<DT>::TB;
    static_assert(ITEMS % NTHR == 0, "whole passes");
#pragma unroll
    for (int it = 0; it < ITEMS / NTHR; ++it) {
        const int idx = it * NTHR + tid;
        const int m = idx / W4, c = (idx - m * W4) * 4;
        const int n0 = row0 + 2 * m;
        f32x4 t0 = {0.0f, 0.0f, 0.0f, 0.0f}, t1 = t0;
        if (vec) {
            if (c < D && n0 < n_valid) t0 = *reinterpret_cast<const f32x4*>(src + (long long)n0 * stride_n + c);
            if (c < D && n0 + 1 < n_valid) t1 = *reinterpret_cast<const f32x4*>(src + (long long)(n0 + 1) * stride_n + c);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c + e < D && n0 < n_valid) t0[e] = src[(long long)n0 * stride_n + c + e];
                if (c + e < D && n0 + 1 < n_valid) t1[e] = src[(long long)(n0 + 1) * stride_n + c + e];
            }
        }
        if constexpr (ROWS) {
            unsigned* r0p = reinterpret_cast<unsigned*>(rimg + (2 * m) * RB + c);
            unsigned* r1p = reinterpret_cast<unsigned*>(rimg + (2 * m + 1) * RB + c);
            r0p[0] = kv_pk(t0[0], t0[1]);
            r0p[1] = kv_pk(t0[2], t0[3]);
            r1p[0] = kv_pk(t1[0], t1[1]);
            r1p[1] = kv_pk(t1[2], t1[3]);
        }
        if constexpr (TRANS) {
            const int pos = ((2 * m) & ~31) + kv_key_slot((2 * m) & 31);      // even: rows 2m, 2m + 1 are adjacent slots
#pragma unroll
            for (int e = 0; e < 4; ++e) *reinterpret_cast<unsigned*>(timg + (c + e) * TB + pos) = kv_pk(t0[e], t1[e]);
        }
    }
}

// the lane's row of a [d][row] accumulator set (O^T, dK^T, dV^T, dQ^T: register r = column dt*32 + kv_acc_row(r, hf)) times mul
template <int DT>
__device__ __forceinline__ void xb_store_row(float* __restrict__ p, const f32x16 (&acc)[DT], float mul, int D, int hf, bool vec) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = dt * 32 + 8 * q + 4 * hf;
            if (vec) {
                if (c < D) {
                    const f32x4 v = {acc[dt][4 * q] * mul, acc[dt][4 * q + 1] * mul, acc[dt][4 * q + 2] * mul, acc[dt][4 * q + 3] * mul};
                    *reinterpret_cast<f32x4*>(p + c) = v;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < D) p[c + e] = acc[dt][4 * q + e] * mul;
            }
        }
}

constexpr int XB_THR = 512;       // 8 waves, two per SIMD, as the fp32 DT = 1, 2 kernels

// S^T tiles of one key chunk (key on the register index, the lane's query on the column), dead positions -inf
template <int DT>
__device__ __forceinline__ void xb_fwd_scores(f32x16 (&sacc)[XCH], const unsigned short* __restrict__ Kr, const bf16x8_t (&qf)[2 * DT],
                                              const AttnXArgs& a, const unsigned char* mb, int qrow, int kc, int l31, int hf) {
    constexpr int RB = XbShape<DT>::RB;
#pragma unroll
    for (int j = 0; j < XCH; ++j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[j][r] = 0.0f;
        const unsigned dbits = (kc + j < a.nkt) ? x_dead_bits<true>(a, mb, qrow, (kc + j) * 32, hf) : 0xffffu;
        if (kc + j < a.nkt) {
            const unsigned short* kp = Kr + (j * 32 + l31) * RB + 8 * hf;
#pragma unroll
            for (int ks = 0; ks < 2 * DT; ++ks)
                sacc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(kp + 16 * ks), qf[ks], sacc[j], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[j][r] = ((dbits >> r) & 1u) ? -INFINITY : sacc[j][r];
    }
}

// forward: two sweeps over the keys.  The first forms S and keeps the row maximum only; the second rounds p = exp(scale S - max)
// against that FINAL maximum, so r(p) is the value the one-head-per-work-group bf16 kernels (and the rounded oracle) round, whatever
// the chunking.  A running maximum would round p against the maximum of the chunks seen so far and rescale r(p) afterwards:
// r(p c) != r(p) c, an error of the size of the rounding itself (measured: 1e-3 of max |o|, passed on through delta to 2-3e-3 of
// max |dq|, |dk|, against 2-5e-4 with the final maximum).  The first sweep costs the K fills and a third of the MFMAs once more.
template <int DT>
__global__ __launch_bounds__(XB_THR) void attn_x_fwd_bf16_kernel(const AttnXArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int TB = XbShape<DT>::TB, XW = XB_THR / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hf = lane >> 5;
    const int bh = blockIdx.x, bi = bh / a.H, hi = bh - bi * a.H;
    const int D = a.D, nkt = a.nkt;
    unsigned short* Kr = reinterpret_cast<unsigned short*>(smem);        // [CH][RB]
    unsigned short* Vt = Kr + XbShape<DT>::ROWS;                           // [32*DT][TB]

    const float* qb = a.q + bi * a.qsb + hi * a.qsh;
    const float* kb = a.k + bi * a.ksb + hi * a.ksh;
    const float* vb = a.v + bi * a.vsb + hi * a.vsh;
    float* ob = a.out + bi * a.osb + hi * a.osh;
    const unsigned char* mb = a.mask ? a.mask + bi * a.msb + hi * a.msh : nullptr;

    const float sc2 = a.scale * LOG2E_X;
    const int qt = blockIdx.y * XW + wave;       // tiles past nqt run on zero rows and store nothing
    const int qrow = qt * 32 + l31;
    const bool q_ok = qt < a.nqt && qrow < a.Nq;
    bf16x8_t qf[2 * DT];
#pragma unroll
    for (int ks = 0; ks < 2 * DT; ++ks) qf[ks] = xb_grow8(qb + (long long)(q_ok ? qrow : 0) * a.qsn, 16 * ks + 8 * hf, D, q_ok, a.vec);

    f32x16 sacc[XCH];
    float mx = -INFINITY;
    for (int kc = 0; kc < nkt; kc += XCH) {
        __syncthreads();
        xb_fill<DT, XB_THR, true, false>(Kr, nullptr, kb, a.ksn, kc * 32, a.Nk, D, tid, a.vec);
        __syncthreads();
        xb_fwd_scores<DT>(sacc, Kr, qf, a, mb, qrow, kc, l31, hf);
#pragma unroll
        for (int j = 0; j < XCH; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[j][r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mxs = (mx == -INFINITY) ? 0.0f : mx * sc2;

    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.0f;
    float lsum = 0.0f;
    for (int kc = 0; kc < nkt; kc += XCH) {
        __syncthreads();                         // every wave is done with the previous chunk
        if (nkt > XCH) xb_fill<DT, XB_THR, true, false>(Kr, nullptr, kb, a.ksn, kc * 32, a.Nk, D, tid, a.vec);   // one chunk: still there
        xb_fill<DT, XB_THR, false, true>(nullptr, Vt, vb, a.vsn, kc * 32, a.Nk, D, tid, a.vec);
        __syncthreads();
        xb_fwd_scores<DT>(sacc, Kr, qf, a, mb, qrow, kc, l31, hf);
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < XCH; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = exp2f(sacc[j][r] * sc2 - mxs);
                sacc[j][r] = p;
                sum += p;
            }
        lsum += sum + __shfl_xor(sum, 32);
#pragma unroll
        for (int j = 0; j < XCH; ++j) {
            if (kc + j < nkt) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const bf16x8_t pb = kv_acc8(sacc[j], s2);
                    const unsigned short* vp = Vt + l31 * TB + j * 32 + 16 * s2 + 8 * hf;
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(vp + dt * 32 * TB), pb, oacc[dt], 0, 0, 0);
                }
            }
        }
    }
    if (q_ok) {
        const float inv = lsum > 0.0f ? 1.0f / lsum : 0.0f;      // every key dead: o = 0
        xb_store_row<DT>(ob + (long long)qrow * a.osn, oacc, inv, D, hf, a.vec && ((uintptr_t)ob % 16 == 0));
        if (hf == 0 && a.lse) a.lse[(long long)bh * a.Nq + qrow] = lsum > 0.0f ? mx * a.scale + logf(lsum) : -FLT_MAX;
    }
}

// dK, dV: key-stationary, as attn_x_bwd_kv_kernel.  A wave's own K, V rows are bf16 fragments in registers; the queries are swept in
// chunks whose Q and dO images are held twice, as rows (S, dP: the reduction runs over d) and transposed (dV^T, dK^T: over queries).
template <int DT>
__global__ __launch_bounds__(XB_THR) void attn_x_bwd_kv_bf16_kernel(const AttnXArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RB = XbShape<DT>::RB, TB = XbShape<DT>::TB, CH = XCH * 32, XW = XB_THR / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hf = lane >> 5;
    const int bh = blockIdx.x, bi = bh / a.H, hi = bh - bi * a.H;
    const int D = a.D;
    unsigned short* Qr = reinterpret_cast<unsigned short*>(smem);         // [CH][RB]
    unsigned short* dOr = Qr + XbShape<DT>::ROWS;                          // [CH][RB]
    unsigned short* Qt = dOr + XbShape<DT>::ROWS;                          // [32*DT][TB]
    unsigned short* dOt = Qt + XbShape<DT>::TRANS;                         // [32*DT][TB]
    float* lse_s = reinterpret_cast<float*>(dOt + XbShape<DT>::TRANS);     // [CH]
    float* dl_s = lse_s + CH;                                               // [CH]

    const float* qb = a.q + bi * a.qsb + hi * a.qsh;
    const float* kb = a.k + bi * a.ksb + hi * a.ksh;
    const float* vb = a.v + bi * a.vsb + hi * a.vsh;
    const float* dob = a.d_o + bi * a.osb + hi * a.osh;
    float* dkb = a.dk + bi * a.ksb + hi * a.ksh;
    float* dvb = a.dv + bi * a.vsb + hi * a.vsh;
    const unsigned char* mb = a.mask ? a.mask + bi * a.msb + hi * a.msh : nullptr;
    const float sc2 = a.scale * LOG2E_X;

    const int jt = blockIdx.y * XW + wave;
    const int key = jt * 32 + l31;
    const bool k_ok = jt < a.nkt && key < a.Nk;
    bf16x8_t kf[2 * DT], vf[2 * DT];
#pragma unroll
    for (int ks = 0; ks < 2 * DT; ++ks) {
        kf[ks] = xb_grow8(kb + (long long)(k_ok ? key : 0) * a.ksn, 16 * ks + 8 * hf, D, k_ok, a.vec);
        vf[ks] = xb_grow8(vb + (long long)(k_ok ? key : 0) * a.vsn, 16 * ks + 8 * hf, D, k_ok, a.vec);
    }

    f32x16 dkacc[DT], dvacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            dkacc[dt][r] = 0.0f;
            dvacc[dt][r] = 0.0f;
        }
    for (int qc = 0; qc < a.nqt; qc += XCH) {
        __syncthreads();
        xb_fill<DT, XB_THR, true, true>(Qr, Qt, qb, a.qsn, qc * 32, a.Nq, D, tid, a.vec);
        xb_fill<DT, XB_THR, true, true>(dOr, dOt, dob, a.osn, qc * 32, a.Nq, D, tid, a.vec);
        for (int n = tid; n < CH; n += XB_THR) {
            const int qn = qc * 32 + n;
            lse_s[n] = (qn < a.Nq) ? a.lse_in[(long long)bh * a.Nq + qn] * LOG2E_X : INFINITY;      // exp2(-inf) = 0 on pad rows
            dl_s[n] = (qn < a.Nq) ? a.delta_in[(long long)bh * a.Nq + qn] : 0.0f;
        }
        __syncthreads();
        for (int qq = 0; qq < XCH && qc + qq < a.nqt; ++qq) {
            f32x16 sacc, pacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[r] = 0.0f;
                pacc[r] = 0.0f;
            }
            const unsigned short* qp = Qr + (qq * 32 + l31) * RB + 8 * hf;
            const unsigned short* dp = dOr + (qq * 32 + l31) * RB + 8 * hf;
#pragma unroll
            for (int ks = 0; ks < 2 * DT; ++ks) {
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(qp + 16 * ks), kf[ks], sacc, 0, 0, 0);  // S[q][key]
                pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(dp + 16 * ks), vf[ks], pacc, 0, 0, 0);  // dP[q][key]
            }
            const unsigned db = x_dead_bits<false>(a, mb, key, (qc + qq) * 32, hf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ql = qq * 32 + kv_acc_row(r, hf), qrow = qc * 32 + ql;
                float p = exp2f(sacc[r] * sc2 - lse_s[ql]);
                if (jt >= a.nkt || qrow >= a.Nq || ((db >> r) & 1u)) p = 0.0f;          // select, never multiply: exp2 may be inf on a dead row
                sacc[r] = p;
                pacc[r] = p == 0.0f ? 0.0f : p * a.scale * (pacc[r] - dl_s[ql]);
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8_t pb = kv_acc8(sacc, s2), sb = kv_acc8(pacc, s2);
                const int off = l31 * TB + qq * 32 + 16 * s2 + 8 * hf;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    dvacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(dOt + off + dt * 32 * TB), pb, dvacc[dt], 0, 0, 0);
                    dkacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Qt + off + dt * 32 * TB), sb, dkacc[dt], 0, 0, 0);
                }
            }
        }
    }
    if (k_ok) {
        xb_store_row<DT>(dkb + (long long)key * a.ksn, dkacc, 1.0f, D, hf, a.vec && ((uintptr_t)dkb % 16 == 0));
        xb_store_row<DT>(dvb + (long long)key * a.vsn, dvacc, 1.0f, D, hf, a.vec && ((uintptr_t)dvb % 16 == 0));
    }
}

// dQ: query-stationary, as attn_x_bwd_q_kernel.  Own Q, dO rows as bf16 fragments; K, V chunks as rows, K also transposed (dQ^T).
template <int DT>
__global__ __launch_bounds__(XB_THR) void attn_x_bwd_q_bf16_kernel(const AttnXArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RB = XbShape<DT>::RB, TB = XbShape<DT>::TB, XW = XB_THR / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hf = lane >> 5;
    const int bh = blockIdx.x, bi = bh / a.H, hi = bh - bi * a.H;
    const int D = a.D, nkt = a.nkt;
    unsigned short* Kr = reinterpret_cast<unsigned short*>(smem);         // [CH][RB]
    unsigned short* Vr = Kr + XbShape<DT>::ROWS;                           // [CH][RB]
    unsigned short* Kt = Vr + XbShape<DT>::ROWS;                           // [32*DT][TB]

    const float* qb = a.q + bi * a.qsb + hi * a.qsh;
    const float* kb = a.k + bi * a.ksb + hi * a.ksh;
    const float* vb = a.v + bi * a.vsb + hi * a.vsh;
    const float* dob = a.d_o + bi * a.osb + hi * a.osh;
    float* dqb = a.dq + bi * a.qsb + hi * a.qsh;
    const unsigned char* mb = a.mask ? a.mask + bi * a.msb + hi * a.msh : nullptr;
    const float sc2 = a.scale * LOG2E_X;

    const int qt = blockIdx.y * XW + wave;
    const int qrow = qt * 32 + l31;
    const bool q_ok = (qt < a.nqt) && (qrow < a.Nq);
    bf16x8_t qf[2 * DT], dof[2 * DT];
#pragma unroll
    for (int ks = 0; ks < 2 * DT; ++ks) {
        qf[ks] = xb_grow8(qb + (long long)(q_ok ? qrow : 0) * a.qsn, 16 * ks + 8 * hf, D, q_ok, a.vec);
        dof[ks] = xb_grow8(dob + (long long)(q_ok ? qrow : 0) * a.osn, 16 * ks + 8 * hf, D, q_ok, a.vec);
    }
    const float lse2 = q_ok ? a.lse_in[(long long)bh * a.Nq + qrow] * LOG2E_X : INFINITY;
    const float dl = q_ok ? a.delta_in[(long long)bh * a.Nq + qrow] : 0.0f;

    f32x16 dqacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dqacc[dt][r] = 0.0f;
    for (int kc = 0; kc < nkt; kc += XCH) {
        __syncthreads();
        xb_fill<DT, XB_THR, true, true>(Kr, Kt, kb, a.ksn, kc * 32, a.Nk, D, tid, a.vec);
        xb_fill<DT, XB_THR, true, false>(Vr, nullptr, vb, a.vsn, kc * 32, a.Nk, D, tid, a.vec);
        __syncthreads();
        for (int j = 0; j < XCH && kc + j < nkt; ++j) {
            f32x16 sacc, pacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sacc[r] = 0.0f;
                pacc[r] = 0.0f;
            }
            const unsigned short* kp = Kr + (j * 32 + l31) * RB + 8 * hf;
            const unsigned short* vp = Vr + (j * 32 + l31) * RB + 8 * hf;
#pragma unroll
            for (int ks = 0; ks < 2 * DT; ++ks) {
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(kp + 16 * ks), qf[ks], sacc, 0, 0, 0);   // S^T[key][q]
                pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(vp + 16 * ks), dof[ks], pacc, 0, 0, 0);  // dP^T[key][q]
            }
            const unsigned db = x_dead_bits<true>(a, mb, qrow, (kc + j) * 32, hf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = exp2f(sacc[r] * sc2 - lse2);
                const bool dead = !q_ok || ((db >> r) & 1u);
                pacc[r] = dead ? 0.0f : p * a.scale * (pacc[r] - dl);                             // dS^T
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8_t sb = kv_acc8(pacc, s2);
                const unsigned short* kt = Kt + l31 * TB + j * 32 + 16 * s2 + 8 * hf;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    dqacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(kt + dt * 32 * TB), sb, dqacc[dt], 0, 0, 0);
            }
        }
    }
    if (q_ok) xb_store_row<DT>(dqb + (long long)qrow * a.qsn, dqacc, 1.0f, D, hf, a.vec && ((uintptr_t)dqb % 16 == 0));
}

int x_check(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const char* who) {
    if (!d || !e) return kv_fail(KANVIT_EINVAL, "%s: null descriptor", who);
    if (d->B < 0 || d->H < 1 || d->N < 1 || e->Nk < 1 || d->D < 1) return kv_fail(KANVIT_EINVAL, "%s: bad sizes", who);
    if (d->D > KANVIT_ATTN_X_MAX_D || (d->D & 1)) return kv_fail(KANVIT_EINVAL, "%s: D=%d must be even and <= %d", who, d->D, KANVIT_ATTN_X_MAX_D);
    if ((long long)d->B * d->H > 0x7fffffffLL) return kv_fail(KANVIT_EINVAL, "%s: B*H too large", who);
    if (!(d->scale > 0.0f)) return kv_fail(KANVIT_EINVAL, "%s: scale=%g must be positive (the running maximum is taken over the raw scores)", who, (double)d->scale);
    if (d->causal && e->Nk > d->N)
        return kv_fail(KANVIT_EINVAL, "%s: causal with k_len=%d > q_len=%d is ill-defined in the reference (utils.py:169,183: the first k_len - q_len queries see no key)", who, e->Nk, d->N);
    if ((d->flags & KANVIT_FLAG_BF16_MFMA) && d->D > KANVIT_ATTN_MAX_D)
        return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_BF16_MFMA covers D <= %d in the general attention kernels; D=%d runs exact fp32 only (pass no flag)",
                       who, KANVIT_ATTN_MAX_D, d->D);
    if ((long long)(d->N + 127) / 128 > 65535 || (long long)(e->Nk + 127) / 128 > 65535) return kv_fail(KANVIT_EINVAL, "%s: sequence too long for one launch", who);
    return 0;
}

AttnXArgs x_args(const kanvit_attn_desc* d, const kanvit_attn_ext* e) {
    AttnXArgs a{};
    a.B = d->B; a.H = d->H; a.Nq = d->N; a.Nk = e->Nk; a.D = d->D; a.causal = d->causal; a.scale = d->scale;
    a.nqt = (d->N + 31) / 32;
    a.nkt = (e->Nk + 31) / 32;
    a.qsb = d->q_stride_b; a.qsh = d->q_stride_h; a.qsn = d->q_stride_n;
    a.ksb = d->k_stride_b; a.ksh = d->k_stride_h; a.ksn = d->k_stride_n;
    a.vsb = d->v_stride_b; a.vsh = d->v_stride_h; a.vsn = d->v_stride_n;
    a.osb = d->o_stride_b; a.osh = d->o_stride_h; a.osn = d->o_stride_n;
    a.vec = (d->D % 4 == 0);
    for (long long sd : {a.qsb, a.qsh, a.qsn, a.ksb, a.ksh, a.ksn, a.vsb, a.vsh, a.vsn, a.osb, a.osh, a.osn}) a.vec = a.vec && (sd % 4 == 0);
    a.mask = (const unsigned char*)e->mask;
    a.msb = e->mask_stride_b; a.msh = e->mask_stride_h; a.msq = e->mask_stride_q; a.msk = e->mask_stride_k;
    return a;
}

// LDS of a work-group: the two chunk buffers (CH rows each) and, unless aliased onto them, one 32-row staging tile per wave
template <int DT>
constexpr size_t x_stage_floats() {
    static_assert(!XShape<DT>::ALIAS || XShape<DT>::W * 32 <= 2 * XCH * 32, "aliased staging tiles must lie inside the chunk buffers");
    return XShape<DT>::ALIAS ? 0 : (size_t)XShape<DT>::W * 32 * (32 * DT + 1);
}

template <int DT>
int x_launch_fwd(const AttnXArgs& a, hipStream_t st) {
    constexpr int KS = 32 * DT + 1, CH = XCH * 32, XTHR = XShape<DT>::THR, XW = XShape<DT>::W;
    const size_t lds = sizeof(float) * ((size_t)2 * CH * KS + x_stage_floats<DT>());
    static_assert(sizeof(float) * ((size_t)2 * CH * KS + x_stage_floats<DT>()) <= 160 * 1024, "forward LDS over 160 KiB");
    KV_ALLOW_LDS(160 * 1024, (attn_x_fwd_kernel<DT>));
    hipLaunchKernelGGL((attn_x_fwd_kernel<DT>), dim3((unsigned)(a.B * a.H), (unsigned)((a.nqt + XW - 1) / XW)), dim3(XTHR), lds, st, a);
    KV_LAUNCH_CHECK("attn_x_fwd_kernel");
    return 0;
}

template <int DT>
int x_launch_bwd(const AttnXArgs& a, hipStream_t st) {
    constexpr int KS = 32 * DT + 1, CH = XCH * 32, XTHR = XShape<DT>::THR, XW = XShape<DT>::W;
    const size_t lds_kv = sizeof(float) * ((size_t)2 * CH * KS + 2 * (size_t)CH + x_stage_floats<DT>());
    const size_t lds_q = sizeof(float) * ((size_t)2 * CH * KS + x_stage_floats<DT>());
    static_assert(sizeof(float) * ((size_t)2 * CH * KS + 2 * (size_t)CH + x_stage_floats<DT>()) <= 160 * 1024, "dK/dV LDS over 160 KiB");
    KV_ALLOW_LDS(160 * 1024, (attn_x_bwd_kv_kernel<DT>));
    KV_ALLOW_LDS(160 * 1024, (attn_x_bwd_q_kernel<DT>));
    hipLaunchKernelGGL((attn_x_bwd_kv_kernel<DT>), dim3((unsigned)(a.B * a.H), (unsigned)((a.nkt + XW - 1) / XW)), dim3(XTHR), lds_kv, st, a);
    KV_LAUNCH_CHECK("attn_x_bwd_kv_kernel");
    hipLaunchKernelGGL((attn_x_bwd_q_kernel<DT>), dim3((unsigned)(a.B * a.H), (unsigned)((a.nqt + XW - 1) / XW)), dim3(XTHR), lds_q, st, a);
    KV_LAUNCH_CHECK("attn_x_bwd_q_kernel");
    return 0;
}

// bf16 twins: LDS of the three kernels (bf16 images; the dK/dV kernel also keeps the chunk's lse and delta)
template <int DT>
int xb_launch_fwd(const AttnXArgs& a, hipStream_t st) {
    constexpr int XW = XB_THR / 64;
    constexpr size_t lds = 2 * ((size_t)XbShape<DT>::ROWS + XbShape<DT>::TRANS);
    KV_ALLOW_LDS(lds, (attn_x_fwd_bf16_kernel<DT>));
    hipLaunchKernelGGL((attn_x_fwd_bf16_kernel<DT>), dim3((unsigned)(a.B * a.H), (unsigned)((a.nqt + XW - 1) / XW)), dim3(XB_THR), lds, st, a);
    KV_LAUNCH_CHECK("attn_x_fwd_bf16_kernel");
    return 0;
}

template <int DT>
int xb_launch_bwd(const AttnXArgs& a, hipStream_t st) {
    constexpr int XW = XB_THR / 64;
    constexpr size_t lds_kv = 2 * (2 * (size_t)XbShape<DT>::ROWS + 2 * (size_t)XbShape<DT>::TRANS) + sizeof(float) * 2 * XCH * 32;
    constexpr size_t lds_q = 2 * (2 * (size_t)XbShape<DT>::ROWS + XbShape<DT>::TRANS);
    static_assert(lds_kv <= 160 * 1024 && (2 * (2 * (size_t)XbShape<DT>::ROWS + 2 * (size_t)XbShape<DT>::TRANS)) % 16 == 0, "dK/dV LDS");
    KV_ALLOW_LDS(lds_kv, (attn_x_bwd_kv_bf16_kernel<DT>));
    KV_ALLOW_LDS(lds_q, (attn_x_bwd_q_bf16_kernel<DT>));
    hipLaunchKernelGGL((attn_x_bwd_kv_bf16_kernel<DT>), dim3((unsigned)(a.B * a.H), (unsigned)((a.nkt + XW - 1) / XW)), dim3(XB_THR), lds_kv, st, a);
    KV_LAUNCH_CHECK("attn_x_bwd_kv_bf16_kernel");
    hipLaunchKernelGGL((attn_x_bwd_q_bf16_kernel<DT>), dim3((unsigned)(a.B * a.H), (unsigned)((a.nqt + XW - 1) / XW)), dim3(XB_THR), lds_q, st, a);
    KV_LAUNCH_CHECK("attn_x_bwd_q_bf16_kernel");
    return 0;
}

// ---- single-query attention (kanvit_attn_q1_*): ONE query per (batch, head) against all Nk keys and values ------------------
// The head of a ViT reads only the class token, so its last block needs one attention row per head.  With one query there is no
// matrix product left: the forward is a pass over K (scores) and a pass over V (output), the backward one pass that reads K and V
// and writes dK and dV -- plain fp32 on the vector pipe, HBM-bound.
//   work-group  256 threads = 16 lane groups of 16 lanes for one (batch, head); lane group g takes the keys j = g, g + 16, ...
//   lane        `sub` of a group holds the columns (t*16 + sub)*V .. + V of a row, t < ceil(D / (16 V)): one V-wide load per lane,
//               a group reads 16*V consecutive floats of a row (V = 4: 256 bytes)
//   sums        over d inside a group by four xor-shuffles; over the keys first inside a lane group in key order, then over the 16
//               groups in group order through the LDS: one fixed order, no atomics, bitwise reproducible
// V = 4 needs D % 4 == 0 and 16-byte aligned rows, V = 2 (D is even) 8-byte aligned rows, V = 1 takes anything.
// The probabilities go through their own output p[B][H][Nk]: raw scores, then exp(s - max), then the normalised values, so any Nk
// is served without an LDS bound.  A thread reads back only what the barrier before it has made visible.
struct AttnQ1Args {
    const float* q;        // [B][H][D] through qsb, qsh
    const float* k;        // [B][H][Nk][D] through ksb, ksh, ksn
    const float* v;
    const float* o_in;     // backward: the forward's o, through osb, osh
    const float* d_o;      // through osb, osh
    float* o;
    float* p;              // [B][H][Nk] contiguous
    float* dq;
    float* dk;
    float* dv;
    long long qsb, qsh, ksb, ksh, ksn, vsb, vsh, vsn, osb, osh;
    int H, Nk, D;
    float scale;
};

constexpr int Q1_THR = 256, Q1_GROUPS = Q1_THR / 16;

template <int V>
struct Q1Frag {
    static constexpr int T = KANVIT_ATTN_X_MAX_D / (16 * V);
    float f[T][V];
};

template <int V>
__device__ __forceinline__ void q1_zero(Q1Frag<V>& r) {
#pragma unroll
    for (int t = 0; t < Q1Frag<V>::T; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) r.f[t][e] = 0.0f;
}

// the lane's columns of one row (zero past D)
template <int V>
__device__ __forceinline__ void q1_load(Q1Frag<V>& r, const float* __restrict__ row, int sub, int D) {
#pragma unroll
    for (int t = 0; t < Q1Frag<V>::T; ++t) {
        const int c = (t * 16 + sub) * V;
        if (c < D) {
            if constexpr (V == 4) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(row + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) r.f[t][e] = u[e];
            } else if constexpr (V == 2) {
                const float2 u = *reinterpret_cast<const float2*>(row + c);
                r.f[t][0] = u.x;
                r.f[t][1] = u.y;
            } else {
                r.f[t][0] = row[c];
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) r.f[t][e] = 0.0f;
        }
    }
}

// row[c] = mul * r for the lane's columns
template <int V>
__device__ __forceinline__ void q1_store(float* __restrict__ row, const Q1Frag<V>& r, float mul, int sub, int D) {
#pragma unroll
    for (int t = 0; t < Q1Frag<V>::T; ++t) {
        const int c = (t * 16 + sub) * V;
        if (c < D) {
            if constexpr (V == 4) {
                const f32x4 u = {mul * r.f[t][0], mul * r.f[t][1], mul * r.f[t][2], mul * r.f[t][3]};
                *reinterpret_cast<f32x4*>(row + c) = u;
            } else if constexpr (V == 2) {
                *reinterpret_cast<float2*>(row + c) = make_float2(mul * r.f[t][0], mul * r.f[t][1]);
            } else {
                row[c] = mul * r.f[t][0];
            }
        }
    }
}

// sum over d of a * b, the same value in all 16 lanes of the group
template <int V>
__device__ __forceinline__ float q1_dot(const Q1Frag<V>& a, const Q1Frag<V>& b) {
    float s = 0.0f;
#pragma unroll
    for (int t = 0; t < Q1Frag<V>::T; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) s = fmaf(a.f[t][e], b.f[t][e], s);
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    return s;
}

template <int V>
__device__ __forceinline__ void q1_axpy(Q1Frag<V>& acc, float a, const Q1Frag<V>& x) {
#pragma unroll
    for (int t = 0; t < Q1Frag<V>::T; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) acc.f[t][e] = fmaf(a, x.f[t][e], acc.f[t][e]);
}

// out[c] = mul * sum over the 16 lane groups, in group order, of their partial rows (red: [Q1_GROUPS][KANVIT_ATTN_X_MAX_D])
template <int V>
__device__ __forceinline__ void q1_reduce_groups(float* __restrict__ red, const Q1Frag<V>& acc, float* __restrict__ out, float mul,
                                                 int tid, int D) {
    const int sub = tid & 15, grp = tid >> 4;
#pragma unroll
    for (int t = 0; t < Q1Frag<V>::T; ++t) {
        const int c = (t * 16 + sub) * V;
        if (c < D) {
#pragma unroll
            for (int e = 0; e < V; ++e) red[grp * KANVIT_ATTN_X_MAX_D + c + e] = acc.f[t][e];
        }
    }
    __syncthreads();
    if (tid < D) {
        float s = 0.0f;
#pragma unroll
        for (int g = 0; g < Q1_GROUPS; ++g) s += red[g * KANVIT_ATTN_X_MAX_D + tid];
        out[tid] = mul * s;
    }
}

// maximum (IS_MAX) or sum of one value per thread over the work-group, the same bits in every thread; wred: [Q1_THR / 64]
template <bool IS_MAX>
__device__ __forceinline__ float q1_block_reduce(float x, float* __restrict__ wred, int tid) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float y = __shfl_xor(x, m);
        x = IS_MAX ? fmaxf(x, y) : x + y;
    }
    __syncthreads();                 // the previous use of wred is over
    if ((tid & 63) == 0) wred[tid >> 6] = x;
    __syncthreads();
    float r = wred[0];
#pragma unroll
    for (int w = 1; w < Q1_THR / 64; ++w) r = IS_MAX ? fmaxf(r, wred[w]) : r + wred[w];
    return r;
}

template <int V>
__global__ __launch_bounds__(Q1_THR) void attn_q1_fwd_kernel(const AttnQ1Args a) {
    __shared__ float red[Q1_GROUPS * KANVIT_ATTN_X_MAX_D];
    __shared__ float wred[Q1_THR / 64];
    const int tid = threadIdx.x, sub = tid & 15, grp = tid >> 4;
    const long long bh = blockIdx.x, bi = bh / a.H, hi = bh - bi * a.H;
    const int D = a.D, Nk = a.Nk;
    const float* kb = a.k + bi * a.ksb + hi * a.ksh;
    const float* vb = a.v + bi * a.vsb + hi * a.vsh;
    float* pb = a.p + bh * Nk;

    Q1Frag<V> qf;
    q1_load<V>(qf, a.q + bi * a.qsb + hi * a.qsh, sub, D);

    // scores: s_j = scale q.k_j, kept in p; the maximum over the keys
    float mx = -INFINITY;
    for (int j = grp; j < Nk; j += Q1_GROUPS) {
        Q1Frag<V> kf;
        q1_load<V>(kf, kb + (long long)j * a.ksn, sub, D);
        const float s = a.scale * q1_dot<V>(qf, kf);
        if (sub == 0) pb[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = q1_block_reduce<true>(mx, wred, tid);      // its barriers also publish the scores

    float sum = 0.0f;
    for (int j = tid; j < Nk; j += Q1_THR) {
        const float e = expf(pb[j] - mx);
        pb[j] = e;
        sum += e;
    }
    sum = q1_block_reduce<false>(sum, wred, tid);   // >= 1: the key of the maximum contributes exp(0)
    const float inv = 1.0f / sum;

    Q1Frag<V> oacc;
    q1_zero<V>(oacc);
    for (int j = grp; j < Nk; j += Q1_GROUPS) {
        Q1Frag<V> vf;
        q1_load<V>(vf, vb + (long long)j * a.vsn, sub, D);
        q1_axpy<V>(oacc, pb[j] * inv, vf);
    }
    q1_reduce_groups<V>(red, oacc, a.o + bi * a.osb + hi * a.osh, 1.0f, tid, D);      // its barrier: every read of exp(s - max) is done
    for (int j = tid; j < Nk; j += Q1_THR) pb[j] *= inv;                             // the thread that wrote exp(s - max)[j]
}

// one pass: dP_j = do.v_j, ds_j = p_j (dP_j - delta) with delta = sum_j p_j dP_j = do.o, dv_j = p_j do, dk_j = scale ds_j q,
// dq = scale sum_j ds_j k_j
template <int V>
__global__ __launch_bounds__(Q1_THR) void attn_q1_bwd_kernel(const AttnQ1Args a) {
    __shared__ float red[Q1_GROUPS * KANVIT_ATTN_X_MAX_D];
    const int tid = threadIdx.x, sub = tid & 15, grp = tid >> 4;
    const long long bh = blockIdx.x, bi = bh / a.H, hi = bh - bi * a.H;
    const int D = a.D, Nk = a.Nk;
    const float* kb = a.k + bi * a.ksb + hi * a.ksh;
    const float* vb = a.v + bi * a.vsb + hi * a.vsh;
    float* dkb = a.dk + bi * a.ksb + hi * a.ksh;
    float* dvb = a.dv + bi * a.vsb + hi * a.vsh;
    const float* pb = a.p + bh * Nk;

    Q1Frag<V> qf, dof, of;
    q1_load<V>(qf, a.q + bi * a.qsb + hi * a.qsh, sub, D);
    q1_load<V>(dof, a.d_o + bi * a.osb + hi * a.osh, sub, D);
    q1_load<V>(of, a.o_in + bi * a.osb + hi * a.osh, sub, D);
    const float delta = q1_dot<V>(dof, of);

    Q1Frag<V> dqacc;
    q1_zero<V>(dqacc);
    for (int j = grp; j < Nk; j += Q1_GROUPS) {
        Q1Frag<V> kf, vf;
        q1_load<V>(vf, vb + (long long)j * a.vsn, sub, D);
        q1_load<V>(kf, kb + (long long)j * a.ksn, sub, D);
        const float pj = pb[j];
        const float ds = pj * (q1_dot<V>(dof, vf) - delta);
        q1_store<V>(dvb + (long long)j * a.vsn, dof, pj, sub, D);
        q1_store<V>(dkb + (long long)j * a.ksn, qf, a.scale * ds, sub, D);
        q1_axpy<V>(dqacc, ds, kf);
    }
    q1_reduce_groups<V>(red, dqacc, a.dq + bi * a.qsb + hi * a.qsh, a.scale, tid, D);
}

int q1_check(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const char* who) {
    if (!d || !e) return kv_fail(KANVIT_EINVAL, "%s: null descriptor", who);
    if (d->B < 0 || d->H < 1 || e->Nk < 1 || d->D < 1) return kv_fail(KANVIT_EINVAL, "%s: bad sizes", who);
    if (d->N != 1) return kv_fail(KANVIT_EINVAL, "%s: q_len=%d, this entry takes ONE query per head (kanvit_attn_x_* take any)", who, d->N);
    if (d->D > KANVIT_ATTN_X_MAX_D || (d->D & 1)) return kv_fail(KANVIT_EINVAL, "%s: D=%d must be even and <= %d", who, d->D, KANVIT_ATTN_X_MAX_D);
    if ((long long)d->B * d->H > 0x7fffffffLL) return kv_fail(KANVIT_EINVAL, "%s: B*H too large", who);
    if (!(d->scale == d->scale) || d->scale - d->scale != 0.0f) return kv_fail(KANVIT_EINVAL, "%s: scale must be finite", who);
    if (d->causal || e->mask) return kv_fail(KANVIT_EINVAL, "%s: no causal / mask form (kanvit_attn_x_* have them)", who);
    if (d->flags) return kv_fail(KANVIT_EINVAL, "%s: flags=%d: one mode, exact fp32 (KANVIT_FLAG_BF16_MFMA is not taken; pass no flag)", who, d->flags);
    return 0;
}

AttnQ1Args q1_args(const kanvit_attn_desc* d, const kanvit_attn_ext* e) {
    AttnQ1Args a{};
    a.H = d->H; a.Nk = e->Nk; a.D = d->D; a.scale = d->scale;
    a.qsb = d->q_stride_b; a.qsh = d->q_stride_h;
    a.ksb = d->k_stride_b; a.ksh = d->k_stride_h; a.ksn = d->k_stride_n;
    a.vsb = d->v_stride_b; a.vsh = d->v_stride_h; a.vsn = d->v_stride_n;
    a.osb = d->o_stride_b; a.osh = d->o_stride_h;
    return a;
}

// widest row piece every operand allows: 4 floats (16-byte rows), 2 (D is even: 8-byte rows) or 1
int q1_width(const AttnQ1Args& a, std::initializer_list<const void*> ptrs) {
    long long m = a.D;
    for (long long sd : {a.qsb, a.qsh, a.ksb, a.ksh, a.ksn, a.vsb, a.vsh, a.vsn, a.osb, a.osh}) m |= sd;
    uintptr_t pm = 0;
    for (const void* p : ptrs) pm |= (uintptr_t)p;
    if (m % 4 == 0 && pm % 16 == 0) return 4;
    if (m % 2 == 0 && pm % 8 == 0) return 2;
    return 1;
}

}  // namespace

extern "C" {

int kanvit_attn_q1_fwd(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const float* q, const float* k, const float* v, float* o,
                       float* p, void* stream) {
    if (int rc = q1_check(d, e, "kanvit_attn_q1_fwd")) return rc;
    if (d->B == 0) return 0;
    if (!q || !k || !v || !o || !p) return kv_fail(KANVIT_EINVAL, "kanvit_attn_q1_fwd: null q/k/v/o/p");
    AttnQ1Args a = q1_args(d, e);
    a.q = q; a.k = k; a.v = v; a.o = o; a.p = p;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(d->B * d->H));
    switch (q1_width(a, {q, k, v})) {
        case 4: hipLaunchKernelGGL(attn_q1_fwd_kernel<4>, grid, dim3(Q1_THR), 0, st, a); break;
        case 2: hipLaunchKernelGGL(attn_q1_fwd_kernel<2>, grid, dim3(Q1_THR), 0, st, a); break;
        default: hipLaunchKernelGGL(attn_q1_fwd_kernel<1>, grid, dim3(Q1_THR), 0, st, a); break;
    }
    KV_LAUNCH_CHECK("attn_q1_fwd_kernel");
    return 0;
}

int kanvit_attn_q1_bwd(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const float* q, const float* k, const float* v, const float* o,
                       const float* p, const float* d_o, float* dq, float* dk, float* dv, void* stream) {
    if (int rc = q1_check(d, e, "kanvit_attn_q1_bwd")) return rc;
    if (d->B == 0) return 0;
    if (!q || !k || !v || !o || !p || !d_o || !dq || !dk || !dv) return kv_fail(KANVIT_EINVAL, "kanvit_attn_q1_bwd: null argument");
    AttnQ1Args a = q1_args(d, e);
    a.q = q; a.k = k; a.v = v; a.o_in = o; a.p = const_cast<float*>(p); a.d_o = d_o; a.dq = dq; a.dk = dk; a.dv = dv;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(d->B * d->H));
    switch (q1_width(a, {q, k, v, o, d_o, dq, dk, dv})) {
        case 4: hipLaunchKernelGGL(attn_q1_bwd_kernel<4>, grid, dim3(Q1_THR), 0, st, a); break;
        case 2: hipLaunchKernelGGL(attn_q1_bwd_kernel<2>, grid, dim3(Q1_THR), 0, st, a); break;
        default: hipLaunchKernelGGL(attn_q1_bwd_kernel<1>, grid, dim3(Q1_THR), 0, st, a); break;
    }
    KV_LAUNCH_CHECK("attn_q1_bwd_kernel");
    return 0;
}

int kanvit_attn_x_fwd(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const float* q, const float* k, const float* v, float* o,
                      float* lse, void* stream) {
    if (int rc = x_check(d, e, "kanvit_attn_x_fwd")) return rc;
    if (!q || !k || !v || !o) return kv_fail(KANVIT_EINVAL, "kanvit_attn_x_fwd: null q/k/v/o");
    if (d->B == 0) return 0;
    AttnXArgs a = x_args(d, e);
    a.q = q; a.k = k; a.v = v; a.out = o; a.lse = lse;
    a.vec = a.vec && (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0);
    hipStream_t st = (hipStream_t)stream;
    if (d->flags & KANVIT_FLAG_BF16_MFMA) return d->D <= 32 ? xb_launch_fwd<1>(a, st) : xb_launch_fwd<2>(a, st);     // x_check: D <= 64
    return d->D <= 32 ? x_launch_fwd<1>(a, st) : d->D <= 64 ? x_launch_fwd<2>(a, st) : d->D <= 96 ? x_launch_fwd<3>(a, st) : x_launch_fwd<4>(a, st);
}

size_t kanvit_attn_x_bwd_workspace(const kanvit_attn_desc* d, const kanvit_attn_ext* e) {
    if (!d || !e || d->B < 0 || d->H < 1 || d->N < 1) return 0;
    return (sizeof(float) * (size_t)d->B * d->H * d->N + 15) / 16 * 16;         // rowsum(dO*O), "D" of utils.py:286
}

int kanvit_attn_x_bwd(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const float* q, const float* k, const float* v, const float* o,
                      const float* lse, const float* d_o, float* dq, float* dk, float* dv, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (int rc = x_check(d, e, "kanvit_attn_x_bwd")) return rc;
    if (!q || !k || !v || !o || !lse || !d_o || !dq || !dk || !dv) return kv_fail(KANVIT_EINVAL, "kanvit_attn_x_bwd: null argument");
    if (d->B == 0) return 0;
    const size_t need = kanvit_attn_x_bwd_workspace(d, e);
    if (!workspace || workspace_bytes < need) return kv_fail(KANVIT_ENOMEM, "kanvit_attn_x_bwd: workspace %zu bytes < required %zu", workspace_bytes, need);
    AttnXArgs a = x_args(d, e);
    a.q = q; a.k = k; a.v = v; a.o = o; a.lse_in = lse; a.d_o = d_o;
    a.dq = dq; a.dk = dk; a.dv = dv; a.delta = (float*)workspace; a.delta_in = (const float*)workspace;
    a.vec = a.vec && (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)d_o) % 16 == 0);
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)d->B * d->H * d->N;
    hipLaunchKernelGGL(attn_x_delta_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, a);
    KV_LAUNCH_CHECK("attn_x_delta_kernel");
    if (d->flags & KANVIT_FLAG_BF16_MFMA) return d->D <= 32 ? xb_launch_bwd<1>(a, st) : xb_launch_bwd<2>(a, st);
    return d->D <= 32 ? x_launch_bwd<1>(a, st) : d->D <= 64 ? x_launch_bwd<2>(a, st) : d->D <= 96 ? x_launch_bwd<3>(a, st) : x_launch_bwd<4>(a, st);
}

}  // extern "C"
