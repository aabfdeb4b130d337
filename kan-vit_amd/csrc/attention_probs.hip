// Attention probabilities: p[b, h, i, :] = softmax_j(scale * q[b, h, i, :] . k[b, h, j, :]) for the first `rows` queries of every
// (batch, head) -- the matrix the fused attention kernels never materialise (they keep o and the row log-sum-exp only).  A
// diagnostic (attention maps, attention rollout), not on any training path: fp32 on the vector pipe, one kernel, one mode.
//
// Domain and semantics are kanvit_attn_x_fwd's (csrc/attention_x.hip): independent query / key lengths of any size, D even and
// <= KANVIT_ATTN_X_MAX_D, q and k read through the descriptor's strides (the packed [B, N, 3, H, D] views are read in place), a byte
// mask with four strides (0 broadcasts), `causal` (key j > query i dead, k_len <= q_len).  A position is dead when causal or the
// mask says so; a dead position gets exactly 0.0 and a query with no live key an all-zero row (the counterpart of o = 0,
// lse = -FLT_MAX).
//
// Form: a work-group of four waves owns PR_ROWS = 32 consecutive queries of one (batch, head), eight per wave, and walks the keys in
// LDS chunks of 64 rows: lane l of every wave owns key 64*chunk + l, so a wave's store of one query row is 64 consecutive floats.
// The score q . k is a compensated fp32 dot product (Ogita, Rump and Oishi's Dot2: the rounding error of every product, from one
// fma, and of every addition, from TwoSum, is collected in a second fp32 word c), so a score is the pair s + c with an error of a
// few 2^-48 of sum |q_c k_c|.  A plain fmaf chain loses 2^-24 of the running sum per step: at saturated inputs (scores in the
// hundreds, raw sums in the thousands) that alone moved an entry of P by 1.2e-5.  The keys are swept THREE times by the same code:
//   sweep 0   m = max of fl(s + c) over the live keys  (lane-private over its keys, then a butterfly over the wave: exact in any
//             order; softmax does not care which shift near the maximum is taken, only that a row uses one)
//   sweep 1   l = sum of e_j = exp2(((s_j - m) + c_j) * scale * log2 e) over the live keys (lane-private in key order, then the butterfly)
//   sweep 2   p_j = e_j * (1 / l), stored
// Recomputing instead of parking raw scores in p keeps p write-only (no read of global memory the kernel itself wrote), and taking
// the FINAL maximum before the first exponential -- not a running one -- makes the e_j of sweep 2 bit for bit the terms summed in
// sweep 1, so a row sums to 1 within the error of one fp32 sum and one multiplication.  (s - m) is formed before the multiplication
// by scale * log2 e: the difference of two close scores is exact, so a saturated row keeps the score's full accuracy.
// No workspace, no atomics.  With a single key chunk (k_len <= 64) the chunk is filled once.
//
// Reproducibility: the value of p[b, h, i, j] is a function of q[b, h, i, :], k[b, h, :, :], the dead positions of row i and
// scale only.  The queries of a wave do not mix (one accumulator, one maximum and one sum per query), the key -> lane assignment
// and the butterfly depend on k_len alone, and the 16-byte and scalar tile fills load the same values: the bits do not depend on
// `rows`, on the other samples or heads of the launch, or on the layout q and k arrive in.
#include "kanvit_common.h"

#include <initializer_list>

namespace {

constexpr int PR_THR = 256;                 // four waves
constexpr int PR_RW = 8;                    // queries per wave
constexpr int PR_ROWS = PR_RW * PR_THR / 64;
constexpr int PR_CH = 64;                   // keys per LDS chunk: one per lane
constexpr float PR_LOG2E = 1.4426950408889634f;

struct AttnProbsArgs {
    const float* q;
    const float* k;
    const unsigned char* mask;      // nonzero = attend; element (b, h, i, j) at mask[b*msb + h*msh + i*msq + j*msk] (0 strides broadcast)
    float* p;
    long long msb, msh, msq, msk;
    long long qsb, qsh, qsn, ksb, ksh, ksn;
    long long psb, psh, psq;
    int H, Nq, Nk, D, causal, rows, ntiles;
    int vec;          // rows are 16-byte aligned pieces (D % 4 == 0, strides % 4 == 0, aligned bases): tile fills use 16-byte loads
    float scale;
};

// dst[rows][ld] <- src rows row0.. (row stride stride_n), zero beyond n_valid rows; columns 0 .. D-1
__device__ __forceinline__ void pr_load_tile(float* __restrict__ dst, int ld, const float* __restrict__ src, long long stride_n, int row0,
                                             int rows, int n_valid, int D, int tid, bool vec) {
    if (vec) {
        const int W4 = D / 4;
        for (int idx = tid; idx < rows * W4; idx += PR_THR) {
            const int r = idx / W4, c = (idx - r * W4) * 4;
            const int n = row0 + r;
            f32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
            if (n < n_valid) t = *reinterpret_cast<const f32x4*>(src + (long long)n * stride_n + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[r * ld + c + e] = t[e];
        }
        return;
    }
    for (int idx = tid; idx < rows * D; idx += PR_THR) {
        const int r = idx / D, c = idx - r * D;
        const int n = row0 + r;
        dst[r * ld + c] = (n < n_valid) ? src[(long long)n * stride_n + c] : 0.0f;
    }
}

__device__ __forceinline__ float pr_wave_max(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s));
    return v;
}

__device__ __forceinline__ float pr_wave_sum(float v) {      // a + b = b + a: every lane ends with the same bits
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// one term of the compensated dot product: s + c += a * b.  The __f*_rn forms keep the compiler from contracting or reassociating
// the error-free transformations.
__device__ __forceinline__ void pr_dot2(float a, float b, float& s, float& c) {
    const float p = __fmul_rn(a, b);
    const float pe = fmaf(a, b, -p);                     // a*b = p + pe exactly
    const float t = __fadd_rn(s, p);
    const float z = __fsub_rn(t, s);
    const float se = __fadd_rn(__fsub_rn(s, __fsub_rn(t, z)), __fsub_rn(p, z));      // s + p = t + se exactly
    s = t;
    c = __fadd_rn(c, __fadd_rn(pe, se));
}

// grid: (batch, head, 32-query tile) flattened, the tile fastest
__global__ __launch_bounds__(PR_THR) void attn_probs_kernel(const AttnProbsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, KS = D + 1;                       // D is even: an odd row stride, lane l reads bank (l*KS + c) % 64 -- no conflict
    float* Q_s = smem;                                   // [PR_ROWS][D]: 8-byte aligned pairs (D is even)
    float* K_s = smem + PR_ROWS * D;                     // [PR_CH][KS]
    const long long bh = blockIdx.x / a.ntiles;
    const int tile = (int)(blockIdx.x - bh * a.ntiles);
    const long long bi = bh / a.H, hi = bh - bi * a.H;
    const float* qb = a.q + bi * a.qsb + hi * a.qsh;
    const float* kb = a.k + bi * a.ksb + hi * a.ksh;
    float* pb = a.p + bi * a.psb + hi * a.psh;
    const unsigned char* mb = a.mask ? a.mask + bi * a.msb + hi * a.msh : nullptr;

    const int row0 = tile * PR_ROWS + wave * PR_RW;      // this wave's first query
    const bool active = row0 < a.rows;                   // wave-uniform; an idle wave still fills tiles and meets the barriers
    const float sc2 = a.scale * PR_LOG2E;
    const int nch = (int)(((long long)a.Nk + PR_CH - 1) / PR_CH);

    pr_load_tile(Q_s, D, qb, a.qsn, tile * PR_ROWS, PR_ROWS, a.Nq, D, tid, a.vec);      // visible after the first chunk's barrier

    float mx[PR_RW], sum[PR_RW], inv[PR_RW];
#pragma unroll
    for (int r = 0; r < PR_RW; ++r) {
        mx[r] = -INFINITY;
        sum[r] = 0.0f;
        inv[r] = 0.0f;
    }
    const float* qw = Q_s + wave * PR_RW * D;
    const float* kp = K_s + lane * KS;

#pragma unroll 1
    for (int sweep = 0; sweep < 3; ++sweep) {
#pragma unroll 1
        for (int ch = 0; ch < nch; ++ch) {
            if (sweep == 0 || nch > 1) {
                __syncthreads();                         // every wave is done with the previous chunk
                pr_load_tile(K_s, KS, kb, a.ksn, ch * PR_CH, PR_CH, a.Nk, D, tid, a.vec);
                __syncthreads();
            }
            if (!active) continue;
            const int key = ch * PR_CH + lane;
            // dead positions of this lane's key, a bit per query; the mask bytes are read before the scores are formed
            unsigned dead = 0;
#pragma unroll
            for (int r = 0; r < PR_RW; ++r) {
                const int qi = row0 + r;
                bool d = key >= a.Nk || (a.causal && key > qi);
                if (!d && mb) {
                    const int qc = qi < a.Nq ? qi : a.Nq - 1;
                    d = mb[(long long)qc * a.msq + (long long)key * a.msk] == 0;
                }
                dead |= (d ? 1u : 0u) << r;
            }
            float s[PR_RW], cs[PR_RW];                   // the score is s + cs
#pragma unroll
            for (int r = 0; r < PR_RW; ++r) {
                s[r] = 0.0f;
                cs[r] = 0.0f;
            }
#pragma unroll 1
            for (int c = 0; c < D; c += 2) {
                const float k0 = kp[c], k1 = kp[c + 1];
#pragma unroll
                for (int r = 0; r < PR_RW; ++r) {
                    const float2 q2 = *reinterpret_cast<const float2*>(qw + r * D + c);      // wave-uniform address: an LDS broadcast
                    pr_dot2(q2.x, k0, s[r], cs[r]);
                    pr_dot2(q2.y, k1, s[r], cs[r]);
                }
            }
            if (sweep == 0) {
#pragma unroll
                for (int r = 0; r < PR_RW; ++r) mx[r] = fmaxf(mx[r], ((dead >> r) & 1u) ? -INFINITY : s[r] + cs[r]);
            } else {
#pragma unroll
                for (int r = 0; r < PR_RW; ++r) {
                    const float e = ((dead >> r) & 1u) ? 0.0f : exp2f(((s[r] - mx[r]) + cs[r]) * sc2);      // select, never multiply
                    if (sweep == 1) {
                        sum[r] += e;
                    } else if (key < a.Nk && row0 + r < a.rows) {
                        pb[(long long)(row0 + r) * a.psq + key] = e * inv[r];
                    }
                }
            }
        }
        if (sweep == 0) {
#pragma unroll
            for (int r = 0; r < PR_RW; ++r) {
                const float m = pr_wave_max(mx[r]);
                mx[r] = (m == -INFINITY) ? 0.0f : m;     // no live key: every e is selected to 0 anyway
            }
        } else if (sweep == 1) {
#pragma unroll
            for (int r = 0; r < PR_RW; ++r) {
                const float l = pr_wave_sum(sum[r]);
                inv[r] = l > 0.0f ? 1.0f / l : 0.0f;     // every key dead: an all-zero row
            }
        }
    }
}

}  // namespace

extern "C" {

int kanvit_attn_probs(const kanvit_attn_desc* d, const kanvit_attn_ext* e, const float* q, const float* k, float* p, int64_t p_stride_b,
                      int64_t p_stride_h, int64_t p_stride_q, int32_t rows, void* stream) {
    const char* who = "kanvit_attn_probs";
    if (!d || !e) return kv_fail(KANVIT_EINVAL, "%s: null descriptor (d and e are both required)", who);
    if (!q || !k || !p) return kv_fail(KANVIT_EINVAL, "%s: null q/k/p", who);
    if (d->B < 1 || d->H < 1 || d->N < 1 || e->Nk < 1)
        return kv_fail(KANVIT_EINVAL, "%s: bad sizes B=%d H=%d N=%d Nk=%d (each must be >= 1)", who, d->B, d->H, d->N, e->Nk);
    if (d->D < 2 || d->D > KANVIT_ATTN_X_MAX_D || (d->D & 1)) return kv_fail(KANVIT_EINVAL, "%s: D=%d must be even and <= %d", who, d->D, KANVIT_ATTN_X_MAX_D);
    if (!(d->scale > 0.0f)) return kv_fail(KANVIT_EINVAL, "%s: scale=%g must be positive", who, (double)d->scale);
    if (d->flags & KANVIT_FLAG_BF16_MFMA)
        return kv_fail(KANVIT_EINVAL, "%s: KANVIT_FLAG_BF16_MFMA is not supported: the map has no bf16 mode (clear the flag)", who);
    if (d->flags) return kv_fail(KANVIT_EINVAL, "%s: flags=%d must be 0", who, d->flags);
    if (d->causal && e->Nk > d->N)
        return kv_fail(KANVIT_EINVAL, "%s: causal with k_len=%d > q_len=%d is ill-defined in the reference (utils.py:169,183: the first k_len - q_len queries see no key)", who, e->Nk, d->N);
    if (rows < 1 || rows > d->N) return kv_fail(KANVIT_EINVAL, "%s: rows=%d must be in [1, N=%d]", who, rows, d->N);
    if (p_stride_q < e->Nk) return kv_fail(KANVIT_EINVAL, "%s: p_stride_q=%lld must be >= Nk=%d", who, (long long)p_stride_q, e->Nk);
    const long long ntiles = ((long long)rows + PR_ROWS - 1) / PR_ROWS;
    const long long blocks = (long long)d->B * d->H * ntiles;
    if (blocks > 0x7fffffffLL) return kv_fail(KANVIT_EINVAL, "%s: B*H*ceil(rows/%d)=%lld work-groups are too many for one launch", who, PR_ROWS, blocks);

    AttnProbsArgs a{};
    a.q = q; a.k = k; a.p = p;
    a.mask = (const unsigned char*)e->mask;
    a.msb = e->mask_stride_b; a.msh = e->mask_stride_h; a.msq = e->mask_stride_q; a.msk = e->mask_stride_k;
    a.qsb = d->q_stride_b; a.qsh = d->q_stride_h; a.qsn = d->q_stride_n;
    a.ksb = d->k_stride_b; a.ksh = d->k_stride_h; a.ksn = d->k_stride_n;
    a.psb = p_stride_b; a.psh = p_stride_h; a.psq = p_stride_q;
    a.H = d->H; a.Nq = d->N; a.Nk = e->Nk; a.D = d->D; a.causal = d->causal; a.rows = rows; a.ntiles = (int)ntiles;
    a.scale = d->scale;
    a.vec = (d->D % 4 == 0) && (((uintptr_t)q | (uintptr_t)k) % 16 == 0);
    for (long long sd : {a.qsb, a.qsh, a.qsn, a.ksb, a.ksh, a.ksn}) a.vec = a.vec && (sd % 4 == 0);
    const size_t lds = sizeof(float) * ((size_t)PR_ROWS * d->D + (size_t)PR_CH * (d->D + 1));      // 48.25 KiB at D = 128
    hipLaunchKernelGGL(attn_probs_kernel, dim3((unsigned)blocks), dim3(PR_THR), lds, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("attn_probs_kernel");
    return 0;
}

}  // extern "C"
