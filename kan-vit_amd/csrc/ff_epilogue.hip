// Backward epilogue of the feed-forward's first Linear + ReLU (reference model.py:25-29): the ReLU mask
// of the incoming gradient and the bias gradient in ONE pass over [M, N].
//     dh[m][n]  = y[m][n] <= 0 ? 0 : dy[m][n]         (what autograd's threshold_backward does for ReLU(inplace) on the saved y)
//     dbias[n]  = sum_m dh[m][n]
// Stock torch runs two passes (threshold_backward: read dy, y, write dh; then sum(0): read dh again -- 12 x 310 MB per ViT-B
// step for the second one).  Here a work-group owns a band of rows x 1024 columns: each thread streams one float4 column group
// down the band (EP_ROWS rows in flight), writes the masked gradient and keeps its four column sums in registers; the bands'
// partial sums go to the workspace and are added in band order by a second, tiny kernel -- deterministic, no float atomics.
// HBM-bound: the sums ride for free on the traffic of the mask pass.  Measured on [25216, 3072] (tools/time_ff_epilogue.py): stock
// 227 us (157 + 60), this 177 us = 930 MB at 5.2 TB/s.  Rejected: whole rows per work-group (up to 4 column groups per thread:
// 224-281 us), 16 rows in flight with 2 work-groups per CU (same time, more registers), 8 work-groups per CU (186 us).
#include "../../include/kanvit.h"
#include "kanvit_common.h"

namespace {

#ifndef EP_ROWS
#define EP_ROWS 8                             // rows in flight per thread (tools/build_variant.sh -DEP_ROWS=4 for A/B timing)
#endif
#ifndef EP_WGS_PER_CU
#define EP_WGS_PER_CU 4
#endif
constexpr int EP_THREADS = 256;
constexpr int EP_COLS = EP_THREADS * 4;       // columns per work-group

// Every byte is touched once: non-temporal loads and stores (measured 185 -> 177 us on [25216, 3072]; stores alone, 187).
// (In the ViT-B step, 30 steps, A/B in one process each: stock epilogue 89.32 ms, this kernel with plain accesses 89.03, loads
// non-temporal 88.89, both 88.80.)
#define EP_LD(p) __builtin_nontemporal_load(p)
#define EP_ST(v, p) __builtin_nontemporal_store(v, p)
__global__ __launch_bounds__(EP_THREADS) void relu_bwd_bias_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                   float* __restrict__ dh, float* __restrict__ part, long long M, int N,
                                                                   long long rows_per_band) {
    const int c = (blockIdx.x * EP_THREADS + threadIdx.x) * 4;
    if (c >= N) return;
    const long long r0 = (long long)blockIdx.y * rows_per_band;
    long long r1 = r0 + rows_per_band;
    if (r1 > M) r1 = M;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    long long r = r0;
    for (; r + EP_ROWS <= r1; r += EP_ROWS) {             // EP_ROWS rows in flight
        f32x4 g[EP_ROWS], a[EP_ROWS];
#pragma unroll
        for (int q = 0; q < EP_ROWS; ++q) {
            g[q] = EP_LD(reinterpret_cast<const f32x4*>(dy + (r + q) * N + c));
            a[q] = EP_LD(reinterpret_cast<const f32x4*>(y + (r + q) * N + c));
        }
#pragma unroll
        for (int q = 0; q < EP_ROWS; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) g[q][e] = a[q][e] <= 0.0f ? 0.0f : g[q][e];      // threshold_backward's own comparison (a NaN activation passes the gradient)
            EP_ST(g[q], reinterpret_cast<f32x4*>(dh + (r + q) * N + c));
            s += g[q];                         // rows added in order
        }
    }
    for (; r < r1; ++r) {
        f32x4 g = *reinterpret_cast<const f32x4*>(dy + r * N + c);
        const f32x4 a = *reinterpret_cast<const f32x4*>(y + r * N + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = a[e] <= 0.0f ? 0.0f : g[e];
        *reinterpret_cast<f32x4*>(dh + r * N + c) = g;
        s += g;
    }
    *reinterpret_cast<f32x4*>(part + (long long)blockIdx.y * N + c) = s;
}

// The same pass on bf16 tensors (torch.autocast: dy, y and dh are bf16; the column sums stay fp32, as torch's
// `dy.sum(0, dtype=float32)`): 8-byte loads of four bf16 per thread, the same 1024 columns per work-group and band partials.
typedef unsigned short ep_u16x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(EP_THREADS) void relu_bwd_bias_bf16_kernel(const unsigned short* __restrict__ dy, const unsigned short* __restrict__ y,
                                                                        unsigned short* __restrict__ dh, float* __restrict__ part, long long M,
                                                                        int N, long long rows_per_band) {
    const int c = (blockIdx.x * EP_THREADS + threadIdx.x) * 4;
    if (c >= N) return;
    const long long r0 = (long long)blockIdx.y * rows_per_band;
    long long r1 = r0 + rows_per_band;
    if (r1 > M) r1 = M;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int RB = 2 * EP_ROWS;                         // rows in flight (half the bytes per row)
    long long r = r0;
    for (; r + RB <= r1; r += RB) {
        ep_u16x4 g[RB], a[RB];
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            g[q] = EP_LD(reinterpret_cast<const ep_u16x4*>(dy + (r + q) * N + c));
            a[q] = EP_LD(reinterpret_cast<const ep_u16x4*>(y + (r + q) * N + c));
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // !(y <= 0) on the bf16 bit pattern (threshold_backward's comparison): positive and not zero, or a NaN of either sign
                const unsigned short yb = a[q][e];
                const bool pos = ((yb & 0x8000u) == 0 && yb != 0) || ((yb & 0x7f80u) == 0x7f80u && (yb & 0x007fu));
                g[q][e] = pos ? g[q][e] : (unsigned short)0;
                s[e] += __builtin_bit_cast(float, (unsigned)g[q][e] << 16);      // rows added in order
            }
            EP_ST(g[q], reinterpret_cast<ep_u16x4*>(dh + (r + q) * N + c));
        }
    }
    for (; r < r1; ++r) {
        ep_u16x4 g = *reinterpret_cast<const ep_u16x4*>(dy + r * N + c);
        const ep_u16x4 a = *reinterpret_cast<const ep_u16x4*>(y + r * N + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned short yb = a[e];
            const bool pos = ((yb & 0x8000u) == 0 && yb != 0) || ((yb & 0x7f80u) == 0x7f80u && (yb & 0x007fu));
            g[e] = pos ? g[e] : (unsigned short)0;
            s[e] += __builtin_bit_cast(float, (unsigned)g[e] << 16);
        }
        *reinterpret_cast<ep_u16x4*>(dh + r * N + c) = g;
    }
    *reinterpret_cast<f32x4*>(part + (long long)blockIdx.y * N + c) = s;
}

// out[c] = sum over the bands of part[band][c], in a fixed order: 32 columns x 8 band groups per work-group (group k adds bands
// k, k + 8, ... with eight loads in flight, then the eight group sums are added in order).  One thread per column walking all
// the bands is a serial chain of ~40 dependent round trips on 12 work-groups -- it took longer than the pass it finishes.
__global__ __launch_bounds__(256) void colsum_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int N, int bands) {
    __shared__ float sub[8][33];
    const int cl = threadIdx.x & 31, k = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float s = 0.0f;
    if (c < N) {
        int w = k;
        for (; w + 56 < bands; w += 64) {
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = part[(long long)(w + 8 * j) * N + c];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += t[j];
        }
        for (; w < bands; w += 8) s += part[(long long)w * N + c];
    }
    sub[k][cl] = s;
    __syncthreads();
    if (k == 0 && c < N) {
        float t = sub[0][cl];
#pragma unroll
        for (int j = 1; j < 8; ++j) t += sub[j][cl];
        out[c] = t;
    }
}

int ep_bands(long long M, int N) {
    const long long gx = (N + EP_COLS - 1) / EP_COLS;
    long long bands = ((long long)EP_WGS_PER_CU * 256 + gx - 1) / gx;          // ~EP_WGS_PER_CU work-groups per CU over the chip
    const long long maxb = (M + 15) / 16;                  // at least 16 rows per band
    if (bands > maxb) bands = maxb;
    if (bands < 1) bands = 1;
    if (bands > 65535) bands = 65535;
    return (int)bands;
}

}  // namespace

extern "C" {

size_t kanvit_relu_bwd_bias_workspace(int64_t M, int N) {
    if (M <= 0 || N <= 0) return 0;
    return sizeof(float) * (size_t)ep_bands(M, N) * (size_t)N;
}

static int relu_bwd_bias_impl(bool bf16, int64_t M, int N, const void* dy, const void* y, void* dh, float* dbias, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (M < 0 || N < 1 || (N & 3)) return kv_fail(KANVIT_EINVAL, "kanvit_relu_bwd_bias: N=%d must be a positive multiple of 4 (M=%lld)", N, (long long)M);
    if (!dbias) return kv_fail(KANVIT_EINVAL, "kanvit_relu_bwd_bias: null dbias");
    hipStream_t st = (hipStream_t)stream;
    if (M == 0) {
        KV_HIP_CHECK(hipMemsetAsync(dbias, 0, sizeof(float) * (size_t)N, st));
        return 0;
    }
    if (!dy || !y || !dh) return kv_fail(KANVIT_EINVAL, "kanvit_relu_bwd_bias: null dy/y/dh");
    if (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)dh) & 15) return kv_fail(KANVIT_EINVAL, "kanvit_relu_bwd_bias: dy / y / dh must be 16-byte aligned");
    const size_t need = kanvit_relu_bwd_bias_workspace(M, N);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))
        return kv_fail(KANVIT_ENOMEM, "kanvit_relu_bwd_bias: workspace %zu bytes < required %zu (or not 16-byte aligned)", workspace_bytes, need);
    const int bands = ep_bands(M, N);
    const long long rpb = (M + bands - 1) / bands;
    dim3 grid((unsigned)((N + EP_COLS - 1) / EP_COLS), (unsigned)((M + rpb - 1) / rpb), 1);
    if (bf16)
        hipLaunchKernelGGL(relu_bwd_bias_bf16_kernel, grid, dim3(EP_THREADS), 0, st, (const unsigned short*)dy, (const unsigned short*)y,
                           (unsigned short*)dh, (float*)workspace, (long long)M, N, rpb);
    else
        hipLaunchKernelGGL(relu_bwd_bias_kernel, grid, dim3(EP_THREADS), 0, st, (const float*)dy, (const float*)y, (float*)dh, (float*)workspace,
                           (long long)M, N, rpb);
    KV_LAUNCH_CHECK("relu_bwd_bias_kernel");
    hipLaunchKernelGGL(colsum_reduce_kernel, dim3((unsigned)((N + 31) / 32)), dim3(256), 0, st, (const float*)workspace, dbias, N, (int)grid.y);
    KV_LAUNCH_CHECK("colsum_reduce_kernel");
    return 0;
}

int kanvit_relu_bwd_bias(int64_t M, int N, const float* dy, const float* y, float* dh, float* dbias, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return relu_bwd_bias_impl(false, M, N, dy, y, dh, dbias, workspace, workspace_bytes, stream);
}

int kanvit_relu_bwd_bias_bf16(int64_t M, int N, const void* dy, const void* y, void* dh, float* dbias, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return relu_bwd_bias_impl(true, M, N, dy, y, dh, dbias, workspace, workspace_bytes, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// The feed-forward's other helper pass, kanvit_split3_bf16 (kanvit/dense.py calls both): the two small passes share this translation
// unit, which keeps the build at the 19 parallel compiles tests/test_attention_map_cpu.py counts.
// fp32 -> three-term bf16 split images for the "bf16x3" feed-forward mode (kanvit/dense.py):
//     v = hi + lo + O(2^-17 |v|),  hi = bf16(v),  lo = bf16(v - hi)
// A product a.b is then formed as a_hi.b_hi + a_hi.b_lo + a_lo.b_hi on the bf16 matrix cores with fp32 accumulation (the
// a_lo.b_lo term, ~2^-16 relative, is dropped): one bf16 GEMM over a K axis that is three times as long.  This kernel writes
// the K-concatenated operand image in one pass, optionally fusing what sits between two GEMMs of the reference's
// Linear -> ReLU -> Linear block (model.py:25-29): + bias, ReLU, or the ReLU mask of the backward pass.
//   pattern 0 ("A"): out[m] = [ hi | hi | lo ]        pattern 1 ("B"): out[m] = [ hi | lo | hi ]
// so that  A-image . B-image^T  =  hi.hi + hi.lo + lo.hi.
namespace {

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned short f2bf(float v) {      // round to nearest even
    const __bf16 b = (__bf16)v;
    return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

// one thread = 8 consecutive columns of one row
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                     const unsigned short* __restrict__ mask, long long mask_ld,
                                                     unsigned short* __restrict__ out, long long M, int K, int relu, int pattern) {
    const int k8 = K / 8;
    const long long total = M * k8;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long m = idx / k8;
        const int c = (int)(idx - m * k8) * 8;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(x + m * K + c);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(x + m * K + c + 4);
        float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        if (bias) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += bias[c + e];
        }
        if (relu) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.0f);
        }
        if (mask) {             // keep where the saved activation (its hi part) is positive: ReLU backward
            const u32x4_t mk = *reinterpret_cast<const u32x4_t*>(mask + m * mask_ld + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned short h = (unsigned short)((mk[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                if (!(bf2f(h) > 0.0f)) v[e] = 0.0f;
            }
        }
        unsigned short hi[8], lo[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hi[e] = f2bf(v[e]);
            lo[e] = f2bf(v[e] - bf2f(hi[e]));
        }
        const u32x4_t H = {(unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16),
                           (unsigned)hi[4] | ((unsigned)hi[5] << 16), (unsigned)hi[6] | ((unsigned)hi[7] << 16)};
        const u32x4_t L = {(unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16),
                           (unsigned)lo[4] | ((unsigned)lo[5] << 16), (unsigned)lo[6] | ((unsigned)lo[7] << 16)};
        unsigned short* o = out + m * 3 * K + c;
        *reinterpret_cast<u32x4_t*>(o) = H;
        *reinterpret_cast<u32x4_t*>(o + K) = pattern ? L : H;
        *reinterpret_cast<u32x4_t*>(o + 2 * K) = pattern ? H : L;
    }
}

}  // namespace

extern "C" {

int kanvit_split3_bf16(int64_t M, int K, const float* x, const float* bias, int relu, const void* mask_hi, int64_t mask_ld,
                       void* out, int pattern, void* stream) {
    if (M < 0 || K < 8 || (K & 7)) return kv_fail(KANVIT_EINVAL, "kanvit_split3_bf16: K=%d must be a positive multiple of 8", K);
    if (M == 0) return 0;
    if (!x || !out) return kv_fail(KANVIT_EINVAL, "kanvit_split3_bf16: null x/out");
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)(mask_hi ? mask_hi : out)) & 15 || (mask_hi && (mask_ld & 7)))
        return kv_fail(KANVIT_EINVAL, "kanvit_split3_bf16: pointers must be 16-byte aligned (mask_ld a multiple of 8)");
    const long long total = (long long)M * (K / 8);
    long long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(split3_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, bias,
                       (const unsigned short*)mask_hi, (long long)mask_ld, (unsigned short*)out, (long long)M, K, relu, pattern ? 1 : 0);
    KV_LAUNCH_CHECK("split3_kernel");
    return 0;
}

}  // extern "C"
