// Soft-target cross-entropy, forward and gradient in one walk (ops.soft_cross_entropy): the target of row b is
//     t_c = (1 - eps) (w [c == y1] + (1 - w) [c == y2]) + eps / C        (label smoothing eps; Mixup / CutMix pair (y1, y2, w))
// and with m = max z, s = sum exp(z - m), p = exp(z - m) / s:
//     loss_b = log s + sum_c t_c (m - z_c)        (= lse(z) - t.z because sum t = 1; every term is >= 0: nothing cancels)
//     dz_bc  = (p_c - t_c) * (1 / B)
// One wave per row with the lane on the class index, as metrics_update_kernel (metrics.hip) walks it: max, then sum exp and sum
// (m - z) together, then the gradient.  A row's bits depend on the row alone (fixed lane assignment, fixed xor-shuffle tree); 1 / B is
// rounded once on the host.  The mean is soft_ce_mean_kernel: one work-group, thread t adds rows t, t + 256, ... in order, then a fixed
// LDS tree.
#include "../../include/kanvit.h"
#include "kanvit_common.h"

namespace {

constexpr int SC_ROWS = 4, SC_THREADS = 64 * SC_ROWS;

struct SoftCeArgs {
    const float* logits;
    const long long* y1;
    const long long* y2;
    const float* w;
    float* loss_rows;
    float* dlogits;
    float* loss;
    long long ld, B;
    int C;
    float eps, inv_B;
};

__global__ __launch_bounds__(SC_THREADS) void soft_ce_kernel(const SoftCeArgs a) {
    const int lane = threadIdx.x & 63, C = a.C;
    const long long row = (long long)blockIdx.x * SC_ROWS + (threadIdx.x >> 6);
    if (row >= a.B) return;                              // a whole wave at once; the kernel has no barrier
    const float* z = a.logits + row * a.ld;
    float* dz = a.dlogits + row * C;
    const long long l1 = a.y1[row], l2 = a.y2 ? a.y2[row] : l1;
    const float w = a.w ? a.w[row] : 1.f;
    if (l1 < 0 || l1 >= C || l2 < 0 || l2 >= C) {        // a label outside [0, C) is never an index: the row counts 0, its gradient is 0
        for (int c = lane; c < C; c += 64) dz[c] = 0.f;
        if (lane == 0) a.loss_rows[row] = 0.f;
        return;
    }
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, z[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float s = 0.f, d = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float zc = z[c];
        s += expf(zc - m);
        d += m - zc;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        d += __shfl_xor(d, o);
    }
    const float keep = 1.f - a.eps, u = a.eps / (float)C;
    const float t1 = keep * w, t2 = keep * (1.f - w);
    if (lane == 0) a.loss_rows[row] = logf(s) + (t1 * (m - z[l1]) + t2 * (m - z[l2])) + u * d;
    const float inv_s = 1.f / s;
    for (int c = lane; c < C; c += 64) {
        const float t = u + (c == l1 ? t1 : 0.f) + (c == l2 ? t2 : 0.f);
        dz[c] = (expf(z[c] - m) * inv_s - t) * a.inv_B;
    }
}

// The ordered sum of rows[0 .. n) by one work-group of 256 threads (valid in thread 0): thread t adds rows t, t + 256, ... in order,
// then a fixed LDS tree.  soft_ce_mean_kernel's sum, and mae_mean_kernel's (mae.hip).
__device__ __forceinline__ float sc_ordered_sum(const float* rows, long long n) {
    __shared__ float part[256];
    float s = 0.f;
    for (long long r = threadIdx.x; r < n; r += 256) s += rows[r];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(256) void soft_ce_mean_kernel(const SoftCeArgs a) {
    const float s = sc_ordered_sum(a.loss_rows, a.B);
    if (threadIdx.x == 0) a.loss[0] = s / (float)a.B;
}

}  // namespace

extern "C" {

int kanvit_soft_ce(const float* logits, int64_t ld, const int64_t* y1, const int64_t* y2, const float* w, int64_t B, int C, float eps,
                   float* loss_rows, float* dlogits, float* loss, void* stream) {
    if (C < 2) return kv_fail(KANVIT_EINVAL, "kanvit_soft_ce: C=%d: at least two classes", C);
    if (B < 1) return kv_fail(KANVIT_EINVAL, "kanvit_soft_ce: B=%lld: at least one row", (long long)B);
    if (ld < C) return kv_fail(KANVIT_EINVAL, "kanvit_soft_ce: row stride ld=%lld is below C=%d", (long long)ld, C);
    if (!(eps >= 0.f && eps < 1.f)) return kv_fail(KANVIT_EINVAL, "kanvit_soft_ce: eps=%g must be in [0, 1)", (double)eps);
    if (!logits || !y1 || !loss_rows || !dlogits || !loss) return kv_fail(KANVIT_EINVAL, "kanvit_soft_ce: null logits/y1/loss_rows/dlogits/loss");
    if ((y2 == nullptr) != (w == nullptr))
        return kv_fail(KANVIT_EINVAL, "kanvit_soft_ce: %s without %s (y2 and w come together)", y2 ? "y2" : "w", y2 ? "w" : "y2");
    if ((B + SC_ROWS - 1) / SC_ROWS > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "kanvit_soft_ce: B=%lld: too many rows for one launch", (long long)B);
    if ((uintptr_t)logits & 3 || (uintptr_t)y1 & 7 || (uintptr_t)y2 & 7 || (uintptr_t)w & 3 || (uintptr_t)loss_rows & 3 || (uintptr_t)dlogits & 3 ||
        (uintptr_t)loss & 3)
        return kv_fail(KANVIT_EINVAL, "kanvit_soft_ce: a pointer is not aligned to its element size");
    SoftCeArgs a;
    a.logits = logits;
    a.y1 = (const long long*)y1;
    a.y2 = (const long long*)y2;
    a.w = w;
    a.loss_rows = loss_rows;
    a.dlogits = dlogits;
    a.loss = loss;
    a.ld = ld, a.B = B, a.C = C, a.eps = eps, a.inv_B = 1.f / (float)B;
    hipLaunchKernelGGL(soft_ce_kernel, dim3((unsigned)((B + SC_ROWS - 1) / SC_ROWS)), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("soft_ce_kernel");
    hipLaunchKernelGGL(soft_ce_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("soft_ce_mean_kernel");
    return 0;
}

}  // extern "C"

// masked-autoencoder pretraining: token restore and the masked-patch loss share this unit (and sc_ordered_sum)
#include "mae.hip"
