// Epoch metrics (kanvit/metrics.py): accuracy, balanced accuracy, weighted F1 and one-vs-rest ROC-AUC are exact functions of small
// integer tables -- the C x C confusion matrix, and per class the Mann-Whitney pair counts
//     gt_c = #{(i, j): label_i = c, label_j != c, p[i][c] > p[j][c]},   eq_c = the same with ==
// so nothing but C*C + 2*C integers goes to the host, and integer sums make every result independent of the order of the atomics.
//
// metrics_update_kernel: one launch per step.  A work-group takes MU_ROWS consecutive rows, one wave per row; the wave walks its row
// with the lane on the class index (the logits' contiguous axis): max + first argmax, sum of exp(z - max), then p = exp(z - max) / sum,
// MU_COLS classes at a time, written into an LDS tile [class][row] and stored from there with the lane on the ROW index -- probs_t is
// class-major, so those stores are contiguous along n.  A row's arithmetic (which lane adds what, the shuffle tree) depends on nothing
// but the row itself: feeding an epoch in other batch sizes gives the same bits.
// A step's batch is small (128 rows) and the kernel is bound by the latency of a wave's dependent passes over a row, so a wave gets
// ONE row: 16 waves of 16 rows measured 4.5 us per launch at 128 x 100 against 9.4 us for 4 waves with 4 rows each (replayed graph;
// the argmax + softmax launches this replaces: 5.6 us).  16 rows still make 64-byte runs of every class-major store.
#include "../../include/kanvit.h"
#include "kanvit_common.h"

namespace {

constexpr int MU_ROWS = 16, MU_COLS = 64, MU_THREADS = 1024;

struct MetricsUpdateArgs {
    const void* logits;
    const long long* labels;
    float* probs_t;
    int* labels_out;
    int* preds_out;
    unsigned long long* confusion;
    long long ld, B, n0, cap;
    int C;
};

template <bool BF16>
__device__ __forceinline__ float mu_logit(const void* base, long long i) {
    if constexpr (BF16)
        return __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(base)[i] << 16);      // bf16 -> fp32, exact
    else
        return reinterpret_cast<const float*>(base)[i];
}

template <bool BF16>
__global__ __launch_bounds__(MU_THREADS) void metrics_update_kernel(const MetricsUpdateArgs a) {
    __shared__ float tile[MU_COLS][MU_ROWS + 1];         // +1: the waves' column-strided writes and the row-strided reads both miss conflicts
    __shared__ float row_max[MU_ROWS], row_sum[MU_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = a.C;
    const long long row0 = (long long)blockIdx.x * MU_ROWS;
    for (int r = wave; r < MU_ROWS; r += MU_THREADS / 64) {
        const long long row = row0 + r;
        if (row >= a.B) break;
        const long long zb = row * a.ld;
        float m = -INFINITY;
        int am = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {             // ascending c per lane: '>' keeps the first of equal maxima
            const float z = mu_logit<BF16>(a.logits, zb + c);
            if (z > m || am == 0x7fffffff) m = z, am = c;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float m2 = __shfl_xor(m, o);
            const int a2 = __shfl_xor(am, o);
            if (m2 > m || (m2 == m && a2 < am)) m = m2, am = a2;
        }
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += expf(mu_logit<BF16>(a.logits, zb + c) - m);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) {
            row_max[r] = m;
            row_sum[r] = s;
            const long long lab = a.labels[row];
            const bool ok = lab >= 0 && lab < C;         // a label outside [0, C): the row is dropped from every table
            a.labels_out[a.n0 + row] = ok ? (int)lab : -1;
            a.preds_out[a.n0 + row] = am;
            if (ok) atomicAdd(&a.confusion[lab * C + am], 1ull);
        }
    }
    __syncthreads();
    const int rows = (int)(a.B - row0 < MU_ROWS ? a.B - row0 : MU_ROWS);
    for (int c0 = 0; c0 < C; c0 += MU_COLS) {
        const int c = c0 + lane;
        if (c < C)
            for (int r = wave; r < rows; r += MU_THREADS / 64)
                tile[lane][r] = expf(mu_logit<BF16>(a.logits, (row0 + r) * a.ld + c) - row_max[r]) / row_sum[r];
        __syncthreads();
        const int r = threadIdx.x % MU_ROWS;
        if (r < rows)
            for (int cc = threadIdx.x / MU_ROWS; cc < MU_COLS && c0 + cc < C; cc += MU_THREADS / MU_ROWS)
                a.probs_t[(long long)(c0 + cc) * a.cap + a.n0 + row0 + r] = tile[cc][r];
        __syncthreads();
    }
}

// The pair counts.  Three small passes group the positives' own-class probabilities by class (histogram of the labels, one-block
// exclusive scan, scatter through atomic cursors: pos[off[c] .. off[c+1]) = { p[i][c] : label_i = c }, in any order), then
// metrics_pairs_kernel runs one work-group per (class c, tile of AP_TILE samples): a thread keeps AP_PER of the tile's p[j][c] in
// registers (lane on n: contiguous), NaN where sample j is no negative of c (its own class, a dropped row, past n) so that neither
// comparison counts it, and walks the class's positives through LDS in chunks of AP_CHUNK -- every lane reads the same address, a
// broadcast.  32-bit counts per thread (at most AP_PER * n <= 2^30), one reduction per wave, one 64-bit atomic per wave and table.
constexpr int AP_THREADS = 256, AP_PER = 4, AP_TILE = AP_THREADS * AP_PER, AP_CHUNK = 1024;
constexpr long long AP_MAX_N = 1ll << 28;

struct MetricsPairArgs {
    const float* probs_t;
    const int* labels;
    int* hist;          // [C]     samples per class
    int* cursor;        // [C]     scatter cursors, start at off[c]
    int* off;           // [C + 1] exclusive scan of hist
    float* pos;         // [n]     the positives' own-class probabilities, grouped by class
    unsigned long long* counts;
    long long cap;
    int n, C, tiles;
};

__global__ __launch_bounds__(256) void metrics_hist_kernel(const MetricsPairArgs a) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n; i += gridDim.x * 256) {
        const int l = a.labels[i];
        if ((unsigned)l < (unsigned)a.C) atomicAdd(&a.hist[l], 1);
    }
}

__global__ __launch_bounds__(256) void metrics_scan_kernel(const MetricsPairArgs a) {
    __shared__ int part[256];
    const int per = (a.C + 255) / 256, lo = threadIdx.x * per, hi = lo + per < a.C ? lo + per : a.C;
    int s = 0;
    for (int c = lo; c < hi; ++c) s += a.hist[c];
    part[threadIdx.x] = s;
    __syncthreads();
    int base = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) base += part[t];
    for (int c = lo; c < hi; ++c) {
        a.off[c] = base;
        a.cursor[c] = base;
        base += a.hist[c];
    }
    if (threadIdx.x == 255) a.off[a.C] = base;           // the last thread's running sum ends at the total, whatever its own range
}

__global__ __launch_bounds__(256) void metrics_scatter_kernel(const MetricsPairArgs a) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n; i += gridDim.x * 256) {
        const int l = a.labels[i];
        if ((unsigned)l < (unsigned)a.C) a.pos[atomicAdd(&a.cursor[l], 1)] = a.probs_t[(long long)l * a.cap + i];
    }
}

__global__ __launch_bounds__(AP_THREADS) void metrics_pairs_kernel(const MetricsPairArgs a) {
    __shared__ float chunk[AP_CHUNK];
    const int c = blockIdx.x / a.tiles, tile = blockIdx.x - c * a.tiles;
    const int p0 = a.off[c], np = a.off[c + 1] - p0;
    if (np == 0) return;                                 // uniform over the work-group: nobody waits at a barrier
    float x[AP_PER];
#pragma unroll
    for (int e = 0; e < AP_PER; ++e) {
        const int j = tile * AP_TILE + e * AP_THREADS + (int)threadIdx.x;
        const int l = j < a.n ? a.labels[j] : -1;
        x[e] = ((unsigned)l < (unsigned)a.C && l != c) ? a.probs_t[(long long)c * a.cap + j] : __builtin_nanf("");
    }
    unsigned gt = 0, eq = 0;
    for (int k0 = 0; k0 < np; k0 += AP_CHUNK) {
        const int len = np - k0 < AP_CHUNK ? np - k0 : AP_CHUNK;
        __syncthreads();                                 // the previous chunk has been read by every wave
        for (int k = threadIdx.x; k < len; k += AP_THREADS) chunk[k] = a.pos[p0 + k0 + k];
        __syncthreads();
        for (int k = 0; k < len; ++k) {
            const float v = chunk[k];
#pragma unroll
            for (int e = 0; e < AP_PER; ++e) {
                gt += v > x[e] ? 1u : 0u;
                eq += v == x[e] ? 1u : 0u;
            }
        }
    }
    unsigned long long g = gt, q = eq;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        g += __shfl_xor(g, o);
        q += __shfl_xor(q, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (g) atomicAdd(&a.counts[2 * c], g);
        if (q) atomicAdd(&a.counts[2 * c + 1], q);
    }
}

// workspace of the pair counts: hist[C] | cursor[C] | off[C + 1] (int32, rounded up to 16 bytes) | pos[n] (fp32)
size_t ap_table_bytes(int C) { return (((size_t)3 * C + 1) * sizeof(int) + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int kanvit_metrics_update(const void* logits, int logits_bf16, int64_t ld, const int64_t* labels, int64_t B, int C, int64_t n0, int64_t cap,
                          float* probs_t, int32_t* labels_out, int32_t* preds_out, int64_t* confusion, void* stream) {
    if (!logits || !labels || !probs_t || !labels_out || !preds_out || !confusion)
        return kv_fail(KANVIT_EINVAL, "kanvit_metrics_update: null logits/labels/probs_t/labels_out/preds_out/confusion");
    if (logits_bf16 != 0 && logits_bf16 != 1) return kv_fail(KANVIT_EINVAL, "kanvit_metrics_update: logits_bf16=%d is 0 (float32) or 1 (bfloat16)", logits_bf16);
    if (C < 2) return kv_fail(KANVIT_EINVAL, "kanvit_metrics_update: C=%d: at least two classes", C);
    if (B < 1) return kv_fail(KANVIT_EINVAL, "kanvit_metrics_update: B=%lld: at least one row", (long long)B);
    if (ld < C) return kv_fail(KANVIT_EINVAL, "kanvit_metrics_update: row stride ld=%lld is below C=%d", (long long)ld, C);
    if (n0 < 0 || cap < 1 || B > cap || n0 > cap - B)
        return kv_fail(KANVIT_EINVAL, "kanvit_metrics_update: n0=%lld + B=%lld exceeds cap=%lld", (long long)n0, (long long)B, (long long)cap);
    if ((uintptr_t)logits & (logits_bf16 ? 1 : 3) || (uintptr_t)labels & 7 || (uintptr_t)probs_t & 3 || (uintptr_t)labels_out & 3 ||
        (uintptr_t)preds_out & 3 || (uintptr_t)confusion & 7)
        return kv_fail(KANVIT_EINVAL, "kanvit_metrics_update: a pointer is not aligned to its element size");
    MetricsUpdateArgs a;
    a.logits = logits;
    a.labels = (const long long*)labels;
    a.probs_t = probs_t;
    a.labels_out = labels_out;
    a.preds_out = preds_out;
    a.confusion = (unsigned long long*)confusion;
    a.ld = ld, a.B = B, a.n0 = n0, a.cap = cap, a.C = C;
    const unsigned blocks = (unsigned)((B + MU_ROWS - 1) / MU_ROWS);
    if (logits_bf16)
        hipLaunchKernelGGL(metrics_update_kernel<true>, dim3(blocks), dim3(MU_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(metrics_update_kernel<false>, dim3(blocks), dim3(MU_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("metrics_update_kernel");
    return 0;
}

size_t kanvit_metrics_auc_pairs_workspace(int64_t n, int C) {
    if (n < 1 || n > AP_MAX_N || C < 2) return 0;
    return ap_table_bytes(C) + (size_t)n * sizeof(float);
}

int kanvit_metrics_auc_pairs(const float* probs_t, const int32_t* labels, int64_t n, int C, int64_t cap, int64_t* counts, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (!probs_t || !labels || !counts || !workspace) return kv_fail(KANVIT_EINVAL, "kanvit_metrics_auc_pairs: null probs_t/labels/counts/workspace");
    if (C < 2) return kv_fail(KANVIT_EINVAL, "kanvit_metrics_auc_pairs: C=%d: at least two classes", C);
    if (n < 1) return kv_fail(KANVIT_EINVAL, "kanvit_metrics_auc_pairs: n=%lld: at least one sample", (long long)n);
    if (n > cap) return kv_fail(KANVIT_EINVAL, "kanvit_metrics_auc_pairs: n=%lld exceeds cap=%lld", (long long)n, (long long)cap);
    if (n > AP_MAX_N) return kv_fail(KANVIT_EINVAL, "kanvit_metrics_auc_pairs: n=%lld is above 2^28 samples", (long long)n);
    const long long tiles = (n + AP_TILE - 1) / AP_TILE;
    if (tiles * C > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "kanvit_metrics_auc_pairs: n=%lld, C=%d: too many (class, tile) work-groups", (long long)n, C);
    if (workspace_bytes < kanvit_metrics_auc_pairs_workspace(n, C))
        return kv_fail(KANVIT_EINVAL, "kanvit_metrics_auc_pairs: workspace of %zu bytes, %zu needed", workspace_bytes, kanvit_metrics_auc_pairs_workspace(n, C));
    if ((uintptr_t)probs_t & 3 || (uintptr_t)labels & 3 || (uintptr_t)counts & 7 || (uintptr_t)workspace & 15)
        return kv_fail(KANVIT_EINVAL, "kanvit_metrics_auc_pairs: a pointer is not aligned (workspace: 16 bytes)");
    hipStream_t st = (hipStream_t)stream;
    MetricsPairArgs a;
    a.probs_t = probs_t;
    a.labels = labels;
    a.hist = (int*)workspace;
    a.cursor = a.hist + C;
    a.off = a.cursor + C;
    a.pos = (float*)((char*)workspace + ap_table_bytes(C));
    a.counts = (unsigned long long*)counts;
    a.cap = cap, a.n = (int)n, a.C = C, a.tiles = (int)tiles;
    KV_HIP_CHECK(hipMemsetAsync(a.hist, 0, (size_t)C * sizeof(int), st));
    KV_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)C * 2 * sizeof(int64_t), st));
    long long blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(metrics_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    KV_LAUNCH_CHECK("metrics_hist_kernel");
    hipLaunchKernelGGL(metrics_scan_kernel, dim3(1), dim3(256), 0, st, a);
    KV_LAUNCH_CHECK("metrics_scan_kernel");
    hipLaunchKernelGGL(metrics_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    KV_LAUNCH_CHECK("metrics_scatter_kernel");
    hipLaunchKernelGGL(metrics_pairs_kernel, dim3((unsigned)(tiles * C)), dim3(AP_THREADS), 0, st, a);
    KV_LAUNCH_CHECK("metrics_pairs_kernel");
    return 0;
}

}  // extern "C"
