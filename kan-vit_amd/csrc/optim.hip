// The optimizer step (kanvit/optim.py: KanvitAdamW): global-norm clipping, decoupled weight decay, a learning-rate schedule from a
// device table and a weight EMA in ONE pass over the parameters and ONE extra pass over the gradients.
//
// A launch takes up to KANVIT_OPTIM_MAX_TENSORS tensors BY VALUE in its argument block: gradients are new allocations on every eager
// step, so a device-side pointer table would be re-uploaded per step, and pointers in the kernel arguments are what a HIP-graph
// capture keeps.  A work-group takes ONE chunk of OPT_CHUNK elements of ONE tensor and finds the tensor by a binary search of its
// index in first[] (the tensors' first work-group indices): blockIdx is uniform over the wave, so the search runs on the scalar unit.
//
// A thread owns OPT_VEC consecutive elements per round, OPT_ROUNDS rounds per chunk.  Where the tensor's p and g are 16-byte aligned
// the four travel as one 16-byte access, otherwise as four 4-byte ones (--dp hands gradients as views into a bucket, at any 4-byte
// offset); which thread computes which element, and in which order anything is added, is the same in both, so the bits are too.
// The flat m / v / e slices start at multiples of four elements of 16-byte-aligned buffers.
//
//   optim_sumsq_kernel  one float64 partial per chunk: squares in float64 (the product of two floats is exact there), a thread adds
//                       its own elements in index order, then a fixed LDS tree.  No atomics: the same bits on every run.
//   optim_begin_kernel  one work-group: thread t adds the partials t, t + 256, ... in order, a fixed tree, then norm = (float)sqrt(S),
//                       coef = (float)min(1, max_norm / (sqrt(S) + 1e-6)) in float64 (clip_grad_norm_'s rule, rounded once), t += 1.
//   optim_adamw_kernel  the update, a fixed sequence of fp32 operations none of which is contracted (include/kanvit.h states it).
#include "../../include/kanvit.h"
#include "kanvit_common.h"

namespace {

constexpr int OPT_THREADS = 256, OPT_VEC = 4, OPT_ROUNDS = 4, OPT_CHUNK = OPT_THREADS * OPT_VEC * OPT_ROUNDS;
static_assert(OPT_CHUNK == KANVIT_OPTIM_CHUNK, "include/kanvit.h states the chunk");

struct OptimArgs {
    float* p[KANVIT_OPTIM_MAX_TENSORS];
    const float* g[KANVIT_OPTIM_MAX_TENSORS];
    long long off[KANVIT_OPTIM_MAX_TENSORS];         // first element of the tensor's slice in the flat state buffers
    long long numel[KANVIT_OPTIM_MAX_TENSORS];
    unsigned first[KANVIT_OPTIM_MAX_TENSORS + 1];    // first work-group of tensor i; first[n] = the grid
    unsigned decay[KANVIT_OPTIM_MAX_TENSORS];
    float* m;
    float* v;
    float* e;
    double* partials;           // optim_sumsq_kernel: one per work-group
    const float* table;         // [rows][4]
    const long long* step;
    const float* norm_coef;     // (norm, coef) of optim_begin_kernel, or null: no clipping
    long long rows;
    int n, has_wd;
    float b1, ob1, b2, ob2, eps, d, od;
};
// HIP passes at most 4 KB of kernel arguments; the runtime's own hidden arguments (256 bytes here) follow the block
static_assert(sizeof(OptimArgs) <= 4096 - 256, "KANVIT_OPTIM_MAX_TENSORS: the argument block must stay within the 4 KB limit");

// the tensor of work-group b: the last i with first[i] <= b (tensors without elements have no work-group and are passed over)
__device__ __forceinline__ int opt_find(const OptimArgs& a, unsigned b) {
    int lo = 0, hi = a.n;                            // first[lo] <= b < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_sumsq_kernel(const OptimArgs a) {
    __shared__ double part[OPT_THREADS];
    const int i = opt_find(a, blockIdx.x);
    const long long n = a.numel[i], base = (long long)(blockIdx.x - a.first[i]) * OPT_CHUNK;
    const float* g = a.g[i];
    const bool wide = ((uintptr_t)g & 15) == 0;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < OPT_ROUNDS; ++r) {
        const long long j = base + ((long long)r * OPT_THREADS + threadIdx.x) * OPT_VEC;
        float x[OPT_VEC] = {0.f, 0.f, 0.f, 0.f};     // past the end: + 0.0, which changes no sum of squares
        if (j + OPT_VEC <= n) {
            if (wide) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(g + j);
                x[0] = q[0], x[1] = q[1], x[2] = q[2], x[3] = q[3];
            } else {
#pragma unroll
                for (int k = 0; k < OPT_VEC; ++k) x[k] = g[j + k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < OPT_VEC; ++k)
                if (j + k < n) x[k] = g[j + k];
        }
#pragma unroll
        for (int k = 0; k < OPT_VEC; ++k) s += (double)x[k] * (double)x[k];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = OPT_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.partials[blockIdx.x] = part[0];
}

struct OptimBeginArgs {
    const double* partials;
    long long n_partials;
    double max_norm;            // <= 0: clipping is off, coef = 1
    long long* step;
    float* norm_coef;
};

__global__ __launch_bounds__(OPT_THREADS) void optim_begin_kernel(const OptimBeginArgs a) {
    __shared__ double part[OPT_THREADS];
    double s = 0.0;
    for (long long k = threadIdx.x; k < a.n_partials; k += OPT_THREADS) s += a.partials[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = OPT_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float norm = __builtin_nanf(""), coef = 1.f;             // no partials: the norm was not taken
        if (a.partials) {
            const double root = sqrt(part[0]);
            norm = (float)root;
            if (a.max_norm > 0.0) {
                const double c = a.max_norm / (root + 1e-6);
                coef = (float)(c > 1.0 ? 1.0 : c);              // a NaN norm stays a NaN coefficient, as torch's clamp leaves it
            }
        }
        a.norm_coef[0] = norm;
        a.norm_coef[1] = coef;
        a.step[0] += 1;
    }
}

// one element of the update; every operation rounds once
template <bool EMA>
__device__ __forceinline__ void opt_update(const OptimArgs& a, bool clip, float coef, bool decay, float r0, float r1, float r2, float& p, float g,
                                           float& m, float& v, float& e) {
#pragma clang fp contract(off)
    if (clip) g = __fmul_rn(g, coef);
    if (decay) p = __fmul_rn(p, r0);
    m = __fadd_rn(__fmul_rn(a.b1, m), __fmul_rn(a.ob1, g));
    v = __fadd_rn(__fmul_rn(a.b2, v), __fmul_rn(__fmul_rn(a.ob2, g), g));
    // sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the HIP header maps that name to the native (1 ulp) square root;
    // sqrtf compiles to the correctly rounded expansion (scaled v_sqrt_f32 and two fma corrections)
    const float den = __fadd_rn(__fdiv_rn(sqrtf(v), r2), a.eps);
    p = __fsub_rn(p, __fmul_rn(r1, __fdiv_rn(m, den)));
    if constexpr (EMA) e = __fadd_rn(__fmul_rn(a.d, e), __fmul_rn(a.od, p));
}

template <bool EMA>
__global__ __launch_bounds__(OPT_THREADS) void optim_adamw_kernel(const OptimArgs a) {
    const int i = opt_find(a, blockIdx.x);
    const long long n = a.numel[i], base = (long long)(blockIdx.x - a.first[i]) * OPT_CHUNK;
    float* p = a.p[i];
    const float* g = a.g[i];
    float* m = a.m + a.off[i];
    float* v = a.v + a.off[i];
    [[maybe_unused]] float* e = EMA ? a.e + a.off[i] : nullptr;
    const bool wide = (((uintptr_t)p | (uintptr_t)g) & 15) == 0;
    long long t = a.step[0];                         // optim_begin_kernel has counted this step already: t >= 1
    t = t < 1 ? 1 : (t > a.rows ? a.rows : t);       // past the table's end: its last row
    const float* row = a.table + (t - 1) * 4;
    const float r0 = row[0], r1 = row[1], r2 = row[2];
    const bool clip = a.norm_coef != nullptr, decay = a.has_wd && a.decay[i];
    const float coef = clip ? a.norm_coef[1] : 1.f;
#pragma unroll
    for (int r = 0; r < OPT_ROUNDS; ++r) {
        const long long j = base + ((long long)r * OPT_THREADS + threadIdx.x) * OPT_VEC;
        if (j + OPT_VEC <= n) {
            f32x4 pv, gv;
            if (wide) {
                pv = *reinterpret_cast<const f32x4*>(p + j);
                gv = *reinterpret_cast<const f32x4*>(g + j);
            } else {
#pragma unroll
                for (int k = 0; k < OPT_VEC; ++k) pv[k] = p[j + k], gv[k] = g[j + k];
            }
            f32x4 mv = *reinterpret_cast<const f32x4*>(m + j), vv = *reinterpret_cast<const f32x4*>(v + j), ev = {0.f, 0.f, 0.f, 0.f};
            if constexpr (EMA) ev = *reinterpret_cast<const f32x4*>(e + j);
#pragma unroll
            for (int k = 0; k < OPT_VEC; ++k) {
                float pk = pv[k], mk = mv[k], vk = vv[k], ek = ev[k];
                opt_update<EMA>(a, clip, coef, decay, r0, r1, r2, pk, gv[k], mk, vk, ek);
                pv[k] = pk, mv[k] = mk, vv[k] = vk, ev[k] = ek;
            }
            if (wide) {
                *reinterpret_cast<f32x4*>(p + j) = pv;
            } else {
#pragma unroll
                for (int k = 0; k < OPT_VEC; ++k) p[j + k] = pv[k];
            }
            *reinterpret_cast<f32x4*>(m + j) = mv;
            *reinterpret_cast<f32x4*>(v + j) = vv;
            if constexpr (EMA) *reinterpret_cast<f32x4*>(e + j) = ev;
        } else {
            for (int k = 0; k < OPT_VEC && j + k < n; ++k) {         // the tensor's last, partial group: element by element
                float pk = p[j + k], mk = m[j + k], vk = v[j + k], ek = 0.f;
                if constexpr (EMA) ek = e[j + k];
                opt_update<EMA>(a, clip, coef, decay, r0, r1, r2, pk, g[j + k], mk, vk, ek);
                p[j + k] = pk, m[j + k] = mk, v[j + k] = vk;
                if constexpr (EMA) e[j + k] = ek;
            }
        }
    }
}

// the tensor list of a multi-tensor launch into OptimArgs, validated; `grid` = its work-groups
int opt_fill(const char* who, OptimArgs& a, int n, void* const* params, const void* const* grads, const int64_t* offsets, const int64_t* numel,
             const int32_t* decay, int64_t state_numel, long long& grid) {
    if (n < 0 || n > KANVIT_OPTIM_MAX_TENSORS)
        return kv_fail(KANVIT_EINVAL, "%s: n=%d tensors: one launch takes 0..%d (kanvit_optim_max_tensors)", who, n, KANVIT_OPTIM_MAX_TENSORS);
    if (n > 0 && (!grads || !numel || (params == nullptr) != (offsets == nullptr)))
        return kv_fail(KANVIT_EINVAL, "%s: null grads/numel/params/offsets array", who);
    grid = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) return kv_fail(KANVIT_EINVAL, "%s: tensor %d has numel=%lld", who, i, (long long)numel[i]);
        if (numel[i] > 0 && (!grads[i] || (params && !params[i]))) return kv_fail(KANVIT_EINVAL, "%s: tensor %d has a null pointer", who, i);
        if ((uintptr_t)grads[i] & 3 || (params && (uintptr_t)params[i] & 3))
            return kv_fail(KANVIT_EINVAL, "%s: tensor %d: a pointer is not aligned to 4 bytes", who, i);
        if (offsets && (offsets[i] < 0 || offsets[i] % 4 != 0 || offsets[i] > state_numel || numel[i] > state_numel - offsets[i]))
            return kv_fail(KANVIT_EINVAL, "%s: tensor %d: state slice offset=%lld, numel=%lld: the offset is a multiple of 4 and the slice lies "
                           "inside the %lld state elements", who, i, (long long)offsets[i], (long long)numel[i], (long long)state_numel);
        a.p[i] = params ? (float*)params[i] : nullptr;
        a.g[i] = (const float*)grads[i];
        a.off[i] = offsets ? offsets[i] : 0;
        a.numel[i] = numel[i];
        a.decay[i] = decay ? (decay[i] != 0) : 0u;
        a.first[i] = (unsigned)grid;
        grid += (numel[i] + OPT_CHUNK - 1) / OPT_CHUNK;
        if (grid > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "%s: more than 2^31 - 1 chunks of %d elements in one launch", who, OPT_CHUNK);
    }
    for (int i = n; i <= KANVIT_OPTIM_MAX_TENSORS; ++i) a.first[i] = (unsigned)grid;
    a.n = n;
    return 0;
}

}  // namespace

extern "C" {

int kanvit_optim_max_tensors(void) { return KANVIT_OPTIM_MAX_TENSORS; }

size_t kanvit_optim_sumsq_workspace(int n, const int64_t* numel) {
    if (n < 0 || (n > 0 && !numel)) return 0;
    size_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) return 0;
        chunks += ((size_t)numel[i] + OPT_CHUNK - 1) / OPT_CHUNK;
    }
    return chunks * sizeof(double);
}

int kanvit_optim_sumsq(int n, const void* const* grads, const int64_t* numel, void* workspace, size_t workspace_bytes, void* stream) {
    OptimArgs a = {};
    long long grid = 0;
    if (int rc = opt_fill("kanvit_optim_sumsq", a, n, nullptr, grads, nullptr, numel, nullptr, 0, grid)) return rc;
    if (grid == 0) return 0;
    if (!workspace) return kv_fail(KANVIT_EINVAL, "kanvit_optim_sumsq: null workspace");
    if ((uintptr_t)workspace & 7) return kv_fail(KANVIT_EINVAL, "kanvit_optim_sumsq: the workspace is not aligned to 8 bytes");
    if (workspace_bytes < (size_t)grid * sizeof(double))
        return kv_fail(KANVIT_EINVAL, "kanvit_optim_sumsq: workspace of %zu bytes, %zu needed (kanvit_optim_sumsq_workspace)", workspace_bytes,
                       (size_t)grid * sizeof(double));
    a.partials = (double*)workspace;
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned)grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("optim_sumsq_kernel");
    return 0;
}

int kanvit_optim_begin(const void* partials, int64_t n_partials, double max_norm, int64_t* step, float* norm_coef, void* stream) {
    if (!step || !norm_coef) return kv_fail(KANVIT_EINVAL, "kanvit_optim_begin: null step/norm_coef");
    if (n_partials < 0) return kv_fail(KANVIT_EINVAL, "kanvit_optim_begin: n_partials=%lld is negative", (long long)n_partials);
    if (n_partials > 0 && !partials) return kv_fail(KANVIT_EINVAL, "kanvit_optim_begin: null partials with n_partials=%lld", (long long)n_partials);
    if (max_norm != max_norm) return kv_fail(KANVIT_EINVAL, "kanvit_optim_begin: max_norm is NaN (<= 0: no clipping)");
    if (max_norm > 0.0 && !partials) return kv_fail(KANVIT_EINVAL, "kanvit_optim_begin: max_norm=%g needs the partials of kanvit_optim_sumsq", max_norm);
    if ((uintptr_t)partials & 7 || (uintptr_t)step & 7 || (uintptr_t)norm_coef & 3)
        return kv_fail(KANVIT_EINVAL, "kanvit_optim_begin: a pointer is not aligned to its element size");
    OptimBeginArgs a;
    a.partials = (const double*)partials;
    a.n_partials = n_partials;
    a.max_norm = max_norm;
    a.step = (long long*)step;
    a.norm_coef = norm_coef;
    hipLaunchKernelGGL(optim_begin_kernel, dim3(1), dim3(OPT_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("optim_begin_kernel");
    return 0;
}

int kanvit_optim_adamw(int n, void* const* params, const void* const* grads, const int64_t* offsets, const int64_t* numel, const int32_t* decay,
                       float* exp_avg, float* exp_avg_sq, float* ema, int64_t state_numel, const float* table, int64_t table_rows,
                       const int64_t* step, const float* norm_coef, int has_wd, float b1, float ob1, float b2, float ob2, float eps, float d,
                       float od, void* stream) {
    if (!exp_avg || !exp_avg_sq || !table || !step) return kv_fail(KANVIT_EINVAL, "kanvit_optim_adamw: null exp_avg/exp_avg_sq/table/step");
    if (state_numel < 0) return kv_fail(KANVIT_EINVAL, "kanvit_optim_adamw: state_numel=%lld is negative", (long long)state_numel);
    if (table_rows < 1) return kv_fail(KANVIT_EINVAL, "kanvit_optim_adamw: table_rows=%lld: the table has at least one row", (long long)table_rows);
    if (n > 0 && (!params || !offsets || !decay)) return kv_fail(KANVIT_EINVAL, "kanvit_optim_adamw: null params/offsets/decay array");
    if ((uintptr_t)exp_avg & 15 || (uintptr_t)exp_avg_sq & 15 || (uintptr_t)ema & 15)
        return kv_fail(KANVIT_EINVAL, "kanvit_optim_adamw: exp_avg/exp_avg_sq/ema are not aligned to 16 bytes");
    if ((uintptr_t)table & 3 || (uintptr_t)step & 7 || (uintptr_t)norm_coef & 3)
        return kv_fail(KANVIT_EINVAL, "kanvit_optim_adamw: table/step/norm_coef is not aligned to its element size");
    OptimArgs a = {};
    long long grid = 0;
    if (int rc = opt_fill("kanvit_optim_adamw", a, n, params, grads, offsets, numel, decay, state_numel, grid)) return rc;
    if (grid == 0) return 0;
    a.m = exp_avg, a.v = exp_avg_sq, a.e = ema;
    a.table = table, a.rows = table_rows;
    a.step = (const long long*)step;
    a.norm_coef = norm_coef;
    a.has_wd = has_wd != 0;
    a.b1 = b1, a.ob1 = ob1, a.b2 = b2, a.ob2 = ob2, a.eps = eps, a.d = d, a.od = od;
    if (ema)
        hipLaunchKernelGGL(optim_adamw_kernel<true>, dim3((unsigned)grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(optim_adamw_kernel<false>, dim3((unsigned)grid), dim3(OPT_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("optim_adamw_kernel");
    return 0;
}

}  // extern "C"

// KAN edge pruning (kanvit_edge_select, kanvit_mask_rows) compiles as part of this unit: its multi-tensor launch follows the one above
#include "edge_prune.hip"
