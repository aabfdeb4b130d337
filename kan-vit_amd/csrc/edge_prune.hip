// KAN edge pruning: which edges of a layer go, and holding them at zero.
// Compiled inside the optim unit (optim.hip includes this file at its end, as addln.hip includes patch_drop.hip): kanvit_mask_rows
// follows the optimizer's multi-tensor chunking, and the unit count of the build stays what the tests count.
//
//   kanvit_edge_select   mask[groups][E] (uint8, 1 = keep) and kept[groups] from the score table A[groups][E].  ONE work-group of
//                        SEL_THREADS per group (a launch happens a handful of times per run): an exact radix select on the 31-bit keys
//                        bits(a) & 0x7fffffff -- four byte-wise passes, each an LDS histogram of the keys that still carry the prefix
//                        found so far (integer LDS atomics: the counts do not depend on their order) -- gives the n_prune-th smallest
//                        key T and the number of keys below it; then ONE pass in index order prunes every key below T and the first
//                        n_prune - count_less keys equal to T, ranked by a block-wide prefix sum over laps of SEL_LAP consecutive
//                        entries.  The threshold modes skip the select (T = key(t), nothing equal to T is pruned); REL first takes
//                        the group's largest key (an LDS integer max).  No global atomics, no workspace, nothing from other groups.
//   kanvit_mask_rows     x[e] = masks[k][e / run[k]] ? x[e] : +0.0f over up to KANVIT_MASK_MAX_TENSORS tensors passed by value.  A
//                        select needs no read of x: a kept element is not touched at all, a masked one is overwritten, so the kernel
//                        moves the mask bytes and the zeros only.  A thread owns MR_VEC consecutive elements per round as in
//                        optim.hip; four masked elements of a 16-byte-aligned tensor leave as one 16-byte store, anything else as
//                        4-byte stores -- the same bytes either way.  run is no power of two: the mask is indexed per element, from
//                        ONE 64-bit division per thread and chunk (the rounds step the quotient and remainder by a uniform stride).

namespace {

constexpr int SEL_THREADS = 1024, SEL_VPT = 4, SEL_LAP = SEL_THREADS * SEL_VPT, SEL_WAVES = SEL_THREADS / 64;static_assert(SEL_LAP == KANVIT_EDGE_SELECT_LAP, "include/kanvit.h states the lap");

struct EdgeSelectArgs {
    const float* A;
    unsigned char* mask;
    long long* kept;
    long long E, n_prune;
    float threshold;
    int mode;
};

__device__ __forceinline__ unsigned sel_key(float a) { return __float_as_uint(a) & 0x7fffffffu; }

__global__ __launch_bounds__(SEL_THREADS) void edge_select_kernel(const EdgeSelectArgs a) {
    __shared__ unsigned hist[256];
    __shared__ unsigned wave_eq[2][SEL_WAVES];
    __shared__ unsigned sh_prefix, sh_rank, sh_less, sh_max, sh_pruned;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long E = a.E;
    const float* A = a.A + (long long)blockIdx.x * E;
    unsigned char* mask = a.mask + (long long)blockIdx.x * E;

    unsigned T = 0, need_eq = 0;                     // prune key < T, and the first need_eq entries with key == T
    if (t == 0) sh_max = 0, sh_pruned = 0;
    if (a.mode == KANVIT_PRUNE_ABS) {
        T = sel_key(a.threshold);
        __syncthreads();
    } else if (a.mode == KANVIT_PRUNE_REL) {
        __syncthreads();
        unsigned m = 0;
        for (long long i = t; i < E; i += SEL_THREADS) {
            const unsigned k = sel_key(A[i]);
            m = k > m ? k : m;
        }
        atomicMax(&sh_max, m);
        __syncthreads();
        T = sel_key(__fmul_rn(a.threshold, __uint_as_float(sh_max)));
    } else if (a.n_prune > 0) {
        // the key of rank n_prune (1-based) in ascending order: per pass, the bucket of byte `shift` in which that rank falls among
        // the keys that carry the prefix; sh_less collects the keys of the lower buckets, i.e. those below the final key
        if (t == 0) sh_prefix = 0, sh_rank = (unsigned)a.n_prune, sh_less = 0;
        const long long laps = (E + SEL_THREADS - 1) / SEL_THREADS;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (t < 256) hist[t] = 0;
            __syncthreads();
            const unsigned prefix = sh_prefix, himask = shift == 24 ? 0u : ~0u << (shift + 8);
            for (long long l = 0; l < laps; ++l) {                   // a uniform trip count: the ballots below see whole waves
                const long long i = l * SEL_THREADS + t;
                const unsigned k = i < E ? sel_key(A[i]) : 0u;
                const bool in = i < E && (k & himask) == prefix;
                const unsigned bin = (k >> shift) & 255u;
                const unsigned long long act = __ballot(in);
                if (act == 0) continue;
                // scores of one layer crowd into a few buckets: a wave whose keys all fall into one adds its count once
                const unsigned fb = (unsigned)__shfl((int)bin, __ffsll((long long)act) - 1);
                if (__ballot(in && bin == fb) == act) {
                    if (lane == __ffsll((long long)act) - 1) atomicAdd(&hist[fb], (unsigned)__popcll(act));
                } else if (in) {
                    atomicAdd(&hist[bin], 1u);
                }
            }
            __syncthreads();
            if (t == 0) {
                unsigned below = 0, b = 0;
                const unsigned r = sh_rank;                          // 1 <= r <= the keys that carry the prefix
                while (b < 255 && below + hist[b] < r) below += hist[b], ++b;
                sh_prefix = prefix | (b << shift);
                sh_rank = r - below;
                sh_less += below;
            }
            __syncthreads();
        }
        T = sh_prefix;
        need_eq = (unsigned)a.n_prune - sh_less;
    } else {
        __syncthreads();
    }

    // the index-ordered pass: thread t owns entries lap * SEL_LAP + SEL_VPT t .. + SEL_VPT - 1
    unsigned run_eq = 0, pruned = 0;                 // run_eq: the entries equal to T in the laps before this one (uniform)
    int buf = 0;
    for (long long base = 0; base < E; base += SEL_LAP, buf ^= 1) {
        const long long j = base + (long long)t * SEL_VPT;
        unsigned k[SEL_VPT], eq = 0;
#pragma unroll
        for (int e = 0; e < SEL_VPT; ++e) {
            k[e] = j + e < E ? sel_key(A[j + e]) : 0xffffffffu;      // past the end: above every key, equal to none
            eq += k[e] == T ? 1u : 0u;
        }
        unsigned at = 0;                             // entries equal to T in front of this thread's, from the group's first
        if (need_eq > 0) {
            unsigned inc = eq;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned v = (unsigned)__shfl_up((int)inc, d);
                if (lane >= d) inc += v;
            }
            if (lane == 63) wave_eq[buf][wave] = inc;
            __syncthreads();                         // wave_eq[buf] is rewritten two laps on, behind the next lap's barrier
            unsigned before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < SEL_WAVES; ++w) {
                const unsigned s = wave_eq[buf][w];
                before += w < wave ? s : 0u;
                total += s;
            }
            at = run_eq + before + inc - eq;
            run_eq += total;
        }
#pragma unroll
        for (int e = 0; e < SEL_VPT; ++e) {
            if (j + e < E) {
                bool drop = k[e] < T;
                if (k[e] == T) drop = at < need_eq, ++at;
                mask[j + e] = drop ? 0 : 1;
                pruned += drop ? 1u : 0u;
            }
        }
    }
    atomicAdd(&sh_pruned, pruned);
    __syncthreads();
    if (t == 0) a.kept[blockIdx.x] = E - (long long)sh_pruned;
}

constexpr int MR_THREADS = 256, MR_VEC = 4, MR_ROUNDS = 4, MR_STRIDE = MR_THREADS * MR_VEC, MR_CHUNK = MR_STRIDE * MR_ROUNDS;
static_assert(MR_CHUNK == KANVIT_MASK_CHUNK, "include/kanvit.h states the chunk");

struct MaskRowsArgs {
    float* x[KANVIT_MASK_MAX_TENSORS];
    const unsigned char* mask[KANVIT_MASK_MAX_TENSORS];
    long long numel[KANVIT_MASK_MAX_TENSORS];
    long long run[KANVIT_MASK_MAX_TENSORS];
    unsigned first[KANVIT_MASK_MAX_TENSORS + 1];     // first work-group of tensor i; first[n] = the grid
    int n;
};
static_assert(sizeof(MaskRowsArgs) <= 4096 - 256, "KANVIT_MASK_MAX_TENSORS: the argument block must stay within the 4 KB limit");

__global__ __launch_bounds__(MR_THREADS) void mask_rows_kernel(const MaskRowsArgs a) {
    int lo = 0, hi = a.n;                            // the tensor of this work-group: the last i with first[i] <= blockIdx (opt_find)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first[mid] <= blockIdx.x)
            lo = mid;
        else
            hi = mid;
    }
    const long long n = a.numel[lo], run = a.run[lo], base = (long long)(blockIdx.x - a.first[lo]) * MR_CHUNK;
    float* x = a.x[lo];
    const unsigned char* mask = a.mask[lo];
    const bool wide = ((uintptr_t)x & 15) == 0;
    const long long dq = MR_STRIDE / run, dr = MR_STRIDE % run;      // a round's step in rows and inside the row: uniform
    long long j = base + (long long)threadIdx.x * MR_VEC;
    long long row = j / run, rem = j - row * run;
#pragma unroll
    for (int r = 0; r < MR_ROUNDS; ++r) {
        if (j < n) {
            bool keep[MR_VEC];
            long long q = row, s = rem;
            bool none = true;
#pragma unroll
            for (int k = 0; k < MR_VEC; ++k) {
                keep[k] = j + k < n ? mask[q] != 0 : true;           // past the end: not touched
                none = none && !keep[k];
                if (++s == run) s = 0, ++q;
            }
            if (none && wide) {                      // all four inside the tensor and masked
                *reinterpret_cast<f32x4*>(x + j) = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int k = 0; k < MR_VEC; ++k)
                    if (!keep[k]) x[j + k] = 0.f;
            }
        }
        j += MR_STRIDE;
        row += dq, rem += dr;
        if (rem >= run) rem -= run, ++row;
    }
}

}  // namespace

extern "C" {

int kanvit_edge_select(const float* A, int64_t groups, int64_t E, int mode, float threshold, int64_t n_prune, uint8_t* mask, int64_t* kept,
                       void* stream) {
    if (mode != KANVIT_PRUNE_COUNT && mode != KANVIT_PRUNE_ABS && mode != KANVIT_PRUNE_REL)
        return kv_fail(KANVIT_EINVAL, "kanvit_edge_select: mode=%d is none of KANVIT_PRUNE_COUNT / _ABS / _REL", mode);
    if (groups < 0 || groups > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "kanvit_edge_select: groups=%lld must be in 0..2^31-1", (long long)groups);
    if (E < 1 || E > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "kanvit_edge_select: E=%lld must be in 1..2^31-1", (long long)E);
    if (mode == KANVIT_PRUNE_COUNT) {
        if (n_prune < 0 || n_prune > E - 1)
            return kv_fail(KANVIT_EINVAL, "kanvit_edge_select: n_prune=%lld must be in 0..E-1=%lld (a group keeps its strongest edge)",
                           (long long)n_prune, (long long)(E - 1));
    } else if (!(threshold >= 0.0f) || threshold > 3.402823466e+38f || (mode == KANVIT_PRUNE_REL && threshold > 1.0f)) {
        return kv_fail(KANVIT_EINVAL, "kanvit_edge_select: threshold=%g must be finite and >= 0%s", (double)threshold,
                       mode == KANVIT_PRUNE_REL ? ", and <= 1 in KANVIT_PRUNE_REL (the maximum stays)" : "");
    }
    if (!A || !mask || !kept) return kv_fail(KANVIT_EINVAL, "kanvit_edge_select: null A/mask/kept");
    if ((uintptr_t)A & 3 || (uintptr_t)kept & 7) return kv_fail(KANVIT_EINVAL, "kanvit_edge_select: A/kept is not aligned to its element size");
    if (groups == 0) return 0;
    EdgeSelectArgs a = {};
    a.A = A, a.mask = mask, a.kept = (long long*)kept;
    a.E = E, a.n_prune = mode == KANVIT_PRUNE_COUNT ? n_prune : 0;
    a.threshold = threshold, a.mode = mode;
    hipLaunchKernelGGL(edge_select_kernel, dim3((unsigned)groups), dim3(SEL_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("edge_select_kernel");
    return 0;
}

int kanvit_mask_max_tensors(void) { return KANVIT_MASK_MAX_TENSORS; }

int kanvit_mask_rows(int n, void* const* tensors, const int64_t* numel, const int64_t* run, const uint8_t* const* masks, void* stream) {
    if (n < 0 || n > KANVIT_MASK_MAX_TENSORS)
        return kv_fail(KANVIT_EINVAL, "kanvit_mask_rows: n=%d tensors: one launch takes 0..%d (kanvit_mask_max_tensors)", n, KANVIT_MASK_MAX_TENSORS);
    if (n > 0 && (!tensors || !numel || !run || !masks)) return kv_fail(KANVIT_EINVAL, "kanvit_mask_rows: null tensors/numel/run/masks array");
    MaskRowsArgs a = {};
    long long grid = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) return kv_fail(KANVIT_EINVAL, "kanvit_mask_rows: tensor %d has numel=%lld", i, (long long)numel[i]);
        if (run[i] < 1 || numel[i] % run[i] != 0)
            return kv_fail(KANVIT_EINVAL, "kanvit_mask_rows: tensor %d: run=%lld must be >= 1 and divide numel=%lld", i, (long long)run[i],
                           (long long)numel[i]);
        if (numel[i] > 0 && (!tensors[i] || !masks[i])) return kv_fail(KANVIT_EINVAL, "kanvit_mask_rows: tensor %d has a null pointer", i);
        if ((uintptr_t)tensors[i] & 3) return kv_fail(KANVIT_EINVAL, "kanvit_mask_rows: tensor %d is not aligned to 4 bytes", i);
        a.x[i] = (float*)tensors[i];
        a.mask[i] = masks[i];
        a.numel[i] = numel[i];
        a.run[i] = run[i];
        a.first[i] = (unsigned)grid;
        grid += (numel[i] + MR_CHUNK - 1) / MR_CHUNK;
        if (grid > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "kanvit_mask_rows: more than 2^31 - 1 chunks of %d elements in one launch", MR_CHUNK);
    }
    for (int i = n; i <= KANVIT_MASK_MAX_TENSORS; ++i) a.first[i] = (unsigned)grid;
    a.n = n;
    if (grid == 0) return 0;
    hipLaunchKernelGGL(mask_rows_kernel, dim3((unsigned)grid), dim3(MR_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("mask_rows_kernel");
    return 0;
}

}  // extern "C"
