// PatchDropout (Liu et al. 2023; timm's patch_drop_rate): in training every sample keeps K of its P patch tokens plus the class token.
// Compiled inside the addln unit (addln.hip includes this file at its end, as batch_u8.hip includes randaug.hip): it shares sd_mix, the
// splitmix64 step of kanvit_depth_scales, and the unit count of the build stays what the tests count.
//
//   kanvit_patch_keep            idx[B][K]: the kept patch numbers of every sample, ascending -- a hash of (seed, device counter, b, p), no
//                                RNG state; one launch that reads the counter in every work-group and bumps it once (protocol below)
//   kanvit_patch_gather          rows[B*K][I] = the kept patches out of the NCHW batch (patchify restricted to idx): a pure copy
//   kanvit_tokens_assemble_fwd   out[B][K+1][O] = [cls + pos[0]; tokens[b*K + j] + pos[1 + idx[b][j]]]: one fp32 add per element
//   kanvit_tokens_assemble_bwd   dtokens = dout without its class rows (a copy), dcls = sum_b dout[b][0] in a fixed order
//
// The three row kernels share one walk: a work-group of 256 threads is cut into sub-groups of LPR = 2^k lanes, k chosen on the host so
// that one sub-group spans a row's vectors (at most a wave: wider rows take several steps); sub-group r of work-group g takes rows
// g * RPB + r, + gridDim * RPB, ...; the element decomposition (channel, line, column of a patch element) is done once per lane, outside
// the row loop.  VEC = 4 moves float4 where every address involved is a multiple of 16 bytes, VEC = 1 is the general form.

namespace {

constexpr int PD_THREADS = 256;
constexpr int PD_KEEP_GRID = 128;        // work-groups of patch_keep_kernel: group g draws samples g, g + 128, ...
constexpr int PD_ROW_GRID = 2048;        // work-groups of the row kernels at most (8 per CU)
constexpr int PD_TICKET_SHIFT = 48;      // the counter's top 16 bits carry the launch's ticket while it runs
constexpr int PD_CHUNK = KANVIT_PATCH_KEEP_MAX_P / PD_THREADS;      // consecutive patches one thread owns in the prefix sum
static_assert(PD_CHUNK * PD_THREADS == KANVIT_PATCH_KEEP_MAX_P, "the prefix sum gives every thread PD_CHUNK consecutive patches");
static_assert(PD_KEEP_GRID < (1 << 16), "the ticket has 16 bits");

struct PatchKeepArgs {
    unsigned long long seed_mixed;       // mix(seed ^ KANVIT_PATCH_KEEP_TAG)
    unsigned long long* counter;
    int* idx;                            // [B][K]
    long long B;
    int P, K;
};

// Counter protocol.  ONE atomic per work-group is both its read and its ticket: old = atomicAdd(counter, 1 << 48) returns the step
// count c in the low 48 bits (nothing changes those while tickets are out) and, in the top 16, how many groups came before.  The group
// that draws ticket gridDim - 1 knows every other group has already read -- atomics on one address are totally ordered -- so it alone
// adds 1 - (gridDim << 48): tickets back to 0, c + 1 in place.  No second buffer, so launches on different counters never meet.
__global__ __launch_bounds__(PD_THREADS) void patch_keep_kernel(const PatchKeepArgs a) {
    __shared__ unsigned long long keys[KANVIT_PATCH_KEEP_MAX_P];
    __shared__ unsigned char kept[KANVIT_PATCH_KEEP_MAX_P];
    __shared__ int wave_sum[PD_THREADS / 64];
    __shared__ unsigned long long ticket;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) {
        const unsigned long long old = atomicAdd(a.counter, 1ull << PD_TICKET_SHIFT);
        if ((old >> PD_TICKET_SHIFT) == gridDim.x - 1) atomicAdd(a.counter, 1ull - ((unsigned long long)gridDim.x << PD_TICKET_SHIFT));
        ticket = old;
    }
    __syncthreads();
    const unsigned long long c = ticket & ((1ull << PD_TICKET_SHIFT) - 1ull);
    const unsigned long long base = sd_mix(a.seed_mixed + c);
    const int P = a.P, K = a.K;
    for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
        const unsigned long long bb = base + ((unsigned long long)b << 32);
        for (int p = t; p < P; p += PD_THREADS) keys[p] = sd_mix(bb + (unsigned long long)p);
        __syncthreads();
        // rank of (key, p) among the sample's P pairs: every lane reads the same keys[q] (an LDS broadcast)
        for (int p = t; p < P; p += PD_THREADS) {
            const unsigned long long k = keys[p];
            int rank = 0;
#pragma unroll 8
            for (int q = 0; q < P; ++q) {
                const unsigned long long kq = keys[q];
                rank += (kq < k || (kq == k && q < p)) ? 1 : 0;
            }
            kept[p] = rank < K ? 1 : 0;
        }
        __syncthreads();
        // exclusive prefix sum of the flags in patch order: thread t owns patches PD_CHUNK t .. PD_CHUNK t + PD_CHUNK - 1
        int flag[PD_CHUNK], n = 0;
#pragma unroll
        for (int e = 0; e < PD_CHUNK; ++e) {
            const int p = t * PD_CHUNK + e;
            flag[e] = p < P ? kept[p] : 0;
            n += flag[e];
        }
        int inc = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(inc, d);
            if (lane >= d) inc += v;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        int at = inc - n;
        for (int w = 0; w < wave; ++w) at += wave_sum[w];
        int* row = a.idx + b * K;
#pragma unroll
        for (int e = 0; e < PD_CHUNK; ++e)
            if (flag[e]) row[at++] = t * PD_CHUNK + e;           // the ranks are a permutation: exactly K flags, at < K
        __syncthreads();                                         // keys / kept / wave_sum are rewritten for the next sample
    }
}

template <int VEC>
struct PdVec { typedef float type; };
template <>
struct PdVec<4> { typedef f32x4 type; };

struct PatchGatherArgs {
    const float* images;
    const int* idx;
    float* rows;
    long long ldr;
    int R, K;                   // R = B * K rows
    int C, H, W, n, ph, pw, I;
    int lpr_log2;
};

template <int VEC>
__global__ __launch_bounds__(PD_THREADS) void patch_gather_kernel(const PatchGatherArgs a) {
    typedef typename PdVec<VEC>::type V;
    const int lpr = 1 << a.lpr_log2, rpb = PD_THREADS >> a.lpr_log2;
    const int r = threadIdx.x >> a.lpr_log2, l = threadIdx.x & (lpr - 1);
    const int plane = a.ph * a.pw, nv = a.I / VEC;
    const long long image = (long long)a.C * a.H * a.W;
    for (int iv = l; iv < nv; iv += lpr) {
        const int i = iv * VEC;
        const int c = i / plane, rem = i - c * plane, iy = rem / a.pw, ix = rem - iy * a.pw;
        const long long off = ((long long)c * a.H + iy) * a.W + ix;
        for (long long row = (long long)blockIdx.x * rpb + r; row < a.R; row += (long long)gridDim.x * rpb) {
            const int b = (int)row / a.K;
            const int p = a.idx[row];
            const int py = p / a.n, px = p - py * a.n;
            const float* src = a.images + b * image + (long long)py * a.ph * a.W + px * a.pw + off;
            *reinterpret_cast<V*>(a.rows + row * a.ldr + i) = *reinterpret_cast<const V*>(src);
        }
    }
}

struct AssembleArgs {
    const float* tokens;
    const float* cls;
    const float* pos;
    const int* idx;
    float* out;
    long long ldt;
    int R, K, O;                // R = B * (K + 1) rows
    int lpr_log2;
};

template <int VEC>
__global__ __launch_bounds__(PD_THREADS) void tokens_assemble_fwd_kernel(const AssembleArgs a) {
    typedef typename PdVec<VEC>::type V;
    const int lpr = 1 << a.lpr_log2, rpb = PD_THREADS >> a.lpr_log2;
    const int r = threadIdx.x >> a.lpr_log2, l = threadIdx.x & (lpr - 1);
    const int nv = a.O / VEC, N = a.K + 1;
    for (int iv = l; iv < nv; iv += lpr) {
        const int o = iv * VEC;
        for (long long row = (long long)blockIdx.x * rpb + r; row < a.R; row += (long long)gridDim.x * rpb) {
            const int b = (int)row / N, j = (int)row - b * N;
            V v;
            if (j == 0) {
                v = *reinterpret_cast<const V*>(a.cls + o) + *reinterpret_cast<const V*>(a.pos + o);
            } else {
                const long long tr = (long long)b * a.K + (j - 1);
                v = *reinterpret_cast<const V*>(a.tokens + tr * a.ldt + o) +
                    *reinterpret_cast<const V*>(a.pos + (long long)(1 + a.idx[tr]) * a.O + o);
            }
            *reinterpret_cast<V*>(a.out + row * a.O + o) = v;
        }
    }
}

constexpr int PD_SUM_COLS = 32;                        // columns one work-group of the dcls part sums
constexpr int PD_SUM_SLICES = PD_THREADS / PD_SUM_COLS;

struct AssembleBwdArgs {
    const float* dout;          // [B][K + 1][O]
    float* dtokens;             // [B * K][O], or NULL
    float* dcls;                // [O], or NULL
    int R, K, O, B;             // R = B * K rows
    int lpr_log2, copy_groups;
};

// Work-groups [0, copy_groups) copy the patch-token rows; the ones behind them each sum PD_SUM_COLS columns of the class rows: slice s
// adds samples s, s + 8, ... in that order, then one thread per column adds the eight slices in order -- the same tree every run.
template <int VEC>
__global__ __launch_bounds__(PD_THREADS) void tokens_assemble_bwd_kernel(const AssembleBwdArgs a) {
    typedef typename PdVec<VEC>::type V;
    __shared__ float part[PD_SUM_SLICES][PD_SUM_COLS];
    const long long sample = (long long)(a.K + 1) * a.O;
    if ((int)blockIdx.x < a.copy_groups) {
        const int lpr = 1 << a.lpr_log2, rpb = PD_THREADS >> a.lpr_log2;
        const int r = threadIdx.x >> a.lpr_log2, l = threadIdx.x & (lpr - 1);
        const int nv = a.O / VEC;
        for (int iv = l; iv < nv; iv += lpr) {
            const int o = iv * VEC;
            for (long long row = (long long)blockIdx.x * rpb + r; row < a.R; row += (long long)a.copy_groups * rpb) {
                const int b = (int)row / a.K;
                *reinterpret_cast<V*>(a.dtokens + row * a.O + o) = *reinterpret_cast<const V*>(a.dout + (row + b + 1) * a.O + o);
            }
        }
        return;
    }
    const int col = threadIdx.x % PD_SUM_COLS, s = threadIdx.x / PD_SUM_COLS;
    const int o = ((int)blockIdx.x - a.copy_groups) * PD_SUM_COLS + col;
    float acc = 0.0f;
    if (o < a.O)
        for (int b = s; b < a.B; b += PD_SUM_SLICES) acc += a.dout[b * sample + o];
    part[s][col] = acc;
    __syncthreads();
    if (s == 0 && o < a.O) {
        float v = part[0][col];
#pragma unroll
        for (int k = 1; k < PD_SUM_SLICES; ++k) v += part[k][col];
        a.dcls[o] = v;
    }
}

// lanes of a sub-group: the power of two that covers nv vectors, a wave at most
int pd_lpr_log2(int nv) {
    int k = 0;
    while (k < 6 && (1 << k) < nv) ++k;
    return k;
}

int pd_row_grid(long long rows, int lpr_log2) {
    const long long rpb = PD_THREADS >> lpr_log2;
    const long long g = (rows + rpb - 1) / rpb;
    return (int)(g < PD_ROW_GRID ? g : PD_ROW_GRID);
}

bool pd_mis(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

}  // namespace

extern "C" {

int kanvit_patch_keep(int64_t B, int P, int K, uint64_t seed, uint64_t* counter, int32_t* idx, void* stream) {
    if (P < 1 || P > KANVIT_PATCH_KEEP_MAX_P)
        return kv_fail(KANVIT_EINVAL, "kanvit_patch_keep: P=%d: one sample's keys live in LDS, 1..%d patches", P, KANVIT_PATCH_KEEP_MAX_P);
    if (K < 1 || K > P) return kv_fail(KANVIT_EINVAL, "kanvit_patch_keep: K=%d must be in 1..P=%d", K, P);
    if (B < 0 || B > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "kanvit_patch_keep: B=%lld must be in 0..2^31-1", (long long)B);
    if (!counter || (B > 0 && !idx)) return kv_fail(KANVIT_EINVAL, "kanvit_patch_keep: null counter/idx");
    if (pd_mis(counter, 7) || pd_mis(idx, 3)) return kv_fail(KANVIT_EINVAL, "kanvit_patch_keep: counter/idx is not aligned to its element size");
    if (B == 0) return 0;
    PatchKeepArgs a = {};
    a.seed_mixed = sd_mix(seed ^ KANVIT_PATCH_KEEP_TAG);
    a.counter = (unsigned long long*)counter;
    a.idx = idx;
    a.B = B;
    a.P = P;
    a.K = K;
    const int grid = (int)(B < PD_KEEP_GRID ? B : PD_KEEP_GRID);
    hipLaunchKernelGGL(patch_keep_kernel, dim3(grid), dim3(PD_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("patch_keep_kernel");
    return 0;
}

int kanvit_patch_gather(const kanvit_patch_desc* p, int64_t B, int K, const int32_t* idx, const float* images, float* rows, int64_t ldr,
                        void* stream) {
    if (!p) return kv_fail(KANVIT_EINVAL, "kanvit_patch_gather: null descriptor");
    if (p->C < 1 || p->H < 1 || p->W < 1 || p->n_patches < 1 || p->H % p->n_patches || p->W % p->n_patches)
        return kv_fail(KANVIT_EINVAL, "kanvit_patch_gather: C=%d H=%d W=%d n_patches=%d: sizes >= 1, n_patches divides H and W", p->C, p->H,
                       p->W, p->n_patches);
    const int ph = p->H / p->n_patches, pw = p->W / p->n_patches;
    const long long I = (long long)p->C * ph * pw, P = (long long)p->n_patches * p->n_patches;
    if (K < 1 || K > P) return kv_fail(KANVIT_EINVAL, "kanvit_patch_gather: K=%d must be in 1..P=%lld", K, P);
    if (B < 0 || B * K > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "kanvit_patch_gather: B=%lld: B >= 0 and B*K rows < 2^31", (long long)B);
    if (I > 0x7fffffffll || ldr < I) return kv_fail(KANVIT_EINVAL, "kanvit_patch_gather: ldr=%lld is below the row length I=%lld", (long long)ldr, I);
    if (B == 0) return 0;
    if (!idx || !images || !rows) return kv_fail(KANVIT_EINVAL, "kanvit_patch_gather: null idx/images/rows");
    if (pd_mis(idx, 3) || pd_mis(images, 3) || pd_mis(rows, 3)) return kv_fail(KANVIT_EINVAL, "kanvit_patch_gather: idx/images/rows is not 4-byte aligned");
    PatchGatherArgs a = {};
    a.images = images; a.idx = idx; a.rows = rows; a.ldr = ldr;
    a.R = (int)(B * K); a.K = K;
    a.C = p->C; a.H = p->H; a.W = p->W; a.n = p->n_patches; a.ph = ph; a.pw = pw; a.I = (int)I;
    // float4 moves: a patch line is whole vectors (so are I, W and an image), and both tensors start and step in multiples of 16 bytes
    const bool vec = pw % 4 == 0 && ldr % 4 == 0 && !pd_mis(images, 15) && !pd_mis(rows, 15);
    a.lpr_log2 = pd_lpr_log2(vec ? a.I / 4 : a.I);
    const int grid = pd_row_grid(a.R, a.lpr_log2);
    if (vec) hipLaunchKernelGGL(patch_gather_kernel<4>, dim3(grid), dim3(PD_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(patch_gather_kernel<1>, dim3(grid), dim3(PD_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("patch_gather_kernel");
    return 0;
}

int kanvit_tokens_assemble_fwd(int64_t B, int K, int O, const float* tokens, int64_t ldt, const float* cls, const float* pos,
                               const int32_t* idx, float* out, void* stream) {
    if (K < 1 || O < 1) return kv_fail(KANVIT_EINVAL, "kanvit_tokens_assemble_fwd: K=%d O=%d must be >= 1", K, O);
    if (B < 0 || B * ((long long)K + 1) > 0x7fffffffll)
        return kv_fail(KANVIT_EINVAL, "kanvit_tokens_assemble_fwd: B=%lld: B >= 0 and B*(K+1) rows < 2^31", (long long)B);
    if (ldt < O) return kv_fail(KANVIT_EINVAL, "kanvit_tokens_assemble_fwd: ldt=%lld is below the row length O=%d", (long long)ldt, O);
    if (!cls || !pos) return kv_fail(KANVIT_EINVAL, "kanvit_tokens_assemble_fwd: null cls/pos");
    if (B == 0) return 0;
    if (!tokens || !idx || !out) return kv_fail(KANVIT_EINVAL, "kanvit_tokens_assemble_fwd: null tokens/idx/out");
    if (pd_mis(tokens, 3) || pd_mis(cls, 3) || pd_mis(pos, 3) || pd_mis(idx, 3) || pd_mis(out, 3))
        return kv_fail(KANVIT_EINVAL, "kanvit_tokens_assemble_fwd: a pointer is not 4-byte aligned");
    AssembleArgs a = {};
    a.tokens = tokens; a.cls = cls; a.pos = pos; a.idx = idx; a.out = out; a.ldt = ldt;
    a.R = (int)(B * (K + 1)); a.K = K; a.O = O;
    const bool vec = O % 4 == 0 && ldt % 4 == 0 && !pd_mis(tokens, 15) && !pd_mis(cls, 15) && !pd_mis(pos, 15) && !pd_mis(out, 15);
    a.lpr_log2 = pd_lpr_log2(vec ? O / 4 : O);
    const int grid = pd_row_grid(a.R, a.lpr_log2);
    if (vec) hipLaunchKernelGGL(tokens_assemble_fwd_kernel<4>, dim3(grid), dim3(PD_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(tokens_assemble_fwd_kernel<1>, dim3(grid), dim3(PD_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("tokens_assemble_fwd_kernel");
    return 0;
}

int kanvit_tokens_assemble_bwd(int64_t B, int K, int O, const float* dout, float* dtokens, float* dcls, void* stream) {
    if (K < 1 || O < 1) return kv_fail(KANVIT_EINVAL, "kanvit_tokens_assemble_bwd: K=%d O=%d must be >= 1", K, O);
    if (B < 0 || B * ((long long)K + 1) > 0x7fffffffll)
        return kv_fail(KANVIT_EINVAL, "kanvit_tokens_assemble_bwd: B=%lld: B >= 0 and B*(K+1) rows < 2^31", (long long)B);
    if ((B > 0 && !dout) || (!dtokens && !dcls)) return kv_fail(KANVIT_EINVAL, "kanvit_tokens_assemble_bwd: null dout, or neither dtokens nor dcls");
    if (pd_mis(dout, 3) || pd_mis(dtokens, 3) || pd_mis(dcls, 3))
        return kv_fail(KANVIT_EINVAL, "kanvit_tokens_assemble_bwd: a pointer is not 4-byte aligned");
    AssembleBwdArgs a = {};
    a.dout = dout; a.dtokens = dtokens; a.dcls = dcls;
    a.R = (int)(B * K); a.K = K; a.O = O; a.B = (int)B;
    const bool vec = O % 4 == 0 && !pd_mis(dout, 15) && !pd_mis(dtokens, 15);
    a.lpr_log2 = pd_lpr_log2(vec ? O / 4 : O);
    a.copy_groups = dtokens && a.R > 0 ? pd_row_grid(a.R, a.lpr_log2) : 0;
    const int grid = a.copy_groups + (dcls ? (O + PD_SUM_COLS - 1) / PD_SUM_COLS : 0);
    if (grid == 0) return 0;
    if (vec) hipLaunchKernelGGL(tokens_assemble_bwd_kernel<4>, dim3(grid), dim3(PD_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(tokens_assemble_bwd_kernel<1>, dim3(grid), dim3(PD_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("tokens_assemble_bwd_kernel");
    return 0;
}

}  // extern "C"
