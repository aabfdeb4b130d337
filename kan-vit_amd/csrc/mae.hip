// Masked-autoencoder pretraining (He et al. 2022) on top of PatchDropout's keep table: the two passes the kept-token path lacks.
// Compiled inside the soft_ce unit (soft_ce.hip includes this file at its end, as addln.hip includes patch_drop.hip): the loss shares
// sc_ordered_sum, the row sum of soft_ce_mean_kernel, and the unit count of the build stays what the tests count.
//
//   kanvit_tokens_restore_fwd   out[B][P+1][O] = [y[b][0] + pos[0]; (y[b][1+j] if p == idx[b][j] else mask_token) + pos[1+p]]: the decoder's
//                               sequence, one fp32 add per element
//   kanvit_tokens_restore_bwd   dy = the rows of dout the kept tokens came from (a copy), dmask = the sum of the dropped rows in a fixed tree
//   kanvit_mae_loss             per dropped patch: target straight out of NCHW, per-patch normalisation, squared error and dpred in one walk;
//                               kept rows and the class row of dpred are written as +0; then the ordered mean over the masked patches
//
// idx is kanvit_patch_keep's table: every row strictly ascending, so "is p kept, and as which token" is a binary search of K entries that
// every lane of a row's sub-group makes on the same addresses (a broadcast).  The row kernels walk as patch_drop.hip's do: sub-groups of
// LPR = 2^k lanes per row, sub-group r of work-group g takes rows g * RPB + r, + gridDim * RPB, ...; VEC = 4 moves float4 where every
// address involved is a multiple of 16 bytes, VEC = 1 is the general form.

namespace {

constexpr int MAE_THREADS = 256;
constexpr int MAE_ROW_GRID = 2048;       // work-groups of the row kernels at most (8 per CU); further rows are further laps of the walk
constexpr int MAE_SUM_SLICES = 128;      // slices of the dmask sum: one thread each, per column vector
constexpr int MAE_SUM_CT = MAE_THREADS / MAE_SUM_SLICES;      // column vectors one work-group of the dmask part sums
constexpr int MAE_SUM_AHEAD = 8;         // rows a slice has in flight
static_assert(MAE_SUM_SLICES * MAE_SUM_CT == MAE_THREADS && (MAE_SUM_SLICES & (MAE_SUM_SLICES - 1)) == 0, "the slice tree halves");

template <int VEC>
struct MaeVec { typedef float type; };
template <>
struct MaeVec<4> { typedef f32x4 type; };

// number of entries of the ascending row ir[0..K) that are below p; p is kept iff that entry equals p
__device__ __forceinline__ int mae_lower_bound(const int* ir, int K, int p) {
    int lo = 0, hi = K;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ir[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct RestoreArgs {
    const float* y;             // [B][K + 1][O]
    const float* mask;          // [O]
    const float* pos;           // [P + 1][O]
    const int* idx;             // [B][K]
    float* out;                 // [B][P + 1][O]
    long long R;                // B * (P + 1) rows
    int P, K, O;
    int lpr_log2;
};

template <int VEC>
__global__ __launch_bounds__(MAE_THREADS) void tokens_restore_fwd_kernel(const RestoreArgs a) {
    typedef typename MaeVec<VEC>::type V;
    const int lpr = 1 << a.lpr_log2, rpb = MAE_THREADS >> a.lpr_log2;
    const int r = threadIdx.x >> a.lpr_log2, l = threadIdx.x & (lpr - 1);
    const int nv = a.O / VEC, N = a.P + 1, K = a.K;
    for (long long row = (long long)blockIdx.x * rpb + r; row < a.R; row += (long long)gridDim.x * rpb) {
        const long long b = row / N;
        const int t = (int)(row - b * N);
        const float* src = a.y + b * (K + 1) * a.O;               // the class row
        if (t > 0) {
            const int* ir = a.idx + b * K;
            const int j = mae_lower_bound(ir, K, t - 1);
            src = (j < K && ir[j] == t - 1) ? src + (long long)(1 + j) * a.O : a.mask;
        }
        const float* pr = a.pos + (long long)t * a.O;
        float* dst = a.out + row * a.O;
        for (int iv = l; iv < nv; iv += lpr) {
            const int o = iv * VEC;
            *reinterpret_cast<V*>(dst + o) = *reinterpret_cast<const V*>(src + o) + *reinterpret_cast<const V*>(pr + o);
        }
    }
}

struct RestoreBwdArgs {
    const float* dout;          // [B][P + 1][O]
    const int* idx;             // [B][K]
    float* dy;                  // [B][K + 1][O], or NULL
    float* dmask;               // [O], or NULL
    long long R;                // B * (K + 1) rows of dy
    long long n, per_slice;     // n = B * (P - K) dropped rows, per_slice = ceil(n / MAE_SUM_SLICES)
    int P, K, O;
    int lpr_log2, sum_groups;
};

// Work-groups [0, sum_groups) sum the mask-token gradient, the ones behind them copy dy's rows.
// The addition tree of dmask, per column: the n = B (P - K) dropped rows are numbered in (sample, ascending patch) order; slice s of 128
// adds rows s L .. min(n, (s + 1) L) - 1 to +0 in that order, L = ceil(n / 128); then the slices are folded in LDS, slice s += slice
// s + h for h = 64, 32, .. 1.  (B, P, K) fix n and L, so they fix the tree: the grid, the vector form and the clock have no say.
template <int VEC>
__global__ __launch_bounds__(MAE_THREADS) void tokens_restore_bwd_kernel(const RestoreBwdArgs a) {
    typedef typename MaeVec<VEC>::type V;
    __shared__ V part[MAE_SUM_SLICES][MAE_SUM_CT];
    const int P = a.P, K = a.K, D = a.P - a.K;
    if ((int)blockIdx.x >= a.sum_groups) {
        const int lpr = 1 << a.lpr_log2, rpb = MAE_THREADS >> a.lpr_log2;
        const int r = threadIdx.x >> a.lpr_log2, l = threadIdx.x & (lpr - 1);
        const int nv = a.O / VEC, N = K + 1;
        const long long g = (long long)blockIdx.x - a.sum_groups, groups = (long long)gridDim.x - a.sum_groups;
        for (long long row = g * rpb + r; row < a.R; row += groups * rpb) {
            const long long b = row / N;
            const int j = (int)(row - b * N);
            const float* src = a.dout + (b * (P + 1) + (j ? 1 + a.idx[b * K + j - 1] : 0)) * a.O;
            float* dst = a.dy + row * a.O;
            for (int iv = l; iv < nv; iv += lpr) *reinterpret_cast<V*>(dst + iv * VEC) = *reinterpret_cast<const V*>(src + iv * VEC);
        }
        return;
    }
    const int ct = threadIdx.x % MAE_SUM_CT, s = threadIdx.x / MAE_SUM_CT;
    const int o = ((int)blockIdx.x * MAE_SUM_CT + ct) * VEC;
    const long long first = s * a.per_slice, last = first + a.per_slice < a.n ? first + a.per_slice : a.n;
    V acc = {};
    if (o < a.O && first < last) {
        long long b = first / D;
        int r = (int)(first - b * D);
        const int* ir = a.idx + b * K;
        // the r-th dropped patch of the sample: j kept patches lie before it, the entries with ir[j] - j <= r (ascending in j)
        int j = 0, hi = K;
        while (j < hi) {
            const int mid = (j + hi) >> 1;
            if (ir[mid] - mid <= r) j = mid + 1;
            else hi = mid;
        }
        int p = r + j;
        for (long long left = last - first; left > 0; left -= MAE_SUM_AHEAD) {
            const int m = left < MAE_SUM_AHEAD ? (int)left : MAE_SUM_AHEAD;
            const float* src[MAE_SUM_AHEAD];
            V v[MAE_SUM_AHEAD];
#pragma unroll
            for (int u = 0; u < MAE_SUM_AHEAD; ++u) {
                if (u < m) {                                     // rows below n only: b < B and the table is read inside its B rows
                    while (j < K && ir[j] == p) ++j, ++p;
                    src[u] = a.dout + (b * (P + 1) + 1 + p) * a.O + o;
                    ++p;
                    if (++r == D) ++b, r = 0, p = 0, j = 0, ir += K;
                }
            }
#pragma unroll
            for (int u = 0; u < MAE_SUM_AHEAD; ++u)
                if (u < m) v[u] = *reinterpret_cast<const V*>(src[u]);
#pragma unroll
            for (int u = 0; u < MAE_SUM_AHEAD; ++u)
                if (u < m) acc += v[u];
        }
    }
    part[s][ct] = acc;
    __syncthreads();
    for (int h = MAE_SUM_SLICES / 2; h > 0; h >>= 1) {
        if (s < h) part[s][ct] += part[s + h][ct];
        __syncthreads();
    }
    if (s == 0 && o < a.O) *reinterpret_cast<V*>(a.dmask + o) = part[0][ct];
}

struct MaeLossArgs {
    const float* images;        // [B][C][H][W]
    const float* pred;          // [B][P + 1][I]
    const int* idx;             // [B][K]
    float* rows;                // [B][P]
    float* dpred;               // [B][P + 1][I]
    float* loss;
    long long R, n_rows;        // R = B * (P + 1) rows of pred, n_rows = B * P entries of rows
    int P, K, C, H, W, n, ph, pw, I;
    int norm_pix;
    float scale, divisor;       // 2 / (I B (P - K)) rounded once on the host; float(B (P - K))
};

// One wave per row of pred, four rows per work-group; a lane holds elements (lane + 64 e) VEC .. + VEC - 1, e < NE, of the row's patch
// in registers: the target is read once for the mean, the variance and the error.  A row's bits depend on the row alone: fixed lane
// assignment, fixed xor-shuffle trees.  The element decomposition (channel, line, column) is done once per lane, outside the row loop.
template <int VEC, int NE>
__global__ __launch_bounds__(MAE_THREADS) void mae_loss_kernel(const MaeLossArgs a) {
    typedef typename MaeVec<VEC>::type V;
    const int lane = threadIdx.x & 63, I = a.I, P = a.P, K = a.K, N = a.P + 1;
    const int plane = a.ph * a.pw;
    const long long image = (long long)a.C * a.H * a.W;
    int off[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int i = (lane + 64 * e) * VEC;
        const int c = i / plane, rem = i - c * plane, iy = rem / a.pw, ix = rem - iy * a.pw;
        off[e] = (c * a.H + iy) * a.W + ix;                      // used where i < I only
    }
    for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < a.R; row += (long long)gridDim.x * 4) {
        const long long b = row / N;
        const int t = (int)(row - b * N), p = t - 1;
        float* dz = a.dpred + row * I;
        bool kept = t == 0;
        if (!kept) {
            const int* ir = a.idx + b * K;
            const int j = mae_lower_bound(ir, K, p);
            kept = j < K && ir[j] == p;
        }
        if (kept) {                                              // the class row and the kept patches: no error, no gradient
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = (lane + 64 * e) * VEC;
                if (i < I) *reinterpret_cast<V*>(dz + i) = V{};
            }
            if (t > 0 && lane == 0) a.rows[b * P + p] = 0.f;
            continue;
        }
        const int py = p / a.n, px = p - py * a.n;
        const float* src = a.images + b * image + (long long)py * a.ph * a.W + px * a.pw;
        const float* z = a.pred + row * I;
        V tv[NE];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = (lane + 64 * e) * VEC;
            tv[e] = V{};
            if (i < I) {
                tv[e] = *reinterpret_cast<const V*>(src + off[e]);
                if constexpr (VEC == 4) s += (tv[e][0] + tv[e][1]) + (tv[e][2] + tv[e][3]);
                else s += tv[e];
            }
        }
        float mu = 0.f, sd = 1.f;
        if (a.norm_pix) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            mu = s / (float)I;
            float q = 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = (lane + 64 * e) * VEC;
                if (i < I) {
                    const V d = tv[e] - mu;
                    if constexpr (VEC == 4) q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
                    else q += d * d;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
            sd = sqrtf(q / (float)(I - 1) + 1e-6f);              // unbiased, as Tensor.var; the epsilon keeps a constant patch finite
        }
        float err = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = (lane + 64 * e) * VEC;
            if (i < I) {
                const V that = a.norm_pix ? (tv[e] - mu) / sd : tv[e];
                const V d = *reinterpret_cast<const V*>(z + i) - that;
                if constexpr (VEC == 4) err += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
                else err += d * d;
                *reinterpret_cast<V*>(dz + i) = d * a.scale;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) err += __shfl_xor(err, o);
        if (lane == 0) a.rows[b * P + p] = err / (float)I;
    }
}

// loss = (the ordered sum of the B P entries of rows: soft_ce_mean_kernel's tree) / float(B (P - K)); kept entries are +0
__global__ __launch_bounds__(256) void mae_mean_kernel(const MaeLossArgs a) {
    const float s = sc_ordered_sum(a.rows, a.n_rows);
    if (threadIdx.x == 0) a.loss[0] = s / a.divisor;
}

// lanes of a sub-group: the power of two that covers nv vectors, a wave at most
int mae_lpr_log2(int nv) {
    int k = 0;
    while (k < 6 && (1 << k) < nv) ++k;
    return k;
}

int mae_row_grid(long long rows, int lpr_log2) {
    const long long rpb = MAE_THREADS >> lpr_log2;
    const long long g = (rows + rpb - 1) / rpb;
    return (int)(g < MAE_ROW_GRID ? g : MAE_ROW_GRID);
}

bool mae_mis(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

// the domain the two restore entry points share
int mae_restore_domain(const char* who, int64_t B, int P, int K, int O) {
    if (P < 2 || P > KANVIT_PATCH_KEEP_MAX_P)
        return kv_fail(KANVIT_EINVAL, "%s: P=%d: idx is kanvit_patch_keep's table, 2..%d patches", who, P, KANVIT_PATCH_KEEP_MAX_P);
    if (K < 1 || K >= P) return kv_fail(KANVIT_EINVAL, "%s: K=%d must be in 1..P-1=%d (at least one kept and one masked patch)", who, K, P - 1);
    if (O < 1) return kv_fail(KANVIT_EINVAL, "%s: O=%d must be >= 1", who, O);
    if (B < 0 || B * ((long long)P + 1) > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "%s: B=%lld: B >= 0 and B*(P+1) rows < 2^31", who, (long long)B);
    return 0;
}

template <int VEC>
void mae_loss_launch(const MaeLossArgs& a, int grid, hipStream_t st) {
    const int nv = (a.I + VEC - 1) / VEC;
    if (nv <= 64 * (VEC == 4 ? 1 : 2)) hipLaunchKernelGGL((mae_loss_kernel<VEC, VEC == 4 ? 1 : 2>), dim3(grid), dim3(MAE_THREADS), 0, st, a);
    else if (nv <= 64 * (VEC == 4 ? 4 : 16)) hipLaunchKernelGGL((mae_loss_kernel<VEC, VEC == 4 ? 4 : 16>), dim3(grid), dim3(MAE_THREADS), 0, st, a);
    else hipLaunchKernelGGL((mae_loss_kernel<VEC, KANVIT_MAE_MAX_I / 64 / VEC>), dim3(grid), dim3(MAE_THREADS), 0, st, a);
}

}  // namespace

extern "C" {

int kanvit_tokens_restore_fwd(int64_t B, int P, int K, int O, const float* y, const float* mask_token, const float* pos, const int32_t* idx,
                              float* out, void* stream) {
    if (const int rc = mae_restore_domain("kanvit_tokens_restore_fwd", B, P, K, O)) return rc;
    if (!mask_token || !pos) return kv_fail(KANVIT_EINVAL, "kanvit_tokens_restore_fwd: null mask_token/pos");
    if (B > 0 && (!y || !idx || !out)) return kv_fail(KANVIT_EINVAL, "kanvit_tokens_restore_fwd: null y/idx/out");
    if (mae_mis(y, 3) || mae_mis(mask_token, 3) || mae_mis(pos, 3) || mae_mis(idx, 3) || mae_mis(out, 3))
        return kv_fail(KANVIT_EINVAL, "kanvit_tokens_restore_fwd: a pointer is not 4-byte aligned");
    if (B == 0) return 0;
    RestoreArgs a = {};
    a.y = y; a.mask = mask_token; a.pos = pos; a.idx = idx; a.out = out;
    a.R = B * ((long long)P + 1); a.P = P; a.K = K; a.O = O;
    const bool vec = O % 4 == 0 && !mae_mis(y, 15) && !mae_mis(mask_token, 15) && !mae_mis(pos, 15) && !mae_mis(out, 15);
    a.lpr_log2 = mae_lpr_log2(vec ? O / 4 : O);
    const int grid = mae_row_grid(a.R, a.lpr_log2);
    if (vec) hipLaunchKernelGGL(tokens_restore_fwd_kernel<4>, dim3(grid), dim3(MAE_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(tokens_restore_fwd_kernel<1>, dim3(grid), dim3(MAE_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("tokens_restore_fwd_kernel");
    return 0;
}

int kanvit_tokens_restore_bwd(int64_t B, int P, int K, int O, const float* dout, const int32_t* idx, float* dy, float* dmask, void* stream) {
    if (const int rc = mae_restore_domain("kanvit_tokens_restore_bwd", B, P, K, O)) return rc;
    if (!dy && !dmask) return kv_fail(KANVIT_EINVAL, "kanvit_tokens_restore_bwd: null dy and dmask: neither gradient is wanted");
    if (B > 0 && (!dout || !idx)) return kv_fail(KANVIT_EINVAL, "kanvit_tokens_restore_bwd: null dout/idx");
    if (mae_mis(dout, 3) || mae_mis(idx, 3) || mae_mis(dy, 3) || mae_mis(dmask, 3))
        return kv_fail(KANVIT_EINVAL, "kanvit_tokens_restore_bwd: a pointer is not 4-byte aligned");
    RestoreBwdArgs a = {};
    a.dout = dout; a.idx = idx; a.dy = dy; a.dmask = dmask;
    a.R = B * ((long long)K + 1); a.P = P; a.K = K; a.O = O;
    a.n = B * (long long)(P - K);
    a.per_slice = (a.n + MAE_SUM_SLICES - 1) / MAE_SUM_SLICES;
    const bool vec = O % 4 == 0 && !mae_mis(dout, 15) && !mae_mis(dy, 15) && !mae_mis(dmask, 15);
    const int nv = vec ? O / 4 : O;
    a.lpr_log2 = mae_lpr_log2(nv);
    a.sum_groups = dmask ? (nv + MAE_SUM_CT - 1) / MAE_SUM_CT : 0;          // B = 0: the sum of no rows, dmask = +0
    const int grid = a.sum_groups + (dy && a.R > 0 ? mae_row_grid(a.R, a.lpr_log2) : 0);
    if (grid == 0) return 0;
    if (vec) hipLaunchKernelGGL(tokens_restore_bwd_kernel<4>, dim3(grid), dim3(MAE_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(tokens_restore_bwd_kernel<1>, dim3(grid), dim3(MAE_THREADS), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("tokens_restore_bwd_kernel");
    return 0;
}

int kanvit_mae_loss(const kanvit_patch_desc* p, int64_t B, int K, const int32_t* idx, const float* images, const float* pred, int norm_pix,
                    float* rows, float* loss, float* dpred, void* stream) {
    if (!p) return kv_fail(KANVIT_EINVAL, "kanvit_mae_loss: null descriptor");
    if (p->C < 1 || p->H < 1 || p->W < 1 || p->n_patches < 1 || p->H % p->n_patches || p->W % p->n_patches)
        return kv_fail(KANVIT_EINVAL, "kanvit_mae_loss: C=%d H=%d W=%d n_patches=%d: sizes >= 1, n_patches divides H and W", p->C, p->H, p->W,
                       p->n_patches);
    const int ph = p->H / p->n_patches, pw = p->W / p->n_patches;
    const long long I = (long long)p->C * ph * pw, P = (long long)p->n_patches * p->n_patches;
    if (K < 1 || K >= P) return kv_fail(KANVIT_EINVAL, "kanvit_mae_loss: K=%d must be in 1..P-1=%lld (at least one kept and one masked patch)", K, P - 1);
    if (I > KANVIT_MAE_MAX_I)
        return kv_fail(KANVIT_EINVAL, "kanvit_mae_loss: I=%lld values per patch: a wave holds one patch in registers, at most %d", I, KANVIT_MAE_MAX_I);
    if (I < 2 && norm_pix) return kv_fail(KANVIT_EINVAL, "kanvit_mae_loss: I=1 with norm_pix: one value has no variance");
    if (B < 1 || B * (P + 1) > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "kanvit_mae_loss: B=%lld: B >= 1 and B*(P+1) rows < 2^31", (long long)B);
    if ((long long)p->C * p->H * p->W > 0x7fffffffll) return kv_fail(KANVIT_EINVAL, "kanvit_mae_loss: an image of C*H*W >= 2^31 values");
    if (!idx || !images || !pred || !rows || !loss || !dpred) return kv_fail(KANVIT_EINVAL, "kanvit_mae_loss: null idx/images/pred/rows/loss/dpred");
    if (mae_mis(idx, 3) || mae_mis(images, 3) || mae_mis(pred, 3) || mae_mis(rows, 3) || mae_mis(loss, 3) || mae_mis(dpred, 3))
        return kv_fail(KANVIT_EINVAL, "kanvit_mae_loss: a pointer is not 4-byte aligned");
    MaeLossArgs a = {};
    a.images = images; a.pred = pred; a.idx = idx; a.rows = rows; a.dpred = dpred; a.loss = loss;
    a.R = B * (P + 1); a.n_rows = B * P;
    a.P = (int)P; a.K = K; a.C = p->C; a.H = p->H; a.W = p->W; a.n = p->n_patches; a.ph = ph; a.pw = pw; a.I = (int)I;
    a.norm_pix = norm_pix ? 1 : 0;
    const double masked = (double)B * (double)(P - K);
    a.scale = (float)(2.0 / ((double)I * masked));
    a.divisor = (float)masked;
    // float4 moves: a patch line is whole vectors (so are I, W and an image), and the three tensors start in multiples of 16 bytes
    const bool vec = pw % 4 == 0 && !mae_mis(images, 15) && !mae_mis(pred, 15) && !mae_mis(dpred, 15);
    const long long g = (a.R + 3) / 4;
    const int grid = (int)(g < MAE_ROW_GRID ? g : MAE_ROW_GRID);
    if (vec) mae_loss_launch<4>(a, grid, (hipStream_t)stream);
    else mae_loss_launch<1>(a, grid, (hipStream_t)stream);
    KV_LAUNCH_CHECK("mae_loss_kernel");
    hipLaunchKernelGGL(mae_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("mae_mean_kernel");
    return 0;
}

}  // extern "C"
