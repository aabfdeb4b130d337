// Register-form forward of the fused KAN layers, exact fp32 (split out of kan_layer.hip; see kan_layer_common.h).
#include "kan_layer_common.h"

namespace {

// =============================================================================================
// forward, register-operand form (fp32 exact).  Because the fp32 MFMA and VALU work serialise on a SIMD no matter which
// wave issues them (section header above), nothing is gained by evaluating the basis in other waves -- and the LDS basis
// tile, its barriers and the producer waves are pure overhead.  Here every lane generates its own MFMA A operand:
//   the K index is permuted so that lane half hf owns whole features: k-step s of a chunk <-> (feature j = s / GP of the
//   half's ICH features, basis index g = s % GP); A[row = lane&31][k = hf] = phi_g(x[row][i0 + hf*ICH + j]) comes straight
//   from a BasisGen in registers, and the W chunk is staged with the same permutation (row (s, hf) <- k = feature*GP + g).
// 256 threads = 4 waves x 32 rows; LDS holds only two W chunk buffers (float4 global loads prefetched into registers one
// chunk ahead); x is read by each lane directly (ICH consecutive floats of its row per chunk); one barrier per chunk.
// Epilogue: the product is computed flipped (accumulator registers run along the output row), so every lane stores float4 row
// segments straight from its registers -- no transposition through the LDS.
// Requirements (plan_fwd_reg in kan_layer.hip): O % (32*NT) == 0, I % IC == 0, IC in {8, 4, 2}, 16-byte aligned rows when IC == 8.
// =============================================================================================
// GPC > 0: the number of basis functions per feature is a compile-time constant (the shapes the reference instantiates).  The
// chunk body is then fully unrolled and the W fragments are read from LDS ONE K-STEP AHEAD into a second register set, with
// scheduling fences pinning "reads of step s+1, then MFMAs of step s": an LDS read takes ~100 cycles from issue to use and
// the round-1 form (read -> s_waitcnt lgkmcnt(0) -> two MFMAs, the same destination registers every time) left the matrix
// pipe idle for most of that on every second MFMA (59 % busy in the PMC pass).  GPC == 0 keeps the runtime-GP loop.
// The body takes its block coordinates as arguments: the kernel below hands the LAST row tiles of a shared-basis (NSH = 3) launch
// to the NSH = 1 body, one projection per work-group (kv_tail_first_tile).
template <int FAM, int NT, int NSH, int ICH, int GPC, int ACT>
__device__ __forceinline__ void kan_fwd_reg_body(const LayerArgs& a, float* __restrict__ smem, const int bx, const int by) {
    constexpr int BN = 32 * NT;
    constexpr int WROW = NSH * BN;
    constexpr int V4 = BN / 4;
    constexpr int IC = 2 * ICH;
    constexpr bool RBF = (FAM == KV_RBF);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hf = lane >> 5;
    const int ntn = a.O / BN;
    const int gs = bx / ntn;
    const int n0 = (bx - gs * ntn) * BN;
    const int nsets = a.groups / NSH;
    const long long m0 = (long long)by * BM;
    // CHEBY: T0 = cos(0 * acos t) is the constant 1, so the g = 0 k rows only add the per-column constant b[o] = sum_i W[i*GP][o].
    // The GPC instantiation contracts g >= 1 on the matrix cores and sums those rows on the VALU of the staging threads (below).
    constexpr int G0 = (FAM == KV_CHEBY && GPC > 0) ? 1 : 0;
    const int GP = GPC > 0 ? GPC : a.GP, GPE = GP - G0, KC = IC * GPE;      // k rows per chunk (even); compile-time in the GPC instantiations (host: a.GP == GPC)
    const int nch = a.I / IC;
    const int WSZ = KC * WROW;
    const int mrem = (m0 + BM <= a.M) ? BM : (int)(a.M - m0);
    float* W_s = smem;                            // [2][KC][WROW], row (2s + hf)

    const BasisArgs b = make_basis(a, gs);
    const int xcol = (NSH == 1 ? gs % a.xmod : gs) * a.I;
    const int row = wave * 32 + l31;
    const bool row_ok = row < mrem;
    const float* xrow = a.x + (m0 + (row_ok ? row : 0)) * a.ldx + xcol + hf * ICH;
    const float* urow = (RBF && a.u) ? a.u + (m0 + (row_ok ? row : 0)) * a.ldu + (long long)gs * a.I + hf * ICH : xrow;
    // patch gather: the lane's row is a patch of an NCHW image; its ICH features of a chunk are ICH consecutive pixels of one
    // image line (host-checked: the chunk width divides the patch width), and the chunks are visited in order, so the
    // position inside the patch advances incrementally: no division in the chunk loop
    long long yrow = m0 + row;                    // output row of this lane's input row
    const float* posrow = nullptr;                // position embedding row added to it
    bool cls_owner = false;                       // this lane also writes its sample's class-token row
    float ln_mean = 0.0f, ln_rstd = 1.0f;        // KANVIT_FLAG_FUSED_LN: statistics of this lane's row over the group's x slice
    const float* ln_gb = nullptr;                 // gamma of this lane's first feature (beta I floats further on)
    if constexpr (RBF) {
        if (a.ln) {
            kv_ln_row_stats<ICH>(xrow, nch, a.I, a.ln_eps, ln_mean, ln_rstd);
            ln_gb = b.bp + a.G + hf * ICH;
            if (hf == 0 && row_ok && gs < a.xmod) {
                float2 st = {ln_mean, ln_rstd};
                *reinterpret_cast<float2*>(a.stats + ((m0 + row) * a.xmod + gs) * 2) = st;
            }
        }
    }
    int pg_ix = 0, pg_iy = 0, pg_off = 0, pg_pw = 0, pg_ph = 0;
    if (a.pg) {
        const int P = a.pg_n * a.pg_n;
        pg_ph = a.pg_H / a.pg_n;
        pg_pw = a.pg_W / a.pg_n;
        const long long m = m0 + (row_ok ? row : 0);
        const long long smp = m / P;
        const int pidx = (int)(m - smp * P);
        const int py = pidx / a.pg_n, px = pidx - py * a.pg_n;
        xrow = a.x + ((smp * a.pg_C) * a.pg_H + (long long)py * pg_ph) * a.pg_W + px * pg_pw;      // patch origin in channel 0
        pg_ix = pg_off = hf * ICH;
        yrow = m + (smp + 1) * a.pg_pre;
        posrow = a.pos ? a.pos + (long long)(pidx + a.pg_pre) * a.O : nullptr;
        cls_owner = a.pg_pre && a.cls && pidx == 0;
    }

    // W staging: thread -> (LDS row lr = tid / V4 (+ 256/V4 per pass), 4 columns wc); LDS row (s, h) <- global k
    const int wc = (tid & (V4 - 1)) * 4, wr0 = tid / V4;
    constexpr int WRS = 256 / V4;
    constexpr int WQ = (NSH == 3) ? 4 : 8;        // passes held in registers (host guarantees ceil(KC / WRS) <= WQ)
    f32x4 wreg[NSH][WQ];
    int koff[WQ];                                 // natural k offset (times O) of the LDS rows this thread stages, or -1
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
        const int lr = wr0 + q * WRS;             // LDS row = 2*s + h
        const int s_ = lr >> 1, h_ = lr & 1;
        const int j_ = s_ / GPE, g_ = s_ - j_ * GPE + G0;
        koff[q] = (lr < KC) ? ((h_ * ICH + j_) * GP + g_) * a.O : -1;
    }
    // CHEBY T0 rows: thread tid < WROW sums the rows of features NB0*part .. NB0*part + NB0-1 of every chunk (part = tid / (WROW/4)) for
    // the 4 columns cc of the work-group's WROW; the four parts are added in a fixed order after the loop.  The order of every column's
    // sum does not depend on NSH, so the NSH = 1 tail pieces form the same bits as the shared launch.
    constexpr int NB0 = G0 ? IC / 4 : 1;
    static_assert(!G0 || (IC % 4 == 0 && WROW <= 256), "T0 sums: four parts of a chunk, one thread per part and 4 columns");
    const int t0t = tid % WROW, t0part = t0t / (WROW / 4), t0cc = (t0t % (WROW / 4)) * 4;
    const int t0g = (NSH == 1) ? gs : (t0cc / BN) * nsets + gs;
    const float* t0src = a.w + (long long)t0g * a.K * a.O + (long long)(t0part * NB0) * GP * a.O + n0 + t0cc % BN;
    f32x4 w0reg[NB0];
    f32x4 bpart = {0.0f, 0.0f, 0.0f, 0.0f};
    auto load_w = [&](int c) {
#pragma unroll
        for (int p = 0; p < NSH; ++p) {
            const int g = (NSH == 1) ? gs : p * nsets + gs;
            const float* src = a.w + ((long long)g * a.K + (long long)c * IC * GP) * a.O + n0 + wc;      // chunk base (natural k order)
#pragma unroll
            for (int q = 0; q < WQ; ++q)      // unconditional: a predicated load is a branch around it plus an s_waitcnt vmcnt(1) in front of every
                if (q * WRS < KC)             // load (two in flight instead of all of them); rows past KC re-read row 0 and are never stored
                    wreg[p][q] = *reinterpret_cast<const f32x4*>(src + (koff[q] >= 0 ? koff[q] : 0));
        }
        if constexpr (G0 > 0) {                   // every thread loads (threads past WROW repeat a column and never add)
#pragma unroll
            for (int r = 0; r < NB0; ++r) w0reg[r] = *reinterpret_cast<const f32x4*>(t0src + ((long long)c * IC + r) * GP * a.O);
        }
    };
    auto store_w = [&](int buf) {
        float* dst = W_s + buf * WSZ + wc;
#pragma unroll
        for (int p = 0; p < NSH; ++p)
#pragma unroll
            for (int q = 0; q < WQ; ++q)
                if (koff[q] >= 0) *reinterpret_cast<f32x4*>(dst + (wr0 + q * WRS) * WROW + p * BN) = wreg[p][q];
        if constexpr (G0 > 0) {                   // the chunk's T0 rows of this part, in feature order
#pragma unroll
            for (int r = 0; r < NB0; ++r) bpart += w0reg[r];
        }
    };

    f32x16 acc[NSH * NT];
#pragma unroll
    for (int t = 0; t < NSH * NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    float xv[ICH], uv[ICH];
    auto load_x = [&](int c) {                    // called for c = 0, 1, 2, ... in order
        const float* xs = a.pg ? xrow + pg_off : xrow + c * IC;
        if constexpr (ICH == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(xs);
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[e] = v[e];
            if (RBF && !a.ln) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(urow + c * IC);
#pragma unroll
                for (int e = 0; e < 4; ++e) uv[e] = w4[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < ICH; ++e) {
                xv[e] = xs[e];
                if (RBF && !a.ln) uv[e] = urow[c * IC + e];
            }
        }
        if constexpr (RBF) {
            if (a.ln) {                           // u = (x - mean) * rstd * gamma + beta, the operation order of nn.LayerNorm
#pragma unroll
                for (int e = 0; e < ICH; ++e) uv[e] = (xv[e] - ln_mean) * ln_rstd * ln_gb[c * IC + e] + ln_gb[a.I + c * IC + e];
            }
        }
        if (a.pg) {                               // next chunk: IC pixels further along the line, then next line, then next channel
            pg_ix += IC;
            pg_off += IC;
            if (pg_ix >= pg_pw) {
                pg_ix -= pg_pw;
                pg_off += a.pg_W - pg_pw;
                if (++pg_iy == pg_ph) {
                    pg_iy = 0;
                    pg_off += (a.pg_H - pg_ph) * a.pg_W;
                }
            }
        }
    };

    // SINE with a compile-time basis size: the phases p[i][g] of the chunk's features travel one chunk ahead like x.  Read inside
    // the basis evaluation they are issued AFTER the next chunk's W / x prefetch, and memory returns in order: every chunk then
    // began by waiting for its own prefetch (s_waitcnt vmcnt(3) behind eight 16-byte loads).
    constexpr bool SINE_PH = (FAM == KV_SINE && GPC > 0);
    constexpr int NPH = SINE_PH ? ICH * GPC : 1;
    float phv[NPH];
    auto load_ph = [&](int c) {
        if constexpr (SINE_PH) {
            const float* ps = b.bp + GPC + (long long)(c * IC + hf * ICH) * GPC;      // [ICH features][GPC phases], contiguous
            if constexpr ((ICH * GPC) % 4 == 0) {
#pragma unroll
                for (int e4 = 0; e4 < NPH / 4; ++e4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(ps + 4 * e4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) phv[4 * e4 + e] = v[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < NPH; ++e) phv[e] = ps[e];
            }
        }
    };

    load_w(0);
    load_x(0);
    load_ph(0);
    store_w(0);
    __syncthreads();

    for (int c = 0; c < nch; ++c) {
        float xc[ICH], uc[ICH], phc[NPH];
#pragma unroll
        for (int e = 0; e < ICH; ++e) {
            xc[e] = xv[e];
            uc[e] = RBF ? uv[e] : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < NPH; ++e) phc[e] = phv[e];
        if (c + 1 < nch) {                        // prefetch the next chunk; lands while this chunk's MFMAs run
            load_w(c + 1);
            load_x(c + 1);
            load_ph(c + 1);
        }
        const float* wp = W_s + (c & 1) * WSZ + hf * WROW + l31;
        if constexpr (GPC > 0) {
            constexpr int GPCE = GPC - G0;
            constexpr int VH = ICH * GPCE;              // k-steps of this chunk (one generated value per lane and step)
            constexpr int NTT = NSH * NT;
            float phi[VH];
#pragma unroll
            for (int j = 0; j < ICH; ++j) {
                BasisGen<FAM, kv_gc(FAM, GPC), ACT> gen;       // compile-time G: one base activation per feature, no branch per value (host-checked has_base)
                gen.init(b, xc[j], uc[j], c * IC + hf * ICH + j);
#pragma unroll
                for (int g = 0; g < GPC; ++g) {
                    if constexpr (SINE_PH) phi[j * GPC + g] = kv_sin(__fadd_rn(__fmul_rn(xc[j], b.bp[g]), phc[j * GPC + g]));      // BasisGen<KV_SINE>::next with the phase from registers
                    else {
                        const float v = gen.next(g);      // (CHEBY: next(0) is the constant 1, folded away)
                        if (g >= G0) phi[j * GPCE + g - G0] = v;
                    }
                }
            }
            float wa[2][NTT];
#pragma unroll
            for (int t = 0; t < NTT; ++t) wa[0][t] = wp[t * 32];
#pragma unroll
            for (int s2 = 0; s2 < VH; ++s2) {
                if (s2 + 1 < VH) {
#pragma unroll
                    for (int t = 0; t < NTT; ++t) wa[(s2 + 1) & 1][t] = wp[(2 * (s2 + 1)) * WROW + t * 32];
                }
                __builtin_amdgcn_sched_barrier(0);      // the reads of step s2+1 are issued before the MFMAs of step s2 ...
#pragma unroll
                for (int t = 0; t < NTT; ++t)           // flipped product Y^T = W^T . Phi^T: accumulator rows = y columns
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[s2 & 1][t], phi[s2], acc[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);      // ... and nothing else is hoisted across (register budget: 2 waves per SIMD)
            }
        } else {
#pragma unroll
        for (int j = 0; j < ICH; ++j) {
            BasisGen<FAM, -1, ACT> gen;
            gen.init(b, xc[j], uc[j], c * IC + hf * ICH + j);
            const float* wj = wp + (2 * j * GP) * WROW;
            for (int g = 0; g < GP; ++g) {
                const float av = gen.next(g);
#pragma unroll
                for (int t = 0; t < NSH * NT; ++t)      // flipped product Y^T = W^T . Phi^T: accumulator rows = y columns
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wj[(2 * g) * WROW + t * 32], av, acc[t], 0, 0, 0);
            }
        }
        }
        if (c + 1 < nch) store_w((c + 1) & 1);
        __syncthreads();
    }

    // CHEBY: b = ((part 0 + part 1) + part 2) + part 3 per column, through the LDS (the W buffers are dead after the last barrier)
    float* b_s = smem + 4 * WROW;                 // [WROW]; the parts at [4][WROW] in front of it
    if constexpr (G0 > 0) {
        if (tid < WROW) *reinterpret_cast<f32x4*>(smem + t0part * WROW + t0cc) = bpart;
        __syncthreads();
        if (tid < WROW / 4) {
            const f32x4 s = ((*reinterpret_cast<const f32x4*>(smem + t0cc) + *reinterpret_cast<const f32x4*>(smem + WROW + t0cc)) +
                             *reinterpret_cast<const f32x4*>(smem + 2 * WROW + t0cc)) + *reinterpret_cast<const f32x4*>(smem + 3 * WROW + t0cc);
            *reinterpret_cast<f32x4*>(b_s + t0cc) = s;
        }
        __syncthreads();
    }

    // epilogue: with the flipped product, accumulator registers 4q..4q+3 of a tile are 4 consecutive y columns of the lane's
    // OWN row (column 8q + 4hf + 0..3 of the tile): float4 stores straight from registers, no staging tile, no barrier
    if (row < mrem) {
#pragma unroll
        for (int t = 0; t < NSH * NT; ++t) {
            const int p = t / NT, nt = t - p * NT;
            const int g = (NSH == 1) ? gs : p * nsets + gs;
            const int col = n0 + nt * 32 + 4 * hf;
            float* yp = a.y + yrow * a.ldy + (long long)g * a.O + col;
            const float* bp = a.bias ? a.bias + (long long)g * a.O + col : nullptr;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v = {acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]};
                if constexpr (G0 > 0) v += *reinterpret_cast<const f32x4*>(b_s + t * 32 + 8 * q + 4 * hf);
                if (bp) v += *reinterpret_cast<const f32x4*>(bp + 8 * q);
                if (posrow) v += *reinterpret_cast<const f32x4*>(posrow + col + 8 * q);
                *reinterpret_cast<f32x4*>(yp + 8 * q) = v;
                if (cls_owner) {                  // the class-token row of this sample: cls + pos[0] (model.py:150-152), this column tile
                    f32x4 cv = *reinterpret_cast<const f32x4*>(a.cls + col + 8 * q);
                    if (a.pos) cv += *reinterpret_cast<const f32x4*>(a.pos + col + 8 * q);
                    *reinterpret_cast<f32x4*>(yp - a.ldy + 8 * q) = cv;
                }
            }
        }
    }
}

// TAIL (NSH = 3 only): grid rows [tail_y0, ...) are the sub-divided end of the launch -- row tile tail_y0 + t / 3, projection t % 3,
// run by the one-projection body (it re-evaluates the basis; same k order per output, so the results are bitwise the shared ones).
template <int FAM, int NT, int NSH, int ICH, int GPC, bool TAIL, int ACT>
__device__ __forceinline__ void kan_fwd_reg_kbody(const LayerArgs& a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if constexpr (TAIL) {
        static_assert(NSH == 3, "the tail hands single projections of a shared-basis launch to the NSH = 1 body");
        const int ty = (int)blockIdx.y - a.tail_y0;
        if (ty >= 0) {
            const int tile = ty / 3, proj = ty - 3 * tile;
            kan_fwd_reg_body<FAM, NT, 1, ICH, GPC, ACT>(a, smem, proj * (int)gridDim.x + (int)blockIdx.x, a.tail_y0 + tile);
            return;
        }
    }
    kan_fwd_reg_body<FAM, NT, NSH, ICH, GPC, ACT>(a, smem, (int)blockIdx.x, (int)blockIdx.y);
}
template <int FAM, int NT, int NSH, int ICH, int GPC = 0, bool TAIL = false>
__global__ __launch_bounds__(256, GPC ? 2 : 1) void kan_fwd_reg_kernel(const LayerArgs a) {
    kan_fwd_reg_kbody<FAM, NT, NSH, ICH, GPC, TAIL, KV_ACT_SILU>(a);
}
// the same kernel for a BSPLINE / RBF base activation other than SiLU (code in the launch arguments)
template <int FAM, int NT, int NSH, int ICH, int GPC = 0, bool TAIL = false>
__global__ __launch_bounds__(256, GPC ? 2 : 1) void kan_fwd_reg_act_kernel(const LayerArgs a) {
    kan_fwd_reg_kbody<FAM, NT, NSH, ICH, GPC, TAIL, KV_ACT_DYN>(a);
}

// ---- register-operand forward (fp32 exact): launches what plan_fwd_reg (kan_layer.hip) chose --------------------------
template <int FAM, int NT, int NSH, int ICH, int GPC = 0>
int launch_fwd_reg(const LayerArgs& a, const LayerFwdPlan& p, hipStream_t st) {
    const dim3 grid(p.gx, p.gy, 1);
    if constexpr (NSH == 3 && GPC > 0) {
        if (p.tail_y0 != 0x7fffffff) {            // a.tail_y0 = p.tail_y0: the sub-divided end of the launch
            KV_ACT_ALLOW_LDS(FAM, a.base_act, 160 * 1024, kan_fwd_reg_kernel, kan_fwd_reg_act_kernel, (FAM, NT, NSH, ICH, GPC, true));
            KV_ACT_LAUNCH(FAM, a.base_act, kan_fwd_reg_kernel, kan_fwd_reg_act_kernel, (FAM, NT, NSH, ICH, GPC, true), grid, dim3(256), p.lds, st, a);
            KV_LAUNCH_CHECK("kan_fwd_reg_kernel");
            return 0;
        }
    }
    KV_ACT_ALLOW_LDS(FAM, a.base_act, 160 * 1024, kan_fwd_reg_kernel, kan_fwd_reg_act_kernel, (FAM, NT, NSH, ICH, GPC));
    KV_ACT_LAUNCH(FAM, a.base_act, kan_fwd_reg_kernel, kan_fwd_reg_act_kernel, (FAM, NT, NSH, ICH, GPC), grid, dim3(256), p.lds, st, a);
    KV_LAUNCH_CHECK("kan_fwd_reg_kernel");
    return 0;
}

// the instantiations: p.gpc > 0 names the pipelined compile-time-GP twin of (family, ICH) in KV_REG_BASES, 0 the run-time-GP loop
template <int FAM, int NT, int NSH>
int launch_fwd_reg_ich(const LayerArgs& a, const LayerFwdPlan& p, hipStream_t st) {
    if (p.gpc && p.ich == 4) {
        if constexpr (FAM == KV_LINEAR) return launch_fwd_reg<FAM, NT, NSH, 4, 1>(a, p, st);
        if constexpr (FAM == KV_CHEBY) return launch_fwd_reg<FAM, NT, NSH, 4, 5>(a, p, st);
        if constexpr (FAM == KV_BSPLINE || FAM == KV_RBF) return launch_fwd_reg<FAM, NT, NSH, 4, 9>(a, p, st);
        if constexpr (FAM == KV_SINE) return launch_fwd_reg<FAM, NT, NSH, 4, 4>(a, p, st);
    }
    if (p.gpc && p.ich == 2) {
        if constexpr (FAM == KV_BSPLINE || FAM == KV_RBF) return launch_fwd_reg<FAM, NT, NSH, 2, 9>(a, p, st);
    }
    if (p.gpc && p.ich == 1) {
        if constexpr (FAM == KV_SINE) return launch_fwd_reg<FAM, NT, NSH, 1, 28>(a, p, st);
        if constexpr (FAM == KV_FOURIER) return launch_fwd_reg<FAM, NT, NSH, 1, 56>(a, p, st);
    }
    if (p.gpc) return kv_fail(KANVIT_EINVAL, "internal: no register forward <family %d, ICH %d, GP %d>", FAM, p.ich, p.gpc);
    if (p.ich == 4) return launch_fwd_reg<FAM, NT, NSH, 4>(a, p, st);
    if (p.ich == 2) return launch_fwd_reg<FAM, NT, NSH, 2>(a, p, st);
    return launch_fwd_reg<FAM, NT, NSH, 1>(a, p, st);
}

template <int FAM>
int launch_fwd_reg_shape(const LayerArgs& a, const LayerFwdPlan& p, hipStream_t st) {
    if (p.nsh == 3) {
        if constexpr (kv_shared_basis<FAM>()) {
            if (p.nt == 1) return launch_fwd_reg_ich<FAM, 1, 3>(a, p, st);
            return launch_fwd_reg_ich<FAM, 2, 3>(a, p, st);
        }
    }
    if (p.nt == 1) return launch_fwd_reg_ich<FAM, 1, 1>(a, p, st);
    if (p.nt == 2) return launch_fwd_reg_ich<FAM, 2, 1>(a, p, st);
    return launch_fwd_reg_ich<FAM, 4, 1>(a, p, st);
}

}  // namespace

int kv_fwd_reg(int family, const LayerArgs& a, const LayerFwdPlan& p, hipStream_t st) {
#define KV_CALL(F) launch_fwd_reg_shape<F>(a, p, st)
    KV_FAMILY_SWITCH(family, KV_CALL)
#undef KV_CALL
}
