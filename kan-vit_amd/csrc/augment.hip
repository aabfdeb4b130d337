// A training batch from a dataset that lives in HBM as uint8: gather by index, random crop out of the zero-padded image, random
// horizontal flip, ToTensor and Normalize in ONE pass (kanvit/data.py).  The reference does this per sample on the host
// (train.py:100-118: RandomHorizontalFlip, RandomCrop(32, padding=4), ToTensor, Normalize) and copies every batch to the device.
//
//   out[b][c][y][x] = lut[c][ images[idx[b]][sy][sx'][c] ]   sy = y + dy - pad_y,  sx = x + dx - pad_x,  sx' = flip ? W-1-sx : sx
//                   = lut[c][0]  where (sy, sx) lies outside the image (the zero padding, normalised)
//
// (dy, dx, flip) are a pure function of (seed, epoch, idx[b]) -- three splitmix64 steps per thread, no RNG state, no second launch --
// so a sample's pixels do not depend on the batch size, its position in the batch or the rank.  lut[c][v] = ((v/255) - mean[c]) / std[c]
// is built by the host with the reference's own fp32 operations: a channel has 256 possible values, the kernel does no floating-point
// arithmetic, and the output equals the CPU transform bit for bit.
//
// The kernel is bound by its stores (4 bytes out per byte in).  Work item = VEC consecutive x of one (b, y, c) row, c inside y: the
// W/VEC * C lanes of one image row read one contiguous W*C-byte stretch of the NHWC source between them, and every lane stores
// VEC * 4 bytes (16 in the vector form) of a contiguous output row.
//
// The training loop's other off-model kernels live here too: the Mixup / CutMix form of the same pass (mix_u8_kernel), its resampling
// form (resample_u8_kernel: bilinear resize of a per-sample box to the model's size, RandomResizedCrop from a table), the fused
// soft-target cross-entropy (loss and gradient in one walk over a logits row) and the epoch metrics (softmax / argmax / confusion
// update per step, and the pair counts of the one-vs-rest ROC-AUC per epoch) and the fused AdamW step (global-norm clipping, schedule
// table, weight EMA: kanvit/optim.py), further down.
#include "../../include/kanvit.h"
#include "kanvit_common.h"

#include <type_traits>

namespace {

__host__ __device__ __forceinline__ unsigned long long aug_mix(unsigned long long z) {     // one splitmix64 step
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct AugArgs {
    const unsigned char* images;
    const long long* labels;
    const long long* idx;
    const float* lut;
    float* out;
    long long* y_out;
    int* params_out;
    long long N, B;
    int H, W, C, pad_y, pad_x, flip;
    unsigned long long seed_epoch;      // mix(mix(seed) + epoch): the part of the hash every sample shares
};

template <int VEC>
__global__ __launch_bounds__(256) void augment_u8_kernel(const AugArgs a) {
    __shared__ float lut[4 * 256];
    for (int i = threadIdx.x; i < a.C * 256; i += 256) lut[i] = a.lut[i];
    __syncthreads();
    const int WV = a.W / VEC, H = a.H, W = a.W, C = a.C;
    const long long total = a.B * H * C * WV;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long row = t / WV;                    // (b, y, c)
        const int x0 = (int)(t - row * WV) * VEC;
        const long long by = row / C;
        const int c = (int)(row - by * C);
        const long long b = by / H;
        const int y = (int)(by - b * H);
        const long long s = a.idx[b];
        const unsigned long long h = aug_mix(a.seed_epoch + (unsigned long long)s);
        const int dy = (int)((unsigned)(h & 0xFFFFFu) % (unsigned)(2 * a.pad_y + 1));
        const int dx = (int)((unsigned)((h >> 20) & 0xFFFFFu) % (unsigned)(2 * a.pad_x + 1));
        const int fl = a.flip ? (int)((h >> 40) & 1u) : 0;
        const bool sample_ok = s >= 0 && s < a.N;        // the caller validates idx; an entry outside the dataset is never dereferenced
        if (c == 0 && y == 0 && x0 == 0) {
            if (a.y_out) a.y_out[b] = (sample_ok && a.labels) ? a.labels[s] : -1;
            if (a.params_out) {
                a.params_out[3 * b + 0] = dy;
                a.params_out[3 * b + 1] = dx;
                a.params_out[3 * b + 2] = fl;
            }
        }
        const int sy = y + dy - a.pad_y;
        const bool row_ok = sample_ok && sy >= 0 && sy < H;
        const unsigned char* src = a.images + (((sample_ok ? s : 0) * H + (row_ok ? sy : 0)) * W) * C + c;     // not read when !row_ok
        const float* l = lut + c * 256;
        float v[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int sx = x0 + e + dx - a.pad_x;
            const bool ok = row_ok && sx >= 0 && sx < W;
            const int fx = fl ? W - 1 - sx : sx;
            const int byte = ok ? (int)src[(long long)fx * C] : 0;
            v[e] = l[byte];
        }
        float* o = a.out + ((b * C + c) * H + y) * W + x0;
        if constexpr (VEC == 4) {
            *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            o[0] = v[0];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Mixup / CutMix on the same pass (kanvit/data.py: mix_table).  The epoch's table names, per DATASET index s, a partner j (or -1), the
// weight w of s's own label and a box in output coordinates.  a = augment_u8's value for s, p = augment_u8's value for j with j's
// OWN crop and flip (the hash of (seed, epoch, j)), so both operands -- and with them the output -- are functions of (seed, epoch, s)
// and the table row alone, never of the batch:
//     out = a                                         j < 0
//     out = inside the box ? p : a                    box non-empty  (CutMix: look-ups only)
//     out = fadd(fmul(w, a), fmul(1 - w, p))          otherwise      (Mixup: three roundings, never contracted into an fma, so a
//                                                                     float32 restatement on the host gives the same bits)
// Same work item as augment_u8_kernel (VEC consecutive x of one (b, y, c) row), up to twice its reads for the same stores.
struct MixArgs {
    AugArgs g;
    const long long* partner;
    const float* weight;
    const int* box;
    long long* y2_out;
    float* w_out;
};

// aug_params / aug_fetch restate augment_u8_kernel's gather for one sample, so that the mix kernel can take it twice.  augment_u8_kernel
// keeps its own body: routed through them it compiles to 5 % more instructions, and it is the kernel every --data-npz step runs.
struct AugParams {
    int dy, dx, fl;
};

__device__ __forceinline__ AugParams aug_params(const AugArgs& a, long long s) {
    const unsigned long long h = aug_mix(a.seed_epoch + (unsigned long long)s);
    AugParams p;
    p.dy = (int)((unsigned)(h & 0xFFFFFu) % (unsigned)(2 * a.pad_y + 1));
    p.dx = (int)((unsigned)((h >> 20) & 0xFFFFFu) % (unsigned)(2 * a.pad_x + 1));
    p.fl = a.flip ? (int)((h >> 40) & 1u) : 0;
    return p;
}

// augment_u8's values of sample s (valid: s in [0, N)) at row y, channel c, columns x0 .. x0 + VEC - 1
template <int VEC>
__device__ __forceinline__ void aug_fetch(const AugArgs& a, const float* l, long long s, bool valid, int y, int c, int x0, float* v) {
    const AugParams q = aug_params(a, s);
    const int sy = y + q.dy - a.pad_y;
    const bool row_ok = valid && sy >= 0 && sy < a.H;
    const unsigned char* src = a.images + (((valid ? s : 0) * a.H + (row_ok ? sy : 0)) * a.W) * a.C + c;       // not read when !row_ok
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int sx = x0 + e + q.dx - a.pad_x;
        const bool ok = row_ok && sx >= 0 && sx < a.W;
        const int fx = q.fl ? a.W - 1 - sx : sx;
        v[e] = l[ok ? (int)src[(long long)fx * a.C] : 0];
    }
}

__device__ __forceinline__ float mix_blend(float w, float w1, float a, float p) {
#pragma clang fp contract(off)
    const float wa = __fmul_rn(w, a);
    const float wp = __fmul_rn(w1, p);
    return __fadd_rn(wa, wp);
}

template <int VEC>
__global__ __launch_bounds__(256) void mix_u8_kernel(const MixArgs m) {
    __shared__ float lut[4 * 256];
    const AugArgs& a = m.g;
    for (int i = threadIdx.x; i < a.C * 256; i += 256) lut[i] = a.lut[i];
    __syncthreads();
    const int WV = a.W / VEC, H = a.H, W = a.W, C = a.C;
    const long long total = a.B * H * C * WV;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long row = t / WV;                    // (b, y, c)
        const int x0 = (int)(t - row * WV) * VEC;
        const long long by = row / C;
        const int c = (int)(row - by * C);
        const long long b = by / H;
        const int y = (int)(by - b * H);
        const long long s = a.idx[b];
        const bool sample_ok = s >= 0 && s < a.N;        // as augment_u8: the caller validates idx and the table
        const long long j = sample_ok ? m.partner[s] : -1;
        const bool mixed = j >= 0 && j < a.N;            // a partner outside the dataset is never dereferenced: the row stays unmixed
        const float w = sample_ok ? m.weight[s] : 1.f;
        if (c == 0 && y == 0 && x0 == 0) {
            const long long lab = (sample_ok && a.labels) ? a.labels[s] : -1;
            if (a.y_out) a.y_out[b] = lab;
            if (m.y2_out) m.y2_out[b] = (mixed && a.labels) ? a.labels[j] : lab;
            if (m.w_out) m.w_out[b] = w;
        }
        const float* l = lut + c * 256;
        float v[VEC];
        aug_fetch<VEC>(a, l, s, sample_ok, y, c, x0, v);
        if (mixed) {
            const int* bx = m.box + 4 * s;
            const int y0 = bx[0], y1 = bx[1], bx0 = bx[2], bx1 = bx[3];
            const bool cut = y0 < y1 && bx0 < bx1;
            if (!cut || (y >= y0 && y < y1 && x0 < bx1 && x0 + VEC > bx0)) {     // CutMix rows and columns outside the box keep a
                float p[VEC];
                aug_fetch<VEC>(a, l, j, true, y, c, x0, p);
                const float w1 = 1.f - w;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    if (cut)
                        v[e] = (x0 + e >= bx0 && x0 + e < bx1) ? p[e] : v[e];
                    else
                        v[e] = mix_blend(w, w1, v[e], p[e]);
                }
            }
        }
        float* o = a.out + ((b * C + c) * H + y) * W + x0;
        if constexpr (VEC == 4) {
            *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            o[0] = v[0];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Bilinear resize / RandomResizedCrop to the model's size on the same pass (kanvit/data.py: crop_table).  The epoch's crop table
// names, per DATASET index s, a box (y0, x0, bh, bw, flip) of source pixels in the coordinates of the possibly flipped, zero-padded
// image; the output [OH][OW] is the bilinear resize of that box with half-pixel centres and the taps clamped to the box
// (F.interpolate(crop, size, mode="bilinear", align_corners=False, antialias=False)).  A tap's value is augment_u8's: lut[c][byte],
// lut[c][0] outside the image.  The fp32 operations are fixed and never contracted (include/kanvit.h states the sequence), so a float32
// restatement on the host gives the same bits, and at bh == OH, bw == OW the second weights are 0 and the output is the tap itself.
//
// The kernel is bound by the instructions it issues, not by its stores, so the work item is shaped to share them:
// VEC consecutive ox by RES_ROWS consecutive oy of one (b, c) plane.  What depends on the sample and the columns alone -- the index and
// table rows, the two divisions, the x taps and weights, the source byte offsets -- is computed once per item (ResCols::init), and a
// row costs its own y taps, its loads and the blend (ResCols::row); lanes that are neighbours in x store neighbouring 16 bytes of one
// output row.  Where the VEC = 4 outputs span at most RES_WIN source columns (always at 3x upsampling and beyond: four outputs then
// lie within 1 1/3 source pixels) each of the two source rows is fetched as a window of RES_WIN columns -- 6 byte loads and 6 table
// look-ups instead of 16 -- the eight taps are picked out of it with selects, and a window is kept for the next output row, which at
// 7x upsampling reads the same source rows six times out of seven.  Loads are unconditional at addresses clamped into the image, the
// padding rule is a select on the table index: no branch per tap.
// A thread walks the items t0, t0 + stride, ... with its position kept as the mixed-radix number (b, c, og, xg) and advanced by the
// stride's digits with carries: t0 and the stride are below 2^19 (2048 work-groups at the most), so the only divisions are 32-bit
// ones, once per thread.
constexpr int RES_WIN = 3, RES_ROWS = 4;

struct ResArgs {
    const unsigned char* images;
    const long long* labels;
    const long long* idx;
    const float* lut;
    const int* crop;            // [N][5] or null: (0, 0, H, W, 0) for every sample
    const long long* partner;   // the three mix tables: the <*, true> kernels only
    const float* weight;
    const int* box;
    float* out;
    long long* y_out;
    long long* y2_out;
    float* w_out;
    long long N, B, total;      // total work items
    int H, W, C, OH, OW;
};

struct ResAxis {
    int t0, t1;                 // the two taps, box-local
    float w0, w1;
};

// one axis of the resize: output coordinate o of an axis that maps n source pixels (scale = n / outputs)
__device__ __forceinline__ ResAxis res_axis(float scale, int o, int n) {
#pragma clang fp contract(off)
    const float src = fmaxf(__fsub_rn(__fmul_rn(scale, __fadd_rn((float)o, 0.5f)), 0.5f), 0.f);
    ResAxis r;
    r.t0 = min((int)src, n - 1);
    r.t1 = min(r.t0 + 1, n - 1);
    r.w1 = __fsub_rn(src, (float)r.t0);
    r.w0 = __fsub_rn(1.f, r.w1);
    return r;
}

// m ? hi : lo for m all ones or zero, as one bit-select on the vector unit: a mask kept in a vector register, where a lane mask per
// output would cost a scalar register pair each (the mixing form holds two ResCols and runs out of them)
__device__ __forceinline__ float res_select(unsigned m, float hi, float lo) {
    return __uint_as_float((m & __float_as_uint(hi)) | (~m & __float_as_uint(lo)));
}

__device__ __forceinline__ float res_blend(const ResAxis& x, const ResAxis& y, float t00, float t01, float t10, float t11) {
#pragma clang fp contract(off)
    const float top = __fadd_rn(__fmul_rn(x.w0, t00), __fmul_rn(x.w1, t01));
    const float bot = __fadd_rn(__fmul_rn(x.w0, t10), __fmul_rn(x.w1, t11));
    return __fadd_rn(__fmul_rn(y.w0, top), __fmul_rn(y.w1, bot));
}

// What the RES_ROWS rows of one work item share: sample s (valid: s in [0, N)) under ITS crop row at channel c, output columns
// x0 .. x0 + VEC - 1.
template <int VEC>
struct ResCols {
    bool ok;                    // a sample and a non-empty box: otherwise every value is padding and nothing is read
    bool win;                   // row<true> serves: the item's first taps are columns ub = rx[0].t0 and ub + 1 at the most (see init), or !ok
    int y0, x0, bh, bw, fl;
    int at0, at1;               // w0 / w1 hold the windows of source rows at0 / at1 (at first of row INT_MIN, which is all padding)
    float scale_y;
    const unsigned char* img;   // the sample's channel c
    ResAxis rx[VEC];
    int off[RES_WIN];           // byte offsets of the window's columns in a source row, clamped into it
    int keep[RES_WIN];          // ... and 0xFF where the column lies inside the image, 0 where it is padding (byte & keep: the table index)
    unsigned up[VEC];           // all ones where the output's first tap is column ub + 1, zero where it is ub
    float w0[RES_WIN], w1[RES_WIN];

    // box-local column u -> byte offset in a source row (clamped into the row: a load there is always inside the image) and the mask
    // of its byte.  Unsigned sum: a table row the caller did not validate wraps instead of overflowing.
    __device__ __forceinline__ int column(const ResArgs& a, int u, int& mask) const {
        const int sx = (int)((unsigned)x0 + (unsigned)u);
        mask = (sx >= 0 && sx < a.W) ? 0xFF : 0;
        const int fx = fl ? a.W - 1 - sx : sx;
        return min(max(fx, 0), a.W - 1) * a.C;
    }

    __device__ __forceinline__ void init(const ResArgs& a, const float* l, long long s, bool valid, int c, int ox0) {
        y0 = 0, x0 = 0, bh = a.H, bw = a.W, fl = 0;
        if (a.crop && valid) {
            const int* q = a.crop + 5 * s;
            y0 = q[0], x0 = q[1], bh = q[2], bw = q[3], fl = q[4];
        }
        ok = valid && bh >= 1 && bw >= 1;
        win = VEC == 4;
        if (!ok) return;
        scale_y = __fdiv_rn((float)bh, (float)a.OH);
        const float scale_x = __fdiv_rn((float)bw, (float)a.OW);
        img = a.images + s * a.H * a.W * a.C + c;
#pragma unroll
        for (int e = 0; e < VEC; ++e) rx[e] = res_axis(scale_x, ox0 + e, bw);
        if constexpr (VEC == 4) {
            // The taps do not decrease along x.  If the last output's first tap is ub or ub + 1, every output's taps are (ub, ub + 1) or
            // (ub + 1, ub + 2) with each column clamped to bw - 1 -- t1 = min(t0 + 1, bw - 1) -- so the window of columns
            // min(ub + k, bw - 1), k = 0, 1, 2, holds all eight taps of a source row, and an output picks its pair by t0 != ub.
            static_assert(RES_WIN == 3, "the window is the columns ub, ub + 1, ub + 2");
            const int ub = rx[0].t0;
            win = rx[3].t0 - ub <= 1;
            if (win) {
#pragma unroll
                for (int k = 0; k < RES_WIN; ++k) {
                    off[k] = column(a, min(ub + k, bw - 1), keep[k]);
                    w0[k] = w1[k] = l[0];
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e) up[e] = rx[e].t0 != ub ? ~0u : 0u;
                at0 = at1 = INT_MIN;                     // y0 + a tap reaches it only from an unvalidated table, and that row is padding too
            }
        }
    }

    // The values of output row oy.  WIN: through the windows, for an item with `win` (VEC == 4); otherwise tap by tap.  The two are
    // separate so that the kernel can run them in separate row loops: what either keeps across rows is live in its own loop only.
    template <bool WIN>
    __device__ __forceinline__ void row(const ResArgs& a, const float* l, int oy, float* v) {
        if (!ok) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = l[0];
            return;
        }
        const ResAxis ry = res_axis(scale_y, oy, bh);
        const int sy0 = (int)((unsigned)y0 + (unsigned)ry.t0), sy1 = (int)((unsigned)y0 + (unsigned)ry.t1);
        const int keep0 = (sy0 >= 0 && sy0 < a.H) ? 0xFF : 0, keep1 = (sy1 >= 0 && sy1 < a.H) ? 0xFF : 0;
        const long long pitch = (long long)a.W * a.C;
        const unsigned char* row0 = img + min(max(sy0, 0), a.H - 1) * pitch;       // clamped like the columns
        const unsigned char* row1 = img + min(max(sy1, 0), a.H - 1) * pitch;
        if constexpr (WIN) {
            if (at0 != sy0) {
#pragma unroll
                for (int k = 0; k < RES_WIN; ++k) w0[k] = l[(int)row0[off[k]] & keep0 & keep[k]];
                at0 = sy0;
            }
            if (at1 != sy1) {
#pragma unroll
                for (int k = 0; k < RES_WIN; ++k) w1[k] = l[(int)row1[off[k]] & keep1 & keep[k]];
                at1 = sy1;
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                v[e] = res_blend(rx[e], ry, res_select(up[e], w0[1], w0[0]), res_select(up[e], w0[2], w0[1]), res_select(up[e], w1[1], w1[0]),
                                 res_select(up[e], w1[2], w1[1]));
            return;
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            int m0, m1;
            const int o0 = column(a, rx[e].t0, m0), o1 = column(a, rx[e].t1, m1);
            v[e] = res_blend(rx[e], ry, l[(int)row0[o0] & keep0 & m0], l[(int)row0[o1] & keep0 & m1], l[(int)row1[o0] & keep1 & m0],
                             l[(int)row1[o1] & keep1 & m1]);
        }
    }
};

template <int VEC, bool MIX>
__global__ __launch_bounds__(256) void resample_u8_kernel(const ResArgs a) {
    __shared__ float lut[4 * 256];
    for (int i = threadIdx.x; i < a.C * 256; i += 256) lut[i] = a.lut[i];
    __syncthreads();
    const unsigned WV = (unsigned)a.OW / VEC, OG = ((unsigned)a.OH + RES_ROWS - 1) / RES_ROWS, C = (unsigned)a.C;
    const unsigned t0 = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    unsigned xg = t0 % WV, r = t0 / WV;                  // the item's digits (b, c, og, xg) ...
    unsigned og = r % OG;
    r /= OG;
    unsigned c = r % C;
    long long b = r / C;
    const unsigned s_xg = stride % WV, s_r = stride / WV, s_og = s_r % OG, s_c = (s_r / OG) % C, s_b = s_r / OG / C;      // ... and the stride's
    for (long long t = t0; t < a.total; t += stride) {
        const long long s = a.idx[b];
        const bool sample_ok = s >= 0 && s < a.N;        // the caller validates idx and the tables; nothing outside them is dereferenced
        const int x0 = (int)xg * VEC;
        const float* l = lut + c * 256;
        ResCols<VEC> own;
        own.init(a, l, s, sample_ok, (int)c, x0);
        const bool first = c == 0 && og == 0 && xg == 0;
        long long lab = -1;
        if (first) {
            if (sample_ok && a.labels) lab = a.labels[s];
            if (a.y_out) a.y_out[b] = lab;
        }
        [[maybe_unused]] ResCols<VEC> par;                // the partner under ITS crop row
        [[maybe_unused]] bool mixed = false, cut = false;
        [[maybe_unused]] int by0 = 0, by1 = 0, bx0 = 0, bx1 = 0;
        [[maybe_unused]] float w = 1.f, w1 = 0.f;
        if constexpr (MIX) {
            const long long j = sample_ok ? a.partner[s] : -1;
            mixed = j >= 0 && j < a.N;                   // a partner outside the dataset is never dereferenced: the row stays unmixed
            w = sample_ok ? a.weight[s] : 1.f;
            w1 = 1.f - w;
            if (first) {
                if (a.y2_out) a.y2_out[b] = (mixed && a.labels) ? a.labels[j] : lab;
                if (a.w_out) a.w_out[b] = w;
            }
            if (mixed) {
                const int* bx = a.box + 4 * s;
                by0 = bx[0], by1 = bx[1], bx0 = bx[2], bx1 = bx[3];
                cut = by0 < by1 && bx0 < bx1;
                mixed = !cut || (x0 < bx1 && x0 + VEC > bx0);       // CutMix columns outside the box keep a
                if (mixed) par.init(a, l, j, true, (int)c, x0);
            }
        }
        const int oy0 = (int)og * RES_ROWS, oy_end = min(oy0 + RES_ROWS, a.OH);
        float* const o0 = a.out + ((b * C + c) * a.OH + oy0) * a.OW + x0;
        auto rows = [&](auto through_windows) {
            constexpr bool WIN = decltype(through_windows)::value;
            float* o = o0;
#pragma unroll 1
            for (int oy = oy0; oy < oy_end; ++oy, o += a.OW) {
                float v[VEC];
                own.template row<WIN>(a, l, oy, v);
                if constexpr (MIX) {
                    if (mixed && (!cut || (oy >= by0 && oy < by1))) {        // CutMix rows outside the box keep a
                        float p[VEC];
                        par.template row<WIN>(a, l, oy, p);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            if (cut)
                                v[e] = (x0 + e >= bx0 && x0 + e < bx1) ? p[e] : v[e];
                            else
                                v[e] = mix_blend(w, w1, v[e], p[e]);
                        }
                    }
                }
                if constexpr (VEC == 4) {
                    *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
                } else {
                    o[0] = v[0];
                }
            }
        };
        if (VEC == 4 && own.win && (!mixed || par.win))
            rows(std::integral_constant<bool, VEC == 4>{});
        else
            rows(std::false_type{});
        xg += s_xg;                                      // every digit and its stride digit are below the radix: one carry each
        unsigned k = xg >= WV ? 1u : 0u;
        xg -= k ? WV : 0u;
        og += s_og + k;
        k = og >= OG ? 1u : 0u;
        og -= k ? OG : 0u;
        c += s_c + k;
        k = c >= C ? 1u : 0u;
        c -= k ? C : 0u;
        b += s_b + k;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Soft-target cross-entropy, forward and gradient in one walk (ops.soft_cross_entropy): the target of row b is
//     t_c = (1 - eps) (w [c == y1] + (1 - w) [c == y2]) + eps / C        (label smoothing eps; Mixup / CutMix pair (y1, y2, w))
// and with m = max z, s = sum exp(z - m), p = exp(z - m) / s:
//     loss_b = log s + sum_c t_c (m - z_c)        (= lse(z) - t.z because sum t = 1; every term is >= 0: nothing cancels)
//     dz_bc  = (p_c - t_c) * (1 / B)
// One wave per row with the lane on the class index, as metrics_update_kernel walks it: max, then sum exp and sum (m - z) together,
// then the gradient.  A row's bits depend on the row alone (fixed lane assignment, fixed xor-shuffle tree); 1 / B is rounded once on
// the host.  The mean is soft_ce_mean_kernel: one work-group, thread t adds rows t, t + 256, ... in order, then a fixed LDS tree.
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

__global__ __launch_bounds__(256) void soft_ce_mean_kernel(const SoftCeArgs a) {
    __shared__ float part[256];
    float s = 0.f;
    for (long long r = threadIdx.x; r < a.B; r += 256) s += a.loss_rows[r];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.loss[0] = part[0] / (float)a.B;
}

int aug_check_shape(const char* who, int64_t N, int H, int W, int C, int pad_y, int pad_x) {
    if (N < 1) return kv_fail(KANVIT_EINVAL, "%s: N=%lld: the dataset holds at least one image", who, (long long)N);
    if (C < 1 || C > 4) return kv_fail(KANVIT_EINVAL, "%s: C=%d must be in 1..4 (the look-up table is staged as C x 1 KB)", who, C);
    if (H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return kv_fail(KANVIT_EINVAL, "%s: H=%d, W=%d must be in 1..2^20", who, H, W);
    if (pad_y < 0 || pad_y > H) return kv_fail(KANVIT_EINVAL, "%s: pad_y=%d must be in 0..H=%d", who, pad_y, H);
    if (pad_x < 0 || pad_x > W) return kv_fail(KANVIT_EINVAL, "%s: pad_x=%d must be in 0..W=%d", who, pad_x, W);
    return 0;
}

int res_check_shape(const char* who, int64_t N, int H, int W, int C, int OH, int OW) {
    if (N < 1) return kv_fail(KANVIT_EINVAL, "%s: N=%lld: the dataset holds at least one image", who, (long long)N);
    if (C < 1 || C > 4) return kv_fail(KANVIT_EINVAL, "%s: C=%d must be in 1..4 (the look-up table is staged as C x 1 KB)", who, C);
    if (H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return kv_fail(KANVIT_EINVAL, "%s: H=%d, W=%d must be in 1..2^20", who, H, W);
    if (OH < 1 || OW < 1 || OH > (1 << 20) || OW > (1 << 20)) return kv_fail(KANVIT_EINVAL, "%s: OH=%d, OW=%d must be in 1..2^20", who, OH, OW);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
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

// ---------------------------------------------------------------------------------------------------------------------------
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

int kanvit_augment_u8_supported(int64_t N, int H, int W, int C, int pad_y, int pad_x) {
    return aug_check_shape("kanvit_augment_u8_supported", N, H, W, C, pad_y, pad_x) == 0 ? 1 : 0;
}

int kanvit_augment_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, float* out, int64_t* y_out,
                      int32_t* params_out, int64_t N, int64_t B, int H, int W, int C, int pad_y, int pad_x, int flip, uint64_t seed,
                      uint64_t epoch, void* stream) {
    if (int rc = aug_check_shape("kanvit_augment_u8", N, H, W, C, pad_y, pad_x)) return rc;
    if (B < 0) return kv_fail(KANVIT_EINVAL, "kanvit_augment_u8: B=%lld is negative", (long long)B);
    if (flip != 0 && flip != 1) return kv_fail(KANVIT_EINVAL, "kanvit_augment_u8: flip=%d is 0 (never) or 1 (with probability 1/2)", flip);
    if (B == 0) return 0;
    if (!images || !idx || !lut || !out) return kv_fail(KANVIT_EINVAL, "kanvit_augment_u8: null images/idx/lut/out");
    if (y_out && !labels) return kv_fail(KANVIT_EINVAL, "kanvit_augment_u8: y_out without labels");
    if ((uintptr_t)out & 3 || (uintptr_t)lut & 3 || (uintptr_t)idx & 7 || (uintptr_t)labels & 7 || (uintptr_t)y_out & 7 || (uintptr_t)params_out & 3)
        return kv_fail(KANVIT_EINVAL, "kanvit_augment_u8: a pointer is not aligned to its element size");
    AugArgs a;
    a.images = images;
    a.labels = (const long long*)labels;
    a.idx = (const long long*)idx;
    a.lut = lut;
    a.out = out;
    a.y_out = (long long*)y_out;
    a.params_out = params_out;
    a.N = N, a.B = B, a.H = H, a.W = W, a.C = C, a.pad_y = pad_y, a.pad_x = pad_x, a.flip = flip;
    a.seed_epoch = aug_mix(aug_mix(seed) + epoch);
    // the form is decided here: 16-byte stores need whole groups of four x and an aligned base (every row then starts aligned too)
    const bool vec = (W % 4 == 0) && ((uintptr_t)out & 15) == 0;
    const long long total = (long long)B * H * C * (vec ? W / 4 : W);
    long long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;           // grid-stride beyond: 8 work-groups per CU's worth of table fills at the most
    if (vec)
        hipLaunchKernelGGL(augment_u8_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(augment_u8_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("augment_u8_kernel");
    return 0;
}

int kanvit_mix_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, const int64_t* partner,
                  const float* weight, const int32_t* box, float* out, int64_t* y_out, int64_t* y2_out, float* w_out, int64_t N, int64_t B,
                  int H, int W, int C, int pad_y, int pad_x, int flip, uint64_t seed, uint64_t epoch, void* stream) {
    if (int rc = aug_check_shape("kanvit_mix_u8", N, H, W, C, pad_y, pad_x)) return rc;
    if (B < 0) return kv_fail(KANVIT_EINVAL, "kanvit_mix_u8: B=%lld is negative", (long long)B);
    if (flip != 0 && flip != 1) return kv_fail(KANVIT_EINVAL, "kanvit_mix_u8: flip=%d is 0 (never) or 1 (with probability 1/2)", flip);
    if (B == 0) return 0;
    if (!images || !idx || !lut || !out) return kv_fail(KANVIT_EINVAL, "kanvit_mix_u8: null images/idx/lut/out");
    if (!partner || !weight || !box) return kv_fail(KANVIT_EINVAL, "kanvit_mix_u8: null partner/weight/box (the three tables come together)");
    if ((y_out || y2_out) && !labels) return kv_fail(KANVIT_EINVAL, "kanvit_mix_u8: y_out / y2_out without labels");
    if ((uintptr_t)out & 3 || (uintptr_t)lut & 3 || (uintptr_t)idx & 7 || (uintptr_t)labels & 7 || (uintptr_t)y_out & 7 || (uintptr_t)y2_out & 7 ||
        (uintptr_t)partner & 7 || (uintptr_t)weight & 3 || (uintptr_t)box & 3 || (uintptr_t)w_out & 3)
        return kv_fail(KANVIT_EINVAL, "kanvit_mix_u8: a pointer is not aligned to its element size");
    MixArgs m;
    AugArgs& a = m.g;
    a.images = images;
    a.labels = (const long long*)labels;
    a.idx = (const long long*)idx;
    a.lut = lut;
    a.out = out;
    a.y_out = (long long*)y_out;
    a.params_out = nullptr;
    a.N = N, a.B = B, a.H = H, a.W = W, a.C = C, a.pad_y = pad_y, a.pad_x = pad_x, a.flip = flip;
    a.seed_epoch = aug_mix(aug_mix(seed) + epoch);
    m.partner = (const long long*)partner;
    m.weight = weight;
    m.box = box;
    m.y2_out = (long long*)y2_out;
    m.w_out = w_out;
    const bool vec = (W % 4 == 0) && ((uintptr_t)out & 15) == 0;        // as kanvit_augment_u8 decides it
    const long long total = (long long)B * H * C * (vec ? W / 4 : W);
    long long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (vec)
        hipLaunchKernelGGL(mix_u8_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m);
    else
        hipLaunchKernelGGL(mix_u8_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, m);
    KV_LAUNCH_CHECK("mix_u8_kernel");
    return 0;
}

int kanvit_resample_u8_supported(int64_t N, int H, int W, int C, int OH, int OW) {
    return res_check_shape("kanvit_resample_u8_supported", N, H, W, C, OH, OW) == 0 ? 1 : 0;
}

int kanvit_resample_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, const int32_t* crop,
                       const int64_t* partner, const float* weight, const int32_t* box, float* out, int64_t* y_out, int64_t* y2_out,
                       float* w_out, int64_t N, int64_t B, int H, int W, int C, int OH, int OW, void* stream) {
    if (int rc = res_check_shape("kanvit_resample_u8", N, H, W, C, OH, OW)) return rc;
    if (B < 0) return kv_fail(KANVIT_EINVAL, "kanvit_resample_u8: B=%lld is negative", (long long)B);
    if (B == 0) return 0;
    if (B > (1ll << 62) / ((long long)C * OH * OW)) return kv_fail(KANVIT_EINVAL, "kanvit_resample_u8: B=%lld: too many output pixels for one launch", (long long)B);
    if (!images || !idx || !lut || !out) return kv_fail(KANVIT_EINVAL, "kanvit_resample_u8: null images/idx/lut/out");
    const bool mix = partner || weight || box;
    if (mix && (!partner || !weight || !box))
        return kv_fail(KANVIT_EINVAL, "kanvit_resample_u8: null %s (the three mix tables partner/weight/box come together or not at all)",
                       !partner ? "partner" : !weight ? "weight" : "box");
    if ((y2_out || w_out) && !mix) return kv_fail(KANVIT_EINVAL, "kanvit_resample_u8: y2_out / w_out without the mix tables");
    if ((y_out || y2_out) && !labels) return kv_fail(KANVIT_EINVAL, "kanvit_resample_u8: y_out / y2_out without labels");
    if ((uintptr_t)out & 3 || (uintptr_t)lut & 3 || (uintptr_t)idx & 7 || (uintptr_t)labels & 7 || (uintptr_t)crop & 3 || (uintptr_t)y_out & 7 ||
        (uintptr_t)y2_out & 7 || (uintptr_t)partner & 7 || (uintptr_t)weight & 3 || (uintptr_t)box & 3 || (uintptr_t)w_out & 3)
        return kv_fail(KANVIT_EINVAL, "kanvit_resample_u8: a pointer is not aligned to its element size");
    ResArgs a;
    a.images = images;
    a.labels = (const long long*)labels;
    a.idx = (const long long*)idx;
    a.lut = lut;
    a.crop = crop;
    a.partner = (const long long*)partner;
    a.weight = weight;
    a.box = box;
    a.out = out;
    a.y_out = (long long*)y_out;
    a.y2_out = (long long*)y2_out;
    a.w_out = w_out;
    a.N = N, a.B = B, a.H = H, a.W = W, a.C = C, a.OH = OH, a.OW = OW;
    const bool vec = (OW % 4 == 0) && ((uintptr_t)out & 15) == 0;       // as kanvit_augment_u8 decides it, on the output's width
    a.total = (long long)B * C * ((OH + RES_ROWS - 1) / RES_ROWS) * (vec ? OW / 4 : OW);       // items of RES_ROWS rows by 4 (or 1) columns
    long long blocks = (a.total + 255) / 256;
    if (blocks > 2048) blocks = 2048;           // the kernel's 32-bit index arithmetic relies on this cap: t0 and the stride stay below 2^19
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (vec && mix)
        hipLaunchKernelGGL((resample_u8_kernel<4, true>), grid, block, 0, st, a);
    else if (vec)
        hipLaunchKernelGGL((resample_u8_kernel<4, false>), grid, block, 0, st, a);
    else if (mix)
        hipLaunchKernelGGL((resample_u8_kernel<1, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((resample_u8_kernel<1, false>), grid, block, 0, st, a);
    KV_LAUNCH_CHECK("resample_u8_kernel");
    return 0;
}

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
