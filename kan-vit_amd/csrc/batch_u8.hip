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
// mix_u8_kernel (Mixup / CutMix) and resample_u8_kernel (bilinear resize, RandomResizedCrop, Random Erasing) are forms of the same pass,
// further down; the four entry points share one host path (batch_check_shape, batch_check_operands, batch_vec_form, batch_grid), below the kernels.
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
// stride's digits with carries: t0 and the stride are below 2^19 (BATCH_MAX_GROUPS work-groups at the most), so the only divisions
// are 32-bit ones, once per thread.
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

// ---------------------------------------------------------------------------------------------------------------------------
// Random Erasing on the same pass (kanvit/data.py: erase_table).  The epoch's erase table names, per DATASET index s, a box
// (y0, y1, x0, x1), half open, in OUTPUT coordinates; inside it the resampled value of s is replaced by a fill BEFORE mixing, and the
// partner is erased under ITS OWN row before it is pasted or blended in.  The fill is 0 (the dataset mean, normalised) or, with a noise
// table of T = 2^k entries, noise[h >> (64 - k)], h = mix(mix(noise_key + s) + ((c OH + y) OW + x)): a look-up, no floating-point
// arithmetic, a function of (noise_key, s, c, y, x) alone.  The box test is a comparison on output coordinates -- no sums of table
// entries -- so any int32 row is safe, and an inverted or empty one erases nothing.
// Erasing is a compile-time parameter of the one body (resample_u8_body); the erasing forms take their arguments as EraseArgs, the
// others keep ResArgs, their kernel name and with them the registers they had before erasing existed.
// The noise table is read through the caches, not staged in LDS: at the recipe's defaults 4 % of the pixels are erased, so most
// work-groups never touch it, while staging would cost EVERY work-group a fill four times the look-up table's (16 KB at T = 4096)
// and could not hold the 256 KB the ABI allows; the table is shared by all work-groups and stays in L2.
struct EraseArgs : ResArgs {
    const int* erase;           // [N][4]
    const float* noise;         // [2^(64 - noise_shift)] or null: the fill is 0
    unsigned long long noise_key;
    int noise_shift;
};

// One sample's erase row against the columns x0 .. x0 + VEC - 1 of a work item.
template <int VEC>
struct ResErase {
    int y0, y1;
    unsigned cols;              // bit e: column x0 + e lies inside the box
    unsigned long long base;    // mix(noise_key + s)

    __device__ __forceinline__ void init(const EraseArgs& a, long long s, bool valid, int ox0) {
        y0 = y1 = 0, cols = 0, base = 0;
        if (!valid) return;     // no sample: no row is read
        const int* q = a.erase + 4 * s;
        y0 = q[0], y1 = q[1];
        const int ex0 = q[2], ex1 = q[3];
#pragma unroll
        for (int e = 0; e < VEC; ++e) cols |= (ox0 + e >= ex0 && ox0 + e < ex1) ? 1u << e : 0u;
        base = aug_mix(a.noise_key + (unsigned long long)s);
    }
    __device__ __forceinline__ bool hits(int oy) const { return cols != 0 && oy >= y0 && oy < y1; }     // some column of row oy is erased
    __device__ __forceinline__ bool whole() const { return cols == (1u << VEC) - 1; }                    // ... then: all of them are
    __device__ __forceinline__ void fill(const EraseArgs& a, int c, int oy, int ox0, float* v) const {
        const unsigned long long at = ((unsigned long long)c * a.OH + oy) * a.OW + ox0;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if (cols >> e & 1u) v[e] = a.noise ? a.noise[aug_mix(base + (at + e)) >> a.noise_shift] : 0.f;
    }
};

template <int VEC, bool MIX, bool ERASE>
__device__ __forceinline__ void resample_u8_body(const std::conditional_t<ERASE, EraseArgs, ResArgs> a) {
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
        [[maybe_unused]] ResErase<VEC> own_er, par_er;    // ... and their erase rows
        if constexpr (ERASE) own_er.init(a, s, sample_ok, x0);
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
                if (mixed) {
                    par.init(a, l, j, true, (int)c, x0);
                    if constexpr (ERASE) par_er.init(a, j, true, x0);
                }
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
                if constexpr (ERASE) {                   // a row of the item that lies wholly inside the box is not fetched
                    const bool hit = own_er.hits(oy);
                    if (!(hit && own_er.whole())) own.template row<WIN>(a, l, oy, v);
                    if (hit) own_er.fill(a, (int)c, oy, x0, v);
                } else {
                    own.template row<WIN>(a, l, oy, v);
                }
                if constexpr (MIX) {
                    if (mixed && (!cut || (oy >= by0 && oy < by1))) {        // CutMix rows outside the box keep a
                        float p[VEC];
                        if constexpr (ERASE) {
                            const bool hit = par_er.hits(oy);
                            if (!(hit && par_er.whole())) par.template row<WIN>(a, l, oy, p);
                            if (hit) par_er.fill(a, (int)c, oy, x0, p);
                        } else {
                            par.template row<WIN>(a, l, oy, p);
                        }
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

// The one body under two kernel names: resample_u8_kernel<VEC, MIX> is the ERASE = false form and keeps the name, the argument type
// and the registers it had before erasing existed; erase_u8_kernel<VEC, MIX> is the ERASE = true form.  The body takes the arguments
// by value: by reference the <4, true> form needs one more VGPR and spills SGPRs.
template <int VEC, bool MIX>
__global__ __launch_bounds__(256) void resample_u8_kernel(const ResArgs a) {
    resample_u8_body<VEC, MIX, false>(a);
}

template <int VEC, bool MIX>
__global__ __launch_bounds__(256) void erase_u8_kernel(const EraseArgs a) {
    resample_u8_body<VEC, MIX, true>(a);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The host path the entry points share: shape and operand checks, the AugArgs fill, the store form and the grid.
int batch_check_shape(const char* who, int64_t N, int H, int W, int C) {
    if (N < 1) return kv_fail(KANVIT_EINVAL, "%s: N=%lld: the dataset holds at least one image", who, (long long)N);
    if (C < 1 || C > 4) return kv_fail(KANVIT_EINVAL, "%s: C=%d must be in 1..4 (the look-up table is staged as C x 1 KB)", who, C);
    if (H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return kv_fail(KANVIT_EINVAL, "%s: H=%d, W=%d must be in 1..2^20", who, H, W);
    return 0;
}

int aug_check_shape(const char* who, int64_t N, int H, int W, int C, int pad_y, int pad_x) {
    if (int rc = batch_check_shape(who, N, H, W, C)) return rc;
    if (pad_y < 0 || pad_y > H) return kv_fail(KANVIT_EINVAL, "%s: pad_y=%d must be in 0..H=%d", who, pad_y, H);
    if (pad_x < 0 || pad_x > W) return kv_fail(KANVIT_EINVAL, "%s: pad_x=%d must be in 0..W=%d", who, pad_x, W);
    return 0;
}

int res_check_shape(const char* who, int64_t N, int H, int W, int C, int OH, int OW) {
    if (int rc = batch_check_shape(who, N, H, W, C)) return rc;
    if (OH < 1 || OW < 1 || OH > (1 << 20) || OW > (1 << 20)) return kv_fail(KANVIT_EINVAL, "%s: OH=%d, OW=%d must be in 1..2^20", who, OH, OW);
    return 0;
}

// noise_len: 0 (no table: the fill is 0) or the table's length, a power of two so that the top bits of a hash index it
int erase_check_shape(const char* who, int64_t N, int H, int W, int C, int OH, int OW, int noise_len) {
    if (int rc = res_check_shape(who, N, H, W, C, OH, OW)) return rc;
    if (noise_len != 0 && (noise_len < 2 || noise_len > 65536 || (noise_len & (noise_len - 1))))
        return kv_fail(KANVIT_EINVAL, "%s: noise_len=%d must be a power of two in 2..65536 (or 0 with a null noise: the fill is 0)", who, noise_len);
    return 0;
}

// What the launches check of their batch size and pointers.  Pointers an entry point does not have are passed null (flip: 0);
// y_names is how it names its label outputs.  Returns KANVIT_EINVAL, 0 for the empty batch (B == 0: nothing to launch, whatever the
// pointers) or BATCH_GO.
constexpr int BATCH_GO = 1;

int batch_check_operands(const char* who, const char* y_names, int64_t B, int flip, const uint8_t* images, const int64_t* labels, const int64_t* idx,
                         const float* lut, const int32_t* crop, const int64_t* partner, const float* weight, const int32_t* box, const float* out,
                         const int64_t* y_out, const int64_t* y2_out, const float* w_out, const int32_t* params_out) {
    if (B < 0) return kv_fail(KANVIT_EINVAL, "%s: B=%lld is negative", who, (long long)B);
    if (flip != 0 && flip != 1) return kv_fail(KANVIT_EINVAL, "%s: flip=%d is 0 (never) or 1 (with probability 1/2)", who, flip);
    if (B == 0) return 0;
    if (!images || !idx || !lut || !out) return kv_fail(KANVIT_EINVAL, "%s: null images/idx/lut/out", who);
    if ((y_out || y2_out) && !labels) return kv_fail(KANVIT_EINVAL, "%s: %s without labels", who, y_names);
    if ((uintptr_t)out & 3 || (uintptr_t)lut & 3 || (uintptr_t)idx & 7 || (uintptr_t)labels & 7 || (uintptr_t)crop & 3 || (uintptr_t)y_out & 7 ||
        (uintptr_t)y2_out & 7 || (uintptr_t)partner & 7 || (uintptr_t)weight & 3 || (uintptr_t)box & 3 || (uintptr_t)w_out & 3 ||
        (uintptr_t)params_out & 3)
        return kv_fail(KANVIT_EINVAL, "%s: a pointer is not aligned to its element size", who);
    return BATCH_GO;
}

// the fields of AugArgs, which kanvit_augment_u8 and kanvit_mix_u8 (inside MixArgs) share
void batch_fill(AugArgs& a, const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, float* out, int64_t* y_out,
                int32_t* params_out, int64_t N, int64_t B, int H, int W, int C, int pad_y, int pad_x, int flip, uint64_t seed, uint64_t epoch) {
    a.images = images;
    a.labels = (const long long*)labels;
    a.idx = (const long long*)idx;
    a.lut = lut;
    a.out = out;
    a.y_out = (long long*)y_out;
    a.params_out = params_out;
    a.N = N, a.B = B, a.H = H, a.W = W, a.C = C, a.pad_y = pad_y, a.pad_x = pad_x, a.flip = flip;
    a.seed_epoch = aug_mix(aug_mix(seed) + epoch);
}

// the form of a launch: 16-byte stores need whole groups of four x and an aligned base (every output row then starts aligned too)
bool batch_vec_form(int width, const float* out) { return (width % 4 == 0) && ((uintptr_t)out & 15) == 0; }

// Work-groups of a launch over `total` work items; the kernels stride over the grid beyond (8 work-groups per CU's worth of table
// fills at the most).  resample_u8_kernel's 32-bit digit arithmetic relies on this cap: t0 and the stride stay below 2^19.
constexpr long long BATCH_MAX_GROUPS = 2048;

dim3 batch_grid(long long total) {
    const long long blocks = (total + 255) / 256;
    return dim3((unsigned)(blocks > BATCH_MAX_GROUPS ? BATCH_MAX_GROUPS : blocks));
}

template <int VEC, bool MIX, bool ERASE>
void res_dispatch(const EraseArgs& a, hipStream_t st) {
    const dim3 grid = batch_grid(a.total), block(256);
    if constexpr (ERASE)
        hipLaunchKernelGGL((erase_u8_kernel<VEC, MIX>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((resample_u8_kernel<VEC, MIX>), grid, block, 0, st, static_cast<const ResArgs&>(a));       // the ResArgs part alone
}

template <bool ERASE>
void res_dispatch(const EraseArgs& a, bool vec, bool mix, hipStream_t st) {
    if (vec && mix)
        res_dispatch<4, true, ERASE>(a, st);
    else if (vec)
        res_dispatch<4, false, ERASE>(a, st);
    else if (mix)
        res_dispatch<1, true, ERASE>(a, st);
    else
        res_dispatch<1, false, ERASE>(a, st);
}

// kanvit_resample_u8 (erase, noise null; noise_len, noise_key 0) and kanvit_erase_u8: one set of checks, one launch.  Without an erase
// table both launch the same kernels with the same arguments.
int res_launch(const char* who, const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, const int32_t* crop,
               const int64_t* partner, const float* weight, const int32_t* box, float* out, int64_t* y_out, int64_t* y2_out, float* w_out, int64_t N,
               int64_t B, int H, int W, int C, int OH, int OW, const int32_t* erase, const float* noise, int noise_len, uint64_t noise_key,
               void* stream) {
    if (int rc = erase_check_shape(who, N, H, W, C, OH, OW, noise_len)) return rc;
    if (B > (1ll << 62) / ((long long)C * OH * OW)) return kv_fail(KANVIT_EINVAL, "%s: B=%lld: too many output pixels for one launch", who, (long long)B);
    const int rc = batch_check_operands(who, "y_out / y2_out", B, 0, images, labels, idx, lut, crop, partner, weight, box, out, y_out, y2_out, w_out,
                                        nullptr);
    if (rc != BATCH_GO) return rc;
    const bool mix = partner || weight || box;
    if (mix && (!partner || !weight || !box))
        return kv_fail(KANVIT_EINVAL, "%s: null %s (the three mix tables partner/weight/box come together or not at all)", who,
                       !partner ? "partner" : !weight ? "weight" : "box");
    if ((y2_out || w_out) && !mix) return kv_fail(KANVIT_EINVAL, "%s: y2_out / w_out without the mix tables", who);
    if (noise && !erase) return kv_fail(KANVIT_EINVAL, "%s: noise without erase (the noise fills the erase boxes)", who);
    if ((noise != nullptr) != (noise_len != 0))
        return kv_fail(KANVIT_EINVAL, "%s: noise_len=%d with %s noise (a table and its length come together; both absent: the fill is 0)", who,
                       noise_len, noise ? "a" : "a null");
    if ((uintptr_t)erase & 3 || (uintptr_t)noise & 3) return kv_fail(KANVIT_EINVAL, "%s: erase / noise is not aligned to its element size", who);
    EraseArgs a;
    a.erase = erase;
    a.noise = noise;
    a.noise_key = noise_key;
    a.noise_shift = 64;
    for (int t = noise_len; t > 1; t >>= 1) --a.noise_shift;       // 64 - log2(noise_len); not used without a table
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
    const bool vec = batch_vec_form(OW, out);
    a.total = (long long)B * C * ((OH + RES_ROWS - 1) / RES_ROWS) * (vec ? OW / 4 : OW);       // items of RES_ROWS rows by 4 (or 1) columns
    if (erase)
        res_dispatch<true>(a, vec, mix, (hipStream_t)stream);
    else
        res_dispatch<false>(a, vec, mix, (hipStream_t)stream);
    KV_LAUNCH_CHECK(erase ? "erase_u8_kernel" : "resample_u8_kernel");
    return 0;
}

}  // namespace

extern "C" {

int kanvit_augment_u8_supported(int64_t N, int H, int W, int C, int pad_y, int pad_x) {
    return aug_check_shape("kanvit_augment_u8_supported", N, H, W, C, pad_y, pad_x) == 0 ? 1 : 0;
}

int kanvit_augment_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, float* out, int64_t* y_out,
                      int32_t* params_out, int64_t N, int64_t B, int H, int W, int C, int pad_y, int pad_x, int flip, uint64_t seed,
                      uint64_t epoch, void* stream) {
    const char* who = "kanvit_augment_u8";
    if (int rc = aug_check_shape(who, N, H, W, C, pad_y, pad_x)) return rc;
    const int rc = batch_check_operands(who, "y_out", B, flip, images, labels, idx, lut, nullptr, nullptr, nullptr, nullptr, out, y_out, nullptr,
                                        nullptr, params_out);
    if (rc != BATCH_GO) return rc;
    AugArgs a;
    batch_fill(a, images, labels, idx, lut, out, y_out, params_out, N, B, H, W, C, pad_y, pad_x, flip, seed, epoch);
    const bool vec = batch_vec_form(W, out);
    const dim3 grid = batch_grid((long long)B * H * C * (vec ? W / 4 : W));
    if (vec)
        hipLaunchKernelGGL(augment_u8_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(augment_u8_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("augment_u8_kernel");
    return 0;
}

int kanvit_mix_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, const int64_t* partner,
                  const float* weight, const int32_t* box, float* out, int64_t* y_out, int64_t* y2_out, float* w_out, int64_t N, int64_t B,
                  int H, int W, int C, int pad_y, int pad_x, int flip, uint64_t seed, uint64_t epoch, void* stream) {
    const char* who = "kanvit_mix_u8";
    if (int rc = aug_check_shape(who, N, H, W, C, pad_y, pad_x)) return rc;
    const int rc = batch_check_operands(who, "y_out / y2_out", B, flip, images, labels, idx, lut, nullptr, partner, weight, box, out, y_out, y2_out,
                                        w_out, nullptr);
    if (rc != BATCH_GO) return rc;
    if (!partner || !weight || !box) return kv_fail(KANVIT_EINVAL, "kanvit_mix_u8: null partner/weight/box (the three tables come together)");
    MixArgs m;
    batch_fill(m.g, images, labels, idx, lut, out, y_out, nullptr, N, B, H, W, C, pad_y, pad_x, flip, seed, epoch);
    m.partner = (const long long*)partner;
    m.weight = weight;
    m.box = box;
    m.y2_out = (long long*)y2_out;
    m.w_out = w_out;
    const bool vec = batch_vec_form(W, out);
    const dim3 grid = batch_grid((long long)B * H * C * (vec ? W / 4 : W));
    if (vec)
        hipLaunchKernelGGL(mix_u8_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, m);
    else
        hipLaunchKernelGGL(mix_u8_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, m);
    KV_LAUNCH_CHECK("mix_u8_kernel");
    return 0;
}

int kanvit_resample_u8_supported(int64_t N, int H, int W, int C, int OH, int OW) {
    return res_check_shape("kanvit_resample_u8_supported", N, H, W, C, OH, OW) == 0 ? 1 : 0;
}

int kanvit_resample_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, const int32_t* crop,
                       const int64_t* partner, const float* weight, const int32_t* box, float* out, int64_t* y_out, int64_t* y2_out,
                       float* w_out, int64_t N, int64_t B, int H, int W, int C, int OH, int OW, void* stream) {
    return res_launch("kanvit_resample_u8", images, labels, idx, lut, crop, partner, weight, box, out, y_out, y2_out, w_out, N, B, H, W, C, OH, OW,
                      nullptr, nullptr, 0, 0, stream);
}

int kanvit_erase_u8_supported(int64_t N, int H, int W, int C, int OH, int OW, int noise_len) {
    return erase_check_shape("kanvit_erase_u8_supported", N, H, W, C, OH, OW, noise_len) == 0 ? 1 : 0;
}

int kanvit_erase_u8(const uint8_t* images, const int64_t* labels, const int64_t* idx, const float* lut, const int32_t* crop,
                    const int64_t* partner, const float* weight, const int32_t* box, float* out, int64_t* y_out, int64_t* y2_out, float* w_out,
                    int64_t N, int64_t B, int H, int W, int C, int OH, int OW, const int32_t* erase, const float* noise, int noise_len,
                    uint64_t noise_key, void* stream) {
    return res_launch("kanvit_erase_u8", images, labels, idx, lut, crop, partner, weight, box, out, y_out, y2_out, w_out, N, B, H, W, C, OH, OW, erase,
                      noise, noise_len, noise_key, stream);
}

}  // extern "C"

// The other kernel of the data path, in a file of its own but in this translation unit (kanvit/build.py: one unit per family): the
// per-epoch RandAugment pass that writes the uint8 copy of the dataset the kernels above then read.  It shares nothing but the unit.
#include "randaug.hip"
