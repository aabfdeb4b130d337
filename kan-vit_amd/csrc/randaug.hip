// RandAugment as one uint8 -> uint8 pass over the GPU-resident dataset, once per epoch (kanvit/data.py: randaug_table,
// GpuDataset(randaug=...); semantics: include/kanvit.h, kanvit_randaug_u8).  Compiled as part of the data
// path's translation unit: batch_u8.hip includes this file at its end (kanvit/build.py).
//
// One work-group of 256 threads per image, striding over the images beyond RANDAUG_MAX_GROUPS.  The image lives in LDS: two
// ping-pong buffers of H W C bytes (rounded up to 16) and, behind them, a C x 256 int32 area that is a histogram first and a look-up
// table afterwards, and 64 bytes of reduction scratch.  All of it is dynamic LDS sized to the image, so that a 3 KB CIFAR image
// leaves the CU as many work-groups as the registers allow.  Op k reads buffer `cur` and writes buffer `nxt`; the last op writes global memory, 16 or 4
// bytes per store where the image size and both base pointers allow it.  An identity row in front of the last costs nothing.
//
// Every op is integer arithmetic and every reduction is an integer sum, a ballot or an LDS integer atomic: the bytes do not depend
// on the order in which threads arrive.  The ops that map a byte to a byte (INVERT .. BRIGHTNESS, and AUTOCONTRAST, EQUALIZE,
// CONTRAST once their statistics are known) all go through the table: thread t computes entry t, and one loop applies it.
// COLOR, SHARPNESS and AFFINE read more than their own byte and compute in place.
#include "kanvit_common.h"

namespace {

constexpr int RA_THREADS = 256;
// Work-groups of a launch; the kernel strides over the images beyond (8 work-groups of 256 threads on each of 256 CUs).
constexpr long long RANDAUG_MAX_GROUPS = 2048;
constexpr int RA_Q16 = 65536;
constexpr int RA_SCRATCH_BYTES = 64;        // 4 ballot masks (32 bytes), then 4 wave totals

struct RaArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int32_t* table;
    long long N;
    int H, W, C, K;
    int S;          // H W C
    int buf;        // S rounded up to 16: the size of one LDS image buffer
};

__device__ __forceinline__ int ra_clamp(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// blend(d, v, f) of include/kanvit.h; d, v in 0..255 and f in 0..2^17, so every term fits 32 bits
__device__ __forceinline__ int ra_blend(int d, int v, int f) { return ra_clamp((d * RA_Q16 + f * (v - d) + 32768) >> 16); }

__device__ __forceinline__ int ra_grey(const uint8_t* px) { return (19595 * px[0] + 38470 * px[1] + 7471 * px[2] + 32768) >> 16; }

// i / C for C in 1..4 without a runtime division
__device__ __forceinline__ int ra_pixel_of(int i, int C) { return C == 1 ? i : C == 2 ? i >> 1 : C == 3 ? i / 3 : i >> 2; }

// an op whose parameters are outside their range, and an op this image cannot take, is the identity
__device__ __forceinline__ int ra_effective_op(int op, int p0, int p1, int C) {
    switch (op) {
        case KANVIT_RA_AUTOCONTRAST:
        case KANVIT_RA_EQUALIZE:
        case KANVIT_RA_INVERT:
        case KANVIT_RA_AFFINE: return op;
        case KANVIT_RA_POSTERIZE: return (p0 >= 0 && p0 <= 8) ? op : KANVIT_RA_IDENTITY;
        case KANVIT_RA_SOLARIZE: return (p0 >= 0 && p0 <= 256) ? op : KANVIT_RA_IDENTITY;
        case KANVIT_RA_SOLARIZE_ADD: return (p0 >= 0 && p0 <= 255 && p1 >= 0 && p1 <= 256) ? op : KANVIT_RA_IDENTITY;
        case KANVIT_RA_COLOR: return (p0 >= 0 && p0 <= 2 * RA_Q16 && C >= 3) ? op : KANVIT_RA_IDENTITY;
        case KANVIT_RA_BRIGHTNESS:
        case KANVIT_RA_CONTRAST:
        case KANVIT_RA_SHARPNESS: return (p0 >= 0 && p0 <= 2 * RA_Q16) ? op : KANVIT_RA_IDENTITY;
        default: return KANVIT_RA_IDENTITY;
    }
}

// the byte-to-byte ops with no statistics: entry v of their table
__device__ __forceinline__ int ra_point(int op, int p0, int p1, int v) {
    switch (op) {
        case KANVIT_RA_INVERT: return 255 - v;
        case KANVIT_RA_POSTERIZE: return v & ~(0xFF >> p0);
        case KANVIT_RA_SOLARIZE: return v < p0 ? v : 255 - v;
        case KANVIT_RA_SOLARIZE_ADD: return v < p1 ? (v + p0 > 255 ? 255 : v + p0) : v;
        default: return ra_blend(0, v, p0);       // BRIGHTNESS
    }
}

// the sum of v over the work-group, in every thread; `totals` is 4 ints of LDS
__device__ __forceinline__ int ra_block_sum(int v, int* totals) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) totals[threadIdx.x >> 6] = v;
    __syncthreads();
    const int sum = totals[0] + totals[1] + totals[2] + totals[3];
    __syncthreads();                        // totals may be written again
    return sum;
}

// the sum of v over the threads in front of this one; `totals` is 4 ints of LDS
__device__ __forceinline__ int ra_block_scan_exclusive(int v, int* totals) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) totals[wave] = inc;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < 3; ++w)
        if (w < wave) before += totals[w];
    __syncthreads();
    return before + inc - v;
}

// out[i] = f(i, y, x, c, in[i]) for the S bytes of one image, (y, x, c) the row, column and channel of byte i: VEC bytes per LDS load
// and per store, one division per VEC bytes.  S is a multiple of VEC; in (LDS) and out (LDS or global memory) are aligned to it.
template <int VEC, typename F>
__device__ __forceinline__ void ra_emit(uint8_t* out, const uint8_t* in, int S, int C, int W, F f) {
    for (int i0 = threadIdx.x * VEC; i0 < S; i0 += RA_THREADS * VEC) {
        const int p = ra_pixel_of(i0, C);
        int c = i0 - p * C, y = p / W, x = p - y * W;
        if constexpr (VEC == 1) {
            out[i0] = (uint8_t)f(i0, y, x, c, (int)in[i0]);
        } else {
            uint32_t v[VEC / 4], w[VEC / 4];
            if constexpr (VEC == 16) {
                const uint4 q = *reinterpret_cast<const uint4*>(in + i0);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
                v[0] = *reinterpret_cast<const uint32_t*>(in + i0);
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const uint32_t b = (uint32_t)f(i0 + j, y, x, c, (int)((v[j >> 2] >> (8 * (j & 3))) & 255u)) & 255u;
                w[j >> 2] = (j & 3) ? (w[j >> 2] | (b << (8 * (j & 3)))) : b;
                if (++c == C) {
                    c = 0;
                    if (++x == W) x = 0, ++y;
                }
            }
            if constexpr (VEC == 16)
                *reinterpret_cast<uint4*>(out + i0) = make_uint4(w[0], w[1], w[2], w[3]);
            else
                *reinterpret_cast<uint32_t*>(out + i0) = w[0];
        }
    }
}

// The table of AUTOCONTRAST (equalize == false) or EQUALIZE for every channel, built in `lut` [C][256] from the histogram of `cur`.
__device__ __forceinline__ void ra_histogram_table(const uint8_t* cur, int* lut, int* scratch, int S, int C, int HW, bool equalize) {
    const int t = threadIdx.x;
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(scratch);
    int* totals = scratch + 8;
    for (int i = t; i < C * 256; i += RA_THREADS) lut[i] = 0;
    __syncthreads();
    for (int i = t; i < S; i += RA_THREADS) atomicAdd(&lut[(i - ra_pixel_of(i, C) * C) * 256 + cur[i]], 1);
    __syncthreads();
    for (int c = 0; c < C; ++c) {
        int* row = lut + c * 256;
        const int h = row[t];
        const unsigned long long m = __ballot(h > 0);
        if ((t & 63) == 0) masks[t >> 6] = m;
        __syncthreads();
        int lo = 256, hi = -1, bins = 0;            // the first and the last bin that is not empty, and how many are not
        for (int w = 3; w >= 0; --w)
            if (masks[w]) lo = 64 * w + __ffsll((long long)masks[w]) - 1;
        for (int w = 0; w < 4; ++w) {
            if (masks[w]) hi = 64 * w + 63 - __clzll((long long)masks[w]);
            bins += __popcll(masks[w]);
        }
        int entry = t;
        if (equalize) {
            const int last = row[hi];                                // read by everyone before the scan's barriers, written after
            const int before = ra_block_scan_exclusive(h, totals);   // the pixels below bin t
            const int step = (HW - last) / 255;
            if (bins > 1 && step > 0) entry = min(255, (step / 2 + before) / step);
        } else if (hi > lo && t >= lo && t <= hi) {
            entry = ((t - lo) * 255) / (hi - lo);
        }
        row[t] = entry;
        __syncthreads();                            // the masks are written again for the next channel
    }
}

template <int VEC>
__global__ __launch_bounds__(RA_THREADS) void randaug_u8_kernel(RaArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ra_lds[];
    int* lut = reinterpret_cast<int*>(ra_lds + 2 * a.buf);
    int* scratch = lut + a.C * 256;
    const int S = a.S, C = a.C, H = a.H, W = a.W, HW = a.H * a.W, t = threadIdx.x;
    for (long long s = blockIdx.x; s < a.N; s += gridDim.x) {
        const uint8_t* src = a.src + s * S;
        uint8_t* cur = ra_lds;
        uint8_t* nxt = ra_lds + a.buf;
        for (int i = t * VEC; i < S; i += RA_THREADS * VEC) {
            if constexpr (VEC == 16)
                *reinterpret_cast<uint4*>(cur + i) = *reinterpret_cast<const uint4*>(src + i);
            else if constexpr (VEC == 4)
                *reinterpret_cast<uint32_t*>(cur + i) = *reinterpret_cast<const uint32_t*>(src + i);
            else
                cur[i] = src[i];
        }
        __syncthreads();
        for (int k = 0; k < a.K; ++k) {
            const int32_t* row = a.table + (s * a.K + k) * 8;
            const int p0 = row[1], p1 = row[2];
            const int op = ra_effective_op(row[0], p0, p1, C);
            const bool last = k == a.K - 1;
            if (op == KANVIT_RA_IDENTITY && !last) continue;
            uint8_t* out = last ? a.dst + s * S : nxt;
            const uint8_t* in = cur;
            if (op == KANVIT_RA_IDENTITY) {
                ra_emit<VEC>(out, in, S, C, W, [=](int, int, int, int, int v) { return v; });
            } else if (op == KANVIT_RA_COLOR) {
                ra_emit<VEC>(out, in, S, C, W, [=](int i, int, int, int c, int v) { return c == 3 ? v : ra_blend(ra_grey(in + i - c), v, p0); });
            } else if (op == KANVIT_RA_SHARPNESS) {
                ra_emit<VEC>(out, in, S, C, W, [=](int i, int y, int x, int, int v) {
                    if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return v;
                    const int up = i - W * C, down = i + W * C;
                    const int sum = in[up - C] + in[up] + in[up + C] + in[i - C] + in[i + C] + in[down - C] + in[down] + in[down + C];
                    return ra_blend((sum + 5 * v + 6) / 13, v, p0);
                });
            } else if (op == KANVIT_RA_AFFINE) {
                const long long a00 = p0, a01 = p1, a02 = 2ll * row[3], a10 = row[4], a11 = row[5], a12 = 2ll * row[6];
                const int fill = row[7];
                ra_emit<VEC>(out, in, S, C, W, [=](int, int y, int x, int c, int) {
                    const long long xs = (a00 * (2 * x + 1) + a01 * (2 * y + 1) + a02) >> 17;
                    const long long ys = (a10 * (2 * x + 1) + a11 * (2 * y + 1) + a12) >> 17;
                    if (xs < 0 || xs >= W || ys < 0 || ys >= H) return (fill >> (8 * c)) & 255;
                    return (int)in[((int)ys * W + (int)xs) * C + c];
                });
            } else {
                int stride = 0;                     // of the table between channels: 0 where one table serves them all
                if (op == KANVIT_RA_AUTOCONTRAST || op == KANVIT_RA_EQUALIZE) {
                    ra_histogram_table(in, lut, scratch, S, C, HW, op == KANVIT_RA_EQUALIZE);
                    stride = 256;
                } else if (op == KANVIT_RA_CONTRAST) {
                    int g = 0;
                    for (int p = t; p < HW; p += RA_THREADS) g += C >= 3 ? ra_grey(in + p * C) : (int)in[p * C];
                    const int mean = (ra_block_sum(g, scratch + 8) + HW / 2) / HW;
                    lut[t] = ra_blend(mean, t, p0);
                    __syncthreads();
                } else {
                    lut[t] = ra_point(op, p0, p1, t);
                    __syncthreads();
                }
                ra_emit<VEC>(out, in, S, C, W, [=](int, int, int, int c, int v) { return lut[c * stride + v]; });
            }
            if (!last) {
                __syncthreads();                    // nxt is complete, and the table may be overwritten
                uint8_t* swap = cur;
                cur = nxt;
                nxt = swap;
            }
        }
        __syncthreads();                            // every read of this image is done before the next one is loaded
    }
}

}  // namespace

extern "C" {

int kanvit_randaug_u8(const uint8_t* src, uint8_t* dst, const int32_t* table, long long N, int H, int W, int C, int K, void* stream) {
    const char* who = "kanvit_randaug_u8";
    if (N < 0) return kv_fail(KANVIT_EINVAL, "%s: N=%lld is negative", who, N);
    if (C < 1 || C > 4) return kv_fail(KANVIT_EINVAL, "%s: C=%d must be in 1..4", who, C);
    if (H < 1 || W < 1) return kv_fail(KANVIT_EINVAL, "%s: H=%d, W=%d must be positive", who, H, W);
    if (H > KANVIT_RA_MAX_BYTES || W > KANVIT_RA_MAX_BYTES || (long long)H * W * C > KANVIT_RA_MAX_BYTES)
        return kv_fail(KANVIT_EINVAL, "%s: an image of H=%d x W=%d x C=%d bytes exceeds %d (the image and its copy live in LDS)", who, H, W, C,
                       KANVIT_RA_MAX_BYTES);
    if (K < 1 || K > KANVIT_RA_MAX_OPS) return kv_fail(KANVIT_EINVAL, "%s: K=%d must be in 1..%d", who, K, KANVIT_RA_MAX_OPS);
    if (N == 0) return 0;
    if (!src || !dst || !table) return kv_fail(KANVIT_EINVAL, "%s: null src/dst/table", who);
    const int S = H * W * C;
    if (N > (1ll << 62) / S) return kv_fail(KANVIT_EINVAL, "%s: N=%lld: too many bytes for one launch", who, N);
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst, bytes = (uintptr_t)N * (uintptr_t)S;
    if (s0 == d0) return kv_fail(KANVIT_EINVAL, "%s: src == dst (an op reads more than the byte it writes; give a second buffer)", who);
    if (s0 < d0 + bytes && d0 < s0 + bytes) return kv_fail(KANVIT_EINVAL, "%s: src and dst overlap", who);
    if ((uintptr_t)table & 3) return kv_fail(KANVIT_EINVAL, "%s: table is not aligned to its element size", who);
    RaArgs a;
    a.src = src, a.dst = dst, a.table = table;
    a.N = N, a.H = H, a.W = W, a.C = C, a.K = K, a.S = S, a.buf = (S + 15) & ~15;
    const size_t lds = 2 * (size_t)a.buf + (size_t)C * 256 * sizeof(int) + RA_SCRATCH_BYTES;
    const dim3 grid((unsigned)(N > RANDAUG_MAX_GROUPS ? RANDAUG_MAX_GROUPS : N)), block(RA_THREADS);
    const uintptr_t both = s0 | d0 | (uintptr_t)S;              // every image of both arrays starts on a multiple of what divides all three
    if (both % 16 == 0)
        hipLaunchKernelGGL(randaug_u8_kernel<16>, grid, block, lds, (hipStream_t)stream, a);
    else if (both % 4 == 0)
        hipLaunchKernelGGL(randaug_u8_kernel<4>, grid, block, lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(randaug_u8_kernel<1>, grid, block, lds, (hipStream_t)stream, a);
    KV_LAUNCH_CHECK("randaug_u8_kernel");
    return 0;
}

}  // extern "C"
