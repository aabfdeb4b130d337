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
#include "../../include/kanvit.h"
#include "kanvit_common.h"

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

int aug_check_shape(const char* who, int64_t N, int H, int W, int C, int pad_y, int pad_x) {
    if (N < 1) return kv_fail(KANVIT_EINVAL, "%s: N=%lld: the dataset holds at least one image", who, (long long)N);
    if (C < 1 || C > 4) return kv_fail(KANVIT_EINVAL, "%s: C=%d must be in 1..4 (the look-up table is staged as C x 1 KB)", who, C);
    if (H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return kv_fail(KANVIT_EINVAL, "%s: H=%d, W=%d must be in 1..2^20", who, H, W);
    if (pad_y < 0 || pad_y > H) return kv_fail(KANVIT_EINVAL, "%s: pad_y=%d must be in 0..H=%d", who, pad_y, H);
    if (pad_x < 0 || pad_x > W) return kv_fail(KANVIT_EINVAL, "%s: pad_x=%d must be in 0..W=%d", who, pad_x, W);
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

}  // extern "C"
