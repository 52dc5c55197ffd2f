// Greyscale PNG scanlines of the test loop's slices, quantised on the device (reference engine.py:157-159 writes input,
// target and prediction of every slice with plt.imsave(..., cmap="gray")).  n float32 images (n, H, W) become the
// bytes zlib takes as they are: (n, H, 1 + W * depth / 8), byte 0 of every row the PNG filter type 0.
//   depth 8, "stretch": matplotlib's Normalize + gray colormap on the image's own finite limits, restated operation by operation
//     (gray_level8 below); the limits are a two-stage minimum / maximum (per-workgroup partials, one finish), no atomics.
//   depth 16, "fixed": round-half-even(clamp(x, 0, 1) * 65535), big-endian.
// HBM-bound and small (a batch of 3 x 16 slices of 512 x 512 reads 50 MB and writes 12.6 MB).  The row stride 1 + W * depth / 8
// is odd or unaligned in general, so the output is taken as ONE byte stream: a thread assembles one 4-byte word of it, aligned
// in memory whatever the buffer's own alignment, from the up to four (row, column) positions it covers -- filter bytes and row
// ends included -- and the at most three bytes before the first and after the last whole word are single byte stores.  Every
// byte of the buffer is written exactly once and nothing outside it is touched.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)      // every operation below rounds on its own

namespace {

constexpr unsigned GP_MAX_BLOCKS = 2048;      // grid cap of the elementwise passes (256 CUs x 8); the rest is strided
constexpr unsigned GP_MAX_PARTS = 64;         // partial limits per image (one wave finishes them)
constexpr unsigned GP_PART_PIXELS = 4096;     // pixels per partial before an image gets another one: 16 per thread

__host__ __device__ inline unsigned gp_parts(unsigned HW) {
    const unsigned p = (HW + GP_PART_PIXELS - 1) / GP_PART_PIXELS;
    return p < 1 ? 1 : (p > GP_MAX_PARTS ? GP_MAX_PARTS : p);
}

__device__ __forceinline__ bool gp_finite(float v) { return fabsf(v) < INFINITY; }      // false for NaN and +-Inf

// stage 1: unit u = (image u / P, part u % P) -> partial[u] = (min, max) of the finite pixels part, part + P, ... x 256 of the image
__global__ __launch_bounds__(256) void gray_limits_kernel(const float* __restrict__ x, unsigned HW, unsigned P, unsigned units,
                                                          float2* __restrict__ partial) {
    __shared__ float smn[4], smx[4];
    const unsigned tid = threadIdx.x;
    for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
        const unsigned i = u / P, p = u - i * P;
        const float* img = x + (long long)i * HW;
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll 4
        for (unsigned e = p * 256 + tid; e < HW; e += P * 256) {
            const float v = img[e];
            if (gp_finite(v)) { mn = fminf(mn, v); mx = fmaxf(mx, v); }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off, 64)); mx = fmaxf(mx, __shfl_xor(mx, off, 64)); }
        if ((tid & 63) == 0) { smn[tid >> 6] = mn; smx[tid >> 6] = mx; }
        __syncthreads();
        if (tid == 0)
            partial[u] = make_float2(fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3])), fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3])));
        __syncthreads();      // smn / smx are written again by the next unit
    }
}

// stage 2: one wave per image, P <= 64 partials -> limits[i].  (minimum and maximum do not depend on the order)
__global__ __launch_bounds__(64) void gray_limits_finish_kernel(const float2* __restrict__ partial, unsigned P, unsigned n,
                                                                float2* __restrict__ limits) {
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
        float mn = INFINITY, mx = -INFINITY;
        if (threadIdx.x < P) { const float2 v = partial[i * P + threadIdx.x]; mn = v.x; mx = v.y; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off, 64)); mx = fmaxf(mx, __shfl_xor(mx, off, 64)); }
        if (threadIdx.x == 0) limits[i] = make_float2(mn, mx);
    }
}

// matplotlib 3.10 / numpy 2, float32 image: Normalize.__call__ subtracts and divides IN PLACE by float64 scalars -- each result
// is formed in float64 and rounded to float32 once -- and the divisor vmax - vmin is never rounded to float32; Colormap.__call__
// multiplies by N = 256 in float32, moves 256 to 255, truncates, and sends what is below 0 / at or above 256 to the ends.
__device__ __forceinline__ unsigned gray_level8(float x, float vmin, float vmax, const unsigned char* lut) {
    if (!gp_finite(x)) return 0u;
    if (vmin == vmax) return lut[0];
    float r = (float)((double)x - (double)vmin);
    r = (float)((double)r / ((double)vmax - (double)vmin));      // correctly rounded float64 division, then one rounding
    float t = r * 256.f;
    if (t == 256.f) t = 255.f;
    const int k = t >= 256.f ? 255 : (t < 0.f ? 0 : (int)t);
    return lut[k];
}

__device__ __forceinline__ unsigned gray_level16(float x) {
    if (!gp_finite(x)) return 0u;
    return (unsigned)rintf(fminf(fmaxf(x, 0.f), 1.f) * 65535.f);      // rintf: to nearest, ties to even
}

// Byte (row q of the n * H rows, column c of the 1 + W * DEPTH / 8 of a row) of the output; keeps the row's image limits
// between calls, since the bytes a thread asks for are consecutive.
template <int DEPTH>
struct RowBytes {
    const float* x; const float2* limits; const unsigned char* lut;
    unsigned H, W;
    unsigned row = 0xffffffffu;
    float vmin = 0.f, vmax = 0.f;
    __device__ __forceinline__ unsigned at(unsigned q, unsigned c) {
        if (c == 0) return 0u;                                   // PNG filter type 0 (None)
        if (DEPTH == 8) {
            if (q != row) { const float2 l = limits[q / H]; vmin = l.x; vmax = l.y; row = q; }
            return gray_level8(x[(long long)q * W + (c - 1)], vmin, vmax, lut);
        }
        const unsigned v = gray_level16(x[(long long)q * W + ((c - 1) >> 1)]);
        return ((c - 1) & 1) ? (v & 255u) : (v >> 8);            // most significant byte first
    }
};

template <int DEPTH>
__global__ __launch_bounds__(256) void gray_rows_kernel(const float* __restrict__ x, unsigned H, unsigned W, unsigned total,
                                                        const unsigned char* __restrict__ lut, const float2* __restrict__ limits,
                                                        unsigned char* __restrict__ out, unsigned head, unsigned nwords) {
    __shared__ unsigned char lut_s[256];
    if (DEPTH == 8) {
        lut_s[threadIdx.x] = lut[threadIdx.x];
        __syncthreads();
    }
    const unsigned S = 1 + W * (DEPTH / 8);
    RowBytes<DEPTH> rb{x, limits, lut_s, H, W};
    // whole words: out + head is 4-byte aligned
    for (unsigned w = blockIdx.x * 256 + threadIdx.x; w < nwords; w += gridDim.x * 256) {
        const unsigned b = head + 4 * w;
        unsigned q = b / S, c = b - q * S;
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            word |= rb.at(q, c) << (8 * k);
            if (++c == S) { c = 0; ++q; }
        }
        *reinterpret_cast<unsigned*>(out + b) = word;
    }
    // the up to 3 bytes before the first word and the up to 3 after the last one
    if (blockIdx.x == 0 && threadIdx.x < 6) {
        const unsigned e = threadIdx.x;
        const unsigned b = e < head ? e : head + 4 * nwords + (e - head);
        if (b < total) {
            const unsigned q = b / S;
            out[b] = (unsigned char)rb.at(q, b - q * S);
        }
    }
}

bool gray_png_shape_ok(int n, int H, int W, int depth) {
    if (n <= 0 || H <= 0 || W <= 0 || (depth != 8 && depth != 16)) return false;
    const long long S = 1 + (long long)W * (depth / 8);
    return (long long)n * H * S < (1ll << 31);      // byte offsets are 32-bit in the kernels
}

}  // namespace

extern "C" size_t mtd_gray_png_rows_ws_bytes(int n, int H, int W, int depth) {
    if (!gray_png_shape_ok(n, H, W, depth) || depth != 8) return 0;
    return ((size_t)n * gp_parts((unsigned)H * (unsigned)W) + (size_t)n) * sizeof(float2);
}

extern "C" int mtd_gray_png_rows(const float* x, int n, int H, int W, int depth, const unsigned char* lut, unsigned char* out,
                                 void* ws, void* stream) {
    if (!x || !out || !gray_png_shape_ok(n, H, W, depth)) return MTD_EINVAL;
    if (depth == 8 && (!lut || !ws)) return MTD_EINVAL;
    if (((uintptr_t)x & 3) || (depth == 8 && ((uintptr_t)ws & 7))) return MTD_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const unsigned total = (unsigned)n * (unsigned)H * (1u + (unsigned)W * (unsigned)(depth / 8));
    unsigned head = (unsigned)((4 - ((uintptr_t)out & 3)) & 3);
    if (head > total) head = total;
    const unsigned nwords = (total - head) / 4;
    unsigned blocks = (nwords + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > GP_MAX_BLOCKS ? GP_MAX_BLOCKS : blocks);
    if (depth == 8) {
        const unsigned P = gp_parts(HW), units = (unsigned)n * P;
        float2* partial = (float2*)ws;
        float2* limits = partial + units;
        hipLaunchKernelGGL(gray_limits_kernel, dim3(units < GP_MAX_BLOCKS ? units : GP_MAX_BLOCKS), dim3(256), 0, s, x, HW, P, units, partial);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(gray_limits_finish_kernel, dim3((unsigned)n < GP_MAX_BLOCKS ? (unsigned)n : GP_MAX_BLOCKS), dim3(64), 0, s,
                           (const float2*)partial, P, (unsigned)n, limits);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(gray_rows_kernel<8>, dim3(blocks), dim3(256), 0, s, x, (unsigned)H, (unsigned)W, total, lut,
                           (const float2*)limits, out, head, nwords);
    } else {
        hipLaunchKernelGGL(gray_rows_kernel<16>, dim3(blocks), dim3(256), 0, s, x, (unsigned)H, (unsigned)W, total,
                           (const unsigned char*)nullptr, (const float2*)nullptr, out, head, nwords);
    }
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
