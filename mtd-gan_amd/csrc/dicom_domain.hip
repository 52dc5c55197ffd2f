// The two ends of an evaluation run, where a CT series enters and leaves in the stored pixel values of its DICOM files
// (dicom_io.py).  The reference does both on the host in numpy: get_pixels_hu (create_datasets/Mayo.py:19-43) on
// the way in, dicom_denormalize + save_dicom (utils.py:167-194) on the way out.  Here they are three elementwise kernels, restated
// operation by operation so that the integers are the reference's:
//   stored -> HU            int16 view of the word, -2000 -> 0, float64 slope with a truncating cast, int16 intercept with wrap-around
//   stored -> window        the same, then the window of mtd_hu_window (csrc/sampler.hip) in the same operations; optional HU output
//   window -> stored        fp32 denormalisation (product, then sum), fp32 intercept, truncating cast, fp32 slope division
// HBM-bound (6 to 8 bytes per pixel).  The pixel arrays are taken as ONE run of S * H * W elements: a lane handles the 8 pixels of
// one 16-byte vector of the 16-bit array that sets the grid (the stored words on the way in, the output on the way out), aligned in
// memory whatever the tensor's own offset, and the at most 7 pixels before the first and after the last whole vector are scalar.
// The other arrays of a launch use 16-byte accesses when they share that phase and scalar ones when they do not.  A vector may
// straddle slices: (slope, intercept) are looked up per pixel, reloaded only where the slice changes.  Every output element is
// written exactly once and nothing outside the arrays is touched.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)      // numpy rounds after every operation

namespace {

constexpr unsigned DD_MAX_BLOCKS = 2048;      // grid cap (256 CUs x 8); the rest is strided
typedef short i16x8 __attribute__((ext_vector_type(8)));

// casts to int16 that saturate (the reference's numpy casts are defined only inside the range; NaN gives 0)
__device__ __forceinline__ int sat16(double x) { return x != x ? 0 : (x <= -32768.0 ? -32768 : (x >= 32767.0 ? 32767 : (int)x)); }
__device__ __forceinline__ int sat16(float x) { return x != x ? 0 : (x <= -32768.f ? -32768 : (x >= 32767.f ? 32767 : (int)x)); }

// (slope, intercept) of the slice a pixel lies in, kept while consecutive pixels stay in it.  at(i) positions on pixel i; step()
// is called BEFORE each pixel is used and moves to the next slice only when a pixel of it is really there, so rescale[2 S] is
// never read.
struct SliceCursor {
    const double* rescale;
    unsigned HW, r;
    long long s;
    double slope;
    float slope_f, icpt_f;
    int icpt16;
    bool scaled;
    __device__ __forceinline__ void load() {
        slope = rescale[2 * s];
        const double ic = rescale[2 * s + 1];
        scaled = slope != 1.0;
        slope_f = (float)slope;
        icpt_f = (float)ic;            // save_dicom: np.float32(intercept)
        icpt16 = sat16(ic);            // get_pixels_hu: np.int16(intercept), toward zero
    }
    __device__ __forceinline__ void at(unsigned i) {
        const unsigned q = i / HW;
        s = q; r = i - q * HW;
        load();
    }
    __device__ __forceinline__ void step() {
        if (r == HW) { r = 0; ++s; load(); }
        ++r;
    }
};
// (at(i) leaves r = offset of pixel i; step() then counts it: after at(i), step() must see r < HW, which at() guarantees)

// get_pixels_hu on one word
__device__ __forceinline__ short stored_to_hu(short word, const SliceCursor& c) {
    int p = word;
    if (p == -2000) p = 0;
    if (c.scaled) p = sat16(c.slope * (double)p);
    return (short)(p + c.icpt16);                                   // 16-bit wrap-around
}

// mtd_hu_window's operations (csrc/sampler.hip: window)
__device__ __forceinline__ float hu_window(short hu, float a_min, float a_max) {
    const float v = ((float)hu - a_min) / (a_max - a_min);
    return fminf(fmaxf(v, 0.f), 1.f);
}

// dicom_denormalize + save_dicom on one value
__device__ __forceinline__ short window_to_stored(float v, const SliceCursor& c, float a_min, float range, int clip, int rounding) {
    if (clip) v = fminf(fmaxf(v, 0.f), 1.f);
    float hu = range * v;
    hu = hu + a_min;
    const float t = hu - c.icpt_f;
    int s = sat16(rounding ? rintf(t) : truncf(t));                 // rintf: to nearest, ties to even
    if (c.scaled) {
        const float q = (float)s / c.slope_f;
        s = sat16(rounding ? rintf(q) : truncf(q));
    }
    return (short)s;
}

__device__ __forceinline__ void load8(const short* p, bool vec, short (&v)[8]) {
    if (vec) {
        const i16x8 w = *reinterpret_cast<const i16x8*>(p);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = w[k];
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[k];
    }
}
__device__ __forceinline__ void load8(const float* p, bool vec, float (&v)[8]) {
    if (vec) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = a[k]; v[4 + k] = b[k]; }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[k];
    }
}
__device__ __forceinline__ void store8(short* p, bool vec, const short (&v)[8]) {
    if (vec) {
        i16x8 w;
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = v[k];
        *reinterpret_cast<i16x8*>(p) = w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = v[k];
    }
}
__device__ __forceinline__ void store8(float* p, bool vec, const float (&v)[8]) {
    if (vec) {
        *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = v[k];
    }
}

// Pixel index of edge element e of 14: the `head` pixels before the first whole vector, then those after the last (>= N: none).
__device__ __forceinline__ unsigned edge_pixel(unsigned e, unsigned head, unsigned nvec) {
    return e < head ? e : head + 8 * nvec + (e - head);
}

// stored + head is 16-byte aligned; out_vec / hu_vec: out + head / hu_out + head are too
template <bool WIN, bool HUOUT>
__global__ __launch_bounds__(256) void stored_in_kernel(const short* __restrict__ stored, unsigned N, unsigned HW,
                                                        const double* __restrict__ rescale, float a_min, float a_max,
                                                        float* __restrict__ out, short* __restrict__ hu_out, unsigned head,
                                                        unsigned nvec, bool out_vec, bool hu_vec) {
    SliceCursor c;
    c.rescale = rescale; c.HW = HW;
    for (unsigned w = blockIdx.x * 256 + threadIdx.x; w < nvec; w += gridDim.x * 256) {
        const unsigned i = head + 8 * w;
        short in[8], hu[8];
        float f[8];
        load8(stored + i, true, in);
        c.at(i);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            c.step();
            hu[k] = stored_to_hu(in[k], c);
            if (WIN) f[k] = hu_window(hu[k], a_min, a_max);
        }
        if (WIN) store8(out + i, out_vec, f);
        if (HUOUT) store8(hu_out + i, hu_vec, hu);
    }
    if (blockIdx.x == 0 && threadIdx.x < 14) {
        const unsigned i = edge_pixel(threadIdx.x, head, nvec);
        if (i < N) {
            c.at(i);
            c.step();
            const short hu = stored_to_hu(stored[i], c);
            if (WIN) out[i] = hu_window(hu, a_min, a_max);
            if (HUOUT) hu_out[i] = hu;
        }
    }
}

// out + head is 16-byte aligned; v_vec / ref_vec: v + head / ref + head are too
template <bool OUTSIDE>
__global__ __launch_bounds__(256) void stored_out_kernel(const float* __restrict__ v, unsigned N, unsigned HW,
                                                         const double* __restrict__ rescale, float a_min, float a_max, int clip,
                                                         int rounding, const short* __restrict__ ref, short* __restrict__ out,
                                                         unsigned head, unsigned nvec, bool v_vec, bool ref_vec) {
    const float range = a_max - a_min;
    SliceCursor c;
    c.rescale = rescale; c.HW = HW;
    for (unsigned w = blockIdx.x * 256 + threadIdx.x; w < nvec; w += gridDim.x * 256) {
        const unsigned i = head + 8 * w;
        float f[8];
        short in[8], res[8];
        load8(v + i, v_vec, f);
        if (OUTSIDE) load8(ref + i, ref_vec, in);
        c.at(i);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            c.step();
            res[k] = window_to_stored(f[k], c, a_min, range, clip, rounding);
            if (OUTSIDE) {
                const float h = (float)stored_to_hu(in[k], c);
                if (h < a_min || h > a_max) res[k] = in[k];
            }
        }
        store8(out + i, true, res);
    }
    if (blockIdx.x == 0 && threadIdx.x < 14) {
        const unsigned i = edge_pixel(threadIdx.x, head, nvec);
        if (i < N) {
            c.at(i);
            c.step();
            short res = window_to_stored(v[i], c, a_min, range, clip, rounding);
            if (OUTSIDE) {
                const short word = ref[i];
                const float h = (float)stored_to_hu(word, c);
                if (h < a_min || h > a_max) res = word;
            }
            out[i] = res;
        }
    }
}

// N = S H W when the shape is one these kernels take (32-bit pixel indices), else 0
unsigned dd_pixels(int S, int H, int W) {
    if (S <= 0 || H <= 0 || W <= 0) return 0;
    const long long HW = (long long)H * W;
    if (HW >= (1ll << 31) || (long long)S * HW >= (1ll << 31)) return 0;
    return (unsigned)((long long)S * HW);
}

// pixels before the first 16-byte boundary of a 16-bit array (at most N), and the whole vectors after them
void dd_split(const void* p, unsigned N, unsigned& head, unsigned& nvec) {
    head = (unsigned)(((16 - ((uintptr_t)p & 15)) & 15) / 2);
    if (head > N) head = N;
    nvec = (N - head) / 8;
}

unsigned dd_blocks(unsigned nvec) {
    const unsigned b = (nvec + 255) / 256;
    return b < 1 ? 1 : (b > DD_MAX_BLOCKS ? DD_MAX_BLOCKS : b);
}

template <typename T>
bool dd_vec(const T* p, unsigned head) { return (((uintptr_t)(p + head)) & 15) == 0; }

}  // namespace

extern "C" int mtd_stored_to_window(const short* stored, int S, int H, int W, const double* rescale, float a_min, float a_max,
                                    float* out, short* hu_out, void* stream) {
    const unsigned N = dd_pixels(S, H, W);
    if (!stored || !rescale || !out || !N || !(a_max > a_min)) return MTD_EINVAL;
    if (((uintptr_t)stored & 1) || ((uintptr_t)hu_out & 1) || ((uintptr_t)out & 3) || ((uintptr_t)rescale & 7)) return MTD_EALIGN;
    unsigned head, nvec;
    dd_split(stored, N, head, nvec);
    const bool out_vec = dd_vec(out, head), hu_vec = hu_out && dd_vec(hu_out, head);
    hipStream_t s = (hipStream_t)stream;
    if (hu_out)
        hipLaunchKernelGGL((stored_in_kernel<true, true>), dim3(dd_blocks(nvec)), dim3(256), 0, s, stored, N, (unsigned)H * (unsigned)W,
                           rescale, a_min, a_max, out, hu_out, head, nvec, out_vec, hu_vec);
    else
        hipLaunchKernelGGL((stored_in_kernel<true, false>), dim3(dd_blocks(nvec)), dim3(256), 0, s, stored, N, (unsigned)H * (unsigned)W,
                           rescale, a_min, a_max, out, (short*)nullptr, head, nvec, out_vec, false);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_stored_to_hu(const short* stored, int S, int H, int W, const double* rescale, short* hu_out, void* stream) {
    const unsigned N = dd_pixels(S, H, W);
    if (!stored || !rescale || !hu_out || !N) return MTD_EINVAL;
    if (((uintptr_t)stored & 1) || ((uintptr_t)hu_out & 1) || ((uintptr_t)rescale & 7)) return MTD_EALIGN;
    unsigned head, nvec;
    dd_split(stored, N, head, nvec);
    hipLaunchKernelGGL((stored_in_kernel<false, true>), dim3(dd_blocks(nvec)), dim3(256), 0, (hipStream_t)stream, stored, N,
                       (unsigned)H * (unsigned)W, rescale, 0.f, 1.f, (float*)nullptr, hu_out, head, nvec, false, dd_vec(hu_out, head));
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_window_to_stored(const float* v, int S, int H, int W, const double* rescale, float a_min, float a_max, int clip,
                                    int rounding, int outside, const short* ref_stored, short* out, void* stream) {
    const unsigned N = dd_pixels(S, H, W);
    if (!v || !rescale || !out || !N || !(a_max > a_min)) return MTD_EINVAL;
    if ((rounding != 0 && rounding != 1) || (outside != 0 && outside != 1) || (outside == 1 && !ref_stored)) return MTD_EINVAL;
    if (((uintptr_t)v & 3) || ((uintptr_t)out & 1) || ((uintptr_t)ref_stored & 1) || ((uintptr_t)rescale & 7)) return MTD_EALIGN;
    unsigned head, nvec;
    dd_split(out, N, head, nvec);
    const bool v_vec = dd_vec(v, head);
    hipStream_t s = (hipStream_t)stream;
    if (outside)
        hipLaunchKernelGGL((stored_out_kernel<true>), dim3(dd_blocks(nvec)), dim3(256), 0, s, v, N, (unsigned)H * (unsigned)W, rescale,
                           a_min, a_max, clip != 0, rounding, ref_stored, out, head, nvec, v_vec, dd_vec(ref_stored, head));
    else
        hipLaunchKernelGGL((stored_out_kernel<false>), dim3(dd_blocks(nvec)), dim3(256), 0, s, v, N, (unsigned)H * (unsigned)W, rescale,
                           a_min, a_max, clip != 0, rounding, (const short*)nullptr, out, head, nvec, v_vec, false);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
