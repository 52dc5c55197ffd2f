// Device side of FID's InceptionV3 feature network (reference module/piq/feature_extractors/fid_inception.py:134-168 and the block
// forwards :198-316, called from metrics.py:17-31): what the network needs beside the conv kernels -- the input resize, the three
// 3x3 pools and the final mean over the map.  All of it is memory-bound and small next to the 94 convolutions.
//
//   resize_bilinear_kernel   F.interpolate(mode="bilinear", align_corners=False, no antialias) of 1..4 channels into an NHWC map,
//                            optionally followed by 2 x - 1.  The source is addressed by (batch, channel, pixel) strides, so an NCHW
//                            batch is read as it is and leaves as NHWC.  Source coordinates in double (fp32 coordinates at 299
//                            pixels carry a position error of ~2e-5 pixels); a zero weight selects the other sample as it is, so
//                            an equal-size "resize" is a bit-exact copy.
//   pool3x3_kernel<VEC>      one output pixel x (four channels | one channel) per thread and round; source and destination have
//                            their own pixel stride, so a pool reads a block's input and writes into its concat slice.
//                            max: nn.MaxPool2d's scan from -inf over the taps inside the image (padding never wins, NaN does);
//                            avg: sum of the taps inside the image in row-major order, divided by their number.
//   global_avgpool_kernel    one thread per (image, channel): the H W values in pixel order, summed in double.  The order is the
//                            thread's own, so the result does not depend on the grid; no atomics.
#include "common.h"

namespace {

constexpr int INC_THREADS = 256;
constexpr int INC_MAX_BLOCKS = 4096;

struct ResizeParams {
    const float* in;
    float* out;
    long long in_sb, in_sc, in_sp;      // element strides of the source: batch, channel, pixel
    int B, C, H, W, OH, OW, out_ld, normalize;
    double sy, sx;                      // H / OH, W / OW
};

__global__ __launch_bounds__(INC_THREADS) void resize_bilinear_kernel(const ResizeParams p) {
    const long long total = (long long)p.B * p.OH * p.OW;
    const long long step = (long long)gridDim.x * INC_THREADS;
    for (long long e = (long long)blockIdx.x * INC_THREADS + threadIdx.x; e < total; e += step) {
        const int ox = (int)(e % p.OW);
        const long long t = e / p.OW;
        const int oy = (int)(t % p.OH);
        const long long b = t / p.OH;
        // area_pixel_compute_source_index: scale (dst + 0.5) - 0.5, negative values clamped to 0
        double fy = ((double)oy + 0.5) * p.sy - 0.5, fx = ((double)ox + 0.5) * p.sx - 0.5;
        fy = fy < 0.0 ? 0.0 : fy;
        fx = fx < 0.0 ? 0.0 : fx;
        int y0 = (int)fy, x0 = (int)fx;
        y0 = y0 > p.H - 1 ? p.H - 1 : y0;
        x0 = x0 > p.W - 1 ? p.W - 1 : x0;
        const int y1 = y0 + (y0 < p.H - 1 ? 1 : 0), x1 = x0 + (x0 < p.W - 1 ? 1 : 0);
        const float ly = (float)(fy - (double)y0), lx = (float)(fx - (double)x0);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const float* src = p.in + b * p.in_sb;
        const long long o00 = ((long long)y0 * p.W + x0) * p.in_sp, o01 = ((long long)y0 * p.W + x1) * p.in_sp;
        const long long o10 = ((long long)y1 * p.W + x0) * p.in_sp, o11 = ((long long)y1 * p.W + x1) * p.in_sp;
        float* dst = p.out + e * p.out_ld;
        for (int c = 0; c < p.C; ++c) {
            const float* s = src + c * p.in_sc;
            const float top = lx == 0.f ? s[o00] : hx * s[o00] + lx * s[o01];
            float v = top;
            if (ly != 0.f) {
                const float bot = lx == 0.f ? s[o10] : hx * s[o10] + lx * s[o11];
                v = hy * top + ly * bot;
            }
            dst[c] = p.normalize ? 2.f * v - 1.f : v;
        }
    }
}

struct PoolParams {
    const float* in;
    float* out;
    int in_ld, out_ld;
    int B, H, W, C, OH, OW;
    int stride, pad, avg;
};

// nn.MaxPool2d's comparison: a larger value or a NaN replaces the running maximum
__device__ __forceinline__ float pool_max(float r, float v) { return (v > r || v != v) ? v : r; }

template <bool VEC>
__global__ __launch_bounds__(INC_THREADS) void pool3x3_kernel(const PoolParams p) {
    constexpr int V = VEC ? 4 : 1;
    const int CV = p.C / V;
    const long long total = (long long)p.B * p.OH * p.OW * CV;
    const long long step = (long long)gridDim.x * INC_THREADS;
    for (long long e = (long long)blockIdx.x * INC_THREADS + threadIdx.x; e < total; e += step) {
        const int c = (int)(e % CV) * V;
        const long long opix = e / CV;
        const int ox = (int)(opix % p.OW);
        const long long t = opix / p.OW;
        const int oy = (int)(t % p.OH);
        const long long b = t / p.OH;
        float acc[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = p.avg ? 0.f : -INFINITY;
        int taps = 0;
        for (int ty = 0; ty < 3; ++ty) {
            const int iy = oy * p.stride - p.pad + ty;
            if ((unsigned)iy >= (unsigned)p.H) continue;
            for (int tx = 0; tx < 3; ++tx) {
                const int ix = ox * p.stride - p.pad + tx;
                if ((unsigned)ix >= (unsigned)p.W) continue;
                const float* s = p.in + ((b * p.H + iy) * p.W + ix) * p.in_ld + c;
                float v[V];
                if (VEC) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(s);
#pragma unroll
                    for (int k = 0; k < V; ++k) v[k] = q[k];
                } else {
                    v[0] = s[0];
                }
#pragma unroll
                for (int k = 0; k < V; ++k) acc[k] = p.avg ? acc[k] + v[k] : pool_max(acc[k], v[k]);
                ++taps;
            }
        }
        if (p.avg) {
            const float n = (float)taps;      // 4 in a corner, 6 on an edge, 9 inside (count_include_pad=False)
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = acc[k] / n;
        }
        float* d = p.out + opix * p.out_ld + c;
        if (VEC) {
            f32x4 q;
#pragma unroll
            for (int k = 0; k < V; ++k) q[k] = acc[k];
            *reinterpret_cast<f32x4*>(d) = q;
        } else {
            d[0] = acc[0];
        }
    }
}

__global__ __launch_bounds__(INC_THREADS) void global_avgpool_kernel(const float* __restrict__ in, int in_ld, float* __restrict__ out, int out_ld,
                                                                     int B, int HW, int C) {
    const long long total = (long long)B * C;
    const long long step = (long long)gridDim.x * INC_THREADS;
    for (long long e = (long long)blockIdx.x * INC_THREADS + threadIdx.x; e < total; e += step) {
        const int c = (int)(e % C);
        const long long b = e / C;
        const float* s = in + b * HW * in_ld + c;
        double sum = 0.0;
        for (int i = 0; i < HW; ++i) sum += (double)s[(long long)i * in_ld];
        out[b * out_ld + c] = (float)(sum / (double)HW);
    }
}

unsigned inc_blocks(long long total) {
    long long blocks = (total + INC_THREADS - 1) / INC_THREADS;
    return (unsigned)(blocks > INC_MAX_BLOCKS ? INC_MAX_BLOCKS : blocks);
}

}  // namespace

extern "C" int mtd_resize_bilinear(const float* in, long long in_sb, long long in_sc, long long in_sp, float* out, int out_ld, int B, int C,
                                   int H, int W, int OH, int OW, int normalize, void* stream) {
    if (!in || !out || B <= 0 || C <= 0 || C > MTD_RESIZE_MAX_C || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return MTD_EINVAL;
    if (out_ld < C || in_sb <= 0 || in_sc <= 0 || in_sp <= 0) return MTD_EINVAL;
    ResizeParams p;
    p.in = in, p.out = out, p.in_sb = in_sb, p.in_sc = in_sc, p.in_sp = in_sp;
    p.B = B, p.C = C, p.H = H, p.W = W, p.OH = OH, p.OW = OW, p.out_ld = out_ld, p.normalize = normalize ? 1 : 0;
    p.sy = (double)H / (double)OH, p.sx = (double)W / (double)OW;
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3(inc_blocks((long long)B * OH * OW)), dim3(INC_THREADS), 0, (hipStream_t)stream, p);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_pool3x3(const float* in, int in_ld, float* out, int out_ld, int B, int H, int W, int C, int mode, void* stream) {
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || in_ld < C || out_ld < C) return MTD_EINVAL;
    if (mode != MTD_POOL_MAX_S2 && mode != MTD_POOL_MAX_S1P1 && mode != MTD_POOL_AVG_S1P1) return MTD_EINVAL;
    if (mode == MTD_POOL_MAX_S2 && (H < 3 || W < 3)) return MTD_EINVAL;
    PoolParams p;
    p.in = in, p.out = out, p.in_ld = in_ld, p.out_ld = out_ld, p.B = B, p.H = H, p.W = W, p.C = C;
    p.stride = mode == MTD_POOL_MAX_S2 ? 2 : 1;
    p.pad = mode == MTD_POOL_MAX_S2 ? 0 : 1;
    p.avg = mode == MTD_POOL_AVG_S1P1 ? 1 : 0;
    p.OH = mode == MTD_POOL_MAX_S2 ? (H - 3) / 2 + 1 : H;
    p.OW = mode == MTD_POOL_MAX_S2 ? (W - 3) / 2 + 1 : W;
    const bool vec = (C % 4) == 0 && (in_ld % 4) == 0 && (out_ld % 4) == 0 && aligned16(in) && aligned16(out);
    const long long total = (long long)B * p.OH * p.OW * (vec ? C / 4 : C);
    if (vec) hipLaunchKernelGGL(pool3x3_kernel<true>, dim3(inc_blocks(total)), dim3(INC_THREADS), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(pool3x3_kernel<false>, dim3(inc_blocks(total)), dim3(INC_THREADS), 0, (hipStream_t)stream, p);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_global_avgpool(const float* in, int in_ld, float* out, int out_ld, int B, int H, int W, int C, void* stream) {
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || in_ld < C || out_ld < C) return MTD_EINVAL;
    if ((long long)H * W >= (1ll << 31)) return MTD_EINVAL;
    hipLaunchKernelGGL(global_avgpool_kernel, dim3(inc_blocks((long long)B * C)), dim3(INC_THREADS), 0, (hipStream_t)stream, in, in_ld, out, out_ld,
                       B, H * W, C);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
