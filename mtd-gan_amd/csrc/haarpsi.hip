// The Haar wavelet perceptual similarity index of the test loop (the reference vendors it in module/piq: haarpsi.py, haarpsi
// with scales = 3) of single-channel fp32 images in [0, 1], image by image, for up to three sources a[k] against one target b
// (the convention of mtd_iqa_each, whose conventions this file follows).  DESIGN 3.16.
//   * filter arithmetic in fp32: the rescale by 255, the 2 x 2 average pool and the box sums of the Haar filters (their
//     weights +-1/k are powers of two, so a coefficient is a difference of box sums, scaled exactly);
//   * from the coefficients on in double: the similarity ratios, a true 1 / (1 + exp(-z)) and every per-image sum, in a fixed
//     order (thread-strided, then block_sum256's tree; the tile partials of an image are summed by one workgroup in the same
//     way), no atomics: an image's numbers do not depend on the batch it is in, on its source slot or on the other sources;
//   * a 32 x 32 tile of the (subsampled) map keeps its 39 x 39 halo of both images in LDS -- 3 pixels above and to the left, 4
//     below and to the right, the window of the k = 8 filter with piq's asymmetric zero padding -- and all six coefficient maps
//     (k = 2, 4, 8, two orientations) come from it.  With subsample the halo is pooled on the way in from the 2 x 2 source
//     pixels: the subsampled image is never stored.
// Launches per batch: 1 tiles + 1 finish, for all na * B pairs.
#include "each_metric.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int HT = 32;                        // output tile
constexpr int HB = 3, HA = 4;                 // halo before (above / left) and after (below / right)
constexpr int HL = HT + HB + HA;              // 39
constexpr int HP_PARTS = 4;                   // (num, den) of the filter as it is, then of its transpose

// Pixel (y, x) of the map the filters see: 255 * image, with SUB after piq's zero padding at the bottom and the right by
// max(H % 2, W % 2) and its 2 x 2 average pool.  0 <= y < h, 0 <= x < w; then 2y < H and 2x < W, and only row 2y + 1 or column
// 2x + 1 can be the padded one.  The products are rounded on their own, as the reference's rescaled tensor holds them.
template <bool SUB>
__device__ __forceinline__ float hp_pixel(const float* __restrict__ img, int H, int W, int y, int x) {
    if (!SUB) return __fmul_rn(255.f, img[(long long)y * W + x]);
    const int y0 = 2 * y, x0 = 2 * x;
    const bool yb = y0 + 1 < H, xb = x0 + 1 < W;
    const float* r0 = img + (long long)y0 * W + x0;
    float s = __fmul_rn(255.f, r0[0]);
    s += xb ? __fmul_rn(255.f, r0[1]) : 0.f;
    s += yb ? __fmul_rn(255.f, r0[W]) : 0.f;
    s += (yb && xb) ? __fmul_rn(255.f, r0[W + 1]) : 0.f;
    return 0.25f * s;
}

// The six coefficients of one image at one pixel; P[r * HL + c] is the map at (y - 3 + r, x - 3 + c), zero beyond it.
// cf[2 s + o]: scale s (k = 2, 4, 8), o = 0 the filter as it is (top k/2 rows +1/k, bottom k/2 rows -1/k), o = 1 its transpose.
// The k x k window starts k/2 - 1 before the pixel: rows and columns 3..4, 2..5, 0..7 of P.
__device__ __forceinline__ void hp_coefficients(const float* P, float (&cf)[6]) {
    float t2 = 0.f, b2 = 0.f, d2 = 0.f, t4 = 0.f, b4 = 0.f, d4 = 0.f, t8 = 0.f, b8 = 0.f, d8 = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float* row = P + r * HL;
        const float l2 = row[3], r2 = row[4];
        const float l4 = row[2] + l2, r4 = r2 + row[5];
        const float l8 = (row[0] + row[1]) + l4, r8 = r4 + (row[6] + row[7]);
        if (r < 4) t8 += l8 + r8; else b8 += l8 + r8;
        d8 += l8 - r8;
        if (r >= 2 && r <= 5) {
            if (r < 4) t4 += l4 + r4; else b4 += l4 + r4;
            d4 += l4 - r4;
        }
        if (r == 3) { t2 = l2 + r2; d2 += l2 - r2; }
        if (r == 4) { b2 = l2 + r2; d2 += l2 - r2; }
    }
    cf[0] = 0.5f * (t2 - b2);
    cf[1] = 0.5f * d2;
    cf[2] = 0.25f * (t4 - b4);
    cf[3] = 0.25f * d4;
    cf[4] = 0.125f * (t8 - b8);
    cf[5] = 0.125f * d8;
}

// grid (tiles of w, tiles of h, na * B); blockIdx.z = source * B + image.  The four sums of the tile go to partial[4 blk], blk
// the linear workgroup index, so the partials of one (source, image) are contiguous.
template <bool SUB>
__global__ __launch_bounds__(256) void haarpsi_tiles_kernel(EachSets src, const float* __restrict__ b, int B, int H, int W, int h, int w,
                                                            float c, float alpha, double* __restrict__ partial) {
    __shared__ float As[HL * HL], Bs[HL * HL];
    __shared__ double red[HP_PARTS * 256];
    const int si = blockIdx.z / B, i = blockIdx.z - si * B;
    const float* __restrict__ a = each_pick(src, si) + (long long)i * H * W;
    const float* __restrict__ bi = b + (long long)i * H * W;
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * HT, ty0 = blockIdx.y * HT;
    for (int e = tid; e < HL * HL; e += 256) {
        const int ly = e / HL, lx = e - ly * HL;
        const int y = ty0 + ly - HB, x = tx0 + lx - HB;
        float va = 0.f, vb = 0.f;                                // the filters' zero padding
        if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) {
            va = hp_pixel<SUB>(a, H, W, y, x);
            vb = hp_pixel<SUB>(bi, H, W, y, x);
        }
        As[e] = va;
        Bs[e] = vb;
    }
    __syncthreads();
    const double cd = (double)c, ad = (double)alpha;
    double sums[HP_PARTS] = {0.0, 0.0, 0.0, 0.0};
    for (int e = tid; e < HT * HT; e += 256) {
        const int ly = e / HT, lx = e - ly * HT;
        if (ty0 + ly < h && tx0 + lx < w) {
            float ca[6], cb[6];
            hp_coefficients(As + ly * HL + lx, ca);
            hp_coefficients(Bs + ly * HL + lx, cb);
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const double wt = (double)fmaxf(fabsf(ca[4 + o]), fabsf(cb[4 + o]));
                double sim = 0.0;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    // (the products of two floats are exact in double: equal magnitudes give exactly 1)
                    const double ma = (double)fabsf(ca[2 * s + o]), mb = (double)fabsf(cb[2 * s + o]);
                    sim += (2.0 * (ma * mb) + cd) / (ma * ma + mb * mb + cd);
                }
                const double sg = 1.0 / (1.0 + exp(-ad * (0.5 * sim)));
                sums[2 * o] += sg * wt;
                sums[2 * o + 1] += wt;
            }
        }
    }
    block_sum256(sums, red);
    each_store(partial, sums);
}

// One workgroup per (source, image) g: the image's tile partials in a fixed order (thread t takes tiles t, t + 256, ..., then
// the tree), then piq's closing formula in thread 0, with float32's eps as its public float32 call has it.
__global__ __launch_bounds__(256) void haarpsi_finish_kernel(const double* __restrict__ partial, int tiles, float alpha,
                                                             double* __restrict__ out, double* __restrict__ parts) {
    __shared__ double red[HP_PARTS * 256];
    const int g = blockIdx.x;
    double sums[HP_PARTS];
    each_fold(partial + (long long)HP_PARTS * g * tiles, tiles, sums, red);
    if (threadIdx.x != 0) return;
    if (parts) {
#pragma unroll
        for (int q = 0; q < HP_PARTS; ++q) parts[(long long)HP_PARTS * g + q] = sums[q];
    }
    const double eps = (double)FLT_EPSILON;
    const double s = ((sums[0] + sums[2]) + eps) / ((sums[1] + sums[3]) + eps);
    const double lg = log(s / (1.0 - s)) / (double)alpha;      // two all-zero images: s = 1, +inf, as piq gives
    out[g] = lg * lg;
}

struct HpPlan {
    bool ok;
    int h, w, tx, ty;
    long long doubles;
};

HpPlan haarpsi_plan(int na, int B, int H, int W, int subsample) {
    HpPlan p = {};
    if (na < 1 || na > 3 || B < 1 || (long long)na * B > 65535) return p;
    if (H < 16 || W < 16 || (long long)H * W > (1LL << 30)) return p;       // piq's 2^(scales + 1); pixel indices of one image stay in int
    const int pad = subsample ? ((H % 2) | (W % 2)) : 0;
    p.h = subsample ? (H + pad) / 2 : H;
    p.w = subsample ? (W + pad) / 2 : W;
    p.tx = (p.w + HT - 1) / HT;
    p.ty = (p.h + HT - 1) / HT;
    if (p.ty > 65535) return p;                                             // the grid's y limit
    p.doubles = (long long)HP_PARTS * na * B * p.tx * p.ty;
    if (p.doubles > (1LL << 40) / (long long)sizeof(double)) return p;
    p.ok = true;
    return p;
}

}  // namespace

extern "C" size_t mtd_haarpsi_ws_bytes(int na, int B, int H, int W, int subsample) {
    const HpPlan p = haarpsi_plan(na, B, H, W, subsample);
    return p.ok ? (size_t)p.doubles * sizeof(double) : 0;
}

extern "C" int mtd_haarpsi_each(const float* const a[3], int na, const float* b, int B, int H, int W, int subsample, float c, float alpha,
                                double* out, double* parts, void* ws, void* stream) {
    if (!a || !b || !out || !ws || !(c > 0.f) || !(alpha > 0.f)) return MTD_EINVAL;
    const HpPlan p = haarpsi_plan(na, B, H, W, subsample);
    if (!p.ok) return MTD_EINVAL;
    EachSets src = {};                           // the sources
    for (int k = 0; k < na; ++k) {
        if (!a[k]) return MTD_EINVAL;
        src.p[k] = a[k];
    }
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)ws;
    const dim3 grid(p.tx, p.ty, na * B);
    if (subsample) hipLaunchKernelGGL(haarpsi_tiles_kernel<true>, grid, dim3(256), 0, s, src, b, B, H, W, p.h, p.w, c, alpha, partial);
    else hipLaunchKernelGGL(haarpsi_tiles_kernel<false>, grid, dim3(256), 0, s, src, b, B, H, W, p.h, p.w, c, alpha, partial);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(haarpsi_finish_kernel, dim3(na * B), dim3(256), 0, s, (const double*)partial, p.tx * p.ty, alpha, out, parts);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
