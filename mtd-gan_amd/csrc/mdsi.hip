// The mean deviation similarity index of the test loop (the reference vendors it in module/piq: mdsi.py) of single-channel fp32
// images in [0, 1], image by image, for up to three sources a[k] against one target b (the convention of mtd_fsim_each and
// mtd_haarpsi_each).  DESIGN 3.19.  piq runs a single-channel image as three equal colour channels: the LHM channels of the
// pooled image are the pooled value times the row sums of piq's matrix (summed product by product, as the matrix product does).
//   * everything is double from the first operation on the fp32 pixels, and every per-image sum runs in a fixed order
//     (block_sum256's tree over a 16 x 16 tile, the tiles of an image by one workgroup in the same way), no floating-point
//     atomics: an image's numbers depend neither on the batch it is in, nor on its source slot, nor on the other sources;
//   * two passes over the pooled map: the per-image mean of the complex map z = gcs^q, then the sum of |z - mean|^rho with z
//     recomputed by the same function (nothing per pixel is stored);
//   * the expressions are grouped so that an image against itself gives z = 1 at every pixel exactly, hence a mean of exactly 1
//     and a score of exactly 0.
// Launches per chunk of the batch: tiles (pass one), finish (means), tiles (pass two), finish (scores).
#include "each_metric.h"
#include <float.h>
#include <math.h>

#pragma clang fp contract(off)      // no fused multiply-adds: equal inputs give equal maps and ratios of exactly 1

namespace {

constexpr int MD_CT = 16;                     // the tile: 16 x 16 pooled pixels, one per thread, with an 18 x 18 halo
constexpr int MD_HL = MD_CT + 2;
constexpr int MD_MIN_N = MTD_MDSI_MIN_SIDE, MD_MAX_N = MTD_MDSI_MAX_SIDE;
constexpr long long MD_WS_TARGET = 16LL << 20;

struct MdOpts { double c1, c2, c3, alpha, beta, gamma, rho, q, o; int mult; };

// Pixel (y, x) of the pooled map of 255 * image: piq pads [(k - 1) / 2, k / 2] ZEROS on each axis (k >= 2), then avg_pool2d with
// kernel and stride k (floor; the padding counts in the divisor).  0 <= y < (H + k - 1) / k, likewise x.
__device__ __forceinline__ double md_pixel(const float* __restrict__ img, int H, int W, int k, int y, int x) {
    if (k == 1) return 255.0 * (double)img[(long long)y * W + x];
    const int y0 = y * k - (k - 1) / 2, x0 = x * k - (k - 1) / 2;
    double s = 0.0;
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const int yy = y0 + dy, xx = x0 + dx;
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) s += 255.0 * (double)img[(long long)yy * W + xx];
        }
    return s / (double)(k * k);
}

// Prewitt magnitude at the centre of a 3 x 3 neighbourhood of the 18-wide halo tile (zero padding is in the tile).  piq's
// weights are +-1 / 3 rounded to fp32, in a float64 run too.
__device__ __forceinline__ double md_prewitt(double a, double b, double c, double d, double f, double g, double h, double i) {
    const double third = (double)(1.f / 3.f);
    const double gx = third * ((c - a) + (f - d) + (i - g));
    const double gy = third * ((g - a) + (h - b) + (i - c));
    return sqrt(gx * gx + gy * gy);
}

struct MdZ { double re, im; };

// (|base|^e, e * atan2(0, base)) of a real base as real and imaginary part: piq's pow_for_complex on a 4-D tensor.
__device__ __forceinline__ MdZ md_real_pow(double base, double e) {
    const double r = pow(fabs(base), e), phi = atan2(0.0, base) * e;
    return {r * cos(phi), r * sin(phi)};
}

// z = gcs^q at a pooled pixel from the three gradient magnitudes and the chromaticity channels.
__device__ __forceinline__ MdZ md_z(double ga, double gb, double gavg, double Ha, double Hb, double Ma, double Mb, const MdOpts& o) {
    const double gs = each_similarity(ga, gb, o.c1) + each_similarity(ga, gavg, o.c2) - each_similarity(gb, gavg, o.c2);
    const double cs = (2.0 * (Ha * Hb + Ma * Mb) + o.c3) / ((Ha * Ha + Hb * Hb) + (Ma * Ma + Mb * Mb) + o.c3);
    if (!o.mult) return md_real_pow(o.alpha * gs + (1.0 - o.alpha) * cs, o.q);
    const MdZ g = md_real_pow(gs, o.gamma), c = md_real_pow(cs, o.beta);
    const double re = g.re * c.re, im = g.im + c.im;               // (as piq combines the two: product of the first, sum of the second components)
    const double r = pow(sqrt(re * re + im * im), o.q), phi = atan2(im, re) * o.q;
    return {r * cos(phi), r * sin(phi)};
}

// grid (ceil(wp / 16), ceil(hp / 16), na * Bc); blockIdx.z = source * Bc + image of the chunk.  PASS 1: the tile's sums of
// re z and im z -> partial[2 * blk ..]; PASS 2: its sum of |z - mean|^rho -> partial[blk].
template <int PASS>
__global__ __launch_bounds__(256) void mdsi_tile_kernel(EachSets imgs, int Bc, int i0, int H, int W, int k, int hp, int wp, MdOpts o,
                                                        const double* __restrict__ mean, double* __restrict__ partial) {
    __shared__ double Pa[MD_HL * MD_HL], Pb[MD_HL * MD_HL], La[MD_HL * MD_HL], Lb[MD_HL * MD_HL];
    __shared__ double red[2 * 256];
    const int s = blockIdx.z / Bc, i = blockIdx.z - s * Bc;
    const float* __restrict__ a = each_pick(imgs, s) + (long long)(i0 + i) * H * W;         // sets 0..2: the sources; 3: the target
    const float* __restrict__ b = imgs.p[3] + (long long)(i0 + i) * H * W;
    const int tx0 = blockIdx.x * MD_CT, ty0 = blockIdx.y * MD_CT;
    // the row sums of piq's RGB -> LHM matrix, its entries rounded to fp32 as piq holds them, product by product
    const double l0 = (double)0.2989f, l1 = (double)0.587f, l2 = (double)0.114f;
    const double h0 = (double)0.3f, h1 = (double)0.04f, h2 = (double)-0.35f;
    const double m0 = (double)0.34f, m1 = (double)-0.6f, m2 = (double)0.17f;
    for (int e = threadIdx.x; e < MD_HL * MD_HL; e += 256) {
        const int ly = e / MD_HL, lx = e - ly * MD_HL;
        const int y = ty0 + ly - 1, x = tx0 + lx - 1;
        double va = 0.0, vb = 0.0;                               // the gradient filters' zero padding
        if ((unsigned)y < (unsigned)hp && (unsigned)x < (unsigned)wp) {
            va = md_pixel(a, H, W, k, y, x);
            vb = md_pixel(b, H, W, k, y, x);
        }
        Pa[e] = va;
        Pb[e] = vb;
        La[e] = va * l0 + va * l1 + va * l2;
        Lb[e] = vb * l0 + vb * l1 + vb * l2;
    }
    __syncthreads();
    const int ly = threadIdx.x / MD_CT, lx = threadIdx.x - ly * MD_CT;
    double sums[2] = {0.0, 0.0};
    if (ty0 + ly < hp && tx0 + lx < wp) {
        const int c = (ly + 1) * MD_HL + lx + 1;
        double na[8], nb[8], nv[8];
        const int off[8] = {-MD_HL - 1, -MD_HL, -MD_HL + 1, -1, 1, MD_HL - 1, MD_HL, MD_HL + 1};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            na[j] = La[c + off[j]];
            nb[j] = Lb[c + off[j]];
            nv[j] = (na[j] + nb[j]) / 2.0;
        }
        const double ga = md_prewitt(na[0], na[1], na[2], na[3], na[4], na[5], na[6], na[7]);
        const double gb = md_prewitt(nb[0], nb[1], nb[2], nb[3], nb[4], nb[5], nb[6], nb[7]);
        const double gv = md_prewitt(nv[0], nv[1], nv[2], nv[3], nv[4], nv[5], nv[6], nv[7]);
        const double pa = Pa[c], pb = Pb[c];
        const MdZ z = md_z(ga, gb, gv, pa * h0 + pa * h1 + pa * h2, pb * h0 + pb * h1 + pb * h2, pa * m0 + pa * m1 + pa * m2,
                           pb * m0 + pb * m1 + pb * m2, o);
        if (PASS == 1) {
            sums[0] = z.re;
            sums[1] = z.im;
        } else {
            const double dr = z.re - mean[2 * blockIdx.z], di = z.im - mean[2 * blockIdx.z + 1];
            sums[0] = pow(sqrt(dr * dr + di * di), o.rho);
        }
    }
    block_sum256(sums, red);
    if (PASS == 1) {
        each_store(partial, sums);
    } else {
        const double dev[1] = {sums[0]};
        each_store(partial, dev);
    }
}

// One workgroup per (source, image of the chunk) g: the tile partials in a fixed order.  PASS 1: mean[2 g ..] = sums / n.
// PASS 2: the score (sum / n)^(o / rho), and the parts (mean re, mean im, sum of the deviations).
template <int PASS>
__global__ __launch_bounds__(256) void mdsi_finish_kernel(const double* __restrict__ partial, int tiles, double n, int Bc, int i0, int B, MdOpts o,
                                                          double* __restrict__ mean, double* __restrict__ out, double* __restrict__ parts) {
    __shared__ double red[2 * 256];
    const int g = blockIdx.x, s = g / Bc, i = g - s * Bc;
    constexpr int Q = PASS == 1 ? 2 : 1;
    double sums[Q];
    each_fold(partial + (long long)Q * g * tiles, tiles, sums, red);
    if (threadIdx.x != 0) return;
    if constexpr (PASS == 1) {
        mean[2 * g] = sums[0] / n;
        mean[2 * g + 1] = sums[1] / n;
        return;
    }
    const long long at = (long long)s * B + i0 + i;
    out[at] = pow(sums[0] / n, o.o / o.rho);
    if (parts) {
        parts[MTD_MDSI_PARTS * at] = mean[2 * g];
        parts[MTD_MDSI_PARTS * at + 1] = mean[2 * g + 1];
        parts[MTD_MDSI_PARTS * at + 2] = sums[0];
    }
}

struct MdPlan {
    bool ok;
    int Bc, hp, wp, tiles;
    long long mean, partial, bytes;
};

// The workspace holds, per source and image of a chunk, two doubles per tile and the two means.  Bc is the largest count for
// which that stays within 16 MiB (each_chunk).
MdPlan mdsi_plan(int na, int B, int H, int W, int k) {
    MdPlan p = {};
    if (na < 1 || na > 3 || B < 1 || B > (1 << 24) || k < 1 || k > 8) return p;
    if (H < MD_MIN_N || H > MD_MAX_N || W < MD_MIN_N || W > MD_MAX_N) return p;
    p.hp = (H + k - 1) / k;
    p.wp = (W + k - 1) / k;
    p.tiles = ((p.hp + MD_CT - 1) / MD_CT) * ((p.wp + MD_CT - 1) / MD_CT);
    const long long per_image = (long long)na * (p.tiles * 16LL + 16);
    const long long Bc = p.Bc = each_chunk(MD_WS_TARGET, per_image, B);
    p.mean = 0;
    p.partial = p.mean + (long long)na * Bc * 16;
    p.bytes = p.partial + (long long)na * Bc * p.tiles * 16;
    p.ok = true;
    return p;
}

}  // namespace

extern "C" size_t mtd_mdsi_ws_bytes(int na, int B, int H, int W, int k) {
    const MdPlan p = mdsi_plan(na, B, H, W, k);
    return p.ok ? (size_t)p.bytes : 0;
}

extern "C" int mtd_mdsi_each(const void* const* srcs, int na, const void* target, int B, int H, int W, int k, const double* options, int mult,
                             double* out, double* parts, void* ws, void* stream) {
    if (!srcs || !target || !options || !out || !ws || (mult != 0 && mult != 1)) return MTD_EINVAL;
    const MdPlan p = mdsi_plan(na, B, H, W, k);
    if (!p.ok) return MTD_EINVAL;
    for (int j = 0; j < MTD_MDSI_OPTIONS; ++j)
        if (!each_finite(options[j])) return MTD_EINVAL;
    const MdOpts o = {options[0], options[1], options[2], options[3], options[4], options[5], options[6], options[7], options[8], mult};
    if (!(o.c1 > 0.0) || !(o.c2 > 0.0) || !(o.c3 > 0.0) || !(o.rho > 0.0)) return MTD_EINVAL;
    EachSets imgs = {};
    imgs.p[3] = (const float*)target;
    for (int a = 0; a < na; ++a) {
        if (!srcs[a]) return MTD_EINVAL;
        imgs.p[a] = (const float*)srcs[a];
    }
    hipStream_t s = (hipStream_t)stream;
    double* mean = (double*)((char*)ws + p.mean);
    double* partial = (double*)((char*)ws + p.partial);
    const dim3 grid((p.wp + MD_CT - 1) / MD_CT, (p.hp + MD_CT - 1) / MD_CT, 1);
    const double n = (double)p.hp * (double)p.wp;
    for (int i0 = 0; i0 < B; i0 += p.Bc) {
        const int Bc = (B - i0) < p.Bc ? (B - i0) : p.Bc;
        hipLaunchKernelGGL(mdsi_tile_kernel<1>, dim3(grid.x, grid.y, na * Bc), dim3(256), 0, s, imgs, Bc, i0, H, W, k, p.hp, p.wp, o,
                           (const double*)mean, partial);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(mdsi_finish_kernel<1>, dim3(na * Bc), dim3(256), 0, s, (const double*)partial, p.tiles, n, Bc, i0, B, o, mean, out, parts);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(mdsi_tile_kernel<2>, dim3(grid.x, grid.y, na * Bc), dim3(256), 0, s, imgs, Bc, i0, H, W, k, p.hp, p.wp, o,
                           (const double*)mean, partial);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(mdsi_finish_kernel<2>, dim3(na * Bc), dim3(256), 0, s, (const double*)partial, p.tiles, n, Bc, i0, B, o, mean, out, parts);
        MTD_LAUNCH_CHECK();
    }
    return MTD_OK;
}
