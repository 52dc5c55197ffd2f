// The visual saliency-induced index of the test loop (the reference vendors it in module/piq: vsi.py) of single-channel fp32
// images in [0, 1], image by image, for up to three sources a[k] against one target b (the convention of mtd_fsim_each and
// mtd_haarpsi_each).  DESIGN 3.19.  piq runs a single-channel image as three equal colour channels.
//   * the saliency map (SDSP) of an image is a log-Gabor band-pass of the three Lab channels of the image resampled to
//     256 x 256 -- forward and inverse 2-D FFTs as radix-2 passes over lines held in LDS (lds_fft.h), fp32 --, times a centre
//     prior and a colour prior, resampled back to H x W and stretched to [0, 1] by its own minimum and maximum;
//   * every DISTINCT image set is transformed once: a source whose pointer equals the target's (gt in the test loop) shares the
//     target's maps, and the target's maps serve all sources;
//   * the resampling, the Lab conversion, everything after the transforms and every per-image sum are double, the sums in a fixed
//     order (block_sum256's tree over a tile, the tiles of an image by one workgroup in the same way), no floating-point atomics:
//     an image's numbers depend neither on the batch it is in, nor on its source slot, nor on the other sources;
//   * the H x W saliency map is never stored: its minimum and maximum come from one pass over the resampled values, and the
//     combine stage resamples again with the same function (no contraction in this file: the same bits).
// Launches per chunk of the batch: resample + Lab + rows forward, columns (forward, filter, inverse), rows inverse + priors,
// minimum / maximum of the resampled map (tiles, then per image), combine, finish.
#include "each_metric.h"
#include "lds_fft.h"
#include <float.h>
#include <math.h>

#pragma clang fp contract(off)      // no fused multiply-adds: the same expression gives the same bits wherever it is inlined

namespace {

constexpr int VS_N = 256, VS_LN = 8;          // SDSP's working size: piq's size_to_use
constexpr int VS_NN = VS_N * VS_N;
constexpr int VS_LD = VS_N + 1;
constexpr int VS_RL = 4;                      // rows of a row tile: 3 channels x 4 rows of 256 points in LDS
constexpr int VS_RT = VS_N / VS_RL;           // row tiles of an image
constexpr int VS_CW = 16;                     // columns of a column tile: 16 lines of 256 points in LDS
constexpr int VS_UP = 4096;                   // resampled pixels of a minimum / maximum workgroup
constexpr int VS_CT = 16;                     // the combine tile: 16 x 16 pooled pixels, one per thread, with an 18 x 18 halo
constexpr int VS_HL = VS_CT + 2;
constexpr int VS_SUMS = 4;                    // num, den, sum of the source's pooled saliency, sum of its gradient map
constexpr int VS_MIN_N = MTD_VSI_MIN_SIDE, VS_MAX_N = MTD_VSI_MAX_SIDE;
constexpr long long VS_WS_TARGET = 64LL << 20;

struct VsOpts { double c1, c2, c3, alpha, beta, sigma_d, sigma_c; };

// Pixel (dy, dx) of 255 * image resampled to 256 x 256 as interpolate(mode='bilinear', align_corners=False) does it: source
// coordinate (d + 0.5) * in / 256 - 0.5 clamped at 0, two taps per axis, no antialiasing.
__device__ __forceinline__ double vs_resample(const float* __restrict__ img, int H, int W, int dy, int dx) {
    double fy = ((double)dy + 0.5) * ((double)H / (double)VS_N) - 0.5, fx = ((double)dx + 0.5) * ((double)W / (double)VS_N) - 0.5;
    fy = fy < 0.0 ? 0.0 : fy;
    fx = fx < 0.0 ? 0.0 : fx;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 > H - 1 ? H - 1 : y0;
    x0 = x0 > W - 1 ? W - 1 : x0;
    const int y1 = y0 + (y0 < H - 1), x1 = x0 + (x0 < W - 1);
    const double ly = fmin(fmax(fy - (double)y0, 0.0), 1.0), lx = fmin(fmax(fx - (double)x0, 0.0), 1.0);
    const float* r0 = img + (long long)y0 * W;
    const float* r1 = img + (long long)y1 * W;
    const double top = (1.0 - lx) * (255.0 * (double)r0[x0]) + lx * (255.0 * (double)r0[x1]);
    const double bot = (1.0 - lx) * (255.0 * (double)r1[x0]) + lx * (255.0 * (double)r1[x1]);
    return (1.0 - ly) * top + ly * bot;
}

// piq's rgb2lab of a grey value v in [0, 255]: the sRGB curve, the rows of the D65 matrix summed product by product, the division
// by the D50 / 2 degree white, the cube-root / kappa branch.  The matrix and the white are rounded to fp32, as piq holds them in
// a float64 run too.
__device__ __forceinline__ double vs_lab_f(double t) { return t > 0.008856 ? pow(t, 1.0 / 3.0) : (903.3 * t + 16.0) / 116.0; }
__device__ __forceinline__ void vs_lab(double v, double& L, double& a, double& b) {
    const double t = v / 255.0;
    const double lin = t <= 0.04045 ? t / 12.92 : pow((t + 0.055) / 1.055, 2.4);
    const double X = lin * (double)0.4124564f + lin * (double)0.3575761f + lin * (double)0.1804375f;
    const double Y = lin * (double)0.2126729f + lin * (double)0.7151522f + lin * (double)0.0721750f;
    const double Z = lin * (double)0.0193339f + lin * (double)0.1191920f + lin * (double)0.9503041f;
    const double fx = vs_lab_f(X / (double)0.9642119944211994f), fy = vs_lab_f(Y / 1.0), fz = vs_lab_f(Z / (double)0.8251882845188288f);
    L = 116.0 * fy - 16.0;
    a = 500.0 * fx - 500.0 * fy;
    b = 200.0 * fy - 200.0 * fz;
}

// Six running extremes (min L, max L, min a, max a, min b, max b, or fewer) of a workgroup through LDS; thread 0 has them.
template <int N>
__device__ __forceinline__ void vs_block_extremes(double (&v)[N], double* red) {
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < N; ++q) red[q * 256 + t] = v[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const double u = red[q * 256 + t], w = red[q * 256 + t + s];
                red[q * 256 + t] = (q & 1) ? fmax(u, w) : fmin(u, w);          // even entries are minima, odd ones maxima
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = red[q * 256];
}

// ---- 1. resample + Lab + forward rows of the three channels.  grid (VS_RT, sets * Bc); slot = set * Bc + image of the chunk.
// spec: (slot, channel, 256, 256) complex; ab: (slot, 2, 256, 256) doubles; ext: (slot, VS_RT, 6) the tile's extremes.
__global__ __launch_bounds__(256) void vsi_rows_fwd_kernel(EachSets imgs, int Bc, int i0, int H, int W, float2* __restrict__ spec,
                                                           double* __restrict__ ab, double* __restrict__ ext) {
    __shared__ float2 buf[3 * VS_RL * VS_LD];
    __shared__ float2 tw[256];
    __shared__ double red[6 * 256];
    const int slot = blockIdx.y, set = slot / Bc, i = slot - set * Bc;
    const float* __restrict__ img = each_pick(imgs, set) + (long long)(i0 + i) * H * W;
    const int y0 = blockIdx.x * VS_RL;
    fs_twiddles(tw, VS_N);
    double ex[6] = {DBL_MAX, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX, -DBL_MAX};
    for (int e = threadIdx.x; e < VS_RL * VS_N; e += 256) {
        const int r = e >> VS_LN, x = e & (VS_N - 1);
        double L, a, b;
        vs_lab(vs_resample(img, H, W, y0 + r, x), L, a, b);
        const long long at = (long long)(y0 + r) * VS_N + x;
        ab[((long long)slot * 2 + 0) * VS_NN + at] = a;
        ab[((long long)slot * 2 + 1) * VS_NN + at] = b;
        const int j = fs_brev(x, VS_LN);
        buf[(0 * VS_RL + r) * VS_LD + j] = make_float2((float)L, 0.f);
        buf[(1 * VS_RL + r) * VS_LD + j] = make_float2((float)a, 0.f);
        buf[(2 * VS_RL + r) * VS_LD + j] = make_float2((float)b, 0.f);
        ex[0] = fmin(ex[0], L);
        ex[1] = fmax(ex[1], L);
        ex[2] = fmin(ex[2], a);
        ex[3] = fmax(ex[3], a);
        ex[4] = fmin(ex[4], b);
        ex[5] = fmax(ex[5], b);
    }
    __syncthreads();
    fs_lds_fft<-1>(buf, 3 * VS_RL, VS_LN, VS_LD, tw);
    for (int e = threadIdx.x; e < 3 * VS_RL * VS_N; e += 256) {
        const int line = e >> VS_LN, x = e & (VS_N - 1);
        const int ch = line / VS_RL, r = line - ch * VS_RL;
        spec[(((long long)slot * 3 + ch) * VS_N + y0 + r) * VS_N + x] = buf[line * VS_LD + x];
    }
    vs_block_extremes(ex, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) ext[((long long)slot * VS_RT + blockIdx.x) * 6 + q] = ex[q];
    }
}

// ---- 2. columns, in place: a workgroup owns VS_CW whole columns of one channel: forward transform, times the log-Gabor table
// (while the lines are put into bit-reversed order for the way back), inverse transform.  grid (256 / VS_CW, 3, slots).
__global__ __launch_bounds__(256) void vsi_cols_kernel(float2* spec, const float* __restrict__ lg) {
    __shared__ float2 buf[VS_CW * VS_LD];
    __shared__ float2 tw[256];
    const int x0 = blockIdx.x * VS_CW;
    float2* base = spec + ((long long)blockIdx.z * 3 + blockIdx.y) * VS_NN + x0;
    fs_twiddles(tw, VS_N);
    for (int e = threadIdx.x; e < VS_CW * VS_N; e += 256) {
        const int r = e / VS_CW, c = e - r * VS_CW;
        buf[c * VS_LD + fs_brev(r, VS_LN)] = base[(long long)r * VS_N + c];
    }
    __syncthreads();
    fs_lds_fft<-1>(buf, VS_CW, VS_LN, VS_LD, tw);
    for (int e = threadIdx.x; e < VS_CW * VS_N; e += 256) {
        const int r = e / VS_CW, c = e - r * VS_CW;
        const int j = fs_brev(r, VS_LN);
        if (r <= j) {                                            // the pair (r, j) trades places, each times its own filter value
            const float gr = lg[r * VS_N + x0 + c], gj = lg[j * VS_N + x0 + c];
            const float2 u = buf[c * VS_LD + r], v = buf[c * VS_LD + j];
            buf[c * VS_LD + r] = make_float2(v.x * gj, v.y * gj);
            buf[c * VS_LD + j] = make_float2(u.x * gr, u.y * gr);
        }
    }
    __syncthreads();
    fs_lds_fft<1>(buf, VS_CW, VS_LN, VS_LD, tw);
    for (int e = threadIdx.x; e < VS_CW * VS_N; e += 256) {
        const int r = e / VS_CW, c = e - r * VS_CW;
        base[(long long)r * VS_N + c] = buf[c * VS_LD + r];
    }
}

// ---- 3. inverse rows of the three channels of a row tile, then vs_m = S_F S_D S_C at 256 x 256.  grid (VS_RT, slots).
__global__ __launch_bounds__(256) void vsi_rows_inv_kernel(const float2* __restrict__ spec, const double* __restrict__ ab,
                                                           const double* __restrict__ ext, VsOpts o, double* __restrict__ vsm) {
    __shared__ float2 buf[3 * VS_RL * VS_LD];
    __shared__ float2 tw[256];
    __shared__ double lim[4];                                    // min a, max a, min b, max b of the image
    const int slot = blockIdx.y, y0 = blockIdx.x * VS_RL;
    fs_twiddles(tw, VS_N);
    if (threadIdx.x < 4) {
        const int q = 2 + threadIdx.x;
        double v = ext[(long long)slot * VS_RT * 6 + q];
        for (int t = 1; t < VS_RT; ++t) {
            const double w = ext[((long long)slot * VS_RT + t) * 6 + q];
            v = (q & 1) ? fmax(v, w) : fmin(v, w);
        }
        lim[threadIdx.x] = v;
    }
    for (int e = threadIdx.x; e < 3 * VS_RL * VS_N; e += 256) {
        const int line = e >> VS_LN, x = e & (VS_N - 1);
        const int ch = line / VS_RL, r = line - ch * VS_RL;
        buf[line * VS_LD + fs_brev(x, VS_LN)] = spec[(((long long)slot * 3 + ch) * VS_N + y0 + r) * VS_N + x];
    }
    __syncthreads();
    fs_lds_fft<1>(buf, 3 * VS_RL, VS_LN, VS_LD, tw);
    const double inv = 1.0 / (double)VS_NN, eps = (double)FLT_EPSILON;
    for (int e = threadIdx.x; e < VS_RL * VS_N; e += 256) {
        const int r = e >> VS_LN, x = e & (VS_N - 1);
        const double fl = (double)buf[(0 * VS_RL + r) * VS_LD + x].x * inv, fa = (double)buf[(1 * VS_RL + r) * VS_LD + x].x * inv,
                     fb = (double)buf[(2 * VS_RL + r) * VS_LD + x].x * inv;
        const double s_f = sqrt(fl * fl + fa * fa + fb * fb);
        const double cy = (double)(y0 + r - VS_N / 2 + 1), cx = (double)(x - VS_N / 2 + 1);          // piq: grid * 256 + 1
        const double s_d = exp(-(cy * cy + cx * cx) / (o.sigma_d * o.sigma_d));
        const long long at = (long long)(y0 + r) * VS_N + x;
        const double na = (ab[((long long)slot * 2 + 0) * VS_NN + at] - lim[0]) / (lim[1] - lim[0] + eps);
        const double nb = (ab[((long long)slot * 2 + 1) * VS_NN + at] - lim[2]) / (lim[3] - lim[2] + eps);
        const double s_c = 1.0 - exp(-(na * na + nb * nb) / (o.sigma_c * o.sigma_c));
        vsm[(long long)slot * VS_NN + at] = s_f * s_d * s_c;
    }
}

// Pixel (y, x) of the 256 x 256 map resampled to H x W as interpolate(mode='bilinear', align_corners=True) does it.
__device__ __forceinline__ double vs_up(const double* __restrict__ m, int H, int W, int y, int x) {
    const double fy = (H > 1 ? (double)(VS_N - 1) / (double)(H - 1) : 0.0) * (double)y;
    const double fx = (W > 1 ? (double)(VS_N - 1) / (double)(W - 1) : 0.0) * (double)x;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 > VS_N - 1 ? VS_N - 1 : y0;
    x0 = x0 > VS_N - 1 ? VS_N - 1 : x0;
    const int y1 = y0 + (y0 < VS_N - 1), x1 = x0 + (x0 < VS_N - 1);
    const double ly = fmin(fmax(fy - (double)y0, 0.0), 1.0), lx = fmin(fmax(fx - (double)x0, 0.0), 1.0);
    const double top = (1.0 - lx) * m[y0 * VS_N + x0] + lx * m[y0 * VS_N + x1];
    const double bot = (1.0 - lx) * m[y1 * VS_N + x0] + lx * m[y1 * VS_N + x1];
    return (1.0 - ly) * top + ly * bot;
}

// ---- 4a. the extremes of VS_UP resampled pixels.  grid (ceil(H W / VS_UP), slots) -> ext2 (slot, blocks, 2).
__global__ __launch_bounds__(256) void vsi_up_extremes_kernel(const double* __restrict__ vsm, int H, int W, double* __restrict__ ext2) {
    __shared__ double red[2 * 256];
    const double* __restrict__ m = vsm + (long long)blockIdx.y * VS_NN;
    const int n = H * W;
    double ex[2] = {DBL_MAX, -DBL_MAX};
    for (int e = blockIdx.x * VS_UP + threadIdx.x; e < (blockIdx.x + 1) * VS_UP && e < n; e += 256) {
        const int y = e / W, x = e - y * W;
        const double v = vs_up(m, H, W, y, x);
        ex[0] = fmin(ex[0], v);
        ex[1] = fmax(ex[1], v);
    }
    vs_block_extremes(ex, red);
    if (threadIdx.x == 0) {
        ext2[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2] = ex[0];
        ext2[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2 + 1] = ex[1];
    }
}

// ---- 4b. one workgroup per slot: the extremes of its blocks (at most 256) -> lim2 (slot, 2).
__global__ __launch_bounds__(256) void vsi_up_limits_kernel(const double* __restrict__ ext2, int blocks, double* __restrict__ lim2) {
    __shared__ double red[2 * 256];
    double ex[2] = {DBL_MAX, -DBL_MAX};
    for (int t = threadIdx.x; t < blocks; t += 256) {
        ex[0] = fmin(ex[0], ext2[((long long)blockIdx.x * blocks + t) * 2]);
        ex[1] = fmax(ex[1], ext2[((long long)blockIdx.x * blocks + t) * 2 + 1]);
    }
    vs_block_extremes(ex, red);
    if (threadIdx.x == 0) {
        lim2[2 * blockIdx.x] = ex[0];
        lim2[2 * blockIdx.x + 1] = ex[1];
    }
}

// Pixel (y, x) of the pooled maps: piq pads [k / 2, (k - 1) / 2] in REPLICATE mode on each axis (k >= 2), then avg_pool2d with
// kernel and stride k (floor).  0 <= y < (H + k - 1) / k, likewise x.  -> the pooled 255 * image and the pooled saliency,
// stretched to [0, 1] by the map's own limits before the pooling.
__device__ __forceinline__ double vs_pooled_pixel(const float* __restrict__ img, int H, int W, int k, int y, int x) {
    if (k == 1) return 255.0 * (double)img[(long long)y * W + x];
    double s = 0.0;
    for (int dy = 0; dy < k; ++dy) {
        int yy = y * k - k / 2 + dy;
        yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
        for (int dx = 0; dx < k; ++dx) {
            int xx = x * k - k / 2 + dx;
            xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
            s += 255.0 * (double)img[(long long)yy * W + xx];
        }
    }
    return s / (double)(k * k);
}

__device__ __forceinline__ double vs_pooled_saliency(const double* __restrict__ m, double lo, double hi, int H, int W, int k, int y, int x) {
    const double eps = (double)FLT_EPSILON;
    if (k == 1) return (vs_up(m, H, W, y, x) - lo) / (hi - lo + eps);
    double s = 0.0;
    for (int dy = 0; dy < k; ++dy) {
        int yy = y * k - k / 2 + dy;
        yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
        for (int dx = 0; dx < k; ++dx) {
            int xx = x * k - k / 2 + dx;
            xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
            s += (vs_up(m, H, W, yy, xx) - lo) / (hi - lo + eps);
        }
    }
    return s / (double)(k * k);
}

__device__ __forceinline__ double vs_scharr(const double* P) {         // P: the pixel in the 18-wide halo tile
    const double a = P[-VS_HL - 1], b = P[-VS_HL], c = P[-VS_HL + 1], d = P[-1], f = P[1], g = P[VS_HL - 1], hh = P[VS_HL], i = P[VS_HL + 1];
    const double gx = (3.0 * (c - a) + 10.0 * (f - d) + 3.0 * (i - g)) / 16.0;
    const double gy = (3.0 * (g - a) + 10.0 * (hh - b) + 3.0 * (i - c)) / 16.0;
    return sqrt(gx * gx + gy * gy);
}

// ---- 5. combine.  grid (ceil(wp / 16), ceil(hp / 16), na * Bc); blockIdx.z = source * Bc + image of the chunk.
__global__ __launch_bounds__(256) void vsi_combine_kernel(EachSets imgs, EachMap map, int Bc, int i0, int H, int W, int k, int hp, int wp, VsOpts o,
                                                          const double* __restrict__ vsm, const double* __restrict__ lim2,
                                                          double* __restrict__ partial) {
    __shared__ double Pa[VS_HL * VS_HL], Pb[VS_HL * VS_HL], La[VS_HL * VS_HL], Lb[VS_HL * VS_HL];
    __shared__ double red[VS_SUMS * 256];
    const int s = blockIdx.z / Bc, i = blockIdx.z - s * Bc;
    const int sa_set = each_pick(map, s), sb_set = map.tgt;
    const float* __restrict__ a = each_pick(imgs, sa_set) + (long long)(i0 + i) * H * W;
    const float* __restrict__ b = each_pick(imgs, sb_set) + (long long)(i0 + i) * H * W;
    const long long sa = (long long)sa_set * Bc + i, sb = (long long)sb_set * Bc + i;
    const int tx0 = blockIdx.x * VS_CT, ty0 = blockIdx.y * VS_CT;
    // the row sums of piq's RGB -> LMN matrix, its entries rounded to fp32 as piq holds them, product by product
    const double l0 = (double)0.06f, l1 = (double)0.63f, l2 = (double)0.27f;
    const double m0 = (double)0.30f, m1 = (double)0.04f, m2 = (double)-0.35f;
    const double n0 = (double)0.34f, n1 = (double)-0.6f, n2 = (double)0.17f;
    for (int e = threadIdx.x; e < VS_HL * VS_HL; e += 256) {
        const int ly = e / VS_HL, lx = e - ly * VS_HL;
        const int y = ty0 + ly - 1, x = tx0 + lx - 1;
        double va = 0.0, vb = 0.0;                               // the gradient filters' zero padding
        if ((unsigned)y < (unsigned)hp && (unsigned)x < (unsigned)wp) {
            va = vs_pooled_pixel(a, H, W, k, y, x);
            vb = vs_pooled_pixel(b, H, W, k, y, x);
        }
        Pa[e] = va;
        Pb[e] = vb;
        La[e] = va * l0 + va * l1 + va * l2;
        Lb[e] = vb * l0 + vb * l1 + vb * l2;
    }
    __syncthreads();
    const int ly = threadIdx.x / VS_CT, lx = threadIdx.x - ly * VS_CT;
    double sums[VS_SUMS] = {0.0, 0.0, 0.0, 0.0};
    if (ty0 + ly < hp && tx0 + lx < wp) {
        const int c = (ly + 1) * VS_HL + lx + 1;
        const double va = vs_pooled_saliency(vsm + sa * VS_NN, lim2[2 * sa], lim2[2 * sa + 1], H, W, k, ty0 + ly, tx0 + lx);
        const double vb = vs_pooled_saliency(vsm + sb * VS_NN, lim2[2 * sb], lim2[2 * sb + 1], H, W, k, ty0 + ly, tx0 + lx);
        const double ga = vs_scharr(La + c), gb = vs_scharr(Lb + c);
        const double pa = Pa[c], pb = Pb[c];
        const double s_vs = each_similarity(va, vb, o.c1), s_gm = each_similarity(ga, gb, o.c2);
        const double s_m = each_similarity(pa * m0 + pa * m1 + pa * m2, pb * m0 + pb * m1 + pb * m2, o.c3);
        const double s_n = each_similarity(pa * n0 + pa * n1 + pa * n2, pb * n0 + pb * n1 + pb * n2, o.c3);
        const double s_c = s_m * s_n;
        const double s_c_pow = pow(fabs(s_c), o.beta) * cos(o.beta * atan2(0.0, s_c));          // the real part of the complex power
        const double vm = va > vb ? va : vb;
        sums[0] = s_vs * pow(s_gm, o.alpha) * s_c_pow * vm;
        sums[1] = vm;
        sums[2] = va;
        sums[3] = ga;
    }
    block_sum256(sums, red);
    each_store(partial, sums);
}

// ---- 6. one workgroup per (source, image of the chunk) g: the tile partials in a fixed order, then (num + eps) / (den + eps).
__global__ __launch_bounds__(256) void vsi_finish_kernel(const double* __restrict__ partial, int tiles, EachMap map, int Bc, int i0, int B,
                                                         const double* __restrict__ lim2, double* __restrict__ out, double* __restrict__ parts) {
    __shared__ double red[VS_SUMS * 256];
    const int g = blockIdx.x, s = g / Bc, i = g - s * Bc;
    double sums[VS_SUMS];
    each_fold(partial + (long long)VS_SUMS * g * tiles, tiles, sums, red);
    if (threadIdx.x != 0) return;
    const long long at = (long long)s * B + i0 + i;
    const double eps = (double)FLT_EPSILON;
    if (parts) {
        double* pp = parts + at * MTD_VSI_PARTS;
#pragma unroll
        for (int q = 0; q < VS_SUMS; ++q) pp[q] = sums[q];
        const long long slot = (long long)each_pick(map, s) * Bc + i;
        pp[VS_SUMS] = lim2[2 * slot];
        pp[VS_SUMS + 1] = lim2[2 * slot + 1];
    }
    out[at] = (sums[0] + eps) / (sums[1] + eps);
}

struct VsPlan {
    bool ok;
    int Bc, hp, wp, tiles, blocks;
    long long spec, ab, vsm, ext, ext2, lim2, partial, bytes;        // byte offsets into the workspace, and its size
};

// The workspace holds one chunk of Bc images of every set (na sources + the target: the pointers may all differ).  Per image of
// a chunk and set: the three spectra (24 * 65536 bytes), a and b (16 * 65536), vs_m (8 * 65536), the extremes of the row tiles
// and of the resampled blocks, the two limits; per image and source the tile partials.  Bc is the largest count for which that
// stays within 64 MiB (each_chunk).
VsPlan vsi_plan(int na, int B, int H, int W, int k) {
    VsPlan p = {};
    if (na < 1 || na > 3 || B < 1 || B > (1 << 24) || k < 1 || k > 8) return p;
    if (H < VS_MIN_N || H > VS_MAX_N || W < VS_MIN_N || W > VS_MAX_N) return p;
    p.hp = (H + k - 1) / k;
    p.wp = (W + k - 1) / k;
    p.tiles = ((p.hp + VS_CT - 1) / VS_CT) * ((p.wp + VS_CT - 1) / VS_CT);
    p.blocks = (H * W + VS_UP - 1) / VS_UP;
    const long long sets = na + 1;
    const long long per_slot = 48LL * VS_NN + VS_RT * 48LL + p.blocks * 16LL + 16;
    const long long per_image = sets * per_slot + (long long)na * p.tiles * VS_SUMS * 8;
    const long long Bc = p.Bc = each_chunk(VS_WS_TARGET, per_image, B);
    const long long slots = sets * Bc;
    p.spec = 0;
    p.ab = p.spec + slots * 24 * VS_NN;
    p.vsm = p.ab + slots * 16 * VS_NN;
    p.ext = p.vsm + slots * 8 * VS_NN;
    p.ext2 = p.ext + slots * VS_RT * 48;
    p.lim2 = p.ext2 + slots * p.blocks * 16;
    p.partial = p.lim2 + slots * 16;
    p.bytes = p.partial + (long long)na * Bc * p.tiles * VS_SUMS * 8;
    p.ok = true;
    return p;
}

}  // namespace

extern "C" size_t mtd_vsi_ws_bytes(int na, int B, int H, int W, int k) {
    const VsPlan p = vsi_plan(na, B, H, W, k);
    return p.ok ? (size_t)p.bytes : 0;
}

extern "C" int mtd_vsi_each(const void* const* srcs, int na, const void* target, int B, int H, int W, int k, const float* log_gabor,
                            const double* options, double* out, double* parts, void* ws, void* stream) {
    if (!srcs || !target || !log_gabor || !options || !out || !ws) return MTD_EINVAL;
    const VsPlan p = vsi_plan(na, B, H, W, k);
    if (!p.ok) return MTD_EINVAL;
    for (int j = 0; j < MTD_VSI_OPTIONS; ++j)
        if (!each_finite(options[j])) return MTD_EINVAL;
    const VsOpts o = {options[0], options[1], options[2], options[3], options[4], options[5], options[6]};
    if (!(o.c1 > 0.0) || !(o.c2 > 0.0) || !(o.c3 > 0.0) || o.sigma_d == 0.0 || o.sigma_c == 0.0) return MTD_EINVAL;
    EachSets imgs;
    EachMap map;
    const int sets = each_sets(srcs, na, target, imgs, map);
    if (sets < 0) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    float2* spec = (float2*)(base + p.spec);
    double* ab = (double*)(base + p.ab);
    double* vsm = (double*)(base + p.vsm);
    double* ext = (double*)(base + p.ext);
    double* ext2 = (double*)(base + p.ext2);
    double* lim2 = (double*)(base + p.lim2);
    double* partial = (double*)(base + p.partial);
    const dim3 tiles((p.wp + VS_CT - 1) / VS_CT, (p.hp + VS_CT - 1) / VS_CT, 1);
    for (int i0 = 0; i0 < B; i0 += p.Bc) {
        const int Bc = (B - i0) < p.Bc ? (B - i0) : p.Bc;
        const int slots = sets * Bc;
        hipLaunchKernelGGL(vsi_rows_fwd_kernel, dim3(VS_RT, slots), dim3(256), 0, s, imgs, Bc, i0, H, W, spec, ab, ext);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(vsi_cols_kernel, dim3(VS_N / VS_CW, 3, slots), dim3(256), 0, s, spec, log_gabor);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(vsi_rows_inv_kernel, dim3(VS_RT, slots), dim3(256), 0, s, (const float2*)spec, (const double*)ab, (const double*)ext, o, vsm);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(vsi_up_extremes_kernel, dim3(p.blocks, slots), dim3(256), 0, s, (const double*)vsm, H, W, ext2);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(vsi_up_limits_kernel, dim3(slots), dim3(256), 0, s, (const double*)ext2, p.blocks, lim2);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(vsi_combine_kernel, dim3(tiles.x, tiles.y, na * Bc), dim3(256), 0, s, imgs, map, Bc, i0, H, W, k, p.hp, p.wp, o,
                           (const double*)vsm, (const double*)lim2, partial);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(vsi_finish_kernel, dim3(na * Bc), dim3(256), 0, s, (const double*)partial, p.tiles, map, Bc, i0, B, (const double*)lim2, out,
                           parts);
        MTD_LAUNCH_CHECK();
    }
    return MTD_OK;
}
