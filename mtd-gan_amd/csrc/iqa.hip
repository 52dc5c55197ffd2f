// Full-reference image-quality metrics of the test loop beside PSNR / SSIM (the reference vendors them in module/piq): MS-SSIM
// (piq/ssim.py: multi_scale_ssim), VIFp (piq/vif.py: vif_p) and GMSD (piq/gmsd.py: gmsd) of single-channel fp32 images, image
// by image, for up to three sources a[k] against one target b (the convention of mtd_image_metrics_each).  DESIGN 3.14.
//   * filter arithmetic in fp32; every per-image sum in double with a fixed order (thread-strided, then block_sum256's tree; the
//     tile partials of an image are summed by one workgroup in the same way), no atomics: an image's numbers do not depend on
//     the batch it is in, nor on which source slot it sits in;
//   * the windows are VALID (no padding): a 32 x 32 tile of outputs loads a (32 + N - 1)^2 halo of both images into LDS and
//     applies the N-tap Gaussian separably to the five moment maps a, b, a^2, b^2, ab, as image_metrics_each_kernel does;
//   * the pyramids (MS-SSIM: four 2 x 2 average pools; VIFp: three filtered and subsampled levels) live in the caller's workspace.
// Launches per batch: MS-SSIM 1 pyramid + 5 levels + 1 finish, VIFp 3 levels down + 4 scales + 1 finish, GMSD 1 + 1 finish.
#include "each_metric.h"
#include <math.h>

namespace {

constexpr int IT = 32;                        // output tile of every kernel here
constexpr int MS_LEVELS = 5, MS_WIN = 11, VIF_SCALES = 4;
constexpr int PARTS = 20;                     // stage values per (source, image): 10 MS-SSIM, 8 VIFp, 2 GMSD

struct IqaWeights { float w[17]; };           // the 1-D window (by value: its reads are unrolled, the weights stay in scalar registers)

// ------------------------------------------------------------------------------------------------ MS-SSIM pyramid
// Level l (1..4) of piq's pyramid: replicate-pad level l-1 on the left and top by p[l] = max(h % 2, w % 2) of level l-1, then a
// 2 x 2 average pool with stride 2 (floor).  Every level is computed straight from level 0 with the additions of the level-by-
// level form in the same order (the scale by 0.25 is exact), so one launch builds all four levels of all images and the
// values have the bits of four successive pools.
struct MsDims { int h[MS_LEVELS], w[MS_LEVELS], p[MS_LEVELS]; long long off[MS_LEVELS]; };

template <int L>
__device__ __forceinline__ float ms_pool(const float* __restrict__ img, const MsDims& d, int y, int x) {
    if constexpr (L == 0) {
        return img[(long long)y * d.w[0] + x];
    } else {
        const int p = d.p[L];
        const int y1 = 2 * y - p + 1, x1 = 2 * x - p + 1;         // >= 0; y1 <= h[L-1] - 1 because h[L] = (h[L-1] + p) / 2
        const int y0 = max(y1 - 1, 0), x0 = max(x1 - 1, 0);       // the replicated row / column
        float s = ms_pool<L - 1>(img, d, y0, x0);
        s += ms_pool<L - 1>(img, d, y0, x1);
        s += ms_pool<L - 1>(img, d, y1, x0);
        s += ms_pool<L - 1>(img, d, y1, x1);
        return 0.25f * s;
    }
}

// grid (pixels of level 1 / 256, 4 levels, (na + 1) * B images); ws level l holds image z at off[l] + z * h[l] * w[l]
__global__ __launch_bounds__(256) void ms_pyramid_kernel(EachSets src, int B, MsDims d, float* __restrict__ ws) {
    const int l = blockIdx.y + 1;
    const int z = blockIdx.z, slot = z / B, i = z - slot * B;
    const int hw = d.h[l] * d.w[l];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= hw) return;
    const int y = e / d.w[l], x = e - y * d.w[l];
    const float* img = each_pick(src, slot) + (long long)i * d.h[0] * d.w[0];
    float v;
    if (l == 1) v = ms_pool<1>(img, d, y, x);
    else if (l == 2) v = ms_pool<2>(img, d, y, x);
    else if (l == 3) v = ms_pool<3>(img, d, y, x);
    else v = ms_pool<4>(img, d, y, x);
    ws[d.off[l] + (long long)z * hw + e] = v;
}

// ------------------------------------------------------------------------------------------------ VIFp levels
// Scale s > 1 of vif_p: the valid N x N Gaussian of that scale on the level before, every second row and column kept.
// out (slots * B, oh, ow), oh = (h - N + 2) / 2.  A thread per output; the taps come through the caches.
template <int N>
__global__ __launch_bounds__(256) void vif_down_kernel(EachSets src, int B, int h, int w, IqaWeights wt, float* __restrict__ out, int oh, int ow) {
    const int z = blockIdx.z, slot = z / B, i = z - slot * B;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= oh * ow) return;
    const int y = e / ow, x = e - y * ow;
    const float* img = each_pick(src, slot) + (long long)i * h * w + (long long)(2 * y) * w + 2 * x;      // rows 2y .. 2y + N - 1 <= h - 1
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < N; ++r) {
        float row = 0.f;
#pragma unroll
        for (int c = 0; c < N; ++c) row = fmaf(wt.w[c], img[r * w + c], row);
        acc = fmaf(wt.w[r], row, acc);
    }
    out[(long long)z * oh * ow + e] = acc;
}

// ------------------------------------------------------------------------------------------------ windowed moments
enum { IQA_SSIM = 0, IQA_VIF = 1 };

// One level of MS-SSIM (MODE IQA_SSIM: sums of the cs map and of the SSIM map) or one scale of VIFp (MODE IQA_VIF: sums of
// log10(1 + g^2 s_t / (s_v + sigma_n)) and of log10(1 + s_t / sigma_n)) over a 32 x 32 tile of the (h - N + 1) x (w - N + 1) map
// of valid N x N windows.  blockIdx.z = source * B + image; the two sums go to partial[2 blk], blk the linear workgroup index,
// so the partials of one (source, image) are contiguous.
template <int N, int MODE>
__global__ __launch_bounds__(256) void iqa_moments_kernel(EachSets src, const float* __restrict__ b, int B, int h, int w, IqaWeights wt,
                                                          float sigma_n, double* __restrict__ partial) {
    constexpr int HL = IT + N - 1;
    __shared__ float As[HL * HL], Bs[HL * HL];
    __shared__ float Hs[5][HL * IT];
    __shared__ double red[2 * 256];
    const int si = blockIdx.z / B, i = blockIdx.z - si * B;
    const float* __restrict__ a = each_pick(src, si);
    const long long img = (long long)i * h * w;
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * IT, ty0 = blockIdx.y * IT;
    const int oh = h - N + 1, ow = w - N + 1;
    for (int e = tid; e < HL * HL; e += 256) {
        const int ly = e / HL, lx = e - ly * HL;
        const int y = ty0 + ly, x = tx0 + lx;
        float va = 0.f, vb = 0.f;                    // (beyond the image: read only by outputs that are masked below)
        if (y < h && x < w) {
            va = a[img + (long long)y * w + x];
            vb = b[img + (long long)y * w + x];
        }
        As[e] = va;
        Bs[e] = vb;
    }
    __syncthreads();
    for (int e = tid; e < HL * IT; e += 256) {       // horizontal pass: HL rows x 32 columns, five moments
        const int ly = e / IT, lx = e - ly * IT;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float va = As[ly * HL + lx + k], vb = Bs[ly * HL + lx + k];
            m[0] = fmaf(wt.w[k], va, m[0]);
            m[1] = fmaf(wt.w[k], vb, m[1]);
            m[2] = fmaf(wt.w[k], va * va, m[2]);
            m[3] = fmaf(wt.w[k], vb * vb, m[3]);
            m[4] = fmaf(wt.w[k], va * vb, m[4]);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) Hs[q][e] = m[q];
    }
    __syncthreads();
    double s0 = 0.0, s1 = 0.0;
    for (int e = tid; e < IT * IT; e += 256) {
        const int ly = e / IT, lx = e - ly * IT;
        if (ty0 + ly < oh && tx0 + lx < ow) {
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < N; ++k)
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(wt.w[k], Hs[q][(ly + k) * IT + lx], m[q]);
            // The products are rounded on their own (no fma into the subtractions and sums that follow), as the reference's
            // tensors hold them: an image against itself then gives exactly 1 in both ratios of the SSIM expression.
            const float maa = __fmul_rn(m[0], m[0]), mbb = __fmul_rn(m[1], m[1]), mab = __fmul_rn(m[0], m[1]);
            const float saa = m[2] - maa, sbb = m[3] - mbb, sab = m[4] - mab;
            if (MODE == IQA_SSIM) {
                const float c1 = 1e-4f, c2 = 9e-4f;
                const float cs = (2.f * sab + c2) / (saa + sbb + c2);
                const float ss = ((2.f * mab + c1) / (maa + mbb + c1)) * cs;
                s0 += (double)cs;
                s1 += (double)ss;
            } else {
                // vif_p's corrections in its order; a is the prediction, b the target
                const float eps = 1e-8f;
                float st = fmaxf(sbb, 0.f);
                const float sp = fmaxf(saa, 0.f);
                float g = sab / (st + eps);
                float sv = sp - g * sab;
                if (!(st >= eps)) { g = 0.f; sv = sp; st = 0.f; }
                if (!(sp >= eps)) { g = 0.f; sv = 0.f; }
                if (!(g >= 0.f)) sv = sp;
                g = fmaxf(g, 0.f);
                if (!(sv > eps)) sv = eps;
                s0 += (double)log10f(1.f + (g * g) * st / (sv + sigma_n));
                s1 += (double)log10f(1.f + st / sigma_n);
            }
        }
    }
    double sums[2] = {s0, s1};
    block_sum256(sums, red);
    each_store(partial, sums);
}

// ------------------------------------------------------------------------------------------------ GMSD
// gmsd: zero-pad bottom and right by max(H % 2, W % 2), 2 x 2 average pool (hp x wp), Prewitt / 3 in x and y with zero padding 1,
// magnitude, GMS = (2 ma mb + t) / (ma^2 + mb^2 + t); per tile the sums of GMS and GMS^2.  A 32 x 32 tile of the pooled map
// keeps its 34 x 34 pooled halo of both images in LDS (the pool is taken on the way in: the input is read once, plus halo).
__device__ __forceinline__ float pooled(const float* __restrict__ img, int H, int W, int py, int px) {
    const int y0 = 2 * py, x0 = 2 * px;
    const bool yb = y0 + 1 < H, xb = x0 + 1 < W;                 // y0 < H and x0 < W hold for every pooled pixel
    const float* r0 = img + (long long)y0 * W + x0;
    float s = r0[0];
    s += xb ? r0[1] : 0.f;
    s += yb ? r0[W] : 0.f;
    s += (yb && xb) ? r0[W + 1] : 0.f;
    return 0.25f * s;
}

__global__ __launch_bounds__(256) void gmsd_kernel(EachSets src, const float* __restrict__ b, int B, int H, int W, int hp, int wp,
                                                   double* __restrict__ partial) {
    constexpr int PL = IT + 2;
    __shared__ float Pa[PL * PL], Pb[PL * PL];
    __shared__ double red[2 * 256];
    const int si = blockIdx.z / B, i = blockIdx.z - si * B;
    const float* __restrict__ a = each_pick(src, si) + (long long)i * H * W;
    const float* __restrict__ bi = b + (long long)i * H * W;
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * IT, ty0 = blockIdx.y * IT;
    for (int e = tid; e < PL * PL; e += 256) {
        const int ly = e / PL, lx = e - ly * PL;
        const int py = ty0 + ly - 1, px = tx0 + lx - 1;
        float va = 0.f, vb = 0.f;                                // the convolution's zero padding
        if ((unsigned)py < (unsigned)hp && (unsigned)px < (unsigned)wp) {
            va = pooled(a, H, W, py, px);
            vb = pooled(bi, H, W, py, px);
        }
        Pa[e] = va;
        Pb[e] = vb;
    }
    __syncthreads();
    const float third = 1.f / 3.f, t = 170.f / (255.f * 255.f);
    double s0 = 0.0, s1 = 0.0;
    for (int e = tid; e < IT * IT; e += 256) {
        const int ly = e / IT, lx = e - ly * IT;
        if (ty0 + ly < hp && tx0 + lx < wp) {
            float mag[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float* P = (q == 0 ? Pa : Pb) + ly * PL + lx;        // P[r * PL + c]: pooled (y - 1 + r, x - 1 + c)
                float gx = 0.f, gy = 0.f;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    gx = fmaf(-third, P[r * PL], gx);
                    gx = fmaf(third, P[r * PL + 2], gx);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) gy = fmaf(-third, P[c], gy);
#pragma unroll
                for (int c = 0; c < 3; ++c) gy = fmaf(third, P[2 * PL + c], gy);
                mag[q] = sqrtf(gx * gx + gy * gy);
            }
            // (products rounded on their own: equal magnitudes give exactly 1, so an image against itself scores exactly 0)
            const float gms = (2.f * __fmul_rn(mag[0], mag[1]) + t) / (__fmul_rn(mag[0], mag[0]) + __fmul_rn(mag[1], mag[1]) + t);
            s0 += (double)gms;
            s1 += (double)gms * (double)gms;
        }
    }
    double sums[2] = {s0, s1};
    block_sum256(sums, red);
    each_store(partial, sums);
}

// ------------------------------------------------------------------------------------------------ finish
// One workgroup per (source, image) g: per stage the image's tile partials in a fixed order (thread t takes tiles t, t + 256,
// ..., then the tree), then the closing formula in thread 0.
struct IqaFinish {
    int mode, stages;                         // 0 MS-SSIM, 1 VIFp, 2 GMSD
    long long off[MS_LEVELS];                 // doubles: stage s holds (na * B, tiles[s], 2)
    int tiles[MS_LEVELS];
    double count[MS_LEVELS];                  // pixels of the stage's map
};

__global__ __launch_bounds__(256) void iqa_finish_kernel(const double* __restrict__ partial, IqaFinish f, double* __restrict__ out,
                                                         double* __restrict__ parts) {
    __shared__ double red[2 * 256];
    const int g = blockIdx.x;
    double st[MS_LEVELS][2];
    for (int s = 0; s < f.stages; ++s) {
        double sums[2];
        each_fold(partial + f.off[s] + 2LL * g * f.tiles[s], f.tiles[s], sums, red);
        st[s][0] = sums[0];
        st[s][1] = sums[1];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double* pp = parts ? parts + (long long)g * PARTS : nullptr;
    if (f.mode == 0) {
        const double wl[MS_LEVELS] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};       // a float32 tensor in the reference
        double score = 1.0;
        for (int s = 0; s < MS_LEVELS; ++s) {
            const double cs = st[s][0] / f.count[s], ss = st[s][1] / f.count[s];
            if (pp) { pp[2 * s] = cs; pp[2 * s + 1] = ss; }
            const double v = s < MS_LEVELS - 1 ? cs : ss;
            score *= pow(v > 0.0 ? v : 0.0, wl[s]);
        }
        out[g] = score;
    } else if (f.mode == 1) {
        double num = 0.0, den = 0.0;
        for (int s = 0; s < VIF_SCALES; ++s) {
            if (pp) { pp[10 + 2 * s] = st[s][0]; pp[11 + 2 * s] = st[s][1]; }
            num += st[s][0];
            den += st[s][1];
        }
        out[g] = (num + 1e-8) / (den + 1e-8);
    } else {
        const double mean = st[0][0] / f.count[0];
        double var = st[0][1] / f.count[0] - mean * mean;
        var = var > 0.0 ? var : 0.0;
        if (pp) { pp[18] = mean; pp[19] = var; }
        out[g] = sqrt(var);
    }
}

// ------------------------------------------------------------------------------------------------ host side
int tiles_of(int oh, int ow) { return ((oh + IT - 1) / IT) * ((ow + IT - 1) / IT); }
int vif_window(int s) { return (1 << (4 - s)) + 1; }           // scale s = 0..3: 17, 9, 5, 3

// the normalised 2-D Gaussian of the reference is the outer product of this 1-D one
IqaWeights gaussian(int n, double sigma) {
    IqaWeights g = {};
    double e[17], sum = 0.0;
    for (int k = 0; k < n; ++k) { const double c = k - (n - 1) / 2.0; e[k] = exp(-c * c / (2.0 * sigma * sigma)); sum += e[k]; }
    for (int k = 0; k < n; ++k) g.w[k] = (float)(e[k] / sum);
    return g;
}

// Workspace: the doubles (tile partials: MS-SSIM levels, VIFp scales, GMSD) first, then the float pyramids.
struct IqaPlan {
    bool ok;
    MsDims ms;                                // off[] in floats from the start of the float region
    int vh[VIF_SCALES], vw[VIF_SCALES];
    long long voff[VIF_SCALES];               // floats; level 0 is the input
    long long ms_part[MS_LEVELS], vif_part[VIF_SCALES], gmsd_part;      // doubles
    int hp, wp;
    long long doubles, floats;
};

IqaPlan iqa_plan(int mask, int na, int B, int H, int W) {
    IqaPlan p = {};
    if (mask < 1 || mask > 7 || na < 1 || na > 3 || B <= 0 || H <= 0 || W <= 0 || (long long)(na + 1) * B > 65535) return p;
    if ((long long)H * W > (1LL << 30)) return p;             // pixel indices of one image stay in int
    const int side = H < W ? H : W;
    if (((mask & 1) && side < 161) || ((mask & 2) && side < 41) || ((mask & 4) && side < 2)) return p;
    const long long nimg = (long long)na * B, nall = (long long)(na + 1) * B;
    if (mask & 1) {
        p.ms.h[0] = H; p.ms.w[0] = W; p.ms.p[0] = 0;
        for (int l = 0; l < MS_LEVELS; ++l) {
            if (l > 0) {
                const int pad = (p.ms.h[l - 1] % 2) | (p.ms.w[l - 1] % 2);
                p.ms.p[l] = pad;
                p.ms.h[l] = (p.ms.h[l - 1] + pad) / 2;
                p.ms.w[l] = (p.ms.w[l - 1] + pad) / 2;
                p.ms.off[l] = p.floats;
                p.floats += nall * p.ms.h[l] * p.ms.w[l];
            }
            p.ms_part[l] = p.doubles;
            p.doubles += 2 * nimg * tiles_of(p.ms.h[l] - MS_WIN + 1, p.ms.w[l] - MS_WIN + 1);
        }
    }
    if (mask & 2) {
        p.vh[0] = H; p.vw[0] = W;
        for (int s = 0; s < VIF_SCALES; ++s) {
            const int n = vif_window(s);
            if (s > 0) {
                p.vh[s] = (p.vh[s - 1] - n + 2) / 2;
                p.vw[s] = (p.vw[s - 1] - n + 2) / 2;
                p.voff[s] = p.floats;
                p.floats += nall * p.vh[s] * p.vw[s];
            }
            p.vif_part[s] = p.doubles;
            p.doubles += 2 * nimg * tiles_of(p.vh[s] - n + 1, p.vw[s] - n + 1);
        }
    }
    if (mask & 4) {
        const int pad = (H % 2) | (W % 2);
        p.hp = (H + pad) / 2;
        p.wp = (W + pad) / 2;
        p.gmsd_part = p.doubles;
        p.doubles += 2 * nimg * tiles_of(p.hp, p.wp);
    }
    p.doubles = (p.doubles + 1) & ~1LL;                        // the float region starts 16-byte aligned
    p.ok = true;
    return p;
}

// the B-image blocks of the slots of a workspace level
EachSets level_slots(const float* base, int slots, long long per_slot) {
    EachSets s = {};
    for (int k = 0; k < slots; ++k) s.p[k] = base + k * per_slot;
    return s;
}

template <int N, int MODE>
int moments_launch(const EachSets& a, const float* b, int na, int B, int h, int w, const IqaWeights& wt, float sigma_n, double* partial,
                   hipStream_t s) {
    const dim3 grid((w - N + 1 + IT - 1) / IT, (h - N + 1 + IT - 1) / IT, na * B);
    hipLaunchKernelGGL((iqa_moments_kernel<N, MODE>), grid, dim3(256), 0, s, a, b, B, h, w, wt, sigma_n, partial);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

template <int N>
int down_launch(const EachSets& in, int slots, int B, int h, int w, const IqaWeights& wt, float* out, int oh, int ow, hipStream_t s) {
    const dim3 grid((oh * ow + 255) / 256, 1, slots * B);
    hipLaunchKernelGGL((vif_down_kernel<N>), grid, dim3(256), 0, s, in, B, h, w, wt, out, oh, ow);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

}  // namespace

extern "C" size_t mtd_iqa_ws_bytes(int which_mask, int na, int B, int H, int W) {
    const IqaPlan p = iqa_plan(which_mask, na, B, H, W);
    if (!p.ok) return 0;
    return (size_t)p.doubles * sizeof(double) + (size_t)p.floats * sizeof(float);
}

extern "C" int mtd_iqa_each(const float* const a[3], int na, const float* b, int B, int H, int W, int which_mask, float sigma_n_sq,
                            double* out, double* parts, void* ws, void* stream) {
    if (!a || !b || !out || !ws || !(sigma_n_sq > 0.f)) return MTD_EINVAL;
    const IqaPlan p = iqa_plan(which_mask, na, B, H, W);
    if (!p.ok) return MTD_EINVAL;
    for (int k = 0; k < na; ++k)
        if (!a[k]) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* dws = (double*)ws;
    float* fws = (float*)(dws + p.doubles);
    const int nimg = na * B;
    EachSets src = {}, all = {};               // the sources; the sources and the target behind them
    for (int k = 0; k < na; ++k) src.p[k] = all.p[k] = a[k];
    all.p[na] = b;
    int row = 0, rc;
    if (which_mask & 1) {
        const MsDims& d = p.ms;
        hipLaunchKernelGGL(ms_pyramid_kernel, dim3((d.h[1] * d.w[1] + 255) / 256, MS_LEVELS - 1, (na + 1) * B), dim3(256), 0, s, all, B, d, fws);
        MTD_LAUNCH_CHECK();
        const IqaWeights wt = gaussian(MS_WIN, 1.5);
        IqaFinish f = {};
        f.mode = 0;
        f.stages = MS_LEVELS;
        for (int l = 0; l < MS_LEVELS; ++l) {
            const long long per_slot = (long long)B * d.h[l] * d.w[l];
            const EachSets lv = l == 0 ? src : level_slots(fws + d.off[l], na, per_slot);
            const float* tb = l == 0 ? b : fws + d.off[l] + na * per_slot;
            if ((rc = moments_launch<MS_WIN, IQA_SSIM>(lv, tb, na, B, d.h[l], d.w[l], wt, 0.f, dws + p.ms_part[l], s)) != MTD_OK) return rc;
            f.off[l] = p.ms_part[l];
            f.tiles[l] = tiles_of(d.h[l] - MS_WIN + 1, d.w[l] - MS_WIN + 1);
            f.count[l] = (double)(d.h[l] - MS_WIN + 1) * (double)(d.w[l] - MS_WIN + 1);
        }
        hipLaunchKernelGGL(iqa_finish_kernel, dim3(nimg), dim3(256), 0, s, (const double*)dws, f, out + (long long)row * nimg, parts);
        MTD_LAUNCH_CHECK();
        ++row;
    }
    if (which_mask & 2) {
        IqaFinish f = {};
        f.mode = 1;
        f.stages = VIF_SCALES;
        for (int sc = 0; sc < VIF_SCALES; ++sc) {
            const int n = vif_window(sc), h = p.vh[sc], w = p.vw[sc];
            const IqaWeights wt = gaussian(n, n / 5.0);
            if (sc > 0) {
                const int ph = p.vh[sc - 1], pw = p.vw[sc - 1];
                const EachSets in = sc == 1 ? all : level_slots(fws + p.voff[sc - 1], na + 1, (long long)B * ph * pw);
                float* o = fws + p.voff[sc];
                rc = sc == 1 ? down_launch<9>(in, na + 1, B, ph, pw, wt, o, h, w, s)
                   : sc == 2 ? down_launch<5>(in, na + 1, B, ph, pw, wt, o, h, w, s)
                             : down_launch<3>(in, na + 1, B, ph, pw, wt, o, h, w, s);
                if (rc != MTD_OK) return rc;
            }
            const long long per_slot = (long long)B * h * w;
            const EachSets lv = sc == 0 ? src : level_slots(fws + p.voff[sc], na, per_slot);
            const float* tb = sc == 0 ? b : fws + p.voff[sc] + na * per_slot;
            double* part = dws + p.vif_part[sc];
            rc = sc == 0 ? moments_launch<17, IQA_VIF>(lv, tb, na, B, h, w, wt, sigma_n_sq, part, s)
               : sc == 1 ? moments_launch<9, IQA_VIF>(lv, tb, na, B, h, w, wt, sigma_n_sq, part, s)
               : sc == 2 ? moments_launch<5, IQA_VIF>(lv, tb, na, B, h, w, wt, sigma_n_sq, part, s)
                         : moments_launch<3, IQA_VIF>(lv, tb, na, B, h, w, wt, sigma_n_sq, part, s);
            if (rc != MTD_OK) return rc;
            f.off[sc] = p.vif_part[sc];
            f.tiles[sc] = tiles_of(h - n + 1, w - n + 1);
            f.count[sc] = (double)(h - n + 1) * (double)(w - n + 1);
        }
        hipLaunchKernelGGL(iqa_finish_kernel, dim3(nimg), dim3(256), 0, s, (const double*)dws, f, out + (long long)row * nimg, parts);
        MTD_LAUNCH_CHECK();
        ++row;
    }
    if (which_mask & 4) {
        const dim3 grid((p.wp + IT - 1) / IT, (p.hp + IT - 1) / IT, nimg);
        hipLaunchKernelGGL(gmsd_kernel, grid, dim3(256), 0, s, src, b, B, H, W, p.hp, p.wp, dws + p.gmsd_part);
        MTD_LAUNCH_CHECK();
        IqaFinish f = {};
        f.mode = 2;
        f.stages = 1;
        f.off[0] = p.gmsd_part;
        f.tiles[0] = tiles_of(p.hp, p.wp);
        f.count[0] = (double)p.hp * (double)p.wp;
        hipLaunchKernelGGL(iqa_finish_kernel, dim3(nimg), dim3(256), 0, s, (const double*)dws, f, out + (long long)row * nimg, parts);
        MTD_LAUNCH_CHECK();
        ++row;
    }
    return MTD_OK;
}
