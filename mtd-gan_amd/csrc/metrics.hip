// Pixel metrics of the evaluation loops (reference metrics.py:172-244, used by engine.py:78-183): squared error (RMSE,
// PSNR) and SSIM with the 11x11 Gaussian window (sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2) of a batch of
// single-channel images, as sums over all pixels in double precision with a fixed-order reduction.
// HBM-bound: both images are read once (a 32x32 output tile loads a 42x42 halo of each into LDS; the Gaussian is applied
// separably to the five moment maps a, b, a^2, b^2, ab in LDS).  Algorithmic bytes: 8 per pixel.
#include "common.h"

namespace {

constexpr int MT = 32;            // output tile
constexpr int MR = 5;             // window radius
constexpr int MH = MT + 2 * MR;   // 42

// Up to three sources against one b, image by image: blockIdx.z = source * B + image.  The sources arrive by value (the
// selects below keep them in scalar registers).  One 32x32 tile per workgroup; its two sums go to partial[2 blk], blk the
// linear workgroup index, so a source's partials are contiguous, image after image.
struct EachSources { const float* a[3]; int clip[3]; };

__global__ __launch_bounds__(256) void image_metrics_each_kernel(EachSources src, const float* __restrict__ b, int B, int H, int W,
                                                                 double* __restrict__ partial) {
    __shared__ float As[MH * MH], Bs[MH * MH];
    __shared__ float Hs[5][MH * MT];
    __shared__ double red[2 * 256];
    const int si = blockIdx.z / B, i = blockIdx.z - si * B;
    const float* __restrict__ a = si == 0 ? src.a[0] : (si == 1 ? src.a[1] : src.a[2]);
    const int clip_a = si == 0 ? src.clip[0] : (si == 1 ? src.clip[1] : src.clip[2]);
    const long long img = (long long)i * H * W;
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * MT, ty0 = blockIdx.y * MT;
    float gw[11];
    {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) { gw[k] = expf(-(float)((k - 5) * (k - 5)) / 4.5f); s += gw[k]; }
#pragma unroll
        for (int k = 0; k < 11; ++k) gw[k] /= s;
    }
    for (int e = tid; e < MH * MH; e += 256) {
        const int ly = e / MH, lx = e - ly * MH;
        const int y = ty0 + ly - MR, x = tx0 + lx - MR;
        float va = 0.f, vb = 0.f;
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
            va = a[img + (long long)y * W + x];
            vb = b[img + (long long)y * W + x];
            if (clip_a) va = fminf(fmaxf(va, 0.f), 1.f);
        }
        As[e] = va;
        Bs[e] = vb;
    }
    __syncthreads();
    // horizontal pass: 42 rows x 32 columns, five moments
    for (int e = tid; e < MH * MT; e += 256) {
        const int ly = e / MT, lx = e - ly * MT;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float va = As[ly * MH + lx + k], vb = Bs[ly * MH + lx + k];
            m[0] = fmaf(gw[k], va, m[0]);
            m[1] = fmaf(gw[k], vb, m[1]);
            m[2] = fmaf(gw[k], va * va, m[2]);
            m[3] = fmaf(gw[k], vb * vb, m[3]);
            m[4] = fmaf(gw[k], va * vb, m[4]);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) Hs[q][e] = m[q];
    }
    __syncthreads();
    // Two scalars, not an array: which products of the SSIM expression below the compiler fuses into fmas follows how it
    // vectorises this loop, and with the sums in an array it chooses otherwise (the SSIM sum then moves by 1e-8 of itself).
    double sse = 0.0, ssum = 0.0;
    for (int e = tid; e < MT * MT; e += 256) {
        const int ly = e / MT, lx = e - ly * MT;
        const int y = ty0 + ly, x = tx0 + lx;
        if (y < H && x < W) {
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 11; ++k)
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(gw[k], Hs[q][(ly + k) * MT + lx], m[q]);
            const float mu1 = m[0], mu2 = m[1];
            const float s11 = m[2] - mu1 * mu1, s22 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
            const float c1 = 1e-4f, c2 = 9e-4f;
            const float v = ((2.f * mu1 * mu2 + c1) * (2.f * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2));
            ssum += (double)v;
            const float d = As[(ly + MR) * MH + lx + MR] - Bs[(ly + MR) * MH + lx + MR];
            sse += (double)d * (double)d;
        }
    }
    double sums[2] = {sse, ssum};
    block_sum256(sums, red);
    if (tid == 0) {
        partial[2 * blk] = sums[0];
        partial[2 * blk + 1] = sums[1];
    }
}

// One workgroup per group of `per_group` consecutive partials (gridDim.x groups): thread t takes t, t + 256, ... of the group's
// own numbering, then the tree.  A group is one (source, image) for mtd_image_metrics_each and the whole batch for
// mtd_image_metrics, so an image alone in a batch gets the same sums from either.
__global__ __launch_bounds__(256) void image_metrics_finish_kernel(const double* __restrict__ partial, long long per_group,
                                                                   double* __restrict__ out) {
    __shared__ double red[2 * 256];
    const double* p = partial + 2 * per_group * blockIdx.x;
    double sums[2] = {0.0, 0.0};
    for (long long i = threadIdx.x; i < per_group; i += 256) { sums[0] += p[2 * i]; sums[1] += p[2 * i + 1]; }
    block_sum256(sums, red);
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = sums[0]; out[2 * blockIdx.x + 1] = sums[1]; }
}

long long metric_blocks(int B, int H, int W) { return (long long)B * ((H + MT - 1) / MT) * ((W + MT - 1) / MT); }

// tiles of `na` sources x B images, then their partials summed in `groups` equal groups: out (groups, 2)
int metrics_launch(const EachSources& src, int na, const float* b, int B, int H, int W, int groups, double* out, void* ws, hipStream_t s) {
    const dim3 grid((W + MT - 1) / MT, (H + MT - 1) / MT, na * B);
    hipLaunchKernelGGL(image_metrics_each_kernel, grid, dim3(256), 0, s, src, b, B, H, W, (double*)ws);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(image_metrics_finish_kernel, dim3(groups), dim3(256), 0, s, (const double*)ws, metric_blocks(na * B, H, W) / groups, out);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

}  // namespace

extern "C" size_t mtd_image_metrics_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)metric_blocks(B, H, W) * 2 * sizeof(double);
}

extern "C" int mtd_image_metrics(const float* a, const float* b, int B, int H, int W, int clip_a, double* out2, void* ws, void* stream) {
    if (!a || !b || !out2 || !ws || B <= 0 || H <= 0 || W <= 0 || B > 65535) return MTD_EINVAL;
    // one source, and the whole batch as one group of the finish
    return metrics_launch(EachSources{{a, nullptr, nullptr}, {clip_a, 0, 0}}, 1, b, B, H, W, 1, out2, ws, (hipStream_t)stream);
}

extern "C" size_t mtd_image_metrics_each_ws_bytes(int na, int B, int H, int W) {
    if (na < 1 || na > 3 || B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)na * (size_t)metric_blocks(B, H, W) * 2 * sizeof(double);
}

extern "C" int mtd_image_metrics_each(const float* const a[3], int na, const float* b, int B, int H, int W, const int clip_a[3],
                                      double* out, void* ws, void* stream) {
    if (!a || !clip_a || !b || !out || !ws || na < 1 || na > 3 || B <= 0 || H <= 0 || W <= 0 || (long long)na * B > 65535) return MTD_EINVAL;
    EachSources src;
    for (int k = 0; k < 3; ++k) {
        src.a[k] = k < na ? a[k] : nullptr;
        src.clip[k] = k < na ? clip_a[k] : 0;
        if (k < na && !a[k]) return MTD_EINVAL;
    }
    return metrics_launch(src, na, b, B, H, W, na * B, out, ws, (hipStream_t)stream);
}
