// Device side of the perceptual metrics of the test loop (reference metrics.py:43-168, used by engine.py:139-140): what the
// VGG-19 feature stack needs beside the 3x3 conv kernels -- the 2x2 max-pool -- and the texture-matching loss's hot part,
// the L1 distance between the per-patch Gram matrices of two feature maps.
//
//   maxpool2x2_kernel      NHWC fp32, kernel 2, stride 2, floor semantics (an odd last row / column is dropped), one float4 of
//                          channels per thread and round, 64-bit pixel indices.  HBM-bound: 4 reads + 1 write per output float4.
//   patch_gram_l1_kernel   a workgroup owns one 16x16 patch and one pair (ci, cj >= ci) of 64-channel tiles.  It stages the
//                          256 x 64 slabs of tile ci and tile cj in LDS, every element once, 64 pixels at a time (32 KiB per
//                          workgroup: four workgroups share a CU and one's loads run under another's MFMAs), as
//                          [32-channel half][pixel][32 channels] -- the 64 lanes of a v_mfma_f32_32x32x2_f32 operand
//                          (channel = lane & 31, pixel = 2 step + (lane >> 5)) then read 64 consecutive floats, conflict-free --
//                          and each of its four waves forms one 32 x 32 block of G = sum over the 256 pixels of f f^T in 128 MFMA
//                          steps, first for X, then, through the SAME loop body, for Y (so that X == Y gives exactly 0).
//                          |G(X) - G(Y)| is taken on the accumulators and summed in double; the Gram matrices never reach
//                          memory.  G is symmetric: off-diagonal tile pairs count twice.
//   *_finish_kernel        fixed-order sum of the per-workgroup partials in double (no floating-point atomics anywhere).
#include "common.h"

namespace {

constexpr int POOL_THREADS = 256;
constexpr int POOL_MAX_BLOCKS = MTD_MAXPOOL_MAX_BLOCKS;

__global__ __launch_bounds__(POOL_THREADS) void maxpool2x2_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                                  int OH, int OW, int C4, long long total) {
    const long long step = (long long)gridDim.x * POOL_THREADS;
    for (long long e = (long long)blockIdx.x * POOL_THREADS + threadIdx.x; e < total; e += step) {
        const int c4 = (int)(e % C4);
        const long long opix = e / C4;                       // (b * OH + oy) * OW + ox
        const int ox = (int)(opix % OW);
        const long long t = opix / OW;
        const int oy = (int)(t % OH);
        const long long b = t / OH;
        const long long ipix = (b * H + 2 * oy) * W + 2 * ox;
        const f32x4* p = reinterpret_cast<const f32x4*>(in) + ipix * C4 + c4;
        const f32x4 v00 = p[0], v01 = p[C4], v10 = p[(long long)W * C4], v11 = p[(long long)W * C4 + C4];
        f32x4 m;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // nn.MaxPool2d's scan: row-major over the window from -inf, a NaN wins (and the first of equal values stays)
            float r = -INFINITY;
            r = (v00[k] > r || v00[k] != v00[k]) ? v00[k] : r;
            r = (v01[k] > r || v01[k] != v01[k]) ? v01[k] : r;
            r = (v10[k] > r || v10[k] != v10[k]) ? v10[k] : r;
            r = (v11[k] > r || v11[k] != v11[k]) ? v11[k] : r;
            m[k] = r;
        }
        reinterpret_cast<f32x4*>(out)[opix * C4 + c4] = m;
    }
}

constexpr int GP = 16;                 // patch side
constexpr int GPIX = GP * GP;          // pixels per patch = K of the Gram product
constexpr int GT = 64;                 // channels per tile
constexpr int GCH = 64;                // pixels staged at a time: 2 x 16 KiB of LDS per workgroup, so four workgroups share a CU
constexpr int GSLAB = GCH * GT;        // floats per staged slab

// slab[half][pixel][32] <- F[pixels chunk * GCH .. + GCH - 1 of the patch][c0 .. c0 + 63]
__device__ __forceinline__ void stage_slab(float* __restrict__ slab, const float* __restrict__ F, long long pix0, int w, int C, int c0, int chunk) {
#pragma unroll
    for (int e = threadIdx.x; e < GCH * (GT / 4); e += 256) {
        const int local = e >> 4, pixel = chunk * GCH + local, c = (e & 15) * 4;
        const long long gp = pix0 + (long long)(pixel >> 4) * w + (pixel & 15);
        const f32x4 v = *reinterpret_cast<const f32x4*>(F + gp * C + c0 + c);
        *reinterpret_cast<f32x4*>(slab + (c >> 5) * (GCH * 32) + local * 32 + (c & 31)) = v;
    }
}

__global__ __launch_bounds__(256) void patch_gram_l1_kernel(const float* __restrict__ X, const float* __restrict__ Y, int h, int w, int C,
                                                            int ph, int pw, double* __restrict__ partial) {
    __shared__ float slabs[2 * GSLAB];               // tile ci, tile cj
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // tile pair: blockIdx.y counts (ci, cj) with cj >= ci row by row
    const int nt = C / GT;
    int ci = 0, left = blockIdx.y;
    while (left >= nt - ci) { left -= nt - ci; ++ci; }
    const int cj = ci + left;
    const bool diag = ci == cj;
    const int patch = blockIdx.x;
    const int px = patch % pw, t = patch / pw, py = t % ph;
    const long long b = t / ph;
    const long long pix0 = (b * h + (long long)py * GP) * w + (long long)px * GP;
    float* sa = slabs;
    float* sb = diag ? slabs : slabs + GSLAB;
    const float* pa = sa + (wave >> 1) * (GCH * 32) + lane;         // A operand: rows of the block = channels of tile ci
    const float* pb = sb + (wave & 1) * (GCH * 32) + lane;          // B operand: columns = channels of tile cj
    f32x16 gx;
    double sum = 0.0;
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {
        const float* F = which ? Y : X;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 1
        for (int chunk = 0; chunk < GPIX / GCH; ++chunk) {
            __syncthreads();                         // the slabs of the chunk before have been read
            stage_slab(sa, F, pix0, w, C, ci * GT, chunk);
            if (!diag) stage_slab(sb, F, pix0, w, C, cj * GT, chunk);
            __syncthreads();
#pragma unroll
            for (int s = 0; s < GCH / 2; ++s) acc = mfma32(pa[s * 64], pb[s * 64], acc);
        }
        if (which == 0) {
            gx = acc;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) sum += (double)fabsf(gx[r] - acc[r]);
        }
    }
    red[tid] = sum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = diag ? red[0] : 2.0 * red[0];
}

__global__ __launch_bounds__(256) void gram_l1_finish_kernel(const double* __restrict__ partial, long long nblk, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (long long i = threadIdx.x; i < nblk; i += 256) s += partial[i];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

// One workgroup per image.  The partials sit at pair * patches + patch with an image's P1 patches contiguous; image i's are
// walked in the linear order pair * P1 + p of a one-image call (thread = index mod 256, the same tree), so out[i * out_stride]
// has the bits gram_l1_finish_kernel gives that image alone.
__global__ __launch_bounds__(256) void gram_l1_each_finish_kernel(const double* __restrict__ partial, long long patches, int P1, int pairs,
                                                                  double* __restrict__ out, long long out_stride) {
    __shared__ double red[256];
    const double* p = partial + (long long)blockIdx.x * P1;
    const int n1 = pairs * P1;                       // below 2^31: checked by mtd_patch_gram_l1_each
    double s = 0.0;
    for (int i = threadIdx.x; i < n1; i += 256) {
        const int pair = i / P1, q = i - pair * P1;
        s += p[(long long)pair * patches + q];
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) out[(long long)blockIdx.x * out_stride] = s;
}

struct Scales { double s[MTD_SCALED_SUMS_MAX]; };

__global__ void scaled_sums_kernel(const double* __restrict__ in, int groups, int per, Scales sc, float* __restrict__ out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    double s = 0.0;
    for (int i = 0; i < per; ++i) s += sc.s[i] * in[g * per + i];
    out[g] = (float)s;
}

bool gram_shape_ok(int B, int h, int w, int C) {
    return B > 0 && h >= GP && w >= GP && (C == 64 || C == 128 || C == 256 || C == 512) &&
           (long long)B * (h / GP) * (w / GP) < (1ll << 31);
}
long long gram_patches(int B, int h, int w) { return (long long)B * (h / GP) * (w / GP); }
int gram_pairs(int C) { const int nt = C / GT; return nt * (nt + 1) / 2; }

}  // namespace

extern "C" int mtd_maxpool2x2(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    if (!in || !out || B <= 0 || H < 2 || W < 2 || C <= 0 || (C & 3)) return MTD_EINVAL;
    if (!aligned16(in) || !aligned16(out)) return MTD_EALIGN;
    const int OH = H / 2, OW = W / 2, C4 = C / 4;
    const long long total = (long long)B * OH * OW * C4;
    long long blocks = (total + POOL_THREADS - 1) / POOL_THREADS;
    if (blocks > POOL_MAX_BLOCKS) blocks = POOL_MAX_BLOCKS;
    hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)blocks), dim3(POOL_THREADS), 0, (hipStream_t)stream, in, out, H, W, OH, OW, C4, total);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" size_t mtd_patch_gram_l1_ws_bytes(int B, int h, int w, int C) {
    if (!gram_shape_ok(B, h, w, C)) return 0;
    return (size_t)gram_patches(B, h, w) * gram_pairs(C) * sizeof(double);
}

extern "C" int mtd_patch_gram_l1(const float* X, const float* Y, int B, int h, int w, int C, double* out, void* ws, void* stream) {
    if (!X || !Y || !out || !ws || !gram_shape_ok(B, h, w, C)) return MTD_EINVAL;
    if (!aligned16(X) || !aligned16(Y)) return MTD_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const long long patches = gram_patches(B, h, w);
    const int pairs = gram_pairs(C);
    hipLaunchKernelGGL(patch_gram_l1_kernel, dim3((unsigned)patches, (unsigned)pairs), dim3(256), 0, s, X, Y, h, w, C, h / GP, w / GP,
                       (double*)ws);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(gram_l1_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, patches * pairs, out);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_patch_gram_l1_each(const float* X, const float* Y, int B, int h, int w, int C, double* out, long long out_stride, void* ws,
                                      void* stream) {
    if (!X || !Y || !out || !ws || out_stride < 1 || !gram_shape_ok(B, h, w, C)) return MTD_EINVAL;
    const long long P1 = gram_patches(1, h, w);
    const int pairs = gram_pairs(C);
    if (P1 * pairs >= (1ll << 31)) return MTD_EINVAL;
    if (!aligned16(X) || !aligned16(Y)) return MTD_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const long long patches = gram_patches(B, h, w);
    hipLaunchKernelGGL(patch_gram_l1_kernel, dim3((unsigned)patches, (unsigned)pairs), dim3(256), 0, s, X, Y, h, w, C, h / GP, w / GP,
                       (double*)ws);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(gram_l1_each_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, (const double*)ws, patches, (int)P1, pairs, out, out_stride);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_scaled_sums_f64(const double* in, int groups, int per, const double* scales_host, float* out, void* stream) {
    if (!in || !scales_host || !out || groups <= 0 || per <= 0 || per > MTD_SCALED_SUMS_MAX) return MTD_EINVAL;
    Scales sc;
    for (int i = 0; i < MTD_SCALED_SUMS_MAX; ++i) sc.s[i] = i < per ? scales_host[i] : 0.0;
    hipLaunchKernelGGL(scaled_sums_kernel, dim3((groups + 63) / 64), dim3(64), 0, (hipStream_t)stream, in, groups, per, sc, out);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
