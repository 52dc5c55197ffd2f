// Device side of LPIPS and DISTS of the test loop (reference module/piq/perceptual.py): what the VGG-16 feature stack needs
// beside the 3x3 conv kernels and the 2x2 max-pool -- DISTS's L2 pooling -- and the two memory-bound reductions over the NHWC
// fp32 feature maps.  Every per-image number is formed in double, in a fixed order, in two stages (workgroup partials in a
// workspace, then a finish): no atomics, and image i of a batch has the bits of a one-image call.
//
//   l2pool3x3s2_kernel       sqrt(sum of the 3x3 Hann taps [[1,2,1],[2,4,2],[1,2,1]] / 16 of x^2 + 1e-12), stride 2, zero padding 1,
//                            ceil(H / 2) x ceil(W / 2) outputs; one float4 of channels per thread and round, row-major taps in fp32.
//                            HBM-bound: at most 9 reads + 1 write per output float4, the reads of neighbouring outputs overlap.
//   lpips_level_kernel       LP = min(C / 4, 64) lanes share a pixel, each with one (C <= 256) or two (C = 512) float4 of its
//                            channels in registers, so that a wave's load is 1 KiB of consecutive addresses; a wave takes
//                            64 / LP consecutive pixels per round.  The squared norms of the target's and the others' channel
//                            vectors are butterfly sums over the LP lanes (every lane ends with the same bits), the division
//                            is one reciprocal per pixel and map, and w_c d(o_c / |o|, t_c / |t|) is added to the lane's running
//                            double.  The target is loaded and normalised once for both others.
//   channel_moments_kernel   threads own a float4 of channels (or the one channel of a C = 1 map) and walk the pixels of the
//                            workgroup's range with a stride of PL = 256 / (C / 4) pixels; the PL pixel lanes meet in LDS.
//   *_finish_kernel          the fixed-order sums of the partials; dists_finish_kernel is the closing formula of DISTS.
#include "each_metric.h"     // each_fold

// No contraction of a * b - c into an fma: a map against itself must give exactly 0 (LPIPS) and exactly S = 1 (DISTS), which holds
// when both sides of a difference are rounded alike.  The fused forms that are wanted are written as fma / fmaf below.
#pragma clang fp contract(off)

namespace {

constexpr int POOL_THREADS = 256;

__global__ __launch_bounds__(POOL_THREADS) void l2pool3x3s2_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                                   int OH, int OW, int C4, long long total) {
    const long long step = (long long)gridDim.x * POOL_THREADS;
    for (long long e = (long long)blockIdx.x * POOL_THREADS + threadIdx.x; e < total; e += step) {
        const int c4 = (int)(e % C4);
        const long long opix = e / C4;                       // (b * OH + oy) * OW + ox
        const int ox = (int)(opix % OW);
        const long long t = opix / OW;
        const int oy = (int)(t % OH);
        const long long b = t / OH;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
                const float wt = (float)((ky == 1 ? 2 : 1) * (kx == 1 ? 2 : 1)) * 0.0625f;
                const f32x4 v = reinterpret_cast<const f32x4*>(in)[((b * H + iy) * W + ix) * C4 + c4];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = fmaf(wt, v[k] * v[k], acc[k]);
            }
        }
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = sqrtf(acc[k] + 1e-12f);
        reinterpret_cast<f32x4*>(out)[opix * C4 + c4] = r;
    }
}

// ---------------------------------------------------------------------------------------------- LPIPS level
constexpr int LP_BLOCKS = MTD_LPIPS_MAX_BLOCKS;

// sum over the LP lanes that share a pixel (LP a power of two, groups aligned): the xor butterfly, after which every lane of
// the group holds the same bits (each step adds the same two numbers in both partners)
template <int LP>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int m = 1; m < LP; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// V float4 per lane and map; LP lanes per pixel; C = 4 * V * LP
template <int V, int LP, bool MAE>
__global__ __launch_bounds__(256) void lpips_level_kernel(const float* __restrict__ T, const float* __restrict__ A, const float* __restrict__ Bm,
                                                          const double* __restrict__ wts, int hw, double* __restrict__ partial) {
    constexpr int PW = 64 / LP;                      // pixels per wave and round
    constexpr int C4 = V * LP;                       // float4 per pixel
    __shared__ double red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cl = lane % LP, pl = lane / LP;
    const long long img = (long long)blockIdx.y * hw;
    double wt[V][4];
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) wt[j][k] = wts[4 * (j * LP + cl) + k];
    double acc_a = 0.0, acc_b = 0.0;
    const int stride = gridDim.x * 4 * PW;
    for (int p0 = (blockIdx.x * 4 + wave) * PW; p0 < hw; p0 += stride) {       // (wave-uniform bound: the shuffles see all lanes)
        const int p = p0 + pl;
        const bool live = p < hw;
        f32x4 vt[V], va[V], vb[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const long long at = (img + p) * C4 + j * LP + cl;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            vt[j] = live ? reinterpret_cast<const f32x4*>(T)[at] : z;
            va[j] = live ? reinterpret_cast<const f32x4*>(A)[at] : z;
            vb[j] = (live && Bm) ? reinterpret_cast<const f32x4*>(Bm)[at] : z;
        }
        double st = 0.0, sa = 0.0, sb = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double t = (double)vt[j][k], a = (double)va[j][k], b = (double)vb[j][k];
                st = fma(t, t, st);
                sa = fma(a, a, sa);
                sb = fma(b, b, sb);
            }
        const double it = 1.0 / (sqrt(group_sum<LP>(st)) + 1e-10);
        const double ia = 1.0 / (sqrt(group_sum<LP>(sa)) + 1e-10);
        const double ib = 1.0 / (sqrt(group_sum<LP>(sb)) + 1e-10);
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double t = (double)vt[j][k] * it;
                const double da = (double)va[j][k] * ia - t, db = (double)vb[j][k] * ib - t;
                acc_a = fma(wt[j][k], MAE ? fabs(da) : da * da, acc_a);
                acc_b = fma(wt[j][k], MAE ? fabs(db) : db * db, acc_b);
            }
    }
    acc_a = group_sum<64>(acc_a);
    acc_b = group_sum<64>(acc_b);
    if (lane == 0) {
        red[0][wave] = acc_a;
        red[1][wave] = acc_b;
    }
    __syncthreads();
    if (tid < 2) {
        const double s = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        if (tid == 0 || Bm) partial[((long long)tid * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
    }
}

// One workgroup per (other, image): its nblk partials in a fixed order (thread t takes t, t + 256, ..., then the tree).
__global__ __launch_bounds__(256) void lpips_level_finish_kernel(const double* __restrict__ partial, int nblk, int B, double* __restrict__ out,
                                                                 long long out_stride, long long other_stride) {
    __shared__ double red[256];
    const int i = blockIdx.x, k = blockIdx.y;
    double s[1];
    each_fold(partial + ((long long)k * B + i) * nblk, nblk, s, red);
    if (threadIdx.x == 0) out[k * other_stride + i * out_stride] = s[0];
}

int lpips_blocks(int hw, int C) {
    const int lp = C / 4 < 64 ? C / 4 : 64;
    const int per_block = 4 * (64 / lp);             // pixels of a workgroup's round
    const long long need = ((long long)hw + per_block - 1) / per_block;
    return (int)(need < LP_BLOCKS ? need : LP_BLOCKS);
}

bool lpips_shape_ok(int B, int h, int w, int C) {
    return B >= 1 && B <= 65535 && h >= 1 && w >= 1 && (long long)h * w < (1ll << 30) && (C == 64 || C == 128 || C == 256 || C == 512);
}

struct Scales8 { double s[MTD_SCALED_SUMS_MAX]; };

__global__ void scaled_sums_f64_kernel(const double* __restrict__ in, int groups, int per, Scales8 sc, double* __restrict__ out, double* __restrict__ parts) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    double s = 0.0;
    for (int i = 0; i < per; ++i) {
        const double v = sc.s[i] * in[g * per + i];
        if (parts) parts[g * per + i] = v;
        s += v;
    }
    out[g] = s;
}

// ---------------------------------------------------------------------------------------------- channel moments
constexpr int CM_MAX_RANGES = MTD_MOMENTS_MAX_RANGES;
constexpr int CM_WALK = MTD_MOMENTS_WALK;            // pixels a thread walks before another range is opened

struct CmPlan {
    bool ok;
    int vec, cg, pl, ranges, per_range, K;
};

CmPlan moments_plan(int B, int h, int w, int C, int n_others) {
    CmPlan p = {};
    if (B < 1 || B > 65535 || h < 1 || w < 1 || (long long)h * w >= (1ll << 30) || n_others < 1 || n_others > 2) return p;
    if (C != 1 && ((C & 3) || C < 4 || C > 1024)) return p;
    p.vec = C == 1 ? 1 : 4;
    p.cg = C / p.vec;                                // channel groups = threads along the channels
    p.pl = 256 / p.cg;                               // pixel lanes
    const long long hw = (long long)h * w, unit = (long long)p.pl * CM_WALK;
    long long r = (hw + unit - 1) / unit;
    p.ranges = (int)(r < CM_MAX_RANGES ? r : CM_MAX_RANGES);
    p.per_range = (int)((hw + p.ranges - 1) / p.ranges);
    p.K = 2 + 3 * n_others;
    p.ok = true;
    return p;
}

template <int VEC>
__device__ __forceinline__ void cm_load(const float* __restrict__ p, long long at, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const f32x4 q = reinterpret_cast<const f32x4*>(p)[at];
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
        v[0] = p[at];
    }
}

// grid (ranges, B).  partial: (B, ranges, K, C) doubles.
template <int VEC, int NO>
__global__ __launch_bounds__(256) void channel_moments_kernel(const float* __restrict__ T, const float* __restrict__ A, const float* __restrict__ Bm,
                                                              int hw, int cg, int pl_n, int per_range, double* __restrict__ partial) {
    constexpr int K = 2 + 3 * NO;
    __shared__ double red[256 * VEC];
    const int tid = threadIdx.x;
    const int g = tid % cg, pl = tid / cg;
    const bool live = pl < pl_n;
    const int r0 = blockIdx.x * per_range, r1 = min(hw, r0 + per_range);
    const long long img = (long long)blockIdx.y * hw;
    double acc[K][VEC];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < VEC; ++c) acc[k][c] = 0.0;
    if (live) {
        for (int p = r0 + pl; p < r1; p += pl_n) {
            const long long at = (img + p) * cg + g;
            float vt[VEC], va[VEC], vb[VEC];
            cm_load<VEC>(T, at, vt);
            cm_load<VEC>(A, at, va);
            if constexpr (NO == 2) cm_load<VEC>(Bm, at, vb);
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                const double t = (double)vt[c], a = (double)va[c];
                acc[0][c] += t;
                acc[1][c] = fma(t, t, acc[1][c]);    // (the product of two floats is exact in double, fused or not)
                acc[2][c] += a;
                acc[3][c] = fma(a, a, acc[3][c]);
                acc[4][c] = fma(a, t, acc[4][c]);
                if constexpr (NO == 2) {
                    const double b = (double)vb[c];
                    acc[5][c] += b;
                    acc[6][c] = fma(b, b, acc[6][c]);
                    acc[7][c] = fma(b, t, acc[7][c]);
                }
            }
        }
    }
    int top = 1;
    while (top < pl_n) top <<= 1;
    const int C = cg * VEC;
    double* dst = partial + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * K * C;
#pragma unroll
    for (int k = 0; k < K; ++k) {                    // (unrolled: acc stays in registers)
        __syncthreads();                             // the sums of the k before have been read
#pragma unroll
        for (int c = 0; c < VEC; ++c) red[tid * VEC + c] = acc[k][c];
        __syncthreads();
        for (int s = top >> 1; s > 0; s >>= 1) {     // halving tree over the pixel lanes: lane pl takes lane pl + s
            if (live && pl < s && pl + s < pl_n) {
#pragma unroll
                for (int c = 0; c < VEC; ++c) red[tid * VEC + c] += red[(tid + s * cg) * VEC + c];
            }
            __syncthreads();
        }
        if (pl == 0) {
#pragma unroll
            for (int c = 0; c < VEC; ++c) dst[(long long)k * C + g * VEC + c] = red[tid * VEC + c];
        }
    }
}

// out (B, C, K): thread per (image, k, channel) adds the ranges in index order
__global__ __launch_bounds__(256) void channel_moments_finish_kernel(const double* __restrict__ partial, int ranges, int K, int C, long long total,
                                                                     double* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const long long t = e / C;
    const int k = (int)(t % K);
    const long long b = t / K;
    const double* p = partial + (b * ranges * K + k) * C + c;
    double s = 0.0;
    for (int r = 0; r < ranges; ++r) s += p[(long long)r * K * C];
    out[(b * C + c) * K + k] = s;
}

// ---------------------------------------------------------------------------------------------- DISTS finish
struct DistsLevels {
    const double* table[MTD_DISTS_LEVELS];
    double n[MTD_DISTS_LEVELS];
};

__device__ const int DISTS_CH[MTD_DISTS_LEVELS] = {3, 64, 128, 256, 512, 512};      // weight channels (level 0's three read the one grey channel)

// grid (rows, B).  Row r reads other `r - (r > self_row)` of the tables; row self_row is the target against itself, whose S1 and
// S2 are exactly 1 in this arithmetic (numerator and denominator are the same expression of the same numbers).
__global__ __launch_bounds__(256) void dists_finish_kernel(DistsLevels lv, int n_others, int self_row, const double* __restrict__ alpha,
                                                           const double* __restrict__ beta, double* __restrict__ out, double* __restrict__ parts) {
    __shared__ double red[256];
    const int row = blockIdx.x, i = blockIdx.y, B = gridDim.y;
    const bool self = row == self_row;
    const int o = (self_row >= 0 && row > self_row) ? row - 1 : row;
    const int K = 2 + 3 * n_others;
    double total = 0.0;
    int w0 = 0;
#pragma unroll 1
    for (int l = 0; l < MTD_DISTS_LEVELS; ++l) {
        const int nc = DISTS_CH[l], Cm = l == 0 ? 1 : nc;
        const double n = lv.n[l];
        double s = 0.0;
        for (int c = threadIdx.x; c < nc; c += 256) {
            double s1 = 1.0, s2 = 1.0;
            if (!self) {
                const double* m = lv.table[l] + ((long long)i * Cm + (l == 0 ? 0 : c)) * K;
                const double mt = m[0] / n, mo = m[2 + 3 * o] / n;
                const double vt = m[1] / n - mt * mt, vo = m[3 + 3 * o] / n - mo * mo;
                const double cov = m[4 + 3 * o] / n - mo * mt;
                s1 = (2.0 * mo * mt + 1e-6) / (mo * mo + mt * mt + 1e-6);
                s2 = (2.0 * cov + 1e-6) / (vo + vt + 1e-6);
            }
            s += alpha[w0 + c] * s1 + beta[w0 + c] * s2;
        }
        __syncthreads();                             // red of the level before has been read
        s = block_sum256(s, red);
        if (threadIdx.x == 0 && parts) parts[((long long)row * B + i) * MTD_DISTS_LEVELS + l] = s;
        total += s;
        w0 += nc;
    }
    if (threadIdx.x == 0) out[(long long)row * B + i] = 1.0 - total;
}

}  // namespace

extern "C" int mtd_l2pool3x3s2(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    if (!in || !out || B <= 0 || H < 1 || W < 1 || C <= 0 || (C & 3)) return MTD_EINVAL;
    if (!aligned16(in) || !aligned16(out)) return MTD_EALIGN;
    const int OH = (H + 1) / 2, OW = (W + 1) / 2, C4 = C / 4;
    const long long total = (long long)B * OH * OW * C4;
    long long blocks = (total + POOL_THREADS - 1) / POOL_THREADS;
    if (blocks > MTD_L2POOL_MAX_BLOCKS) blocks = MTD_L2POOL_MAX_BLOCKS;
    hipLaunchKernelGGL(l2pool3x3s2_kernel, dim3((unsigned)blocks), dim3(POOL_THREADS), 0, (hipStream_t)stream, in, out, H, W, OH, OW, C4, total);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" size_t mtd_lpips_level_ws_bytes(int B, int h, int w, int C) {
    if (!lpips_shape_ok(B, h, w, C)) return 0;
    return (size_t)2 * B * lpips_blocks(h * w, C) * sizeof(double);
}

extern "C" int mtd_lpips_level_each(const float* t, const float* a, const float* b, int B, int h, int w, int C, const double* weights,
                                    int distance, double* out, long long out_stride, long long other_stride, void* ws, void* stream) {
    if (!t || !a || !weights || !out || !ws || out_stride < 1 || !lpips_shape_ok(B, h, w, C)) return MTD_EINVAL;
    if (distance != MTD_LPIPS_MSE && distance != MTD_LPIPS_MAE) return MTD_EINVAL;
    if (!aligned16(t) || !aligned16(a) || (b && !aligned16(b))) return MTD_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int hw = h * w, nblk = lpips_blocks(hw, C);
    const dim3 grid(nblk, B);
    double* partial = (double*)ws;
    const bool mae = distance == MTD_LPIPS_MAE;
#define LPIPS_LAUNCH(V, LP)                                                                                                        \
    do {                                                                                                                           \
        if (mae) hipLaunchKernelGGL((lpips_level_kernel<V, LP, true>), grid, dim3(256), 0, s, t, a, b, weights, hw, partial);      \
        else hipLaunchKernelGGL((lpips_level_kernel<V, LP, false>), grid, dim3(256), 0, s, t, a, b, weights, hw, partial);         \
    } while (0)
    if (C == 64) LPIPS_LAUNCH(1, 16);
    else if (C == 128) LPIPS_LAUNCH(1, 32);
    else if (C == 256) LPIPS_LAUNCH(1, 64);
    else LPIPS_LAUNCH(2, 64);
#undef LPIPS_LAUNCH
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(lpips_level_finish_kernel, dim3(B, b ? 2 : 1), dim3(256), 0, s, (const double*)partial, nblk, B, out, out_stride, other_stride);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_scaled_sums_f64_f64(const double* in, int groups, int per, const double* scales_host, double* out, double* parts, void* stream) {
    if (!in || !scales_host || !out || groups <= 0 || per <= 0 || per > MTD_SCALED_SUMS_MAX) return MTD_EINVAL;
    Scales8 sc;
    for (int i = 0; i < MTD_SCALED_SUMS_MAX; ++i) sc.s[i] = i < per ? scales_host[i] : 0.0;
    hipLaunchKernelGGL(scaled_sums_f64_kernel, dim3((groups + 63) / 64), dim3(64), 0, (hipStream_t)stream, in, groups, per, sc, out, parts);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" size_t mtd_channel_moments_ws_bytes(int B, int h, int w, int C, int n_others) {
    const CmPlan p = moments_plan(B, h, w, C, n_others);
    return p.ok ? (size_t)B * p.ranges * p.K * C * sizeof(double) : 0;
}

extern "C" int mtd_channel_moments_each(const float* t, const float* a, const float* b, int B, int h, int w, int C, double* out, void* ws,
                                        void* stream) {
    if (!t || !a || !out || !ws) return MTD_EINVAL;
    const CmPlan p = moments_plan(B, h, w, C, b ? 2 : 1);
    if (!p.ok) return MTD_EINVAL;
    if (p.vec == 4 && (!aligned16(t) || !aligned16(a) || (b && !aligned16(b)))) return MTD_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int hw = h * w;
    const dim3 grid(p.ranges, B);
    double* partial = (double*)ws;
    if (p.vec == 4 && b) hipLaunchKernelGGL((channel_moments_kernel<4, 2>), grid, dim3(256), 0, s, t, a, b, hw, p.cg, p.pl, p.per_range, partial);
    else if (p.vec == 4) hipLaunchKernelGGL((channel_moments_kernel<4, 1>), grid, dim3(256), 0, s, t, a, b, hw, p.cg, p.pl, p.per_range, partial);
    else if (b) hipLaunchKernelGGL((channel_moments_kernel<1, 2>), grid, dim3(256), 0, s, t, a, b, hw, p.cg, p.pl, p.per_range, partial);
    else hipLaunchKernelGGL((channel_moments_kernel<1, 1>), grid, dim3(256), 0, s, t, a, b, hw, p.cg, p.pl, p.per_range, partial);
    MTD_LAUNCH_CHECK();
    const long long total = (long long)B * p.K * C;
    hipLaunchKernelGGL(channel_moments_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const double*)partial, p.ranges, p.K, C,
                       total, out);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_dists_finish(const double* const tables[MTD_DISTS_LEVELS], const long long pixels[MTD_DISTS_LEVELS], int n_others, int B,
                                int self_row, const double* alpha, const double* beta, double* out, double* parts, void* stream) {
    if (!tables || !pixels || !alpha || !beta || !out || n_others < 1 || n_others > 2 || B < 1 || B > 65535) return MTD_EINVAL;
    if (self_row < -1 || self_row > n_others) return MTD_EINVAL;
    DistsLevels lv;
    for (int l = 0; l < MTD_DISTS_LEVELS; ++l) {
        if (!tables[l] || pixels[l] < 1) return MTD_EINVAL;
        lv.table[l] = tables[l];
        lv.n[l] = (double)pixels[l];
    }
    const int rows = n_others + (self_row >= 0 ? 1 : 0);
    hipLaunchKernelGGL(dists_finish_kernel, dim3(rows, B), dim3(256), 0, (hipStream_t)stream, lv, n_others, self_row, alpha, beta, out, parts);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
