// The two no-reference statistics of the test loop (the reference vendors them in module/piq: brisque.py, tv.py) of single-channel
// fp32 images in [0, 1], image by image, for up to three sources (no target: each image set on its own).  DESIGN 3.21.
//   * everything is double from the first operation on the fp32 pixels, and every per-image sum runs in a fixed order (a wave's 64
//     lanes by shuffles, the four waves of a workgroup and then the tiles of an image in index order), no floating-point atomics:
//     an image's numbers depend neither on the batch it is in, nor on its source slot, nor on the other sources;
//   * a source pointer that occurs twice is computed once and written to both slots;
//   * nothing is read back: where piq would assert (brisque.py:143,164-173) the slice's score and parts are NaN.
// BRISQUE, per chunk of the batch, three launches over both scales at once: the MSCN map n = (x - mu) / (std + 1) of 255 * image
// and of its nearest-neighbour half-size resample (gathered while loading) into the workspace; the 26 moments of n and of its four
// circularly shifted products per tile; one workgroup per image for the tile sums, the ten table look-ups (torch.argmin's first
// minimum), the 36 features, their range scaling and the SVR score.  TV: row-group partial sums, then one small finish.
#include "each_metric.h"
#include <math.h>

#pragma clang fp contract(off)      // products and sums rounded one by one, as the float64 tensor operations of piq round them

namespace {

constexpr int BQ_CT = 16;                                      // the tile: 16 x 16 pixels, one per thread
constexpr int BQ_MAXK = MTD_BRISQUE_MAX_KERNEL;
constexpr int BQ_HL = BQ_CT + BQ_MAXK - 1;                     // its side with the widest halo
constexpr int BQ_M = 26;                                       // moments per scale: n^2, |n|, then per shift six
constexpr int BQ_F = 18;                                       // features per scale
constexpr int BQ_MIN_N = MTD_BRISQUE_MIN_SIDE, BQ_MAX_N = MTD_BRISQUE_MAX_SIDE;
constexpr long long BQ_WS_TARGET = 64LL << 20;

struct BqSrcs {
    EachSets set;               // the distinct source pointers
    int nu;                     // how many
    int count[3];               // output slots of each
    int slot[3][3];
};

struct BqGeo { int H, W, h2, w2, tx0, ty0, tx1, ty1, tiles0, tiles1; float sy, sx; };

// Pixel (y, x) of scale `sc` of 255 * image.  Scale 1 is torch's `nearest` resample of the scaled image to (H / 2, W / 2): source
// index min(floor(dst * scale), size - 1) with scale = size / (size / 2) in fp32.
__device__ __forceinline__ double bq_pixel(const float* __restrict__ img, const BqGeo& g, int sc, int y, int x) {
    if (sc) {
        const int yy = (int)floorf((float)y * g.sy), xx = (int)floorf((float)x * g.sx);
        y = yy < g.H - 1 ? yy : g.H - 1;
        x = xx < g.W - 1 ? xx : g.W - 1;
    }
    return 255.0 * (double)img[(long long)y * g.W + x];
}

// Sums of N values per thread over the workgroup's 256 threads: lanes by shuffles (offsets 32 .. 1), then the four waves in order.
// The totals arrive in tot[0 .. N) (LDS) for every thread after the call's last barrier.
template <int N>
__device__ __forceinline__ void bq_block_sum(double (&v)[N], double* red, double* tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    }
    __syncthreads();                                            // (red and tot may still be read from a call before)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[wave * N + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < N) tot[threadIdx.x] = ((red[threadIdx.x] + red[N + threadIdx.x]) + red[2 * N + threadIdx.x]) + red[3 * N + threadIdx.x];
    __syncthreads();
}

// grid (tiles0 + tiles1, nu * Bc); blockIdx.y = source * Bc + image of the chunk.  maps: per (source, image) H * W doubles of
// scale 0, then h2 * w2 of scale 1.
__global__ __launch_bounds__(256) void brisque_mscn_kernel(BqSrcs srcs, int Bc, int i0, BqGeo g, int ks, const float* __restrict__ taps,
                                                           double* __restrict__ maps) {
    __shared__ double X[BQ_HL * BQ_HL];
    __shared__ double T[BQ_MAXK * BQ_MAXK];
    const int s = blockIdx.y / Bc, i = blockIdx.y - s * Bc;
    const float* __restrict__ img = each_pick(srcs.set, s) + (long long)(i0 + i) * g.H * g.W;
    const int sc = (int)blockIdx.x >= g.tiles0;
    const int tile = sc ? blockIdx.x - g.tiles0 : blockIdx.x;
    const int h = sc ? g.h2 : g.H, w = sc ? g.w2 : g.W, tx = sc ? g.tx1 : g.tx0;
    const int ty0 = (tile / tx) * BQ_CT, tx0 = (tile - (tile / tx) * tx) * BQ_CT;
    const int r = ks / 2, side = BQ_CT + 2 * r;
    for (int e = threadIdx.x; e < ks * ks; e += 256) T[e] = (double)taps[e];
    for (int e = threadIdx.x; e < side * side; e += 256) {
        const int ly = e / side, lx = e - ly * side;
        const int y = ty0 + ly - r, x = tx0 + lx - r;
        X[e] = ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) ? bq_pixel(img, g, sc, y, x) : 0.0;      // the filter's zero padding
    }
    __syncthreads();
    const int ly = threadIdx.x / BQ_CT, lx = threadIdx.x - ly * BQ_CT;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= h || x >= w) return;
    double mu = 0.0, sq = 0.0;
    for (int dy = 0; dy < ks; ++dy)
        for (int dx = 0; dx < ks; ++dx) {
            const double v = X[(ly + dy) * side + lx + dx], t = T[dy * ks + dx];
            mu += v * t;
            sq += (v * v) * t;
        }
    const double sd = sqrt(fabs(sq - mu * mu));
    double* __restrict__ out = maps + (long long)blockIdx.y * ((long long)g.H * g.W + (long long)g.h2 * g.w2) + (sc ? (long long)g.H * g.W : 0);
    out[(long long)y * w + x] = (X[(ly + r) * side + lx + r] - mu) / (sd + 1.0);
}

// The same grid.  partial: per (source, image) and tile BQ_M doubles: the sums of n^2 and |n|, then for the product p of n with
// torch.roll(n, shift), shift = (0, 1), (1, 0), (1, 1), (-1, 1) over (rows, columns) -- roll is circular, roll(n, s)[y] = n[y - s]
// -- the count of p < 0, of p > 0, the sums of p^2 over the negatives and over the positives, of |p| and of p^2.
__global__ __launch_bounds__(256) void brisque_moment_kernel(int Bc, BqGeo g, const double* __restrict__ maps, double* __restrict__ partial) {
    __shared__ double red[4 * BQ_M], tot[BQ_M];
    const int sc = (int)blockIdx.x >= g.tiles0;
    const int tile = sc ? blockIdx.x - g.tiles0 : blockIdx.x;
    const int h = sc ? g.h2 : g.H, w = sc ? g.w2 : g.W, tx = sc ? g.tx1 : g.tx0;
    const int ty0 = (tile / tx) * BQ_CT, tx0 = (tile - (tile / tx) * tx) * BQ_CT;
    const double* __restrict__ n = maps + (long long)blockIdx.y * ((long long)g.H * g.W + (long long)g.h2 * g.w2) + (sc ? (long long)g.H * g.W : 0);
    const int ly = threadIdx.x / BQ_CT, lx = threadIdx.x - ly * BQ_CT;
    const int y = ty0 + ly, x = tx0 + lx;
    double v[BQ_M];
#pragma unroll
    for (int k = 0; k < BQ_M; ++k) v[k] = 0.0;
    if (y < h && x < w) {
        const int yu = y == 0 ? h - 1 : y - 1, yd = y == h - 1 ? 0 : y + 1, xl = x == 0 ? w - 1 : x - 1;
        const double c = n[(long long)y * w + x];
        const double nb[4] = {n[(long long)y * w + xl], n[(long long)yu * w + x], n[(long long)yu * w + xl], n[(long long)yd * w + xl]};
        v[0] = c * c;
        v[1] = fabs(c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double p = c * nb[j], pp = p * p;
            v[2 + 6 * j] = p < 0.0 ? 1.0 : 0.0;
            v[3 + 6 * j] = p > 0.0 ? 1.0 : 0.0;
            v[4 + 6 * j] = p < 0.0 ? pp : 0.0;
            v[5 + 6 * j] = p > 0.0 ? pp : 0.0;
            v[6 + 6 * j] = fabs(p);
            v[7 + 6 * j] = pp;
        }
    }
    bq_block_sum(v, red, tot);
    if (threadIdx.x < BQ_M)
        partial[((long long)blockIdx.y * (g.tiles0 + g.tiles1) + blockIdx.x) * BQ_M + threadIdx.x] = tot[threadIdx.x];
}

// The feature ranges of _scale_features (the MATLAB implementation's), which piq holds as a float32 tensor in a float64 run too.
__device__ const float BQ_RANGES[2 * BQ_F][2] = {
    {0.338f, 10.f}, {0.017204f, 0.806612f}, {0.236f, 1.642f}, {-0.123884f, 0.20293f}, {0.000155f, 0.712298f}, {0.001122f, 0.470257f},
    {0.244f, 1.641f}, {-0.123586f, 0.179083f}, {0.000152f, 0.710456f}, {0.000975f, 0.470984f}, {0.249f, 1.555f}, {-0.135687f, 0.100858f},
    {0.000174f, 0.684173f}, {0.000913f, 0.534174f}, {0.258f, 1.561f}, {-0.143408f, 0.100486f}, {0.000179f, 0.685696f}, {0.000888f, 0.536508f},
    {0.471f, 3.264f}, {0.012809f, 0.703171f}, {0.218f, 1.046f}, {-0.094876f, 0.187459f}, {1.5e-005f, 0.442057f}, {0.001272f, 0.40803f},
    {0.222f, 1.042f}, {-0.115772f, 0.162604f}, {1.6e-005f, 0.444362f}, {0.001374f, 0.40243f}, {0.227f, 0.996f},
    {-0.117188f, 0.09832299999999999f}, {3e-005f, 0.531903f}, {0.001122f, 0.369589f}, {0.228f, 0.99f}, {-0.12243f, 0.098658f},
    {2.8e-005f, 0.530092f}, {0.001118f, 0.370399f}};

// One workgroup per (distinct source, image of the chunk).  tables: gamma, the GGD r_table, the AGGD r_table, nt doubles each.
// weights: (n_sv, 37) doubles, the coefficient and then the support vector.
__global__ __launch_bounds__(256) void brisque_finish_kernel(BqSrcs srcs, int Bc, int i0, int B, BqGeo g, const double* __restrict__ partial,
                                                             const double* __restrict__ tables, int nt, const double* __restrict__ weights,
                                                             int n_sv, double* __restrict__ out, double* __restrict__ parts) {
    __shared__ double red[4 * BQ_M], tot[BQ_M];
    __shared__ double S[2 * BQ_M];               // the moments of both scales
    __shared__ double V[10];                     // the look-up values: per scale rho, then the four ro_hat_norm
    __shared__ double bd[10 * 256];
    __shared__ int bi[10 * 256];
    __shared__ double F[2 * BQ_F], Fs[2 * BQ_F];
    __shared__ int bad;
    const int t = threadIdx.x;
    const int s = blockIdx.x / Bc, i = blockIdx.x - s * Bc;
    const double* p = partial + (long long)blockIdx.x * (g.tiles0 + g.tiles1) * BQ_M;
    for (int sc = 0; sc < 2; ++sc) {
        const int first = sc ? g.tiles0 : 0, count = sc ? g.tiles1 : g.tiles0;
        double v[BQ_M];
#pragma unroll
        for (int k = 0; k < BQ_M; ++k) v[k] = 0.0;
        for (int tile = t; tile < count; tile += 256) {
#pragma unroll
            for (int k = 0; k < BQ_M; ++k) v[k] += p[(long long)(first + tile) * BQ_M + k];
        }
        bq_block_sum(v, red, tot);
        if (t < BQ_M) S[sc * BQ_M + t] = tot[t];
    }
    if (t == 0) bad = 0;
    __syncthreads();
    if (t < 10) {
        const int sc = t / 5, j = t - 5 * sc;
        const double* m = S + sc * BQ_M;
        const double npix = sc ? (double)g.h2 * (double)g.w2 : (double)g.H * (double)g.W;
        double val;
        bool fail;
        if (j == 0) {
            const double sigma_sq = m[0] / npix, e = m[1] / npix;
            fail = !(sqrt(sigma_sq) > 1e-8);                        // torch.isclose(sigma, 0): atol 1e-8
            val = sigma_sq / (e * e);
        } else {
            const double* q = m + 2 + 6 * (j - 1);
            const double sl = sqrt(q[2] / q[0]), sr = sqrt(q[3] / q[1]);
            fail = !(q[0] > 0.0) || !(q[1] > 0.0) || !(sl > 0.0) || !(sr > 0.0);
            const double gh = sl / sr, ea = q[4] / npix;
            const double ro = (ea * ea) / (q[5] / npix), g2 = gh * gh + 1.0;
            val = (ro * (gh * gh * gh + 1.0) * (gh + 1.0)) / (g2 * g2);
        }
        V[t] = val;
        if (fail || !(val == val)) atomicOr(&bad, 1);
    }
    __syncthreads();
    // the first index of the smallest |value - r_table|: each thread the first among its own, then pairs by (distance, index)
#pragma unroll 1
    for (int k = 0; k < 10; ++k) {
        const double* tab = tables + (long long)((k % 5) == 0 ? 1 : 2) * nt;
        const double val = V[k];
        double best = INFINITY;
        int at = nt;
        for (int j = t; j < nt; j += 256) {
            const double d = fabs(val - tab[j]);
            if (d < best) {
                best = d;
                at = j;
            }
        }
        bd[k * 256 + t] = best;
        bi[k * 256 + t] = at;
    }
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (t < half) {
#pragma unroll 1
            for (int k = 0; k < 10; ++k) {
                const double a = bd[k * 256 + t], b = bd[k * 256 + t + half];
                const int ia = bi[k * 256 + t], ib = bi[k * 256 + t + half];
                if (b < a || (b == a && ib < ia)) {
                    bd[k * 256 + t] = b;
                    bi[k * 256 + t] = ib;
                }
            }
        }
        __syncthreads();
    }
    if (t < 10) {
        const int sc = t / 5, j = t - 5 * sc;
        const double* m = S + sc * BQ_M;
        const double npix = sc ? (double)g.h2 * (double)g.w2 : (double)g.H * (double)g.W;
        const int at = bi[t * 256] < nt ? bi[t * 256] : 0;
        const double alpha = tables[at];
        double* f = F + sc * BQ_F;
        if (j == 0) {
            const double sigma = sqrt(m[0] / npix);
            f[0] = alpha;
            f[1] = sigma * sigma;
        } else {
            const double* q = m + 2 + 6 * (j - 1);
            const double sl = sqrt(q[2] / q[0]), sr = sqrt(q[3] / q[1]);
            f += 2 + 4 * (j - 1);
            f[0] = alpha;
            f[1] = (sr - sl) * exp(lgamma(2.0 / alpha) - (lgamma(1.0 / alpha) + lgamma(3.0 / alpha)) / 2.0);
            f[2] = sl * sl;
            f[3] = sr * sr;
        }
    }
    __syncthreads();
    if (t < 2 * BQ_F) {
        const double lo = (double)BQ_RANGES[t][0], hi = (double)BQ_RANGES[t][1];
        Fs[t] = -1.0 + 2.0 * (F[t] - lo) / (hi - lo);
    }
    __syncthreads();
    double acc[1] = {0.0};
    for (int k = t; k < n_sv; k += 256) {
        const double* w = weights + (long long)k * (1 + 2 * BQ_F);
        double dist = 0.0;
#pragma unroll 4
        for (int j = 0; j < 2 * BQ_F; ++j) {
            const double d = Fs[j] - w[1 + j];
            dist += d * d;
        }
        acc[0] += exp(-dist * 0.05) * w[0];
    }
    bq_block_sum(acc, red, tot);
    const int failed = bad;
    const double score = failed ? NAN : tot[0] + 153.591;
    const int count = s == 0 ? srcs.count[0] : (s == 1 ? srcs.count[1] : srcs.count[2]);
    for (int c = 0; c < count; ++c) {
        const int slot = s == 0 ? srcs.slot[0][c] : (s == 1 ? srcs.slot[1][c] : srcs.slot[2][c]);
        const long long at = (long long)slot * B + i0 + i;
        if (t == 0) out[at] = score;
        if (parts && t < MTD_BRISQUE_PARTS) parts[MTD_BRISQUE_PARTS * at + t] = failed ? NAN : (t < 2 * BQ_F ? F[t] : score);
    }
}

struct BqPlan {
    bool ok;
    int Bc;
    BqGeo g;
    long long per_image, partial, bytes;       // doubles of the maps per (source, image); byte offset of the partials; total
};

// The workspace holds, per source and image of a chunk, the two MSCN maps and BQ_M doubles per tile.  Bc is the largest count for
// which that stays within 64 MiB (each_chunk).
BqPlan brisque_plan(int na, int B, int H, int W) {
    BqPlan p = {};
    if (na < 1 || na > 3 || B < 1 || B > (1 << 24)) return p;
    if (H < BQ_MIN_N || H > BQ_MAX_N || W < BQ_MIN_N || W > BQ_MAX_N) return p;
    BqGeo& g = p.g;
    g.H = H;
    g.W = W;
    g.h2 = H / 2;
    g.w2 = W / 2;
    g.sy = (float)H / (float)g.h2;
    g.sx = (float)W / (float)g.w2;
    g.tx0 = (W + BQ_CT - 1) / BQ_CT;
    g.ty0 = (H + BQ_CT - 1) / BQ_CT;
    g.tx1 = (g.w2 + BQ_CT - 1) / BQ_CT;
    g.ty1 = (g.h2 + BQ_CT - 1) / BQ_CT;
    g.tiles0 = g.tx0 * g.ty0;
    g.tiles1 = g.tx1 * g.ty1;
    p.per_image = (long long)H * W + (long long)g.h2 * g.w2;
    const long long bytes_per = (long long)na * 8 * (p.per_image + (long long)(g.tiles0 + g.tiles1) * BQ_M);
    const long long Bc = p.Bc = each_chunk(BQ_WS_TARGET, bytes_per, B);
    p.partial = (long long)na * Bc * p.per_image * 8;
    p.bytes = p.partial + (long long)na * Bc * (g.tiles0 + g.tiles1) * BQ_M * 8;
    p.ok = true;
    return p;
}

// The distinct pointers among the na sources, each with the output slots it fills.
bool distinct_sources(const void* const* srcs, int na, BqSrcs& u) {
    u = {};
    for (int a = 0; a < na; ++a) {
        if (!srcs[a]) return false;
        int k = 0;
        while (k < u.nu && u.set.p[k] != (const float*)srcs[a]) ++k;
        if (k == u.nu) u.set.p[u.nu++] = (const float*)srcs[a];
        u.slot[k][u.count[k]++] = a;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------------------ total variation
constexpr int TV_ROWS = 8;                                     // rows of an image per workgroup of the first launch

// grid (nu * B, ceil(H / TV_ROWS)).  partial: per (source, image) and row group four doubles: the sums of |dy|, |dx|, dy^2, dx^2
// of the pixels of the group (dy against the row below, dx against the column to the right, where there is one).
__global__ __launch_bounds__(256) void tv_rows_kernel(BqSrcs srcs, int B, int H, int W, double* __restrict__ partial) {
    __shared__ double red[4 * 4], tot[4];
    const int s = blockIdx.x / B, i = blockIdx.x - s * B;
    const float* __restrict__ img = each_pick(srcs.set, s) + (long long)i * H * W;
    const int y0 = blockIdx.y * TV_ROWS;
    const int rows = H - y0 < TV_ROWS ? H - y0 : TV_ROWS;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int e = threadIdx.x; e < rows * W; e += 256) {
        const int ly = e / W, x = e - ly * W, y = y0 + ly;
        const double c = (double)img[(long long)y * W + x];
        if (y + 1 < H) {
            const double d = (double)img[(long long)(y + 1) * W + x] - c;
            v[0] += fabs(d);
            v[2] += d * d;
        }
        if (x + 1 < W) {
            const double d = (double)img[(long long)y * W + x + 1] - c;
            v[1] += fabs(d);
            v[3] += d * d;
        }
    }
    bq_block_sum(v, red, tot);
    if (threadIdx.x < 4) partial[((long long)blockIdx.x * gridDim.y + blockIdx.y) * 4 + threadIdx.x] = tot[threadIdx.x];
}

// One wave per (distinct source, image): the row groups in index order, then piq's total_variation for the norm.
__global__ __launch_bounds__(64) void tv_finish_kernel(BqSrcs srcs, int B, int groups, int norm, const double* __restrict__ partial,
                                                       double* __restrict__ out) {
    __shared__ double sums[4];
    const int s = blockIdx.x / B, i = blockIdx.x - s * B;
    if (threadIdx.x < 4) {
        double a = 0.0;
        for (int k = 0; k < groups; ++k) a += partial[((long long)blockIdx.x * groups + k) * 4 + threadIdx.x];
        sums[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double l1 = sums[0] + sums[1], l2 = sums[2] + sums[3];
    const double score = norm == MTD_TV_L1 ? l1 : (norm == MTD_TV_L2 ? sqrt(l2) : l2);
    const int count = s == 0 ? srcs.count[0] : (s == 1 ? srcs.count[1] : srcs.count[2]);
    for (int c = 0; c < count; ++c) {
        const int slot = s == 0 ? srcs.slot[0][c] : (s == 1 ? srcs.slot[1][c] : srcs.slot[2][c]);
        out[(long long)slot * B + i] = score;
    }
}

bool tv_sizes_ok(int na, int B, int H, int W) {
    return na >= 1 && na <= 3 && B >= 1 && B <= (1 << 24) && H >= MTD_TV_MIN_SIDE && H <= MTD_TV_MAX_SIDE && W >= MTD_TV_MIN_SIDE &&
           W <= MTD_TV_MAX_SIDE;
}

}  // namespace

extern "C" size_t mtd_brisque_ws_bytes(int na, int B, int H, int W) {
    const BqPlan p = brisque_plan(na, B, H, W);
    return p.ok ? (size_t)p.bytes : 0;
}

extern "C" int mtd_brisque_each(const void* const* srcs, int na, int B, int H, int W, int ks, const float* taps, const double* tables, int nt,
                                const double* weights, int n_sv, double* out, double* parts, void* ws, void* stream) {
    if (!srcs || !taps || !tables || !weights || !out || !ws) return MTD_EINVAL;
    if (ks < 3 || ks > BQ_MAXK || !(ks & 1) || nt < 1 || n_sv < 1) return MTD_EINVAL;
    const BqPlan p = brisque_plan(na, B, H, W);
    if (!p.ok) return MTD_EINVAL;
    BqSrcs u;
    if (!distinct_sources(srcs, na, u)) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* maps = (double*)ws;
    double* partial = (double*)((char*)ws + p.partial);
    const int tiles = p.g.tiles0 + p.g.tiles1;
    for (int i0 = 0; i0 < B; i0 += p.Bc) {
        const int Bc = (B - i0) < p.Bc ? (B - i0) : p.Bc;
        hipLaunchKernelGGL(brisque_mscn_kernel, dim3(tiles, u.nu * Bc), dim3(256), 0, s, u, Bc, i0, p.g, ks, taps, maps);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(brisque_moment_kernel, dim3(tiles, u.nu * Bc), dim3(256), 0, s, Bc, p.g, (const double*)maps, partial);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(brisque_finish_kernel, dim3(u.nu * Bc), dim3(256), 0, s, u, Bc, i0, B, p.g, (const double*)partial, tables, nt, weights,
                           n_sv, out, parts);
        MTD_LAUNCH_CHECK();
    }
    return MTD_OK;
}

extern "C" size_t mtd_tv_ws_bytes(int na, int B, int H, int W) {
    if (!tv_sizes_ok(na, B, H, W)) return 0;
    return (size_t)na * B * ((H + TV_ROWS - 1) / TV_ROWS) * 4 * sizeof(double);
}

extern "C" int mtd_tv_each(const void* const* srcs, int na, int B, int H, int W, int norm, double* out, void* ws, void* stream) {
    if (!srcs || !out || !ws || !tv_sizes_ok(na, B, H, W)) return MTD_EINVAL;
    if (norm != MTD_TV_L1 && norm != MTD_TV_L2 && norm != MTD_TV_L2_SQUARED) return MTD_EINVAL;
    BqSrcs u;
    if (!distinct_sources(srcs, na, u)) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int groups = (H + TV_ROWS - 1) / TV_ROWS;
    hipLaunchKernelGGL(tv_rows_kernel, dim3(u.nu * B, groups), dim3(256), 0, s, u, B, H, W, (double*)ws);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(tv_finish_kernel, dim3(u.nu * B), dim3(64), 0, s, u, B, groups, norm, (const double*)ws, out);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
