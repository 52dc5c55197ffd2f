// The feature similarity index of the test loop (the reference vendors it in module/piq: fsim.py, fsim with chromatic=False) of
// single-channel fp32 images in [0, 1], image by image, for up to three sources a[k] against one target b (the convention of
// mtd_iqa_each and mtd_haarpsi_each).  DESIGN 3.17.
//   * the phase-congruency map of an image is 16 (scales x orientations) log-Gabor band-pass responses: one forward 2-D FFT and
//     scales * orientations complex inverse ones.  The transforms are radix-2 passes over lines held in LDS, fp32, with twiddles
//     rounded from double; the bit reversal happens in the LDS address of the load, so every array in memory is in natural order;
//   * every DISTINCT image set is transformed once: a source whose pointer equals the target's (gt in the test loop) shares the
//     target's maps, and the target's maps serve all sources;
//   * from the filter responses on in double: the energy before the noise threshold, the threshold itself, phase congruency,
//     the Scharr gradient magnitude, the similarity maps and every per-image sum, in a fixed order (block_sum256's tree over a
//     tile, the tiles of an image by one workgroup in the same way), no floating-point atomics: an image's numbers do not depend
//     on the batch it is in, on its source slot or on the other sources;
//   * the median of the scale-0 squared amplitude is a radix select over the floats' bit patterns (non-negative floats order as
//     unsigned integers): four passes of 8 bits with integer LDS atomics, exact and deterministic, rank (n - 1) / 2 as
//     torch.median takes it.
// Launches per chunk of the batch: rows forward (pooling on load), columns forward, filter + columns inverse, rows inverse +
// energy (one workgroup per orientation and row tile), thresholds, combine, finish.  The responses themselves are never stored; the column-transformed filtered spectra are.
#include "each_metric.h"
#include "lds_fft.h"          // fs_brev, fs_twiddles, fs_lds_fft
#include <float.h>
#include <math.h>

namespace {

constexpr int FS_TILE_PTS = 4096;             // complex points of one LDS transform tile (lines x length): filter + inverse columns
constexpr int FS_FWD_PTS = 1024;              // ... of the two forward passes (one image has few lines: smaller tiles, more workgroups)
constexpr int FS_SEL_THREADS = 1024;          // threads of a selection workgroup
constexpr int FS_ROW_PTS = 1024;              // points per scale of the inverse row pass: all scales of a pixel meet in one workgroup
constexpr int FS_MAX_S = 4, FS_MAX_O = 8;
constexpr int FS_MIN_N = 16, FS_MAX_N = 512;
constexpr int FS_CT = 16;                     // the combine tile: 16 x 16 pixels, one per thread, with an 18 x 18 halo
constexpr int FS_SUMS = 4;                    // num, den, sum pc_a, sum gm_a
constexpr long long FS_WS_TARGET = 64LL << 20;

// Pixel (y, x) of the pooled map: the ks x ks block of 255 * image summed row by row and divided by ks^2 (avg_pool2d with
// stride ks, floor: 0 <= y < H / ks, 0 <= x < W / ks, so the block is inside the image).  The products are rounded on their own.
__device__ __forceinline__ float fs_pixel(const float* __restrict__ img, int W, int ks, int y, int x) {
    const float* p = img + (long long)y * ks * W + (long long)x * ks;
    if (ks == 1) return __fmul_rn(255.f, p[0]);
    float s = 0.f;
    for (int dy = 0; dy < ks; ++dy)
        for (int dx = 0; dx < ks; ++dx) s += __fmul_rn(255.f, p[(long long)dy * W + dx]);
    return __fdiv_rn(s, (float)(ks * ks));
}

// ---- 1. pool on load + forward rows.  grid (h / L, sets * Bc); slot = set * Bc + image of the chunk.
__global__ __launch_bounds__(256) void fsim_rows_fwd_kernel(EachSets imgs, int Bc, int i0, int H, int W, int ks, int h, int lw, int L,
                                                            float2* __restrict__ spec) {
    __shared__ float2 buf[FS_TILE_PTS + 256];
    __shared__ float2 tw[256];
    const int w = 1 << lw, ld = w + 1;
    const int slot = blockIdx.y, set = slot / Bc, i = slot - set * Bc;
    const float* __restrict__ img = each_pick(imgs, set) + (long long)(i0 + i) * H * W;
    const int y0 = blockIdx.x * L;
    fs_twiddles(tw, w);
    for (int e = threadIdx.x; e < (L << lw); e += 256) {
        const int r = e >> lw, x = e & (w - 1);
        buf[r * ld + fs_brev(x, lw)] = make_float2(fs_pixel(img, W, ks, y0 + r, x), 0.f);
    }
    __syncthreads();
    fs_lds_fft<-1>(buf, L, lw, ld, tw);
    float2* __restrict__ out = spec + ((long long)slot * h + y0) * w;
    for (int e = threadIdx.x; e < (L << lw); e += 256) out[e] = buf[(e >> lw) * ld + (e & (w - 1))];
}

// ---- 2. forward columns, in place (a workgroup owns CW whole columns).  grid (w / CW, slots).
// ---- 3. FILTER: the same tile times filter o * S + s, inverse columns, into Y.  grid (w / CW, orientations of the group * S, slots); `filters` starts at the group's first filter.
template <bool FILTER>
__global__ __launch_bounds__(256) void fsim_cols_kernel(const float2* spec, const float* __restrict__ filters, int lh, int w, int lcw,
                                                        float2* dst) {
    __shared__ float2 buf[FS_TILE_PTS + 256];
    __shared__ float2 tw[256];
    const int h = 1 << lh, ld = h + 1, CW = 1 << lcw;
    const int x0 = blockIdx.x * CW;
    const long long slot = FILTER ? blockIdx.z : blockIdx.y;
    const float2* in = spec + slot * h * w + x0;
    const float* __restrict__ f = FILTER ? filters + (long long)blockIdx.y * h * w + x0 : nullptr;
    float2* out = dst + (FILTER ? (slot * gridDim.y + blockIdx.y) : slot) * h * w + x0;
    fs_twiddles(tw, h);
    for (int e = threadIdx.x; e < (h << lcw); e += 256) {
        const int r = e >> lcw, c = e & (CW - 1);
        float2 v = in[(long long)r * w + c];
        if (FILTER) {
            const float g = f[(long long)r * w + c];
            v.x *= g;
            v.y *= g;
        }
        buf[c * ld + fs_brev(r, lh)] = v;
    }
    __syncthreads();
    if (FILTER) fs_lds_fft<1>(buf, CW, lh, ld, tw);
    else fs_lds_fft<-1>(buf, CW, lh, ld, tw);
    for (int e = threadIdx.x; e < (h << lcw); e += 256) {
        const int r = e >> lcw, c = e & (CW - 1);
        out[(long long)r * w + c] = buf[c * ld + r];
    }
}

// ---- 4. inverse rows of all scales of one orientation and the per-pixel quantities.  grid (h / L, orientations of the group (the first is o0), slots).  Per
// orientation: the energy before the threshold, the scale-0 squared amplitude and the sum over the scales of the amplitudes
// (the combine stage adds the orientations' amplitude sums in their order).
__global__ __launch_bounds__(256) void fsim_rows_inv_kernel(const float2* __restrict__ Y, int S, int O, int o0, int h, int lw, int L,
                                                            float* __restrict__ en, float* __restrict__ an2, float* __restrict__ san) {
    __shared__ float2 buf[FS_MAX_S * (FS_ROW_PTS + 64)];
    __shared__ float2 tw[256];
    const int w = 1 << lw, ld = w + 1;
    const long long yo = (long long)blockIdx.z * gridDim.y + blockIdx.y;          // slot * (orientations of this group) + its index in the group
    const long long so = (long long)blockIdx.z * O + o0 + blockIdx.y;             // slot * O + o
    const int y0 = blockIdx.x * L;
    const long long hw = (long long)h * w;
    const int pts = L << lw;
    const double inv = 1.0 / (double)hw, eps = (double)FLT_EPSILON;
    fs_twiddles(tw, w);
    for (int e = threadIdx.x; e < S * pts; e += 256) {
        const int s = e / pts, q = e - s * pts;
        const int r = q >> lw, x = q & (w - 1);
        buf[(s * L + r) * ld + fs_brev(x, lw)] = Y[(yo * S + s) * hw + (long long)(y0 + r) * w + x];
    }
    __syncthreads();
    fs_lds_fft<1>(buf, S * L, lw, ld, tw);
    for (int p = threadIdx.x; p < pts; p += 256) {
        const int r = p >> lw, x = p & (w - 1);
        double ev[FS_MAX_S], od[FS_MAX_S], se = 0.0, sod = 0.0, sa = 0.0;
#pragma unroll
        for (int s = 0; s < FS_MAX_S; ++s) {
            if (s < S) {
                const float2 v = buf[(s * L + r) * ld + x];
                ev[s] = (double)v.x * inv;
                od[s] = (double)v.y * inv;
                se += ev[s];
                sod += od[s];
                sa += sqrt(ev[s] * ev[s] + od[s] * od[s]);
            }
        }
        const double xe = sqrt(se * se + sod * sod) + eps;
        const double me = se / xe, mo = sod / xe;
        double energy = 0.0;
#pragma unroll
        for (int s = 0; s < FS_MAX_S; ++s)
            if (s < S) energy += ev[s] * me + od[s] * mo - fabs(ev[s] * mo - od[s] * me);
        const long long at = so * hw + (long long)y0 * w + p;
        en[at] = (float)energy;
        an2[at] = (float)(ev[0] * ev[0] + od[0] * od[0]);
        san[at] = (float)sa;
    }
}

// ---- 5. the element of rank `rank` (0-based, ascending) of n non-negative floats: radix select on the bit patterns, 8 bits a
// pass from the top.  A pass counts the candidates (the elements that carry the prefix found so far) per value of its byte into
// an LDS histogram with integer atomics -- a thread adds a run of equal bytes at once, since the top bytes of a map's values
// are nearly all the same --, scans the histogram and keeps the bin that holds the rank.  All FS_SEL_THREADS threads call it;
// all return the value.  hist, scan: 256 words each; pass: 2 words.
__device__ __forceinline__ void fs_count(unsigned u, unsigned mask, unsigned prefix, int shift, unsigned& cur, unsigned& cnt, unsigned* hist) {
    if ((u & mask) != prefix) return;
    const unsigned b = (u >> shift) & 255u;
    if (b == cur) {
        ++cnt;
    } else {
        if (cnt) atomicAdd(&hist[cur], cnt);
        cur = b;
        cnt = 1;
    }
}

__device__ __forceinline__ float fs_select(const float* __restrict__ v, int n, unsigned rank, unsigned* hist, unsigned* scan, unsigned* pass) {
    const int t = threadIdx.x;
    const bool vec = (n & 3) == 0 && ((uintptr_t)v & 15) == 0;
    unsigned prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (t < 256) hist[t] = 0;
        __syncthreads();
        unsigned cur = 0, cnt = 0;
        if (vec) {
            const uint4* v4 = reinterpret_cast<const uint4*>(v);
            for (int i = t; i < (n >> 2); i += FS_SEL_THREADS) {
                const uint4 q = v4[i];
                fs_count(q.x, mask, prefix, shift, cur, cnt, hist);
                fs_count(q.y, mask, prefix, shift, cur, cnt, hist);
                fs_count(q.z, mask, prefix, shift, cur, cnt, hist);
                fs_count(q.w, mask, prefix, shift, cur, cnt, hist);
            }
        } else {
            for (int i = t; i < n; i += FS_SEL_THREADS) fs_count(__float_as_uint(v[i]), mask, prefix, shift, cur, cnt, hist);
        }
        if (cnt) atomicAdd(&hist[cur], cnt);
        __syncthreads();
        if (t < 256) scan[t] = hist[t];
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {                     // inclusive scan of the 256 bins
            unsigned add = 0;
            if (t < 256 && t >= d) add = scan[t - d];
            __syncthreads();
            if (t < 256) scan[t] += add;
            __syncthreads();
        }
        if (t < 256) {
            const unsigned incl = scan[t], excl = incl - hist[t];
            if (excl <= rank && rank < incl) {                   // (exactly one bin: the counts are those of the candidates, rank < their number)
                pass[0] = (unsigned)t;
                pass[1] = rank - excl;
            }
        }
        __syncthreads();
        prefix |= pass[0] << shift;
        mask |= 255u << shift;
        rank = pass[1];
        __syncthreads();
    }
    return __uint_as_float(prefix);
}

__global__ __launch_bounds__(FS_SEL_THREADS) void fsim_median_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
    __shared__ unsigned hist[256], scan[256], pass[2];
    const float m = fs_select(v + (long long)blockIdx.x * n, n, (unsigned)(n - 1) / 2u, hist, scan, pass);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}

// grid (O, slots): the noise threshold T of (image, orientation) from the median of its scale-0 squared amplitude.
// consts: em_n[O], sum_an2[O], sum_ai_aj[O].
__global__ __launch_bounds__(FS_SEL_THREADS) void fsim_threshold_kernel(const float* __restrict__ an2, int n, const double* __restrict__ consts,
                                                                        float k, double* __restrict__ T) {
    __shared__ unsigned hist[256], scan[256], pass[2];
    const int o = blockIdx.x, O = gridDim.x;
    const long long at = (long long)blockIdx.y * O + o;
    const float m = fs_select(an2 + at * n, n, (unsigned)(n - 1) / 2u, hist, scan, pass);
    if (threadIdx.x != 0) return;
    const double noise_power = (-(double)m / log(0.5)) / consts[o];
    const double tau = sqrt((2.0 * noise_power * consts[O + o] + 4.0 * noise_power * consts[2 * O + o]) / 2.0);
    const double pi_2 = 1.57079632679489661923;
    T[at] = (tau * sqrt(pi_2) + (double)k * sqrt((2.0 - pi_2) * tau * tau)) / 1.7;
}

// ---- 6. combine.  grid (w / 16, h / 16, na * Bc); blockIdx.z = source * Bc + image of the chunk; one pixel per thread.
__device__ __forceinline__ double fs_pc(const float* __restrict__ en, const float* __restrict__ san, const double* __restrict__ T, long long slot,
                                        int O, long long hw, long long pix) {
    const double eps = (double)FLT_EPSILON;
    double e = 0.0, a = 0.0;
    for (int o = 0; o < O; ++o) {
        e += fmax((double)en[(slot * O + o) * hw + pix] - T[slot * O + o], 0.0);
        a += (double)san[(slot * O + o) * hw + pix];
    }
    return (e + eps) / (a + eps);
}

__device__ __forceinline__ double fs_scharr(const float* P) {          // P: the pixel's row in the 18-wide halo tile, at its column
    constexpr int HL = FS_CT + 2;
    const double a = P[-HL - 1], b = P[-HL], c = P[-HL + 1], d = P[-1], f = P[1], g = P[HL - 1], hh = P[HL], i = P[HL + 1];
    const double gx = (3.0 * (c - a) + 10.0 * (f - d) + 3.0 * (i - g)) / 16.0;
    const double gy = (3.0 * (g - a) + 10.0 * (hh - b) + 3.0 * (i - c)) / 16.0;
    return sqrt(gx * gx + gy * gy);
}

__global__ __launch_bounds__(256) void fsim_combine_kernel(EachSets imgs, EachMap map, int Bc, int i0, int H, int W, int ks, int h, int w, int O,
                                                           const float* __restrict__ en, const float* __restrict__ san,
                                                           const double* __restrict__ T, double* __restrict__ partial) {
    constexpr int HL = FS_CT + 2;
    __shared__ float As[HL * HL], Bs[HL * HL];
    __shared__ double red[FS_SUMS * 256];
    const int k = blockIdx.z / Bc, i = blockIdx.z - k * Bc;
    const int sa_set = each_pick(map, k), sb_set = map.tgt;
    const float* __restrict__ a = each_pick(imgs, sa_set) + (long long)(i0 + i) * H * W;
    const float* __restrict__ b = each_pick(imgs, sb_set) + (long long)(i0 + i) * H * W;
    const long long sa = (long long)sa_set * Bc + i, sb = (long long)sb_set * Bc + i;
    const int tx0 = blockIdx.x * FS_CT, ty0 = blockIdx.y * FS_CT;
    for (int e = threadIdx.x; e < HL * HL; e += 256) {
        const int ly = e / HL, lx = e - ly * HL;
        const int y = ty0 + ly - 1, x = tx0 + lx - 1;
        float va = 0.f, vb = 0.f;                                // the gradient filters' zero padding
        if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) {
            va = fs_pixel(a, W, ks, y, x);
            vb = fs_pixel(b, W, ks, y, x);
        }
        As[e] = va;
        Bs[e] = vb;
    }
    __syncthreads();
    const int ly = threadIdx.x / FS_CT, lx = threadIdx.x - ly * FS_CT;
    const long long hw = (long long)h * w, pix = (long long)(ty0 + ly) * w + tx0 + lx;
    const double pa = fs_pc(en, san, T, sa, O, hw, pix), pb = fs_pc(en, san, T, sb, O, hw, pix);
    const double ga = fs_scharr(As + (ly + 1) * HL + lx + 1), gb = fs_scharr(Bs + (ly + 1) * HL + lx + 1);
    const double PC = each_similarity(pa, pb, 0.85), GM = each_similarity(ga, gb, 160.0);
    const double pm = pa > pb ? pa : pb;
    double sums[FS_SUMS] = {GM * PC * pm, pm, pa, ga};
    block_sum256(sums, red);
    each_store(partial, sums);
}

// ---- 7. one workgroup per (source, image of the chunk) g: the tile partials in a fixed order, then score = num / den.
__global__ __launch_bounds__(256) void fsim_finish_kernel(const double* __restrict__ partial, int tiles, EachMap map, int Bc, int i0, int B, int O,
                                                          const double* __restrict__ T, double* __restrict__ out, double* __restrict__ parts) {
    __shared__ double red[FS_SUMS * 256];
    const int g = blockIdx.x, k = g / Bc, i = g - k * Bc;
    double sums[FS_SUMS];
    each_fold(partial + (long long)FS_SUMS * g * tiles, tiles, sums, red);
    if (threadIdx.x != 0) return;
    const long long at = (long long)k * B + i0 + i;
    if (parts) {
        double* pp = parts + at * (FS_SUMS + O);
#pragma unroll
        for (int q = 0; q < FS_SUMS; ++q) pp[q] = sums[q];
        const long long slot = (long long)each_pick(map, k) * Bc + i;
        for (int o = 0; o < O; ++o) pp[FS_SUMS + o] = T[slot * O + o];
    }
    out[at] = sums[0] / sums[1];
}

int fs_log2(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

struct FsPlan {
    bool ok;
    int Bc;                                    // images of a chunk
    int Og;                                    // orientations whose filtered spectra are held at a time
    long long spec, Y, en, an2, san, T, partial, bytes;      // byte offsets into the workspace, and its size
};

// The workspace holds one chunk of Bc images of every set (na sources + the target: the pointers may all differ).  Per image of
// a chunk and set: the spectrum (8 hw), the column-transformed filtered spectra (8 O S hw), the energy, squared-amplitude and
// amplitude-sum maps (4 O hw each), O thresholds; per image and source the tile partials.  Bc is the largest count for
// which that stays within 64 MiB, at least 1 and at most B.  Where not even one image fits, the filtered spectra of Og < O
// orientations are held at a time (8 Og S hw): Og is the largest count with which one image fits, at least 1, and the
// orientations are walked in groups of Og.
FsPlan fsim_plan(int na, int B, int h, int w, int S, int O) {
    FsPlan p = {};
    if (na < 1 || na > 3 || B < 1 || B > (1 << 24)) return p;
    if (h < FS_MIN_N || h > FS_MAX_N || w < FS_MIN_N || w > FS_MAX_N || (h & (h - 1)) || (w & (w - 1))) return p;
    if (S < 1 || S > FS_MAX_S || O < 1 || O > FS_MAX_O) return p;
    const long long hw = (long long)h * w, sets = na + 1, tiles = (h / FS_CT) * (w / FS_CT);
    int Og = O;
    long long per_image = 0;
    for (;; --Og) {
        per_image = sets * (hw * (8 + 8LL * Og * S + 12LL * O) + 8LL * O) + na * tiles * FS_SUMS * 8;
        if (per_image <= FS_WS_TARGET || Og == 1) break;
    }
    p.Og = Og;
    const long long Bc = p.Bc = each_chunk(FS_WS_TARGET, per_image, B);
    const long long slots = sets * Bc;
    p.spec = 0;
    p.Y = p.spec + slots * hw * 8;
    p.en = p.Y + slots * Og * S * hw * 8;         // (every map starts on a multiple of 1 KiB: the selection reads 16 bytes a lane)
    p.an2 = p.en + slots * O * hw * 4;
    p.san = p.an2 + slots * O * hw * 4;
    p.T = p.san + slots * O * hw * 4;
    p.partial = p.T + slots * O * 8;
    p.bytes = p.partial + na * Bc * tiles * FS_SUMS * 8;
    p.ok = true;
    return p;
}

}  // namespace

extern "C" size_t mtd_fsim_ws_bytes(int na, int B, int h, int w, int scales, int orientations) {
    const FsPlan p = fsim_plan(na, B, h, w, scales, orientations);
    return p.ok ? (size_t)p.bytes : 0;
}

extern "C" int mtd_fsim_median(const float* values, int n, int count, float* out, void* stream) {
    if (!values || !out || n < 1 || count < 1 || count > 65535) return MTD_EINVAL;
    hipLaunchKernelGGL(fsim_median_kernel, dim3(count), dim3(FS_SEL_THREADS), 0, (hipStream_t)stream, values, n, out);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_fsim_each(const void* const* srcs, int na, const void* target, int B, int H, int W, int ks, int scales, int orientations,
                             float k, const float* filters, const double* consts, double* out, double* parts, void* ws, void* stream) {
    if (!srcs || !target || !filters || !consts || !out || !ws) return MTD_EINVAL;
    if (H < 1 || W < 1 || ks < 1 || ks > 64 || (long long)H * W > (1LL << 30) || !(k == k)) return MTD_EINVAL;
    const int h = H / ks, w = W / ks, S = scales, O = orientations;
    const FsPlan p = fsim_plan(na, B, h, w, S, O);
    if (!p.ok) return MTD_EINVAL;
    EachSets imgs;
    EachMap map;
    const int sets = each_sets(srcs, na, target, imgs, map);
    if (sets < 0) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    float2* spec = (float2*)(base + p.spec);
    float2* Y = (float2*)(base + p.Y);
    double* T = (double*)(base + p.T);
    double* partial = (double*)(base + p.partial);
    float* en = (float*)(base + p.en);
    float* an2 = (float*)(base + p.an2);
    float* san = (float*)(base + p.san);
    const int lh = fs_log2(h), lw = fs_log2(w);
    const int Lf = (FS_FWD_PTS / w) < h ? (FS_FWD_PTS / w) : h;            // rows of a forward row tile
    const int CF = (FS_FWD_PTS / h) < w ? (FS_FWD_PTS / h) : w;            // columns of a forward column tile
    const int CW = (FS_TILE_PTS / h) < w ? (FS_TILE_PTS / h) : w;          // columns of a filter + inverse column tile
    const int Li = (FS_ROW_PTS / w) < h ? (FS_ROW_PTS / w) : h;            // rows of an inverse row tile
    const int tiles = (h / FS_CT) * (w / FS_CT);
    for (int i0 = 0; i0 < B; i0 += p.Bc) {
        const int Bc = (B - i0) < p.Bc ? (B - i0) : p.Bc;
        const int slots = sets * Bc;
        hipLaunchKernelGGL(fsim_rows_fwd_kernel, dim3(h / Lf, slots), dim3(256), 0, s, imgs, Bc, i0, H, W, ks, h, lw, Lf, spec);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(fsim_cols_kernel<false>, dim3(w / CF, slots), dim3(256), 0, s, (const float2*)spec, (const float*)nullptr, lh, w,
                           fs_log2(CF), spec);
        MTD_LAUNCH_CHECK();
        for (int o0 = 0; o0 < O; o0 += p.Og) {                                 // (one group where a whole image fits: p.Og == O)
            const int og = (O - o0) < p.Og ? (O - o0) : p.Og;
            hipLaunchKernelGGL(fsim_cols_kernel<true>, dim3(w / CW, og * S, slots), dim3(256), 0, s, (const float2*)spec,
                               filters + (long long)o0 * S * h * w, lh, w, fs_log2(CW), Y);
            MTD_LAUNCH_CHECK();
            hipLaunchKernelGGL(fsim_rows_inv_kernel, dim3(h / Li, og, slots), dim3(256), 0, s, (const float2*)Y, S, O, o0, h, lw, Li, en, an2, san);
            MTD_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(fsim_threshold_kernel, dim3(O, slots), dim3(FS_SEL_THREADS), 0, s, (const float*)an2, h * w, consts, k, T);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(fsim_combine_kernel, dim3(w / FS_CT, h / FS_CT, na * Bc), dim3(256), 0, s, imgs, map, Bc, i0, H, W, ks, h, w, O,
                           (const float*)en, (const float*)san, (const double*)T, partial);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(fsim_finish_kernel, dim3(na * Bc), dim3(256), 0, s, (const double*)partial, tiles, map, Bc, i0, B, O, (const double*)T, out,
                           parts);
        MTD_LAUNCH_CHECK();
    }
    return MTD_OK;
}
