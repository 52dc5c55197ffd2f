// Res-FFT-Conv spectral path for maps of any size 16 <= H, W <= 512 (inference on cropped slices, reduced fields of view,
// scanner matrices that are not powers of two).  The power-of-two squares keep their kernels (resfft_any.hip, resfft.hip);
// these serve the shapes those refuse.  Same three stages and the same spectrum layout [B][kw 0..W/2][h 0..H-1][Re 32 | Im 32]:
//   rows forward   a pair of image rows as one complex transform of length W, split into the two half spectra (odd H: the
//                  last row has a zero partner);
//   columns        a complex transform of length H per column, the 64 x 64 mix on the matrix cores (+ bias, ReLU), the inverse
//                  transform (three launches: the transforms work on channel groups, the mix needs all 32 channels at once);
//   rows back      the complex-to-real transform of length W (two rows per transform) with the residual epilogue.
// Transforms: a line of one channel group (GCG = 8 channels, lane = channel) lives in LDS as [len][8] re + im.
//   * 7-smooth lengths: in-place mixed-radix passes (radix 4, 2, 3, 5, 7).  Forward: decimation in frequency, natural in,
//     digit-reversed out; inverse: the transposed passes in reverse order, digit-reversed in, natural out.  A per-workgroup
//     table maps a frequency to its digit-reversed place.
//   * lengths with a prime factor above 7: Bluestein.  X_k = w_k sum_n (x_n w_n) conj(w_{k-n}), w_n = exp(-i pi (n^2 mod 2N) / N):
//     a circular convolution of power-of-two length M >= 2N - 1 (M <= 1024) done as forward pass (DIF), product with the
//     filter's spectrum (in the DIF output order, 1/M folded in), inverse passes (DIT).  The filter spectrum of each Bluestein
//     length is built by a one-workgroup launch into the caller's workspace before the transform that needs it.  The
//     inverse transform is conj(F(conj X)).  LDS: M x 8 channels x 8 bytes = 64 KB at M = 1024, plus tables.
// Twiddle angles come from integer-reduced indices (j q step < len; n^2 mod 2N in 64 bits) and go through sincospif.
#include "common.h"

namespace {

constexpr int GCG = 8;            // channels per workgroup: four workgroups per line
constexpr int GNT = 256;          // threads per workgroup
constexpr int GMAXST = 12;        // passes of a plan (1024 = 4^5: five)

struct GenPlan {
    int n;                        // transform length
    int len;                      // length in LDS: n (mixed radix) or the Bluestein convolution length M
    int blue;                     // 1: Bluestein
    int nst;                      // passes
    int rad[GMAXST];              // radices of the passes, decimation-in-frequency order
};

// what a kernel gets: the radices as 4-bit fields of one word (a run-time indexed array in the kernel arguments would be copied
// to scratch memory)
struct DevPlan {
    int n, len, blue, nst;
    unsigned long long rad;
    __device__ int r(int s) const { return (int)((rad >> (4 * s)) & 15); }
};

// host side: radices of a 7-smooth length (4 first, then 2, 3, 5, 7); false if a prime factor above 7 is left
bool factorize(int len, GenPlan& p) {
    int r = len;
    p.nst = 0;
    const int order[5] = {4, 2, 3, 5, 7};
    for (int q : order)
        while (r % q == 0 && p.nst < GMAXST) {
            p.rad[p.nst++] = q;
            r /= q;
        }
    return r == 1;
}

bool make_plan(int n, GenPlan& p) {
    if (n < 16 || n > 512) return false;
    p.n = n;
    if (factorize(n, p)) {
        p.len = n;
        p.blue = 0;
        return true;
    }
    int m = 1;
    while (m < 2 * n - 1) m <<= 1;
    p.len = m;
    p.blue = 1;
    return factorize(m, p);
}

inline size_t filter_bytes(const GenPlan& p) { return p.blue ? (size_t)p.len * 8 : 0; }

DevPlan dev_plan(const GenPlan& p) {
    DevPlan d{p.n, p.len, p.blue, p.nst, 0ull};
    for (int s = 0; s < p.nst; ++s) d.rad |= (unsigned long long)p.rad[s] << (4 * s);
    return d;
}

// ---------------------------------------------------------------------------------------------------------- device
// y_q = sum_t x_t exp(SIGN 2 pi i t q / R), in registers
template <int R, int SIGN>
__device__ __forceinline__ void dft_small(float* xr, float* xi) {
    if constexpr (R == 2) {
        const float ar = xr[0], ai = xi[0];
        xr[0] = ar + xr[1]; xi[0] = ai + xi[1];
        xr[1] = ar - xr[1]; xi[1] = ai - xi[1];
    } else if constexpr (R == 4) {
        const float s0r = xr[0] + xr[2], s0i = xi[0] + xi[2], d0r = xr[0] - xr[2], d0i = xi[0] - xi[2];
        const float s1r = xr[1] + xr[3], s1i = xi[1] + xi[3], d1r = xr[1] - xr[3], d1i = xi[1] - xi[3];
        // SIGN i (d1): (-SIGN d1i, SIGN d1r)
        xr[0] = s0r + s1r; xi[0] = s0i + s1i;
        xr[2] = s0r - s1r; xi[2] = s0i - s1i;
        xr[1] = d0r - SIGN * d1i; xi[1] = d0i + SIGN * d1r;
        xr[3] = d0r + SIGN * d1i; xi[3] = d0i - SIGN * d1r;
    } else {
        // odd R: pairs t, R - t; cos / sin of 2 pi k / R
        constexpr float C3[3] = {1.f, -0.5f, -0.5f};
        constexpr float S3[3] = {0.f, 0.86602540378443865f, -0.86602540378443865f};
        constexpr float C5[5] = {1.f, 0.30901699437494742f, -0.80901699437494742f, -0.80901699437494742f, 0.30901699437494742f};
        constexpr float S5[5] = {0.f, 0.95105651629515357f, 0.58778525229247313f, -0.58778525229247313f, -0.95105651629515357f};
        constexpr float C7[7] = {1.f, 0.62348980185873353f, -0.22252093395631440f, -0.90096886790241913f, -0.90096886790241913f,
                                 -0.22252093395631440f, 0.62348980185873353f};
        constexpr float S7[7] = {0.f, 0.78183148246802981f, 0.97492791218182361f, 0.43388373911755812f, -0.43388373911755812f,
                                 -0.97492791218182361f, -0.78183148246802981f};
        const float* C = R == 3 ? C3 : R == 5 ? C5 : C7;
        const float* S = R == 3 ? S3 : R == 5 ? S5 : S7;
        constexpr int H = (R - 1) / 2;
        float ar[H], ai[H], dr[H], di[H];
#pragma unroll
        for (int t = 1; t <= H; ++t) {
            ar[t - 1] = xr[t] + xr[R - t]; ai[t - 1] = xi[t] + xi[R - t];
            dr[t - 1] = xr[t] - xr[R - t]; di[t - 1] = xi[t] - xi[R - t];
        }
        float yr[R], yi[R];
        yr[0] = xr[0]; yi[0] = xi[0];
#pragma unroll
        for (int t = 0; t < H; ++t) { yr[0] += ar[t]; yi[0] += ai[t]; }
#pragma unroll
        for (int q = 1; q <= H; ++q) {
            float pr = xr[0], pi = xi[0], mr = 0.f, mi = 0.f;      // sum a C, sum d S
#pragma unroll
            for (int t = 1; t <= H; ++t) {
                const int k = (t * q) % R;
                pr += ar[t - 1] * C[k]; pi += ai[t - 1] * C[k];
                mr += dr[t - 1] * S[k]; mi += di[t - 1] * S[k];
            }
            // y_q = p + SIGN i m, y_{R-q} = p - SIGN i m
            yr[q] = pr - SIGN * mi; yi[q] = pi + SIGN * mr;
            yr[R - q] = pr + SIGN * mi; yi[R - q] = pi - SIGN * mr;
        }
#pragma unroll
        for (int q = 0; q < R; ++q) { xr[q] = yr[q]; xi[q] = yi[q]; }
    }
}

// One pass over [len][CG] in LDS for the blocks of sub-length L: butterflies (blk, j), points blk L + j + t m, m = L / R.
// DIF: R-point DFT, then the twiddles w_L^(j q); DIT (its transpose): twiddles first, then the DFT.  twc / tws: cos / sin of
// 2 pi i / len, i < len (the twiddle index j q len / L < len).
template <int R, int SIGN, bool DIF, int CG>
__device__ __forceinline__ void fft_pass(float* re, float* im, const float* twc, const float* tws, int len, int L) {
    const int m = L / R, step = len / L, items = (len / R) * CG;
    for (int e = threadIdx.x; e < items; e += blockDim.x) {
        const int c = e % CG, bi = e / CG;
        const int blk = bi / m, j = bi - blk * m;
        const int base = (blk * L + j) * CG + c;
        float xr[R], xi[R];
#pragma unroll
        for (int t = 0; t < R; ++t) { xr[t] = re[base + t * m * CG]; xi[t] = im[base + t * m * CG]; }
        if (!DIF) {
#pragma unroll
            for (int q = 1; q < R; ++q) {
                const int ix = j * q * step;
                const float cs = twc[ix], sn = SIGN * tws[ix];
                const float r0 = xr[q];
                xr[q] = r0 * cs - xi[q] * sn; xi[q] = r0 * sn + xi[q] * cs;
            }
        }
        dft_small<R, SIGN>(xr, xi);
        if (DIF) {
#pragma unroll
            for (int q = 1; q < R; ++q) {
                const int ix = j * q * step;
                const float cs = twc[ix], sn = SIGN * tws[ix];
                const float r0 = xr[q];
                xr[q] = r0 * cs - xi[q] * sn; xi[q] = r0 * sn + xi[q] * cs;
            }
        }
#pragma unroll
        for (int t = 0; t < R; ++t) { re[base + t * m * CG] = xr[t]; im[base + t * m * CG] = xi[t]; }
    }
}

template <int SIGN, bool DIF, int CG>
__device__ __forceinline__ void fft_pass_any(int r, float* re, float* im, const float* twc, const float* tws, int len, int L) {
    switch (r) {
        case 4: fft_pass<4, SIGN, DIF, CG>(re, im, twc, tws, len, L); break;
        case 2: fft_pass<2, SIGN, DIF, CG>(re, im, twc, tws, len, L); break;
        case 3: fft_pass<3, SIGN, DIF, CG>(re, im, twc, tws, len, L); break;
        case 5: fft_pass<5, SIGN, DIF, CG>(re, im, twc, tws, len, L); break;
        default: fft_pass<7, SIGN, DIF, CG>(re, im, twc, tws, len, L); break;
    }
}

// natural in, digit-reversed out (unnormalised); ends with a barrier
template <int SIGN, int CG>
__device__ void fft_dif(float* re, float* im, const float* twc, const float* tws, const DevPlan& p) {
    int L = p.len;
    for (int s = 0; s < p.nst; ++s) {
        fft_pass_any<SIGN, true, CG>(p.r(s), re, im, twc, tws, p.len, L);
        L /= p.r(s);
        __syncthreads();
    }
}

// digit-reversed in, natural out (unnormalised); ends with a barrier
template <int SIGN, int CG>
__device__ void fft_dit(float* re, float* im, const float* twc, const float* tws, const DevPlan& p) {
    int L = 1;
    for (int s = p.nst - 1; s >= 0; --s) {
        L *= p.r(s);
        fft_pass_any<SIGN, false, CG>(p.r(s), re, im, twc, tws, p.len, L);
        __syncthreads();
    }
}

// place of frequency k in the DIF output: k = q1 + r1 (q2 + r2 (...)) -> q1 len / r1 + q2 len / (r1 r2) + ...
__device__ __forceinline__ int digit_rev(int k, const DevPlan& p) {
    int pos = 0, L = p.len;
    for (int s = 0; s < p.nst; ++s) {
        const int r = p.r(s), m = L / r, q = k % r;
        k /= r;
        pos += q * m;
        L = m;
    }
    return pos;
}

// Workgroup tables in LDS: twiddles (len), and either the digit-reversal map (mixed radix) or the chirp w_n (Bluestein, n < N)
struct GenLds {
    float* re;
    float* im;
    float* twc;
    float* tws;
    int* drev;
    float* chc;
    float* chs;
};

__host__ __device__ inline size_t gen_lds_floats(int len, int cg) { return (size_t)len * (2 * cg + 4); }

__device__ GenLds gen_tables(float* lds, const DevPlan& p, int cg) {
    GenLds t;
    t.re = lds;
    t.im = lds + p.len * cg;
    t.twc = t.im + p.len * cg;
    t.tws = t.twc + p.len;
    t.drev = reinterpret_cast<int*>(t.tws + p.len);
    t.chc = t.tws + p.len;
    t.chs = t.chc + p.len;
    for (int i = threadIdx.x; i < p.len; i += blockDim.x) {
        float sn, cs;
        sincospif((float)(2 * i) / (float)p.len, &sn, &cs);
        t.twc[i] = cs;
        t.tws[i] = sn;
    }
    if (p.blue) {
        for (int nn = threadIdx.x; nn < p.n; nn += blockDim.x) {
            const long long r = ((long long)nn * nn) % (2LL * p.n);       // exp(-i pi n^2 / N) = exp(-i pi (n^2 mod 2N) / N)
            float sn, cs;
            sincospif((float)r / (float)p.n, &sn, &cs);
            t.chc[nn] = cs;
            t.chs[nn] = -sn;
        }
    } else {
        for (int k = threadIdx.x; k < p.len; k += blockDim.x) t.drev[k] = digit_rev(k, p);
    }
    __syncthreads();
    return t;
}

// A line transform: put() the N inputs (every place 0..N-1 once), run(), get() the N outputs.  INV: the inverse transform.
template <bool INV>
struct Line {
    GenLds t;
    DevPlan p;
    const float2* filt;
    __device__ void put(int k, int c, float vr, float vi) {
        if (!p.blue) {
            const int pos = (INV ? t.drev[k] : k) * GCG + c;
            t.re[pos] = vr;
            t.im[pos] = vi;
        } else {
            if (INV) vi = -vi;
            const float cs = t.chc[k], sn = t.chs[k];
            t.re[k * GCG + c] = vr * cs - vi * sn;
            t.im[k * GCG + c] = vr * sn + vi * cs;
        }
    }
    // (Bluestein: the zero padding n = N .. M-1; called in the put phase)
    __device__ void pad() {
        if (!p.blue) return;
        for (int e = p.n * GCG + (int)threadIdx.x; e < p.len * GCG; e += blockDim.x) {
            t.re[e] = 0.f;
            t.im[e] = 0.f;
        }
    }
    __device__ void run() {
        __syncthreads();
        if (!p.blue) {
            if (INV) fft_dit<+1, GCG>(t.re, t.im, t.twc, t.tws, p);
            else fft_dif<-1, GCG>(t.re, t.im, t.twc, t.tws, p);
            return;
        }
        fft_dif<-1, GCG>(t.re, t.im, t.twc, t.tws, p);
        for (int e = threadIdx.x; e < p.len * GCG; e += blockDim.x) {
            const float2 f = filt[e / GCG];
            const float ar = t.re[e], ai = t.im[e];
            t.re[e] = ar * f.x - ai * f.y;
            t.im[e] = ar * f.y + ai * f.x;
        }
        __syncthreads();
        fft_dit<+1, GCG>(t.re, t.im, t.twc, t.tws, p);
    }
    __device__ void get(int n, int c, float& vr, float& vi) const {
        if (!p.blue) {
            const int pos = (INV ? n : t.drev[n]) * GCG + c;
            vr = t.re[pos];
            vi = t.im[pos];
        } else {
            const float zr = t.re[n * GCG + c], zi = t.im[n * GCG + c], cs = t.chc[n], sn = t.chs[n];
            vr = zr * cs - zi * sn;
            vi = zr * sn + zi * cs;
            if (INV) vi = -vi;
        }
    }
};

// Bluestein filter spectrum for one length: b_m = conj(w_m) at m and M - m (m < N), zero between; DIF order, times 1/M.
// One workgroup.
__global__ __launch_bounds__(GNT) void bluestein_filter_kernel(DevPlan p, float2* __restrict__ filt) {
    extern __shared__ float lds[];
    GenLds t = gen_tables(lds, p, 1);
    for (int m = threadIdx.x; m < p.len; m += blockDim.x) {
        const int src = m < p.n ? m : (m > p.len - p.n ? p.len - m : -1);
        t.re[m] = src >= 0 ? t.chc[src] : 0.f;
        t.im[m] = src >= 0 ? -t.chs[src] : 0.f;
    }
    __syncthreads();
    fft_dif<-1, 1>(t.re, t.im, t.twc, t.tws, p);
    const float inv = 1.f / (float)p.len;
    for (int m = threadIdx.x; m < p.len; m += blockDim.x) filt[m] = make_float2(t.re[m] * inv, t.im[m] * inv);
}

// rows forward: workgroup (group g, row pair, image b); R[b][kw][h][Re 32 | Im 32], scale 1/sqrt(W)
__global__ __launch_bounds__(GNT) void rfft_rows_gen_kernel(const float* __restrict__ x, int x_ld, float* __restrict__ R, int H,
                                                            DevPlan p, const float2* __restrict__ filt) {
    extern __shared__ float lds[];
    const int g = blockIdx.x, h = 2 * blockIdx.y, b = blockIdx.z, W = p.n, nkw = W / 2 + 1;
    const bool two = h + 1 < H;
    Line<false> ln{gen_tables(lds, p, GCG), p, filt};
    const float* r0 = x + (long long)(b * H + h) * W * x_ld + g * GCG;
    for (int e = threadIdx.x; e < W * GCG; e += blockDim.x) {
        const int w = e / GCG, c = e % GCG;
        const float vr = r0[(long long)w * x_ld + c];
        const float vi = two ? r0[((long long)W + w) * x_ld + c] : 0.f;
        ln.put(w, c, vr, vi);
    }
    ln.pad();
    ln.run();
    const float sc = 0.5f * rsqrtf((float)W);
    for (int e = threadIdx.x; e < nkw * GCG; e += blockDim.x) {
        const int kw = e / GCG, c = e % GCG;
        float zkr, zki, zmr, zmi;
        ln.get(kw, c, zkr, zki);
        ln.get(kw == 0 ? 0 : W - kw, c, zmr, zmi);
        float* o = R + ((long long)(b * nkw + kw) * H + h) * 64 + g * GCG + c;
        o[0] = (zkr + zmr) * sc;
        o[32] = (zki - zmi) * sc;
        if (two) {
            o[64] = (zki + zmi) * sc;
            o[96] = (zmr - zkr) * sc;
        }
    }
}

// columns: workgroup (group g, column kw, image b), a transform of length H along the column (src may be dst: a workgroup
// reads its whole line before it writes).  INV: the inverse, which also zeroes the imaginary halves of column 0 and (even W) column W/2 -- the complex-to-real step does not read them.
template <bool INV>
__global__ __launch_bounds__(GNT) void cols_gen_kernel(const float* src, float* dst, int W, DevPlan p,
                                                       const float2* __restrict__ filt) {
    extern __shared__ float lds[];
    const int g = blockIdx.x, kw = blockIdx.y, b = blockIdx.z, H = p.n, nkw = W / 2 + 1;
    Line<INV> ln{gen_tables(lds, p, GCG), p, filt};
    const long long base = (long long)(b * nkw + kw) * H * 64 + g * GCG;
    for (int e = threadIdx.x; e < H * GCG; e += blockDim.x) {
        const int h = e / GCG, c = e % GCG;
        ln.put(h, c, src[base + h * 64 + c], src[base + h * 64 + 32 + c]);
    }
    ln.pad();
    ln.run();
    const float sc = rsqrtf((float)H);
    const bool edge = INV && (kw == 0 || 2 * kw == W);
    for (int e = threadIdx.x; e < H * GCG; e += blockDim.x) {
        const int h = e / GCG, c = e % GCG;
        float vr, vi;
        ln.get(h, c, vr, vi);
        dst[base + h * 64 + c] = vr * sc;
        dst[base + h * 64 + 32 + c] = edge ? 0.f : vi * sc;
    }
}

// channel mix in place over nrows spectrum rows of 64 floats: y[o] = relu(sum_k w2t[k][o] z[k] + b2[o]).  64 rows per
// workgroup; wave w takes rows 32 (w & 1) .. +31 and outputs 32 (w >> 1) .. +31 on v_mfma_f32_32x32x2_f32 (as in
// resfft_any.hip: A = W from LDS, B = the rows, padded to 65 floats).
constexpr int MIX_LD = 65;
__global__ __launch_bounds__(GNT) void mix_gen_kernel(float* __restrict__ T, const float* __restrict__ w2t,
                                                      const float* __restrict__ b2, long long nrows) {
    __shared__ float wl[64 * 64 + 64];
    __shared__ float tile[64 * MIX_LD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long row0 = (long long)blockIdx.x * 64;
    for (int i = tid; i < 64 * 64 + 64; i += GNT) wl[i] = i < 4096 ? w2t[i] : b2[i - 4096];
    for (int i = tid; i < 64 * 64; i += GNT) {
        const int r = i >> 6, k = i & 63;
        tile[r * MIX_LD + k] = row0 + r < nrows ? T[(row0 + r) * 64 + k] : 0.f;
    }
    __syncthreads();
    const int tl = wv & 1, ob = wv >> 1;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* z = tile + (tl * 32 + (lane & 31)) * MIX_LD + (lane >> 5);
    const float* wp = wl + (lane >> 5) * 64 + ob * 32 + (lane & 31);
#pragma unroll 8
    for (int s2 = 0; s2 < 32; ++s2) acc = mfma32(wp[s2 * 128], z[s2 * 2], acc);
    __syncthreads();
    float* d = tile + (tl * 32 + (lane & 31)) * MIX_LD + ob * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = mfma32_row(r, lane);
        d[o] = fmaxf(acc[r] + wl[4096 + ob * 32 + o], 0.f);
    }
    __syncthreads();
    for (int i = tid; i < 64 * 64; i += GNT) {
        const int r = i >> 6, k = i & 63;
        if (row0 + r < nrows) T[(row0 + r) * 64 + k] = tile[r * MIX_LD + k];
    }
}

// rows back: workgroup (group g, row pair, image b).  Z = A + i B from the half spectra of rows h, h + 1 (the imaginary
// parts of column 0 and, even W, column W/2 dropped; odd W has no Nyquist column: its last column is mirrored like the
// others), inverse transform: row h = Re, row h + 1 = Im; out = y / sqrt(W) + add1 + add2.
__global__ __launch_bounds__(GNT) void irfft_rows_gen_kernel(const float* __restrict__ T, float* __restrict__ out, int out_ld,
                                                             const float* __restrict__ add1, int add1_ld,
                                                             const float* __restrict__ add2, int add2_ld, int H, DevPlan p,
                                                             const float2* __restrict__ filt) {
    extern __shared__ float lds[];
    const int g = blockIdx.x, h = 2 * blockIdx.y, b = blockIdx.z, W = p.n, nkw = W / 2 + 1;
    const bool two = h + 1 < H;
    Line<true> ln{gen_tables(lds, p, GCG), p, filt};
    for (int e = threadIdx.x; e < nkw * GCG; e += blockDim.x) {
        const int kw = e / GCG, c = e % GCG;
        const float* t = T + ((long long)(b * nkw + kw) * H + h) * 64 + g * GCG + c;
        const bool edge = kw == 0 || 2 * kw == W;
        const float ar = t[0], ai = edge ? 0.f : t[32];
        const float br = two ? t[64] : 0.f, bi = (two && !edge) ? t[96] : 0.f;
        ln.put(kw, c, ar - bi, ai + br);
        if (!edge) ln.put(W - kw, c, ar + bi, br - ai);
    }
    ln.pad();
    ln.run();
    const float sc = rsqrtf((float)W);
    const long long pix0 = (long long)(b * H + h) * W;
    for (int e = threadIdx.x; e < W * GCG; e += blockDim.x) {
        const int w = e / GCG, c = e % GCG;
        float vr, vi;
        ln.get(w, c, vr, vi);
        for (int rr = 0; rr < (two ? 2 : 1); ++rr) {
            const long long px = pix0 + (long long)rr * W + w;
            float o = (rr ? vi : vr) * sc;
            if (add1) o += add1[px * add1_ld + g * GCG + c];
            if (add2) o += add2[px * add2_ld + g * GCG + c];
            out[px * out_ld + g * GCG + c] = o;
        }
    }
}

template <typename K>
int set_lds_gen(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return MTD_OK;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e == hipSuccess ? MTD_OK : (int)e;
}

inline size_t line_lds_bytes(const GenPlan& p) { return gen_lds_floats(p.len, GCG) * 4; }

// the plans of both axes and the workspace split: [filter of W][filter of H]
struct GenPlans {
    GenPlan w, h;
    size_t ws;
};

bool make_plans(int B, int H, int W, GenPlans& ps) {
    if (B <= 0 || B > 65535 || !make_plan(W, ps.w) || !make_plan(H, ps.h)) return false;
    ps.ws = filter_bytes(ps.w) + filter_bytes(ps.h) + 256;
    return true;
}

int launch_filter(const GenPlan& p, float2* filt, hipStream_t s) {
    if (!p.blue) return MTD_OK;
    hipLaunchKernelGGL(bluestein_filter_kernel, dim3(1), dim3(GNT), gen_lds_floats(p.len, 1) * 4, s, dev_plan(p), filt);
    return MTD_OK;
}

}  // namespace

extern "C" size_t mtd_spectral_gen_ws_bytes(int B, int H, int W) {
    GenPlans ps;
    return make_plans(B, H, W, ps) ? ps.ws : 0;
}

extern "C" int mtd_spectral_gen_plan(int n, int* out) {
    GenPlan p;
    if (!out || !make_plan(n, p)) return MTD_EINVAL;
    out[0] = p.blue ? p.len : 0;
    for (int s = 0; s < p.nst; ++s) out[1 + s] = p.rad[s];
    return p.nst;
}

extern "C" int mtd_rfft_rows_gen(const float* x, int x_ld, float* R, int B, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    GenPlans ps;
    if (!x || !R || !ws || x_ld < 32 || !make_plans(B, H, W, ps) || ws_bytes < ps.ws) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    float2* filt = reinterpret_cast<float2*>(ws);
    const size_t lds = line_lds_bytes(ps.w);
    int rc = set_lds_gen(rfft_rows_gen_kernel, lds);
    if (rc != MTD_OK) return rc;
    launch_filter(ps.w, filt, s);
    hipLaunchKernelGGL(rfft_rows_gen_kernel, dim3(32 / GCG, (H + 1) / 2, B), dim3(GNT), lds, s, x, x_ld, R, H, dev_plan(ps.w), (const float2*)filt);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_spec_mix_gen(const float* R, const float* w2t, const float* b2, float* T, int B, int H, int W, void* ws,
                                size_t ws_bytes, void* stream) {
    GenPlans ps;
    if (!R || !w2t || !b2 || !T || !ws || !make_plans(B, H, W, ps) || ws_bytes < ps.ws) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    float2* filt = reinterpret_cast<float2*>(reinterpret_cast<char*>(ws) + filter_bytes(ps.w));
    const size_t lds = line_lds_bytes(ps.h);
    int rc = set_lds_gen(cols_gen_kernel<false>, lds);
    if (rc == MTD_OK) rc = set_lds_gen(cols_gen_kernel<true>, lds);
    if (rc != MTD_OK) return rc;
    launch_filter(ps.h, filt, s);
    const int nkw = W / 2 + 1;
    const dim3 grid(32 / GCG, nkw, B);
    hipLaunchKernelGGL(cols_gen_kernel<false>, grid, dim3(GNT), lds, s, R, T, W, dev_plan(ps.h), (const float2*)filt);
    const long long nrows = (long long)B * nkw * H;
    hipLaunchKernelGGL(mix_gen_kernel, dim3((unsigned)((nrows + 63) / 64)), dim3(GNT), 0, s, T, w2t, b2, nrows);
    hipLaunchKernelGGL(cols_gen_kernel<true>, grid, dim3(GNT), lds, s, (const float*)T, T, W, dev_plan(ps.h), (const float2*)filt);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_irfft_rows_gen(const float* T, float* out, int out_ld, const float* add1, int add1_ld, const float* add2,
                                  int add2_ld, int B, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    GenPlans ps;
    if (!T || !out || !ws || out_ld < 32 || !make_plans(B, H, W, ps) || ws_bytes < ps.ws) return MTD_EINVAL;
    if ((add1 && add1_ld < 32) || (add2 && add2_ld < 32)) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    float2* filt = reinterpret_cast<float2*>(ws);
    const size_t lds = line_lds_bytes(ps.w);
    int rc = set_lds_gen(irfft_rows_gen_kernel, lds);
    if (rc != MTD_OK) return rc;
    launch_filter(ps.w, filt, s);
    hipLaunchKernelGGL(irfft_rows_gen_kernel, dim3(32 / GCG, (H + 1) / 2, B), dim3(GNT), lds, s, T, out, out_ld, add1, add1_ld, add2,
                       add2_ld, H, dev_plan(ps.w), (const float2*)filt);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
