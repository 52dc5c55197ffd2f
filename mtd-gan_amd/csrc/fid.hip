// The Frechet distance of the test loop (reference module/piq/fid.py, used by metrics.py:33-41 and engine.py:179-181) on the
// device, float64 throughout: mean and centred covariance of a feature set, and
//     d^2 = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2)
// with the Newton-Schulz square root of fid.py:42-61 and its data-dependent stop.  DESIGN 3.8.
//
//   fid_mma_kernel<OP, EPI>  the one matrix-pipe kernel: a 64 x 64 tile of the result per workgroup of four waves, each wave a
//                          32 x 32 quarter as 2 x 2 v_mfma_f64_16x16x4_f64 blocks (A operand: row = lane & 15, k = lane >> 4; B:
//                          k = lane >> 4, column = lane & 15; C/D: column = lane & 15, row = (lane >> 4) + 4 * register -- NOT the
//                          map of the other MFMA shapes).  Sixteen k per stage through LDS as [k][row | column]: an operand read
//                          is 16 consecutive doubles per k; the rows carry 16 doubles of padding so that the four k of a read fall
//                          on both halves of the banks.  The next stage's global loads are issued before the MFMAs of this one.
//                          Every global access is index-checked: rows, columns and k beyond the matrix read as 0 and are not
//                          written, so no size is special and no buffer is padded.
//                            OP_MAT    C = A . B of row-major D x D doubles
//                            OP_COV    C = Xc^T . Xc, Xc = (double)X - mu of the (N, D) fp32 features: the centring happens on the
//                                      way into LDS, the centred matrix never reaches memory; k runs over the N samples
//                            EPI_STORE     C = alpha * acc + beta_eye * I
//                            EPI_RESIDUAL  sum over the tile of (R - s * acc)^2, R a D x D matrix: the difference is never
//                                          stored; one partial per workgroup
//   sum kernels            Frobenius norm, traces, |mu1 - mu2|^2, the residual's partials: per-thread strided sums, then a
//                          tree over the workgroup, then (where several workgroups took part) one workgroup over the partials in
//                          index order.  No floating-point atomics anywhere, so a second call gives the same bits.
//   the iteration          every launch of a round reads the state word first and returns when "done" is set; the round's last
//                          launch (one workgroup) finishes the residual, forms err, the trace of the square root and the round
//                          count, and sets "done" when err <= 1e-5.  The host enqueues max_iters rounds and never reads back in
//                          between.
#include "gram64.h"          // f64x4

namespace {

constexpr int FT = 64;                  // tile side
constexpr int FK = 16;                  // k per stage
constexpr int FLD = FT + 16;            // LDS row length in doubles
constexpr int FID_RED_BLOCKS = 256;     // workgroups of a many-workgroup sum

enum { OP_MAT = 0, OP_COV = 1 };
enum { EPI_STORE = 0, EPI_RESIDUAL = 1 };

// state words (ints) and scalars (doubles) at the front of the workspace
enum { ST_DONE = 0, ST_ITERS = 1, ST_NONFINITE = 2, ST_WORDS = 16 };
enum { SC_NORM = 0, SC_ERR = 1, SC_TRS = 2, SC_BASE = 3, SC_WORDS = 8 };

struct FidWs {
    int* state;
    double* scal;
    double* partial;         // max(FID_RED_BLOCKS, tiles^2) doubles
    double* mat[6];          // M, Y0, Y1, Z0, Z1, T
};

inline long long fid_tiles(int D) { return (D + FT - 1) / FT; }
inline size_t fid_partials(int D) {
    const long long t = fid_tiles(D) * fid_tiles(D);
    return (size_t)(t > FID_RED_BLOCKS ? t : FID_RED_BLOCKS);
}
inline size_t fid_head_bytes(int D) {
    size_t b = ST_WORDS * sizeof(int) + SC_WORDS * sizeof(double) + fid_partials(D) * sizeof(double);
    return (b + 255) & ~(size_t)255;
}
inline FidWs fid_carve(void* ws, int D) {
    FidWs w;
    char* p = (char*)ws;
    w.state = (int*)p;
    w.scal = (double*)(p + ST_WORDS * sizeof(int));
    w.partial = w.scal + SC_WORDS;
    double* m = (double*)(p + fid_head_bytes(D));
    for (int i = 0; i < 6; ++i) w.mat[i] = m + (size_t)i * D * D;
    return w;
}

struct MmaArgs {
    const double* A;         // OP_MAT: left factor
    const double* B;         // OP_MAT: right factor
    const float* X;          // OP_COV: features (N, D)
    const double* mu;        // OP_COV: column means
    double* C;               // EPI_STORE
    const double* R;         // EPI_RESIDUAL: the matrix the scaled product is taken from
    double* partial;         // EPI_RESIDUAL
    const double* s_dev;     // EPI_RESIDUAL: the scale on the device (NULL: s_host)
    double s_host;
    double alpha, beta_eye;  // EPI_STORE
    const int* state;        // NULL, or the iteration's state: nothing happens once state[ST_DONE] is set
    int D;                   // side of the result
    int K;                   // length of the sum: D (OP_MAT), N (OP_COV)
};

template <int OP>
__device__ __forceinline__ void fid_fetch(const MmaArgs& a, int m0, int n0, int k0, double (&ra)[4], double (&rb)[4]) {
    const int tid = threadIdx.x;
    if (OP == OP_MAT) {
        // A: 64 rows x 16 k, four consecutive k of one row per thread
        const int m = m0 + (tid >> 2), kb = k0 + (tid & 3) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) ra[q] = (m < a.D && kb + q < a.K) ? a.A[(long long)m * a.D + kb + q] : 0.0;
        // B: 16 k x 64 columns, four consecutive columns of one k per thread
        const int k = k0 + (tid >> 4), nb = n0 + (tid & 15) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) rb[q] = (k < a.K && nb + q < a.D) ? a.B[(long long)k * a.D + nb + q] : 0.0;
    } else {
        // both operands are column ranges of the centred features: 16 samples x 64 columns each
        const int k = k0 + (tid >> 4), c = (tid & 15) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ma = m0 + c + q, nb = n0 + c + q;
            ra[q] = (k < a.K && ma < a.D) ? (double)a.X[(long long)k * a.D + ma] - a.mu[ma] : 0.0;
            rb[q] = (k < a.K && nb < a.D) ? (double)a.X[(long long)k * a.D + nb] - a.mu[nb] : 0.0;
        }
    }
}

template <int OP>
__device__ __forceinline__ void fid_stage(double (*As)[FLD], double (*Bs)[FLD], const double (&ra)[4], const double (&rb)[4]) {
    const int tid = threadIdx.x;
    if (OP == OP_MAT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) As[(tid & 3) * 4 + q][tid >> 2] = ra[q];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) As[tid >> 4][(tid & 15) * 4 + q] = ra[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) Bs[tid >> 4][(tid & 15) * 4 + q] = rb[q];
}

template <int OP, int EPI>
__global__ __launch_bounds__(256) void fid_mma_kernel(MmaArgs a) {
    if (a.state && a.state[ST_DONE]) return;
    __shared__ double As[FK][FLD];
    __shared__ double Bs[FK][FLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * FT, n0 = blockIdx.x * FT;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l15 = lane & 15, l4 = lane >> 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    double ra[4], rb[4];
    fid_fetch<OP>(a, m0, n0, 0, ra, rb);
    for (int k0 = 0; k0 < a.K; k0 += FK) {
        __syncthreads();                               // the stage before has been read
        fid_stage<OP>(As, Bs, ra, rb);
        __syncthreads();
        if (k0 + FK < a.K) fid_fetch<OP>(a, m0, n0, k0 + FK, ra, rb);
#pragma unroll
        for (int kk = 0; kk < FK; kk += 4) {
            const double a0 = As[kk + l4][wm + l15], a1 = As[kk + l4][wm + 16 + l15];
            const double b0 = Bs[kk + l4][wn + l15], b1 = Bs[kk + l4][wn + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    double sum = 0.0;
    const double s = EPI == EPI_RESIDUAL ? (a.s_dev ? a.s_dev[0] : a.s_host) : 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + i * 16 + l4 + 4 * r, col = n0 + wn + j * 16 + l15;
                if (row < a.D && col < a.D) {
                    const long long at = (long long)row * a.D + col;
                    if (EPI == EPI_STORE) {
                        a.C[at] = a.alpha * acc[i][j][r] + (row == col ? a.beta_eye : 0.0);
                    } else {
                        const double d = a.R[at] - s * acc[i][j][r];
                        sum += d * d;
                    }
                }
            }
    if (EPI == EPI_RESIDUAL) {
        __syncthreads();
        double* red = &As[0][0];                        // FK * FLD >= 256 doubles
        const double t = block_sum256(sum, red);
        if (tid == 0) a.partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}

// ---- statistics ---------------------------------------------------------------------------------------------------------
// mean of each column, the samples in index order
__global__ __launch_bounds__(256) void fid_mean_kernel(const float* __restrict__ X, int N, int D, double* __restrict__ mu) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D) return;
    double s = 0.0;
    for (int i = 0; i < N; ++i) s += (double)X[(long long)i * D + j];
    mu[j] = s / (double)N;
}

// ---- sums ---------------------------------------------------------------------------------------------------------------
// partial[b] = sum of squares of the elements b * 256 + t, + 256 * blocks, ... of M (fixed assignment)
__global__ __launch_bounds__(256) void fid_sumsq_kernel(const double* __restrict__ M, long long n, double* __restrict__ partial) {
    __shared__ double red[256];
    double s = 0.0;
    const long long step = (long long)gridDim.x * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += step) s += M[e] * M[e];
    const double t = block_sum256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// One workgroup: |M|_F from the partials, |mu1 - mu2|^2 + tr S1 + tr S2, and the state of a fresh solve.
__global__ __launch_bounds__(256) void fid_setup_kernel(const double* __restrict__ partial, int nparts, const double* __restrict__ mu1,
                                                        const double* __restrict__ s1, const double* __restrict__ mu2,
                                                        const double* __restrict__ s2, int D, int* __restrict__ state,
                                                        double* __restrict__ scal) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double p = 0.0, dm = 0.0, t1 = 0.0, t2 = 0.0;
    for (int i = tid; i < nparts; i += 256) p += partial[i];
    for (int i = tid; i < D; i += 256) {
        const double d = mu1[i] - mu2[i];
        dm += d * d;
        t1 += s1[(long long)i * D + i];
        t2 += s2[(long long)i * D + i];
    }
    p = block_sum256(p, red);
    __syncthreads();
    dm = block_sum256(dm, red);
    __syncthreads();
    t1 = block_sum256(t1, red);
    __syncthreads();
    t2 = block_sum256(t2, red);
    if (tid == 0) {
        scal[SC_NORM] = sqrt(p);
        scal[SC_ERR] = 0.0;
        scal[SC_TRS] = 0.0;
        scal[SC_BASE] = dm + t1 + t2;                  // fid.py:91, left to right
        state[ST_DONE] = 0;
        state[ST_ITERS] = 0;
        state[ST_NONFINITE] = 0;
    }
}

// Y0 = M / |M|_F, Z0 = I
__global__ __launch_bounds__(256) void fid_start_kernel(const double* __restrict__ M, const double* __restrict__ scal, int D,
                                                        double* __restrict__ Y, double* __restrict__ Z) {
    const long long n = (long long)D * D, step = (long long)gridDim.x * 256;
    const double norm = scal[SC_NORM];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += step) {
        Y[e] = M[e] / norm;
        Z[e] = (e / D == e % D) ? 1.0 : 0.0;
    }
}

// out = in + offset * I
__global__ __launch_bounds__(256) void fid_offset_kernel(const double* __restrict__ in, double offset, int D, double* __restrict__ out) {
    const long long n = (long long)D * D, step = (long long)gridDim.x * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += step)
        out[e] = in[e] + ((e / D == e % D) ? offset : 0.0);
}

// The last launch of a round, one workgroup: err = |M - S S|_F / |M|_F from the residual's partials, tr S = sqrt(|M|_F) tr Y,
// the round count, and the stop (fid.py:56-59: isclose(err, 0, atol = 1e-5) is err <= 1e-5; a NaN never stops).
__global__ __launch_bounds__(256) void fid_round_kernel(const double* __restrict__ partial, int nparts, const double* __restrict__ Y, int D,
                                                        int round, int* __restrict__ state, double* __restrict__ scal) {
    if (state[ST_DONE]) return;
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double p = 0.0, tr = 0.0;
    for (int i = tid; i < nparts; i += 256) p += partial[i];
    for (int i = tid; i < D; i += 256) tr += Y[(long long)i * D + i];
    p = block_sum256(p, red);
    __syncthreads();
    tr = block_sum256(tr, red);
    if (tid == 0) {
        const double norm = scal[SC_NORM];
        const double err = sqrt(p) / norm;
        scal[SC_ERR] = err;
        scal[SC_TRS] = tr * sqrt(norm);
        state[ST_ITERS] = round;
        if (err <= 1e-5) state[ST_DONE] = 1;
    }
}

// isfinite(S).all() of fid.py:85 on S = Y sqrt(|M|_F), Y the iterate of the round the solve ended at (round r is in Yb[r & 1]).
// Every workgroup that meets a non-finite element stores the same 1: an integer flag, no ordering to depend on.
__global__ __launch_bounds__(256) void fid_finite_kernel(const double* __restrict__ Yb0, const double* __restrict__ Yb1, int D,
                                                         int* __restrict__ state, const double* __restrict__ scal) {
    const double* Y = (state[ST_ITERS] & 1) ? Yb1 : Yb0;
    const double rs = sqrt(scal[SC_NORM]);
    const long long n = (long long)D * D, step = (long long)gridDim.x * 256;
    bool bad = false;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += step) {
        const double v = Y[e] * rs;
        bad |= !(fabs(v) <= 1.7976931348623157e308);
    }
    if (bad) state[ST_NONFINITE] = 1;
}

__global__ void fid_result_kernel(const int* __restrict__ state, const double* __restrict__ scal, double* __restrict__ out,
                                  int* __restrict__ iters) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[0] = scal[SC_BASE] - 2 * scal[SC_TRS];
    out[1] = scal[SC_TRS];
    out[2] = scal[SC_ERR];
    out[3] = state[ST_NONFINITE] ? 0.0 : 1.0;
    iters[0] = state[ST_ITERS];
}

__global__ __launch_bounds__(256) void fid_finish_sum_kernel(const double* __restrict__ partial, int nparts, double* __restrict__ out) {
    __shared__ double red[256];
    double p = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) p += partial[i];
    p = block_sum256(p, red);
    if (threadIdx.x == 0) out[0] = p;
}

unsigned ew_blocks(long long n) {
    long long b = (n + 255) / 256;
    return (unsigned)(b > FID_RED_BLOCKS ? FID_RED_BLOCKS : b);
}

template <int OP, int EPI>
int launch_mma(const MmaArgs& a, hipStream_t s) {
    const unsigned t = (unsigned)fid_tiles(a.D);
    hipLaunchKernelGGL((fid_mma_kernel<OP, EPI>), dim3(t, t), dim3(256), 0, s, a);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

int gemm(const double* A, const double* B, double* C, int D, double alpha, double beta_eye, const int* state, hipStream_t s) {
    MmaArgs a = {};
    a.A = A; a.B = B; a.C = C; a.D = D; a.K = D; a.alpha = alpha; a.beta_eye = beta_eye; a.state = state;
    return launch_mma<OP_MAT, EPI_STORE>(a, s);
}

int residual(const double* R, const double* Y, const double* s_dev, double s_host, int D, double* partial, const int* state, hipStream_t s) {
    MmaArgs a = {};
    a.A = Y; a.B = Y; a.R = R; a.partial = partial; a.s_dev = s_dev; a.s_host = s_host; a.D = D; a.K = D; a.state = state;
    return launch_mma<OP_MAT, EPI_RESIDUAL>(a, s);
}

}  // namespace

#define FID_TRY(call)                  \
    do {                               \
        const int rc__ = (call);       \
        if (rc__ != MTD_OK) return rc__; \
    } while (0)

extern "C" size_t mtd_fid_ws_bytes(int D) {
    if (D < 1 || D > 16384) return 0;
    return fid_head_bytes(D) + (size_t)6 * D * D * sizeof(double);
}

extern "C" int mtd_fid_stats(const float* X, int N, int D, double* mu, double* sigma, void* ws, void* stream) {
    (void)ws;                                          // the statistics need no scratch; the argument keeps the family's shape
    if (!X || !mu || !sigma || N < 2 || D < 1 || D > 16384) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fid_mean_kernel, dim3((D + 255) / 256), dim3(256), 0, s, X, N, D, mu);
    MTD_LAUNCH_CHECK();
    MmaArgs a = {};
    a.X = X; a.mu = mu; a.C = sigma; a.D = D; a.K = N; a.alpha = 1.0 / (double)(N - 1); a.beta_eye = 0.0;
    return launch_mma<OP_COV, EPI_STORE>(a, s);
}

extern "C" int mtd_fid_gemm(const double* A, const double* B, double* C, int D, double alpha, double beta_eye, void* stream) {
    if (!A || !B || !C || D < 1 || D > 16384) return MTD_EINVAL;
    return gemm(A, B, C, D, alpha, beta_eye, nullptr, (hipStream_t)stream);
}

extern "C" int mtd_fid_residual(const double* A, const double* Y, double scale, int D, double* out, void* ws, void* stream) {
    if (!A || !Y || !out || !ws || D < 1 || D > 16384) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const FidWs w = fid_carve(ws, D);
    FID_TRY(residual(A, Y, nullptr, scale, D, w.partial, nullptr, s));
    hipLaunchKernelGGL(fid_finish_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)w.partial, (int)(fid_tiles(D) * fid_tiles(D)), out);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_fid_distance(const double* mu1, const double* s1, const double* mu2, const double* s2, int D, double offset,
                                int max_iters, double* out, int* iters, void* ws, void* stream) {
    if (!mu1 || !s1 || !mu2 || !s2 || !out || !iters || !ws || D < 1 || D > 16384 || max_iters <= 0) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const FidWs w = fid_carve(ws, D);
    double* M = w.mat[0];
    double* Yb[2] = {w.mat[1], w.mat[2]};
    double* Zb[2] = {w.mat[3], w.mat[4]};
    double* T = w.mat[5];
    const long long n = (long long)D * D;
    const unsigned eb = ew_blocks(n);
    const int tiles2 = (int)(fid_tiles(D) * fid_tiles(D));
    const double *p1 = s1, *p2 = s2;
    if (offset != 0.0) {                               // fid.py:87-88; the two slots are not written before round 1
        hipLaunchKernelGGL(fid_offset_kernel, dim3(eb), dim3(256), 0, s, s1, offset, D, Yb[1]);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(fid_offset_kernel, dim3(eb), dim3(256), 0, s, s2, offset, D, Zb[1]);
        MTD_LAUNCH_CHECK();
        p1 = Yb[1];
        p2 = Zb[1];
    }
    FID_TRY(gemm(p1, p2, M, D, 1.0, 0.0, nullptr, s));
    hipLaunchKernelGGL(fid_sumsq_kernel, dim3(eb), dim3(256), 0, s, (const double*)M, n, w.partial);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(fid_setup_kernel, dim3(1), dim3(256), 0, s, (const double*)w.partial, (int)eb, mu1, s1, mu2, s2, D, w.state, w.scal);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(fid_start_kernel, dim3(eb), dim3(256), 0, s, (const double*)M, (const double*)w.scal, D, Yb[0], Zb[0]);
    MTD_LAUNCH_CHECK();
    for (int r = 1; r <= max_iters; ++r) {
        const double *Y = Yb[(r - 1) & 1], *Z = Zb[(r - 1) & 1];
        double *Yn = Yb[r & 1], *Zn = Zb[r & 1];
        FID_TRY(gemm(Z, Y, T, D, -0.5, 1.5, w.state, s));                    // T = 0.5 (3 I - Z Y)
        FID_TRY(gemm(Y, T, Yn, D, 1.0, 0.0, w.state, s));
        FID_TRY(gemm(T, Z, Zn, D, 1.0, 0.0, w.state, s));
        FID_TRY(residual(M, Yn, w.scal + SC_NORM, 0.0, D, w.partial, w.state, s));      // S S = |M|_F (Y Y)
        hipLaunchKernelGGL(fid_round_kernel, dim3(1), dim3(256), 0, s, (const double*)w.partial, tiles2, (const double*)Yn, D, r, w.state, w.scal);
        MTD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(fid_finite_kernel, dim3(eb), dim3(256), 0, s, (const double*)Yb[0], (const double*)Yb[1], D, w.state, (const double*)w.scal);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(fid_result_kernel, dim3(1), dim3(64), 0, s, (const int*)w.state, (const double*)w.scal, out, iters);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
