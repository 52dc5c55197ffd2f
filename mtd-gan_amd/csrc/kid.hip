// The Kernel Inception Distance (reference module/piq/kid.py) on the device, float64 throughout: the polynomial-kernel MMD^2
// estimate between two feature sets and its variance estimate, per subset and averaged over the subsets.  DESIGN 3.15.
//     K(A, B) = (gamma A B^T + coef0)^degree,   mmd2 = (Kt_XX_sum + Kt_YY_sum) / (m (m - 1)) - 2 K_XY_sum / m^2   (unbiased)
// The three m x m kernel matrices of a subset are never stored: every 64 x 64 tile is reduced where it is computed.
//
//   kid_gram_sums_kernel   one workgroup of four waves per 64 x 64 tile of one kernel matrix of one subset (grid x, y: the tile;
//                          grid z = 3 * subset + matrix, matrix 0 = XX, 1 = YY, 2 = XY).  Tile shape, operand maps and LDS
//                          layout are those of fid_mma_kernel (fid.hip; its header has the f64 MFMA lane map).  The product is
//                          NT: both operands are rows of (N, D) fp32 features with k = D contiguous, addressed through the
//                          subset's index table (row = idx[s][i]); a thread fetches four consecutive k of one row (one 16-byte
//                          load where D and the base allow, value by value otherwise) and widens them on the way into LDS.
//                          Rows beyond m, k beyond D and rows whose index lies outside the matrix read as 0.  Epilogue per
//                          element: t = gamma acc + coef0, t^degree by repeated multiplication; then per tile the 64 row sums,
//                          the 64 column sums and the sum of squares (for XX and YY without the diagonal) and the diagonal's
//                          sum and sum of squares (for XY: its trace), to the workspace record of (subset, matrix, tile).
//                          The sums over a row's 32 columns inside a wave are four xor-shuffles in a fixed order, the two
//                          waves that share a row meet in LDS; likewise the columns.
//   kid_finish_kernel      one workgroup per subset: adds the tile partials of each row / column in tile-index order (the four
//                          vectors Kt_XX_sums, Kt_YY_sums, K_XY_sums_1, K_XY_sums_0 live in registers only), their sums, squared
//                          norms and the two dot products by per-thread strided sums and the workgroup's halving tree, then
//                          mmd2 and var_est in kid.py's order of operations.
//   kid_mean_kernel        the means over the subsets, in subset order.
// No floating-point atomics anywhere: a second call gives the same bits, and a subset's values depend neither on its place
// among the S subsets nor on S.
#include "gram64.h"          // f64x4, gram64_fetch

namespace {

constexpr int KT = 64;                  // tile side
constexpr int KK = 16;                  // k per stage
constexpr int KLD = KT + 16;            // LDS row length in doubles
constexpr int KREC = 2 * KT + 4;        // a tile's record: 64 row sums, 64 column sums, sum of squares, diagonal sum, diagonal sum of squares, 0
static_assert(KREC == MTD_KID_TILE_REC, "the header documents the workspace by this record length");
constexpr int KID_MAX_M = 1 << 20;
constexpr int KID_SUMS = 17;            // the sums the finish kernel reduces over the workgroup

struct KidArgs {
    const float* X;
    const float* Y;
    const int* xi;
    const int* yi;
    double* ws;
    double gamma, coef0;
    int Nx, Ny, D, m, degree;
};

inline long long kid_tiles(int m) { return (m + KT - 1) / KT; }

__global__ __launch_bounds__(256) void kid_gram_sums_kernel(KidArgs a) {
    __shared__ double As[KK][KLD];
    __shared__ double Bs[KK][KLD];
    __shared__ double part[2][2][KT];                 // [rows | columns][which of the two waves][index in the tile]
    __shared__ double red[3 * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.z / 3, mat = blockIdx.z % 3;
    const int m0 = blockIdx.y * KT, n0 = blockIdx.x * KT;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l15 = lane & 15, l4 = lane >> 4;
    const float* FA = mat == 1 ? a.Y : a.X;
    const float* FB = mat == 0 ? a.X : a.Y;
    const int* ia = (mat == 1 ? a.yi : a.xi) + (long long)s * a.m;
    const int* ib = (mat == 0 ? a.xi : a.yi) + (long long)s * a.m;
    const int NA = mat == 1 ? a.Ny : a.Nx, NB = mat == 0 ? a.Nx : a.Ny;
    // the feature row this thread stages for each operand: tile row tid >> 2, k group tid & 3
    int rowa = -1, rowb = -1;
    if (m0 + (tid >> 2) < a.m) {
        const int r = ia[m0 + (tid >> 2)];
        rowa = (r >= 0 && r < NA) ? r : -1;
    }
    if (n0 + (tid >> 2) < a.m) {
        const int r = ib[n0 + (tid >> 2)];
        rowb = (r >= 0 && r < NB) ? r : -1;
    }
    const bool veca = (a.D & 3) == 0 && ((uintptr_t)FA & 15) == 0, vecb = (a.D & 3) == 0 && ((uintptr_t)FB & 15) == 0;
    const int kq = (tid & 3) * 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    float ra[4], rb[4];
    gram64_fetch(FA, rowa, a.D, kq, veca, ra);
    gram64_fetch(FB, rowb, a.D, kq, vecb, rb);
    for (int k0 = 0; k0 < a.D; k0 += KK) {
        __syncthreads();                               // the stage before has been read
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            As[kq + q][tid >> 2] = (double)ra[q];
            Bs[kq + q][tid >> 2] = (double)rb[q];
        }
        __syncthreads();
        if (k0 + KK < a.D) {
            gram64_fetch(FA, rowa, a.D, k0 + KK + kq, veca, ra);
            gram64_fetch(FB, rowb, a.D, k0 + KK + kq, vecb, rb);
        }
#pragma unroll
        for (int kk = 0; kk < KK; kk += 4) {
            const double a0 = As[kk + l4][wm + l15], a1 = As[kk + l4][wm + 16 + l15];
            const double b0 = Bs[kk + l4][wn + l15], b1 = Bs[kk + l4][wn + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // ---- epilogue: the kernel values of this lane's 16 elements, reduced at once
    const bool drop_diag = mat != 2;
    double rs[2][4], cs[2] = {0.0, 0.0}, sq = 0.0, dsum = 0.0, dsq = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rs[i][r] = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + i * 16 + l4 + 4 * r, col = n0 + wn + j * 16 + l15;
                double v = 0.0;
                if (row < a.m && col < a.m) {
                    const double t = a.gamma * acc[i][j][r] + a.coef0;
                    v = t;
                    for (int d = 1; d < a.degree; ++d) v *= t;
                    if (row == col) {
                        dsum += v;
                        dsq += v * v;
                        if (drop_diag) v = 0.0;
                    }
                }
                rs[i][r] += v;
                cs[j] += v;
                sq += v * v;
            }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double x = rs[i][r];
            x += __shfl_xor(x, 1);
            x += __shfl_xor(x, 2);
            x += __shfl_xor(x, 4);
            x += __shfl_xor(x, 8);
            if (l15 == 0) part[0][wave & 1][wm + i * 16 + l4 + 4 * r] = x;
        }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        double x = cs[j];
        x += __shfl_xor(x, 16);
        x += __shfl_xor(x, 32);
        if (l4 == 0) part[1][wave >> 1][wn + j * 16 + l15] = x;
    }
    double three[3] = {sq, dsum, dsq};
    block_sum256(three, red);                          // (its barriers also publish `part`)
    double* rec = a.ws + (((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * KREC;
    if (tid < 2 * KT) rec[tid] = part[tid >> 6][0][tid & 63] + part[tid >> 6][1][tid & 63];
    if (tid == 0) {
        rec[2 * KT + 0] = three[0];
        rec[2 * KT + 1] = three[1];
        rec[2 * KT + 2] = three[2];
        rec[2 * KT + 3] = 0.0;
    }
}

// One workgroup per subset.  out2: (S, 2) [mmd2, var]; parts: NULL or (S, MTD_KID_PARTS).
__global__ __launch_bounds__(256) void kid_finish_kernel(const double* __restrict__ ws, int m, int mmd_est, int want_var, int var_at_m,
                                                         double* __restrict__ out2, double* __restrict__ parts) {
    __shared__ double red[KID_SUMS * 256];
    const int tid = threadIdx.x, s = blockIdx.x;
    const int T = (m + KT - 1) / KT;
    const long long TT = (long long)T * T;
    const double* wxx = ws + ((long long)s * 3 + 0) * TT * KREC;
    const double* wyy = ws + ((long long)s * 3 + 1) * TT * KREC;
    const double* wxy = ws + ((long long)s * 3 + 2) * TT * KREC;
    enum { XX_SUM, YY_SUM, XY_SUM, XX_SQN, YY_SQN, XY1_SQN, XY0_SQN, DOT_XX, DOT_YY, XX_2, YY_2, XY_2, DIAG_X, DIAG_Y, TRACE_XY, DIAG2_X, DIAG2_Y };
    double v[KID_SUMS];
#pragma unroll
    for (int k = 0; k < KID_SUMS; ++k) v[k] = 0.0;
    for (int i = tid; i < m; i += 256) {
        const int t = i >> 6, e = i & 63;
        double xx = 0.0, yy = 0.0, xy1 = 0.0, xy0 = 0.0;
        for (int u = 0; u < T; ++u) {                   // tile-index order
            const long long along_row = ((long long)t * T + u) * KREC + e;
            xx += wxx[along_row];
            yy += wyy[along_row];
            xy1 += wxy[along_row];
            xy0 += wxy[((long long)u * T + t) * KREC + KT + e];
        }
        v[XX_SUM] += xx;
        v[YY_SUM] += yy;
        v[XY_SUM] += xy0;                               // kid.py:95: K_XY_sums_0.sum()
        v[XX_SQN] += xx * xx;
        v[YY_SQN] += yy * yy;
        v[XY1_SQN] += xy1 * xy1;
        v[XY0_SQN] += xy0 * xy0;
        v[DOT_XX] += xx * xy1;
        v[DOT_YY] += yy * xy0;
    }
    for (long long e = tid; e < TT; e += 256) {
        v[XX_2] += wxx[e * KREC + 2 * KT];
        v[YY_2] += wyy[e * KREC + 2 * KT];
        v[XY_2] += wxy[e * KREC + 2 * KT];
    }
    for (int d = tid; d < T; d += 256) {
        const long long e = ((long long)d * T + d) * KREC + 2 * KT;
        v[DIAG_X] += wxx[e + 1];
        v[DIAG_Y] += wyy[e + 1];
        v[TRACE_XY] += wxy[e + 1];
        v[DIAG2_X] += wxx[e + 2];
        v[DIAG2_Y] += wyy[e + 2];
    }
    block_sum256(v, red);
    if (tid != 0) return;
    const double dm = (double)m, m1 = dm - 1.0, m2 = dm - 2.0;
    const double Kt_XX_sum = v[XX_SUM], Kt_YY_sum = v[YY_SUM], K_XY_sum = v[XY_SUM];
    double mmd2;
    if (mmd_est == MTD_KID_BIASED) {                    // kid.py:98
        mmd2 = (Kt_XX_sum + v[DIAG_X]) / (dm * dm) + (Kt_YY_sum + v[DIAG_Y]) / (dm * dm) - 2.0 * K_XY_sum / (dm * dm);
    } else {                                            // kid.py:101-105
        mmd2 = (Kt_XX_sum + Kt_YY_sum) / (dm * m1);
        if (mmd_est == MTD_KID_UNBIASED) mmd2 -= 2.0 * K_XY_sum / (dm * dm);
        else mmd2 -= 2.0 * (K_XY_sum - v[TRACE_XY]) / (dm * m1);
    }
    double zeta1 = 0.0, zeta2 = 0.0, var = 0.0;
    if (want_var) {                                     // kid.py:110-138, term by term and left to right
        const double Kt_XX_2_sum = v[XX_2], Kt_YY_2_sum = v[YY_2], K_XY_2_sum = v[XY_2];
        const double dot_XX_XY = v[DOT_XX], dot_YY_YX = v[DOT_YY];
        const double mm1 = dm * m1, sq_sums = Kt_XX_sum * Kt_XX_sum + Kt_YY_sum * Kt_YY_sum;
        zeta1 = 1.0 / (dm * m1 * m2) * (v[XX_SQN] - Kt_XX_2_sum + v[YY_SQN] - Kt_YY_2_sum)
              - 1.0 / (mm1 * mm1) * sq_sums
              + 1.0 / (dm * dm * m1) * (v[XY1_SQN] + v[XY0_SQN] - 2.0 * K_XY_2_sum)
              - 2.0 / (dm * dm * dm * dm) * (K_XY_sum * K_XY_sum)
              - 2.0 / (dm * dm * m1) * (dot_XX_XY + dot_YY_YX)
              + 2.0 / (dm * dm * dm * m1) * (Kt_XX_sum + Kt_YY_sum) * K_XY_sum;
        zeta2 = 1.0 / mm1 * (Kt_XX_2_sum + Kt_YY_2_sum)
              - 1.0 / (mm1 * mm1) * sq_sums
              + 2.0 / (dm * dm) * K_XY_2_sum
              - 2.0 / (dm * dm * dm * dm) * (K_XY_sum * K_XY_sum)
              - 4.0 / (dm * dm * m1) * (dot_XX_XY + dot_YY_YX)
              + 4.0 / (dm * dm * dm * m1) * (Kt_XX_sum + Kt_YY_sum) * K_XY_sum;
        const double vm = (double)var_at_m, vv = vm * (vm - 1.0);
        var = 4.0 * (vm - 2.0) / vv * zeta1 + 2.0 / vv * zeta2;
    }
    out2[2 * s] = mmd2;
    out2[2 * s + 1] = var;
    if (parts) {
        double* p = parts + (long long)s * MTD_KID_PARTS;
        p[0] = Kt_XX_sum; p[1] = Kt_YY_sum; p[2] = K_XY_sum;
        p[3] = v[DIAG_X]; p[4] = v[DIAG_Y]; p[5] = v[TRACE_XY];
        p[6] = v[DIAG2_X]; p[7] = v[DIAG2_Y];
        p[8] = v[XX_2]; p[9] = v[YY_2]; p[10] = v[XY_2];
        p[11] = v[XX_SQN]; p[12] = v[YY_SQN]; p[13] = v[XY1_SQN]; p[14] = v[XY0_SQN];
        p[15] = v[DOT_XX]; p[16] = v[DOT_YY];
        p[17] = zeta1; p[18] = zeta2; p[19] = mmd2; p[20] = var;
    }
}

// out[0], out[1] = the means of the (S, 2) table behind them, the subsets in order
__global__ void kid_mean_kernel(double* __restrict__ out, int S) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a = 0.0, b = 0.0;
    for (int s = 0; s < S; ++s) {
        a += out[2 + 2 * s];
        b += out[3 + 2 * s];
    }
    out[0] = a / (double)S;
    out[1] = b / (double)S;
}

bool kid_sizes_ok(int m, int S) { return m >= 2 && m <= KID_MAX_M && S >= 1 && 3LL * S <= 65535; }

}  // namespace

extern "C" size_t mtd_kid_ws_bytes(int m, int S) {
    if (!kid_sizes_ok(m, S)) return 0;
    return (size_t)S * 3 * (size_t)(kid_tiles(m) * kid_tiles(m)) * KREC * sizeof(double);
}

extern "C" int mtd_kid(const float* X, int Nx, const float* Y, int Ny, int D, const int* xi, const int* yi, int m, int S, int degree,
                       double gamma, double coef0, int mmd_est, int want_var, int var_at_m, double* out, double* parts, void* ws,
                       void* stream) {
    if (!X || !Y || !xi || !yi || !out || !ws) return MTD_EINVAL;
    if (!kid_sizes_ok(m, S) || D < 1 || degree < 1 || degree > 8 || m > Nx || m > Ny) return MTD_EINVAL;
    if (mmd_est != MTD_KID_UNBIASED && mmd_est != MTD_KID_BIASED && mmd_est != MTD_KID_USTAT) return MTD_EINVAL;
    if (want_var && (m < 3 || var_at_m < 2)) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    KidArgs a = {};
    a.X = X; a.Y = Y; a.xi = xi; a.yi = yi; a.ws = (double*)ws; a.gamma = gamma; a.coef0 = coef0;
    a.Nx = Nx; a.Ny = Ny; a.D = D; a.m = m; a.degree = degree;
    const unsigned t = (unsigned)kid_tiles(m);
    hipLaunchKernelGGL(kid_gram_sums_kernel, dim3(t, t, 3 * S), dim3(256), 0, s, a);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(kid_finish_kernel, dim3(S), dim3(256), 0, s, (const double*)ws, m, mmd_est, want_var ? 1 : 0, var_at_m, out + 2, parts);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(kid_mean_kernel, dim3(1), dim3(64), 0, s, out, S);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
