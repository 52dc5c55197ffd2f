// The Multi-Scale Intrinsic Distance (reference module/piq/msid.py) and the Inception Score (module/piq/isc.py) on the device,
// float64 arithmetic on (N, D) fp32 feature rows.  DESIGN 3.20.  MSID's descriptor of one feature set, stage by stage:
//
//   neighbours   msid_sqnorm_kernel: dd[j] = |X[j]|^2, one wave per row.  Then per panel of P rows (P * N doubles, at most
//                MSID_PANEL_BYTES: the N x N matrix is never held whole) msid_dist_kernel: dist[i][j] = dd[j] - 2 Xi . Xj, the
//                products on v_mfma_f64_16x16x4_f64 with the tile shape, operand maps and LDS layout of kid_gram_sums_kernel
//                (kid.hip), and msid_select_kernel: one wave per row takes the k + 1 smallest of its row in k + 1 rounds, each
//                the smallest (value, index) pair after the pair of the round before -- a running selection, not a sort; ties
//                go to the lower index; NaN is never taken (a row short of candidates is filled with -1).
//   graph        an N x ceil(N / 32) bit mask, zeroed, takes bit (i, j) and bit (j, i) of every neighbour j != i of every row i
//                (atomicOr on words: idempotent, so the order does not matter); a row's popcount is its degree, one workgroup
//                scans the degrees to the CSR offsets, one wave per row writes its set bits as sorted columns.
//   Lanczos      msid.py's _lanczos_m on nv starting vectors at once.  V is (m, N, nv): a neighbour's nv values are contiguous.
//                A workgroup of 256 threads owns a chunk of rows and 64 columns (thread = column x one of four row lanes); every
//                column dot product is two-stage in a fixed order: the thread's rows in order, the four row lanes in order (LDS),
//                to the chunk's slot in `part`; then the chunks in order.  The two global conditions live in words on the device:
//                more[i][p] (some innerprod of step i exceeded 1e-5 after p extra passes; written by the reduce kernel with
//                atomicOr on a zeroed word, read at entry by the kernels of pass p + 1) and stopped[i] (step i does not run;
//                stopped[i + 1] is written by the one kernel that stores V[i + 1], which itself reads stopped[i]).  No kernel
//                waits for another workgroup; the number of launches depends on m alone.
//   quadrature   one thread per starting vector: implicit QL on the m x m tridiagonal, carrying the first row of the
//                eigenvector matrix only; then sum_j f(-t lambda_j) v_0j^2 for every temperature and f = exp, identity; the
//                mean over the vectors in vector order.
//   descriptor   ((tr_exp - tr_id / exp_ts) + sub) / div * 1e6 with the three tables computed by the caller on the host.
// The distance of two descriptors: max c |dp - dt| or the l2 norm.  The Inception Score: one workgroup per split.
// No floating-point atomics anywhere: two calls on the same inputs give the same bits.
#include <limits.h>
#include "gram64.h"          // f64x4, gram64_fetch

namespace {

constexpr int MT = 64;                  // tile side of the distance product
constexpr int MK = 16;                  // k per stage
constexpr int MLD = MT + 16;            // LDS row length in doubles
constexpr long long MSID_PANEL_BYTES = 32LL << 20;
constexpr int MSID_MAX_N = MTD_MSID_MAX_N;
constexpr int MSID_MAX_M = 32;
constexpr int MSID_MAX_NV = 4096;
constexpr int MSID_MAX_TS = 65536;
constexpr int LZ_PASSES = 100;          // msid.py:120
constexpr int LZ_MAX_CHUNKS = 128;

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int msid_panel_rows(int N) {
    long long p = MSID_PANEL_BYTES / (8LL * N) / MT * MT;
    const long long all = ((long long)N + MT - 1) / MT * MT;
    if (p < MT) p = MT;
    return (int)(p < all ? p : all);
}
inline int lz_chunk_rows(int N) { return 64 * ((N + 64 * LZ_MAX_CHUNKS - 1) / (64 * LZ_MAX_CHUNKS)); }
inline int lz_chunks(int N) { return (N + lz_chunk_rows(N) - 1) / lz_chunk_rows(N); }
inline bool msid_graph_ok(int N, int k) { return k >= 1 && k <= 63 && N <= MSID_MAX_N && N >= k + 2; }      // (np.argpartition(dists, k + 1) needs k + 1 < N)
inline bool msid_lz_ok(int m, int nv) { return m >= 2 && m <= MSID_MAX_M && nv >= 1 && nv <= MSID_MAX_NV; }

// ------------------------------------------------------------------------------------------------------------ neighbours
__device__ __forceinline__ double wave_sum64(double x) {
    x += __shfl_xor(x, 1);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, 4);
    x += __shfl_xor(x, 8);
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
    return x;
}

__global__ __launch_bounds__(256) void msid_sqnorm_kernel(const float* __restrict__ X, int N, int D, double* __restrict__ dd) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* x = X + (long long)row * D;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = (double)x[d];
        s += v * v;
    }
    s = wave_sum64(s);
    if (lane == 0) dd[row] = s;
}

// dist[(i - row0) * N + j] = dd[j] - 2 Xi . Xj for row0 <= i < row0 + rows, 0 <= j < N.  grid (ceil(N / 64), ceil(rows / 64)).
__global__ __launch_bounds__(256) void msid_dist_kernel(const float* __restrict__ X, int N, int D, const double* __restrict__ dd, int row0,
                                                        int rows, double* __restrict__ dist) {
    __shared__ double As[MK][MLD];
    __shared__ double Bs[MK][MLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * MT, n0 = blockIdx.x * MT;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int ra_ = m0 + (tid >> 2), rb_ = n0 + (tid >> 2);
    const int rowa = ra_ < rows ? row0 + ra_ : -1, rowb = rb_ < N ? rb_ : -1;
    const bool vec = (D & 3) == 0 && ((uintptr_t)X & 15) == 0;
    const int kq = (tid & 3) * 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    float ra[4], rb[4];
    gram64_fetch(X, rowa, D, kq, vec, ra);
    gram64_fetch(X, rowb, D, kq, vec, rb);
    for (int k0 = 0; k0 < D; k0 += MK) {
        __syncthreads();                               // the stage before has been read
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            As[kq + q][tid >> 2] = (double)ra[q];
            Bs[kq + q][tid >> 2] = (double)rb[q];
        }
        __syncthreads();
        if (k0 + MK < D) {
            gram64_fetch(X, rowa, D, k0 + MK + kq, vec, ra);
            gram64_fetch(X, rowb, D, k0 + MK + kq, vec, rb);
        }
#pragma unroll
        for (int kk = 0; kk < MK; kk += 4) {
            const double a0 = As[kk + l4][wm + l15], a1 = As[kk + l4][wm + 16 + l15];
            const double b0 = Bs[kk + l4][wn + l15], b1 = Bs[kk + l4][wn + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + i * 16 + l4 + 4 * r, col = n0 + wn + j * 16 + l15;
                if (row < rows && col < N) dist[(long long)row * N + col] = dd[col] - 2.0 * acc[i][j][r];
            }
}

// One wave per row of the panel: nbr[(row0 + r) * k1 + s] = the index of the s-th smallest of dist[r][0..N), s < k1.
__global__ __launch_bounds__(256) void msid_select_kernel(const double* __restrict__ dist, int N, int row0, int rows, int k1, int* __restrict__ nbr) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const double* row = dist + (long long)r * N;
    int* out = nbr + (long long)(row0 + r) * k1;
    double pv = 0.0;
    int pj = -1;
    for (int s = 0; s < k1; ++s) {
        double bv = 0.0;
        int bj = INT_MAX;
        if (pj != INT_MAX) {
            for (int j = lane; j < N; j += 64) {
                const double v = row[j];
                const bool after = pj < 0 ? v == v : (v > pv || (v == pv && j > pj));
                if (after && (bj == INT_MAX || v < bv)) { bv = v; bj = j; }          // (j rises: an equal value keeps the lower index)
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double ov = __shfl_xor(bv, o);
                const int oj = __shfl_xor(bj, o);
                if (oj != INT_MAX && (bj == INT_MAX || ov < bv || (ov == bv && oj < bj))) { bv = ov; bj = oj; }
            }
        }
        if (lane == 0) out[s] = bj == INT_MAX ? -1 : bj;
        pv = bv;
        pj = bj;
    }
}

// ------------------------------------------------------------------------------------------------------------ graph
__global__ void msid_mask_kernel(const int* __restrict__ nbr, int N, int k1, int W, unsigned* __restrict__ mask) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)N * k1) return;
    const int i = (int)(e / k1), j = nbr[e];
    if (j < 0 || j >= N || j == i) return;
    atomicOr(&mask[(long long)i * W + (j >> 5)], 1u << (j & 31));
    atomicOr(&mask[(long long)j * W + (i >> 5)], 1u << (i & 31));
}

__global__ __launch_bounds__(256) void msid_degree_kernel(const unsigned* __restrict__ mask, int N, int W, int* __restrict__ deg) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    int c = 0;
    for (int w = lane; w < W; w += 64) c += __popc(mask[(long long)row * W + w]);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) c += __shfl_xor(c, o);
    if (lane == 0) deg[row] = c;
}

// one workgroup: rowptr[0..N] = the exclusive scan of deg[0..N)
__global__ __launch_bounds__(256) void msid_scan_kernel(const int* __restrict__ deg, int N, int* __restrict__ rowptr) {
    __shared__ int sums[256];
    const int tid = threadIdx.x, per = (N + 255) / 256;
    const int a = min(N, tid * per), b = min(N, a + per);
    int s = 0;
    for (int i = a; i < b; ++i) s += deg[i];
    sums[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = sums[t];
            sums[t] = run;
            run += v;
        }
        rowptr[N] = run;
    }
    __syncthreads();
    int run = sums[tid];
    for (int i = a; i < b; ++i) {
        rowptr[i] = run;
        run += deg[i];
    }
}

// one wave per row: its set bits as rising columns at col[rowptr[row]..]
__global__ __launch_bounds__(256) void msid_fill_kernel(const unsigned* __restrict__ mask, int N, int W, const int* __restrict__ rowptr,
                                                        long long cap, int* __restrict__ col) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    long long base = rowptr[row];
    for (int w0 = 0; w0 < W; w0 += 64) {
        const int w = w0 + lane;
        unsigned word = w < W ? mask[(long long)row * W + w] : 0u;
        const int c = __popc(word);
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        long long pos = base + incl - c;
        while (word) {
            const int b = __ffs(word) - 1;
            if (pos >= 0 && pos < cap) col[pos] = w * 32 + b;
            ++pos;
            word &= word - 1;
        }
        base += __shfl(incl, 63);
    }
}

// ------------------------------------------------------------------------------------------------------------ Lanczos
struct LzArgs {
    const int* rowptr;
    const int* col;
    const double* sc;       // normalised: 1 / sqrt(degree); else: the degree
    double* V;              // (m, N, nv)
    double* w;              // (N, nv)
    double* part;           // (m + 2, B, nv): the chunks' partial sums, slot by slot.  LZ_S_DOT: what lz_sq / lz_spmv / lz_subt write;
                            // LZ_S_VTW + jb: V[jb] . w; LZ_S_WW(m): w . w of the first step.  No kernel reads a slot it writes.
    double* red;            // (m, nv): V^T w
    double* beta;           // (nv)
    double* T;              // (nv, m, m)
    int* more;              // (m, LZ_PASSES)
    int* stopped;           // (m + 1)
    int N, nv, m, B, chunk, normalized, col_len;
};
enum { LZ_S_DOT = 0, LZ_S_VTW = 1 };
__device__ __forceinline__ int LZ_S_WW(int m) { return m + 1; }

struct LzPos { int cx, ry, c, r0, r1; bool cv; };
__device__ __forceinline__ LzPos lz_pos(const LzArgs& a) {
    LzPos p;
    p.cx = threadIdx.x & 63;
    p.ry = threadIdx.x >> 6;
    p.c = blockIdx.y * 64 + p.cx;
    p.cv = p.c < a.nv;
    p.r0 = blockIdx.x * a.chunk;
    p.r1 = min(a.N, p.r0 + a.chunk);
    return p;
}
// the four row lanes' values of a column, added in lane order, to the chunk's place in slot `slot`
__device__ __forceinline__ void lz_put(const LzArgs& a, const LzPos& p, double v, int slot, double* sh) {
    sh[p.ry * 64 + p.cx] = v;
    __syncthreads();
    if (p.ry == 0 && p.cv) a.part[((long long)slot * a.B + blockIdx.x) * a.nv + p.c] = ((sh[p.cx] + sh[64 + p.cx]) + sh[128 + p.cx]) + sh[192 + p.cx];
    __syncthreads();
}
// the chunks of a slot in chunk order
__device__ __forceinline__ double lz_total(const LzArgs& a, int slot, int c) {
    double s = 0.0;
    for (int b = 0; b < a.B; ++b) s += a.part[((long long)slot * a.B + b) * a.nv + c];
    return s;
}
__device__ __forceinline__ bool lz_skip(const LzArgs& a, int i, int p) { return a.stopped[i] != 0 || (p >= 1 && a.more[i * LZ_PASSES + p - 1] == 0); }

__global__ void msid_scale_kernel(const int* __restrict__ rowptr, int N, int normalized, double* __restrict__ sc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double d = (double)(rowptr[i + 1] - rowptr[i]);
    sc[i] = normalized ? 1.0 / sqrt(d) : d;
}

// slot 0 <- sum src^2 per column
__global__ __launch_bounds__(256) void lz_sq_kernel(LzArgs a, const double* __restrict__ src) {
    __shared__ double sh[256];
    const LzPos p = lz_pos(a);
    double s = 0.0;
    if (p.cv)
        for (int r = p.r0 + p.ry; r < p.r1; r += 4) {
            const double v = src[(long long)r * a.nv + p.c];
            s += v * v;
        }
    lz_put(a, p, s, LZ_S_DOT, sh);
}

// V[0] = start / |start| (msid.py:77-78)
__global__ __launch_bounds__(256) void lz_start_kernel(LzArgs a, const double* __restrict__ src) {
    const LzPos p = lz_pos(a);
    if (!p.cv) return;
    const double nrm = sqrt(lz_total(a, LZ_S_DOT, p.c));
    for (int r = p.r0 + p.ry; r < p.r1; r += 4) a.V[(long long)r * a.nv + p.c] = src[(long long)r * a.nv + p.c] / nrm;
}

// w = L V[i] - beta V[i - 1] (i >= 1); slot 0 <- w . V[i]
__global__ __launch_bounds__(256) void lz_spmv_kernel(LzArgs a, int i) {
    __shared__ double sh[256];
    if (lz_skip(a, i, 0)) return;
    const LzPos p = lz_pos(a);
    const double* Vi = a.V + (long long)i * a.N * a.nv;
    const double* Vo = i >= 1 ? a.V + (long long)(i - 1) * a.N * a.nv : nullptr;
    double s = 0.0;
    if (p.cv) {
        const double be = Vo ? a.beta[p.c] : 0.0;
        for (int r = p.r0 + p.ry; r < p.r1; r += 4) {
            const int e0 = max(0, a.rowptr[r]), e1 = min(a.col_len, a.rowptr[r + 1]);
            const double sr = a.sc[r], vr = Vi[(long long)r * a.nv + p.c];
            const double diag = a.normalized ? vr : sr * vr;
            double acc = 0.0;
            bool placed = false;                         // the diagonal takes its place among the sorted columns
            for (int e = e0; e < e1; ++e) {
                const int j = a.col[e];
                if (j < 0 || j >= a.N) continue;
                if (!placed && j > r) { acc += diag; placed = true; }
                const double lij = a.normalized ? -(sr * a.sc[j]) : -1.0;
                acc += lij * Vi[(long long)j * a.nv + p.c];
            }
            if (!placed) acc += diag;
            if (Vo) acc -= be * Vo[(long long)r * a.nv + p.c];
            a.w[(long long)r * a.nv + p.c] = acc;
            s += acc * vr;
        }
    }
    lz_put(a, p, s, LZ_S_DOT, sh);
}

// slots LZ_S_VTW + 0..nb-1 <- V[jb] . w
__device__ __forceinline__ void lz_vtw(const LzArgs& a, const LzPos& p, int nb, double* sh) {
    for (int jb = 0; jb < nb; ++jb) {
        const double* Vj = a.V + (long long)jb * a.N * a.nv;
        double s = 0.0;
        if (p.cv)
            for (int r = p.r0 + p.ry; r < p.r1; r += 4) s += Vj[(long long)r * a.nv + p.c] * a.w[(long long)r * a.nv + p.c];
        lz_put(a, p, s, LZ_S_VTW + jb, sh);
    }
}

enum { LZ_FIRST = 0, LZ_MIDDLE = 1, LZ_LAST = 2 };
// alpha = the total of LZ_S_DOT -> T[i][i]; unless LZ_LAST: w -= alpha V[i], then LZ_S_WW <- w . w (LZ_FIRST: msid.py:82-83) or
// the LZ_S_VTW slots <- V^T w (msid.py:105,108)
__global__ __launch_bounds__(256) void lz_alpha_kernel(LzArgs a, int i, int mode) {
    __shared__ double sh[256];
    if (lz_skip(a, i, 0)) return;
    const LzPos p = lz_pos(a);
    const double alpha = p.cv ? lz_total(a, LZ_S_DOT, p.c) : 0.0;
    if (blockIdx.x == 0 && p.ry == 0 && p.cv) a.T[((long long)p.c * a.m + i) * a.m + i] = alpha;
    if (mode == LZ_LAST) return;
    const double* Vi = a.V + (long long)i * a.N * a.nv;
    double s = 0.0;
    if (p.cv)
        for (int r = p.r0 + p.ry; r < p.r1; r += 4) {
            const long long at = (long long)r * a.nv + p.c;
            const double v = a.w[at] - alpha * Vi[at];
            a.w[at] = v;
            s += v * v;
        }
    if (mode == LZ_FIRST) lz_put(a, p, s, LZ_S_WW(a.m), sh);
    else lz_vtw(a, p, i + 1, sh);
}

// red[jb][c] <- the totals of the LZ_S_VTW slots 0..nb-1; check: more[i][p] |= some total > 1e-5 (msid.py:121, signed)
__global__ __launch_bounds__(256) void lz_reduce_kernel(LzArgs a, int i, int p, int nb, int check) {
    if (lz_skip(a, i, p)) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    int over = 0;
    if (e < nb * a.nv) {
        const double s = lz_total(a, LZ_S_VTW + e / a.nv, e % a.nv);
        a.red[e] = s;
        over = s > 1e-5 ? 1 : 0;
    }
    if (check && __syncthreads_or(over) && threadIdx.x == 0) atomicOr(&a.more[i * LZ_PASSES + p], 1);
}

// w -= sum_jb<=i V[jb] red[jb] (msid.py:109,126); LZ_S_DOT <- w . w
__global__ __launch_bounds__(256) void lz_subt_kernel(LzArgs a, int i, int p) {
    __shared__ double sh[256];
    if (lz_skip(a, i, p)) return;
    const LzPos q = lz_pos(a);
    double s = 0.0;
    if (q.cv)
        for (int r = q.r0 + q.ry; r < q.r1; r += 4) {
            const long long at = (long long)r * a.nv + q.c;
            double corr = 0.0;
            for (int jb = 0; jb <= i; ++jb) corr += a.V[(long long)jb * a.N * a.nv + at] * a.red[jb * a.nv + q.c];
            const double v = a.w[at] - corr;
            a.w[at] = v;
            s += v * v;
        }
    lz_put(a, q, s, LZ_S_DOT, sh);
}

// w /= sqrt(w . w) (the total of LZ_S_DOT; i == 0: of LZ_S_WW); p == 0: that is beta -> T[i][i + 1], T[i + 1][i] (msid.py:110-115).  i == 0: V[1] = w
// (msid.py:90-91); else the LZ_S_VTW slots <- V^T w (msid.py:118,128), unless nothing reads them (the last extra pass).
__global__ __launch_bounds__(256) void lz_norm_kernel(LzArgs a, int i, int p) {
    __shared__ double sh[256];
    if (lz_skip(a, i, p)) return;
    const LzPos q = lz_pos(a);
    const double nrm = q.cv ? sqrt(lz_total(a, i == 0 ? LZ_S_WW(a.m) : LZ_S_DOT, q.c)) : 1.0;
    if (p == 0 && blockIdx.x == 0 && q.ry == 0 && q.cv) {
        a.beta[q.c] = nrm;
        a.T[((long long)q.c * a.m + i) * a.m + i + 1] = nrm;
        a.T[((long long)q.c * a.m + i + 1) * a.m + i] = nrm;
    }
    double* V1 = i == 0 ? a.V + (long long)a.N * a.nv : nullptr;
    if (q.cv)
        for (int r = q.r0 + q.ry; r < q.r1; r += 4) {
            const long long at = (long long)r * a.nv + q.c;
            const double v = a.w[at] / nrm;
            a.w[at] = v;
            if (V1) V1[at] = v;
        }
    if (i == 0 || p == LZ_PASSES) return;
    lz_vtw(a, q, i + 1, sh);
}

// V[i + 1] = w (msid.py:130); stopped[i + 1] = stopped[i] or every |beta| <= 1e-6 or the extra passes did not converge (msid.py:132)
__global__ __launch_bounds__(256) void lz_store_kernel(LzArgs a, int i) {
    const bool skip = a.stopped[i] != 0;
    const LzPos q = lz_pos(a);
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        int big = 0;
        for (int c = threadIdx.x; c < a.nv; c += 256) big |= fabs(a.beta[c]) > 1e-6 ? 1 : 0;
        const int any_big = __syncthreads_or(big);
        if (threadIdx.x == 0) a.stopped[i + 1] = (skip || !any_big || a.more[i * LZ_PASSES + LZ_PASSES - 1] != 0) ? 1 : 0;
    }
    if (skip || !q.cv) return;
    double* Vn = a.V + (long long)(i + 1) * a.N * a.nv;
    for (int r = q.r0 + q.ry; r < q.r1; r += 4) Vn[(long long)r * a.nv + q.c] = a.w[(long long)r * a.nv + q.c];
}

// ------------------------------------------------------------------------------------------------------------ quadrature
// One thread per starting vector.  q: (2, nts, nv).
__global__ __launch_bounds__(64) void msid_quad_kernel(const double* __restrict__ T, int nv, int m, const double* __restrict__ ts, int nts,
                                                       double* __restrict__ q) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= nv) return;
    double d[MSID_MAX_M], e[MSID_MAX_M], z[MSID_MAX_M];
    const double* Tv = T + (long long)v * m * m;
    for (int j = 0; j < m; ++j) {
        d[j] = Tv[j * m + j];
        e[j] = j + 1 < m ? Tv[j * m + j + 1] : 0.0;
        z[j] = j == 0 ? 1.0 : 0.0;
    }
    // implicit QL with Wilkinson's shift; the rotations are applied to the first row of the eigenvector matrix only.  A zero
    // off-diagonal splits the matrix: the rows an early break left zero come out as eigenvalue 0 with first component 0.
    for (int l = 0; l < m; ++l) {
        for (int iter = 0; iter < 60; ++iter) {
            int mm = l;
            for (; mm < m - 1; ++mm) {
                const double dd = fabs(d[mm]) + fabs(d[mm + 1]);
                if (fabs(e[mm]) + dd == dd) break;
            }
            if (mm == l) break;
            double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
            double r = hypot(g, 1.0);
            g = d[mm] - d[l] + e[l] / (g + copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            int i = mm - 1;
            for (; i >= l; --i) {
                double f = s * e[i];
                const double b = c * e[i];
                r = hypot(f, g);
                e[i + 1] = r;
                if (r == 0.0) {
                    d[i + 1] -= p;
                    e[mm] = 0.0;
                    break;
                }
                s = f / r;
                c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2.0 * c * b;
                p = s * r;
                d[i + 1] = g + p;
                g = c * r - b;
                f = z[i + 1];
                z[i + 1] = s * z[i] + c * f;
                z[i] = c * z[i] - s * f;
            }
            if (r == 0.0 && i >= l) continue;
            d[l] -= p;
            e[l] = g;
            e[mm] = 0.0;
        }
    }
    for (int t = 0; t < nts; ++t) {
        const double tt = ts[t];
        double se = 0.0, si = 0.0;
        for (int j = 0; j < m; ++j) {
            const double x = -(tt * d[j]), w = z[j] * z[j];
            se += exp(x) * w;
            si += x * w;
        }
        q[(long long)t * nv + v] = se;
        q[((long long)nts + t) * nv + v] = si;
    }
}

// traces[f][t] = n * mean over the vectors, in vector order (msid.py:199)
__global__ void msid_traces_kernel(const double* __restrict__ q, int nv, int nts, int N, double* __restrict__ traces) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * nts) return;
    double s = 0.0;
    for (int v = 0; v < nv; ++v) s += q[(long long)e * nv + v];
    traces[e] = (double)N * (s / (double)nv);
}

// tables: (3, nts) = exp(ts), sub, div (msid.py:218-220, 242-256, 289)
__global__ void msid_descriptor_kernel(const double* __restrict__ traces, const double* __restrict__ tables, int nts, double* __restrict__ desc) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nts) return;
    const double subee = traces[t] - traces[nts + t] / tables[t];
    desc[t] = (subee + tables[nts + t]) / tables[2 * nts + t] * 1e6;
}

// one workgroup: out[0] = max_t c[t] |dp - dt| (c given) or the l2 norm of dp - dt
__global__ __launch_bounds__(256) void msid_distance_kernel(const double* __restrict__ dp, const double* __restrict__ dt, const double* __restrict__ c,
                                                            int nts, double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double v = 0.0;
    bool bad = false;
    for (int t = tid; t < nts; t += 256) {
        const double d = dp[t] - dt[t];
        if (c) {
            const double x = c[t] * fabs(d);
            bad = bad || x != x;
            if (x > v) v = x;
        } else v += d * d;
    }
    if (!c) {
        v = block_sum256(v, red);
        if (tid == 0) out[0] = sqrt(v);
        return;
    }
    red[tid] = bad ? __builtin_nan("") : v;                // (np.amax hands a NaN on)
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const double x = red[tid], y = red[tid + s];
            red[tid] = (x != x || y != y) ? __builtin_nan("") : (x > y ? x : y);
        }
        __syncthreads();
    }
    if (tid == 0) out[0] = red[0];
}

// ------------------------------------------------------------------------------------------------------------ Inception Score
// One workgroup per split of R = N / S rows (isc.py:43-52).  ws: mx (N), sm (N), kl (N), lpy (S, D).  scores[s] = exp(mean KL).
__global__ __launch_bounds__(256) void is_split_kernel(const float* __restrict__ X, int R, int D, double* __restrict__ mx, double* __restrict__ sm,
                                                       double* __restrict__ kl, double* __restrict__ lpy, double* __restrict__ scores) {
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.x;
    const long long row0 = (long long)s * R;
    double* ly = lpy + (long long)s * D;
    for (int r = wave; r < R; r += 4) {                  // the row's softmax: its maximum and the sum of exp(x - max)
        const float* x = X + (row0 + r) * D;
        double m = -__builtin_inf();
        bool nan = false;
        for (int d = lane; d < D; d += 64) {
            const double v = (double)x[d];
            nan = nan || v != v;
            if (v > m) m = v;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double t = __shfl_xor(m, o);
            if (t > m) m = t;
        }
        double e = 0.0;
        for (int d = lane; d < D; d += 64) e += exp((double)x[d] - m);
        e = wave_sum64(e);
        if (__any(nan)) e = __builtin_nan("");
        if (lane == 0) {
            mx[row0 + r] = m;
            sm[row0 + r] = e;
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int d = tid; d < D; d += 256) {                 // p_y: the column means, the rows in order
        double a = 0.0;
        for (int r = 0; r < R; ++r) a += exp((double)X[(row0 + r) * D + d] - mx[row0 + r]) / sm[row0 + r];
        ly[d] = log(a / (double)R);
    }
    __threadfence_block();
    __syncthreads();
    for (int r = wave; r < R; r += 4) {                  // KL(p_yx || p_y) = sum p log p - p log p_y; a zero p contributes 0
        const float* x = X + (row0 + r) * D;
        const double m = mx[row0 + r], e = sm[row0 + r];
        double a = 0.0;
        for (int d = lane; d < D; d += 64) {
            const double p = exp((double)x[d] - m) / e;
            a += p == 0.0 ? 0.0 : p * log(p) - p * ly[d];
        }
        a = wave_sum64(a);
        if (lane == 0) kl[row0 + r] = a;
    }
    __threadfence_block();
    __syncthreads();
    double a = 0.0;
    for (int r = tid; r < R; r += 256) a += kl[row0 + r];
    a = block_sum256(a, red);
    if (tid == 0) scores[s] = exp(a / (double)R);
}

// out[0] = the mean, out[1] = the unbiased standard deviation of out[2..2 + S) (isc.py:55; S == 1: nan)
__global__ void is_finish_kernel(double* __restrict__ out, int S) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += out[2 + s];
    const double mean = a / (double)S;
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += (out[2 + s] - mean) * (out[2 + s] - mean);
    out[0] = mean;
    out[1] = sqrt(v / (double)(S - 1));
}

// ------------------------------------------------------------------------------------------------------------ workspace
size_t nbr_ws(int N) { return al256((size_t)N * 8) + al256((size_t)msid_panel_rows(N) * N * 8); }
size_t graph_ws(int N) { return al256((size_t)N * ((N + 31) / 32) * 4) + al256((size_t)N * 4); }
struct LzLayout { size_t sc, w, part, red, beta, flags, V, end; };
LzLayout lz_layout(int N, int m, int nv) {
    LzLayout l;
    size_t o = 0;
    l.sc = o; o += al256((size_t)N * 8);
    l.w = o; o += al256((size_t)N * nv * 8);
    l.part = o; o += al256((size_t)(m + 2) * lz_chunks(N) * nv * 8);
    l.red = o; o += al256((size_t)m * nv * 8);
    l.beta = o; o += al256((size_t)nv * 8);
    l.flags = o; o += al256((size_t)(m * LZ_PASSES + m + 1) * 4);
    l.V = o; o += al256((size_t)m * N * nv * 8);
    l.end = o;
    return l;
}
size_t quad_ws(int nv, int nts) { return al256((size_t)2 * nts * nv * 8); }

}  // namespace

extern "C" size_t mtd_msid_ws_bytes(int N, int D, int k, int m, int nv, int nts) {
    if (D < 1 || !msid_graph_ok(N, k) || !msid_lz_ok(m, nv) || nts < 1 || nts > MSID_MAX_TS) return 0;
    size_t b = nbr_ws(N);
    if (graph_ws(N) > b) b = graph_ws(N);
    if (lz_layout(N, m, nv).end > b) b = lz_layout(N, m, nv).end;
    if (quad_ws(nv, nts) > b) b = quad_ws(nv, nts);
    return b;
}

extern "C" int mtd_msid_panel_rows(int N) { return N >= 1 && N <= MSID_MAX_N ? msid_panel_rows(N) : 0; }

extern "C" int mtd_msid_distances(const float* X, int N, int D, int row0, int rows, double* dist, void* ws, void* stream) {
    if (!X || !dist || !ws || N < 1 || N > MSID_MAX_N || D < 1 || row0 < 0 || rows < 1 || (long long)row0 + rows > N) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* dd = (double*)ws;
    hipLaunchKernelGGL(msid_sqnorm_kernel, dim3((N + 3) / 4), dim3(256), 0, s, X, N, D, dd);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(msid_dist_kernel, dim3((N + MT - 1) / MT, (rows + MT - 1) / MT), dim3(256), 0, s, X, N, D, (const double*)dd, row0, rows, dist);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_msid_neighbours(const float* X, int N, int D, int k, int* nbr, void* ws, void* stream) {
    if (!X || !nbr || !ws || D < 1 || !msid_graph_ok(N, k)) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* dd = (double*)ws;
    double* panel = (double*)((char*)ws + al256((size_t)N * 8));
    const int P = msid_panel_rows(N);
    hipLaunchKernelGGL(msid_sqnorm_kernel, dim3((N + 3) / 4), dim3(256), 0, s, X, N, D, dd);
    MTD_LAUNCH_CHECK();
    for (int row0 = 0; row0 < N; row0 += P) {
        const int rows = N - row0 < P ? N - row0 : P;
        hipLaunchKernelGGL(msid_dist_kernel, dim3((N + MT - 1) / MT, (rows + MT - 1) / MT), dim3(256), 0, s, X, N, D, (const double*)dd, row0, rows, panel);
        MTD_LAUNCH_CHECK();
        hipLaunchKernelGGL(msid_select_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, (const double*)panel, N, row0, rows, k + 1, nbr);
        MTD_LAUNCH_CHECK();
    }
    return MTD_OK;
}

extern "C" int mtd_msid_graph(const int* nbr, int N, int k, int* rowptr, int* col, void* ws, void* stream) {
    if (!nbr || !rowptr || !col || !ws || !msid_graph_ok(N, k)) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int W = (N + 31) / 32, k1 = k + 1;
    unsigned* mask = (unsigned*)ws;
    int* deg = (int*)((char*)ws + al256((size_t)N * W * 4));
    if (hipMemsetAsync(mask, 0, (size_t)N * W * 4, s) != hipSuccess) return MTD_EINVAL;
    const long long edges = (long long)N * k1;
    hipLaunchKernelGGL(msid_mask_kernel, dim3((unsigned)((edges + 255) / 256)), dim3(256), 0, s, nbr, N, k1, W, mask);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(msid_degree_kernel, dim3((N + 3) / 4), dim3(256), 0, s, (const unsigned*)mask, N, W, deg);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(msid_scan_kernel, dim3(1), dim3(256), 0, s, (const int*)deg, N, rowptr);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(msid_fill_kernel, dim3((N + 3) / 4), dim3(256), 0, s, (const unsigned*)mask, N, W, (const int*)rowptr, 2 * edges, col);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_msid_lanczos(const int* rowptr, const int* col, int col_len, int N, const double* start, int nv, int m, int normalized,
                                double* T, double* V, void* ws, void* stream) {
    if (!rowptr || !col || !start || !T || !ws || col_len < 0 || N < 2 || N > MSID_MAX_N || !msid_lz_ok(m, nv)) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const LzLayout l = lz_layout(N, m, nv);
    char* base = (char*)ws;
    LzArgs a = {};
    a.rowptr = rowptr; a.col = col; a.sc = (const double*)(base + l.sc);
    a.V = V ? V : (double*)(base + l.V);
    a.w = (double*)(base + l.w); a.part = (double*)(base + l.part); a.red = (double*)(base + l.red); a.beta = (double*)(base + l.beta);
    a.T = T; a.more = (int*)(base + l.flags); a.stopped = a.more + m * LZ_PASSES;
    a.N = N; a.nv = nv; a.m = m; a.B = lz_chunks(N); a.chunk = lz_chunk_rows(N); a.normalized = normalized ? 1 : 0; a.col_len = col_len;
    if (hipMemsetAsync(a.more, 0, (size_t)(m * LZ_PASSES + m + 1) * 4, s) != hipSuccess) return MTD_EINVAL;
    if (hipMemsetAsync(T, 0, (size_t)nv * m * m * 8, s) != hipSuccess) return MTD_EINVAL;
    if (hipMemsetAsync(a.V, 0, (size_t)m * N * nv * 8, s) != hipSuccess) return MTD_EINVAL;
    const dim3 grid(a.B, (nv + 63) / 64), blk(256);
#define LZ_RUN(kernel, ...)                                       \
    do {                                                          \
        hipLaunchKernelGGL(kernel, grid, blk, 0, s, __VA_ARGS__); \
        MTD_LAUNCH_CHECK();                                       \
    } while (0)
#define LZ_REDUCE(i, p, nb, check)                                                                                            \
    do {                                                                                                                      \
        hipLaunchKernelGGL(lz_reduce_kernel, dim3(((nb) * nv + 255) / 256), blk, 0, s, a, i, p, nb, check);                   \
        MTD_LAUNCH_CHECK();                                                                                                   \
    } while (0)
    hipLaunchKernelGGL(msid_scale_kernel, dim3((N + 255) / 256), blk, 0, s, rowptr, N, a.normalized, (double*)(base + l.sc));
    MTD_LAUNCH_CHECK();
    LZ_RUN(lz_sq_kernel, a, start);
    LZ_RUN(lz_start_kernel, a, start);
    LZ_RUN(lz_spmv_kernel, a, 0);
    LZ_RUN(lz_alpha_kernel, a, 0, (int)LZ_FIRST);
    LZ_RUN(lz_norm_kernel, a, 0, 0);
    for (int i = 1; i < m; ++i) {
        LZ_RUN(lz_spmv_kernel, a, i);
        if (i == m - 1) {
            LZ_RUN(lz_alpha_kernel, a, i, (int)LZ_LAST);
            break;
        }
        LZ_RUN(lz_alpha_kernel, a, i, (int)LZ_MIDDLE);
        LZ_REDUCE(i, 0, i + 1, 0);
        LZ_RUN(lz_subt_kernel, a, i, 0);
        LZ_RUN(lz_norm_kernel, a, i, 0);
        LZ_REDUCE(i, 0, i + 1, 1);
        for (int p = 1; p <= LZ_PASSES; ++p) {
            LZ_RUN(lz_subt_kernel, a, i, p);
            LZ_RUN(lz_norm_kernel, a, i, p);
            if (p < LZ_PASSES) LZ_REDUCE(i, p, i + 1, 1);
        }
        LZ_RUN(lz_store_kernel, a, i);
    }
#undef LZ_RUN
#undef LZ_REDUCE
    return MTD_OK;
}

extern "C" int mtd_msid_quadrature(const double* T, int nv, int m, int N, const double* ts, int nts, double* traces, void* ws, void* stream) {
    if (!T || !ts || !traces || !ws || N < 1 || !msid_lz_ok(m, nv) || nts < 1 || nts > MSID_MAX_TS) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* q = (double*)ws;
    hipLaunchKernelGGL(msid_quad_kernel, dim3((nv + 63) / 64), dim3(64), 0, s, T, nv, m, ts, nts, q);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(msid_traces_kernel, dim3((2 * nts + 255) / 256), dim3(256), 0, s, (const double*)q, nv, nts, N, traces);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_msid_combine(const double* traces, const double* tables, int nts, double* desc, void* stream) {
    if (!traces || !tables || !desc || nts < 1 || nts > MSID_MAX_TS) return MTD_EINVAL;
    hipLaunchKernelGGL(msid_descriptor_kernel, dim3((nts + 255) / 256), dim3(256), 0, (hipStream_t)stream, traces, tables, nts, desc);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_msid_distance(const double* dp, const double* dt, const double* c, int nts, int mode, double* out, void* stream) {
    if (!dp || !dt || !out || nts < 1 || nts > MSID_MAX_TS || (mode != MTD_MSID_MAX && mode != MTD_MSID_L2) || (mode == MTD_MSID_MAX && !c))
        return MTD_EINVAL;
    hipLaunchKernelGGL(msid_distance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, dp, dt, mode == MTD_MSID_MAX ? c : (const double*)nullptr, nts, out);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_msid_descriptor(const float* X, int N, int D, int k, int m, int nv, int normalized, const double* start, const double* ts,
                                   const double* tables, int nts, int* nbr, int* rowptr, int* col, double* T, double* traces, double* desc,
                                   void* ws, void* stream) {
    if (!X || !start || !ts || !tables || !nbr || !rowptr || !col || !T || !traces || !desc || !ws) return MTD_EINVAL;
    if (mtd_msid_ws_bytes(N, D, k, m, nv, nts) == 0) return MTD_EINVAL;
    int rc = mtd_msid_neighbours(X, N, D, k, nbr, ws, stream);
    if (rc == MTD_OK) rc = mtd_msid_graph(nbr, N, k, rowptr, col, ws, stream);
    if (rc == MTD_OK) rc = mtd_msid_lanczos(rowptr, col, 2 * N * (k + 1), N, start, nv, m, normalized, T, nullptr, ws, stream);
    if (rc == MTD_OK) rc = mtd_msid_quadrature(T, nv, m, N, ts, nts, traces, ws, stream);
    if (rc == MTD_OK) rc = mtd_msid_combine(traces, tables, nts, desc, stream);
    return rc;
}

extern "C" size_t mtd_is_ws_bytes(int N, int D, int S) {
    if (N < 1 || D < 1 || S < 1 || S > 65535 || N / S < 1) return 0;
    return 3 * al256((size_t)N * 8) + al256((size_t)S * D * 8);
}

extern "C" int mtd_inception_score(const float* X, int N, int D, int S, double* out, void* ws, void* stream) {
    if (!X || !out || !ws || mtd_is_ws_bytes(N, D, S) == 0) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    const size_t n8 = al256((size_t)N * 8);
    hipLaunchKernelGGL(is_split_kernel, dim3(S), dim3(256), 0, s, X, N / S, D, (double*)base, (double*)(base + n8), (double*)(base + 2 * n8),
                       (double*)(base + 3 * n8), out + 2);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(is_finish_kernel, dim3(1), dim3(64), 0, s, out, S);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
