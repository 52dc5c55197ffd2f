// Task weightings of the discriminator step next to PCGrad (module/weight_methods.py of the reference: :275-316 linear
// scalarisations, :375-406 STL / uncertainty weighting, :471-588 CAGrad, :591-602 RLW, :678-724 dynamic weight average).
// Two single-wavefront kernels, no host read:
//   task_weights_kernel   the T device-resident task losses -> the T factors c_k = d loss / d L_k the loss cotangents are
//                         scaled by (mtd_loss_term.wptr), the weighted loss and the weight vector the method reports, the
//                         gradient of the uncertainty weighting's log sigmas; the dynamic weight average keeps its cost ring
//                         and its iteration counter in device memory.
//   cagrad_coeff_kernel   the T x T Gram matrix -> the T coefficients of CAGrad's merged gradient.  The inner problem
//                         min_x phi(x) = x^T A b + c0 sqrt(x^T A x + 1e-8) over the simplex is convex; its minimiser is a
//                         stationary point of phi on the face that supports it.  On a face S the stationarity condition
//                         A_SS x + nu 1 = -u (A b)_S, 1^T x = 1 with u = sqrt(x^T A x + 1e-8) / c0 is linear in x for a given
//                         u: x = x0 + u x1, and u solves (q11 - c0^2) u^2 + 2 q01 u + q00 + 1e-8 = 0 (q.. = x.^T A x.) -- a
//                         closed form per face.  One lane per face (2^T - 1 <= 15) solves its (|S| + 1)-square system in
//                         fp64, the feasible candidate with the smallest phi wins (ties: the lowest face index).  A face
//                         whose system is singular has a direction along which phi is constant, so a smaller face holds the
//                         same minimum: it is skipped.  Fixed work, no iteration count that depends on the data.
#include "common.h"

namespace {

constexpr int MAXT = 4;

__global__ __launch_bounds__(64) void task_weights_kernel(int method, const float* __restrict__ losses, int T, float* __restrict__ state,
                                                          const float* __restrict__ params, int window, float temp,
                                                          float* __restrict__ c_out, float* __restrict__ aux) {
    __shared__ float ratio[MAXT];
    const int lane = threadIdx.x;
    if (method == MTD_TW_DWA) {
        // state: [0] iteration counter (int bits), [1 .. 1+T) the weights, then the ring of 2 * window rows of T costs
        const int it = __float_as_int(state[0]);
        float* w = state + 1;
        float* ring = state + 1 + MAXT;
        const int R = 2 * window;
        if (lane < T) {
            ring[(it % R) * T + lane] = losses[lane];          // the oldest row is the one replaced
            // chronological order from the oldest row: (it + 1 + j) % R; the first `window` rows against the last
            float old_s = 0.f, new_s = 0.f;
            for (int j = 0; j < window; ++j) old_s += ring[((it + 1 + j) % R) * T + lane];
            for (int j = window; j < R; ++j) new_s += ring[((it + 1 + j) % R) * T + lane];
            ratio[lane] = (new_s / (float)window) / (old_s / (float)window);
        }
        __syncthreads();
        if (lane != 0) return;
        float wk[MAXT];
        for (int k = 0; k < T; ++k) wk[k] = w[k];
        if (it > window) {
            float e[MAXT], s = 0.f;
            for (int k = 0; k < T; ++k) { e[k] = expf(ratio[k] / temp); s += e[k]; }
            for (int k = 0; k < T; ++k) { wk[k] = ((float)T * e[k]) / s; w[k] = wk[k]; }
        }
        float loss = 0.f;
        for (int k = 0; k < T; ++k) { loss += wk[k] * losses[k]; c_out[k] = wk[k] / (float)T; aux[1 + k] = wk[k]; }
        aux[0] = loss / (float)T;
        state[0] = __int_as_float(it < 0x7fffffff ? it + 1 : it);
        return;
    }
    if (lane != 0) return;
    float loss = 0.f;
    if (method == MTD_TW_LS || method == MTD_TW_STL) {
        for (int k = 0; k < T; ++k) { const float w = params[k]; loss += losses[k] * w; c_out[k] = w; aux[1 + k] = w; }
    } else if (method == MTD_TW_SCALEINV) {
        for (int k = 0; k < T; ++k) { const float w = params[k]; loss += logf(losses[k]) * w; c_out[k] = w / losses[k]; aux[1 + k] = w; }
    } else if (method == MTD_TW_UW) {
        for (int k = 0; k < T; ++k) {
            const float s = state[k], e = expf(-s);
            loss += 0.5f * (e * losses[k] + s);
            c_out[k] = 0.5f * e;
            aux[1 + k] = e;
            aux[1 + MAXT + k] = 0.5f * (1.f - e * losses[k]);        // d loss / d s_k
        }
    } else {    // MTD_TW_RLW: softmax of the host's normal draw (params: a pinned slot)
        float z[MAXT], m = params[0], s = 0.f;
        for (int k = 0; k < T; ++k) { z[k] = params[k]; m = fmaxf(m, z[k]); }
        for (int k = 0; k < T; ++k) { z[k] = expf(z[k] - m); s += z[k]; }
        for (int k = 0; k < T; ++k) { const float w = z[k] / s; loss += losses[k] * w; c_out[k] = w; aux[1 + k] = w; }
    }
    aux[0] = loss;
}

__device__ double phi_of(const double* A, int T, const double* x, double c0) {
    double lin = 0.0, q = 0.0;
    for (int i = 0; i < T; ++i) {
        double ax = 0.0, ab = 0.0;
        for (int j = 0; j < T; ++j) { ax += A[i * T + j] * x[j]; ab += A[i * T + j]; }
        lin += x[i] * ab / (double)T;
        q += x[i] * ax;
    }
    return lin + c0 * sqrt((q > 0.0 ? q : 0.0) + 1e-8);
}

__global__ __launch_bounds__(64) void cagrad_coeff_kernel(const double* __restrict__ gram, int T, float alpha, float* __restrict__ coeff) {
    __shared__ double best_phi[16];
    __shared__ double best_x[16][MAXT];
    const int lane = threadIdx.x;
    const int nfaces = (1 << T) - 1;
    double A[MAXT * MAXT];
    double mean = 0.0, scale = 0.0;
    for (int i = 0; i < T * T; ++i) { A[i] = gram[i]; mean += A[i]; scale = fmax(scale, fabs(A[i])); }
    mean /= (double)(T * T);
    const double c0 = (double)alpha * sqrt((mean > 0.0 ? mean : 0.0) + 1e-8) + 1e-8;
    if (lane < nfaces) {
        const int mask = lane + 1;
        int idx[MAXT], m = 0;
        for (int i = 0; i < T; ++i) if (mask >> i & 1) idx[m++] = i;
        double phi_best = 1e300, x_best[MAXT] = {0, 0, 0, 0};
        auto consider = [&](const double* xs) {        // xs: the face's m entries; feasible up to rounding -> clamp, renormalise, true phi
            double x[MAXT] = {0, 0, 0, 0}, s = 0.0;
            for (int a = 0; a < m; ++a) {
                if (!(xs[a] >= -1e-9) || !(xs[a] <= 1.0 + 1e-9)) return;
                x[idx[a]] = xs[a] > 0.0 ? xs[a] : 0.0;
                s += x[idx[a]];
            }
            if (!(s > 0.0)) return;
            for (int i = 0; i < T; ++i) x[i] /= s;
            const double p = phi_of(A, T, x, c0);
            if (p < phi_best) { phi_best = p; for (int i = 0; i < T; ++i) x_best[i] = x[i]; }
        };
        if (m == 1) {
            const double one = 1.0;
            consider(&one);
        } else {
            // [A_SS 1; 1^T 0] [x; nu] = [0; 1] and = [-(A b)_S; 0]: Gaussian elimination with partial pivoting, two right-hand sides
            const int n = m + 1;
            double M[5][7];
            for (int a = 0; a < m; ++a) {
                double ab = 0.0;
                for (int j = 0; j < T; ++j) ab += A[idx[a] * T + j];
                for (int b = 0; b < m; ++b) M[a][b] = A[idx[a] * T + idx[b]];
                M[a][m] = scale;                   // (the multiplier column in the units of A: keeps the pivots comparable)
                M[a][n] = 0.0;
                M[a][n + 1] = -ab / (double)T;
            }
            for (int b = 0; b < m; ++b) M[m][b] = scale;
            M[m][m] = 0.0; M[m][n] = scale; M[m][n + 1] = 0.0;
            bool ok = scale > 0.0;
            for (int col = 0; col < n && ok; ++col) {
                int piv = col;
                for (int r = col + 1; r < n; ++r) if (fabs(M[r][col]) > fabs(M[piv][col])) piv = r;
                if (!(fabs(M[piv][col]) > 1e-13 * scale)) { ok = false; break; }
                if (piv != col) for (int c = 0; c < n + 2; ++c) { const double t = M[col][c]; M[col][c] = M[piv][c]; M[piv][c] = t; }
                for (int r = 0; r < n; ++r) {
                    if (r == col) continue;
                    const double f = M[r][col] / M[col][col];
                    for (int c = col; c < n + 2; ++c) M[r][c] -= f * M[col][c];
                }
            }
            if (ok) {
                double x0[MAXT], x1[MAXT];
                for (int a = 0; a < m; ++a) { x0[a] = M[a][n] / M[a][a]; x1[a] = M[a][n + 1] / M[a][a]; }
                double q00 = 0.0, q01 = 0.0, q11 = 0.0;
                for (int a = 0; a < m; ++a)
                    for (int b = 0; b < m; ++b) {
                        const double v = A[idx[a] * T + idx[b]];
                        q00 += x0[a] * v * x0[b]; q01 += x0[a] * v * x1[b]; q11 += x1[a] * v * x1[b];
                    }
                // (q11 - c0^2) u^2 + 2 q01 u + (q00 + 1e-8) = 0, u > 0
                const double qa = q11 - c0 * c0, qb = 2.0 * q01, qc = (q00 > 0.0 ? q00 : 0.0) + 1e-8;
                double roots[2];
                int nr = 0;
                if (fabs(qa) <= 1e-300) {
                    if (qb != 0.0) roots[nr++] = -qc / qb;
                } else {
                    const double disc = qb * qb - 4.0 * qa * qc;
                    if (disc >= 0.0) {
                        const double sq = sqrt(disc);
                        const double t = -0.5 * (qb + (qb >= 0.0 ? sq : -sq));        // the numerically stable pair t / qa, qc / t
                        roots[nr++] = t / qa;
                        if (t != 0.0) roots[nr++] = qc / t;
                    }
                }
                for (int r = 0; r < nr; ++r) {
                    const double u = roots[r];
                    if (!(u > 0.0) || !(u < 1e300)) continue;
                    double xs[MAXT];
                    for (int a = 0; a < m; ++a) xs[a] = x0[a] + u * x1[a];
                    consider(xs);
                }
            }
        }
        best_phi[lane] = phi_best;
        for (int i = 0; i < MAXT; ++i) best_x[lane][i] = x_best[i];
    }
    __syncthreads();
    if (lane != 0) return;
    int win = 0;
    for (int f = 1; f < nfaces; ++f) if (best_phi[f] < best_phi[win]) win = f;       // (the vertices are always feasible: win is finite)
    double x[MAXT], q = 0.0;
    for (int i = 0; i < T; ++i) x[i] = (double)(float)best_x[win][i];                // the reference moves ww to fp32 (:533)
    for (int i = 0; i < T; ++i)
        for (int j = 0; j < T; ++j) q += x[i] * A[i * T + j] * x[j];
    const double lam = c0 / (sqrt(q > 0.0 ? q : 0.0) + 1e-8);
    const double resc = (double)T / (1.0 + (double)alpha * (double)alpha);           // rescale = 1, then x n_tasks (:541, :563)
    for (int i = 0; i < T; ++i) coeff[i] = (float)(resc * (1.0 / (double)T + lam * x[i]));
    coeff[MAXT] = (float)best_phi[win];
    for (int i = 0; i < T; ++i) coeff[MAXT + 1 + i] = (float)best_x[win][i];
}

}  // namespace

extern "C" int mtd_task_weights(int method, const float* losses, int T, float* state, const float* params, int window, float temp,
                                float* c_out, float* aux_out, void* stream) {
    if (T <= 0 || T > MAXT || !losses || !c_out || !aux_out) return MTD_EINVAL;
    if (method < MTD_TW_LS || method > MTD_TW_DWA) return MTD_EINVAL;
    if ((method == MTD_TW_UW || method == MTD_TW_DWA) && !state) return MTD_EINVAL;
    if (method != MTD_TW_UW && method != MTD_TW_DWA && !params) return MTD_EINVAL;
    if (method == MTD_TW_DWA && (window <= 0 || window > (1 << 20) || !(temp > 0.f))) return MTD_EINVAL;
    hipLaunchKernelGGL(task_weights_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, method, losses, T, state, params, window, temp, c_out, aux_out);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" size_t mtd_task_weights_state_floats(int method, int T, int window) {
    if (T <= 0 || T > MAXT) return 0;
    if (method == MTD_TW_UW) return (size_t)T;
    if (method == MTD_TW_DWA) return window > 0 ? (size_t)1 + MAXT + (size_t)2 * window * T : 0;
    return 0;
}

extern "C" int mtd_cagrad_coeff(const double* gram, int T, float c, float* coeff_out, void* stream) {
    if (T <= 0 || T > MAXT || !gram || !coeff_out || !(c >= 0.f)) return MTD_EINVAL;
    hipLaunchKernelGGL(cagrad_coeff_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, gram, T, c, coeff_out);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
