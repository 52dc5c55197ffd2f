// The Winograd weight transform of one 3x3 filter, shared by wino_weights_kernel (conv_winograd.hip: reads the filter from the
// weights) and adamw_views_kernel (adamw.hip: has the filter it just updated in LDS).  One copy of the arithmetic, so that the two
// produce the same bits: where a product is fused into a sum is written out (fmaf) and nothing else is contracted, since the
// compiler's own choice depends on the code around an expression.  The forms are those wino_weights_kernel has always had.
#pragma once

// t = G g  (4 x 3);  G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1] down the rows
__device__ __forceinline__ void wino_w_rows(const float (&g)[3][3], float (&t)[4][3]) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        t[0][b] = g[0][b];
        t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
        t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
        t[3][b] = g[2][b];
    }
}

// one row of u = t Gx^T: u[0 .. PXr) from t = (t0, t1, t2);  Gx = G (F(2,3), PXr = 4) or
// [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1] (F(4,3), PXr = 6) along the rows.
// (The split-bf16 form of wino_weights_kernel splits exactly these values: its three planes sum to the fp32 form's bits.)
__device__ __forceinline__ void wino_w_cols(float t0, float t1, float t2, int PXr, float (&u)[6]) {
#pragma clang fp contract(off)
    if (PXr == 6) {
        // -e -+ f and h +- k with e = (t0 + t2) / 6, f = t1 / 6, h = t0 / 24 + t2 / 6, k = t1 / 12: f and k go into their
        // sums as one fma each, h rounds both products first
        const float ne = (t0 + t2) * -(1.f / 6.f);
        const float h = t0 * (1.f / 24.f) + t2 * (1.f / 6.f);
        u[0] = 0.25f * t0;
        u[1] = __builtin_fmaf(t1, -(1.f / 6.f), ne);
        u[2] = __builtin_fmaf(t1, 1.f / 6.f, ne);
        u[3] = __builtin_fmaf(t1, 1.f / 12.f, h);
        u[4] = __builtin_fmaf(t1, -(1.f / 12.f), h);
        u[5] = t2;
    } else {
        u[0] = t0;
        u[1] = 0.5f * (t0 + t1 + t2);
        u[2] = 0.5f * (t0 - t1 + t2);
        u[3] = t2;
        u[4] = u[5] = 0.f;
    }
}

// u = t Gx^T (4 x PX) into  dst[xi][C/8][N][8]  at (n, ck = c / 8, c8 = c % 8)
__device__ __forceinline__ void wino_w_store(float* __restrict__ dst, int N, int C, int PXr, const float (&t)[4][3], int n, int ck, int c8) {
    const long long xs = (long long)(C / 8) * N * 8;          // stride between positions xi = a * PX + b
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        float* o = dst + (((long long)(a * PXr) * (C / 8) + ck) * N + n) * 8 + c8;
        float u[6];
        wino_w_cols(t[a][0], t[a][1], t[a][2], PXr, u);
        o[0] = u[0];
        o[xs] = u[1];
        o[2 * xs] = u[2];
        o[3 * xs] = u[3];
        if (PXr == 6) {
            o[4 * xs] = u[4];
            o[5 * xs] = u[5];
        }
    }
}
