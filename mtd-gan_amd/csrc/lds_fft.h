// Radix-2 transforms of lines held in LDS, by the 256 threads of a workgroup: shared by csrc/fsim.hip and
// csrc/vsi.hip.  fp32, twiddles rounded from double; the bit reversal happens in the LDS address of the caller's
// load, so every array in memory is in natural order.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int fs_brev(int i, int ln) { return (int)(__brev((unsigned)i) >> (32 - ln)); }

// tw[t] = e^{2 pi i t / n}, t < n / 2 <= 256, rounded from double.
__device__ __forceinline__ void fs_twiddles(float2* tw, int n) {
    const int t = threadIdx.x;
    if (t < n / 2) {
        double s, c;
        sincospi(2.0 * (double)t / (double)n, &s, &c);
        tw[t] = make_float2((float)c, (float)s);
    }
}

// In-place transforms of `lines` lines of n = 2^ln complex points in LDS (line l at buf + l * ld), by the 256 threads of the
// workgroup: X[k] = sum_j x[j] e^{SIGN 2 pi i j k / n}, unnormalised.  Radix-2 decimation in time: the input is in bit-reversed
// order, the output in natural order.  The caller has synchronised after its stores (and after fs_twiddles); the function ends
// with a barrier.
template <int SIGN>
__device__ __forceinline__ void fs_lds_fft(float2* buf, int lines, int ln, int ld, const float2* tw) {
    const int total = lines << (ln - 1);
    const int jm = (1 << (ln - 1)) - 1;
    for (int s = 1; s <= ln; ++s) {
        const int half = 1 << (s - 1);
        for (int e = threadIdx.x; e < total; e += 256) {
            const int l = e >> (ln - 1), j = e & jm;
            const int k = j & (half - 1);
            float2* p = buf + l * ld + ((j >> (s - 1)) << s) + k;
            const float2 w = tw[k << (ln - s)];
            const float2 u = p[0], v = p[half];
            float tr, ti;
            if (SIGN > 0) { tr = v.x * w.x - v.y * w.y; ti = v.x * w.y + v.y * w.x; }
            else { tr = v.x * w.x + v.y * w.y; ti = v.y * w.x - v.x * w.y; }
            p[0] = make_float2(u.x + tr, u.y + ti);
            p[half] = make_float2(u.x - tr, u.y - ti);
        }
        __syncthreads();
    }
}
