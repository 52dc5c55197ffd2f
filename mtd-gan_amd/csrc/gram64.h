// What the float64 MFMA kernels share: the accumulator type of v_mfma_f64_16x16x4_f64 (fid.hip, kid.hip, msid.hip) and the fetch
// of four fp32 values of a feature row that kid_gram_sums_kernel and msid_dist_kernel widen on the way into LDS.
#pragma once
#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

// four consecutive k of one feature row, as stored; row < 0: zeros
__device__ __forceinline__ void gram64_fetch(const float* __restrict__ F, int row, int D, int kb, bool vec, float (&r)[4]) {
    if (row >= 0 && vec && kb + 3 < D) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(F + (long long)row * D + kb);
        r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = (row >= 0 && kb + q < D) ? F[(long long)row * D + kb + q] : 0.f;
    }
}

}  // namespace
