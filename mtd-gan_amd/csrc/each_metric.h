// The framework of an image-by-image metric of the test loop: up to three sources a[k] of B images each against
// one target b, an image's numbers depending neither on its batch, nor on its source slot, nor on the other sources.
//   * the image sets travel as kernel arguments and are picked with a chain of selects (no dynamically indexed array: the
//     pointers stay in scalar registers); an image set passed twice is one set, transformed once;
//   * a tile kernel leaves Q sums per workgroup at Q * (its linear index), so the partials of one (source, image) are contiguous;
//     one workgroup per (source, image) folds them in a fixed order -- thread t takes tiles t, t + 256, ..., then block_sum256's
//     tree -- and writes out[source * B + i0 + i];
//   * a metric with a workspace per image walks the batch in chunks of each_chunk() images.
// A helper with a contractible expression fixes its own contraction state: the including files differ in theirs.
#pragma once
#include "common.h"

namespace {

struct EachSets { const float* p[4]; };        // image sets, B images each
struct EachMap { int src[3]; int tgt; };       // set of source k, set of the target

__device__ __forceinline__ const float* each_pick(const EachSets& s, int k) { return k == 0 ? s.p[0] : (k == 1 ? s.p[1] : (k == 2 ? s.p[2] : s.p[3])); }
__device__ __forceinline__ int each_pick(const EachMap& m, int k) { return k == 0 ? m.src[0] : (k == 1 ? m.src[1] : m.src[2]); }

// sums[q] <- the sum over the image's tiles of p[Q * tile + q]; valid in thread 0.  `red` holds Q * 256 doubles.
template <int Q>
__device__ __forceinline__ void each_fold(const double* __restrict__ p, int tiles, double (&sums)[Q], double* red) {
#pragma unroll
    for (int q = 0; q < Q; ++q) sums[q] = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 256) {
#pragma unroll
        for (int q = 0; q < Q; ++q) sums[q] += p[Q * t + q];
    }
    block_sum256(sums, red);
}

__device__ __forceinline__ long long each_block() { return ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; }

// thread 0 stores the workgroup's Q sums where each_fold looks for them
template <int Q>
__device__ __forceinline__ void each_store(double* __restrict__ partial, const double (&sums)[Q]) {
    if (threadIdx.x != 0) return;
    const long long blk = each_block();
#pragma unroll
    for (int q = 0; q < Q; ++q) partial[Q * blk + q] = sums[q];
}

// piq's similarity_map.  Without contraction into fused multiply-adds, so that equal maps give a ratio of exactly 1.
__device__ __forceinline__ double each_similarity(double a, double b, double c) {
#pragma clang fp contract(off)
    return (2.0 * a * b + c) / (a * a + b * b + c);
}

// The distinct image sets among the target and the na sources (set 0 is the target's) and who uses which.  -> their number, or
// -1 on a null source.
inline int each_sets(const void* const* srcs, int na, const void* target, EachSets& sets, EachMap& map) {
    sets = {};
    map = {};
    int n = 0;
    sets.p[n] = (const float*)target;
    map.tgt = n++;
    for (int a = 0; a < na; ++a) {
        if (!srcs[a]) return -1;
        int at = -1;
        for (int d = 0; d < n; ++d)
            if (sets.p[d] == (const float*)srcs[a]) at = d;
        if (at < 0) {
            sets.p[n] = (const float*)srcs[a];
            at = n++;
        }
        map.src[a] = at;
    }
    return n;
}

// Images of a chunk: as many as keep the workspace within `target_bytes`, at least 1, at most B and 8192 (sets * chunk and
// na * chunk index a grid dimension).
inline int each_chunk(long long target_bytes, long long bytes_per_image, int B) {
    long long c = target_bytes / bytes_per_image;
    c = c < 1 ? 1 : (c > B ? B : c);
    return (int)(c > 8192 ? 8192 : c);
}

inline bool each_finite(double v) { return v == v && v - v == 0.0; }

}  // namespace
