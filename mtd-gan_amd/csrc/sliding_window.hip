// Sliding-window inference around a patch predictor (inferers.py; the reference evaluates its patch-trained models with
// monai's sliding_window_inference, engine.py:345,378,835): cut roi-sized windows out of whole slices, blend the predictions
// back with an importance map, divide by the summed weights.  Three small memory-bound launches, plain C++; and their
// multi-output forms for a predictor with several outputs (the reference's module/sliding_window.py runs its multi-task
// discriminators this way): up to four planes blended / finished by one launch, and a gather that also flags nonzero windows.
//
// The window list is never materialised.  Per axis of length `size` with roi r and interval iv there are n windows with
//     start(d) = min(d * iv, size - r),   n = ceil((size - r) / iv) + 1   (so (n - 2) * iv < size - r: starts strictly increase),
// and global window g of a (B, H, W) batch is (image, iy, ix) = (g / (ny nx), (g / nx) % ny, g % nx).  Since the starts increase,
// the windows that cover a coordinate c form the contiguous index range [cover_lo(c), cover_hi(c)], found with two divisions.
//
// Blend and finish are in the gather formulation: a thread owns an output pixel and walks its covering windows in increasing
// global index.  No atomics; every sum has one fixed order, and since the running value is carried through the accumulator
// between launches, cutting the window list into chunks differently adds the same terms in the same order: same bits.
// A pixel covered by exactly one window takes that window's prediction as it is (no multiply, no divide), so without
// overlap the result is the plain tiling of the predictions under any importance map.
#include "common.h"

namespace {

struct SwGeom {
    int B, H, W, rh, rw, ny, nx, ivy, ivx;
};

__device__ __forceinline__ int sw_start(int d, int iv, int size, int r) { return min(d * iv, size - r); }
// first / last window index of an axis that covers coordinate c (0 <= c < size)
__device__ __forceinline__ int cover_lo(int c, int iv, int r, int n) { return c < r ? 0 : min((c - r) / iv + 1, n - 1); }
__device__ __forceinline__ int cover_hi(int c, int iv, int size, int r, int n) {
    return c >= sw_start(n - 1, iv, size, r) ? n - 1 : c / iv;
}

// ---- gather: windows [w0, w0 + n) -> (n, rh, rw).  blockIdx.x = window of the chunk (its decode is wave-uniform),
// blockIdx.y * 256 + threadIdx.x = VEC-wide piece of the window.  VEC = 4: rw % 4 == 0 and `out` 16-byte aligned, so every
// store is one 16-byte vector; the load is one as well when the window's first column and the row pitch keep the source
// aligned (uniform per window), four scalar loads otherwise.
template <int VEC>
__global__ __launch_bounds__(256) void sw_gather_kernel(const float* __restrict__ in, float* __restrict__ out, SwGeom g, long long w0,
                                                        int src_vec_ok) {
    const long long gw = w0 + blockIdx.x;
    const int per = g.ny * g.nx;
    const int b = (int)(gw / per), r = (int)(gw - (long long)b * per);
    const int iy = r / g.nx, ix = r - iy * g.nx;
    const int y0 = sw_start(iy, g.ivy, g.H, g.rh), x0 = sw_start(ix, g.ivx, g.W, g.rw);
    const int cols = g.rw / VEC;
    const int e = blockIdx.y * 256 + threadIdx.x;
    if (e >= g.rh * cols) return;
    const int ry = e / cols, cx = (e - ry * cols) * VEC;
    const float* src = in + ((long long)b * g.H + y0 + ry) * g.W + x0 + cx;
    float* dst = out + ((long long)blockIdx.x * g.rh + ry) * g.rw + cx;
    if (VEC == 4) {
        f32x4 v;
        if (src_vec_ok && (x0 & 3) == 0) v = *reinterpret_cast<const f32x4*>(src);
        else v = f32x4{src[0], src[1], src[2], src[3]};
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
        dst[0] = src[0];
    }
}

// ---- blend: acc(B, H, W) += sum over the chunk's windows [w0, w1) of map * pred.  Launched over the rows [ylo, ylo + gridDim.y)
// and columns [xlo, xlo + gridDim.x * 256) that bound the chunk, images b0 + blockIdx.z; a pixel that no window of the chunk
// covers returns before it loads or stores anything.
__global__ __launch_bounds__(256) void sw_blend_kernel(const float* __restrict__ pred, const float* __restrict__ map, float* __restrict__ acc,
                                                       SwGeom g, long long w0, long long w1, int b0, int ylo, int xlo, int xhi) {
    const int x = xlo + blockIdx.x * 256 + threadIdx.x;
    const int y = ylo + blockIdx.y, b = b0 + blockIdx.z;
    if (x >= xhi) return;
    const int iy0 = cover_lo(y, g.ivy, g.rh, g.ny), iy1 = cover_hi(y, g.ivy, g.H, g.rh, g.ny);
    const int ix0 = cover_lo(x, g.ivx, g.rw, g.nx), ix1 = cover_hi(x, g.ivx, g.W, g.rw, g.nx);
    // the chunk's share of this image's windows, [lo, hi] in (iy * nx + ix), intersected with the covering ranges
    const long long per = (long long)g.ny * g.nx, base = (long long)b * per;
    const long long lo = max(w0 - base, 0ll), hi = min(w1 - base, per) - 1;
    if (hi < lo) return;
    const int iya = max(iy0, (int)(lo / g.nx)), iyb = min(iy1, (int)(hi / g.nx));
    const bool single = iy0 == iy1 && ix0 == ix1;
    float* a = acc + ((long long)b * g.H + y) * g.W + x;
    float s = 0.f;
    bool any = false;
    for (int iy = iya; iy <= iyb; ++iy) {
        const int dy = y - sw_start(iy, g.ivy, g.H, g.rh);
        const long long row = (long long)iy * g.nx;
        const int ixa = (int)max((long long)ix0, lo - row), ixb = (int)min((long long)ix1, hi - row);
        for (int ix = ixa; ix <= ixb; ++ix) {
            if (!any) { s = *a; any = true; }
            const int o = dy * g.rw + (x - sw_start(ix, g.ivx, g.W, g.rw));
            const float p = pred[(base + row + ix - w0) * g.rh * g.rw + o];
            s = single ? p : __builtin_fmaf(map[o], p, s);
        }
    }
    if (any) *a = s;
}

// ---- finish: out = acc / wsum (acc itself where one window covers the pixel), wsum = the map summed over the covering windows
// in the blend's order -- recomputed here from the geometry, never stored.  out may be acc.
__global__ __launch_bounds__(256) void sw_finish_kernel(const float* acc, const float* __restrict__ map, float* out, SwGeom g, int clip) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, b = blockIdx.z;
    if (x >= g.W) return;
    const int iy0 = cover_lo(y, g.ivy, g.rh, g.ny), iy1 = cover_hi(y, g.ivy, g.H, g.rh, g.ny);
    const int ix0 = cover_lo(x, g.ivx, g.rw, g.nx), ix1 = cover_hi(x, g.ivx, g.W, g.rw, g.nx);
    const long long i = ((long long)b * g.H + y) * g.W + x;
    float v = acc[i];
    if (!(iy0 == iy1 && ix0 == ix1)) {
        float ws = 0.f;
        for (int iy = iy0; iy <= iy1; ++iy) {
            const int dy = y - sw_start(iy, g.ivy, g.H, g.rh);
            for (int ix = ix0; ix <= ix1; ++ix) ws += map[dy * g.rw + (x - sw_start(ix, g.ivx, g.W, g.rw))];
        }
        v = v / ws;
    }
    if (clip) v = fminf(fmaxf(v, 0.f), 1.f);
    out[i] = v;
}

// ---- gather + flags: sw_gather_kernel plus one byte per window of the chunk, 1 if the window holds an element != 0.0f (so -0.0f
// counts as zero and a NaN as nonzero).  flags[0, n) is zeroed by the entry before this launch; several workgroups serve one
// window and every wave that saw a nonzero element stores the constant 1 from its first lane: a plain byte store, whoever
// comes last writes the same value.
template <int VEC>
__global__ __launch_bounds__(256) void sw_gather_flags_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                              unsigned char* __restrict__ flags, SwGeom g, long long w0, int src_vec_ok) {
    const long long gw = w0 + blockIdx.x;
    const int per = g.ny * g.nx;
    const int b = (int)(gw / per), r = (int)(gw - (long long)b * per);
    const int iy = r / g.nx, ix = r - iy * g.nx;
    const int y0 = sw_start(iy, g.ivy, g.H, g.rh), x0 = sw_start(ix, g.ivx, g.W, g.rw);
    const int cols = g.rw / VEC;
    const int e = blockIdx.y * 256 + threadIdx.x;
    if (e >= g.rh * cols) return;              // e grows with the lane: a wave whose first lane left has left altogether
    const int ry = e / cols, cx = (e - ry * cols) * VEC;
    const float* src = in + ((long long)b * g.H + y0 + ry) * g.W + x0 + cx;
    float* dst = out + ((long long)blockIdx.x * g.rh + ry) * g.rw + cx;
    bool nz;
    if (VEC == 4) {
        f32x4 v;
        if (src_vec_ok && (x0 & 3) == 0) v = *reinterpret_cast<const f32x4*>(src);
        else v = f32x4{src[0], src[1], src[2], src[3]};
        *reinterpret_cast<f32x4*>(dst) = v;
        nz = v[0] != 0.f || v[1] != 0.f || v[2] != 0.f || v[3] != 0.f;
    } else {
        const float v = src[0];
        dst[0] = v;
        nz = v != 0.f;
    }
    if (__any(nz) && (threadIdx.x & 63) == 0) flags[blockIdx.x] = 1;
}

// ---- multi-plane blend and finish: up to SW_MAX_PLANES outputs of one predictor pass in one launch.  The descriptors travel in
// the kernel arguments by value and every loop over them is unrolled over the template's plane count, so p[k] is a set of
// scalar registers (an array indexed at run time would live in scratch).  Per plane the operation sequence is sw_blend_kernel's
// / sw_finish_kernel's: the same bits as one single-plane launch per plane.
enum { SW_MAX_PLANES = 4 };
struct SwBlendPlane {
    const float* pred;      // map: (n, rh, rw); window scalar: (n)
    float* acc;             // (B, H, W)
    int scalar;             // 1: every pixel of window w contributes pred[w]
};
struct SwBlendPlanes { SwBlendPlane p[SW_MAX_PLANES]; };
struct SwFinishPlane {
    const float* acc;
    float* out;             // may be acc
    int clip;
};
struct SwFinishPlanes { SwFinishPlane p[SW_MAX_PLANES]; };

template <int NP>
__global__ __launch_bounds__(256) void sw_blend_multi_kernel(SwBlendPlanes P, const float* __restrict__ map, SwGeom g, long long w0,
                                                             long long w1, int b0, int ylo, int xlo, int xhi) {
    const int x = xlo + blockIdx.x * 256 + threadIdx.x;
    const int y = ylo + blockIdx.y, b = b0 + blockIdx.z;
    if (x >= xhi) return;
    const int iy0 = cover_lo(y, g.ivy, g.rh, g.ny), iy1 = cover_hi(y, g.ivy, g.H, g.rh, g.ny);
    const int ix0 = cover_lo(x, g.ivx, g.rw, g.nx), ix1 = cover_hi(x, g.ivx, g.W, g.rw, g.nx);
    const long long per = (long long)g.ny * g.nx, base = (long long)b * per;
    const long long lo = max(w0 - base, 0ll), hi = min(w1 - base, per) - 1;
    if (hi < lo) return;
    const int iya = max(iy0, (int)(lo / g.nx)), iyb = min(iy1, (int)(hi / g.nx));
    const bool single = iy0 == iy1 && ix0 == ix1;
    const long long pix = ((long long)b * g.H + y) * g.W + x;
    float s[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) s[k] = 0.f;
    bool any = false;
    for (int iy = iya; iy <= iyb; ++iy) {
        const int dy = y - sw_start(iy, g.ivy, g.H, g.rh);
        const long long row = (long long)iy * g.nx;
        const int ixa = (int)max((long long)ix0, lo - row), ixb = (int)min((long long)ix1, hi - row);
        for (int ix = ixa; ix <= ixb; ++ix) {
            if (!any) {
#pragma unroll
                for (int k = 0; k < NP; ++k) s[k] = P.p[k].acc[pix];
                any = true;
            }
            const int o = dy * g.rw + (x - sw_start(ix, g.ivx, g.W, g.rw));
            const long long w = base + row + ix - w0;
            const float m = map[o];
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const float p = P.p[k].scalar ? P.p[k].pred[w] : P.p[k].pred[w * g.rh * g.rw + o];
                s[k] = single ? p : __builtin_fmaf(m, p, s[k]);
            }
        }
    }
    if (any) {
#pragma unroll
        for (int k = 0; k < NP; ++k) P.p[k].acc[pix] = s[k];
    }
}

template <int NP>
__global__ __launch_bounds__(256) void sw_finish_multi_kernel(SwFinishPlanes P, const float* __restrict__ map, SwGeom g) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, b = blockIdx.z;
    if (x >= g.W) return;
    const int iy0 = cover_lo(y, g.ivy, g.rh, g.ny), iy1 = cover_hi(y, g.ivy, g.H, g.rh, g.ny);
    const int ix0 = cover_lo(x, g.ivx, g.rw, g.nx), ix1 = cover_hi(x, g.ivx, g.W, g.rw, g.nx);
    const long long i = ((long long)b * g.H + y) * g.W + x;
    const bool single = iy0 == iy1 && ix0 == ix1;
    float ws = 0.f;
    if (!single) {
        for (int iy = iy0; iy <= iy1; ++iy) {
            const int dy = y - sw_start(iy, g.ivy, g.H, g.rh);
            for (int ix = ix0; ix <= ix1; ++ix) ws += map[dy * g.rw + (x - sw_start(ix, g.ivx, g.W, g.rw))];
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        float v = P.p[k].acc[i];
        if (!single) v = v / ws;
        if (P.p[k].clip) v = fminf(fmaxf(v, 0.f), 1.f);
        P.p[k].out[i] = v;
    }
}

// number of windows of an axis under the start rule, or 0 when (size, r, iv) are no valid axis
int sw_axis_count(int size, int r, int iv) {
    if (r <= 0 || size < r || iv <= 0 || iv > r) return 0;
    if (size == r) return 1;
    return (size - r + iv - 1) / iv + 1;
}
int sw_host_start(int d, int iv, int size, int r) { return d * iv < size - r ? d * iv : size - r; }

// validates the geometry shared by the three entries; total windows in *total
bool sw_geom(int B, int H, int W, int rh, int rw, int ivy, int ivx, SwGeom* g, long long* total) {
    if (B <= 0 || H <= 0 || W <= 0) return false;
    const int ny = sw_axis_count(H, rh, ivy), nx = sw_axis_count(W, rw, ivx);
    if (ny == 0 || nx == 0) return false;
    if ((long long)B * H * W >= (1ll << 31) || (long long)ny * nx >= (1ll << 31) || H > 65535 || B > 65535) return false;
    *g = SwGeom{B, H, W, rh, rw, ny, nx, ivy, ivx};
    *total = (long long)B * ny * nx;
    return true;
}

// the rows [ylo, yhi), columns [xlo, xhi) and images [b0, b1] that bound the chunk [w0, w0 + n): O(1) host arithmetic on its
// first and last window
struct SwBounds {
    int b0, b1, ylo, yhi, xlo, xhi;
};
SwBounds sw_chunk_bounds(const SwGeom& g, long long w0, int n) {
    const long long per = (long long)g.ny * g.nx, wl = w0 + n - 1;
    const int b0 = (int)(w0 / per), b1 = (int)(wl / per);
    const int iyf = (int)((w0 - b0 * per) / g.nx), ixf = (int)((w0 - b0 * per) % g.nx);
    const int iyl = (int)((wl - b1 * per) / g.nx), ixl = (int)((wl - b1 * per) % g.nx);
    SwBounds c{b0, b1, 0, g.H, 0, g.W};
    if (b0 == b1) {
        c.ylo = sw_host_start(iyf, g.ivy, g.H, g.rh);
        c.yhi = sw_host_start(iyl, g.ivy, g.H, g.rh) + g.rh;
        if (iyf == iyl) {
            c.xlo = sw_host_start(ixf, g.ivx, g.W, g.rw);
            c.xhi = sw_host_start(ixl, g.ivx, g.W, g.rw) + g.rw;
        }
    }
    return c;
}

}  // namespace

extern "C" int mtd_sw_gather(const float* in, int B, int H, int W, int rh, int rw, int ivy, int ivx, long long w0, int n, float* out,
                             void* stream) {
    SwGeom g;
    long long total;
    if (!in || !out || !sw_geom(B, H, W, rh, rw, ivy, ivx, &g, &total)) return MTD_EINVAL;
    if (w0 < 0 || n <= 0 || w0 + n > total || (long long)n * rh * rw >= (1ll << 31)) return MTD_EINVAL;
    if ((long long)rh * rw > 65535ll * 256) return MTD_EINVAL;      // (grid.y; a roi of 16M pixels is no window)
    hipStream_t s = (hipStream_t)stream;
    if ((rw & 3) == 0 && aligned16(out)) {
        const int pieces = rh * (rw / 4);
        const int src_vec_ok = aligned16(in) && (W & 3) == 0;
        hipLaunchKernelGGL(sw_gather_kernel<4>, dim3(n, (pieces + 255) / 256), dim3(256), 0, s, in, out, g, w0, src_vec_ok);
    } else {
        const int pieces = rh * rw;
        hipLaunchKernelGGL(sw_gather_kernel<1>, dim3(n, (pieces + 255) / 256), dim3(256), 0, s, in, out, g, w0, 0);
    }
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_sw_gather_flags(const float* in, int B, int H, int W, int rh, int rw, int ivy, int ivx, long long w0, int n, float* out,
                                   unsigned char* flags, void* stream) {
    SwGeom g;
    long long total;
    if (!in || !out || !flags || !sw_geom(B, H, W, rh, rw, ivy, ivx, &g, &total)) return MTD_EINVAL;
    if (w0 < 0 || n <= 0 || w0 + n > total || (long long)n * rh * rw >= (1ll << 31)) return MTD_EINVAL;
    if ((long long)rh * rw > 65535ll * 256) return MTD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(flags, 0, (size_t)n, s);
    if (e != hipSuccess) return (int)e;
    if ((rw & 3) == 0 && aligned16(out)) {
        const int pieces = rh * (rw / 4);
        const int src_vec_ok = aligned16(in) && (W & 3) == 0;
        hipLaunchKernelGGL(sw_gather_flags_kernel<4>, dim3(n, (pieces + 255) / 256), dim3(256), 0, s, in, out, flags, g, w0, src_vec_ok);
    } else {
        const int pieces = rh * rw;
        hipLaunchKernelGGL(sw_gather_flags_kernel<1>, dim3(n, (pieces + 255) / 256), dim3(256), 0, s, in, out, flags, g, w0, 0);
    }
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_sw_blend(const float* pred, const float* map, int B, int H, int W, int rh, int rw, int ivy, int ivx, long long w0,
                            int n, float* acc, void* stream) {
    SwGeom g;
    long long total;
    if (!pred || !map || !acc || !sw_geom(B, H, W, rh, rw, ivy, ivx, &g, &total)) return MTD_EINVAL;
    if (w0 < 0 || n <= 0 || w0 + n > total || (long long)n * rh * rw >= (1ll << 31)) return MTD_EINVAL;
    const SwBounds c = sw_chunk_bounds(g, w0, n);
    hipLaunchKernelGGL(sw_blend_kernel, dim3((c.xhi - c.xlo + 255) / 256, c.yhi - c.ylo, c.b1 - c.b0 + 1), dim3(256), 0, (hipStream_t)stream,
                       pred, map, acc, g, w0, w0 + n, c.b0, c.ylo, c.xlo, c.xhi);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_sw_blend_multi(int nplanes, const float* const* preds, const int* scalar, float* const* accs, const float* map, int B,
                                  int H, int W, int rh, int rw, int ivy, int ivx, long long w0, int n, void* stream) {
    SwGeom g;
    long long total;
    if (nplanes < 1 || nplanes > SW_MAX_PLANES || !preds || !scalar || !accs || !map) return MTD_EINVAL;
    if (!sw_geom(B, H, W, rh, rw, ivy, ivx, &g, &total)) return MTD_EINVAL;
    if (w0 < 0 || n <= 0 || w0 + n > total || (long long)n * rh * rw >= (1ll << 31)) return MTD_EINVAL;
    SwBlendPlanes P = {};
    for (int k = 0; k < nplanes; ++k) {
        if (!preds[k] || !accs[k]) return MTD_EINVAL;
        P.p[k] = SwBlendPlane{preds[k], accs[k], scalar[k] ? 1 : 0};
    }
    const SwBounds c = sw_chunk_bounds(g, w0, n);
    const dim3 grid((c.xhi - c.xlo + 255) / 256, c.yhi - c.ylo, c.b1 - c.b0 + 1);
    hipStream_t s = (hipStream_t)stream;
#define SW_BLEND_MULTI(NP) \
    hipLaunchKernelGGL(sw_blend_multi_kernel<NP>, grid, dim3(256), 0, s, P, map, g, w0, w0 + n, c.b0, c.ylo, c.xlo, c.xhi)
    switch (nplanes) {
        case 1: SW_BLEND_MULTI(1); break;
        case 2: SW_BLEND_MULTI(2); break;
        case 3: SW_BLEND_MULTI(3); break;
        default: SW_BLEND_MULTI(4); break;
    }
#undef SW_BLEND_MULTI
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_sw_finish_multi(int nplanes, const float* const* accs, const int* clip01, float* const* outs, const float* map, int B,
                                   int H, int W, int rh, int rw, int ivy, int ivx, void* stream) {
    SwGeom g;
    long long total;
    if (nplanes < 1 || nplanes > SW_MAX_PLANES || !accs || !clip01 || !outs || !map) return MTD_EINVAL;
    if (!sw_geom(B, H, W, rh, rw, ivy, ivx, &g, &total)) return MTD_EINVAL;
    SwFinishPlanes P = {};
    for (int k = 0; k < nplanes; ++k) {
        if (!accs[k] || !outs[k]) return MTD_EINVAL;
        P.p[k] = SwFinishPlane{accs[k], outs[k], clip01[k] ? 1 : 0};
    }
    const dim3 grid((W + 255) / 256, H, B);
    hipStream_t s = (hipStream_t)stream;
#define SW_FINISH_MULTI(NP) hipLaunchKernelGGL(sw_finish_multi_kernel<NP>, grid, dim3(256), 0, s, P, map, g)
    switch (nplanes) {
        case 1: SW_FINISH_MULTI(1); break;
        case 2: SW_FINISH_MULTI(2); break;
        case 3: SW_FINISH_MULTI(3); break;
        default: SW_FINISH_MULTI(4); break;
    }
#undef SW_FINISH_MULTI
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

extern "C" int mtd_sw_finish(const float* acc, const float* map, int B, int H, int W, int rh, int rw, int ivy, int ivx, int clip01,
                             float* out, void* stream) {
    SwGeom g;
    long long total;
    if (!acc || !map || !out || !sw_geom(B, H, W, rh, rw, ivy, ivx, &g, &total)) return MTD_EINVAL;
    hipLaunchKernelGGL(sw_finish_kernel, dim3((W + 255) / 256, H, B), dim3(256), 0, (hipStream_t)stream, acc, map, out, g, clip01 ? 1 : 0);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
