// Sliding-window inference around a patch predictor (inferers.py; the reference evaluates its patch-trained models with
// monai's sliding_window_inference, engine.py:345,378,835): cut roi-sized windows out of whole slices, blend the predictions
// back with an importance map, divide by the summed weights.  Three small memory-bound launches, plain C++.
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

extern "C" int mtd_sw_blend(const float* pred, const float* map, int B, int H, int W, int rh, int rw, int ivy, int ivx, long long w0,
                            int n, float* acc, void* stream) {
    SwGeom g;
    long long total;
    if (!pred || !map || !acc || !sw_geom(B, H, W, rh, rw, ivy, ivx, &g, &total)) return MTD_EINVAL;
    if (w0 < 0 || n <= 0 || w0 + n > total || (long long)n * rh * rw >= (1ll << 31)) return MTD_EINVAL;
    // the rows, columns and images that bound the chunk: O(1) host arithmetic on its first and last window
    const long long per = (long long)g.ny * g.nx, wl = w0 + n - 1;
    const int b0 = (int)(w0 / per), b1 = (int)(wl / per);
    const int iyf = (int)((w0 - b0 * per) / g.nx), ixf = (int)((w0 - b0 * per) % g.nx);
    const int iyl = (int)((wl - b1 * per) / g.nx), ixl = (int)((wl - b1 * per) % g.nx);
    int ylo = 0, yhi = H, xlo = 0, xhi = W;
    if (b0 == b1) {
        ylo = sw_host_start(iyf, ivy, H, rh);
        yhi = sw_host_start(iyl, ivy, H, rh) + rh;
        if (iyf == iyl) {
            xlo = sw_host_start(ixf, ivx, W, rw);
            xhi = sw_host_start(ixl, ivx, W, rw) + rw;
        }
    }
    hipLaunchKernelGGL(sw_blend_kernel, dim3((xhi - xlo + 255) / 256, yhi - ylo, b1 - b0 + 1), dim3(256), 0, (hipStream_t)stream, pred, map,
                       acc, g, w0, w0 + n, b0, ylo, xlo, xhi);
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
