// Fused multi-tensor AdamW (torch.optim.AdamW semantics as wired at train.py:122-126 / optimizers.py:8-9:
// decoupled weight decay, no amsgrad).  One launch updates every parameter tensor of a network:
// HBM-bound, algorithmic bytes = 4 reads + 3 writes of 4 B per element (p, g, m, v -> p, m, v).  mtd_adamw_views: the same launch
// also writes the Winograd and [tap][n][c] views of the 3x3 weights it updates, from the new values and not from memory.
#include "common.h"
#include "wino_weight_transform.h"

namespace {

constexpr int AW_ELEMS = 2048;   // elements per block

// The update of element e; returns the new parameter.  Which products are fused into their sums is WRITTEN here, not left to the
// compiler (it chooses by the code around an expression: adamw_kernel's loop and adamw_views_kernel's tile loop came out
// differently): m and denom are one fma each, v and p round their products first -- the forms adamw_kernel has always had.
__device__ __forceinline__ float adamw_update(const mtd_adamw_tensor& t, long long e, float decay, float beta1, float beta2, float step_size,
                                              float inv_sqrt_bc2, float eps) {
#pragma clang fp contract(off)
    const float g = t.g[e];
    float p = t.p[e] * decay;
    const float m = __builtin_fmaf(beta1, t.m[e], (1.f - beta1) * g);
    const float v = beta2 * t.v[e] + (1.f - beta2) * g * g;
    const float denom = __builtin_fmaf(sqrtf(v), inv_sqrt_bc2, eps);
    p -= step_size * (m / denom);
    t.p[e] = p;
    t.m[e] = m;
    t.v[e] = v;
    return p;
}

__global__ __launch_bounds__(256) void adamw_kernel(const mtd_adamw_tensor* __restrict__ T, int count, float decay, float beta1,
                                                    float beta2, float step_size, float inv_sqrt_bc2, float eps,
                                                    const float* __restrict__ dyn) {
    if (dyn) {      // step-dependent scalars from device memory (hipGraph replay: kernel arguments are frozen)
        decay = dyn[0];
        step_size = dyn[1];
        inv_sqrt_bc2 = dyn[2];
    }
    int acc = 0, ti = -1, local = 0;
    for (int t = 0; t < count; ++t) {
        int nb = (int)((T[t].n + AW_ELEMS - 1) / AW_ELEMS);
        if ((int)blockIdx.x < acc + nb) { ti = t; local = blockIdx.x - acc; break; }
        acc += nb;
    }
    if (ti < 0) return;
    const mtd_adamw_tensor t = T[ti];
    const long long base = (long long)local * AW_ELEMS;
    for (int i = threadIdx.x; i < AW_ELEMS; i += 256) {
        const long long e = base + i;
        if (e < t.n) {
            adamw_update(t, e, decay, beta1, beta2, step_size, inv_sqrt_bc2, eps);
        }
    }
}

// ---- the update and, from the values it has just computed, the derived views of the 3x3 weights (mtd_adamw_views).
// A workgroup of a viewed tensor [N][C][9] owns a tile of 16 n x 16 c filters: 16 runs of 144 contiguous floats.  It updates them
// element by element like adamw_kernel (coalesced over each run) and leaves the new parameters in LDS; then every thread takes one
// filter of the tile per view out of LDS and writes it in that view's order: the Winograd forms [xi][C/8][N][8] with
// wino_weights_kernel's arithmetic (wino_weight_transform.h), the [tap][n][c] pack as a copy.  The tile is square so that both the
// forward view (n, c) and the data-gradient view (c, n) get 512-byte runs of the Winograd layout per position (8 c8 x 16 n).
constexpr int AV_TILE = 16;
constexpr int AV_ROW = AV_TILE * 9;            // floats of one n of the tile
constexpr int AV_LD = AV_ROW + 1;              // its LDS stride: filters of neighbouring n 17 banks apart

__device__ __forceinline__ int adamw_views_blocks(const mtd_adamw_tensor& t, const mtd_adamw_views_span& s) {
    return s.N ? (s.N / AV_TILE) * (s.C / AV_TILE) : (int)((t.n + AW_ELEMS - 1) / AW_ELEMS);
}

__global__ __launch_bounds__(256) void adamw_views_kernel(const mtd_adamw_tensor* __restrict__ T, const mtd_adamw_views_span* __restrict__ S,
                                                          int count, const mtd_wino_weight_desc* __restrict__ W,
                                                          const mtd_pack_desc* __restrict__ P, float decay, float beta1, float beta2,
                                                          float step_size, float inv_sqrt_bc2, float eps, const float* __restrict__ dyn) {
    __shared__ float tile[AV_TILE * AV_LD];
    if (dyn) {
        decay = dyn[0];
        step_size = dyn[1];
        inv_sqrt_bc2 = dyn[2];
    }
    int acc = 0, ti = -1, local = 0;
    for (int t = 0; t < count; ++t) {
        const int nb = adamw_views_blocks(T[t], S[t]);
        if ((int)blockIdx.x < acc + nb) { ti = t; local = blockIdx.x - acc; break; }
        acc += nb;
    }
    if (ti < 0) return;
    const mtd_adamw_tensor t = T[ti];
    const mtd_adamw_views_span s = S[ti];
    if (s.N == 0) {                                // no views: adamw_kernel's block
        const long long base = (long long)local * AW_ELEMS;
        for (int i = threadIdx.x; i < AW_ELEMS; i += 256) {
            const long long e = base + i;
            if (e < t.n) adamw_update(t, e, decay, beta1, beta2, step_size, inv_sqrt_bc2, eps);
        }
        return;
    }
    const int ctiles = s.C / AV_TILE;
    const int n0 = (local / ctiles) * AV_TILE, c0 = (local % ctiles) * AV_TILE;
    for (int i = threadIdx.x; i < AV_TILE * AV_ROW; i += 256) {
        const int row = i / AV_ROW, j = i - row * AV_ROW;
        const long long e = ((long long)(n0 + row) * s.C + c0) * 9 + j;
        tile[row * AV_LD + j] = adamw_update(t, e, decay, beta1, beta2, step_size, inv_sqrt_bc2, eps);
    }
    __syncthreads();
    {   // Winograd views: thread = (c8, n, chunk of 8 c) of the VIEW's tile, c8 fastest like wino_weights_kernel's threads
        const int c8 = threadIdx.x & 7, vn = (threadIdx.x >> 3) & 15, vck = threadIdx.x >> 7, vc = vck * 8 + c8;
        for (int k = 0; k < s.wino_count; ++k) {
            const mtd_wino_weight_desc* w = W + s.wino_first + k;
            const bool fwd = w->sc == 9;           // (n, c) of the view = (n, c) of the weight; else the transposed (data-gradient) view
            const float* f = tile + (fwd ? vn : vc) * AV_LD + (fwd ? vc : vn) * 9;
            float g[3][3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) g[a][b] = f[w->kmap[a * 3 + b]];
            float tt[4][3];
            wino_w_rows(g, tt);
            wino_w_store(w->dst, w->N, w->C, (w->px & 15) == 6 ? 6 : 4, tt, (fwd ? n0 : c0) + vn, (fwd ? c0 : n0) / 8 + vck, c8);
        }
    }
    {   // [tap][n][c] views: thread = (c, n) of the view's tile
        const int vc = threadIdx.x & 15, vn = threadIdx.x >> 4;
        for (int k = 0; k < s.pack_count; ++k) {
            const mtd_pack_desc* d = P + s.pack_first + k;
            const bool fwd = d->sc == 9;
            const float* f = tile + (fwd ? vn : vc) * AV_LD + (fwd ? vc : vn) * 9;
            float* o = d->dst + (long long)((fwd ? n0 : c0) + vn) * d->C + (fwd ? c0 : n0) + vc;
            const long long tstride = (long long)d->N * d->C;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) o[tap * tstride] = f[tap];
        }
    }
}

}  // namespace

extern "C" int mtd_adamw_multi(const mtd_adamw_tensor* tensors_dev, const mtd_adamw_tensor* tensors_host, int count, float lr,
                               float beta1, float beta2, float eps, float wd, int step, void* stream) {
    if (!tensors_dev || !tensors_host || count <= 0 || step <= 0) return MTD_EINVAL;
    long long blocks = 0;
    for (int i = 0; i < count; ++i) {
        if (!tensors_host[i].p || !tensors_host[i].g || !tensors_host[i].m || !tensors_host[i].v || tensors_host[i].n <= 0) return MTD_EINVAL;
        blocks += (tensors_host[i].n + AW_ELEMS - 1) / AW_ELEMS;
    }
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1);
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    const float decay = 1.f - lr * wd;
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tensors_dev, count, decay, beta1, beta2,
                       step_size, inv_sqrt_bc2, eps, (const float*)nullptr);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

// Same update with the three step-dependent scalars precomputed by the caller (FusedAdamW computes them once in
// double precision for both its eager and its captured path, so the two produce identical parameters).
extern "C" int mtd_adamw_multi_pre(const mtd_adamw_tensor* tensors_dev, const mtd_adamw_tensor* tensors_host, int count, float beta1,
                                   float beta2, float eps, float decay, float step_size, float inv_sqrt_bc2, void* stream) {
    if (!tensors_dev || !tensors_host || count <= 0) return MTD_EINVAL;
    long long blocks = 0;
    for (int i = 0; i < count; ++i) {
        if (!tensors_host[i].p || !tensors_host[i].g || !tensors_host[i].m || !tensors_host[i].v || tensors_host[i].n <= 0) return MTD_EINVAL;
        blocks += (tensors_host[i].n + AW_ELEMS - 1) / AW_ELEMS;
    }
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tensors_dev, count, decay, beta1, beta2,
                       step_size, inv_sqrt_bc2, eps, (const float*)nullptr);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

// Same update with (decay, step_size, 1/sqrt(bias_correction2)) read from dyn[0..2] in device memory, so that a
// captured hipGraph can be replayed with a new step count: the host refreshes the three floats before each replay.
extern "C" int mtd_adamw_multi_dyn(const mtd_adamw_tensor* tensors_dev, const mtd_adamw_tensor* tensors_host, int count, float beta1,
                                   float beta2, float eps, const float* dyn, void* stream) {
    if (!tensors_dev || !tensors_host || count <= 0 || !dyn) return MTD_EINVAL;
    long long blocks = 0;
    for (int i = 0; i < count; ++i) {
        if (!tensors_host[i].p || !tensors_host[i].g || !tensors_host[i].m || !tensors_host[i].v || tensors_host[i].n <= 0) return MTD_EINVAL;
        blocks += (tensors_host[i].n + AW_ELEMS - 1) / AW_ELEMS;
    }
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tensors_dev, count, 0.f, beta1, beta2, 0.f,
                       0.f, eps, dyn);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}

// The update plus the derived views of the 3x3 weights in one launch (include/mtdgan_hip.h).  Every view is checked against its
// tensor here: the kernel writes views without bounds checks.
extern "C" int mtd_adamw_views(const mtd_adamw_tensor* tensors_dev, const mtd_adamw_tensor* tensors_host, int count,
                               const mtd_adamw_views_span* spans_dev, const mtd_adamw_views_span* spans_host,
                               const mtd_wino_weight_desc* wino_dev, const mtd_wino_weight_desc* wino_host, int n_wino,
                               const mtd_pack_desc* pack_dev, const mtd_pack_desc* pack_host, int n_pack, float beta1, float beta2,
                               float eps, float decay, float step_size, float inv_sqrt_bc2, const float* dyn, void* stream) {
    if (!tensors_dev || !tensors_host || !spans_dev || !spans_host || count <= 0 || n_wino < 0 || n_pack < 0) return MTD_EINVAL;
    if ((n_wino > 0 && (!wino_dev || !wino_host)) || (n_pack > 0 && (!pack_dev || !pack_host))) return MTD_EINVAL;
    long long blocks = 0;
    for (int i = 0; i < count; ++i) {
        const mtd_adamw_tensor& t = tensors_host[i];
        const mtd_adamw_views_span& s = spans_host[i];
        if (!t.p || !t.g || !t.m || !t.v || t.n <= 0) return MTD_EINVAL;
        if (s.N == 0) {
            if (s.wino_count || s.pack_count) return MTD_EINVAL;
            blocks += (t.n + AW_ELEMS - 1) / AW_ELEMS;
            continue;
        }
        if (s.N < 0 || s.C <= 0 || (s.N % AV_TILE) || (s.C % AV_TILE) || t.n != (long long)s.N * s.C * 9) return MTD_EINVAL;
        if (s.wino_count < 0 || s.pack_count < 0 || s.wino_first < 0 || s.pack_first < 0 ||
            (long long)s.wino_first + s.wino_count > n_wino || (long long)s.pack_first + s.pack_count > n_pack) return MTD_EINVAL;
        // a view is the forward (N, C) or the transposed (C, N) reading of this tensor
        auto shape_ok = [&](const float* src, int vN, int vC, long long sn, long long sc) {
            return src == t.p && ((vN == s.N && vC == s.C && sn == 9LL * s.C && sc == 9) ||
                                  (vN == s.C && vC == s.N && sn == 9 && sc == 9LL * s.C));
        };
        for (int k = 0; k < s.wino_count; ++k) {
            const mtd_wino_weight_desc& w = wino_host[s.wino_first + k];
            if (!w.dst || w.st != 1 || !(w.px == 0 || w.px == 4 || w.px == 6) || !shape_ok(w.src, w.N, w.C, w.sn, w.sc)) return MTD_EINVAL;
            for (int j = 0; j < 9; ++j)
                if (w.kmap[j] < 0 || w.kmap[j] > 8) return MTD_EINVAL;
        }
        for (int k = 0; k < s.pack_count; ++k) {
            const mtd_pack_desc& d = pack_host[s.pack_first + k];
            if (!d.dst || d.T != 9 || !shape_ok(d.src, d.N, d.C, d.sn, d.sc)) return MTD_EINVAL;
        }
        blocks += (long long)(s.N / AV_TILE) * (s.C / AV_TILE);
    }
    if (blocks > 0x7fffffffLL) return MTD_EINVAL;
    hipLaunchKernelGGL(adamw_views_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tensors_dev, spans_dev, count, wino_dev,
                       pack_dev, decay, beta1, beta2, step_size, inv_sqrt_bc2, eps, dyn);
    MTD_LAUNCH_CHECK();
    return MTD_OK;
}
