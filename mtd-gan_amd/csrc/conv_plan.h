// The planners of the forward and data-gradient convs: layer arguments in; kernel, tile shape and split of K out.  Plain C++17 host
// arithmetic (no HIP header: tests/conv_plan_dump.cpp compiles it with g++), included by conv_igemm.hip and through it by
// conv_winograd.hip (with conv_wino_s2.h) and conv_c32_bwd.hip.  tests/golden/conv_plans.csv pins every result over a grid of
// layer shapes (tests/test_conv_plan_cpu.py).
#pragma once
#include <stddef.h>
#include "host_util.h"

namespace {

// ---- the kernels of the conv family (profiler family 0).  The numbers are an interface: the profiler's records,
// kernels.IGEMM_CONFIGS, mtd_conv_igemm_override (0 .. 10), tests and tools index by them.
enum ConvKernel : int {
    CK_AUTO = -1,                                                   // mtd_conv_igemm_override: the default rule
    CK_IGEMM_256x32 = 0, CK_IGEMM_128x32, CK_IGEMM_256x64, CK_IGEMM_64x64, CK_IGEMM_128x128, CK_IGEMM_32x128,      // igemm_kernel: BM x BN
    CK_TB_128x32, CK_TB_256x32,                                     // tap-block kernel with one / two blocks per wave
    CK_V2_128x128,                                                  // both operands through LDS by LDS-DMA
    CK_C32P,                                                        // persistent kernel of the generator-shaped layers
    CK_C32T,                                                        // halo-tile kernel of the generator-shaped layers on 64-pixel rows
    CK_C32_BWD,                                                     // conv_c32_bwd.hip: data and weight gradient in one launch
    CK_C32T_TAIL,                                                   // Res-FFT block tail (mtd_resfft_block_tail)
    CK_C32_BWD_IRFFT,                                               // conv_c32_bwd.hip: ... closing the backward pass of a Res-FFT block
    CK_WINO_NB2, CK_WINO_NB4,                                       // Winograd F(2x2, 3x3): 64- / 128-channel workgroups
    CK_MULTI_256x32, CK_MULTI_128x32, CK_MULTI_256x64, CK_MULTI_64x64, CK_MULTI_128x128, CK_MULTI_32x128,         // igemm_multi_kernel
    CK_WINO_NB2_LEAN,                                               // ... two lean workgroups per CU
    CK_WINO6_NB2, CK_WINO6_NB1,                                     // Winograd F(2x4, 3x3): 64- / 32-channel workgroups
    CK_WINO_C32, CK_WINO_C32_ADD,                                   // the persistent 32 -> 32 channel form (conv_wino_c32.h)
    CK_WINO3_PX6, CK_WINO3_PX4,                                     // the split-bf16 forms (conv_winograd_split.h)
    CK_WINO32_NB2, CK_WINO32_NB2_LEAN, CK_WINO32_NB4,               // F(3x3, 2x2) of the 4x4 / stride-2 layers (conv_wino_s2.h)
    CK_WINO_C32_MASK, CK_WINO_C32_MASK_ADD,                         // ... with a mask operand and a second output
    CK_WINO_MULTI6_NB2, CK_WINO_MULTI_NB2, CK_WINO_MULTI_NB4, CK_WINO_MULTI_NB2_LEAN,      // two or three problems of one shape per launch
    CK_WINO_C32_F16, CK_WINO_C32_F16_ADD,                           // binary16 activation storage (whole-slice inference)
    CK_COUNT
};
constexpr int CK_FORCE_TILES = CK_V2_128x128 + 1;                   // overrides below this number name a tile kernel

// name: the kernel symbol of a rocprofv3 table (kernels.IGEMM_CONFIGS).  WM x WN accumulator blocks of 32 x 32 per wave, WGM x
// WGN waves per workgroup: the template arguments of the tile kernels (the tap-block kernels have WM alone, igemm_v2_kernel is
// built for 2, 2, 2, 2), and the workgroup tile is BM = 32 WM WGM pixels by BN = 32 WN WGN channels.  multi: the kernel's form
// that takes several problems of one shape in one launch.
struct ConvKernelDesc { const char* name; int WM, WN, WGM, WGN; ConvKernel multi; };
constexpr ConvKernelDesc kConvKernel[CK_COUNT] = {
    {"igemm_kernel<2, 1, 4, 1>", 2, 1, 4, 1, CK_MULTI_256x32},
    {"igemm_kernel<1, 1, 4, 1>", 1, 1, 4, 1, CK_MULTI_128x32},
    {"igemm_kernel<2, 2, 4, 1>", 2, 2, 4, 1, CK_MULTI_256x64},
    {"igemm_kernel<1, 1, 2, 2>", 1, 1, 2, 2, CK_MULTI_64x64},
    {"igemm_kernel<2, 2, 2, 2>", 2, 2, 2, 2, CK_MULTI_128x128},
    {"igemm_kernel<1, 1, 1, 4>", 1, 1, 1, 4, CK_MULTI_32x128},
    {"igemm_tb_kernel<1>", 1, 1, 4, 1, CK_AUTO},
    {"igemm_tb_kernel<2>", 2, 1, 4, 1, CK_AUTO},
    {"igemm_v2_kernel<0>", 2, 2, 2, 2, CK_AUTO},
    {"igemm_c32p_kernel", 0, 0, 0, 0, CK_AUTO},
    {"igemm_c32t_kernel", 0, 0, 0, 0, CK_AUTO},
    {"c32_bwd_kernel", 0, 0, 0, 0, CK_AUTO},
    {"igemm_c32t_kernel<4, true, true, true>", 0, 0, 0, 0, CK_AUTO},
    {"c32_bwd_kernel<1, true>", 0, 0, 0, 0, CK_AUTO},
    {"wino_conv_kernel<2, false, 4>", 0, 0, 0, 0, CK_WINO_MULTI_NB2},
    {"wino_conv_kernel<4, false, 4>", 0, 0, 0, 0, CK_WINO_MULTI_NB4},
    {"igemm_multi_kernel<2, 1, 4, 1>", 2, 1, 4, 1, CK_AUTO},
    {"igemm_multi_kernel<1, 1, 4, 1>", 1, 1, 4, 1, CK_AUTO},
    {"igemm_multi_kernel<2, 2, 4, 1>", 2, 2, 4, 1, CK_AUTO},
    {"igemm_multi_kernel<1, 1, 2, 2>", 1, 1, 2, 2, CK_AUTO},
    {"igemm_multi_kernel<2, 2, 2, 2>", 2, 2, 2, 2, CK_AUTO},
    {"igemm_multi_kernel<1, 1, 1, 4>", 1, 1, 1, 4, CK_AUTO},
    {"wino_conv_kernel<2, true, 4>", 0, 0, 0, 0, CK_WINO_MULTI_NB2_LEAN},
    {"wino_conv_kernel<2, false, 6>", 0, 0, 0, 0, CK_WINO_MULTI6_NB2},
    {"wino_conv_kernel<1, false, 6>", 0, 0, 0, 0, CK_AUTO},
    {"wino_c32_kernel<false, false>", 0, 0, 0, 0, CK_AUTO},
    {"wino_c32_kernel<true, false>", 0, 0, 0, 0, CK_AUTO},
    {"wino_conv3_kernel<6>", 0, 0, 0, 0, CK_AUTO},
    {"wino_conv3_kernel<4>", 0, 0, 0, 0, CK_AUTO},
    {"wino32_conv_kernel<2, false>", 0, 0, 0, 0, CK_AUTO},
    {"wino32_conv_kernel<2, true>", 0, 0, 0, 0, CK_AUTO},
    {"wino32_conv_kernel<4, false>", 0, 0, 0, 0, CK_AUTO},
    {"wino_c32_kernel<false, true>", 0, 0, 0, 0, CK_AUTO},
    {"wino_c32_kernel<true, true>", 0, 0, 0, 0, CK_AUTO},
    {"wino_conv_multi_kernel<2, false, 6>", 0, 0, 0, 0, CK_AUTO},
    {"wino_conv_multi_kernel<2, false, 4>", 0, 0, 0, 0, CK_AUTO},
    {"wino_conv_multi_kernel<4, false, 4>", 0, 0, 0, 0, CK_AUTO},
    {"wino_conv_multi_kernel<2, true, 4>", 0, 0, 0, 0, CK_AUTO},
    {"wino_c32_kernel<false, false, _Float16>", 0, 0, 0, 0, CK_AUTO},
    {"wino_c32_kernel<true, false, _Float16>", 0, 0, 0, 0, CK_AUTO},
};
constexpr int conv_kernel_bm(int k) { return 32 * kConvKernel[k].WM * kConvKernel[k].WGM; }
constexpr int conv_kernel_bn(int k) { return 32 * kConvKernel[k].WN * kConvKernel[k].WGN; }

// What the tuning hooks ask for (the globals live with the API entry points that own them).  cfg, split: mtd_conv_igemm_override
// (a tile kernel, CK_C32P or CK_C32T; slices of K); f4_min_w: mtd_conv_winograd_f4_min_w (narrowest map that takes F(2x4, 3x3),
// 0 = never, -1 = the default); wino_split: the run-time option "wino_split" (the split-bf16 Winograd kernel).
struct ConvForce { int cfg = CK_AUTO, split = -1, f4_min_w = -1, wino_split = 0; };

// ---- lab switches (host_util.h: environment variables of a -DMTD_LAB build, read once; the shipped library has the defaults
// compiled in).  X(field, variable, default)
#define CONV_LAB_SWITCHES(X)                                                                                                               \
    X(igemm_plan, "MTD_IGEMM_PLAN", 1)                 /* 2: round 2's rules for the large 3x3 grids (make_plan) */                        \
    X(igemm_xcd, "MTD_IGEMM_XCD", 1)                   /* IgemmParams::xcd_map */                                                          \
    X(igemm_nt, "MTD_IGEMM_NT", 0)                     /* IgemmParams::nt_store */                                                         \
    X(splitk_fin, "MTD_SPLITK_FIN", 1)                 /* split-K finish inside the kernel where the caller brought counters ... */        \
    X(splitk_fin_max, "MTD_SPLITK_FIN_MAX", 8)         /* ... up to this many slices (0: the separate epilogue launch) */                  \
    X(c32t_variant, "MTD_C32T_VARIANT", 0)             /* halo-tile kernel: 1 = two image rows per tile, single-buffered */                \
    X(c32t_stagger, "MTD_C32T_STAGGER", 0)             /* ... its start stagger */                                                         \
    X(c32t_wide, "MTD_C32T_WIDE", 1)                   /* halo-tile kernel: the 16-byte epilogue where the operands allow it */            \
    X(tail_lab, "MTD_TAIL_LAB", 0)                     /* Res-FFT block tail: stage switches that produce WRONG results */                 \
    X(wino_f4, "MTD_WINO_F4", 1)                       /* 0: F(2x4, 3x3) off ... */                                                        \
    X(wino_f4_min_w, "MTD_WINO_F4_MIN_W", 8)           /* ... else on maps at least this wide (ConvForce::f4_min_w -1) */                  \
    X(wino_f4_nb1, "MTD_WINO_F4_NB1", 0)               /* F(2x4): 32-channel workgroups in place of a split of K (wino_plan) */            \
    X(wino_nb2_maxc, "MTD_WINO_NB2_MAXC", 0)           /* 64-channel workgroups for layers of at most this many input channels */          \
    X(wino_splitk_minsteps, "MTD_WINO_SPLITK_MINSTEPS", 2) /* K steps per slice at least */                                                \
    X(wino_splitk, "MTD_WINO_SPLITK", 0)               /* > 0: this many slices */                                                         \
    X(wino_lean, "MTD_WINO_LEAN", 1)                   /* lean form: 0 never, 1 by wino_plan's rule, 2 whenever NB = 2 */                  \
    X(wino_c32_kernel, "MTD_WINO_C32_KERNEL", 1)       /* 0: the general kernel's 32-channel workgroups (wino_c32_takes) */                \
    X(wino_xcd, "MTD_WINO_XCD", -1)                    /* >= 0: WinoParams::xcd_order */                                                   \
    X(wino_pair_split, "MTD_WINO_PAIR_SPLIT", 0)       /* > 0: plan every group as if it held this many problems */                        \
    X(wino_s2_splitk, "MTD_WINO_S2_SPLITK", 0)         /* stride-2 form, > 0: this many slices */                                          \
    X(wino_s2_lean, "MTD_WINO_S2_LEAN", 1)             /* ... its lean form, as MTD_WINO_LEAN */                                           \
    X(wino_s2_nb, "MTD_WINO_S2_NB", 0)                 /* ... 4 / 2: 128- / 64-channel workgroups whatever pays */
struct ConvLab {
#define X(field, name, dflt) int field = dflt;
    CONV_LAB_SWITCHES(X)
#undef X
};
inline const ConvLab& conv_lab() {
    static const ConvLab lab = [] {
        ConvLab l;
#define X(field, name, dflt) if (const char* e = mtd_lab_env(name)) l.field = atoi(e);
        CONV_LAB_SWITCHES(X)
#undef X
        return l;
    }();
    return lab;
}
#ifdef MTD_LAB
constexpr bool kSplitkFinBuilt = true;
#else
constexpr bool kSplitkFinBuilt = false;      // the in-kernel split-K finish exists in lab builds only
#endif

// ---- tile and chunk sizes of the kernels
constexpr int KC = 32;              // conv_igemm.hip: channels per K chunk
constexpr int TB_MAXT = 9;          // taps of the tap-block kernel
constexpr int MULTI_MAX = 4;        // problems per igemm_multi_kernel launch
constexpr int C32T_W = 64, C32T_R = 4;      // halo-tile kernel: pixels per image row, image rows per tile
constexpr int WT = 32;              // conv_winograd.hip, conv_wino_s2.h: tiles per workgroup
constexpr int WKC = 16;             // ... channels per K step
constexpr int WINO_MULTI_MAX = 3;   // problems per wino_conv_multi_kernel launch

// ---- arguments
inline int check_args(const mtd_conv_args& a) {
    if (!a.in || !a.w || !a.out) return MTD_EINVAL;
    if (a.C <= 0 || a.N <= 0 || (a.C % 32) || (a.N % 32)) return MTD_EINVAL;
    const mtd_geom& g = a.g;
    if (g.B <= 0 || g.IH <= 0 || g.IW <= 0 || g.OH <= 0 || g.OW <= 0) return MTD_EINVAL;
    if (g.TH <= 0 || g.TW <= 0 || g.TH * g.TW > 16) return MTD_EINVAL;
    if (geom_pixels(g) > (1ll << 30)) return MTD_EINVAL;
    if (a.in_ld < a.C || a.out_ld < a.N || (a.in_ld % 4)) return MTD_EINVAL;
    if (!aligned16(a.in)) return MTD_EALIGN;
    if (a.w_sc != 1 || a.w_st < 0) return MTD_EINVAL;                     // packed / natively c-contiguous weight view
    if (!aligned16(a.w) || (a.w_sn % 4) || (a.g.TH * a.g.TW > 1 && (a.w_st % 4))) return MTD_EALIGN;
    if (a.add1 && a.add1_ld < a.N) return MTD_EINVAL;
    if (a.add2 && a.add2_ld < a.N) return MTD_EINVAL;
    if (a.mask && a.mask_ld < a.N) return MTD_EINVAL;
    if (a.out2 && a.out2_ld < a.N) return MTD_EINVAL;
    // the furthest output pixel must stay inside the OHF x OWF image
    if ((g.OH - 1) * g.out_sy + g.out_oy >= g.OHF || (g.OW - 1) * g.out_sx + g.out_ox >= g.OWF) return MTD_EINVAL;
    return MTD_OK;
}

// ---- the kernels' domains and the derived flags of the launch parameters
inline int conv_taps(const mtd_conv_args& a) { return a.g.TH * a.g.TW; }
// the generator-shaped layers: 32 input channels, nine taps, at least 32768 pixels
inline bool gen_shape(const mtd_conv_args& a) { return a.C == 32 && conv_taps(a) == 9 && geom_pixels(a.g) >= 32768; }
// output pixel index == launch-grid pixel index
inline bool out_identity(const mtd_geom& g) { return g.out_sy == 1 && g.out_sx == 1 && g.out_oy == 0 && g.out_ox == 0 && g.OHF == g.OH && g.OWF == g.OW; }
// 32 consecutive launch-grid pixels (from a multiple of 32) map to output pixels pix0 + r * out_sx
inline bool out_linear(const mtd_geom& g) { return out_identity(g) || (g.OW % 32 == 0); }
// every tap of a 3x3 geometry within one pixel of the output position
inline bool taps_within_one(const mtd_geom& g) {
    for (int i = 0; i < 3; ++i) {
        const int dy = g.off_y + i * g.tap_dy, dx = g.off_x + i * g.tap_dx;
        if (dy < -1 || dy > 1 || dx < -1 || dx > 1) return false;
    }
    return true;
}

// 16-byte epilogue vectors (EpiWide): every operand row 16-byte aligned
inline bool wide_epilogue_ok(const mtd_conv_args& a) {
    if (!aligned16(a.out) || (a.out_ld % 4)) return false;
    if (a.bias && !aligned16(a.bias)) return false;
    if (a.add1 && (!aligned16(a.add1) || (a.add1_ld % 4))) return false;
    if (a.add2 && (!aligned16(a.add2) || (a.add2_ld % 4))) return false;
    if (a.mask && (!aligned16(a.mask) || (a.mask_ld % 4))) return false;
    if (a.out2 && (!aligned16(a.out2) || (a.out2_ld % 4))) return false;
    return true;
}

// the 16-byte form of the split-K finish (splitk_epilogue_kernel): every row stride a multiple of 4 floats, 16-byte aligned bases,
// M N < 2^31
inline bool splitk_vec_ok(const mtd_conv_args& a, long long M) {
    if (M * a.N >= (1ll << 31) || !aligned16(a.ws) || !aligned16(a.out) || (a.out_ld % 4)) return false;
    if (a.bias && !aligned16(a.bias)) return false;
    if (a.add1 && (!aligned16(a.add1) || (a.add1_ld % 4))) return false;
    if (a.add2 && (!aligned16(a.add2) || (a.add2_ld % 4))) return false;
    if (a.mask && (!aligned16(a.mask) || (a.mask_ld % 4))) return false;
    return true;
}

// IgemmParams::wide of a launch of `count` sets that share set 0's epilogue operands: bit 0 = every epilogue operand row is
// 16-byte aligned, bit 1 = so are the split-K slabs of every set
inline int conv_wide(const mtd_conv_args* a, int count, int splitk) {
    bool slabs16 = splitk > 1 && (a[0].N % 4) == 0;
    for (int i = 0; i < count; ++i) slabs16 = slabs16 && aligned16(a[i].ws);
    return (wide_epilogue_ok(a[0]) ? 1 : 0) | (slabs16 ? 2 : 0);
}

// the halo-tile kernel's geometry: 3x3, stride 1, every tap within one pixel of the output position, 64-pixel rows
inline bool c32t_eligible(const mtd_conv_args& a) {
    const mtd_geom& g = a.g;
    if (a.C != 32 || g.TH != 3 || g.TW != 3 || g.in_sy != 1 || g.in_sx != 1) return false;
    if (g.OW != C32T_W || g.IW != C32T_W || g.IH != g.OH || (g.OH % C32T_R)) return false;
    return out_identity(g) && taps_within_one(g);
}

// ---- the split of K: `chunks` K steps of `kc` channels over `want` slices -- every slice at least min_steps of them, at most cap
// slices, at least one -- in slices of equal length; the count is what slices of that length leave
struct SplitK { int splitk, c_per_split; };
inline SplitK split_k(int chunks, int kc, long long want, int cap, int min_steps = 1) {
    long long sk = want;
    if (sk > chunks / min_steps) sk = chunks / min_steps;
    if (sk > cap) sk = cap;
    if (sk < 1) sk = 1;
    const int cps = (chunks + (int)sk - 1) / (int)sk;
    return {(chunks + cps - 1) / cps, cps * kc};
}
inline size_t splitk_ws_bytes(const mtd_conv_args& a, int splitk) {
    return splitk > 1 ? (size_t)splitk * (size_t)geom_pixels(a.g) * a.N * sizeof(float) : 0;
}

// ---- the implicit-GEMM tile kernels (conv_igemm.hip)
#ifndef S2DG_PLAN
#define S2DG_PLAN 1      // round-5 tile rules for the four-class stride-2 data gradients (make_plan)
#endif
struct Plan { int cfg, BM, BN, splitk, c_per_split; };

// an override that names a tile kernel this layer can run on
inline bool force_takes(const mtd_conv_args& a, const ConvForce& f) {
    if (f.cfg < 0 || f.cfg >= CK_FORCE_TILES || a.N % conv_kernel_bn(f.cfg)) return false;
    return (f.cfg != CK_TB_128x32 && f.cfg != CK_TB_256x32) || conv_taps(a) <= TB_MAXT;
}

// The tile kernel and the split of K of one launch of `sets` problems of a's shape (arguments that passed check_args).
inline Plan make_plan(const mtd_conv_args& a, const ConvForce& f, int sets = 1) {
    const ConvLab& lab = conv_lab();
    const long long M = geom_pixels(a.g) * sets;        // tile choice by the pixels of the whole grid (all sets)
    const int T = conv_taps(a);
    const int chunks = a.C / KC;
    const auto plan_of = [&](int cfg, const SplitK& s) { return Plan{cfg, conv_kernel_bm(cfg), conv_kernel_bn(cfg), s.splitk, s.c_per_split}; };
    if (force_takes(a, f)) return plan_of(f.cfg, split_k(chunks, KC, f.split > 0 ? f.split : 1, chunks));
    // Derived from the standalone sweep of all 109 conv shapes of the training step (tools/tune_igemm.py, profiles/):
    // fp32 MFMA is slow enough (64 clk per 32x32x2) that one 32x32 accumulator tile per wave at high occupancy beats the
    // register-blocked tiles almost everywhere; the wide tiles only pay for the huge-M, thin-K first-stage layers.
    int cfg = CK_IGEMM_128x32;
    if ((M >= 131072 && a.N >= 64) || (M >= 32768 && a.N >= 256 && a.C <= 64) || (M >= 65536 && a.N >= 128) ||
        (M >= 16384 && a.N >= 512 && a.C <= 128)) cfg = CK_IGEMM_256x32;
    else if (M >= 32768 && a.N == 64 && a.C >= 128) cfg = CK_IGEMM_64x64;
    // tap-block kernel (all taps of a channel chunk per barrier; 41 KB of LDS = 3 workgroups per CU): 5-9 % faster on the
    // paired-pass shapes (profiles/r1_igemm_tile_sweep.txt) when several chunks stream and the grid fits one round of residency
    if (cfg == CK_IGEMM_128x32 && a.C >= 128 && M >= 4096 && T == TB_MAXT) {        // (1x1 layers: 30-40 % slower there)
        const long long b6 = ((M + 127) / 128) * (a.N / 32);
        const long long sk6 = b6 <= 256 ? 512 / b6 : 1;
        if (b6 * sk6 <= 768) cfg = CK_TB_128x32;
    }
    // Round 2, after the transposed accumulator blocks (the 256 x 64 tile lost its scratch spill and both tap-block forms their
    // dword epilogues): the standalone sweep of the step's 98 shapes (profiles/r2_igemm_tile_sweep.txt) puts the 256 x 64 tile
    // 5-9 % ahead on every large 3x3 grid, 1.25 ms per step over all shapes.  INSIDE the step the rules below (MTD_IGEMM_PLAN=2)
    // move 7.0 ms of launches onto that tile and 1.6 ms onto the two-block tap-block kernel and the family's total does not
    // change (20.63 -> 20.58 ms in the one-stream trace, step 40.26 vs 40.40 ms): standalone timings on repeated launches
    // do not predict the in-step ranking at this margin.  Off by default.
    const bool round2 = lab.igemm_plan >= 2 && sets == 1 && T == TB_MAXT;
    if (round2) {
        const long long MN = M * a.N;
        if ((a.N % 64) == 0 && a.C >= 64 && MN >= (4ll << 20) && !(M >= 65536 && a.N >= 256 && a.C <= 64)) {
            cfg = CK_IGEMM_256x64;     // 256 x 64, four blocks per wave: 5-9 % over the 128 / 256 x 32 tiles on every grid this large
        } else if (a.C >= 128 && MN >= (2ll << 20) && MN < (4ll << 20) && (M / 256) * (a.N / 32) >= 256 && a.N <= 256) {
            cfg = CK_TB_256x32;        // tap-block kernel with two blocks per wave: 16384 x 128, 32768 x 64, 8192 x 256
        }
    }
    // Round 5: the four-class stride-2 data gradients (sets == 4, 2 x 2 taps) had kept round 2's tiles; re-timed on the step's shapes
    // (tools/s2_dgrad_probe.py, us per launch, plan -> new): 65536 x 4 pixels, 64 channels 119 -> 108 (256 x 64 tile); 16384 x 4, 128:
    // 90 -> 87; 4096 x 4, 256: 95 -> 79 (256 x 32); the G step's unpaired passes 32768 x 4, 64: 61 -> 57; 8192 x 4, 128: 58 -> 48;
    // 2048 x 4, 256: 60 -> 44 (128 x 32 WITHOUT the split of K).  The 512-channel levels keep the plan.
    bool unsplit = false;
    if (S2DG_PLAN && sets == 4 && T == 4) {
        if ((a.N == 64 && M >= 131072) || (a.N == 128 && M >= 32768)) { cfg = CK_IGEMM_256x64; unsplit = true; }
        else if (a.N == 256 && M >= 16384) { cfg = CK_IGEMM_256x32; unsplit = true; }
        else if (a.N == 256 && M >= 8192) { cfg = CK_IGEMM_128x32; unsplit = true; }
    }
    // ... and the first 4 x 4 stride-2 forward conv (down1: 64 -> 64 channels; tools/s2_fwd_probe.py): 65536 pixels 99 -> 82 us on the
    // 256 x 64 tile, the G step's 32768 pixels 64 -> 45 on the 64 x 64 tile, both unsplit; the deeper levels keep the plan (it is the best there)
    if (S2DG_PLAN && sets == 1 && T == 16 && a.N == 64 && a.C == 64) {
        if (M >= 65536) { cfg = CK_IGEMM_256x64; unsplit = true; }
        else if (M >= 32768) { cfg = CK_IGEMM_64x64; unsplit = true; }
    }
    const int BM = conv_kernel_bm(cfg), BN = conv_kernel_bn(cfg);
    const long long blocks = ((geom_pixels(a.g) + BM - 1) / BM) * (a.N / BN) * sets;
    long long sk = blocks <= 256 ? 512 / blocks : 1;      // fill ~2 workgroups per CU; never split a grid that already does
    if (blocks > 256 && blocks <= 512 && chunks * T <= 32) sk = 2;      // ... unless its workgroups are short (2x2-tap data gradients: -22 %)
    if (round2 && blocks == 256) {
        // a grid of exactly one workgroup per CU: the register-blocked tiles do not want the split at all, the tap-block
        // kernel only when its K loop is long (4096 x 256 x 256: 45 us unsplit, 51 split; 2048 x 512 x 512: 91 / 87)
        if (cfg == CK_IGEMM_256x64 || cfg == CK_TB_256x32) sk = 1;
        else if (cfg == CK_TB_128x32 && (long long)a.C * 9 < 4096) sk = 1;
    }
    if (unsplit) sk = 1;
    return plan_of(cfg, split_k(chunks, KC, sk, 32));
}

// The route of mtd_conv_igemm (sets == 1) and mtd_conv_igemm_multi: `kernel` is the ConvKernel that runs, or MTD_E* where the
// arguments are refused; `multi`: one launch of the multi form for all sets (else one launch per set, each by its own route);
// `plan` is the tile plan of those launches (the halo-tile and the persistent kernel have none of their own: it sizes the
// workspace query all the same, as it always has).
struct ConvRoute { int kernel; bool multi; Plan plan; };
inline ConvRoute conv_igemm_route(const mtd_conv_args& a, int sets, const ConvForce& f) {
    const bool gen = gen_shape(a);
    if (sets > 1) {
        // a multi call runs as single launches where the plan picks a kernel without a multi form, under an override beyond the
        // multi forms, and on the generator-shaped layers
        const Plan pl = make_plan(a, f, sets);
        const ConvKernel multi = kConvKernel[pl.cfg].multi;
        if (multi != CK_AUTO && f.cfg <= CK_IGEMM_32x128 && !gen) return {multi, true, pl};
    }
    const Plan pl = make_plan(a, f);
    const bool c32t = (f.cfg == CK_AUTO || f.cfg == CK_C32T) && gen, c32p = (f.cfg == CK_AUTO || f.cfg == CK_C32P) && gen;
    // generator-shaped layers on 64-pixel rows: halo tiles of four image rows, one persistent workgroup per CU
    if (c32t && c32t_eligible(a) && a.act != MTD_ACT_RELU_ADD) return {CK_C32T, false, pl};
    if (a.out2) return {MTD_EINVAL, false, pl};               // second output: halo-tile kernel only
    // the residual after the activation: the persistent kernel only (its two epilogue forms implement it; no split-K, no mask)
    if (a.act == MTD_ACT_RELU_ADD && !(c32p && !a.mask)) return {MTD_EINVAL, false, pl};
    // generator-shaped layers: persistent kernel, two 32-pixel tiles per wave at M = 131072
    if (c32p) return {CK_C32P, false, pl};
    return {pl.cfg, false, pl};
}

// mtd_conv_relu_add_ok: does the route take these arguments (that passed check_args) with act = MTD_ACT_RELU_ADD?
inline bool conv_relu_add_ok(const mtd_conv_args& a, const ConvForce& f) {
    mtd_conv_args r = a;
    r.act = MTD_ACT_RELU_ADD;
    return conv_igemm_route(r, 1, f).kernel >= 0;
}
// mtd_resfft_block_tail_ok: the halo-tile kernel's launches that can close a Res-FFT-Conv block (CK_C32T_TAIL): C = N = 32 on
// 64 x 64 patches (the spectrum's), no add / mask operands, the 16-byte epilogue
inline bool c32t_tail_ok(const mtd_conv_args& a) {
    if (a.N != 32 || !gen_shape(a) || !c32t_eligible(a)) return false;
    if (a.add1 || a.add2 || a.mask || a.scale2 || !wide_epilogue_ok(a)) return false;
    return a.g.OH == 64;
}

// IgemmParams::fin: the last workgroup to arrive at a tile sums the slabs and runs the epilogue (1: in 16-byte vectors, 2: value
// by value) when the caller brought arrival counters for every output tile; 0: the separate epilogue launch
inline int conv_fin(const mtd_conv_args& a, const Plan& pl) {
    const ConvLab& lab = conv_lab();
    const long long M = geom_pixels(a.g);
    const long long tiles = ((M + pl.BM - 1) / pl.BM) * (a.N / pl.BN);
    if (!(pl.splitk > 1 && kSplitkFinBuilt && lab.splitk_fin && pl.cfg != CK_TB_256x32 && a.tile_ctr && tiles <= (long long)a.tile_ctr_len &&
          pl.splitk <= lab.splitk_fin_max)) return 0;
    return splitk_vec_ok(a, M) ? 1 : 2;
}

// ---- Winograd F(2x2, 3x3) / F(2x4, 3x3) (conv_winograd.hip)
// Which transform along x does this layer take?  4 = the patch width of F(2x2, 3x3), 6 = F(2x4, 3x3): maps whose width is a
// multiple of 4 and at least MTD_WINO_F4_MIN_W (default 8: on the 4-pixel-wide maps a tile row is one tile and the transformed
// weights -- 24 / 9 of the filter instead of 16 / 9 -- are what the launch streams).  MTD_WINO_F4=0 switches the form off.
inline int conv_f4_min_w(const ConvForce& f) { return f.f4_min_w >= 0 ? f.f4_min_w : (conv_lab().wino_f4 ? conv_lab().wino_f4_min_w : 0); }
inline int wino_patch_w(const mtd_conv_args& a, const ConvForce& f) {
    const int min_w = conv_f4_min_w(f);
    const int pxw = (min_w > 0 && (a.g.OW % 4) == 0 && a.g.OW >= min_w) ? 6 : 4;
    // the split-bf16 kernel (conv_winograd_split.h) takes every layer whose N is a multiple of 64 (bit 4 of the code); the
    // generator's 32 -> 32 layers keep the fp32 forms (the persistent kernel of conv_wino_c32.h)
    return pxw | ((f.wino_split && (a.N % 64) == 0) ? 16 : 0);
}
// the patch width the transformed weights in a->w were built for travels in a->w_st (6: F(2x4, 3x3); anything else: 4)
// (bit 4: the split-bf16 form)
inline int wino_args_px(const mtd_conv_args& a) { return ((a.w_st & 15) == 6 ? 6 : 4) | ((a.w_st & 16) && a.w_st < 32 ? 16 : 0); }

// the kernel's domain: 3x3, stride 1, "same" size, even height and width, every tap within one pixel of the output position,
// output pixel == launch pixel, C a multiple of 16, N a multiple of 64 (or C = N = 32 in the F(2x4) form), the input view inside 32-bit byte offsets
inline bool wino_eligible(const mtd_conv_args& a, const ConvForce& f) {
    const mtd_geom& g = a.g;
    if (g.TH != 3 || g.TW != 3 || g.in_sy != 1 || g.in_sx != 1) return false;
    if (g.IH != g.OH || g.IW != g.OW || (g.OH & 1) || (g.OW & 1)) return false;
    if (!out_identity(g) || !taps_within_one(g)) return false;
    if (g.tap_dy == 0 || g.tap_dx == 0) return false;
    if (a.C % 16) return false;
    if (a.out2 && !(a.N == 32 && a.C == 32 && a.mask)) return false;      // (a second output: the persistent 32 -> 32 kernel's MASKED2 form only; mtd_conv_winograd_ok checks that it takes the launch)
    // N a multiple of 64; or the generator's 32 -> 32 channel layers in the F(2x4) form: the persistent kernel of conv_wino_c32.h
    // (wino_c32_takes), else this kernel's 32-channel workgroups (NB = 1).  (Whether conv() sends them here is the host's
    // threshold, kernels.WINO_C32_MIN_HW: whole-slice inference yes, the 64 x 64 training patches no -- DESIGN 3.8.)
    if ((a.N % 64) && !(a.N == 32 && a.C == 32 && wino_patch_w(a, f) == 6)) return false;
    if (a.act == MTD_ACT_RELU_ADD && !((a.N % 64) != 0 && !a.mask)) return false;      // residual after the activation: that form only
    return true;
}

// The persistent 32 -> 32 channel kernel (conv_wino_c32.h) takes a layer of the F(2x4) form with one residual operand at most,
// no scales, no mask, 16-byte aligned rows everywhere and buffers inside 31-bit byte offsets.  MTD_WINO_C32_KERNEL=0: the
// general kernel's 32-channel workgroups instead (lab switch).
inline bool wino_c32_takes(const mtd_conv_args& a, int pxcode) {
    const int px = pxcode;       // (a split code, 20 / 22, never matches 6: N % 64 == 0 there)
    if (!conv_lab().wino_c32_kernel || px != 6 || a.C != 32 || a.N != 32) return false;
    if (a.scale || a.scale2 || a.add2 || (a.out2 && !a.mask)) return false;
    if (a.mask && (a.act == MTD_ACT_RELU_ADD || !aligned16(a.mask) || (a.mask_ld % 4))) return false;
    if (a.out2 && (!aligned16(a.out2) || (a.out2_ld % 4))) return false;
    if (!wide_epilogue_ok(a) || !aligned16(a.in) || (a.in_ld % 4)) return false;
    const long long M = geom_pixels(a.g);
    if (M / 8 >= (1ll << 23)) return false;
    if (((M - 1) * a.out_ld + a.N) * 4 >= (1ll << 31)) return false;
    if (a.add1 && ((M - 1) * a.add1_ld + a.N) * 4 >= (1ll << 31)) return false;
    if (a.mask && ((M - 1) * a.mask_ld + a.N) * 4 >= (1ll << 31)) return false;
    if (a.out2 && ((M - 1) * a.out2_ld + a.N) * 4 >= (1ll << 31)) return false;
    return true;
}

// mtd_conv_winograd_ok: the arguments one launch of mtd_conv_winograd takes
inline bool wino_args_ok(const mtd_conv_args* a, const ConvForce& f) {
    if (!a || !a->in || !a->w || !a->out) return false;
    if (a->C <= 0 || a->N <= 0 || a->in_ld < a->C || a->out_ld < a->N) return false;
    if (!wino_eligible(*a, f)) return false;
    const long long npix = (long long)a->g.B * a->g.IH * a->g.IW;
    if (((npix - 1) * a->in_ld + a->C) * 4 >= (1ll << 31)) return false;
    if (geom_pixels(a->g) * a->N >= (1ll << 31)) return false;
    if ((long long)144 * a->N * a->C >= (1ll << 31)) return false;          // (the transformed weights inside 31-bit byte offsets, split form included)
    // a mask on a 32 -> 32 layer / a second output: only the persistent kernel carries them in this form (the general kernel's
    // 32-channel workgroups take a mask, never a second output -- and the caller's MASKED2 launches must not end up there)
    if (a->out2 && !wino_c32_takes(*a, wino_patch_w(*a, f))) return false;
    return true;
}

// kernel: the ConvKernel of a single launch (kConvKernel[kernel].multi: of a group)
struct WinoPlan { int nb, lean, splitk, c_per_split, px; ConvKernel kernel; };

inline WinoPlan wino_plan(const mtd_conv_args& a, int pxcode, int sets = 1) {
    const ConvLab& lab = conv_lab();
    WinoPlan pl{};
    const int px = pxcode & 15;
    const bool split3 = (pxcode & 16) != 0;
    pl.px = px;
    const int tile_px = 2 * (px - 2);                            // output pixels per tile
    pl.nb = (a.N % 128 == 0 && px == 4) ? 4 : 2;
    // F(2x4): a tile block is 256 pixels x 64 channels; where that leaves the grid short (the mid-size maps: 4096 .. 16384 pixels)
    // 32-channel workgroups (NB = 1) can stand in for a split of K -- no slabs, no finishing launch, but every 32 output channels
    // repeat the input transform, and a transform instruction is paid in full beside the fp32 MFMAs.  The form won
    // 0.2 ms per step while the transform cost 170 vector instructions per K step; at 116 the split of K is ahead by 0.15 ms
    // (29.15 against 29.31 ms), so it is off by default now (MTD_WINO_F4_NB1=1: on).
    if (px == 6 && lab.wino_f4_nb1) {
        const long long t = geom_pixels(a.g) / tile_px;
        if (((t + WT - 1) / WT) * (a.N / 64) <= 128 && a.C >= 128) pl.nb = 1;
    }
    if (a.N % 64) pl.nb = 1;                                     // (F(2x4) only: wino_eligible)
    if (split3) pl.nb = 2;                                       // the split-bf16 kernel: 64-channel workgroups only
    // (lab, MTD_WINO_NB2_MAXC=64: the narrow form with its lean variant for layers with four K steps whatever their N -- 5 % less time
    // for those launches (123 -> 116 us, 226 -> 213 us), 0.08 ms per step, but the input is then read per 64 instead of per 128 output
    // channels: 62 -> 80 MB of fabric traffic per launch.  Off.)
    if (a.C <= lab.wino_nb2_maxc) pl.nb = 2;
    const long long tiles = geom_pixels(a.g) / tile_px;
    long long blocks = ((tiles + WT - 1) / WT) * (a.N / (32 * pl.nb));
    if (blocks < 192 && pl.nb == 4 && a.N % 64 == 0 && !split3) {          // more, narrower workgroups before splitting K
        pl.nb = 2;
        blocks = ((tiles + WT - 1) / WT) * (a.N / 64);
    }
    const int chunks = a.C / WKC;                                // K steps of 16 channels
    // K steps per slice at least: 2 since the end of round 5 (rounds 3-5: 4).  In the concurrent step the layers this frees -- C = 64 ... 128 on
    // grids of 64 ... 128 workgroups -- gain more from the second half of the chip than the extra slab costs: 27.45 -> 27.33 ms in four A/B
    // pairs (1: 27.37 / 27.44, 3: 27.42 / 27.40; a cap on the split or a target of 384 / 512 workgroups loses 0.4 ... 1.8 ms)
    // (sets > 1: the group form.s grid holds that many problems and the split of K is planned for the whole grid: wino_group_sets)
    const long long grid_blocks = blocks * sets;
    const SplitK s = lab.wino_splitk > 0 ? split_k(chunks, WKC, lab.wino_splitk, chunks)
                                         : split_k(chunks, WKC, grid_blocks <= 128 ? 256 / grid_blocks : 1, 16, lab.wino_splitk_minsteps);
    pl.splitk = s.splitk;
    pl.c_per_split = s.c_per_split;
    // two lean workgroups per CU where a workgroup has few K steps and the grid has at least two per CU (MTD_WINO_LEAN: 0 never,
    // 1 by this rule, 2 whenever NB = 2)
    const long long grid = ((tiles + WT - 1) / WT) * (a.N / (32 * pl.nb)) * pl.splitk;
    pl.lean = px == 4 && pl.nb == 2 && lab.wino_lean && (lab.wino_lean == 2 || (s.c_per_split / WKC <= 8 && grid >= 512)) && !split3;
    // (one profiler id per INSTANTIATION, so that a record's name is one kernel symbol of a rocprofv3 table)
    pl.kernel = split3 ? (px == 6 ? CK_WINO3_PX6 : CK_WINO3_PX4)
              : px == 6 ? (pl.nb == 1 ? CK_WINO6_NB1 : CK_WINO6_NB2)
              : pl.nb == 4 ? CK_WINO_NB4 : pl.lean ? CK_WINO_NB2_LEAN : CK_WINO_NB2;
    return pl;
}
// the persistent 32 -> 32 channel kernel's forms (`half`: binary16 activation storage, no mask form)
inline ConvKernel wino_c32_kernel_of(const mtd_conv_args& a, bool half) {
    if (half) return a.add1 ? CK_WINO_C32_F16_ADD : CK_WINO_C32_F16;
    if (a.mask) return a.add1 ? CK_WINO_C32_MASK_ADD : CK_WINO_C32_MASK;
    return a.add1 ? CK_WINO_C32_ADD : CK_WINO_C32;
}

// The split of K of a group of `count` problems is planned for the WHOLE grid (mtd_conv_winograd_group; lab: MTD_WINO_PAIR_SPLIT =
// n plans every group as if it held n problems, 1: per problem)
inline int wino_group_sets(int count) { return conv_lab().wino_pair_split > 0 ? conv_lab().wino_pair_split : count; }

// mtd_conv_winograd_group_ok: the general fp32 kernels only (not the persistent 32-channel kernel, not the split-bf16 form)
inline bool wino_group_ok(const mtd_conv_args* a, int count, const ConvForce& f) {
    if (!a || count < 2 || count > WINO_MULTI_MAX) return false;
    const int px = wino_args_px(a[0]);
    const long long M = geom_pixels(a[0].g);
    for (int i = 0; i < count; ++i) {
        if (!wino_args_ok(&a[i], f)) return false;
        if (__builtin_memcmp(&a[0].g, &a[i].g, sizeof(mtd_geom)) != 0 || a[0].N != a[i].N || a[0].C != a[i].C) return false;
        if (wino_args_px(a[i]) != px || wino_c32_takes(a[i], px) || !aligned16(a[i].w)) return false;
    }
    if ((px & 16) || (a[0].N % 64)) return false;
    if ((px & 15) == 6 && (a[0].g.OW % 4)) return false;
    const WinoPlan pl = wino_plan(a[0], px, wino_group_sets(count));
    if ((px & 15) == 6 && pl.nb != 2) return false;
    // the problems' slab sums go through ONE launch of the 16-byte epilogue: all need it (else: single launches)
    if (pl.splitk > 1)
        for (int i = 0; i < count; ++i)
            if (!splitk_vec_ok(a[i], M)) return false;
    return true;
}

// WinoParams::xcd_order / W32Params::xcd_order: which operand the workgroups of an XCD share, the heavier one (1: the weights)
inline int xcd_order_of(double wbytes, double ibytes) { return wbytes >= ibytes ? 1 : 2; }
inline int wino_xcd_order(const mtd_conv_args& a, int px) {
    if (conv_lab().wino_xcd >= 0) return conv_lab().wino_xcd;
    return xcd_order_of(4.0 * px * a.C * a.N * 4, (double)geom_pixels(a.g) * a.C * 4);
}

// ---- Winograd F(3x3, 2x2) of the 4x4 / stride-2 layers (conv_wino_s2.h)
struct W32Form { int groups, ps, base_y, base_x; int kmap[16]; };

// Which form is this geometry?  forward: 4x4 taps at stride 2 (tap = 2 j + phase); class: 2x2 taps at stride 1
inline bool wino32_form(const mtd_geom& g, W32Form& f) {
    if (g.TH != g.TW || g.in_sy != g.in_sx || g.tap_dy != g.tap_dx) return false;
    if (g.TH == 4 && g.in_sy == 2 && g.tap_dy == 1) {
        f.groups = 4; f.ps = 2; f.base_y = g.off_y; f.base_x = g.off_x;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px)
                for (int jy = 0; jy < 2; ++jy)
                    for (int jx = 0; jx < 2; ++jx)
                        f.kmap[(py * 2 + px) * 4 + jy * 2 + jx] = (g.ky0 + (2 * jy + py) * g.ky_step) * g.KW + (g.kx0 + (2 * jx + px) * g.kx_step);
        return true;
    }
    if (g.TH == 2 && g.in_sy == 1 && (g.tap_dy == 1 || g.tap_dy == -1)) {
        const bool rev = g.tap_dy < 0;
        f.groups = 1; f.ps = 1; f.base_y = g.off_y - (rev ? 1 : 0); f.base_x = g.off_x - (rev ? 1 : 0);
        for (int i = 0; i < 16; ++i) f.kmap[i] = 0;
        for (int jy = 0; jy < 2; ++jy)
            for (int jx = 0; jx < 2; ++jx) {
                const int ty = rev ? 1 - jy : jy, tx = rev ? 1 - jx : jx;
                f.kmap[jy * 2 + jx] = (g.ky0 + ty * g.ky_step) * g.KW + (g.kx0 + tx * g.kx_step);
            }
        return true;
    }
    return false;
}

inline bool wino32_eligible(const mtd_conv_args* a, int count) {
    if (!a || count < 1 || count > 4) return false;
    W32Form f0;
    if (!wino32_form(a[0].g, f0)) return false;
    for (int i = 0; i < count; ++i) {
        const mtd_conv_args& s = a[i];
        if (!s.in || !s.w || !s.out || s.C <= 0 || s.N <= 0 || s.in_ld < s.C || s.out_ld < s.N) return false;
        if ((s.C % 16) || (s.N % 64) || s.out2 || s.act == MTD_ACT_RELU_ADD || (s.in_ld % 4) || !aligned16(s.in) || !aligned16(s.w)) return false;
        W32Form f;
        if (!wino32_form(s.g, f) || f.groups != f0.groups) return false;
        const mtd_geom &g = s.g, &h = a[0].g;
        if (g.out_sy < 1 || g.out_sx < 1) return false;
        if ((g.OH - 1) * g.out_sy + g.out_oy >= g.OHF || (g.OW - 1) * g.out_sx + g.out_ox >= g.OWF) return false;
        if (i) {      // one shape, one set of operands: the classes differ in offsets, filter entries and where their pixels land
            if (g.B != h.B || g.IH != h.IH || g.IW != h.IW || g.OH != h.OH || g.OW != h.OW || g.OHF != h.OHF || g.OWF != h.OWF ||
                g.out_sy != h.out_sy || g.out_sx != h.out_sx) return false;
            if (s.in != a[0].in || s.in_ld != a[0].in_ld || s.C != a[0].C || s.N != a[0].N || s.out != a[0].out || s.out_ld != a[0].out_ld ||
                s.scale != a[0].scale || s.scale2 != a[0].scale2 || s.scale_split != a[0].scale_split || s.bias != a[0].bias ||
                s.add1 != a[0].add1 || s.add1_ld != a[0].add1_ld || s.add2 != a[0].add2 || s.add2_ld != a[0].add2_ld || s.act != a[0].act ||
                s.mask != a[0].mask || s.mask_ld != a[0].mask_ld || s.mask_slope != a[0].mask_slope) return false;
        }
        const long long npix = (long long)g.B * g.IH * g.IW;
        if (((npix - 1) * s.in_ld + s.C) * 4 >= (1ll << 31)) return false;
        if (geom_pixels(g) * s.N >= (1ll << 31)) return false;
        if ((long long)64 * f.groups * s.N * s.C >= (1ll << 31)) return false;
        if ((long long)g.B * g.OHF * g.OWF * s.out_ld >= (1ll << 31)) return false;
    }
    return true;
}

struct W32Plan { int splitk, c_per_split, tiles_x, tiles_y, ntiles, lean, pays, nb; ConvKernel kernel; };

inline W32Plan wino32_plan_nb(const mtd_conv_args& a, int count, int groups, int nb) {
    const ConvLab& lab = conv_lab();
    W32Plan pl{};
    pl.tiles_x = (a.g.OW + 2) / 3;
    pl.tiles_y = (a.g.OH + 2) / 3;
    pl.ntiles = a.g.B * pl.tiles_x * pl.tiles_y;
    pl.nb = nb;
    const long long blocks = (long long)((pl.ntiles + WT - 1) / WT) * (a.N / (32 * pl.nb)) * count;
    const int chunks = groups * a.C / WKC;
    const SplitK s = lab.wino_s2_splitk > 0 ? split_k(chunks, WKC, lab.wino_s2_splitk, chunks)
                                            : split_k(chunks, WKC, blocks <= 128 ? 256 / blocks : 1, 16, 4);
    pl.splitk = s.splitk;
    pl.c_per_split = s.c_per_split;
    const long long grid = blocks * pl.splitk;
    pl.lean = pl.nb == 2 && lab.wino_s2_lean && (lab.wino_s2_lean == 2 || (s.c_per_split / WKC <= 8 && grid >= 384));
    // Does the form pay against the implicit GEMM (tools/wino_s2_probe.py, profiles/r5_wino_s2_probe.txt)?  A workgroup is 32 tiles x 64
    // (or 128) channels with a fixed cost outside its K loop, so: forward -- where the grid fills the 256 CUs' rounds to 80 % (1.2 .. 1.5x
    // on down1 / down3 at both batch sizes and down2 at 32 images); data gradient -- K is the layer's output channels, only down1's four
    // steps in the two-per-CU form come out ahead (1.36 .. 1.42x; down2: 1.09x at 64 images, 0.72x at 32).
    const double fill = (double)grid / (double)(((grid + 255) / 256) * 256);
    pl.pays = groups == 4 ? (fill >= 0.8) : (pl.lean && chunks <= 4);
    pl.kernel = pl.nb == 4 ? CK_WINO32_NB4 : pl.lean ? CK_WINO32_NB2_LEAN : CK_WINO32_NB2;
    return pl;
}

inline W32Plan wino32_plan(const mtd_conv_args& a, int count, int groups) {
    const int lab_nb = conv_lab().wino_s2_nb;
    if (lab_nb == 4 && a.N % 128 == 0) return wino32_plan_nb(a, count, groups, 4);
    W32Plan pl = wino32_plan_nb(a, count, groups, 2);
    // forward grids the 64-channel workgroups leave short (down2 at 64 images: 144 of them, 0.93x): 128-channel workgroups and the
    // split of K that goes with them (72 x 3: 1.19x)
    if (!pl.pays && groups == 4 && a.N % 128 == 0 && lab_nb != 2) {
        const W32Plan p4 = wino32_plan_nb(a, count, groups, 4);
        if (p4.pays) pl = p4;
    }
    return pl;
}
inline int wino32_xcd_order(const mtd_conv_args& a, int count, int groups) {
    return xcd_order_of(64.0 * groups * a.C * a.N * count, (double)a.g.B * a.g.IH * a.g.IW * a.C * 4);
}

}  // namespace
