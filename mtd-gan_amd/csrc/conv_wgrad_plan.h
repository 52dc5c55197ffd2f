// The weight-gradient planner: layer geometry in, kernel and pixel split out.  Plain C++17 host arithmetic (no HIP header:
// tests/wgrad_plan_dump.cpp compiles it with g++), included by conv_wgrad.hip and by the three Winograd kernel headers for the
// chunk sizes.  tests/golden/wgrad_plans.csv pins every result over a grid of layer shapes (tests/test_wgrad_plan_cpu.py).
#pragma once
#include <stddef.h>
#include "host_util.h"

namespace {

// ---- the plans.  The numbers are an interface: the profiler's records, kernels.WGRAD_CONFIGS, mtd_conv_wgrad_plan_cfg,
// mtd_conv_wgrad_override, tests and tools index by them (14 and 17 are retired).
enum WgradCfg : int {
    WCFG_KEEP_LDS = -2,                     // mtd_conv_wgrad_override only: keep the LDS-staged kernels (A/B comparison)
    WCFG_AUTO = -1,                         // mtd_conv_wgrad_override: the default rule
    WCFG_T9 = 0, WCFG_T4, WCFG_64_T1, WCFG_T8, WCFG_T3, WCFG_T1, WCFG_64_T3,     // wgrad_kernel<WN, WC, TG>: LDS-staged
    WCFG_ROW3, WCFG_ROW3_REV, WCFG_ROW1,    // row-window kernel: 3x3 forward / transposed tap order, 1x1
    WCFG_BLK8, WCFG_BLK4, WCFG_BLK2,        // block-window kernel on 8x8, 4x4, 2x2 maps
    WCFG_TAPS = 13,                         // all-taps kernel of the 4x4 layers
    WCFG_S2 = 15,                           // stride-2 halo-window kernel
    WCFG_WINO = 16,                         // Winograd F(2x2, 3x3) on 64 x 64 blocks (conv_wgrad_wino.h)
    WCFG_WINO_S2 = 18,                      // Winograd F(3x3, 2x2) of the 4x4 / stride-2 layers (conv_wgrad_wino_s2.h)
    WCFG_WINO32 = 19,                       // Winograd F(2x2, 3x3) on one 32 x 32 block (conv_wgrad_wino32.h)
    WCFG_COUNT
};

// name: the profiler's (kernels.WGRAD_CONFIGS).  WN x WC blocks of 32 x 32 per wave; TG taps per workgroup (0: all of them).
// pairs: the kernel takes two problems in one launch (WgradParams::pair_ns; the Winograd kernels have a pair form of their
// own, wgrad_pair_plan).  half_scale: the kernel applies mtd_wgrad_args.half_scale.
// (A 64 x 64 tile with a whole filter row per workgroup, wgrad_kernel<2, 2, 4>, needs 256 accumulator registers and spilled
// 600 bytes per lane: not instantiated.)
struct WgradCfgDesc { const char* name; int WN, WC, TG; bool pairs, half_scale; };
constexpr WgradCfgDesc kWgradCfg[WCFG_COUNT] = {
    {"wgrad_kernel<1, 1, 9>", 1, 1, 9, true, true},
    {"wgrad_kernel<1, 1, 4>", 1, 1, 4, true, true},
    {"wgrad_kernel<2, 2, 1>", 2, 2, 1, true, true},
    {"wgrad_kernel<1, 1, 8>", 1, 1, 8, true, true},
    {"wgrad_kernel<1, 1, 3>", 1, 1, 3, true, true},
    {"wgrad_kernel<1, 1, 1>", 1, 1, 1, true, true},
    {"wgrad_kernel<2, 2, 3>", 2, 2, 3, true, true},
    {"wgrad_row_kernel<3, 3, 1>", 1, 1, 0, false, false},
    {"wgrad_row_kernel<3, 3, -1>", 1, 1, 0, false, false},
    {"wgrad_row_kernel<1, 1, 1>", 1, 1, 0, false, false},
    {"wgrad_blk_kernel<8>", 1, 1, 0, true, true},
    {"wgrad_blk_kernel<4>", 1, 1, 0, true, true},
    {"wgrad_blk_kernel<2>", 1, 1, 0, true, true},
    {"wgrad_taps_kernel", 1, 1, 0, true, true},
    {"?", 0, 0, 0, false, false},
    {"wgrad_s2_kernel", 1, 1, 0, true, false},
    {"wgrad_wino_kernel", 2, 2, 0, false, false},
    {"?", 0, 0, 0, false, false},
    {"wgrad_wino_s2_kernel", 2, 2, 0, false, false},
    {"wgrad_wino32_kernel", 1, 1, 0, false, false},
};
inline bool wgrad_cfg_lds_staged(int cfg) { return cfg >= 0 && cfg < WCFG_COUNT && kWgradCfg[cfg].TG > 0; }

// cfg: the kernel; WN, WC, TG as in the table (TG = the layer's taps where the table says all); ppw: pixels per wave -- per
// WORKGROUP for the all-taps kernel, 8 x 8 pixel blocks per workgroup for the stride-2 kernel, chunks of tiles per slice for the
// Winograd kernels; nsplit: pixel slices = slabs; ntg: tap groups; nw: waves per workgroup.
struct WPlan { int cfg, WN, WC, TG, ppw, nsplit, ntg, nw; };

// What the tuning hooks ask for (mtd_conv_wgrad_override, mtd_conv_wgrad_pair_mode; the globals live with the API).
// pair_mode 0: never pair, 1: the default rule, 2: Winograd kernels only, 3: every kernel that has a pair form, -1: the lab
// switch MTD_WGRAD_PAIR.  nw: waves per workgroup of the register-operand kernels (lab switch MTD_WGRAD_NW), 0 = the plan's.
struct WgradForce { int cfg = WCFG_AUTO, split = -1, nw = 0, pair_mode = -1; };

// ---- lab switches (host_util.h: environment variables of a -DMTD_LAB build, read once; the shipped library has the defaults
// compiled in).  X(field, variable, default)
#define WGRAD_LAB_SWITCHES(X)                                                                                                              \
    X(t16_plan, "MTD_WGRAD_T16_PLAN", 1)               /* 4x4 layers on the LDS-staged kernels: round 6's thresholds (0: round 5's) */     \
    X(wino32, "MTD_WGRAD_WINO32", 1)                   /* plan 19 where it applies ... */                                                  \
    X(wino32_min_hw, "MTD_WGRAD_WINO32_MIN_HW", 32)    /* ... on maps of at least this many pixels a side */                               \
    X(wino_s2, "MTD_WGRAD_WINO_S2", 1)                 /* plan 18 ... */                                                                   \
    X(wino_s2_min_hw, "MTD_WGRAD_WINO_S2_MIN_HW", 8)   /* ... on output maps of at least this many pixels a side */                        \
    X(s2, "MTD_WGRAD_S2", 1)                           /* plan 15 */                                                                       \
    X(s2_wgs, "MTD_WGRAD_S2_WGS", 512)                 /* its workgroup target */                                                          \
    X(s2_db, "MTD_WGRAD_S2_DB", 0)                     /* its double-buffered form */                                                      \
    X(taps, "MTD_WGRAD_TAPS", 1)                       /* plan 13 ... */                                                                   \
    X(taps_maxm, "MTD_WGRAD_TAPS_MAXM", 128)           /* ... up to this many pixels */                                                    \
    X(taps_wgs, "MTD_WGRAD_TAPS_WGS", 256)             /* its workgroup target */                                                          \
    X(wino, "MTD_WGRAD_WINO", 1)                       /* plan 16 ... */                                                                   \
    X(wino_min_hw, "MTD_WGRAD_WINO_MIN_HW", 8)         /* ... on maps of at least this many pixels a side */                               \
    X(nw, "MTD_WGRAD_NW", 0)                           /* 4 or 8: WgradForce::nw */                                                        \
    X(lds_pad, "MTD_WGRAD_LDS_PAD", 65536)             /* bytes of unused dynamic LDS of the 3x3 row-window launch (conv_wgrad.hip) */     \
    X(fused_reduce, "MTD_WGRAD_FUSED_REDUCE", 1)       /* one-launch slab sum and scatter */                                               \
    X(scalar2, "MTD_WGRAD_SCALAR2", 1)                 /* thin layers: both reduce stages in one launch */                                 \
    X(pair, "MTD_WGRAD_PAIR", 1)                       /* WgradForce::pair_mode -1 */
struct WgradLab {
#define X(field, name, dflt) int field = dflt;
    WGRAD_LAB_SWITCHES(X)
#undef X
};
inline const WgradLab& wgrad_lab() {
    static const WgradLab lab = [] {
        WgradLab l;
#define X(field, name, dflt) if (const char* e = mtd_lab_env(name)) l.field = atoi(e);
        WGRAD_LAB_SWITCHES(X)
#undef X
        return l;
    }();
    return lab;
}

// ---- arguments
inline bool is_direct(const mtd_wgrad_args& a) { return (a.N % 32) || (a.C % 32); }

inline int check_wargs(const mtd_wgrad_args& a) {
    if (!a.p || !a.q || !a.dw) return MTD_EINVAL;
    if (a.N <= 0 || a.C <= 0) return MTD_EINVAL;
    if (is_direct(a)) {
        if (a.N != 1 && a.C != 1) return MTD_EINVAL;
        const mtd_geom& g = a.g;
        if (g.B <= 0 || g.TH <= 0 || g.TW <= 0 || g.TH * g.TW > 16) return MTD_EINVAL;
        if (a.p_ld < a.N || a.q_ld < a.C) return MTD_EINVAL;
        return MTD_OK;
    }
    const mtd_geom& g = a.g;
    if (g.B <= 0 || g.IH <= 0 || g.IW <= 0 || g.OH <= 0 || g.OW <= 0) return MTD_EINVAL;
    if (g.TH <= 0 || g.TW <= 0 || g.TH * g.TW > 16) return MTD_EINVAL;
    if (geom_pixels(g) > (1ll << 30)) return MTD_EINVAL;
    if (a.p_ld < a.N || a.q_ld < a.C || (a.p_ld % 4) || (a.q_ld % 4)) return MTD_EINVAL;
    if (!aligned16(a.p) || !aligned16(a.q)) return MTD_EALIGN;
    if (a.half_scale && (!a.half_scale2 || a.m_first <= 0 || (a.m_first % 32) || a.m_first >= geom_pixels(g))) return MTD_EINVAL;
    return MTD_OK;
}

// ---- the kernels' domains
// row-window kernel: stride 1, rows of a multiple of 16 output pixels, 3x3 (unit tap spacing) or 1x1
inline bool row_window_ok(const mtd_wgrad_args& a) {
    const mtd_geom& g = a.g;
    if (g.in_sy != 1 || g.in_sx != 1 || (g.OW % 16) != 0) return false;
    if (g.TH == 1 && g.TW == 1) return true;
    return g.TH == 3 && g.TW == 3 && (g.tap_dx == 1 || g.tap_dx == -1);
}

// block-window kernel: 3x3 / stride 1 / pad 1 on square 8x8, 4x4 or 2x2 maps (forward tap order)
inline int block_window_w(const mtd_wgrad_args& a) {
    const mtd_geom& g = a.g;
    if (g.in_sy != 1 || g.in_sx != 1 || g.TH != 3 || g.TW != 3 || g.tap_dy != 1 || g.tap_dx != 1) return 0;
    if (g.off_y != -1 || g.off_x != -1 || g.IH != g.OH || g.IW != g.OW || g.OH != g.OW) return 0;
    return (g.OW == 8 || g.OW == 4 || g.OW == 2) ? g.OW : 0;
}

// stride-2 halo-window kernel: the forward geometry of Conv2d(k4, s2, p1) on whole 8 x 8 blocks of output pixels
inline bool wgrad_s2_ok(const mtd_wgrad_args& a) {
    const mtd_geom& g = a.g;
    return g.TH == 4 && g.TW == 4 && g.in_sy == 2 && g.in_sx == 2 && g.off_y == -1 && g.off_x == -1 && g.tap_dy == 1 && g.tap_dx == 1 &&
           (g.OH % 8) == 0 && (g.OW % 8) == 0;
}

// Winograd F(2x2, 3x3), conv_wgrad_wino.h: forward-oriented 3x3 / stride 1 / pad 1, even map sides, N and C multiples of 64
constexpr int WGW_T = 8;                       // tiles per chunk (also of conv_wgrad_wino_s2.h)
inline bool wgrad_wino_ok(const mtd_wgrad_args& a) {
    const mtd_geom& g = a.g;
    if (g.TH != 3 || g.TW != 3 || g.in_sy != 1 || g.in_sx != 1 || g.tap_dy != 1 || g.tap_dx != 1 || g.off_y != -1 || g.off_x != -1) return false;
    if (g.ky0 != 0 || g.kx0 != 0 || g.ky_step != 1 || g.kx_step != 1 || g.KW != 3) return false;
    if (g.IH != g.OH || g.IW != g.OW || (g.OH & 1) || (g.OW & 1)) return false;
    if ((a.N % 64) || (a.C % 64)) return false;
    if (!aligned16(a.p) || !aligned16(a.q) || (a.p_ld % 4) || (a.q_ld % 4)) return false;
    return true;
}
// (n, c) blocks and tiles of a layer in the form it takes
inline long long wgrad_wino_blocks(const mtd_wgrad_args& a) { return (long long)(a.N / 64) * (a.C / 64); }
inline long long wgrad_wino_tiles(const mtd_wgrad_args& a, long long images) { return images * (a.g.OH / 2) * (a.g.OW / 2); }

// Winograd F(3x3, 2x2), conv_wgrad_wino_s2.h: the forward geometry of Conv2d(k4, s2, p1), N and C multiples of 64
inline bool wgrad_wino_s2_ok(const mtd_wgrad_args& a) {
    const mtd_geom& g = a.g;
    if (g.TH != 4 || g.TW != 4 || g.in_sy != 2 || g.in_sx != 2 || g.tap_dy != 1 || g.tap_dx != 1 || g.off_y != -1 || g.off_x != -1) return false;
    if (g.ky0 != 0 || g.kx0 != 0 || g.ky_step != 1 || g.kx_step != 1 || g.KW != 4) return false;
    if (g.IH != 2 * g.OH || g.IW != 2 * g.OW) return false;
    if ((a.N % 64) || (a.C % 64)) return false;
    if (!aligned16(a.p) || !aligned16(a.q) || (a.p_ld % 4) || (a.q_ld % 4)) return false;
    return true;
}
inline long long wgrad_wino_s2_blocks(const mtd_wgrad_args& a) { return (long long)(a.N / 64) * (4 * a.C / 64); }
inline long long wgrad_wino_s2_tiles(const mtd_wgrad_args& a, long long images) { return images * ((a.g.OH + 2) / 3) * ((a.g.OW + 2) / 3); }

// Winograd F(2x2, 3x3) on one 32 x 32 block, conv_wgrad_wino32.h: 3x3 / stride 1 / pad 1 in the forward (tap_d = +1, off = -1) or
// the transposed (tap_d = -1, off = +1) tap order, N = C = 32, even height, width a multiple of 4 (tile rows of an even number of tiles)
constexpr int W32_T = 16;                      // tiles per chunk
inline bool wgrad_wino32_ok(const mtd_wgrad_args& a) {
    const mtd_geom& g = a.g;
    if (g.TH != 3 || g.TW != 3 || g.in_sy != 1 || g.in_sx != 1 || g.tap_dy != g.tap_dx) return false;
    if (!((g.tap_dy == 1 && g.off_y == -1 && g.off_x == -1) || (g.tap_dy == -1 && g.off_y == 1 && g.off_x == 1))) return false;
    if (g.ky0 != 0 || g.kx0 != 0 || g.ky_step != 1 || g.kx_step != 1 || g.KW != 3) return false;
    if (g.IH != g.OH || g.IW != g.OW || (g.OH & 1) || (g.OW & 3)) return false;
    if (a.N != 32 || a.C != 32) return false;
    if (!aligned16(a.p) || !aligned16(a.q) || (a.p_ld % 4) || (a.q_ld % 4)) return false;
    return true;
}

// ---- the pixel split
inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// `units` of work (pixels, 8 x 8 blocks, chunks of tiles) over `want` slices -- at most max_ns, then at least min_ns, never more
// than there are units.  A slice is `parts` runs (the waves of a workgroup) of `per` units each, per a multiple of `round`;
// the slice count is what runs of that length leave.
struct WSplit { long long per, ns; };
inline WSplit wgrad_split(long long units, long long want, long long max_ns, long long min_ns = 1, int parts = 1, int round = 1) {
    long long ns = want;
    if (ns > max_ns) ns = max_ns;
    if (ns < min_ns) ns = min_ns;
    if (ns > units) ns = units;
    const long long per = ceil_div(ceil_div(units, ns * parts), round) * round;
    return {per, ceil_div(units, per * parts)};
}
// slices that bring the launch to `wgs` workgroups of `tiles` (n, c, tap group) tiles each, unless the override names a count
inline long long want_splits(const WgradForce& f, long long wgs, long long tiles) { return f.split > 0 ? f.split : ceil_div(wgs, tiles); }

inline WPlan wplan_of(int cfg, int T, const WSplit& s, int nw) {
    const WgradCfgDesc& d = kWgradCfg[cfg];
    const int TG = d.TG ? d.TG : T;
    return WPlan{cfg, d.WN, d.WC, TG, (int)s.per, (int)s.ns, (T + TG - 1) / TG, nw};
}

// The plan of one layer (arguments that passed check_wargs and are not is_direct).  div: 2 while planning ONE of the two problems
// of a pair launch (half the workgroup targets).  div and f are parameters, not globals, so that concurrent callers (main thread
// + autograd's backward thread, several devices) cannot see each other's values.
inline WPlan make_wplan(const mtd_wgrad_args& a, int div, const WgradForce& f) {
    const WgradLab& lab = wgrad_lab();
    const mtd_geom& g = a.g;
    const int T = g.TH * g.TW;
    const long long M = geom_pixels(g);
    const bool n64 = a.N % 64 == 0 && a.C % 64 == 0;
    // a kernel beyond the LDS-staged ones: the default rule with its lab switch on, or the override names it
    const auto takes = [&](int lab_switch, WgradCfg cfg) { return (lab_switch && f.cfg == WCFG_AUTO) || f.cfg == cfg; };
    const auto side_ge = [&](int hw) { return g.OH >= hw && g.OW >= hw; };
    const long long tiles32 = (long long)(a.N / 32) * (a.C / 32);

    // Winograd on one 32 x 32 block: the generator's 32 -> 32 layers (where the row-window kernel is the plan otherwise).  About
    // one workgroup per CU, at least four chunks of 16 tiles per slice; fewer than two slices: not this kernel.
    if (takes(lab.wino32, WCFG_WINO32) && wgrad_wino32_ok(a) && side_ge(lab.wino32_min_hw)) {
        const long long chunks = ceil_div(wgrad_wino_tiles(a, g.B), W32_T);
        const WSplit s = wgrad_split(chunks, want_splits(f, 256 / div, 1), chunks / 4);
        if (s.ns >= 2) return wplan_of(WCFG_WINO32, T, s, 8);
    }
    // Winograd form of the 4x4 / stride-2 layers, planned like plan 16 below
    if (takes(lab.wino_s2, WCFG_WINO_S2) && wgrad_wino_s2_ok(a) && side_ge(lab.wino_s2_min_hw)) {
        const long long chunks = ceil_div(wgrad_wino_s2_tiles(a, g.B), WGW_T);
        const WSplit s = wgrad_split(chunks, want_splits(f, 256, wgrad_wino_s2_blocks(a)), chunks / 4, 2);
        if (s.ns >= 2) return wplan_of(WCFG_WINO_S2, T, s, 8);
    }
    // halo-window kernel: 8 x 8 pixel blocks; ~512 workgroups of the single-buffer form, two per CU (51 KB of LDS each), which take
    // turns on the matrix cores: 46.6-49.6 us per layer against 51-54 for 256 double-buffered workgroups and 57 for wgrad_kernel<2,2,1>
    if (takes(lab.s2, WCFG_S2) && wgrad_s2_ok(a)) {
        const long long NB = (long long)g.B * (g.OH / 8) * (g.OW / 8);
        return wplan_of(WCFG_S2, T, wgrad_split(NB, want_splits(f, lab.s2_wgs / div, tiles32), NB), 4);
    }
    // all-taps kernel: ~one workgroup per CU; pixels per workgroup a multiple of 32
    if (g.TH == 4 && g.TW == 4 && ((lab.taps && f.cfg == WCFG_AUTO && M <= lab.taps_maxm) || f.cfg == WCFG_TAPS))
        return wplan_of(WCFG_TAPS, T, wgrad_split(M, want_splits(f, lab.taps_wgs / div, tiles32), ceil_div(M, 32), 1, 1, 32), 4);
    // Winograd F(2x2, 3x3): about one workgroup per CU, at least four chunks of eight tiles per slice, and always through slabs
    // (two slices or more: the kernel has no direct-store form; a layer too small for that stays on the kernels below)
    if (takes(lab.wino, WCFG_WINO) && wgrad_wino_ok(a) && side_ge(lab.wino_min_hw)) {
        const long long chunks = ceil_div(wgrad_wino_tiles(a, g.B), WGW_T);
        const WSplit s = wgrad_split(chunks, want_splits(f, 256, wgrad_wino_blocks(a)), chunks / 4, 2);
        if (s.ns >= 2) return wplan_of(WCFG_WINO, T, s, 8);
    }
    // register-operand kernels (row window, block window): ~one workgroup per CU, at least 32 pixels per wave.  Four waves per
    // workgroup; eight (two per SIMD, same workgroup count and slab traffic) measured 1 % faster standalone and no different
    // inside the step, so it stays a lab switch (MTD_WGRAD_NW=8; the 8x8 window kernel needs more than 256 registers)
    const int bw = block_window_w(a);
    if ((row_window_ok(a) || bw) && f.cfg != WCFG_KEEP_LDS) {
        const int cfg = bw ? (bw == 8 ? WCFG_BLK8 : (bw == 4 ? WCFG_BLK4 : WCFG_BLK2)) : (T == 1 ? WCFG_ROW1 : (g.tap_dx > 0 ? WCFG_ROW3 : WCFG_ROW3_REV));
        const int nw = (f.nw == 8 && bw != 8) ? 8 : 4;
        return wplan_of(cfg, T, wgrad_split(M, want_splits(f, 256 / div, tiles32), ceil_div(M, 128), 1, nw, 32), nw);
    }
    // LDS-staged kernels (strided convs and feature maps narrower than 16 pixels); choices from tools/census.py --sweep-wgrad.
    // 4x4 taps (round 6, tools/wgrad_s2_small_probe.py: both halves of a paired pass are one launch now, so down4 has 1024 pixels
    // and down5 256): 64 x 64 tiles with one tap each from 1024 pixels on (108 us against 140 for 32 x 32 tiles x 3 taps), 32 x 32
    // tiles with one tap each up to 256 pixels (42 us against 51)
    int cfg;
    if (T == 1 && n64) cfg = WCFG_64_T1;
    else if (T <= 4) cfg = WCFG_T4;
    else if (T <= 9) cfg = (M <= 2048) ? WCFG_T3 : WCFG_T9;       // few pixels, many tiles: 3 taps per wave, no pixel split
    else if (!lab.t16_plan) cfg = (M >= 2048 && n64) ? WCFG_64_T1 : WCFG_T3;
    else if (M >= 1024 && n64) cfg = WCFG_64_T1;
    else cfg = (M <= 256) ? WCFG_T1 : WCFG_T3;
    if (wgrad_cfg_lds_staged(f.cfg) && a.N % (32 * kWgradCfg[f.cfg].WN) == 0 && a.C % (32 * kWgradCfg[f.cfg].WC) == 0) cfg = f.cfg;
    // aim for >= 512 workgroups; every wave gets a multiple of 32 pixels, at least 32
    const WgradCfgDesc& d = kWgradCfg[cfg];
    const long long tiles = (long long)(a.N / (32 * d.WN)) * (a.C / (32 * d.WC)) * ((T + d.TG - 1) / d.TG);
    return wplan_of(cfg, T, wgrad_split(M, want_splits(f, 512 / div, tiles), ceil_div(M, 128), 1, 4, 32), 4);
}

// mtd_wgrad_args.half_scale: the register-operand kernels only (their K loops walk whole 32-pixel chunks of one half)
inline bool wgrad_half_scale_ok(const mtd_wgrad_args& a, const WgradForce& f) {
    if (!a.half_scale || check_wargs(a) != MTD_OK || is_direct(a)) return false;
    return kWgradCfg[make_wplan(a, 1, f).cfg].half_scale;
}

// ---- the two batch halves of a paired discriminator pass in ONE launch: images [0, b_first) and [b_first, B) of a, each with a
// weight gradient of its own.  ok: the layer has the form; half: the plan of ONE half (half.cfg the kernel, half.nsplit slices
// per half, 2 half.nsplit slabs).  The Winograd kernels align their slices to the image ranges (half.ppw chunks per slice); the
// kernels of WgradCfgDesc::pairs run the plan of one half with half the workgroup targets on both.
struct WPairPlan { bool ok; WPlan half; };
inline WPairPlan wgrad_pair_plan(const mtd_wgrad_args& a, int b_first, const WgradForce& f) {
    const WPairPlan none{false, WPlan{}};
    if (check_wargs(a) != MTD_OK || is_direct(a)) return none;
    if (b_first <= 0 || 2 * b_first != a.g.B) return none;
    const int mode = f.pair_mode >= 0 ? f.pair_mode : wgrad_lab().pair;
    if (!mode) return none;
    mtd_wgrad_args h = a;
    h.g.B = b_first;
    const int cfg = make_wplan(h, 1, f).cfg;
    if (cfg == WCFG_WINO || cfg == WCFG_WINO_S2) {      // the two ranges together: about one workgroup per CU
        const bool s2 = cfg == WCFG_WINO_S2;
        const long long blocks = s2 ? wgrad_wino_s2_blocks(a) : wgrad_wino_blocks(a);
        const long long chunks = ceil_div(s2 ? wgrad_wino_s2_tiles(a, b_first) : wgrad_wino_tiles(a, b_first), WGW_T);
        return {true, wplan_of(cfg, a.g.TH * a.g.TW, wgrad_split(chunks, ceil_div(128, blocks), chunks / 4), 8)};
    }
    // By default only the stride-2 halo-window kernel (`down` layers with output maps of at least 8x8: 14-21 us less per
    // pair).  The small-map kernels lose: their single launches have one pixel split and write the gradient themselves, a pair
    // launch has two slabs per (n, c) tile and a reduce (down4 132 -> 210 us, down6 26 -> 102 us, conv5x 47 -> 66 us;
    // tools/wgrad_pair_probe.py).
    if (mode == 2 || (mode != 3 && cfg != WCFG_S2) || !kWgradCfg[cfg].pairs) return none;
    return {true, make_wplan(h, 2, f)};
}

// ---- workspace: nsplit slabs and the staging areas of the reduce
constexpr int GS = 64;   // slabs summed per reduce stage (eight loads in flight per thread: 64 slabs cost less than a second launch)

inline size_t wgrad_ws_floats(const mtd_wgrad_args& a, int nsplit) {
    const long long T = a.g.TH * a.g.TW;
    const long long stride = T * a.N * a.C + a.N;
    long long total = (long long)nsplit * stride;
    long long ns = nsplit;
    while (ns > GS) {           // intermediate stages
        ns = (ns + GS - 1) / GS;
        total += ns * stride;
    }
    return (size_t)total;
}

}  // namespace
