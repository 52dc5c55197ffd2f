// Prints the weight-gradient planner's answers (mtd-gan_amd/csrc/conv_wgrad_plan.h) over a fixed grid of layer shapes, one CSV row per
// shape and override: tests/test_wgrad_plan_cpu.py compares the output with tests/golden/wgrad_plans.csv.  Host only, no GPU.
//   wgrad_plan_dump        the grid under the default rule and under every override (rows "D")
//   wgrad_plan_dump lab    a few small maps with the Winograd kernels' minimum map side lowered to 2 (rows "L"; the switches are
//                          environment variables of a -DMTD_LAB build, so the program is compiled with it): the only way to a
//                          Winograd-eligible layer with fewer than two slices, which must fall through to the other kernels
// Regenerate the table after a plan changed on purpose:  ./wgrad_plan_dump > wgrad_plans.csv && ./wgrad_plan_dump lab >> wgrad_plans.csv
#include <stdio.h>
#include <string.h>
#include "../mtd-gan_amd/csrc/conv_wgrad_plan.h"

// ---- the planner's answers
static WgradForce force_of(int fcfg, int fsplit, int pair_mode = -1) {
    WgradForce f;
    f.cfg = fcfg;
    f.split = fsplit;
    f.pair_mode = pair_mode;
    return f;
}
static WPlan dump_plan(const mtd_wgrad_args& a, int div, int fcfg, int fsplit) { return make_wplan(a, div, force_of(fcfg, fsplit)); }
// {mtd_conv_wgrad_pair_ok, kernel, slices per half, units per slice, workspace floats}
static void dump_pair(const mtd_wgrad_args& a, int b_first, int pair_mode, int fcfg, int fsplit, long long out[5]) {
    const WPairPlan pp = wgrad_pair_plan(a, b_first, force_of(fcfg, fsplit, pair_mode));
    for (int i = 0; i < 5; ++i) out[i] = 0;
    if (!pp.ok) return;
    out[0] = pp.half.cfg == WCFG_WINO ? 2 : 1;
    out[1] = pp.half.cfg;
    out[2] = pp.half.nsplit;
    out[3] = pp.half.ppw;
    out[4] = (long long)wgrad_ws_floats(a, 2 * pp.half.nsplit);
}
static int dump_half(const mtd_wgrad_args& a, int fcfg, int fsplit) { return wgrad_half_scale_ok(a, force_of(fcfg, fsplit)) ? 1 : 0; }
static const char* dump_cfg_name(int cfg) { return kWgradCfg[cfg].name; }
static const int kDumpCfgCount = WCFG_COUNT;
// ---- (end of the planner's answers)

// geometries field for field as kernels.geom_fwd / kernels.geom_dgrad_s1 build them; H x W is the launch grid (the output map)
enum { K1 = 0, K3 = 1, K3T = 2, K4S2 = 3 };
static mtd_geom geom_fwd(int B, int IH, int IW, int k, int s, int p) {
    const int OH = (IH + 2 * p - k) / s + 1, OW = (IW + 2 * p - k) / s + 1;
    return mtd_geom{B, IH, IW, OH, OW, s, s, -p, -p, 1, 1, k, k, k, 0, 0, 1, 1, OH, OW, 1, 1, 0, 0};
}
static mtd_geom geom_dgrad_s1(int B, int H, int W, int k, int p) {
    const int GH = H + 2 * p - k + 1, GW = W + 2 * p - k + 1;
    return mtd_geom{B, GH, GW, H, W, 1, 1, p, p, -1, -1, k, k, k, 0, 0, 1, 1, H, W, 1, 1, 0, 0};
}
static float* const FAKE = (float*)4096;          // non-null, 16-byte aligned, never dereferenced
static mtd_wgrad_args args_of(int kind, int B, int H, int W, int N, int C) {
    mtd_wgrad_args a;
    memset(&a, 0, sizeof(a));
    a.g = kind == K1 ? geom_fwd(B, H, W, 1, 1, 0) : kind == K3 ? geom_fwd(B, H, W, 3, 1, 1) : kind == K3T ? geom_dgrad_s1(B, H, W, 3, 1)
                                                                                                             : geom_fwd(B, 2 * H, 2 * W, 4, 2, 1);
    const int T = a.g.TH * a.g.TW;
    a.p = FAKE; a.p_ld = N; a.N = N;
    a.q = FAKE; a.q_ld = C; a.C = C;
    a.dw = FAKE; a.w_sn = (long long)C * T; a.w_sc = T;
    return a;
}

static void row(const char* mode, int kind, int B, int H, int W, int N, int C, int fcfg, int fsplit) {
    const mtd_wgrad_args a = args_of(kind, B, H, W, N, C);
    if (check_wargs(a) != MTD_OK || is_direct(a)) { printf("%s,%d,%d,%d,%d,%d,%d,%d,%d,invalid\n", mode, kind, B, H, W, N, C, fcfg, fsplit); return; }
    printf("%s,%d,%d,%d,%d,%d,%d,%d,%d", mode, kind, B, H, W, N, C, fcfg, fsplit);
    int nsplit = 0;
    for (int div = 1; div <= 2; ++div) {
        const WPlan pl = dump_plan(a, div, fcfg, fsplit);
        printf(",%d,%d,%d,%d,%d,%d,%d,%d", pl.cfg, pl.WN, pl.WC, pl.TG, pl.ppw, pl.nsplit, pl.ntg, pl.nw);
        if (div == 1) nsplit = pl.nsplit;
    }
    for (int pair_mode = 1; pair_mode <= 3; ++pair_mode) {
        long long pr[5];
        dump_pair(a, B / 2, pair_mode, fcfg, fsplit, pr);
        printf(",%lld,%lld,%lld,%lld,%lld", pr[0], pr[1], pr[2], pr[3], pr[4]);
    }
    mtd_wgrad_args h = a;                           // half_scale over pixels [0, 32) / the rest (refused on maps of 32 pixels or fewer)
    h.half_scale = h.half_scale2 = FAKE;
    h.m_first = 32;
    printf(",%d,%lld\n", dump_half(h, fcfg, fsplit), (long long)wgrad_ws_floats(a, nsplit));
}

int main(int argc, char** argv) {
    const bool lab = argc > 1 && !strcmp(argv[1], "lab");
    if (argc > 1 && !strcmp(argv[1], "names")) {     // the plan numbers and their kernels
        for (int c = 0; c < kDumpCfgCount; ++c) printf("%d,%s\n", c, dump_cfg_name(c));
        return 0;
    }
    if (lab) {
        setenv("MTD_WGRAD_WINO_MIN_HW", "2", 1);
        setenv("MTD_WGRAD_WINO_S2_MIN_HW", "2", 1);
        for (int side = 2; side <= 6; side += 2)
            for (int B = 1; B <= 2; ++B) {
                row("L", K3, B, side, side, 64, 64, -1, -1);
                row("L", K4S2, B, side, side, 64, 64, -1, -1);
            }
        return 0;
    }
    printf("mode,kind,B,H,W,N,C,fcfg,fsplit,cfg,WN,WC,TG,ppw,nsplit,ntg,nw,cfg2,WN2,WC2,TG2,ppw2,nsplit2,ntg2,nw2,"
           "p1ok,p1cfg,p1ns,p1per,p1ws,p2ok,p2cfg,p2ns,p2per,p2ws,p3ok,p3cfg,p3ns,p3per,p3ws,half,ws\n");
    // the default rule: every 61st point of kinds x maps x N x C x B (61 is coprime to every extent, so each value of each axis
    // meets many values of the others) ...
    static const int maps[12][2] = {{1, 1}, {2, 2}, {4, 4}, {6, 6}, {8, 8}, {12, 12}, {16, 16}, {32, 32}, {64, 64}, {8, 16}, {12, 32}, {32, 12}};
    static const int chans[8] = {32, 64, 96, 128, 192, 256, 512, 1024};
    static const int batches[6] = {1, 2, 4, 16, 32, 64};
    for (int i = 0; i < 4 * 12 * 8 * 8 * 6; i += 61) {
        const int b = i % 6, c = (i / 6) % 8, n = (i / 48) % 8, m = (i / 384) % 12, kind = i / 4608;
        row("D", kind, batches[b], maps[m][0], maps[m][1], chans[n], chans[c], -1, -1);
    }
    // ... and one layer or more per kernel: the model's own, the two LDS-staged plans the grid above misses (0: a 3x3 layer of
    // more than 2048 pixels whose rows are no multiple of 16; 5: a 4x4 / stride-2 layer of 128 < M <= 256 pixels on a map below
    // 8 x 8), small maps.  These also go through every override: each plan number the planner reacts to, 7 as one it does not
    // (any number but -1 switches the default rule's special kernels off), and forced slice counts.
    static const int layers[14][6] = {{K1, 4, 16, 16, 64, 64},  {K1, 2, 64, 64, 32, 128},  {K3, 2, 64, 64, 32, 32},   {K3T, 2, 64, 64, 32, 32}, {K3, 4, 32, 32, 64, 64},
                                      {K3, 16, 8, 8, 128, 64},  {K3, 16, 4, 4, 128, 128},  {K3, 32, 2, 2, 512, 512},  {K3, 32, 12, 12, 32, 32}, {K3, 4, 6, 6, 96, 96},
                                      {K4S2, 4, 32, 32, 64, 64}, {K4S2, 16, 4, 4, 64, 128}, {K4S2, 32, 2, 2, 256, 256}, {K4S2, 2, 16, 16, 32, 32}};
    static const int forces[17][2] = {{-1, -1}, {-2, -1}, {0, -1}, {1, -1}, {2, -1}, {3, -1}, {4, -1}, {5, -1}, {6, -1}, {7, -1}, {13, -1}, {15, -1},
                                      {16, -1}, {18, -1}, {19, -1}, {-1, 1}, {-1, 3}};
    for (const auto& l : layers)
        for (const auto& f : forces) row("D", l[0], l[1], l[2], l[3], l[4], l[5], f[0], f[1]);
    for (const auto& l : layers) row("D", l[0], l[1], l[2], l[3], l[4], l[5], 16, 1000);       // more slices than the layer can have
    for (const auto& l : layers) row("D", l[0], l[1], l[2], l[3], l[4], l[5], 15, 1000);
    return 0;
}
