// Prints the answers of the forward-conv planners (mtd-gan_amd/csrc/conv_plan.h) over fixed grids of layer shapes, one CSV row per shape
// and override: tests/test_conv_plan_cpu.py compares the output with tests/golden/conv_plans_{igemm,wino,s2}.csv.  Host only, no GPU.
//   conv_plan_dump igemm | wino | s2     the table of one planner: the default rule and every override (rows "D")
//   conv_plan_dump igemm lab             the lab switch MTD_IGEMM_PLAN=2 (rows "L"; environment variables of a -DMTD_LAB build, so the
//                                        program is compiled with it): round 2's rules for the large 3x3 grids, off by default
//   conv_plan_dump names                 the kernel numbers and their names
//   conv_plan_dump <table> dense         a denser grid of the same axes (not committed: for comparing two planners once)
// Regenerate a table after a plan changed on purpose:  ./conv_plan_dump igemm > conv_plans_igemm.csv && ./conv_plan_dump igemm lab >> conv_plans_igemm.csv
#include <stdio.h>
#include <string.h>
#include "../mtd-gan_amd/csrc/conv_plan.h"

// ---- the planners' answers
// the route (a ConvKernel or MTD_E*), the plan of a launch of `sets` problems, the derived flags and the answers of the workspace,
// mtd_conv_relu_add_ok and mtd_resfft_block_tail_ok queries
struct IgemmAns { int route, cfg, BM, BN, splitk, cps, wide, fin; long long ws; int relu, tail; };
static IgemmAns dump_igemm(const mtd_conv_args& a, int sets, int fcfg, int fsplit) {
    ConvForce f;
    f.cfg = fcfg;
    f.split = fsplit;
    IgemmAns r{};
    r.route = check_args(a);
    if (r.route != MTD_OK) return r;
    const ConvRoute rt = conv_igemm_route(a, sets, f);
    const Plan pl = make_plan(a, f, sets);
    return {rt.kernel, pl.cfg, pl.BM, pl.BN, pl.splitk, pl.c_per_split, conv_wide(&a, 1, pl.splitk), conv_fin(a, pl), (long long)splitk_ws_bytes(a, rt.plan.splitk),
            conv_relu_add_ok(a, f) ? 1 : 0, c32t_tail_ok(a) ? 1 : 0};
}
// a: the layer (w_st free); the plan is that of the launch whose weights were built for the code `px`
struct WinoAns { int ok, px, nb, lean, splitk, cps, c32, g2, g3, xcd; long long ws; };
static WinoAns dump_wino(mtd_conv_args a, int f4_min_w, int wino_split) {
    ConvForce f;
    f.f4_min_w = f4_min_w;
    f.wino_split = wino_split;
    WinoAns r{};
    r.ok = wino_args_ok(&a, f) ? 1 : 0;
    if (!r.ok) return r;
    r.px = wino_patch_w(a, f);
    a.w_st = r.px;
    const int code = wino_args_px(a);
    const WinoPlan pl = wino_plan(a, code);
    const mtd_conv_args g[3] = {a, a, a};
    r.nb = pl.nb; r.lean = pl.lean; r.splitk = pl.splitk; r.cps = pl.c_per_split;
    r.c32 = wino_c32_takes(a, code) ? 1 : 0;
    r.g2 = wino_group_ok(g, 2, f) ? 1 : 0;
    r.g3 = wino_group_ok(g, 3, f) ? 1 : 0;
    r.xcd = wino_xcd_order(a, pl.px);
    r.ws = (long long)splitk_ws_bytes(a, pl.splitk);
    return r;
}
struct W32Ans { int elig, groups, nb, lean, pays, splitk; long long ws; };
static W32Ans dump_w32(const mtd_conv_args* a, int count) {
    W32Ans r{};
    r.elig = wino32_eligible(a, count) ? 1 : 0;
    if (!r.elig) return r;
    W32Form f;
    wino32_form(a[0].g, f);
    const W32Plan pl = wino32_plan(a[0], count, f.groups);
    return {1, f.groups, pl.nb, pl.lean, pl.pays, pl.splitk, (long long)splitk_ws_bytes(a[0], pl.splitk)};
}
static const char* dump_kernel_name(int k) { return kConvKernel[k].name; }
static const int kDumpKernelCount = CK_COUNT;
// ---- (end of the planners' answers)

// geometries field for field as kernels.geom_fwd / geom_dgrad_s1 / geom_dgrad_s2 build them; H x W is the launch grid
enum { K1 = 0, K3 = 1, K3T = 2, K4S2 = 3, KDG = 4 };
static mtd_geom geom_fwd(int B, int IH, int IW, int k, int s, int p) {
    const int OH = (IH + 2 * p - k) / s + 1, OW = (IW + 2 * p - k) / s + 1;
    return mtd_geom{B, IH, IW, OH, OW, s, s, -p, -p, 1, 1, k, k, k, 0, 0, 1, 1, OH, OW, 1, 1, 0, 0};
}
static mtd_geom geom_dgrad_s1(int B, int H, int W, int k, int p) {
    const int GH = H + 2 * p - k + 1, GW = W + 2 * p - k + 1;
    return mtd_geom{B, GH, GW, H, W, 1, 1, p, p, -1, -1, k, k, k, 0, 0, 1, 1, H, W, 1, 1, 0, 0};
}
static mtd_geom geom_dgrad_s2(int B, int H, int W, int py, int px) {      // class (py, px) of the data gradient of Conv2d(k4, s2, p1)
    const int ky0 = (py + 1) & 1, kx0 = (px + 1) & 1;
    const int oy = (py + 1 - ky0) / 2, ox = (px + 1 - kx0) / 2;
    return mtd_geom{B, H / 2, W / 2, H / 2, W / 2, 1, 1, oy, ox, -1, -1, 2, 2, 4, ky0, kx0, 2, 2, H, W, 2, 2, py, px};
}

// Operands are fake addresses that are never dereferenced: 16-byte aligned, or 4 bytes past that.  var: bits that vary the operands --
enum { V_OUT4 = 1,        // out 4 bytes off alignment
       V_WS4 = 2,         // ws 4 bytes off
       V_BIAS4 = 4,       // a bias, 4 bytes off
       V_MASK = 8,        // a mask ...
       V_MASK4 = 16,      // ... 4 bytes off
       V_ADD1 = 32,       // a residual operand
       V_OUT2 = 64,       // a second output
       V_RELU_ADD = 128,  // act = MTD_ACT_RELU_ADD
       V_CTR = 256,       // arrival counters for 2^20 tiles
       V_LD2 = 512 };     // out_ld = N + 2: rows of the output not 16-byte aligned
static char* const FAKE = (char*)4096;
static mtd_conv_args args_of(int kind, int cls, int B, int H, int W, int N, int C, int var) {
    mtd_conv_args a;
    memset(&a, 0, sizeof(a));
    a.g = kind == K1 ? geom_fwd(B, H, W, 1, 1, 0) : kind == K3 ? geom_fwd(B, H, W, 3, 1, 1) : kind == K3T ? geom_dgrad_s1(B, H, W, 3, 1)
        : kind == K4S2 ? geom_fwd(B, 2 * H, 2 * W, 4, 2, 1) : geom_dgrad_s2(B, 2 * H, 2 * W, cls >> 1, cls & 1);
    a.in = (const float*)FAKE; a.in_ld = C; a.C = C;
    a.w = (const float*)FAKE; a.w_sn = C; a.w_sc = 1; a.w_st = (long long)N * C; a.N = N;       // packed weights [tap][n][c]
    a.out = (float*)(FAKE + ((var & V_OUT4) ? 4 : 0)); a.out_ld = N + ((var & V_LD2) ? 2 : 0);
    a.ws = (float*)(FAKE + ((var & V_WS4) ? 4 : 0)); a.ws_bytes = (size_t)1 << 40;
    if (var & V_BIAS4) a.bias = (const float*)(FAKE + 4);
    if (var & V_MASK) { a.mask = (const float*)(FAKE + ((var & V_MASK4) ? 4 : 0)); a.mask_ld = N; }
    if (var & V_ADD1) { a.add1 = (const float*)FAKE; a.add1_ld = N; }
    if (var & V_OUT2) { a.out2 = (float*)FAKE; a.out2_ld = N; }
    if (var & V_RELU_ADD) a.act = MTD_ACT_RELU_ADD;
    if (var & V_CTR) { a.tile_ctr = (unsigned*)FAKE; a.tile_ctr_len = 1 << 20; }
    return a;
}

struct Shape { int kind, B, H, W, N, C, var; };

static const char* kIgemmHeader = "mode,kind,B,H,W,N,C,var,sets,fcfg,fsplit,route,cfg,BM,BN,splitk,cps,wide,fin,ws,relu,tail,mroute,mcfg,mBM,mBN,msplitk,mcps,mwide,mws";
static void igemm_row(const char* mode, const Shape& s, int sets, int fcfg, int fsplit) {
    const mtd_conv_args a = args_of(s.kind, 0, s.B, s.H, s.W, s.N, s.C, s.var);
    const IgemmAns r = dump_igemm(a, 1, fcfg, fsplit), m = dump_igemm(a, sets, fcfg, fsplit);
    printf("%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%lld,%d,%d,%d,%d,%d,%d,%d,%d,%d,%lld\n", mode, s.kind, s.B, s.H, s.W, s.N, s.C, s.var, sets, fcfg,
           fsplit, r.route, r.cfg, r.BM, r.BN, r.splitk, r.cps, r.wide, r.fin, r.ws, r.relu, r.tail, m.route, m.cfg, m.BM, m.BN, m.splitk, m.cps, m.wide, m.ws);
}
static const char* kWinoHeader = "mode,kind,B,H,W,N,C,var,f4,wsplit,ok,px,nb,lean,splitk,cps,c32,g2,g3,xcd,ws";
static void wino_row(const char* mode, const Shape& s, int f4, int wsplit) {
    const WinoAns r = dump_wino(args_of(s.kind, 0, s.B, s.H, s.W, s.N, s.C, s.var), f4, wsplit);
    printf("%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%lld\n", mode, s.kind, s.B, s.H, s.W, s.N, s.C, s.var, f4, wsplit, r.ok, r.px, r.nb, r.lean,
           r.splitk, r.cps, r.c32, r.g2, r.g3, r.xcd, r.ws);
}
static const char* kS2Header = "mode,kind,B,H,W,N,C,var,sets,elig,groups,nb,lean,pays,splitk,ws";
static void s2_row(const char* mode, const Shape& s, int sets) {
    mtd_conv_args a[4];
    for (int i = 0; i < 4; ++i) a[i] = args_of(s.kind, i, s.B, s.H, s.W, s.N, s.C, s.var);      // (the classes of a data gradient; copies otherwise)
    const W32Ans r = dump_w32(a, sets);
    printf("%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%lld\n", mode, s.kind, s.B, s.H, s.W, s.N, s.C, s.var, sets, r.elig, r.groups, r.nb, r.lean, r.pays, r.splitk, r.ws);
}

// the axes of the grids: launch grids from 2 x 2 to 128 x 128, some not square, some with a width that is no multiple of 4; batches
// that bring the pixel counts across every threshold of make_plan (4096 ... 131072)
static const int kMaps[12][2] = {{2, 2}, {4, 4}, {6, 6}, {8, 8}, {16, 16}, {32, 32}, {64, 64}, {128, 128}, {8, 16}, {12, 32}, {64, 32}, {6, 10}};
static const int kChans[5] = {32, 64, 128, 256, 512};
static const int kBatches[6] = {1, 2, 4, 8, 16, 32};
// point i of kinds x maps x N x C x B x sets
static Shape grid_point(int i, int* sets) {
    const int b = i % 6, c = (i / 6) % 5, n = (i / 30) % 5, m = (i / 150) % 12, set = (i / 1800) % 4, kind = i / 7200;
    *sets = set + 1;
    return Shape{kind, kBatches[b], kMaps[m][0], kMaps[m][1], kChans[n], kChans[c], 0};
}
static const int kGridPoints = 5 * 4 * 12 * 5 * 5 * 6;

static void igemm_table(bool lab, bool dense) {
    if (lab) {
        setenv("MTD_IGEMM_PLAN", "2", 1);
        // round 2's tiles: 256 x 64 (cfg 2) on the large 3x3 grids, the two-block tap-block kernel (7) on the next smaller ones, and the
        // unsplit grids of exactly 256 workgroups (cfg 2, 7, and 6 while its K loop is short: C = 128, 256 but not 512)
        static const Shape L[8] = {{K3, 4, 64, 64, 256, 64, 0},  {K3, 4, 64, 64, 128, 128, 0}, {K3, 8, 64, 64, 64, 128, 0},  {K3T, 2, 64, 64, 256, 256, 0},
                                   {K3, 1, 64, 64, 256, 128, 0}, {K3, 1, 64, 64, 256, 256, 0}, {K3, 1, 64, 64, 256, 512, 0}, {K3, 16, 64, 64, 256, 64, 0}};
        for (const Shape& s : L) {
            igemm_row("L", s, 1, -1, -1);
            igemm_row("L", s, 2, -1, -1);
        }
        return;
    }
    puts(kIgemmHeader);
    // the default rule: every 131st point of the axes (131 is coprime to every extent, so each value of each axis meets many values
    // of the others); dense: every 7th
    for (int i = 0; i < kGridPoints; i += dense ? 7 : 131) {
        int sets;
        const Shape s = grid_point(i, &sets);
        igemm_row("D", s, sets, -1, -1);
    }
    // ... the layers that the rules of make_plan and the route name: down1 (4x4 / stride 2, 64 -> 64) at 65536 and 32768 pixels; the
    // four-class data gradients at 131072 x 64, 32768 x 128, 16384 x 256 and 8192 x 256; the generator-shaped layers on 64-pixel
    // rows (halo tiles) and on wider rows (persistent kernel); the tap-block kernel; 64 x 64 tiles
    static const Shape layers[12] = {{K4S2, 16, 64, 64, 64, 64, 0}, {K4S2, 8, 64, 64, 64, 64, 0},   {KDG, 8, 64, 64, 64, 128, 0},  {KDG, 8, 32, 32, 128, 256, 0},
                                     {KDG, 16, 16, 16, 256, 512, 0}, {KDG, 8, 16, 16, 256, 512, 0}, {K3, 8, 64, 64, 32, 32, 0},    {K3T, 2, 128, 128, 32, 32, 0},
                                     {K3, 1, 64, 64, 128, 128, 0},  {K3, 8, 64, 64, 64, 128, 0},    {K1, 16, 16, 16, 512, 512, 0}, {K3, 32, 64, 64, 64, 64, 0}};
    for (const Shape& s : layers)
        for (int sets = 1; sets <= 4; ++sets) igemm_row("D", s, sets, -1, -1);
    // ... every override: the tile kernels 0 .. 8, the persistent kernel 9, the halo-tile kernel 10, with forced slice counts
    static const int splits[4] = {-1, 1, 3, 1000};
    for (int l = 6; l < 10; ++l)
        for (int fcfg = -1; fcfg <= 10; ++fcfg)
            for (int fsplit : splits) igemm_row("D", layers[l], l == 9 ? 2 : 1, fcfg, fsplit);
    for (int fcfg = 0; fcfg <= 10; ++fcfg) igemm_row("D", layers[10], 4, fcfg, 3);
    // ... operands that decide `wide`, `fin`, the form of the split-K finish and the route: on a split layer and on the two
    // generator-shaped layers
    static const int vars[16] = {V_OUT4, V_WS4, V_BIAS4, V_MASK, V_MASK | V_MASK4, V_ADD1, V_OUT2, V_RELU_ADD, V_RELU_ADD | V_MASK, V_RELU_ADD | V_ADD1, V_CTR,
                                 V_CTR | V_WS4, V_LD2, V_OUT2 | V_MASK, V_CTR | V_LD2, V_OUT2 | V_RELU_ADD};
    static const int varied[3] = {6, 7, 10};
    for (int l : varied)
        for (int var : vars) {
            Shape s = layers[l];
            s.var = var;
            igemm_row("D", s, 1, -1, -1);
        }
}

static void wino_table(bool dense) {
    puts(kWinoHeader);
    // 3x3 forward and transposed (and a few 1x1 / 4x4 layers, which the kernel refuses) under both F(2x4) thresholds and both weight forms
    for (int i = 0; i < 3 * 12 * 5 * 5 * 6 * 4; i += dense ? 5 : 67) {
        const int b = i % 6, c = (i / 6) % 5, n = (i / 30) % 5, m = (i / 150) % 12, f = (i / 1800) % 4, kind = 1 + (i / 7200) % 3;
        wino_row("D", Shape{kind, kBatches[b], kMaps[m][0], kMaps[m][1], kChans[n], kChans[c], 0}, (f & 1) ? 8 : 0, f >> 1);
    }
    // the generator's 32 -> 32 layers: the persistent kernel with and without an add or a mask; operands it refuses (the general
    // kernel's 32-channel workgroups then, or nothing where a second output is asked for); maps that split K; 128-channel workgroups
    static const Shape layers[8] = {{K3, 1, 128, 128, 32, 32, 0}, {K3T, 2, 64, 64, 32, 32, 0}, {K3, 16, 4, 4, 512, 512, 0},  {K3, 32, 2, 2, 256, 128, 0},
                                    {K3, 8, 64, 64, 128, 64, 0},  {K3, 4, 6, 10, 128, 256, 0}, {K3T, 8, 32, 32, 64, 64, 0}, {K3, 2, 16, 16, 64, 128, 0}};
    static const int vars[12] = {0, V_ADD1, V_MASK, V_MASK | V_ADD1, V_MASK | V_OUT2, V_OUT2, V_OUT4, V_MASK | V_MASK4, V_RELU_ADD, V_RELU_ADD | V_MASK, V_WS4, V_LD2};
    for (const Shape& l : layers)
        for (int var : vars)
            for (int f = 0; f < 4; ++f) {
                if (var && l.N != 32 && (f != 1 || (var != V_WS4 && var != V_LD2 && var != V_RELU_ADD))) continue;
                Shape s = l;
                s.var = var;
                wino_row("D", s, (f & 1) ? 8 : 0, f >> 1);
            }
}

static void s2_table(bool dense) {
    puts(kS2Header);
    // 4x4 / stride-2 forward layers (one set) and the classes of their data gradients (1 .. 4 sets); the other kinds are refused
    for (int i = 0; i < kGridPoints; i += dense ? 7 : 41) {
        int sets;
        const Shape s = grid_point(i, &sets);
        if (s.kind < K3T) continue;
        s2_row("D", s, s.kind == KDG ? sets : 1);
    }
    // the discriminator's down1 .. down3 at 64 and 32 images, forward and data gradient
    static const Shape layers[6] = {{K4S2, 64, 32, 32, 64, 64, 0},  {K4S2, 64, 16, 16, 128, 64, 0},  {K4S2, 32, 16, 16, 128, 64, 0},
                                    {K4S2, 64, 8, 8, 256, 128, 0}, {K4S2, 32, 32, 32, 64, 64, V_RELU_ADD}, {K4S2, 32, 32, 32, 64, 64, V_OUT2}};
    for (const Shape& l : layers) {
        s2_row("D", l, 1);
        Shape d = l;      // the data gradient: N and C change places
        d.kind = KDG; d.N = l.C; d.C = l.N;
        for (int sets = 1; sets <= 4; ++sets) s2_row("D", d, sets);
    }
}

int main(int argc, char** argv) {
    const char* table = argc > 1 ? argv[1] : "";
    const bool lab = argc > 2 && !strcmp(argv[2], "lab"), dense = argc > 2 && !strcmp(argv[2], "dense");
    if (!strcmp(table, "names")) {
        for (int k = 0; k < kDumpKernelCount; ++k) printf("%d,%s\n", k, dump_kernel_name(k));
    } else if (!strcmp(table, "igemm")) {
        igemm_table(lab, dense);
    } else if (!strcmp(table, "wino") && !lab) {
        wino_table(dense);
    } else if (!strcmp(table, "s2") && !lab) {
        s2_table(dense);
    } else {
        fprintf(stderr, "usage: conv_plan_dump igemm [lab | dense] | wino [dense] | s2 [dense] | names\n");
        return 2;
    }
    return 0;
}
