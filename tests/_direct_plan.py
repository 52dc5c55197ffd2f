"""The branch choice of csrc/conv_direct.hip restated in plain Python: which of its seven kernels a launch of mtd_conv_direct
(conv_plan) or of mtd_conv_wgrad with min(N, C) == 1 (wgrad_plan) runs, and the launch numbers the host derives on the way.

The library has no hook that says which direct kernel ran, so tests/test_direct_conv_gpu.py reaches the kernels' branches by shape,
leading dimension and alignment alone and relies on these restatements to land where its case table claims;
tests/test_direct_conv_plan_cpu.py proves the table from them.  Both functions follow the C++ statement by statement -- the line
ranges of csrc/conv_direct.hip are cited beside each part -- and have to follow it when it changes.  The shipped library is built
without MTD_LAB, so every mtd_lab_env() switch of the planners has its default (MTD_C1_TILE 1, MTD_C1_WGS 512, MTD_N1_PLANES 1,
MTD_N1_R 8, MTD_WIDE_WGS 512).

A geometry is anything with the fields of mtd_geom (mtd_gan_amd._lib.Geom)."""

EINVAL, EALIGN = -1, -2                                # MTD_EINVAL, MTD_EALIGN (include/mtdgan_hip.h)
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_RELU_ADD = 0, 1, 2, 3
GENERIC_MAX_BLOCKS = 8192                              # one pass of direct_fwd_kernel: 8192 workgroups of 256 (n, pixel) pairs
WGRAD_GS = 64                                          # conv_wgrad.hip: slabs summed per reduce stage


def is_pow2(v):                                        # conv_direct.hip:682
    return v > 0 and (v & (v - 1)) == 0


def _ceil(a, b):
    return -(-a // b)


def identity(g):                                       # conv_direct.hip:744
    return g.out_sy == 1 and g.out_sx == 1 and g.out_oy == 0 and g.out_ox == 0 and g.OHF == g.OH and g.OWF == g.OW


def _taps(g):
    """(tap_dy, tap_dx) of every tap in launch order (conv_direct.hip:757-762, 717-719)."""
    return [((t // g.TW) * g.tap_dy, (t % g.TW) * g.tap_dx) for t in range(g.TH * g.TW)]


def _near_unique(g):
    """Every tap within one pixel of the output position, no neighbourhood position twice (conv_direct.hip:772-777, 805-810)."""
    seen = set()
    for dy, dx in _taps(g):
        dy, dx = g.off_y + dy, g.off_x + dx
        if dy < -1 or dy > 1 or dx < -1 or dx > 1 or (dy, dx) in seen:
            return False
        seen.add((dy, dx))
    return True


def _same_size_stride1(g):
    return g.in_sy == 1 and g.in_sx == 1 and g.OH == g.IH and g.OW == g.IW


def conv_plan(g, N, C, in_ld, out_ld, in_aligned=True, out_aligned=True, act=ACT_NONE, add1=False, add2=False, mask=False,
              scale2=False, scale_split=0, out2=False, w_sc=1):
    """mtd_conv_direct (conv_direct.hip:736-848).  in_aligned / out_aligned: is the operand's base 16-byte aligned.  Returns a dict:
    refusal (an error code, nothing else is filled then) or label and the launch numbers of that kernel."""
    # ---- 737-742: refusals before any launch
    if out2 or act == ACT_RELU_ADD:
        return dict(refusal=EINVAL)
    if C <= 0 or N <= 0 or g.B <= 0 or g.TH <= 0 or g.TW <= 0:
        return dict(refusal=EINVAL)
    if in_ld < C or out_ld < N:
        return dict(refusal=EINVAL)
    if (C & 3) == 0 and ((in_ld & 3) or not in_aligned):
        return dict(refusal=EALIGN)
    if (g.OH - 1) * g.out_sy + g.out_oy >= g.OHF or (g.OW - 1) * g.out_sx + g.out_ox >= g.OWF:
        return dict(refusal=EINVAL)
    # ---- 743-749
    Mpix = g.B * g.OH * g.OW
    total = Mpix * N
    ident = identity(g)
    T = g.TH * g.TW
    if not scale2:
        scale_split = 0                                # (kernels._conv_args)
    fast_c1 = C == 1 and N % 4 == 0 and is_pow2(N // 4) and N // 4 <= 256 and T <= 16 and Mpix < 2 ** 31
    fast_n1 = (N == 1 and C % 4 == 0 and is_pow2(C // 4) and C // 4 <= 64 and T <= 16 and Mpix < 2 ** 31
               and in_ld % 4 == 0 and in_aligned)
    plan = dict(refusal=None, M=Mpix, T=T, identity=ident)
    vec_store = out_ld % 4 == 0 and out_aligned        # 756
    if fast_c1:
        # ---- 763-798: fwd_c1_tile_kernel or fwd_c1_kernel
        G = N // 4
        PL = 256 // G
        ppb = max(_ceil(Mpix, 2048), PL)
        nblk = _ceil(Mpix, ppb)
        near = _same_size_stride1(g) and ident and T <= 9 and _near_unique(g)         # 771-777
        R = R_first = 0
        if near and g.OW % PL == 0 and (not scale2 or scale_split % (g.OH * g.OW) == 0):          # 780
            R_first = R = max(_ceil(Mpix, 512) // g.OW, 1)                            # 784-785
            while R > 1 and g.OH % R:                                                 # 786
                R -= 1
            if R < 1 or (R + 2) * (g.OW + 2) * 4 > 48 * 1024:                         # 787
                R = 0
        plan.update(G=G, PL=PL, vec_store=vec_store)
        if R > 0:                                                                     # 789-796
            plain = not add1 and not add2 and not mask and vec_store
            if plain and act in (ACT_LRELU, ACT_RELU, ACT_NONE):
                label = "c1_tile_plain_" + {ACT_LRELU: "lrelu", ACT_RELU: "relu", ACT_NONE: "none"}[act]
            else:
                label = "c1_tile_general"
            plan.update(label=label, R=R, R_first=R_first, nblk=g.B * g.OH // R, lds=(R + 2) * (g.OW + 2) * 4)
        else:
            plan.update(label="c1", ppb=ppb, nblk=nblk)                               # 798
        return plan
    if fast_n1:
        # ---- 799-813: fwd_n1_planes_kernel takes 3x3 "same" layers on 64-pixel rows, C = 32 / 64 / 128
        planes = (C in (32, 64, 128) and T <= 9 and ident and _same_size_stride1(g) and g.OW == 64 and g.OH % 8 == 0
                  and w_sc > 0 and not (scale2 and scale_split % (g.OH * g.OW)) and _near_unique(g)
                  and ((g.B * g.IH * g.IW - 1) * in_ld + C) * 4 < 2 ** 31)
        if planes:                                                                    # 814-830
            R = 8
            plan.update(label=f"n1_planes_{C // 32}", R=R, nblk=g.B * g.OH // R, lds=9 * (R + 2) * 66 * 4,
                        in_bytes=((g.B * g.IH * g.IW - 1) * in_ld + C) * 4)
        else:                                                                         # 831-838
            G = C // 4
            PPW = 64 // G
            ppb = max(_ceil(Mpix, 2048), 4 * PPW)
            plan.update(label="n1", G=G, PPW=PPW, ppb=ppb, nblk=_ceil(Mpix, ppb))
        return plan
    # ---- 843-845: direct_fwd_kernel, one thread per (pixel, n), grid-stride past 8192 workgroups
    blocks = min(_ceil(total, 256), GENERIC_MAX_BLOCKS)
    plan.update(label="generic", total=total, nblk=blocks, passes=_ceil(total, 256 * blocks), vec_loads=(C & 3) == 0)
    return plan


def _wide_plan(g, N, C, p_ld, q_ld, wide_aligned):
    """wide_plan (conv_direct.hip:685-732): None where the fast weight-gradient path does not apply."""
    T = g.TH * g.TW
    n_is_one = N == 1
    V = max(N, C)
    if T > 16:                                                                        # 691
        return None
    if n_is_one:                                                                      # 692-697
        if not _same_size_stride1(g):
            return None
        Mw = g.B * g.IH * g.IW
    else:
        Mw = g.B * g.OH * g.OW
    if V == 1:                                                                        # 698-706
        CL = 1
    else:
        if V % 4:
            return None
        CL = V // 4
        if not is_pow2(CL) or CL > 64:
            return None
        ld = q_ld if n_is_one else p_ld
        if ld % 4 or not wide_aligned:
            return None
    if (T * V + V) * 4 * 4 > 48 * 1024:                                               # 707
        return None
    PPW = 64 // CL
    ppb = max(_ceil(Mw, 512), 4 * PPW * 4)                                            # 711-715
    near = True                                                                       # 716-724
    for dy, dx in _taps(g):
        ddy = -(g.off_y + dy) if n_is_one else g.off_y + dy
        ddx = -(g.off_x + dx) if n_is_one else g.off_x + dx
        near = near and -1 <= ddy <= 1 and -1 <= ddx <= 1
    GW, GH = (g.IW, g.IH) if n_is_one else (g.OW, g.OH)                               # 726-730
    tile_rows = 0
    if (near and _same_size_stride1(g) and GW > 0 and ppb % GW == 0 and GH % (ppb // GW) == 0
            and (ppb // GW + 2) * (GW + 2) * 4 <= 16 * 1024):
        tile_rows = ppb // GW
    return dict(T=T, V=V, Mw=Mw, CL=CL, PPW=PPW, ppb=ppb, tile_rows=tile_rows, GW=GW, GH=GH, n_is_one=n_is_one)


def wgrad_plan(g, N, C, p_ld, q_ld, wide_aligned=True):
    """mtd_conv_wgrad with min(N, C) == 1: check_wargs (conv_wgrad_plan.h), then mtd_direct_wgrad_launch
    (conv_direct.hip:917-957).  wide_aligned: is the base of the V-channel operand (q when N == 1, else p) 16-byte aligned."""
    assert N == 1 or C == 1
    T = g.TH * g.TW
    if N <= 0 or C <= 0 or g.B <= 0 or g.TH <= 0 or g.TW <= 0 or T > 16 or p_ld < N or q_ld < C:
        return dict(refusal=EINVAL)
    wp = _wide_plan(g, N, C, p_ld, q_ld, wide_aligned)
    if wp is not None:                                                                # 918-930: wgrad_wide_kernel<1 | 4>
        nblk = _ceil(wp["Mw"], wp["ppb"])
        step = 4 * wp["PPW"]
        if wp["tile_rows"] > 0:
            fast = T == 9 and step <= wp["GW"]                                        # 537
            label = "wide_tile_fast" if fast else "wide_tile_general"
        else:
            label = "wide_gather"
        wp.update(refusal=None, label=label, nblk=nblk, VEC=1 if wp["V"] == 1 else 4, step=step,
                  ragged=wp["Mw"] % wp["ppb"], slab_stride=T * N * C + N)
        return wp
    # ---- 932-956: direct_wgrad_kernel<1 | 2 | 8>
    M = g.B * g.OH * g.OW
    V = max(N, C)
    if V > 2048:                                                                      # 937
        return dict(refusal=EINVAL)
    VL = 1
    while VL < V and VL < 256:                                                        # 938-939
        VL <<= 1
    PL = 256 // VL
    CH = _ceil(V, VL)
    ppb = max(_ceil(M, 1024), PL * 8)                                                 # 944-946
    nblk = _ceil(M, ppb)
    inst = 1 if CH <= 1 else 2 if CH <= 2 else 8                                      # 951-954 (CH <= 8 by V <= 2048)
    return dict(refusal=None, label=f"dwgrad_{inst}", T=T, V=V, M=M, VL=VL, PL=PL, CH=CH, ppb=ppb, nblk=nblk, ragged=M % ppb,
                n_is_one=N == 1, slab_stride=T * N * C + N)


def wgrad_ws_floats(plan):
    """wgrad_ws_floats (conv_wgrad_plan.h) for a plan of wgrad_plan: the slabs and every intermediate reduce stage."""
    ns, stride = plan["nblk"], plan["slab_stride"]
    total = ns * stride
    while ns > WGRAD_GS:
        ns = _ceil(ns, WGRAD_GS)
        total += ns * stride
    return total
