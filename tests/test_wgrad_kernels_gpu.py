"""Every slab-producing weight-gradient kernel of the LDS-staged, row-window and block-window families and every slab reduce
(mtd-gan_amd/csrc/conv_wgrad.hip behind the planner conv_wgrad_plan.h), forced through mtd_conv_wgrad_override and compared with
float64 autograd (tests/_wgrad_ref.py; tests/test_wgrad_ref_cpu.py shows on the CPU what the bound can see).

  test                                    plans    kernels
  test_lds_staged_kernels                 0 .. 6   wgrad_kernel<1,1,9> <1,1,4> <2,2,1> <1,1,8> <1,1,3> <1,1,1> <2,2,3>, wgrad_finish_kernel
  test_row_window_kernels                 7, 8, 9  wgrad_row_kernel<3,3,1> <3,3,-1> <1,1,1>, wgrad_finish_kernel
  test_row_window_channel_slices          7        wgrad_row_kernel<3,3,1> on operands with p_ld > N, q_ld > C
  test_block_window_kernels               10 .. 12 wgrad_blk_kernel<8> <4> <2>, wgrad_finish_kernel
  test_pair_form_vs_float64               4, 11,   the pair form (WgradParams::pair_ns) of wgrad_kernel<1,1,3>, wgrad_blk_kernel<4>,
                                          13, 15   wgrad_taps_kernel, wgrad_s2_kernel; wgrad_finish_kernel with gridDim.y == 2
  test_half_scale_form_vs_float64         0, 12    mtd_wgrad_args.half_scale in wgrad_kernel<1,1,9>, wgrad_blk_kernel<2>
  test_reduce_routes                      7        wgrad_finish_kernel (<= 16 slabs), wgrad_reduce_finish_kernel<4> (17 .. 128),
                                                   wgrad_reduce_finish_kernel<8> (129 .. 1024)
  test_staged_reduce                      9        slab_group_sum_kernel (64 + 8 slabs), then wgrad_finish_kernel
  test_deferred_table                     4, 7,    wgrad_reduce_multi_kernel (kernels.DeferredWgrads, flush_wgrads)
                                          9, 11

Protocol of every launch (_run): operands from rnd(seed) in NHWC; dw and db filled with NaN (write mode) or a constant (accumulate);
the override set in try / finally; mtd_conv_wgrad_plan_cfg must name the forced plan, so a test of plan N fails if the planner routes
the layer elsewhere; the slab count comes from mtd_conv_wgrad_slabs (0: the kernel wrote dw itself) and is asserted where the case
aims at one; the gradient itself comes from kernels.wgrad.

The bound: rel(dw) and rel(db) against float64 below max(1e-5, 2 * rel(seq32, ref64)), seq32 the fp32 one-chain evaluation of the same
sums on the CPU -- never another GPU kernel.  The floor decides everywhere but on the layers of 16384 pixels and more.

The pixel split is ceil(M / (128 j)) slices of 128 j pixels (four waves of 32 j), so a forced count is a wish: test_reduce_routes'
layer of 20480 pixels answers 17 with 16 slabs and 128 or 129 with 80, and three more layers of exactly 17, 128 and 129 slices of
128 pixels stand on the limits of the routes."""
import ctypes as C

import pytest
import torch

import _wgrad_ref as R
from _metrics import rel

pytestmark = pytest.mark.gpu
FILL_DW, FILL_DB = 0.25, -0.5
NAN = float("nan")


def _geom(K, c):
    return K.geom_fwd(c.B, c.IH, c.IW, c.k, c.s, c.p) if c.kind == "conv" else K.geom_dgrad_s1(c.B, *R.out_hw(c), c.k, c.p)


def _view(c, view, fill, guard=0):
    """The gradient tensor of W(n, c, tap) as OIHW [N, C, k, k] or IOHW [C, N, k, k], its strides, and the buffer it lies in (with `guard`
    NaN elements on either side)."""
    T = c.k * c.k
    shape, sn, sc = ((c.N, c.C, c.k, c.k), c.C * T, T) if view == "oihw" else ((c.C, c.N, c.k, c.k), T, c.N * T)
    flat = torch.full((2 * guard + c.N * c.C * T,), NAN, device="cuda")
    dw = flat[guard:guard + c.N * c.C * T].view(shape)
    dw.fill_(fill)
    return dw, sn, sc, flat


def _as_view(c, view, dw_ref):
    """The reference (OIHW for a conv, IOHW for a transposed conv) in the layout of the view."""
    return dw_ref if view == ("oihw" if c.kind == "conv" else "iohw") else dw_ref.permute(1, 0, 2, 3)


def _max_split(c):
    return (R.pixels(c) + 127) // 128


def _run(c, p, q, cfg, split, view, accumulate=False, half=None):
    """One forced launch: (dw, db, slab count); dw in the view's layout, both as float64 on the CPU without the accumulate fill."""
    from mtd_gan_amd import _lib, kernels as K
    L = _lib.lib()
    geom = _geom(K, c)
    dw, sn, sc, _ = _view(c, view, 0.0)
    db = torch.zeros(c.N, device="cuda")
    bits = 3 if accumulate else 0
    L.mtd_conv_wgrad_override(cfg, split)
    try:
        a = K._wgrad_args(p, q, geom, c.N, c.C, dw, sn, sc, db, bits, half)
        assert L.mtd_conv_wgrad_plan_cfg(C.byref(a)) == cfg
        need = L.mtd_conv_wgrad_ws_bytes(C.byref(a))
        assert need > 0
        ws = K.workspace(need, p.device)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
        ns, stride = C.c_int(-1), C.c_longlong(0)
        _lib.check(L.mtd_conv_wgrad_slabs(C.byref(a), C.byref(ns), C.byref(stride), K.stream_ptr()), "mtd_conv_wgrad_slabs")
        assert stride.value == c.k * c.k * c.N * c.C + c.N
        dw.fill_(FILL_DW if accumulate else NAN)
        db.fill_(FILL_DB if accumulate else NAN)
        K.wgrad(p, q, geom, c.N, c.C, dw, sn, sc, db=db, accumulate=accumulate, accumulate_bias=accumulate, half=half)
        torch.cuda.synchronize()
    finally:
        L.mtd_conv_wgrad_override(-1, -1)
    dw64, db64 = dw.double().cpu(), db.double().cpu()
    if accumulate:
        dw64, db64 = dw64 - FILL_DW, db64 - FILL_DB
    return dw64, db64, ns.value


def _check(tag, dw, db, dw_ref, db_ref, bound_dw, bound_db):
    assert dw.shape == dw_ref.shape and db.shape == db_ref.shape
    e_dw, e_db = rel(dw, dw_ref), rel(db, db_ref)
    print(f"WGRAD {tag}: dw {e_dw:.3e} (bound {bound_dw:.2e}) db {e_db:.3e} (bound {bound_db:.2e})")
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), tag
    assert e_dw < bound_dw and e_db < bound_db, (tag, e_dw, bound_dw, e_db, bound_db)


def _forced(family, c, cfg, view, splits, p=None, q=None):
    """The case under plan cfg with every split of `splits` (-1: the plan's own): write mode, and for a forced single split also
    accumulate mode into the constant fill.  The slab count is asserted for the forced splits 1 and ceil(M / 128)."""
    ref = R.case_ref(c)
    if p is None:
        p, q = ref.gy.cuda(), ref.x.cuda()
    for split in splits:
        for accumulate in ((False, True) if split == 1 else (False,)):
            dw, db, ns = _run(c, p, q, cfg, split, view, accumulate)
            if split == 1:
                assert ns == 0
            elif split == _max_split(c):
                assert ns == split
            else:
                assert ns == 0 or 2 <= ns <= _max_split(c)
            _check(f"{family} {c.name} plan {cfg} split {split} slabs {ns} {view}{' accumulate' if accumulate else ''}",
                   dw, db, _as_view(c, view, ref.dw), ref.db, ref.bound_dw, ref.bound_db)


def _splits(c):
    return sorted({1, -1, _max_split(c)}, key=lambda s: (s < 0, s))


# ---- a. LDS-staged kernels: maps the register-operand kernels refuse
LDS_CASES = ([(R.A1[(32, 96)], cfg) for cfg in (0, 1, 3, 4, 5)] + [(R.A1[(64, 64)], cfg) for cfg in (2, 6)] +
             [(R.A2[(32, 96)], cfg) for cfg in (0, 1, 3, 4, 5)] + [(R.A2[(64, 64)], cfg) for cfg in (2, 6)] +
             [(R.A3[(32, 96)], cfg) for cfg in (1, 5)] + [(R.A3[(64, 64)], 2)] + [(R.A4, cfg) for cfg in (0, 4)])


@pytest.mark.parametrize("c,cfg", LDS_CASES, ids=lambda v: v.name if isinstance(v, R.Case) else f"plan{v}")
def test_lds_staged_kernels(hip_lib, c, cfg):
    """wgrad_kernel<WN, WC, TG>.  a1: 3x3 on 3 x 12 x 20 (720 pixels: the last 32-pixel chunk of a single split is half filled; tap
    groups 9, 4+4+1, 8+1, 3+3+3, nine of 1); a2: 4x4 / stride 2 on 12 x 20 -> 6 x 10 (180 pixels; tap groups 9+7, four of 4, 8+8, five
    of 3 plus 1, sixteen of 1); a3: 1x1 on 5 x 6 x 6; a4: the transposed tap order (geom_dgrad_s1) into the IOHW view on 3 x 12 x 12.
    Splits: 1 (direct write, also accumulating), the plan's, ceil(M / 128) (waves of one chunk, the last ones empty)."""
    _forced("lds", c, cfg, "iohw" if c.kind == "convT" else "oihw", _splits(c))


# ---- b. row-window kernels
ROW_CASES = ([(c, 7) for c in (*R.B_SQ.values(), *R.B_WIDE.values())] + [(c, 8) for c in (*R.B_SQ_T.values(), *R.B_WIDE_T.values())] +
             [(c, 9) for c in R.B_1X1.values()])


@pytest.mark.parametrize("c,cfg", ROW_CASES, ids=lambda v: v.name if isinstance(v, R.Case) else f"plan{v}")
def test_row_window_kernels(hip_lib, c, cfg):
    """wgrad_row_kernel<3, 3, 1> / <3, 3, -1> (into the IOHW view) / <1, 1, 1> with (N, C) = (32, 64) and (64, 64) -- the latter
    has to be forced, its default 3x3 plan is the Winograd kernel.  3 x 16 x 16: 768 pixels; 1 x 6 x 32: 192 pixels, where a single
    split gives the waves 64 pixels each and leaves the fourth empty, and the split of two has 32-pixel waves, two of them empty in
    its second slab."""
    _forced("row", c, cfg, "iohw" if c.kind == "convT" else "oihw", _splits(c))


def test_row_window_channel_slices(hip_lib):
    """Operands that are channel slices [..., 32:32 + N] of wider tensors (p_ld > N, q_ld > C) with one more image behind them,
    everything outside the slices NaN: a read beside the slice or past the last pixel (the buffer range ends with the last pixel's
    last channel) shows in the result."""
    c = R.B_WIDE[(32, 64)]
    ref = R.case_ref(c)
    oh, ow = R.out_hw(c)
    pw = torch.full((c.B + 1, oh, ow, c.N + 64), NAN, device="cuda")
    qw = torch.full((c.B + 1, c.IH, c.IW, c.C + 64), NAN, device="cuda")
    p, q = pw[:c.B, :, :, 32:32 + c.N], qw[:c.B, :, :, 32:32 + c.C]
    p.copy_(ref.gy)
    q.copy_(ref.x)
    _forced("row-slices", c, 7, "oihw", _splits(c), p, q)


# ---- c. block-window kernels
@pytest.mark.parametrize("c", list(R.C_BLK.values()), ids=lambda c: c.name)
def test_block_window_kernels(hip_lib, c):
    """wgrad_blk_kernel<8> / <4> / <2>, (N, C) = (64, 32): 3 x 8 x 8 (192 pixels), 5 x 4 x 4 (80: the third wave's chunk half filled),
    5 x 2 x 2 (20 pixels: the second 16-pixel half of the only chunk holds one image), 9 x 2 x 2 (36: a second chunk of four pixels)."""
    _forced("blk", c, {8: 10, 4: 11, 2: 12}[c.IW], "oihw", sorted({1, _max_split(c)}))


# ---- d. pair and half_scale forms, each half against float64 of that half
@pytest.mark.parametrize("c,cfg", [(R.D_PAIR_LDS, 4), (R.D_PAIR_BLK4, 11), (R.D_PAIR_TAPS, 13), (R.D_PAIR_S2, 15)], ids=lambda v: v.name if isinstance(v, R.Case) else f"plan{v}")
def test_pair_form_vs_float64(hip_lib, c, cfg):
    """kernels.wgrad_pair under mtd_conv_wgrad_pair_mode(3): both halves of the batch in ONE launch of the forced kernel (slabs
    0 .. ns - 1 the first half's), summed by one finish launch into two gradients; the bias gradient is the sum of both halves.
    a2 with four images on wgrad_kernel<1, 1, 3>; 6 x 4 x 4 on the block-window kernel; plans 13 and 15 on the smallest shapes of
    test_kernels_gpu.test_all_taps_weight_gradient_forced that have an even batch (2 x 512 -> 512 on 4 x 4, 2 x 128 -> 64 on 16 x 16)."""
    from mtd_gan_amd import _lib, kernels as K
    L = _lib.lib()
    Bh = c.B // 2
    x, gy = R.operands(c)
    h1, h2 = R.half_ref(c, 0, Bh), R.half_ref(c, Bh, c.B)
    p, q = gy.cuda(), x.cuda()
    geom = _geom(K, c)
    d1, sn, sc, _ = _view(c, "oihw", NAN)
    d2 = torch.full_like(d1, NAN)
    db = torch.full((c.N,), NAN, device="cuda")
    L.mtd_conv_wgrad_pair_mode(3)
    L.mtd_conv_wgrad_override(cfg, -1)
    try:
        a = K._wgrad_args(p, q, geom, c.N, c.C, d1, sn, sc, db, 0)
        assert L.mtd_conv_wgrad_pair_ok(C.byref(a), Bh) == 1
        ah = K._wgrad_args(p[:Bh], q[:Bh], K.mtd_geom_with_batch(geom, Bh), c.N, c.C, d1, sn, sc, db, 0)
        assert L.mtd_conv_wgrad_plan_cfg(C.byref(ah)) == cfg             # the pair launch runs the plan of one half
        # (no slab query for pair launches: the workspace says one slab per half, so the sum is wgrad_finish_kernel with two rows)
        assert L.mtd_conv_wgrad_pair_ws_bytes(C.byref(a), Bh) == 4 * 2 * (c.k * c.k * c.N * c.C + c.N)
        K.wgrad_pair(p, q, geom, Bh, c.N, c.C, d1, d2, sn, sc, db=db, accumulate_bias=False)
        torch.cuda.synchronize()
    finally:
        L.mtd_conv_wgrad_override(-1, -1)
        L.mtd_conv_wgrad_pair_mode(-1)
    _check(f"pair {c.name} plan {cfg} first half", d1.double().cpu(), db.double().cpu(), h1.dw, h1.db + h2.db, h1.bound_dw, max(h1.bound_db, h2.bound_db))
    _check(f"pair {c.name} plan {cfg} second half", d2.double().cpu(), db.double().cpu(), h2.dw, h1.db + h2.db, h2.bound_dw, max(h1.bound_db, h2.bound_db))


@pytest.mark.parametrize("c,cfg,b_first", [(R.A1[(32, 96)], 0, 2), (R.D_HALF_BLK2, 12, 8)], ids=lambda v: v.name if isinstance(v, R.Case) else str(v))
def test_half_scale_form_vs_float64(hip_lib, c, cfg, b_first):
    """kernels.wgrad(half=(s1, s2, m_first)): the cotangent of pixels [0, m_first) times s1, the rest times s2, as the kernel uses it.
    dw against s1 ref64(first images) + s2 ref64(the rest), db against the unscaled sum.  m_first = 480 (a1) and 32 (2 x 2 maps): whole
    images and a multiple of 32."""
    ref, h1, h2 = R.case_ref(c), R.half_ref(c, 0, b_first), R.half_ref(c, b_first, c.B)
    oh, ow = R.out_hw(c)
    m_first = b_first * oh * ow
    assert m_first % 32 == 0
    s1, s2 = torch.tensor([1.7], device="cuda"), torch.tensor([0.45], device="cuda")
    want = s1.item() * h1.dw + s2.item() * h2.dw
    for split in _splits(c):
        dw, db, ns = _run(c, ref.gy.cuda(), ref.x.cuda(), cfg, split, "oihw", half=(s1, s2, m_first))
        _check(f"half_scale {c.name} plan {cfg} split {split} slabs {ns}", dw, db, want, ref.db, ref.bound_dw, ref.bound_db)


# ---- e. reduce routes
FINISH, RF4, RF8 = (1, 16), (16, 128), (128, 1024)          # (lo, hi]: slab counts of wgrad_finish_kernel, wgrad_reduce_finish_kernel<4>, <8>
ROUTES = [(R.E_LAYER, 2, 2, FINISH), (R.E_LAYER, 16, 16, FINISH), (R.E_LAYER, 17, 16, FINISH), (R.E_LAYER, 128, 80, RF4), (R.E_LAYER, 129, 80, RF4),
          (R.E_LAYER, 160, 160, RF8), (R.E_17, 17, 17, RF4), (R.E_128, 128, 128, RF4), (R.E_129, 129, 129, RF8)]


def _reduce_case(family, c, cfg, split, slabs):
    ref = R.case_ref(c)
    p, q = ref.gy.cuda(), ref.x.cuda()
    for view, accumulate in (("oihw", False), ("iohw", True)):
        dw, db, ns = _run(c, p, q, cfg, split, view, accumulate)
        assert ns == slabs
        _check(f"{family} {c.name} plan {cfg} split {split} slabs {ns} {view}{' accumulate' if accumulate else ''}",
               dw, db, _as_view(c, view, ref.dw), ref.db, ref.bound_dw, ref.bound_db)


@pytest.mark.parametrize("c,split,slabs,route", ROUTES, ids=lambda v: v.name if isinstance(v, R.Case) else str(v))
def test_reduce_routes(hip_lib, c, split, slabs, route):
    """3x3, 32 -> 32 on the row-window kernel (forced: the default plan is the Winograd kernel).  5 x 64 x 64 (20480 pixels) under the
    forced splits 2, 16, 17, 128, 129, 160: its slab counts are ceil(20480 / (128 j)), so they come out as 2, 16, 16, 80, 80, 160 --
    wgrad_finish_kernel, wgrad_reduce_finish_kernel<4> and <8> (160: a ragged count for the 8 x 8 run layout).  The limits of the routes
    need layers of their own: 34 x 64 (17 slabs, the first count of <4>), 4 x 64 x 64 (128, its last), 3 x 86 x 64 (129, the first of <8>).
    Each once into the OIHW view with the bias gradient and once accumulating into the IOHW view."""
    assert route[0] < slabs <= route[1] and (c.k * c.k * c.N * c.C + c.N) // 4 <= 16 * 4096
    _reduce_case("reduce", c, 7, split, slabs)


def test_staged_reduce(hip_lib):
    """1x1, 512 -> 512 on 9 x 32 x 32 under the forced split 72: 72 slabs of 65664 float4 units each -- more than 64 slabs and more than
    16 * 4096 units, so two slab_group_sum_kernel groups (64 + 8 slabs) and wgrad_finish_kernel over their two sums.  No default
    plan of the training step comes here."""
    c = R.E_STAGED
    assert (c.N * c.C + c.N) // 4 > 16 * 4096
    _reduce_case("staged", c, 9, 72, 72)


# ---- f. deferred table
def test_deferred_table(hip_lib):
    """Four layers of different taps, channels and slab counts in one kernels.DeferredWgrads, summed by ONE flush_wgrads
    (wgrad_reduce_multi_kernel): a1 on plan 4 (6 slabs), the 20480-pixel layer at the forced split 17 (16 slabs; IOHW, accumulating),
    5 x 4 x 4 on the block-window kernel (its largest split is 1: the kernel writes the gradient itself and the table gets no entry),
    1x1 on 3 x 16 x 16 (6 slabs; IOHW).  NaN guards directly before and after every dw must survive."""
    from mtd_gan_amd import _lib, kernels as K
    L = _lib.lib()
    assert K.DEFER_WGRADS
    layers = [(R.A1[(32, 96)], 4, -1, "oihw", False, 6), (R.E_LAYER, 7, 17, "iohw", True, 16), (R.C_BLK[(4, 5)], 11, 1, "oihw", False, 0),
              (R.B_1X1[(32, 64)], 9, -1, "iohw", False, 6)]
    defer = K.DeferredWgrads()
    out, slabs = [], []
    for c, cfg, split, view, accumulate, _ in layers:
        ref = R.case_ref(c)
        p, q = ref.gy.cuda(), ref.x.cuda()
        dw, sn, sc, flat = _view(c, view, FILL_DW if accumulate else NAN, guard=64)
        db = torch.full((c.N,), FILL_DB if accumulate else NAN, device="cuda")
        geom = _geom(K, c)
        L.mtd_conv_wgrad_override(cfg, split)
        try:
            assert L.mtd_conv_wgrad_plan_cfg(C.byref(K._wgrad_args(p, q, geom, c.N, c.C, dw, sn, sc, db, 3 if accumulate else 0))) == cfg
            before = len(defer.conv)
            K.wgrad(p, q, geom, c.N, c.C, dw, sn, sc, db=db, accumulate=accumulate, accumulate_bias=accumulate, defer=defer)
            slabs.append(defer.conv[-1].nslab if len(defer.conv) > before else 0)
        finally:
            L.mtd_conv_wgrad_override(-1, -1)
        out.append((dw, db, flat, p, q))
    assert slabs == [l[5] for l in layers]
    K.flush_wgrads(defer)
    torch.cuda.synchronize()
    for (c, cfg, split, view, accumulate, ns), (dw, db, flat, _, _) in zip(layers, out):
        ref = R.case_ref(c)
        dw64, db64 = dw.double().cpu(), db.double().cpu()
        if accumulate:
            dw64, db64 = dw64 - FILL_DW, db64 - FILL_DB
        _check(f"deferred {c.name} plan {cfg} split {split} slabs {ns} {view}{' accumulate' if accumulate else ''}",
               dw64, db64, _as_view(c, view, ref.dw), ref.db, ref.bound_dw, ref.bound_db)
        assert bool(torch.isnan(flat[:64]).all()) and bool(torch.isnan(flat[-64:]).all()), c.name
