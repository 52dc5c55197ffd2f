"""The vector-ALU convolution kernels of csrc/conv_direct.hip (the layers with one channel on one side: the first and last layer
of both networks, conv11, the *_dconv61/62 pixel heads, Linear 512 -> 1) branch by branch against float64 on the CPU, through
kernels.conv / kernels.wgrad as the models call them: direct_fwd_kernel, fwd_c1_kernel, fwd_c1_tile_kernel (its three PLAIN forms
and the general epilogue), fwd_n1_kernel, fwd_n1_planes_kernel<1 | 2 | 4>, wgrad_wide_kernel<1 | 4> (fast tile, general tile and
gather form) and direct_wgrad_kernel<1 | 2 | 8>.

The library does not say which direct kernel ran.  Every case below declares the kernel it is there for (`label`), and
tests/_direct_plan.py -- the planners restated -- says where its shapes, leading dimensions and alignments land;
tests/test_direct_conv_plan_cpu.py proves label by label and edge by edge that the table covers what its comments claim.  Each item
here feeds the argument struct of the launch it made (kernels.CALL_LOG) to the same restatement and fails if the label drifted.

Reference: F.conv2d / F.conv_transpose2d / autograd in float64, the epilogue act(scale conv + bias + add1 + add2) (mask > 0 ? 1 :
slope) restated in float64.  Operands are channel slices of wider tensors filled with NaN (pixel stride a multiple of 4 and larger
than the channel count unless the case is about something else); outputs are NaN beforehand, have guard channels on both sides
and a guard image behind the batch, and the guards keep their bits.  A weight-gradient case runs once into NaN (overwrite) and twice
with accumulate=True into a pre-filled dw / db: the same bits both times (the kernels sum in a fixed order).

Bound: _metrics.rel < max(1e-5, 4 e_ref), e_ref the error of torch's fp32 CPU result of the same operation against the same
float64 reference (the factor 4: another legitimate fp32 summation order, nothing more).  Measured values: DESIGN 3.5.

Not here: the binary16-storage instances (tests/test_half_storage_gpu.py holds them to one rounding of the fp32 launches tested
here)."""
import pytest
import torch
import torch.nn.functional as F

import _direct_plan as plan
from _metrics import rel
from _spectral_stages import SPARE_BITS, _bits, _randn, _same_bits

pytestmark = pytest.mark.gpu

BOUND = 1e-5
ACTS = {"none": plan.ACT_NONE, "relu": plan.ACT_RELU, "lrelu": plan.ACT_LRELU}
SCALE, SCALE2 = 0.7, 1.3

FWD3 = ("fwd", 3, 1, 1)          # (kind, k, stride, padding): y = conv2d(x); H, W: the input map
FWD1 = ("fwd", 1, 1, 0)
FWD4S2 = ("fwd", 4, 2, 1)
DG3 = ("dgrad_s1", 3, 1)         # (kind, k, padding): dx = conv_transpose2d(g) of a stride-1 layer, reversed tap order; H, W: dx
DGS2 = ("dgrad_s2",)             # dx of a 4x4 stride-2 layer: four launches, one per parity, into one map; H, W: dx
TCONV3 = ("tconv", 3, 1)         # (weight gradients only) a stride-1 ConvTranspose2d layer: weights [C][N][k][k]


def _conv(id, label, kind, B, C, N, H, W, act="none", add1=False, add2=False, mask=False, slope=0.2, split=None, bias=True,
          out_ld=None, out_off=4):
    """A launch of C -> N channels.  split: the launch pixel from which scale2 holds (a paired pass); out_ld / out_off: pixel stride and
    first channel of the output slice (default: N rounded up to 4, plus 8; 4)."""
    return dict(id=id, label=label, kind=kind, B=B, C=C, N=N, H=H, W=W, act=act, add1=add1, add2=add2, mask=mask, slope=slope,
                split=split, bias=bias, out_ld=out_ld, out_off=out_off)


FULL = dict(add1=True, add2=True, mask=True)

CONV_CASES = [
    # ---- fwd_c1_tile_kernel: 1 -> N on whole rows, 3x3 neighbourhood, width a multiple of PL = 256 / (N / 4)
    _conv("c1t_lrelu", "c1_tile_plain_lrelu", FWD3, 2, 1, 32, 32, 32, act="lrelu"),             # PL = 32, R = 1
    _conv("c1t_relu", "c1_tile_plain_relu", FWD3, 2, 1, 32, 32, 32, act="relu"),
    _conv("c1t_none", "c1_tile_plain_none", FWD3, 2, 1, 32, 32, 32),
    _conv("c1t_g1", "c1_tile_plain_none", FWD3, 1, 1, 4, 4, 256),                               # G = 1: one thread per pixel
    _conv("c1t_pl1", "c1_tile_plain_lrelu", FWD3, 1, 1, 1024, 8, 8, act="lrelu"),               # PL = 1: all threads on one pixel
    _conv("c1t_r2", "c1_tile_plain_lrelu", FWD3, 16, 1, 128, 64, 8, act="lrelu"),               # R = 2
    _conv("c1t_r3to2", "c1_tile_plain_lrelu", FWD3, 24, 1, 128, 64, 8, act="lrelu"),            # R = 3 does not divide 64: 2
    _conv("c1t_r3to1", "c1_tile_plain_relu", FWD3, 44, 1, 128, 35, 8, act="relu"),              # height 35: R 3 -> 2 -> 1
    _conv("c1t_full", "c1_tile_general", FWD3, 2, 1, 32, 32, 32, act="lrelu", **FULL),
    _conv("c1t_scalar", "c1_tile_general", FWD3, 2, 1, 32, 32, 32, act="relu", add1=True, out_ld=41, out_off=5),   # scalar stores
    _conv("c1t_pair", "c1_tile_plain_lrelu", FWD3, 2, 1, 32, 32, 32, act="lrelu", split=1024),  # scale2 from image 1 on
    _conv("c1t_dgrad", "c1_tile_plain_none", DG3, 2, 1, 32, 32, 32),                            # reversed tap order
    _conv("c1t_dgrad_mask", "c1_tile_general", DG3, 2, 1, 32, 32, 32, mask=True, slope=0.0, bias=False),
    _conv("c1t_1x1", "c1_tile_plain_none", FWD1, 2, 1, 32, 32, 32),                             # T = 1: eight zero weights
    # ---- fwd_c1_kernel: every other 1 -> N layer with N / 4 a power of two
    _conv("c1_w20", "c1", FWD3, 2, 1, 32, 20, 20, act="lrelu"),                                 # width no multiple of PL
    _conv("c1_k4s2", "c1", FWD4S2, 2, 1, 64, 16, 16, act="lrelu"),                              # T = 16
    _conv("c1_pair_mid", "c1", FWD3, 2, 1, 32, 32, 32, act="lrelu", split=1500),                # the split inside image 1
    _conv("c1_big", "c1", FWD3, 3, 1, 256, 53, 53, act="relu"),                                 # M > 2048 PL, M % ppb != 0
    _conv("c1_dgrad_s2", "c1", DGS2, 2, 1, 32, 16, 16),                                         # four parities into one map
    _conv("c1_full", "c1", FWD3, 2, 1, 32, 20, 20, act="lrelu", out_ld=41, out_off=5, **FULL),
    # ---- fwd_n1_kernel: C -> 1, C / 4 = G lanes per pixel
    _conv("n1_g1", "n1", FWD3, 2, 4, 1, 9, 7, act="lrelu"),
    _conv("n1_g2", "n1", FWD3, 2, 8, 1, 9, 7, act="lrelu"),
    _conv("n1_g8", "n1", FWD3, 2, 32, 1, 9, 7, act="lrelu"),
    _conv("n1_g64", "n1", FWD3, 2, 256, 1, 9, 7, act="lrelu"),
    _conv("n1_nblk9", "n1", FWD3, 2, 32, 1, 11, 13),                                            # nblk % 8 == 1
    _conv("n1_nblk23", "n1", FWD3, 7, 32, 1, 15, 7),                                            # nblk % 8 == 7
    _conv("n1_k4s2", "n1", FWD4S2, 2, 64, 1, 16, 16),
    _conv("n1_full", "n1", FWD3, 2, 32, 1, 9, 7, act="lrelu", split=70, **FULL),                # the split inside image 1
    _conv("n1_dgrad_s2", "n1", DGS2, 2, 32, 1, 16, 16),
    _conv("n1_h12", "n1", FWD3, 1, 32, 1, 12, 64),                                              # height no multiple of 8: not the planes
    # ---- fwd_n1_planes_kernel<C / 32>: C -> 1 on 64-pixel rows, eight rows per workgroup
    _conv("pl_32_one", "n1_planes_1", FWD3, 1, 32, 1, 8, 64),                                   # one workgroup: both halos are borders
    _conv("pl_64_one", "n1_planes_2", FWD3, 1, 64, 1, 8, 64),
    _conv("pl_128_one", "n1_planes_4", FWD3, 1, 128, 1, 8, 64),
    _conv("pl_32", "n1_planes_1", FWD3, 3, 32, 1, 16, 64),                                      # interior halos, image boundaries
    _conv("pl_64", "n1_planes_2", FWD3, 3, 64, 1, 16, 64),
    _conv("pl_128", "n1_planes_4", FWD3, 3, 128, 1, 16, 64),
    _conv("pl_dgrad", "n1_planes_2", DG3, 2, 64, 1, 16, 64),
    _conv("pl_1x1", "n1_planes_1", FWD1, 2, 32, 1, 16, 64),
    _conv("pl_full", "n1_planes_4", FWD3, 3, 128, 1, 16, 64, act="relu", split=1024, **FULL),
    # ---- direct_fwd_kernel: everything else
    _conv("g_1to1", "generic", FWD3, 2, 1, 1, 16, 16, act="lrelu"),
    _conv("g_3to1", "generic", FWD3, 2, 3, 1, 9, 7),                                            # the scalar channel loop
    _conv("g_1to3", "generic", FWD3, 2, 1, 3, 9, 7),
    _conv("g_96to1", "generic", FWD3, 2, 96, 1, 9, 7),                                          # C / 4 no power of two
    _conv("g_1to96", "generic", FWD3, 2, 1, 96, 9, 7),
    _conv("g_linear", "generic", FWD1, 5, 512, 1, 1, 1),                                        # Linear 512 -> 1
    _conv("g_two_passes", "generic", FWD3, 2, 1, 96, 128, 128, act="lrelu"),                    # 3.1 M outputs: a second grid pass
    _conv("g_full", "generic", FWD3, 2, 1, 3, 9, 7, act="lrelu", split=70, **FULL),
    _conv("g_dgrad_s2", "generic", DGS2, 2, 3, 1, 16, 16),
]


def _wg(id, label, kind, B, C, N, H, W, db=True, wide_off=4):
    """The weight gradient of a C -> N layer on an H x W input map.  wide_off: first channel of the many-channel operand in its tensor."""
    return dict(id=id, label=label, kind=kind, B=B, C=C, N=N, H=H, W=W, db=db, wide_off=wide_off)


WGRAD_CASES = [
    # ---- wgrad_wide_kernel, tile form with constant offsets and four loads in flight
    _wg("wf_4_c1", "wide_tile_fast", FWD3, 1, 1, 4, 4, 256),
    _wg("wf_4_n1", "wide_tile_fast", FWD3, 1, 4, 1, 4, 256),
    _wg("wf_32_c1", "wide_tile_fast", FWD3, 2, 1, 32, 32, 32),
    _wg("wf_32_n1", "wide_tile_fast", FWD3, 2, 32, 1, 32, 32),
    _wg("wf_128_c1", "wide_tile_fast", FWD3, 64, 1, 128, 40, 8),                                # five steps per lane: 4 + 1
    _wg("wf_128_n1", "wide_tile_fast", FWD3, 64, 128, 1, 40, 8),
    _wg("wf_256_c1", "wide_tile_fast", FWD3, 2, 1, 256, 16, 16),
    _wg("wf_256_n1", "wide_tile_fast", FWD3, 2, 256, 1, 16, 16, db=False),
    _wg("wf_tconv", "wide_tile_fast", TCONV3, 2, 32, 1, 32, 32),                                # the generator's decoder.0
    # ---- the general tile form
    _wg("wt_1", "wide_tile_general", FWD3, 1, 1, 1, 32, 32),                                    # V = 1: wgrad_wide_kernel<1>
    _wg("wt_1x1", "wide_tile_general", FWD1, 2, 1, 32, 32, 32),                                 # T = 1
    _wg("wt_narrow", "wide_tile_general", FWD3, 2, 32, 1, 16, 16),                              # width < 4 PPW
    # ---- the global-gather form
    _wg("wg_k4s2", "wide_gather", FWD4S2, 2, 1, 64, 16, 16),
    _wg("wg_odd_c1", "wide_gather", FWD3, 1, 1, 32, 20, 28),                                    # ragged last workgroup
    _wg("wg_odd_n1", "wide_gather", FWD3, 1, 32, 1, 20, 28, db=False),
    # ---- direct_wgrad_kernel<1 | 2 | 8>
    _wg("dw_96_c1", "dwgrad_1", FWD3, 2, 1, 96, 9, 7),
    _wg("dw_96_n1", "dwgrad_1", FWD3, 2, 96, 1, 9, 7, db=False),
    _wg("dw_6_c1", "dwgrad_1", FWD3, 2, 1, 6, 9, 7),                                            # V % 4 != 0
    _wg("dw_6_n1", "dwgrad_1", FWD3, 2, 6, 1, 9, 7),
    _wg("dw_linear", "dwgrad_2", FWD1, 5, 512, 1, 1, 1),                                        # the Linear head
    _wg("dw_2048_n1", "dwgrad_8", FWD1, 3, 2048, 1, 1, 1),
    _wg("dw_2048_c1", "dwgrad_8", FWD1, 3, 1, 2048, 1, 1),
    _wg("dw_misaligned", "dwgrad_1", FWD3, 1, 32, 1, 32, 32, wide_off=1),                       # the slice starts one float in
    _wg("dw_n1_s2", "dwgrad_1", FWD4S2, 2, 32, 1, 16, 16, db=False),                            # N == 1 with stride 2
    _wg("dw_256_k4", "dwgrad_1", FWD4S2, 2, 1, 256, 16, 16),                                    # 17 x 256 sums per wave exceed the LDS limit
]


# ------------------------------------------------------------------------------------- what a case launches (no device needed)
def _up4(n):
    return (n + 3) // 4 * 4


def conv_shapes(case):
    """(input map, output map, weight shape) of a conv case, maps as (H, W)."""
    kind, C, N, H, W = case["kind"], case["C"], case["N"], case["H"], case["W"]
    if kind[0] == "fwd":
        _, k, s, p = kind
        return (H, W), ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1), (N, C, k, k)
    if kind[0] == "dgrad_s1":
        _, k, p = kind
        return (H + 2 * p - k + 1, W + 2 * p - k + 1), (H, W), (C, N, k, k)
    return (H // 2, W // 2), (H, W), (C, N, 4, 4)


def conv_launches(case):
    """[(geom, w_sn, w_sc)]: the launches of a conv case, as the models make them."""
    from mtd_gan_amd import kernels as K
    kind, B, C, N, H, W = case["kind"], case["B"], case["C"], case["N"], case["H"], case["W"]
    if kind[0] == "fwd":
        _, k, s, p = kind
        return [(K.geom_fwd(B, H, W, k, s, p), C * k * k, k * k)]
    if kind[0] == "dgrad_s1":
        _, k, p = kind
        return [(K.geom_dgrad_s1(B, H, W, k, p), k * k, N * k * k)]
    return [(K.geom_dgrad_s2(B, H, W, py, px), 16, N * 16) for py in range(2) for px in range(2)]


def conv_lds(case):
    """(in_ld, in_off, out_ld, out_off) of a conv case's slices."""
    out_ld = case["out_ld"] if case["out_ld"] is not None else _up4(case["N"]) + 8
    return _up4(case["C"]) + 8, 4, out_ld, case["out_off"]


def conv_plans(case):
    """The restated plan of every launch of a conv case, from the table alone."""
    in_ld, in_off, out_ld, out_off = conv_lds(case)
    return [plan.conv_plan(g, case["N"], case["C"], in_ld, out_ld, in_aligned=in_off % 4 == 0, out_aligned=out_off % 4 == 0,
                           act=ACTS[case["act"]], add1=case["add1"], add2=case["add2"], mask=case["mask"],
                           scale2=case["split"] is not None, scale_split=case["split"] or 0, w_sc=w_sc)
            for g, _, w_sc in conv_launches(case)]


def wgrad_launch(case):
    """(geom, w_sn, w_sc, dw shape, output map) of a weight-gradient case."""
    from mtd_gan_amd import kernels as K
    kind, B, C, N, H, W = case["kind"], case["B"], case["C"], case["N"], case["H"], case["W"]
    if kind[0] == "fwd":
        _, k, s, p = kind
        g = K.geom_fwd(B, H, W, k, s, p)
        return g, C * k * k, k * k, (N, C, k, k), (g.OH, g.OW)
    _, k, p = kind
    g = K.geom_dgrad_s1(B, H + k - 1 - 2 * p, W + k - 1 - 2 * p, k, p)      # input (H, W) -> output (H + k - 1 - 2 p, ...)
    assert (g.IH, g.IW) == (H, W)
    return g, k * k, N * k * k, (C, N, k, k), (g.OH, g.OW)


def wgrad_lds(case):
    """(p_ld, p_off, q_ld, q_off): the cotangent (N channels) and the layer input (C channels) as slices."""
    p_off = case["wide_off"] if case["C"] == 1 and case["N"] > 1 else 4
    q_off = case["wide_off"] if case["N"] == 1 and case["C"] > 1 else 4
    return _up4(case["N"]) + 8, p_off, _up4(case["C"]) + 8, q_off


def wgrad_case_plan(case):
    p_ld, p_off, q_ld, q_off = wgrad_lds(case)
    wide_off = q_off if case["N"] == 1 else p_off
    return plan.wgrad_plan(wgrad_launch(case)[0], case["N"], case["C"], p_ld, q_ld, wide_aligned=wide_off % 4 == 0)


# ------------------------------------------------------------------------------------------------------------- device helpers
def _nan(*shape):
    t = torch.empty(shape, dtype=torch.float32, device="cuda")
    _bits(t).fill_(SPARE_BITS)
    return t


def _slice(v, ld, off):
    """v (B, C, H, W) on the CPU -> (base, view): channels off .. off + C of the first B images of a (B + 1, H, W, ld) NaN tensor."""
    b, c, h, w = v.shape
    assert off + c <= ld
    base = _nan(b + 1, h, w, ld)
    view = base[:b, :, :, off:off + c]
    view.copy_(v.permute(0, 2, 3, 1))
    return base, view


def _flat(v, lead=64, tail=64):
    """v on the CPU -> (flat, view): v's values `lead` floats into a NaN buffer, `tail` more NaN behind them."""
    flat = _nan(lead + v.numel() + tail)
    view = flat[lead:lead + v.numel()].view(v.shape)
    view.copy_(v)
    return flat, view


def _only_view_changed(base, view_index):
    """Every word of base outside base[view_index] is still the sentinel NaN."""
    bits = _bits(base).clone()
    bits[view_index] = SPARE_BITS
    return bool((bits == SPARE_BITS).all())


def _mask_values(shape, seed):
    """Positive and negative values, +0 and -0."""
    kind = torch.randint(0, 4, shape, generator=torch.Generator().manual_seed(seed))
    mag = _randn(*shape, seed=seed + 1).abs() + 0.05
    m = torch.where(kind < 2, torch.where(kind == 0, mag, -mag), torch.zeros(()))
    m[kind == 3] = -0.0
    return m


def _report(record_property, what, case, e, e_ref):
    print(f"\n{what} {case['label']} {case['id']}: rel {e:.3e}, e_ref {e_ref:.3e}")
    record_property(f"{what}_{case['label']}", f"{e:.3e}")
    record_property(f"{what}_e_ref", f"{e_ref:.3e}")


def _within(e, e_ref):
    return e < max(BOUND, 4.0 * e_ref)


def _logged(K, kind, struct):
    """The argument structs of the `kind` launches in kernels.CALL_LOG; every logged call must be of that kind."""
    assert K.CALL_LOG and all(k == kind for k, _ in K.CALL_LOG), [k for k, _ in K.CALL_LOG or []]
    return [struct.from_buffer_copy(raw) for _, raw in K.CALL_LOG]


# ------------------------------------------------------------------------------------------------ forward and data gradient
def _epilogue(conv, scale, bias, add1, add2, act, mask, slope):
    """act(scale conv + bias + add1 + add2) (mask > 0 ? 1 : slope) in conv's own precision."""
    v = conv * scale
    if bias is not None:
        v = v + bias.to(v.dtype).view(1, -1, 1, 1)
    for a in (add1, add2):
        if a is not None:
            v = v + a.to(v.dtype)
    if act == "relu":
        v = torch.where(v > 0, v, torch.zeros((), dtype=v.dtype))
    elif act == "lrelu":
        v = torch.where(v > 0, v, v * 0.2)
    if mask is not None:
        v = v * torch.where(mask > 0, 1.0, slope).to(v.dtype)
    return v


def _conv_reference(case, x, w, dtype):
    kind = case["kind"]
    x, w = x.to(dtype), w.to(dtype)
    if kind[0] == "fwd":
        return F.conv2d(x, w, stride=kind[2], padding=kind[3])
    if kind[0] == "dgrad_s1":
        return F.conv_transpose2d(x, w, stride=1, padding=kind[2])
    return F.conv_transpose2d(x, w, stride=2, padding=1)


@pytest.mark.parametrize("case", CONV_CASES, ids=[c["id"] for c in CONV_CASES])
def test_direct_conv(hip_lib, record_property, case):
    """One launch (four for a stride-2 data gradient) of mtd_conv_direct through kernels.conv against float64."""
    from mtd_gan_amd import _lib, kernels as K
    B, C, N = case["B"], case["C"], case["N"]
    (IH, IW), (OH, OW), wshape = conv_shapes(case)
    in_ld, in_off, out_ld, out_off = conv_lds(case)
    T = wshape[2] * wshape[3]
    x = _randn(B, C, IH, IW, seed=11)
    w = _randn(*wshape, seed=12, scale=(C * T) ** -0.5)
    bias = _randn(N, seed=13, scale=0.1) if case["bias"] else None
    add1 = _randn(B, N, OH, OW, seed=14) if case["add1"] else None
    add2 = _randn(B, N, OH, OW, seed=15) if case["add2"] else None
    mask = _mask_values((B, N, OH, OW), seed=16) if case["mask"] else None
    m = torch.arange(B * OH * OW).view(B, 1, OH, OW)
    split = case["split"]
    assert split is None or case["kind"][0] != "dgrad_s2"          # (launch pixels are output pixels for the other kinds)
    scale = torch.where(m < split, SCALE, SCALE2) if split is not None else torch.full((1, 1, 1, 1), SCALE)
    ref = _epilogue(_conv_reference(case, x, w, torch.float64), scale.double(), bias, add1, add2, case["act"], mask, case["slope"])
    cpu32 = _epilogue(_conv_reference(case, x, w, torch.float32), scale.float(), bias, add1, add2, case["act"], mask, case["slope"])
    e_ref = rel(cpu32, ref)

    xb, xv = _slice(x, in_ld, in_off)
    wf, wd = _flat(w)
    operands = [(xb, xv), (wf, wd)]
    kw = dict(scale=torch.tensor([SCALE], device="cuda"), act=ACTS[case["act"]])
    if split is not None:
        kw.update(scale2=torch.tensor([SCALE2], device="cuda"), scale_split=split)
    if bias is not None:
        operands.append(_flat(bias))
        kw["bias"] = operands[-1][1]
    for name, t in (("add1", add1), ("add2", add2), ("mask", mask)):
        if t is not None:
            operands.append(_slice(t, _up4(N) + 4, 4))
            kw[name] = operands[-1][1]
    if mask is not None:
        kw["mask_slope"] = case["slope"]
    keeps = [b.clone() for b, _ in operands]
    ob = _nan(B + 1, OH, OW, out_ld)
    view_index = (slice(0, B), slice(None), slice(None), slice(out_off, out_off + N))
    ov = ob[view_index]
    saved, K.CALL_LOG = K.CALL_LOG, []
    try:
        for g, w_sn, w_sc in conv_launches(case):
            K.conv(xv, wd, g, N, C, w_sn, w_sc, ov, **kw)
        structs = _logged(K, "direct", _lib.ConvArgs)
    finally:
        K.CALL_LOG = saved
    for a in structs:          # the launch's own argument struct through the restated planner
        got = plan.conv_plan(a.g, a.N, a.C, a.in_ld, a.out_ld, in_aligned=a.inp % 16 == 0, out_aligned=a.out % 16 == 0, act=a.act,
                             add1=bool(a.add1), add2=bool(a.add2), mask=bool(a.mask), scale2=bool(a.scale2),
                             scale_split=a.scale_split, out2=bool(a.out2), w_sc=a.w_sc)
        assert got["refusal"] is None and got["label"] == case["label"], (got, case["label"])
    got = ov.cpu().permute(0, 3, 1, 2)
    e = rel(got, ref)
    _report(record_property, "direct_conv", case, e, e_ref)
    assert bool(torch.isfinite(got).all()), "the output is not finite"
    assert _only_view_changed(ob, view_index), "guard channels or the guard image changed"
    assert all(_same_bits(b, k) for (b, _), k in zip(operands, keeps)), "an input changed"
    if mask is not None and case["slope"] == 0.0:
        assert bool((got[~(mask > 0)] == 0.0).all()), "an entry whose mask is not positive is not exactly 0"
    assert _within(e, e_ref), f"rel {e:.3e} against float64 (fp32 on the CPU: {e_ref:.3e})"


# ------------------------------------------------------------------------------------------------------- weight gradient
def _wgrad_reference(case, x, cot, wshape, dtype):
    """(dw, db) of sum(y cot) by autograd, y the layer's output without activation."""
    kind, N = case["kind"], case["N"]
    w = torch.zeros(wshape, dtype=dtype, requires_grad=True)
    b = torch.zeros(N, dtype=dtype, requires_grad=True)
    if kind[0] == "fwd":
        y = F.conv2d(x.to(dtype), w, b, stride=kind[2], padding=kind[3])
    else:
        y = F.conv_transpose2d(x.to(dtype), w, b, stride=1, padding=kind[2])
    (y * cot.to(dtype)).sum().backward()
    return w.grad, b.grad


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c["id"] for c in WGRAD_CASES])
def test_direct_wgrad(hip_lib, record_property, case):
    """mtd_conv_wgrad with min(N, C) == 1 through kernels.wgrad: dw and db against float64 autograd, written into NaN, then twice
    with accumulate=True into a pre-filled dw / db (equal bits both times)."""
    from mtd_gan_amd import _lib, kernels as K
    B, C, N, H, W = case["B"], case["C"], case["N"], case["H"], case["W"]
    g, w_sn, w_sc, wshape, (OH, OW) = wgrad_launch(case)
    p_ld, p_off, q_ld, q_off = wgrad_lds(case)
    x = _randn(B, C, H, W, seed=21)
    cot = _randn(B, N, OH, OW, seed=22)
    ref_dw, ref_db = _wgrad_reference(case, x, cot, wshape, torch.float64)
    cpu_dw, cpu_db = _wgrad_reference(case, x, cot, wshape, torch.float32)
    e_ref = max(rel(cpu_dw, ref_dw), rel(cpu_db, ref_db) if case["db"] else 0.0)
    pre_dw, pre_db = _randn(*wshape, seed=23), _randn(N, seed=24)
    nan_dw, nan_db = torch.full(wshape, float("nan")), torch.full((N,), float("nan"))

    pb, pv = _slice(cot, p_ld, p_off)
    qb, qv = _slice(x, q_ld, q_off)
    keeps = [pb.clone(), qb.clone()]
    saved, K.CALL_LOG = K.CALL_LOG, []
    try:
        runs = []
        for fill_dw, fill_db, accumulate in ((nan_dw, nan_db, False), (pre_dw, pre_db, True), (pre_dw, pre_db, True)):
            dflat, dw = _flat(fill_dw)
            bflat, db = _flat(fill_db)
            if accumulate is False:
                _bits(dflat).fill_(SPARE_BITS)
                _bits(bflat).fill_(SPARE_BITS)
            bkeep = bflat.clone()
            K.wgrad(pv, qv, g, N, C, dw, w_sn, w_sc, db=db if case["db"] else None, accumulate=accumulate)
            runs.append((dflat, dw, bflat, db, bkeep))
        structs = _logged(K, "wgrad", _lib.WgradArgs)
    finally:
        K.CALL_LOG = saved
    for a in structs:
        wide = a.q if a.N == 1 else a.p
        got = plan.wgrad_plan(a.g, a.N, a.C, a.p_ld, a.q_ld, wide_aligned=wide % 16 == 0)
        assert got["refusal"] is None and got["label"] == case["label"], (got, case["label"])
    e = 0.0
    for k, (dflat, dw, bflat, db, bkeep) in enumerate(runs):
        acc = float(k > 0)
        assert bool(torch.isfinite(dw).all()), "dw is not finite"
        assert _only_view_changed(dflat, slice(64, 64 + dw.numel())), "the floats around dw changed"
        e = max(e, rel(dw.cpu(), ref_dw + acc * pre_dw.double()))
        if case["db"]:
            assert bool(torch.isfinite(db).all()), "db is not finite"
            assert _only_view_changed(bflat, slice(64, 64 + N)), "the floats around db changed"
            e = max(e, rel(db.cpu(), ref_db + acc * pre_db.double()))
        else:
            assert _same_bits(bflat, bkeep), "a bias gradient nobody asked for was written"
    _report(record_property, "direct_wgrad", case, e, e_ref)
    assert _same_bits(pb, keeps[0]) and _same_bits(qb, keeps[1]), "an input changed"
    assert _same_bits(runs[1][0], runs[2][0]) and _same_bits(runs[1][2], runs[2][2]), "two accumulate runs give different bits"
    assert _within(e, e_ref), f"rel {e:.3e} against float64 (fp32 on the CPU: {e_ref:.3e})"
