"""Every kernel of the implicit-GEMM conv family (mtd-gan_amd/csrc/conv_igemm.hip behind the planner conv_plan.h), launched through the
C ABI (mtd_conv_igemm / mtd_conv_igemm_multi -- never kernels.conv(), which sends most 3x3 layers to the Winograd kernels), forced
through mtd_conv_igemm_override and compared with float64 (tests/_conv_ref.py; tests/test_conv_ref_cpu.py shows on the CPU what the
bound can see).

  test                                  kernels
  test_tile_kernels                     igemm_kernel<2,1,4,1> <1,1,4,1> <2,2,4,1> <1,1,2,2> <2,2,2,2> <1,1,1,4>, igemm_tb_kernel<1> <2>,
                                        igemm_v2_kernel<0> (ids 0 .. 8), bare conv, forced splits 1, 2 (3): splitk_epilogue_kernel
  test_epilogue_forms                   ids 0 .. 8 with the whole epilogue on aligned views (16-byte epilogue, splitk_epilogue_kernel) and
                                        on views offset by one channel (value-by-value epilogue, splitk_epilogue_scalar_kernel)
  test_splitk_finish_second_pass        splitk_epilogue_kernel / splitk_epilogue_scalar_kernel past their 2048 workgroups
  test_multi_forms                      igemm_multi_kernel<...> (ids 16 .. 21), splitk_epilogue_multi_kernel, and its fall-back to one
                                        splitk_epilogue_scalar_kernel per problem
  test_persistent_kernel                igemm_c32p_kernel on 61-pixel rows (ragged last tile), its MTD_ACT_RELU_ADD form
  test_persistent_kernel_loops          igemm_c32p_kernel past 512 workgroups
  test_halo_tile_kernel                 igemm_c32t_kernel<4, true, true> (wide) and <4, true> on images of 172 and 512 rows, second output
  test_below_the_generator_threshold    32512 pixels: a tile kernel

Protocol of every launch (_run): arguments from kernels._conv_args; the override set in try / finally; the workspace sized by
mtd_conv_igemm[_multi]_ws_bytes under the override and filled with NaN; the launch bracketed by the launch profiler, whose ONE record
must name the expected kernel (kernels.IGEMM_CONFIGS[id]), the slice count the case aims at and the case's M, N, C and taps -- a case
whose kernel the route does not take fails, it never passes on another kernel.  Outputs (and second outputs) are channel views of
wider NaN-filled buffers: afterwards every element of the view is finite, every element outside it still NaN, and
rel(out, ref64) < max(1e-5, 2 * rel(seq32, ref64)), seq32 the fp32 one-chain evaluation of the same sums on the CPU -- never another
GPU kernel.  The four parity classes of a stride-2 data gradient go into one output; after launch i exactly (i + 1) M pixels are
finite, so every pixel is written exactly once.

Coverage, from the lines the tests print on an MI355X (pytest -s; 777 comparisons, all passing).  Launches with split 1 / with more
slices, the largest rel against float64 and where it fell.  The bound is the floor 1e-5 in every case: the yardstick's own error is
0.5e-6 .. 2.9e-6.  The profiler's record names the main kernel; which finish kernel follows it, and which epilogue build the halo-tile
kernel takes, is the host's rule in conv_igemm.hip (aligned views: 16-byte forms; views offset by one channel: the scalar forms).

  kernel                                          split 1   > 1   largest rel   at
  igemm_kernel<2, 1, 4, 1>                             24    25   2.82e-06      epilogue LeakyReLU, a1, split 2
  igemm_kernel<1, 1, 4, 1>                             45    47   2.86e-06      epilogue ReLU, a1, split 2
  igemm_kernel<2, 2, 4, 1>                             24    25   2.82e-06      epilogue LeakyReLU, a1, split 2
  igemm_kernel<1, 1, 2, 2>                             24    25   2.82e-06      epilogue LeakyReLU, a1, split 2
  igemm_kernel<2, 2, 2, 2>                             24    25   2.82e-06      epilogue LeakyReLU, a1, split 2
  igemm_kernel<1, 1, 1, 4>                             24    25   2.82e-06      epilogue LeakyReLU, a1, split 2
  igemm_tb_kernel<1>                                   23    24   3.39e-06      epilogue LeakyReLU, a1, split 1
  igemm_tb_kernel<2>                                   23    24   3.39e-06      epilogue LeakyReLU, a1, split 1
  igemm_v2_kernel<0>                                   24    25   2.82e-06      epilogue LeakyReLU, a1, split 2
  igemm_multi_kernel<...> (each of the six)             6     6   3.68e-06      two a1 problems, split 1
  igemm_c32p_kernel                                    13     -   2.59e-06      e1 forward, N 96, LeakyReLU + mask
  igemm_c32t_kernel<4, true, true> (16-byte)           12     -   2.35e-06      e3 forward 1 x 512 x 64, N 32, mask + out2
  igemm_c32t_kernel<4, true> (dword)                   12     -   2.35e-06      the same on offset views (the same bits)
  splitk_epilogue_kernel                                -   189   2.86e-06      (2.80e-06 past its 2048 workgroups, c_5x64x64)
  splitk_epilogue_scalar_kernel                         -    56   2.86e-06      (2.80e-06 past its 2048 workgroups, c_5x64x64)
  splitk_epilogue_multi_kernel                          -    18   2.82e-06      two a1 problems, split 2
  splitk_epilogue_scalar_kernel, one per problem        -    18   2.82e-06      three a1 problems on offset views, split 2

Largest per family: tile kernels 2.34e-06 (a5, tap-block kernel), epilogue forms 3.39e-06, finish past one pass 2.80e-06, multi
forms 3.68e-06, persistent 2.59e-06 (1.46e-06 where it loops), halo-tile 2.35e-06, under the threshold 1.61e-06.  Aligned and offset
views give the same figures everywhere.

The profiler assertion is what catches a dropped override: with a6 (i) pointed at N = 64 and id 4 forced (BN = 128 does not divide
64, force_takes refuses, the plan's own tile runs) the launch fails on the record's kernel name; the numbers alone would pass."""
import ctypes as C

import pytest
import torch

import _conv_ref as R
from _metrics import rel

pytestmark = pytest.mark.gpu
NAN = float("nan")
ALIGNED, OFFSET = "aligned", "offset"      # output / epilogue operand views: ld = N + 32 from channel 0; ld = N + 4 from channel 1
TILE_IDS = tuple(range(9))
TB_IDS = (6, 7)                            # the tap-block kernels: at most nine taps
MULTI0 = 16                                # igemm_multi_kernel of tile id i: 16 + i


def expected_split(c, forced):
    """Slices of a forced split (conv_plan.h split_k): `forced` slices of equal length in 32-channel chunks; what they leave."""
    chunks = c.C // 32
    sk = max(1, min(forced, chunks))
    cps = -(-chunks // sk)
    return -(-chunks // cps)


_DEV = {}


def _dev(c):
    """The case's gathered tensor and weights on the device, kept for the process (the packed weight views are keyed by address)."""
    if c not in _DEV:
        x, w = R.operands(c)
        _DEV[c] = (x.cuda(), w.cuda())
    return _DEV[c]


def _wide(shape, mode):
    """(buffer, view [..., N]) of NaN: ld = N + 32 and offset 0, or ld = N + 4 and offset one channel."""
    N = shape[-1]
    buf = torch.full((*shape[:-1], N + (32 if mode == ALIGNED else 4)), NAN, device="cuda")
    return buf, (buf[..., :N] if mode == ALIGNED else buf[..., 1:1 + N])


def _outside(buf, N, mode):
    return buf[..., N:] if mode == ALIGNED else torch.cat([buf[..., :1], buf[..., N + 1:]], -1)


def _put(t, mode):
    _, v = _wide(tuple(t.shape), mode)
    v.copy_(t)
    return v


class _Layer:
    """The device operands of one (case, epilogue): the gathered tensor (in_slice: channels 8 .. 8 + C of a NaN tensor of C + 16), the
    weights, the NaN-filled output views and the epilogue operands as views of `mode`."""

    def __init__(self, c, e=R.BARE, mode=ALIGNED, in_slice=False):
        self.c, self.e, self.mode, self.ref = c, e, mode, R.case_ref(c, e)
        x, self.w = _dev(c)
        if in_slice:
            wide = torch.full((*x.shape[:3], c.C + 16), NAN, device="cuda")
            self.x = wide[..., 8:8 + c.C]
            self.x.copy_(x)
        else:
            self.x = x
        shape = (c.B, *R.out_hw(c), c.N)
        self.buf, self.out = _wide(shape, mode)
        self.buf2, self.out2 = _wide(shape, mode) if e.out2 else (None, None)
        kw = {"act": e.act}
        if e.scale is not None:
            kw["scale"] = torch.tensor([e.scale], device="cuda")
        if e.scale2 is not None:
            kw["scale2"], kw["scale_split"] = torch.tensor([e.scale2], device="cuda"), e.split
        if e.bias:
            kw["bias"] = _put(self.ref.ops["bias"], mode)
        for k in ("add1", "add2", "mask"):
            if getattr(e, k):
                kw[k] = _put(self.ref.ops[k], mode)
        if e.mask:
            kw["mask_slope"] = R.SLOPE
        if e.out2:
            kw["out2"] = self.out2
        self.kw = kw

    def args(self, cls=None):
        from mtd_gan_amd import kernels as K
        c = self.c
        if c.kind == "fwd":
            geom = K.geom_fwd(c.B, c.H, c.W, c.k, c.s, c.p)
        elif c.kind == "dgrad1":
            geom = K.geom_dgrad_s1(c.B, c.H, c.W, c.k, c.p)
        else:
            geom = K.geom_dgrad_s2(c.B, c.H, c.W, *cls)
        T = c.k * c.k
        w_sn, w_sc = (c.C * T, T) if c.kind == "fwd" else (T, c.N * T)
        return K._conv_args(self.x, self.w, geom, c.N, c.C, w_sn, w_sc, self.out, **self.kw)

    def written_pixels(self):
        return int(torch.isfinite(self.out).all(-1).sum())

    def check(self, tag, cls=None):
        """The pixels of launch `cls` against float64; nothing outside the views touched."""
        c, ref = self.c, self.ref
        for name, buf, view, want in (("out", self.buf, self.out, ref.out), ("out2", self.buf2, self.out2, ref.out2)):
            if view is None:
                continue
            got, want = R.class_view(view.double().cpu(), cls), R.class_view(want, cls)
            assert got.shape == want.shape
            err = rel(got, want) if bool(torch.isfinite(got).all()) else float("inf")
            print(f"IGEMM {tag} {name}: {err:.3e} (bound {ref.bound:.2e}, yardstick {ref.yard:.2e})")
            assert bool(torch.isfinite(got).all()), (tag, name)
            assert bool(torch.isnan(_outside(buf, c.N, self.mode)).all()), (tag, name)
            assert err < ref.bound, (tag, name, err, ref.bound)


def _run(tag, args, cfg, split, kernel_id, want_split, multi=False):
    """ONE call of mtd_conv_igemm (args: one argument set) or mtd_conv_igemm_multi (several) under the override (cfg, split); its one
    profiler record must name kernel_id, want_split slices and the launch's M, N, C, taps."""
    from mtd_gan_amd import _lib, kernels as K
    L = _lib.lib()
    n = len(args)
    assert multi or n == 1
    arr = (_lib.ConvArgs * n)(*args)
    L.mtd_conv_igemm_override(cfg, split)
    try:
        K.prof_enable(8)
        need = L.mtd_conv_igemm_multi_ws_bytes(arr, n) if multi else L.mtd_conv_igemm_ws_bytes(C.byref(arr[0]))
        need = (need + 255) & ~255
        ws = torch.full((max(need * n, 256),), 0xFF, dtype=torch.uint8, device="cuda")      # (NaN as floats)
        for i in range(n if need else 0):
            arr[i].ws, arr[i].ws_bytes = ws.data_ptr() + i * need, need
        rc = L.mtd_conv_igemm_multi(arr, n, K.stream_ptr()) if multi else L.mtd_conv_igemm(C.byref(arr[0]), K.stream_ptr())
        recs = K.prof_collect(8) if rc == 0 else []
        torch.cuda.synchronize()
    finally:
        K.prof_enable(0)
        L.mtd_conv_igemm_override(-1, -1)
    _lib.check(rc, "mtd_conv_igemm_multi" if multi else "mtd_conv_igemm")
    a = arr[0]
    M = a.g.B * a.g.OH * a.g.OW * n
    assert len(recs) == 1, (tag, recs)
    r = recs[0]
    print(f"IGEMM {tag}: {r['kernel']} split {r['splitk']} M {r['M']} N {r['N']} C {r['C']} taps {r['taps']}")
    assert r["kernel"] == K.IGEMM_CONFIGS[kernel_id], (tag, r["kernel"], K.IGEMM_CONFIGS[kernel_id])
    assert (r["splitk"], r["M"], r["N"], r["C"], r["taps"]) == (want_split, M, a.N, a.C, a.g.TH * a.g.TW), (tag, r)


def _single_launches(tag, layer, cfg, split, kernel_id=None, want_split=None):
    """The layer as one launch per class; after launch i exactly (i + 1) M pixels of the output are written."""
    c = layer.c
    kernel_id = cfg if kernel_id is None else kernel_id
    want_split = expected_split(c, split) if want_split is None else want_split
    for i, cls in enumerate(R.classes(c)):
        t = f"{tag} {c.name}{'' if cls is None else f' class {cls[0]}{cls[1]}'} id {cfg} split {split} {layer.mode}"
        _run(t, [layer.args(cls)], cfg, split, kernel_id, want_split)
        assert layer.written_pixels() == (i + 1) * R.pixels(c), t
        layer.check(t, cls)


def _name(v):
    return v.name if isinstance(v, R.Case) else str(v)


# ---- a. the tile kernels, bare conv
TILE_CASES = (R.A1, R.A2, R.A3, *R.A4, R.A5, R.A6I, R.A6II)
TILE_SPLITS = {R.A1: (1, 2, 3)}            # forced splits; every other case: 1 and 2
# (where force_takes refuses -- more than nine taps on a tap-block kernel -- the case is not generated)
TILE_PARAMS = [(c, cfg) for c in TILE_CASES for cfg in TILE_IDS if not (cfg in TB_IDS and R.taps(c) > 9)]


@pytest.mark.parametrize("c,cfg", TILE_PARAMS, ids=_name)
def test_tile_kernels(hip_lib, c, cfg):
    """a1: 3x3 on 3 x 12 x 20, C 96 (M = 720: the last 32-row block half full, the last tile ragged for BM 64, 128 and 256, image borders
    inside every tile; forced split 2 gives slices of 2 and 1 chunks, 3 one chunk each).  a2: 4x4 / stride 2 / padding 1 (16 taps: not
    the tap-block kernels).  a3: 1x1 on 5 x 6 x 6, the native weight view.  a4: 3x3 on 3 x 2 x 2 and 3 x 1 x 1, C 256 (taps skipped for the
    whole workgroup; M = 12 and 3).  a5: geom_dgrad_s1 on 2 x 10 x 14 (mirrored taps, the packed transposed view).  a6: geom_dgrad_s2, four
    launches into one dx: (i) 2 x 12 x 20, classes of 6 x 10 (value-by-value strided epilogue); (ii) 1 x 16 x 64, classes of 8 x 32
    (out_linear with step 2)."""
    for split in TILE_SPLITS.get(c, (1, 2)):
        _single_launches("tile", _Layer(c), cfg, split)


# ---- b. the epilogue forms
@pytest.mark.parametrize("cfg", TILE_IDS)
def test_epilogue_forms(hip_lib, cfg):
    """scale and scale2 with scale_split 333 on a1 (inside a 32-row block and inside an image) and 100 on the classes of a6 (ii), bias,
    add1, add2, a mask with exact zeros and slope 0.2; LeakyReLU on every kernel, none and ReLU on the default tile.  The input is a
    channel slice [..., 8:8 + C] of a NaN tensor (in_ld > C); outputs and operands are views with ld = N + 32 from channel 0 (16-byte
    epilogue, 16-byte slab finish) and with ld = N + 4 from channel 1 (dword / value-by-value epilogue, scalar slab finish)."""
    acts = (R.ACT_LRELU, R.ACT_NONE, R.ACT_RELU) if cfg == 1 else (R.ACT_LRELU,)
    for c, at in ((R.A1, R.A1_SPLIT), (R.A6II, R.A6II_SPLIT)):
        for act in acts:
            for mode in (ALIGNED, OFFSET):
                for split in (1, 2):
                    _single_launches(f"epilogue act {act}", _Layer(c, R.full_epi(act, at), mode, in_slice=True), cfg, split)


# ---- c. the split-K finish kernels past one grid pass
@pytest.mark.parametrize("mode", (ALIGNED, OFFSET))
def test_splitk_finish_second_pass(hip_lib, mode):
    """3x3, 64 -> 128 on 5 x 64 x 64 under (1, 2): M N = 2 621 440 values -- more than the 2048 x 256 x 4 of one pass of
    splitk_epilogue_kernel and than the 2048 x 256 of splitk_epilogue_scalar_kernel (the offset view)."""
    c = R.C_FIN
    assert R.pixels(c) * c.N > 2048 * 256 * 4
    _single_launches("finish", _Layer(c, R.E_BIAS_LRELU, mode), 1, 2)


# ---- d. the multi forms
@pytest.mark.parametrize("cfg", range(6))
def test_multi_forms(hip_lib, cfg):
    """igemm_multi_kernel of every tile, BN = 128 included.  The four classes of a6 (i) and (ii) as ONE mtd_conv_igemm_multi call with the
    whole epilogue, split 1 and 2: on aligned views the grouped 16-byte finish (splitk_epilogue_multi_kernel), on the offset views one
    scalar finish per problem.  Then two and three independent a1 problems (own weights, operands, outputs; the three on offset views)."""
    for c, at in ((R.A6I, R.A6I_SPLIT), (R.A6II, R.A6II_SPLIT)):
        for mode in (ALIGNED, OFFSET):
            for split in (1, 2):
                layer = _Layer(c, R.full_epi(R.ACT_LRELU, at), mode, in_slice=True)
                tag = f"multi {c.name} id {cfg} split {split} {mode}"
                _run(tag, [layer.args(cls) for cls in R.classes(c)], cfg, split, MULTI0 + cfg, expected_split(c, split), multi=True)
                assert layer.written_pixels() == 4 * R.pixels(c), tag
                for cls in R.classes(c):
                    layer.check(f"{tag} class {cls[0]}{cls[1]}", cls)
    sets = (R.A1, *R.A1_MORE)
    for count, mode in ((2, ALIGNED), (3, OFFSET)):
        for split in (1, 2):
            layers = [_Layer(c, R.full_epi(R.ACT_LRELU, R.A1_SPLIT), mode) for c in sets[:count]]
            tag = f"multi {count} x a1 id {cfg} split {split} {mode}"
            _run(tag, [l.args() for l in layers], cfg, split, MULTI0 + cfg, expected_split(R.A1, split), multi=True)
            for l in layers:
                l.check(f"{tag} {l.c.name}")


# ---- e. the generator-shaped kernels
@pytest.mark.parametrize("e", (R.BARE, R.E_RELU_ADD, R.E_LRELU_MASK), ids=("bare", "relu_add", "lrelu_mask"))
@pytest.mark.parametrize("c", list(R.E1.values()), ids=_name)
def test_persistent_kernel(hip_lib, c, e):
    """igemm_c32p_kernel by the automatic route on 9 x 61 x 61 (M = 33 489: rows of 61 pixels, a last tile of 17), N 32 and 96, forward and
    mirrored taps: bare; relu(conv + bias) + add1 (MTD_ACT_RELU_ADD, which mtd_conv_relu_add_ok must grant); LeakyReLU and mask."""
    from mtd_gan_amd import _lib, kernels as K
    assert R.pixels(c) % 32 == 17
    layer = _Layer(c, e)
    if e.act == R.ACT_RELU_ADD:
        assert _lib.lib().mtd_conv_relu_add_ok(C.byref(layer.args())) == 1
    _single_launches("persistent", layer, -1, -1, K.IGEMM_CFG_C32P, 1)


def test_persistent_kernel_loops(hip_lib):
    """33 x 64 x 64 (M = 135 168) under the override 9: 4224 tiles of 32 pixels want 528 workgroups, the grid has 512 and its waves loop
    (the automatic route gives 64-pixel rows to the halo-tile kernel)."""
    from mtd_gan_amd import kernels as K
    c = R.E2
    assert ((R.pixels(c) + 31) // 32 + 7) // 8 > 512
    _single_launches("persistent loop", _Layer(c), K.IGEMM_CFG_C32P, -1, K.IGEMM_CFG_C32P, 1)


@pytest.mark.parametrize("c", list(R.E3.values()), ids=_name)
def test_halo_tile_kernel(hip_lib, c):
    """igemm_c32t_kernel by the automatic route on images that are not 64 rows high: 3 x 172 x 64 (129 tiles of four rows, 43 per image)
    and 1 x 512 x 64 (exactly 32 768 pixels), N 32 and 64, forward and mirrored taps.  Aligned views take its 16-byte epilogue build, views
    offset by one channel the dword build; on N 32 also with a mask and the second output (the value before the mask factor)."""
    from mtd_gan_amd import kernels as K
    assert R.pixels(c) >= 32768 and c.H % 4 == 0 and c.H != 64
    for e in ((R.BARE, R.E_MASK_OUT2) if c.N == 32 else (R.BARE,)):
        for mode in (ALIGNED, OFFSET):
            _single_launches(f"halo{' mask out2' if e.out2 else ''}", _Layer(c, e, mode), -1, -1, K.IGEMM_CFG_C32T, 1)


def test_below_the_generator_threshold(hip_lib):
    """1 x 508 x 64 = 32 512 pixels, just under the 32 768 of the generator-shaped kernels: the record names a tile kernel (the default
    tile, unsplit: one K chunk)."""
    from mtd_gan_amd import kernels as K
    assert R.pixels(R.E4) < 32768 and K.IGEMM_CFG_128x32 < K.IGEMM_CFG_TILES
    _single_launches("threshold", _Layer(R.E4), -1, -1, K.IGEMM_CFG_128x32, 1)
