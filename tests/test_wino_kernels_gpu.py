"""Every fp32 kernel of the Winograd forward / data-gradient family (mtd-gan_amd/csrc/conv_winograd.hip, conv_winograd_split.h,
conv_wino_c32.h, conv_wino_s2.h behind the planner conv_plan.h), launched through the C ABI (mtd_conv_winograd, mtd_conv_winograd_group,
mtd_conv_winograd_s2 -- never kernels.conv()) on weights built by mtd_winograd_weights / mtd_winograd_s2_weights with the library's
kmap, and compared with float64 (tests/_wino_ref.py; tests/test_wino_ref_cpu.py shows on the CPU what the bound can see).

  test                                  kernels
  test_general_kernels                  wino_conv_kernel<2, false, 4> (split 2 and 1), <2, false, 6>, <4, false, 4>, <2, true, 4>; after a split
                                        launch splitk_epilogue_kernel (aligned views) / splitk_epilogue_scalar_kernel (offset views)
  test_split_bf16_kernels               wino_conv3_kernel<4>, <6> under mtd_set_option("wino_split", 1), their own yardstick
  test_32_channel_workgroups            wino_conv_kernel<1, false, 6>: a scale operand, a mask 4 bytes off alignment, MTD_ACT_RELU_ADD with add2
  test_group_launches                   wino_conv_multi_kernel<2, false, 4>, <2, false, 6>, <4, false, 4>, <2, true, 4>: two forward convs on aligned
                                        views (split K: splitk_epilogue_multi_kernel), three data gradients on offset views
                                        (mtd_conv_winograd_group_ok refuses them where K is split: single launches)
  test_persistent_32_channel_kernel     wino_c32_kernel<false, false>, <true, false> (add + ReLU, MTD_ACT_RELU_ADD), <false, true>, <true, true>
                                        on one block, a ragged fifth block and 276 blocks on 256 workgroups
  test_stride2_kernels                  wino32_conv_kernel<2, false> (forward, split 4; four classes in one launch), <2, true>, <4, false>
  test_weight_transforms                wino_weights_kernel (px 4, 6, 20, 22), wino32_weights_kernel (groups 1, 4)

Protocol of every launch (_run): arguments from kernels._conv_args with a.w = the transformed weights (a buffer of NaN the transform
kernel wrote into) and a.w_st = the form's code; mtd_conv_winograd_f4_min_w and the option "wino_split" set in try / finally; the
workspace sized by the _ws_bytes queries and filled with NaN; the launch bracketed by the launch profiler, whose ONE record must name
the expected kernel (kernels.IGEMM_CONFIGS), the slice count, M, N, C and taps -- a case whose kernel the plan does not take fails on
the record's name, it never passes on another kernel.  Outputs, second outputs, bias, add1, add2 and mask are channel views of wider
NaN-filled buffers (aligned: ld = N + 32 from channel 0; offset: ld = N + 4 from channel 1 -- the value-by-value epilogue and slab
finish); with an epilogue the input is the channel slice [..., 8:8 + C] of a NaN tensor.  Afterwards every element of the view is
finite, every element outside it still NaN, and rel(out, ref64) < max(1e-5, 2 rel(yardstick, ref64)): the yardstick is the same form
in fp32 on the CPU as one chain over K -- never another GPU kernel.

Coverage, from the lines the tests print on an MI355X (pytest -s; 136 comparisons, all passing).  Comparisons after launches with
split 1 / with more slices, the largest rel against float64 and where it fell.  Every one of the 19 fp32 kernel names of the family
in kernels.IGEMM_CONFIGS stands in an asserted profiler record; none could not be reached (the two _Float16 forms belong to
test_half_storage_gpu.py).  The record names the main kernel; which finish kernel follows a split launch is the host's rule in
conv_igemm.hip (aligned views: 16-byte forms; views offset by one channel: the scalar form; a group: one launch for all problems).

  kernel                                      split 1   > 1   largest rel   at
  wino_conv_kernel<2, false, 4>                     8    11   1.46e-06      w1 C 48 data gradient, epilogue, aligned, split 1
  wino_conv_kernel<2, false, 6>                     -    11   4.14e-06      w2 data gradient, epilogue, aligned, split 2
  wino_conv_kernel<4, false, 4>                     8     -   1.46e-06      w3 data gradient, epilogue, aligned
  wino_conv_kernel<2, true, 4>                      8     -   2.21e-06      w4 forward, epilogue, aligned
  wino_conv_kernel<1, false, 6>                     8     -   4.17e-06      w5 forward, mask 4 bytes off alignment
  wino_conv3_kernel<4>                              -     8   1.03e-06      w1 data gradient, epilogue, aligned, split 2
  wino_conv3_kernel<6>                              -     8   4.27e-06      w2 forward, epilogue, aligned, split 2
  wino_conv_multi_kernel<2, false, 4>               -     2   1.01e-06      two forward w1 problems, split 2
  wino_conv_multi_kernel<2, false, 6>               -     2   3.38e-06      two forward w2 problems, split 2
  wino_conv_multi_kernel<4, false, 4>               5     -   1.48e-06      three w3 data gradients on offset views
  wino_conv_multi_kernel<2, true, 4>                5     -   2.21e-06      two forward w4 problems
  wino_c32_kernel<false, false>                     6     -   4.95e-06      p3 data gradient, bare
  wino_c32_kernel<true, false>                     12     -   4.55e-06      p3 data gradient, relu(conv + b + add1)
  wino_c32_kernel<false, true>                      6     -   8.98e-06      p3 data gradient, LeakyReLU + mask (bound 1.64e-05)
  wino_c32_kernel<true, true>                      12     -   6.36e-06      p3 data gradient, mask + add1 + out2 (bound 1.16e-05)
  wino32_conv_kernel<2, false>                      4     4   1.61e-06      s2a four classes in one launch, epilogue
  wino32_conv_kernel<2, true>                       4     -   2.26e-06      s2b, epilogue
  wino32_conv_kernel<4, false>                      -     4   2.32e-06      s2c, epilogue, split 3
  splitk_epilogue_kernel (16-byte)                  -    20   4.27e-06      wino_conv3_kernel<6>, w2 forward, aligned
  splitk_epilogue_scalar_kernel (value by value)    -    26   4.27e-06      wino_conv3_kernel<6>, w2 forward, offset
  splitk_epilogue_multi_kernel (a group's finish)   -     4   3.38e-06      two forward w2 problems

The yardstick's own error (rel against float64), per form: F(2x2) 0.9e-6 .. 1.9e-6, F(3x3, 2x2) 1.6e-6 .. 4.0e-6, F(2x4) 1.3e-6 ..
8.8e-6, split-bf16 F(2x2) 2.3e-6 .. 2.9e-6, split-bf16 F(2x4) 6.9e-6 .. 1.1e-5: the bound is the floor 1e-5 except on the F(2x4)
forms, where it reaches 1.8e-5 (fp32, mask epilogues) and 2.1e-5 (split-bf16).  On the general, split-bf16 and stride-2 kernels aligned
and offset views give the same figures.  Weight transforms: at most 0.57 x 2^-22 of a position's largest entry (fp32 and split forms), 0.44 x 2^-22 for the
stride-2 form."""
import ctypes as C

import pytest
import torch

import _conv_ref as R
import _wino_ref as Wn
from _metrics import rel

pytestmark = pytest.mark.gpu
NAN = float("nan")
ALIGNED, OFFSET = "aligned", "offset"      # views: ld = N + 32 from channel 0; ld = N + 4 from channel 1
PX = {Wn.F22: 4, Wn.F24: 6}

_DEV, _WT = {}, {}


def _dev(c):
    if c not in _DEV:
        x, w = R.operands(c)
        _DEV[c] = (x.cuda(), w.cuda())
    return _DEV[c]


def _wide(shape, mode):
    N = shape[-1]
    buf = torch.full((*shape[:-1], N + (32 if mode == ALIGNED else 4)), NAN, device="cuda")
    return buf, (buf[..., :N] if mode == ALIGNED else buf[..., 1:1 + N])


def _outside(buf, N, mode):
    return buf[..., N:] if mode == ALIGNED else torch.cat([buf[..., :1], buf[..., N + 1:]], -1)


def _put(t, mode):
    _, v = _wide(tuple(t.shape), mode)
    v.copy_(t)
    return v


def _geom(c, cls=None):
    from mtd_gan_amd import kernels as K
    if c.kind == "fwd":
        return K.geom_fwd(c.B, c.H, c.W, c.k, c.s, c.p)
    if c.kind == "dgrad1":
        return K.geom_dgrad_s1(c.B, c.H, c.W, c.k, c.p)
    return K.geom_dgrad_s2(c.B, c.H, c.W, *cls)


def _strides(c):
    """(w_sn, w_sc) of the view W(n, c, tap) of the case's weights (torch's layout)."""
    T = c.k * c.k
    return (c.C * T, T) if c.kind == "fwd" else (T, c.N * T)


def _transform(c, code, cls=None):
    """The transformed weights of the case for the form `code` (4, 6, 20, 22: mtd_winograd_weights; "s2": mtd_winograd_s2_weights
    for the forward geometry or class `cls`), in a NaN-filled buffer, kept for the process: (buffer, floats the form occupies)."""
    from mtd_gan_amd import _lib, kernels as K
    key = (c, code, cls)
    if key in _WT:
        return _WT[key]
    L = _lib.lib()
    _, w = _dev(c)
    geom = _geom(c, cls)
    sn, sc = _strides(c)
    if code == "s2":
        groups, km = C.c_int(0), (C.c_int * 16)()
        _lib.check(L.mtd_winograd_s2_kmap(C.byref(geom), C.byref(groups), km), "mtd_winograd_s2_kmap")
        assert groups.value == (4 if c.kind == "fwd" else 1)
        dst = torch.full((16 * groups.value * c.N * c.C + 1024,), NAN, device="cuda")        # (the kernel writes 16 groups N C floats)
        d = _lib.WinoS2WeightDesc()
        d.src, d.dst, d.sn, d.sc, d.st, d.N, d.C, d.groups = w.data_ptr(), dst.data_ptr(), sn, sc, 1, c.N, c.C, groups.value
        for i in range(16):
            d.kmap[i] = km[i]
        used = 16 * groups.value * c.N * c.C
        assert used <= dst.numel()
        tab, host = K.device_table([d], w.device)
        _lib.check(L.mtd_winograd_s2_weights(tab.data_ptr(), C.cast(host, C.c_void_p), 1, K.stream_ptr()), "mtd_winograd_s2_weights")
    else:
        dst = torch.full((L.mtd_winograd_weight_floats(c.N, c.C),), NAN, device="cuda")         # (36 N C: enough for every form)
        assert code in (4, 6, 20, 22) and (6 if code & 16 else 4) * (code & 15) * c.N * c.C <= dst.numel()
        km = (C.c_int * 9)()
        _lib.check(L.mtd_winograd_kmap(C.byref(geom), km), "mtd_winograd_kmap")
        d = _lib.WinoWeightDesc()
        d.src, d.dst, d.sn, d.sc, d.st, d.N, d.C, d.px = w.data_ptr(), dst.data_ptr(), sn, sc, 1, c.N, c.C, code
        for i in range(9):
            d.kmap[i] = km[i]
        used = (6 if code & 16 else 4) * (code & 15) * c.N * c.C
        tab, host = K.device_table([d], w.device)
        _lib.check(L.mtd_winograd_weights(tab.data_ptr(), C.cast(host, C.c_void_p), 1, K.stream_ptr()), "mtd_winograd_weights")
    torch.cuda.synchronize()
    assert used <= dst.numel() and bool(torch.isnan(dst[used:]).all()), (c.name, code)
    _WT[key] = (dst, used)
    return _WT[key]


class _Layer:
    """The device operands of one (case, epilogue): the gathered tensor (in_slice: channels 8 .. 8 + C of a NaN tensor of C + 16), the
    weights, the NaN-filled output views and the epilogue operands as views of `mode` (the mask of `mask_mode`)."""

    def __init__(self, c, e=R.BARE, mode=ALIGNED, in_slice=False, form=None, pipe=Wn.FP32, mask_mode=None):
        self.c, self.e, self.mode, self.form, self.pipe = c, e, mode, form or Wn.form_of(c), pipe
        self.ref = Wn.case_ref(c, e, self.form, pipe)
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
                kw[k] = _put(self.ref.ops[k], (mask_mode or mode) if k == "mask" else mode)
        if e.mask:
            kw["mask_slope"] = R.SLOPE
        if e.out2:
            kw["out2"] = self.out2
        self.kw = kw

    def code(self):
        return "s2" if self.form == Wn.S2 else PX[self.form] + (16 if self.pipe == Wn.SPLIT else 0)

    def args(self, cls=None):
        from mtd_gan_amd import kernels as K
        c = self.c
        a = K._conv_args(self.x, self.w, _geom(c, cls), c.N, c.C, *_strides(c), self.out, pack=False, **self.kw)
        a.w = _transform(c, self.code(), cls)[0].data_ptr()
        a.w_sn, a.w_sc, a.w_st = 0, 0, (0 if self.form == Wn.S2 else self.code())
        return a

    def check(self, tag):
        """The whole output against float64; nothing outside the views touched."""
        c, ref = self.c, self.ref
        for name, buf, view, want in (("out", self.buf, self.out, ref.out), ("out2", self.buf2, self.out2, ref.out2)):
            if view is None:
                continue
            got = view.double().cpu()
            assert got.shape == want.shape
            finite = bool(torch.isfinite(got).all())
            err = rel(got, want) if finite else float("inf")
            print(f"WINO {tag} {name}: {err:.3e} (bound {ref.bound:.2e}, yardstick {ref.yard:.2e})")
            assert finite, (tag, name)
            assert bool(torch.isnan(_outside(buf, c.N, self.mode)).all()), (tag, name)
            assert err < ref.bound, (tag, name, err, ref.bound)


def _run(tag, layers, api, kernel, want_split, split_option=0, classes=(None,)):
    """ONE call of mtd_conv_winograd (api "single": one layer), mtd_conv_winograd_group ("group": one problem per layer) or
    mtd_conv_winograd_s2 ("s2": one layer, one set per class); its one profiler record must name `kernel`, want_split slices and
    the launch's M, N, C, taps."""
    from mtd_gan_amd import _lib, kernels as K
    L = _lib.lib()
    old_min_w = L.mtd_conv_winograd_f4_min_w(8)
    assert L.mtd_set_option(b"wino_split", split_option) == 0
    try:
        args = [l.args(cls) for l in layers for cls in classes]
        n = len(args)
        assert (api == "single" and n == 1) or (api == "group" and n == len(layers) > 1) or (api == "s2" and len(layers) == 1)
        arr = (_lib.ConvArgs * n)(*args)
        if api != "s2":
            for i, l in enumerate(layers):
                assert L.mtd_conv_winograd_ok(C.byref(arr[i])) == 1, tag
                assert L.mtd_conv_winograd_patch_w(C.byref(arr[i])) == l.code(), tag
        need = L.mtd_conv_winograd_s2_ws_bytes(arr, n) if api == "s2" else L.mtd_conv_winograd_ws_bytes(C.byref(arr[0]))
        assert (need > 0) == (want_split > 1) or api == "group", (tag, need)       # (a group may split K less than a single launch)
        need = (need + 255) & ~255
        ws = torch.full((max(need * n, 256),), 0xFF, dtype=torch.uint8, device="cuda")      # (NaN as floats)
        for i in range(n if need else 0):
            arr[i].ws, arr[i].ws_bytes = ws.data_ptr() + i * need, need
        if api == "group":
            assert L.mtd_conv_winograd_group_ok(arr, n) == 1, tag
        K.prof_enable(8)
        if api == "single":
            rc, what = L.mtd_conv_winograd(C.byref(arr[0]), K.stream_ptr()), "mtd_conv_winograd"
        elif api == "group":
            rc, what = L.mtd_conv_winograd_group(arr, n, K.stream_ptr()), "mtd_conv_winograd_group"
        else:
            rc, what = L.mtd_conv_winograd_s2(arr, n, K.stream_ptr()), "mtd_conv_winograd_s2"
        recs = K.prof_collect(8) if rc == 0 else []
        torch.cuda.synchronize()
    finally:
        K.prof_enable(0)
        L.mtd_conv_winograd_f4_min_w(old_min_w)
        L.mtd_set_option(b"wino_split", 0)
    _lib.check(rc, what)
    a = arr[0]
    assert len(recs) == 1, (tag, recs)
    r = recs[0]
    print(f"WINO {tag}: {r['kernel']} split {r['splitk']} M {r['M']} N {r['N']} C {r['C']} taps {r['taps']}")
    assert kernel in K.IGEMM_CONFIGS and r["kernel"] == kernel, (tag, r["kernel"], kernel)
    assert (r["splitk"], r["M"], r["N"], r["C"], r["taps"]) == (want_split, a.g.B * a.g.OH * a.g.OW * n, a.N, a.C, a.g.TH * a.g.TW), (tag, r)


def _single(tag, layer, kernel, want_split, split_option=0):
    t = f"{tag} {layer.c.name} {'bare' if layer.e == R.BARE else 'epilogue act ' + str(layer.e.act)} {layer.mode} split {want_split}"
    _run(t, [layer], "single", kernel, want_split, split_option)
    layer.check(t)


def _epi_name(e):
    return "bare" if e == R.BARE else "epi"


# ---- a. the general fp32 kernels
GENERAL = {"w1": (Wn.W1, "wino_conv_kernel<2, false, 4>", 2), "w1s": (Wn.W1S, "wino_conv_kernel<2, false, 4>", 1),
           "w2": (Wn.W2, "wino_conv_kernel<2, false, 6>", 2), "w3": (Wn.W3, "wino_conv_kernel<4, false, 4>", 1),
           "w4": (Wn.W4, "wino_conv_kernel<2, true, 4>", 1)}


@pytest.mark.parametrize("kind", ("fwd", "dgrad1"))
@pytest.mark.parametrize("name", list(GENERAL))
def test_general_kernels(hip_lib, name, kind):
    """w1: 3 x 10 x 14, N 64 (105 tiles of 2x2: the last workgroup holds 9, workgroups span images), C 80: two slices of 3 and 2 K steps;
    w1s: C 48, unsplit.  w2: 3 x 6 x 20, C 80 (45 tiles of 2x4, five per tile row, split 2).  w3: 3 x 64 x 66, C 32, N 256 (198 workgroups
    of 128 channels).  w4: 4 x 58 x 58, C 64, N 320 (530 workgroups, four K steps: the lean form).  Each forward and as geom_dgrad_s1,
    bare and with the whole epilogue (scale_split inside a tile row; the input a channel slice), on aligned and on offset views."""
    pair, kernel, split = GENERAL[name]
    c = pair[kind]
    for e in (R.BARE, Wn.full(name.rstrip("s"))):
        for mode in (ALIGNED, OFFSET):
            _single("general", _Layer(c, e, mode, in_slice=e != R.BARE), kernel, split)


# ---- b. the split-bf16 kernels
@pytest.mark.parametrize("kind", ("fwd", "dgrad1"))
@pytest.mark.parametrize("name", ("w1", "w2"))
def test_split_bf16_kernels(hip_lib, name, kind):
    """w1 and w2 after mtd_set_option("wino_split", 1): weights as three bf16 planes (px 20 / 22), wino_conv3_kernel<4> / <6>, against
    the bound of the split-bf16 yardstick."""
    c = GENERAL[name][0][kind]
    kernel = {"w1": "wino_conv3_kernel<4>", "w2": "wino_conv3_kernel<6>"}[name]
    for e in (R.BARE, Wn.full(name)):
        for mode in (ALIGNED, OFFSET):
            _single("bf16x3", _Layer(c, e, mode, in_slice=e != R.BARE, pipe=Wn.SPLIT), kernel, 2, split_option=1)


# ---- c. the F(2x4) kernel's 32-channel workgroups
@pytest.mark.parametrize("kind", ("fwd", "dgrad1"))
def test_32_channel_workgroups(hip_lib, kind):
    """2 x 10 x 12, C = N = 32, where the persistent kernel refuses the launch: a scale operand (aligned and offset views), a mask 4 bytes
    off alignment beside an aligned output, MTD_ACT_RELU_ADD with two residual operands."""
    c = Wn.W5[kind]
    kernel = "wino_conv_kernel<1, false, 6>"
    for mode in (ALIGNED, OFFSET):
        _single("nb1 scale", _Layer(c, Wn.E_SCALE, mode, in_slice=True), kernel, 1)
    _single("nb1 mask off alignment", _Layer(c, Wn.E_MASK, ALIGNED, mask_mode=OFFSET), kernel, 1)
    _single("nb1 relu_add", _Layer(c, Wn.E_RELU_ADD2, ALIGNED), kernel, 1)


# ---- d. the group form
GROUPS = {"w1": ("wino_conv_multi_kernel<2, false, 4>", 2), "w2": ("wino_conv_multi_kernel<2, false, 6>", 2),
          "w3": ("wino_conv_multi_kernel<4, false, 4>", 1), "w4": ("wino_conv_multi_kernel<2, true, 4>", 1)}


@pytest.mark.parametrize("name", list(GROUPS))
def test_group_launches(hip_lib, name):
    """Two forward problems (own weights, operands, seeds) of w1 .. w4 as ONE mtd_conv_winograd_group call on aligned views (split K:
    the group's one-launch finish); three data-gradient problems on offset views -- where K is split mtd_conv_winograd_group_ok
    must refuse them (the one-launch finish needs 16-byte rows) and they run singly, else they are one group launch."""
    from mtd_gan_amd import _lib
    kernel, split = GROUPS[name]
    layers = [_Layer(c, Wn.full(name), ALIGNED, in_slice=True) for c in Wn.group_cases(name, 2)]
    tag = f"group 2 x {name} aligned split {split}"
    _run(tag, layers, "group", kernel, split)
    for l in layers:
        l.check(f"{tag} {l.c.name}")
    layers = [_Layer(c, Wn.full(name), OFFSET, in_slice=True) for c in Wn.group_cases(name, 3)]
    tag = f"group 3 x {name} offset split {split}"
    if split > 1:
        arr = (_lib.ConvArgs * 3)(*[l.args() for l in layers])
        ws = torch.zeros(256, device="cuda")
        for a in arr:
            a.ws, a.ws_bytes = ws.data_ptr(), 1 << 40       # (a query: nothing is launched)
        assert _lib.lib().mtd_conv_winograd_group_ok(arr, 3) == 0, tag
        for l in layers:
            _single(f"{tag}: singly", l, GENERAL[name][1], split)
    else:
        _run(tag, layers, "group", kernel, split)
        for l in layers:
            l.check(f"{tag} {l.c.name}")


# ---- e. the persistent 32 -> 32 channel kernel
C32_KERNEL = {R.BARE: "wino_c32_kernel<false, false>", Wn.E_ADD_RELU: "wino_c32_kernel<true, false>", Wn.E_RELU_ADD: "wino_c32_kernel<true, false>",
              Wn.E_MASK: "wino_c32_kernel<false, true>", Wn.E_MASK_ADD_OUT2: "wino_c32_kernel<true, true>"}


@pytest.mark.parametrize("kind", ("fwd", "dgrad1"))
@pytest.mark.parametrize("pair", (Wn.P1, Wn.P2, Wn.P3), ids=("p1", "p2", "p3"))
def test_persistent_32_channel_kernel(hip_lib, pair, kind):
    """1 x 8 x 12 (12 tiles: one block, seven idle workgroups), 3 x 10 x 20 (75 tiles: a ragged fifth block), 5 x 84 x 84 (276 blocks on 256
    workgroups: the walk wraps rows and images): bare; relu(conv + b + add1); relu(conv + b) + add1; LeakyReLU and mask; bias, add1,
    LeakyReLU, mask and the second output.  Aligned views only (the kernel's domain); the input a channel slice with an epilogue."""
    c = pair[kind]
    for e in Wn.C32_EPIS:
        _single("c32", _Layer(c, e, ALIGNED, in_slice=e != R.BARE), C32_KERNEL[e], 1)


# ---- f. F(3x3, 2x2) of the 4x4 / stride-2 layers
S2_CASES = {"s2a_fwd": (Wn.S2A, "s2a", "wino32_conv_kernel<2, false>", 4), "s2a_dgrad": (Wn.S2A_D, "s2a", "wino32_conv_kernel<2, false>", 1),
            "s2b_dgrad": (Wn.S2B_D, "s2b", "wino32_conv_kernel<2, true>", 1), "s2c_fwd": (Wn.S2C, "s2c", "wino32_conv_kernel<4, false>", 3)}


@pytest.mark.parametrize("name", list(S2_CASES))
def test_stride2_kernels(hip_lib, name):
    """s2a: forward on 3 x 20 x 28, C 64, N 64 (10 x 14 outputs: ragged 3x3 tiles both ways, split 4) and the four classes of its data
    gradient in ONE launch.  s2b: the four classes of a data gradient with 48 x 48 class maps, batch 4, N 192, C 64 (384 workgroups,
    four K steps: the lean form).  s2c: forward on 3 x 160 x 160, C 64, N 128 (128-channel workgroups, split 3).  Bare and with the
    whole epilogue, aligned and offset views."""
    c, key, kernel, split = S2_CASES[name]
    for e in (R.BARE, Wn.full(key)):
        for mode in (ALIGNED, OFFSET):
            layer = _Layer(c, e, mode, in_slice=e != R.BARE)
            tag = f"s2 {c.name} {_epi_name(e)} {mode} split {split}"
            _run(tag, [layer], "s2", kernel, split, classes=R.classes(c))
            layer.check(tag)


# ---- g. the weight transforms
def _per_position(tag, got, want):
    """max |got - want| <= 2^-22 max |want|, position by position ([K, P, N]): a transformed weight is a three-term sum of
    three-term sums of fp32 values, a few roundings of 2^-24 each at the scale of the position's largest entries."""
    err = ((got.double() - want).abs().amax((0, 2)) / want.abs().amax((0, 2))).max().item()
    print(f"WINO weights {tag}: {err * 2 ** 22:.3f} x 2^-22")
    assert bool(torch.isfinite(got).all()) and err <= 2.0 ** -22, (tag, err)


@pytest.mark.parametrize("kind", ("fwd", "dgrad1"))
@pytest.mark.parametrize("pair", (Wn.W1S, Wn.W1), ids=("c48", "c80"))
def test_weight_transforms(hip_lib, pair, kind):
    """mtd_winograd_weights for px 4, 6, 20, 22 on the forward view and on the transposed, mirrored view of the data gradient (N 64, C 48 and
    80) against G g G^T in float64 in the documented layouts; the three bf16 planes of the split codes sum, bit for bit, to the fp32
    transform of the same view (px 4 / 6).  (Before this file the F(2x4) split form rounded e, f, h and k of wino_weight_transform.h
    separately where the fp32 form fuses two products into their sums: 13 % of its values were one rounding away from the fp32
    transform.  Both forms now go through wino_w_cols.)"""
    c = pair[kind]
    _, w = R.operands(c)
    for form in (Wn.F22, Wn.F24):
        P = Wn.positions(form)
        want = Wn.weight_transform64(Wn.gmat(c, w), form)
        dst, used = _transform(c, PX[form])
        got = Wn.unpack_weights(dst.cpu(), P, c.N, c.C)
        _per_position(f"{c.name} px {PX[form]}", got, want)
        dst3, used3 = _transform(c, PX[form] + 16)
        planes = Wn.unpack_split_weights(dst3.view(torch.bfloat16).cpu(), P, c.N, c.C)
        total = planes[0].double() + planes[1].double() + planes[2].double()
        assert torch.equal(total.float().double(), total)           # (the sum is an fp32 value: nothing was rounded away)
        _per_position(f"{c.name} px {PX[form] + 16}", total, want)
        differ = int((total != got.double()).sum())
        print(f"WINO weights {c.name} px {PX[form] + 16}: {differ} of {total.numel()} values differ from the fp32 transform")
        assert differ == 0, (c.name, form, differ)


@pytest.mark.parametrize("c", (Wn.S2A, Wn.S2A_D), ids=("groups4", "groups1"))
def test_stride2_weight_transforms(hip_lib, c):
    """mtd_winograd_s2_weights for the forward geometry (four phases) and for every class of the data gradient (one group)."""
    _, w = R.operands(c)
    probs = Wn.problems(c, torch.zeros(c.B, *R.gathered_hw(c), c.C), w, torch.double)
    for cls, _, g in probs:
        dst, used = _transform(c, "s2", cls)
        K = g.shape[1]
        assert used == 16 * K * c.N
        _per_position(f"{c.name} class {cls}", Wn.unpack_weights(dst.cpu(), 16, c.N, K), Wn.weight_transform64(g, Wn.S2))
