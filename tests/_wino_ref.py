"""CPU references of the Winograd forward / data-gradient conv launches (mtd-gan_amd/csrc/conv_winograd.hip, conv_winograd_split.h,
conv_wino_c32.h, conv_wino_s2.h) for tests/test_wino_ref_cpu.py and tests/test_wino_kernels_gpu.py.  Torch only, no device.  Cases,
epilogues, operands, the float64 conv and the epilogue contract are those of tests/_conv_ref.py.

  forms      F22 = F(2x2, 3x3), F24 = F(2x4, 3x3) (3x3 stride-1 "same" layers and their data gradients), S2 = F(3x3, 2x2) over the four
             phases of a 4x4 / stride-2 / padding-1 conv, or over one parity class of its data gradient.  The matrices are restated
             from the kernels' headers: G and the F(4,3) weight matrix from wino_weight_transform.h, B^T and A^T from
             conv_winograd.hip, G and A^T of F(3,2) from conv_wino_s2.h
  wino64     Y = A^T [ sum_k (G g G^T) (.) (B^T d B) ] A  in float64: must equal conv64 (a check of this restatement)
  wino_seq32 the yardstick: the weight transform with the header's arithmetic in fp32, the input transform in fp32, ONE accumulation
             chain per (tile, position, output channel) over the K index in the kernels' order (channel; for the stride-2 forward
             form phase-major), the inverse transform and the epilogue in fp32 -- for the first 32 output channels.  No kernel has
             a longer chain (they split it over K steps and slabs)
  SPLIT      the split-bf16 yardstick (conv_winograd_split.h): both transformed operands split EXACTLY into three bf16 pieces, the
             six retained piece products a1 b3, a3 b1, a2 b2, a1 b2, a2 b1, a1 b1 accumulated in fp32 in one chain
  bound      max(FLOOR, MARGIN * rel(yardstick, ref64 on the same block)), the constants of _conv_ref.py; the yardstick is measured
             against the reference, never against a kernel
  perturbed  ref64 with one error each (STRUCTURAL, PRECISION): what the bound has to be able to see (test_wino_ref_cpu.py)"""
import collections
import functools

import torch
import torch.nn.functional as F

import _conv_ref as R
from _conv_ref import BARE, FLOOR, MARGIN, Case, Epi, conv64, epi_operands, epilogue, full_epi, operands      # noqa: F401 (the GPU file's names)
from _metrics import rel

F22, F24, S2 = "f22", "f24", "s2"
FP32, SPLIT = "fp32", "bf16x3"

# F(2,3): interpolation points 0, +-1, inf
BT_23 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
G_23 = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
AT_23 = [[1, 1, 1, 0], [0, 1, -1, -1]]
# F(4,3): 0, +-1, +-2, inf
BT_43 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
G_43 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
AT_43 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
# F(3,2): the input transform of F(2,3)
G_32 = [[1, 0], [.5, .5], [.5, -.5], [0, 1]]
AT_32 = [[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, -1]]

Form = collections.namedtuple("Form", "BTy BTx Gy Gx ATy ATx")
FORMS = {F22: Form(BT_23, BT_23, G_23, G_23, AT_23, AT_23), F24: Form(BT_23, BT_43, G_23, G_43, AT_23, AT_43),
         S2: Form(BT_23, BT_23, G_32, G_32, AT_32, AT_32)}


def patch_hw(form):
    return len(FORMS[form].BTy), len(FORMS[form].BTx)


def tile_hw(form):
    """Output pixels of a tile."""
    return len(FORMS[form].ATy), len(FORMS[form].ATx)


def positions(form):
    ph, pw = patch_hw(form)
    return ph * pw


def _m(rows, dtype):
    return torch.tensor(rows, dtype=torch.double).to(dtype)


def form_of(c, f4=True):
    """The form a case's launch takes: the stride-2 form for 4x4 filters, F(2x4) on maps whose width is a multiple of 4 and at least 8
    (conv_plan.h wino_patch_w; f4 False: after mtd_conv_winograd_f4_min_w(0)), F(2x2) elsewhere."""
    if c.k == 4:
        return S2
    return F24 if (f4 and R.out_hw(c)[1] % 4 == 0 and R.out_hw(c)[1] >= 8) else F22


# ---- a launch as correlations: per class, an image [B, K, Hh, Ww] (float64 / fp32 NCHW) whose patch of tile (ty, tx) starts at
# (eh ty, ew tx), a filter [N, K, r, r] at correlation positions, and the launch grid
def gmat(c, w):
    """[N, C, 3, 3]: the filter entry at correlation position (a, b) (input offset -1 + a, -1 + b) of a stride-1 launch -- the data
    gradient reads the mirrored filter with the channel roles exchanged (mtd_winograd_kmap)."""
    return w if c.kind == "fwd" else w.permute(1, 0, 2, 3).flip(2, 3)


def problems(c, x, w, dtype, fwd_taps=False):
    """[(cls, image, filter)] of the launch.  fwd_taps: the data gradient with the forward tap map (a perturbation)."""
    xn = R._nchw(x, dtype)
    wd = w.detach().to(dtype)
    if c.k == 3:
        g = wd.permute(1, 0, 2, 3) if (fwd_taps and c.kind == "dgrad1") else gmat(c, wd)
        return [(None, F.pad(xn, (1, 1, 1, 1)), g.contiguous())]
    assert (c.k, c.s, c.p) == (4, 2, 1)
    xp = F.pad(xn, (1, 1, 1, 1))
    if c.kind == "fwd":         # K = (phase, channel), phase-major: tap 2 j + phase of the 4x4 filter at position j of the phase
        ph = [(py, px) for py in (0, 1) for px in (0, 1)]
        return [(None, torch.cat([xp[:, :, py::2, px::2] for py, px in ph], 1), torch.cat([wd[:, :, py::2, px::2] for py, px in ph], 1).contiguous())]
    gh, gw = R.grid_hw(c)
    out = []
    for py, px in R.classes(c):   # class (py, px): position j reads cotangent row oy + py - 1 + j and multiplies filter row ky0 + 2 (1 - j)
        ky0, kx0 = (py + 1) & 1, (px + 1) & 1
        out.append(((py, px), xp[:, :, py:py + gh + 1, px:px + gw + 1], wd[:, :, ky0::2, kx0::2].flip(2, 3).permute(1, 0, 2, 3).contiguous()))
    return out


def tiles_hw(c, form):
    gh, gw = R.grid_hw(c)
    eh, ew = tile_hw(form)
    return -(-gh // eh), -(-gw // ew)


def _patches(c, img, form):
    """[B T, K, ph, pw]: the patches of all tiles, image by image, tile rows first; zeros past a ragged last tile."""
    ph, pw = patch_hw(form)
    eh, ew = tile_hw(form)
    ty, tx = tiles_hw(c, form)
    need_h, need_w = eh * (ty - 1) + ph, ew * (tx - 1) + pw
    img = F.pad(img, (0, max(0, need_w - img.shape[3]), 0, max(0, need_h - img.shape[2])))[:, :, :need_h, :need_w]
    B, K = img.shape[:2]
    u = F.unfold(img, (ph, pw), stride=(eh, ew)).view(B, K, ph, pw, ty * tx)
    return u.permute(0, 4, 1, 2, 3).reshape(B * ty * tx, K, ph, pw)


def input_transform(d, form, dtype):
    """U = B^T d B of patches d [T, K, ph, pw] -> [K, T, P], position xi = pw a + b."""
    f = FORMS[form]
    u = torch.einsum("ai,tkij,bj->ktab", _m(f.BTy, dtype), d.to(dtype), _m(f.BTx, dtype))
    return u.reshape(u.shape[0], u.shape[1], -1).contiguous()


def weight_transform64(g, form):
    """G g G^T of filters g [N, K, r, r] in float64 -> [K, P, N]."""
    f = FORMS[form]
    u = torch.einsum("ai,nkij,bj->kabn", _m(f.Gy, torch.double), g.double(), _m(f.Gx, torch.double))
    return u.reshape(u.shape[0], -1, u.shape[3]).contiguous()


def _fma32(a, b, c):
    """fmaf on fp32 tensors: the product is exact in float64, one rounding of the sum to float64 and one to fp32."""
    return (a.double() * b.double() + c.double()).float()


def weight_transform32(g, form):
    """The same in fp32 with the arithmetic of wino_weight_transform.h (wino_w_rows, wino_w_store) and of wino32_weights_kernel
    (conv_wino_s2.h) -> [K, P, N]."""
    g = g.float()
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    if form == S2:
        t = [g[:, :, 0], 0.5 * (g[:, :, 0] + g[:, :, 1]), 0.5 * (g[:, :, 0] - g[:, :, 1]), g[:, :, 1]]          # [N, K, 2] each
        rows = [[ta[..., 0], 0.5 * (ta[..., 0] + ta[..., 1]), 0.5 * (ta[..., 0] - ta[..., 1]), ta[..., 1]] for ta in t]
    else:
        t = [g[:, :, 0], 0.5 * (g[:, :, 0] + g[:, :, 1] + g[:, :, 2]), 0.5 * (g[:, :, 0] - g[:, :, 1] + g[:, :, 2]), g[:, :, 2]]
        rows = []
        for ta in t:
            t0, t1, t2 = ta[..., 0], ta[..., 1], ta[..., 2]
            if form == F24:
                ne = (t0 + t2) * -f32(1 / 6)
                h = t0 * f32(1 / 24) + t2 * f32(1 / 6)
                rows.append([0.25 * t0, _fma32(t1, -f32(1 / 6), ne), _fma32(t1, f32(1 / 6), ne), _fma32(t1, f32(1 / 12), h),
                             _fma32(t1, -f32(1 / 12), h), t2])
            else:
                rows.append([t0, 0.5 * (t0 + t1 + t2), 0.5 * (t0 - t1 + t2), t2])
    u = torch.stack([torch.stack(r, 0) for r in rows], 0)          # [a, b, N, K]
    return u.reshape(-1, *u.shape[2:]).permute(2, 0, 1).contiguous()


def split3(x):
    """x (fp32) -> three fp32 tensors holding bf16 values with x = hi + mid + lo exactly (w3_split of conv_winograd.hip: bit masks and
    exact subtractions)."""
    def top(v):
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    x = x.float()
    h = top(x)
    r = x - h
    m = top(r)
    return h, m, r - m


def _inverse(acc, c, form, dtype):
    """Y = A^T m A of accumulators [T, P, n] -> the class image [B, gh, gw, n]."""
    f = FORMS[form]
    ph, pw = patch_hw(form)
    eh, ew = tile_hw(form)
    ty, tx = tiles_hw(c, form)
    gh, gw = R.grid_hw(c)
    n = acc.shape[-1]
    y = torch.einsum("ea,tabn,fb->tefn", _m(f.ATy, dtype), acc.view(-1, ph, pw, n), _m(f.ATx, dtype))
    y = y.reshape(c.B, ty, tx, eh, ew, n).permute(0, 1, 3, 2, 4, 5).reshape(c.B, ty * eh, tx * ew, n)
    return y[:, :gh, :gw]


def _assemble(c, parts, n, dtype):
    oh, ow = R.out_hw(c)
    out = torch.zeros(c.B, oh, ow, n, dtype=dtype)
    for cls, y in parts:
        R.class_view(out, cls).copy_(y)
    return out


def wino64(form, c, x, w, n=32, fwd_taps=False):
    """The form in float64 for the first n output channels, [B, OHF, OWF, n]."""
    parts = []
    for cls, img, g in problems(c, x, w, torch.double, fwd_taps):
        U = input_transform(_patches(c, img, form), form, torch.double)           # [K, T, P]
        Wt = weight_transform64(g[:n], form)                                        # [K, P, n]
        parts.append((cls, _inverse(torch.einsum("ktp,kpn->tpn", U, Wt), c, form, torch.double)))
    return _assemble(c, parts, n, torch.double)


def wino_seq32(form, c, x, w, pipe=FP32, n=32):
    """The yardstick: one fp32 chain per (tile, position, channel) over K; pipe SPLIT: the six bf16 piece products per term."""
    parts = []
    for cls, img, g in problems(c, x, w, torch.float32):
        U = input_transform(_patches(c, img, form), form, torch.float32)
        Wt = weight_transform32(g[:n], form)
        acc = torch.zeros(U.shape[1], U.shape[2], n)
        if pipe == SPLIT:
            a, b = split3(U), split3(Wt)
            for k in range(U.shape[0]):
                for i, j in ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)):
                    acc.add_(a[i][k].unsqueeze(-1) * b[j][k].unsqueeze(0))
        else:
            for k in range(U.shape[0]):
                acc.add_(U[k].unsqueeze(-1) * Wt[k].unsqueeze(0))
        parts.append((cls, _inverse(acc, c, form, torch.float32)))
    return _assemble(c, parts, n, torch.float32)


# ---- references, once per process
@functools.lru_cache(maxsize=None)
def _acc64(c):
    return conv64(c, *operands(c))


@functools.lru_cache(maxsize=None)
def _acc_seq(c, form, pipe):
    return wino_seq32(form, c, *operands(c), pipe)


Ref = collections.namedtuple("Ref", "x w ops out out2 yard bound")


@functools.lru_cache(maxsize=None)
def case_ref(c, e=BARE, form=None, pipe=FP32):
    form = form or form_of(c)
    x, w = operands(c)
    ops = epi_operands(c, e)
    out, out2 = epilogue(c, e, ops, _acc64(c), torch.double)
    seq, _ = epilogue(c, e, ops, _acc_seq(c, form, pipe), torch.float32, 32)
    yard = rel(seq, out[..., :32])
    return Ref(x, w, ops, out, out2, yard, max(FLOOR, MARGIN * yard))


# ---- the split of K the planner gives (conv_plan.h split_k): K steps of 16 channels, slices of equal length
def k_total(c, form):
    return 4 * c.C if (form == S2 and c.kind == "fwd") else c.C


def last_slab(c, form, split=2):
    """K indices [k0, K) of the last of `split` slices."""
    K = k_total(c, form)
    chunks = K // 16
    sk = max(1, min(split, chunks))
    cps = -(-chunks // sk)
    ns = -(-chunks // cps)
    return (ns - 1) * cps * 16, K


def _k_part(c, form, x, w, k0, k1):
    """conv64 of the terms with K index in [k0, k1)."""
    if form == S2 and c.kind == "fwd":          # K = (2 py + px) C + channel: the filter entries of the other phases / channels zeroed
        keep = torch.zeros(c.C, 4, 4, dtype=torch.bool)
        for ky in range(4):
            for kx in range(4):
                kk = (2 * (ky & 1) + (kx & 1)) * c.C + torch.arange(c.C)
                keep[:, ky, kx] = (kk >= k0) & (kk < k1)
        return conv64(c, x, w * keep)
    return conv64(c, x[..., k0:k1], w[k0:k1] if c.kind != "fwd" else w[:, k0:k1])


# ---- perturbations: (perturbed result, the part of the reference it is compared with)
STRUCTURAL = ("block", "border_clamp", "scale_tile", "col_shift", "slab_lost", "slab_twice", "bias_next", "fwd_taps", "phase_lost", "parity")
PRECISION = ("round10", "bf16")
PERTURBATIONS = STRUCTURAL + PRECISION


def applies(c, e, form, what):
    if what in ("slab_lost", "slab_twice"):
        return k_total(c, form) >= 32
    if what == "border_clamp":
        return c.kind != "dgrad2"
    if what == "scale_tile":
        return e.scale2 is not None and e.split > 0
    if what == "bias_next":
        return e.bias
    if what == "fwd_taps":
        return c.kind == "dgrad1"
    if what == "phase_lost":
        return form == S2 and c.kind == "fwd"
    if what == "parity":
        return c.kind == "dgrad2"
    return True


def _mid_tile(c, form):
    """(image, tile row, tile column) of a tile in the middle of the launch."""
    ty, tx = tiles_hw(c, form)
    return c.B // 2, ty // 2, tx // 2


def perturbed(c, e, form, what):
    ref = case_ref(c, e, form)
    x, w, ops = ref.x, ref.w, ref.ops
    acc = _acc64(c)
    cls = R.classes(c)[0]
    gh, gw = R.grid_hw(c)
    eh, ew = tile_hw(form)
    ph, pw = patch_hw(form)

    def finish(a, ee=e, oo=ops):
        return epilogue(c, ee, oo, a, torch.double)[0], ref.out

    def tile_view(a, b, ty, tx):
        return R.class_view(a, cls)[b, ty * eh:min(gh, ty * eh + eh), tx * ew:min(gw, tx * ew + ew)]

    if what == "block":                     # tile in the middle, a position in the middle of the patch, the last K step
        b, ty, tx = _mid_tile(c, form)
        _, img, g = problems(c, x, w, torch.double)[0]
        img = F.pad(img, (0, pw, 0, ph))
        d = img[b:b + 1, :, ty * eh:ty * eh + ph, tx * ew:tx * ew + pw]
        K = d.shape[1]
        U = input_transform(d, form, torch.double)[K - 16:]                       # [16, 1, P]
        Wt = weight_transform64(g, form)[K - 16:]                                   # [16, P, N]
        xi = pw + 1
        m = torch.zeros(1, ph * pw, c.N, dtype=torch.double)
        m[0, xi] = torch.einsum("k,kn->n", U[:, 0, xi], Wt[:, xi])
        f = FORMS[form]
        y = torch.einsum("ea,abn,fb->efn", _m(f.ATy, torch.double), m.view(ph, pw, c.N), _m(f.ATx, torch.double))
        a = acc.clone()
        v = tile_view(a, b, ty, tx)
        v -= y[:v.shape[0], :v.shape[1]]
        return finish(a)
    if what == "border_clamp":              # the pixel above the first pixel of a tile in the first row of the last image: that pixel, not zero
        tx = tiles_hw(c, form)[1] // 2
        xn = R._nchw(x[c.B - 1:], torch.double)
        if c.k == 3:
            x0 = tx * ew                    # patch column 1 of tile tx; inside the tile it reaches output columns x0 (b = 1) and x0 + 1 (b = 0)
            g = gmat(c, w.double())
            delta = torch.zeros(2, c.N, dtype=torch.double)
            delta[0] = g[:, :, 0, 1] @ xn[0, :, 0, x0]
            delta[1] = g[:, :, 0, 0] @ xn[0, :, 0, x0]
            a = acc.clone()
            a[c.B - 1, 0, x0:x0 + 2] += delta
            return finish(a)
        x0 = 2 * tx * ew                    # stride-2 forward: input column x0 of row -1 reaches the outputs ox with 2 ox - 1 + kx = x0
        a = acc.clone()
        for kx in range(4):
            if (x0 + 1 - kx) % 2 == 0 and 0 <= (x0 + 1 - kx) // 2 < gw:
                a[c.B - 1, 0, (x0 + 1 - kx) // 2] += w[:, :, 0, kx].double() @ xn[0, :, 0, x0]
        return finish(a)
    if what == "scale_tile":                # the tile that scale_split falls into takes the scale of its first pixel throughout
        b, r = divmod(e.split, gh * gw)
        y, xx = divmod(r, gw)
        ty, tx = y // eh, xx // ew
        assert xx % ew != 0, "scale_split must fall inside a tile row"
        v, _ = epilogue(c, e, ops, acc, torch.double)
        other, _ = epilogue(c, e._replace(scale2=None), ops, acc, torch.double)
        hit = torch.zeros(acc.shape[:3], dtype=torch.bool)
        tile_view(hit, b, ty, tx).fill_(True)
        hit &= R.launch_index(c) >= e.split
        assert int(hit.sum()) >= 1
        return torch.where(hit.unsqueeze(-1), other, v), ref.out
    if what == "col_shift":
        b, ty, tx = _mid_tile(c, form)
        a = acc.clone()
        v = tile_view(a, b, ty, tx)
        v.copy_(v.roll(1, 1))
        return finish(a)
    if what in ("slab_lost", "slab_twice"):
        part = _k_part(c, form, x, w, *last_slab(c, form))
        return finish(acc + part if what == "slab_twice" else acc - part)
    if what == "bias_next":
        return finish(acc, oo=dict(ops, bias=ops["bias"].roll(-1)))
    if what == "fwd_taps":
        return finish(_nhwc64(F.conv2d(R._nchw(x, torch.double), w.double().permute(1, 0, 2, 3), None, padding=1)))
    if what == "phase_lost":                # the K steps of the last phase (py, px) = (1, 1)
        return finish(acc - _k_part(c, form, x, w, 3 * c.C, 4 * c.C))
    if what == "parity":                    # class (0, 0) written where class (0, 1) belongs
        v = ref.out.clone()
        v[:, 0::2, 1::2] = ref.out[:, 0::2, 0::2]
        return v, ref.out
    if what == "round10":
        return finish(conv64(c, R.round_mantissa(x, 10), R.round_mantissa(w, 10)))
    if what == "bf16":
        return finish(conv64(c, x.bfloat16().float(), w.bfloat16().float()))
    raise ValueError(what)


def _nhwc64(t):
    return t.permute(0, 2, 3, 1).contiguous()


def low_plane_dropped(c, e, form, n=32):
    """The split form with the low bf16 plane of BOTH transformed operands dropped, evaluated in float64 on the first n channels:
    (perturbed, reference block)."""
    ref = case_ref(c, e, form, SPLIT)
    parts = []
    for cls, img, g in problems(c, ref.x, ref.w, torch.float32):
        a = split3(input_transform(_patches(c, img, form), form, torch.float32))
        b = split3(weight_transform32(g[:n], form))
        U, Wt = a[0].double() + a[1].double(), b[0].double() + b[1].double()
        parts.append((cls, _inverse(torch.einsum("ktp,kpn->tpn", U, Wt), c, form, torch.double)))
    got, _ = epilogue(c, e, ref.ops, _assemble(c, parts, n, torch.double), torch.double, n)
    return got, ref.out[..., :n]


# ---- the documented layouts of the transformed weights (include/mtdgan_hip.h)
def unpack_weights(buf, P, N, K):
    """[xi][K / 8][N][8] floats -> [K, P, N]."""
    return buf[:P * N * K].view(P, K // 8, N, 8).permute(1, 3, 0, 2).reshape(K, P, N)


def unpack_split_weights(buf16, P, N, K):
    """[xi][K / 16][plane 0 .. 2][N][16] bf16 -> three [K, P, N] fp32 tensors."""
    v = buf16[:P * N * K * 3].view(P, K // 16, 3, N, 16).float()
    return [v[:, :, i].permute(1, 3, 0, 2).reshape(K, P, N) for i in range(3)]


# ---- the launches of the GPU tests
def _c(name, kind, B, H, W, Cc, N, k, s, p, seed):
    return Case(name, kind, B, H, W, Cc, N, k, s, p, seed)


def _pair(name, B, H, W, Cc, N, seed):
    """A 3x3 stride-1 layer as the forward launch and as the data gradient (geom_dgrad_s1) of the same shape."""
    return {kind: _c(f"{name}_{kind}", kind, B, H, W, Cc, N, 3, 1, 1, seed + (7 if kind == "dgrad1" else 0)) for kind in ("fwd", "dgrad1")}


W1 = _pair("w1_3x10x14_c80", 3, 10, 14, 80, 64, 5000)          # F(2x2): 105 tiles, split 2 (3 + 2 K steps)
W1S = _pair("w1_3x10x14_c48", 3, 10, 14, 48, 64, 5100)         # ... split 1
W2 = _pair("w2_3x6x20_c80", 3, 6, 20, 80, 64, 5200)            # F(2x4): 45 tiles, split 2
W3 = _pair("w3_3x64x66", 3, 64, 66, 32, 256, 5300)             # 128-channel workgroups
W4 = _pair("w4_4x58x58", 4, 58, 58, 64, 320, 5400)             # lean
W5 = _pair("w5_2x10x12", 2, 10, 12, 32, 32, 5500)              # 32-channel workgroups of the F(2x4) form
MORE = {name: [{k: v._replace(name=f"{v.name}_set{i}", seed=v.seed + 20 * i) for k, v in p.items()} for i in (1, 2)]
        for name, p in (("w1", W1), ("w2", W2), ("w3", W3), ("w4", W4))}         # further problems of one group launch
BASE = {"w1": W1, "w2": W2, "w3": W3, "w4": W4}


def group_cases(name, count):
    """The problems of one group launch: two forward convs, or three data gradients."""
    kind = "fwd" if count == 2 else "dgrad1"
    return [BASE[name][kind]] + [p[kind] for p in MORE[name][:count - 1]]


P1 = _pair("p1_1x8x12", 1, 8, 12, 32, 32, 5600)                # persistent 32 -> 32 form: one block
P2 = _pair("p2_3x10x20", 3, 10, 20, 32, 32, 5700)              # 75 tiles: a ragged fifth block
P3 = _pair("p3_5x84x84", 5, 84, 84, 32, 32, 5800)              # 276 blocks on 256 workgroups
S2A = _c("s2a_fwd_3x20x28", "fwd", 3, 20, 28, 64, 64, 4, 2, 1, 6000)           # 10 x 14 outputs: ragged 3x3 tiles, split 4
S2A_D = _c("s2a_dgrad2_3x20x28", "dgrad2", 3, 20, 28, 64, 64, 4, 2, 1, 6100)   # its data gradient: four classes of 10 x 14
S2B_D = _c("s2b_dgrad2_4x96x96", "dgrad2", 4, 96, 96, 64, 192, 4, 2, 1, 6200)  # classes of 48 x 48: the lean form
S2C = _c("s2c_fwd_3x160x160", "fwd", 3, 160, 160, 64, 128, 4, 2, 1, 6300)      # 128-channel workgroups, split 3

# scale_split of the full epilogue: inside the first row of a tile (and inside an image)
SPLITS = {"w1": 14 * 4 + 14 * 10 + 5, "w2": 20 * 2 + 20 * 6 + 6, "w3": 66 * 64 + 66 * 10 + 33, "w4": 58 * 58 * 2 + 58 * 6 + 7,
          "w5": 12 * 10 + 12 * 4 + 6, "s2a": 14 * 10 + 14 * 3 + 4, "s2b": 48 * 48 + 48 * 6 + 7, "s2c": 80 * 80 + 80 * 3 + 4}
LRELU = R.ACT_LRELU


def full(name):
    return full_epi(LRELU, SPLITS[name])


E_ADD_RELU = Epi(None, None, 0, True, True, False, R.ACT_RELU, False, False)
E_RELU_ADD = R.E_RELU_ADD
E_RELU_ADD2 = Epi(None, None, 0, True, True, True, R.ACT_RELU_ADD, False, False)
E_SCALE = Epi(R.SCALE, None, 0, True, False, False, LRELU, False, False)
E_MASK = R.E_LRELU_MASK
E_MASK_ADD_OUT2 = Epi(None, None, 0, True, True, False, LRELU, True, True)
C32_EPIS = (BARE, E_ADD_RELU, E_RELU_ADD, E_MASK, E_MASK_ADD_OUT2)


def _refs():
    """Every (case, epilogue, form, pipe) the GPU tests compare with."""
    r = []
    for name, pair in (("w1", W1), ("w1", W1S), ("w2", W2), ("w3", W3), ("w4", W4)):
        for c in pair.values():
            r += [(c, e, form_of(c), FP32) for e in (BARE, full(name))]
    for name, pair in (("w1", W1), ("w2", W2)):
        for c in pair.values():
            r += [(c, e, form_of(c), SPLIT) for e in (BARE, full(name))]
    for name in MORE:
        r += [(c, full(name), form_of(c), FP32) for c in group_cases(name, 2)[1:] + group_cases(name, 3)[1:]]
    r += [(c, e, F24, FP32) for c in W5.values() for e in (E_SCALE, E_MASK, E_RELU_ADD2)]
    r += [(c, e, F24, FP32) for pair in (P1, P2, P3) for c in pair.values() for e in C32_EPIS]
    r += [(c, e, S2, FP32) for c, name in ((S2A, "s2a"), (S2A_D, "s2a"), (S2B_D, "s2b"), (S2C, "s2c")) for e in (BARE, full(name))]
    return r


REFS = _refs()
