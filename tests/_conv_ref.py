"""CPU references of the implicit-GEMM conv launches  out[pix, n] = epilogue(sum_{tap, c} in[gather(pix, tap), c] * W(n, c, tap))
(mtd-gan_amd/csrc/conv_igemm.hip, contract in include/mtdgan_hip.h) for tests/test_conv_ref_cpu.py and tests/test_igemm_kernels_gpu.py.
Torch only, no device.

  ref64      the conv in float64 (F.conv2d; F.conv_transpose2d for the stride-1 data gradient; autograd of F.conv2d for the stride-2
             one) and the epilogue contract in float64:  v = acc * (pix < scale_split ? scale : scale2) + bias + add1 + add2, the
             activation, out2 = v, out = v * (mask > 0 ? 1 : slope); MTD_ACT_RELU_ADD adds the residuals after the ReLU
  seq32      the yardstick: the same sums in fp32 as ONE accumulation chain per output over (tap, channel) in the kernels' K order,
             for the first 32 output channels and all pixels -- K rank-1 steps on an [M, 32] matrix built from F.unfold columns --
             and the same epilogue in fp32.  No kernel has a longer chain (they split it over k-steps, chunks and slabs), so a kernel
             that sums the right products is no further from float64
  bound      max(FLOOR, MARGIN * rel(seq32, ref64 on the same block)); the yardstick is measured against the reference, never a kernel
  perturbed  ref64 with one error each (PERTURBATIONS): what the bound has to be able to see (test_conv_ref_cpu.py)
  Case, Epi, case_ref
             the launches of the GPU tests, their operands (NHWC, fp32) and references, computed once per process

A Case is one launch shape.  B x H x W is the LAYER's input-side map: the gathered tensor of kind "fwd" (Conv2d(C -> N, k, s, p),
weights OIHW [N, C, k, k]); the OUTPUT of the data-gradient kinds "dgrad1" (Conv2d(N -> C, k, 1, p) backward: geom_dgrad_s1) and
"dgrad2" (Conv2d(N -> C, 4, 2, 1) backward: the four parity classes of geom_dgrad_s2), whose weights are OIHW [C, N, k, k] and whose
gathered tensor is the cotangent [B, OH, OW, C].  C: channels of the gathered tensor (the K side), N: output channels of the launch."""
import collections
import functools

import torch
import torch.nn.functional as F

from _metrics import rel

FLOOR = 1e-5          # the constants of _wgrad_ref.py
MARGIN = 2.0
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_RELU_ADD = 0, 1, 2, 3
SCALE, SCALE2, SLOPE = 0.7, 1.3, 0.2

Case = collections.namedtuple("Case", "name kind B H W C N k s p seed")
# the epilogue of a launch: scale / scale2 / mask_slope as Python floats or None, scale_split in launch pixels, the rest flags
Epi = collections.namedtuple("Epi", "scale scale2 split bias add1 add2 act mask out2")
BARE = Epi(None, None, 0, False, False, False, ACT_NONE, False, False)


def full_epi(act, split):
    return Epi(SCALE, SCALE2, split, True, True, True, act, True, False)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def f32(v):
    """The value a kernel reads from an fp32 scalar."""
    return torch.tensor(v, dtype=torch.float32).double().item()


def gathered_hw(c):
    if c.kind == "fwd":
        return c.H, c.W
    return (c.H + 2 * c.p - c.k) // c.s + 1, (c.W + 2 * c.p - c.k) // c.s + 1


def out_hw(c):
    """The output image of the launch (OHF x OWF)."""
    if c.kind == "fwd":
        return (c.H + 2 * c.p - c.k) // c.s + 1, (c.W + 2 * c.p - c.k) // c.s + 1
    return c.H, c.W


def classes(c):
    """The launches that fill the output: one, or the four parity classes (py, px) of a stride-2 data gradient."""
    return [(0, 0), (0, 1), (1, 0), (1, 1)] if c.kind == "dgrad2" else [None]


def grid_hw(c):
    """The launch grid per image (OH x OW)."""
    oh, ow = out_hw(c)
    return (oh // 2, ow // 2) if c.kind == "dgrad2" else (oh, ow)


def pixels(c):
    """M of one launch."""
    gh, gw = grid_hw(c)
    return c.B * gh * gw


def taps(c):
    return 4 if c.kind == "dgrad2" else c.k * c.k


def weight_shape(c):
    return (c.N, c.C, c.k, c.k) if c.kind == "fwd" else (c.C, c.N, c.k, c.k)


def class_view(t, cls):
    """The pixels of [B, OHF, OWF, ...] that launch `cls` writes, as [B, OH, OW, ...]."""
    return t if cls is None else t[:, cls[0]::2, cls[1]::2]


def launch_index(c):
    """[B, OHF, OWF]: the launch-grid pixel index m (the argument of scale_split) behind every output pixel."""
    oh, ow = out_hw(c)
    gh, gw = grid_hw(c)
    m = torch.arange(c.B * gh * gw).view(c.B, gh, gw)
    if c.kind != "dgrad2":
        return m
    return m.repeat_interleave(2, 1).repeat_interleave(2, 2)


# ---- operands
def operands(c):
    """(gathered tensor NHWC fp32, weights in torch's layout fp32), the weights scaled so that outputs have unit scale."""
    gh, gw = gathered_hw(c)
    x = rnd(c.B, gh, gw, c.C, seed=c.seed)
    w = rnd(*weight_shape(c), seed=c.seed + 1, scale=(c.C * taps(c)) ** -0.5)
    return x, w


def epi_operands(c, e):
    """bias [N], add1 / add2 / mask [B, OHF, OWF, N] (fp32; the mask with exact zeros), or None each."""
    oh, ow = out_hw(c)
    shape = (c.B, oh, ow, c.N)
    ops = {"bias": rnd(c.N, seed=c.seed + 2, scale=0.5) if e.bias else None,
           "add1": rnd(*shape, seed=c.seed + 3) if e.add1 else None,
           "add2": rnd(*shape, seed=c.seed + 4) if e.add2 else None,
           "mask": rnd(*shape, seed=c.seed + 5) if e.mask else None}
    if e.mask:
        ops["mask"].view(-1)[::5] = 0.0
    return ops


def _nchw(t, dtype):
    return t.detach().to(dtype).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- the conv itself
def conv64(c, x, w):
    """The bare conv in float64, NHWC [B, OHF, OWF, N]."""
    xd, wd = _nchw(x, torch.double), w.detach().double()
    if c.kind == "fwd":
        return _nhwc(F.conv2d(xd, wd, None, stride=c.s, padding=c.p))
    if c.kind == "dgrad1":
        return _nhwc(F.conv_transpose2d(xd, wd, None, stride=1, padding=c.p))
    assert (c.k, c.s, c.p) == (4, 2, 1)
    z = torch.zeros(c.B, c.N, c.H, c.W, dtype=torch.double, requires_grad=True)
    y = F.conv2d(z, wd, None, stride=2, padding=1)
    assert y.shape == xd.shape, (y.shape, xd.shape)
    (y * xd).sum().backward()
    return _nhwc(z.grad)


def columns(c, x, dtype, cls=None):
    """[M, T, C]: for every launch pixel, in launch order, the gathered value of every tap, the taps in the kernels' order
    (mtd_geom: tap (ty, tx) reads iy = oy * in_s + off + ty * tap_d)."""
    xn = _nchw(x, dtype)
    B, Cc = xn.shape[:2]
    if c.kind == "fwd":
        cols = F.unfold(xn, c.k, padding=c.p, stride=c.s).view(B, Cc, c.k * c.k, -1)
    elif c.kind == "dgrad1":                    # out[Y] += g[Y + p - ky] w[ky]: the flipped window of padding k - 1 - p
        cols = F.unfold(xn, c.k, padding=c.k - 1 - c.p).view(B, Cc, c.k * c.k, -1).flip(2)
    else:                                       # class (py, px): the 2 x 2 window of rows oy + py - 1, oy + py; tap ty reads row oy + off - ty
        gh, gw = grid_hw(c)
        u = F.unfold(xn, 2, padding=1).view(B, Cc, 4, gh + 1, gw + 1)
        cols = u[:, :, :, cls[0]:cls[0] + gh, cls[1]:cls[1] + gw].reshape(B, Cc, 4, -1).flip(2)
    return cols.permute(0, 3, 2, 1).reshape(-1, cols.shape[2], Cc)


def wmat(c, w, dtype, cls=None):
    """[T, C, N]: W(n, c, tap) of the launch, the taps in the order of columns()."""
    wd = w.detach().to(dtype)
    if c.kind == "fwd":
        return wd.reshape(c.N, c.C, -1).permute(2, 1, 0).contiguous()
    if c.kind == "dgrad1":
        return wd.reshape(c.C, c.N, -1).permute(2, 0, 1).contiguous()
    ky0, kx0 = (cls[0] + 1) & 1, (cls[1] + 1) & 1       # tap (ty, tx) multiplies the filter entry (ky0 + 2 ty, kx0 + 2 tx)
    return wd[:, :, ky0::2, kx0::2].reshape(c.C, c.N, 4).permute(2, 0, 1).contiguous()


def _chain(c, x, w, acc_dtype):
    """[B, OHF, OWF, 32] in fp32: every output of the first 32 channels as ONE chain over (tap, channel), the accumulator rounded to
    acc_dtype after every step."""
    oh, ow = out_hw(c)
    gh, gw = grid_hw(c)
    out = torch.zeros(c.B, oh, ow, 32)
    for cls in classes(c):
        cols = columns(c, x, torch.float32, cls)
        M, T, Cc = cols.shape
        ct = cols.reshape(M, T * Cc).t().contiguous()
        wm = wmat(c, w, torch.float32, cls)[:, :, :32].reshape(T * Cc, 32).contiguous()
        acc = torch.zeros(M, 32, dtype=acc_dtype)
        for kk in range(T * Cc):
            step = ct[kk].unsqueeze(1) * wm[kk].unsqueeze(0)
            acc = (acc.float() + step).to(acc_dtype) if acc_dtype != torch.float32 else acc.add_(step)
        class_view(out, cls).copy_(acc.float().view(c.B, gh, gw, 32))
    return out


def epilogue(c, e, ops, acc, dtype, n=None):
    """(out, out2) of the accumulators acc [B, OHF, OWF, n] (the first n channels) in `dtype`, by the contract of mtdgan_hip.h."""
    sl = slice(0, n if n is not None else c.N)
    v = acc.to(dtype)
    if e.scale is not None:
        s = torch.full(v.shape[:3], f32(e.scale), dtype=torch.double)
        if e.scale2 is not None and e.split > 0:
            s = torch.where(launch_index(c) < e.split, s, torch.full_like(s, f32(e.scale2)))
        v = v * s.to(dtype).unsqueeze(-1)
    if e.bias:
        v = v + ops["bias"][sl].to(dtype)
    if e.act == ACT_RELU_ADD:
        v = v.clamp_min(0)
    for k in ("add1", "add2"):
        if getattr(e, k):
            v = v + ops[k][..., sl].to(dtype)
    if e.act == ACT_RELU:
        v = v.clamp_min(0)
    elif e.act == ACT_LRELU:
        v = torch.where(v > 0, v, torch.tensor(f32(0.2), dtype=dtype) * v)
    out2 = v
    if e.mask:
        v = v * torch.where(ops["mask"][..., sl] > 0, 1.0, f32(SLOPE)).to(dtype)
    return v, out2


# ---- references, once per process
@functools.lru_cache(maxsize=None)
def _acc64(c):
    return conv64(c, *operands(c))


@functools.lru_cache(maxsize=None)
def _acc_chain(c, acc_dtype):
    return _chain(c, *operands(c), acc_dtype)


Ref = collections.namedtuple("Ref", "x w ops out out2 yard bound")


@functools.lru_cache(maxsize=None)
def case_ref(c, e=BARE):
    x, w = operands(c)
    ops = epi_operands(c, e)
    out, out2 = epilogue(c, e, ops, _acc64(c), torch.double)
    seq, _ = epilogue(c, e, ops, _acc_chain(c, torch.float32), torch.float32, 32)
    yard = rel(seq, out[..., :32])
    return Ref(x, w, ops, out, out2, yard, max(FLOOR, MARGIN * yard))


def bound(c, e=BARE):
    return case_ref(c, e).bound


# ---- perturbations: (perturbed result, the part of the reference it is compared with)
STRUCTURAL = ("product", "border_tap", "chunk", "slab_lost", "slab_twice", "scale_half", "bias_next", "parity")
PRECISION = ("round10", "bf16", "acc16")
PERTURBATIONS = STRUCTURAL + PRECISION


def applies(c, e, what):
    if what in ("slab_lost", "slab_twice"):
        return c.C >= 64
    if what == "scale_half":
        return e.scale2 is not None and e.split > 0
    if what == "bias_next":
        return e.bias
    if what == "parity":
        return c.kind == "dgrad2"
    return True


def round_mantissa(t, bits):
    """fp32 values rounded to nearest to `bits` explicit mantissa bits."""
    drop = 23 - bits
    i = t.detach().float().contiguous().view(torch.int32)
    i = (i + (1 << (drop - 1))) & ~((1 << drop) - 1)
    return i.view(torch.float32)


def last_slab(c, split=2):
    """Channels [c0, c1) of the last of `split` K slices (conv_plan.h split_k: slices of equal length in 32-channel chunks)."""
    chunks = c.C // 32
    sk = max(1, min(split, chunks))
    cps = -(-chunks // sk)
    ns = -(-chunks // cps)
    return (ns - 1) * cps * 32, c.C


def _valid_tap(cols_px):
    """cols_px [m, T, C] -> the last tap that lies inside the image for every one of these pixels."""
    live = (cols_px.abs().sum(2) > 0).all(0)
    assert bool(live.any())
    return int(live.nonzero().max())


def perturbed(c, e, what):
    ref = case_ref(c, e)
    x, w, ops = ref.x, ref.w, ref.ops
    acc = _acc64(c)
    cls = classes(c)[0]
    gh, gw = grid_hw(c)
    M = pixels(c)

    def finish(a, ee=e, oo=ops):
        return epilogue(c, ee, oo, a, torch.double)[0], ref.out

    def sub_rows(m0, m1, delta):            # the accumulators of launch pixels [m0, m1) of class cls minus delta [m1 - m0, N]
        a = acc.clone()
        v = class_view(a, cls).reshape(M, c.N)      # (a copy for a strided class view)
        v[m0:m1] -= delta
        class_view(a, cls).copy_(v.view(c.B, gh, gw, c.N))
        return a

    if what in ("product", "border_tap", "chunk"):
        # launch pixels [m0, m1): one pixel in the middle; the first row of the last image; a 32-pixel block in the middle
        m0, m1 = {"product": (M // 2, M // 2 + 1), "border_tap": ((c.B - 1) * gh * gw, (c.B - 1) * gh * gw + gw),
                  "chunk": (32 * (M // 64), min(M, 32 * (M // 64) + 32))}[what]
        b0, b1 = m0 // (gh * gw), (m1 - 1) // (gh * gw) + 1         # (the columns of the images they lie in)
        cols = columns(c._replace(B=b1 - b0), x[b0:b1], torch.double, cls)[m0 - b0 * gh * gw:m1 - b0 * gh * gw]
        wm = wmat(c, w, torch.double, cls)
        t = _valid_tap(cols)
        if what == "product":               # one channel of one tap: a channel of typical size
            ch = int(cols[0, t].abs().argsort()[c.C // 2])
            return finish(sub_rows(m0, m1, cols[0, t, ch] * wm[t, ch].unsqueeze(0)))
        if what == "border_tap":            # one tap
            return finish(sub_rows(m0, m1, cols[:, t] @ wm[t]))
        return finish(sub_rows(m0, m1, cols[:, t, c.C - 32:] @ wm[t, c.C - 32:]))      # one (tap, 32-channel chunk) step
    if what in ("slab_lost", "slab_twice"):
        c0, c1 = last_slab(c)
        part = conv64(c, x[..., c0:c1], w[c0:c1] if c.kind != "fwd" else w[:, c0:c1])
        return finish(acc + part if what == "slab_twice" else acc - part)
    if what == "scale_half":                # the last pixel of the first half takes the second half's scale
        v, _ = epilogue(c, e, ops, acc, torch.double)
        other, _ = epilogue(c, e._replace(scale=e.scale2, scale2=e.scale), ops, acc, torch.double)
        hit = (launch_index(c) == e.split - 1)
        if cls is not None:
            only = torch.zeros_like(hit)
            class_view(only, cls).fill_(True)
            hit &= only
        assert int(hit.sum()) == 1
        return torch.where(hit.unsqueeze(-1), other, v), ref.out
    if what == "bias_next":
        return finish(acc, oo=dict(ops, bias=ops["bias"].roll(-1)))
    if what == "parity":                    # class (0, 0) written where class (0, 1) belongs
        v = ref.out.clone()
        v[:, 0::2, 1::2] = ref.out[:, 0::2, 0::2]
        return v, ref.out
    if what == "round10":
        return finish(conv64(c, round_mantissa(x, 10), round_mantissa(w, 10)))
    if what == "bf16":
        return finish(conv64(c, x.bfloat16().float(), w.bfloat16().float()))
    if what == "acc16":
        return epilogue(c, e, ops, _acc_chain(c, torch.float16), torch.float32, 32)[0], ref.out[..., :32]
    raise ValueError(what)


# ---- the launches of the GPU tests
def _c(name, kind, B, H, W, Cc, N, k, s, p, seed):
    return Case(name, kind, B, H, W, Cc, N, k, s, p, seed)


# a: the tile kernels on the smallest maps that reach their branches (N = 128: every BN divides it)
A1 = _c("a1_3x12x20", "fwd", 3, 12, 20, 96, 128, 3, 1, 1, 1000)
A1_MORE = [_c(f"a1_3x12x20_set{i}", "fwd", 3, 12, 20, 96, 128, 3, 1, 1, 1000 + 10 * i) for i in (1, 2)]      # further problems of one multi launch
A2 = _c("a2_4x4s2_3x12x20", "fwd", 3, 12, 20, 64, 128, 4, 2, 1, 1100)
A3 = _c("a3_1x1_5x6x6", "fwd", 5, 6, 6, 64, 128, 1, 1, 0, 1200)
A4 = [_c("a4_3x2x2", "fwd", 3, 2, 2, 256, 128, 3, 1, 1, 1300), _c("a4_3x1x1", "fwd", 3, 1, 1, 256, 128, 3, 1, 1, 1310)]
A5 = _c("a5_dgrad1_2x10x14", "dgrad1", 2, 10, 14, 128, 128, 3, 1, 1, 1400)
A6I = _c("a6i_dgrad2_2x12x20", "dgrad2", 2, 12, 20, 64, 128, 4, 2, 1, 1500)
A6II = _c("a6ii_dgrad2_1x16x64", "dgrad2", 1, 16, 64, 64, 128, 4, 2, 1, 1510)
A1_SPLIT, A6II_SPLIT, A6I_SPLIT = 333, 100, 37      # scale_split: inside a 32-row block and inside an image
# c: split-K finish past one grid pass (M N = 2 621 440)
C_FIN = _c("c_5x64x64", "fwd", 5, 64, 64, 64, 128, 3, 1, 1, 2000)
# e: the generator-shaped kernels (C = 32, nine taps, >= 32768 pixels)
E1 = {(kind, N): _c(f"e1_{kind}_9x61x61_n{N}", kind, 9, 61, 61, 32, N, 3, 1, 1, 3000 + N + (7 if kind == "dgrad1" else 0))
      for kind in ("fwd", "dgrad1") for N in (32, 96)}
E2 = _c("e2_33x64x64", "fwd", 33, 64, 64, 32, 32, 3, 1, 1, 3200)
E3 = {(kind, B, H, N): _c(f"e3_{kind}_{B}x{H}x64_n{N}", kind, B, H, 64, 32, N, 3, 1, 1, 3300 + H + N + (7 if kind == "dgrad1" else 0))
      for kind in ("fwd", "dgrad1") for (B, H) in ((3, 172), (1, 512)) for N in (32, 64)}
E4 = _c("e4_1x508x64", "fwd", 1, 508, 64, 32, 32, 3, 1, 1, 3400)

E_RELU_ADD = Epi(None, None, 0, True, True, False, ACT_RELU_ADD, False, False)
E_LRELU_MASK = Epi(None, None, 0, False, False, False, ACT_LRELU, True, False)
E_MASK_OUT2 = Epi(None, None, 0, False, False, False, ACT_NONE, True, True)
E_BIAS_LRELU = Epi(None, None, 0, True, False, False, ACT_LRELU, False, False)


def _refs():
    """Every (case, epilogue) the GPU tests compare with."""
    r = [(c, BARE) for c in (A1, A2, A3, *A4, A5, A6I, A6II)]
    r += [(A1, full_epi(act, A1_SPLIT)) for act in (ACT_NONE, ACT_RELU, ACT_LRELU)]
    r += [(A6II, full_epi(act, A6II_SPLIT)) for act in (ACT_NONE, ACT_RELU, ACT_LRELU)]
    r += [(C_FIN, E_BIAS_LRELU)]
    r += [(A6I, full_epi(ACT_LRELU, A6I_SPLIT))] + [(c, full_epi(ACT_LRELU, A1_SPLIT)) for c in A1_MORE]
    r += [(c, e) for c in E1.values() for e in (BARE, E_RELU_ADD, E_LRELU_MASK)]
    r += [(E2, BARE), (E4, BARE)]
    r += [(c, BARE) for c in E3.values()] + [(c, E_MASK_OUT2) for c in E3.values() if c.N == 32]
    return r


REFS = _refs()
