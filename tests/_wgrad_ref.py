"""CPU references of the weight gradient  dW(n, c, tap) = sum_pix P[pix, n] * Q[gather(pix, tap), c],  db[n] = sum_pix P[pix, n]
(mtd-gan_amd/csrc/conv_wgrad.hip) for tests/test_wgrad_ref_cpu.py and tests/test_wgrad_kernels_gpu.py.  Torch only, no device.

  ref64      float64 autograd with zero parameters: the value every kernel is compared with
  seq32      the same sums in fp32 as ONE accumulation chain over all pixels, one pixel per step, in pixel order, on the first
             32 x 32 channel block: the yardstick.  Its chain is at least as long as any kernel's (the kernels split it over
             k-steps of two pixels, waves and slabs), so a kernel that sums the right terms is no further from float64
  perturbed  ref64 with one structural error (a lost pixel, a lost 32-pixel chunk, a zeroed border column, a slab lost or summed
             twice): what the bound has to be able to see (test_wgrad_ref_cpu.py)
  Case, make_ref, case_ref, half_ref
             the layer shapes of the GPU tests, their operands (NHWC, fp32) and references, computed once per process

Operands are NHWC: x [B, IH, IW, C] is the gathered tensor (the layer's input), gy [B, OH, OW, N] the cotangent.  kind "conv":
Conv2d(k, s, p), dw in OIHW [N, C, k, k]; kind "convT": ConvTranspose2d(k, 1, p), dw in IOHW [C, N, k, k] (torch's layouts)."""
import collections
import functools

import torch
import torch.nn.functional as F

from _metrics import rel

FLOOR = 1e-5          # the floor of the existing float64 tests (test_kernels_gpu.TOL * 1e-2)
MARGIN = 2.0          # the project's margin over a yardstick: the maximum over all elements against the yardstick's 32 x 32 block


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _nchw(t, dtype):
    return t.detach().cpu().to(dtype).permute(0, 3, 1, 2).contiguous()


def ref64(x, gy, kind, k, s, p):
    """(dw, db) in float64."""
    xd, gd = _nchw(x, torch.double), _nchw(gy, torch.double)
    Cc, N = xd.shape[1], gd.shape[1]
    db = gd.sum(dim=(0, 2, 3))
    if k == 1 and s == 1 and p == 0:            # one matmul, [N, M] x [M, C]
        dw = gd.permute(1, 0, 2, 3).reshape(N, -1) @ xd.permute(0, 2, 3, 1).reshape(-1, Cc)
        return (dw.view(N, Cc, 1, 1) if kind == "conv" else dw.t().contiguous().view(Cc, N, 1, 1)), db
    if kind == "conv":
        w = torch.zeros(N, Cc, k, k, dtype=torch.double, requires_grad=True)
        y = F.conv2d(xd, w, None, stride=s, padding=p)
    else:
        assert s == 1
        w = torch.zeros(Cc, N, k, k, dtype=torch.double, requires_grad=True)
        y = F.conv_transpose2d(xd, w, None, stride=1, padding=p)
    assert y.shape == gd.shape, (y.shape, gd.shape)
    (y * gd).sum().backward()
    return w.grad, db


def _columns(x, kind, k, s, p, dtype):
    """[M, C, k * k]: for every output pixel, in pixel order, the input value each tap of each channel multiplies."""
    xn = _nchw(x, dtype)
    B, Cc = xn.shape[:2]
    if kind == "conv":
        cols = F.unfold(xn, k, padding=p, stride=s).view(B, Cc, k * k, -1)
    else:                                       # y[Y, X] += x[Y + p - ky, X + p - kx] w[ky, kx]: the flipped window of padding k - 1 - p
        cols = F.unfold(xn, k, padding=k - 1 - p).view(B, Cc, k * k, -1).flip(2)
    return cols.permute(0, 3, 1, 2).reshape(-1, Cc, k * k)


def seq32(x, gy, kind, k, s, p):
    """(dw, db) of the first 32 x 32 channel block in fp32, one rank-1 update per pixel, in the layout of ref64."""
    cols = _columns(x[..., :32], kind, k, s, p, torch.float32).reshape(-1, 32 * k * k).contiguous()
    g = gy[..., :32].detach().cpu().float().reshape(-1, 32).contiguous()
    assert cols.shape[0] == g.shape[0]
    acc = torch.zeros(32, 32 * k * k)
    bacc = torch.zeros(32)
    for m in range(g.shape[0]):
        acc.addr_(g[m], cols[m])
        bacc += g[m]
    dw = acc.view(32, 32, k, k)
    return (dw if kind == "conv" else dw.permute(1, 0, 2, 3).contiguous()), bacc


def block32(dw, db):
    """The part of a full (dw, db) that seq32 computes."""
    return dw[:32, :32], db[:32]


# ---- structural errors (ref = ref64 of the same operands; the sums are linear in both operands, so an error is ref64 of the part
# of an operand it loses, over the images that part touches)
def _partial(x, gy, kind, k, s, p, m0, m1):
    """ref64 of the cotangent pixels [m0, m1) alone."""
    B, OH, OW, N = gy.shape
    per = OH * OW
    b0, b1 = m0 // per, (m1 - 1) // per + 1
    g = torch.zeros(b1 - b0, OH, OW, N)
    g.view(-1, N)[m0 - b0 * per:m1 - b0 * per] = gy.reshape(-1, N)[m0:m1]
    return ref64(x[b0:b1], g, kind, k, s, p)


def slab_range(M, want, idx):
    """Pixels of slab idx when the planner is asked for `want` slabs of a register-operand or LDS-staged kernel (conv_wgrad_plan.h
    wgrad_split: four waves of a multiple of 32 pixels each)."""
    def ceil_div(a, b):
        return (a + b - 1) // b
    per_wave = 32 * ceil_div(ceil_div(M, 4 * want), 32)
    return idx * 4 * per_wave, min(M, (idx + 1) * 4 * per_wave)


def perturbed(ref, x, gy, kind, k, s, p, what, m0=0, m1=0):
    """(dw, db) with one structural error.  what: "pixel" (cotangent pixel m0 lost), "chunk" (pixels m0 .. m0 + 31 lost), "column" (the
    first column of image m0 of x zeroed), "slab_lost" / "slab_twice" (pixels [m0, m1))."""
    dw, db = ref
    if what == "column":
        xz = torch.zeros_like(x[m0:m0 + 1])
        xz[:, :, 0] = x[m0, :, 0]
        return dw - ref64(xz, gy[m0:m0 + 1], kind, k, s, p)[0], db
    if what == "pixel":
        m1 = m0 + 1
    elif what == "chunk":
        m1 = m0 + 32
    d = _partial(x, gy, kind, k, s, p, m0, m1)
    sign = 1.0 if what == "slab_twice" else -1.0
    return dw + sign * d[0], db + sign * d[1]


# ---- the layers of the GPU tests
# B images of an IH x IW input with C channels, N output channels; seed: of the operands
Case = collections.namedtuple("Case", "name kind B IH IW N C k s p seed")


def out_hw(c):
    if c.kind == "convT":
        return c.IH + c.k - 1 - 2 * c.p, c.IW + c.k - 1 - 2 * c.p
    return (c.IH + 2 * c.p - c.k) // c.s + 1, (c.IW + 2 * c.p - c.k) // c.s + 1


def pixels(c):
    oh, ow = out_hw(c)
    return c.B * oh * ow


Ref = collections.namedtuple("Ref", "x gy dw db yard_dw yard_db bound_dw bound_db")


def make_ref(x, gy, kind, k, s, p):
    dw, db = ref64(x, gy, kind, k, s, p)
    sdw, sdb = seq32(x, gy, kind, k, s, p)
    bdw, bdb = block32(dw, db)
    yard_dw, yard_db = rel(sdw, bdw), rel(sdb, bdb)
    return Ref(x, gy, dw, db, yard_dw, yard_db, max(FLOOR, MARGIN * yard_dw), max(FLOOR, MARGIN * yard_db))


def operands(c):
    oh, ow = out_hw(c)
    return rnd(c.B, c.IH, c.IW, c.C, seed=c.seed), rnd(c.B, oh, ow, c.N, seed=c.seed + 1)


@functools.lru_cache(maxsize=None)
def case_ref(c):
    x, gy = operands(c)
    return make_ref(x, gy, c.kind, c.k, c.s, c.p)


@functools.lru_cache(maxsize=None)
def half_ref(c, b0, b1):
    """The reference of images [b0, b1) of the case's operands alone (one half of a pair or half_scale launch)."""
    x, gy = operands(c)
    return make_ref(x[b0:b1], gy[b0:b1], c.kind, c.k, c.s, c.p)


def _c(name, kind, B, IH, IW, N, Cc, k, s, p, seed):
    return Case(name, kind, B, IH, IW, N, Cc, k, s, p, seed)


# a: maps the register-operand kernels refuse (rows no multiple of 16 pixels, no square 8 / 4 / 2 map)
A1 = {nc: _c(f"a1_{nc[0]}x{nc[1]}", "conv", 3, 12, 20, nc[0], nc[1], 3, 1, 1, 100 + nc[0]) for nc in ((32, 96), (64, 64))}
A2 = {nc: _c(f"a2_{nc[0]}x{nc[1]}", "conv", 3, 12, 20, nc[0], nc[1], 4, 2, 1, 110 + nc[0]) for nc in ((32, 96), (64, 64))}
A3 = {nc: _c(f"a3_{nc[0]}x{nc[1]}", "conv", 5, 6, 6, nc[0], nc[1], 1, 1, 0, 120 + nc[0]) for nc in ((32, 96), (64, 64))}
A4 = _c("a4_32x96", "convT", 3, 12, 12, 32, 96, 3, 1, 1, 130)
# b: rows of a multiple of 16 pixels
ROW_NC = ((32, 64), (64, 64))
B_SQ = {nc: _c(f"b_16x16_{nc[0]}x{nc[1]}", "conv", 3, 16, 16, nc[0], nc[1], 3, 1, 1, 200 + nc[0]) for nc in ROW_NC}
B_WIDE = {nc: _c(f"b_6x32_{nc[0]}x{nc[1]}", "conv", 1, 6, 32, nc[0], nc[1], 3, 1, 1, 210 + nc[0]) for nc in ROW_NC}
B_SQ_T = {nc: _c(f"bT_16x16_{nc[0]}x{nc[1]}", "convT", 3, 16, 16, nc[0], nc[1], 3, 1, 1, 220 + nc[0]) for nc in ROW_NC}
B_WIDE_T = {nc: _c(f"bT_6x32_{nc[0]}x{nc[1]}", "convT", 1, 6, 32, nc[0], nc[1], 3, 1, 1, 230 + nc[0]) for nc in ROW_NC}
B_1X1 = {nc: _c(f"b_1x1_{nc[0]}x{nc[1]}", "conv", 3, 16, 16, nc[0], nc[1], 1, 1, 0, 240 + nc[0]) for nc in ROW_NC}
# c: square 8 / 4 / 2 maps
C_BLK = {(W, B): _c(f"c_{W}x{W}_B{B}", "conv", B, W, W, 64, 32, 3, 1, 1, 300 + 10 * W + B) for W, B in ((8, 3), (4, 5), (2, 5), (2, 9))}
# d: pair launches (two halves of the batch) and half_scale launches
D_PAIR_LDS = _c("d_pair_a2_B4", "conv", 4, 12, 20, 32, 96, 4, 2, 1, 400)
D_PAIR_BLK4 = _c("d_pair_4x4_B6", "conv", 6, 4, 4, 64, 32, 3, 1, 1, 410)
D_PAIR_TAPS = _c("d_pair_taps", "conv", 2, 4, 4, 512, 512, 4, 2, 1, 420)
D_PAIR_S2 = _c("d_pair_s2", "conv", 2, 16, 16, 64, 128, 4, 2, 1, 430)
D_HALF_BLK2 = _c("d_half_2x2_B16", "conv", 16, 2, 2, 64, 32, 3, 1, 1, 440)
# e: slab counts on either side of every reduce route's limit.  E_LAYER can have 160, 80, 54, 40, ... slabs (20480 pixels in slices of a
# multiple of 128); the other three have exactly 17, 128 and 129 slices of 128 pixels
E_LAYER = _c("e_5x64x64", "conv", 5, 64, 64, 32, 32, 3, 1, 1, 500)
E_17 = _c("e_34x64", "conv", 1, 34, 64, 32, 32, 3, 1, 1, 510)
E_128 = _c("e_4x64x64", "conv", 4, 64, 64, 32, 32, 3, 1, 1, 520)
E_129 = _c("e_3x86x64", "conv", 3, 86, 64, 32, 32, 3, 1, 1, 530)
E_STAGED = _c("e_staged_512", "conv", 9, 32, 32, 512, 512, 1, 1, 0, 540)

# every reference the GPU tests compare with: (case, image range or None)
HALVES = [(D_PAIR_LDS, 0, 2), (D_PAIR_LDS, 2, 4), (D_PAIR_BLK4, 0, 3), (D_PAIR_BLK4, 3, 6), (D_PAIR_TAPS, 0, 1), (D_PAIR_TAPS, 1, 2),
          (D_PAIR_S2, 0, 1), (D_PAIR_S2, 1, 2), (A1[(32, 96)], 0, 2), (A1[(32, 96)], 2, 3), (D_HALF_BLK2, 0, 8), (D_HALF_BLK2, 8, 16)]
FULL = ([*A1.values(), *A2.values(), *A3.values(), A4, *B_SQ.values(), *B_WIDE.values(), *B_SQ_T.values(), *B_WIDE_T.values(),
         *B_1X1.values(), *C_BLK.values(), D_HALF_BLK2, E_LAYER, E_17, E_128, E_129, E_STAGED])
REDUCE_CASES = {E_LAYER: (2, 16, 17, 128, 129, 160), E_17: (17,), E_128: (128,), E_129: (129,), E_STAGED: (72,)}       # forced splits
