"""CPU model of whole-slice generator inference with binary16 activation storage.

The oracle's Res-FFT-Conv block and generator (oracle/mtdgan_oracle.py::resfft_block, ::generator_forward) written with the
SEPARABLE transform -- rows, then columns, as oracle/mtdgan_oracle.py::irfft2_ortho_explicit does for the way back and as the
kernels of csrc/resfft_any.hip do both ways -- and a rounding hook `q` at exactly the stores of the storage contract:

    encoder / decoder outputs            q(relu(conv(t) + b)),  q(relu(deconv(t) + b + skip))
    the block's spatial branch           img = q(x + relu(conv3x3(x) + b))
    the row-transformed map              R   = q(rfft(x) along W, ortho)              (real and imaginary parts each)
    the column-inverse-transformed map   T   = q(ifft(relu(W2 [Re; Im] fft(R) + b2)) along H, ortho)
    the block output                     q(img + c2r(T) along W)

Everything between two hooks is fp32; the network's input and its output (the last layer adds the fp32 input) pass no hook.
q = identity gives the oracle's generator up to the summation order of the transforms; q = half_round gives the yardstick of
tests/test_half_storage_gpu.py.
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mtdgan_oracle as orc  # noqa: E402


def identity(t):
    return t


def half_round(t):
    """fp32 -> binary16 (round to nearest even, saturating at +-65504) -> fp32: one store and the load that follows it."""
    return t.clamp(-65504.0, 65504.0).half().float()


def _c2r_rows(tr, ti, W):
    """The c2r step of oracle irfft2_ortho_explicit along W (only Re of columns 0 and W/2 is used), by the library's 1-D transform:
    the explicit cosine / sine product of the oracle's function costs a few 1e-6 of fp32 summation error per block."""
    ti = ti.clone()
    ti[..., 0] = 0.0
    ti[..., -1] = 0.0
    return torch.fft.irfft(torch.complex(tr, ti), n=W, dim=3, norm="ortho")


def block(x, w_img, b_img, w_fft, b_fft, q):
    """x: (B, 32, H, W), already in storage precision.  Returns q(x + relu(conv3x3 x) + irfft2(relu(conv1x1 [Re; Im] rfft2 x)))."""
    H, W = x.shape[-2:]
    img = q(x + F.relu(F.conv2d(x, w_img, b_img, padding=1)))
    r = torch.fft.rfft(x, n=W, dim=3, norm="ortho")                          # rows: (B, 32, H, W/2 + 1)
    rr, ri = q(r.real), q(r.imag)                                            # R
    s = torch.fft.fft(torch.complex(rr, ri), n=H, dim=2, norm="ortho")       # columns
    z = F.relu(F.conv2d(torch.cat([s.real, s.imag], dim=1), w_fft, b_fft))
    zr, zi = torch.chunk(z, 2, dim=1)
    t = torch.fft.ifft(torch.complex(zr, zi), n=H, dim=2, norm="ortho")      # columns back
    tr, ti = q(t.real), q(t.imag)                                            # T
    return q(img + _c2r_rows(tr, ti, W))


def generator_forward(state, x, q=identity, pre=""):
    """oracle generator_forward with `q` at the storage contract's stores.  x and the result are fp32 (B, 1, S, S)."""
    L = orc.G_LAYERS

    def blk(i, t):
        p = f"{pre}enforce.{i}."
        return block(t, state[p + "img_conv.weight"], state[p + "img_conv.bias"], state[p + "fft_conv.weight"], state[p + "fft_conv.bias"], q)

    enc = lambda i, t: q(F.relu(F.conv2d(t, state[f"{pre}encoder.{i}.weight"], state[f"{pre}encoder.{i}.bias"], padding=1)))
    dec = lambda i, t: F.conv_transpose2d(t, state[f"{pre}decoder.{i}.weight"], state[f"{pre}decoder.{i}.bias"], padding=1)
    skips = []
    t = x
    for i in range(L):
        t = blk(i, enc(i, t))
        skips.append(t)
    t = blk(L, enc(L, t))
    t = q(F.relu(dec(L, t) + skips[L - 1]))
    for j in range(1, L):
        t = blk(L + j, t)
        t = q(F.relu(dec(L - j, t) + skips[L - 1 - j]))
    t = blk(2 * L, t)
    return F.relu(dec(0, t) + x)
