"""Restatement of the Haar wavelet perceptual similarity index the test loop takes from the reference's module/piq (haarpsi.py:
haarpsi with scales = 3) for single-channel images in [0, 1], in plain torch ops on whatever dtype and device the inputs have
(float64 on the CPU for the tests' reference values, float32 on the GPU for tools/haarpsi_timing.py's torch-op form).
`haarpsi` returns (score (B,), part sums (B, 4)); the part sums are laid out as the kernels' `parts`: (num, den) of the
orientation of the Haar filter as it is (top rows +, bottom rows -), then of its transpose, num = sum sigmoid(alpha sim) w and
den = sum w over the pixels.

The operations are the reference's in its order, so that a float64 run differs from the reference's float64 run in the order of
its sums alone (tests/test_haarpsi_cpu.py: 1e-12); eps is the dtype's, as in the reference.  The kernels add float32's eps to
double sums: against den > 1 (every row of the fixture; the smallest den there is about 1e3) that moves 1 - s by less than
1.2e-7 / den relative, far below the kernels' bounds.

CASES / case_inputs: the shapes and seeded inputs shared by tools/pin_haarpsi.py (which writes tests/golden/haarpsi_piq.npz from
the reference itself) and the tests."""
import os
import zlib

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "haarpsi_piq.npz")
MIN_SIDE = 16
PART_NAMES = ("num (filter)", "den (filter)", "num (transpose)", "den (transpose)")

# (B, H, W, subsample, c, alpha).  The kernels' tile is 32 x 32 in the subsampled image: 64 x 64 is exactly one tile, 66 x 70
# and 65 x 130 are one past a tile in each dimension; 16 x 16 is all halo (the k = 8 window is the whole 8 x 8 map); 17 x 22,
# 22 x 17 and 17 x 17 are the three parities of the padding rule.
CASES = ((2, 16, 16, True, 30.0, 4.2), (1, 17, 22, True, 30.0, 4.2), (1, 22, 17, True, 30.0, 4.2), (1, 17, 17, True, 30.0, 4.2),
         (1, 64, 64, True, 30.0, 4.2), (1, 66, 70, True, 30.0, 4.2), (1, 65, 130, True, 30.0, 4.2), (1, 131, 64, True, 30.0, 4.2),
         (2, 256, 192, True, 30.0, 4.2), (1, 512, 512, True, 30.0, 4.2),
         (1, 16, 16, False, 30.0, 4.2), (1, 33, 40, False, 30.0, 4.2), (1, 64, 65, False, 30.0, 4.2),
         (1, 66, 70, True, 10.0, 2.0))


def case_inputs(index):
    """(input, target, pred) of case `index`: contiguous float32 (B, 1, H, W).  The target is uniform noise under three 5 x 5 box
    filters, stretched to [0.05, 0.95] per image; input = target + N(0, 0.08^2), pred = target + N(0, 0.02^2), clipped to [0, 1]."""
    B, H, W = CASES[index][:3]
    g = torch.Generator().manual_seed(1600 + index)
    z = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
    box = torch.full((1, 1, 5, 5), 1.0 / 25.0, dtype=torch.float64)
    for _ in range(3):
        z = F.conv2d(F.pad(z, (2, 2, 2, 2), mode="replicate"), box)
    lo, hi = z.amin(dim=(1, 2, 3), keepdim=True), z.amax(dim=(1, 2, 3), keepdim=True)
    y = 0.05 + 0.9 * (z - lo) / (hi - lo)
    x = (y + 0.08 * torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    pred = (y + 0.02 * torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    return x.float().contiguous(), y.float().contiguous(), pred.float().contiguous()


def crc(*tensors):
    c = 0
    for t in tensors:
        c = zlib.crc32(t.contiguous().numpy().tobytes(), c)
    return c


def _haar_filter(k, like):
    f = torch.ones((k, k)) / k
    f[k // 2:, :] = -f[k // 2:, :]
    return torch.stack([f.unsqueeze(0), f.unsqueeze(0).transpose(-1, -2)]).to(like)          # (2, 1, k, k)


def _check(a, b):
    if a.dim() != 4 or a.shape != b.shape or a.shape[1] != 1:
        raise AssertionError("haarpsi: two (B,1,H,W) tensors of one shape expected")
    if a.shape[-1] < MIN_SIDE or a.shape[-2] < MIN_SIDE:
        raise ValueError(f"haarpsi: images of at least {MIN_SIDE}x{MIN_SIDE} expected, got {a.shape[-2]}x{a.shape[-1]}")


def haarpsi(a, b, subsample=True, c=30.0, alpha=4.2):
    """-> (score (B,), part sums (B, 4)) of a against the target b, in the dtype of a."""
    _check(a, b)
    a, b = a * 255, b * 255
    if subsample:
        p = max(a.shape[2] % 2, a.shape[3] % 2)
        a, b = (F.avg_pool2d(F.pad(t, [0, p, 0, p]), kernel_size=2, stride=2, padding=0) for t in (a, b))
    ca, cb = [], []
    for scale in range(3):
        k = 2 ** (scale + 1)
        pad = [k // 2 - 1, k // 2, k // 2 - 1, k // 2]
        f = _haar_filter(k, a)
        ca.append(F.conv2d(F.pad(a, pad), f))
        cb.append(F.conv2d(F.pad(b, pad), f))
    ca, cb = torch.cat(ca, dim=1), torch.cat(cb, dim=1)                     # (B, 6, h, w): scale-major, (filter, transpose)
    w = torch.max(ca[:, 4:].abs(), cb[:, 4:].abs())                         # (B, 2, h, w)
    sims = []
    for o in range(2):
        ma, mb = ca[:, (o, o + 2)].abs(), cb[:, (o, o + 2)].abs()
        sims.append(((2.0 * ma * mb + c) / (ma ** 2 + mb ** 2 + c)).sum(dim=1, keepdim=True) / 2)
    sim = torch.cat(sims, dim=1)
    weighted = (sim * alpha).sigmoid() * w
    num, den = weighted.sum(dim=(2, 3)), w.sum(dim=(2, 3))                  # (B, 2) each
    parts = torch.stack([num[:, 0], den[:, 0], num[:, 1], den[:, 1]], dim=1)
    eps = torch.finfo(sim.dtype).eps
    s = (weighted.sum(dim=(1, 2, 3)) + eps) / (w.sum(dim=(1, 2, 3)) + eps)
    return (torch.log(s / (1 - s)) / alpha) ** 2, parts
