"""Restatement of the visual saliency-induced index the test loop takes from the reference's module/piq (vsi.py: vsi, data_range
1) for single-channel images in [0, 1], in plain torch ops on whatever dtype and device the inputs have (float64 on the CPU for
the tests' reference values, float32 on the GPU for tools/vsi_mdsi_timing.py's torch-op form), with torch.fft where the reference
calls the removed torch.rfft / torch.ifft.
`vsi` returns (score (B,), parts (B, 6)); the parts are laid out as the kernels' `parts`: num = sum s vs_max, den = sum vs_max,
the sum of the source's pooled saliency map, the sum of its gradient-magnitude map, and the minimum and maximum of its saliency
map at H x W before it is stretched to [0, 1].

Written from the formulas, in this project's own terms: a grey image stands for three equal colour channels, so a colour matrix
acts through its row sums (taken product by product, as a matrix product takes them); the spectrum is a complex tensor.  The
colour matrices, the white point and the frequency grid are rounded to float32 first, as the reference holds them in a float64
run too.  A float64 run differs from the reference's float64 run in the order of its operations alone
(tests/test_vsi_mdsi_cpu.py: 1e-11); eps is the dtype's, as in the reference.

CASES / case_inputs: the shapes and seeded inputs shared by tools/pin_vsi_mdsi.py (which writes tests/golden/vsi_mdsi_piq.npz
from the reference itself), tests/_mdsi_ref.py and the tests."""
import os
import zlib

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vsi_mdsi_piq.npz")
MIN_SIDE, MAX_SIDE = 16, 1024
SIDE = 256                                                      # SDSP's working size
DEFAULTS = dict(c1=1.27, c2=386., c3=130., alpha=0.4, beta=0.02, omega_0=0.021, sigma_f=1.34, sigma_d=145., sigma_c=0.001)
OTHER = dict(c1=1.5, c2=300., c3=100., alpha=0.5, beta=0.05, omega_0=0.03, sigma_f=1.2, sigma_d=120., sigma_c=0.002)
MDSI_DEFAULTS = dict(c1=140., c2=55., c3=550., combination="sum", alpha=0.6, beta=0.1, gamma=0.2, rho=1., q=0.25, o=0.25)
MDSI_OTHER = dict(c1=120., c2=60., c3=500., combination="mult", alpha=0.6, beta=0.15, gamma=0.25, rho=2., q=0.5, o=0.5)
PART_NAMES = ("num", "den", "sum vs", "sum gm", "min vs_m", "max vs_m")
QUANTITY = ("sums", "sums", "sums", "sums", "limits", "limits")          # the quantity class of each part (the fixture's spread)

# (B, H, W, inputs, VSI options, MDSI options).  Upsampling into SDSP, k = 1, a batch of two; not square, no power of two; 64 x 64;
# 128 x 96; downsampling with a non-integer ratio; k = 2 from 1.504 with an odd side (both pad rules); k = 2 from the half-to-even
# 1.5; k = 3; every option off its default (MDSI: 'mult'); a constant image pair; a source with negative gs_total (MDSI).
CASES = ((2, 16, 16, "noise", DEFAULTS, MDSI_DEFAULTS), (1, 24, 40, "noise", DEFAULTS, MDSI_DEFAULTS), (1, 64, 64, "noise", DEFAULTS, MDSI_DEFAULTS),
         (1, 128, 96, "noise", DEFAULTS, MDSI_DEFAULTS), (1, 300, 500, "noise", DEFAULTS, MDSI_DEFAULTS), (1, 385, 400, "noise", DEFAULTS, MDSI_DEFAULTS),
         (1, 384, 512, "noise", DEFAULTS, MDSI_DEFAULTS), (1, 641, 648, "noise", DEFAULTS, MDSI_DEFAULTS), (1, 48, 80, "noise", OTHER, MDSI_OTHER),
         (1, 64, 64, "constant", DEFAULTS, MDSI_DEFAULTS), (1, 64, 64, "faint", DEFAULTS, MDSI_DEFAULTS))
CONSTANT, FAINT = 9, 10


def kernel_size(H, W):
    """The pooling kernel: Python's round, half to even (384 -> 2, 640 -> 2, 641 -> 3)."""
    return max(1, round(min(H, W) / 256))


def case_inputs(index):
    """(input, target, pred) of case `index`: contiguous float32 (B, 1, H, W).  "noise": the target is uniform noise under three
    5 x 5 box filters, stretched to [0.05, 0.95] per image; input = target + N(0, 0.08^2), pred = target + N(0, 0.02^2), clipped to
    [0, 1].  "constant": input and pred 0.5, target 0.25 everywhere.  "faint": the target is the uniform noise itself
    (steep), the input the target at a fiftieth of its contrast around 0.5: a nearly flat source against a textured target, where
    MDSI's gs_total is negative at most pixels."""
    B, H, W, kind = CASES[index][:4]
    if kind == "constant":
        half = torch.full((B, 1, H, W), 0.5)
        return half, torch.full((B, 1, H, W), 0.25), half.clone()
    g = torch.Generator().manual_seed(2100 + index)
    z = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
    box = torch.full((1, 1, 5, 5), 1.0 / 25.0, dtype=torch.float64)
    for _ in range(0 if kind == "faint" else 3):
        z = F.conv2d(F.pad(z, (2, 2, 2, 2), mode="replicate"), box)
    lo, hi = z.amin(dim=(1, 2, 3), keepdim=True), z.amax(dim=(1, 2, 3), keepdim=True)
    y = 0.05 + 0.9 * (z - lo) / (hi - lo)
    x = (y + 0.08 * torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    pred = (y + 0.02 * torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    if kind == "faint":
        x = 0.5 + 0.02 * (y - 0.5)
    return x.float().contiguous(), y.float().contiguous(), pred.float().contiguous()


def crc(*tensors):
    c = 0
    for t in tensors:
        c = zlib.crc32(t.contiguous().numpy().tobytes(), c)
    return c


def _f32(values, like):
    """Constants the reference keeps as float32 tensors, in the dtype of `like`."""
    return torch.tensor(values, dtype=torch.float32).to(like)


def _grey_through(matrix, v):
    """The three output channels of a 3 x 3 colour matrix applied to the grey image v (three equal channels)."""
    m = _f32(matrix, v)
    return [v * m[j, 0] + v * m[j, 1] + v * m[j, 2] for j in range(3)]


def grey_to_lab(v):
    """v: grey values in [0, 255] -> (L, a, b): sRGB decoding, the D65 RGB -> XYZ matrix, the D50 white of the 2 degree
    observer, the CIE cube-root curve with its linear piece below 0.008856."""
    t = v / 255
    lin = torch.where(t <= 0.04045, t / 12.92, ((t + 0.055) / 1.055) ** 2.4)
    xyz = _grey_through([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]], lin)
    white = _f32([0.9642119944211994, 1.0, 0.8251882845188288], v)
    fx, fy, fz = (torch.where(c / white[j] > 0.008856, (c / white[j]) ** (1.0 / 3.0), (903.3 * (c / white[j]) + 16.0) / 116.0)
                  for j, c in enumerate(xyz))
    return 116.0 * fy - 16.0, 500.0 * fx - 500.0 * fy, 200.0 * fy - 200.0 * fz


def _centred_axis(n):
    """The n sample positions of an even axis centred on zero, in units of the axis length, float32: -1/2 .. 1/2 - 1/n."""
    return torch.arange(-n / 2, n / 2) / n


def log_gabor_table(omega_0=0.021, sigma_f=1.34):
    """SDSP's (256, 256) float32 log-Gabor filter, zero frequency at [0, 0]: built on the centred frequency grid, cut off
    beyond radius 1/2, rolled so that the zero frequency comes first, the zero frequency itself set to zero.  Every element goes
    through the reference's float32 operations in the reference's order (the fixture holds the CRC of the reference's table)."""
    f = _centred_axis(SIDE)
    rho = torch.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
    rho = torch.roll(rho * (rho <= 0.5), (-(SIDE // 2), -(SIDE // 2)), (0, 1))
    rho[0, 0] = 1
    table = torch.exp(-torch.log(rho / omega_0) ** 2 / (2 * sigma_f ** 2))
    table[0, 0] = 0
    return table


def saliency(v, size, omega_0=0.021, sigma_f=1.34, sigma_d=145., sigma_c=0.001):
    """SDSP of the grey images v (B, 1, H, W) in [0, 255] -> (the saliency map at `size` stretched to [0, 1], its minimum and
    maximum before the stretch, each (B,))."""
    eps = torch.finfo(v.dtype).eps
    small = F.interpolate(v, size=(SIDE, SIDE), mode="bilinear", align_corners=False)
    lab = torch.cat(grey_to_lab(small), dim=1)                                       # (B, 3, 256, 256)
    band = torch.fft.ifft2(torch.fft.fft2(lab) * log_gabor_table(omega_0, sigma_f).to(v)).real
    frequency_prior = torch.sqrt((band ** 2).sum(dim=1, keepdim=True))
    c = (_centred_axis(SIDE) * SIDE + 1).to(v)                                       # the reference's pixel coordinates: -127 .. 128
    centre_prior = torch.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / sigma_d ** 2)
    lo, hi = lab.amin(dim=(2, 3), keepdim=True), lab.amax(dim=(2, 3), keepdim=True)
    stretched = (lab - lo) / (hi - lo + eps)
    warm_prior = 1 - torch.exp(-(stretched[:, 1:] ** 2).sum(dim=1, keepdim=True) / sigma_c ** 2)
    vs = F.interpolate(frequency_prior * centre_prior * warm_prior, size=size, mode="bilinear", align_corners=True)
    lo, hi = vs.amin(dim=(2, 3), keepdim=True), vs.amax(dim=(2, 3), keepdim=True)
    return (vs - lo) / (hi - lo + eps), lo.flatten(), hi.flatten()


def pool(x, k, before, after, mode):
    """Pad `before` / `after` pixels on both axes in `mode`, then average k x k blocks (stride k, floor)."""
    if k > 1:
        x = F.pad(x, [before, after, before, after], mode=mode)
    return F.avg_pool2d(x, k)


def scharr_map(x):
    """Magnitude of the horizontal and vertical Scharr derivatives (weights 3, 10, 3 over 16), zero padding."""
    smooth, diff = torch.tensor([3., 10., 3.]).to(x) / 16, torch.tensor([-1., 0., 1.]).to(x)
    g = F.conv2d(x, torch.stack([torch.outer(smooth, diff), torch.outer(diff, smooth)])[:, None], padding=1)
    return torch.sqrt(g[:, :1] ** 2 + g[:, 1:] ** 2)


def similarity(a, b, c):
    return (2.0 * a * b + c) / (a ** 2 + b ** 2 + c)


def real_part_of_power(s, e):
    """Re(s^e) of real s on the principal branch: |s|^e cos(e arg s), arg s = pi for negative s."""
    return s.abs() ** e * torch.cos(e * torch.atan2(torch.zeros_like(s), s))


def check(a, b):
    if a.dim() != 4 or a.shape != b.shape or a.shape[1] != 1:
        raise AssertionError("two (B,1,H,W) tensors of one shape expected")


def vsi(a, b, c1=1.27, c2=386., c3=130., alpha=0.4, beta=0.02, omega_0=0.021, sigma_f=1.34, sigma_d=145., sigma_c=0.001):
    """-> (score (B,), parts (B, 6)) of a against the target b, in the dtype of a."""
    check(a, b)
    eps = torch.finfo(a.dtype).eps
    a, b = a * 255, b * 255
    size = a.shape[2:]
    k = kernel_size(*size)
    (vs_a, lo_a, hi_a), (vs_b, _, _) = (saliency(t, size, omega_0, sigma_f, sigma_d, sigma_c) for t in (a, b))
    pooled = lambda t: pool(t, k, k // 2, (k - 1) // 2, "replicate")          # noqa: E731
    vs_a, vs_b = pooled(vs_a), pooled(vs_b)
    lmn = [[0.06, 0.63, 0.27], [0.30, 0.04, -0.35], [0.34, -0.6, 0.17]]
    (l_a, m_a, n_a), (l_b, m_b, n_b) = ([pooled(c) for c in _grey_through(lmn, t)] for t in (a, b))
    gm_a, gm_b = scharr_map(l_a), scharr_map(l_b)
    colour = real_part_of_power(similarity(m_a, m_b, c3) * similarity(n_a, n_b, c3), beta)
    s = similarity(vs_a, vs_b, c1) * similarity(gm_a, gm_b, c2) ** alpha * colour
    weight = torch.maximum(vs_a, vs_b)
    num, den = (s * weight).sum(dim=[1, 2, 3]), weight.sum(dim=[1, 2, 3])
    parts = torch.stack([num, den, vs_a.sum(dim=[1, 2, 3]), gm_a.sum(dim=[1, 2, 3]), lo_a, hi_a], dim=1)
    return (num + eps) / (den + eps), parts
