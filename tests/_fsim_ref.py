"""Restatement of the feature similarity index the test loop takes from the reference's module/piq (fsim.py: fsim with
chromatic=False, data_range 1) for single-channel images in [0, 1], in plain torch ops on whatever dtype and device the inputs
have (float64 on the CPU for the tests' reference values, float32 on the GPU for tools/fsim_timing.py's torch-op form), with
torch.fft where the reference calls the removed torch.rfft / torch.ifft.
`fsim` returns (score (B,), parts (B, 4 + orientations)); the parts are laid out as the kernels' `parts`: num = sum GM PC pc_max,
den = sum pc_max, the sum of the source's phase-congruency map, the sum of its gradient-magnitude map, then the source's noise
thresholds T_0 .. T_{O-1}.

Written from reading the reference, in this project's own terms: the responses are complex tensors (even = real, odd =
imaginary part), the thresholds come in the (B, O) form the kernels use.  A float64 run differs from the reference's float64 run
in the order of its operations alone (tests/test_fsim_cpu.py: 1e-11); eps is the dtype's, as in the reference.  Only the filter
table keeps the reference's float32 operation order element by element, because the reference builds it in float32 even in a
float64 run: its bytes are those of the reference's table (the fixture holds their CRC-32 per case).

CASES / case_inputs: the shapes and seeded inputs shared by tools/pin_fsim.py (which writes tests/golden/fsim_piq.npz from the
reference itself) and the tests."""
import math
import os
import zlib

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fsim_piq.npz")
MIN_SIDE, MAX_SIDE = 16, 512                                    # of the pooled map, each a power of two (the kernels' lengths)
DEFAULTS = dict(scales=4, orientations=4, min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2, k=2.0)
OTHER = dict(scales=3, orientations=6, min_length=4, mult=3, sigma_f=0.6, delta_theta=1.5, k=1.5)
T1, T2 = 0.85, 160

# (B, H, W, options): the shortest length and a batch of two; row and column lengths that differ, both ways; the training patch;
# a 512-long column with ks = 1; ks = 2 and ks = 3; options other than the defaults.
CASES = ((2, 16, 16, DEFAULTS), (1, 32, 32, DEFAULTS), (1, 32, 64, DEFAULTS), (1, 64, 32, DEFAULTS), (1, 16, 128, DEFAULTS),
         (2, 64, 64, DEFAULTS), (1, 128, 256, DEFAULTS), (1, 256, 256, DEFAULTS), (1, 512, 256, DEFAULTS), (1, 512, 512, DEFAULTS),
         (1, 1536, 768, DEFAULTS), (1, 64, 64, OTHER))


def part_names(orientations):
    return ("num", "den", "sum pc", "sum gm") + tuple(f"T_{o}" for o in range(orientations))


def case_inputs(index):
    """(input, target, pred) of case `index`: contiguous float32 (B, 1, H, W).  The target is uniform noise under three 5 x 5 box
    filters, stretched to [0.05, 0.95] per image; input = target + N(0, 0.08^2), pred = target + N(0, 0.02^2), clipped to [0, 1]."""
    B, H, W = CASES[index][:3]
    g = torch.Generator().manual_seed(1700 + index)
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


def pooled_size(H, W):
    """-> (ks, h, w): the reference's average-pool kernel (Python's round: 384 -> 2, 640 -> 2) and the pooled map's sides."""
    ks = max(1, round(min(H, W) / 256))
    return ks, H // ks, W // ks


def _signed_bins(n):
    """Frequency bin numbers of an n-point transform in storage order, zero first: 0 .. then the negative ones (the reference's
    centred axis, (i - n / 2) / n for even n and (i - (n - 1) / 2) / (n - 1) for odd n, rolled back by n // 2)."""
    i = torch.arange(n)
    centred = (i - n // 2).float() / n if n % 2 == 0 else (i.float() - (n - 1) / 2) / (n - 1)
    return torch.roll(centred, -(n // 2))


def _band(rho, wavelength, sigma_f):
    """Log-Gabor radial profile of one scale on the radius map rho (rho[0, 0] already 1)."""
    centre = 1.0 / wavelength
    return torch.exp(-torch.log(rho / centre) ** 2 / (2 * math.log(sigma_f) ** 2))


def _wedge(phi_sin, phi_cos, angle, width):
    """Angular Gaussian of one orientation: the angle between each frequency's direction and `angle`, from the sine and the
    cosine of the difference so that it does not wrap."""
    off = torch.atan2(phi_sin * math.cos(angle) - phi_cos * math.sin(angle), phi_cos * math.cos(angle) + phi_sin * math.sin(angle))
    return torch.exp(-off.abs() ** 2 / (2 * width ** 2))


def filter_table(h, w, scales=4, orientations=4, min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2):
    """The (orientations * scales, h, w) float32 table of log-Gabor filters, orientation-major, zero frequency at [0, 0].  Every
    element goes through the reference's float32 operations in the reference's order (tests/golden/fsim_piq.npz holds the CRC
    of the reference's own table per case), loop by loop over the scales and the orientations."""
    v, u = torch.meshgrid(_signed_bins(h), _signed_bins(w), indexing="ij")          # vertical, horizontal frequency
    rho = torch.sqrt(v ** 2 + u ** 2)
    smooth = 1.0 / (1.0 + (rho / 0.45) ** 30)                                         # Butterworth low-pass, order 15
    phi = torch.atan2(-u, v)
    rho[0, 0] = 1                                                                     # (the log of the radius at zero frequency)
    phi_sin, phi_cos = phi.sin(), phi.cos()
    table = torch.empty(orientations, scales, h, w)
    for o in range(orientations):
        wedge = _wedge(phi_sin, phi_cos, o * math.pi / orientations, math.pi / (orientations * delta_theta))
        for s in range(scales):
            band = _band(rho, min_length * mult ** s, sigma_f) * smooth
            band[0, 0] = 0
            table[o, s] = wedge * band
    return table.view(orientations * scales, h, w)


def noise_constants(bank):
    """(3, O) from the (O, S, h, w) filter bank: the power of the finest filter, and of the bank's spatial kernels (real part of
    the inverse transform, scaled by sqrt(h w)) the summed squares and the summed products of every pair of scales."""
    O, S, h, w = bank.shape
    kernels = torch.fft.ifft2(bank).real * math.sqrt(h * w)
    squares = (kernels ** 2).sum(dim=(1, 2, 3))
    pairs = sum(((kernels[:, s] * kernels[:, t]).sum(dim=(1, 2)) for s in range(S) for t in range(s + 1, S)), torch.zeros(O).to(bank))
    return torch.stack([(bank[:, 0] ** 2).sum(dim=(1, 2)), squares, pairs])


def phase_congruency(x, scales=4, orientations=4, min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2, k=2.0):
    """-> (pc (B, 1, h, w), T (B, orientations)) of the pooled, 255-scaled images x (B, 1, h, w).  Complex arithmetic: the even
    and odd responses are the real and imaginary parts of `resp`."""
    eps = torch.finfo(x.dtype).eps
    B, _, h, w = x.shape
    bank = filter_table(h, w, scales, orientations, min_length, mult, sigma_f, delta_theta).to(x).view(orientations, scales, h, w)
    resp = torch.fft.ifft2(torch.fft.fft2(x).unsqueeze(2) * bank)                    # (B, O, S, h, w)
    amp = resp.abs()
    mean = resp.sum(dim=2, keepdim=True)                                              # the summed response vector of an orientation ...
    mean = mean / (mean.abs() + eps)                                                  # ... as a direction
    along = resp * mean.conj()                                                        # real: along the mean direction, imaginary: across it
    energy = (along.real - along.imag.abs()).sum(dim=2)                               # (B, O, h, w)
    power, squares, pairs = noise_constants(bank)
    median = (amp[:, :, 0] ** 2).flatten(2).median(dim=2).values                      # (B, O): the lower middle value
    tau = torch.sqrt((median / math.log(2)) / power * (squares + 2 * pairs))          # Rayleigh parameter of the noise energy
    T = tau * (math.sqrt(math.pi / 2) + k * math.sqrt(2 - math.pi / 2)) / 1.7
    above = (energy - T[:, :, None, None]).clamp_min(0)
    pc = (above.sum(dim=1) + eps) / (amp.sum(dim=(1, 2)) + eps)
    return pc.unsqueeze(1), T


def gradient_map(x):
    """Magnitude of the horizontal and vertical Scharr derivatives (weights 3, 10, 3 over 16), zero padding."""
    smooth, diff = torch.tensor([3., 10., 3.]).to(x) / 16, torch.tensor([-1., 0., 1.]).to(x)
    across, down = torch.outer(smooth, diff), torch.outer(diff, smooth)
    g = F.conv2d(x, torch.stack([across, down])[:, None], padding=1)
    return torch.hypot(g[:, :1], g[:, 1:])


def _similarity(a, b, c):
    return (2.0 * a * b + c) / (a ** 2 + b ** 2 + c)


def _check(a, b):
    if a.dim() != 4 or a.shape != b.shape or a.shape[1] != 1:
        raise AssertionError("fsim: two (B,1,H,W) tensors of one shape expected")


def fsim(a, b, scales=4, orientations=4, min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2, k=2.0):
    """-> (score (B,), parts (B, 4 + orientations)) of a against the target b, in the dtype of a."""
    _check(a, b)
    ks = pooled_size(a.shape[2], a.shape[3])[0]
    a, b = (F.avg_pool2d(t * 255, ks) for t in (a, b))
    opts = dict(scales=scales, orientations=orientations, min_length=min_length, mult=mult, sigma_f=sigma_f, delta_theta=delta_theta, k=k)
    (pc_a, T_a), (pc_b, _) = phase_congruency(a, **opts), phase_congruency(b, **opts)
    gm_a, gm_b = gradient_map(a), gradient_map(b)
    weight = torch.maximum(pc_a, pc_b)
    num = (_similarity(gm_a, gm_b, T2) * _similarity(pc_a, pc_b, T1) * weight).sum(dim=[1, 2, 3])
    den = weight.sum(dim=[1, 2, 3])
    parts = torch.cat([torch.stack([num, den, pc_a.sum(dim=[1, 2, 3]), gm_a.sum(dim=[1, 2, 3])], dim=1), T_a], dim=1)
    return num / den, parts
