"""Restatement of the two no-reference statistics the test loop takes from the reference's module/piq (brisque.py: brisque,
tv.py: total_variation; data_range 1) for single-channel images in [0, 1], in plain torch ops on whatever dtype and device the
inputs have (float64 on the CPU for the tests' reference values, float32 on the GPU for tools/brisque_tv_timing.py's torch-op
form).  Written from the formulas, in this project's own terms.

`brisque` returns (score (B,), features (B, 36), indices (B, 10), values (B, 10)): the features before the range scaling in the
kernels' order (per scale alpha, sigma^2, then for the shifts (0,1), (1,0), (1,1), (-1,1) alpha, eta, sigma_l^2, sigma_r^2); the
ten table positions behind the alpha features (per scale the GGD's, then the four AGGD's) and the values that were looked up.
Unlike the reference it does not assert: an image whose MSCN map has no variance, or a product map without values of both signs,
comes out as NaN (the kernels' rule).

CASES / case_inputs / case_svm: the shapes, seeded inputs and seeded support vector regressions shared by tools/pin_brisque_tv.py
(which writes tests/golden/brisque_tv_piq.npz from the reference itself) and the tests."""
import math
import os
import zlib

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brisque_tv_piq.npz")
MIN_SIDE, MAX_SIDE = 16, 1024
PARTS = 37
ALPHA_AT = (0, 2, 6, 10, 14, 18, 20, 24, 28, 32)                # the features that are table values, in the order of the look-ups
ETA_AT = (3, 7, 11, 15, 21, 25, 29, 33)
SIGMA_AT = tuple(j for j in range(36) if j not in ALPHA_AT + ETA_AT)
SHIFTS = ((0, 1), (1, 0), (1, 1), (-1, 1))
NORMS = ("l1", "l2", "l2_squared")
KINDS = ("texture", "smooth", "uniform")                        # what (input, target, pred) hold in every case

# (B, H, W, options, n_sv).  The minimum side (the second scale is 8 x 8, barely larger than the 7 x 7 filter); odd and
# rectangular (the nearest rule, the wrap of the rolls); a 3 x 3 filter; a 9 x 9 filter with another sigma; more than one tile per
# axis with a ragged edge; the loop's own shape.
CASES = ((3, 16, 16, {}, 1), (2, 17, 23, {}, 64), (1, 33, 40, dict(kernel_size=3), 774), (3, 64, 64, dict(kernel_size=9, kernel_sigma=1.5), 1),
         (2, 96, 131, {}, 64), (1, 512, 512, {}, 774))

# the feature ranges of the range scaling (the MATLAB implementation's), held in float32 as the reference holds them
RANGES = ((0.338, 10), (0.017204, 0.806612), (0.236, 1.642), (-0.123884, 0.20293), (0.000155, 0.712298), (0.001122, 0.470257),
          (0.244, 1.641), (-0.123586, 0.179083), (0.000152, 0.710456), (0.000975, 0.470984), (0.249, 1.555), (-0.135687, 0.100858),
          (0.000174, 0.684173), (0.000913, 0.534174), (0.258, 1.561), (-0.143408, 0.100486), (0.000179, 0.685696), (0.000888, 0.536508),
          (0.471, 3.264), (0.012809, 0.703171), (0.218, 1.046), (-0.094876, 0.187459), (1.5e-005, 0.442057), (0.001272, 0.40803),
          (0.222, 1.042), (-0.115772, 0.162604), (1.6e-005, 0.444362), (0.001374, 0.40243), (0.227, 0.996),
          (-0.117188, 0.09832299999999999), (3e-005, 0.531903), (0.001122, 0.369589), (0.228, 0.99), (-0.12243, 0.098658),
          (2.8e-005, 0.530092), (0.001118, 0.370399))


def crc(*tensors):
    """CRC-32 of the tensors' bytes, one after the other."""
    c = 0
    for t in tensors:
        c = zlib.crc32(t.contiguous().numpy().tobytes(), c)
    return c


def case_inputs(index):
    """(input, target, pred) of case `index`: contiguous float32 (B, 1, H, W) in [0, 1].  input: a noisy texture (uniform noise
    under three 5 x 5 box filters, stretched to [0.05, 0.95] per image, plus N(0, 0.08^2)); target: nearly smooth (another such
    field in [0.2, 0.8] plus N(0, 0.003^2)); pred: uniform noise."""
    B, H, W = CASES[index][:3]
    g = torch.Generator().manual_seed(3100 + index)
    box = torch.full((1, 1, 5, 5), 1.0 / 25.0, dtype=torch.float64)

    def field(lo, hi):
        z = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
        for _ in range(3):
            z = F.conv2d(F.pad(z, (2, 2, 2, 2), mode="replicate"), box)
        a, b = z.amin(dim=(1, 2, 3), keepdim=True), z.amax(dim=(1, 2, 3), keepdim=True)
        return lo + (hi - lo) * (z - a) / (b - a)
    x = (field(0.05, 0.95) + 0.08 * torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    y = (field(0.2, 0.8) + 0.003 * torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    pred = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
    return x.float().contiguous(), y.float().contiguous(), pred.float().contiguous()


def seeded_svm(n_sv, seed):
    """(sv_coef (n_sv, 1), sv (n_sv, 36)) in float64: support vectors uniform in [-1, 1], coefficients N(0, 4^2) of both signs."""
    g = torch.Generator().manual_seed(seed)
    sv = 2 * torch.rand(n_sv, 36, generator=g, dtype=torch.float64) - 1
    coef = 4 * torch.randn(n_sv, 1, generator=g, dtype=torch.float64)
    if n_sv > 1:
        coef[0], coef[1] = coef[0].abs(), -coef[1].abs()
    return coef, sv


def case_svm(index):
    return seeded_svm(CASES[index][4], 4100 + index)


def gaussian_taps(kernel_size, kernel_sigma):
    """The (k, k) float32 filter, normalised in two dimensions, float32 at every step."""
    c = torch.arange(kernel_size).to(dtype=torch.float32)
    c -= (kernel_size - 1) / 2.
    sq = c ** 2
    t = (-(sq.unsqueeze(0) + sq.unsqueeze(1)) / (2 * kernel_sigma ** 2)).exp()
    t /= t.sum()
    return t


def shape_tables(like):
    """(gamma, the GGD r_table, the AGGD r_table) in the dtype and on the device of `like`; the grid is built in float32 first."""
    gamma = torch.arange(0.2, 10.001, 0.001).to(like)
    one, two, three = torch.lgamma(1. / gamma), torch.lgamma(2. / gamma), torch.lgamma(3. / gamma)
    return gamma, (one + three - 2 * two).exp(), torch.exp(2 * two - one - three)


def _scene_statistics(img, taps, tables):
    """The 18 features, five table positions and five looked-up values of one scale: (B, 18), (B, 5), (B, 5)."""
    gamma, r_ggd, r_aggd = tables
    k = taps.shape[-1]
    mu = F.conv2d(img, taps, padding=k // 2)
    second = F.conv2d(img ** 2, taps, padding=k // 2)
    n = (img - mu) / ((second - mu ** 2).abs().sqrt() + 1)
    n = n[:, 0]                                                           # (B, h, w)
    nan = torch.full_like(n[:, 0, 0], float("nan"))
    mean_sq = n.pow(2).mean(dim=(-1, -2))
    sigma = mean_sq.sqrt()
    rho = mean_sq / n.abs().mean(dim=(-1, -2)) ** 2
    rho = torch.where(sigma > 1e-8, rho, nan)
    feats, where, values = [], [], []

    def look_up(v, table):
        at = (v[:, None] - table[None, :]).abs().argmin(dim=-1)
        at = torch.where(torch.isnan(v), torch.zeros_like(at), at)
        where.append(at)
        values.append(v)
        return torch.where(torch.isnan(v), v, gamma[at])
    feats += [look_up(rho, r_ggd), sigma.pow(2)]
    for shift in SHIFTS:
        p = n * torch.roll(n, shifts=shift, dims=(-2, -1))
        neg, pos = p < 0, p > 0
        count_l, count_r = neg.sum(dim=(-1, -2)).to(p), pos.sum(dim=(-1, -2)).to(p)
        sigma_l = ((p * neg).pow(2).sum(dim=(-1, -2)) / count_l).sqrt()
        sigma_r = ((p * pos).pow(2).sum(dim=(-1, -2)) / count_r).sqrt()
        ok = (count_l > 0) & (count_r > 0) & (sigma_l > 0) & (sigma_r > 0)
        ratio = sigma_l / sigma_r
        r_hat = p.abs().mean(dim=(-1, -2)).pow(2) / p.pow(2).mean(dim=(-1, -2))
        r_norm = torch.where(ok, (r_hat * (ratio.pow(3) + 1) * (ratio + 1)) / (ratio.pow(2) + 1).pow(2), nan)
        alpha = look_up(r_norm, r_aggd)
        eta = (sigma_r - sigma_l) * torch.exp(torch.lgamma(2. / alpha) - (torch.lgamma(1. / alpha) + torch.lgamma(3. / alpha)) / 2)
        feats += [alpha, eta, sigma_l.pow(2), sigma_r.pow(2)]
    return torch.stack(feats, dim=-1), torch.stack(where, dim=-1), torch.stack(values, dim=-1)


def score_of(features, coef, sv):
    """The range scaling and the support vector regression on (B, 36) features."""
    ranges = torch.tensor(RANGES).to(features)                            # float32 first, as the reference holds them
    scaled = -1 + 2 * (features - ranges[:, 0]) / (ranges[:, 1] - ranges[:, 0])
    dist = (scaled[:, None, :] - sv.to(features)[None, :, :]).pow(2).sum(dim=-1)
    return torch.exp(-dist * 0.05) @ coef.to(features).reshape(-1) + 153.591


def brisque(x, coef, sv, kernel_size=7, kernel_sigma=7 / 6):
    """x: (B, 1, H, W) in [0, 1].  -> (score (B,), features (B, 36), indices (B, 10), values (B, 10)); NaN rows where the
    reference would assert."""
    taps = gaussian_taps(kernel_size, kernel_sigma).view(1, 1, kernel_size, kernel_size).to(x)
    tables = shape_tables(x)
    img = x * 255
    per_scale = []
    for scale in range(2):
        per_scale.append(_scene_statistics(img, taps, tables))
        img = F.interpolate(img, size=(img.shape[2] // 2, img.shape[3] // 2), mode="nearest")
    features, where, values = (torch.cat([a[j] for a in per_scale], dim=-1) for j in range(3))
    score = score_of(features, coef, sv)
    failed = torch.isnan(features).any(dim=-1)
    nan = torch.full_like(score, float("nan"))
    return torch.where(failed, nan, score), torch.where(failed[:, None], nan[:, None], features), where, values


def total_variation(x, norm_type="l2"):
    """x: (B, 1, H, W).  -> (B,)."""
    dx, dy = x[:, :, :, 1:] - x[:, :, :, :-1], x[:, :, 1:, :] - x[:, :, :-1, :]
    if norm_type == "l1":
        return dy.abs().sum(dim=(1, 2, 3)) + dx.abs().sum(dim=(1, 2, 3))
    total = dy.pow(2).sum(dim=(1, 2, 3)) + dx.pow(2).sum(dim=(1, 2, 3))
    if norm_type == "l2":
        return total.sqrt()
    assert norm_type == "l2_squared", norm_type
    return total


def nearest_index(size):
    """The source index of every destination index of the half-size `nearest` resample: min(floor(dst * scale), size - 1) with
    scale = size / (size // 2) in float32."""
    import numpy as np
    half = size // 2
    scale = np.float32(size) / np.float32(half)
    return [min(int(math.floor(np.float32(d) * scale)), size - 1) for d in range(half)]
