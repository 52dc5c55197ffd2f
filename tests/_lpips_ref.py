"""Restatement of LPIPS and DISTS as the test loop takes them from the reference's module/piq (perceptual.py: LPIPS, DISTS on
torchvision's VGG-16 `features`, single-channel images in [0, 1]) in plain torch ops, in the dtype it is asked for (float64 on
the CPU for the tests' reference values, float32 on the GPU for tools/lpips_timing.py's torch-op form).  It does not import the
reference; tools/pin_lpips.py pins the reference's own numbers in tests/golden/lpips_dists_piq.npz and tests/test_lpips_cpu.py
holds this file to them.

  features(sd, x, pool)     the five NCHW maps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of the grey image broadcast against the
                            ImageNet constants, with nn.MaxPool2d(2, 2) ("max") or DISTS's L2 pooling ("l2")
  l2pool(x)                 sqrt(hann3x3 * x^2 + 1e-12), stride 2, padding 1
  lpips_level(fo, ft, w)    sum over channels and pixels of w_c d(fo_c / (|fo| + 1e-10), ft_c / (|ft| + 1e-10)), per image
  moments(ft, fo...)        the per-image, per-channel sums the kernels tabulate
  dists_finish(...)         DISTS's closing formula from such tables
  lpips / dists             the per-image scores and per-level parts

CASES / case_inputs / seeded_*: the shapes, seeded inputs and seeded weights shared by tools/pin_lpips.py and the tests; the
weights are regenerated from the seed, never stored."""
import math
import os
import zlib

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_dists_piq.npz")
# torchvision vgg16().features: (index, C_in, C_out) of every conv; pools at 4, 9, 16, 23; taps after the ReLUs at 3, 8, 15, 22, 29
CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
         (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
POOLS = (4, 9, 16, 23)
TAPS = (3, 8, 15, 22, 29)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
LPIPS_CHANNELS = (64, 128, 256, 512, 512)
DISTS_CHANNELS = (3, 64, 128, 256, 512, 512)

# (B, H, W, distance): a batch of two with sides that pool evenly; odd sides (37 -> 19 -> 10 -> 5 -> 3 with the L2 pool, 18 -> 9 -> 4
# -> 2 with the max pool); the smallest side with an odd one; the mae distance.
CASES = ((2, 48, 40, "mse"), (1, 50, 37, "mse"), (2, 16, 17, "mse"), (1, 32, 24, "mae"))


def case_inputs(index):
    """(input, target, pred) of case `index`: contiguous float32 (B, 1, H, W).  The target is uniform noise under two 3 x 3 box
    filters, stretched to [0.05, 0.95] per image; input = target + N(0, 0.08^2), pred = target + N(0, 0.02^2), clipped to [0, 1]."""
    B, H, W = CASES[index][:3]
    g = torch.Generator().manual_seed(1800 + index)
    z = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
    box = torch.full((1, 1, 3, 3), 1.0 / 9.0, dtype=torch.float64)
    for _ in range(2):
        z = F.conv2d(F.pad(z, (1, 1, 1, 1), mode="replicate"), box)
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


def seeded_state_dict(seed=0):
    """A torchvision-layout VGG-16 state dict with He-normal weights (std = sqrt(2 / (9 C_in))) and N(0, 0.05) biases; one
    classifier entry stands for the keys the product side must ignore."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cin, cout in CONVS:
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"features.{idx}.bias"] = torch.randn(cout, generator=g) * 0.05
    sd["classifier.0.bias"] = torch.zeros(8)
    return sd


def seeded_lpips_weights(seed=1):
    """Five (1, C, 1, 1) float32 tensors drawn uniformly from [0, 1 / C): non-negative, as LPIPS's learned weights are."""
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(1, c, 1, 1, generator=g) / c for c in LPIPS_CHANNELS]


def seeded_dists_weights(seed=2):
    """{'alpha', 'beta'}: (1, 1475, 1, 1) float32 each, positive, normalised so that sum(alpha) + sum(beta) = 1 (up to rounding)."""
    g = torch.Generator().manual_seed(seed)
    n = sum(DISTS_CHANNELS)
    a, b = torch.rand(n, generator=g, dtype=torch.float64) + 0.1, torch.rand(n, generator=g, dtype=torch.float64) + 0.1
    total = a.sum() + b.sum()
    return {"alpha": (a / total).float().view(1, n, 1, 1), "beta": (b / total).float().view(1, n, 1, 1)}


def l2pool(x):
    """(B, C, H, W) -> (B, C, ceil(H/2), ceil(W/2))."""
    k = torch.tensor([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]], dtype=x.dtype, device=x.device) / 16.0
    C = x.shape[1]
    out = F.conv2d(x * x, k.expand(C, 1, 3, 3), stride=2, padding=1, groups=C)
    return (out + 1e-12).sqrt()


def normalised(x, dtype=torch.float64):
    """The grey (B, 1, H, W) image as the three ImageNet-normalised channels.  The constants are float32 numbers in every dtype,
    as the reference holds them (torch.tensor(mean) of a list of Python floats, cast to the image's dtype afterwards)."""
    mean = torch.tensor(MEAN, dtype=torch.float32, device=x.device).to(dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32, device=x.device).to(dtype).view(1, 3, 1, 1)
    return (x.to(dtype) - mean) / std


def features(sd, x, pool="max", dtype=torch.float64):
    """x: (B, 1, H, W).  The five NCHW maps."""
    t = normalised(x, dtype)
    convs = {idx: (sd[f"features.{idx}.weight"].to(t), sd[f"features.{idx}.bias"].to(t)) for idx, _, _ in CONVS}
    maps = []
    for idx in range(29):
        if idx in convs:
            t = F.relu(F.conv2d(t, convs[idx][0], convs[idx][1], padding=1))      # (the ReLU of index idx + 1)
            if idx + 1 in TAPS:
                maps.append(t)
        elif idx in POOLS:
            t = F.max_pool2d(t, 2, 2) if pool == "max" else l2pool(t)
    return maps


def lpips_level(fo, ft, w, distance="mse"):
    """fo, ft: (B, C, h, w); w: C weights.  (B,) sums over channels and pixels (the spatial mean is this over h * w)."""
    no = fo / (torch.sqrt((fo * fo).sum(dim=1, keepdim=True)) + 1e-10)
    nt = ft / (torch.sqrt((ft * ft).sum(dim=1, keepdim=True)) + 1e-10)
    d = (no - nt) ** 2 if distance == "mse" else (no - nt).abs()
    return (d * w.to(d).view(1, -1, 1, 1)).sum(dim=(1, 2, 3))


def lpips(sd, weights, a, y, distance="mse", dtype=torch.float64):
    """-> (score (B,), parts (B, 5)): parts are the per-level spatial means summed over the channels."""
    fa, fy = features(sd, a, "max", dtype), features(sd, y, "max", dtype)
    parts = torch.stack([lpips_level(o, t, w.flatten(), distance) / (t.shape[2] * t.shape[3]) for o, t, w in zip(fa, fy, weights)], dim=1)
    return parts.sum(dim=1), parts


def moments(ft, *others):
    """ft, others: (B, C, h, w) -> (B, C, 2 + 3 n): (sum t, sum t^2) and per other map (sum o, sum o^2, sum o t) over the pixels."""
    cols = [ft.sum(dim=(2, 3)), (ft * ft).sum(dim=(2, 3))]
    for fo in others:
        cols += [fo.sum(dim=(2, 3)), (fo * fo).sum(dim=(2, 3)), (fo * ft).sum(dim=(2, 3))]
    return torch.stack(cols, dim=2)


def dists_finish(tables, pixels, alpha, beta, other=0):
    """tables: six (B, C, K) moment tables (C = 1, 64, 128, 256, 512, 512); alpha, beta: 1475 entries each.
    -> (score (B,), parts (B, 6)) for other map `other`."""
    alpha, beta = alpha.flatten().to(tables[0]), beta.flatten().to(tables[0])
    parts, c0 = [], 0
    for tb, n, nc in zip(tables, pixels, DISTS_CHANNELS):
        mt, mo = tb[:, :, 0] / n, tb[:, :, 2 + 3 * other] / n
        vt, vo = tb[:, :, 1] / n - mt * mt, tb[:, :, 3 + 3 * other] / n - mo * mo
        cov = tb[:, :, 4 + 3 * other] / n - mo * mt
        s1 = (2 * mo * mt + 1e-6) / (mo * mo + mt * mt + 1e-6)
        s2 = (2 * cov + 1e-6) / (vo + vt + 1e-6)
        parts.append((alpha[c0:c0 + nc] * s1 + beta[c0:c0 + nc] * s2).sum(dim=1))     # (level 0: one channel against three weights)
        c0 += nc
    parts = torch.stack(parts, dim=1)
    return 1 - parts.sum(dim=1), parts


def dists_maps(sd, x, dtype=torch.float64):
    """The six maps of DISTS: the raw image and the five maps of the L2-pooled network."""
    return [x.to(dtype)] + features(sd, x, "l2", dtype)


def dists(sd, weights, a, y, dtype=torch.float64):
    """-> (score (B,), parts (B, 6)): parts are the per-level sums of alpha S1 + beta S2."""
    fa, fy = dists_maps(sd, a, dtype), dists_maps(sd, y, dtype)
    tables = [moments(t, o) for o, t in zip(fa, fy)]
    return dists_finish(tables, [t.shape[2] * t.shape[3] for t in fy], weights["alpha"], weights["beta"])
