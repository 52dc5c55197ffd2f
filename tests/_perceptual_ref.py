"""Plain-torch restatement of the perceptual metrics' definitions, for the parity tests: the VGG-19 feature stack up to
relu5_1 on a single-channel image repeated to three channels (no ImageNet normalisation), the perceptual loss PL and the
texture-matching loss TML (non-overlapping 16 x 16 patches, unnormalised Gram matrices, L1 mean), both weighted
[1/32, 1/16, 1/8, 1/4, 1] over the five maps.  Runs on the CPU in the dtype it is asked for (float64 as the reference side)."""
import math

import torch
import torch.nn.functional as F

# torchvision vgg19().features: (index, C_in, C_out) of every conv up to relu5_1; 'P' = MaxPool2d(2, 2)
CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (16, 256, 256),
         (19, 256, 512), (21, 512, 512), (23, 512, 512), (25, 512, 512), (28, 512, 512))
POOLS = (4, 9, 18, 27)
TAPS = (1, 6, 11, 20, 29)
WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)
PATCH = 16


def seeded_state_dict(seed=0):
    """A torchvision-layout VGG-19 state dict with He-normal weights (std = sqrt(2 / (9 C_in)), three input channels in the
    first layer) and N(0, 0.05) biases; one classifier entry stands for the keys the product side must ignore."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cin, cout in CONVS:
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"features.{idx}.bias"] = torch.randn(cout, generator=g) * 0.05
    sd["classifier.0.bias"] = torch.zeros(8)
    return sd


def features(sd, x, dtype=torch.float64):
    """x: (B, 1, H, W).  The five NCHW maps relu1_1 ... relu5_1."""
    t = x.to(dtype).repeat(1, 3, 1, 1)
    convs = {idx: (sd[f"features.{idx}.weight"].to(dtype), sd[f"features.{idx}.bias"].to(dtype)) for idx, _, _ in CONVS}
    maps = []
    for idx in range(30):
        if idx in convs:
            t = F.relu(F.conv2d(t, convs[idx][0], convs[idx][1], padding=1))      # (the ReLU of index idx + 1)
            if idx + 1 in TAPS:
                maps.append(t)
        elif idx in POOLS:
            t = F.max_pool2d(t, 2, 2)
    return maps


def patches(f):
    """(B, C, h, w) -> (B * P, C, 256): the non-overlapping 16 x 16 patches, remainder rows and columns dropped."""
    B, C, h, w = f.shape
    ph, pw = h // PATCH, w // PATCH
    f = f[:, :, :ph * PATCH, :pw * PATCH].reshape(B, C, ph, PATCH, pw, PATCH)
    return f.permute(0, 2, 4, 1, 3, 5).reshape(B * ph * pw, C, PATCH * PATCH)


def gram(f):
    p = patches(f)
    return p @ p.transpose(1, 2)


def pl(fx, fy):
    return sum(w * (a - b).abs().mean() for w, a, b in zip(WEIGHTS, fx, fy))


def tml(fx, fy):
    return sum(w * (gram(a) - gram(b)).abs().mean() for w, a, b in zip(WEIGHTS, fx, fy))
