"""Restatement of the three full-reference metrics the test loop takes from the reference's module/piq -- MS-SSIM
(ssim.py: multi_scale_ssim), VIFp (vif.py: vif_p) and GMSD (gmsd.py: gmsd) -- for single-channel images in [0, 1], in plain
torch ops on whatever dtype and device the inputs have (float64 on the CPU for the tests' reference values, float32 on the
GPU for tools/iqa_timing.py's torch-op form).  Each function returns (score (B,), stage values (B, n)); `all_parts` lays the
stage values out as the kernels' `parts`: [0..9] MS-SSIM (cs mean, SSIM mean) of the five levels, [10..17] VIFp (num, den) of
the four scales, [18..19] GMSD (mean, population variance) of the GMS map.

The windows are built as the reference builds them -- in float32, then converted -- so that a float64 run differs from the
reference's float64 run in the order of its sums alone (tests/test_iqa_cpu.py: 1e-12).

CASES / case_inputs: the shapes and seeded inputs shared by tools/pin_iqa.py (which writes tests/golden/iqa_piq.npz from the
reference itself) and the tests."""
import os
import zlib

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iqa_piq.npz")
METRICS = ("ms_ssim", "vif", "gmsd")
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_MIN, VIF_MIN, GMSD_MIN = 161, 41, 2
PART_SLICES = {"ms_ssim": slice(0, 10), "vif": slice(10, 18), "gmsd": slice(18, 20)}
STAGE_NAMES = ([f"ms_ssim level {l} {what}" for l in range(5) for what in ("cs mean", "ssim mean")]
               + [f"vif scale {s} {what}" for s in range(1, 5) for what in ("num", "den")] + ["gmsd mean", "gmsd variance"])

# (metrics, B, H, W); the inputs of case i come from orc.synthetic_ldct(B, seed=100 + i, size=max(H, W)), cropped
CASES = ((("ms_ssim",), 2, 161, 161), (("ms_ssim",), 1, 163, 176), (("ms_ssim",), 1, 176, 163), (("ms_ssim",), 1, 321, 200),
         (("vif",), 3, 41, 41), (("vif",), 2, 47, 58), (("vif",), 1, 100, 77),
         (("gmsd",), 3, 17, 22), (("gmsd",), 2, 33, 33), (("gmsd",), 2, 64, 64), (("gmsd",), 1, 100, 77),
         (METRICS, 1, 512, 512))


def case_inputs(index):
    """(input, target, pred) of case `index`: contiguous float32 (B, 1, H, W); pred is the midpoint of input and target."""
    import mtdgan_oracle as orc
    _, B, H, W = CASES[index]
    x, y = orc.synthetic_ldct(B, seed=100 + index, size=max(H, W))
    x, y = x[:, :, :H, :W].contiguous(), y[:, :, :H, :W].contiguous()
    return x, y, (0.5 * (x + y)).contiguous()


def crc(*tensors):
    c = 0
    for t in tensors:
        c = zlib.crc32(t.contiguous().numpy().tobytes(), c)
    return c


def _ms_window(like):
    coords = torch.arange(11, dtype=torch.float32) - 5.0
    g = coords ** 2
    g = (-(g.unsqueeze(0) + g.unsqueeze(1)) / (2 * 1.5 ** 2)).exp()
    g = g / g.sum()
    return g.view(1, 1, 11, 11).to(like)


def _vif_window(n, like):
    r = torch.arange(-(n // 2), n // 2 + 1)
    x, y = r.view(1, n), r.view(n, 1)
    k = torch.exp(-(x * x + y * y) / (2.0 * (n / 5) ** 2))
    k = k / torch.sum(k)
    return k.view(1, 1, n, n).to(like)


def _check(name, a, b, min_side):
    if a.dim() != 4 or a.shape != b.shape or a.shape[1] != 1:
        raise AssertionError(f"{name}: two (B,1,H,W) tensors of one shape expected")
    if a.shape[-1] < min_side or a.shape[-2] < min_side:
        raise ValueError(f"{name}: images of at least {min_side}x{min_side} expected, got {a.shape[-2]}x{a.shape[-1]}")


def ms_ssim(a, b):
    _check("ms_ssim", a, b, MS_MIN)
    k = _ms_window(a)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    parts = []
    for level in range(5):
        if level > 0:
            p = max(a.shape[2] % 2, a.shape[3] % 2)
            a, b = (F.avg_pool2d(F.pad(t, [p, 0, p, 0], mode="replicate"), kernel_size=2) for t in (a, b))
        mu1, mu2 = F.conv2d(a, k), F.conv2d(b, k)
        mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s11 = F.conv2d(a * a, k) - mu11
        s22 = F.conv2d(b * b, k) - mu22
        s12 = F.conv2d(a * b, k) - mu12
        cs = (2 * s12 + c2) / (s11 + s22 + c2)
        ss = ((2 * mu12 + c1) / (mu11 + mu22 + c1)) * cs
        parts += [cs.mean(dim=(1, 2, 3)), ss.mean(dim=(1, 2, 3))]
    parts = torch.stack(parts, dim=1)                                        # (B, 10)
    v = torch.relu(torch.cat([parts[:, 0:8:2], parts[:, 9:10]], dim=1))      # cs of levels 0..3, SSIM of level 4
    w = torch.tensor(MS_WEIGHTS).to(a)
    return torch.prod(v ** w.view(1, 5), dim=1), parts


def vif(a, b, sigma_n_sq=2.0):
    """a: the prediction, b: the target (the metric is not symmetric).  No rescaling to [0, 255], as the vendored vif_p."""
    _check("vif", a, b, VIF_MIN)
    eps = 1e-8
    parts = []
    for scale in range(1, 5):
        n = 2 ** (5 - scale) + 1
        k = _vif_window(n, a)
        if scale > 1:
            a, b = F.conv2d(a, k)[:, :, ::2, ::2], F.conv2d(b, k)[:, :, ::2, ::2]
        mu_t, mu_p = F.conv2d(b, k), F.conv2d(a, k)
        st = torch.relu(F.conv2d(b ** 2, k) - mu_t * mu_t)
        sp = torch.relu(F.conv2d(a ** 2, k) - mu_p * mu_p)
        stp = F.conv2d(b * a, k) - mu_t * mu_p
        g = stp / (st + eps)
        sv = sp - g * stp
        zero = torch.zeros_like(g)
        g = torch.where(st >= eps, g, zero)
        sv = torch.where(st >= eps, sv, sp)
        st = torch.where(st >= eps, st, zero)
        g = torch.where(sp >= eps, g, zero)
        sv = torch.where(sp >= eps, sv, zero)
        sv = torch.where(g >= 0, sv, sp)
        g = torch.relu(g)
        sv = torch.where(sv > eps, sv, torch.ones_like(sv) * eps)
        parts += [torch.log10(1.0 + (g ** 2.) * st / (sv + sigma_n_sq)).sum(dim=(1, 2, 3)), torch.log10(1.0 + st / sigma_n_sq).sum(dim=(1, 2, 3))]
    parts = torch.stack(parts, dim=1)                                        # (B, 8)
    num, den = 0, 0
    for s in range(4):
        num, den = num + parts[:, 2 * s], den + parts[:, 2 * s + 1]
    return (num + eps) / (den + eps), parts


def gmsd(a, b):
    _check("gmsd", a, b, GMSD_MIN)
    p = max(a.shape[2] % 2, a.shape[3] % 2)
    a, b = (F.avg_pool2d(F.pad(t, [0, p, 0, p]), kernel_size=2, stride=2) for t in (a, b))
    kx = torch.tensor([[[-1., 0., 1.], [-1., 0., 1.], [-1., 0., 1.]]]) / 3
    k = torch.stack([kx, kx.transpose(-1, -2)]).to(a)
    ma, mb = (torch.sqrt(torch.sum(F.conv2d(t, k, padding=1) ** 2, dim=-3, keepdim=True)) for t in (a, b))
    t = 170 / (255. ** 2)
    gms = (2.0 * ma * mb + t) / (ma ** 2 + mb ** 2 + t)
    mean = gms.mean(dim=(1, 2, 3), keepdim=True)
    var = ((gms - mean) ** 2).mean(dim=(1, 2, 3))
    return var.sqrt(), torch.stack([mean.flatten(), var], dim=1)


FUNCS = {"ms_ssim": ms_ssim, "vif": vif, "gmsd": gmsd}


def all_parts(a, b, which=METRICS, dtype=torch.float64, sigma_n_sq=2.0):
    """-> ({metric: score (B,)}, parts (B, 20); the entries of metrics not in `which` are NaN) of a against the target b."""
    a, b = a.to(dtype), b.to(dtype)
    parts = torch.full((a.shape[0], 20), float("nan"), dtype=dtype, device=a.device)
    scores = {}
    for m in which:
        scores[m], parts[:, PART_SLICES[m]] = vif(a, b, sigma_n_sq) if m == "vif" else FUNCS[m](a, b)
    return scores, parts
