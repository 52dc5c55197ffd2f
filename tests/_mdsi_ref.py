"""Restatement of the mean deviation similarity index the test loop takes from the reference's module/piq (mdsi.py: mdsi,
data_range 1) for single-channel images in [0, 1], in plain torch ops on whatever dtype and device the inputs have (float64 on
the CPU for the tests' reference values, float32 on the GPU for tools/vsi_mdsi_timing.py's torch-op form).
`mdsi` returns (score (B,), parts (B, 3)); the parts are laid out as the kernels' `parts`: the means over the pooled map of the
real and the imaginary part of z = gcs^q, and the sum of |z - mean|^rho.

Written from the formulas, in this project's own terms: z is a complex tensor; a grey image stands for three equal colour
channels (tests/_vsi_ref._grey_through).  The colour matrix and the Prewitt weights (+-1/3) are rounded to float32 first, as the
reference holds them in a float64 run too.  The cases and their seeded inputs are those of tests/_vsi_ref.py."""
import torch
import torch.nn.functional as F

from _vsi_ref import _grey_through, check, kernel_size, pool, similarity

PART_NAMES = ("mean re", "mean im", "sum dev")


def prewitt_map(x):
    """Magnitude of the horizontal and vertical Prewitt derivatives (weights 1, 1, 1 over 3, the third rounded to float32), zero
    padding."""
    third = (torch.ones(3) / 3).to(x)
    diff = torch.tensor([-1., 0., 1.]).to(x)
    g = F.conv2d(x, torch.stack([torch.outer(third, diff), torch.outer(diff, third)])[:, None], padding=1)
    return torch.sqrt(g[:, :1] ** 2 + g[:, 1:] ** 2)


def principal_power(z, e):
    """z^e on the principal branch, from the modulus and the argument; the argument of a negative real is pi."""
    return torch.polar(z.abs() ** e, torch.angle(z) * e)


def _complex(x):
    return torch.complex(x, torch.zeros_like(x))


def gs_total(a, b):
    """The gradient similarity map of the pooled luminances behind `mdsi` with the default constants (tools/pin_vsi_mdsi.py
    checks that the "faint" case has negative values here)."""
    return _maps(a, b, 140., 55., 550.)[0]


def _maps(a, b, c1, c2, c3):
    """a, b: (B, 1, H, W) in [0, 1] -> (gs_total, cs_total) on the pooled map."""
    k = kernel_size(*a.shape[2:])
    a, b = (pool(t * 255, k, (k - 1) // 2, k // 2, "constant") for t in (a, b))
    lhm = [[0.2989, 0.587, 0.114], [0.3, 0.04, -0.35], [0.34, -0.6, 0.17]]
    (l_a, h_a, m_a), (l_b, h_b, m_b) = (_grey_through(lhm, t) for t in (a, b))
    g_a, g_b, g_avg = prewitt_map(l_a), prewitt_map(l_b), prewitt_map((l_a + l_b) / 2)
    gs = similarity(g_a, g_b, c1) + similarity(g_a, g_avg, c2) - similarity(g_b, g_avg, c2)
    cs = (2 * (h_a * h_b + m_a * m_b) + c3) / (h_a ** 2 + h_b ** 2 + m_a ** 2 + m_b ** 2 + c3)
    return gs, cs


def mdsi(a, b, c1=140., c2=55., c3=550., combination="sum", alpha=0.6, beta=0.1, gamma=0.2, rho=1., q=0.25, o=0.25):
    """-> (score (B,), parts (B, 3)) of a against the target b, in the dtype of a."""
    check(a, b)
    gs, cs = _maps(a, b, c1, c2, c3)
    if combination == "sum":
        gcs = _complex(alpha * gs + (1 - alpha) * cs)
    elif combination == "mult":
        g, c = principal_power(_complex(gs), gamma), principal_power(_complex(cs), beta)
        gcs = torch.complex(g.real * c.real, g.imag + c.imag)          # (the reference's combination: not the complex product)
    else:
        raise ValueError(combination)
    z = principal_power(gcs, q)
    mean = z.mean(dim=[1, 2, 3], keepdim=True)
    dev = ((z - mean).abs() ** rho).sum(dim=[1, 2, 3])
    n = z.shape[2] * z.shape[3]
    return (dev / n) ** (o / rho), torch.stack([mean.real.flatten(), mean.imag.flatten(), dev], dim=1)
