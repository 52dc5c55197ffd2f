"""Plain-torch float64 restatement of the FID statistic (reference module/piq/fid.py): statistics, Newton-Schulz square root
with its stop, distance and singular fallback -- what the GPU tests compare against, pinned to the reference's own numbers by
tests/test_fid_cpu.py through tests/golden/fid_cases.npz (tools/pin_fid.py).  Also the seeded feature recipe of the cases."""
import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fid_cases.npz")
# (N1, N2, D, decay): the end-to-end cases; each also runs as FID(target, target)
CASES = ((24, 24, 64, 0), (40, 33, 96, 0), (200, 150, 96, 3), (16, 16, 130, 0), (7, 9, 200, 0), (300, 300, 64, 3), (48, 40, 520, 0))
MAX_ITERS, ATOL, EPS = 100, 1e-5, 1e-6


def features(N, D, decay, seed):
    """relu(randn(N, D) @ mix + shift) * scale in fp32: mix = randn(D, D) / sqrt(D) and shift = 0.5 randn(D) from the seed,
    scale = logspace(0, -decay, D).  With N < D the covariance products are rank deficient, with decay 3 ill conditioned too.

    The fixture holds numbers computed from these features on another machine, so they must come out the same to the bit
    wherever this runs, and an fp32 matrix product does not (its blocking, and with it its rounding, follows the CPU).  Hence
    every normal draw is rounded to a multiple of 1/16, the product is taken on those integers in float64 -- exact in any
    order -- and the rest is one correctly rounded float64 operation per element; the scale is a running product.  `crc` in the
    fixture is the check (tests/test_fid_cpu.py)."""
    g = torch.Generator().manual_seed(seed)
    mix = torch.round(torch.randn(D, D, generator=g).double() * 16)
    shift = torch.round(torch.randn(D, generator=g).double() * 16) / 32
    z = torch.round(torch.randn(N, D, generator=g).double() * 16)
    ratio = 10.0 ** (-decay / max(D - 1, 1))
    steps = [1.0]
    for _ in range(D - 1):
        steps.append(steps[-1] * ratio)
    scale = torch.tensor(steps, dtype=torch.float64)
    y = (z @ mix) / (256.0 * math.sqrt(D)) + shift
    return (torch.relu(y) * scale).float().contiguous()


def crc(*tensors):
    """CRC-32 of the tensors' bytes, in order."""
    import zlib
    c = 0
    for t in tensors:
        c = zlib.crc32(t.contiguous().numpy().tobytes(), c)
    return c


def case_features(case, index):
    """(predicted, target) feature sets of case number `index`."""
    N1, N2, D, decay = case
    return features(N1, D, decay, 1000 + 2 * index), features(N2, D, decay, 1001 + 2 * index)


def statistics(x):
    """Mean, then the centred product over N - 1, of the float64 copy of the features."""
    x = x.double()
    mu = x.mean(dim=0)
    xc = x - mu
    return mu, (xc.t() @ xc) / (x.shape[0] - 1)


def sqrtm(A, max_iters=MAX_ITERS):
    """(S, err, rounds, errs): S ~ sqrt(A) by Newton-Schulz on A / |A|_F; stops at |A - S S|_F / |A|_F <= 1e-5."""
    norm = A.norm()
    Y = A / norm
    eye = torch.eye(A.shape[0], dtype=A.dtype)
    Z = eye.clone()
    S, err, errs = None, None, []
    for r in range(1, max_iters + 1):
        T = 0.5 * (3.0 * eye - Z @ Y)
        Y, Z = Y @ T, T @ Z
        S = Y * torch.sqrt(norm)
        err = (A - S @ S).norm() / norm
        errs.append(err.item())
        if abs(err.item()) <= ATOL:
            break
    return S, err.item(), r, errs


def distance(stats1, stats2, offset=None):
    """dict(fid, tr, err, rounds, finite, fallback, errs) in float64.  offset=None: the first solve and, if its square root is not
    finite, the second with 1e-6 on both diagonals; a number: that one solve with the offset on both diagonals."""
    (mu1, s1), (mu2, s2) = stats1, stats2
    eye = torch.eye(s1.shape[0], dtype=s1.dtype)
    o = 0.0 if offset is None else offset
    S, err, rounds, errs = sqrtm((s1 + o * eye) @ (s2 + o * eye))
    finite, fallback = bool(torch.isfinite(S).all()), False
    if offset is None and not finite:
        S, err, rounds, errs = sqrtm((s1 + EPS * eye) @ (s2 + EPS * eye))
        fallback = True
    d = mu1 - mu2
    tr = torch.trace(S)
    fid = d.dot(d) + torch.trace(s1) + torch.trace(s2) - 2 * tr
    return dict(fid=fid.item(), tr=tr.item(), err=err, rounds=rounds, finite=finite, fallback=fallback, errs=errs)


def base(stats1, stats2):
    """|mu1 - mu2|^2 + tr S1 + tr S2: the size of the terms the distance is a difference of."""
    d = stats1[0] - stats2[0]
    return (d.dot(d) + torch.trace(stats1[1]) + torch.trace(stats2[1])).item()


def fid(a, b):
    return distance(statistics(a), statistics(b))


def golden():
    """The fixture as a list of dicts, one per entry: case, index, same (FID(target, target)), fid64, fid32, tr, rounds, base, tol, crc
    (of the two feature sets)."""
    z = np.load(GOLDEN)
    return json.loads(str(z["meta"])), [dict(case=tuple(int(v) for v in z["case"][i]), index=int(z["index"][i]), same=bool(z["same"][i]),
                                            fid64=float(z["fid64"][i]), fid32=np.float32(z["fid32"][i]), tr=float(z["tr"][i]),
                                            rounds=int(z["rounds"][i]), base=float(z["base"][i]), tol=float(z["tol"][i]), crc=int(z["crc"][i]))
                                       for i in range(len(z["fid64"]))]
