"""Error measures shared by the GPU parity tests."""
import torch


def rel(a, b):
    """The larger of two errors of a against the reference b:
      * max |a - b| / max |b|                         (a tensor-wide bound), and
      * max over elements of |a - b| / (|b| + rms(b))  (element-wise: relative for the elements that carry the tensor's
        energy, absolute at the scale of the tensor's RMS -- not of its largest element -- for the small ones, so an error
        hidden under one large entry, or spread over many small ones, still shows)."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    d = (a - b).abs()
    e_max = d.max().item() / (b.abs().max().item() + 1e-30)
    rms = b.pow(2).mean().sqrt().item()
    e_el = (d / (b.abs() + rms + 1e-30)).max().item()
    return max(e_max, e_el)


def one_rounding(name, h, f):
    """|h - f| <= 2^-11 |f| + 2^-24 for every element: half a unit in the last place of binary16 (relative, and the subnormal floor).
    No slack for another summation order: every binary16 form is a template instance of the fp32 kernel it is compared with (same
    lanes, same sums; the storage type only changes the loads' widening and the stores' rounding)."""
    h, f = h.double().cpu(), f.double().cpu()
    assert h.shape == f.shape and torch.isfinite(h).all()
    excess = ((h - f).abs() - (2.0 ** -11 * f.abs() + 2.0 ** -24)).max().item()
    worst = ((h - f).abs() / (2.0 ** -11 * f.abs() + 2.0 ** -24)).max().item()
    print(f"{name}: max |h - f| / (2^-11 |f| + 2^-24) = {worst:.4f}, max |f| = {f.abs().max().item():.3f}")
    assert excess <= 0.0, (name, worst)
