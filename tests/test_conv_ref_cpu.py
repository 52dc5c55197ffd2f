"""What the bound of tests/test_igemm_kernels_gpu.py can see, shown on the CPU (tests/_conv_ref.py; no device).

For every (case, epilogue) the GPU file compares with:
  * the columns / weight matrices that seq32 sums are the conv's own terms (their float64 product IS ref64's conv), and the yardstick
    is within the bound by construction;
  * every perturbation of _conv_ref.PERTURBATIONS that applies to the case -- a lost product, a lost tap on a border row, a lost
    (tap, chunk) step of a 32-pixel block, a split-K slab lost or summed twice, the other half's scale one pixel early, the bias of the
    next channel, a parity class on its neighbour's pixels; operands rounded to 10 mantissa bits or to bfloat16, the K sum kept in
    binary16 -- is at least 10 x the case's bound away from ref64.
The second is a condition on the inputs, not a measurement: a case that fails it gets another seed, scale or shape, never
another factor.  Each test prints the yardstick's error, the bound and the ratios."""
import pytest
import torch

import _conv_ref as R
from _metrics import rel

FACTOR = 10.0


def _id(v):
    if isinstance(v, R.Case):
        return v.name
    e = v
    return "bare" if e == R.BARE else "epi" + "".join(str(int(bool(f))) for f in (e.scale, e.scale2, e.bias, e.add1, e.add2, e.mask, e.out2)) + f"a{e.act}s{e.split}"


@pytest.mark.parametrize("c,e", R.REFS, ids=_id)
def test_bound_sees_every_perturbation(c, e):
    ref = R.case_ref(c, e)
    assert ref.yard < ref.bound and ref.bound >= R.FLOOR
    assert ref.yard < R.FLOOR, (c.name, ref.yard)         # (an fp32 chain of at most 2304 terms; a wrong column order would show here)
    ratios = {}
    for what in R.PERTURBATIONS:
        if R.applies(c, e, what):
            got, want = R.perturbed(c, e, what)
            assert got.shape == want.shape
            ratios[what] = rel(got, want) / ref.bound
    print(f"CONVREF {c.name} {_id(e)}: yardstick {ref.yard:.3e} bound {ref.bound:.2e} smallest ratio {min(ratios.values()):.1f}  " +
          " ".join(f"{k} {v:.0f}" for k, v in ratios.items()))
    assert min(ratios.values()) >= FACTOR, (c.name, ratios)


@pytest.mark.parametrize("c", sorted({c for c, _ in R.REFS if R.pixels(c) <= 40000}), ids=_id)
def test_columns_are_the_terms_of_the_conv(c):
    """sum over (tap, channel) of columns x weight matrix in float64 == F.conv2d / conv_transpose2d / autograd in float64."""
    x, w = R.operands(c)
    acc = R.conv64(c, x, w)
    gh, gw = R.grid_hw(c)
    for cls in R.classes(c):
        got = torch.einsum("mtc,tcn->mn", R.columns(c, x, torch.double, cls), R.wmat(c, w, torch.double, cls))
        want = R.class_view(acc, cls).reshape(-1, c.N)
        assert (got - want).abs().max().item() < 1e-12 * max(1.0, want.abs().max().item()), (c.name, cls)


def test_expected_slices():
    """last_slab follows the planner's split of K: 96 channels in two slices are chunks 2 + 1."""
    assert R.last_slab(R.A1, 2) == (64, 96) and R.last_slab(R.A1, 3) == (64, 96) and R.last_slab(R.A2, 2) == (32, 64)
