"""What the bound of tests/test_wino_kernels_gpu.py can see, shown on the CPU (tests/_wino_ref.py; no device).

For every (case, epilogue, form, pipe) the GPU file compares with:
  * the Winograd form restated from the kernels' headers, evaluated in float64, IS the conv (wino64 == conv64 to 1e-12 of the largest
    output) -- forward, mirrored taps, the four phases of the stride-2 form and the parity classes of its data gradient;
  * the yardstick (fp32 transforms, one fp32 chain over K; the split-bf16 form: six piece products per term) is within the bound;
  * every structural perturbation of _wino_ref.STRUCTURAL that applies to the case -- one (tile, position, K step) product block
    lost, a padding pixel taken from the clamped neighbour, a whole tile on the scale of its first pixel, a tile's columns shifted
    by one, a split-K slab lost or summed twice, the bias of the next channel, the data gradient with the forward tap map, one
    phase of the stride-2 form lost, a parity class on its neighbour's pixels -- and operands rounded to 10 mantissa bits or to
    bfloat16 are at least 10 x the case's bound away from ref64.
The last is a condition on the inputs, not a measurement: a case that fails it gets another seed or shape, never another factor.
Each test prints the yardstick's error, the bound and the ratios.

test_low_plane_dropped: the split-bf16 form without the low plane of both transformed operands (products of 16-bit instead of 24-bit
significands, evaluated in float64).  Measured on 3 x 10 x 14 / 3 x 6 x 20, C 80, N 64, forward and data gradient, bare and full epilogue:
F(2x2) rel 5.2e-5 .. 9.3e-5 = 5.2 .. 9.3 x the bound (the floor 1e-5) -- BELOW 10 x: on that form the bound sees a dropped low plane,
but without the margin asked of every other perturbation; F(2x4) rel 2.0e-4 .. 2.9e-4 = 10.2 .. 20.5 x its bound (1.4e-5 .. 2.1e-5).
The guard for it remains the assertion e3 <= 2 e32 of test_kernels_gpu.py::test_winograd_conv_vs_torch; the bound is not bent
to catch it."""
import pytest
import torch

import _conv_ref as R
import _wino_ref as Wn
from _metrics import rel

FACTOR = 10.0


def _eid(e):
    return "bare" if e == R.BARE else "epi" + "".join(str(int(bool(f))) for f in (e.scale, e.scale2, e.bias, e.add1, e.add2, e.mask, e.out2)) + f"a{e.act}s{e.split}"


def _id(v):
    return f"{v[0].name}-{_eid(v[1])}-{v[2]}-{v[3]}"


@pytest.mark.parametrize("ref", Wn.REFS, ids=_id)
def test_bound_sees_every_perturbation(ref):
    c, e, form, pipe = ref
    r = Wn.case_ref(c, e, form, pipe)
    assert r.yard < r.bound and r.bound >= Wn.FLOOR
    ratios = {}
    for what in Wn.PERTURBATIONS:
        if Wn.applies(c, e, form, what):
            got, want = Wn.perturbed(c, e, form, what)
            assert got.shape == want.shape
            ratios[what] = rel(got, want) / r.bound
    print(f"WINOREF {c.name} {_eid(e)} {form} {pipe}: yardstick {r.yard:.3e} bound {r.bound:.2e} smallest ratio {min(ratios.values()):.1f}  " +
          " ".join(f"{k} {v:.0f}" for k, v in ratios.items()))
    assert min(ratios.values()) >= FACTOR, (c.name, ratios)


@pytest.mark.parametrize("cf", sorted({(c, form) for c, _, form, _ in Wn.REFS}), ids=lambda v: f"{v[0].name}-{v[1]}")
def test_the_form_is_the_conv(cf):
    """wino64 == conv64 on the first 32 output channels; F(2x2) too where the case takes F(2x4) by default."""
    c, form = cf
    x, w = R.operands(c)
    want = Wn._acc64(c)[..., :32]
    for f in {form, Wn.form_of(c, f4=False)}:
        got = Wn.wino64(f, c, x, w)
        assert got.shape == want.shape
        err = (got - want).abs().max().item() / max(1.0, want.abs().max().item())
        print(f"WINOREF {c.name} {f}: |wino64 - conv64| / max = {err:.2e}")
        assert err < 1e-12, (c.name, f, err)


@pytest.mark.parametrize("ref", [r for r in Wn.REFS if r[3] == Wn.SPLIT], ids=_id)
def test_low_plane_dropped(ref):
    """Printed, not asserted against the factor (module docstring): the ratio lies near 1."""
    c, e, form, _ = ref
    r = Wn.case_ref(c, e, form, Wn.SPLIT)
    got, want = Wn.low_plane_dropped(c, e, form)
    err = rel(got, want)
    print(f"WINOREF {c.name} {_eid(e)} {form}: low plane dropped {err:.3e} = {err / r.bound:.2f} x bound {r.bound:.2e} (yardstick {r.yard:.2e})")
    assert err > r.yard          # (it is an error: larger than the six-product form's own)


def test_split_is_exact():
    """x = hi + mid + lo exactly, every piece a bf16 value."""
    x = R.rnd(4096, seed=7) * torch.logspace(-20, 20, 4096)
    h, m, l = Wn.split3(x)
    assert torch.equal(h.double() + m.double() + l.double(), x.double())
    for p in (h, m, l):
        assert torch.equal(p.bfloat16().float(), p)


def test_expected_slices():
    """last_slab follows the planner's split of K in steps of 16 channels: 80 channels in two slices are 3 + 2 steps; the stride-2
    forward form sums 4 C."""
    assert Wn.last_slab(Wn.W1["fwd"], Wn.F22, 2) == (48, 80) and Wn.last_slab(Wn.S2A, Wn.S2, 4) == (192, 256)
    assert Wn.last_slab(Wn.S2C, Wn.S2, 3) == (192, 256)
