"""The references of tests/test_wgrad_kernels_gpu.py checked against each other on the CPU (tests/_wgrad_ref.py), for every layer shape
the GPU tests use:

  * the fp32 yardstick (seq32: one accumulation chain over all pixels) stays below the 1e-5 floor of the bound
    max(1e-5, 2 * rel(seq32, ref64)), so the float64 reference with a plain fp32 evaluation is inside the bound by itself;
  * every structural error -- one cotangent pixel lost, one 32-pixel chunk lost, one border column of one image zeroed, and for the
    layers of the reduce tests one slab lost or summed twice -- moves the gradient by at least ten times that bound, so the GPU
    assertions can see the smallest of them.

Each test prints the yardstick's error and the smallest error of a perturbed reference."""
import pytest

import _wgrad_ref as R
from _metrics import rel

REFS = [(c, None, None) for c in R.FULL] + list(R.HALVES)


def _id(v):
    c, b0, b1 = v
    return c.name if b0 is None else f"{c.name}[{b0}:{b1}]"


@pytest.mark.parametrize("which", REFS, ids=_id)
def test_yardstick_inside_and_structural_errors_outside_the_bound(which):
    c, b0, b1 = which
    ref = R.case_ref(c) if b0 is None else R.half_ref(c, b0, b1)
    assert ref.yard_dw < R.FLOOR and ref.yard_db < R.FLOOR, (ref.yard_dw, ref.yard_db)
    x, gy = ref.x, ref.gy
    M = gy.shape[0] * gy.shape[1] * gy.shape[2]
    sites = [("pixel", M // 2, 0), ("pixel", M - 1, 0), ("column", 0, 0), ("column", gy.shape[0] - 1, 0)]
    if M >= 32:
        sites.append(("chunk", 32 * (M // 32 - 1), 0))          # the last whole chunk
    for want in R.REDUCE_CASES.get(c, ()) if b0 is None else ():
        m0, m1 = R.slab_range(M, want, 1)
        sites += [("slab_lost", m0, m1), ("slab_twice", m0, m1)]
    worst = {}
    for what, m0, m1 in sites:
        dw, db = R.perturbed((ref.dw, ref.db), x, gy, c.kind, c.k, c.s, c.p, what, m0, m1)
        e = rel(dw, ref.dw) / ref.bound_dw
        if what != "column":                                    # (the bias gradient does not see the input)
            e = min(e, rel(db, ref.db) / ref.bound_db)
        worst[what] = min(worst.get(what, float("inf")), e)
    print(f"{_id(which)}: M = {M}, yardstick dw {ref.yard_dw:.2e} db {ref.yard_db:.2e}, bound dw {ref.bound_dw:.1e} db {ref.bound_db:.1e}, "
          "smallest perturbation / bound: " + ", ".join(f"{k} {v:.0f}" for k, v in worst.items()))
    assert min(worst.values()) >= 10.0, worst


def test_references_agree_on_a_transposed_layer():
    """ref64 of a ConvTranspose2d layer is ref64 of the Conv2d with swapped channel roles and flipped taps (guards the tap order of
    the "convT" branch of seq32 and ref64 against each other and against a second formulation)."""
    import torch
    x, gy = R.rnd(2, 6, 5, 32, seed=1), R.rnd(2, 6, 5, 32, seed=2)
    dwT, dbT = R.ref64(x, gy, "convT", 3, 1, 1)
    # y = convT(x, w)  <=>  x-gradient form: dw[c, n, ky, kx] = sum gy[Y, X, n] x[Y + 1 - ky, X + 1 - kx, c] = conv weight gradient with
    # the roles of x and gy exchanged
    dw2, _ = R.ref64(gy, x, "conv", 3, 1, 1)
    assert rel(dwT, dw2) < 1e-12
    sdw, sdb = R.seq32(x, gy, "convT", 3, 1, 1)
    assert rel(sdw, dwT) < R.FLOOR and rel(sdb, dbT) < R.FLOOR
    assert torch.equal(torch.as_tensor(R.slab_range(20480, 17, 1)), torch.as_tensor((1280, 2560)))
