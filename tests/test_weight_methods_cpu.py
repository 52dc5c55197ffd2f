"""Host side of the task weightings next to PCGrad (module/weight_methods.py): the METHODS table, constructor signatures against
the reference's (recorded in tests/golden/weight_methods_b2.npz), the exported symbols, and the numpy model of the CAGrad
coefficient kernel on every Gram case of tests/golden/cagrad_gram_cases.npz.  No GPU."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = {"stl", "ls", "uw", "pcgrad", "cagrad", "scaleinvls", "rlw", "dwa"}


@pytest.fixture(scope="module")
def built_lib():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    return ctypes.CDLL(_lib.LIB_PATH)


def _meta():
    z = np.load(os.path.join(GOLD, "weight_methods_b2.npz"))
    return json.loads(str(z["meta"]))


def test_methods_table_has_exactly_the_eight_keys():
    from mtd_gan_amd.module import weight_methods as WM
    assert set(WM.METHODS) == KEYS
    names = dict(stl="STL", ls="LinearScalarization", uw="Uncertainty", pcgrad="PCGrad", cagrad="CAGrad",
                 scaleinvls="ScaleInvariantLinearScalarization", rlw="RLW", dwa="DynamicWeightAverage")
    for k, n in names.items():
        assert WM.METHODS[k] is getattr(WM, n)


def test_constructor_signatures_equal_the_reference():
    from mtd_gan_amd.module import weight_methods as WM
    sigs = _meta()["signatures"]
    for key in sorted(KEYS):
        ps = list(inspect.signature(WM.METHODS[key].__init__).parameters.values())[1:]
        got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in ps]
        assert got == sigs[key], (key, got, sigs[key])


@pytest.mark.parametrize("name", ["mgda", "imtl", "nashmtl"])
def test_the_three_methods_left_out_still_fail_the_assertion(name):
    from mtd_gan_amd.module.weight_methods import WeightMethods
    with pytest.raises(AssertionError):
        WeightMethods(name, n_tasks=3, device=torch.device("cpu"))


def test_host_objects_build_without_a_gpu_and_report_like_the_reference():
    from mtd_gan_amd.module.weight_methods import WeightMethods
    cpu = torch.device("cpu")
    assert WeightMethods("uw", n_tasks=3, device=cpu).parameters()[0].requires_grad
    assert WeightMethods("ls", n_tasks=3, device=cpu).parameters() == []
    assert WeightMethods("stl", n_tasks=3, device=cpu, main_task=1).method.weights.tolist() == [0.0, 1.0, 0.0]
    assert WeightMethods("dwa", n_tasks=3, device=cpu).method.iteration_window == 25
    assert WeightMethods("cagrad", n_tasks=3, device=cpu).method.c == 0.4
    with pytest.raises(RuntimeError):          # the weights come from a HIP kernel: host losses are refused, not computed elsewhere
        WeightMethods("ls", n_tasks=3, device=cpu).get_weighted_loss(torch.ones(3))


def test_library_exports_the_new_symbols(built_lib):
    from mtd_gan_amd import _lib
    for s in ("mtd_task_weights", "mtd_task_weights_state_floats", "mtd_cagrad_coeff"):
        assert s in _lib.EXPORTS and hasattr(built_lib, s), s
    assert "wptr" in [f[0] for f in _lib.LossTerm._fields_]


def test_recorded_step_says_why_a_method_stays_eager():
    from mtd_gan_amd.module.weight_methods import WeightMethods
    from mtd_gan_amd.train_step import RecordedTrainStep
    cpu = torch.device("cpu")
    for m, kw in (("ls", {}), ("scaleinvls", {}), ("stl", dict(main_task=0)), ("dwa", {}), ("cagrad", {}), ("pcgrad", {})):
        assert RecordedTrainStep.method_refusal(WeightMethods(m, n_tasks=3, device=cpu, **kw)) is None, m
    assert "draw" in RecordedTrainStep.method_refusal(WeightMethods("rlw", n_tasks=3, device=cpu))
    assert "log sigmas" in RecordedTrainStep.method_refusal(WeightMethods("uw", n_tasks=3, device=cpu))
    assert "mean" in RecordedTrainStep.method_refusal(WeightMethods("pcgrad", n_tasks=3, device=cpu, reduction="mean"))


def test_cagrad_host_model_reaches_the_tight_minimum_on_every_case():
    """The numpy model of mtd_cagrad_coeff (the enumeration the kernel runs) against scipy SLSQP at ftol 1e-14, recorded in the
    fixture: phi is not above the tight value by more than the slack measured between the reference's own default-tolerance
    solve and the tight one (2 x the 99th percentile, relative), on EVERY case; the merged gradient is within the measured band
    on all but at most 1 % of the cases; nothing is NaN on the degenerate matrices."""
    from mtd_gan_amd.module.weight_methods import cagrad_host_model
    z = np.load(os.path.join(GOLD, "cagrad_gram_cases.npz"))
    band = json.loads(str(z["band"]))
    assert band["within"] >= 0.99
    over, worst_phi, worst = 0, -1.0, 0.0
    N = len(z["T"])
    for i in range(N):
        T = int(z["T"][i])
        A = z["gram"][i, :T, :T]
        coeff, phi, ww = cagrad_host_model(A, float(z["c"][i]))
        assert np.all(np.isfinite(coeff)) and np.isfinite(phi), (i, str(z["kind"][i]))
        assert abs(ww.sum() - 1.0) < 1e-9 and ww.min() >= 0.0
        pt = float(z["phi_tight"][i])
        worst_phi = max(worst_phi, (phi - pt) / abs(pt))
        assert phi <= pt + band["phi_rel_slack"] * abs(pt), (i, str(z["kind"][i]), phi, pt)
        ct = z["coeff_tight"][i, :T]
        d = coeff - ct
        e = np.sqrt(max(d @ A @ d, 0.0)) / (np.sqrt(max(ct @ A @ ct, 0.0)) + 1e-30)
        worst = max(worst, e)
        over += e > band["merged_bound"]
    print(f"{N} cases: phi_model - phi_tight (relative) worst {worst_phi:.2e} (slack {band['phi_rel_slack']:.2e}); merged difference worst "
          f"{worst:.2e} (bound {band['merged_bound']:.2e}), {over} over")
    assert over <= band["max_excluded"] * N
