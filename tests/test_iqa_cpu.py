"""MS-SSIM, VIFp and GMSD without a GPU: the float64 restatement of tests/_iqa_ref.py against what the reference's
own module/piq computed (tests/golden/iqa_piq.npz, written by tools/pin_iqa.py), the conditions the fixture's inputs were chosen
to meet, the size rules, the test loop's option check, and the argument refusals of the entry points that need no device
(through the built library's ABI, with addresses of host memory)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _iqa_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    return _lib.lib()


def _rel(got, want):
    """Largest relative distance over the entries whose reference value is not 0; those must be 0 in `got` too."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert (got[want == 0] == 0).all()
    nz = want != 0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_float64_restatement_agrees_with_the_reference(golden, index):
    """The same operations in float64; only the order of the sums differs: 1e-12 relative on every score and stage value."""
    metrics, B, H, W = R.CASES[index]
    x, y, pred = R.case_inputs(index)
    assert R.crc(x, y, pred) == int(golden[f"crc_{index}"]), "the seeded inputs are not the ones the fixture was written from"
    for k, src in enumerate((x, y, pred)):
        scores, parts = R.all_parts(src, y, metrics)
        for m in metrics:
            e = _rel(scores[m].numpy(), golden[f"{m}_{index}_score64"][k])
            assert e <= 1e-12, (m, k, e)
            got, want = parts[:, R.PART_SLICES[m]].numpy(), golden[f"{m}_{index}_parts64"][k]
            for j in range(want.shape[1]):
                e = _rel(got[:, j], want[:, j])
                assert e <= 1e-12, (R.STAGE_NAMES[R.PART_SLICES[m].start + j], k, e)


def test_fixture_is_well_conditioned(golden):
    """Conditions on the chosen inputs, not tolerances: every MS-SSIM level value above 0.5 (relu inactive, powers well
    conditioned), every VIFp den above 0; and both precisions of the reference are there for every case and metric."""
    for index, (metrics, B, H, W) in enumerate(R.CASES):
        for m in metrics:
            for tag, dt in (("32", np.float32), ("64", np.float64)):
                n = R.PART_SLICES[m].stop - R.PART_SLICES[m].start
                assert golden[f"{m}_{index}_score{tag}"].shape == (3, B) and golden[f"{m}_{index}_score{tag}"].dtype == dt
                assert golden[f"{m}_{index}_parts{tag}"].shape == (3, B, n) and golden[f"{m}_{index}_parts{tag}"].dtype == dt
            p = golden[f"{m}_{index}_parts64"]
            if m == "ms_ssim":
                assert (np.concatenate([p[..., 0:8:2], p[..., 9:10]], axis=-1) > 0.5).all(), index
            if m == "vif":
                assert (p[..., 1::2] > 0).all(), index
    assert os.path.getsize(R.GOLDEN) < 64 * 1024


def test_size_rules_of_the_restatement():
    for fn, lo in ((R.ms_ssim, 161), (R.vif, 41)):
        ok = torch.rand(1, 1, lo, lo + 3, dtype=torch.float64, generator=torch.Generator().manual_seed(lo))
        score, _ = fn(ok, ok.flip(-1))
        assert tuple(score.shape) == (1,) and bool(torch.isfinite(score).all())
        for small in (ok[:, :, :lo - 1], ok[:, :, :, :lo - 1]):
            with pytest.raises(ValueError, match=str(lo)):
                fn(small, small)


class _NoLoader:
    def __iter__(self):
        raise AssertionError("the loader must not be read before the option is checked")


@pytest.mark.parametrize("bad", ["ms_ssim", ("psnr",), ("vif", "vif"), 3, ("ms_ssim", 1), {"vif": True}])
def test_engine_refuses_a_bad_test_iqa_before_anything_runs(bad):
    import types
    from mtd_gan_amd import engine
    model = types.SimpleNamespace(test_iqa=bad)          # no Generator: anything past the option check would fail otherwise
    with pytest.raises(ValueError, match="ms_ssim.*vif.*gmsd"):
        engine.test_MTD_GAN_Ours(model, None, _NoLoader(), torch.device("cpu"), None)


def test_engine_option_values():
    import types
    from mtd_gan_amd import engine
    opt = lambda **kw: engine._iqa_option(types.SimpleNamespace(**kw))          # noqa: E731
    assert opt() is None and opt(test_iqa=None) is None and opt(test_iqa=False) is None and opt(test_iqa=()) is None
    assert opt(test_iqa=True) == ("ms_ssim", "vif", "gmsd")
    assert opt(test_iqa=("gmsd", "ms_ssim")) == ("ms_ssim", "gmsd") and opt(test_iqa=["vif"]) == ("vif",)


def test_header_declares_and_lib_binds_the_entry_points(built_lib):
    from mtd_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    for n in ("mtd_iqa_ws_bytes", "mtd_iqa_each"):
        assert re.search(r"^(size_t|int) %s\(" % n, header, re.M), n
        assert n in _lib.EXPORTS and len(getattr(built_lib, n).argtypes) > 0, n
    assert len(built_lib.mtd_iqa_each.argtypes) == 12 and len(built_lib.mtd_iqa_ws_bytes.argtypes) == 5


def test_refusals_return_before_any_launch(built_lib):
    """The refused calls touch neither their pointers nor the device."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    f, q = built_lib.mtd_iqa_each, built_lib.mtd_iqa_ws_bytes
    # GMSD alone at (na 3, B 2, 100 x 77): a 50 x 39 pooled map in 2 x 2 tiles, two doubles per tile and (source, image)
    assert q(4, 3, 2, 100, 77) == 3 * 2 * 4 * 2 * 8
    assert q(7, 3, 1, 512, 512) > 0 and q(1, 1, 1, 161, 161) > 0 and q(2, 1, 1, 41, 41) > 0 and q(4, 1, 1, 2, 2) > 0
    for mask, na, B, H, W in ((0, 3, 1, 512, 512), (8, 3, 1, 512, 512), (7, 0, 1, 512, 512), (7, 4, 1, 512, 512), (7, 3, 0, 512, 512),
                              (1, 3, 1, 160, 512), (1, 3, 1, 512, 160), (7, 3, 1, 160, 160), (2, 3, 1, 40, 64), (2, 3, 1, 64, 40),
                              (4, 3, 1, 1, 8), (4, 3, 1, 8, 1), (4, 3, 16384, 8, 8), (4, 1, 1, 40000, 40000)):
        assert q(mask, na, B, H, W) == 0, (mask, na, B, H, W)
        assert f(ptrs, na, p, B, H, W, mask, 2.0, p, p, p, None) == -1, (mask, na, B, H, W)
    assert f(None, 3, p, 1, 64, 64, 4, 2.0, p, p, p, None) == -1
    assert f(ptrs, 3, None, 1, 64, 64, 4, 2.0, p, p, p, None) == -1
    assert f(ptrs, 3, p, 1, 64, 64, 4, 2.0, None, p, p, None) == -1
    assert f(ptrs, 3, p, 1, 64, 64, 4, 2.0, p, p, None, None) == -1
    assert f((ctypes.c_void_p * 3)(p, None, p), 3, p, 1, 64, 64, 4, 2.0, p, p, p, None) == -1
    assert f(ptrs, 3, p, 1, 64, 64, 2, 0.0, p, p, p, None) == -1            # sigma_n_sq must be positive


def test_python_surface_refusals_without_a_device():
    from mtd_gan_amd import metrics as M
    x = torch.zeros(2, 1, 176, 176)
    for fn in (M.iqa_metrics_each, M.iqa_metrics_per_slice, M.compute_MS_SSIM, M.compute_VIF, M.compute_GMSD):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(x, x, x)
        with pytest.raises(AssertionError):
            fn(x[:1], x, x)
    for fn in (M.compute_MS_SSIM, M.compute_VIF, M.compute_GMSD):
        with pytest.raises(NotImplementedError):
            fn(x, x, x, data_range=255.0)
    for bad in ((), ("psnr",), ("vif", "vif"), 5):
        with pytest.raises(ValueError, match="ms_ssim"):
            M.iqa_metrics_each(x, x, x, which=bad)
    assert M.IQA_METRICS == R.METRICS and M.IQA_PARTS == 20
    assert M.IQA_MIN_SIDE == {"ms_ssim": R.MS_MIN, "vif": R.VIF_MIN, "gmsd": R.GMSD_MIN}
