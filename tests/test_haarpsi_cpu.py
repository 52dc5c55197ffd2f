"""HaarPSI without a GPU: the float64 restatement of tests/_haarpsi_ref.py against what the reference's own
module/piq/haarpsi.py computed (tests/golden/haarpsi_piq.npz, written by tools/pin_haarpsi.py), the conditions the fixture's
inputs were chosen to meet, the size rule, the test loop's option check, and the argument refusals of the entry points that
need no device (through the built library's ABI, with addresses of host memory)."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import _haarpsi_ref as R

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
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert (want != 0).all()
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_float64_restatement_agrees_with_the_reference(golden, index):
    """The same operations in float64; only the order of the sums differs: 1e-12 relative on every score and part sum."""
    B, H, W, subsample, c, alpha = R.CASES[index]
    x, y, pred = R.case_inputs(index)
    assert tuple(x.shape) == (B, 1, H, W) and x.dtype == torch.float32
    assert R.crc(x, y, pred) == int(golden[f"crc_{index}"]), "the seeded inputs are not the ones the fixture was written from"
    for k, src in enumerate((x, y, pred)):
        score, parts = R.haarpsi(src.double(), y.double(), subsample, c, alpha)
        e = _rel(score.numpy(), golden[f"score64_{index}"][k])
        assert e <= 1e-12, ("score", k, e)
        for j in range(4):
            e = _rel(parts[:, j].numpy(), golden[f"parts64_{index}"][k][:, j])
            assert e <= 1e-12, (R.PART_NAMES[j], k, e)


def test_fixture_conditions(golden):
    """Conditions on the chosen inputs, not tolerances: den > 1 on every row (eps cannot matter), both precisions of the reference
    for every case, the cases of _haarpsi_ref, the recorded float32 -> float64 distances those of the stored values."""
    meta = json.loads(str(golden["meta"]))
    assert [tuple(cs) for cs in meta["cases"]] == [tuple(cs) for cs in R.CASES]
    spread = {"score": 0.0, "parts": 0.0}
    for index, (B, H, W, subsample, c, alpha) in enumerate(R.CASES):
        for tag, dt in (("32", np.float32), ("64", np.float64)):
            assert golden[f"score{tag}_{index}"].shape == (3, B) and golden[f"score{tag}_{index}"].dtype == dt
            assert golden[f"parts{tag}_{index}"].shape == (3, B, 4) and golden[f"parts{tag}_{index}"].dtype == dt
            assert (golden[f"parts{tag}_{index}"][..., 1::2] > 1).all(), index
        for what in ("score", "parts"):
            spread[what] = max(spread[what], _rel(golden[f"{what}32_{index}"], golden[f"{what}64_{index}"]))
        s = golden[f"score64_{index}"]
        assert (np.abs(s[1] - 1) < 1e-13).all() and (s[0] < s[2]).all() and (s[2] < 0.99).all(), index      # gt, input, pred
    assert spread == meta["spread"]
    assert os.path.getsize(R.GOLDEN) < 64 * 1024


@pytest.mark.parametrize("subsample", [True, False])
def test_size_rule_of_the_restatement(subsample):
    ok = torch.rand(1, 1, 16, 19, dtype=torch.float64, generator=torch.Generator().manual_seed(16))
    score, parts = R.haarpsi(ok, ok.flip(-1), subsample)
    assert tuple(score.shape) == (1,) and tuple(parts.shape) == (1, 4) and bool(torch.isfinite(score).all())
    for small in (ok[:, :, :15], ok[:, :, :, :15]):
        with pytest.raises(ValueError, match="16x16"):
            R.haarpsi(small, small, subsample)


class _NoLoader:
    def __iter__(self):
        raise AssertionError("the loader must not be read before the option is checked")


BAD_OPTIONS = ["yes", 3, ("c", 30.0), dict(scales=3), dict(c=30.0, reduction="mean"), dict(subsample=1), dict(subsample=None),
               dict(c=0.0), dict(alpha=-4.2), dict(c="30"), dict(alpha=True)]


@pytest.mark.parametrize("bad", BAD_OPTIONS)
def test_engine_refuses_a_bad_test_haarpsi_before_anything_runs(bad):
    from mtd_gan_amd import engine
    model = types.SimpleNamespace(test_haarpsi=bad)      # no Generator: anything past the option check would fail otherwise
    with pytest.raises(ValueError, match="test_haarpsi.*c, alpha.*subsample"):
        engine.test_MTD_GAN_Ours(model, None, _NoLoader(), torch.device("cpu"), None)


def test_engine_option_values():
    from mtd_gan_amd import engine
    opt = lambda **kw: engine._haarpsi_option(types.SimpleNamespace(**kw))          # noqa: E731
    assert opt() is None and opt(test_haarpsi=None) is None and opt(test_haarpsi=False) is None
    assert opt(test_haarpsi=True) == {}
    assert opt(test_haarpsi=dict(c=10, alpha=2.0)) == dict(c=10, alpha=2.0)
    assert opt(test_haarpsi=dict(subsample=False)) == dict(subsample=False)
    assert opt(test_haarpsi=dict(c=30.0, alpha=4.2, subsample=True)) == dict(c=30.0, alpha=4.2, subsample=True)
    for bad in BAD_OPTIONS:
        with pytest.raises(ValueError):
            opt(test_haarpsi=bad)
    assert engine._iqa_option(types.SimpleNamespace(test_haarpsi=True)) is None          # the two options do not see each other


def test_check_options_is_the_one_rule():
    """metrics.haarpsi_check_options: what the loop's option and haarpsi_each both go by (the latter before it touches a device:
    the shape and CUDA checks come first, so it is called directly here)."""
    import numpy as np
    from mtd_gan_amd import metrics as M
    assert M.HAARPSI_OPTIONS == ("c", "alpha", "subsample")
    for ok in (dict(), dict(c=10, alpha=2.0), dict(subsample=False), dict(c=30.0, alpha=4.2, subsample=True), dict(c=np.float64(3.0))):
        M.haarpsi_check_options(**ok)
    for bad in (dict(c=0.0), dict(alpha=-4.2), dict(c="30"), dict(alpha=True), dict(c=float("inf")), dict(alpha=float("nan")),
                dict(c=np.float32(30.0)), dict(alpha=torch.tensor(4.2))):
        with pytest.raises(ValueError, match="c and alpha must be positive"):
            M.haarpsi_check_options(**bad)
    for bad in (1, 0, None, "yes", np.bool_(True)):
        with pytest.raises(ValueError, match="subsample must be a bool"):
            M.haarpsi_check_options(subsample=bad)


def test_header_declares_and_lib_binds_the_entry_points(built_lib):
    from mtd_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    for n in ("mtd_haarpsi_ws_bytes", "mtd_haarpsi_each"):
        assert re.search(r"^(size_t|int) %s\(" % n, header, re.M), n
        assert n in _lib.EXPORTS and len(getattr(built_lib, n).argtypes) > 0, n
    assert len(built_lib.mtd_haarpsi_each.argtypes) == 13 and len(built_lib.mtd_haarpsi_ws_bytes.argtypes) == 5
    assert re.search(r"^#define MTD_HAARPSI_MIN_SIDE 16$", header, re.M) and re.search(r"^#define MTD_HAARPSI_PARTS 4$", header, re.M)


def test_refusals_return_before_any_launch(built_lib):
    """The refused calls touch neither their pointers nor the device."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    f, q = built_lib.mtd_haarpsi_each, built_lib.mtd_haarpsi_ws_bytes
    # (na 3, B 2, 131 x 64): subsampled a 66 x 32 map in 3 x 1 tiles, as it is a 131 x 64 map in 5 x 2; four doubles per tile
    assert q(3, 2, 131, 64, 1) == 3 * 2 * 3 * 4 * 8 and q(3, 2, 131, 64, 0) == 3 * 2 * 10 * 4 * 8
    assert q(1, 1, 16, 16, 1) == 4 * 8 and q(3, 1, 512, 512, 1) == 3 * 64 * 4 * 8 and q(3, 21845, 16, 16, 0) > 0
    for na, B, H, W, sub in ((0, 1, 64, 64, 1), (4, 1, 64, 64, 1), (3, 0, 64, 64, 1), (3, -1, 64, 64, 0), (3, 21846, 16, 16, 1),
                             (1, 65536, 16, 16, 1), (3, 1, 15, 64, 1), (3, 1, 64, 15, 1), (3, 1, 15, 64, 0), (3, 1, 64, 15, 0),
                             (1, 1, 40000, 40000, 1), (1, 1, 16, 1 << 27, 0), (1, 1, 1 << 22, 16, 0)):
        assert q(na, B, H, W, sub) == 0, (na, B, H, W, sub)
        assert f(ptrs, na, p, B, H, W, sub, 30.0, 4.2, p, p, p, None) == -1, (na, B, H, W, sub)
    assert f(None, 3, p, 1, 64, 64, 1, 30.0, 4.2, p, p, p, None) == -1
    assert f(ptrs, 3, None, 1, 64, 64, 1, 30.0, 4.2, p, p, p, None) == -1
    assert f(ptrs, 3, p, 1, 64, 64, 1, 30.0, 4.2, None, p, p, None) == -1
    assert f(ptrs, 3, p, 1, 64, 64, 1, 30.0, 4.2, p, p, None, None) == -1
    assert f((ctypes.c_void_p * 3)(p, None, p), 3, p, 1, 64, 64, 1, 30.0, 4.2, p, p, p, None) == -1
    assert f((ctypes.c_void_p * 3)(p, p, None), 3, p, 1, 64, 64, 0, 30.0, 4.2, p, None, p, None) == -1
    for c, alpha in ((0.0, 4.2), (-30.0, 4.2), (30.0, 0.0), (30.0, -1.0), (float("nan"), 4.2), (30.0, float("nan"))):
        assert f(ptrs, 3, p, 1, 64, 64, 1, c, alpha, p, p, p, None) == -1, (c, alpha)


def test_python_surface_refusals_without_a_device():
    from mtd_gan_amd import metrics as M
    x = torch.zeros(2, 1, 64, 64)
    for fn in (M.haarpsi_each, M.haarpsi_per_slice, M.compute_HaarPSI):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(x, x, x)
        with pytest.raises(AssertionError):
            fn(x[:1], x, x)
        with pytest.raises(AssertionError):
            fn(x[:, :, :32], x, x)
        with pytest.raises(AssertionError):
            fn(x[0], x[0], x[0])
    with pytest.raises(NotImplementedError):
        M.compute_HaarPSI(x, x, x, data_range=255.0)
    assert M.HAARPSI_MIN_SIDE == R.MIN_SIDE == 16
    assert M.IQA_METRICS == ("ms_ssim", "vif", "gmsd") and M.IQA_PARTS == 20          # the neighbours stay as they are
