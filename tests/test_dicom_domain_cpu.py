"""Stored DICOM pixel values <-> HU <-> window without a GPU: the numpy restatement of tests/_dicom_ref.py against
what the reference's own get_pixels_hu and dicom_denormalize + save_dicom gave (tests/golden/dicom_domain.npz, written by
tools/pin_dicom_domain.py) -- integers, so equality -- the library's new entry points (declared, bound, exported, refusing bad
arguments before any launch), and the refusals of dicom_io and of the two test-loop switches."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _dicom_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtd_stored_to_hu", "mtd_stored_to_window", "mtd_window_to_stored")
PAIRS = [(1, -1024), (1.0, -1024.0), (2, -1000), (0.5, -1024), (1.5, -8192)]


# --------------------------------------------------------------------------------------------- restatement and fixture
def test_restatement_reproduces_the_reference_hu():
    meta, z = D.load()
    assert len(meta["hu_cases"]) == 10
    for j, c in enumerate(meta["hu_cases"]):
        stored, want = z[f"hu{j}.stored"], z[f"hu{j}.hu"]
        assert str(stored.dtype) == c["dtype"] and want.dtype == np.int16
        got = D.stored_to_hu(stored[None], (c["slope"], c["intercept"]))[0]
        assert got.dtype == np.int16 and np.array_equal(got, want), (j, c)


def test_restatement_reproduces_the_reference_pixel_data():
    meta, z = D.load()
    assert len(meta["map_cases"]) == 10
    for j, c in enumerate(meta["map_cases"]):
        v = z[f"map{j}.v"]
        r = (c["slope"], c["intercept"])
        raw = D.window_to_stored(v[None], r, c["a_min"], c["a_max"], clip=False)[0]
        clipped = D.window_to_stored(v[None], r, c["a_min"], c["a_max"], clip=True)[0]
        assert np.array_equal(raw, z[f"map{j}.raw"]), (j, c)
        assert np.array_equal(clipped, z[f"map{j}.clipped"]), (j, c)
        assert not np.array_equal(z[f"map{j}.raw"], z[f"map{j}.clipped"])          # the entries outside [0, 1] are there


def test_fixture_holds_the_cases_that_matter():
    meta, z = D.load()
    seen = [(c["slope"], c["intercept"]) for c in meta["hu_cases"]]
    assert seen == [p for p in PAIRS for _ in range(2)]
    assert [type(s) for s, _ in seen[:4]] == [int, int, float, float]                # 1 and 1.0 as a header gives them
    assert [(c["slope"], c["intercept"]) for c in meta["map_cases"]] == [p for p in PAIRS for _ in range(2)]
    assert {(c["a_min"], c["a_max"]) for c in meta["map_cases"]} == {(-1024.0, 3072.0), (-160.0, 240.0)}
    for j, c in enumerate(meta["hu_cases"]):
        stored, hu = z[f"hu{j}.stored"], z[f"hu{j}.hu"]
        if c["dtype"] == "uint16":
            assert (stored == 63536).sum() >= 2                                       # -2000 in a uint16 array
        words = stored.view(np.int16) if stored.dtype == np.uint16 else stored
        assert (hu[words == -2000] == np.int16(c["intercept"])).all() and (words == -2000).any()
        if c["slope"] not in (1, 2):                                                  # negative products with a fraction:
            prod = c["slope"] * np.where(words == -2000, 0, words).astype(np.float64)
            frac = (prod < 0) & (prod != np.floor(prod))
            assert frac.any()                                                         # trunc and floor differ there,
            assert np.array_equal(hu[frac], (np.trunc(prod[frac]) + c["intercept"]).astype(np.int16))      # and the reference truncates
    for j in range(10):
        v = z[f"map{j}.v"]
        assert (v < 0).any() and (v > 1).any() and v.dtype == np.float32
        assert np.array_equal(v.reshape(-1)[:401], np.arange(401, dtype=np.float32) / np.float32(400))
    assert os.path.getsize(D.GOLD) < 100 * 1024


def test_truncation_loses_the_window_grid_and_nearest_keeps_it():
    """Why `rounding="nearest"` exists.  400 * fl(k / 400) is not k for every k in float32, so on the training window [-160, 240]
    the reference's truncating cast returns HU - 1 (HU + 1 below zero) for a few of the 401 HU values of the window's own grid;
    on its own pair [-1024, 3072], whose width is a power of two, every product is exact.  Rounding to nearest recovers every
    value on both."""
    for (a_min, a_max), exact in (((-1024.0, 3072.0), True), ((-160.0, 240.0), False)):
        hu = np.arange(int(a_min), int(a_max) + 1).astype(np.int16)[None]
        v = D.window(hu, a_min, a_max)
        back = D.window_to_stored(v, (1, 0), a_min, a_max)
        assert np.array_equal(back, hu) == exact
        assert int((back != hu).sum()) == (0 if exact else 12)                      # -53, -52, -41, -40, 49 ... of the 401
        assert np.abs(back.astype(np.int32) - hu).max() <= 1
        assert np.array_equal(D.window_to_stored(v, (1, 0), a_min, a_max, rounding="nearest"), hu)


def test_restatement_options():
    v = np.float32([[[-0.5, 0.0, 0.00125, 0.00375, 0.5, 1.0, 2.0, np.nan]]])          # 400 v - 160: -160, -159.5, -158.5, 40
    assert D.window_to_stored(v, (1, 0), -160, 240).tolist() == [[[-160, -160, -159, -158, 40, 240, 240, -160]]]
    assert D.window_to_stored(v, (1, 0), -160, 240, rounding="nearest").tolist() == [[[-160, -160, -160, -158, 40, 240, 240, -160]]]
    assert D.window_to_stored(v, (1, 0), -160, 240, clip=False).tolist() == [[[-360, -160, -159, -158, 40, 240, 640, 0]]]
    big = np.float32([[[-100.0, 100.0]]])                                              # beyond int16: saturation
    assert D.window_to_stored(big, (1, 0), -1024, 3072, clip=False).tolist() == [[[-32768, 32767]]]
    assert D.window_to_stored(big, (0.5, 0), -1024, 3072, clip=False).tolist() == [[[-32768, 32767]]]
    ref = np.int16([[[-1000 + 1024, 0 + 1024, 240 + 1024, 241 + 1024, -160 + 1024, -161 + 1024, -2000, 3000]]])
    v = np.full((1, 1, 8), 0.5, dtype=np.float32)
    got = D.window_to_stored(v, (1, -1024), -160, 240, outside="input", reference=ref)
    assert got.tolist() == [[[24, 1064, 1064, 1265, 1064, 863, -2000, 3000]]]           # 40 HU = word 1064 inside the window
    assert D.stored_to_hu(np.uint16([[[63536, 65535, 0]]]), (1, -1024)).tolist() == [[[-1024, -1025, -1024]]]
    assert D.stored_to_hu(np.int16([[[32767, -3]]]), (1, 10)).tolist() == [[[-32759, 7]]]                    # 16-bit wrap-around
    assert D.stored_to_hu(np.int16([[[30000, -30000, -3]]]), (2, 0)).tolist() == [[[32767, -32768, -6]]]     # saturation


# ------------------------------------------------------------------------------------------------------------- library
@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    return _lib.lib()


def test_library_exports_the_entry_points(built_lib):
    from mtd_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    build = open(os.path.join(ROOT, "mtd-gan_amd", "_build.py")).read()
    assert '"dicom_domain.hip"' in build and os.path.exists(os.path.join(ROOT, "mtd-gan_amd", "csrc", "dicom_domain.hip"))
    for n in NEW:
        assert re.search(r"^int %s\(" % n, header, re.M), n
        assert n in _lib.EXPORTS and hasattr(built_lib, n) and len(getattr(built_lib, n).argtypes) > 0, n
    assert [len(getattr(built_lib, n).argtypes) for n in NEW] == [7, 10, 13]
    assert "SATURATES" in header


def test_refusals_return_before_any_launch(built_lib):
    """The refused calls touch neither their pointers nor the device: they can be made here, with addresses of host memory."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    hu, win, back = (getattr(built_lib, n) for n in NEW)
    for S, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1 << 13, 512, 512), (2, 1 << 16, 1 << 15)):       # the last two: 2^31 pixels and more
        assert hu(p, S, H, W, p, p, None) == -1, (S, H, W)
        assert win(p, S, H, W, p, -160.0, 240.0, p, None, None) == -1, (S, H, W)
        assert back(p, S, H, W, p, -160.0, 240.0, 1, 0, 0, None, p, None) == -1, (S, H, W)
    assert hu(None, 1, 4, 4, p, p, None) == -1 and hu(p, 1, 4, 4, None, p, None) == -1 and hu(p, 1, 4, 4, p, None, None) == -1
    assert win(None, 1, 4, 4, p, -160.0, 240.0, p, None, None) == -1 and win(p, 1, 4, 4, p, -160.0, 240.0, None, None, None) == -1
    assert win(p, 1, 4, 4, p, 240.0, 240.0, p, None, None) == -1 and win(p, 1, 4, 4, p, float("nan"), 240.0, p, None, None) == -1
    assert back(p, 1, 4, 4, p, 240.0, -160.0, 1, 0, 0, None, p, None) == -1
    assert back(None, 1, 4, 4, p, -160.0, 240.0, 1, 0, 0, None, p, None) == -1
    assert back(p, 1, 4, 4, p, -160.0, 240.0, 1, 2, 0, None, p, None) == -1          # rounding
    assert back(p, 1, 4, 4, p, -160.0, 240.0, 1, 0, 2, p, p, None) == -1             # outside
    assert back(p, 1, 4, 4, p, -160.0, 240.0, 1, 0, 1, None, p, None) == -1          # outside = input without the input
    assert hu(p + 1, 1, 4, 4, p, p, None) == -2 and hu(p, 1, 4, 4, p + 4, p, None) == -2 and hu(p, 1, 4, 4, p, p + 1, None) == -2
    assert win(p, 1, 4, 4, p, -160.0, 240.0, p + 2, None, None) == -2 and win(p, 1, 4, 4, p, -160.0, 240.0, p, p + 1, None) == -2
    assert back(p + 2, 1, 4, 4, p, -160.0, 240.0, 1, 0, 0, None, p, None) == -2
    assert back(p, 1, 4, 4, p, -160.0, 240.0, 1, 0, 1, p + 1, p, None) == -2


# ------------------------------------------------------------------------------------------------------ public checks
def test_cpu_tensors_and_wrong_dtypes_are_refused_by_name():
    from mtd_gan_amd import dicom_io
    s, v = torch.zeros(1, 4, 4, dtype=torch.int16), torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="stored_to_hu.*CUDA"):
        dicom_io.stored_to_hu(s, (1, -1024))
    with pytest.raises(RuntimeError, match="stored_to_window.*CUDA"):
        dicom_io.stored_to_window(s, (1, -1024))
    with pytest.raises(RuntimeError, match="window_to_stored.*CUDA"):
        dicom_io.window_to_stored(v, (1, -1024), -160.0, 240.0)
    with pytest.raises(RuntimeError, match="stored_to_hu"):
        dicom_io.stored_to_hu(np.zeros((1, 4, 4), dtype=np.int16), (1, -1024))
    with pytest.raises(RuntimeError, match="stored_to_hu.*float32"):
        dicom_io.stored_to_hu(v, (1, -1024))
    with pytest.raises(RuntimeError, match="stored_to_window.*int32"):
        dicom_io.stored_to_window(s.int(), (1, -1024))
    with pytest.raises(RuntimeError, match="window_to_stored.*float16"):
        dicom_io.window_to_stored(v.half(), (1, -1024), -160.0, 240.0)
    with pytest.raises(RuntimeError, match="denoise_series.*float32"):
        dicom_io.denoise_series(lambda x: x, np.zeros((2, 4, 4), dtype=np.float32), (1, -1024), a_min=-160.0, a_max=240.0)


def test_options_are_checked_before_the_tensors():
    from mtd_gan_amd import dicom_io
    v = torch.zeros(1, 4, 4)
    with pytest.raises(ValueError, match="rounding"):
        dicom_io.window_to_stored(v, (1, 0), -160.0, 240.0, rounding="floor")
    with pytest.raises(ValueError, match="outside"):
        dicom_io.window_to_stored(v, (1, 0), -160.0, 240.0, outside="keep")
    with pytest.raises(ValueError, match="reference"):
        dicom_io.window_to_stored(v, (1, 0), -160.0, 240.0, outside="input")
    with pytest.raises(ValueError, match="a_max"):
        dicom_io.window_to_stored(v, (1, 0), 240.0, -160.0)
    s = np.zeros((2, 4, 4), dtype=np.int16)
    with pytest.raises(ValueError, match="rounding"):
        dicom_io.denoise_series(lambda x: x, s, (1, 0), a_min=-160.0, a_max=240.0, rounding="floor")
    with pytest.raises(ValueError, match="outside"):
        dicom_io.denoise_series(lambda x: x, s, (1, 0), a_min=-160.0, a_max=240.0, outside="keep")
    with pytest.raises(ValueError, match="batch"):
        dicom_io.denoise_series(lambda x: x, s, (1, 0), a_min=-160.0, a_max=240.0, batch=0)
    with pytest.raises(ValueError, match="S, H, W"):
        dicom_io.denoise_series(lambda x: x, s[0], (1, 0), a_min=-160.0, a_max=240.0)
    with pytest.raises(ValueError, match="out must"):
        dicom_io.denoise_series(lambda x: x, s, (1, 0), a_min=-160.0, a_max=240.0, out=np.zeros((2, 4, 4), dtype=np.uint16))


def test_rescale_table():
    from mtd_gan_amd import dicom_io
    cpu = torch.device("cpu")
    t = dicom_io.rescale_table((2, -1000), 3, cpu)
    assert t.dtype == torch.float64 and t.tolist() == [[2.0, -1000.0]] * 3 and t.is_contiguous()
    t = dicom_io.rescale_table(np.float32([[1, -1024], [0.5, -8192]]), 2, cpu)
    assert t.dtype == torch.float64 and t.tolist() == [[1.0, -1024.0], [0.5, -8192.0]]
    assert dicom_io.rescale_table(torch.tensor([[1.5, 3.0]]), 1, cpu).tolist() == [[1.5, 3.0]]
    for bad in ([[1, -1024], [1, -1024]], [1, -1024, 0], [[1, -1024, 0]] * 3, 1.0, []):
        with pytest.raises(ValueError, match="rescale"):
            dicom_io.rescale_table(bad, 3, cpu)


class _Model:
    class Generator:
        @staticmethod
        def eval():
            pass


def test_the_switches_are_checked_before_the_loop_starts():
    from mtd_gan_amd import engine
    assert engine._StoredInput.from_model(_Model()) is None and engine._DcmSink.from_model(_Model(), None) is None
    for falsy in (False, None, 0, {}):
        m = _Model()
        m.test_from_stored = m.test_save_dcm = falsy
        assert engine._StoredInput.from_model(m) is None and engine._DcmSink.from_model(m, None) is None
    m = _Model()
    m.test_from_stored = True
    s = engine._StoredInput.from_model(m)
    assert (s.a_min, s.a_max) == (-160.0, 240.0)
    m.test_from_stored = dict(a_min=-1024, a_max=3072)
    s = engine._StoredInput.from_model(m)
    assert (s.a_min, s.a_max) == (-1024.0, 3072.0)
    for bad in ("yes", dict(window=400), dict(a_min=240.0), 7):
        m.test_from_stored = bad
        with pytest.raises(ValueError, match="test_from_stored"):
            engine._StoredInput.from_model(m)
    m.test_save_dcm = "dcm/"
    with pytest.raises(ValueError, match="test_save_dcm"):
        engine._DcmSink.from_model(m, s)
    sink = lambda path, pixels, k: None      # noqa: E731
    m.test_save_dcm = sink
    assert engine._DcmSink.from_model(m, s).write is sink


def test_the_loop_refuses_a_sink_without_stored_input_and_a_batch_without_per_slice():
    from mtd_gan_amd import engine
    calls = []
    batch = dict(n_20=torch.zeros(2, 1, 8, 8, dtype=torch.int16), n_100=torch.zeros(2, 1, 8, 8, dtype=torch.int16),
                 rescale_n_20=[[1, -1024]] * 2, rescale_n_100=[[1, -1024]] * 2)
    m = _Model()
    m.test_save_dcm = lambda *a: calls.append(a)
    with pytest.raises(ValueError, match="test_save_dcm needs model.test_from_stored"):
        engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), [batch], torch.device("cpu"), None)
    m.test_from_stored = True
    with pytest.raises(ValueError, match="test_save_dcm.*test_per_slice"):
        engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), [batch], torch.device("cpu"), None)
    m.test_save_dcm = None                                           # stored input alone: batches must say what they are
    with pytest.raises(ValueError, match="test_from_stored.*rescale_n_20"):
        engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), [dict(n_20=batch["n_20"], n_100=batch["n_100"])], torch.device("cpu"), None)
    with pytest.raises(ValueError, match="test_from_stored.*int16 or uint16"):
        engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), [dict(batch, n_20=torch.zeros(2, 1, 8, 8))], torch.device("cpu"), None)
    assert calls == []


def test_mayo_front_end_names_the_device_route():
    from mtd_gan_amd.create_datasets import Mayo
    assert "dicom_io.stored_to_hu" in Mayo.__doc__
