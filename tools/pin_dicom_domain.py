"""Golden data for the stored-pixel <-> HU <-> window kernels (tests/test_dicom_domain_{cpu,gpu}.py).  TEST
INFRASTRUCTURE: needs the reference checkout that oracle/_refboot.py points at; it is not needed to run the tests.

    python tools/pin_dicom_domain.py

Runs the reference's own get_pixels_hu (create_datasets/Mayo.py) and dicom_denormalize + save_dicom (utils.py) -- plain numpy --
with a stub `pydicom` whose read_file / dcmread return an object that carries pixel_array, RescaleSlope, RescaleIntercept and a
save_as that keeps what it is given, and empty `monai.transforms` / `monai.data` modules.  Writes tests/golden/dicom_domain.npz:
  meta                 JSON: the cases, (slope, intercept) with their Python types (int or float, as a DICOM header gives them)
  hu{j}.stored / .hu   stored words (int16 or uint16, (16, 24)) and get_pixels_hu's int16 answer
  map{j}.v / .raw / .clipped   a float32 value map (16, 40), and save_dicom's PixelData (int16) after dicom_denormalize(v, a_min,
                       a_max) and after dicom_denormalize(clip(v, 0, 1), a_min, a_max)
Every case stays inside int16 at every cast (checked here in float64), so the reference's casts are defined."""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refboot  # noqa: E402

PAIRS = [(1, -1024), (1.0, -1024.0), (2, -1000), (0.5, -1024), (1.5, -8192)]
WINDOWS = [(-1024.0, 3072.0), (-160.0, 240.0)]
HU_SHAPE, MAP_SHAPE = (16, 24), (16, 40)


class _Dcm:
    def __init__(self, pixels, slope, intercept):
        self.pixel_array, self.RescaleSlope, self.RescaleIntercept = pixels, slope, intercept
        self.saved = None

    def save_as(self, path):
        self.saved = (path, np.frombuffer(self.PixelData, dtype=np.int16).copy())


def boot():
    _refboot.boot()
    mo = sys.modules["monai"]
    mo.transforms = sys.modules["monai.transforms"] = types.ModuleType("monai.transforms")
    mo.data = sys.modules["monai.data"] = types.ModuleType("monai.data")
    mo.data.Dataset, mo.data.list_data_collate = object, None
    files = {}
    pd = sys.modules["pydicom"]
    pd.read_file = pd.dcmread = lambda path: files[path]
    from create_datasets.Mayo import get_pixels_hu
    from utils import dicom_denormalize, save_dicom
    return files, get_pixels_hu, dicom_denormalize, save_dicom


def inside(x):
    assert np.all(np.abs(np.asarray(x, dtype=np.float64)) < 32767), "a case leaves int16"


def stored_words(rng, slope, intercept, unsigned):
    """Words whose every intermediate stays inside int16, with the padding value, negative products and both signs."""
    n = HU_SHAPE[0] * HU_SHAPE[1]
    room = (32000 - abs(intercept)) / abs(slope)
    lo, hi = -int(min(room, 9000)), int(min(room, 20000))
    p = rng.integers(lo, hi, size=n).astype(np.int64)
    p[:8] = [-2000, -2000, -1001, -1, -3, 1, 3, 1001]              # padding; odd negatives: trunc(-500.5) = -500, floor = -501
    p[8:16] = [0, -7, -333, lo, hi - 1, -1999, -2001, 2000]
    inside(slope * np.where(p == -2000, 0, p).astype(np.float64))
    inside(np.trunc(slope * np.where(p == -2000, 0, p).astype(np.float64)) + intercept)
    p = p.astype(np.int16).reshape(HU_SHAPE)
    return p.view(np.uint16).copy() if unsigned else p


def value_map(rng):
    n = MAP_SHAPE[0] * MAP_SHAPE[1]
    v = rng.uniform(-0.2, 1.2, size=n).astype(np.float32)
    v[:401] = np.arange(401, dtype=np.float32) / np.float32(400)   # exactly k / 400: the window's own grid
    v[401:409] = [-0.2, -1e-3, -0.0, 0.0, 1.0, 1.0 + 1e-6, 1.2, 0.5]
    return v.reshape(MAP_SHAPE)


def main():
    files, get_pixels_hu, dicom_denormalize, save_dicom = boot()
    rng = np.random.default_rng(20241019)
    arrays, meta = {}, dict(hu_cases=[], map_cases=[])
    for slope, intercept in PAIRS:
        for unsigned in (False, True):
            j = len(meta["hu_cases"])
            words = stored_words(rng, slope, intercept, unsigned)
            if unsigned:
                assert (words == 63536).sum() >= 2                 # -2000 as a uint16 array holds it
            files["in"] = _Dcm(words.copy(), slope, intercept)
            hu = get_pixels_hu("in")
            assert hu.dtype == np.int16 and hu.shape == HU_SHAPE
            arrays[f"hu{j}.stored"], arrays[f"hu{j}.hu"] = words, hu
            meta["hu_cases"].append(dict(slope=slope, intercept=intercept, dtype=str(words.dtype)))
    for slope, intercept in PAIRS:
        for a_min, a_max in WINDOWS:
            j = len(meta["map_cases"])
            v = value_map(rng)
            got = []
            for x in (v, np.clip(v, 0, 1)):
                hu = dicom_denormalize(x, a_min, a_max)
                assert hu.dtype == np.float32
                inside(hu.astype(np.float64) - intercept)
                inside((hu.astype(np.float64) - intercept) / slope)
                files["orig"] = _Dcm(None, slope, intercept)
                save_dicom("orig", hu, "saved")
                path, pixels = files["orig"].saved
                assert path == "saved" and pixels.size == v.size
                got.append(pixels.reshape(MAP_SHAPE))
            arrays[f"map{j}.v"], arrays[f"map{j}.raw"], arrays[f"map{j}.clipped"] = v, got[0], got[1]
            meta["map_cases"].append(dict(slope=slope, intercept=intercept, a_min=a_min, a_max=a_max))
    out = os.path.join(ROOT, "tests", "golden", "dicom_domain.npz")
    np.savez_compressed(out, meta=np.array(json.dumps(meta)), **arrays)
    print(f"{out}: {len(meta['hu_cases'])} HU cases, {len(meta['map_cases'])} value maps, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
