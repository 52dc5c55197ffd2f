"""Host side of the test loop's PNG output without a GPU: the encoder against an independent decoder (and PIL where
it imports), the numpy restatement of the 8-bit mode against matplotlib's imsave itself, the file names, the writer's error
path, and the library's new entry points (declared, bound, exported, refusing bad arguments before any launch)."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

import _png_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtd_gray_png_rows_ws_bytes", "mtd_gray_png_rows")


# ------------------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1), (37, 91), (64, 64)])
def test_encode_png_round_trips(shape, depth):
    from mtd_gan_amd import image_io
    H, W = shape
    g = np.random.RandomState(H * 1000 + W + depth)
    a = g.rand(1, H, W).astype(np.float32) * 1.5 - 0.25
    rows = P.rows(a, depth)[0]
    assert rows.shape == (H, image_io.row_bytes(W, depth))
    want = P.levels8(a[0]) if depth == 8 else P.levels16(a[0])
    for level in (1, 6):
        data = image_io.encode_png(rows, H, W, depth, level)
        assert isinstance(data, bytes)
        got, d = P.decode_png(data)
        assert d == depth and got.dtype == want.dtype and np.array_equal(got, want)
    assert image_io.encode_png(rows.tobytes(), H, W, depth, 6) == data          # bytes and arrays alike
    with pytest.raises(ValueError):
        image_io.encode_png(rows.tobytes()[:-1], H, W, depth, 6)
    with pytest.raises(ValueError):
        image_io.encode_png(rows, H, W, 4, 6)
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    assert im.size == (W, H) and im.mode in ("L", "I;16", "I;16B", "I")
    assert np.array_equal(np.asarray(im).astype(np.uint16), want.astype(np.uint16))


def test_the_gray_table_is_not_the_identity():
    from mtd_gan_amd import image_io
    assert np.array_equal(image_io.GRAY_LUT, P.LUT) and P.LUT.dtype == np.uint8
    below = np.nonzero(P.LUT != np.arange(256))[0]
    assert len(below) == 24 and list(below[:3]) == [33, 37, 41] and (P.LUT[below] == below - 1).all()
    assert P.LUT[0] == 0 and P.LUT[255] == 255


# ------------------------------------------------------------------------------- the restatement against matplotlib
def _imsave_red(a):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from PIL import Image
    buf = io.BytesIO()
    plt.imsave(buf, a, cmap="gray", format="png")
    rgba = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    assert rgba.shape == a.shape + (4,) and (rgba[..., 3] == 255).all()
    assert np.array_equal(rgba[..., 0], rgba[..., 1]) and np.array_equal(rgba[..., 0], rgba[..., 2])
    return rgba[..., 0]


def _slices_512():
    """24 slices of 512 x 512: uniform in [0, 1); stretched and clipped to exact 0 / 1 plateaus; scaled to [-1, 2]."""
    for seed in range(24):
        a = np.random.RandomState(seed).rand(512, 512).astype(np.float32)
        if seed % 3 == 1:
            a = np.clip(a * np.float32(1.5) - np.float32(0.25), 0, 1).astype(np.float32)
        elif seed % 3 == 2:
            a = (a * np.float32(3) - np.float32(1)).astype(np.float32)
        yield f"512^2 seed {seed}", a


def _mixed_sizes():
    """40 images: ten each of 512^2, 64^2, 37 x 91 and 16 x 16 (normal deviates), the last 16 x 16 a constant."""
    for shape in ((512, 512), (64, 64), (37, 91), (16, 16)):
        for seed in range(10):
            a = np.random.RandomState(1000 + 10 * shape[1] + seed).randn(*shape).astype(np.float32)
            if shape == (16, 16) and seed == 9:
                a = np.full(shape, 0.375, dtype=np.float32)
            yield f"{shape} seed {seed}", a


def test_restatement_equals_imsave():
    """The cause of the few one-level differences a plain float32 restatement shows was found in Normalize.__call__: the in-place
    `resdat -= vmin; resdat /= (vmax - vmin)` run with float64 scalars (numpy 2 promotes the operation to float64 and rounds the
    result back to float32), so the divisor vmax - vmin is never rounded to float32.  With that the restatement is matplotlib's
    arithmetic and EVERY pixel must be equal."""
    pytest.importorskip("matplotlib")
    pytest.importorskip("PIL.Image")
    pixels = 0
    for tag, a in list(_slices_512()) + list(_mixed_sizes()):
        got, want = P.levels8(a), _imsave_red(a)
        differ = int((got != want).sum())
        pixels += a.size
        assert differ == 0, f"{tag}: {differ} of {a.size} pixels differ from imsave"
    assert pixels == 34 * 512 * 512 + 10 * (64 * 64 + 37 * 91 + 16 * 16)


def test_restatement_of_the_16_bit_mode():
    a = np.array([[-0.5, 0.0, 1.0, 1.5, 0.5, 0.25, 1.0 / 65535, 2.5 / 65535, 3.5 / 65535, np.nan, np.inf, -np.inf]], dtype=np.float32)
    want = [0, 0, 65535, 65535, np.rint(np.float32(0.5) * np.float32(65535)), np.rint(np.float32(0.25) * np.float32(65535)), 1,
            np.rint(np.float32(2.5 / 65535) * np.float32(65535)), np.rint(np.float32(3.5 / 65535) * np.float32(65535)), 0, 0, 0]
    assert P.levels16(a).tolist() == [[int(v) for v in want]]
    assert P.levels16(np.float32([[0.5]]))[0, 0] == 32768          # 32767.5: the tie goes to the even level
    r = P.rows(a[None], 16)
    assert r.shape == (1, 1, 25) and r[0, 0, 0] == 0 and list(r[0, 0, 5:7]) == [255, 255] and list(r[0, 0, 13:15]) == [0, 1]


def test_restatement_handles_non_finite_and_constant_images():
    a = np.array([[0.0, 1.0, np.nan, np.inf], [0.5, -np.inf, 0.25, 1.0]], dtype=np.float32)
    assert P.levels8(a).tolist() == [[0, 255, 0, 0], [int(P.LUT[128]), 0, int(P.LUT[64]), 255]]
    assert (P.levels8(np.full((3, 5), 7.0, dtype=np.float32)) == P.LUT[0]).all()
    assert (P.levels8(np.full((2, 2), np.nan, dtype=np.float32)) == 0).all()
    big = np.array([[-3e38, 3e38, 0.0]], dtype=np.float32)           # vmax - vmin overflows float32, not the float64 divisor
    assert P.levels8(big).tolist() == [[0, 255, int(P.LUT[128])]]    # (x - vmin itself rounds to float32 infinity at the top)


# --------------------------------------------------------------------------------------------------------------- names
def test_png_names():
    from mtd_gan_amd import image_io
    dcm = "/data/test/L506/quarter_1mm/L506_QD_1_1.CT.0003.0007.2015.12.22.20.45.42.541197.358793241_0007.dcm"
    full = dcm.replace("quarter", "full").replace("_0007.dcm", "_0008.dcm")
    ref = (dcm.split("_")[-1].replace(".dcm", "_gt_n_20.png"), full.split("_")[-1].replace(".dcm", "_gt_n_100.png"),
           dcm.split("_")[-1].replace(".dcm", "_pred_n_100.png"))                          # engine.py:157-159
    assert image_io.png_names(dcm, full) == ref == ("0007_gt_n_20.png", "0008_gt_n_100.png", "0007_pred_n_100.png")
    assert image_io.png_names("L333_QD_3_1.CT.0004.0042.IMA", "L333_FD_3_1.CT.0004.0042.IMA") == (
        "1.CT.0004.0042_gt_n_20.png", "1.CT.0004.0042_gt_n_100.png", "1.CT.0004.0042_pred_n_100.png")
    assert image_io.png_names("L000_0001.dcm") == ("0001_gt_n_20.png", "0001_gt_n_100.png", "0001_pred_n_100.png")
    assert image_io.png_names(None, None, 5) == ("slice_5_gt_n_20.png", "slice_5_gt_n_100.png", "slice_5_pred_n_100.png")
    assert image_io.png_names() == ("slice_0_gt_n_20.png", "slice_0_gt_n_100.png", "slice_0_pred_n_100.png")
    assert "collide" in image_io.png_names.__doc__


# -------------------------------------------------------------------------------------------------------------- writer
def test_writer_writes_and_close_raises_the_first_worker_error(tmp_path):
    from mtd_gan_amd import image_io
    a = np.random.RandomState(5).rand(6, 37, 91).astype(np.float32)
    rows8, rows16 = P.rows(a, 8), P.rows(a, 16)
    w = image_io.PngWriter(threads=2, level=1)
    for i in range(6):
        w.submit(str(tmp_path / f"a{i}.png"), rows8[i], 37, 91, 8)
        w.submit(str(tmp_path / f"b{i}.png"), rows16[i], 37, 91, 16)
    w.close()
    w.close()                                                                               # a second close is a no-op
    for i in range(6):
        assert np.array_equal(P.decode_png((tmp_path / f"a{i}.png").read_bytes())[0], P.levels8(a[i]))
        assert np.array_equal(P.decode_png((tmp_path / f"b{i}.png").read_bytes())[0], P.levels16(a[i]))
    with pytest.raises(RuntimeError):
        w.submit(str(tmp_path / "late.png"), rows8[0], 37, 91, 8)
    assert w.waited >= 0.0

    bad = image_io.PngWriter(threads=2, level=1)
    bad.submit(str(tmp_path / "ok.png"), rows8[0], 37, 91, 8)
    bad.submit(str(tmp_path / "no_such_directory" / "x.png"), rows8[1], 37, 91, 8)
    bad.submit(str(tmp_path / "short.png"), rows8[2][:-1], 37, 91, 8)
    with pytest.raises((OSError, ValueError)):
        bad.close()
    assert (tmp_path / "ok.png").exists() and not (tmp_path / "short.png").exists()


def test_writer_threads_come_from_the_environment_not_the_machine(monkeypatch):
    from mtd_gan_amd import image_io
    for name in ("OMP_NUM_THREADS", "MAX_JOBS", "CMAKE_BUILD_PARALLEL_LEVEL"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(os, "cpu_count", lambda: 4096)
    assert image_io.default_threads() == 4
    monkeypatch.setenv("MAX_JOBS", "6")
    assert image_io.default_threads() == 6
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert image_io.default_threads() == 3
    monkeypatch.setenv("OMP_NUM_THREADS", "4096")
    assert image_io.default_threads() == 32
    w = image_io.PngWriter(level=1)
    assert w.threads == 32
    w.close()
    with pytest.raises(ValueError):
        image_io.PngWriter(threads=-1)


# ------------------------------------------------------------------------------------------------------ public checks
def test_cpu_tensors_and_wrong_dtypes_are_refused_by_name():
    from mtd_gan_amd import image_io
    with pytest.raises(RuntimeError, match="gray_png_rows.*CUDA"):
        image_io.gray_png_rows(torch.zeros(1, 4, 4))
    with pytest.raises(RuntimeError, match="gray_png_rows"):
        image_io.gray_png_rows(np.zeros((1, 4, 4), dtype=np.float32))


def test_the_switch_is_checked_before_the_loop_starts(tmp_path):
    from mtd_gan_amd import engine

    class M:
        pass

    assert engine._PngSink.from_model(M(), str(tmp_path)) is None
    for falsy in (False, None, 0, {}):
        m = M()
        m.test_save_png = falsy
        assert engine._PngSink.from_model(m, str(tmp_path)) is None
    for bad in ("yes", dict(depth=12), dict(bits=8)):
        m = M()
        m.test_save_png = bad
        with pytest.raises(ValueError, match="test_save_png"):
            engine._PngSink.from_model(m, str(tmp_path))
    m = M()
    m.test_save_png = True
    with pytest.raises(ValueError, match="save_dir"):
        engine._PngSink.from_model(m, None)
    m.test_save_png = dict(depth=16, level=1, threads=3)
    sink = engine._PngSink.from_model(m, str(tmp_path / "out"))
    assert (sink.depth, sink.writer.level, sink.writer.threads) == (16, 1, 3) and (tmp_path / "out").is_dir()
    sink.writer.close()


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
    for n in NEW:
        assert re.search(r"^(size_t|int) %s\(" % n, header, re.M), n
        assert n in _lib.EXPORTS and hasattr(built_lib, n) and len(getattr(built_lib, n).argtypes) > 0, n
    assert len(built_lib.mtd_gray_png_rows.argtypes) == 9 and len(built_lib.mtd_gray_png_rows_ws_bytes.argtypes) == 4


def test_refusals_return_before_any_launch(built_lib):
    """The refused calls touch neither their pointers nor the device: they can be made here, with addresses of host memory."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    f, ws = built_lib.mtd_gray_png_rows, built_lib.mtd_gray_png_rows_ws_bytes
    assert ws(3, 512, 512, 8) == (3 * 64 + 3) * 8              # 64 partial limits per 512 x 512 image and the limits
    assert ws(70, 8, 8, 8) == (70 + 70) * 8 and ws(1, 1, 7, 8) == 16 and ws(2, 100, 77, 8) == (2 * 2 + 2) * 8
    assert ws(3, 512, 512, 16) == 0 and ws(3, 512, 512, 12) == 0 and ws(0, 4, 4, 8) == 0 and ws(1, 0, 4, 8) == 0
    assert ws(1 << 13, 512, 512, 8) == 0                        # 2^31 bytes of scanlines and more
    for n, H, W, depth in ((0, 4, 4, 8), (1, 0, 4, 8), (1, 4, -1, 8), (1, 4, 4, 12), (1, 4, 4, 0), (1 << 13, 512, 512, 8), (1 << 12, 512, 512, 16)):
        assert f(p, n, H, W, depth, p, p, p, None) == -1, (n, H, W, depth)
    assert f(None, 1, 4, 4, 8, p, p, p, None) == -1 and f(p, 1, 4, 4, 8, p, None, p, None) == -1
    assert f(p, 1, 4, 4, 8, None, p, p, None) == -1 and f(p, 1, 4, 4, 8, p, p, None, None) == -1     # depth 8 needs lut and ws
    assert f(p + 2, 1, 4, 4, 8, p, p, p, None) == -2 and f(p, 1, 4, 4, 8, p, p, p + 4, None) == -2
    assert f(p + 2, 1, 4, 4, 16, None, p, None, None) == -2
