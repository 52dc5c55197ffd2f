"""Host side of the per-slice metrics without a GPU: the two entry points are declared, bound and exported, the
argument refusals that need no device (through the built library's ABI), the public functions' argument checks, and the host
arithmetic that turns the per-image sums into the (input, gt, pred) triples."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtd_image_metrics_each_ws_bytes", "mtd_image_metrics_each", "mtd_patch_gram_l1_each")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    return _lib.lib()


def test_header_declares_and_lib_binds_the_entry_points(built_lib):
    from mtd_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    for n in NEW:
        assert re.search(r"^(size_t|int) %s\(" % n, header, re.M), n
        assert n in _lib.EXPORTS and len(getattr(built_lib, n).argtypes) > 0, n
    assert len(built_lib.mtd_image_metrics_each.argtypes) == 10 and len(built_lib.mtd_patch_gram_l1_each.argtypes) == 10
    assert re.search(r"mtd_patch_gram_l1_each\(const float\* X, const float\* Y, int B, int h, int w, int C, double\* out, long long out_stride",
                     header)


def test_refusals_return_before_any_launch(built_lib):
    """The refused calls touch neither their pointers nor the device: they can be made here, with addresses of host memory."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    flags = (ctypes.c_int * 3)(0, 0, 1)
    f = built_lib.mtd_image_metrics_each
    assert built_lib.mtd_image_metrics_each_ws_bytes(3, 8, 512, 512) == 3 * 8 * 256 * 2 * 8
    assert built_lib.mtd_image_metrics_each_ws_bytes(4, 8, 512, 512) == 0
    for na, B in ((0, 1), (4, 1), (1, 0), (3, 21846)):
        assert f(ptrs, na, p, B, 32, 32, flags, p, p, None) == -1, (na, B)
    assert f(ptrs, 2, None, 1, 32, 32, flags, p, p, None) == -1
    g = built_lib.mtd_patch_gram_l1_each
    assert g(p, p, 2, 16, 16, 64, p, 0, p, None) == -1
    assert g(p, p, 2, 15, 16, 64, p, 1, p, None) == -1
    assert g(p, p, 2, 16, 16, 96, p, 1, p, None) == -1
    assert g(p + 4, p, 2, 16, 16, 64, p, 1, p, None) == -2


def test_cpu_tensors_and_mismatched_shapes_are_refused():
    from mtd_gan_amd import metrics as M
    import _perceptual_ref as R
    v = M.VGG19Features(R.seeded_state_dict(1))
    x = torch.zeros(2, 1, 256, 256)
    for fn in (M.pixel_metrics_each, M.pixel_metrics_per_slice):
        with pytest.raises(RuntimeError):
            fn(x, x, x)
        with pytest.raises(AssertionError):
            fn(x[:1], x, x)
        with pytest.raises(AssertionError):
            fn(x[:, 0], x[:, 0], x[:, 0])
    with pytest.raises(RuntimeError):
        M.perceptual_metrics_per_slice(x, x, x, v)
    with pytest.raises(AssertionError):
        M.perceptual_metrics_per_slice(x[:1], x, x, v)
    with pytest.raises(TypeError):
        M.perceptual_metrics_per_slice(x, x, x, None)
    maps = torch.zeros(2, 16, 16, 64)
    with pytest.raises(ValueError):                      # as patch_gram_l1: CPU maps, mismatched maps
        M.patch_gram_l1_each(maps, maps)
    with pytest.raises(ValueError):
        M.patch_gram_l1_each(maps, maps[:1])


def test_triples_from_the_sums_use_the_formulas_of_pixel_metrics():
    from mtd_gan_amd import metrics as M
    n = 100 * 77
    sums = [[[3.25, 6000.5], [0.75, 7000.25]], [[0.0, float(n)], [0.0, float(n)]], [[1e-3, 7699.0], [2.5, 7600.0]]]
    t = M._slice_triples(sums, n)
    assert sorted(t) == ["psnr", "rmse", "ssim"] and all(len(v) == 2 and all(len(e) == 3 for e in v) for v in t.values())
    for i in range(2):
        for k in range(3):
            sse, ssum = sums[k][i]
            assert t["rmse"][i][k] == float(np.sqrt(np.float32(sse / n)))
            assert t["psnr"][i][k] == M._psnr(sse, n, 1.0)
            assert t["ssim"][i][k] == float(np.float32(ssum / n))
    assert t["rmse"][0][1] == 0.0 and t["ssim"][1][1] == 1.0 and abs(t["psnr"][0][1] - 100.0) < 1e-4
