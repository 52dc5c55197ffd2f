"""CPU side of the per-stage tests of the power-of-two spectral kernels (csrc/resfft_any.hip): the batches of
test_spectral_pow2_stages_gpu.py really give every persistent kernel more units than workgroups, and the entry points check their
arguments before anything is launched."""
import ctypes

import pytest

import test_spectral_pow2_stages_gpu as stages

MTD_EINVAL, MTD_EALIGN = -1, -2


def test_larger_batches_exceed_every_grid():
    """At the larger batch of each side every one of the three kernels has more units than workgroups (some workgroup takes a second
    unit), at one image less at least one of them has not, and a batch of one is a single round everywhere."""
    assert set(stages.SIDES) == {64, 128, 256, 512}
    for S, (one, more) in stages.SIDES.items():
        for kernel, (units, grid) in stages.units_and_grids(S, more).items():
            assert units > grid, (S, more, kernel, units, grid)
        assert any(units <= grid for units, grid in stages.units_and_grids(S, more - 1).values()), (S, more)
        assert all(units <= grid for units, grid in stages.units_and_grids(S, one).values()), (S, one)
    # the figures of the launchers, written out: units on workgroups for (rows, mix)
    table = {S: tuple(stages.units_and_grids(S, stages.SIDES[S][1])[k] for k in ("rows", "mix")) for S in stages.SIDES}
    assert table == {64: ((544, 512), (544, 512)), 128: ((576, 512), (576, 512)), 256: ((640, 512), (640, 256)),
                     512: ((512, 256), (512, 256))}
    # a ragged last round at 128 and 256: more units than workgroups, fewer than two rounds of them
    for S in (128, 256):
        units, grid = stages.units_and_grids(S, stages.SIDES[S][1])["rows"]
        assert grid < units < 2 * grid


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__  # noqa: F401  (puts the repository root on sys.path)
    from mtd_gan_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for suffix in ("", "_h"):
        getattr(L, "mtd_rfft_rows_any" + suffix).argtypes = [vp, ci, vp, ci, ci, vp]
        getattr(L, "mtd_spec_mix_any" + suffix).argtypes = [vp, vp, vp, vp, ci, ci, vp]
        getattr(L, "mtd_irfft_rows_any" + suffix).argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, ci, vp]
    return L


@pytest.mark.parametrize("suffix", ["", "_h"])
def test_entry_points_refuse_without_a_device(lib, suffix):
    """Arguments are checked before any launch: sides other than 64 (fp32 only) / 128 / 256 / 512, pixel strides under 32 channels,
    strides and bases that 16-byte accesses cannot take."""
    fake, off8 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)
    rf = getattr(lib, "mtd_rfft_rows_any" + suffix)
    mx = getattr(lib, "mtd_spec_mix_any" + suffix)
    ir = getattr(lib, "mtd_irfft_rows_any" + suffix)
    for S in (32, 96, 1024) + ((64,) if suffix else ()):
        assert rf(fake, 32, fake, 1, S, None) == MTD_EINVAL
        assert mx(fake, fake, fake, fake, 1, S, None) == MTD_EINVAL
        assert ir(fake, fake, 32, fake, 32, fake, 32, 1, S, None) == MTD_EINVAL
    S = 128
    assert rf(fake, 32, fake, 0, S, None) == MTD_EINVAL
    assert rf(None, 32, fake, 1, S, None) == MTD_EINVAL
    assert mx(fake, None, fake, fake, 1, S, None) == MTD_EINVAL
    assert ir(fake, None, 32, None, 0, None, 0, 1, S, None) == MTD_EINVAL
    # pixel strides
    assert rf(fake, 28, fake, 1, S, None) == MTD_EINVAL
    assert ir(fake, fake, 28, None, 0, None, 0, 1, S, None) == MTD_EINVAL
    assert ir(fake, fake, 32, fake, 28, None, 0, 1, S, None) == MTD_EINVAL
    assert ir(fake, fake, 32, None, 0, fake, 28, 1, S, None) == MTD_EINVAL
    assert rf(fake, 34, fake, 1, S, None) == MTD_EALIGN
    assert ir(fake, fake, 34, None, 0, None, 0, 1, S, None) == MTD_EALIGN
    assert ir(fake, fake, 32, fake, 34, None, 0, 1, S, None) == MTD_EALIGN
    assert ir(fake, fake, 32, None, 0, fake, 34, 1, S, None) == MTD_EALIGN
    # bases 8 bytes off a 16-byte boundary
    assert rf(off8, 32, fake, 1, S, None) == MTD_EALIGN
    assert rf(fake, 32, off8, 1, S, None) == MTD_EALIGN
    assert mx(off8, fake, fake, fake, 1, S, None) == MTD_EALIGN
    assert mx(fake, fake, fake, off8, 1, S, None) == MTD_EALIGN
    assert ir(off8, fake, 32, None, 0, None, 0, 1, S, None) == MTD_EALIGN
    assert ir(fake, off8, 32, None, 0, None, 0, 1, S, None) == MTD_EALIGN
    assert ir(fake, fake, 32, off8, 32, None, 0, 1, S, None) == MTD_EALIGN
    assert ir(fake, fake, 32, None, 0, off8, 32, 1, S, None) == MTD_EALIGN
