"""CPU side of the per-stage tests of the training spectral kernels (csrc/resfft.hip, csrc/resfft4.hip): the sign-mask encoder of
test_spectral_train_stages_gpu.py is a bijection that agrees with the probes of test_kernels_gpu.py, its batch lists reach the
branches of the slab reduces that its docstrings name, its workspace formula is the library's, and the entry points check their
arguments before anything is launched."""
import ctypes

import numpy as np
import pytest

import test_spectral_train_stages_gpu as stages

MTD_EINVAL, MTD_EALIGN = -1, -2


# ------------------------------------------------------------------------------------------------------- the sign mask
def test_mask_positions_are_a_bijection():
    """(k2, kh, o) -> (word, bit) hits each of the 128 x 64 bits of a unit once, and encode / decode are inverses."""
    word, bit = stages.mask_positions()
    assert word.shape == bit.shape == (2, 64, 64)
    assert word.min() == 0 and word.max() == 127 and bit.min() == 0 and bit.max() == 63
    assert len(np.unique(word * 64 + bit)) == 128 * 64
    # the first column of a pair owns words 0..63, the second 64..127
    assert word[0].max() == 63 and word[1].min() == 64
    rng = np.random.default_rng(5)
    pos = rng.integers(0, 2, size=(2, 33, 64, 64)).astype(bool)
    by = stages.mask_encode(pos, absent=0xA5).numpy()
    assert by.shape == (2 * 17 * 128 * 8,)
    assert np.array_equal(stages.mask_decode(by, 2).numpy(), pos)
    words = by.view("<u8").reshape(2, 17, 128)
    assert (words[:, 16, 64:] == 0xA5A5A5A5A5A5A5A5).all()
    # one set element sets one bit, at the restated position
    one = np.zeros((1, 33, 64, 64), dtype=bool)
    one[0, 7, 45, 38] = True
    w = stages.mask_encode(one).numpy().view("<u8").reshape(17, 128)
    assert np.count_nonzero(w) == 1 and w[3, word[1, 45, 38]] == np.uint64(1) << np.uint64(bit[1, 45, 38])


def test_mask_positions_agree_with_the_probes_of_the_path_test():
    """The five elements that test_kernels_gpu.py::test_spectral_path_kernels looks up, by its own index arithmetic
    ([b][pair][col][kh half][out half][register], bit)."""
    word, bit = stages.mask_positions()
    for (b_, kw_, kh_, o_) in [(0, 0, 0, 0), (1, 5, 37, 40), (2, 32, 63, 63), (0, 17, 12, 31), (2, 31, 45, 2)]:
        r32 = kh_ & 31
        e_ = (r32 & 3) + 4 * (r32 >> 3)
        probe_word = np.ravel_multi_index((kw_ % 2, kh_ >> 5, o_ >> 5, e_), (2, 2, 2, 16))
        probe_bit = (o_ & 31) + 32 * ((r32 >> 2) & 1)
        assert (word[kw_ % 2, kh_, o_], bit[kw_ % 2, kh_, o_]) == (probe_word, probe_bit), (b_, kw_, kh_, o_)
        pos = np.zeros((3, 33, 64, 64), dtype=bool)
        pos[b_, kw_, kh_, o_] = True
        words = stages.mask_encode(pos).numpy().view("<u8").reshape(3, 17, 2, 2, 2, 16)
        assert (int(words[b_, kw_ // 2, kw_ % 2, kh_ >> 5, o_ >> 5, e_]) >> probe_bit) & 1 == 1


# ------------------------------------------------------------------------------------------------------ the slab counts
def test_reduce_batches_reach_every_branch_of_the_fused_sum():
    """block_slab_sum<8>: 64 runs of per = ceil(17 B / 64) slabs, each as 8-load batches, then one 4-load batch, then single loads."""
    assert stages.REDUCE_BATCHES == (1, 4, 16, 29, 45, 240)
    full = {}
    for B in stages.REDUCE_BATCHES:
        per, runs = stages.run_batches(17 * B)
        assert per == -(-17 * B // 64) and len(runs) == 64
        assert sum(8 * a + 4 * b + c for a, b, c in runs) == 17 * B            # every slab is in one run
        assert all(b <= 1 and c <= 3 for _, b, c in runs)
        full[B] = (per, runs[0], sum(1 for r in runs if r == (0, 0, 0)))
    # (per, the split of a full run, empty runs)
    assert full[1] == (1, (0, 0, 1), 47)                 # 17 slabs: one each, 47 runs empty
    assert full[4] == (2, (0, 0, 2), 30)                 # 68 slabs: two per run
    assert full[16] == (5, (0, 1, 1), 9)                 # a 4-load batch plus a single load
    assert full[29] == (8, (1, 0, 0), 2)                 # exactly one 8-load batch
    assert full[45] == (12, (1, 1, 0), 0)                # an 8-load plus a 4-load batch
    assert full[240] == (64, (8, 0, 0), 0)               # eight 8-load batches in every run
    assert stages.run_batches(17 * 240)[1][63] == (6, 0, 0)                     # (the last run is ragged: 48 slabs)
    assert 17 * 240 <= stages.FUSED_MAX < 17 * 241                               # 240 is the largest batch of the fused path


def test_fallback_batches_reach_every_level_shape():
    assert stages.FALLBACK_BATCHES == (1, 3, 61, 241)
    assert stages.fallback_levels(17 * 1) == [17]                                # mix_finish_kernel alone
    assert stages.fallback_levels(17 * 3) == [51, 2] and 51 - stages.MIX_GS == 19           # one level, a ragged second group
    assert stages.fallback_levels(17 * 61) == [1037, 33, 2] and 1037 % stages.MIX_GS and 33 % stages.MIX_GS    # two levels, ragged
    assert stages.fallback_levels(17 * 241) == [4097, 129, 5]
    assert all(17 * B <= stages.FUSED_MAX for B in stages.FALLBACK_BATCHES[:3])  # (these need the misaligned dw2)


# ------------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__  # noqa: F401  (puts the repository root on sys.path)
    from mtd_gan_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.mtd_rfft_rows.argtypes = [vp, ci, vp, ci, ci, vp]
    L.mtd_irfft_rows.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, ci, ci, vp]
    for name in ("mtd_spec_mix_fwd", "mtd_spec_mix_fwd4", "mtd_spec_mix_bwd", "mtd_spec_mix_bwd4"):
        getattr(L, name).argtypes = [vp, vp, vp, vp, vp, vp, ci, vp]
    L.mtd_spec_mix_wgrad_reduce.argtypes = [vp, ci, vp, vp, ci, vp]
    L.mtd_spec_mix_wgrad_reduce_multi.argtypes = [vp, vp, ci, vp]
    for name in ("mtd_spec_mix_bwd_ws_bytes", "mtd_spec_mix_zmask_bytes"):
        getattr(L, name).argtypes = [ci]
        getattr(L, name).restype = ctypes.c_size_t
    return L


def test_workspace_size_is_the_sum_of_the_levels(lib):
    for B in stages.FALLBACK_BATCHES + stages.REDUCE_BATCHES:
        assert lib.mtd_spec_mix_bwd_ws_bytes(B) == 4 * stages.ws_floats(B), B
        assert lib.mtd_spec_mix_zmask_bytes(B) == B * stages.UNITS * stages.WORDS * 8
    assert stages.ws_floats(3) == (51 + 2) * stages.SLAB and stages.ws_floats(241) == (4097 + 129 + 5) * stages.SLAB
    assert lib.mtd_spec_mix_bwd_ws_bytes(0) == 0 and lib.mtd_spec_mix_zmask_bytes(-1) == 0


def test_entry_points_refuse_without_a_device(lib):
    """Null pointers, batches <= 0, pixel strides under 32 channels and bases that 16-byte accesses cannot take are refused before
    any launch."""
    from mtd_gan_amd._lib import MixReduceDesc
    fake, off8 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)
    # rows forward
    assert lib.mtd_rfft_rows(None, 32, fake, 1, 0, None) == MTD_EINVAL
    assert lib.mtd_rfft_rows(fake, 32, None, 1, 0, None) == MTD_EINVAL
    assert lib.mtd_rfft_rows(fake, 32, fake, 0, 0, None) == MTD_EINVAL
    assert lib.mtd_rfft_rows(fake, 31, fake, 1, 0, None) == MTD_EINVAL
    # rows back
    assert lib.mtd_irfft_rows(None, fake, 32, None, 0, None, 0, None, 0, 1, None) == MTD_EINVAL
    assert lib.mtd_irfft_rows(fake, None, 32, None, 0, None, 0, None, 0, 1, None) == MTD_EINVAL
    assert lib.mtd_irfft_rows(fake, fake, 32, None, 0, None, 0, None, 0, 0, None) == MTD_EINVAL
    assert lib.mtd_irfft_rows(fake, fake, 31, None, 0, None, 0, None, 0, 1, None) == MTD_EINVAL
    assert lib.mtd_irfft_rows(fake, fake, 32, fake, 31, None, 0, None, 0, 1, None) == MTD_EINVAL
    assert lib.mtd_irfft_rows(fake, fake, 32, None, 0, fake, 31, None, 0, 1, None) == MTD_EINVAL
    assert lib.mtd_irfft_rows(fake, fake, 32, None, 0, None, 0, fake, 31, 1, None) == MTD_EINVAL
    # forward mix, both forms: R, w2t, b2, T are required (S_save and Z may be null), B > 0
    for f in (lib.mtd_spec_mix_fwd, lib.mtd_spec_mix_fwd4):
        for k in range(4):
            args = [fake] * 6
            args[k] = None
            assert f(*args, 1, None) == MTD_EINVAL, k
        assert f(fake, fake, fake, fake, None, None, 0, None) == MTD_EINVAL
    assert lib.mtd_spec_mix_fwd4(off8, fake, fake, fake, None, None, 1, None) == MTD_EALIGN
    # backward mix, both forms: every pointer is required
    for f in (lib.mtd_spec_mix_bwd, lib.mtd_spec_mix_bwd4):
        for k in range(6):
            args = [fake] * 6
            args[k] = None
            assert f(*args, 1, None) == MTD_EINVAL, k
        assert f(fake, fake, fake, fake, fake, fake, 0, None) == MTD_EINVAL
    assert lib.mtd_spec_mix_bwd4(off8, fake, fake, fake, fake, fake, 1, None) == MTD_EALIGN
    assert lib.mtd_spec_mix_bwd4(fake, fake, off8, fake, fake, fake, 1, None) == MTD_EALIGN
    # reduce
    assert lib.mtd_spec_mix_wgrad_reduce(None, 1, fake, fake, 0, None) == MTD_EINVAL
    assert lib.mtd_spec_mix_wgrad_reduce(fake, 1, None, fake, 0, None) == MTD_EINVAL
    assert lib.mtd_spec_mix_wgrad_reduce(fake, 1, fake, None, 0, None) == MTD_EINVAL
    assert lib.mtd_spec_mix_wgrad_reduce(fake, 0, fake, fake, 0, None) == MTD_EINVAL

    # reduce of a table: the host copy of the table is what is checked; the fault sits in the second of two descriptors
    def desc(ws=4096, dw2=4096, db2=4096, nslab=17):
        d = MixReduceDesc()
        d.ws, d.dw2, d.db2, d.nslab, d.accumulate = ws, dw2, db2, nslab, 0
        return d

    def table(**fault):
        return (MixReduceDesc * 2)(desc(nslab=4096), desc(**fault))

    multi = lib.mtd_spec_mix_wgrad_reduce_multi
    good = table()
    assert multi(None, good, 2, None) == MTD_EINVAL
    assert multi(fake, None, 2, None) == MTD_EINVAL
    assert multi(fake, good, 0, None) == MTD_EINVAL
    assert multi(fake, good, -1, None) == MTD_EINVAL
    assert multi(fake, table(nslab=4097), 2, None) == MTD_EINVAL
    assert multi(fake, table(nslab=0), 2, None) == MTD_EINVAL
    assert multi(fake, table(ws=None), 2, None) == MTD_EINVAL
    assert multi(fake, table(dw2=None), 2, None) == MTD_EINVAL
    assert multi(fake, table(db2=None), 2, None) == MTD_EINVAL
    assert multi(fake, table(ws=4096 + 8), 2, None) == MTD_EALIGN
    assert multi(fake, table(dw2=4096 + 4), 2, None) == MTD_EALIGN
