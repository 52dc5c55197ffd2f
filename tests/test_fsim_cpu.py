"""FSIM without a GPU: the float64 restatement of tests/_fsim_ref.py against what the reference's own
module/piq/fsim.py computed (tests/golden/fsim_piq.npz, written by tools/pin_fsim.py), the conditions the fixture's inputs were
chosen to meet, the pooling rule, the host filter table and its constants, the test loop's option check, and the argument
refusals of the entry points that need no device (through the built library's ABI, with addresses of host memory)."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import _fsim_ref as R

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
    """The same operations in float64; the FFT and the order of the sums may differ: 1e-11 relative on every score, sum and
    threshold (where the fixture was written the two agreed bit for bit: the same FFT library under both)."""
    B, H, W, opts = R.CASES[index]
    x, y, pred = R.case_inputs(index)
    assert tuple(x.shape) == (B, 1, H, W) and x.dtype == torch.float32
    assert R.crc(x, y, pred) == int(golden[f"crc_{index}"]), "the seeded inputs are not the ones the fixture was written from"
    names = R.part_names(opts["orientations"])
    for k, src in enumerate((x, y, pred)):
        score, parts = R.fsim(src.double(), y.double(), **opts)
        assert tuple(parts.shape) == (B, len(names))
        e = _rel(score.numpy(), golden[f"score64_{index}"][k])
        assert e <= 1e-11, ("score", k, e)
        for j, name in enumerate(names):
            e = _rel(parts[:, j].numpy(), golden[f"parts64_{index}"][k][:, j])
            assert e <= 1e-11, (name, k, e)


def test_fixture_conditions(golden):
    """Conditions on the chosen inputs, not tolerances: den > 1 on every row (eps cannot matter), every threshold positive, the
    target against itself exactly 1.0, both precisions of the reference for every case, the cases of _fsim_ref, the recorded
    float32 -> float64 distances those of the stored values."""
    meta = json.loads(str(golden["meta"]))
    assert [(B, H, W, opts) for B, H, W, opts in meta["cases"]] == [tuple(cs) for cs in R.CASES]
    spread = {"score": 0.0, "sums": 0.0, "T": 0.0}
    for index, (B, H, W, opts) in enumerate(R.CASES):
        n = 4 + opts["orientations"]
        for tag, dt in (("32", np.float32), ("64", np.float64)):
            assert golden[f"score{tag}_{index}"].shape == (3, B) and golden[f"score{tag}_{index}"].dtype == dt
            assert golden[f"parts{tag}_{index}"].shape == (3, B, n) and golden[f"parts{tag}_{index}"].dtype == dt
            assert (golden[f"parts{tag}_{index}"][..., 1] > 1).all(), index
            assert (golden[f"parts{tag}_{index}"][..., 4:] > 0).all(), index
            assert (golden[f"score{tag}_{index}"][1] == 1.0).all(), index
        p32, p64 = golden[f"parts32_{index}"], golden[f"parts64_{index}"]
        spread["score"] = max(spread["score"], _rel(golden[f"score32_{index}"], golden[f"score64_{index}"]))
        spread["sums"] = max(spread["sums"], _rel(p32[..., :4], p64[..., :4]))
        spread["T"] = max(spread["T"], _rel(p32[..., 4:], p64[..., 4:]))
        s = golden[f"score64_{index}"]
        assert (s[0] < s[2]).all() and (s[2] < 1.0).all() and (s[0] > 0.5).all(), index          # input, pred
    assert spread == meta["spread"]
    assert os.path.getsize(R.GOLDEN) < 64 * 1024


POOLING = [((64, 64), (1, 64, 64)), ((256, 256), (1, 256, 256)), ((383, 400), (1, 383, 400)), ((384, 384), (2, 192, 192)),
           ((512, 512), (2, 256, 256)), ((640, 640), (2, 320, 320)), ((641, 700), (3, 213, 233)), ((1024, 1024), (4, 256, 256)),
           ((1536, 768), (3, 512, 256)), ((512, 256), (1, 512, 256)), ((520, 512), (2, 260, 256)), ((16, 2048), (1, 16, 2048))]


@pytest.mark.parametrize("size, want", POOLING)
def test_pooling_rule(size, want):
    """H, W -> ks, h, w: Python's round (to even: 384 / 256 = 1.5 -> 2, 640 / 256 = 2.5 -> 2), stride ks, floor -- and the sizes
    the restatement's avg_pool2d really gives."""
    from mtd_gan_amd import metrics as M
    assert M.fsim_pooled_size(*size) == want and R.pooled_size(*size) == want
    if size[0] * size[1] <= 1 << 20:
        pooled = torch.nn.functional.avg_pool2d(torch.zeros(1, 1, *size), want[0])
        assert tuple(pooled.shape[2:]) == want[1:]


def test_a_size_that_does_not_pool_to_powers_of_two_is_refused_by_name():
    from mtd_gan_amd import metrics as M
    for size, pooled in (((520, 512), "260x256"), ((384, 384), "192x192"), ((32, 8), "32x8"), ((2048, 16), "2048x16"), ((1024, 1024), "256x256")):
        x = torch.zeros(1, 1, *size)
        if pooled == "256x256":
            with pytest.raises(RuntimeError, match="CUDA"):           # (a size that is fine gets as far as the device check)
                M.fsim_each(x, x, x)
            continue
        with pytest.raises(ValueError, match=pooled):
            M.fsim_each(x, x, x)


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_host_filter_table_has_the_bytes_of_the_references(golden, index):
    """metrics.fsim_filter_table (broadcast factors for all scales and orientations at once) and the restatement's table (filter
    by filter) are written independently; both must give the bytes of the table the reference's own _construct_filters built
    when the fixture was written (its CRC-32).  The three constants against the restatement's, which sums pair by pair."""
    from mtd_gan_amd import metrics as M
    B, H, W, opts = R.CASES[index]
    ks, h, w = R.pooled_size(H, W)
    o = {k: v for k, v in opts.items() if k != "k"}
    S, O = o["scales"], o["orientations"]
    table = M.fsim_filter_table(h, w, **o)
    assert table.dtype == torch.float32 and tuple(table.shape) == (O * S, h, w) and table.is_contiguous()
    assert R.crc(table) == int(golden[f"filters_crc_{index}"]), "the host table is not the reference's"
    assert R.crc(R.filter_table(h, w, **o)) == int(golden[f"filters_crc_{index}"]), "the restatement's table is not the reference's"
    assert (table[:, 0, 0] == 0).all() and float(table.max()) <= 1.0 and float(table.min()) >= 0.0
    consts = M.fsim_constants(table, S, O)
    assert consts.dtype == torch.float64 and tuple(consts.shape) == (3, O)
    want = R.noise_constants(table.double().view(O, S, h, w))
    for j in range(3):
        assert _rel(consts[j], want[j]) <= 1e-12, j


class _NoLoader:
    def __iter__(self):
        raise AssertionError("the loader must not be read before the option is checked")


BAD_OPTIONS = ["yes", 3, ("scales", 4), dict(c=30.0), dict(scales=4, reduction="mean"), dict(scales=0), dict(scales=5), dict(scales=4.0),
               dict(scales=True), dict(orientations=0), dict(orientations=9), dict(orientations="4"), dict(min_length=0), dict(mult=-2),
               dict(sigma_f=0.0), dict(sigma_f=1.0), dict(delta_theta=0), dict(k=None), dict(k=float("nan")), dict(k="2"), dict(chromatic=False)]


@pytest.mark.parametrize("bad", BAD_OPTIONS)
def test_engine_refuses_a_bad_test_fsim_before_anything_runs(bad):
    from mtd_gan_amd import engine
    model = types.SimpleNamespace(test_fsim=bad)      # no Generator: anything past the option check would fail otherwise
    with pytest.raises(ValueError, match="test_fsim.*scales.*orientations.*delta_theta"):
        engine.test_MTD_GAN_Ours(model, None, _NoLoader(), torch.device("cpu"), None)


def test_engine_option_values():
    from mtd_gan_amd import engine
    opt = lambda **kw: engine._fsim_option(types.SimpleNamespace(**kw))          # noqa: E731
    assert opt() is None and opt(test_fsim=None) is None and opt(test_fsim=False) is None
    assert opt(test_fsim=True) == {}
    assert opt(test_fsim=dict(scales=3, k=1.5)) == dict(scales=3, k=1.5)
    assert opt(test_fsim=dict(R.OTHER)) == R.OTHER and opt(test_fsim=dict(R.DEFAULTS)) == R.DEFAULTS
    assert opt(test_fsim=dict(k=-1, sigma_f=1.5)) == dict(k=-1, sigma_f=1.5)
    for bad in BAD_OPTIONS:
        with pytest.raises(ValueError):
            opt(test_fsim=bad)
    assert engine._haarpsi_option(types.SimpleNamespace(test_fsim=True)) is None          # the options do not see each other
    assert engine._fsim_option(types.SimpleNamespace(test_haarpsi=True, test_iqa=True)) is None


def test_header_declares_and_lib_binds_the_entry_points(built_lib):
    from mtd_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    for n in ("mtd_fsim_ws_bytes", "mtd_fsim_each", "mtd_fsim_median"):
        assert re.search(r"^(size_t|int) %s\(" % n, header, re.M), n
        assert n in _lib.EXPORTS and len(getattr(built_lib, n).argtypes) > 0, n
    assert len(built_lib.mtd_fsim_each.argtypes) == 16 and len(built_lib.mtd_fsim_ws_bytes.argtypes) == 6
    for name, value in (("MTD_FSIM_SUMS", 4), ("MTD_FSIM_MIN_SIDE", 16), ("MTD_FSIM_MAX_SIDE", 512)):
        assert re.search(r"^#define %s %d$" % (name, value), header, re.M), name


def _ws_model(na, B, h, w, S, O):
    """The chunk rule of DESIGN 3.17 restated: (images per chunk, orientations held at a time, bytes)."""
    hw, sets, tiles = h * w, na + 1, (h // 16) * (w // 16)
    for Og in range(O, 0, -1):
        per_image = sets * (hw * (8 + 8 * Og * S + 12 * O) + 8 * O) + na * tiles * 32
        if per_image <= 64 << 20:
            break
    Bc = max(1, min(B, (64 << 20) // per_image, 8192))
    return Bc, Og, Bc * per_image


def test_workspace_follows_the_chunk_rule_and_stays_bounded(built_lib):
    q = built_lib.mtd_fsim_ws_bytes
    for args in ((3, 1, 256, 256, 4, 4), (3, 8, 256, 256, 4, 4), (3, 1000, 256, 256, 4, 4), (1, 64, 256, 256, 4, 4), (3, 2, 16, 16, 4, 4),
                 (3, 64, 64, 64, 4, 4), (2, 5, 64, 32, 3, 6), (3, 1, 512, 512, 4, 8), (3, 100000, 16, 16, 1, 1), (3, 4, 256, 256, 4, 8),
                 (3, 1, 512, 256, 4, 4), (3, 1, 512, 512, 1, 1)):
        assert q(*args) == _ws_model(*args)[2], args
    for B in (1, 8, 64, 1 << 20):                  # 256 x 256 pooled maps: within 64 MiB whatever the batch and the options are
        for na in (1, 2, 3):
            for S in (1, 2, 3, 4):
                for O in (1, 2, 3, 4, 5, 6, 7, 8):
                    assert 0 < q(na, B, 256, 256, S, O) <= 64 << 20, (na, B, S, O)
    assert q(3, 8, 256, 256, 4, 4) == q(3, 1, 256, 256, 4, 4)      # (one image of every set per chunk there)
    assert _ws_model(3, 64, 64, 64, 4, 4)[:2] == (22, 4)           # 64 x 64 patches: 22 images of every set per chunk
    assert _ws_model(3, 1, 256, 256, 4, 4)[:2] == (1, 4)           # the defaults at 256 x 256: every orientation at once
    assert _ws_model(3, 1, 256, 256, 4, 8)[:2] == (1, 4)           # eight orientations there: two groups of four
    assert _ws_model(3, 1, 512, 512, 4, 4)[:2] == (1, 1)           # a 512 x 512 pooled map: one orientation at a time (and 88 MiB)


def test_refusals_return_before_any_launch(built_lib):
    """The refused calls touch neither their pointers nor the device."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    f, q, m = built_lib.mtd_fsim_each, built_lib.mtd_fsim_ws_bytes, built_lib.mtd_fsim_median

    def each(srcs=ptrs, na=3, target=p, B=1, H=64, W=64, ks=1, S=4, O=4, k=2.0, filters=p, consts=p, out=p, parts=p, ws=p):
        return f(srcs, na, target, B, H, W, ks, S, O, k, filters, consts, out, parts, ws, None)
    # (na, B, H, W, ks, S, O): na outside 1..3, B < 1, pooled sides that are no power of two or outside 16..512, S, O out of range
    for na, B, H, W, ks, S, O in ((0, 1, 64, 64, 1, 4, 4), (4, 1, 64, 64, 1, 4, 4), (3, 0, 64, 64, 1, 4, 4), (3, -1, 64, 64, 1, 4, 4),
                                  (3, 1, 520, 512, 2, 4, 4), (3, 1, 48, 64, 1, 4, 4), (3, 1, 64, 48, 1, 4, 4), (3, 1, 8, 64, 1, 4, 4),
                                  (3, 1, 64, 8, 1, 4, 4), (3, 1, 1024, 64, 1, 4, 4), (3, 1, 64, 1024, 1, 4, 4), (3, 1, 64, 64, 8, 4, 4),
                                  (3, 1, 64, 64, 1, 0, 4), (3, 1, 64, 64, 1, 5, 4), (3, 1, 64, 64, 1, 4, 0), (3, 1, 64, 64, 1, 4, 9),
                                  (3, 1, 64, 64, 0, 4, 4), (3, 1, 64, 64, -1, 4, 4), (1, 1, 65536, 32768, 128, 4, 4)):
        if ks > 0:
            assert q(na, B, H // ks, W // ks, S, O) == 0 or ks > 64, (na, B, H, W, ks, S, O)
        assert each(na=na, B=B, H=H, W=W, ks=ks, S=S, O=O) == -1, (na, B, H, W, ks, S, O)
    for null in ("srcs", "target", "filters", "consts", "out", "ws"):
        assert each(**{null: None}) == -1, null
    assert each(srcs=(ctypes.c_void_p * 3)(p, None, p)) == -1
    assert each(srcs=(ctypes.c_void_p * 3)(p, p, None), parts=None) == -1
    assert each(k=float("nan")) == -1
    for args in ((None, 16, 1, p), (p, 16, 1, None), (p, 0, 1, p), (p, 16, 0, p), (p, 16, 65536, p)):
        assert m(*args, None) == -1, args


def test_python_surface_refusals_without_a_device():
    from mtd_gan_amd import metrics as M
    x = torch.zeros(2, 1, 64, 64)
    for fn in (M.fsim_each, M.fsim_per_slice, M.compute_FSIM):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(x, x, x)
        with pytest.raises(AssertionError):
            fn(x[:1], x, x)
        with pytest.raises(AssertionError):
            fn(x[:, :, :32], x, x)
        with pytest.raises(AssertionError):
            fn(x[0], x[0], x[0])
        with pytest.raises(ValueError, match="64x48"):
            fn(x[:, :, :, :48], x[:, :, :, :48], x[:, :, :, :48])
        for kw in (dict(scales=5), dict(orientations=0), dict(sigma_f=1.0), dict(min_length=0), dict(k=None)):
            with pytest.raises(ValueError, match="fsim"):
                fn(x, x, x, **kw)
    with pytest.raises(NotImplementedError):
        M.compute_FSIM(x, x, x, data_range=255.0)
    assert (M.FSIM_MIN_SIDE, M.FSIM_MAX_SIDE) == (R.MIN_SIDE, R.MAX_SIDE) == (16, 512)
    assert M.FSIM_OPTIONS == tuple(R.DEFAULTS) and M.HAARPSI_MIN_SIDE == 16          # the neighbours stay as they are
