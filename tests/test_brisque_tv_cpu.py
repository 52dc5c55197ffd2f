"""BRISQUE and total variation without a GPU: the float64 restatement of tests/_brisque_ref.py against what the
reference's own module/piq/brisque.py and tv.py computed (tests/golden/brisque_tv_piq.npz, written by tools/pin_brisque_tv.py),
the host tables against the reference's own (the CRC-32 of its bytes where they are portable), the forms brisque_weights takes, the option checks, the test loop's two
table entries, and the argument refusals of the entry points that need no device (through the built library's ABI, with
addresses of host memory)."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import _brisque_ref as R

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
    zero = want == 0
    assert (got[zero] == 0).all(), (got, want)
    return float(np.max(np.abs(got - want)[~zero] / np.abs(want[~zero]))) if (~zero).any() else 0.0


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_float64_restatement_agrees_with_the_reference(golden, index):
    """The same operations in float64; only the order of a few sums differs (the regression's matrix product, the filter): the
    table positions are equal, the features and scores within 1e-10 relative, the total variation within 1e-12."""
    B, H, W, opts, n_sv = R.CASES[index]
    sets = R.case_inputs(index)
    coef, sv = R.case_svm(index)
    assert all(tuple(t.shape) == (B, 1, H, W) and t.dtype == torch.float32 and 0 <= float(t.min()) and float(t.max()) <= 1 for t in sets)
    assert R.crc(*sets) == int(golden[f"crc_{index}"]), "the seeded inputs are not the ones the fixture was written from"
    assert R.crc(coef, sv) == int(golden[f"svm_crc_{index}"]) and tuple(sv.shape) == (n_sv, 36)
    assert float(sv.min()) >= -1 and float(sv.max()) <= 1 and (n_sv == 1 or (float(coef.min()) < 0 < float(coef.max())))
    for k, x in enumerate(sets):
        score, features, where, values = R.brisque(x.double(), coef, sv, **opts)
        assert np.array_equal(where.numpy(), golden[f"where64_{index}"][k]), (k, where, golden[f"where64_{index}"][k])
        assert _rel(values.numpy(), golden[f"values64_{index}"][k]) <= 1e-10
        assert _rel(features.numpy(), golden[f"features64_{index}"][k]) <= 1e-10
        assert _rel(score.numpy(), golden[f"score64_{index}"][k]) <= 1e-10
        for j, norm in enumerate(R.NORMS):
            assert _rel(R.total_variation(x.double(), norm).numpy(), golden[f"tv64_{index}"][j, k]) <= 1e-12, (norm, k)


def test_fixture_conditions(golden):
    meta = json.loads(str(golden["meta"]))
    assert [tuple(c) for c in meta["cases"]] == [tuple(c) for c in json.loads(json.dumps(R.CASES))]
    assert set(meta["spread"]) == {"score", "sigma", "eta", "tv"} and all(0 < v < 1e-3 for v in meta["spread"].values())
    assert meta["margin"] >= 1e-9
    assert sorted(c[4] for c in R.CASES) == [1, 1, 64, 64, 774, 774]
    for index, (B, H, W, opts, n_sv) in enumerate(R.CASES):
        for tag in ("32", "64"):
            assert golden[f"score{tag}_{index}"].shape == (3, B) and np.isfinite(golden[f"score{tag}_{index}"]).all()
            assert golden[f"features{tag}_{index}"].shape == (3, B, 36) and np.isfinite(golden[f"features{tag}_{index}"]).all()
            assert golden[f"where{tag}_{index}"].shape == (3, B, 10) and golden[f"tv{tag}_{index}"].shape == (3, 3, B)
        # the alpha features are the grid's values at the stored positions
        gamma = R.shape_tables(torch.zeros(1, dtype=torch.float64))[0].numpy()
        assert np.array_equal(golden[f"features64_{index}"][..., list(R.ALPHA_AT)], gamma[golden[f"where64_{index}"]])
    assert os.path.getsize(R.GOLDEN) < 256 << 10


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_host_gaussian_table_has_the_bytes_of_the_references(golden, index):
    from mtd_gan_amd import metrics as M
    opts = R.CASES[index][3]
    table = M.brisque_gaussian_table(**opts)
    k = opts.get("kernel_size", 7)
    assert table.dtype == torch.float32 and tuple(table.shape) == (k, k) and table.is_contiguous()
    assert R.crc(table) == int(golden[f"gaussian_crc_{index}"])
    assert abs(float(table.double().sum()) - 1) < 1e-6 and torch.equal(table, table.t())
    assert M.brisque_gaussian_table(**opts) is table                   # cached


def test_host_shape_tables_are_the_references(golden):
    """The grid has the reference's bytes.  The two r_tables are float64 lgamma and exp of it, which torch evaluates with another
    vector routine per CPU instruction set: on the machine that pinned the fixture the bytes are equal (the CRC-32s), on another
    the last bits differ.  So every one of the 9801 entries is held to the reference's within 1e-13 relative, and the CRC-32s
    are printed.  Where the bound comes from: a table entry is exp of a sum of four lgamma values of magnitude up to 25.6 (at
    gamma = 0.2: lgamma(15) and 2 lgamma(10)), whose unit in the last place is 3.6e-15; routines good to one such unit, three
    roundings of the additions and exp's own leave each machine within about 1.3e-14 of the exact entry (an absolute error of
    the exponent is a relative error of the entry), two machines within 2.6e-14 of each other; 1e-13 is four times that and
    four orders of magnitude inside the 1e-9 margin the pin tool asserts around every look-up."""
    from mtd_gan_amd import metrics as M
    tables = M.brisque_ggd_tables()
    assert tables.dtype == torch.float64 and tuple(tables.shape) == (3, 9801) and tables.is_contiguous()
    assert R.crc(tables[0]) == int(golden["gamma_crc"])
    assert torch.equal(tables[0], tables[0].float().double())          # the grid is float32's, widened
    for row, name in ((1, "ggd"), (2, "aggd")):
        want = golden[f"{name}_table"]
        assert want.dtype == np.float64 and want.shape == (9801,) and R.crc(torch.from_numpy(want)) == int(golden[f"{name}_crc"])
        e = _rel(tables[row].numpy(), want)
        print(f"{name} r_table: CRC-32 {'equal' if R.crc(tables[row]) == int(golden[name + '_crc']) else 'differs'}, largest relative distance {e:.2e}")
        assert e <= 1e-13, (name, e)
        assert (np.diff(tables[row].numpy()) * (-1 if row == 1 else 1) > 0).all()      # strictly monotone: the look-up has one answer
    ours = R.shape_tables(torch.zeros(1, dtype=torch.float64))
    assert all(torch.equal(a, b) for a, b in zip(ours, tables))        # the restatement's tables are the same
    assert M.brisque_ggd_tables() is tables


def test_brisque_weights_forms(tmp_path):
    from mtd_gan_amd import metrics as M
    coef, sv = R.seeded_svm(5, 1)
    table = M.brisque_weights((coef, sv))
    assert table.dtype == torch.float64 and tuple(table.shape) == (5, 37) and table.is_contiguous()
    assert torch.equal(table[:, 0], coef.flatten()) and torch.equal(table[:, 1:], sv)
    assert torch.equal(M.brisque_weights([coef.flatten(), sv]), table)                  # (n_sv,) and a list
    assert torch.equal(M.brisque_weights((coef.float(), sv.float())), torch.cat([coef.float().double(), sv.float().double()], dim=1))
    assert torch.equal(M.brisque_weights(table), table)                                 # a table it returned
    path = tmp_path / "brisque_svm_weights.pt"
    torch.save((coef, sv), path)                                                        # the layout of piq's file
    assert torch.equal(M.brisque_weights(str(path)), table) and torch.equal(M.brisque_weights(path), table)
    nan = sv.clone()
    nan[2, 3] = float("nan")
    inf = coef.clone()
    inf[0] = float("inf")
    for bad in ((coef, sv[:, :35]), (coef[:4], sv), (coef.reshape(1, 5), sv), (coef, sv.reshape(5, 6, 6)), (coef, sv, sv), (coef,), sv, None, 3.0,
                dict(sv_coef=coef, sv=sv), (coef.long(), sv), (coef, nan), (inf, sv), (coef[:0], sv[:0]), table[:, :36], table.float(), (1.0, sv)):
        with pytest.raises(ValueError, match="brisque_weights"):
            M.brisque_weights(bad)
    with pytest.raises(OSError):
        M.brisque_weights(str(tmp_path / "absent.pt"))


def test_option_checks():
    from mtd_gan_amd import metrics as M
    assert M.BRISQUE_OPTIONS == ("kernel_size", "kernel_sigma") and M.TV_OPTIONS == ("norm_type",) and M.TV_NORMS == R.NORMS
    assert (M.BRISQUE_MIN_SIDE, M.BRISQUE_MAX_SIDE, M.BRISQUE_PARTS) == (R.MIN_SIDE, R.MAX_SIDE, R.PARTS) == (16, 1024, 37)
    M.brisque_check_options()
    for k in (3, 5, 7, 9, 11, 13, 15):
        M.brisque_check_options(kernel_size=k, kernel_sigma=0.5)
    M.brisque_check_options(kernel_sigma=3, interpolation="nearest")
    for bad in (dict(kernel_size=1), dict(kernel_size=4), dict(kernel_size=8), dict(kernel_size=17), dict(kernel_size=7.0), dict(kernel_size=True),
                dict(kernel_size="7"), dict(kernel_sigma=0), dict(kernel_sigma=-1.0), dict(kernel_sigma=float("inf")), dict(kernel_sigma=float("nan")),
                dict(kernel_sigma=None), dict(kernel_sigma=True)):
        with pytest.raises(ValueError, match="brisque: kernel_"):
            M.brisque_check_options(**bad)
    for mode in ("bilinear", "bicubic", "area", "nearest-exact", None):
        with pytest.raises(ValueError, match="brisque.*'nearest' only"):
            M.brisque_check_options(interpolation=mode)
    for norm in R.NORMS:
        M.tv_check_options(norm)
    M.tv_check_options()
    for bad in ("L2", "l3", "", None, 2, ("l1",)):
        with pytest.raises(ValueError, match="tv: norm_type"):
            M.tv_check_options(bad)


class _NoLoader:
    def __iter__(self):
        raise AssertionError("the loader was touched before the option was checked")


def _entry(attr):
    from mtd_gan_amd import engine
    e, = (e for e in engine._PER_SLICE if e.attr == attr)
    return lambda **kw: e.parse(types.SimpleNamespace(**kw), e)


def test_engine_entries_sit_last_in_the_table():
    from mtd_gan_amd import engine
    assert [e.attr for e in engine._PER_SLICE] == ["test_iqa", "test_haarpsi", "test_fsim", "test_lpips", "test_dists", "test_vsi", "test_mdsi",
                                                   "test_brisque", "test_tv"]
    bq, tv = engine._PER_SLICE[-2:]
    assert (bq.each, bq.columns) == ("brisque_each", {"brisque": "BRISQUE"}) and (tv.each, tv.columns) == ("tv_each", {"tv": "TV"})
    assert engine._per_slice_options(types.SimpleNamespace()) == []


def test_engine_option_values():
    from mtd_gan_amd import metrics as M
    bq, tv = _entry("test_brisque"), _entry("test_tv")
    pair = R.seeded_svm(3, 2)
    table = M.brisque_weights(pair)
    for off in (None, False, (), {}, ""):
        assert bq(test_brisque=off) is None
    assert bq() is None and tv() is None and tv(test_tv=None) is None and tv(test_tv=False) is None
    got = bq(test_brisque=pair)
    assert set(got) == {"weights"} and torch.equal(got["weights"], table) and got["weights"].dtype == torch.float64
    got = bq(test_brisque=dict(weights=pair, kernel_size=9, kernel_sigma=1.5))
    assert set(got) == {"weights", "kernel_size", "kernel_sigma"} and torch.equal(got["weights"], table) and got["kernel_size"] == 9 and got["kernel_sigma"] == 1.5
    assert set(bq(test_brisque=dict(weights=table))) == {"weights"}
    assert tv(test_tv=True) == {} and tv(test_tv=dict(norm_type="l1")) == dict(norm_type="l1")
    assert bq(test_tv=True, test_mdsi=True) is None and tv(test_brisque=pair) is None          # the options do not see each other


BAD_BRISQUE = [True, dict(weights=True), dict(kernel_size=7), dict(weights=None, kernel_size=7), 3.0, "absent_file.pt",
               (torch.zeros(3, 1), torch.zeros(3, 35)), dict(weights=(torch.zeros(3), torch.zeros(3, 36)), kernel_size=8),
               dict(weights=(torch.zeros(3), torch.zeros(3, 36)), interpolation="nearest"), dict(weights=(torch.zeros(3), torch.zeros(3, 36)), sigma=1.0),
               dict(weights=(torch.zeros(3), torch.zeros(3, 36)), kernel_sigma=0)]
BAD_TV = [dict(norm_type="l3"), dict(norm="l1"), "l1", 1, ("l1",), dict(norm_type="l1", parts=True)]


@pytest.mark.parametrize("bad", BAD_BRISQUE)
def test_engine_refuses_a_bad_test_brisque_before_anything_runs(bad):
    from mtd_gan_amd import engine
    model = types.SimpleNamespace(test_brisque=bad)      # no Generator: anything past the option check would fail otherwise
    with pytest.raises(ValueError, match="test_brisque"):
        engine.test_MTD_GAN_Ours(model, None, _NoLoader(), torch.device("cpu"), None)


def test_engine_true_says_that_no_weights_ship():
    from mtd_gan_amd import engine
    for cfg in (True, dict(weights=True)):
        with pytest.raises(ValueError, match="test_brisque: no weights ship with this package"):
            engine.test_MTD_GAN_Ours(types.SimpleNamespace(test_brisque=cfg), None, _NoLoader(), torch.device("cpu"), None)


@pytest.mark.parametrize("bad", BAD_TV)
def test_engine_refuses_a_bad_test_tv_before_anything_runs(bad):
    from mtd_gan_amd import engine
    model = types.SimpleNamespace(test_tv=bad)
    with pytest.raises(ValueError, match="test_tv.*norm_type"):
        engine.test_MTD_GAN_Ours(model, None, _NoLoader(), torch.device("cpu"), None)


def test_header_declares_and_lib_binds_the_entry_points(built_lib):
    from mtd_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    for n, arity in (("mtd_brisque_ws_bytes", 4), ("mtd_brisque_each", 15), ("mtd_tv_ws_bytes", 4), ("mtd_tv_each", 9)):
        assert re.search(r"^(size_t|int) %s\(" % n, header, re.M), n
        assert n in _lib.EXPORTS and len(getattr(built_lib, n).argtypes) == arity, n
    for name, value in (("MTD_BRISQUE_PARTS", 37), ("MTD_BRISQUE_MIN_SIDE", 16), ("MTD_BRISQUE_MAX_SIDE", 1024), ("MTD_BRISQUE_MAX_KERNEL", 15),
                        ("MTD_TV_MIN_SIDE", 16), ("MTD_TV_MAX_SIDE", 1024), ("MTD_TV_L1", 0), ("MTD_TV_L2", 1), ("MTD_TV_L2_SQUARED", 2)):
        assert re.search(r"^#define %s %d$" % (name, value), header, re.M), name


def _brisque_ws_model(na, B, H, W):
    """The chunk rule of DESIGN 3.21 restated: (images per chunk, bytes)."""
    tiles = -(-H // 16) * -(-W // 16) + -(-(H // 2) // 16) * -(-(W // 2) // 16)
    per_image = na * 8 * (H * W + (H // 2) * (W // 2) + tiles * 26)
    Bc = max(1, min(B, (64 << 20) // per_image, 8192))
    return Bc, Bc * per_image


def test_workspaces_follow_the_chunk_rule_and_stay_bounded(built_lib):
    for args in ((3, 1, 512, 512), (3, 8, 512, 512), (3, 1000, 512, 512), (1, 64, 256, 256), (3, 2, 16, 16), (3, 3, 17, 23), (2, 5, 385, 400),
                 (3, 1, 1024, 1024), (3, 100000, 16, 16), (3, 2, 96, 131)):
        assert built_lib.mtd_brisque_ws_bytes(*args) == _brisque_ws_model(*args)[1], args
        na, B, H, W = args
        assert built_lib.mtd_tv_ws_bytes(*args) == na * B * -(-H // 8) * 32, args
    for B in (1, 8, 64, 1 << 20):
        for na in (1, 2, 3):
            for H, W in ((16, 16), (512, 512), (1024, 1024), (1024, 16)):
                assert 0 < built_lib.mtd_brisque_ws_bytes(na, B, H, W) <= 64 << 20, (na, B, H, W)
    assert _brisque_ws_model(3, 64, 512, 512)[0] == 7                # 512 x 512 slices: seven images of every set per chunk
    assert _brisque_ws_model(3, 8000, 16, 16)[0] == 7516


def test_refusals_return_before_any_launch(built_lib):
    """The refused calls touch neither their pointers nor the device."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)

    def bq(srcs=ptrs, na=3, B=1, H=64, W=64, ks=7, taps=p, tables=p, nt=9801, weights=p, n_sv=4, out=p, parts=p, ws=p):
        return built_lib.mtd_brisque_each(srcs, na, B, H, W, ks, taps, tables, nt, weights, n_sv, out, parts, ws, None)

    def tv(srcs=ptrs, na=3, B=1, H=64, W=64, norm=1, out=p, ws=p):
        return built_lib.mtd_tv_each(srcs, na, B, H, W, norm, out, ws, None)
    for na, B, H, W in ((0, 1, 64, 64), (4, 1, 64, 64), (3, 0, 64, 64), (3, -1, 64, 64), (3, 1, 15, 64), (3, 1, 64, 15), (3, 1, 1025, 64),
                        (3, 1, 64, 1025), (3, 1, 65536, 65536)):
        assert built_lib.mtd_brisque_ws_bytes(na, B, H, W) == 0 and built_lib.mtd_tv_ws_bytes(na, B, H, W) == 0, (na, B, H, W)
        assert bq(na=na, B=B, H=H, W=W) == -1 and tv(na=na, B=B, H=H, W=W) == -1, (na, B, H, W)
    for null in ("srcs", "taps", "tables", "weights", "out", "ws"):
        assert bq(**{null: None}) == -1, null
    for null in ("srcs", "out", "ws"):
        assert tv(**{null: None}) == -1, null
    for f in (bq, tv):
        assert f(srcs=(ctypes.c_void_p * 3)(p, None, p)) == -1
    for ks in (1, 2, 4, 8, 16, 17, -3):
        assert bq(ks=ks) == -1, ks
    assert bq(nt=0) == -1 and bq(n_sv=0) == -1 and bq(n_sv=-1) == -1
    for norm in (-1, 3):
        assert tv(norm=norm) == -1, norm


def test_python_surface_refusals_without_a_device():
    from mtd_gan_amd import metrics as M
    x = torch.zeros(2, 1, 64, 64)
    pair = R.seeded_svm(2, 3)
    bq = lambda fn: (lambda *a, **kw: fn(*a, weights=kw.pop("weights", pair), **kw))          # noqa: E731
    for fn, name in ((bq(M.brisque_each), "brisque"), (bq(M.brisque_per_slice), "brisque"), (bq(M.compute_BRISQUE), "brisque"), (M.tv_each, "tv"),
                     (M.tv_per_slice, "tv"), (M.compute_TV, "tv")):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(x, x, x)
        with pytest.raises(AssertionError):
            fn(x[:1], x, x)
        with pytest.raises(AssertionError):
            fn(x[0], x[0], x[0])
        with pytest.raises(ValueError, match=name + ".*64x15"):
            fn(x[:, :, :, :15], x[:, :, :, :15], x[:, :, :, :15])
        big = torch.zeros(1, 1, 1025, 16)
        with pytest.raises(ValueError, match="1025x16"):
            fn(big, big, big)
    with pytest.raises(TypeError):
        M.brisque_each(x, x, x)                                        # the weights are the caller's to hand over
    with pytest.raises(ValueError, match="kernel_size"):
        M.brisque_each(x, x, x, weights=pair, kernel_size=6)
    with pytest.raises(ValueError, match="'nearest' only"):
        M.brisque_each(x, x, x, weights=pair, interpolation="bilinear")
    with pytest.raises(ValueError, match="brisque_weights"):
        M.brisque_each(x, x, x, weights=(pair[0], pair[1][:, :35]))
    with pytest.raises(ValueError, match="norm_type"):
        M.tv_each(x, x, x, norm_type="l0")
    for fn in (bq(M.compute_BRISQUE), M.compute_TV):
        with pytest.raises(NotImplementedError):
            fn(x, x, x, data_range=255.0)
