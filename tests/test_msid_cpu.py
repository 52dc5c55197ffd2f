"""Host side of MSID and the Inception Score without a GPU: the float64 restatement the GPU tests compare against
(tests/_msid_ref.py) reproduces what the reference's module/piq/msid.py and isc.py computed on every fixture entry
(tests/golden/msid_is_cases.npz, tools/pin_msid.py), draws its starting vectors in piq's order, and computes the temperature
tables in the dtype of ts as metrics.msid_tables does; the refusals of metrics.msid_distance64 / inception_score64 and of the
two engine options come before the library is touched; the entry points are declared and bound."""
import os
import re

import numpy as np
import pytest
import torch

import _msid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSID_ENTRIES = ("mtd_msid_ws_bytes", "mtd_msid_panel_rows", "mtd_msid_distances", "mtd_msid_neighbours", "mtd_msid_graph", "mtd_msid_lanczos",
                "mtd_msid_quadrature", "mtd_msid_combine", "mtd_msid_distance", "mtd_msid_descriptor", "mtd_is_ws_bytes", "mtd_inception_score")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    return _lib.lib()


def test_fixture_covers_the_cases():
    meta, z = R.golden()
    assert meta["cases"] == len(R.CASES) == len(z["score64"]) and meta["is_cases"] == len(R.IS_CASES) and meta["early_breaks"] >= 1
    sizes = {(c["Np"], c["Nt"]) for c in R.CASES}
    assert {(7, 8), (9, 9), (40, 40), (65, 65), (130, 300), (64, 64)} <= sizes
    opts = [c["opts"] for c in R.CASES]
    for want in (dict(niters=16), dict(k=2, m=3, niters=33), dict(m=2), dict(rademacher=True), dict(normalized_laplacian=False),
                 dict(normalize="complete"), dict(normalize="er"), dict(normalize="none"), dict(msid_mode="l2")):
        assert want in opts
    assert any(c["D"] == 2048 and c["Np"] == 64 for c in R.CASES) and R.CASES[R.UNEQUAL_F64]["ts"] == "f64x5"
    assert (z["dtol"] > 0).all() and (z["stol"] > 0).all()
    filled, ms = z["filled"], np.array([R.options(c)["m"] for c in R.CASES])
    assert (filled < ms[:, None]).any() and (filled[2:] == ms[2:, None]).all()      # the small sets break early, the others never


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_restatement_reproduces_the_reference(index):
    """Also the draw order: the fixture holds piq's values after np.random.seed(seed of the case)."""
    _, z = R.golden()
    case = R.CASES[index]
    p, t = R.case_features(case)
    assert p.dtype == torch.float32 and tuple(p.shape) == (case["Np"], case["D"]) and tuple(t.shape) == (case["Nt"], case["D"])
    assert R.crc(p, t) == int(z["crc"][index]), "the seeded features differ from those the fixture was computed on"
    got = R.msid(case)
    for side, key in enumerate(("pred", "targ")):
        want = z[f"desc_{index}_{side}"]
        diff = np.abs(got[key]["desc"] - want).max()
        print(f"#{index}.{side}: restatement against the reference max |diff| {diff:.2e} tol {z['dtol'][index, side]:.2e} filled {got[key]['filled']}")
        assert diff <= z["dtol"][index, side] and got[key]["filled"] == z["filled"][index, side]
        assert got[key]["gap"] > 1e-6
    assert abs(got["score"] - z["score64"][index]) <= z["stol"][index]
    other = R.msid(dict(case, seed=case["seed"] + 100), *(x.numpy() for x in (p, t)))      # other vectors, another value
    assert np.abs(other["pred"]["desc"] - z[f"desc_{index}_0"]).max() > 1e3 * z["dtol"][index, 0]


@pytest.mark.parametrize("index", range(len(R.IS_CASES)))
def test_inception_score_restatement(index):
    _, z = R.golden()
    x = R.is_features(index)
    assert R.crc(x) == int(z["is_crc"][index])
    mean, std, parts = R.inception_score(x.numpy(), R.IS_CASES[index][2])
    assert abs(mean - z["is_val"][index, 0]) <= z["is_tol"][index, 0] and len(parts) == R.IS_CASES[index][2]
    if R.IS_CASES[index][2] == 1:
        assert np.isnan(std) and np.isnan(z["is_val"][index, 1])
    else:
        assert abs(std - z["is_val"][index, 1]) <= z["is_tol"][index, 1]
    if index + 1 < len(R.IS_CASES):
        S = min(R.IS_CASES[index][2], R.IS_CASES[index + 1][2])
        d = abs(R.inception_score(x.numpy(), S)[0] - R.inception_score(R.is_features(index + 1).numpy(), S)[0])
        assert abs(d - z["is_dist"][index, 0]) <= 1e-11 * d + 1e-11 and z["is_dist"][index, 0] == z["is_dist"][index, 1]


def test_tables_follow_the_dtype_of_ts():
    from mtd_gan_amd import metrics as M
    ts32 = torch.logspace(-1, 1, 256).numpy()
    for n, k, mode in ((130, 5, "empty"), (300, 5, "complete"), (40, 2, "er"), (40, 5, "none")):
        for ts in (ts32, ts32.astype(np.float64)):
            a, ca = M.msid_tables(ts, n, k, mode)
            b, cb = R.tables(ts, n, k, mode)
            assert a.dtype == np.float64 and np.array_equal(a, b) and np.array_equal(ca, cb)
        a32, a64 = M.msid_tables(ts32, n, k, mode)[0], M.msid_tables(ts32.astype(np.float64), n, k, mode)[0]
        assert np.array_equal(a32[0], np.exp(ts32).astype(np.float64)) and not np.array_equal(a32[1], a64[1])
    assert M._msid_ts(None).dtype == np.float32 and np.array_equal(M._msid_ts(None), ts32)


def test_refusals_come_before_the_library(monkeypatch):
    from mtd_gan_amd import _lib, metrics as M

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    x, y = torch.zeros(12, 4), torch.zeros(14, 4)
    bad = [dict(k=0), dict(k=64), dict(k=11), dict(k=2.0), dict(k=True), dict(m=1), dict(m=33), dict(niters=0), dict(niters=4097),
           dict(normalize="full"), dict(msid_mode="l1"), dict(ts=np.ones((2, 2))), dict(ts=np.arange(3)), dict(ts=np.zeros(0)),
           dict(starting_vectors=np.zeros((12, 100))), dict(starting_vectors=(np.zeros((12, 100)), np.zeros((14, 99)))),
           dict(starting_vectors=(np.zeros((12, 100), dtype=np.float32), np.zeros((14, 100))))]
    for kw in bad:
        with pytest.raises(ValueError):
            M.msid_distance64(x, y, **kw)
    with pytest.raises(ValueError):
        M.msid_distance64(x[:6], y)                          # N = 6 < k + 2
    with pytest.raises(ValueError):
        M.msid_descriptor64(x, normalize="er", k=0)
    with pytest.raises(ValueError):
        M.compute_MSID(x, y, x, parts=True)
    with pytest.raises(TypeError):
        M.msid_distance64(x.double(), y)
    with pytest.raises(AssertionError):
        M.msid_distance64(x[0], y)
    for kw in (dict(num_splits=0), dict(num_splits=13), dict(num_splits=2.0), dict(num_splits=True)):
        with pytest.raises(ValueError):
            M.inception_score64(x, **kw)
    with pytest.raises(ValueError):
        M.is_distance64(x, y, distance="l3")
    with pytest.raises(ValueError):
        M.is_distance64(y, x, num_splits=13)                 # the target is too short
    np.random.seed(3)
    state = np.random.get_state()[1].copy()
    with pytest.raises(RuntimeError, match="CUDA"):          # good arguments on CPU tensors: no fallback, and still no library
        M.msid_distance64(x, y)
    assert not np.array_equal(np.random.get_state()[1], state)      # (the draws were made)
    np.random.seed(3)
    want = (np.random.randn(12, 100), np.random.randn(14, 100))     # ... the predicted set's first
    np.random.seed(3)
    got = [M._msid_plan(n, None, 5, 10, 100, False, True, "empty", None)[2] for n in (12, 14)]
    assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    np.random.seed(3)
    assert np.array_equal(M._msid_plan(12, None, 5, 10, 100, True, True, "empty", None)[2].numpy(), np.sign(want[0]))
    with pytest.raises(RuntimeError, match="CUDA"):
        M.inception_score64(x)
    with pytest.raises(RuntimeError, match="CUDA"):
        M.is_distance64(x, y, num_splits=3, distance="l2")


def test_test_loop_options_are_checked_first():
    from mtd_gan_amd import engine

    class Model:
        pass
    for attr, option, good in (("test_msid", engine._msid_option, dict(k=3, msid_mode="l2")), ("test_is", engine._is_option, dict(num_splits=2))):
        m = Model()
        assert option(m) is None
        setattr(m, attr, False)
        assert option(m) is None
        setattr(m, attr, True)
        with pytest.raises(ValueError, match="fid_features"):
            option(m)
        m.fid_features = lambda t: t
        assert option(m) == {}
        setattr(m, attr, good)
        assert option(m) == good
        for cfg in (3, "yes", dict(parts=True), {1: 2}):
            setattr(m, attr, cfg)
            with pytest.raises(ValueError, match=attr):
                option(m)


def test_new_entry_points_are_declared_and_bound(built_lib):
    from mtd_gan_amd import _lib, metrics as M
    hdr = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    declared = set(re.findall(r"\b(mtd_[a-z0-9_]+)\s*\(", hdr))
    for n in MSID_ENTRIES:
        assert n in _lib.EXPORTS and n in declared and len(getattr(built_lib, n).argtypes) > 0, n
    assert int(re.search(r"#define\s+MTD_MSID_MAX_N\s+(\d+)", hdr).group(1)) == M.MSID_MAX_N
    # the size queries need no device: out-of-range sizes give 0, the panel of distances stays within 32 MiB (or one tile row)
    L = built_lib
    assert L.mtd_msid_ws_bytes(1000, 2048, 5, 10, 100, 256) > 0
    for bad in ((6, 8, 5, 10, 100, 256), (32769, 8, 5, 10, 100, 256), (100, 0, 5, 10, 100, 256), (100, 8, 0, 10, 100, 256), (100, 8, 64, 10, 100, 256),
                (100, 8, 5, 1, 100, 256), (100, 8, 5, 33, 100, 256), (100, 8, 5, 10, 0, 256), (100, 8, 5, 10, 4097, 256), (100, 8, 5, 10, 100, 0)):
        assert L.mtd_msid_ws_bytes(*bad) == 0, bad
    for N in (7, 64, 65, 1000, 5000, 32768):
        P = L.mtd_msid_panel_rows(N)
        assert P % 64 == 0 and 64 <= P <= (N + 63) // 64 * 64 and (P * N * 8 <= 32 << 20 or P == 64)
    assert L.mtd_is_ws_bytes(10, 4, 11) == 0 and L.mtd_is_ws_bytes(10, 4, 0) == 0 and L.mtd_is_ws_bytes(10, 4, 10) > 0
