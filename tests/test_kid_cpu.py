"""Host side of KID without a GPU: the float64 restatement the GPU tests compare against (tests/_kid_ref.py) reproduces what the
reference's module/piq/kid.py computed on every fixture entry (tests/golden/kid_cases.npz, tools/pin_kid.py), draws its subsets
in piq's order and takes whole sets in sorted order; the refusals of metrics.kid_distance64 come before the library is
touched; the entry points are declared and bound."""
import os
import re

import pytest
import torch

import _kid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KID_ENTRIES = ("mtd_kid_ws_bytes", "mtd_kid")
ENTRIES = R.entries()


def test_fixture_covers_the_cases():
    meta, rows = R.golden()
    assert [(r["index"], r["same"]) for r in rows] == ENTRIES and meta["entries"] == len(rows)
    assert len(meta["spread"]) == len(meta["vspread"]) == len(rows)
    assert all(r["tol"] >= 1e-12 * r["base"] > 0 for r in rows)
    assert all(r["vtol"] >= 1e-12 * r["vbase"] > 0 for r in rows if r["has_var"])
    # the bound tells float64 work from float32 work: piq's own float32 value misses it somewhere
    assert any(r["has_32"] and abs(float(r["mmd2_32"]) - r["mmd2_64"]) > r["tol"] for r in rows)
    sizes = {(c["Np"], c["D"]) for c in R.WHOLE}
    assert sizes == {(2, 1), (3, 1), (5, 7), (63, 15), (64, 16), (65, 17), (130, 33), (200, 520), (211, 2048), (96, 96)}


@pytest.mark.parametrize("entry", range(len(ENTRIES)))
def test_restatement_reproduces_the_reference(entry):
    """Also the draw order: the subset cases hold piq's values after torch.manual_seed(seed of the case), and the restatement
    draws from the same seed."""
    _, rows = R.golden()
    row = rows[entry]
    index, same = ENTRIES[entry]
    case = R.CASES[index]
    a, b = R.case_features(case, index)
    assert a.dtype == torch.float32 and tuple(a.shape) == (case["Np"], case["D"]) and tuple(b.shape) == (case["Nt"], case["D"])
    assert R.crc(a, b) == row["crc"], "the seeded features differ from those the fixture was computed on"
    p = b if same else a
    got = R.kid(p, b, case, ret_var=row["has_var"])
    print(f"#{index} same={same}: restatement {got['mmd2']:.15e} reference {row['mmd2_64']:.15e} |diff| {abs(got['mmd2'] - row['mmd2_64']):.2e} tol {row['tol']:.2e}; "
          f"var {got['var']:.6e} / {row['var_64']:.6e} |diff| {abs(got['var'] - row['var_64']):.2e} vtol {row['vtol']:.2e}")
    assert abs(got["mmd2"] - row["mmd2_64"]) <= row["tol"]
    assert abs(got["var"] - row["var_64"]) <= row["vtol"]
    assert abs(got["base"] - row["base"]) <= 1e-12 * row["base"] and abs(got["vbase"] - row["vbase"]) <= 1e-12 * row["vbase"]
    if case["subsets"] is not None:                      # another seed gives other subsets and another value
        other = R.kid(p, b, dict(case, seed=case["seed"] + 100), ret_var=row["has_var"])
        assert abs(other["mmd2"] - row["mmd2_64"]) > 1e3 * row["tol"]


def test_draw_order_and_the_sorted_whole_set_rule():
    from mtd_gan_amd import metrics as M
    torch.manual_seed(5)
    p1, t1 = torch.randperm(9)[:4], torch.randperm(7)[:4]
    p2, t2 = torch.randperm(9)[:4], torch.randperm(7)[:4]
    after = torch.randperm(5)
    for draw in (R.draw, M.kid_draw_subsets):
        torch.manual_seed(5)
        pi, ti = draw(9, 7, 4, 2)
        assert torch.equal(pi, torch.stack([p1, p2])) and torch.equal(ti, torch.stack([t1, t2]))
        assert torch.equal(torch.randperm(5), after)      # the generator is where piq leaves it
        torch.manual_seed(5)
        pi, ti = draw(7, 9, 7, 2)                          # the predicted set whole: sorted; the target's subset as drawn
        assert torch.equal(pi, torch.arange(7).repeat(2, 1))
        torch.manual_seed(5)
        torch.randperm(7)
        assert torch.equal(ti[0], torch.randperm(9)[:7])
    # the whole-set value does not depend on the seed
    case = R.CASES[5]
    a, b = R.case_features(case, 5)
    assert R.kid(a, b, dict(case, seed=1))["mmd2"] == R.kid(a, b, dict(case, seed=2))["mmd2"]


def test_refusals_come_before_the_library(monkeypatch):
    from mtd_gan_amd import _lib, metrics as M

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    x, y = torch.zeros(6, 4), torch.zeros(5, 4)
    bad = [dict(), dict(average=True, n_subsets=2, subset_size=6),                 # m = 6 > N_targ = 5, twice
           dict(average=True, n_subsets=2, subset_size=1), dict(average=True, subset_size=2, ret_var=True),
           dict(average=True, subset_size=3, n_subsets=0), dict(average=True, subset_size=3, n_subsets=M.KID_MAX_SUBSETS + 1),
           dict(average=True, subset_size=3, degree=0), dict(average=True, subset_size=3, degree=9), dict(average=True, subset_size=3, degree=2.0),
           dict(average=True, subset_size=3, degree=True), dict(average=True, subset_size=3, mmd_est="u"),
           dict(subsets=(torch.zeros(1, 3, dtype=torch.long), torch.full((1, 3), 5))), dict(subsets=(torch.zeros(1, 3), torch.zeros(1, 3))),
           dict(subsets=(torch.zeros(1, 3, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long))),
           dict(subsets=(torch.tensor([[0, 1, -1]]), torch.zeros(1, 3, dtype=torch.long))),
           dict(average=True, subset_size=3, ret_var=True, var_at_m=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            M.kid_distance64(x, y, **kw)
    with pytest.raises(ValueError):
        M.kid_distance64(x[:1], y)                           # m = 1
    with pytest.raises(ValueError):
        M.kid_distance64(x[:2], y, ret_var=True)             # m = 2 with the variance
    with pytest.raises(ValueError):
        M.compute_KID(x, y, x, parts=True)
    with pytest.raises(TypeError):
        M.kid_distance64(x.double(), y)
    with pytest.raises(AssertionError):
        M.kid_distance64(x, torch.zeros(5, 3))
    with pytest.raises(AssertionError):
        M.kid_distance64(x[0], y)
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="CUDA"):          # good arguments on CPU tensors: no fallback, and still no library
        M.kid_distance64(x[:5], y)
    assert not torch.equal(torch.get_rng_state(), state)     # (the draw was made)


def test_test_loop_option_is_checked_first():
    from mtd_gan_amd import engine

    class Model:
        pass
    m = Model()
    assert engine._kid_option(m) is None
    m.test_kid = False
    assert engine._kid_option(m) is None
    m.test_kid = True
    with pytest.raises(ValueError, match="fid_features"):
        engine._kid_option(m)
    m.fid_features = lambda t: t
    assert engine._kid_option(m) == {}
    m.test_kid = dict(ret_var=True, degree=2)
    assert engine._kid_option(m) == dict(ret_var=True, degree=2)
    for cfg in (3, "yes", dict(parts=True), {1: 2}):
        m.test_kid = cfg
        with pytest.raises(ValueError, match="test_kid"):
            engine._kid_option(m)


def test_new_entry_points_are_declared_and_bound():
    from mtd_gan_amd import _lib, metrics as M
    hdr = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    declared = set(re.findall(r"\b(mtd_[a-z0-9_]+)\s*\(", hdr))
    for n in KID_ENTRIES:
        assert n in _lib.EXPORTS, n
        assert n in declared, n
    assert int(re.search(r"#define\s+MTD_KID_PARTS\s+(\d+)", hdr).group(1)) == M.KID_PARTS == len(R.PARTS)
    assert M.KID_MMD_ESTS == R.MMD_ESTS
