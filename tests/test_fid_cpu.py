"""Host side of FID without a GPU: the float64 restatement the GPU tests compare against (tests/_fid_ref.py) reproduces what the
reference's module/piq/fid.py computed on every fixture case (tests/golden/fid_cases.npz, tools/pin_fid.py); the new entry points
are declared and bound; compute_feat's handling of the extractor; the refusals of fid_statistics."""
import os
import re

import numpy as np
import pytest
import torch

import _fid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FID_ENTRIES = ("mtd_fid_ws_bytes", "mtd_fid_stats", "mtd_fid_gemm", "mtd_fid_residual", "mtd_fid_distance")


def test_fixture_covers_the_cases():
    meta, rows = R.golden()
    assert [(r["case"], r["same"]) for r in rows] == [(c, s) for c in R.CASES for s in (False, True)]
    assert [r["index"] for r in rows] == [i for i in range(len(R.CASES)) for _ in range(2)]
    assert all(r["tol"] >= 1e-12 * r["base"] > 0 and 2 <= r["rounds"] < R.MAX_ITERS for r in rows)
    assert meta["atol"] == R.ATOL and meta["max_iters"] == R.MAX_ITERS


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_restatement_reproduces_the_reference(index):
    _, rows = R.golden()
    a, b = R.case_features(R.CASES[index], index)
    assert a.dtype == torch.float32 and tuple(a.shape) == R.CASES[index][0:3:2] and tuple(b.shape) == R.CASES[index][1:3]
    assert R.crc(a, b) == rows[2 * index]["crc"] == rows[2 * index + 1]["crc"], "the seeded features differ from those the fixture was computed on"
    sb = R.statistics(b)
    for row in rows[2 * index:2 * index + 2]:
        sa = sb if row["same"] else R.statistics(a)
        got = R.distance(sa, sb)
        print(f"{row['case']} same={row['same']}: restatement {got['fid']:.15e} reference {row['fid64']:.15e} |diff| {abs(got['fid'] - row['fid64']):.2e} "
              f"tol {row['tol']:.2e}; rounds {got['rounds']} / {row['rounds']}")
        assert not got["fallback"] and got["finite"]
        assert abs(got["fid"] - row["fid64"]) <= row["tol"]
        assert abs(got["tr"] - row["tr"]) <= row["tol"]
        assert got["rounds"] == row["rounds"]
        assert abs(R.base(sa, sb) - row["base"]) <= 1e-12 * row["base"]
        f32 = np.float32(got["fid"])
        assert abs(float(f32) - float(row["fid32"])) <= float(np.spacing(np.abs(row["fid32"])))


def test_restatement_fallback_and_non_finite_input():
    a, b = R.case_features(R.CASES[0], 0)
    sa, sb = R.statistics(a), R.statistics(b)
    plain = R.distance(sa, sb)
    off = R.distance(sa, sb, offset=R.EPS)
    assert off["finite"] and off["fid"] != plain["fid"] and abs(off["fid"] - plain["fid"]) < 1e-3
    bad = (sa[0], sa[1].clone())
    bad[1][3, 5] = float("inf")
    got = R.distance(bad, sb)
    assert got["fallback"] and got["rounds"] == R.MAX_ITERS and not np.isfinite(got["fid"])


def test_new_entry_points_are_declared_and_bound():
    from mtd_gan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    declared = set(re.findall(r"\b(mtd_[a-z0-9_]+)\s*\(", hdr))
    for n in FID_ENTRIES:
        assert n in _lib.EXPORTS, n
        assert n in declared, n


def test_compute_feat_with_a_stub_extractor():
    from mtd_gan_amd import metrics as M
    seen = []

    def extractor(x):
        seen.append(x)
        return [x[:, :, ::2, ::2] * 2.0]                        # a list of one (B, 3, h, w) map

    g = torch.Generator().manual_seed(5)
    x, y, p = (torch.rand(2, 1, 6, 4, generator=g) for _ in range(3))
    out = M.compute_feat(x, y, p, extractor=extractor)
    assert len(out) == 3 and len(seen) == 3
    for src, got, fed in zip((x, y, p), out, seen):
        assert tuple(fed.shape) == (2, 3, 6, 4) and all(torch.equal(fed[:, c], src[:, 0]) for c in range(3))
        assert tuple(got.shape) == (2, 3 * 3 * 2)
        assert torch.equal(got, (src.repeat(1, 3, 1, 1)[:, :, ::2, ::2] * 2.0).flatten(1))
    # a bare tensor and a one-element tuple are taken as well
    assert torch.equal(M.compute_feat(x, y, p, extractor=lambda t: t.mean(dim=(2, 3)))[0], x.repeat(1, 3, 1, 1).mean(dim=(2, 3)))
    assert tuple(M.compute_feat(x, y, p, device="cpu", extractor=lambda t: (t,))[2].shape) == (2, 72)
    with pytest.raises(AssertionError, match="one layer"):
        M.compute_feat(x, y, p, extractor=lambda t: [t, t])
    with pytest.raises(AssertionError):
        M.compute_feat(x, y[:1], p, extractor=extractor)
    with pytest.raises(TypeError):
        M.compute_feat(x, y, p, extractor=None)


def test_fid_statistics_refusals():
    from mtd_gan_amd import metrics as M
    with pytest.raises(RuntimeError):
        M.fid_statistics(torch.zeros(4, 8))                     # CPU tensor
    with pytest.raises(ValueError):
        M.fid_statistics(torch.zeros(1, 8))                     # N < 2 (the reference: NaN)
    with pytest.raises(AssertionError):
        M.fid_statistics(torch.zeros(4, 2, 8))
    with pytest.raises(RuntimeError):
        M.compute_FID(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 8))
    with pytest.raises(RuntimeError):
        M.fid_distance64((torch.zeros(8, dtype=torch.float64), torch.zeros(8, 8, dtype=torch.float64)),
                         (torch.zeros(8, dtype=torch.float64), torch.zeros(8, 8, dtype=torch.float64)))
