"""BRISQUE and total variation on the device (csrc/brisque.hip) against the reference's own float64 scores, features
and table positions (tests/golden/brisque_tv_piq.npz, written by tools/pin_brisque_tv.py from the reference's own functions).

Bounds.  The fixture's `meta` records the largest relative distance between the reference's OWN float32 and float64 values over
all cases, per quantity class: the scores, the sigma^2 features, the eta features, the total variation.  A quantity's bound is
that distance: the kernels (double, from fp32 sources) are at least as close to float64 as the float32 path a user of the
reference gets.  The alpha features are table values: their positions in the grid must be EQUAL to the reference's float64
positions (the pin tool asserts that no looked-up value lies within 1e-9 of a midpoint between two entries).  What the reference
cannot pin -- a constant slice, on which it asserts, and batch independence -- is held to the float64 restatement of
tests/_brisque_ref.py and to bit equality."""
import ctypes
import json
import math
import types

import numpy as np
import pytest
import torch

import _brisque_ref as R
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu

WHO = ("input", "gt", "pred")


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def bounds(golden):
    out = json.loads(str(golden["meta"]))["spread"]
    print("bounds:", out)
    return out


_inputs = {}


def inputs(index):
    """Case `index`: ((input, target, pred) on the device, the weight table on the device).  Made once, shared, never modified."""
    if index not in _inputs:
        from mtd_gan_amd import metrics as M
        _inputs[index] = tuple(t.cuda() for t in R.case_inputs(index)), M.brisque_weights(R.case_svm(index)).cuda()
    return _inputs[index]


def _brisque(index, *tensors, **kw):
    from mtd_gan_amd import metrics as M
    return M.brisque_each(*tensors, weights=inputs(index)[1], **R.CASES[index][3], **kw)


def _worst(got, want, what, bound, report):
    e = float(np.max(np.abs(got - want) / np.abs(want)))
    if not e <= bound:
        report.append(f"{what}: relative distance {e:.3e} > {bound:.3e}\n  hip {got.tolist()}\n  float64 {want.tolist()}")
    return e


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_scores_features_and_positions_against_the_references_float64(hip_lib, golden, bounds, index):
    from mtd_gan_amd import metrics as M
    B, H, W, opts, n_sv = R.CASES[index]
    sets, _ = inputs(index)
    score, parts = _brisque(index, *sets, parts=True)
    for t, shape in ((score, (3, B)), (parts, (3, B, R.PARTS))):
        assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape
    score, parts = score.cpu().numpy(), parts.cpu().numpy()
    assert np.array_equal(parts[..., 36], score) and np.isfinite(parts).all()
    gamma = M.brisque_ggd_tables()[0].numpy()
    where = np.searchsorted(gamma, parts[..., list(R.ALPHA_AT)])
    assert np.array_equal(gamma[where.clip(0, len(gamma) - 1)], parts[..., list(R.ALPHA_AT)]), "an alpha feature is no value of the grid"
    assert np.array_equal(where, golden[f"where64_{index}"]), (where - golden[f"where64_{index}"])
    report, want = [], golden[f"features64_{index}"]
    worst = dict(sigma=_worst(parts[..., list(R.SIGMA_AT)], want[..., list(R.SIGMA_AT)], "sigma^2 features", bounds["sigma"], report),
                 eta=_worst(parts[..., list(R.ETA_AT)], want[..., list(R.ETA_AT)], "eta features", bounds["eta"], report),
                 score=_worst(score, golden[f"score64_{index}"], "scores", bounds["score"], report))
    tv = np.stack([M.tv_each(*sets, norm_type=norm).cpu().numpy() for norm in R.NORMS])
    assert tv.shape == (3, 3, B) and tv.dtype == np.float64
    worst["tv"] = _worst(tv, golden[f"tv64_{index}"], "total variation", bounds["tv"], report)
    print(f"case {index} {B}x{H}x{W} {opts} n_sv {n_sv}: largest relative distance {worst}")
    assert not report, "\n".join(report)


def test_an_image_does_not_depend_on_its_batch_slot_or_neighbours(hip_lib):
    from mtd_gan_amd import _lib, kernels as K, metrics as M
    for index in (0, 1):                                          # 16 x 16 (B = 3) and the odd 17 x 23 (B = 2)
        (x, y, pred), table = inputs(index)
        B, H, W, opts, _ = R.CASES[index]
        full, full_parts = _brisque(index, x, y, pred, parts=True)
        tv = M.tv_each(x, y, pred)
        for i in range(B):                                        # alone, B = 1
            one, one_parts = _brisque(index, x[i:i + 1], y[i:i + 1], pred[i:i + 1], parts=True)
            assert torch.equal(full[:, i], one[:, 0]) and torch.equal(full_parts[:, i], one_parts[:, 0]), (index, i)
            assert torch.equal(tv[:, i], M.tv_each(x[i:i + 1], y[i:i + 1], pred[i:i + 1])[:, 0]), (index, i)
        x3, y3, p3 = (torch.cat([t[1:2], t[:1], t[1:2]]) for t in (x, y, pred))      # in a batch of 3, other neighbours
        out, out_parts = _brisque(index, x3, y3, p3, parts=True)
        assert torch.equal(out[:, 1], full[:, 0]) and torch.equal(out[:, 0], full[:, 1]) and torch.equal(out[:, 2], full[:, 1]), index
        assert torch.equal(out_parts[:, 1], full_parts[:, 0]) and torch.equal(M.tv_each(x3, y3, p3)[:, 1], tv[:, 0])
        swapped, swapped_parts = _brisque(index, pred, x, y, parts=True)              # the other two image sets exchanged
        assert torch.equal(swapped[[1, 2, 0]], full) and torch.equal(swapped_parts[[1, 2, 0]], full_parts), index
        assert torch.equal(M.tv_each(pred, x, y)[[1, 2, 0]], tv)
        same = _brisque(index, y, y, y)                                              # target as every source: computed once
        assert torch.equal(same[0], full[1]) and torch.equal(same[1], full[1]) and torch.equal(same[2], full[1]), index
        assert torch.equal(_brisque(index, x, y, y.clone()), torch.stack([full[0], full[1], full[1]])), index
        assert torch.equal(M.tv_each(y, y, x), torch.stack([tv[1], tv[1], tv[0]]))
        assert torch.equal(_brisque(index, x, y, pred), full)                         # parts=False: the same scores
        # na = 1 through the ABI: the target alone
        L = _lib.lib()
        o1 = torch.empty(B, dtype=torch.float64, device="cuda")
        p1 = torch.empty((B, M.BRISQUE_PARTS), dtype=torch.float64, device="cuda")
        ptrs = (ctypes.c_void_p * 3)(y.data_ptr(), None, None)
        ks = opts.get("kernel_size", 7)
        taps = M.brisque_gaussian_table(**opts).cuda()
        ggd = M.brisque_ggd_tables().cuda()
        ws = K.workspace(L.mtd_brisque_ws_bytes(1, B, H, W), o1.device)
        assert L.mtd_brisque_each(ptrs, 1, B, H, W, ks, taps.data_ptr(), ggd.data_ptr(), ggd.shape[1], table.data_ptr(), table.shape[0], o1.data_ptr(),
                                  p1.data_ptr(), ws.data_ptr(), K.stream_ptr()) == 0
        assert torch.equal(o1, full[1]) and torch.equal(p1, full_parts[1]), index
        ws = K.workspace(L.mtd_tv_ws_bytes(1, B, H, W), o1.device)
        assert L.mtd_tv_each(ptrs, 1, B, H, W, 1, o1.data_ptr(), ws.data_ptr(), K.stream_ptr()) == 0
        assert torch.equal(o1, tv[1]), index


def test_across_the_chunk_boundary(hip_lib):
    """More 16 x 16 images than a chunk of the workspace holds (7516 of every set in 64 MiB)."""
    from mtd_gan_amd import _lib
    (x, y, pred), _ = inputs(0)
    L = _lib.lib()
    chunk = 7516
    assert L.mtd_brisque_ws_bytes(3, chunk, 16, 16) == L.mtd_brisque_ws_bytes(3, chunk + 3, 16, 16) > L.mtd_brisque_ws_bytes(3, chunk - 1, 16, 16)
    full, full_parts = _brisque(0, x, y, pred, parts=True)
    reps = (chunk + 5) // 3
    many, many_parts = _brisque(0, *(t.repeat(reps, 1, 1, 1) for t in (x, y, pred)), parts=True)
    for i in (0, chunk - 1, chunk, chunk + 1, 3 * reps - 1):
        assert torch.equal(many[:, i], full[:, i % 3]) and torch.equal(many_parts[:, i], full_parts[:, i % 3]), i


def test_a_constant_slice_is_nan_and_leaves_its_neighbours_alone(hip_lib):
    """Where the reference asserts: NaN for that slice alone.  A constant slice's MSCN map is zero but at the border (the filter's
    zero padding), where it is positive: its product maps have no negative value.  A black slice's map is zero everywhere.  The
    restatement gives NaN at the same places."""
    from mtd_gan_amd import metrics as M
    index = 0
    (x, y, pred), table = inputs(index)
    coef, sv = R.case_svm(index)
    const = torch.full_like(x[:1], 0.375)
    xs, ys, ps = (torch.cat([t[:1], const, t[2:3]]) for t in (x, y, pred))
    full, full_parts = _brisque(index, x, y, pred, parts=True)
    out, parts = _brisque(index, xs, ys, ps, parts=True)
    assert torch.isnan(out[:, 1]).all() and torch.isnan(parts[:, 1]).all()
    assert torch.equal(out[:, [0, 2]], full[:, [0, 2]]) and torch.equal(parts[:, [0, 2]], full_parts[:, [0, 2]])
    want = R.brisque(xs.cpu().double(), coef, sv)[0]
    assert torch.isnan(want[1]) and not torch.isnan(want[[0, 2]]).any()
    tv = M.tv_each(xs, ys, ps)
    assert tv[:, 1].tolist() == [0.0] * 3 and torch.equal(tv[:, [0, 2]], M.tv_each(x, y, pred)[:, [0, 2]])
    for norm in ("l1", "l2_squared"):
        assert M.tv_each(xs, ys, ps, norm_type=norm)[:, 1].tolist() == [0.0] * 3
    assert M.compute_TV(const, const, const) == (0.0, 0.0, 0.0) and all(math.isnan(v) for v in M.compute_BRISQUE(const, const, const, weights=table))
    black = torch.zeros_like(const)
    assert torch.isnan(M.brisque_each(black, const, black, weights=table)).all()


def test_per_slice_and_compute_are_the_same_values(hip_lib):
    from mtd_gan_amd import metrics as M
    (x, y, pred), table = inputs(1)
    coef, sv = R.case_svm(1)
    for each, per_slice, compute, kw in ((M.brisque_each, M.brisque_per_slice, M.compute_BRISQUE, dict(weights=table)),
                                         (M.tv_each, M.tv_per_slice, M.compute_TV, {})):
        vals = each(x, y, pred, **kw).tolist()
        assert per_slice(x, y, pred, **kw) == [tuple(vals[k][i] for k in range(3)) for i in range(2)]
        got = compute(x, y, pred, **kw)
        assert isinstance(got, tuple) and len(got) == 3 and all(isinstance(v, float) for v in got)
        for k in range(3):
            mean = (vals[k][0] + vals[k][1]) / 2
            assert abs(got[k] - mean) <= 4e-16 * abs(mean), (k, got[k], mean)
    # the weights in every form, on the host or the device; the options arrive
    base = M.brisque_each(x, y, pred, weights=table)
    assert torch.equal(M.brisque_each(x, y, pred, weights=(coef, sv)), base) and torch.equal(M.brisque_each(x, y, pred, weights=table.cpu()), base)
    assert not torch.equal(M.brisque_each(x, y, pred, weights=table, kernel_size=5), base)
    assert not torch.equal(M.brisque_each(x, y, pred, weights=table, kernel_sigma=1.0), base)
    l1, l2, sq = (M.tv_each(x, y, pred, norm_type=norm) for norm in R.NORMS)
    assert torch.equal(M.tv_each(x, y, pred), l2) and torch.equal(l2, sq.sqrt()) and (l1 > l2).all()


def test_refusals(hip_lib):
    from mtd_gan_amd import metrics as M
    x = torch.zeros(1, 1, 64, 64, device="cuda")
    _, table = inputs(0)
    bq = lambda *a, **kw: M.brisque_each(*a, weights=kw.pop("weights", table), **kw)          # noqa: E731
    for each in (bq, M.tv_each):
        with pytest.raises(RuntimeError, match="CUDA"):
            each(x.cpu(), x, x)
        for bad, size in ((x[:, :, :15, :], "15x64"), (torch.zeros(1, 1, 16, 1025, device="cuda"), "16x1025")):
            with pytest.raises(ValueError, match=size):
                each(bad, bad, bad)
    for k in (6, 8, 17):
        with pytest.raises(ValueError, match="kernel_size"):
            bq(x, x, x, kernel_size=k)
    with pytest.raises(ValueError, match="'nearest' only"):
        bq(x, x, x, interpolation="bicubic")
    with pytest.raises(ValueError, match="brisque_weights"):
        bq(x, x, x, weights=(torch.zeros(4), torch.zeros(4, 35)))
    with pytest.raises(ValueError, match="brisque_weights"):
        bq(x, x, x, weights=table[:, :36])
    with pytest.raises(ValueError, match="norm_type"):
        M.tv_each(x, x, x, norm_type="tv")
    with pytest.raises(NotImplementedError):
        M.compute_TV(x, x, x, data_range=255)
    big = torch.rand(1, 1, 1024, 1024, device="cuda")                 # the largest slice
    assert torch.isfinite(bq(big, big, big)).all() and tuple(M.tv_each(big, big, big).shape) == (3, 1)
    small = torch.rand(1, 1, 16, 1024, device="cuda")
    assert tuple(bq(small, small, small, kernel_size=15).shape) == (3, 1)


# -------------------------------------------------------------------------------------------------------------- engine
PIXEL_KEYS = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in WHO]
MDSI_KEYS = [f"{who}_mdsi" for who in WHO]
BRISQUE_KEYS = [f"{who}_brisque" for who in WHO]
TV_KEYS = [f"{who}_tv" for who in WHO]


class _Pointwise(torch.nn.Module):
    """A stand-in generator whose output for a slice has the same bits in any batch (tests/test_iqa_gpu.py's)."""

    def forward(self, x):
        return 1.05 * x - 0.02


def _loader(x, y, per_batch):
    n = x.shape[0]
    names = [f"L000_{i:04d}.dcm" for i in range(n)]
    return [dict(n_20=x[i:i + per_batch], n_100=y[i:i + per_batch], path_n_20=names[i:i + per_batch], path_n_100=names[i:i + per_batch])
            for i in range(0, n, per_batch)]


def _run(model, loader, tmp_path, tag):
    from mtd_gan_amd import engine
    d = tmp_path / tag
    res = engine.test_MTD_GAN_Ours(model, torch.nn.L1Loss(), loader, torch.device("cuda"), str(d))
    return res, open(d / "pred_results.csv", "rb").read()


@pytest.fixture(scope="module")
def slices():
    return orc.synthetic_ldct(4, seed=9, size=64)


def test_engine_with_test_brisque_and_test_tv(hip_lib, tmp_path, slices):
    from mtd_gan_amd import engine, metrics as M
    x, y = slices
    by_two, by_one = _loader(x, y, 2), _loader(x, y, 1)
    pair = R.seeded_svm(64, 7)
    m = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_per_slice=True)

    # the attributes absent, None, False: the dict and the CSV bytes of the loop as it was
    plain, plain_csv = _run(m, by_two, tmp_path, "plain")
    assert list(plain.keys()) == PIXEL_KEYS
    assert plain_csv.splitlines()[0] == b",PATH,RMSE,PSNR,SSIM"
    for off in (None, False):
        m.test_brisque = m.test_tv = off
        assert _run(m, by_two, tmp_path, f"off_{off!r}") == (plain, plain_csv)

    # per slice: keys after the others, two columns after SSIM, the values of the _each functions on the loop's own clipped prediction
    m.test_brisque, m.test_tv = pair, True
    res, csv = _run(m, by_two, tmp_path, "each")
    assert list(res.keys()) == PIXEL_KEYS + BRISQUE_KEYS + TV_KEYS and {k: res[k] for k in PIXEL_KEYS} == plain
    lines = csv.decode().splitlines()
    assert lines[0] == ",PATH,RMSE,PSNR,SSIM,BRISQUE,TV" and len(lines) == 5
    assert [ln.split(",")[:5] for ln in lines] == [ln.split(",") for ln in plain_csv.decode().splitlines()]
    xd, yd = x.cuda(), y.cuda()
    clipped = (1.05 * xd - 0.02).clamp(0, 1)
    vals = M.brisque_each(xd, yd, clipped, weights=pair).tolist(), M.tv_each(xd, yd, clipped).tolist()
    meters = {}
    for i in range(4):
        assert lines[1 + i].split(",")[5:] == [str(vals[0][2][i]), str(vals[1][2][i])]
        for j, name in enumerate(("brisque", "tv")):
            for k, who in enumerate(WHO):
                meters.setdefault(f"{who}_{name}", engine._Meter()).update(vals[j][k][i], 1)
    assert {k: res[k] for k in BRISQUE_KEYS + TV_KEYS} == {k: round(mm.global_avg, 7) for k, mm in meters.items()}
    assert all(math.isfinite(res[k]) and res[k] > 0 for k in BRISQUE_KEYS + TV_KEYS)

    # beside test_mdsi: behind its keys and column, which stay what they are
    m.test_mdsi = True
    all_, all_csv = _run(m, by_two, tmp_path, "all")
    del m.test_brisque, m.test_tv
    others, others_csv = _run(m, by_two, tmp_path, "others")
    assert list(others.keys()) == PIXEL_KEYS + MDSI_KEYS and list(all_.keys()) == PIXEL_KEYS + MDSI_KEYS + BRISQUE_KEYS + TV_KEYS
    assert {k: all_[k] for k in others} == others and {k: all_[k] for k in BRISQUE_KEYS + TV_KEYS} == {k: res[k] for k in BRISQUE_KEYS + TV_KEYS}
    all_lines = all_csv.decode().splitlines()
    assert all_lines[0] == ",PATH,RMSE,PSNR,SSIM,MDSI,BRISQUE,TV"
    assert [ln.split(",")[:6] for ln in all_lines] == [ln.split(",") for ln in others_csv.decode().splitlines()]
    assert [ln.split(",")[6:] for ln in all_lines[1:]] == [ln.split(",")[5:] for ln in lines[1:]]
    del m.test_mdsi

    # the default path on batches of one: the same keys, columns and -- the generator is pointwise -- the same values
    m.test_brisque, m.test_tv = pair, True
    del m.test_per_slice
    ones, ones_csv = _run(m, by_one, tmp_path, "ones")
    assert list(ones.keys()) == list(res.keys())
    assert [ln.split(",")[5:] for ln in ones_csv.decode().splitlines()] == [ln.split(",")[5:] for ln in lines]
    assert all(ones[k] == res[k] for k in BRISQUE_KEYS + TV_KEYS)
    # ... and a batch of two as ONE sample: the mean over its slices
    twos, twos_csv = _run(m, by_two, tmp_path, "twos")
    assert list(twos.keys()) == list(res.keys())
    for j, ln in enumerate(twos_csv.decode().splitlines()[1:]):
        for c in range(2):
            mean = (vals[c][2][2 * j] + vals[c][2][2 * j + 1]) / 2
            assert abs(float(ln.split(",")[5 + c]) - mean) <= 4e-16 * abs(mean)

    # the dict forms reach the kernels
    m.test_per_slice = True
    m.test_brisque, m.test_tv = dict(weights=pair, kernel_size=9, kernel_sigma=1.5), dict(norm_type="l1")
    other, other_csv = _run(m, by_two, tmp_path, "dict")
    want = M.brisque_each(xd, yd, clipped, weights=pair, kernel_size=9, kernel_sigma=1.5).tolist(), M.tv_each(xd, yd, clipped, norm_type="l1").tolist()
    assert [ln.split(",")[5:] for ln in other_csv.decode().splitlines()[1:]] == [[str(want[0][2][i]), str(want[1][2][i])] for i in range(4)]
    assert list(other.keys()) == list(res.keys()) and other["pred_brisque"] != res["pred_brisque"] and other["pred_tv"] != res["pred_tv"]


def test_a_per_slice_batch_is_read_once(hip_lib, slices, monkeypatch):
    """Under test_per_slice the 6 B values join the batch's single host read: with the options one device tensor per batch crosses
    to the host, as without (the weight table goes to the device once, before the loop)."""
    from mtd_gan_amd import engine, metrics as M
    x, y = slices
    pair = R.seeded_svm(64, 7)
    M.brisque_each(x.cuda(), y.cuda(), x.cuda(), weights=pair)           # (the tables are uploaded before the reads are counted)
    reads = []

    def counted(name):
        real = getattr(torch.Tensor, name)

        def wrapper(self, *a, **kw):
            if self.is_cuda:
                reads.append((name, tuple(self.shape)))
            return real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, wrapper)
    for name in ("tolist", "item", "cpu", "numpy", "__float__"):
        counted(name)
    m = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_per_slice=True)
    loader = [dict(n_20=x.cuda(), n_100=y.cuda())]
    engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, torch.device("cuda"), None)
    assert reads == [("tolist", (7 * 4,))], reads
    del reads[:]
    m.test_brisque, m.test_tv = pair, True
    res = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, torch.device("cuda"), None)
    assert reads == [("tolist", (13 * 4,))], reads
    assert list(res.keys()) == PIXEL_KEYS + BRISQUE_KEYS + TV_KEYS
