"""HaarPSI on the device (csrc/haarpsi.hip) against the reference's own float64 scores (tests/golden/haarpsi_piq.npz)
and the float64 restatement of tests/_haarpsi_ref.py, which tests/test_haarpsi_cpu.py holds to the reference's float64 values.

Bounds.  The fixture's `meta` records the largest relative distance between the reference's OWN float32 and float64 values over
all cases: 6.2e-6 for its scores, 1.26e-7 for its part sums.  The kernels have to be at least as close to float64 as that
float32 path, which is what users of piq call today.  SCORE_BOUND and PARTS_BOUND are four times the distances measured on the
MI355X (MEASURED_SCORE, MEASURED_PARTS; the factor allows for compiler changes), and never above the fixture's."""
import json
import math
import types

import numpy as np
import pytest
import torch

import _haarpsi_ref as R
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu

MEASURED_SCORE, MEASURED_PARTS = 1.82e-7, 5.7e-8          # (so the bounds are 7.3e-7, and for the part sums the fixture's 1.26e-7)
WHO = ("input", "gt", "pred")


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def bounds(golden):
    """(score bound, part-sum bound)"""
    spread = json.loads(str(golden["meta"]))["spread"]
    out = (min(4 * MEASURED_SCORE, spread["score"]), min(4 * MEASURED_PARTS, spread["parts"]))
    print("bounds (score, parts):", out, "the reference's own float32 distances:", spread)
    return out


_reference = {}


def reference(index):
    """Case `index`: the inputs and, per source, the restatement's float64 (score (B,), part sums (B, 4)).  Computed once, shared,
    never modified."""
    if index not in _reference:
        B, H, W, subsample, c, alpha = R.CASES[index]
        x, y, pred = R.case_inputs(index)
        _reference[index] = ((x, y, pred), [R.haarpsi(src.double(), y.double(), subsample, c, alpha) for src in (x, y, pred)])
    return _reference[index]


def _each(index, *tensors, **kw):
    from mtd_gan_amd import metrics as M
    B, H, W, subsample, c, alpha = R.CASES[index]
    return M.haarpsi_each(*tensors, c=c, alpha=alpha, subsample=subsample, **kw)


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_part_sums_then_scores_against_float64(hip_lib, golden, bounds, index):
    """The four sums against the restatement, the scores against the reference's own float64 scores."""
    B, H, W, subsample, c, alpha = R.CASES[index]
    (x, y, pred), ref = reference(index)
    out, parts = _each(index, x.cuda(), y.cuda(), pred.cuda(), parts=True)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (3, B)
    assert parts.is_cuda and parts.dtype == torch.float64 and tuple(parts.shape) == (3, B, 4)
    out, parts = out.tolist(), parts.tolist()
    want = golden[f"score64_{index}"]
    worst = [0.0, 0.0]
    report = []
    for k, who in enumerate(WHO):
        for i in range(B):
            for j in range(4):
                got, w = parts[k][i][j], float(ref[k][1][i, j])
                e = abs(got - w) / abs(w)
                worst[1] = max(worst[1], e)
                if e > bounds[1]:
                    report.append(f"{who} image {i} {R.PART_NAMES[j]}: hip {got!r} float64 {w!r} relative distance {e:.3e} > {bounds[1]:.3e}")
            got, w = out[k][i], float(want[k][i])
            e = abs(got - w) / abs(w)
            worst[0] = max(worst[0], e)
            if e > bounds[0]:
                report.append(f"{who} image {i} score: hip {got!r} float64 {w!r} relative distance {e:.3e} > {bounds[0]:.3e}")
    print(f"case {index} {B}x{H}x{W} subsample={subsample} c={c} alpha={alpha}: largest relative distance (score, parts) {worst}")
    assert not report, "\n".join(report)
    assert all(abs(out[1][i] - 1.0) <= bounds[0] for i in range(B))              # the target against itself


@pytest.mark.parametrize("index", [0, 8])
def test_an_image_does_not_depend_on_its_batch_slot_or_neighbours(hip_lib, index):
    import ctypes
    from mtd_gan_amd import _lib, kernels as K
    B, H, W, subsample, c, alpha = R.CASES[index]
    assert B == 2
    x, y, pred = (t.cuda() for t in reference(index)[0])
    # a batch of 3: slice 0, slice 1, slice 0 again
    x3, y3, p3 = (torch.cat([t, t[:1]]) for t in (x, y, pred))
    out, parts = _each(index, x3, y3, p3, parts=True)
    assert torch.equal(out[:, 0], out[:, 2]) and torch.equal(parts[:, 0], parts[:, 2])
    for i in range(2):
        one, one_parts = _each(index, x[i:i + 1], y[i:i + 1], pred[i:i + 1], parts=True)
        assert torch.equal(out[:, i], one[:, 0]), (i, out[:, i], one[:, 0])
        assert torch.equal(parts[:, i], one_parts[:, 0]), i
    two, two_parts = _each(index, x, y, pred, parts=True)
    assert torch.equal(two, out[:, :2]) and torch.equal(two_parts, parts[:, :2])
    swapped, swapped_parts = _each(index, pred, y, x, parts=True)                   # another slot, other neighbours
    assert torch.equal(swapped[[2, 1, 0]], two) and torch.equal(swapped_parts[[2, 1, 0]], two_parts)
    same = _each(index, x, y, x)
    assert torch.equal(same[0], two[0]) and torch.equal(same[2], two[0])
    assert torch.equal(_each(index, x, y, pred), two)                               # parts=False: the same scores
    # na = 1 through the ABI: the source alone
    L = _lib.lib()
    for k, src in enumerate((x, y, pred)):
        src = src.contiguous()
        o1 = torch.empty(B, dtype=torch.float64, device="cuda")
        p1 = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        ws = K.workspace(L.mtd_haarpsi_ws_bytes(1, B, H, W, int(subsample)), o1.device)
        ptrs = (ctypes.c_void_p * 3)(src.data_ptr(), None, None)
        assert L.mtd_haarpsi_each(ptrs, 1, y.data_ptr(), B, H, W, int(subsample), c, alpha, o1.data_ptr(), p1.data_ptr(), ws.data_ptr(),
                                  K.stream_ptr()) == 0
        assert torch.equal(o1, two[k]) and torch.equal(p1, two_parts[k]), k


def test_per_slice_and_compute_are_the_same_values(hip_lib):
    from mtd_gan_amd import metrics as M
    x, y, pred = (t.cuda() for t in reference(8)[0])
    each = M.haarpsi_each(x, y, pred).tolist()
    per = M.haarpsi_per_slice(x, y, pred)
    assert per == [tuple(each[k][i] for k in range(3)) for i in range(2)]
    got = M.compute_HaarPSI(x, y, pred)
    assert isinstance(got, tuple) and len(got) == 3 and all(isinstance(v, float) for v in got)
    for k in range(3):
        mean = (each[k][0] + each[k][1]) / 2
        assert abs(got[k] - mean) <= 4e-16 * abs(mean), (k, got[k], mean)
    # the parameters arrive: case 13's c and alpha on case 5's shape, subsample off on case 12
    x, y, pred = (t.cuda() for t in reference(13)[0])
    assert M.compute_HaarPSI(x, y, pred, c=10.0, alpha=2.0) == tuple(v[0] for v in M.haarpsi_each(x, y, pred, c=10.0, alpha=2.0).tolist())
    assert abs(M.compute_HaarPSI(x, y, pred, c=10.0, alpha=2.0)[0] - M.compute_HaarPSI(x, y, pred)[0]) > 1e-3
    assert abs(M.compute_HaarPSI(x, y, pred, subsample=False)[0] - M.compute_HaarPSI(x, y, pred)[0]) > 1e-3


def test_edge_values(hip_lib, bounds):
    from mtd_gan_amd import metrics as M
    z = torch.zeros(1, 1, 16, 16, device="cuda")
    for subsample in (True, False):
        out, parts = M.haarpsi_each(z, z, z, subsample=subsample, parts=True)
        assert out.tolist() == [[math.inf]] * 3 and parts.tolist() == [[[0.0] * 4]] * 3          # piq: s = 1, log(1 / 0)
    x = reference(5)[0][0].cuda()
    for subsample in (True, False):
        same = M.haarpsi_each(x, x, x, subsample=subsample).tolist()
        assert all(abs(v[0] - 1.0) <= bounds[0] for v in same), same
    # a constant image responds at its border alone (the filters' zero padding); against a textured one the score is below 1
    flat = torch.full_like(x, 0.5)
    assert all(abs(v[0] - 1.0) <= bounds[0] for v in M.haarpsi_each(flat, flat, flat).tolist())
    v = M.haarpsi_each(flat, x, x).tolist()
    assert 0.0 < v[0][0] < 1.0 and abs(v[1][0] - 1.0) <= bounds[0]


def test_refusals(hip_lib):
    from mtd_gan_amd import metrics as M
    x = torch.zeros(1, 1, 40, 40, device="cuda")
    with pytest.raises(RuntimeError, match="CUDA"):
        M.haarpsi_each(x.cpu(), x, x)
    with pytest.raises(RuntimeError, match="CUDA"):
        M.compute_HaarPSI(x, x, x.cpu())
    with pytest.raises(NotImplementedError):
        M.compute_HaarPSI(x, x, x, data_range=255)
    for subsample in (True, False):
        for small in (x[:, :, :15, :], x[:, :, :, :15]):
            with pytest.raises(ValueError, match="16x16"):
                M.haarpsi_each(small, small, small, subsample=subsample)
        ok = x[:, :, :16, :17]
        assert tuple(M.haarpsi_each(ok, ok, ok, subsample=subsample).shape) == (3, 1)
    for kw in (dict(c=0.0), dict(alpha=0.0), dict(c=-1.0), dict(alpha=-4.2)):
        with pytest.raises(ValueError, match="positive"):
            M.haarpsi_each(x, x, x, **kw)


# -------------------------------------------------------------------------------------------------------------- engine
PIXEL_KEYS = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in WHO]
IQA_KEYS = [f"{who}_gmsd" for who in WHO]          # (64 x 64 slices: GMSD is the one test_iqa metric small enough)
HAARPSI_KEYS = [f"{who}_haarpsi" for who in WHO]


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


def test_engine_with_test_haarpsi(hip_lib, tmp_path, slices):
    from mtd_gan_amd import engine, metrics as M
    x, y = slices
    by_two, by_one = _loader(x, y, 2), _loader(x, y, 1)
    m = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_per_slice=True)

    # the attribute absent, None, False: the dict and the CSV bytes of the loop as it was
    plain, plain_csv = _run(m, by_two, tmp_path, "plain")
    assert list(plain.keys()) == PIXEL_KEYS
    assert plain_csv.splitlines()[0] == b",PATH,RMSE,PSNR,SSIM"
    for off in (None, False):
        m.test_haarpsi = off
        assert _run(m, by_two, tmp_path, f"off_{off!r}") == (plain, plain_csv)

    # per slice: keys after the others, one column after SSIM, the values of haarpsi_each on the loop's own clipped prediction
    m.test_haarpsi = True
    res, csv = _run(m, by_two, tmp_path, "each")
    assert list(res.keys()) == PIXEL_KEYS + HAARPSI_KEYS and {k: res[k] for k in PIXEL_KEYS} == plain
    lines = csv.decode().splitlines()
    assert lines[0] == ",PATH,RMSE,PSNR,SSIM,HaarPSI" and len(lines) == 5
    assert [ln.split(",")[:5] for ln in lines] == [ln.split(",") for ln in plain_csv.decode().splitlines()]
    xd, yd = x.cuda(), y.cuda()
    clipped = (1.05 * xd - 0.02).clamp(0, 1)
    vals = M.haarpsi_each(xd, yd, clipped).tolist()
    meters = {}
    for i in range(4):
        assert lines[1 + i].split(",")[5:] == [str(vals[2][i])]
        for k, who in enumerate(WHO):
            meters.setdefault(f"{who}_haarpsi", engine._Meter()).update(vals[k][i], 1)
    assert {k: res[k] for k in HAARPSI_KEYS} == {k: round(mm.global_avg, 7) for k, mm in meters.items()}
    assert res["gt_haarpsi"] == 1.0 and 0.0 < res["input_haarpsi"] < 1.0 and 0.0 < res["pred_haarpsi"] < 1.0

    # beside test_iqa: behind its keys and columns, which stay what they are without test_haarpsi
    m.test_iqa = ("gmsd",)
    both, both_csv = _run(m, by_two, tmp_path, "both")
    del m.test_haarpsi
    iqa_only, iqa_csv = _run(m, by_two, tmp_path, "iqa_only")
    assert list(iqa_only.keys()) == PIXEL_KEYS + IQA_KEYS and list(both.keys()) == PIXEL_KEYS + IQA_KEYS + HAARPSI_KEYS
    assert {k: both[k] for k in iqa_only} == iqa_only and {k: both[k] for k in HAARPSI_KEYS} == {k: res[k] for k in HAARPSI_KEYS}
    both_lines = both_csv.decode().splitlines()
    assert both_lines[0] == ",PATH,RMSE,PSNR,SSIM,GMSD,HaarPSI"
    assert [ln.split(",")[:6] for ln in both_lines] == [ln.split(",") for ln in iqa_csv.decode().splitlines()]
    assert [ln.split(",")[6:] for ln in both_lines[1:]] == [ln.split(",")[5:] for ln in lines[1:]]
    del m.test_iqa

    # the default path on batches of one: the same keys, columns and -- the generator is pointwise -- the same values
    m.test_haarpsi = True
    del m.test_per_slice
    ones, ones_csv = _run(m, by_one, tmp_path, "ones")
    assert list(ones.keys()) == list(res.keys())
    assert [ln.split(",")[5:] for ln in ones_csv.decode().splitlines()] == [ln.split(",")[5:] for ln in lines]
    assert all(ones[k] == res[k] for k in HAARPSI_KEYS)
    # ... and a batch of two as ONE sample: the mean over its slices
    twos, twos_csv = _run(m, by_two, tmp_path, "twos")
    assert list(twos.keys()) == list(res.keys())
    for j, ln in enumerate(twos_csv.decode().splitlines()[1:]):
        mean = (vals[2][2 * j] + vals[2][2 * j + 1]) / 2
        assert abs(float(ln.split(",")[5]) - mean) <= 4e-16 * abs(mean)

    # the dict form reaches the kernels
    m.test_per_slice = True
    m.test_haarpsi = dict(c=10, alpha=2.0, subsample=False)
    other, other_csv = _run(m, by_two, tmp_path, "dict")
    want = M.haarpsi_each(xd, yd, clipped, c=10, alpha=2.0, subsample=False).tolist()
    assert [ln.split(",")[5] for ln in other_csv.decode().splitlines()[1:]] == [str(v) for v in want[2]]
    assert list(other.keys()) == list(res.keys()) and other["pred_haarpsi"] != res["pred_haarpsi"]


def test_engine_composes_with_stored_input_and_png(hip_lib, tmp_path):
    """test_haarpsi beside test_iqa, test_from_stored and test_save_png under test_per_slice: the values are those of the windowed
    floats the loop itself computes, and the PNGs are written as without it."""
    import os
    from mtd_gan_amd import dicom_io, engine, metrics as M
    g = torch.Generator().manual_seed(5)
    words = [torch.randint(800, 1300, (2, 1, 64, 64), generator=g).to(torch.int16) for _ in range(2)]
    table = torch.tensor([[1.0, -1024.0], [1.0, -1024.0]])
    batch = dict(n_20=words[0], n_100=words[1], rescale_n_20=table, rescale_n_100=table)
    stand_in = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_iqa=("gmsd",), test_haarpsi=True, test_per_slice=True,
                                     test_from_stored=True, test_save_png=True)
    res = engine.test_MTD_GAN_Ours(stand_in, torch.nn.L1Loss(), [batch], torch.device("cuda"), str(tmp_path))
    assert list(res.keys()) == PIXEL_KEYS + IQA_KEYS + HAARPSI_KEYS
    tab = dicom_io.rescale_table(table, 2, torch.device("cuda"))
    xf, yf = (dicom_io.stored_to_window(w.cuda().contiguous(), tab, dicom_io.A_MIN, dicom_io.A_MAX) for w in words)
    vals = M.haarpsi_each(xf, yf, (1.05 * xf - 0.02).clamp(0, 1)).tolist()
    lines = open(tmp_path / "pred_results.csv").read().splitlines()
    assert lines[0] == ",PATH,RMSE,PSNR,SSIM,GMSD,HaarPSI"
    for i in range(2):
        assert lines[1 + i].split(",")[6:] == [str(vals[2][i])]
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".png")]) == 6


def test_a_per_slice_batch_is_read_once(hip_lib, slices, monkeypatch):
    """Under test_per_slice the 3 B HaarPSI values join the batch's single host read: with the option (and test_iqa beside it)
    one device tensor per batch crosses to the host, as without."""
    from mtd_gan_amd import engine
    x, y = slices
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
    m.test_haarpsi = True
    engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, torch.device("cuda"), None)
    assert reads == [("tolist", (10 * 4,))], reads
    del reads[:]
    m.test_iqa = ("gmsd",)
    res = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, torch.device("cuda"), None)
    assert reads == [("tolist", (13 * 4,))], reads
    assert list(res.keys()) == PIXEL_KEYS + IQA_KEYS + HAARPSI_KEYS
