"""VSI and MDSI on the device (csrc/vsi.hip, csrc/mdsi.hip) against the reference's own float64 scores and parts
(tests/golden/vsi_mdsi_piq.npz, written by tools/pin_vsi_mdsi.py from the reference's own functions).

Bounds.  The fixture's `meta` records the largest relative distance between the reference's OWN float32 and float64 values over
all cases, per quantity class: VSI's scores, its four sums (num, den, sum vs, sum gm) and the two limits of the saliency map;
MDSI's scores, its two means and its deviation sum.  A quantity's bound is four times that distance, the rule FSIM is held to:
the kernels are at least about as close to float64 as the float32 path a user of the reference gets.  Where the reference's
float64 value is exactly zero (the constant pair's saliency, a mean's imaginary part without negative similarities) the kernels'
value must be exactly zero."""
import ctypes
import json
import types

import numpy as np
import pytest
import torch

import _mdsi_ref as MR
import _vsi_ref as R
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu

WHO = ("input", "gt", "pred")
MDSI_QUANTITY = ("means", "means", "dev")


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def bounds(golden):
    spread = json.loads(str(golden["meta"]))["spread"]
    out = {q: 4 * v for q, v in spread.items()}
    print("bounds:", out)
    return out


_inputs = {}


def inputs(index):
    """Case `index`: (input, target, pred) on the device.  Made once, shared, never modified."""
    if index not in _inputs:
        _inputs[index] = tuple(t.cuda() for t in R.case_inputs(index))
    return _inputs[index]


def _vsi(index, *tensors, **kw):
    from mtd_gan_amd import metrics as M
    return M.vsi_each(*tensors, **R.CASES[index][4], **kw)


def _mdsi(index, *tensors, **kw):
    from mtd_gan_amd import metrics as M
    return M.mdsi_each(*tensors, **R.CASES[index][5], **kw)


def _distance(got, want, what, bound, worst, key, report):
    if want == 0:
        if got != 0:
            report.append(f"{what}: hip {got!r} where float64 is exactly 0")
        return
    e = abs(got - want) / abs(want)
    worst[key] = max(worst[key], e)
    if not e <= bound:
        report.append(f"{what}: hip {got!r} float64 {want!r} relative distance {e:.3e} > {bound:.3e}")


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_scores_and_parts_against_the_references_float64(hip_lib, golden, bounds, index):
    B, H, W, kind = R.CASES[index][:4]
    x, y, pred = inputs(index)
    v, vp = _vsi(index, x, y, pred, parts=True)
    m, mp = _mdsi(index, x, y, pred, parts=True)
    for t, shape in ((v, (3, B)), (vp, (3, B, 6)), (m, (3, B)), (mp, (3, B, 3))):
        assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape
    v, vp, m, mp = v.tolist(), vp.tolist(), m.tolist(), mp.tolist()
    worst = dict.fromkeys(bounds, 0.0)
    report = []
    for k, who in enumerate(WHO):
        for i in range(B):
            for j, name in enumerate(R.PART_NAMES):
                q = "vsi_" + R.QUANTITY[j]
                _distance(vp[k][i][j], float(golden[f"vsi_parts64_{index}"][k, i, j]), f"vsi {who} image {i} {name}", bounds[q], worst, q, report)
            _distance(v[k][i], float(golden[f"vsi_score64_{index}"][k, i]), f"vsi {who} image {i} score", bounds["vsi_score"], worst, "vsi_score", report)
            for j, name in enumerate(MR.PART_NAMES):
                q = "mdsi_" + MDSI_QUANTITY[j]
                _distance(mp[k][i][j], float(golden[f"mdsi_parts64_{index}"][k, i, j]), f"mdsi {who} image {i} {name}", bounds[q], worst, q, report)
            _distance(m[k][i], float(golden[f"mdsi_score64_{index}"][k, i]), f"mdsi {who} image {i} score", bounds["mdsi_score"], worst,
                      "mdsi_score", report)
    print(f"case {index} {B}x{H}x{W} {kind}: largest relative distance {worst}")
    assert not report, "\n".join(report)
    assert v[1] == [1.0] * B and m[1] == [0.0] * B                # the target against itself, exactly
    if kind == "constant":
        assert v == [[1.0] * B] * 3                               # through the eps terms, as the reference
    if kind == "faint":
        assert mp[0][0][1] != 0.0                                 # negative gs_total carries its phase into the mean


def test_an_image_against_itself_is_exact_in_a_copy_too(hip_lib):
    """gt as a source shares the target's maps; a copy of it is transformed on its own and still gives exactly 1.0 and 0.0."""
    for index in (0, 5, 8):
        x, y, pred = inputs(index)
        assert _vsi(index, y.clone(), y, y.clone()).tolist() == [[1.0] * y.shape[0]] * 3
        assert _mdsi(index, y.clone(), y, y.clone()).tolist() == [[0.0] * y.shape[0]] * 3


def test_an_image_does_not_depend_on_its_batch_slot_or_neighbours(hip_lib):
    from mtd_gan_amd import _lib, kernels as K, metrics as M
    index = 0
    B, H, W = R.CASES[index][:3]
    assert B == 2
    x, y, pred = inputs(index)
    L = _lib.lib()
    for each, name in ((_vsi, "vsi"), (_mdsi, "mdsi")):
        x3, y3, p3 = (torch.cat([t, t[:1]]) for t in (x, y, pred))              # a batch of 3: slice 0, slice 1, slice 0 again
        out, parts = each(index, x3, y3, p3, parts=True)
        assert torch.equal(out[:, 0], out[:, 2]) and torch.equal(parts[:, 0], parts[:, 2]), name
        for i in range(2):
            one, one_parts = each(index, x[i:i + 1], y[i:i + 1], pred[i:i + 1], parts=True)
            assert torch.equal(out[:, i], one[:, 0]) and torch.equal(parts[:, i], one_parts[:, 0]), (name, i)
        two, two_parts = each(index, x, y, pred, parts=True)
        assert torch.equal(two, out[:, :2]) and torch.equal(two_parts, parts[:, :2]), name
        swapped, swapped_parts = each(index, pred, y, x, parts=True)              # another slot, other neighbours
        assert torch.equal(swapped[[2, 1, 0]], two) and torch.equal(swapped_parts[[2, 1, 0]], two_parts), name
        same = each(index, x, y, x)                                               # one image set in two slots
        assert torch.equal(same[0], two[0]) and torch.equal(same[2], two[0]), name
        assert torch.equal(each(index, x, y.clone(), pred)[[0, 2]], two[[0, 2]]), name
        assert torch.equal(each(index, x, y, pred), two), name                    # parts=False: the same scores
        # across the chunk boundary: more images than a chunk holds (VSI: 5 of every set in 64 MiB; MDSI: 8192)
        k = M.vsi_kernel_size(H, W)
        chunk = 5 if name == "vsi" else 8192
        ws_query = L.mtd_vsi_ws_bytes if name == "vsi" else L.mtd_mdsi_ws_bytes
        assert ws_query(3, chunk, H, W, k) == ws_query(3, chunk + 3, H, W, k) > ws_query(3, chunk - 1, H, W, k)
        reps = (chunk + 4) // 2
        many, many_parts = each(index, *(t.repeat(reps, 1, 1, 1) for t in (x, y, pred)), parts=True)
        for i in (chunk - 1, chunk, chunk + 1, 2 * reps - 1):
            assert torch.equal(many[:, i], two[:, i % 2]) and torch.equal(many_parts[:, i], two_parts[:, i % 2]), (name, i)
        # na = 1 through the ABI: the source alone
        for s, src in enumerate((x, y, pred)):
            o1 = torch.empty(B, dtype=torch.float64, device="cuda")
            ptrs = (ctypes.c_void_p * 3)(src.data_ptr(), None, None)
            ws = K.workspace(ws_query(1, B, H, W, k), o1.device)
            if name == "vsi":
                o = R.CASES[index][4]
                p1 = torch.empty((B, M.VSI_PARTS), dtype=torch.float64, device="cuda")
                opts = (ctypes.c_double * 7)(*(o[n] for n in ("c1", "c2", "c3", "alpha", "beta", "sigma_d", "sigma_c")))
                table = M._vsi_table(o["omega_0"], o["sigma_f"], o1.device)
                assert L.mtd_vsi_each(ptrs, 1, y.data_ptr(), B, H, W, k, table.data_ptr(), opts, o1.data_ptr(), p1.data_ptr(), ws.data_ptr(),
                                      K.stream_ptr()) == 0
            else:
                o = R.CASES[index][5]
                p1 = torch.empty((B, M.MDSI_PARTS), dtype=torch.float64, device="cuda")
                opts = (ctypes.c_double * 9)(*(o[n] for n in ("c1", "c2", "c3", "alpha", "beta", "gamma", "rho", "q", "o")))
                assert L.mtd_mdsi_each(ptrs, 1, y.data_ptr(), B, H, W, k, opts, 0, o1.data_ptr(), p1.data_ptr(), ws.data_ptr(), K.stream_ptr()) == 0
            assert torch.equal(o1, two[s]) and torch.equal(p1, two_parts[s]), (name, s)


def test_per_slice_and_compute_are_the_same_values(hip_lib):
    from mtd_gan_amd import metrics as M
    x, y, pred = inputs(0)
    for each, per_slice, compute in ((M.vsi_each, M.vsi_per_slice, M.compute_VSI), (M.mdsi_each, M.mdsi_per_slice, M.compute_MDSI)):
        vals = each(x, y, pred).tolist()
        assert per_slice(x, y, pred) == [tuple(vals[k][i] for k in range(3)) for i in range(2)]
        got = compute(x, y, pred)
        assert isinstance(got, tuple) and len(got) == 3 and all(isinstance(v, float) for v in got)
        for k in range(3):
            mean = (vals[k][0] + vals[k][1]) / 2
            assert abs(got[k] - mean) <= 4e-16 * abs(mean), (k, got[k], mean)
    # the options arrive: case 8's on its own inputs
    x, y, pred = inputs(8)
    assert M.compute_VSI(x, y, pred, **R.OTHER) == tuple(v[0] for v in M.vsi_each(x, y, pred, **R.OTHER).tolist())
    assert M.compute_MDSI(x, y, pred, **R.MDSI_OTHER) == tuple(v[0] for v in M.mdsi_each(x, y, pred, **R.MDSI_OTHER).tolist())
    for name, v in R.OTHER.items():                                # every option alone moves the input's score
        assert M.compute_VSI(x, y, pred, **{name: v})[0] != M.compute_VSI(x, y, pred)[0], name
    for name, v in R.MDSI_OTHER.items():
        if name not in ("alpha", "beta", "gamma"):
            assert M.compute_MDSI(x, y, pred, **{name: v})[0] != M.compute_MDSI(x, y, pred)[0], name
    assert M.compute_MDSI(x, y, pred, alpha=0.5)[0] != M.compute_MDSI(x, y, pred)[0]
    for name in ("beta", "gamma"):
        assert M.compute_MDSI(x, y, pred, combination="mult", **{name: 0.3})[0] != M.compute_MDSI(x, y, pred, combination="mult")[0], name


def test_refusals(hip_lib):
    from mtd_gan_amd import metrics as M
    x = torch.zeros(1, 1, 64, 64, device="cuda")
    for each, compute, name in ((M.vsi_each, M.compute_VSI, "vsi"), (M.mdsi_each, M.compute_MDSI, "mdsi")):
        with pytest.raises(RuntimeError, match="CUDA"):
            each(x.cpu(), x, x)
        with pytest.raises(RuntimeError, match="CUDA"):
            compute(x, x, x.cpu())
        with pytest.raises(NotImplementedError):
            compute(x, x, x, data_range=255)
        for bad, size in ((x[:, :, :15, :], "15x64"), (torch.zeros(1, 1, 16, 1025, device="cuda"), "16x1025")):
            with pytest.raises(ValueError, match=size):
                each(bad, bad, bad)
        ok = x[:, :, :16, :17]
        assert tuple(each(ok, ok, ok).shape) == (3, 1)
        big = torch.zeros(1, 1, 1024, 1024, device="cuda")           # the largest slice, k = 4
        assert each(big, big, big).tolist() == [[1.0 if name == "vsi" else 0.0]] * 3
        with pytest.raises(ValueError, match=name):
            each(x, x, x, c1=-1.0)


# -------------------------------------------------------------------------------------------------------------- engine
PIXEL_KEYS = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in WHO]
FSIM_KEYS = [f"{who}_fsim" for who in WHO]
VSI_KEYS = [f"{who}_vsi" for who in WHO]
MDSI_KEYS = [f"{who}_mdsi" for who in WHO]


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


def test_engine_with_test_vsi_and_test_mdsi(hip_lib, tmp_path, slices):
    from mtd_gan_amd import engine, metrics as M
    x, y = slices
    by_two, by_one = _loader(x, y, 2), _loader(x, y, 1)
    m = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_per_slice=True)

    # the attributes absent, None, False: the dict and the CSV bytes of the loop as it was
    plain, plain_csv = _run(m, by_two, tmp_path, "plain")
    assert list(plain.keys()) == PIXEL_KEYS
    assert plain_csv.splitlines()[0] == b",PATH,RMSE,PSNR,SSIM"
    for off in (None, False):
        m.test_vsi = m.test_mdsi = off
        assert _run(m, by_two, tmp_path, f"off_{off!r}") == (plain, plain_csv)

    # per slice: keys after the others, two columns after SSIM, the values of the _each functions on the loop's own clipped prediction
    m.test_vsi = m.test_mdsi = True
    res, csv = _run(m, by_two, tmp_path, "each")
    assert list(res.keys()) == PIXEL_KEYS + VSI_KEYS + MDSI_KEYS and {k: res[k] for k in PIXEL_KEYS} == plain
    lines = csv.decode().splitlines()
    assert lines[0] == ",PATH,RMSE,PSNR,SSIM,VSI,MDSI" and len(lines) == 5
    assert [ln.split(",")[:5] for ln in lines] == [ln.split(",") for ln in plain_csv.decode().splitlines()]
    xd, yd = x.cuda(), y.cuda()
    clipped = (1.05 * xd - 0.02).clamp(0, 1)
    vals = M.vsi_each(xd, yd, clipped).tolist(), M.mdsi_each(xd, yd, clipped).tolist()
    meters = {}
    for i in range(4):
        assert lines[1 + i].split(",")[5:] == [str(vals[0][2][i]), str(vals[1][2][i])]
        for j, name in enumerate(("vsi", "mdsi")):
            for k, who in enumerate(WHO):
                meters.setdefault(f"{who}_{name}", engine._Meter()).update(vals[j][k][i], 1)
    assert {k: res[k] for k in VSI_KEYS + MDSI_KEYS} == {k: round(mm.global_avg, 7) for k, mm in meters.items()}
    assert res["gt_vsi"] == 1.0 and 0.0 < res["input_vsi"] < 1.0 and 0.0 < res["pred_vsi"] < 1.0
    assert res["gt_mdsi"] == 0.0 and 0.0 < res["input_mdsi"] < 1.0 and 0.0 < res["pred_mdsi"] < 1.0

    # one of the two alone; beside test_fsim: behind its key and column, which stay what they are
    del m.test_vsi
    only, only_csv = _run(m, by_two, tmp_path, "mdsi_only")
    assert list(only.keys()) == PIXEL_KEYS + MDSI_KEYS and only_csv.splitlines()[0] == b",PATH,RMSE,PSNR,SSIM,MDSI"
    assert {k: only[k] for k in MDSI_KEYS} == {k: res[k] for k in MDSI_KEYS}
    m.test_vsi = True
    m.test_fsim = True
    all_, all_csv = _run(m, by_two, tmp_path, "all")
    del m.test_vsi, m.test_mdsi
    others, others_csv = _run(m, by_two, tmp_path, "others")
    assert list(others.keys()) == PIXEL_KEYS + FSIM_KEYS and list(all_.keys()) == PIXEL_KEYS + FSIM_KEYS + VSI_KEYS + MDSI_KEYS
    assert {k: all_[k] for k in others} == others and {k: all_[k] for k in VSI_KEYS + MDSI_KEYS} == {k: res[k] for k in VSI_KEYS + MDSI_KEYS}
    all_lines = all_csv.decode().splitlines()
    assert all_lines[0] == ",PATH,RMSE,PSNR,SSIM,FSIM,VSI,MDSI"
    assert [ln.split(",")[:6] for ln in all_lines] == [ln.split(",") for ln in others_csv.decode().splitlines()]
    assert [ln.split(",")[6:] for ln in all_lines[1:]] == [ln.split(",")[5:] for ln in lines[1:]]
    del m.test_fsim

    # the default path on batches of one: the same keys, columns and -- the generator is pointwise -- the same values
    m.test_vsi = m.test_mdsi = True
    del m.test_per_slice
    ones, ones_csv = _run(m, by_one, tmp_path, "ones")
    assert list(ones.keys()) == list(res.keys())
    assert [ln.split(",")[5:] for ln in ones_csv.decode().splitlines()] == [ln.split(",")[5:] for ln in lines]
    assert all(ones[k] == res[k] for k in VSI_KEYS + MDSI_KEYS)
    # ... and a batch of two as ONE sample: the mean over its slices
    twos, twos_csv = _run(m, by_two, tmp_path, "twos")
    assert list(twos.keys()) == list(res.keys())
    for j, ln in enumerate(twos_csv.decode().splitlines()[1:]):
        for c in range(2):
            mean = (vals[c][2][2 * j] + vals[c][2][2 * j + 1]) / 2
            assert abs(float(ln.split(",")[5 + c]) - mean) <= 4e-16 * abs(mean)

    # the dict forms reach the kernels
    m.test_per_slice = True
    m.test_vsi, m.test_mdsi = dict(R.OTHER), dict(R.MDSI_OTHER)
    other, other_csv = _run(m, by_two, tmp_path, "dict")
    want = M.vsi_each(xd, yd, clipped, **R.OTHER).tolist(), M.mdsi_each(xd, yd, clipped, **R.MDSI_OTHER).tolist()
    assert [ln.split(",")[5:] for ln in other_csv.decode().splitlines()[1:]] == [[str(want[0][2][i]), str(want[1][2][i])] for i in range(4)]
    assert list(other.keys()) == list(res.keys()) and other["pred_vsi"] != res["pred_vsi"] and other["pred_mdsi"] != res["pred_mdsi"]


def test_a_per_slice_batch_is_read_once(hip_lib, slices, monkeypatch):
    """Under test_per_slice the 6 B values join the batch's single host read: with the options one device tensor per batch crosses
    to the host, as without."""
    from mtd_gan_amd import engine, metrics as M
    x, y = slices
    M.vsi_each(x.cuda(), y.cuda(), x.cuda())           # (the log-Gabor table is uploaded before the reads are counted)
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
    m.test_vsi = m.test_mdsi = True
    res = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, torch.device("cuda"), None)
    assert reads == [("tolist", (13 * 4,))], reads
    assert list(res.keys()) == PIXEL_KEYS + VSI_KEYS + MDSI_KEYS
