"""FSIM on the device (csrc/fsim.hip) against the reference's own float64 scores (tests/golden/fsim_piq.npz) and the
float64 restatement of tests/_fsim_ref.py, which tests/test_fsim_cpu.py holds to the reference's float64 values.

Bounds.  The fixture's `meta` records the largest relative distance between the reference's OWN float32 and float64 values over
all cases, per quantity: its scores, its four sums (num, den, sum pc, sum gm) and its noise thresholds.  A quantity's bound is
four times that distance: an equally careful fp32 pipeline with another FFT factorisation realises another rounding error of
the same size (and the reference's float32 score carries a final float32 rounding that the kernels' double finish does not).
Where the distance measured on the MI355X (MEASURED_*) is known, the bound is min(4 x measured, that ceiling)."""
import json
import math
import types

import numpy as np
import pytest
import torch

import _fsim_ref as R
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu

# The largest relative distances to float64 measured on the MI355X over the twelve cases: the bounds are 1.76e-7 for
# the scores, 5.44e-6 for the sums and 1.036e-5 for the thresholds, each below its ceiling (9.1e-7, 8.1e-6, 1.055e-5).
MEASURED = dict(score=4.4e-8, sums=1.36e-6, T=2.59e-6)
WHO = ("input", "gt", "pred")


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def bounds(golden):
    """{score, sums, T} -> bound"""
    spread = json.loads(str(golden["meta"]))["spread"]
    out = {q: 4 * spread[q] if MEASURED[q] is None else min(4 * MEASURED[q], 4 * spread[q]) for q in ("score", "sums", "T")}
    print("bounds:", out, "the reference's own float32 distances:", spread)
    return out


_reference = {}


def reference(index):
    """Case `index`: the inputs and, per source, the restatement's float64 (score (B,), parts (B, 4 + O)).  Computed once, shared,
    never modified."""
    if index not in _reference:
        B, H, W, opts = R.CASES[index]
        x, y, pred = R.case_inputs(index)
        _reference[index] = ((x, y, pred), [R.fsim(src.double(), y.double(), **opts) for src in (x, y, pred)])
    return _reference[index]


def _each(index, *tensors, **kw):
    from mtd_gan_amd import metrics as M
    return M.fsim_each(*tensors, **R.CASES[index][3], **kw)


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_thresholds_and_sums_then_scores_against_float64(hip_lib, golden, bounds, index):
    """The thresholds and the four sums against the restatement, the scores against the reference's own float64 scores."""
    B, H, W, opts = R.CASES[index]
    O = opts["orientations"]
    names = R.part_names(O)
    (x, y, pred), ref = reference(index)
    out, parts = _each(index, x.cuda(), y.cuda(), pred.cuda(), parts=True)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (3, B)
    assert parts.is_cuda and parts.dtype == torch.float64 and tuple(parts.shape) == (3, B, 4 + O)
    out, parts = out.tolist(), parts.tolist()
    want = golden[f"score64_{index}"]
    worst = dict(score=0.0, sums=0.0, T=0.0)
    report = []
    for k, who in enumerate(WHO):
        for i in range(B):
            for j, name in enumerate(names):
                q = "sums" if j < 4 else "T"
                got, w = parts[k][i][j], float(ref[k][1][i, j])
                e = abs(got - w) / abs(w)
                worst[q] = max(worst[q], e)
                if not e <= bounds[q]:
                    report.append(f"{who} image {i} {name}: hip {got!r} float64 {w!r} relative distance {e:.3e} > {bounds[q]:.3e}")
            got, w = out[k][i], float(want[k][i])
            e = abs(got - w) / abs(w)
            worst["score"] = max(worst["score"], e)
            if not e <= bounds["score"]:
                report.append(f"{who} image {i} score: hip {got!r} float64 {w!r} relative distance {e:.3e} > {bounds['score']:.3e}")
    print(f"case {index} {B}x{H}x{W} {opts}: largest relative distance {worst}")
    assert not report, "\n".join(report)
    assert all(abs(out[1][i] - 1.0) <= bounds["score"] for i in range(B))              # the target against itself


def test_eight_orientations_walk_the_workspace_in_two_groups(hip_lib, golden):
    """orientations=8 on the 256 x 256 case: one image of every set no longer fits the 64 MiB of workspace with all filtered
    spectra at once, so the orientations go in two groups of four.  No fixture row: against the float64
    restatement, each quantity within four times the reference's own float32 distance for that quantity (the fixture's
    ceilings; the distances measured on the twelve pinned cases do not cover these options)."""
    from mtd_gan_amd import metrics as M
    spread = json.loads(str(golden["meta"]))["spread"]
    opts = dict(R.DEFAULTS, orientations=8)
    x, y, pred = reference(7)[0]
    out, parts = M.fsim_each(x.cuda(), y.cuda(), pred.cuda(), parts=True, **opts)
    assert tuple(parts.shape) == (3, 1, 12)
    out, parts = out.tolist(), parts.tolist()
    worst = dict(score=0.0, sums=0.0, T=0.0)
    for k, src in enumerate((x, y, pred)):
        score, want = R.fsim(src.double(), y.double(), **opts)
        worst["score"] = max(worst["score"], abs(out[k][0] - float(score[0])) / float(score[0]))
        for j in range(12):
            q = "sums" if j < 4 else "T"
            worst[q] = max(worst[q], abs(parts[k][0][j] - float(want[0, j])) / abs(float(want[0, j])))
    print("orientations=8 at 256x256: largest relative distance", worst)
    assert all(worst[q] <= 4 * spread[q] for q in worst), (worst, spread)


@pytest.mark.parametrize("index", [0, 5])
def test_an_image_does_not_depend_on_its_batch_slot_or_neighbours(hip_lib, index):
    import ctypes
    from mtd_gan_amd import _lib, kernels as K, metrics as M
    B, H, W, opts = R.CASES[index]
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
    same = _each(index, x, y, x)                                                    # one image set in two slots: transformed once
    assert torch.equal(same[0], two[0]) and torch.equal(same[2], two[0])
    assert torch.equal(_each(index, x, y.clone(), pred)[[0, 2]], two[[0, 2]])       # the target's copy as a source: transformed twice
    assert torch.equal(_each(index, x, y, pred), two)                               # parts=False: the same scores
    # na = 1 through the ABI: the source alone
    L = _lib.lib()
    ks, h, w = M.fsim_pooled_size(H, W)
    o = {k: v for k, v in opts.items() if k != "k"}
    table, consts = M._fsim_tables(h, w, *(o[n] for n in M.FSIM_OPTIONS[:6]), x.device)
    for k, src in enumerate((x, y, pred)):
        src = src.contiguous()
        o1 = torch.empty(B, dtype=torch.float64, device="cuda")
        p1 = torch.empty((B, 4 + o["orientations"]), dtype=torch.float64, device="cuda")
        ws = K.workspace(L.mtd_fsim_ws_bytes(1, B, h, w, o["scales"], o["orientations"]), o1.device)
        ptrs = (ctypes.c_void_p * 3)(src.data_ptr(), None, None)
        assert L.mtd_fsim_each(ptrs, 1, y.data_ptr(), B, H, W, ks, o["scales"], o["orientations"], opts["k"], table.data_ptr(),
                               consts.data_ptr(), o1.data_ptr(), p1.data_ptr(), ws.data_ptr(), K.stream_ptr()) == 0
        assert torch.equal(o1, two[k]) and torch.equal(p1, two_parts[k]), k


def test_the_selection_is_torch_median_bit_for_bit(hip_lib):
    """The radix select of the thresholds on buffers of its own: the element of rank (n - 1) // 2, torch.median's, at the sizes
    of a 16 x 16, a 256 x 256 and a 512 x 512 map -- random squares, all-equal values, two distinct values split exactly in
    half (the lower one is the median), and a buffer with one inf."""
    from mtd_gan_amd import _lib, kernels as K
    L = _lib.lib()
    g = torch.Generator().manual_seed(17)
    for n in (256, 65536, 262144):
        rows = [torch.randn(n, generator=g) ** 2 * 1e3, torch.rand(n, generator=g) * 1e-30, torch.full((n,), 3.25), torch.zeros(n)]
        halves = torch.cat([torch.full((n // 2,), 7.5), torch.full((n // 2,), 7.500001)])
        rows.append(halves[torch.randperm(n, generator=g)])
        with_inf = torch.rand(n, generator=g)
        with_inf[n // 3] = math.inf
        rows.append(with_inf)
        rows.append(torch.cat([torch.zeros(n // 2 - 1), torch.full((n // 2 + 1,), 1e-45)]))          # a denormal above zeros
        v = torch.stack(rows).cuda().contiguous()
        out = torch.empty(len(rows), dtype=torch.float32, device="cuda")
        assert L.mtd_fsim_median(v.data_ptr(), n, len(rows), out.data_ptr(), K.stream_ptr()) == 0
        want = torch.median(v, dim=1).values
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (n, out.tolist(), want.tolist())
        assert float(out[4]) == 7.5 and float(out[2]) == 3.25 and float(out[3]) == 0.0


def test_per_slice_and_compute_are_the_same_values(hip_lib):
    from mtd_gan_amd import metrics as M
    x, y, pred = (t.cuda() for t in reference(5)[0])
    each = M.fsim_each(x, y, pred).tolist()
    per = M.fsim_per_slice(x, y, pred)
    assert per == [tuple(each[k][i] for k in range(3)) for i in range(2)]
    got = M.compute_FSIM(x, y, pred)
    assert isinstance(got, tuple) and len(got) == 3 and all(isinstance(v, float) for v in got)
    for k in range(3):
        mean = (each[k][0] + each[k][1]) / 2
        assert abs(got[k] - mean) <= 4e-16 * abs(mean), (k, got[k], mean)
    # the options arrive: case 11's on its own inputs
    x, y, pred = (t.cuda() for t in reference(11)[0])
    assert M.compute_FSIM(x, y, pred, **R.OTHER) == tuple(v[0] for v in M.fsim_each(x, y, pred, **R.OTHER).tolist())
    assert M.fsim_per_slice(x, y, pred, **R.OTHER) == [tuple(v[0] for v in M.fsim_each(x, y, pred, **R.OTHER).tolist())]
    assert abs(M.compute_FSIM(x, y, pred, **R.OTHER)[0] - M.compute_FSIM(x, y, pred)[0]) > 1e-3
    assert abs(M.compute_FSIM(x, y, pred, k=4.0)[0] - M.compute_FSIM(x, y, pred)[0]) > 1e-4


def test_edge_values(hip_lib, bounds):
    from mtd_gan_amd import metrics as M
    for size in ((16, 16), (64, 32), (512, 512)):
        z = torch.zeros(2, 1, *size, device="cuda")
        out, parts = M.fsim_each(z, z, z.clone(), parts=True)
        assert out.tolist() == [[1.0, 1.0]] * 3, out                  # piq: pc = eps / eps, GM = PC = 1
        n = float(math.prod(M.fsim_pooled_size(*size)[1:]))
        assert parts.tolist() == [[[n, n, n, 0.0] + [0.0] * 4] * 2] * 3
    x = reference(5)[0][0].cuda()
    same = M.fsim_each(x, x, x.clone()).tolist()
    assert all(abs(v - 1.0) <= bounds["score"] for row in same for v in row), same
    # a constant image: rounding noise over rounding noise, in piq too -- finite, nothing more is pinned
    flat = torch.full_like(x, 0.5)
    assert torch.isfinite(M.fsim_each(flat, flat, flat.clone())).all()
    v = M.fsim_each(flat, x, x)
    assert torch.isfinite(v).all() and all(abs(s - 1.0) <= bounds["score"] for s in v[1].tolist())


def test_refusals(hip_lib):
    from mtd_gan_amd import metrics as M
    x = torch.zeros(1, 1, 64, 64, device="cuda")
    with pytest.raises(RuntimeError, match="CUDA"):
        M.fsim_each(x.cpu(), x, x)
    with pytest.raises(RuntimeError, match="CUDA"):
        M.compute_FSIM(x, x, x.cpu())
    with pytest.raises(NotImplementedError):
        M.compute_FSIM(x, x, x, data_range=255)
    for bad, name in ((x[:, :, :48, :], "48x64"), (x[:, :, :, :15], "64x15"), (torch.zeros(1, 1, 520, 512, device="cuda"), "260x256")):
        with pytest.raises(ValueError, match=name):
            M.fsim_each(bad, bad, bad)
    ok = x[:, :, :16, :32]
    assert tuple(M.fsim_each(ok, ok, ok).shape) == (3, 1)
    for kw in (dict(scales=0), dict(scales=5), dict(orientations=9), dict(sigma_f=1.0), dict(delta_theta=-1.2)):
        with pytest.raises(ValueError, match="fsim"):
            M.fsim_each(x, x, x, **kw)


# -------------------------------------------------------------------------------------------------------------- engine
PIXEL_KEYS = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in WHO]
IQA_KEYS = [f"{who}_gmsd" for who in WHO]          # (64 x 64 slices: GMSD is the one test_iqa metric small enough)
HAARPSI_KEYS = [f"{who}_haarpsi" for who in WHO]
FSIM_KEYS = [f"{who}_fsim" for who in WHO]


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


def test_engine_with_test_fsim(hip_lib, tmp_path, slices):
    from mtd_gan_amd import engine, metrics as M
    x, y = slices
    by_two, by_one = _loader(x, y, 2), _loader(x, y, 1)
    m = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_per_slice=True)

    # the attribute absent, None, False: the dict and the CSV bytes of the loop as it was
    plain, plain_csv = _run(m, by_two, tmp_path, "plain")
    assert list(plain.keys()) == PIXEL_KEYS
    assert plain_csv.splitlines()[0] == b",PATH,RMSE,PSNR,SSIM"
    for off in (None, False):
        m.test_fsim = off
        assert _run(m, by_two, tmp_path, f"off_{off!r}") == (plain, plain_csv)

    # per slice: keys after the others, one column after SSIM, the values of fsim_each on the loop's own clipped prediction
    m.test_fsim = True
    res, csv = _run(m, by_two, tmp_path, "each")
    assert list(res.keys()) == PIXEL_KEYS + FSIM_KEYS and {k: res[k] for k in PIXEL_KEYS} == plain
    lines = csv.decode().splitlines()
    assert lines[0] == ",PATH,RMSE,PSNR,SSIM,FSIM" and len(lines) == 5
    assert [ln.split(",")[:5] for ln in lines] == [ln.split(",") for ln in plain_csv.decode().splitlines()]
    xd, yd = x.cuda(), y.cuda()
    clipped = (1.05 * xd - 0.02).clamp(0, 1)
    vals = M.fsim_each(xd, yd, clipped).tolist()
    meters = {}
    for i in range(4):
        assert lines[1 + i].split(",")[5:] == [str(vals[2][i])]
        for k, who in enumerate(WHO):
            meters.setdefault(f"{who}_fsim", engine._Meter()).update(vals[k][i], 1)
    assert {k: res[k] for k in FSIM_KEYS} == {k: round(mm.global_avg, 7) for k, mm in meters.items()}
    assert res["gt_fsim"] == 1.0 and 0.0 < res["input_fsim"] < 1.0 and 0.0 < res["pred_fsim"] < 1.0

    # beside test_iqa and test_haarpsi: behind their keys and columns, which stay what they are without test_fsim
    m.test_iqa = ("gmsd",)
    m.test_haarpsi = True
    all_, all_csv = _run(m, by_two, tmp_path, "all")
    del m.test_fsim
    others, others_csv = _run(m, by_two, tmp_path, "others")
    assert list(others.keys()) == PIXEL_KEYS + IQA_KEYS + HAARPSI_KEYS and list(all_.keys()) == PIXEL_KEYS + IQA_KEYS + HAARPSI_KEYS + FSIM_KEYS
    assert {k: all_[k] for k in others} == others and {k: all_[k] for k in FSIM_KEYS} == {k: res[k] for k in FSIM_KEYS}
    all_lines = all_csv.decode().splitlines()
    assert all_lines[0] == ",PATH,RMSE,PSNR,SSIM,GMSD,HaarPSI,FSIM"
    assert [ln.split(",")[:7] for ln in all_lines] == [ln.split(",") for ln in others_csv.decode().splitlines()]
    assert [ln.split(",")[7:] for ln in all_lines[1:]] == [ln.split(",")[5:] for ln in lines[1:]]
    del m.test_iqa, m.test_haarpsi

    # the default path on batches of one: the same keys, columns and -- the generator is pointwise -- the same values
    m.test_fsim = True
    del m.test_per_slice
    ones, ones_csv = _run(m, by_one, tmp_path, "ones")
    assert list(ones.keys()) == list(res.keys())
    assert [ln.split(",")[5:] for ln in ones_csv.decode().splitlines()] == [ln.split(",")[5:] for ln in lines]
    assert all(ones[k] == res[k] for k in FSIM_KEYS)
    # ... and a batch of two as ONE sample: the mean over its slices
    twos, twos_csv = _run(m, by_two, tmp_path, "twos")
    assert list(twos.keys()) == list(res.keys())
    for j, ln in enumerate(twos_csv.decode().splitlines()[1:]):
        mean = (vals[2][2 * j] + vals[2][2 * j + 1]) / 2
        assert abs(float(ln.split(",")[5]) - mean) <= 4e-16 * abs(mean)

    # the dict form reaches the kernels
    m.test_per_slice = True
    m.test_fsim = dict(R.OTHER)
    other, other_csv = _run(m, by_two, tmp_path, "dict")
    want = M.fsim_each(xd, yd, clipped, **R.OTHER).tolist()
    assert [ln.split(",")[5] for ln in other_csv.decode().splitlines()[1:]] == [str(v) for v in want[2]]
    assert list(other.keys()) == list(res.keys()) and other["pred_fsim"] != res["pred_fsim"]


def test_engine_composes_with_stored_input_and_png(hip_lib, tmp_path):
    """test_fsim beside test_iqa, test_haarpsi, test_from_stored and test_save_png under test_per_slice: the values are those of
    the windowed floats the loop itself computes, and the PNGs are written as without it."""
    import os
    from mtd_gan_amd import dicom_io, engine, metrics as M
    g = torch.Generator().manual_seed(5)
    words = [torch.randint(800, 1300, (2, 1, 64, 64), generator=g).to(torch.int16) for _ in range(2)]
    table = torch.tensor([[1.0, -1024.0], [1.0, -1024.0]])
    batch = dict(n_20=words[0], n_100=words[1], rescale_n_20=table, rescale_n_100=table)
    stand_in = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_iqa=("gmsd",), test_haarpsi=True, test_fsim=True, test_per_slice=True,
                                     test_from_stored=True, test_save_png=True)
    res = engine.test_MTD_GAN_Ours(stand_in, torch.nn.L1Loss(), [batch], torch.device("cuda"), str(tmp_path))
    assert list(res.keys()) == PIXEL_KEYS + IQA_KEYS + HAARPSI_KEYS + FSIM_KEYS
    tab = dicom_io.rescale_table(table, 2, torch.device("cuda"))
    xf, yf = (dicom_io.stored_to_window(w.cuda().contiguous(), tab, dicom_io.A_MIN, dicom_io.A_MAX) for w in words)
    vals = M.fsim_each(xf, yf, (1.05 * xf - 0.02).clamp(0, 1)).tolist()
    lines = open(tmp_path / "pred_results.csv").read().splitlines()
    assert lines[0] == ",PATH,RMSE,PSNR,SSIM,GMSD,HaarPSI,FSIM"
    for i in range(2):
        assert lines[1 + i].split(",")[7:] == [str(vals[2][i])]
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".png")]) == 6


def test_a_per_slice_batch_is_read_once(hip_lib, slices, monkeypatch):
    """Under test_per_slice the 3 B FSIM values join the batch's single host read: with the option (and test_iqa and test_haarpsi
    beside it) one device tensor per batch crosses to the host, as without."""
    from mtd_gan_amd import engine, metrics as M
    x, y = slices
    M.fsim_each(x.cuda(), y.cuda(), x.cuda())          # (the filter table of this size is uploaded before the reads are counted)
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
    m.test_fsim = True
    engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, torch.device("cuda"), None)
    assert reads == [("tolist", (10 * 4,))], reads
    del reads[:]
    m.test_iqa = ("gmsd",)
    m.test_haarpsi = True
    res = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, torch.device("cuda"), None)
    assert reads == [("tolist", (16 * 4,))], reads
    assert list(res.keys()) == PIXEL_KEYS + IQA_KEYS + HAARPSI_KEYS + FSIM_KEYS
