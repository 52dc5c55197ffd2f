"""MS-SSIM, VIFp and GMSD on the device (csrc/iqa.hip) against the float64 restatement of tests/_iqa_ref.py, which
tests/test_iqa_cpu.py holds to the reference's own float64 values.

Bounds.  Per metric, 4 x the largest relative distance between the reference's OWN float32 and float64 values over all cases
of tests/golden/iqa_piq.npz -- its scores for the scores, its stage values for the stage values -- computed here from the
fixture.  The factor 4 covers what the kernels do and torch's float32 path does not: separable passes, fma, tile-order double
sums.  Measured figures: DESIGN 3.14."""
import types

import numpy as np
import pytest
import torch

import _iqa_ref as R
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bounds():
    """{metric: (score bound, stage bound)} from the fixture."""
    g = np.load(R.GOLDEN)
    spread = {m: [0.0, 0.0] for m in R.METRICS}
    for index, (metrics, B, H, W) in enumerate(R.CASES):
        for m in metrics:
            for j, what in enumerate(("score", "parts")):
                v32, v64 = g[f"{m}_{index}_{what}32"].astype(np.float64), g[f"{m}_{index}_{what}64"]
                nz = v64 != 0
                spread[m][j] = max(spread[m][j], float(np.max(np.abs(v32[nz] - v64[nz]) / np.abs(v64[nz]))))
    out = {m: (4 * s[0], 4 * s[1]) for m, s in spread.items()}
    print("bounds (score, stage):", out)
    return out


_reference = {}


def reference(index):
    """Case `index`: the inputs and, per source, the restatement's float64 scores and (B, 20) stage values.  Computed once,
    shared, never modified."""
    if index not in _reference:
        x, y, pred = R.case_inputs(index)
        _reference[index] = ((x, y, pred), [R.all_parts(src, y, R.CASES[index][0]) for src in (x, y, pred)])
    return _reference[index]


def _close(got, want, bound, what):
    if want == 0.0:
        assert got == 0.0, (what, got)
        return 0.0
    e = abs(got - want) / abs(want)
    assert e <= bound, f"{what}: hip {got!r} float64 {want!r} relative distance {e:.3e} > {bound:.3e}"
    return e


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_stages_then_scores_against_float64(hip_lib, bounds, index):
    from mtd_gan_amd import metrics as M
    metrics, B, H, W = R.CASES[index]
    (x, y, pred), ref = reference(index)
    out, parts = M.iqa_metrics_each(x.cuda(), y.cuda(), pred.cuda(), which=metrics, parts=True)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (len(metrics), 3, B)
    assert parts.dtype == torch.float64 and tuple(parts.shape) == (3, B, 20)
    out, parts = out.tolist(), parts.tolist()
    worst = {m: [0.0, 0.0] for m in metrics}
    for r, m in enumerate(metrics):
        sl = R.PART_SLICES[m]
        for k, who in enumerate(("input", "gt", "pred")):
            scores, want_parts = ref[k]
            for i in range(B):
                for j in range(sl.start, sl.stop):
                    e = _close(parts[k][i][j], float(want_parts[i, j]), bounds[m][1], f"case {index} {who} image {i} {R.STAGE_NAMES[j]}")
                    worst[m][1] = max(worst[m][1], e)
                e = _close(out[r][k][i], float(scores[m][i]), bounds[m][0], f"case {index} {who} image {i} {m} score")
                worst[m][0] = max(worst[m][0], e)
        if m != "gmsd":
            assert all(out[r][1][i] > 0.999 for i in range(B))              # the target against itself
        else:
            assert all(out[r][1][i] == 0.0 for i in range(B))
    for j in range(20):                                                    # metrics not asked for leave their stage values alone
        if not any(R.PART_SLICES[m].start <= j < R.PART_SLICES[m].stop for m in metrics):
            assert all(parts[k][i][j] == 0.0 for k in range(3) for i in range(B)), j
    print(f"case {index} {B}x{H}x{W}: largest relative distance (score, stage) {worst}")


@pytest.mark.parametrize("index", [0, 4, 7])
def test_an_image_does_not_depend_on_its_batch_or_slot(hip_lib, index):
    from mtd_gan_amd import metrics as M
    metrics, B, H, W = R.CASES[index]
    assert B >= 2
    x, y, pred = (t.cuda() for t in reference(index)[0])
    out, parts = M.iqa_metrics_each(x, y, pred, which=metrics, parts=True)
    for i in range(B):
        one, one_parts = M.iqa_metrics_each(x[i:i + 1], y[i:i + 1], pred[i:i + 1], which=metrics, parts=True)
        assert torch.equal(out[:, :, i], one[:, :, 0]), (i, out[:, :, i], one[:, :, 0])
        assert torch.equal(parts[:, i], one_parts[:, 0]), i
    swapped, swapped_parts = M.iqa_metrics_each(pred, y, x, which=metrics, parts=True)
    assert torch.equal(swapped[:, [2, 1, 0]], out) and torch.equal(swapped_parts[[2, 1, 0]], parts)
    assert torch.equal(M.iqa_metrics_each(x, y, pred, which=metrics), out)                      # parts=False: the same scores


def test_the_three_together_equal_each_alone(hip_lib):
    """One call with the three metrics (the 512 x 512 case) gives the rows of three calls with one metric each, in the fixed
    order whatever the order of `which`; per_slice and compute_* are those values on the host."""
    from mtd_gan_amd import metrics as M
    x, y, pred = (t.cuda() for t in reference(len(R.CASES) - 1)[0])
    out = M.iqa_metrics_each(x, y, pred)
    assert tuple(out.shape) == (3, 3, 1)
    assert torch.equal(M.iqa_metrics_each(x, y, pred, which=("gmsd", "vif", "ms_ssim")), out)
    for r, m in enumerate(R.METRICS):
        assert torch.equal(M.iqa_metrics_each(x, y, pred, which=(m,))[0], out[r]), m
    per = M.iqa_metrics_per_slice(x, y, pred)
    assert list(per) == list(R.METRICS)
    for r, m in enumerate(R.METRICS):
        assert per[m] == [tuple(out[r, :, 0].tolist())]


def test_compute_functions_are_the_batch_means(hip_lib):
    from mtd_gan_amd import metrics as M
    for index, fn in ((0, M.compute_MS_SSIM), (4, M.compute_VIF), (7, M.compute_GMSD)):
        (m,), B, H, W = R.CASES[index]
        x, y, pred = (t.cuda() for t in reference(index)[0])
        each = M.iqa_metrics_each(x, y, pred, which=(m,))[0].tolist()               # (3, B)
        got = fn(x, y, pred)
        assert isinstance(got, tuple) and len(got) == 3 and all(isinstance(v, float) for v in got)
        for k in range(3):
            mean = sum(each[k]) / B
            assert abs(got[k] - mean) <= 4e-16 * abs(mean), (m, k, got[k], mean)      # B <= 3 doubles summed in another order
    # VIFp's sigma_n_sq is a parameter, on the [0, 1] scale as given
    x, y, pred = (t.cuda() for t in reference(4)[0])
    other = M.compute_VIF(x, y, pred, sigma_n_sq=2.0 / 255 ** 2)
    want, _ = R.vif(pred.cpu().double(), y.cpu().double(), sigma_n_sq=2.0 / 255 ** 2)
    # (no bound of the fixture applies to this sigma_n_sq: the check is that the parameter arrives, 1e-3 against a change of > 1e-2)
    assert abs(other[2] - float(want.mean())) <= 1e-3 * float(want.mean()) and abs(other[2] - M.compute_VIF(x, y, pred)[2]) > 1e-2


def test_refusals(hip_lib):
    from mtd_gan_amd import metrics as M
    x = torch.zeros(1, 1, 176, 176, device="cuda")
    with pytest.raises(RuntimeError):
        M.iqa_metrics_each(x.cpu(), x, x)
    with pytest.raises(RuntimeError):
        M.compute_GMSD(x, x, x.cpu())
    for fn in (M.compute_MS_SSIM, M.compute_VIF, M.compute_GMSD):
        with pytest.raises(NotImplementedError):
            fn(x, x, x, data_range=255)
    for which, lo in (("ms_ssim", 161), ("vif", 41), ("gmsd", 2)):
        for small in (x[:, :, :lo - 1, :], x[:, :, :, :lo - 1]):
            with pytest.raises(ValueError, match=f"{lo}x{lo}"):
                M.iqa_metrics_each(small, small, small, which=(which,))
        ok = x[:, :, :lo, :lo + 1]
        assert tuple(M.iqa_metrics_each(ok, ok, ok, which=(which,)).shape) == (1, 3, 1)
    with pytest.raises(ValueError, match="161x161"):
        M.compute_MS_SSIM(x[:, :, :160], x[:, :, :160], x[:, :, :160])
    with pytest.raises(ValueError):
        M.compute_VIF(x, x, x, sigma_n_sq=0.0)


# -------------------------------------------------------------------------------------------------------------- engine
PIXEL_KEYS = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in ("input", "gt", "pred")]
IQA_KEYS = [f"{who}_{name}" for name in R.METRICS for who in ("input", "gt", "pred")]


def _model():
    """Seeded as tests/test_per_slice_metrics_gpu.py's; slices of 176 x 176 take the any-size path."""
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    torch.manual_seed(3)
    m = MTD_GAN_Method().cuda()
    m.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    m.Generator.allow_any_size = True
    return m


class _Pointwise(torch.nn.Module):
    """A stand-in generator whose output for a slice has the same bits in any batch (the real one may choose another
    convolution plan for another batch size, tests/test_per_slice_metrics_gpu.py::test_engine_per_slice)."""

    def forward(self, x):
        return 1.05 * x - 0.02


def _loader(x, y, per_batch):
    n = x.shape[0]
    names = [f"L000_{i:04d}.dcm" for i in range(n)]
    return [dict(n_20=x[i:i + per_batch], n_100=y[i:i + per_batch], path_n_20=names[i:i + per_batch], path_n_100=names[i:i + per_batch])
            for i in range(0, n, per_batch)], names


def _run(model, loader, tmp_path, tag):
    from mtd_gan_amd import engine
    d = tmp_path / tag
    res = engine.test_MTD_GAN_Ours(model, torch.nn.L1Loss(), loader, torch.device("cuda"), str(d))
    return res, open(d / "pred_results.csv", "rb").read()


def test_engine_with_test_iqa(hip_lib, tmp_path):
    from mtd_gan_amd import engine, kernels as K, metrics as M
    x, y = orc.synthetic_ldct(4, seed=9, size=176)
    by_two, names = _loader(x, y, 2)
    by_one, _ = _loader(x, y, 1)
    m = _model()

    # the attribute absent, None, False: the dict and the CSV bytes of the loop as it was
    m.test_per_slice = True
    plain, plain_csv = _run(m, by_two, tmp_path, "plain")
    assert list(plain.keys()) == PIXEL_KEYS and not any(k.endswith("_vif") for k in plain)
    assert plain_csv.splitlines()[0] == b",PATH,RMSE,PSNR,SSIM"
    for off in (None, False, ()):
        m.test_iqa = off
        assert _run(m, by_two, tmp_path, f"off_{off!r}") == (plain, plain_csv)

    # per slice, all three: keys after the others, three columns after SSIM, the values of iqa_metrics_each on the loop's own
    # clipped prediction
    m.test_iqa = True
    res, csv = _run(m, by_two, tmp_path, "each")
    assert list(res.keys()) == PIXEL_KEYS + IQA_KEYS and {k: res[k] for k in PIXEL_KEYS} == plain
    lines = csv.decode().splitlines()
    assert lines[0] == ",PATH,RMSE,PSNR,SSIM,MS_SSIM,VIF,GMSD" and len(lines) == 5
    assert [ln.split(",")[:5] for ln in lines] == [ln.split(",") for ln in plain_csv.decode().splitlines()]
    meters = {}
    for j, b in enumerate(by_two):
        xb, yb = b["n_20"].cuda(), b["n_100"].cuda()
        with torch.no_grad():
            clipped = K.clip01(m.Generator(xb).contiguous())
        vals = M.iqa_metrics_each(xb, yb, clipped).tolist()
        for i in range(2):
            assert lines[1 + 2 * j + i].split(",")[5:] == [str(vals[r][2][i]) for r in range(3)]
            for r, name in enumerate(R.METRICS):
                for k, who in enumerate(("input", "gt", "pred")):
                    meters.setdefault(f"{who}_{name}", engine._Meter()).update(vals[r][k][i], 1)
    assert {k: res[k] for k in IQA_KEYS} == {k: round(mm.global_avg, 7) for k, mm in meters.items()}
    assert res["gt_ms_ssim"] == 1.0 and res["gt_gmsd"] == 0.0 and 0.5 < res["pred_vif"] < 1.5 and res["pred_gmsd"] > 0.0

    # a subset, in the fixed order whatever the tuple's
    m.test_iqa = ("gmsd", "ms_ssim")
    sub, sub_csv = _run(m, by_two, tmp_path, "subset")
    assert list(sub.keys()) == PIXEL_KEYS + [k for k in IQA_KEYS if not k.endswith("_vif")]
    assert all(sub[k] == res[k] for k in sub)
    sub_lines = sub_csv.decode().splitlines()
    assert sub_lines[0] == ",PATH,RMSE,PSNR,SSIM,MS_SSIM,GMSD"
    assert [ln.split(",")[5:] for ln in sub_lines[1:]] == [[ln.split(",")[5], ln.split(",")[7]] for ln in lines[1:]]

    # the default path on batches of one: the same keys and columns
    m.test_iqa = True
    del m.test_per_slice
    ones, ones_csv = _run(m, by_one, tmp_path, "ones")
    assert list(ones.keys()) == list(res.keys())
    assert ones_csv.decode().splitlines()[0] == lines[0] and len(ones_csv.decode().splitlines()) == 5
    for k in IQA_KEYS:
        print(f"{k}: batches of 2 per slice {res[k]!r}, batches of 1 {ones[k]!r}")

    # ... and the same per-slice values, on a generator whose output for a slice does not depend on the batch: the IQA
    # cells of the two CSVs and the IQA keys are equal
    stand_in = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_iqa=True, test_per_slice=True)
    each_res, each_csv = _run(stand_in, by_two, tmp_path, "stand_in_each")
    del stand_in.test_per_slice
    one_res, one_csv = _run(stand_in, by_one, tmp_path, "stand_in_ones")
    assert list(each_res.keys()) == list(one_res.keys()) == PIXEL_KEYS + IQA_KEYS
    a, b = each_csv.decode().splitlines(), one_csv.decode().splitlines()
    assert a[0] == b[0] == lines[0]
    assert [ln.split(",")[5:] for ln in a[1:]] == [ln.split(",")[5:] for ln in b[1:]]
    assert all(each_res[k] == one_res[k] for k in IQA_KEYS)
    # the default path takes a batch as ONE sample: the mean over its slices
    two_res, two_csv = _run(stand_in, by_two, tmp_path, "stand_in_batches")
    rows = [[float(v) for v in ln.split(",")[5:]] for ln in a[1:]]
    for j, ln in enumerate(two_csv.decode().splitlines()[1:]):
        for r in range(3):
            mean = (rows[2 * j][r] + rows[2 * j + 1][r]) / 2
            assert abs(float(ln.split(",")[5 + r]) - mean) <= 4e-16 * abs(mean)


def test_engine_composes_with_stored_input_and_png(hip_lib, tmp_path):
    """test_iqa beside test_from_stored and test_save_png under test_per_slice: the IQA values are those of the windowed
    floats the loop itself computes, and the PNGs are written as without it."""
    import os
    from mtd_gan_amd import dicom_io, engine, metrics as M
    g = torch.Generator().manual_seed(5)
    words = [torch.randint(800, 1300, (2, 1, 64, 64), generator=g).to(torch.int16) for _ in range(2)]
    table = torch.tensor([[1.0, -1024.0], [1.0, -1024.0]])
    batch = dict(n_20=words[0], n_100=words[1], rescale_n_20=table, rescale_n_100=table)
    stand_in = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_iqa=("vif", "gmsd"), test_per_slice=True, test_from_stored=True,
                                     test_save_png=True)
    res = engine.test_MTD_GAN_Ours(stand_in, torch.nn.L1Loss(), [batch], torch.device("cuda"), str(tmp_path))
    assert list(res.keys()) == PIXEL_KEYS + [k for k in IQA_KEYS if "ms_ssim" not in k]
    tab = dicom_io.rescale_table(table, 2, torch.device("cuda"))
    xf, yf = (dicom_io.stored_to_window(w.cuda().contiguous(), tab, dicom_io.A_MIN, dicom_io.A_MAX) for w in words)
    vals = M.iqa_metrics_each(xf, yf, (1.05 * xf - 0.02).clamp(0, 1), which=("vif", "gmsd")).tolist()
    lines = open(tmp_path / "pred_results.csv").read().splitlines()
    assert lines[0] == ",PATH,RMSE,PSNR,SSIM,VIF,GMSD"
    for i in range(2):
        assert lines[1 + i].split(",")[5:] == [str(vals[0][2][i]), str(vals[1][2][i])]
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".png")]) == 6


def test_engine_composes_with_the_feature_network(hip_lib, tmp_path):
    """test_iqa beside perceptual_vgg under test_per_slice (B = 2 at 256 x 256): the IQA block sits behind the six perceptual
    rows in the batch's one host read; every other key and CSV cell is what the loop gives without test_iqa."""
    import _perceptual_ref as RP
    from mtd_gan_amd import metrics as M
    x, y = orc.synthetic_ldct(2, seed=9, size=256)
    loader, names = _loader(x, y, 2)
    model = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_per_slice=True, perceptual_vgg=M.VGG19Features(RP.seeded_state_dict(0)))
    plain, plain_csv = _run(model, loader, tmp_path, "vgg")
    model.test_iqa = True
    res, csv = _run(model, loader, tmp_path, "vgg_iqa")
    assert list(res.keys()) == list(plain.keys()) + IQA_KEYS and {k: res[k] for k in plain} == plain
    lines, plain_lines = csv.decode().splitlines(), plain_csv.decode().splitlines()
    assert lines[0] == ",PATH,PL,TML,RMSE,PSNR,SSIM,MS_SSIM,VIF,GMSD" and plain_lines[0] == ",PATH,PL,TML,RMSE,PSNR,SSIM"
    assert [ln.split(",")[:7] for ln in lines] == [ln.split(",") for ln in plain_lines]
    xd, yd = x.cuda(), y.cuda()
    vals = M.iqa_metrics_each(xd, yd, (1.05 * xd - 0.02).clamp(0, 1)).tolist()
    for i in range(2):
        assert lines[1 + i].split(",")[7:] == [str(vals[r][2][i]) for r in range(3)]
    for r, name in enumerate(R.METRICS):
        for k, who in enumerate(("input", "gt", "pred")):
            assert res[f"{who}_{name}"] == round((vals[r][k][0] + vals[r][k][1]) / 2, 7)
