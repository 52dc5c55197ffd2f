"""A loader batch of B slices as B samples: the per-image forms of the test loop's reductions against the
one-image calls they must reproduce bit for bit (mtd_image_metrics_each, mtd_patch_gram_l1_each, one loss term per image and
level), the per-slice PL / TML against the float64 restatement of each slice alone, and engine.test_MTD_GAN_Ours under
`model.test_per_slice`.  Bounds where a bound applies are the project's: PSNR 0.01 dB, SSIM 2e-5, RMSE 1e-6, L1 1e-5, PL 1e-3
relative, TML max(1e-3, 4 e32) relative (tests/test_inference_gpu.py, tests/test_perceptual_gpu.py)."""
import ctypes

import pytest
import torch

import _inception_ref as RI
import _perceptual_ref as R
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu
EINVAL, EALIGN = -1, -2
SENTINEL = -7.0


# --------------------------------------------------------------------------------------------------------- pixel sums
def _pixel_case(shape):
    """Data as tests/test_inference_gpu.py::test_pixel_metrics_match_oracle, un-clipped prediction; on the device each set is
    the front of a buffer with a NaN guard image behind it."""
    g = torch.Generator().manual_seed(11)
    y = torch.rand(shape, generator=g)
    x = (y + 0.1 * torch.randn(shape, generator=g)).clip(0, 1)
    p = y + 0.03 * torch.randn(shape, generator=g)
    bufs = []
    for t in (x, y, p):
        buf = torch.cat([t, torch.full((1,) + tuple(shape[1:]), float("nan"))]).cuda()
        bufs.append(buf)
    return (x, y, p), bufs


@pytest.mark.parametrize("shape", [(3, 1, 64, 64), (3, 1, 100, 77), (2, 1, 520, 530)])      # 4, 12 and 289 tiles per image
def test_pixel_sums_bit_for_bit(hip_lib, shape):
    from mtd_gan_amd import kernels as K, metrics as M
    B, _, H, W = shape
    (x, y, p), bufs = _pixel_case(shape)
    xd, yd, pd = (b[:B] for b in bufs)
    each = M.pixel_metrics_each(xd, yd, pd, clip_pred=True)
    assert each.is_cuda and each.dtype == torch.float64 and tuple(each.shape) == (3, B, 2)
    rows = each.tolist()
    for k, (a, clip) in enumerate(((xd, False), (yd, False), (pd, True))):
        for i in range(B):
            sse, ssum, n = M._pair_sums(a[i:i + 1], yd[i:i + 1], clip_a=clip)
            assert n == H * W and rows[k][i] == [sse, ssum], (k, i, rows[k][i], sse, ssum)
    # the public per-slice triples: those of a one-slice pixel_metrics call, and the oracle's within the project's bounds
    pc = p.clip(0, 1)
    pcd = pc.cuda()
    per = M.pixel_metrics_per_slice(xd, yd, pcd)
    assert sorted(per) == ["psnr", "rmse", "ssim"] and all(len(v) == B for v in per.values())
    for i in range(B):
        one = M.pixel_metrics(xd[i:i + 1], yd[i:i + 1], pcd[i:i + 1])
        for name in ("rmse", "psnr", "ssim"):
            assert per[name][i] == one[name], (name, i)
        for k, a in enumerate((x, y, pc)):
            assert abs(per["psnr"][i][k] - orc.psnr(a[i:i + 1], y[i:i + 1]).item()) < 0.01
            assert abs(per["ssim"][i][k] - orc.ssim(a[i:i + 1], y[i:i + 1]).item()) < 2e-5
            assert abs(per["rmse"][i][k] - orc.rmse(a[i:i + 1], y[i:i + 1]).item()) < 1e-6
    # the entry point itself with one and two sources, into the front of a sentinel-filled buffer
    for srcs, clips, want in (((pd,), (1,), rows[2:3]), ((xd, yd), (0, 0), rows[0:2])):
        na = len(srcs)
        big = torch.full((na * B * 2 + 64,), SENTINEL, dtype=torch.float64, device="cuda")
        ws = K.workspace(hip_lib.mtd_image_metrics_each_ws_bytes(na, B, H, W), big.device)
        ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in srcs])
        flags = (ctypes.c_int * 3)(*clips)
        assert hip_lib.mtd_image_metrics_each(ptrs, na, yd.data_ptr(), B, H, W, flags, big.data_ptr(), ws.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert big[:na * B * 2].reshape(na, B, 2).tolist() == want
        assert (big[na * B * 2:] == SENTINEL).all()
    for b in bufs:
        assert torch.isnan(b[B]).all()


def test_pixel_sums_refusals(hip_lib):
    from mtd_gan_amd import kernels as K
    a = torch.zeros(1, 1, 32, 32, device="cuda")
    out = torch.zeros(64, dtype=torch.float64, device="cuda")
    ws = K.workspace(4096, a.device)
    ptrs = (ctypes.c_void_p * 3)(a.data_ptr(), a.data_ptr(), a.data_ptr())
    hole = (ctypes.c_void_p * 3)(a.data_ptr(), None, a.data_ptr())
    flags = (ctypes.c_int * 3)(0, 0, 0)
    f = hip_lib.mtd_image_metrics_each
    assert hip_lib.mtd_image_metrics_each_ws_bytes(3, 2, 100, 77) == 3 * 2 * 12 * 2 * 8
    assert hip_lib.mtd_image_metrics_each_ws_bytes(0, 1, 32, 32) == 0 and hip_lib.mtd_image_metrics_each_ws_bytes(4, 1, 32, 32) == 0
    assert hip_lib.mtd_image_metrics_each_ws_bytes(1, 0, 32, 32) == 0
    for na, B, H, W in ((0, 1, 32, 32), (4, 1, 32, 32), (1, 0, 32, 32), (1, 1, 0, 32), (1, 1, 32, -1), (3, 21846, 32, 32), (1, 65536, 32, 32)):
        assert f(ptrs, na, a.data_ptr(), B, H, W, flags, out.data_ptr(), ws.data_ptr(), None) == EINVAL, (na, B, H, W)
    assert f(None, 1, a.data_ptr(), 1, 32, 32, flags, out.data_ptr(), ws.data_ptr(), None) == EINVAL
    assert f(hole, 2, a.data_ptr(), 1, 32, 32, flags, out.data_ptr(), ws.data_ptr(), None) == EINVAL
    assert f(ptrs, 1, None, 1, 32, 32, flags, out.data_ptr(), ws.data_ptr(), None) == EINVAL
    assert f(ptrs, 1, a.data_ptr(), 1, 32, 32, None, out.data_ptr(), ws.data_ptr(), None) == EINVAL
    assert f(ptrs, 1, a.data_ptr(), 1, 32, 32, flags, None, ws.data_ptr(), None) == EINVAL
    assert f(ptrs, 1, a.data_ptr(), 1, 32, 32, flags, out.data_ptr(), None, None) == EINVAL
    torch.cuda.synchronize()
    assert (out == 0).all()


# ------------------------------------------------------------------------------------------------------ Gram per image
def _relu_normal(shape, seed):
    return torch.relu(torch.randn(shape, generator=torch.Generator().manual_seed(seed)))


# 4 patches x 1 pair; 6 patches x 3 pairs with remainder rows and columns; 8 patches x 36 pairs = 288 partials per image
@pytest.mark.parametrize("shape", [(3, 32, 32, 64), (3, 40, 50, 128), (3, 32, 64, 512)])
def test_gram_per_image_bit_for_bit(hip_lib, shape):
    from mtd_gan_amd import metrics as M
    B, h, w, C = shape
    X, Y = _relu_normal(shape, 100 + C), _relu_normal(shape, 200 + C)
    for t in (X, Y):                                       # the remainder is never read
        t[:, (h // 16) * 16:] = float("nan")
        t[:, :, (w // 16) * 16:] = float("nan")
    Xd, Yd = X.cuda(), Y.cuda()
    each = M.patch_gram_l1_each(Xd, Yd)
    assert each.dtype == torch.float64 and tuple(each.shape) == (B,) and torch.isfinite(each).all() and (each > 0).all()
    for i in range(B):
        assert torch.equal(each[i:i + 1], M.patch_gram_l1(Xd[i:i + 1], Yd[i:i + 1])), i
    assert (M.patch_gram_l1_each(Xd, Xd.clone()) == 0.0).all()
    table = torch.full((5 * B + 3,), SENTINEL, dtype=torch.float64, device="cuda")
    assert M.patch_gram_l1_each(Xd, Yd, out=table, out_stride=5) is table
    written = torch.zeros(5 * B + 3, dtype=torch.bool, device="cuda")
    written[0:5 * B:5] = True
    assert torch.equal(table[written], each) and (table[~written] == SENTINEL).all()


def test_gram_per_image_refusals(hip_lib):
    from mtd_gan_amd import kernels as K, metrics as M
    x = torch.zeros(2, 16, 37, 64, device="cuda")
    out = torch.zeros(16, dtype=torch.float64, device="cuda")
    ws = K.workspace(4096, x.device)
    f = hip_lib.mtd_patch_gram_l1_each
    p = x.data_ptr()
    assert f(p, p, 2, 16, 37, 64, out.data_ptr(), 0, ws.data_ptr(), None) == EINVAL               # out_stride < 1
    assert f(p, p, 2, 16, 37, 64, out.data_ptr(), -3, ws.data_ptr(), None) == EINVAL
    assert f(p, p, 2, 15, 37, 64, out.data_ptr(), 1, ws.data_ptr(), None) == EINVAL               # no patch
    assert f(p, p, 2, 16, 37, 96, out.data_ptr(), 1, ws.data_ptr(), None) == EINVAL               # channels
    assert f(p, p, 0, 16, 37, 64, out.data_ptr(), 1, ws.data_ptr(), None) == EINVAL
    assert f(None, p, 2, 16, 37, 64, out.data_ptr(), 1, ws.data_ptr(), None) == EINVAL
    assert f(p, p, 2, 16, 37, 64, None, 1, ws.data_ptr(), None) == EINVAL
    assert f(p, p, 2, 16, 37, 64, out.data_ptr(), 1, None, None) == EINVAL
    assert f(p + 4, p, 1, 16, 37, 64, out.data_ptr(), 1, ws.data_ptr(), None) == EALIGN
    torch.cuda.synchronize()
    assert (out == 0).all()
    with pytest.raises(ValueError):
        M.patch_gram_l1_each(x, x, out_stride=0)
    with pytest.raises(ValueError):
        M.patch_gram_l1_each(x, x, out=out[:2], out_stride=5)                                      # too short for two images


# ------------------------------------------------------------------------------------------------- PL / TML per slice
@pytest.fixture(scope="module")
def state():
    return R.seeded_state_dict(0)


@pytest.fixture(scope="module")
def vgg(hip_lib, state):
    from mtd_gan_amd.metrics import VGG19Features
    return VGG19Features(state)


@pytest.fixture(scope="module")
def pair_256x272(state):
    """(input, target, pred) at B = 2, 256 x 272 (tests/test_perceptual_gpu.py's triple_256x272 and a second seed) and, per
    slice, the restatement's PL / TML of input and pred against the target of THAT slice alone, in float64 and in float32.
    Computed once, shared, never modified."""
    xs, ys = zip(*(orc.synthetic_ldct(1, seed=s, size=272) for s in (33, 34)))
    x, y = torch.cat(xs)[:, :, :256].contiguous(), torch.cat(ys)[:, :, :256].contiguous()
    pred = (0.5 * (x + y)).contiguous()
    out = {}
    for dtype in (torch.float64, torch.float32):
        ft = R.features(state, y, dtype)
        fo = [R.features(state, t, dtype) for t in (x, pred)]
        sl = lambda maps, i: [m[i:i + 1] for m in maps]                                            # noqa: E731
        out[dtype] = [dict(pl=[R.pl(sl(f, i), sl(ft, i)).item() for f in fo], tml=[R.tml(sl(f, i), sl(ft, i)).item() for f in fo])
                      for i in range(2)]
    return (x, y, pred), out


def _check_against_restatement(six, ref, i, tag):
    """Column i of a (6, B) list of rows against slice i's float64 values at the bounds of test_compute_pl / test_compute_tml."""
    r64, r32 = ref[torch.float64][i], ref[torch.float32][i]
    assert six[1][i] == 0.0 and six[4][i] == 0.0
    for row, k in ((0, 0), (2, 1)):
        got, want = six[row][i], r64["pl"][k]
        print(f"{tag} slice {i} PL entry {row}: float64 {want:.9e} hip {got:.9e} rel {abs(got - want) / abs(want):.3e}")
        assert abs(got - want) <= 1e-3 * abs(want)
        got, want = six[3 + row][i], r64["tml"][k]
        e32 = abs(r32["tml"][k] - want) / abs(want)
        e = abs(got - want) / abs(want)
        print(f"{tag} slice {i} TML entry {row}: float64 {want:.9e} hip {got:.9e}; e32 = {e32:.3e}, hip error = {e:.3e}")
        assert e <= max(1e-3, 4 * e32)


def test_perceptual_per_slice(hip_lib, vgg, pair_256x272):
    from mtd_gan_amd import metrics as M
    (x, y, pred), ref = pair_256x272
    xd, yd, pd = x.cuda(), y.cuda(), pred.cuda()
    got = M.perceptual_metrics_per_slice(xd, yd, pd, vgg)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (6, 2)
    six = got.tolist()
    for i in range(2):
        _check_against_restatement(six, ref, i, "per-slice")
    # the network taken out: on the maps of ONE vgg(...) call, the per-image reductions give the bits of the one-image
    # reductions on slice i of the same maps
    levels = M._stacked_features(vgg, yd, (xd, pd))
    pl, tml = M._pl_each(levels), M._tml_each(levels)
    assert tuple(pl.shape) == (2, 2) and tuple(tml.shape) == (3, 2) and (tml[1] == 0).all()
    for i in range(2):
        one = [(ft[i:i + 1], [f[i:i + 1] for f in fo]) for ft, fo in levels]
        pl1, tml1 = M._pl_values(one, (1, 0, 2)), M._tml_values(one, (1, 0, 2))
        assert torch.equal(pl[:, i], pl1[[0, 2]]), (i, pl[:, i], pl1)
        assert torch.equal(tml[:, i], tml1), (i, tml[:, i], tml1)
    with pytest.raises(ValueError):
        M.perceptual_metrics_per_slice(xd[:, :, :128], yd[:, :, :128], pd[:, :, :128], vgg)


# -------------------------------------------------------------------------------------------------------------- engine
PIXEL_KEYS = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in ("input", "gt", "pred")]
BOUNDS = dict(psnr=0.01, ssim=2e-5, rmse=1e-6)


def _model():
    """Seeded as tests/test_inference_gpu.py::test_eval_loops_mirror_reference_surface."""
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    torch.manual_seed(3)
    m = MTD_GAN_Method().cuda()
    m.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    return m


def _loader(x, y, per_batch):
    n = x.shape[0]
    names = [f"L000_{i:04d}.dcm" for i in range(n)]
    return [dict(n_20=x[i:i + per_batch], n_100=y[i:i + per_batch], path_n_20=names[i:i + per_batch], path_n_100=names[i:i + per_batch])
            for i in range(0, n, per_batch)], names


def _means(samples):
    """Per-sample dicts -> the loop's result, through the same meter arithmetic."""
    from mtd_gan_amd.engine import _Meter
    meters = {}
    for s in samples:
        for k, v in s.items():
            meters.setdefault(k, _Meter()).update(v, 1)
    return {k: round(mm.global_avg, 7) for k, mm in meters.items()}


def _sample(l1, pm):
    s = {"L1_loss": l1}
    for name in ("rmse", "psnr", "ssim"):
        for who, v in zip(("input", "gt", "pred"), pm[name]):
            s[f"{who}_{name}"] = v
    return s


def test_engine_per_slice(hip_lib, tmp_path):
    from mtd_gan_amd import engine, kernels as K, metrics as M
    m = _model()
    x, y = orc.synthetic_ldct(6, seed=9, size=128)
    loader, names = _loader(x, y, 3)
    dev = torch.device("cuda")
    l1 = torch.nn.L1Loss()
    with torch.no_grad():
        raw = [m.Generator(b["n_20"].cuda()) for b in loader]
    clipped = [K.clip01(r.contiguous()) for r in raw]

    # default: a batch is one sample -- without the attribute and with False
    batch_samples = []
    for b, r, c in zip(loader, raw, clipped):
        xb, yb = b["n_20"].cuda(), b["n_100"].cuda()
        batch_samples.append(_sample(float(engine._l1(l1, r, yb)), M.pixel_metrics(xb, yb, c)))
    for setting in ("absent", False):
        if setting != "absent":
            m.test_per_slice = setting
        d = tmp_path / f"default_{setting}"
        res = engine.test_MTD_GAN_Ours(m, l1, loader, dev, str(d))
        assert list(res.keys()) == PIXEL_KEYS and res == _means(batch_samples)
        lines = open(d / "pred_results.csv").read().splitlines()
        assert lines[0] == ",PATH,RMSE,PSNR,SSIM" and len(lines) == 3
        for j, s in enumerate(batch_samples):
            assert lines[1 + j].split(",") == [str(j), names[3 * j], str(s["pred_rmse"]), str(s["pred_psnr"]), str(s["pred_ssim"])]

    # per slice: six rows, six samples
    m.test_per_slice = True
    res = engine.test_MTD_GAN_Ours(m, l1, loader, dev, str(tmp_path / "each"))
    lines = open(tmp_path / "each" / "pred_results.csv").read().splitlines()
    assert lines[0] == ",PATH,RMSE,PSNR,SSIM"
    assert len(lines) == 7, lines
    samples = []
    for b, r, c in zip(loader, raw, clipped):
        xb, yb = b["n_20"].cuda(), b["n_100"].cuda()
        for i in range(3):
            samples.append(_sample(float(engine._l1(l1, r[i:i + 1], yb[i:i + 1])), M.pixel_metrics(xb[i:i + 1], yb[i:i + 1], c[i:i + 1])))
    for j, s in enumerate(samples):
        assert lines[1 + j].split(",") == [str(j), names[j], str(s["pred_rmse"]), str(s["pred_psnr"]), str(s["pred_ssim"])], j
    assert list(res.keys()) == PIXEL_KEYS
    assert res == _means(samples)
    # no paths in the batch: the fallback name counts slices; a loss that is not nn.L1Loss is applied slice by slice
    bare = [dict(n_20=b["n_20"], n_100=b["n_100"]) for b in loader]
    res2 = engine.test_MTD_GAN_Ours(m, lambda p, t: (p - t).abs().mean(), bare, dev, str(tmp_path / "bare"))
    lines2 = open(tmp_path / "bare" / "pred_results.csv").read().splitlines()
    assert [ln.split(",")[1] for ln in lines2[1:]] == [f"slice_{k}" for k in range(6)]
    assert [ln.split(",")[2:] for ln in lines2[1:]] == [ln.split(",")[2:] for ln in lines[1:]]
    assert abs(res2["L1_loss"] - res["L1_loss"]) < 1e-5 and all(res2[k] == res[k] for k in PIXEL_KEYS[1:])

    # a loader of batch 1 over the same six slices on the default path
    del m.test_per_slice
    ones = engine.test_MTD_GAN_Ours(m, l1, _loader(x, y, 1)[0], dev, str(tmp_path / "ones"))
    assert list(ones.keys()) == PIXEL_KEYS
    for k in PIXEL_KEYS:
        bound = 1e-5 if k == "L1_loss" else BOUNDS[k.split("_")[1]]
        print(f"{k}: batch of 3 per slice {res[k]!r}, batches of 1 {ones[k]!r}")
        assert abs(res[k] - ones[k]) <= bound, k
    assert len(open(tmp_path / "ones" / "pred_results.csv").read().splitlines()) == 7


def test_engine_per_slice_with_the_feature_network(hip_lib, vgg, tmp_path):
    """B = 2, one batch, at 256 x 256: every value is what perceptual_metrics_per_slice (held to float64 per slice in
    test_perceptual_per_slice) gives on the loop's own clipped prediction."""
    from mtd_gan_amd import engine, kernels as K, metrics as M
    m = _model()
    m.perceptual_vgg = vgg
    m.test_per_slice = True
    x, y = orc.synthetic_ldct(2, seed=9, size=256)
    loader, names = _loader(x, y, 2)
    res = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, torch.device("cuda"), str(tmp_path))
    six_keys = [f"{who}_{name}" for name in ("pl", "tml") for who in ("input", "gt", "pred")]
    assert list(res.keys()) == ["L1_loss"] + six_keys + PIXEL_KEYS[1:]
    with torch.no_grad():
        clipped = K.clip01(m.Generator(x.cuda()).contiguous())
    six = M.perceptual_metrics_per_slice(x.cuda(), y.cuda(), clipped, vgg).tolist()
    assert {k: res[k] for k in six_keys} == _means([dict(zip(six_keys, [row[i] for row in six])) for i in range(2)])
    assert res["gt_pl"] == 0.0 and res["gt_tml"] == 0.0
    lines = open(tmp_path / "pred_results.csv").read().splitlines()
    assert lines[0] == ",PATH,PL,TML,RMSE,PSNR,SSIM" and len(lines) == 3
    for i in range(2):
        row = lines[1 + i].split(",")
        pm = M.pixel_metrics(x[i:i + 1].cuda(), y[i:i + 1].cuda(), clipped[i:i + 1])
        assert row == [str(i), names[i], str(six[2][i]), str(six[5][i]), str(pm["rmse"][2]), str(pm["psnr"][2]), str(pm["ssim"][2])]
        assert six[2][i] > 0.0 and six[5][i] > 0.0


def test_engine_per_slice_with_fid_features(hip_lib, tmp_path):
    """Set up as tests/test_inception_gpu.py::test_test_loop_with_the_network, with 2 batches of 2 slices."""
    from mtd_gan_amd import engine, kernels as K, metrics as M
    net = M.InceptionV3Features(RI.seeded_state_dict(0))
    m = _model()
    xs, ys = orc.synthetic_ldct(4, seed=9, size=64)
    loader, _ = _loader(xs, ys, 2)
    dev = torch.device("cuda")
    m.test_per_slice = True
    plain = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, None)
    assert list(plain.keys()) == PIXEL_KEYS
    m.fid_features = net
    full = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, str(tmp_path))
    assert list(full.keys()) == PIXEL_KEYS + ["input_fid", "gt_fid", "pred_fid"]
    assert all(full[k] == plain[k] for k in PIXEL_KEYS)
    assert len(open(tmp_path / "pred_results.csv").read().splitlines()) == 5
    per_batch = []
    with torch.no_grad():
        for b in loader:
            xb, yb = b["n_20"].cuda(), b["n_100"].cuda()
            per_batch.append(M.compute_feat(xb, yb, K.clip01(m.Generator(xb).contiguous()), extractor=net))
    feats = [torch.cat([pb[k].float() for pb in per_batch]) for k in range(3)]
    assert all(tuple(f.shape) == (4, 2048) for f in feats)
    triple = torch.stack(M.compute_FID(*feats)).tolist()
    print("FID of four 64 x 64 slices in two batches (input, gt, pred):", triple)
    for who, v in zip(("input", "gt", "pred"), triple):
        assert v == v and abs(v) != float("inf")
        assert full[f"{who}_fid"] == round(v, 7)


# ------------------------------------------------------------------------------ every opt-in per-slice metric at once
class _Pointwise(torch.nn.Module):
    """A stand-in generator whose output for a slice has the same bits in any batch (tests/test_iqa_gpu.py's)."""

    def forward(self, x):
        return 1.05 * x - 0.02


def _keys(*names):
    return [f"{who}_{name}" for name in names for who in ("input", "gt", "pred")]


def test_engine_with_every_per_slice_option(hip_lib, tmp_path, monkeypatch):
    """All seven opt-in metrics of the test loop together, under test_per_slice (batches of 2) and on the default path (batches
    of 1): the keys and the columns are the per-metric tests' in the loop's order, and every option's meters and CSV column are
    EQUAL to those of a run with that option alone -- the same code on the same maps, whatever stands beside it in the batch's
    one host read.  64 x 64 slices, so test_iqa holds VIFp and GMSD (MS-SSIM needs sides of 161)."""
    import types
    import _lpips_ref as RL
    from mtd_gan_amd import engine, metrics as M
    x, y = orc.synthetic_ldct(4, seed=9, size=64)
    net = M.VGG16Features(RL.seeded_state_dict())
    gen = _Pointwise().cuda()
    options = dict(test_iqa=("gmsd", "vif"), test_haarpsi=True, test_fsim=True, test_lpips=RL.seeded_lpips_weights(),
                   test_dists=RL.seeded_dists_weights(), test_vsi=True, test_mdsi=True)
    keys = dict(test_iqa=_keys("vif", "gmsd"), test_haarpsi=_keys("haarpsi"), test_fsim=_keys("fsim"), test_lpips=_keys("lpips"),
                test_dists=_keys("dists"), test_vsi=_keys("vsi"), test_mdsi=_keys("mdsi"))
    columns = dict(test_iqa=["VIF", "GMSD"], test_haarpsi=["HaarPSI"], test_fsim=["FSIM"], test_lpips=["LPIPS"], test_dists=["DISTS"],
                   test_vsi=["VSI"], test_mdsi=["MDSI"])

    def run(tag, per_slice, opts, save=True):
        m = types.SimpleNamespace(Generator=gen, perceptual_vgg16=net, test_per_slice=per_slice, **opts)
        d = tmp_path / tag
        res = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), _loader(x, y, 2 if per_slice else 1)[0], torch.device("cuda"), str(d) if save else None)
        return res, [ln.split(",") for ln in open(d / "pred_results.csv").read().splitlines()] if save else None

    for per_slice in (True, False):
        res, rows = run(f"all_{per_slice}", per_slice, options)
        assert list(res.keys()) == PIXEL_KEYS + sum(keys.values(), [])
        assert ",".join(rows[0]) == ",PATH,RMSE,PSNR,SSIM,VIF,GMSD,HaarPSI,FSIM,LPIPS,DISTS,VSI,MDSI" and len(rows) == 5
        at = 5
        for attr, value in options.items():
            one, one_rows = run(f"{attr}_{per_slice}", per_slice, {attr: value})
            n = len(columns[attr])
            assert list(one.keys()) == PIXEL_KEYS + keys[attr] and one_rows[0] == ["", "PATH", "RMSE", "PSNR", "SSIM"] + columns[attr]
            assert {k: res[k] for k in PIXEL_KEYS + keys[attr]} == one, attr
            assert [r[:5] + r[at:at + n] for r in rows] == one_rows, attr
            at += n
        assert at == len(rows[0])
        if per_slice:
            each = res

    # the batch's one host read under test_per_slice: 7 pixel values and 3 x 8 of the options per slice
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
    again, _ = run("counted", True, options, save=False)
    assert reads == [("tolist", ((7 + 3 * 8) * 2,))] * 2, reads
    assert again == each
