"""PNG scanlines quantised on the device: mtd_gray_png_rows against the numpy restatement of tests/_png_ref.py --
the output is integers and the float operations are the same ones, so the bytes must be EQUAL, no tolerance -- and
engine.test_MTD_GAN_Ours under `model.test_save_png`, whose files are read back with the restatement's own decoder."""
import os

import numpy as np
import pytest
import torch

import _png_ref as P
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu
GUARD = 0xA5

# (1, 1, 7): one row, shorter than two words.  (3, 37, 91): odd row strides 92 / 183, rows that start at every byte phase.
# (3, 512, 512): 64 partial limits per image, more words than one grid pass.  (70, 8, 8): more images than a grid capped per image
# would cover.  (2100, 1, 3): more images than the capped grid of the limits kernels has workgroups (2048), so they stride.
SHAPES = [(1, 1, 7), (1, 16, 16), (3, 37, 91), (2, 64, 64), (3, 512, 512), (70, 8, 8), (2100, 1, 3)]
KINDS = ("uniform", "constant", "maximum", "outside", "plateaus", "nonfinite")


def _images(shape, kind):
    n, H, W = shape
    a = np.random.RandomState(n * 7 + H * 3 + W + len(kind)).rand(n, H, W).astype(np.float32)
    if kind == "constant":                         # image 0 constant (level lut[0] everywhere), the others not
        a[0] = np.float32(0.375)
    elif kind == "maximum":                        # several pixels equal to the maximum (t == 256 -> 255) and to the minimum
        a[:, 0, ::2] = a.max(axis=(1, 2))[:, None]
        a[:, -1, ::3] = a.min(axis=(1, 2))[:, None]
    elif kind == "outside":                        # values below 0 and above 1: ordinary input of the stretch, clamped at depth 16
        a = (a * np.float32(3) - np.float32(1)).astype(np.float32)
    elif kind == "plateaus":                       # exact 0 and 1 plateaus
        a = np.clip(a * np.float32(1.5) - np.float32(0.25), 0, 1).astype(np.float32)
    elif kind == "nonfinite":                      # one image with a NaN and an Inf (and a -Inf where it has room)
        flat = a[-1].reshape(-1)
        flat[0] = np.nan
        flat[-1] = np.inf
        if flat.size > 4:
            flat[flat.size // 2] = -np.inf
    return a


@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scanlines_equal_the_restatement(hip_lib, shape, depth):
    from mtd_gan_amd import image_io, kernels as K
    n, H, W = shape
    S = image_io.row_bytes(W, depth)
    size = n * H * S
    lut = torch.from_numpy(P.LUT.copy()).cuda()
    for j, kind in enumerate(KINDS):
        a = _images(shape, kind)
        want = P.rows(a, depth)
        assert want.shape == (n, H, S)
        xd = torch.from_numpy(a).cuda()
        front = 13 + j                               # the output starts at every byte phase of a word in turn
        big = torch.full((front + size + 67,), GUARD, dtype=torch.uint8, device="cuda")
        out = big[front:front + size].view(n, H, S)
        K.gray_png_rows(xd, depth, lut if depth == 8 else None, out)
        got = big.cpu().numpy()
        body = got[front:front + size].reshape(n, H, S)
        differ = int((body != want).sum())
        print(f"{shape} depth {depth} {kind}: {differ} of {size} bytes differ")
        assert differ == 0, (kind, np.argwhere(body != want)[:5].tolist())
        assert (body[:, :, 0] == 0).all()                                                   # the filter byte of every row
        assert (got[:front] == GUARD).all() and (got[front + size:] == GUARD).all()         # guard bytes keep their bits
        again = image_io.gray_png_rows(xd, depth)                                           # the public call; a second run
        assert again.is_cuda and again.dtype == torch.uint8 and tuple(again.shape) == (n, H, S)
        assert np.array_equal(again.cpu().numpy(), body)
    assert torch.equal(xd.view(torch.int32), torch.from_numpy(a).cuda().view(torch.int32))   # the input is only read


def test_public_function_refuses_what_it_cannot_take(hip_lib):
    from mtd_gan_amd import image_io
    x = torch.zeros(2, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="float32"):
        image_io.gray_png_rows(x.half())
    with pytest.raises(RuntimeError, match="float32"):
        image_io.gray_png_rows(x.to(torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA"):
        image_io.gray_png_rows(x.cpu())
    with pytest.raises(ValueError):
        image_io.gray_png_rows(x[:, None])
    with pytest.raises(ValueError):
        image_io.gray_png_rows(x, depth=12)
    with pytest.raises(ValueError):
        image_io.gray_png_rows(x[:0])
    strided = torch.rand(2, 8, 16, device="cuda")[:, :, ::2]                                 # made contiguous on the way in
    assert np.array_equal(image_io.gray_png_rows(strided).cpu().numpy(), P.rows(strided.cpu().numpy(), 8))


# -------------------------------------------------------------------------------------------------------------- engine
PIXEL_KEYS = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in ("input", "gt", "pred")]


@pytest.fixture(scope="module")
def setup(hip_lib):
    """Model seeded as tests/test_per_slice_metrics_gpu.py builds it and four 64 x 64 slices, made once and never modified."""
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    torch.manual_seed(3)
    m = MTD_GAN_Method().cuda()
    m.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    m.Generator.eval()
    x, y = orc.synthetic_ldct(4, seed=9, size=64)
    return m, x, y


def _raw_predictions(m, x, per_batch):
    """Generator(x) batch by batch as the loop calls it, un-clipped: what the third file of every slice holds."""
    with torch.no_grad():
        pred = torch.cat([m.Generator(x[i:i + per_batch].cuda()) for i in range(0, x.shape[0], per_batch)]).cpu()
    assert float(pred.min()) < float(pred.max())
    return pred


def _loader(x, y, per_batch, paths=True):
    n = x.shape[0]
    names = [f"/data/L{i // 2:03d}/quarter_1mm/L{i // 2:03d}_QD_{i:04d}.dcm" for i in range(n)]
    out = []
    for i in range(0, n, per_batch):
        b = dict(n_20=x[i:i + per_batch], n_100=y[i:i + per_batch])
        if paths:
            b.update(path_n_20=names[i:i + per_batch], path_n_100=[p.replace("quarter", "full").replace("QD", "FD") for p in names[i:i + per_batch]])
        out.append(b)
    return out


def _check_files(d, stems, x, y, pred, depth):
    level = P.levels8 if depth == 8 else P.levels16
    expected = {"pred_results.csv"}
    for i, stem in enumerate(stems):
        for suffix, t in (("_gt_n_20.png", x), ("_gt_n_100.png", y), ("_pred_n_100.png", pred)):
            expected.add(stem + suffix)
            got, dp = P.decode_png(open(os.path.join(d, stem + suffix), "rb").read())
            want = level(t[i, 0].numpy())
            assert dp == depth and got.shape == (64, 64) and np.array_equal(got, want), (stem, suffix, int((got != want).sum()))
    assert set(os.listdir(d)) == expected


def _clear(m):
    for k in ("test_save_png", "test_per_slice"):
        if hasattr(m, k):
            delattr(m, k)


def test_loop_default_path_writes_the_three_files_per_slice(setup, tmp_path):
    from mtd_gan_amd import engine
    m, x, y = setup
    _clear(m)
    pred = _raw_predictions(m, x, 1)
    dev, l1 = torch.device("cuda"), torch.nn.L1Loss()
    plain = engine.test_MTD_GAN_Ours(m, l1, _loader(x, y, 1), dev, str(tmp_path / "plain"))
    m.test_save_png = True
    try:
        res = engine.test_MTD_GAN_Ours(m, l1, _loader(x, y, 1), dev, str(tmp_path / "png"))
        _check_files(str(tmp_path / "png"), [f"{i:04d}" for i in range(4)], x, y, pred, 8)
        assert res == plain and list(res.keys()) == PIXEL_KEYS
        assert open(tmp_path / "png" / "pred_results.csv").read() == open(tmp_path / "plain" / "pred_results.csv").read()
        # a batch of two slices on the default path is one sample: no image to save for it
        with pytest.raises(ValueError, match="test_per_slice"):
            engine.test_MTD_GAN_Ours(m, l1, _loader(x, y, 2), dev, str(tmp_path / "two"))
        with pytest.raises(ValueError, match="save_dir"):
            engine.test_MTD_GAN_Ours(m, l1, _loader(x, y, 1), dev, None)
    finally:
        _clear(m)


def test_loop_per_slice_writes_3b_files_per_batch(setup, tmp_path):
    from mtd_gan_amd import engine
    m, x, y = setup
    _clear(m)
    pred = _raw_predictions(m, x, 2)
    dev, l1 = torch.device("cuda"), torch.nn.L1Loss()
    m.test_per_slice = True
    try:
        plain = engine.test_MTD_GAN_Ours(m, l1, _loader(x[:2], y[:2], 2), dev, None)
        m.test_save_png = dict(depth=8, level=1, threads=2)
        res = engine.test_MTD_GAN_Ours(m, l1, _loader(x[:2], y[:2], 2), dev, str(tmp_path / "one"))
        _check_files(str(tmp_path / "one"), ["0000", "0001"], x, y, pred, 8)            # B = 2: six files
        assert res == plain
        # two batches without paths: the names count slices as the CSV does
        engine.test_MTD_GAN_Ours(m, l1, _loader(x, y, 2, paths=False), dev, str(tmp_path / "bare"))
        _check_files(str(tmp_path / "bare"), [f"slice_{k}" for k in range(4)], x, y, pred, 8)
        rows = open(tmp_path / "bare" / "pred_results.csv").read().splitlines()[1:]
        assert [r.split(",")[1] for r in rows] == [f"slice_{k}" for k in range(4)]
    finally:
        _clear(m)


def test_loop_depth_16(setup, tmp_path):
    from mtd_gan_amd import engine
    m, x, y = setup
    _clear(m)
    pred = _raw_predictions(m, x, 4)
    m.test_save_png = dict(depth=16)
    m.test_per_slice = True
    try:
        engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), _loader(x, y, 4), torch.device("cuda"), str(tmp_path))
        _check_files(str(tmp_path), [f"{i:04d}" for i in range(4)], x, y, pred, 16)
        got, _ = P.decode_png(open(tmp_path / "0002_pred_n_100.png", "rb").read())
        want = np.rint(np.clip(pred[2, 0].numpy(), 0, 1) * np.float32(65535)).astype(np.uint16)
        assert np.array_equal(got, want)
    finally:
        _clear(m)


def test_loop_without_the_attribute_is_unchanged(setup, tmp_path):
    """The result is what the loop's own pieces give on each batch (as tests/test_per_slice_metrics_gpu.py::test_engine_per_slice
    states the default path), and pred_results.csv is the only file."""
    from mtd_gan_amd import engine, kernels as K, metrics as M
    m, x, y = setup
    _clear(m)
    pred = _raw_predictions(m, x, 1)
    dev, l1 = torch.device("cuda"), torch.nn.L1Loss()
    meters = {}
    for i in range(4):
        xb, yb, r = x[i:i + 1].cuda(), y[i:i + 1].cuda(), pred[i:i + 1].cuda()
        s = {"L1_loss": float(engine._l1(l1, r, yb))}
        pm = M.pixel_metrics(xb, yb, K.clip01(r.contiguous()))
        for name in ("rmse", "psnr", "ssim"):
            for who, v in zip(("input", "gt", "pred"), pm[name]):
                s[f"{who}_{name}"] = v
        for k, v in s.items():
            meters.setdefault(k, engine._Meter()).update(v, 1)
    want = {k: round(mm.global_avg, 7) for k, mm in meters.items()}
    for setting in ("absent", False, None, {}):
        if setting != "absent":
            m.test_save_png = setting
        d = tmp_path / f"off_{setting}"
        res = engine.test_MTD_GAN_Ours(m, l1, _loader(x, y, 1), dev, str(d))
        assert list(res.keys()) == PIXEL_KEYS and res == want
        assert os.listdir(d) == ["pred_results.csv"]
    _clear(m)
