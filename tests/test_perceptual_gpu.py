"""The perceptual metrics on the device against float64: the 2x2 max-pool, the per-patch Gram-matrix L1 distance, the five
VGG-19 feature maps, compute_PL / compute_TML end to end, and the test loop's opt-in (model.perceptual_vgg)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _perceptual_ref as R
import mtdgan_oracle as orc
from _metrics import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ------------------------------------------------------------------------------------------------------------ max-pool
def _pool_rounds(shape):
    """Rounds the busiest thread takes, from the launch arithmetic the header states: one float4 of channels per thread and
    round, at most MTD_MAXPOOL_MAX_BLOCKS workgroups of 256 threads."""
    cap = int(re.search(r"#define MTD_MAXPOOL_MAX_BLOCKS (\d+)", open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()).group(1))
    B, H, W, C = shape
    total = B * (H // 2) * (W // 2) * (C // 4)
    threads = 256 * min(cap, -(-total // 256))
    return -(-total // threads)


@pytest.mark.parametrize("shape,rounds", [((2, 5, 7, 64), 1), ((1, 16, 16, 512), 1), ((1, 128, 130, 512), 2)])
def test_maxpool_bits(hip_lib, shape, rounds):
    from mtd_gan_amd import metrics as M
    assert _pool_rounds(shape) == rounds
    B, H, W, C = shape
    g = torch.Generator().manual_seed(11)
    buf = torch.randn((B + 1, H, W, C), generator=g)
    buf[B] = float("nan")                                        # guard image behind the input
    dev = buf.cuda()
    out = M.maxpool2x2(dev[:B])
    ref = F.max_pool2d(buf[:B].permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert tuple(out.shape) == (B, H // 2, W // 2, C)
    assert torch.equal(out.cpu(), ref)
    assert torch.isnan(dev[B]).all()
    # ... and the entry point itself into the front of a larger buffer: nothing is written behind the output
    n = ref.numel()
    big = torch.full((n + 4096,), -7.0, device="cuda")
    assert hip_lib.mtd_maxpool2x2(dev.data_ptr(), big.data_ptr(), B, H, W, C, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(big[:n].cpu(), ref.reshape(-1))
    assert (big[n:] == -7.0).all()


def test_maxpool_refuses_bad_shapes(hip_lib):
    x = torch.zeros(1, 4, 4, 8, device="cuda")
    o = torch.zeros(1, 2, 2, 8, device="cuda")
    assert hip_lib.mtd_maxpool2x2(x.data_ptr(), o.data_ptr(), 1, 4, 4, 6, None) == EINVAL          # C not a multiple of 4
    assert hip_lib.mtd_maxpool2x2(x.data_ptr(), o.data_ptr(), 1, 1, 4, 8, None) == EINVAL
    assert hip_lib.mtd_maxpool2x2(None, o.data_ptr(), 1, 4, 4, 8, None) == EINVAL


# ------------------------------------------------------------------------------------------------- per-patch Gram distance
def _relu_normal(shape, seed):
    return torch.relu(torch.randn(shape, generator=torch.Generator().manual_seed(seed)))


def _gram_case(shape, nan_remainder=False):
    from mtd_gan_amd import metrics as M
    B, h, w, C = shape
    X, Y = _relu_normal(shape, 100 + C), _relu_normal(shape, 200 + C)
    gx, gy = (R.gram(t.double().permute(0, 3, 1, 2)) for t in (X, Y))
    ref = (gx - gy).abs().sum().item()
    bound = 258 * 2.0 ** -24 * (gx + gy).sum().item()
    if nan_remainder:
        for t in (X, Y):
            t[:, (h // 16) * 16:] = float("nan")
            t[:, :, (w // 16) * 16:] = float("nan")
    Xd, Yd = X.cuda(), Y.cuda()
    got = M.patch_gram_l1(Xd, Yd).item()
    same = M.patch_gram_l1(Xd, Xd.clone()).item()
    print(f"patch_gram_l1 {shape}: hip {got:.9e} ref {ref:.9e} |diff| {abs(got - ref):.3e} bound {bound:.3e}")
    assert got == got and abs(got) != float("inf")
    assert abs(got - ref) <= bound
    assert same == 0.0


@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_patch_gram_l1_channels(hip_lib, C):
    _gram_case((2, 16, 16, C))


def test_patch_gram_l1_several_patches(hip_lib):
    _gram_case((1, 32, 32, 512))


def test_patch_gram_l1_never_reads_the_remainder(hip_lib):
    _gram_case((1, 37, 50, 64), nan_remainder=True)


def test_patch_gram_l1_without_a_patch(hip_lib):
    from mtd_gan_amd import kernels as K
    x = torch.zeros(1, 15, 40, 64, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = K.workspace(1024, x.device)
    assert hip_lib.mtd_patch_gram_l1_ws_bytes(1, 15, 40, 64) == 0
    assert hip_lib.mtd_patch_gram_l1(x.data_ptr(), x.data_ptr(), 1, 15, 40, 64, out.data_ptr(), ws.data_ptr(), None) == EINVAL
    assert hip_lib.mtd_patch_gram_l1(x.data_ptr(), x.data_ptr(), 1, 16, 37, 96, out.data_ptr(), ws.data_ptr(), None) == EINVAL


# ------------------------------------------------------------------------------------------------------- feature maps
@pytest.fixture(scope="module")
def state():
    return R.seeded_state_dict(0)


@pytest.fixture(scope="module")
def vgg(state):
    from mtd_gan_amd.metrics import VGG19Features
    return VGG19Features(state)


@pytest.mark.parametrize("B,H,W", [(2, 48, 40), (1, 50, 37), (2, 16, 17)])      # (16 x 17: the documented lower bound, relu5_1 is 1 x 1)
def test_feature_maps(hip_lib, state, vgg, B, H, W):
    x = orc.synthetic_ldct(B, seed=21, size=max(H, W))[0][:, :, :H, :W].contiguous()
    ref = R.features(state, x)
    got = vgg(x.cuda())
    assert len(got) == 5
    for lvl, (g, r) in enumerate(zip(got, ref)):
        assert tuple(g.shape) == (B, r.shape[2], r.shape[3], r.shape[1])
        e = rel(g.permute(0, 3, 1, 2), r)
        print(f"VGG-19 map {lvl + 1} at B={B} {H}x{W}: rel = {e:.3e}")
        assert e < 1e-3, (lvl, e)


def test_feature_maps_of_a_chunked_batch_same_bits(hip_lib, vgg, monkeypatch):
    """A batch beyond the map-size bound is cut into chunks and reassembled: with the bound lowered to just under two images' relu1_1, three
    images run as three chunks and give the bits of three one-image calls, in order, with the shapes of the whole batch."""
    from mtd_gan_amd import metrics as M
    x = orc.synthetic_ldct(3, seed=22, size=48)[0][:, :, :, :40].contiguous().cuda()
    per_image = 48 * 40 * 64 * 4
    assert M._MAX_MAP_BYTES == 2 ** 31 - 1 and M._MAX_MAP_BYTES // (512 * 512 * 64 * 4) == 31      # strictly below 2^31 bytes
    singles = [vgg(x[i:i + 1]) for i in range(3)]
    monkeypatch.setattr(M, "_MAX_MAP_BYTES", 2 * per_image - 1)
    chunked = vgg(x)
    monkeypatch.setattr(M, "_MAX_MAP_BYTES", per_image - 1)
    with pytest.raises(ValueError):
        vgg(x)
    for lvl in range(5):
        assert chunked[lvl].shape[0] == 3 and chunked[lvl].is_contiguous()
        for i in range(3):
            assert torch.equal(chunked[lvl][i], singles[i][lvl][0]), (lvl, i)


def test_compute_pl_at_the_smallest_size(hip_lib, state, vgg):
    from mtd_gan_amd import metrics as M
    x, y = (t[:, :, :16, :17].contiguous() for t in orc.synthetic_ldct(2, seed=23, size=32))
    pred = (0.5 * (x + y)).contiguous()
    ft = R.features(state, y)
    r = [R.pl(R.features(state, t), ft).item() for t in (x, pred)]
    got = [t.item() for t in M.compute_PL(x.cuda(), y.cuda(), pred.cuda(), vgg=vgg)]
    print("PL at 16x17: hip", got, "float64", r)
    assert got[1] == 0.0
    assert abs(got[0] - r[0]) <= 1e-3 * abs(r[0]) and abs(got[2] - r[1]) <= 1e-3 * abs(r[1])


def test_feature_maps_refuse_small_images(hip_lib, vgg):
    with pytest.raises(ValueError):
        vgg(torch.zeros(1, 1, 15, 64, device="cuda"))


# --------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def triple_256x272(state):
    """(input, target, pred) at B = 1, 256 x 272 and the restatement's PL / TML triples in float64 and in float32."""
    x, y = orc.synthetic_ldct(1, seed=33, size=272)
    x, y = x[:, :, :256].contiguous(), y[:, :, :256].contiguous()
    pred = (0.5 * (x + y)).contiguous()
    out = {}
    for dtype in (torch.float64, torch.float32):
        ft = R.features(state, y, dtype)
        fo = [R.features(state, t, dtype) for t in (x, pred)]
        out[dtype] = dict(pl=[R.pl(fo[0], ft).item(), R.pl(ft, ft).item(), R.pl(fo[1], ft).item()],
                          tml=[R.tml(fo[0], ft).item(), R.tml(ft, ft).item(), R.tml(fo[1], ft).item()])
    return (x, y, pred), out


def test_compute_pl(hip_lib, vgg, triple_256x272):
    from mtd_gan_amd import metrics as M
    (x, y, pred), ref = triple_256x272
    got = M.compute_PL(x.cuda(), y.cuda(), pred.cuda(), vgg=vgg)
    assert len(got) == 3 and all(t.is_cuda and t.dim() == 0 for t in got)
    got = [t.item() for t in got]
    r = ref[torch.float64]["pl"]
    print("PL hip", got, "float64", r)
    assert got[1] == 0.0 and r[1] == 0.0
    for k in (0, 2):
        assert abs(got[k] - r[k]) <= 1e-3 * abs(r[k])
    alone = M.compute_PL(x.cuda(), y.cuda(), pred.cuda(), option=False, vgg=vgg)
    assert alone.dim() == 0 and abs(alone.item() - r[2]) <= 1e-3 * abs(r[2])


def test_compute_tml(hip_lib, vgg, triple_256x272):
    from mtd_gan_amd import metrics as M
    (x, y, pred), ref = triple_256x272
    got = M.compute_TML(x.cuda(), y.cuda(), pred.cuda(), vgg=vgg)
    assert len(got) == 3 and all(t.is_cuda and t.dim() == 0 for t in got)
    got = [t.item() for t in got]
    r64, r32 = ref[torch.float64]["tml"], ref[torch.float32]["tml"]
    assert got[1] == 0.0 and r64[1] == 0.0
    for k in (0, 2):
        e32 = abs(r32[k] - r64[k]) / abs(r64[k])
        e = abs(got[k] - r64[k]) / abs(r64[k])
        print(f"TML entry {k}: float64 {r64[k]:.9e} hip {got[k]:.9e}; e32 = {e32:.3e}, hip error = {e:.3e}")
        assert e <= max(1e-3, 4 * e32)
    alone = M.compute_TML(x.cuda(), y.cuda(), pred.cuda(), option=False, vgg=vgg)
    # (pred alone: two stacked images instead of three, so the convolutions may take another plan -- same bound, not the same bits)
    e32 = abs(r32[2] - r64[2]) / abs(r64[2])
    assert alone.dim() == 0 and abs(alone.item() - r64[2]) / abs(r64[2]) <= max(1e-3, 4 * e32)


def test_compute_tml_refuses_small_images(hip_lib, vgg):
    from mtd_gan_amd import metrics as M
    x = torch.zeros(1, 1, 128, 128, device="cuda")
    with pytest.raises(ValueError):
        M.compute_TML(x, x, x, vgg=vgg)


# -------------------------------------------------------------------------------------------------------------- engine
def test_test_loop_with_and_without_the_feature_network(hip_lib, vgg, tmp_path):
    from mtd_gan_amd import engine, kernels as K, metrics as M
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    torch.manual_seed(3)
    m = MTD_GAN_Method().cuda()
    m.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    x, y = orc.synthetic_ldct(1, seed=9, size=256)
    loader = [dict(n_20=x, n_100=y, path_n_20=["L000_0001.dcm"], path_n_100=["L000_0001.dcm"])]
    dev = torch.device("cuda")
    plain_dir, vgg_dir = tmp_path / "plain", tmp_path / "vgg"
    plain = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, str(plain_dir))
    pixel_keys = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in ("input", "gt", "pred")]
    assert list(plain.keys()) == pixel_keys
    assert open(plain_dir / "pred_results.csv").readline() == ",PATH,RMSE,PSNR,SSIM\n"
    m.perceptual_vgg = None
    assert list(engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, None).keys()) == pixel_keys

    m.perceptual_vgg = vgg
    full = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, str(vgg_dir))
    six = [f"{who}_{name}" for name in ("pl", "tml") for who in ("input", "gt", "pred")]
    assert set(full.keys()) == set(pixel_keys) | set(six)
    assert all(full[k] == plain[k] for k in pixel_keys)
    with torch.no_grad():
        pred = K.clip01(m.Generator(x.cuda()).contiguous())
    pl = M.compute_PL(x.cuda(), y.cuda(), pred, vgg=vgg)
    tml = M.compute_TML(x.cuda(), y.cuda(), pred, vgg=vgg)
    for name, triple in (("pl", pl), ("tml", tml)):
        for who, v in zip(("input", "gt", "pred"), triple):
            assert full[f"{who}_{name}"] == round(v.item(), 7), (who, name)
    assert full["gt_pl"] == 0.0 and full["gt_tml"] == 0.0 and full["pred_pl"] > 0.0 and full["pred_tml"] > 0.0
    lines = open(vgg_dir / "pred_results.csv").read().splitlines()
    assert lines[0] == ",PATH,PL,TML,RMSE,PSNR,SSIM" and len(lines) == 2
    row = lines[1].split(",")
    assert row[:2] == ["0", "L000_0001.dcm"] and len(row) == 7
    assert float(row[2]) == pl[2].item() and float(row[3]) == tml[2].item()
    assert open(plain_dir / "pred_results.csv").read().splitlines()[1].split(",")[2:] == row[4:]
