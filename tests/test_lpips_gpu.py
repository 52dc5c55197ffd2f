"""LPIPS and DISTS on the device: the L2 pool, the LPIPS level reduction, the channel moments and the DISTS finish
against the float64 restatement of tests/_lpips_ref.py with bounds derived from the kernels' arithmetic as include/mtdgan_hip.h
states it; the VGG-16 feature maps with both pools; lpips_each / dists_each end to end against the reference's own float64 numbers
(tests/golden/lpips_dists_piq.npz); and the test loop's opt-in (model.perceptual_vgg16, model.test_lpips, model.test_dists)."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import _lpips_ref as R
import mtdgan_oracle as orc
from _metrics import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
U24, U53 = 2.0 ** -24, 2.0 ** -53
WHO = ("input", "gt", "pred")


def _define(name):
    return int(re.search(r"#define %s (\d+)" % name, open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()).group(1))


def _relu_normal(shape, seed):
    return torch.relu(torch.randn(shape, generator=torch.Generator().manual_seed(seed)))


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------ L2 pool
def _pool_rounds(shape):
    """Rounds the busiest thread takes, from the launch arithmetic the header states: one float4 of channels per thread and
    round, at most MTD_L2POOL_MAX_BLOCKS workgroups of 256 threads."""
    cap = _define("MTD_L2POOL_MAX_BLOCKS")
    B, H, W, C = shape
    total = B * ((H + 1) // 2) * ((W + 1) // 2) * (C // 4)
    threads = 256 * min(cap, -(-total // 256))
    return -(-total // threads)


@pytest.mark.parametrize("shape,rounds", [((2, 5, 7, 64), 1), ((1, 16, 16, 512), 1), ((1, 1, 1, 64), 1), ((1, 128, 130, 512), 2)])
def test_l2pool_against_float64(hip_lib, shape, rounds):
    """The bound: x * x rounds once, each of the (at most) nine fmaf(k, x^2, acc) once (k x^2 is exact, k a power of two), the terms
    are non-negative, so the sum is within 10 u of the exact one (u = 2^-24); the constant 1e-12 as a float and its addition
    add 2 u; the square root halves that and rounds once: 12 / 2 + 1 = 7 u relative."""
    from mtd_gan_amd import metrics as M
    assert _pool_rounds(shape) == rounds
    B, H, W, C = shape
    buf = torch.randn((B + 1, H, W, C), generator=torch.Generator().manual_seed(12))
    buf[B] = float("nan")                                        # guard image behind the input
    dev = buf.cuda()
    out = M.l2pool3x3s2(dev[:B])
    ref = R.l2pool(_nchw(buf[:B])).permute(0, 2, 3, 1)
    assert tuple(out.shape) == (B, (H + 1) // 2, (W + 1) // 2, C) == tuple(ref.shape)
    err = float(((out.cpu().double() - ref).abs() / ref).max())
    print(f"l2pool {shape}: largest relative distance to float64 {err / U24:.3f} x 2^-24 (bound 7)")
    assert torch.isfinite(out).all() and err <= 7 * U24 * 1.001
    assert torch.isnan(dev[B]).all()
    # ... and the entry point itself into the front of a larger buffer: nothing is written behind the output
    n = ref.numel()
    big = torch.full((n + 4096,), -7.0, device="cuda")
    assert hip_lib.mtd_l2pool3x3s2(dev.data_ptr(), big.data_ptr(), B, H, W, C, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(big[:n], out.reshape(-1)) and (big[n:] == -7.0).all()


def test_l2pool_refuses_bad_shapes(hip_lib):
    x = torch.zeros(1, 4, 4, 8, device="cuda")
    o = torch.zeros(1, 2, 2, 8, device="cuda")
    assert hip_lib.mtd_l2pool3x3s2(x.data_ptr(), o.data_ptr(), 1, 4, 4, 6, None) == EINVAL          # C not a multiple of 4
    assert hip_lib.mtd_l2pool3x3s2(x.data_ptr(), o.data_ptr(), 1, 0, 4, 8, None) == EINVAL          # an empty map
    assert hip_lib.mtd_l2pool3x3s2(x.data_ptr(), o.data_ptr(), 0, 4, 4, 8, None) == EINVAL
    assert hip_lib.mtd_l2pool3x3s2(None, o.data_ptr(), 1, 4, 4, 8, None) == EINVAL
    assert hip_lib.mtd_l2pool3x3s2(x.data_ptr(), None, 1, 4, 4, 8, None) == EINVAL


# ------------------------------------------------------------------------------------------------------- LPIPS level
def _lpips_launch(hw, C):
    """(nblk, rounds, summation depth, norm depth) from the launch arithmetic the header states."""
    lp = min(C // 4, 64)
    P = 4 * 64 // lp
    nblk = min(-(-hw // P), _define("MTD_LPIPS_MAX_BLOCKS"))
    rounds = -(-hw // (P * nblk))
    depth = (C // lp) * rounds + 6 + 2 + -(-nblk // 256) + 8
    return nblk, rounds, depth, C // lp + int(math.log2(lp))


def _lpips_reference(t, o, w, distance):
    """float64: (sums (B,), the first-order sensitivity Q (B,) of the sums to a relative perturbation of the normalised values)."""
    ft, fo = _nchw(t), _nchw(o)
    s = R.lpips_level(fo, ft, w, distance)
    no = fo / (torch.sqrt((fo * fo).sum(dim=1, keepdim=True)) + 1e-10)
    nt = ft / (torch.sqrt((ft * ft).sum(dim=1, keepdim=True)) + 1e-10)
    mag = no.abs() + nt.abs()
    q = mag if distance == "mae" else 2 * (no - nt).abs() * mag
    return s, (q * w.view(1, -1, 1, 1)).sum(dim=(1, 2, 3))


def _lpips_bound(s, q, hw, C):
    """Absolute bound on |kernel - restatement| per image, u = 2^-53.  A normalised value v / (|v| + 1e-10) carries, in the kernel,
    the norm's sum (depth C / LP + log2 LP over non-negative exact products: that many u, halved by the root), the root, the
    addition, the reciprocal and the product (4 u); in the restatement a sum of C terms in an order of torch's choosing (at most
    C - 1 u, halved), the root, the addition and the division (3 u).  Both perturb d(o, t) through q = d'(.) (|o| + |t|) to first
    order (Q above; 1 % is kept for the second order), the subtraction, the square or absolute value and the weight add 3 u on
    each side.  The sums of the non-negative terms w d then differ by the summation depths: the kernel's from the header,
    torch's at most C h w - 1."""
    _, _, depth, norm_depth = _lpips_launch(hw, C)
    eps = (norm_depth / 2 + 4 + (C - 1) / 2 + 3) * U53
    return 1.01 * (eps * q + (6 + depth + C * hw - 1) * U53 * s)


def _level_case(shape, distance, two, seed=0):
    from mtd_gan_amd import metrics as M
    B, h, w, C = shape
    t, a, b = (_relu_normal(shape, 300 + C + 7 * k + seed) for k in range(3))
    a[0, 0, 0] = 0.0                                            # a pixel whose channels are all zero: 0 / (0 + 1e-10) = 0
    t[B - 1, h - 1, w - 1] = 0.0
    wts = torch.rand(C, generator=torch.Generator().manual_seed(C), dtype=torch.float64) / C
    td, ad, bd, wd = t.cuda(), a.cuda(), b.cuda(), wts.cuda()
    got = M.lpips_level_each(td, ad, bd if two else None, wd, distance).cpu().reshape(2 if two else 1, B)
    assert torch.isfinite(got).all()
    worst = 0.0
    for k, o in enumerate((a, b) if two else (a,)):
        s, q = _lpips_reference(t, o, wts, distance)
        bound = _lpips_bound(s, q, h * w, C)
        err = (got[k] - s).abs()
        worst = max(worst, float((err / s).max()))
        print(f"lpips level {shape} {distance} other {k}: hip {got[k].tolist()} float64 {s.tolist()} |diff| / sum {(err / s).tolist()} "
              f"bound / sum {(bound / s).tolist()}")
        assert (bound / s < 1e-9).all() and (err <= bound).all()
    return (td, ad, bd, wd), got, worst


@pytest.mark.parametrize("distance", ["mse", "mae"])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_lpips_level_channels(hip_lib, C, distance):
    _level_case((2, 3, 5, C), distance, two=True)


def test_lpips_level_one_other_self_batch_and_stride(hip_lib):
    from mtd_gan_amd import metrics as M
    (t, a, b, w), both, _ = _level_case((2, 3, 5, 128), "mse", two=True)
    _, one, _ = _level_case((2, 3, 5, 128), "mse", two=False)
    assert torch.equal(one[0], both[0])                          # the second map changes nothing for the first
    for distance in ("mse", "mae"):
        assert (M.lpips_level_each(t, t.clone(), a, w, distance).cpu()[:2] == 0).all()      # a map against itself: exactly 0
        full = M.lpips_level_each(t, a, b, w, distance).cpu().reshape(2, 2)
        for i in range(2):                                       # image i of a batch has the bits of the one-image call
            alone = M.lpips_level_each(t[i:i + 1], a[i:i + 1], b[i:i + 1], w, distance).cpu()
            assert torch.equal(alone, full[:, i])
    out = torch.full((40,), -7.0, dtype=torch.float64, device="cuda")
    M.lpips_level_each(t, a, b, w, "mse", out=out[3:], out_stride=5, other_stride=20)
    host = out.cpu()
    written = [3, 8, 23, 28]
    assert torch.equal(host[written], both.reshape(-1)[[0, 1, 2, 3]])
    assert (host[[i for i in range(40) if i not in written]] == -7.0).all()


def test_lpips_level_second_grid_round(hip_lib):
    shape = (1, 130, 127, 64)
    nblk, rounds, _, _ = _lpips_launch(130 * 127, 64)
    assert nblk == _define("MTD_LPIPS_MAX_BLOCKS") and rounds == 2
    _level_case(shape, "mse", two=True)


def test_lpips_level_refusals(hip_lib):
    from mtd_gan_amd import kernels as K
    x = torch.zeros(1, 3, 5, 96, device="cuda")
    w = torch.zeros(512, dtype=torch.float64, device="cuda")
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    ws = K.workspace(1 << 16, x.device)
    args = lambda C, dist=0, stride=1: (x.data_ptr(), x.data_ptr(), None, 1, 3, 5, C, w.data_ptr(), dist, out.data_ptr(), stride, 1, ws.data_ptr(), None)  # noqa: E731
    assert hip_lib.mtd_lpips_level_ws_bytes(1, 3, 5, 96) == 0 and hip_lib.mtd_lpips_level_each(*args(96)) == EINVAL
    assert hip_lib.mtd_lpips_level_each(*args(64, dist=2)) == EINVAL and hip_lib.mtd_lpips_level_each(*args(64, stride=0)) == EINVAL
    assert hip_lib.mtd_lpips_level_each(*args(64)) == 0
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------- channel moments, DISTS finish
def _moments_launch(hw, C, n):
    """(ranges, summation depth) from the launch arithmetic the header states."""
    pl = 256 if C == 1 else 256 // (C // 4)
    ranges = min(-(-hw // (pl * _define("MTD_MOMENTS_WALK"))), _define("MTD_MOMENTS_MAX_RANGES"))
    per_range = -(-hw // ranges)
    return ranges, -(-per_range // pl) + math.ceil(math.log2(pl)) + ranges


@pytest.mark.parametrize("shape,ranges", [((2, 5, 7, 1), 1), ((2, 5, 7, 64), 1), ((2, 5, 7, 512), 1), ((2, 24, 23, 64), 2), ((1, 100, 91, 1), 2)])
@pytest.mark.parametrize("two", [True, False])
def test_channel_moments_against_float64(hip_lib, shape, ranges, two):
    """A product of two floats is exact in double, so only the additions round: |kernel - restatement| <= (the kernel's summation
    depth from the header + torch's, at most h w - 1) u times the sum of the absolute values of the terms, u = 2^-53."""
    from mtd_gan_amd import metrics as M
    B, h, w, C = shape
    got_ranges, depth = _moments_launch(h * w, C, 2 if two else 1)
    assert got_ranges == ranges
    t, a, b = (torch.randn(shape, generator=torch.Generator().manual_seed(500 + C + k)) for k in range(3))
    others = (a, b) if two else (a,)
    got = M.channel_moments_each(t.cuda(), a.cuda(), b.cuda() if two else None).cpu()
    ref = R.moments(_nchw(t), *[_nchw(o) for o in others])
    mass = R.moments(_nchw(t).abs(), *[_nchw(o).abs() for o in others])
    assert tuple(got.shape) == (B, C, 2 + 3 * len(others)) == tuple(ref.shape)
    bound = 1.01 * (depth + h * w - 1) * U53 * mass
    err = (got - ref).abs()
    print(f"moments {shape} others {len(others)}: largest |diff| / bound {float((err / bound).max()):.3f}, depth {depth}, "
          f"largest |diff| / mass {float((err / mass).max()):.3e}")
    assert (err <= bound).all()
    full = M.channel_moments_each(t.cuda(), a.cuda(), b.cuda() if two else None)
    for i in range(B):                                           # image i of a batch has the bits of the one-image call
        alone = M.channel_moments_each(t[i:i + 1].cuda(), a[i:i + 1].cuda(), b[i:i + 1].cuda() if two else None)
        assert torch.equal(alone[0], full[i])


def test_channel_moments_refusals(hip_lib):
    from mtd_gan_amd import kernels as K
    x = torch.zeros(1, 3, 5, 8, device="cuda")
    out = torch.zeros(8 * 8, dtype=torch.float64, device="cuda")
    ws = K.workspace(1 << 16, x.device)
    for C in (2, 6, 1028):
        assert hip_lib.mtd_channel_moments_ws_bytes(1, 3, 5, C, 1) == 0
        assert hip_lib.mtd_channel_moments_each(x.data_ptr(), x.data_ptr(), None, 1, 3, 5, C, out.data_ptr(), ws.data_ptr(), None) == EINVAL
    assert hip_lib.mtd_channel_moments_each(None, x.data_ptr(), None, 1, 3, 5, 8, out.data_ptr(), ws.data_ptr(), None) == EINVAL
    assert hip_lib.mtd_channel_moments_each(x.data_ptr(), x.data_ptr(), None, 1, 3, 5, 8, out.data_ptr(), ws.data_ptr(), None) == 0
    torch.cuda.synchronize()


def _level_shapes(B, h, w):
    shapes, hh, ww = [(B, h, w, 1), (B, h, w, 64)], h, w
    for C in (128, 256, 512, 512):
        hh, ww = (hh + 1) // 2, (ww + 1) // 2
        shapes.append((B, hh, ww, C))
    return shapes


def test_dists_finish_on_constant_maps(hip_lib):
    """Maps that are constant over the pixels have variance 0 up to the rounding of sum x^2 / n - mu^2: S2 = (2 cov + 1e-6) /
    (var + var + 1e-6) is 1 within 1e-9, the score is finite, and a map with the target's values gives exactly the self row."""
    from mtd_gan_amd import metrics as M
    dw = M.dists_weights(R.seeded_dists_weights())
    beta_only = torch.stack([torch.zeros(1475, dtype=torch.float64), dw[1] / dw[1].sum()]).cuda()
    tables, pixels = [], []
    for lvl, shape in enumerate(_level_shapes(2, 6, 5)):
        t = torch.full(shape, 0.3 + 0.2 * lvl)
        a = torch.full(shape, 0.9 - 0.1 * lvl)
        tables.append(M.channel_moments_each(t.cuda(), a.cuda(), t.clone().cuda()))
        pixels.append(shape[1] * shape[2])
    out, parts = M.dists_finish(tables, pixels, beta_only, self_row=1, parts=True)
    out, parts = out.cpu(), parts.cpu()
    assert tuple(out.shape) == (3, 2) and tuple(parts.shape) == (3, 2, 6) and torch.isfinite(out).all()
    print("dists on constant maps:", out.tolist())
    assert (out[0].abs() < 1e-9).all()                           # 1 - sum(beta * 1)
    assert torch.equal(out[2], out[1]) and torch.equal(parts[2], parts[1])
    both = M.dists_finish(tables, pixels, dw.cuda(), self_row=-1).cpu()
    assert tuple(both.shape) == (2, 2) and torch.isfinite(both).all() and (both[0] > 1e-3).all()      # S1 < 1 where the means differ


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_dists_finish_on_restated_tables_gives_the_fixture_values(hip_lib, index):
    """The finish alone, on float64 moment tables of the restatement: the fixture's float64 parts and scores (the reference's own)
    within 1e-12, the bound tests/test_lpips_cpu.py holds the restatement to for the same arithmetic in another order."""
    from mtd_gan_amd import metrics as M
    golden = np.load(R.GOLDEN)
    sd, dw = R.seeded_state_dict(), R.seeded_dists_weights()
    x, y, pred = R.case_inputs(index)
    with torch.no_grad():
        fy, fx, fp = (R.dists_maps(sd, t) for t in (y, x, pred))
    tables = [R.moments(t, a, b).contiguous().cuda() for t, a, b in zip(fy, fx, fp)]
    pixels = [t.shape[2] * t.shape[3] for t in fy]
    out, parts = M.dists_finish(tables, pixels, M.dists_weights(dw).cuda(), self_row=1, parts=True)
    e_s = float(np.max(np.abs(out.cpu().numpy() - golden[f"dists64_{index}"])))
    e_p = float(np.max(np.abs(parts.cpu().numpy() - golden[f"dists_parts64_{index}"])))
    print(f"dists finish case {index}: score distance {e_s:.3e} parts distance {e_p:.3e}")
    assert e_s < 1e-12 and e_p < 1e-12


# ------------------------------------------------------------------------------------------------------- feature maps
@pytest.fixture(scope="module")
def state():
    return R.seeded_state_dict()


@pytest.fixture(scope="module")
def vgg(state):
    from mtd_gan_amd.metrics import VGG16Features
    return VGG16Features(state)


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.mark.parametrize("pool", ["max", "l2"])
@pytest.mark.parametrize("B,H,W", [(2, 48, 40), (1, 50, 37), (2, 16, 17)])
def test_feature_maps(hip_lib, state, vgg, B, H, W, pool):
    x = orc.synthetic_ldct(B, seed=21, size=max(H, W))[0][:, :, :H, :W].contiguous()
    with torch.no_grad():
        ref = R.features(state, x, pool)
    got = vgg(x.cuda(), pool=pool)
    assert len(got) == 5
    sides = [(H, W)]
    for _ in range(4):
        sides.append(tuple(s // 2 if pool == "max" else (s + 1) // 2 for s in sides[-1]))
    if (H, W) == (50, 37):
        assert [s[1] for s in sides] == ([37, 18, 9, 4, 2] if pool == "max" else [37, 19, 10, 5, 3])
    for lvl, (g, r, C) in enumerate(zip(got, ref, R.LPIPS_CHANNELS)):
        assert tuple(g.shape) == (B,) + sides[lvl] + (C,) == (B, r.shape[2], r.shape[3], r.shape[1])
        e = rel(g.permute(0, 3, 1, 2), r)
        print(f"VGG-16 map {lvl + 1} ({pool}) at B={B} {H}x{W}: rel = {e:.3e}")
        assert e < 1e-3, (lvl, e)
    # the outermost ring of relu1_2 alone: a mean folded into the bias would be wrong there
    ring = torch.ones(H, W, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    e = rel(got[0].permute(0, 3, 1, 2)[..., ring.cuda()], ref[0][..., ring])
    print(f"VGG-16 relu1_2 ring ({pool}) at B={B} {H}x{W}: rel = {e:.3e}")
    assert e < 1e-3


@pytest.mark.parametrize("pool", ["max", "l2"])
def test_feature_maps_of_a_chunked_batch_same_bits(hip_lib, vgg, monkeypatch, pool):
    from mtd_gan_amd import metrics as M
    x = orc.synthetic_ldct(3, seed=22, size=48)[0][:, :, :, :40].contiguous().cuda()
    per_image = 48 * 40 * 64 * 4
    singles = [vgg(x[i:i + 1], pool=pool) for i in range(3)]
    monkeypatch.setattr(M, "_MAX_MAP_BYTES", 2 * per_image - 1)
    chunked = vgg(x, pool=pool)
    monkeypatch.setattr(M, "_MAX_MAP_BYTES", per_image - 1)
    with pytest.raises(ValueError):
        vgg(x, pool=pool)
    for lvl in range(5):
        assert chunked[lvl].shape[0] == 3 and chunked[lvl].is_contiguous()
        for i in range(3):
            assert torch.equal(chunked[lvl][i], singles[i][lvl][0]), (lvl, i)


def test_feature_maps_refuse_small_images(hip_lib, vgg):
    for pool in ("max", "l2"):
        with pytest.raises(ValueError):
            vgg(torch.zeros(1, 1, 15, 64, device="cuda"), pool=pool)


# --------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_lpips_and_dists_against_the_reference(hip_lib, vgg, golden, index):
    """LPIPS within max(1e-3, 4 e32) relative of the reference's float64 score, e32 the reference's own float32 spread (relative)
    from the fixture's meta -- the rule test_compute_tml holds the same conv stack to; DISTS by the same rule on 1 - score, the
    weighted similarity sum near 1 (e32 absolute, which is relative to a sum near 1)."""
    from mtd_gan_amd import metrics as M
    meta = json.loads(str(golden["meta"]))
    distance = R.CASES[index][3]
    x, y, pred = (t.cuda() for t in R.case_inputs(index))
    lw, dw = R.seeded_lpips_weights(), R.seeded_dists_weights()
    l64, lp64 = golden[f"lpips64_{index}"], golden[f"lpips_parts64_{index}"]
    d64, dp64 = golden[f"dists64_{index}"], golden[f"dists_parts64_{index}"]
    got, parts = M.lpips_each(x, y, pred, vgg=vgg, weights=lw, distance=distance, parts=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == l64.shape and tuple(parts.shape) == lp64.shape
    got, parts = got.cpu().numpy(), parts.cpu().numpy()
    tol_l = max(1e-3, 4 * meta["spread"]["lpips_rel"])
    e = np.abs(got[[0, 2]] - l64[[0, 2]]) / l64[[0, 2]]
    e_p = np.abs(parts[[0, 2]] - lp64[[0, 2]]) / lp64[[0, 2]]
    print(f"LPIPS case {index} ({distance}): hip {got.tolist()} float64 {l64.tolist()} rel {e.max():.3e} parts rel {e_p.max():.3e} (bound {tol_l:.1e})")
    assert (got[1] == 0).all() and (parts[1] == 0).all()
    assert e.max() <= tol_l and e_p.max() <= tol_l
    assert np.array_equal(parts.sum(axis=2)[1], got[1]) and np.allclose(parts.sum(axis=2), got, rtol=1e-14, atol=0)

    got, parts = M.dists_each(x, y, pred, vgg=vgg, weights=dw, parts=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == d64.shape and tuple(parts.shape) == dp64.shape
    got, parts = got.cpu().numpy(), parts.cpu().numpy()
    tol_d = max(1e-3, 4 * meta["spread"]["dists_abs"])
    e = np.abs((1 - got) - (1 - d64)) / (1 - d64)
    e_p = np.abs(parts - dp64) / dp64
    print(f"DISTS case {index}: hip {got.tolist()} float64 {d64.tolist()} rel of 1 - score {e.max():.3e} parts rel {e_p.max():.3e} (bound {tol_d:.1e})")
    assert e.max() <= tol_d and e_p.max() <= tol_d
    assert np.abs(got[1] - d64[1]).max() < 1e-6                  # the gt row: the reference's dists(y, y)


def test_compute_and_per_slice_forms(hip_lib, vgg):
    from mtd_gan_amd import metrics as M
    x, y, pred = (t.cuda() for t in R.case_inputs(0))
    lw, dw = M.lpips_weights(R.seeded_lpips_weights()).cuda(), M.dists_weights(R.seeded_dists_weights()).cuda()
    each_l, each_d = M.lpips_each(x, y, pred, vgg=vgg, weights=lw), M.dists_each(x, y, pred, vgg=vgg, weights=dw)
    for fn, each, kw in ((M.compute_LPIPS, each_l, dict(weights=lw)), (M.compute_DISTS, each_d, dict(weights=dw))):
        triple = fn(x, y, pred, vgg=vgg, **kw)
        assert len(triple) == 3 and all(t.is_cuda and t.dim() == 0 and t.dtype == torch.float64 for t in triple)
        assert torch.equal(torch.stack(triple), each.mean(dim=1))
        with pytest.raises(NotImplementedError):
            fn(x, y, pred, data_range=255.0, vgg=vgg, **kw)
    assert M.lpips_per_slice(x, y, pred, vgg=vgg, weights=lw) == [tuple(each_l[:, i].tolist()) for i in range(2)]
    assert M.dists_per_slice(x, y, pred, vgg=vgg, weights=dw) == [tuple(each_d[:, i].tolist()) for i in range(2)]
    for i in range(2):                                           # a slice alone: other conv plans, the end-to-end bound
        alone = M.lpips_each(x[i:i + 1], y[i:i + 1], pred[i:i + 1], vgg=vgg, weights=lw)
        assert alone[1, 0] == 0 and float(((alone[[0, 2], 0] - each_l[[0, 2], i]).abs() / each_l[[0, 2], i]).max()) <= 1e-3
    with pytest.raises(TypeError):
        M.lpips_each(x, y, pred, vgg=None, weights=lw)
    with pytest.raises(ValueError):
        M.lpips_each(x, y, pred, vgg=vgg, weights=lw, distance="l2")
    with pytest.raises(ValueError):
        M.dists_each(x[:, :, :15], y[:, :, :15], pred[:, :, :15], vgg=vgg, weights=dw)


# -------------------------------------------------------------------------------------------------------------- engine
PIXEL_KEYS = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in WHO]
LPIPS_KEYS = [f"{who}_lpips" for who in WHO]
DISTS_KEYS = [f"{who}_dists" for who in WHO]
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


def test_engine_with_test_lpips_and_test_dists(hip_lib, vgg, golden, tmp_path):
    from mtd_gan_amd import engine, metrics as M
    meta = json.loads(str(golden["meta"]))
    x, y = orc.synthetic_ldct(2, seed=9, size=64)
    lw, dw = R.seeded_lpips_weights(), R.seeded_dists_weights()
    by_two, by_one = _loader(x, y, 2), _loader(x, y, 1)
    m = types.SimpleNamespace(Generator=_Pointwise().cuda())

    # the options absent, None, False (with and without the network): the dict and the CSV bytes of the loop as it was
    plain, plain_csv = _run(m, by_one, tmp_path, "plain")
    assert list(plain.keys()) == PIXEL_KEYS and plain_csv.splitlines()[0] == b",PATH,RMSE,PSNR,SSIM"
    m.perceptual_vgg16 = vgg
    for off in (None, False):
        m.test_lpips = m.test_dists = off
        assert _run(m, by_one, tmp_path, f"off_{off!r}") == (plain, plain_csv)

    # the default path on batches of one: keys after the others, two columns after SSIM, the values of the direct calls
    m.test_lpips, m.test_dists = lw, dw
    res, csv = _run(m, by_one, tmp_path, "ones")
    assert list(res.keys()) == PIXEL_KEYS + LPIPS_KEYS + DISTS_KEYS and {k: res[k] for k in PIXEL_KEYS} == plain
    lines = csv.decode().splitlines()
    assert lines[0] == ",PATH,RMSE,PSNR,SSIM,LPIPS,DISTS" and len(lines) == 3
    assert [ln.split(",")[:5] for ln in lines] == [ln.split(",") for ln in plain_csv.decode().splitlines()]
    xd, yd = x.cuda(), y.cuda()
    clipped = (1.05 * xd - 0.02).clamp(0, 1)
    meters, direct = {}, []
    for i in range(2):
        s = slice(i, i + 1)
        lv = M.lpips_each(xd[s], yd[s], clipped[s], vgg=vgg, weights=lw).mean(dim=1).tolist()
        dv = M.dists_each(xd[s], yd[s], clipped[s], vgg=vgg, weights=dw).mean(dim=1).tolist()
        direct.append((lv, dv))
        assert lines[1 + i].split(",")[5:] == [str(lv[2]), str(dv[2])]
        for name, vals in (("lpips", lv), ("dists", dv)):
            for who, v in zip(WHO, vals):
                meters.setdefault(f"{who}_{name}", engine._Meter()).update(v, 1)
    assert {k: res[k] for k in LPIPS_KEYS + DISTS_KEYS} == {k: round(mm.global_avg, 7) for k, mm in meters.items()}
    assert res["gt_lpips"] == 0.0 and res["input_lpips"] > 0.0 and res["pred_lpips"] > 0.0
    assert abs(res["gt_dists"] - round(meta["gt_dists"], 7)) <= 1e-6 and res["input_dists"] > res["gt_dists"]

    # one option alone, the dict form, and beside test_fsim: behind its keys and column
    del m.test_dists
    m.test_lpips = dict(weights=lw, distance="mae")
    mae, mae_csv = _run(m, by_one, tmp_path, "mae")
    assert list(mae.keys()) == PIXEL_KEYS + LPIPS_KEYS and mae_csv.splitlines()[0] == b",PATH,RMSE,PSNR,SSIM,LPIPS"
    want = M.lpips_each(xd[:1], yd[:1], clipped[:1], vgg=vgg, weights=lw, distance="mae")[2, 0].item()
    assert mae_csv.decode().splitlines()[1].split(",")[5] == str(want) and mae["pred_lpips"] != res["pred_lpips"]
    m.test_lpips, m.test_dists, m.test_fsim = lw, dw, True
    all_, all_csv = _run(m, by_one, tmp_path, "all")
    assert list(all_.keys()) == PIXEL_KEYS + FSIM_KEYS + LPIPS_KEYS + DISTS_KEYS
    assert all_csv.splitlines()[0] == b",PATH,RMSE,PSNR,SSIM,FSIM,LPIPS,DISTS"
    assert {k: all_[k] for k in PIXEL_KEYS + LPIPS_KEYS + DISTS_KEYS} == res
    del m.test_fsim

    # per slice at B = 2: the same keys and columns; each slice's row within the end-to-end bound of the batch-of-one loop's
    # (the conv plans differ with the batch), LPIPS relative, DISTS on 1 - score
    m.test_per_slice = True
    each, each_csv = _run(m, by_two, tmp_path, "each")
    del m.test_lpips, m.test_dists
    plain_each, plain_each_csv = _run(m, by_two, tmp_path, "plain_each")
    assert list(plain_each.keys()) == PIXEL_KEYS and plain_each_csv.splitlines()[0] == b",PATH,RMSE,PSNR,SSIM"
    assert list(each.keys()) == list(res.keys()) and {k: each[k] for k in PIXEL_KEYS} == plain_each
    each_lines = each_csv.decode().splitlines()
    assert each_lines[0] == lines[0] and [ln.split(",")[:5] for ln in each_lines] == [ln.split(",") for ln in plain_each_csv.decode().splitlines()]
    tol_l, tol_d = max(1e-3, 4 * meta["spread"]["lpips_rel"]), max(1e-3, 4 * meta["spread"]["dists_abs"])
    batch_l = M.lpips_each(xd, yd, clipped, vgg=vgg, weights=lw).tolist()
    batch_d = M.dists_each(xd, yd, clipped, vgg=vgg, weights=dw).tolist()
    for i in range(2):
        cells = each_lines[1 + i].split(",")[5:]
        assert cells == [str(batch_l[2][i]), str(batch_d[2][i])]               # the values of the direct calls on the batch
        (lv, dv) = direct[i]
        e_l, e_d = abs(float(cells[0]) - lv[2]) / lv[2], abs(float(cells[1]) - dv[2]) / (1 - dv[2])
        print(f"slice {i}: per-slice batch against the batch-of-one loop: LPIPS rel {e_l:.3e}, DISTS on 1 - score {e_d:.3e}")
        assert e_l <= tol_l and e_d <= tol_d
    assert each["gt_lpips"] == 0.0 and abs(each["pred_lpips"] - res["pred_lpips"]) <= tol_l * res["pred_lpips"] + 1e-7


def test_a_per_slice_batch_is_read_once(hip_lib, vgg, monkeypatch):
    """Under test_per_slice the 3 B LPIPS and 3 B DISTS values join the batch's single host read, behind the FSIM block."""
    from mtd_gan_amd import engine, metrics as M
    x, y = orc.synthetic_ldct(2, seed=9, size=64)
    x, y = x.cuda(), y.cuda()
    lw, dw = M.lpips_weights(R.seeded_lpips_weights()).cuda(), M.dists_weights(R.seeded_dists_weights()).cuda()
    M.fsim_each(x, y, x)                                          # (the filter table of this size is uploaded before the reads are counted)
    vgg(x)
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
    m = types.SimpleNamespace(Generator=_Pointwise().cuda(), test_per_slice=True, perceptual_vgg16=vgg, test_lpips=lw, test_dists=dw)
    loader = [dict(n_20=x, n_100=y)]
    res = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, torch.device("cuda"), None)
    assert reads == [("tolist", (13 * 2,))], reads
    assert list(res.keys()) == PIXEL_KEYS + LPIPS_KEYS + DISTS_KEYS
    del reads[:]
    m.test_fsim = True
    res = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, torch.device("cuda"), None)
    assert reads == [("tolist", (16 * 2,))], reads
    assert list(res.keys()) == PIXEL_KEYS + FSIM_KEYS + LPIPS_KEYS + DISTS_KEYS
