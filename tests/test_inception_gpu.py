"""FID's InceptionV3 feature network on the device (csrc/inception.hip, inception.py, metrics.InceptionV3Features) against float64 on
the CPU: the resize, the three pools and the global pool alone; one conv per geometry the network adds to what the conv kernels
had been tested on (1x7, 7x1, 1x3, 3x1, 5x5 taps, stride 2 without padding, odd maps, the padded 48 / 80 channel layers, the 1- and
3-channel first layer); every block kind alone; the whole network; chunking; the test loop's opt-in (model.fid_features).

Reference: torch in float64 (F.interpolate, the pools, F.conv2d, and tests/_inception_ref.py for blocks and network -- parity is
pinned to that restatement, not to piq's class, which needs torchvision).

Bound, everywhere a sum is rounded: _metrics.rel <= max(1e-5, 4 e_ref), e_ref the error of torch's own fp32 CPU evaluation of the
same operation against the same float64 result (the factor 4: another legitimate fp32 summation order, nothing more) -- the rule
of tests/test_direct_conv_gpu.py.  Max pools and copies are compared bit for bit.  Operands are channel slices of wider tensors
filled with a NaN pattern, with a guard image behind the batch; the guards keep their bits.  Measured values: DESIGN 3.9."""
import pytest
import torch
import torch.nn.functional as F

import _inception_ref as R
import mtdgan_oracle as orc
from _metrics import rel

pytestmark = pytest.mark.gpu

FLOOR = 1e-5
NAN_BITS = 0x7FC12345


def _bound(ref32, ref64):
    e_ref = rel(ref32, ref64)
    return max(FLOOR, 4.0 * e_ref), e_ref


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


class Sliced:
    """An NHWC value as channels off .. off + C - 1 of the first B images of a (B + 1, H, W, ld) tensor of NaNs on the device
    (v = None: the slice is NaN as well, an output)."""

    def __init__(self, shape, ld, off, v=None):
        B, H, W, C = shape
        self.shape, self.off = shape, off
        base = torch.empty((B + 1, H, W, ld), dtype=torch.float32)
        base.view(torch.int32).fill_(NAN_BITS)
        if v is not None:
            base[:B, :, :, off:off + C] = v
        self.base = base.cuda()
        self.view = self.base[:B, :, :, off:off + C]

    def value(self):
        return self.view.cpu()

    def guards_kept(self):
        B, _, _, C = self.shape
        bits = self.base.cpu().view(torch.int32)
        return bool((bits[B] == NAN_BITS).all() and (bits[:B, :, :, :self.off] == NAN_BITS).all()
                    and (bits[:B, :, :, self.off + C:] == NAN_BITS).all())


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("size", [(64, 64), (512, 512), (100, 77)])
def test_resize_bilinear(hip_lib, size, C, normalize):
    from mtd_gan_amd import inception as I
    x = torch.rand(2, C, *size, generator=torch.Generator().manual_seed(size[1] + C))
    fin = (lambda t: 2 * t - 1) if normalize else (lambda t: t)
    ref64 = fin(F.interpolate(x.double(), size=(299, 299), mode="bilinear", align_corners=False))
    ref32 = fin(F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False))
    bound, e_ref = _bound(ref32, ref64)
    got = I.resize_bilinear(x.cuda(), (299, 299), normalize)
    assert tuple(got.shape) == (2, 299, 299, C)
    e = rel(_nchw(got.cpu()), ref64)
    print(f"resize {size} -> 299^2, C={C}, normalize={normalize}: rel {e:.3e}, torch fp32 {e_ref:.3e}, bound {bound:.3e}")
    assert e <= bound


@pytest.mark.parametrize("C", [1, 3])
def test_resize_of_equal_size_is_a_copy(hip_lib, C):
    from mtd_gan_amd import inception as I
    x = _randn(2, C, 299, 299, seed=C)
    got = I.resize_bilinear(x.cuda(), (299, 299), False)
    assert torch.equal(got.cpu().view(torch.int32), _nhwc(x).view(torch.int32))
    # ... and into a slice: the entry point with its own leading dimension writes the C channels only
    out = Sliced((2, 299, 299, C), C + 3, 2)
    assert hip_lib.mtd_resize_bilinear(x.cuda().data_ptr(), C * 299 * 299, 299 * 299, 1, out.view.data_ptr(), C + 3, 2, C, 299, 299, 299, 299, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.value().view(torch.int32), _nhwc(x).view(torch.int32)) and out.guards_kept()


# ------------------------------------------------------------------------------------------------------------- pools
def _pool_ref(x, mode):
    if mode == 0:
        return F.max_pool2d(x, 3, stride=2)
    if mode == 1:
        return F.max_pool2d(x, 3, stride=1, padding=1)
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


def _pool_case(mode, side, C, ld_in, ld_out, off):
    from mtd_gan_amd import inception as I
    x = _randn(2, C, side, side, seed=100 * mode + side + C)
    ref64 = _pool_ref(x.double(), mode)
    oh = ref64.shape[2]
    src = Sliced((2, side, side, C), ld_in, off, _nhwc(x))
    dst = Sliced((2, oh, oh, C), ld_out, off)
    I.pool3x3(src.view, mode, dst.view)
    torch.cuda.synchronize()
    got = _nchw(dst.value())
    assert src.guards_kept() and dst.guards_kept()
    if mode == 2:
        bound, e_ref = _bound(_pool_ref(x, mode), ref64)
        e = rel(got, ref64)
        print(f"avg pool {side}^2 C={C}: rel {e:.3e}, torch fp32 {e_ref:.3e}, bound {bound:.3e}")
        assert e <= bound
    else:
        assert torch.equal(got, ref64.float())


@pytest.mark.parametrize("C", [32, 288])
@pytest.mark.parametrize("side", [8, 9, 17])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pool3x3_in_slices(hip_lib, mode, side, C):
    _pool_case(mode, side, C, C + 8, C + 12, 4)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pool3x3_value_by_value(hip_lib, mode):
    _pool_case(mode, 9, 6, 9, 11, 1)             # strides and channel count that rule the 16-byte form out


def test_pool3x3_padding(hip_lib):
    """The average divides by the taps inside the image (4 in a corner, 6 on an edge): a map of ones stays ones; and the padding
    of the stride-1 max pool never wins: a map of negative values keeps its own maximum."""
    from mtd_gan_amd import inception as I
    ones = torch.ones(2, 9, 9, 32).cuda()
    assert (I.pool3x3(ones, I.POOL_AVG_S1P1) == 1.0).all()
    ramp = torch.arange(81.0).reshape(1, 9, 9, 1).repeat(1, 1, 1, 4).cuda()
    got = I.pool3x3(ramp, I.POOL_AVG_S1P1).cpu()
    assert got[0, 0, 0, 0].item() == (0 + 1 + 9 + 10) / 4 and got[0, 0, 4, 0].item() == (3 + 4 + 5 + 12 + 13 + 14) / 6
    neg = (-1.0 - torch.rand(1, 8, 8, 32, generator=torch.Generator().manual_seed(3)))
    got = I.pool3x3(neg.cuda(), I.POOL_MAX_S1P1).cpu()
    assert (got < 0).all() and torch.equal(_nchw(got), F.max_pool2d(_nchw(neg), 3, stride=1, padding=1))


@pytest.mark.parametrize("hw", [(8, 8), (3, 5)])
def test_global_avgpool(hip_lib, hw):
    from mtd_gan_amd import inception as I
    C = 288
    x = _randn(2, C, *hw, seed=hw[1])
    ref64 = x.double().mean(dim=(2, 3))
    bound, e_ref = _bound(x.mean(dim=(2, 3)), ref64)
    src = Sliced((2, hw[0], hw[1], C), C + 8, 4, _nhwc(x))
    got = I.global_avgpool(src.view)
    e = rel(got.cpu(), ref64)
    print(f"global pool {hw}: rel {e:.3e}, torch fp32 {e_ref:.3e}, bound {bound:.3e}")
    assert tuple(got.shape) == (2, C) and e <= bound and src.guards_kept()
    # the same bits from a contiguous copy of the slice (the order of the sum is one thread's own: nothing depends on the layout or the grid)
    assert torch.equal(I.global_avgpool(src.view.contiguous()), got)


# ---------------------------------------------------------------------------------------------------- conv geometries
def _geo(id, k, s, p, C, N, hw, B=2, real=None):
    """real: the channels that carry data; the rest of C are the zero lanes of a padded 48 / 80 channel map."""
    return pytest.param(dict(k=k, s=s, p=p, C=C, N=N, hw=hw, B=B, real=real or C), id=id)


GEOMETRIES = [
    _geo("1x7_p03_128_17x17", (1, 7), (1, 1), (0, 3), 128, 128, (17, 17), B=1),
    _geo("7x1_p30_128_17x17", (7, 1), (1, 1), (3, 0), 128, 128, (17, 17), B=1),
    _geo("1x7_p03_160to192_7x7", (1, 7), (1, 1), (0, 3), 160, 192, (7, 7), B=1),
    _geo("5x5_p2_48of64_9x9", (5, 5), (1, 1), (2, 2), 64, 64, (9, 9), real=48),
    _geo("3x3_s2_288to384_9x9", (3, 3), (2, 2), (0, 0), 288, 384, (9, 9)),
    _geo("3x3_s2_288to384_8x8", (3, 3), (2, 2), (0, 0), 288, 384, (8, 8)),
    _geo("1x3_p01_384_8x8", (1, 3), (1, 1), (0, 1), 384, 384, (8, 8)),
    _geo("3x1_p10_384_8x8", (3, 1), (1, 1), (1, 0), 384, 384, (8, 8)),
    _geo("3x3_p0_80of96to192_9x9", (3, 3), (1, 1), (0, 0), 96, 192, (9, 9), real=80),
    _geo("first_3x3_s2_1to32_19x19", (3, 3), (2, 2), (0, 0), 1, 32, (19, 19)),
    _geo("first_3x3_s2_3to32_19x19", (3, 3), (2, 2), (0, 0), 3, 32, (19, 19)),
]


@pytest.mark.parametrize("g", GEOMETRIES)
def test_conv_geometry(hip_lib, g):
    from mtd_gan_amd import inception as I
    B, C, N, (H, W), real = g["B"], g["C"], g["N"], g["hw"], g["real"]
    kh, kw = g["k"]
    seed = 7 * C + N + 31 * kh + kw + H
    x = _randn(B, real, H, W, seed=seed)
    w = _randn(N, real, kh, kw, seed=seed + 1) * (2.0 / (real * kh * kw)) ** 0.5
    bias = 0.1 * _randn(N, seed=seed + 2)
    ref64 = F.relu(F.conv2d(x.double(), w.double(), bias.double(), stride=g["s"], padding=g["p"]))
    bound, e_ref = _bound(F.relu(F.conv2d(x, w, bias, stride=g["s"], padding=g["p"])), ref64)
    xp, wp = torch.zeros(B, C, H, W), torch.zeros(N, C, kh, kw)
    xp[:, :real], wp[:, :real] = x, w
    small = C < 32
    src = Sliced((B, H, W, C), C + (5 if small else 8), 2 if small else 4, _nhwc(xp))
    dst = Sliced((B,) + tuple(ref64.shape[2:]) + (N,), N + 8, 4)
    parts = [(t.cuda(), rows) for t, rows in I.split_taps(wp)]
    assert len(parts) == (2 if kh * kw > 16 else 1)
    I.conv_relu(src.view, parts, bias.cuda(), g["k"], g["s"], g["p"], dst.view)
    torch.cuda.synchronize()
    e = rel(_nchw(dst.value()), ref64)
    print(f"conv {g['k']} s{g['s']} p{g['p']} {C}->{N} on {H}x{W}: rel {e:.3e}, torch fp32 {e_ref:.3e}, bound {bound:.3e}")
    assert e <= bound
    assert src.guards_kept() and dst.guards_kept()


def test_shapes_that_do_not_fit_are_refused(hip_lib):
    """Nothing is launched into an output of another shape, or from a map of another channel count."""
    from mtd_gan_amd import inception as I
    x = torch.zeros(1, 9, 9, 32).cuda()
    parts = I.split_taps(torch.zeros(64, 32, 3, 3).cuda())
    bias = torch.zeros(64).cuda()
    for out in (torch.zeros(1, 9, 9, 64), torch.zeros(1, 7, 7, 32), torch.zeros(2, 7, 7, 64)):
        with pytest.raises(ValueError):
            I.conv_relu(x, parts, bias, (3, 3), (1, 1), (0, 0), out.cuda())
    with pytest.raises(ValueError):
        I.conv_relu(torch.zeros(1, 9, 9, 64).cuda(), parts, bias, (3, 3), (1, 1), (0, 0))
    with pytest.raises(ValueError):
        I.pool3x3(x, I.POOL_MAX_S2, torch.zeros(1, 9, 9, 32).cuda())
    with pytest.raises(ValueError):
        I.pool3x3(x, I.POOL_AVG_S1P1, torch.zeros(1, 9, 9, 64).cuda()[:, :, :, :16])
    assert tuple(I.conv_relu(x, parts, bias, (3, 3), (1, 1), (0, 0)).shape) == (1, 7, 7, 64)


# ------------------------------------------------------------------------------------------------- blocks and network
@pytest.fixture(scope="module")
def state():
    return R.seeded_state_dict(0)


@pytest.fixture(scope="module")
def net(hip_lib, state):
    from mtd_gan_amd.metrics import InceptionV3Features
    return InceptionV3Features(state)


@pytest.mark.parametrize("name,side", [("Mixed_5b", 5), ("Mixed_6a", 5), ("Mixed_6c", 7), ("Mixed_7a", 7), ("Mixed_7b", 3), ("Mixed_7c", 3)])
def test_block(net, state, name, side):
    from mtd_gan_amd import inception as I
    cin = I.BLOCKS[name][0]
    x = _randn(2, cin, side, side, seed=cin + side)
    ref64 = R.block(state, name, x.double())
    bound, e_ref = _bound(R.block(state, name, x), ref64)
    got = net.run_block(name, _nhwc(x).cuda())
    assert tuple(got.shape) == (2,) + tuple(ref64.shape[2:]) + (R.WIDTHS[name],)
    e = rel(_nchw(got.cpu()), ref64)
    print(f"block {name} on {side}x{side}: rel {e:.3e}, torch fp32 {e_ref:.3e}, bound {bound:.3e}")
    assert e <= bound


@pytest.fixture(scope="module")
def whole(net, state):
    """The two inputs of the whole-network tests, their float64 features by the restatement (computed once, shared, never
    modified) and the bound from the restatement's own fp32 run."""
    g = torch.Generator().manual_seed(21)
    x1 = torch.rand(2, 1, 64, 64, generator=g)
    x3 = torch.rand(2, 3, 64, 64, generator=g)
    both = torch.cat([x1.repeat(1, 3, 1, 1), x3])
    ref64 = R.features(state, both.double())
    ref32 = R.features(state, both)
    bound, e_ref = _bound(ref32, ref64)
    print(f"whole network: restatement fp32 vs float64 rel {e_ref:.3e}, bound {bound:.3e}")
    return dict(x1=x1, x3=x3, ref1=ref64[:2], ref3=ref64[2:], bound=bound)


def test_whole_network(net, whole):
    one = net(whole["x1"].cuda())
    rep = net(whole["x1"].repeat(1, 3, 1, 1).cuda())
    three = net(whole["x3"].cuda())
    assert all(tuple(t.shape) == (2, 2048) and t.dtype == torch.float32 and torch.isfinite(t).all() for t in (one, rep, three))
    e1, er, e3, ex = rel(one, whole["ref1"]), rel(rep, whole["ref1"]), rel(three, whole["ref3"]), rel(one, rep)
    print(f"whole network, HIP vs float64: 1 channel {e1:.3e}, repeated to 3 {er:.3e}, 3 channels {e3:.3e}; 1 vs repeated {ex:.3e}; bound {whole['bound']:.3e}")
    assert max(e1, er, e3) <= whole["bound"]
    assert ex <= whole["bound"]
    assert whole["ref3"].std(dim=0).mean().item() > 0 and (whole["ref1"] - whole["ref3"]).abs().max().item() > 1e-3      # (the features tell inputs apart)


def test_chunking(net, whole, monkeypatch):
    """A per-launch cap of one image's largest map: a batch of 3 runs as three chunks.  Every chunk gives the bits of the same
    image run alone (a chunk's launches depend on nothing outside it), and the chunked batch agrees with the batch run as ONE chunk
    within twice the network bound (both are within it of the float64 features).  Bit equality with the one-chunk batch is not
    asserted: the implicit GEMM plans its split of K from the pixels of the launch, batch included, so a batch of 3 and three
    batches of 1 sum in different orders (printed)."""
    from mtd_gan_amd import inception as I
    x = torch.cat([whole["x1"], whole["x3"][:1, :1]]).cuda()
    whole_batch = net(x)
    alone = torch.cat([net(x[i:i + 1]) for i in range(3)])
    calls = []
    chunk = net._chunk
    monkeypatch.setattr(net, "_chunk", lambda t, side: (calls.append(t.shape[0]), chunk(t, side))[1])
    monkeypatch.setattr(I, "_MAX_MAP_BYTES", I.InceptionV3Features._largest_map_bytes((299, 299)))
    chunked = net(x)
    assert calls == [1, 1, 1]
    assert torch.equal(chunked.view(torch.int32), alone.view(torch.int32))
    e = rel(chunked, whole_batch)
    print(f"chunked vs one chunk of 3: rel {e:.3e}, same bits: {torch.equal(chunked, whole_batch)}")
    assert e <= 2 * whole["bound"]
    monkeypatch.setattr(I, "_MAX_MAP_BYTES", I.InceptionV3Features._largest_map_bytes((299, 299)) - 1)
    with pytest.raises(ValueError):
        net(x)


def test_without_resize_and_normalize(net, state):
    """resize_input=False / normalize_input=False: the image goes in as it is (here 75 x 80, the smallest height that reaches the
    last block)."""
    from mtd_gan_amd.metrics import InceptionV3Features
    raw = InceptionV3Features(state, resize_input=False, normalize_input=False)
    x = 2 * torch.rand(1, 3, 75, 80, generator=torch.Generator().manual_seed(2)) - 1
    ref64 = R.features(state, x.double(), resize_input=False, normalize_input=False)
    bound, e_ref = _bound(R.features(state, x, resize_input=False, normalize_input=False), ref64)
    e = rel(raw(x.cuda()), ref64)
    print(f"75 x 80 as it is: rel {e:.3e}, torch fp32 {e_ref:.3e}, bound {bound:.3e}")
    assert e <= bound
    with pytest.raises(ValueError):
        raw(torch.zeros(1, 3, 74, 80).cuda())


# ------------------------------------------------------------------------------------------------------------- engine
def test_test_loop_with_the_network(net, tmp_path):
    from mtd_gan_amd import engine, kernels as K, metrics as M
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    torch.manual_seed(3)
    m = MTD_GAN_Method().cuda()
    m.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    xs, ys = orc.synthetic_ldct(3, seed=9, size=64)
    loader = [dict(n_20=xs[i:i + 1], n_100=ys[i:i + 1], path_n_20=[f"L000_000{i}.dcm"], path_n_100=[f"L000_000{i}.dcm"]) for i in range(3)]
    dev = torch.device("cuda")
    plain = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, None)
    pixel_keys = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in ("input", "gt", "pred")]
    assert list(plain.keys()) == pixel_keys

    m.fid_features = net
    full = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, str(tmp_path / "fid"))
    assert list(full.keys()) == pixel_keys + ["input_fid", "gt_fid", "pred_fid"]
    assert all(full[k] == plain[k] for k in pixel_keys)
    with torch.no_grad():
        pred = torch.cat([K.clip01(m.Generator(xs[i:i + 1].cuda()).contiguous()) for i in range(3)])
    feats = [torch.cat([net(t[i:i + 1]) for i in range(3)]) for t in (xs.cuda(), ys.cuda(), pred)]       # slice by slice, as the loop does
    assert all(tuple(f.shape) == (3, 2048) for f in feats)
    triple = torch.stack(M.compute_FID(*feats)).tolist()
    print("FID of three 64 x 64 slices (input, gt, pred):", triple)
    for who, v in zip(("input", "gt", "pred"), triple):
        assert v == v and abs(v) != float("inf")
        assert full[f"{who}_fid"] == round(v, 7)
