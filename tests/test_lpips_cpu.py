"""LPIPS and DISTS without a GPU: the restatement of tests/_lpips_ref.py against what the reference's own
module/piq/perceptual.py computed (tests/golden/lpips_dists_piq.npz, written by tools/pin_lpips.py), the seeded inputs and
weights behind the fixture, the host side of metrics.VGG16Features (the exactly folded first layer, also on the border rows and
columns; the refusals), the two weight loaders, the test loop's option checks, and the argument refusals of the entry points
that need no device (through the built library's ABI, with addresses of host memory)."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _lpips_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def meta(golden):
    return json.loads(str(golden["meta"]))


@pytest.fixture(scope="module")
def seeded():
    return R.seeded_state_dict(), R.seeded_lpips_weights(), R.seeded_dists_weights()


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from mtd_gan_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def restated(seeded):
    """Per case and dtype: (lpips (3, B), lpips parts (3, B, 5), dists (3, B), dists parts (3, B, 6)) of the restatement; computed
    once and shared."""
    sd, lw, dw = seeded
    out = {}
    with torch.no_grad():
        for index, (_, _, _, distance) in enumerate(R.CASES):
            x, y, pred = R.case_inputs(index)
            for dtype in (torch.float64, torch.float32):
                ls = [R.lpips(sd, lw, a, y, distance, dtype) for a in (x, y, pred)]
                ds = [R.dists(sd, dw, a, y, dtype) for a in (x, y, pred)]
                out[index, dtype] = tuple(torch.stack([v[j] for v in vs]).double().numpy() for vs in (ls, ds) for j in (0, 1))
    return out


def test_fixture_meta_and_seeded_crcs(golden, meta, seeded):
    sd, lw, dw = seeded
    assert meta["cases"] == [list(c) for c in R.CASES]
    assert int(golden["crc_vgg16"]) == R.crc(*[sd[k] for k in sorted(sd)])
    assert int(golden["crc_lpips_weights"]) == R.crc(*lw)
    assert int(golden["crc_dists_weights"]) == R.crc(dw["alpha"], dw["beta"])
    assert all((w >= 0).all() for w in lw)
    assert abs(float(dw["alpha"].double().sum() + dw["beta"].double().sum()) - 1.0) < 1e-6
    assert 0 < meta["spread"]["lpips_rel"] < 1e-5 and 0 < meta["spread"]["dists_abs"] < 1e-5


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_input_crcs(golden, index):
    assert int(golden[f"crc_{index}"]) == R.crc(*R.case_inputs(index))


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_float64_restatement_agrees_with_the_reference(golden, restated, index):
    ls, lp, ds, dp = restated[index, torch.float64]
    for name, got in (("lpips", ls), ("lpips_parts", lp), ("dists", ds), ("dists_parts", dp)):
        want = golden[f"{name}64_{index}"]
        err = float(np.max(np.abs(got - want)))
        print(f"case {index} {name}: largest distance to the reference's float64 {err:.3e}")
        assert got.shape == want.shape and err < 1e-12, (name, err)
    assert (ls[1] == 0).all()


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_float32_restatement_stays_within_the_recorded_spread(golden, meta, restated, index):
    """The restatement's float32 run is another float32 evaluation order of the same formulas: it may stray from float64 as far
    as the reference's own float32 run did (meta's spread, the largest over the cases), times 4 for the other order."""
    ls, _, ds, _ = restated[index, torch.float32]
    l64, d64 = golden[f"lpips64_{index}"], golden[f"dists64_{index}"]
    rel = float(np.max(np.abs(ls[[0, 2]] - l64[[0, 2]]) / l64[[0, 2]]))
    ab = float(np.max(np.abs(ds - d64)))
    print(f"case {index}: float32 restatement lpips rel {rel:.3e} dists abs {ab:.3e}")
    assert rel <= 4 * meta["spread"]["lpips_rel"] and ab <= 4 * meta["spread"]["dists_abs"]


def test_gt_rows_of_the_fixture(golden, meta):
    for index in range(len(R.CASES)):
        assert (golden[f"lpips64_{index}"][1] == 0).all() and (golden[f"lpips32_{index}"][1] == 0).all()
        assert np.max(np.abs(golden[f"dists64_{index}"][1] - meta["gt_dists"])) < 1e-6
        assert (golden[f"lpips64_{index}"][[0, 2]] > 0).all()


# ---------------------------------------------------------------------------------------------- VGG16Features on the host
def test_folded_first_layer_equals_the_normalised_conv_also_on_the_border(seeded):
    from mtd_gan_amd import metrics as M
    sd = seeded[0]
    w, b = sd["features.0.weight"].double(), sd["features.0.bias"].double()
    folded = M.vgg16_first_layer(sd["features.0.weight"])
    assert folded.dtype == torch.float64 and tuple(folded.shape) == (64, 2, 3, 3)
    x = R.case_inputs(1)[0].double()                                         # (1, 1, 50, 37)
    want = F.conv2d(R.normalised(x), w, b, padding=1)
    got = F.conv2d(torch.cat([x, torch.ones_like(x)], dim=1), folded, b, padding=1)
    ring = torch.ones(want.shape[-2:], dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    assert float((got - want).abs().max()) < 1e-12 and float((got - want)[..., ring].abs().max()) < 1e-12
    # what folding the mean into the bias would give: right inside, wrong on the ring
    as_bias = F.conv2d(x, folded[:, :1], b + folded[:, 1].sum(dim=(1, 2)), padding=1)
    assert float((as_bias - want)[..., ~ring].abs().max()) < 1e-12 and float((as_bias - want)[..., ring].abs().max()) > 1e-3


def test_vgg16_features_layers_and_refusals(seeded):
    from mtd_gan_amd import metrics as M
    sd = seeded[0]
    net = M.VGG16Features(sd)
    assert [i for i, _, _ in net.layers] == [i for i, _, _ in R.CONVS]
    assert tuple(net.layers[0][1].shape) == (64, 2, 3, 3) and all(w.dtype == torch.float32 and w.is_contiguous() for _, w, _ in net.layers)
    assert torch.equal(net.layers[1][1], sd["features.2.weight"])
    assert M._VGG16_TAPS == R.TAPS and M._VGG16_POOL_AFTER == tuple(p - 1 for p in R.POOLS)
    missing = {k: v for k, v in sd.items() if k != "features.17.bias"}
    with pytest.raises(ValueError, match="features.17.bias"):
        M.VGG16Features(missing)
    wrong = dict(sd)
    wrong["features.10.weight"] = torch.zeros(256, 128, 3, 2)
    with pytest.raises(ValueError, match=r"features.10.weight.*\(256, 128, 3, 2\)"):
        M.VGG16Features(wrong)
    with pytest.raises(ValueError):
        M.VGG16Features(sd, std=(0.2, 0.0, 0.2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 1, 16, 16))
    with pytest.raises(ValueError, match="pool"):
        net(torch.zeros(1, 1, 16, 16), pool="avg")
    # VGG-19's table is untouched by the shared walk
    assert M._VGG19_TAPS == (1, 6, 11, 20, 29) and M._VGG19_POOL_AFTER == (3, 8, 17, 26)


def test_weight_loaders(seeded, tmp_path):
    from mtd_gan_amd import metrics as M
    _, lw, dw = seeded
    t = M.lpips_weights(lw)
    assert t.dtype == torch.float64 and tuple(t.shape) == (1472,) and t.is_contiguous()
    assert torch.equal(t, torch.cat([w.double().flatten() for w in lw]))
    assert M.lpips_weights(tuple(w.flatten() for w in lw)).equal(t) and M.lpips_weights(t) is not None and M.lpips_weights(t).equal(t)
    torch.save(lw, tmp_path / "lpips.pt")
    assert M.lpips_weights(str(tmp_path / "lpips.pt")).equal(t)
    for bad in (lw[:4], lw + [lw[0]], [lw[0], lw[1], lw[2], lw[3], lw[3][:, :100]], {"alpha": 1}, 3.0, [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError, match="lpips_weights"):
            M.lpips_weights(bad)
    with pytest.raises(ValueError, match=r"\(1, 100, 1, 1\)"):
        M.lpips_weights([lw[0], lw[1], lw[2], lw[3], lw[3][:, :100]])
    d = M.dists_weights(dw)
    assert d.dtype == torch.float64 and tuple(d.shape) == (2, 1475) and d.is_contiguous()
    assert torch.equal(d[0], dw["alpha"].double().flatten()) and torch.equal(d[1], dw["beta"].double().flatten())
    assert M.dists_weights({"alpha": dw["alpha"].flatten(), "beta": dw["beta"].flatten(), "other": 1}).equal(d) and M.dists_weights(d).equal(d)
    torch.save(dw, tmp_path / "dists.pt")
    assert M.dists_weights(str(tmp_path / "dists.pt")).equal(d)
    for bad in ({"alpha": dw["alpha"]}, {"alpha": dw["alpha"], "beta": dw["beta"][:, :1474]}, lw, 1.0):
        with pytest.raises(ValueError, match="dists_weights"):
            M.dists_weights(bad)
    with pytest.raises(ValueError, match=r"\(1, 1474, 1, 1\)"):
        M.dists_weights({"alpha": dw["alpha"], "beta": dw["beta"][:, :1474]})


# ---------------------------------------------------------------------------------------------- the test loop's options
class _NoLoader:
    def __iter__(self):
        raise AssertionError("the loader was touched before the option check")


def test_engine_option_values(seeded):
    from mtd_gan_amd import engine, metrics as M
    sd, lw, dw = seeded
    net = M.VGG16Features(sd)
    lp = lambda **kw: engine._lpips_option(types.SimpleNamespace(**kw))          # noqa: E731
    di = lambda **kw: engine._dists_option(types.SimpleNamespace(**kw))          # noqa: E731
    for off in (dict(), dict(test_lpips=None), dict(test_lpips=False), dict(test_lpips={}), dict(test_dists=None), dict(test_dists=False)):
        assert lp(**off) is None and di(**off) is None
    got = lp(test_lpips=lw, perceptual_vgg16=net)
    assert got["vgg"] is net and got["distance"] == "mse" and got["weights"].equal(M.lpips_weights(lw))
    got = lp(test_lpips=dict(weights=lw, distance="mae"), perceptual_vgg16=net)
    assert got["distance"] == "mae" and set(got) == {"vgg", "weights", "distance"}
    got = di(test_dists=dw, perceptual_vgg16=net)
    assert got["vgg"] is net and got["weights"].equal(M.dists_weights(dw)) and set(got) == {"vgg", "weights"}
    assert lp(test_dists=dw, perceptual_vgg16=net) is None and di(test_lpips=lw, perceptual_vgg16=net) is None      # they do not see each other




@pytest.mark.parametrize("which", ("lpips", "dists"))
def test_engine_refuses_bad_options_before_anything_runs(seeded, which):
    from mtd_gan_amd import engine, metrics as M
    sd, lw, dw = seeded
    net = M.VGG16Features(sd)
    good = lw if which == "lpips" else dw
    bad = [True, 5, "no/such/file.pt", dw if which == "lpips" else lw]
    if which == "lpips":
        bad += [dict(weights=lw, distance="l2"), dict(weights=lw, p=1), dict(distance="mae"), lw[:3]]
    else:
        bad += [dict(alpha=dw["alpha"]), dict(alpha=dw["alpha"], beta=dw["beta"][:, :10])]
    for value in bad:
        model = types.SimpleNamespace(perceptual_vgg16=net, **{f"test_{which}": value})       # no Generator: anything past the check would fail
        with pytest.raises(ValueError, match=f"test_{which}"):
            engine.test_MTD_GAN_Ours(model, None, _NoLoader(), torch.device("cpu"), None)
    for vgg in (None, M.VGG19Features, object()):
        model = types.SimpleNamespace(perceptual_vgg16=vgg, **{f"test_{which}": good})
        with pytest.raises(ValueError, match=f"test_{which} needs model.perceptual_vgg16"):
            engine.test_MTD_GAN_Ours(model, None, _NoLoader(), torch.device("cpu"), None)
    model = types.SimpleNamespace(**{f"test_{which}": good})                                   # the attribute absent altogether
    with pytest.raises(ValueError, match="perceptual_vgg16"):
        engine.test_MTD_GAN_Ours(model, None, _NoLoader(), torch.device("cpu"), None)


# ---------------------------------------------------------------------------------------------- the entry points' refusals
def test_header_declares_and_lib_binds_the_entry_points(built_lib):
    from mtd_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "mtdgan_hip.h")).read()
    names = ("mtd_l2pool3x3s2", "mtd_lpips_level_ws_bytes", "mtd_lpips_level_each", "mtd_scaled_sums_f64_f64", "mtd_channel_moments_ws_bytes",
             "mtd_channel_moments_each", "mtd_dists_finish")
    for n in names:
        assert re.search(r"^(size_t|int) %s\(" % n, header, re.M), n
        assert n in _lib.EXPORTS and len(getattr(built_lib, n).argtypes) > 0, n
    assert len(built_lib.mtd_lpips_level_each.argtypes) == 14 and len(built_lib.mtd_channel_moments_each.argtypes) == 10
    for name, value in (("MTD_L2POOL_MAX_BLOCKS", 2048), ("MTD_LPIPS_MAX_BLOCKS", 1024), ("MTD_MOMENTS_MAX_RANGES", 256), ("MTD_MOMENTS_WALK", 32),
                        ("MTD_DISTS_LEVELS", 6), ("MTD_DISTS_WEIGHTS", 1475)):
        assert re.search(r"^#define %s %d$" % (name, value), header, re.M), name
    from mtd_gan_amd import _build
    assert "lpips.hip" in _build.SOURCES


def test_entry_points_refuse_bad_arguments_without_a_device(built_lib):
    """Every refusal below happens before a launch, so host addresses stand in for the device pointers."""
    L = built_lib
    EINVAL = -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    p = (p + 15) & ~15                                                               # (16-byte aligned inside the buffer)
    assert L.mtd_l2pool3x3s2(None, p, 1, 4, 4, 64, None) == EINVAL and L.mtd_l2pool3x3s2(p, None, 1, 4, 4, 64, None) == EINVAL
    for B, H, W, C in ((1, 4, 4, 6), (1, 4, 4, 0), (0, 4, 4, 64), (1, 0, 4, 64), (1, 4, 0, 64)):
        assert L.mtd_l2pool3x3s2(p, p, B, H, W, C, None) == EINVAL, (B, H, W, C)
    # LPIPS level: 15 pixels at C = 64 are one workgroup round of 16 pixels: one partial per (other, image)
    assert L.mtd_lpips_level_ws_bytes(2, 3, 5, 64) == 2 * 2 * 1 * 8
    assert L.mtd_lpips_level_ws_bytes(1, 130, 127, 64) == 2 * 1024 * 8              # capped at MTD_LPIPS_MAX_BLOCKS
    for C in (0, 3, 32, 96, 1024):
        assert L.mtd_lpips_level_ws_bytes(1, 4, 4, C) == 0
        assert L.mtd_lpips_level_each(p, p, p, 1, 4, 4, C, p, 0, p, 1, 1, p, None) == EINVAL, C
    assert L.mtd_lpips_level_ws_bytes(0, 4, 4, 64) == 0 and L.mtd_lpips_level_ws_bytes(1, 0, 4, 64) == 0
    ok = dict(t=p, a=p, b=p, B=1, h=4, w=4, C=64, weights=p, distance=0, out=p, out_stride=1, other_stride=1, ws=p, stream=None)
    for change in (dict(t=None), dict(a=None), dict(weights=None), dict(out=None), dict(ws=None), dict(distance=2), dict(distance=-1),
                   dict(out_stride=0), dict(B=0), dict(h=0)):
        args = dict(ok, **change)
        assert L.mtd_lpips_level_each(*args.values()) == EINVAL, change
    # channel moments: C = 1 or a multiple of 4 up to 1024
    assert L.mtd_channel_moments_ws_bytes(2, 5, 7, 64, 2) == 2 * 1 * 8 * 64 * 8      # 35 pixels: one range
    assert L.mtd_channel_moments_ws_bytes(2, 24, 23, 64, 1) == 2 * 2 * 5 * 64 * 8    # 552 pixels, 16 pixel lanes x 32: two ranges
    assert L.mtd_channel_moments_ws_bytes(1, 5, 7, 1, 2) == 1 * 1 * 8 * 1 * 8
    for C in (0, 2, 3, 6, 1028):
        assert L.mtd_channel_moments_ws_bytes(1, 5, 7, C, 1) == 0
        assert L.mtd_channel_moments_each(p, p, None, 1, 5, 7, C, p, p, None) == EINVAL, C
    assert L.mtd_channel_moments_ws_bytes(1, 5, 7, 64, 0) == 0 and L.mtd_channel_moments_ws_bytes(1, 5, 7, 64, 3) == 0
    for args in ((None, p, None, 1, 5, 7, 64, p, p, None), (p, None, None, 1, 5, 7, 64, p, p, None), (p, p, None, 1, 5, 7, 64, None, p, None),
                 (p, p, None, 1, 5, 7, 64, p, None, None), (p, p, None, 0, 5, 7, 64, p, p, None)):
        assert L.mtd_channel_moments_each(*args) == EINVAL, args
    # DISTS finish
    tables = (ctypes.c_void_p * 6)(*([p] * 6))
    pixels = (ctypes.c_longlong * 6)(35, 35, 12, 4, 2, 1)
    for args in ((None, pixels, 2, 1, 1, p, p, p, None, None), (tables, None, 2, 1, 1, p, p, p, None, None), (tables, pixels, 0, 1, 1, p, p, p, None, None),
                 (tables, pixels, 3, 1, 1, p, p, p, None, None), (tables, pixels, 2, 0, 1, p, p, p, None, None), (tables, pixels, 2, 1, 3, p, p, p, None, None),
                 (tables, pixels, 2, 1, -2, p, p, p, None, None), (tables, pixels, 2, 1, 1, None, p, p, None, None), (tables, pixels, 2, 1, 1, p, None, p, None, None),
                 (tables, pixels, 2, 1, 1, p, p, None, None, None)):
        assert L.mtd_dists_finish(*args) == EINVAL, args
    pixels[3] = 0
    assert L.mtd_dists_finish(tables, pixels, 2, 1, 1, p, p, p, None, None) == EINVAL
    scales = (ctypes.c_double * 5)(1, 1, 1, 1, 1)
    assert L.mtd_scaled_sums_f64_f64(None, 1, 5, scales, p, None, None) == EINVAL and L.mtd_scaled_sums_f64_f64(p, 1, 9, scales, p, None, None) == EINVAL
