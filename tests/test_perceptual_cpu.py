"""Host side of the perceptual metrics (metrics.VGG19Features / compute_PL / compute_TML) without a GPU, and the sanity of the
plain-torch restatement the GPU parity tests compare against."""
import pytest
import torch

import _perceptual_ref as R
import mtdgan_oracle as orc


def test_state_dict_validation_names_the_key():
    from mtd_gan_amd.metrics import VGG19Features
    sd = R.seeded_state_dict(1)
    VGG19Features(sd)                                   # complete: accepted, classifier.* ignored
    missing = {k: v for k, v in sd.items() if k != "features.14.bias"}
    with pytest.raises(ValueError, match=r"features\.14\.bias"):
        VGG19Features(missing)
    wrong = dict(sd)
    wrong["features.19.weight"] = torch.zeros(512, 128, 3, 3)
    with pytest.raises(ValueError, match=r"features\.19\.weight"):
        VGG19Features(wrong)


def test_state_dict_from_a_file(tmp_path):
    from mtd_gan_amd.metrics import VGG19Features
    sd = R.seeded_state_dict(2)
    path = tmp_path / "vgg19.pth"
    torch.save(sd, path)
    v = VGG19Features(str(path))
    assert torch.equal(v.layers[3][1], sd["features.7.weight"]) and torch.equal(v.layers[3][2], sd["features.7.bias"])


def test_first_layer_is_folded_to_one_channel():
    from mtd_gan_amd.metrics import VGG19Features
    sd = R.seeded_state_dict(3)
    v = VGG19Features(sd)
    idx, w, b = v.layers[0]
    assert idx == 0 and tuple(w.shape) == (64, 1, 3, 3) and w.dtype == torch.float32
    assert torch.equal(w, sd["features.0.weight"].double().sum(dim=1, keepdim=True).float())
    assert torch.equal(b, sd["features.0.bias"])
    assert [tuple(l[1].shape[:2]) for l in v.layers[1:]] == [(co, ci) for _, ci, co in R.CONVS[1:]]
    # ... which is the same network on a repeated single-channel image
    x = orc.synthetic_ldct(1, seed=4, size=32)[0].double()
    three = torch.nn.functional.conv2d(x.repeat(1, 3, 1, 1), sd["features.0.weight"].double(), padding=1)
    one = torch.nn.functional.conv2d(x, w.double(), padding=1)
    assert (three - one).abs().max().item() < 1e-6


def test_restatement_shapes_and_zero_distance():
    sd = R.seeded_state_dict(0)
    x, y = orc.synthetic_ldct(1, seed=5, size=48)
    x, y = x[:, :, :, :40], y[:, :, :, :40]
    fx, fy = R.features(sd, x), R.features(sd, y)
    assert [tuple(f.shape) for f in fx] == [(1, 64, 48, 40), (1, 128, 24, 20), (1, 256, 12, 10), (1, 512, 6, 5), (1, 512, 3, 2)]
    assert all(f.dtype == torch.float64 and (f >= 0).all() for f in fx)
    assert R.pl(fx, fx).item() == 0.0 and R.pl(fx, fy).item() > 0.0
    big = [torch.relu(torch.randn(2, 8, 32, 48, dtype=torch.float64, generator=torch.Generator().manual_seed(i))) for i in range(5)]
    assert R.tml(big, big).item() == 0.0
    assert R.tml(big, [b.flip(0) for b in big]).item() > 0.0


def test_restatement_patch_count():
    f = torch.arange(37 * 50, dtype=torch.float64).reshape(1, 1, 37, 50)
    p = R.patches(f)
    assert tuple(p.shape) == (2 * 3, 1, 256)
    assert torch.equal(p[4, 0].reshape(16, 16), f[0, 0, 16:32, 16:32])          # patch (1, 1): row-major over (ph, pw)
    assert tuple(R.gram(torch.zeros(2, 4, 37, 50)).shape) == (12, 4, 4)


def test_cpu_tensors_are_refused():
    from mtd_gan_amd import metrics as M
    v = M.VGG19Features(R.seeded_state_dict(1))
    x = torch.zeros(1, 1, 256, 256)
    for fn in (M.compute_PL, M.compute_TML):
        with pytest.raises(RuntimeError):
            fn(x, x, x, vgg=v)
    with pytest.raises(RuntimeError):
        v(x)
    with pytest.raises(TypeError):
        M.compute_PL(x, x, x, vgg=None)


def test_new_entry_points_are_bound():
    from mtd_gan_amd import _lib
    assert all(n in _lib.EXPORTS for n in ("mtd_maxpool2x2", "mtd_patch_gram_l1_ws_bytes", "mtd_patch_gram_l1", "mtd_scaled_sums_f64"))
