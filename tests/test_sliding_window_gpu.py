"""Sliding-window inference on the device (mtd_gan_amd/inferers.py, csrc/sliding_window.hip): the window gather and the
overlap blend against a float64 blend of the same window predictions, determinism, independence of the chunking, the
generators as predictors against the CPU oracle, and the evaluation loops with `Generator.sliding_window` set."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mtdgan_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
from _metrics import rel  # noqa: E402

from mtd_gan_amd.inferers import sliding_window_inference, window_starts  # noqa: E402

U = 2.0 ** -24


def _map64(roi, mode, sigma_scale=0.125):
    """The importance map of DESIGN 3.6's formula in float64, written out here (not the package's helper)."""
    if mode == "constant":
        return torch.ones(roi, dtype=torch.float64)
    axes = []
    for n in roi:
        t = torch.arange(n, dtype=torch.float64) - (n - 1) / 2.0
        axes.append(torch.exp(-t * t / (2.0 * (n * sigma_scale) ** 2)))
    m = torch.outer(axes[0], axes[1])
    return m.clamp(min=max(m[m != 0].min().item(), 1e-3))


def _blend64(preds, shape, roi, overlap, mode):
    """out[p] = sum_w m(p - s_w) pred_w(p - s_w) / sum_w m(p - s_w) as a plain loop over the windows (images outermost, y
    outer, x inner); preds: (B * ny * nx, 1, rh, rw) on the CPU.  Returns (out float64, k = most windows on one pixel)."""
    B, _, H, W = shape
    ys, xs = window_starts(H, roi[0], overlap), window_starts(W, roi[1], overlap)
    m = _map64(roi, mode)
    num = torch.zeros(B, 1, H, W, dtype=torch.float64)
    den = torch.zeros(B, 1, H, W, dtype=torch.float64)
    cnt = torch.zeros(H, W)
    assert preds.shape[0] == B * len(ys) * len(xs)
    w = 0
    for b in range(B):
        for y in ys:
            for x in xs:
                num[b, 0, y:y + roi[0], x:x + roi[1]] += m * preds[w, 0].double()
                den[b, 0, y:y + roi[0], x:x + roi[1]] += m
                if b == 0:
                    cnt[y:y + roi[0], x:x + roi[1]] += 1
                w += 1
    return num / den, int(cnt.max().item())


class _Recorder:
    """Wraps a predictor and keeps every chunk's output (the window predictions as the device produced them)."""

    def __init__(self, fn):
        self.fn, self.chunks = fn, []

    def __call__(self, w):
        out = self.fn(w)
        self.chunks.append(out.detach().cpu())
        return out

    def predictions(self):
        return torch.cat(self.chunks)


def _flip_predictor(w):
    return 2 * w + w.flip(-1)          # the flip makes a wrong window offset visible; the identity would hide it


def _input(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 0.25


CASES = [((2, 1, 80, 99), (64, 64), 0.3, 3),        # 2 x 2 windows per image, x starts [0, 35]; chunks 3 + 3 + 2 across the images
         ((1, 1, 70, 64), (64, 64), 0.9, 32),       # starts [0, 6] along y, one window along x
         ((1, 1, 64, 64), (64, 64), 0.25, 4),       # one window
         ((1, 1, 50, 70), (32, 48), 0.5, 4)]        # non-square roi


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
@pytest.mark.parametrize("shape,roi,overlap,sw_batch", CASES)
def test_blend_against_float64(hip_lib, shape, roi, overlap, sw_batch, mode):
    x = _input(shape, seed=sum(shape))
    rec = _Recorder(_flip_predictor)
    out = sliding_window_inference(x.cuda(), roi, sw_batch, rec, overlap=overlap, mode=mode)
    assert out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_cuda
    preds = rec.predictions()
    B, ny, nx = shape[0], len(window_starts(shape[2], roi[0], overlap)), len(window_starts(shape[3], roi[1], overlap))
    assert [c.shape[0] for c in rec.chunks] == [min(sw_batch, B * ny * nx - i) for i in range(0, B * ny * nx, sw_batch)]
    # the windows the predictor saw are the windows of the plan, in its order
    w = 0
    for b in range(B):
        for y in window_starts(shape[2], roi[0], overlap):
            for xs in window_starts(shape[3], roi[1], overlap):
                assert torch.equal(preds[w], _flip_predictor(x[b:b + 1, :, y:y + roi[0], xs:xs + roi[1]])[0]), (b, y, xs)
                w += 1
    ref, k = _blend64(preds, shape, roi, overlap, mode)
    bound = 2 * (k + 2) * U * preds.abs().max().item()
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"shape {shape} roi {roi} overlap {overlap} {mode}: k {k}, max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if B * ny * nx == 1:
        assert torch.equal(out.cpu(), preds)          # a single window: the predictor's output, bit for bit


def test_fused_clip_is_the_clamp_of_the_result(hip_lib):
    x = (_input((2, 1, 80, 99), seed=3) * 2).cuda()
    plain = sliding_window_inference(x, (64, 64), 3, _flip_predictor, overlap=0.3, mode="gaussian")
    clipped = sliding_window_inference(x, (64, 64), 3, _flip_predictor, overlap=0.3, mode="gaussian", clip=True)
    assert plain.min().item() < 0 and plain.max().item() > 1
    assert torch.equal(clipped, plain.clamp(0, 1))


def test_same_bits_every_run(hip_lib):
    x = _input((2, 1, 80, 99), seed=11).cuda()
    for mode in ("constant", "gaussian"):
        a = sliding_window_inference(x, (64, 64), 3, _flip_predictor, overlap=0.3, mode=mode)
        b = sliding_window_inference(x, (64, 64), 3, _flip_predictor, overlap=0.3, mode=mode)
        assert torch.equal(a, b), mode


@pytest.mark.parametrize("shape,overlap", [((2, 1, 80, 99), 0.3), ((1, 1, 100, 77), 0.9)])
def test_chunking_does_not_matter(hip_lib, shape, overlap):
    """(1, 1, 100, 77) at overlap 0.9: 7 x 4 windows, up to 28 on one pixel, chunks of 3 start in the middle of a window row."""
    x = _input(shape, seed=13).cuda()
    for mode in ("constant", "gaussian"):
        runs = [sliding_window_inference(x, (64, 64), n, _flip_predictor, overlap=overlap, mode=mode) for n in (1, 3, 1000)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), mode


def test_many_windows_per_pixel_against_float64(hip_lib):
    """Overlap 0.9 on both axes ((1, 1, 100, 77): 7 x 4 windows, 28 on the central pixels) -- the long sums of the timing tool's
    hardest setting at a size a test can afford."""
    shape, roi = (1, 1, 100, 77), (64, 64)
    x = _input(shape, seed=17)
    for mode in ("constant", "gaussian"):
        rec = _Recorder(_flip_predictor)
        out = sliding_window_inference(x.cuda(), roi, 5, rec, overlap=0.9, mode=mode)
        ref, k = _blend64(rec.predictions(), shape, roi, 0.9, mode)
        assert k == 28
        assert (out.cpu().double() - ref).abs().max().item() <= 2 * (k + 2) * U * rec.predictions().abs().max().item()


def _generator():
    from mtd_gan_amd.arch.Ours.networks import ResFFT_Generator
    g = orc.seeded_fill(orc.g_param_shapes(), seed=7)
    G = ResFFT_Generator(1, 32, 10, 3, 1)
    G.load_state_dict(g)
    return G.cuda().eval(), g


def _oracle_windows(forward, x, roi, overlap):
    """forward on every CPU window of x, in the plan's order."""
    out = []
    for b in range(x.shape[0]):
        for y in window_starts(x.shape[2], roi[0], overlap):
            for xs in window_starts(x.shape[3], roi[1], overlap):
                out.append(forward(x[b:b + 1, :, y:y + roi[0], xs:xs + roi[1]]))
    return torch.cat(out)


def test_generator_windowed_matches_oracle(hip_lib, monkeypatch):
    from mtd_gan_amd.arch.Ours.networks import ResFFT_Generator
    G, g = _generator()
    x, y = orc.synthetic_ldct(1, seed=5, size=96)
    assert window_starts(96, 64, 0.5) == [0, 32]
    with torch.no_grad():
        out = sliding_window_inference(x.cuda(), (64, 64), 4, G, overlap=0.5)
        ref, _ = _blend64(_oracle_windows(lambda w: orc.generator_forward(g, w), x, (64, 64), 0.5), x.shape, (64, 64), 0.5, "constant")
        monkeypatch.setattr(ResFFT_Generator, "allow_any_size", True)
        whole = G(x.cuda())
    ref = ref.float()
    assert rel(out.cpu(), ref) < 1e-3
    assert abs(orc.psnr(out.cpu().clip(0, 1), y).item() - orc.psnr(ref.clip(0, 1), y).item()) < 0.01
    assert rel(whole.cpu(), ref) > 1e-3          # the whole-slice pass computes something else: the windowed path really ran


def test_redcnn_generator_on_a_slice(hip_lib):
    from mtd_gan_amd.arch.Ours.networks import REDCNN_Generator
    R = REDCNN_Generator(1, 32, 10, 3, 1)
    R.load_state_dict(orc.seeded_fill({k: tuple(v.shape) for k, v in R.state_dict().items()}, seed=7))
    R.cuda().eval()
    x, _ = orc.synthetic_ldct(1, seed=9, size=96)
    x = x[:, :, :80, :].contiguous()
    assert tuple(x.shape) == (1, 1, 80, 96)
    rec = _Recorder(R)
    with torch.no_grad():
        out = sliding_window_inference(x.cuda(), (64, 64), 3, rec, overlap=0.5)
        with pytest.raises(NotImplementedError, match="64,64"):
            R(x.cuda())                       # without the attribute the module still takes patches only
    preds = rec.predictions()
    ref, k = _blend64(preds, x.shape, (64, 64), 0.5, "constant")
    assert (out.cpu().double() - ref).abs().max().item() <= 2 * (k + 2) * U * preds.abs().max().item()
    # and each window prediction is the oracle's RED-CNN on that window (the project's standing parity bound)
    st = {k: v.cpu() for k, v in R.state_dict().items()}
    assert rel(preds, _oracle_windows(lambda w: orc.redcnn_forward(st, w), x, (64, 64), 0.5)) < 1e-3


def test_redcnn_generator_attribute_routes_forward(hip_lib, monkeypatch):
    from mtd_gan_amd.arch.Ours.networks import REDCNN_Generator
    R = REDCNN_Generator(1, 32, 10, 3, 1)
    R.load_state_dict(orc.seeded_fill({k: tuple(v.shape) for k, v in R.state_dict().items()}, seed=7))
    R.cuda().eval()
    x = orc.synthetic_ldct(1, seed=9, size=96)[0][:, :, :80, :].contiguous().cuda()
    kw = dict(roi_size=(64, 64), sw_batch_size=3, overlap=0.5, mode="gaussian")
    monkeypatch.setattr(REDCNN_Generator, "sliding_window", kw)
    with torch.no_grad():
        assert torch.equal(R(x), sliding_window_inference(x, predictor=R, **kw))
        patch = x[:, :, :64, :64].contiguous()
        routed = R(patch)
    monkeypatch.setattr(REDCNN_Generator, "sliding_window", None)
    with torch.no_grad():
        assert torch.equal(routed, R(patch))          # a roi-sized input takes the usual path
    monkeypatch.setattr(REDCNN_Generator, "sliding_window", kw)
    with pytest.raises(NotImplementedError, match="inference-only"):
        R(x)                                          # grad mode on, parameters require grad


def test_evaluation_loops(hip_lib, monkeypatch, tmp_path):
    from mtd_gan_amd import engine, metrics
    from mtd_gan_amd import kernels as K
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method, ResFFT_Generator
    torch.manual_seed(3)
    m = MTD_GAN_Method().cuda()
    m.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    x, y = orc.synthetic_ldct(1, seed=5, size=96)
    loader = [dict(n_20=x, n_100=y, path_n_20=["L000_0001.dcm"], path_n_100=["L000_0001.dcm"])]
    dev = torch.device("cuda")
    kw = dict(roi_size=(64, 64), sw_batch_size=4, overlap=0.5, mode="constant")
    names = ("pred_psnr", "pred_ssim", "pred_rmse")

    def expected(pred_clipped, pred):
        pm = metrics.pixel_metrics(x.cuda(), y.cuda(), pred_clipped)
        e = {f"pred_{k}": round(pm[k][2], 7) for k in ("psnr", "ssim", "rmse")}
        e["L1_loss"] = round((pred - y.cuda()).abs().mean().item(), 7)
        return e

    # attribute set: the loops compute what the direct call computes
    monkeypatch.setattr(type(m.Generator), "sliding_window", kw)
    assert type(m.Generator) is ResFFT_Generator
    t_sw = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, str(tmp_path))
    v_sw = engine.valid_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, 0, None, 0)
    m.Generator.eval()
    with torch.no_grad():
        direct = sliding_window_inference(x.cuda(), predictor=m.Generator, **kw)
        direct_clipped = sliding_window_inference(x.cuda(), predictor=m.Generator, clip=True, **kw)
    assert torch.equal(direct_clipped, K.clip01(direct))
    e = expected(direct_clipped, direct)
    for n in names:
        assert t_sw[n] == e[n], (n, t_sw[n], e[n])
    assert abs(t_sw["L1_loss"] - e["L1_loss"]) < 1e-6 and abs(v_sw["L1_loss"] - e["L1_loss"]) < 1e-6
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.Generator(x.cuda())                       # gradients enabled and the attribute set
    with pytest.raises(ValueError, match="sliding_window"):
        monkeypatch.setattr(type(m.Generator), "sliding_window", "yes")
        with torch.no_grad():
            m.Generator(x.cuda())

    # attribute unset: the loops are the whole-slice path, as before
    monkeypatch.setattr(type(m.Generator), "sliding_window", None)
    monkeypatch.setattr(ResFFT_Generator, "allow_any_size", True)
    t_ws = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, None)
    with torch.no_grad():
        whole = m.Generator(x.cuda())
    e = expected(K.clip01(whole), whole)
    for n in names:
        assert t_ws[n] == e[n], (n, t_ws[n], e[n])
    assert t_ws["pred_psnr"] != t_sw["pred_psnr"]
