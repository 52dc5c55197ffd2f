"""Stored DICOM pixel values <-> HU <-> window on the device: the three kernels of csrc/dicom_domain.hip against the
reference's recorded integers (tests/golden/dicom_domain.npz) and the numpy restatement of tests/_dicom_ref.py -- integers, and
for the window the very operations of mtd_hu_window, so everything is compared for EQUALITY -- then dicom_io.denoise_series
against the unpipelined composition and engine.test_MTD_GAN_Ours under `test_from_stored` / `test_save_dcm`."""
import numpy as np
import pytest
import torch

import _dicom_ref as D
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu
PAIRS = [(1, -1024), (1.0, -1024.0), (2, -1000), (0.5, -1024), (1.5, -8192)]
# (1, 1, 7) / (1, 1, 8) / (1, 1, 9): around one 8-pixel vector.  (2, 512, 512): more vectors than one grid pass (2048 x 256).
# (3, 5, 7): 35 pixels per slice put slices 1 and 2 off the 16-byte grid and let one vector straddle two slices with different
# (slope, intercept).  (11, 1, 1): a vector spans eight slices.
SHAPES = [(1, 1, 1), (1, 1, 7), (1, 1, 8), (1, 1, 9), (2, 64, 64), (2, 512, 512), (3, 5, 7), (11, 1, 1)]
# element offsets of (stored, float array, second 16-bit array) inside their allocations: all on the 16-byte grid; the stored
# view one pixel off its allocation (7 head pixels; the float array then shares no phase and goes scalar); the other two off
PHASES = [(8, 8, 8), (9, 8, 9), (8, 9, 11)]
G16, G32 = -21846, -7.5          # guard values (0xAAAA as int16)


def _pairs(S, first=0):
    return [PAIRS[(first + s) % len(PAIRS)] for s in range(S)]


def _words(shape, seed, unsigned=False):
    """Stored words that stay inside int16 under every pair of PAIRS, with the padding value and odd negatives."""
    g = np.random.RandomState(seed)
    w = g.randint(-9000, 15500, size=shape).astype(np.int16)
    flat = w.reshape(-1)
    special = np.int16([-2000, -1001, -1, -3, 3, 0, -2000])
    flat[:min(7, flat.size)] = special[:min(7, flat.size)]
    flat[-1] = -2000 if flat.size > 1 else flat[-1]
    return w.view(np.uint16).copy() if unsigned else w


def _guarded(values, front, guard):
    """values on the device inside a larger allocation whose other elements hold `guard`; returns (allocation, view)."""
    t = torch.from_numpy(np.ascontiguousarray(values))
    big = torch.full((front + t.numel() + 19,), guard, dtype=t.dtype if t.dtype != torch.uint16 else torch.int16, device="cuda")
    if t.dtype == torch.uint16:
        big = big.view(torch.uint16)
    view = big[front:front + t.numel()].view(t.shape)
    view.copy_(t.cuda())
    return big, view


def _blank(shape, dtype, front, guard):
    n = int(np.prod(shape))
    big = torch.full((front + n + 19,), guard, dtype=dtype, device="cuda")
    return big, big[front:front + n].view(shape)


def _guards_kept(big, front, n, guard):
    a = big.view(torch.int16) if big.dtype == torch.uint16 else big
    return bool((a[:front] == guard).all()) and bool((a[front + n:] == guard).all())


@pytest.fixture(scope="module")
def lib(hip_lib):
    from mtd_gan_amd import kernels as K

    def call(name, *args):
        K.check(getattr(hip_lib, name)(*args, K.stream_ptr()), name)
    return call


# ----------------------------------------------------------------------------------------------------- stored -> HU, window
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stored_to_hu_and_window(lib, shape):
    from mtd_gan_amd import dicom_io
    from mtd_gan_amd.create_datasets import Mayo
    S, H, W = shape
    n = S * H * W
    for j, (fs, ff, fh) in enumerate(PHASES):
        unsigned = j == 1
        words = _words(shape, 100 + j + n % 97, unsigned)
        pairs = _pairs(S, j)
        want = D.stored_to_hu(words, pairs)
        tab = dicom_io.rescale_table(pairs, S, torch.device("cuda"))
        sbig, sv = _guarded(words, fs, G16)
        assert sv.data_ptr() % 16 == (2 * fs) % 16
        hbig, hv = _blank(shape, torch.int16, fh, G16)
        lib("mtd_stored_to_hu", sv.data_ptr(), S, H, W, tab.data_ptr(), hv.data_ptr())
        got = hv.cpu().numpy()
        assert np.array_equal(got, want), (j, np.argwhere(got != want)[:5].tolist())
        assert _guards_kept(hbig, fh, n, G16) and _guards_kept(sbig, fs, n, G16)
        assert np.array_equal(sv.cpu().numpy(), words)                                          # the input is only read
        # the public calls; the fused window against the two-step route, bit for bit, for two windows
        hu = dicom_io.stored_to_hu(sv, pairs)
        assert hu.dtype == torch.int16 and hu.shape == sv.shape and np.array_equal(hu.cpu().numpy(), want)
        for a_min, a_max in ((-160.0, 240.0), (-1024.0, 3072.0)):
            two_step = Mayo.window_slices(hu, a_min, a_max)
            fbig, fv = _blank(shape, torch.float32, ff, G32)
            h2big, h2v = _blank(shape, torch.int16, fh, G16)
            lib("mtd_stored_to_window", sv.data_ptr(), S, H, W, tab.data_ptr(), a_min, a_max, fv.data_ptr(), h2v.data_ptr())
            assert torch.equal(fv, two_step) and torch.equal(h2v, hu)
            assert _guards_kept(fbig, ff, n, G32) and _guards_kept(h2big, fh, n, G16)
            f2big, f2v = _blank(shape, torch.float32, ff, G32)
            lib("mtd_stored_to_window", sv.data_ptr(), S, H, W, tab.data_ptr(), a_min, a_max, f2v.data_ptr(), None)
            assert torch.equal(f2v, two_step) and _guards_kept(f2big, ff, n, G32)
            win, hu2 = dicom_io.stored_to_window(sv, pairs, a_min, a_max, return_hu=True)
            assert torch.equal(win, two_step) and torch.equal(hu2, hu) and win.dtype == torch.float32
            assert 0.0 <= float(two_step.min()) and float(two_step.max()) <= 1.0
        assert torch.equal(dicom_io.stored_to_window(sv[:, None], pairs), Mayo.window_slices(hu)[:, None])     # (S, 1, H, W), defaults


def test_stored_to_hu_equals_the_reference(hip_lib):
    """The recorded cases, stacked per dtype into five slices with five different (slope, intercept) pairs."""
    from mtd_gan_amd import dicom_io
    meta, z = D.load()
    for dtype in ("int16", "uint16"):
        idx = [j for j, c in enumerate(meta["hu_cases"]) if c["dtype"] == dtype]
        pairs = [(meta["hu_cases"][j]["slope"], meta["hu_cases"][j]["intercept"]) for j in idx]
        assert pairs == PAIRS
        stored = np.stack([z[f"hu{j}.stored"] for j in idx])
        want = np.stack([z[f"hu{j}.hu"] for j in idx])
        got = dicom_io.stored_to_hu(torch.from_numpy(stored).cuda(), pairs).cpu().numpy()
        assert np.array_equal(got, want), (dtype, int((got != want).sum()))
        one = dicom_io.stored_to_hu(torch.from_numpy(stored[3:4]).cuda(), pairs[3]).cpu().numpy()       # one pair for all slices
        assert np.array_equal(one, want[3:4])


# ------------------------------------------------------------------------------------------------------ window -> stored
def test_window_to_stored_equals_the_reference(hip_lib):
    from mtd_gan_amd import dicom_io
    meta, z = D.load()
    for window in ((-1024.0, 3072.0), (-160.0, 240.0)):
        idx = [j for j, c in enumerate(meta["map_cases"]) if (c["a_min"], c["a_max"]) == window]
        pairs = [(meta["map_cases"][j]["slope"], meta["map_cases"][j]["intercept"]) for j in idx]
        assert pairs == PAIRS
        v = torch.from_numpy(np.stack([z[f"map{j}.v"] for j in idx])).cuda()
        for key, clip in (("raw", False), ("clipped", True)):
            want = np.stack([z[f"map{j}.{key}"] for j in idx])
            got = dicom_io.window_to_stored(v, pairs, *window, clip=clip).cpu().numpy()
            assert got.dtype == np.int16 and np.array_equal(got, want), (window, key, int((got != want).sum()))


def _values(shape, seed, scale=1.0):
    g = np.random.RandomState(seed)
    v = (g.rand(*shape) * 1.4 - 0.2).astype(np.float32)
    flat = v.reshape(-1)
    k = min(flat.size, 401)
    flat[:k] = (np.arange(401, dtype=np.float32) / np.float32(400))[::-1][:k]        # the window's own grid, from 1.0 down
    return (v * np.float32(scale)).astype(np.float32)


MODES = [dict(), dict(clip=False), dict(rounding="nearest"), dict(rounding="nearest", clip=False), dict(outside="input"),
         dict(outside="input", rounding="nearest", clip=False), dict(clip=False, scale=1000.0)]       # the last: saturation


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_window_to_stored_modes(lib, shape):
    from mtd_gan_amd import dicom_io
    S, H, W = shape
    n = S * H * W
    for j, mode in enumerate(MODES):
        mode = dict(mode)
        fo, fv_, fr = PHASES[j % 3]
        a_min, a_max = ((-160.0, 240.0), (-1024.0, 3072.0))[j % 2]
        v = _values(shape, 7 * j + n % 89, mode.pop("scale", 1.0))
        pairs = _pairs(S, j)
        words = _words(shape, 31 + j, unsigned=j == 4)
        want = D.window_to_stored(v, pairs, a_min, a_max, reference=words, **mode)
        if "scale" in MODES[j] and n > 1000:
            assert (want == 32767).any() and (want == -32768).any()
        if mode.get("outside") == "input" and n > 1000:
            hu = D.stored_to_hu(words, pairs)
            out = (hu < a_min) | (hu > a_max)
            assert out.any() and not out.all() and np.array_equal(want[out], words.view(np.int16)[out])
        tab = dicom_io.rescale_table(pairs, S, torch.device("cuda"))
        vbig, vv = _guarded(v, fv_, G32)
        rbig, rv = _guarded(words, fr, G16)
        obig, ov = _blank(shape, torch.int16, fo, G16)
        inside = mode.get("outside") == "input"
        lib("mtd_window_to_stored", vv.data_ptr(), S, H, W, tab.data_ptr(), a_min, a_max, int(mode.get("clip", True)),
            dicom_io.ROUNDING[mode.get("rounding", "trunc")], int(inside), rv.data_ptr() if inside else None, ov.data_ptr())
        got = ov.cpu().numpy()
        assert np.array_equal(got, want), (MODES[j], np.argwhere(got != want)[:5].tolist())
        assert _guards_kept(obig, fo, n, G16) and _guards_kept(vbig, fv_, n, G32) and _guards_kept(rbig, fr, n, G16)
        pub = dicom_io.window_to_stored(vv[:, None], pairs, a_min, a_max, reference=rv[:, None] if inside else None, **mode)
        assert pub.shape == (S, 1, H, W) and pub.dtype == torch.int16 and np.array_equal(pub[:, 0].cpu().numpy(), want)


def test_round_trip_returns_the_stored_words(hip_lib):
    """window_to_stored(stored_to_window(s), outside="input", reference=s) == s wherever slope is 1: inside the window the value
    comes back, outside it the input's word is written.  In the reference's truncating mode that holds on its own pair
    [-1024, 3072] (a power-of-two width: every product is exact); on the training window [-160, 240], 400 * fl(k / 400) falls just
    short of k for a few k, truncation then gives the neighbouring integer (tests/test_dicom_domain_cpu.py states which), and it is
    rounding="nearest" that returns every word.  Both are asserted as they are."""
    from mtd_gan_amd import dicom_io
    shape = (6, 64, 64)
    pairs = [(1, -1024), (1.0, -1024.0), (1, 0), (2, -1000), (1, -1024), (0.5, -1024)]
    unit = np.array([p[0] == 1 for p in pairs])
    words = np.random.RandomState(5).randint(-300, 4300, size=shape).astype(np.int16)
    words[0].reshape(-1)[:401] = np.arange(401) - 160 + 1024                   # every HU of the training window
    s = torch.from_numpy(words).cuda()
    # (the padding value is the one word get_pixels_hu itself does not keep: -2000 becomes 0, HU = intercept; where that HU lies
    # inside the window it comes back as word 0, outside it as the input's -2000)
    pad = torch.full((1, 1, 8), -2000, dtype=torch.int16, device="cuda")
    for (a_min, a_max), word in (((-1024.0, 3072.0), 0), ((-160.0, 240.0), -2000)):
        x = dicom_io.stored_to_window(pad, (1, -1024), a_min, a_max)
        assert dicom_io.window_to_stored(x, (1, -1024), a_min, a_max, outside="input", reference=pad).cpu().tolist() == [[[word] * 8]]
    for (a_min, a_max), rounding, exact in (((-1024.0, 3072.0), "trunc", True), ((-160.0, 240.0), "nearest", True),
                                            ((-160.0, 240.0), "trunc", False), ((-1024.0, 3072.0), "nearest", True)):
        x = dicom_io.stored_to_window(s, pairs, a_min, a_max)
        back = dicom_io.window_to_stored(x, pairs, a_min, a_max, rounding=rounding, outside="input", reference=s).cpu().numpy()
        same = (back[unit] == words[unit]).all()
        print(f"round trip [{a_min}, {a_max}] {rounding}: {int((back[unit] != words[unit]).sum())} of {words[unit].size} words differ")
        assert bool(same) == exact
        assert np.array_equal(back, D.window_to_stored(x.cpu().numpy(), pairs, a_min, a_max, rounding=rounding, outside="input", reference=words))
        assert np.abs(back[unit].astype(np.int32) - words[unit]).max() <= 1
    u = torch.from_numpy(words.view(np.uint16).copy()).cuda()                                          # uint16 words come back as their int16 view
    x = dicom_io.stored_to_window(u, pairs, -1024.0, 3072.0)
    back = dicom_io.window_to_stored(x, pairs, -1024.0, 3072.0, outside="input", reference=u).cpu().numpy()
    assert (back[unit] == words[unit]).all()


def test_public_functions_refuse_what_they_cannot_take(hip_lib):
    from mtd_gan_amd import dicom_io
    s = torch.zeros(2, 8, 8, dtype=torch.int16, device="cuda")
    v = torch.zeros(2, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="int16 or uint16"):
        dicom_io.stored_to_hu(v, (1, 0))
    with pytest.raises(RuntimeError, match="float32"):
        dicom_io.window_to_stored(s, (1, 0), -160.0, 240.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        dicom_io.stored_to_window(s.cpu(), (1, 0))
    with pytest.raises(ValueError, match="rescale"):
        dicom_io.stored_to_hu(s, [(1, 0)] * 3)
    with pytest.raises(ValueError, match="S, H, W"):
        dicom_io.stored_to_hu(s[0], (1, 0))
    with pytest.raises(ValueError, match="S, H, W"):
        dicom_io.stored_to_hu(s.reshape(1, 2, 8, 8), (1, 0))
    with pytest.raises(ValueError, match="reference"):
        dicom_io.window_to_stored(v, (1, 0), -160.0, 240.0, outside="input", reference=s[:1])
    with pytest.raises(RuntimeError, match="reference"):
        dicom_io.window_to_stored(v, (1, 0), -160.0, 240.0, outside="input", reference=v)
    with pytest.raises(RuntimeError, match="float64"):
        dicom_io.stored_to_hu(s, torch.ones(2, 2, device="cuda"))
    strided = torch.arange(2 * 8 * 16, device="cuda").to(torch.int16).reshape(2, 8, 16)[:, :, ::2]     # made contiguous on the way in
    assert np.array_equal(dicom_io.stored_to_hu(strided, (2, 1)).cpu().numpy(), D.stored_to_hu(strided.cpu().numpy(), (2, 1)))


# ------------------------------------------------------------------------------------------------------- whole series
@pytest.fixture(scope="module")
def setup(hip_lib):
    """Model seeded as tests/test_png_gpu.py builds it, and five 64 x 64 slice pairs as stored words with their pairs, made once
    and never modified."""
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    from mtd_gan_amd.create_datasets import Mayo
    torch.manual_seed(3)
    m = MTD_GAN_Method().cuda()
    m.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    m.Generator.eval()
    lo, hi = Mayo.synthetic_hu_slices(5, size=64, seed=4)
    pairs = [(1, -1024), (2, -1000), (1.0, -1024.0), (0.5, -1024), (1, -1024)]

    def to_words(hu):
        w = np.stack([np.trunc((hu[s].numpy().astype(np.float64) - icpt) / slope) for s, (slope, icpt) in enumerate(pairs)])
        return w.astype(np.int16)
    return m, to_words(lo), to_words(hi), pairs


def _composition(G, words, pairs, batch, a_min, a_max, outside, rounding):
    from mtd_gan_amd import dicom_io
    out = []
    with torch.no_grad():
        for i in range(0, words.shape[0], batch):
            s = torch.from_numpy(words[i:i + batch]).cuda()
            x = dicom_io.stored_to_window(s, pairs[i:i + batch], a_min, a_max)
            pred = G(x[:, None])
            out.append(dicom_io.window_to_stored(pred, pairs[i:i + batch], a_min, a_max, clip=True, rounding=rounding, outside=outside,
                                                 reference=s[:, None])[:, 0])
    return torch.cat(out)


@pytest.mark.parametrize("S,batch", [(5, 2), (1, 4), (4, 2)])
def test_denoise_series_equals_the_unpipelined_composition(setup, S, batch):
    from mtd_gan_amd import dicom_io
    m, lo, _hi, pairs = setup
    words, pairs = lo[:S], pairs[:S]
    kw = dict(a_min=-160.0, a_max=240.0, batch=batch)
    want = _composition(m.Generator, words, pairs, batch, -160.0, 240.0, "input", "trunc")
    assert want.shape == (S, 64, 64) and not np.array_equal(want.cpu().numpy(), words)
    host = dicom_io.denoise_series(m.Generator, words, pairs, pipelined=True, **kw)                      # numpy in, numpy out; side streams
    assert isinstance(host, np.ndarray) and host.dtype == np.int16 and host.shape == words.shape
    assert np.array_equal(host, want.cpu().numpy())
    plain = dicom_io.denoise_series(m.Generator, torch.from_numpy(words), pairs, **kw)                   # CPU tensor, one stream (the default)
    assert isinstance(plain, torch.Tensor) and not plain.is_cuda and torch.equal(plain, want.cpu())
    dev = dicom_io.denoise_series(m.Generator, torch.from_numpy(words).cuda()[:, None], pairs, **kw)    # device in, device out
    assert dev.is_cuda and dev.shape == (S, 1, 64, 64) and dev.dtype == torch.int16
    after = dev[:, 0].to(torch.int32) + 1                                                                # the caller's stream goes on
    assert torch.equal(dev[:, 0], want) and torch.equal(after, want.to(torch.int32) + 1)
    # uint16 words, the options, and a caller's buffer
    u = words.view(np.uint16).copy()
    buf = np.zeros(words.shape, dtype=np.int16)
    got = dicom_io.denoise_series(m.Generator, u, pairs, a_min=-1024.0, a_max=3072.0, batch=batch, outside="clip", rounding="nearest", out=buf, pipelined=True)
    assert got is buf
    assert np.array_equal(buf, _composition(m.Generator, words, pairs, batch, -1024.0, 3072.0, "clip", "nearest").cpu().numpy())


# -------------------------------------------------------------------------------------------------------------- engine
PIXEL_KEYS = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in ("input", "gt", "pred")]
SWITCHES = ("test_per_slice", "test_from_stored", "test_save_dcm")


def _clear(m):
    for k in SWITCHES:
        if hasattr(m, k):
            delattr(m, k)


def _loaders(lo, hi, pairs, per_batch):
    """The same four slices three ways: stored words with their pairs; the floats window_slices gives on the HU; the HU."""
    from mtd_gan_amd import dicom_io
    from mtd_gan_amd.create_datasets import Mayo
    names = [f"/data/L{i // 2:03d}/quarter_1mm/L{i // 2:03d}_QD_{i:04d}.dcm" for i in range(4)]
    x = Mayo.window_slices(dicom_io.stored_to_hu(torch.from_numpy(lo[:4]).cuda(), pairs[:4])).cpu()[:, None]
    y = Mayo.window_slices(dicom_io.stored_to_hu(torch.from_numpy(hi[:4]).cuda(), pairs[:4])).cpu()[:, None]
    stored, floats = [], []
    for i in range(0, 4, per_batch):
        sl = slice(i, i + per_batch)
        stored.append(dict(n_20=torch.from_numpy(lo[sl])[:, None], n_100=torch.from_numpy(hi[sl].view(np.uint16).copy())[:, None],
                           rescale_n_20=torch.tensor(pairs[sl], dtype=torch.float64), rescale_n_100=pairs[sl], path_n_20=names[sl]))
        floats.append(dict(n_20=x[sl], n_100=y[sl], path_n_20=names[sl]))
    return stored, floats, x


def test_loop_from_stored_words_with_a_dicom_sink(setup, tmp_path):
    from mtd_gan_amd import dicom_io, engine
    m, lo, hi, pairs = setup
    _clear(m)
    stored, floats, x = _loaders(lo, hi, pairs, 2)
    dev, l1 = torch.device("cuda"), torch.nn.L1Loss()
    captured = []
    try:
        m.test_per_slice = True
        plain = engine.test_MTD_GAN_Ours(m, l1, floats, dev, str(tmp_path / "floats"))
        m.test_from_stored = True
        m.test_save_dcm = lambda path, pixels, k: captured.append((path, pixels.copy(), k))
        res = engine.test_MTD_GAN_Ours(m, l1, stored, dev, str(tmp_path / "stored"))
        assert res == plain and list(res.keys()) == PIXEL_KEYS
        assert open(tmp_path / "stored" / "pred_results.csv").read() == open(tmp_path / "floats" / "pred_results.csv").read()
        assert [(p, k) for p, _, k in captured] == [(b["path_n_20"][i], 2 * j + i) for j, b in enumerate(stored) for i in range(2)]
        with torch.no_grad():
            for j in range(2):
                pred = m.Generator(x[2 * j:2 * j + 2].cuda())
                want = dicom_io.window_to_stored(pred, pairs[2 * j:2 * j + 2], -160.0, 240.0, clip=True, outside="input",
                                                 reference=torch.from_numpy(lo[2 * j:2 * j + 2]).cuda()[:, None]).cpu().numpy()
                for i in range(2):
                    got = captured[2 * j + i][1]
                    assert got.dtype == np.int16 and got.shape == (64, 64) and np.array_equal(got, want[i, 0])
        assert not np.array_equal(captured[0][1], lo[0])
        # another window through the dict form: the floats are window_slices' for that window
        m.test_from_stored = dict(a_min=-1024.0, a_max=3072.0)
        m.test_save_dcm = None
        wide = engine.test_MTD_GAN_Ours(m, l1, stored, dev, None)
        assert list(wide.keys()) == PIXEL_KEYS and wide != plain and len(captured) == 4
        # a batch of two slices on the default path is one sample: nothing to hand the sink
        del m.test_per_slice
        m.test_from_stored, m.test_save_dcm = True, lambda *a: captured.append(a)
        with pytest.raises(ValueError, match="test_per_slice"):
            engine.test_MTD_GAN_Ours(m, l1, stored, dev, None)
        assert len(captured) == 4
    finally:
        _clear(m)


def test_loop_default_path_and_absent_switches(setup, tmp_path):
    """Batches of one slice: the stored route equals the float route with the sink called once per slice; and with the
    attributes absent or falsy the float loop gives what its own pieces give on each batch, as before."""
    from mtd_gan_amd import engine, kernels as K, metrics as M
    m, lo, hi, pairs = setup
    _clear(m)
    stored, floats, x = _loaders(lo, hi, pairs, 1)
    dev, l1 = torch.device("cuda"), torch.nn.L1Loss()
    meters = {}
    with torch.no_grad():
        for b in floats:
            xb, yb = b["n_20"].cuda(), b["n_100"].cuda()
            r = m.Generator(xb)
            s = {"L1_loss": float(engine._l1(l1, r, yb))}
            pm = M.pixel_metrics(xb, yb, K.clip01(r.contiguous()))
            for name in ("rmse", "psnr", "ssim"):
                for who, v in zip(("input", "gt", "pred"), pm[name]):
                    s[f"{who}_{name}"] = v
            for k, v in s.items():
                meters.setdefault(k, engine._Meter()).update(v, 1)
    want = {k: round(mm.global_avg, 7) for k, mm in meters.items()}
    try:
        for setting in ("absent", False, None, {}):
            if setting != "absent":
                m.test_from_stored = m.test_save_dcm = setting
            assert engine.test_MTD_GAN_Ours(m, l1, floats, dev, str(tmp_path / f"off_{setting}")) == want
        captured = []
        m.test_from_stored, m.test_save_dcm = True, lambda path, pixels, k: captured.append(k)
        assert engine.test_MTD_GAN_Ours(m, l1, stored, dev, str(tmp_path / "stored")) == want
        assert captured == [0, 1, 2, 3]
        assert open(tmp_path / "stored" / "pred_results.csv").read() == open(tmp_path / "off_absent" / "pred_results.csv").read()
    finally:
        _clear(m)
