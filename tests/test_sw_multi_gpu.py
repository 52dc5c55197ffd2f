"""Multi-output sliding-window inference on the device (inferers.sliding_window_inference_multi, module/sliding_window.py,
csrc/sliding_window.hip: mtd_sw_blend_multi / mtd_sw_finish_multi / mtd_sw_gather_flags): every plane bit for bit the
single-output call on that plane, the blend against the float64 restatement of tests/_sw_multi_ref.py and against the
reference's fp32 values of the committed fixture, the reference's rule for empty chunks, and the discriminators as predictors
against the CPU oracle."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mtdgan_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
import _sw_multi_ref as R  # noqa: E402
from _metrics import rel  # noqa: E402

from mtd_gan_amd.inferers import sliding_window_inference, sliding_window_inference_multi, window_starts  # noqa: E402

NAMES = ("cls", "seg", "rec")
CASES = [((2, 1, 80, 99), (64, 64), 0.3, 3),        # 2 x 2 windows per image; chunks 3 + 3 + 2 span the two images
         ((1, 1, 70, 64), (64, 64), 0.9, 32),       # starts [0, 6] along y, one window along x
         ((1, 1, 64, 64), (64, 64), 0.25, 4),       # one window
         ((1, 1, 50, 70), (32, 48), 0.5, 4),        # non-square roi
         ((1, 1, 41, 47), (30, 30), 0.5, 3)]        # rw % 4 != 0: the scalar gather path (the fixture's case)


def _input(shape):
    return R.case_input(shape, "signed", seed=sum(shape))


def _single(x, roi, sb, overlap, mode, plane):
    """The single-output call on one plane of the toy predictor; "cls_map": the score expanded to the window's shape."""
    def pred(w):
        cls, seg, rec = R.toy_predictor(w)
        return {"seg": seg, "rec": rec}[plane] if plane != "cls_map" else cls.reshape(-1, 1, 1, 1).expand(w.shape).contiguous()
    return sliding_window_inference(x, roi, sb, pred, overlap=overlap, mode=mode)


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
@pytest.mark.parametrize("shape,roi,overlap,sw_batch", CASES)
def test_planes_equal_the_single_output_call_and_the_float64_blend(hip_lib, shape, roi, overlap, sw_batch, mode):
    x = _input(shape)
    rec = R.Recorder(R.toy_predictor)
    out = sliding_window_inference_multi(x.cuda(), roi, sw_batch, rec, overlap=overlap, mode=mode, score_map=True)
    assert sorted(out) == ["cls", "cls_map", "rec", "seg"]
    B, ny, nx = shape[0], len(window_starts(shape[2], roi[0], overlap)), len(window_starts(shape[3], roi[1], overlap))
    assert [c[0].shape[0] for c in rec.chunks] == [min(sw_batch, B * ny * nx - i) for i in range(0, B * ny * nx, sw_batch)]
    preds = rec.predictions(NAMES)
    # the device predictor saw the plan's windows and computed what the CPU computes on them (exact arithmetic)
    ref = R.restate(x, roi, sw_batch, overlap, mode)
    assert torch.equal(preds["cls"].reshape(-1), ref["scores"])
    assert tuple(out["cls"].shape) == (B, ny, nx) and out["cls"].dtype == torch.float32 and out["cls"].is_cuda
    assert torch.equal(out["cls"].cpu().reshape(-1), ref["scores"])
    for plane in ("seg", "rec", "cls_map"):
        got = out[plane]
        assert got.dtype == torch.float32 and tuple(got.shape) == shape and got.is_cuda
        assert torch.equal(got, _single(x.cuda(), roi, sw_batch, overlap, mode, plane)), plane          # bit for bit
        err, bound = (got.cpu().double() - ref[plane]).abs().max().item(), R.bound(ref["k"], ref["maxabs"][plane])
        print(f"shape {shape} roi {roi} overlap {overlap} {mode} {plane}: k {ref['k']}, max err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, plane
    # ... and the blend of the recorded predictions is that blend
    again = R.restate(x, roi, sw_batch, overlap, mode, recorded=preds)
    assert torch.equal(again["seg"], ref["seg"]) and torch.equal(again["rec"], ref["rec"])
    if B * ny * nx == 1:
        assert torch.equal(out["seg"].cpu(), preds["seg"]) and torch.equal(out["rec"].cpu(), preds["rec"])


@pytest.mark.parametrize("shape,overlap", [((2, 1, 80, 99), 0.3), ((1, 1, 100, 77), 0.9)])
def test_same_bits_every_run_and_every_chunking(hip_lib, shape, overlap):
    """(1, 1, 100, 77) at overlap 0.9: 7 x 4 windows, up to 28 on one pixel, chunks of 3 start in the middle of a window row."""
    x = _input(shape).cuda()
    for mode in ("constant", "gaussian"):
        runs = [sliding_window_inference_multi(x, (64, 64), n, R.toy_predictor, overlap=overlap, mode=mode, score_map=True)
                for n in (3, 3, 1, 1000)]
        for other in runs[1:]:
            for k in ("cls", "seg", "rec", "cls_map"):
                assert torch.equal(runs[0][k], other[k]), (mode, k)


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_against_the_reference_values_of_the_fixture(hip_lib, mode):
    """Both sides are fp32 sums of the same <= k terms: twice the bound against float64."""
    shape, roi, overlap, sb, _modes, _kind = R.FIXTURE_CASES["odd_roi"]
    fix = R.load_fixture()
    x = fix["odd_roi/x"]
    from mtd_gan_amd.module.sliding_window import sliding_window_inference_three_output
    cls, seg, rec = sliding_window_inference_three_output(x.cuda(), roi, sb, R.toy_predictor, overlap, mode)
    ref = R.restate(x, roi, sb, overlap, mode)
    assert torch.equal(cls.cpu(), fix[f"odd_roi/{mode}/cls"])
    for name, got in (("seg", seg), ("rec", rec)):
        err, bound = (got.cpu() - fix[f"odd_roi/{mode}/{name}"]).abs().max().item(), 2 * R.bound(ref["k"], ref["maxabs"][name])
        print(f"{mode} {name}: max err against the reference's fp32 {err:.3e}, bound {bound:.3e}")
        assert err <= bound, name


def test_clip_names_the_maps_it_clips(hip_lib):
    x = (_input((2, 1, 80, 99)) * 2).cuda()
    kw = dict(overlap=0.3, mode="gaussian", score_map=True)
    plain = sliding_window_inference_multi(x, (64, 64), 3, R.toy_predictor, **kw)
    clipped = sliding_window_inference_multi(x, (64, 64), 3, R.toy_predictor, clip=("seg", "cls_map"), **kw)
    assert plain["seg"].min().item() < 0 and plain["seg"].max().item() > 1 and plain["cls_map"].max().item() > 1
    assert torch.equal(clipped["seg"], plain["seg"].clamp(0, 1)) and torch.equal(clipped["cls_map"], plain["cls_map"].clamp(0, 1))
    assert torch.equal(clipped["rec"], plain["rec"]) and torch.equal(clipped["cls"], plain["cls"])


def test_fewer_outputs_and_a_bare_tensor(hip_lib):
    x = _input((2, 1, 80, 99)).cuda()
    full = sliding_window_inference_multi(x, (64, 64), 3, R.toy_predictor, overlap=0.3, mode="gaussian")
    two = sliding_window_inference_multi(x, (64, 64), 3, lambda w: R.toy_predictor(w)[1:], overlap=0.3, mode="gaussian",
                                         outputs=("seg", "rec"))
    one = sliding_window_inference_multi(x, (64, 64), 3, lambda w: R.toy_predictor(w)[2], overlap=0.3, mode="gaussian", outputs=("rec",))
    assert sorted(two) == ["rec", "seg"] and sorted(one) == ["rec"]
    assert torch.equal(two["seg"], full["seg"]) and torch.equal(two["rec"], full["rec"]) and torch.equal(one["rec"], full["rec"])
    with pytest.raises(ValueError, match="one tensor per output name"):
        sliding_window_inference_multi(x, (64, 64), 3, lambda w: R.toy_predictor(w)[1:], overlap=0.3)
    with pytest.raises(ValueError, match="predictor output 'seg'"):
        sliding_window_inference_multi(x, (64, 64), 3, lambda w: (w[:, 0, 0, :1], w[:, :, :, :-1], w), overlap=0.3)


# ------------------------------------------------------------------------------------------------ empty chunks
def test_empty_chunks_contribute_no_scores(hip_lib):
    """(2, 1, 80, 99): 4 windows per image, image 1 all zero.  Chunks of 3: [0-2] [3-5] [6-7], the second still holds window 3
    of image 0, so windows 0..5 are kept; chunks of 4: windows 0..3."""
    from mtd_gan_amd.module.sliding_window import sliding_window_inference_three_output
    shape, roi, overlap, _sb, modes, _kind = R.FIXTURE_CASES["empty"]
    fix = R.load_fixture()
    x = fix["empty/x"]
    assert x.min().item() >= 0 and x[1].abs().max().item() == 0 and x[0].abs().max().item() > 0
    maps = {}
    for chunk, kept in ((3, 6), (4, 4)):
        cls, seg, rec = sliding_window_inference_three_output(x.cuda(), roi, chunk, R.toy_predictor, overlap, modes[0])
        ref = R.restate(x, roi, chunk, overlap, modes[0])
        assert tuple(cls.shape) == (kept, 1) and ref["kept"] == list(range(kept))
        assert torch.equal(cls.cpu(), fix[f"empty/c{chunk}/cls"]) and torch.equal(cls.cpu(), ref["cls"])
        maps[chunk] = (seg, rec)
        # the maps do not feel the rule
        plain = sliding_window_inference_multi(x.cuda(), roi, chunk, R.toy_predictor, overlap=overlap, mode=modes[0])
        assert torch.equal(seg, plain["seg"]) and torch.equal(rec, plain["rec"]) and tuple(plain["cls"].shape) == (2, 2, 2)
        assert torch.equal(plain["cls"].reshape(-1)[:kept], cls.reshape(-1))
    assert torch.equal(maps[3][0], maps[4][0]) and torch.equal(maps[3][1], maps[4][1])
    zero = sliding_window_inference_multi(torch.zeros(1, 1, 80, 99).cuda(), roi, 3, R.toy_predictor, overlap=overlap, drop_empty_chunks=True)
    assert tuple(zero["cls"].shape) == (0, 1)


@pytest.mark.parametrize("shape,roi", [((1, 1, 64, 192), (64, 64)), ((1, 1, 30, 90), (30, 30))])       # vector and scalar gather
def test_flags_of_edge_windows(hip_lib, shape, roi):
    """Three windows side by side (overlap 0): one whose only nonzero is its last element, one holding only -0.0, one of
    +0.0; the flags buffer starts as garbage."""
    from mtd_gan_amd import kernels as K
    x = torch.zeros(shape)
    x[0, 0, roi[0] - 1, roi[1] - 1] = 1e-30
    x[0, 0, :, roi[1]:2 * roi[1]] = -0.0
    assert torch.signbit(x[0, 0, 0, roi[1]]).item()
    windows = torch.empty(3, 1, *roi, device="cuda")
    flags = torch.full((3,), 7, dtype=torch.uint8, device="cuda")
    K.sw_gather_flags(x.cuda(), roi, roi, 0, 3, windows, flags)
    assert flags.tolist() == [1, 0, 0]
    assert torch.equal(windows.cpu(), torch.cat([x[:, :, :, i * roi[1]:(i + 1) * roi[1]] for i in range(3)]).reshape(3, 1, *roi))
    assert torch.equal(torch.signbit(windows[1]).cpu(), torch.ones(1, *roi, dtype=torch.bool))     # -0.0 travels as it is
    flags.fill_(7)
    K.sw_gather_flags(x.cuda(), roi, roi, 1, 2, windows, flags)            # a chunk that starts later writes its own entries only
    assert flags.tolist() == [0, 0, 7]


@pytest.mark.parametrize("shape,roi,overlap,sw_batch", CASES)
def test_flags_equal_any_nonzero(hip_lib, shape, roi, overlap, sw_batch):
    """A sparse input: a handful of nonzero pixels (one of them a NaN), so that windows of both kinds exist where the plan has
    more than one window."""
    from mtd_gan_amd import kernels as K
    from mtd_gan_amd.inferers import window_interval
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.zeros(shape)
    B, _, H, W = shape
    x[0, 0, H - 1, W - 1] = 1.0
    x[0, 0, int(torch.randint(H, (1,), generator=g)), 0] = float("nan")
    x[B - 1, 0, 0, W // 2] = -2.0
    ys, xs = window_starts(H, roi[0], overlap), window_starts(W, roi[1], overlap)
    plan = [(b, y, xx) for b in range(B) for y in ys for xx in xs]
    want = [int((x[b, 0, y:y + roi[0], xx:xx + roi[1]] != 0).any().item()) for b, y, xx in plan]
    iv = (window_interval(H, roi[0], overlap), window_interval(W, roi[1], overlap))
    windows = torch.empty(len(plan), 1, *roi, device="cuda")
    flags = torch.full((len(plan),), 9, dtype=torch.uint8, device="cuda")
    for w0 in range(0, len(plan), sw_batch):
        n = min(sw_batch, len(plan) - w0)
        K.sw_gather_flags(x.cuda(), roi, iv, w0, n, windows[w0:], flags[w0:])
    assert flags.tolist() == want
    assert len(set(want)) == 2 or len(plan) <= 2                     # windows of both kinds, where the plan has room for them
    got = windows.cpu()
    for i, (b, y, xx) in enumerate(plan):
        assert torch.equal(got[i, 0].nan_to_num(nan=5.0), x[b, 0, y:y + roi[0], xx:xx + roi[1]].nan_to_num(nan=5.0)), i


# ------------------------------------------------------------------------------------ the discriminators as predictors
def _oracle_windows(forward, x, roi, overlap):
    out = []
    for b in range(x.shape[0]):
        for y in window_starts(x.shape[2], roi[0], overlap):
            for xs in window_starts(x.shape[3], roi[1], overlap):
                out.append(forward(x[b:b + 1, :, y:y + roi[0], xs:xs + roi[1]]))
    return out


def _slice_input():
    x, _ = orc.synthetic_ldct(2, seed=9, size=96)
    return x[:, :, :80, :].contiguous()


def test_multi_task_discriminator_on_slices(hip_lib):
    """(2, 1, 80, 96), overlap 0.5: 2 x 2 windows per image, chunks 3, 3, 2.  Bit equality across chunkings is not asserted:
    the conv plans differ with the batch."""
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    from mtd_gan_amd.module.sliding_window import sliding_window_inference_three_output
    D = MTD_GAN_Method().Discriminator
    dstate = orc.seeded_fill(orc.d_state_shapes(), seed=11)
    D.load_state_dict(dstate)
    D.cuda().eval()
    x = _slice_input()
    assert tuple(x.shape) == (2, 1, 80, 96)
    rec = R.Recorder(D)
    with torch.no_grad():
        out = sliding_window_inference_multi(x.cuda(), (64, 64), 3, rec, overlap=0.5, score_map=True, clip=("rec",))
        with pytest.raises(NotImplementedError, match="64,64"):
            D(x.cuda())                              # the module itself still takes patches only
    assert [c[0].shape[0] for c in rec.chunks] == [3, 3, 2]
    preds = rec.predictions(NAMES)
    # each window's outputs are the oracle's discriminator on that window (the project's standing parity bound)
    with torch.no_grad():
        wins = _oracle_windows(lambda w: orc.discriminator_forward({k: v.clone() for k, v in dstate.items()}, w, train=False), x, (64, 64), 0.5)
    for i, name in enumerate(NAMES):
        assert rel(preds[name], torch.cat([w[i] for w in wins])) < 1e-3, name
    # the blended maps are the float64 blend of the recorded outputs
    ref = R.restate(x, (64, 64), 3, 0.5, "constant", recorded=preds)
    assert torch.equal(out["cls"].cpu().reshape(-1), preds["cls"].reshape(-1)) and tuple(out["cls"].shape) == (2, 2, 2)
    for plane in ("seg", "rec", "cls_map"):
        want = ref[plane].clamp(0, 1) if plane == "rec" else ref[plane]
        assert (out[plane].cpu().double() - want).abs().max().item() <= R.bound(ref["k"], ref["maxabs"][plane]), plane
    # the reference's name gives the same maps (unclipped there) and every score: no chunk of these slices is empty
    with torch.no_grad():
        cls, seg, rrec = sliding_window_inference_three_output(x.cuda(), (64, 64), 3, D, 0.5)
    assert tuple(cls.shape) == (8, 1) and rel(cls.reshape(-1), out["cls"].reshape(-1)) < 1e-5 and rel(seg, out["seg"]) < 1e-5
    assert rel(rrec.clamp(0, 1), out["rec"]) < 1e-5


def test_cls_discriminator_scores_only(hip_lib, monkeypatch):
    from mtd_gan_amd import kernels as K
    from mtd_gan_amd.arch.Ours.networks import CLS_Discriminator
    from mtd_gan_amd.module.sliding_window import sliding_window_inference_cls_output
    D = CLS_Discriminator(1, 64)
    st = orc.seeded_fill({k: tuple(v.shape) for k, v in D.state_dict().items()}, seed=11)
    D.load_state_dict(st)
    D.cuda().eval()
    x = _slice_input()

    def refuse(*a, **k):
        raise AssertionError("a blend or finish launch where only scores are asked for")
    for name in ("sw_blend", "sw_finish", "sw_blend_multi", "sw_finish_multi"):
        monkeypatch.setattr(K, name, refuse)
    with torch.no_grad():
        cls = sliding_window_inference_cls_output(x.cuda(), (64, 64), 3, D, 0.5)
        wins = _oracle_windows(lambda w: orc.discriminator_forward({k: v.clone() for k, v in st.items()}, w, train=False, heads=("cls",))[0],
                               x, (64, 64), 0.5)
    assert tuple(cls.shape) == (8, 1) and cls.dtype == torch.float32 and cls.is_cuda
    assert rel(cls.cpu(), torch.cat(wins)) < 1e-3


# --------------------------------------------------------------------------------------------- entry-point refusals
def test_entry_points_refuse_plane_counts_and_null_planes(hip_lib):
    """With real device buffers behind the pointers: still refused, nothing launched, the accumulators untouched."""
    vp = ctypes.c_void_p
    acc = torch.full((1, 80, 99), 3.0, device="cuda")
    pred = torch.ones(1, 64, 64, device="cuda")
    imap = torch.ones(64, 64, device="cuda")
    geom = (1, 80, 99, 64, 64, 44, 44)
    full = (vp * 5)(*[acc.data_ptr()] * 5)
    preds = (vp * 5)(*[pred.data_ptr()] * 5)
    ints = (ctypes.c_int * 5)(0, 0, 0, 0, 0)
    for n in (0, 5):
        assert hip_lib.mtd_sw_blend_multi(n, preds, ints, full, imap.data_ptr(), *geom, 0, 1, None) == -1
        assert hip_lib.mtd_sw_finish_multi(n, full, ints, full, imap.data_ptr(), *geom, None) == -1
    holed = (vp * 5)(acc.data_ptr(), None, acc.data_ptr(), acc.data_ptr(), acc.data_ptr())
    assert hip_lib.mtd_sw_blend_multi(2, preds, ints, holed, imap.data_ptr(), *geom, 0, 1, None) == -1
    assert hip_lib.mtd_sw_blend_multi(2, (vp * 5)(pred.data_ptr(), None), ints, full, imap.data_ptr(), *geom, 0, 1, None) == -1
    assert hip_lib.mtd_sw_finish_multi(2, holed, ints, full, imap.data_ptr(), *geom, None) == -1
    assert hip_lib.mtd_sw_finish_multi(2, full, ints, holed, imap.data_ptr(), *geom, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), torch.full((1, 80, 99), 3.0))
