"""The general-length spectral kernels (csrc/resfft_gen.hip) stage by stage against torch.fft on the CPU in float64: rows
forward, columns + mix + inverse columns, rows back, and the three chained -- at every mixed-radix length 16..512 and at both
ends (and both parities) of every Bluestein convolution length.  The lengths come from the library's plans, read through
the hip_lib fixture when the first test runs (tests/_gen_lengths.py; tests/test_any_size_plan_cpu.py proves that they leave
no plan out).

Every map is a 32-channel slice (channel offset 8) of a 48-channel NHWC tensor whose other channels hold a sentinel, R and T
are followed by 4096 sentinel floats (NaN: a read of them poisons the output), and the workspace is NaN before each stage (a stage builds the Bluestein filter it
needs itself).  Maps carry one spare image of NaN behind the batch, so a kernel that reads past the last row of the batch
reads defined memory and poisons its output -- a large finite value would not do: the partner row of a row pair cancels out
of the first row's spectrum but for rounding.

Bound: rel < 1e-5 per stage, the bound of the 64-point stage kernels (test_kernels_gpu.py::test_spectral_path_kernels).  A
float32 model of the passes has a tensor-wide error under 3.1e-7 for one transform at every length and under 1e-6 for three
chained.  Measured on an MI355X with _metrics.rel: 1.1e-6 at worst for a row stage, 2.1e-6 for columns + mix, 3.2e-6 for the
chain.  The two sets of figures are not the same measure: rel adds an element-wise term, |a - b| / (|b| + rms),
which exceeds the tensor-wide error by up to max |b| / rms (4 to 5 for these tensors), and the model has not been evaluated
with rel itself, so the factor of about 3 between them is not evidence of kernel error."""
import pytest
import torch

import _gen_lengths as gl
import _spectral_stages as ss
from _spectral_stages import (C, _Report, _cplx, _edges, _mix_reference, _outside_unchanged, _ptr, _randn, _sliced,      # noqa: F401
                              _tail_unchanged)

pytestmark = pytest.mark.gpu

B = 2
H_ROWS = 17                   # rows of the row stages: odd, so the last row of each image has no partner
N_CHUNKS = 8

CHAIN_PAIRS = [(49, 112), (343, 17), (131, 210), (62, 255), (511, 16), (16, 511)]


def _spectrum(nkw, h, fill=None):
    """(flat, S): S = the first B nkw h 64 floats of flat as [B][nkw][h][Re 32 | Im 32]; TAIL sentinel floats follow."""
    return ss._spectrum(B, nkw, h, fill)


def _nan_workspace(K, L, h, w):
    need = L.mtd_spectral_gen_ws_bytes(B, h, w)
    assert need > 0, (h, w)
    ws = K.workspace(need, torch.device("cuda", torch.cuda.current_device()))
    ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    return ws


# ------------------------------------------------------------------------------------------------------------- stages
def _rows_forward(K, L, rep, n):
    """(a) W = n, H = 17: R against rfft along W."""
    h, w, nkw = H_ROWS, n, n // 2 + 1
    x = _randn(B, h, w, C, seed=1000 + n)
    xb, xv = _sliced(x)
    keep = xb.clone()
    flat, R = _spectrum(nkw, h)
    ws = _nan_workspace(K, L, h, w)
    K.check(L.mtd_rfft_rows_gen(xv.data_ptr(), K.ld_of(xv), R.data_ptr(), B, h, w, ws.data_ptr(), ws.numel(), K.stream_ptr()),
            "mtd_rfft_rows_gen")
    ref = torch.fft.rfft(x.double(), dim=2, norm="ortho").permute(0, 2, 1, 3)          # (B, nkw, H, C)
    got = R.cpu()
    rep.err("rows_re", n, got[..., :C], ref.real)
    rep.err("rows_im", n, got[..., C:], ref.imag)
    rep.check(_tail_unchanged(flat), "rows", n, "the floats behind R changed")
    rep.check(torch.equal(xb.view(torch.int32), keep.view(torch.int32)), "rows", n, "the input map changed")


def _columns_mix(K, L, rep, n, w2, b2, w2t, b2d):
    """(b) H = n at W = 16 (column 8 is the Nyquist column) and W = 17 (column 8 is an ordinary one); nkw = 9 both times."""
    for w in (16, 17):
        h, nkw = n, w // 2 + 1
        Rin = _randn(B, nkw, h, 64, seed=2000 + 17 * n + w)                                # not Hermitian-consistent
        rflat, R = _spectrum(nkw, h, Rin)
        keep = rflat.clone()
        tflat, T = _spectrum(nkw, h)
        ws = _nan_workspace(K, L, h, w)
        K.check(L.mtd_spec_mix_gen(R.data_ptr(), w2t.data_ptr(), b2d.data_ptr(), T.data_ptr(), B, h, w, ws.data_ptr(), ws.numel(),
                                   K.stream_ptr()), "mtd_spec_mix_gen")
        got, case = T.cpu(), f"{n} (W = {w})"
        rep.err("mix", case, got, _mix_reference(Rin, w2, b2, w))
        rep.check(bool((got[:, _edges(w), :, C:].contiguous().view(torch.int32) == 0).all()), "mix", case,
                  "an imaginary half of column 0 / W/2 is not exactly zero")
        rep.check(_tail_unchanged(tflat), "mix", case, "the floats behind T changed")
        rep.check(torch.equal(rflat.view(torch.int32), keep.view(torch.int32)), "mix", case, "R or the floats behind it changed")


def _rows_back(K, L, rep, n, adds=(True, True)):
    """(c) W = n, H = 17: out against irfft along W of T (garbage in the imaginary halves of column 0 and the Nyquist column:
    ignored) + add1 + add2."""
    h, w, nkw = H_ROWS, n, n // 2 + 1
    Tin = _randn(B, nkw, h, 64, seed=3000 + n)
    tflat, T = _spectrum(nkw, h, Tin)
    keep = tflat.clone()
    a_cpu = [_randn(B, h, w, C, seed=4000 + 2 * n + i) if use else None for i, use in enumerate(adds)]
    a_dev = [_sliced(a) if a is not None else (None, None) for a in a_cpu]
    a_keep = [b.clone() if b is not None else None for b, _ in a_dev]
    ob, ov = _sliced(torch.full((B, h, w, C), float("nan")))
    ws = _nan_workspace(K, L, h, w)
    (_, a1), (_, a2) = a_dev
    K.check(L.mtd_irfft_rows_gen(T.data_ptr(), ov.data_ptr(), K.ld_of(ov), _ptr(a1), K.ld_of(a1) if a1 is not None else 0,
                                 _ptr(a2), K.ld_of(a2) if a2 is not None else 0, B, h, w, ws.data_ptr(), ws.numel(),
                                 K.stream_ptr()), "mtd_irfft_rows_gen")
    Tc = _cplx(Tin)
    Tc.imag[:, _edges(w)] = 0.0
    ref = torch.fft.irfft(Tc.permute(0, 2, 3, 1), n=w, dim=3, norm="ortho").permute(0, 1, 3, 2)      # (B, H, W, C)
    for a in a_cpu:
        if a is not None:
            ref = ref + a.double()
    case = n if all(adds) else f"{n} (adds {adds})"
    rep.err("back", case, ov.cpu(), ref)
    rep.check(_outside_unchanged(ob), "back", case, "channels outside the output slice changed")
    rep.check(torch.equal(tflat.view(torch.int32), keep.view(torch.int32)), "back", case, "T or the floats behind it changed")
    for (b, _), k in zip(a_dev, a_keep):
        if b is not None:
            rep.check(torch.equal(b.view(torch.int32), k.view(torch.int32)), "back", case, "an add map changed")


@pytest.fixture(scope="module")
def lengths(hip_lib):
    """(plans, smooth, blue) from the library the hip_lib fixture has built and loaded."""
    plans = gl.library_plans(hip_lib)
    return (plans,) + gl.select(plans)


@pytest.fixture(scope="module")
def mix_weights(hip_lib):
    from mtd_gan_amd import kernels as K
    w2 = _randn(64, 64, seed=42, scale=0.125)
    b2 = _randn(64, seed=43, scale=0.1)
    return w2, b2, K.transpose64(w2.cuda()), b2.cuda()


def _all_stages(hip_lib, mix_weights, record_property, lengths):
    from mtd_gan_amd import kernels as K
    assert lengths
    rep = _Report()
    for n in lengths:
        _rows_forward(K, hip_lib, rep, n)
        _columns_mix(K, hip_lib, rep, n, *mix_weights)
        _rows_back(K, hip_lib, rep, n)
    rep.finish(record_property)


# -------------------------------------------------------------------------------------------------------------- items
@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_mixed_radix_stages(hip_lib, lengths, mix_weights, record_property, chunk):
    """Every length 16..512 with a mixed-radix plan, in N_CHUNKS interleaved chunks."""
    _all_stages(hip_lib, mix_weights, record_property, lengths[1][chunk::N_CHUNKS])


@pytest.mark.parametrize("m", [64, 128, 256, 512, 1024])
def test_bluestein_stages(hip_lib, lengths, mix_weights, record_property, m):
    """Both ends, in both parities, of the lengths that take Bluestein convolution length m."""
    _all_stages(hip_lib, mix_weights, record_property, lengths[2].get(m, []))


def test_rows_back_without_adds(hip_lib, lengths, record_property):
    """add1 = None and both adds None, at a mixed-radix (2 3 7) and a Bluestein (M = 64) length."""
    from mtd_gan_amd import kernels as K
    rep = _Report()
    for n in (42, 22):
        assert (lengths[0][n][0] != 0) == (n == 22)
        _rows_back(K, hip_lib, rep, n, adds=(False, True))
        _rows_back(K, hip_lib, rep, n, adds=(False, False))
    rep.finish(record_property)


@pytest.mark.parametrize("H,W", CHAIN_PAIRS)
def test_chained_stages(hip_lib, mix_weights, record_property, H, W):
    """kernels.spectral_branch_gen against irfft2(relu(W2 rfft2(x) + b2)) + add1 + add2, on pairs that mix the plan classes."""
    from mtd_gan_amd import kernels as K
    w2, b2, w2t, b2d = mix_weights
    x = _randn(B, H, W, C, seed=5000 + 600 * H + W)
    adds = [_randn(B, H, W, C, seed=6000 + 600 * H + W + i) for i in range(2)]
    xb, xv = _sliced(x)
    (a1b, a1), (a2b, a2) = [_sliced(a) for a in adds]
    keeps = [t.clone() for t in (xb, a1b, a2b)]
    ob, ov = _sliced(torch.full((B, H, W, C), float("nan")))
    _nan_workspace(K, hip_lib, H, W)
    K.spectral_branch_gen(xv, w2t, b2d, ov, add1=a1, add2=a2)
    f = torch.fft.rfft2(x.double(), s=(H, W), dim=(1, 2), norm="ortho")                  # (B, H, nkw, C)
    y = torch.relu(torch.cat([f.real, f.imag], dim=-1) @ w2.double().t() + b2.double())
    ref = torch.fft.irfft2(torch.complex(y[..., :C].contiguous(), y[..., C:].contiguous()), s=(H, W), dim=(1, 2), norm="ortho")
    ref = ref + adds[0].double() + adds[1].double()
    rep = _Report()
    rep.err("chain", (H, W), ov.cpu(), ref)
    rep.check(_outside_unchanged(ob), "chain", (H, W), "channels outside the output slice changed")
    for t, k in zip((xb, a1b, a2b), keeps):
        rep.check(torch.equal(t.view(torch.int32), k.view(torch.int32)), "chain", (H, W), "an input map changed")
    rep.finish(record_property)
