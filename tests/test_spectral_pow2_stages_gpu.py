"""The whole-slice spectral kernels of the power-of-two squares (csrc/resfft_any.hip: rfft_rows_any_kernel, spec_mix_any_kernel,
irfft_rows_any_kernel) stage by stage against torch.fft on the CPU in float64 -- rows forward, columns + mix + columns back, rows
back, and the three chained -- at every side the entry points take (64, 128, 256, 512), each at a batch of one and at the smallest
batch at which a workgroup of every one of the three persistent kernels takes a second unit (SIDES; test_spectral_pow2_cpu.py proves
that from a restatement of the launcher's grid formula).  Only there do the prefetch of a workgroup's next unit, the split early /
late prefetch of the mix and the reversed walk over more than one round run; at 128 and 256 the last round is ragged as well.

What the generator's own passes cannot show is checked here: the imaginary halves of the columns 0 and S/2 are written as exact
zeros by the rows and the mix, are not read by the mix (they hold NaN) and are ignored by the rows back (finite garbage, and NaN);
maps are 32-channel slices (channel offset 8, pixel stride 48) of sentinel tensors with a spare NaN image behind the batch, the
spectra are followed by NaN sentinels, the residual operands come in every combination, and nothing outside an output changes
(tests/_spectral_stages.py, shared with the general-length module).

fp32 bound: rel < 1e-5 per stage and for the chain, the bound of the other stage kernels (test_kernels_gpu.py::
test_spectral_path_kernels, test_spectral_gen_stages_gpu.py).  binary16 storage (sides 128 / 256 / 512, the larger batch): each
launch against the fp32 launch on the same rounded inputs, one rounding exactly (_metrics.one_rounding); the fp32 launch at that
shape is what the float64 comparison has validated.  Measured values: DESIGN 3.3."""
import pytest
import torch

from _metrics import one_rounding
from _spectral_stages import (C, _Report, _back_reference, _bits, _mix_reference, _outside_unchanged, _ptr, _randn, _same_bits, _sliced,
                              _spectrum, _tail_unchanged)

pytestmark = pytest.mark.gpu

# side -> (a batch of one round, the smallest batch at which each of the three kernels has more units than workgroups)
SIDES = {64: (1, 17), 128: (1, 9), 256: (1, 5), 512: (1, 2)}
HALF_SIDES = (128, 256, 512)
SHAPES = [(S, B) for S, bs in SIDES.items() for B in bs]
GARBAGE = 7777.25             # finite garbage in the imaginary halves of T's columns 0 and S/2


# ------------------------------------------------------------------ a RESTATEMENT of the launchers of csrc/resfft_any.hip
# (persistent_grid, launch_rfft_rows, launch_spec_mix_form<PACK = true>, launch_irfft_rows): it has to follow them.  If the
# grid formula, the LDS footprints or the units per image change there, change them here, and SIDES with them.
N_CU, LDS_PER_CU, MAX_WG_PER_CU = 256, 160 * 1024, 2


def persistent_grid(units, lds_bytes):
    per_cu = max(1, min(MAX_WG_PER_CU, LDS_PER_CU // (lds_bytes + 1024)))
    return min(units, N_CU * per_cu)


def row_lds_bytes(S):
    return S * 256 + S * 4                                    # [S][32] re + im, twiddles


def mix_lds_bytes(S):
    return 2 * S * 34 * 4 + S * 4 + (64 * 64 + 64) * 4        # [S][34] re + im, twiddles, W2 and b2


def units_and_grids(S, B):
    """{kernel: (units, workgroups)} of the three launches at side S and batch B (the mix in its packed form: S/2 units per image)."""
    units = B * S // 2
    return {"rows": (units, persistent_grid(units, row_lds_bytes(S))), "mix": (units, persistent_grid(units, mix_lds_bytes(S))),
            "back": (units, persistent_grid(units, row_lds_bytes(S)))}


# ------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def mix_weights(hip_lib):
    from mtd_gan_amd import kernels as K
    w2 = _randn(64, 64, seed=42, scale=0.125)
    b2 = _randn(64, seed=43, scale=0.1)
    return w2, b2, K.transpose64(w2.cuda()), b2.cuda()


def _edge_halves(t):
    """The imaginary halves of the columns 0 and S/2 of a spectrum (B, S/2 + 1, S, 64)."""
    return t[:, [0, t.shape[1] - 1], :, C:]


def _edges_exactly_zero(t):
    return bool((_bits(_edge_halves(t).contiguous()) == 0).all())


def _rows_input(S, B):
    return _randn(B, S, S, C, seed=1000 + 8 * S + B)


def _mix_input(S, B):
    """R, random and not Hermitian-consistent; (what the kernel gets: NaN in the halves that are not to be read, what the reference gets: zeros)."""
    Rin = _randn(B, S // 2 + 1, S, 64, seed=2000 + 8 * S + B)
    Rref = Rin.clone()
    _edge_halves_set(Rin, float("nan"))
    _edge_halves_set(Rref, 0.0)
    return Rin, Rref


def _edge_halves_set(t, value):
    t[:, 0, :, C:] = value
    t[:, t.shape[1] - 1, :, C:] = value


# --------------------------------------------------------------------------------------------------------- fp32 stages
@pytest.mark.parametrize("S,B", SHAPES)
def test_rows_forward(hip_lib, record_property, S, B):
    """mtd_rfft_rows_any against rfft along W."""
    from mtd_gan_amd import kernels as K
    nkw, case = S // 2 + 1, f"S = {S}, B = {B}"
    x = _rows_input(S, B)
    xb, xv = _sliced(x)
    keep = xb.clone()
    flat, R = _spectrum(B, nkw, S)
    K.check(hip_lib.mtd_rfft_rows_any(xv.data_ptr(), K.ld_of(xv), R.data_ptr(), B, S, K.stream_ptr()), "mtd_rfft_rows_any")
    ref = torch.fft.rfft(x.double(), dim=2, norm="ortho").permute(0, 2, 1, 3)            # (B, nkw, H, C)
    got = R.cpu()
    rep = _Report()
    rep.err("rows_re", case, got[..., :C], ref.real)
    rep.err("rows_im", case, got[..., C:], ref.imag)
    rep.check(_edges_exactly_zero(got), "rows", case, "an imaginary half of column 0 / S/2 is not exactly zero")
    rep.check(_tail_unchanged(flat), "rows", case, "the floats behind R changed")
    rep.check(_same_bits(xb, keep), "rows", case, "the input map changed")
    rep.finish(record_property)


@pytest.mark.parametrize("S,B", SHAPES)
def test_columns_mix(hip_lib, mix_weights, record_property, S, B):
    """mtd_spec_mix_any against ifft_H(relu(W2 fft_H(R) + b2)); the imaginary halves of R's columns 0 and S/2 hold NaN."""
    from mtd_gan_amd import kernels as K
    w2, b2, w2t, b2d = mix_weights
    nkw, case = S // 2 + 1, f"S = {S}, B = {B}"
    Rin, Rref = _mix_input(S, B)
    rflat, R = _spectrum(B, nkw, S, Rin)
    keep = rflat.clone()
    tflat, T = _spectrum(B, nkw, S)
    K.check(hip_lib.mtd_spec_mix_any(R.data_ptr(), w2t.data_ptr(), b2d.data_ptr(), T.data_ptr(), B, S, K.stream_ptr()), "mtd_spec_mix_any")
    got = T.cpu()
    rep = _Report()
    rep.err("mix", case, got, _mix_reference(Rref, w2, b2, S))
    rep.check(_edges_exactly_zero(got), "mix", case, "an imaginary half of column 0 / S/2 is not exactly zero")
    rep.check(_tail_unchanged(tflat), "mix", case, "the floats behind T changed")
    rep.check(_same_bits(rflat, keep), "mix", case, "R or the floats behind it changed")
    rep.finish(record_property)


def _back_cases(S):
    """(add1, add2, what the imaginary halves of T's columns 0 and S/2 hold); both fillings occur with and without operands."""
    if S == 512:
        return [(True, True, GARBAGE), (False, False, float("nan"))]
    return [(True, True, GARBAGE), (True, False, float("nan")), (False, True, GARBAGE), (False, False, float("nan"))]


@pytest.mark.parametrize("S,B", SHAPES)
def test_rows_back(hip_lib, record_property, S, B):
    """mtd_irfft_rows_any against irfft along W + the residual operands that are present."""
    from mtd_gan_amd import kernels as K
    nkw = S // 2 + 1
    Tin = _randn(B, nkw, S, 64, seed=3000 + 8 * S + B)
    ref0 = _back_reference(Tin, S)
    adds_cpu = [_randn(B, S, S, C, seed=4000 + 16 * S + 2 * B + i) for i in range(2)]
    adds_dev = [_sliced(a) for a in adds_cpu]
    adds_keep = [b.clone() for b, _ in adds_dev]
    rep = _Report()
    for use1, use2, fill in _back_cases(S):
        case = f"S = {S}, B = {B}, adds ({use1}, {use2}), edge halves {fill}"
        _edge_halves_set(Tin, fill)
        tflat, T = _spectrum(B, nkw, S, Tin)
        keep = tflat.clone()
        a1 = adds_dev[0][1] if use1 else None
        a2 = adds_dev[1][1] if use2 else None
        ob, ov = _sliced(torch.full((B, S, S, C), float("nan")))
        K.check(hip_lib.mtd_irfft_rows_any(T.data_ptr(), ov.data_ptr(), K.ld_of(ov), _ptr(a1), K.ld_of(a1) if a1 is not None else 0,
                                           _ptr(a2), K.ld_of(a2) if a2 is not None else 0, B, S, K.stream_ptr()), "mtd_irfft_rows_any")
        ref = ref0
        for a, use in zip(adds_cpu, (use1, use2)):
            if use:
                ref = ref + a.double()
        rep.err("back", case, ov.cpu(), ref)
        rep.check(_outside_unchanged(ob), "back", case, "channels outside the output slice, or the spare image, changed")
        rep.check(_same_bits(tflat, keep), "back", case, "T or the floats behind it changed")
        for (b, _), k in zip(adds_dev, adds_keep):
            rep.check(_same_bits(b, k), "back", case, "an add map changed")
    rep.finish(record_property)


@pytest.mark.parametrize("S", list(SIDES))
def test_chained_stages(hip_lib, mix_weights, record_property, S):
    """kernels.spectral_branch_any against irfft2(relu(W2 rfft2(x) + b2)) + add1 + add2 at the larger batch of every side."""
    from mtd_gan_amd import kernels as K
    w2, b2, w2t, b2d = mix_weights
    B = SIDES[S][1]
    x = _randn(B, S, S, C, seed=5000 + S)
    adds = [_randn(B, S, S, C, seed=6000 + 2 * S + i) for i in range(2)]
    xb, xv = _sliced(x)
    (a1b, a1), (a2b, a2) = [_sliced(a) for a in adds]
    keeps = [t.clone() for t in (xb, a1b, a2b)]
    ob, ov = _sliced(torch.full((B, S, S, C), float("nan")))
    K.spectral_branch_any(xv, w2t, b2d, ov, add1=a1, add2=a2)
    f = torch.fft.rfft2(x.double(), s=(S, S), dim=(1, 2), norm="ortho")                  # (B, H, nkw, C)
    y = torch.relu(torch.cat([f.real, f.imag], dim=-1) @ w2.double().t() + b2.double())
    ref = torch.fft.irfft2(torch.complex(y[..., :C].contiguous(), y[..., C:].contiguous()), s=(S, S), dim=(1, 2), norm="ortho")
    ref = ref + adds[0].double() + adds[1].double()
    rep, case = _Report(), f"S = {S}, B = {B}"
    rep.err("chain", case, ov.cpu(), ref)
    rep.check(_outside_unchanged(ob), "chain", case, "channels outside the output slice, or the spare image, changed")
    for t, k in zip((xb, a1b, a2b), keeps):
        rep.check(_same_bits(t, k), "chain", case, "an input map changed")
    rep.finish(record_property)


# ---------------------------------------------------------------------------------------------------- binary16 storage
def _ratio(h, f):
    """max |h - f| / (2^-11 |f| + 2^-24): what one_rounding holds to 1, for the report."""
    h, f = h.double().cpu(), f.double().cpu()
    return ((h - f).abs() / (2.0 ** -11 * f.abs() + 2.0 ** -24)).max().item()


def _one_rounding(record_property, stage, case, h, f):
    assert h.dtype == torch.float16 and f.dtype == torch.float32
    record_property(f"worst_ratio_{stage}", f"{_ratio(h, f):.4f} at {case}")
    one_rounding(f"{stage} {case}", h, f)


@pytest.mark.parametrize("S", HALF_SIDES)
def test_rows_forward_binary16(hip_lib, record_property, S):
    """kernels.rfft_rows_any on a binary16 slice against the fp32 launch on the same values."""
    from mtd_gan_amd import kernels as K
    B, nkw = SIDES[S][1], S // 2 + 1
    case = f"S = {S}, B = {B}"
    xh = _rows_input(S, B).half()
    hb, hv = _sliced(xh, torch.float16)
    fb, fv = _sliced(xh.float())
    keep = hb.clone()
    Rh = K.rfft_rows_any(hv)
    Rf = K.rfft_rows_any(fv)
    assert Rh.dtype == torch.float16 and tuple(Rh.shape) == (B, nkw, S, 64)
    # the same launch into a spectrum with sentinels behind it (the wrapper allocates its own): the same bits, the sentinels kept
    flat, R = _spectrum(B, nkw, S, dtype=torch.float16)
    K.check(hip_lib.mtd_rfft_rows_any_h(hv.data_ptr(), K.ld_of(hv), R.data_ptr(), B, S, K.stream_ptr()), "mtd_rfft_rows_any_h")
    assert _same_bits(R, Rh), "two launches on the same input differ"
    assert _tail_unchanged(flat), "the values behind R changed"
    assert _same_bits(hb, keep), "the input map changed"
    assert _edges_exactly_zero(Rh), "an imaginary half of column 0 / S/2 is not exactly zero"
    _one_rounding(record_property, "rows", case, Rh, Rf)


@pytest.mark.parametrize("S", HALF_SIDES)
def test_columns_mix_binary16(hip_lib, mix_weights, record_property, S):
    """kernels.spec_mix_any on a binary16 spectrum (NaN in the halves that are not to be read) against the fp32 launch."""
    from mtd_gan_amd import kernels as K
    _, _, w2t, b2d = mix_weights
    B, nkw = SIDES[S][1], S // 2 + 1
    case = f"S = {S}, B = {B}"
    Rin = _mix_input(S, B)[0].half()
    rflat, Rh = _spectrum(B, nkw, S, Rin, dtype=torch.float16)
    keep = rflat.clone()
    Th = K.spec_mix_any(Rh, w2t, b2d)
    Tf = K.spec_mix_any(Rin.float().cuda(), w2t, b2d)
    assert Th.dtype == torch.float16 and tuple(Th.shape) == (B, nkw, S, 64)
    tflat, T = _spectrum(B, nkw, S, dtype=torch.float16)
    K.check(hip_lib.mtd_spec_mix_any_h(Rh.data_ptr(), w2t.data_ptr(), b2d.data_ptr(), T.data_ptr(), B, S, K.stream_ptr()), "mtd_spec_mix_any_h")
    assert _same_bits(T, Th), "two launches on the same input differ"
    assert _tail_unchanged(tflat), "the values behind T changed"
    assert _same_bits(rflat, keep), "R or the values behind it changed"
    assert _edges_exactly_zero(Th), "an imaginary half of column 0 / S/2 is not exactly zero"
    _one_rounding(record_property, "mix", case, Th, Tf)


@pytest.mark.parametrize("S", HALF_SIDES)
def test_rows_back_binary16(hip_lib, record_property, S):
    """kernels.irfft_rows_any on binary16 slices against the fp32 launch: two operands with finite garbage in the imaginary halves of
    T's columns 0 and S/2, none with NaN there."""
    from mtd_gan_amd import kernels as K
    B, nkw = SIDES[S][1], S // 2 + 1
    Tin = _randn(B, nkw, S, 64, seed=3000 + 8 * S + B).half()
    adds_cpu = [_randn(B, S, S, C, seed=4000 + 16 * S + 2 * B + i).half() for i in range(2)]
    adds_h = [_sliced(a, torch.float16) for a in adds_cpu]
    adds_f = [_sliced(a.float()) for a in adds_cpu]
    adds_keep = [b.clone() for b, _ in adds_h]
    for use, fill in ((True, GARBAGE), (False, float("nan"))):
        case = f"S = {S}, B = {B}, adds {use}, edge halves {fill}"
        _edge_halves_set(Tin, fill)
        tflat, Th = _spectrum(B, nkw, S, Tin, dtype=torch.float16)
        keep = tflat.clone()
        hb, hv = _sliced(torch.full((B, S, S, C), float("nan")), torch.float16)
        fb, fv = _sliced(torch.full((B, S, S, C), float("nan")))
        K.irfft_rows_any(Th, hv, add1=adds_h[0][1] if use else None, add2=adds_h[1][1] if use else None)
        K.irfft_rows_any(Tin.float().cuda(), fv, add1=adds_f[0][1] if use else None, add2=adds_f[1][1] if use else None)
        assert _outside_unchanged(hb), (case, "channels outside the output slice, or the spare image, changed")
        assert _same_bits(tflat, keep), (case, "T or the values behind it changed")
        for (b, _), k in zip(adds_h, adds_keep):
            assert _same_bits(b, k), (case, "an add map changed")
        _one_rounding(record_property, "back_adds" if use else "back_plain", case, hv, fv)
