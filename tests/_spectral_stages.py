"""What the per-stage tests of the spectral kernels share (test_spectral_gen_stages_gpu.py: the general lengths, csrc/resfft_gen.hip;
test_spectral_pow2_stages_gpu.py: the power-of-two squares, csrc/resfft_any.hip; test_spectral_train_stages_gpu.py: the 64 x 64
training kernels, csrc/resfft.hip and resfft4.hip): maps as channel slices of sentinel tensors, spectra
with sentinel floats behind them, the float64 reference of the column stage and the report of the worst error per stage.

Every map is a 32-channel slice (channel offset 8) of a 48-channel NHWC tensor whose other channels hold a sentinel, with one spare
image of NaN behind the batch; a spectrum is followed by TAIL sentinel values (NaN: a read of them poisons the output).  The maps
and spectra are fp32 unless a binary16 storage type is asked for; the NaN of either type carries a payload of its own."""
import torch

from _metrics import rel

C, LD, OFF = 32, 48, 8
TAIL = 4096                   # sentinel values behind R and T
SENT = 12345.678              # the channels outside a slice
SPARE_BITS = 0x7FC12345       # the spare image and the floats behind R and T: a quiet NaN with a payload of its own
SPARE_BITS_H = 0x7E45         # the same in binary16
BOUND = 1e-5


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale


def _bits(t):
    """t's words as integers (fp32: int32, binary16: int16)."""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _spare(dtype):
    return SPARE_BITS if dtype == torch.float32 else SPARE_BITS_H


def _sliced(v, dtype=torch.float32, ld=LD, off=OFF):
    """v (B, H, W, 32) on the CPU -> (base, view): the view holds v on the device as channels 8..39 of the first B images of a
    (B + 1, H, W, 48) sentinel tensor; the spare image is NaN.  (ld, off: another pixel stride and channel offset.)"""
    b, h, w, _ = v.shape
    base = torch.full((b + 1, h, w, ld), SENT, dtype=dtype, device="cuda")
    _bits(base[b]).fill_(_spare(dtype))
    view = base[:b, :, :, off:off + C]
    view.copy_(v)
    return base, view


def _outside_unchanged(base, off=OFF):
    """The sentinel channels and the spare image of a sliced map, bit for bit."""
    bits = _bits(base)
    want = _bits(torch.tensor(SENT, dtype=base.dtype)).item()
    return bool((bits[:-1, :, :, :off] == want).all() and (bits[:-1, :, :, off + C:] == want).all()
                and (bits[-1] == _spare(base.dtype)).all())


def _spectrum(batch, nkw, h, fill=None, dtype=torch.float32):
    """(flat, S): S = the first batch nkw h 64 values of flat as [batch][nkw][h][Re 32 | Im 32]; TAIL sentinel values follow."""
    n = batch * nkw * h * 64
    flat = torch.empty((n + TAIL,), dtype=dtype, device="cuda")
    _bits(flat[n:]).fill_(_spare(dtype))
    S = flat[:n].view(batch, nkw, h, 64)
    if fill is not None:
        S.copy_(fill)
    else:
        S.fill_(float("nan"))
    return flat, S


def _tail_unchanged(flat):
    return bool((_bits(flat[-TAIL:]) == _spare(flat.dtype)).all())


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _cplx(S):
    """[..., Re 32 | Im 32] -> complex128 on the CPU."""
    S = S.detach().cpu().double()
    return torch.complex(S[..., :C].contiguous(), S[..., C:].contiguous())


def _edges(w):
    return [0] + ([w // 2] if w % 2 == 0 else [])


def _mix_stages(Rin, w2, b2):
    """(S, Z, T) in float64, each (B, nkw, H, [Re 32 | Im 32]): S = fft_H(R), Z = [Re; Im]S W2^T + b2, T = ifft_H(relu Z), both
    ortho; T is the full complex result.  Differentiable in w2 and b2 when they are float64 leaves."""
    X = torch.fft.fft(_cplx(Rin), dim=2, norm="ortho")
    cat = torch.cat([X.real, X.imag], dim=-1)                                            # (B, nkw, H, 64)
    z = cat @ w2.double().t() + b2.double()
    y = torch.relu(z)
    T = torch.fft.ifft(torch.complex(y[..., :C].contiguous(), y[..., C:].contiguous()), dim=2, norm="ortho")
    return cat, z, torch.cat([T.real, T.imag], dim=-1)


def _mix_reference(Rin, w2, b2, w):
    """T = ifft_H(relu(W2 [Re; Im](fft_H(R)) + b2)), both ortho, the imaginary halves of column 0 and (even W) W/2 exactly 0."""
    ref = _mix_stages(Rin, w2, b2)[2]
    ref[:, _edges(w), :, C:] = 0.0
    return ref


def _back_reference(Tin, S):
    """c2r along W of T with the imaginary halves of the columns 0 and S/2 taken as zero, (B, S, S, 32) in float64."""
    Tc = _cplx(Tin)
    Tc.imag[:, [0, S // 2]] = 0.0
    return torch.fft.irfft(Tc.permute(0, 2, 3, 1), n=S, dim=3, norm="ortho").permute(0, 1, 3, 2)


class _Report:
    """Worst error per stage of one test item, and what failed."""

    def __init__(self):
        self.worst, self.fails = {}, []

    def err(self, stage, case, got, ref):
        e = rel(got, ref)
        if not e <= self.worst.get(stage, (-1.0, None))[0]:          # (a NaN error is kept too)
            self.worst[stage] = (e, case)
        if not e < BOUND:
            d = (torch.as_tensor(got).double().cpu() - torch.as_tensor(ref).double().cpu()).abs()
            at = tuple(int(i) for i in torch.unravel_index(d.argmax(), d.shape))
            self.fails.append(f"{stage} {case}: rel {e:.3e}, largest difference at {at}")

    def check(self, ok, stage, case, what):
        if not ok:
            self.fails.append(f"{stage} {case}: {what}")

    def finish(self, record_property):
        text = ", ".join(f"{s} {e:.3e} at {c}" for s, (e, c) in sorted(self.worst.items()))
        for s, (e, c) in self.worst.items():
            record_property(f"worst_{s}", f"{e:.3e} at {c}")
        print(f"\nworst rel per stage: {text}")
        assert not self.fails, f"worst rel per stage: {text}; failed: " + "; ".join(self.fails)
