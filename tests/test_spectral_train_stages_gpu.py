"""The spectral kernels of the training step (64 x 64 patches; csrc/resfft.hip: rfft_rows_kernel, irfft_rows_kernel, the one-wave
spec_mix_fwd_kernel / spec_mix_bwd_kernel and the slab reduces; csrc/resfft4.hip: the four-wave spec_mix_fwd4_kernel<1> /
spec_mix_bwd4_kernel) stage by stage, forward and backward, against torch.fft / matmul on the CPU in float64.

What test_kernels_gpu.py::test_spectral_path_kernels and the whole-step tests cannot show is checked here: the backward mix on
inputs of its own (gT with its halving, every per-unit slab, the single-column last unit of a patch), every bit of the four-wave
sign mask and the words of it that no column owns, the slab reduce on synthetic slabs at every branch of block_slab_sum<8>
(REDUCE_BATCHES), its fallback levels (FALLBACK_BATCHES), the table launch, all eight epilogues of the rows back, odd pixel
strides, and the launch without a tape.  test_spectral_train_cpu.py proves the batch lists from the restatements below.

Maps are 32-channel slices of sentinel tensors with a spare NaN image, spectra, masks and workspaces are followed by sentinels
(tests/_spectral_stages.py).  Bound: _spectral_stages.BOUND (rel < 1e-5) for every stage; measured values: DESIGN 3.2.

Out of scope: spec_mix_fwd4_kernel<2> (a pair of columns per workgroup) is reachable only through a lab variable that the library
reads once per process."""
import ctypes

import numpy as np
import pytest
import torch

from _spectral_stages import (BOUND, C, SPARE_BITS, TAIL, _Report, _back_reference, _bits, _mix_stages, _outside_unchanged, _ptr,
                              _randn, _same_bits, _sliced, _spectrum, _tail_unchanged)

pytestmark = pytest.mark.gpu

NKW, UNITS, WORDS = 33, 17, 128       # columns of a half spectrum, units (column pairs) per patch, 64-bit mask words per unit
FORMS = [True, False]                 # four_wave


# --------------------------------------------------------- RESTATEMENTS of csrc/resfft.hip, resfft4.hip and common.h: they
# have to follow the sources (MIX_SLAB, MIX_GS, the 4096-slab rule of the fused reduce, mask_word / mask_bit, block_slab_sum<8>).
SLAB = 64 * 64 + 128                  # dW2 partial, then one db2 row per column of the unit
MIX_GS = 32                           # slabs per group of a fallback level
FUSED_MAX = 4096                      # the fused reduce takes at most this many slabs
REDUCE_BATCHES = (1, 4, 16, 29, 45, 240)
FALLBACK_BATCHES = (1, 3, 61, 241)    # (241 by the size rule, the others through a dw2 that is not 16-byte aligned)


def mask_positions():
    """(word, bit) of element (k2, kh, o) of a unit's sign mask, each (2, 64, 64)."""
    k2, kh, o = np.meshgrid(np.arange(2), np.arange(64), np.arange(64), indexing="ij")
    r32 = kh & 31
    word = ((k2 * 2 + kh // 32) * 2 + o // 32) * 16 + (r32 & 3) + 4 * (r32 >> 3)
    bit = (o & 31) + 32 * ((r32 >> 2) & 1)
    return word, bit


def _mask_index():
    word, bit = mask_positions()
    return (word * 64 + bit).reshape(-1)


def mask_encode(pos, absent=0x00):
    """pos (B, 33, 64, 64) Boolean over (b, kw, kh, o) -> the mask's bytes (B 17 128 8, little-endian words); every byte of the 64
    words that belong to the absent second column of unit 16 is `absent`."""
    pos = np.asarray(pos, dtype=bool)
    B = pos.shape[0]
    padded = np.zeros((B, 2 * UNITS, 64, 64), dtype=np.uint8)
    padded[:, :NKW] = pos
    bits = np.zeros((B, UNITS, WORDS * 64), dtype=np.uint8)
    bits[:, :, _mask_index()] = padded.reshape(B, UNITS, WORDS * 64)
    by = np.packbits(bits.reshape(B, UNITS, WORDS, 64), axis=-1, bitorder="little")
    by[:, UNITS - 1, WORDS // 2:] = absent
    return torch.from_numpy(by.reshape(-1))


def mask_decode(by, B):
    """The inverse of mask_encode: bytes -> (B, 33, 64, 64) Boolean."""
    by = np.asarray(by, dtype=np.uint8).reshape(B, UNITS, WORDS, 8)
    bits = np.unpackbits(by, axis=-1, bitorder="little").reshape(B, UNITS, WORDS * 64)
    return torch.from_numpy(bits[:, :, _mask_index()].reshape(B, 2 * UNITS, 64, 64)[:, :NKW].astype(bool))


def run_batches(ns):
    """block_slab_sum<8> on ns slabs: (per, [(8-load batches, 4-load batches, single loads) of each of the 64 runs])."""
    per = -(-ns // 64)
    runs = []
    for ty in range(64):
        k0 = min(ns, ty * per)
        n = min(ns, k0 + per) - k0
        runs.append((n // 8, (n % 8) // 4, n % 4))
    return per, runs


def fallback_levels(ns):
    """The slab counts that the fallback reduce walks: [ns, groups of level 1, ...]; mix_finish_kernel sums the last."""
    levels = [ns]
    while levels[-1] > MIX_GS:
        levels.append(-(-levels[-1] // MIX_GS))
    return levels


def ws_floats(B):
    """mix_ws_floats: the unit slabs and every level's group slabs."""
    return sum(fallback_levels(17 * B)) * SLAB


# ------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def mix_weights(hip_lib):
    from mtd_gan_amd import kernels as K
    w2 = _randn(64, 64, seed=42, scale=0.125)
    b2 = _randn(64, seed=43, scale=0.1)
    return w2, b2, w2.cuda(), K.transpose64(w2.cuda()), b2.cuda()


def _form(four_wave):
    return "four" if four_wave else "one"


def _nan_floats(n):
    """n floats of the sentinel NaN on the device."""
    flat = torch.empty((n,), dtype=torch.float32, device="cuda")
    _bits(flat).fill_(SPARE_BITS)
    return flat


def _is_sentinel(t):
    return bool((_bits(t) == SPARE_BITS).all())


def _workspace(L, B):
    """(flat, n): a slab workspace of exactly mtd_spec_mix_bwd_ws_bytes(B) = 4 n bytes with TAIL sentinels behind it, all NaN."""
    nbytes = L.mtd_spec_mix_bwd_ws_bytes(B)
    assert nbytes == 4 * ws_floats(B)
    return _nan_floats(nbytes // 4 + TAIL), nbytes // 4


def _guarded(n, lead):
    """(flat, view): n floats that start `lead` floats into a NaN buffer and are followed by 64 more."""
    flat = _nan_floats(lead + n + 64)
    return flat, flat[lead:lead + n]


def _guards_unchanged(flat, n, lead):
    return _is_sentinel(flat[:lead]) and _is_sentinel(flat[lead + n:])


MASK_TAIL = 0xC3                      # the bytes behind a sign mask


def _mask_buffer(L, B, fill):
    """(flat, Z): a sign mask of mtd_spec_mix_zmask_bytes(B) bytes with TAIL bytes behind it; fill: a byte, or the mask's bytes."""
    n = L.mtd_spec_mix_zmask_bytes(B)
    assert n == B * UNITS * WORDS * 8
    flat = torch.full((n + TAIL,), MASK_TAIL, dtype=torch.uint8, device="cuda")
    if isinstance(fill, int):
        flat[:n].fill_(fill)
    else:
        flat[:n].copy_(fill)
    return flat, flat[:n]


def _mask_tail_unchanged(flat):
    return bool((flat[-TAIL:] == MASK_TAIL).all())


def _rms(t):
    return t.double().pow(2).mean().sqrt().item()


# -------------------------------------------------------------------------------------------------------------- launches
def _rows(L, xv, R, B, col_weight):
    from mtd_gan_amd import kernels as K
    K.check(L.mtd_rfft_rows(xv.data_ptr(), K.ld_of(xv), R.data_ptr(), B, col_weight, K.stream_ptr()), "mtd_rfft_rows")


def _mix_fwd(L, four_wave, R, w2t, b2d, T, S, Z, B):
    from mtd_gan_amd import kernels as K
    f, name = (L.mtd_spec_mix_fwd4, "mtd_spec_mix_fwd4") if four_wave else (L.mtd_spec_mix_fwd, "mtd_spec_mix_fwd")
    K.check(f(R.data_ptr(), w2t.data_ptr(), b2d.data_ptr(), T.data_ptr(), _ptr(S), _ptr(Z), B, K.stream_ptr()), name)


def _mix_bwd(L, four_wave, gR, w2d, S, Z, gT, ws, B):
    from mtd_gan_amd import kernels as K
    f, name = (L.mtd_spec_mix_bwd4, "mtd_spec_mix_bwd4") if four_wave else (L.mtd_spec_mix_bwd, "mtd_spec_mix_bwd")
    K.check(f(gR.data_ptr(), w2d.data_ptr(), S.data_ptr(), Z.data_ptr(), gT.data_ptr(), ws.data_ptr(), B, K.stream_ptr()), name)


def _reduce(L, ws, B, dw2, db2, accumulate):
    from mtd_gan_amd import kernels as K
    K.check(L.mtd_spec_mix_wgrad_reduce(ws.data_ptr(), B, dw2.data_ptr(), db2.data_ptr(), accumulate, K.stream_ptr()),
            "mtd_spec_mix_wgrad_reduce")


def _reduce_multi(L, descs):
    from mtd_gan_amd import kernels as K
    tab, host = K.device_table(descs, torch.device("cuda", torch.cuda.current_device()))
    K.check(L.mtd_spec_mix_wgrad_reduce_multi(tab.data_ptr(), ctypes.cast(host, ctypes.c_void_p), len(descs), K.stream_ptr()),
            "mtd_spec_mix_wgrad_reduce_multi")


# -------------------------------------------------------------------------------------------------- 1. rows forward
@pytest.mark.parametrize("B,col_weight,ld,off", [(1, 0, 48, 8), (1, 1, 48, 8), (3, 0, 48, 8), (3, 1, 48, 8), (1, 1, 33, 1)])
def test_rows_forward(hip_lib, record_property, B, col_weight, ld, off):
    """mtd_rfft_rows against rfft along W, columns 1..31 doubled under col_weight; the last item at an odd pixel stride."""
    case = f"B = {B}, col_weight = {col_weight}, x_ld = {ld}"
    x = _randn(B, 64, 64, C, seed=100 + B)
    xb, xv = _sliced(x, ld=ld, off=off)
    keep = xb.clone()
    flat, R = _spectrum(B, NKW, 64)
    _rows(hip_lib, xv, R, B, col_weight)
    ref = torch.fft.rfft(x.double(), dim=2, norm="ortho").permute(0, 2, 1, 3).clone()    # (B, kw, h, c)
    if col_weight:
        ref[:, 1:32] *= 2.0
    got = R.cpu()
    rep = _Report()
    rep.check(bool(torch.isfinite(got).all()), "rows", case, "R is not finite")
    rep.err("rows_re", case, got[..., :C], ref.real)
    rep.err("rows_im", case, got[..., C:], ref.imag)
    rep.check(bool((got[:, [0, 32], :, C:] == 0.0).all()), "rows", case, "an imaginary half of column 0 / 32 is not exactly zero")
    rep.check(_tail_unchanged(flat), "rows", case, "the floats behind R changed")
    rep.check(_same_bits(xb, keep), "rows", case, "the input map changed")
    rep.finish(record_property)


# ------------------------------------------------------------------------------------------------ 2. forward mix stage
def _forward_case(L, rep, case, four_wave, Rin, w2t, b2d):
    """Launch with the tape and without; checks the sentinels and that both give the same T.  Returns (S, T, Z) on the CPU (Z: the
    mask's bytes, or the float tensor)."""
    B = Rin.shape[0]
    rflat, R = _spectrum(B, NKW, 64, Rin)
    keep = rflat.clone()
    sflat, S = _spectrum(B, NKW, 64)
    tflat, T = _spectrum(B, NKW, 64)
    zflat, Z = _mask_buffer(L, B, 0xFF) if four_wave else _spectrum(B, NKW, 64)
    _mix_fwd(L, four_wave, R, w2t, b2d, T, S, Z, B)
    t2flat, T2 = _spectrum(B, NKW, 64)
    _mix_fwd(L, four_wave, R, w2t, b2d, T2, None, None, B)
    rep.check(_same_bits(T2, T), "mix", case, "the launch without a tape gives another T")
    rep.check(_tail_unchanged(sflat) and _tail_unchanged(tflat) and _tail_unchanged(t2flat), "mix", case, "the floats behind S or T changed")
    rep.check(_mask_tail_unchanged(zflat) if four_wave else _tail_unchanged(zflat), "mix", case, "what lies behind Z changed")
    rep.check(_same_bits(rflat, keep), "mix", case, "R or the floats behind it changed")
    rep.check(bool(torch.isfinite(S).all() and torch.isfinite(T).all()), "mix", case, "S or T is not finite")
    return S.cpu(), T.cpu(), Z.cpu()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("four_wave", FORMS)
def test_forward_mix(hip_lib, mix_weights, record_property, four_wave, B):
    """mtd_spec_mix_fwd4 / mtd_spec_mix_fwd: S, T (Z of the one-wave form) against float64; every bit of the four-wave sign mask
    against the sign of the float64 Z where |Z| >= 2 BOUND rms(Z) (a float32 Z within BOUND of it cannot have another sign there);
    the 64 words of unit 16 that no column owns keep the prefill; the launch without a tape gives the same T."""
    w2, b2, _, w2t, b2d = mix_weights
    form, case = _form(four_wave), f"B = {B}"
    Rin = _randn(B, NKW, 64, 64, seed=200 + B, scale=0.5)
    rep = _Report()
    S, T, Z = _forward_case(hip_lib, rep, case, four_wave, Rin, w2t, b2d)
    S64, Z64, T64 = _mix_stages(Rin, w2, b2)
    rep.err(f"fwd_S_{form}", case, S, S64)
    rep.err(f"fwd_T_{form}", case, T, T64)
    if four_wave:
        margin = 2.0 * BOUND * _rms(Z64)
        sure = Z64.abs() >= margin
        share = 1.0 - sure.double().mean().item()
        print(f"\nsign mask: {sure.numel() - int(sure.sum())} of {sure.numel()} elements under the margin {margin:.3e} (share {share:.3e})")
        record_property("mask_excluded_share", f"{share:.3e}")
        wrong = (mask_decode(Z.numpy(), B) != (Z64 > 0)) & sure
        rep.check(not bool(wrong.any()), "mask", case, f"{int(wrong.sum())} sign bits differ from the float64 Z outside the margin")
        rep.check(share <= 1e-4, "mask", case, f"{share:.3e} of the elements lie under the margin")
        absent = Z.view(B, UNITS, WORDS, 8)[:, UNITS - 1, WORDS // 2:]
        rep.check(bool((absent == 0xFF).all()), "mask", case, "the words of unit 16's absent column were written")
    else:
        rep.check(bool(torch.isfinite(Z).all()), "mix", case, "Z is not finite")
        rep.err(f"fwd_Z_{form}", case, Z, Z64)
    rep.finish(record_property)


@pytest.mark.parametrize("four_wave", FORMS)
def test_forward_mix_exact_zero(hip_lib, mix_weights, record_property, four_wave):
    """A patch of zeros between two random ones, b2 with exact +0 and -0 entries: Z of that patch is b2 exactly, so its mask bits are
    b2 > 0 -- 0 where b2 is +0 or -0 -- and the one-wave Z equals b2."""
    w2, b2, _, w2t, _ = mix_weights
    form, B, case = _form(four_wave), 3, "B = 3, patch 1 zero"
    b2e = b2.clone()
    b2e[[3, 40]] = 0.0
    b2e[[17, 62]] = -0.0
    Rin = _randn(B, NKW, 64, 64, seed=210, scale=0.5)
    Rin[1] = 0.0
    rep = _Report()
    S, T, Z = _forward_case(hip_lib, rep, case, four_wave, Rin, w2t, b2e.cuda())
    S64, Z64, T64 = _mix_stages(Rin, w2, b2e)
    rep.err(f"fwd_S_{form}", case, S, S64)
    rep.err(f"fwd_T_{form}", case, T, T64)
    want = b2e.expand(NKW, 64, 64)
    if four_wave:
        got = mask_decode(Z.numpy(), B)[1]
        rep.check(not bool(got[..., [3, 40, 17, 62]].any()), "mask", case, "a bit of an exactly zero Z is set")
        rep.check(torch.equal(got, want > 0), "mask", case, "the bits of the zero patch are not b2 > 0")
    else:
        rep.check(bool((Z[1] == want).all()), "mix", case, "Z of the zero patch is not b2")
        rep.err(f"fwd_Z_{form}", case, Z, Z64)
    rep.finish(record_property)


# ----------------------------------------------------------------------------------------------- 3. backward mix stage
def _backward_reference(gR, S, pos, w2):
    """float64: gT (B, 33, 64, 64) and the slabs (B, 17, SLAB) of gZ = pos fft_H(gR), gS = gZ W2, gT = ifft_H(gS) halved at
    columns 1..31; slab of unit (b, p): dW2[o][k] = sum over both columns and kh of gZ[.][o] S[.][k], then one db2 row per column."""
    B = gR.shape[0]
    G = torch.fft.fft(torch.complex(gR[..., :C].double(), gR[..., C:].double()), dim=2, norm="ortho")
    gZ = torch.cat([G.real, G.imag], dim=-1) * pos.double()
    gS = gZ @ w2.double()
    T = torch.fft.ifft(torch.complex(gS[..., :C].contiguous(), gS[..., C:].contiguous()), dim=2, norm="ortho")
    gT = torch.cat([T.real, T.imag], dim=-1)
    gT[:, 1:32] *= 0.5
    gZp = torch.zeros(B, 2 * UNITS, 64, 64, dtype=torch.float64)
    Sp = torch.zeros(B, 2 * UNITS, 64, 64, dtype=torch.float64)
    gZp[:, :NKW], Sp[:, :NKW] = gZ, S.double()
    gZp, Sp = gZp.view(B, UNITS, 2, 64, 64), Sp.view(B, UNITS, 2, 64, 64)
    dW = torch.einsum("bpjfo,bpjfk->bpok", gZp, Sp).reshape(B, UNITS, 4096)
    db = gZp.sum(dim=3).reshape(B, UNITS, 128)
    return gT, torch.cat([dW, db], dim=-1)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("four_wave", FORMS)
def test_backward_mix(hip_lib, mix_weights, record_property, four_wave, B):
    """mtd_spec_mix_bwd4 / mtd_spec_mix_bwd on inputs of their own (cotangent, saved spectrum, a random mask): gT and every unit's
    slab against float64.  Four-wave form: the mask goes in through mask_encode, and the words of unit 16 that no column owns change
    nothing, whatever they hold.  One-wave form: the mask is a float Z of positive and negative values, +0 and -0."""
    L = hip_lib
    w2, _, w2d, _, _ = mix_weights
    form, case = _form(four_wave), f"B = {B}"
    gRin = _randn(B, NKW, 64, 64, seed=300 + B)
    Sin = _randn(B, NKW, 64, 64, seed=310 + B, scale=0.5)
    gen = torch.Generator().manual_seed(320 + B)
    kind = torch.randint(0, 4, (B, NKW, 64, 64), generator=gen)          # 0, 1: positive; 2: negative; 3: +0 or -0
    pos = kind < 2
    gflat, gR = _spectrum(B, NKW, 64, gRin)
    sflat, S = _spectrum(B, NKW, 64, Sin)
    if four_wave:
        fills = (0xA5, 0xFF, 0x00)
    else:
        mag = _randn(B, NKW, 64, 64, seed=330 + B).abs() + 0.05
        zero = torch.where(torch.rand(B, NKW, 64, 64, generator=gen) < 0.5, 0.0, -0.0)
        Zin = torch.where(pos, mag, torch.where(kind == 2, -mag, zero))
        assert (Zin == 0).any() and (_bits(Zin) == -2 ** 31).any() and (_bits(Zin) == 0).any()
        fills = (None,)
    gT_ref, slab_ref = _backward_reference(gRin, Sin, pos, w2)
    rep, first = _Report(), None
    for fill in fills:
        zflat, Z = _mask_buffer(L, B, mask_encode(pos.numpy(), absent=fill)) if four_wave else _spectrum(B, NKW, 64, Zin)
        keeps = [t.clone() for t in (gflat, sflat, zflat)]
        tflat, gT = _spectrum(B, NKW, 64)
        wflat, n = _workspace(L, B)
        _mix_bwd(L, four_wave, gR, w2d, S, Z, gT, wflat, B)
        slabs = wflat[:B * UNITS * SLAB].view(B, UNITS, SLAB)
        rep.check(_tail_unchanged(tflat), "bwd", case, "the floats behind gT changed")
        rep.check(_is_sentinel(wflat[B * UNITS * SLAB:]), "bwd", case, "the workspace behind the unit slabs, or its tail, changed")
        rep.check(all(_same_bits(t, k) for t, k in zip((gflat, sflat, zflat), keeps)), "bwd", case, "an input changed")
        if first is None:
            first = (gT, slabs)
            rep.check(bool(torch.isfinite(gT).all() and torch.isfinite(slabs).all()), "bwd", case, "gT or a slab is not finite")
            rep.err(f"bwd_gT_{form}", case, gT.cpu(), gT_ref)
            rep.err(f"bwd_slab_dW2_{form}", case, slabs[..., :4096].cpu(), slab_ref[..., :4096])
            rep.err(f"bwd_slab_db2_{form}", case, slabs[..., 4096:].cpu(), slab_ref[..., 4096:])
            rep.check(bool((slabs[:, UNITS - 1, 4096 + 64:] == 0.0).all()), "bwd", case, "the second db2 row of slab 16 is not exactly zero")
        else:
            rep.check(_same_bits(gT, first[0]) and _same_bits(slabs, first[1]), "bwd", case,
                      f"the unused mask words of unit 16 (bytes {fill:#04x}) reach gT or the slabs")
    rep.finish(record_property)


# ------------------------------------------------------------------------------------ 4., 5. the slab reduce on its own
def _slab_sums(slabs):
    """float64 (dW2 4096, db2 64) of slabs (ns, SLAB): db2 folds the two bias rows."""
    s = slabs.cpu().double().sum(dim=0)
    return s[:4096], s[4096:4096 + 64] + s[4096 + 64:]


def _reduce_case(L, record_property, B, lead):
    """mtd_spec_mix_wgrad_reduce on 17 B random slabs, dw2 `lead` floats into its buffer, both accumulate modes."""
    ns, case = 17 * B, f"B = {B}"
    wflat, n = _workspace(L, B)
    wflat[:ns * SLAB].normal_(generator=torch.Generator(device="cuda").manual_seed(400 + B))
    slab_bits = _bits(wflat[:ns * SLAB]).clone()
    ref_dw, ref_db = _slab_sums(wflat[:ns * SLAB].view(ns, SLAB))
    pre_dw, pre_db = _randn(4096, seed=410 + B, scale=8.0), _randn(64, seed=420 + B, scale=8.0)
    rep = _Report()
    for accumulate in (0, 1):
        mode = f"{case}, accumulate = {accumulate}"
        dflat, dw2 = _guarded(4096, lead)
        bflat, db2 = _guarded(64, 64)
        if accumulate:
            dw2.copy_(pre_dw)
            db2.copy_(pre_db)
        _reduce(L, wflat, B, dw2, db2, accumulate)
        rep.check(bool(torch.isfinite(dw2).all() and torch.isfinite(db2).all()), "reduce", mode, "dw2 or db2 is not finite")
        rep.err("reduce_dW2", mode, dw2.cpu(), ref_dw + pre_dw.double() * accumulate)
        rep.err("reduce_db2", mode, db2.cpu(), ref_db + pre_db.double() * accumulate)
        rep.check(_guards_unchanged(dflat, 4096, lead) and _guards_unchanged(bflat, 64, 64), "reduce", mode, "the floats around dw2 or db2 changed")
        rep.check(torch.equal(_bits(wflat[:ns * SLAB]), slab_bits), "reduce", mode, "the slabs changed")
        rep.check(_is_sentinel(wflat[n:]), "reduce", mode, "the floats behind the workspace changed")
    rep.finish(record_property)


@pytest.mark.parametrize("B", REDUCE_BATCHES)
def test_reduce_fused(hip_lib, record_property, B):
    """mix_reduce_finish_kernel (block_slab_sum<8>) on synthetic slabs: empty runs, two slabs per run, a 4-load batch plus a single
    load, one 8-load batch, an 8- plus a 4-load batch, and the largest batch of the fused path (test_spectral_train_cpu.py)."""
    assert 17 * B <= FUSED_MAX
    _reduce_case(hip_lib, record_property, B, lead=64)


@pytest.mark.parametrize("B", FALLBACK_BATCHES)
def test_reduce_fallback(hip_lib, record_property, B):
    """mix_slab_sum_kernel levels + mix_finish_kernel: through a dw2 that starts 4 bytes off a 16-byte boundary (17 slabs: the finish
    alone; 51: one level with a ragged second group; 1037: two levels), and through more than 4096 slabs with an aligned dw2."""
    lead = 64 if 17 * B > FUSED_MAX else 1
    _reduce_case(hip_lib, record_property, B, lead=lead)


# -------------------------------------------------------------------------------------------- 6. the reduce of a table
def test_reduce_multi(hip_lib, record_property):
    """mtd_spec_mix_wgrad_reduce_multi with three descriptors (17, 68 and 4096 slabs; accumulate 0, 1, 0) against single fused launches
    on the same slabs, bit for bit, and against float64.  4096 is no multiple of 17, so the single launch of the third set is a table
    of one descriptor; the other two go through mtd_spec_mix_wgrad_reduce."""
    from mtd_gan_amd import _lib
    L = hip_lib
    wflat = _nan_floats(FUSED_MAX * SLAB + TAIL)
    wflat[:FUSED_MAX * SLAB].normal_(generator=torch.Generator(device="cuda").manual_seed(600))
    keep = wflat.clone()
    sets = [(4000, 17, 0), (2000, 68, 1), (0, FUSED_MAX, 0)]               # (first slab, slabs, accumulate)
    pre_dw, pre_db = _randn(4096, seed=610, scale=8.0), _randn(64, seed=620, scale=8.0)

    def targets():
        out = []
        for _, _, accumulate in sets:
            dflat, dw2 = _guarded(4096, 64)
            bflat, db2 = _guarded(64, 64)
            if accumulate:
                dw2.copy_(pre_dw)
                db2.copy_(pre_db)
            out.append((dflat, dw2, bflat, db2))
        return out

    def desc(k, tgt):
        s0, ns, accumulate = sets[k]
        d = _lib.MixReduceDesc()
        d.ws, d.dw2, d.db2, d.nslab, d.accumulate = wflat[s0 * SLAB:].data_ptr(), tgt[1].data_ptr(), tgt[3].data_ptr(), ns, accumulate
        return d

    multi, single = targets(), targets()
    _reduce_multi(L, [desc(k, multi[k]) for k in range(3)])
    for k in (0, 1):
        s0, ns, accumulate = sets[k]
        _reduce(L, wflat[s0 * SLAB:], ns // 17, single[k][1], single[k][3], accumulate)
    _reduce_multi(L, [desc(2, single[2])])
    rep = _Report()
    for k, (s0, ns, accumulate) in enumerate(sets):
        case = f"{ns} slabs, accumulate = {accumulate}"
        ref_dw, ref_db = _slab_sums(wflat[s0 * SLAB:(s0 + ns) * SLAB].view(ns, SLAB))
        dflat, dw2, bflat, db2 = multi[k]
        rep.check(bool(torch.isfinite(dw2).all() and torch.isfinite(db2).all()), "multi", case, "dw2 or db2 is not finite")
        rep.err("multi_dW2", case, dw2.cpu(), ref_dw + pre_dw.double() * accumulate)
        rep.err("multi_db2", case, db2.cpu(), ref_db + pre_db.double() * accumulate)
        rep.check(_same_bits(dw2, single[k][1]) and _same_bits(db2, single[k][3]), "multi", case, "not the bits of the single launch")
        for flat, n in ((dflat, 4096), (bflat, 64), (single[k][0], 4096), (single[k][2], 64)):
            rep.check(_guards_unchanged(flat, n, 64), "multi", case, "the floats around dw2 or db2 changed")
    rep.check(_same_bits(wflat, keep), "multi", "all", "the slabs or the floats behind them changed")
    rep.finish(record_property)


# ------------------------------------------------------------------------------------ 7. backward chain with real slabs
CHAIN_SEED = 3009     # see test_backward_chain


@pytest.mark.parametrize("four_wave", FORMS)
def test_backward_chain(hip_lib, mix_weights, record_property, four_wave):
    """kernels.spec_mix_fwd -> kernels.spec_mix_bwd on the forward's own tape, B = 4, once with the reduce launched directly and once
    deferred (DeferredWgrads / flush_wgrads): dw2 and db2 against float64 autograd of the reference block, and the same bits both
    ways.  Nothing is excluded: one ReLU sign taken differently from float64 moves dW2 by about 1 / sqrt(4 33 64) of its RMS, a
    thousand times the bound.  CHAIN_SEED is the seed, of the 4000 from 700 on tried on the CPU, whose float64 Z stays farthest from
    zero: min |Z| = 1.98e-5 rms(Z), the margin of test_forward_mix and twenty times what its Z stage allows a float32 Z to be off
    (seed 700 itself has an element at 4e-8 rms(Z), whose sign no float32 kernel can be held to)."""
    from mtd_gan_amd import kernels as K
    w2, b2, w2d, w2t, b2d = mix_weights
    form, B = _form(four_wave), 4
    case = f"B = {B}"
    Rin = _randn(B, NKW, 64, 64, seed=CHAIN_SEED, scale=0.5)
    cot = _randn(B, NKW, 64, 64, seed=701)
    w64, b64 = w2.double().requires_grad_(True), b2.double().requires_grad_(True)
    _, Z64, T64 = _mix_stages(Rin, w64, b64)
    (T64 * cot.double()).sum().backward()
    nearest = Z64.abs().min().item() / _rms(Z64.detach())
    print(f"\nmin |Z| / rms(Z) of the float64 reference: {nearest:.3e}")
    assert nearest > 1.9 * BOUND, "CHAIN_SEED no longer keeps Z away from zero (did the weights of mix_weights change?)"
    rep = _Report()
    saved = K.SPECMIX4
    K.SPECMIX4 = four_wave
    try:
        R = Rin.cuda()
        T, S, Z = K.spec_mix_fwd(R, w2t, b2d, True)
        assert Z.dtype == (torch.uint8 if four_wave else torch.float32)
        rep.err(f"chain_T_{form}", case, T.cpu(), T64.detach())
        results = []
        for deferred in (False, True):
            dflat, dw2 = _guarded(4096, 64)
            bflat, db2 = _guarded(64, 64)
            defer = K.DeferredWgrads() if deferred else None
            gT = K.spec_mix_bwd(cot.cuda(), w2d, S, Z, dw2.view(64, 64), db2, defer=defer)
            if deferred:
                assert len(defer.mix) == 1, "the reduce was not deferred"
                K.flush_wgrads(defer)
            rep.check(_guards_unchanged(dflat, 4096, 64) and _guards_unchanged(bflat, 64, 64), "chain", case, "the floats around dw2 or db2 changed")
            results.append((gT, dw2, db2))
        rep.check(bool(torch.isfinite(results[0][1]).all() and torch.isfinite(results[0][2]).all()), "chain", case, "dw2 or db2 is not finite")
        rep.err(f"chain_dW2_{form}", case, results[0][1].cpu(), w64.grad.reshape(-1))
        rep.err(f"chain_db2_{form}", case, results[0][2].cpu(), b64.grad)
        rep.check(all(_same_bits(a, b) for a, b in zip(*results)), "chain", case, "the deferred reduce gives other bits than the direct one")
    finally:
        K.SPECMIX4 = saved
    rep.finish(record_property)


# ------------------------------------------------------------------------------------------------------ 8. rows back
@pytest.mark.parametrize("B,ld,off", [(1, 48, 8), (3, 48, 8), (1, 33, 1)])
def test_rows_back(hip_lib, record_property, B, ld, off):
    """mtd_irfft_rows in all eight add1 / add2 / mask variants against irfft along W: the imaginary halves of T's columns 0 and 32
    hold NaN, every operand is a slice of a tensor of its own, the mask holds positive and negative values, +0, -0 and NaN, and every
    entry that is not positive gives exactly 0.  The last item writes an output of odd pixel stride."""
    from mtd_gan_amd import kernels as K
    L = hip_lib
    Tin = _randn(B, NKW, 64, 64, seed=800 + B)
    Tin[:, [0, 32], :, C:] = float("nan")
    ref0 = _back_reference(Tin, 64)
    tflat, T = _spectrum(B, NKW, 64, Tin)
    adds_cpu = [_randn(B, 64, 64, C, seed=810 + 2 * B + i) for i in range(2)]
    gen = torch.Generator().manual_seed(820 + B)
    kind = torch.randint(0, 5, (B, 64, 64, C), generator=gen)             # positive, negative, +0, -0, NaN
    mag = _randn(B, 64, 64, C, seed=830 + B).abs() + 0.05
    mask_cpu = torch.where(kind == 0, mag, torch.where(kind == 1, -mag, torch.zeros(())))
    mask_cpu[kind == 3] = -0.0
    mask_cpu[kind == 4] = float("nan")
    assert all((kind == k).any() for k in range(5)) and (_bits(mask_cpu) == -2 ** 31).any()
    operands = [_sliced(a) for a in adds_cpu] + [_sliced(mask_cpu)]
    keeps = [tflat.clone()] + [b.clone() for b, _ in operands]
    rep = _Report()
    for variant in range(8):
        use = [bool(variant & 1), bool(variant & 2), bool(variant & 4)]
        case = f"B = {B}, out_ld = {ld}, add1 {use[0]}, add2 {use[1]}, mask {use[2]}"
        a1, a2, mk = [v if u else None for (_, v), u in zip(operands, use)]
        ob, ov = _sliced(torch.full((B, 64, 64, C), float("nan")), ld=ld, off=off)
        K.check(L.mtd_irfft_rows(T.data_ptr(), ov.data_ptr(), K.ld_of(ov), _ptr(a1), K.ld_of(a1) if use[0] else 0, _ptr(a2),
                                 K.ld_of(a2) if use[1] else 0, _ptr(mk), K.ld_of(mk) if use[2] else 0, B, K.stream_ptr()), "mtd_irfft_rows")
        ref = ref0
        for a, u in zip(adds_cpu, use[:2]):
            if u:
                ref = ref + a.double()
        got = ov.cpu()
        if use[2]:
            ref = torch.where(mask_cpu > 0, ref, torch.zeros((), dtype=torch.float64))
            rep.check(bool((got[~(mask_cpu > 0)] == 0.0).all()), "back", case, "an entry whose mask is not positive is not exactly 0")
        rep.check(bool(torch.isfinite(got).all()), "back", case, "the output is not finite")
        rep.err("back", case, got, ref)
        rep.check(_outside_unchanged(ob, off), "back", case, "channels outside the output slice, or the spare image, changed")
        rep.check(all(_same_bits(t, k) for t, k in zip([tflat] + [b for b, _ in operands], keeps)), "back", case, "an input changed")
    rep.finish(record_property)
