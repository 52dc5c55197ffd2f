"""CPU side of the general-length spectral path (csrc/resfft_gen.hip): the library's plans and argument checks, and a numpy model
of the kernels' decomposition -- mixed-radix DIF / DIT passes, Bluestein, the row-pair packing and the complex-to-real rules --
against numpy.fft / torch.fft for every length the path takes.  The model reads the plan from the library, so it stays in step
with what the kernels run."""
import ctypes

import numpy as np
import pytest
import torch

MTD_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__  # noqa: F401  (puts the repository root on sys.path)
    from mtd_gan_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.mtd_spectral_gen_ws_bytes.restype = ctypes.c_size_t
    L.mtd_spectral_gen_ws_bytes.argtypes = [ctypes.c_int] * 3
    L.mtd_spectral_gen_plan.argtypes = [ctypes.c_int, ctypes.c_void_p]
    return L


def plan(lib, n):
    out = (ctypes.c_int * 16)()
    k = lib.mtd_spectral_gen_plan(n, out)
    assert k > 0, n
    return out[0], list(out[1:1 + k])


# ---------------------------------------------------------------------------------------------------- model of the passes
def _dft_small(x, r, sign):
    """x: (..., r) -> y_q = sum_t x_t exp(sign 2 pi i t q / r)."""
    t = np.arange(r)
    return x @ np.exp(sign * 2j * np.pi * np.outer(t, t) / r)


def dif(x, rad, sign):
    """In-place decimation in frequency, natural in, digit-reversed out (fft_dif of the kernel): pass s has blocks of L, m = L / r,
    points blk L + j + t m; the r-point DFT, then the twiddles w_L^(j q)."""
    x = x.astype(np.complex128).copy()
    n, L = x.shape[-1], x.shape[-1]
    for r in rad:
        m = L // r
        v = x.reshape(x.shape[:-1] + (n // L, r, m))                   # [blk][t][j]
        y = _dft_small(np.swapaxes(v, -1, -2), r, sign)                # [blk][j][q]
        j, q = np.arange(m)[:, None], np.arange(r)[None, :]
        y = y * np.exp(sign * 2j * np.pi * ((j * q * (n // L)) % n) / n)  # (the kernel's table index j q len / L < len)
        x = np.swapaxes(y, -1, -2).reshape(x.shape)
        L = m
    return x


def dit(x, rad, sign):
    """The transposed passes in reverse order (fft_dit): digit-reversed in, natural out; twiddles first, then the DFT."""
    x = x.astype(np.complex128).copy()
    n, L = x.shape[-1], 1
    for r in reversed(rad):
        L *= r
        m = L // r
        v = np.swapaxes(x.reshape(x.shape[:-1] + (n // L, r, m)), -1, -2)   # [blk][j][q]
        j, q = np.arange(m)[:, None], np.arange(r)[None, :]
        v = v * np.exp(sign * 2j * np.pi * ((j * q * (n // L)) % n) / n)
        x = np.swapaxes(_dft_small(v, r, sign), -1, -2).reshape(x.shape)
    return x


def digit_rev(k, rad, n):
    pos, L = 0, n
    for r in rad:
        m = L // r
        pos += (k % r) * m
        k //= r
        L = m
    return pos


def chirp(n):
    idx = np.arange(n, dtype=np.int64)
    return np.exp(-1j * np.pi * ((idx * idx) % (2 * n)) / n)          # n^2 mod 2N in integers


def line_transform(x, n, m, rad, inverse):
    """What Line<INV> computes over the last axis: the unnormalised DFT (inverse: exp(+...))."""
    if m == 0:
        d = np.array([digit_rev(k, rad, n) for k in range(n)])
        if inverse:
            z = np.zeros_like(x, dtype=np.complex128)
            z[..., d] = x
            return dit(z, rad, +1)
        return dif(x, rad, -1)[..., d]
    w = chirp(n)
    src = np.conj(x) if inverse else x
    a = np.zeros(x.shape[:-1] + (m,), dtype=np.complex128)
    a[..., :n] = src * w
    b = np.zeros(m, dtype=np.complex128)
    b[:n] = np.conj(w)
    b[m - n + 1:] = np.conj(w[1:][::-1])
    filt = dif(b, rad, -1) / m                                          # bluestein_filter_kernel: DIF order, 1/M folded in
    conv = dit(dif(a, rad, -1) * filt, rad, +1)[..., :n]
    y = w * conv
    return np.conj(y) if inverse else y


def test_workspace_query_and_plans_cover_every_length(lib):
    for n in range(16, 513):
        m, rad = plan(lib, n)
        assert lib.mtd_spectral_gen_ws_bytes(1, n, n) > 0
        assert lib.mtd_spectral_gen_ws_bytes(3, n, 528 - n) > 0
        if m == 0:
            assert int(np.prod(rad)) == n and set(rad) <= {2, 3, 4, 5, 7}
        else:
            assert m & (m - 1) == 0 and 2 * n - 1 <= m <= 1024 and int(np.prod(rad)) == m and set(rad) <= {2, 4}
            assert any(n % p == 0 for p in range(11, n + 1) if all(p % d for d in range(2, p)))
    for n in (15, 513, 0, -4, 1024):
        assert lib.mtd_spectral_gen_plan(n, (ctypes.c_int * 16)()) == MTD_EINVAL
    assert lib.mtd_spectral_gen_ws_bytes(1, 15, 64) == 0 and lib.mtd_spectral_gen_ws_bytes(1, 64, 513) == 0
    assert lib.mtd_spectral_gen_ws_bytes(0, 64, 64) == 0


def test_entry_points_refuse_without_a_device(lib):
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    fake = vp(4096)
    ws_n = lib.mtd_spectral_gen_ws_bytes(2, 100, 77)
    rf = lib.mtd_rfft_rows_gen
    rf.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, sz, vp]
    mx = lib.mtd_spec_mix_gen
    mx.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, sz, vp]
    ir = lib.mtd_irfft_rows_gen
    ir.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, sz, vp]
    for (B, H, W) in [(2, 15, 77), (2, 100, 513), (0, 100, 77), (2, 8, 8)]:
        assert rf(fake, 32, fake, B, H, W, fake, 1 << 20, None) == MTD_EINVAL
        assert mx(fake, fake, fake, fake, B, H, W, fake, 1 << 20, None) == MTD_EINVAL
        assert ir(fake, fake, 32, None, 0, None, 0, B, H, W, fake, 1 << 20, None) == MTD_EINVAL
    assert rf(None, 32, fake, 2, 100, 77, fake, ws_n, None) == MTD_EINVAL
    assert rf(fake, 32, fake, 2, 100, 77, None, ws_n, None) == MTD_EINVAL
    assert rf(fake, 16, fake, 2, 100, 77, fake, ws_n, None) == MTD_EINVAL
    assert rf(fake, 32, fake, 2, 100, 77, fake, ws_n - 1, None) == MTD_EINVAL
    assert mx(fake, None, fake, fake, 2, 100, 77, fake, ws_n, None) == MTD_EINVAL
    assert mx(fake, fake, fake, None, 2, 100, 77, fake, ws_n, None) == MTD_EINVAL
    assert ir(None, fake, 32, None, 0, None, 0, 2, 100, 77, fake, ws_n, None) == MTD_EINVAL
    assert ir(fake, fake, 32, fake, 8, None, 0, 2, 100, 77, fake, ws_n, None) == MTD_EINVAL


def test_pass_model_matches_numpy_fft_for_every_length(lib):
    rng = np.random.default_rng(3)
    worst = 0.0
    for n in range(16, 513):
        m, rad = plan(lib, n)
        x = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
        f = line_transform(x, n, m, rad, False)
        g = line_transform(x, n, m, rad, True)
        ref_f, ref_g = np.fft.fft(x), np.fft.ifft(x) * n
        worst = max(worst, np.abs(f - ref_f).max() / np.abs(ref_f).max(), np.abs(g - ref_g).max() / np.abs(ref_g).max())
    assert worst < 1e-10, worst


def _spectral_model(lib, x, w2, b2):
    """The three stages of the kernels on x (B, C=32, H, W): rows forward in pairs, columns + mix, rows back in pairs."""
    B, C, H, W = x.shape
    mw, rw = plan(lib, W)
    mh, rh = plan(lib, H)
    nkw = W // 2 + 1
    R = np.zeros((B, C, H, nkw), dtype=np.complex128)
    for h in range(0, H, 2):
        zi = x[:, :, h + 1] if h + 1 < H else 0.0
        Z = line_transform(x[:, :, h] + 1j * zi, W, mw, rw, False)
        Zm = Z[..., (-np.arange(nkw)) % W]
        R[:, :, h] = 0.5 * (Z[..., :nkw] + np.conj(Zm)) / np.sqrt(W)
        if h + 1 < H:
            R[:, :, h + 1] = (0.5 * (Z[..., :nkw] - np.conj(Zm)) / 1j) / np.sqrt(W)
    X = np.moveaxis(line_transform(np.moveaxis(R, 2, -1), H, mh, rh, False), -1, 2) / np.sqrt(H)
    cat = np.concatenate([X.real, X.imag], axis=1)                       # (B, 64, H, nkw)
    y = np.maximum(np.einsum("oc,bchw->bohw", w2, cat) + b2[None, :, None, None], 0.0)
    Y = y[:, :C] + 1j * y[:, C:]
    T = np.moveaxis(line_transform(np.moveaxis(Y, 2, -1), H, mh, rh, True), -1, 2) / np.sqrt(H)
    edge = [0] + ([W // 2] if W % 2 == 0 else [])
    T[..., edge] = T[..., edge].real                                     # (after the inverse column transform)
    out = np.zeros((B, C, H, W))
    for h in range(0, H, 2):
        A = T[:, :, h]
        Bv = T[:, :, h + 1] if h + 1 < H else np.zeros_like(A)
        Z = np.zeros((B, C, W), dtype=np.complex128)
        Z[..., :nkw] = A + 1j * Bv
        k = np.array([kk for kk in range(1, nkw) if 2 * kk != W])
        Z[..., W - k] = np.conj(A[..., k]) + 1j * np.conj(Bv[..., k])
        zz = line_transform(Z, W, mw, rw, True) / np.sqrt(W)
        out[:, :, h] = zz.real
        if h + 1 < H:
            out[:, :, h + 1] = zz.imag
    return out


@pytest.mark.parametrize("H,W", [(16, 17), (17, 16), (45, 64), (100, 77), (23, 19), (96, 30)])
def test_spectral_model_matches_torch_irfft2(lib, H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randn(2, 32, H, W, generator=g, dtype=torch.float64)
    w2 = torch.randn(64, 64, generator=g, dtype=torch.float64) * 0.2
    b2 = torch.randn(64, generator=g, dtype=torch.float64) * 0.1
    f = torch.fft.rfft2(x, s=(H, W), dim=(2, 3), norm="ortho")
    z = torch.relu(torch.einsum("oc,bchw->bohw", w2, torch.cat([f.real, f.imag], 1)) + b2[None, :, None, None])
    ref = torch.fft.irfft2(torch.complex(z[:, :32], z[:, 32:]), s=(H, W), dim=(2, 3), norm="ortho").numpy()
    got = _spectral_model(lib, x.numpy(), w2.numpy(), b2.numpy())
    assert np.abs(got - ref).max() < 1e-9 * np.abs(ref).max()


def test_stage_test_lengths_cover_every_plan(lib):
    """The lengths the per-stage GPU test runs (tests/_gen_lengths.py) leave no class of plan out: every radix, every Bluestein
    convolution length in both parities of n, and every distinct plan (M, radices) the library makes for 16..512."""
    import _gen_lengths as gl
    plans = gl.library_plans(lib)
    assert plans == {n: (plan(lib, n)[0], tuple(plan(lib, n)[1])) for n in range(16, 513)}
    smooth, blue = gl.select(plans)
    chosen = smooth + [n for ns in blue.values() for n in ns]
    assert len(chosen) == len(set(chosen)) and all(16 <= n <= 512 for n in chosen)
    assert all(plans[n][0] == 0 for n in smooth) and all(plans[n][0] == m for m, ns in blue.items() for n in ns)
    assert {r for n in smooth for r in plans[n][1]} == {2, 3, 4, 5, 7}
    assert set(blue) == {64, 128, 256, 512, 1024}
    for m, ns in blue.items():
        assert {n % 2 for n in ns} == {0, 1}, (m, ns)
        of_m = [n for n in plans if plans[n][0] == m]
        assert min(of_m) in ns and max(of_m) in ns, (m, ns)
    assert all(n in chosen for n in gl.MODEL_SIDES)
    assert {plans[n] for n in chosen} == set(plans.values())
