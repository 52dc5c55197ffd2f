"""FID on the device (csrc/fid.hip, metrics.fid_statistics / fid_distance64 / compute_FID, the test loop's opt-in
model.fid_features) against float64: the product and residual stages alone, the statistics, the distance end to end against the
reference's own numbers (tests/golden/fid_cases.npz), the fallback, the refusals and the test loop.

u = 2^-53 below.  A length-n dot product or sum in float64, in any order, is within n u sum|terms| of the exact value (to first
order), so two of them differ by at most 2 n u sum|terms|: the stage bounds are that, nothing in them is measured."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fid_ref as R
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu
EINVAL = -1
U = 2.0 ** -53
SENTINEL = -7.0


def _randn(shape, seed):
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _guarded(t, pad=4096):
    """t on the device as the front of a longer buffer whose rest is NaN; returns (view, whole buffer)."""
    buf = torch.full((t.numel() + pad,), float("nan"), dtype=t.dtype)
    buf[:t.numel()] = t.reshape(-1)
    dev = buf.cuda()
    return dev[:t.numel()].view(t.shape), dev


def _ws(lib, D):
    n = lib.mtd_fid_ws_bytes(D)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------------------------------------------------ product
def _gemm_case(lib, D, alpha, beta):
    A, B = _randn((D, D), 10 + D), _randn((D, D), 20 + D)
    B[0, D - 1] = 3.0                                    # (asymmetric on purpose: a transposed write does not pass)
    Ad, Abuf = _guarded(A)
    Bd, Bbuf = _guarded(B)
    n = D * D
    big = torch.full((n + 4096,), SENTINEL, dtype=torch.float64, device="cuda")
    assert lib.mtd_fid_gemm(Ad.data_ptr(), Bd.data_ptr(), big.data_ptr(), D, alpha, beta, None) == 0
    torch.cuda.synchronize()
    got = big[:n].cpu().view(D, D)
    prod = A @ B
    ref = alpha * prod + beta * torch.eye(D, dtype=torch.float64)
    # the product's bound, scaled; alpha * acc and + beta round once each: 2^-52 |C| more where an epilogue is at work
    bound = abs(alpha) * 2 * D * U * (A.abs() @ B.abs()) + (0.0 if (alpha, beta) == (1.0, 0.0) else 2.0 ** -52) * ref.abs()
    err = (got - ref).abs()
    print(f"gemm D={D} alpha={alpha} beta={beta}: worst |diff| / bound = {(err / bound).max().item():.3e}")
    assert torch.isfinite(got).all()
    assert (err <= bound).all()
    assert (big[n:] == SENTINEL).all()
    assert torch.isnan(Abuf[n:]).all() and torch.isnan(Bbuf[n:]).all()
    assert torch.equal(Ad.cpu(), A) and torch.equal(Bd.cpu(), B)


@pytest.mark.parametrize("D", [1, 5, 16, 64, 96, 130, 200, 520])
def test_gemm(hip_lib, D):
    _gemm_case(hip_lib, D, 1.0, 0.0)


@pytest.mark.parametrize("alpha,beta", [(-0.5, 1.5), (0.3, -2.25), (1.0, 1.0)])
def test_gemm_epilogues(hip_lib, alpha, beta):
    _gemm_case(hip_lib, 130, alpha, beta)


def test_gemm_identity_places_every_element(hip_lib):
    """I . B and B . I with an asymmetric integer B: exact, and any wrong lane-to-element map shows."""
    D = 37
    B = (torch.arange(D * D, dtype=torch.float64).view(D, D) * 3.0 + 1.0).cuda()
    eye = torch.eye(D, dtype=torch.float64, device="cuda")
    out = torch.empty_like(B)
    for lhs, rhs in ((eye, B), (B, eye)):
        assert hip_lib.mtd_fid_gemm(lhs.data_ptr(), rhs.data_ptr(), out.data_ptr(), D, 1.0, 0.0, None) == 0
        assert torch.equal(out, B)


# ----------------------------------------------------------------------------------------------------------- residual
@pytest.mark.parametrize("D", [5, 130, 520])
def test_residual(hip_lib, D):
    Y = _randn((D, D), 30 + D) / D ** 0.5
    s = 1.7
    P = Y @ Y
    A = s * P + 1e-3 * _randn((D, D), 40 + D)          # close to s Y Y, as at the end of the iteration: the difference cancels
    Ad, _ = _guarded(A)
    Yd, _ = _guarded(Y)
    ws = _ws(hip_lib, D)
    outs = []
    for _ in range(2):
        out = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
        assert hip_lib.mtd_fid_residual(Ad.data_ptr(), Yd.data_ptr(), s, D, out.data_ptr(), ws.data_ptr(), None) == 0
        outs.append(out.cpu())
    d = A - s * P
    ref = (d * d).sum().item()
    # per element: the product (2 D u |s| |Y||Y|) and the two roundings of s * p and a - s p on both sides; then d^2 and the sum
    # of D^2 terms
    delta = 2 * D * U * abs(s) * (Y.abs() @ Y.abs()) + 4 * U * (A.abs() + abs(s) * P.abs())
    bound = (2 * d.abs() * delta).sum().item() + 2 * (D * D + 2) * U * ref
    got = outs[0][0].item()
    print(f"residual D={D}: hip {got:.15e} ref {ref:.15e} |diff| {abs(got - ref):.3e} bound {bound:.3e}")
    assert abs(got - ref) <= bound
    assert torch.equal(outs[0], outs[1])                 # bit-identical, and nothing behind out[0]
    assert (outs[0][1:] == SENTINEL).all()


# --------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("N,D", [(2, 5), (7, 200), (24, 64), (33, 96), (200, 96), (16, 130)])
def test_statistics(hip_lib, N, D):
    from mtd_gan_amd import metrics as M
    x = R.features(N, D, 0, seed=50 + N + D)
    buf = torch.full((N + 1, D), float("nan"))
    buf[:N] = x
    dev = buf.cuda()                                     # a guard row of NaN behind X
    mu, sigma = M.fid_statistics(dev[:N])
    assert mu.dtype == torch.float64 and sigma.dtype == torch.float64 and tuple(mu.shape) == (D,) and tuple(sigma.shape) == (D, D)
    xl = x.numpy().astype(np.longdouble)
    mu_ref = (xl.sum(axis=0) / N).astype(np.float64)     # 24-bit values in a 64-bit significand: exact up to the last rounding
    mean_abs = x.double().abs().mean(dim=0).numpy()
    mu_err = np.abs(mu.cpu().numpy() - mu_ref)
    print(f"stats N={N} D={D}: mu worst |diff| / bound = {(mu_err / (N * U * mean_abs + 1e-300)).max():.3e}")
    assert (mu_err <= N * U * mean_abs).all()
    mu64, sig_ref = R.statistics(x)
    xc = (x.double() - mu64).abs()
    bound = (N + 8) * 2.0 ** -52 * (xc.t() @ xc) / (N - 1)
    got = sigma.cpu()
    err = (got - sig_ref).abs()
    print(f"stats N={N} D={D}: sigma worst |diff| / bound = {(err / (bound + 1e-300)).max().item():.3e}; "
          f"asymmetry {(got - got.t()).abs().max().item():.3e}")
    assert torch.isfinite(got).all()
    assert (err <= bound).all()
    assert ((got - got.t()).abs() <= bound).all()        # both triangles are computed
    assert torch.isnan(dev[N]).all()
    # the entry point itself into the front of larger buffers: nothing behind mu and sigma changes
    big_mu = torch.full((D + 64,), SENTINEL, dtype=torch.float64, device="cuda")
    big_sigma = torch.full((D * D + 4096,), SENTINEL, dtype=torch.float64, device="cuda")
    assert hip_lib.mtd_fid_stats(dev.data_ptr(), N, D, big_mu.data_ptr(), big_sigma.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(big_mu[:D], mu) and torch.equal(big_sigma[:D * D].view(D, D), sigma)
    assert (big_mu[D:] == SENTINEL).all() and (big_sigma[D * D:] == SENTINEL).all()


def test_statistics_of_a_strided_view(hip_lib):
    from mtd_gan_amd import metrics as M
    x = R.features(9, 24, 0, seed=3).cuda()
    mu, sigma = M.fid_statistics(x[:, ::2])
    mu2, sigma2 = M.fid_statistics(x[:, ::2].contiguous())
    assert torch.equal(mu, mu2) and torch.equal(sigma, sigma2)
    with pytest.raises(ValueError):
        M.fid_statistics(x[:1])
    with pytest.raises(TypeError):
        M.fid_statistics(x.double())


# --------------------------------------------------------------------------------------------------------- end to end
def _solve(lib, s1, s2, offset=0.0, max_iters=R.MAX_ITERS):
    """mtd_fid_distance on two (mu, sigma) device pairs: ([fid, tr, err, finite], iters)."""
    D = s1[0].numel()
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    iters = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ws = _ws(lib, D)
    assert lib.mtd_fid_distance(s1[0].data_ptr(), s1[1].data_ptr(), s2[0].data_ptr(), s2[1].data_ptr(), D, offset, max_iters,
                                out.data_ptr(), iters.data_ptr(), ws.data_ptr(), None) == 0
    return out.tolist(), iters.item()


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_distance_against_the_reference(hip_lib, index):
    from mtd_gan_amd import metrics as M
    _, rows = R.golden()
    a, b = R.case_features(R.CASES[index], index)
    assert R.crc(a, b) == rows[2 * index]["crc"], "the seeded features differ from those the fixture was computed on"
    a, b = a.cuda(), b.cuda()
    sb = M.fid_statistics(b)
    for row in rows[2 * index:2 * index + 2]:
        sa = sb if row["same"] else M.fid_statistics(a)
        got = M.fid_distance64(sa, sb)
        assert got.is_cuda and got.dim() == 0 and got.dtype == torch.float64
        out, iters = _solve(hip_lib, sa, sb)
        print(f"{row['case']} same={row['same']}: hip {got.item():.15e} reference {row['fid64']:.15e} |diff| {abs(got.item() - row['fid64']):.2e} "
              f"tol {row['tol']:.2e}; rounds {iters} / {row['rounds']}; err {out[2]:.3e}")
        assert abs(got.item() - row["fid64"]) <= row["tol"]
        assert abs(out[1] - row["tr"]) <= row["tol"]
        assert iters == row["rounds"]
        assert out[3] == 1.0 and out[2] <= R.ATOL
        assert out[0] == got.item()                       # bit-identical on a second call
        assert torch.equal(M.fid_distance64(sa, sb), got)
    triple = M.compute_FID(a, b, a)
    assert len(triple) == 3 and all(t.is_cuda and t.dim() == 0 and t.dtype == torch.float32 for t in triple)
    for t, row in zip(triple, (rows[2 * index], rows[2 * index + 1], rows[2 * index])):
        assert abs(float(t.item()) - float(row["fid32"])) <= float(np.spacing(np.abs(row["fid32"]))), (t.item(), row["fid32"])
    again = M.compute_FID(a, b, a)
    assert all(torch.equal(p, q) for p, q in zip(triple, again))


def test_stop_is_taken_on_the_device(hip_lib):
    """Fewer rounds than the iteration needs: it ends at max_iters with the err of that round, above the threshold."""
    _, rows = R.golden()
    a, b = (t.cuda() for t in R.case_features(R.CASES[0], 0))
    from mtd_gan_amd import metrics as M
    sa, sb = M.fid_statistics(a), M.fid_statistics(b)
    ref = R.distance(R.statistics(a.cpu()), R.statistics(b.cpu()))
    assert ref["rounds"] == rows[0]["rounds"] > 3
    out, iters = _solve(hip_lib, sa, sb, max_iters=3)
    assert iters == 3 and out[2] > R.ATOL
    assert abs(out[2] - ref["errs"][2]) <= 1e-6 * ref["errs"][2]


# ------------------------------------------------------------------------------------------------------------ fallback
def test_offset_solve(hip_lib):
    _, rows = R.golden()
    a, b = R.case_features(R.CASES[0], 0)
    sa, sb = R.statistics(a), R.statistics(b)
    ref = R.distance(sa, sb, offset=R.EPS)
    out, iters = _solve(hip_lib, tuple(t.cuda() for t in sa), tuple(t.cuda() for t in sb), offset=R.EPS)
    print(f"offset solve: hip {out[0]:.15e} restatement {ref['fid']:.15e} |diff| {abs(out[0] - ref['fid']):.2e} tol {rows[0]['tol']:.2e}")
    assert abs(out[0] - ref["fid"]) <= rows[0]["tol"]
    assert iters == ref["rounds"] and out[3] == 1.0
    plain, _ = _solve(hip_lib, tuple(t.cuda() for t in sa), tuple(t.cuda() for t in sb))
    assert plain[0] != out[0]


def test_non_finite_covariance_takes_the_second_solve(hip_lib, capsys):
    from mtd_gan_amd import metrics as M
    a, b = R.case_features(R.CASES[0], 0)
    sa, sb = R.statistics(a), R.statistics(b)
    sa[1][3, 5] = float("inf")
    ref = R.distance(sa, sb)
    assert ref["fallback"] and not np.isfinite(ref["fid"])
    da, db = tuple(t.cuda() for t in sa), tuple(t.cuda() for t in sb)
    out, iters = _solve(hip_lib, da, db)
    assert out[3] == 0.0 and iters == R.MAX_ITERS
    capsys.readouterr()
    got = M.fid_distance64(da, db)
    assert "adding 1e-06 to diagonal" in capsys.readouterr().out
    assert not np.isfinite(got.item())


# ------------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments(hip_lib):
    L = hip_lib
    x = torch.zeros(4, 8, device="cuda")
    mu = torch.zeros(8, dtype=torch.float64, device="cuda")
    s = torch.eye(8, dtype=torch.float64, device="cuda")
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    it = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = _ws(L, 8)
    p = lambda t: t.data_ptr()      # noqa: E731
    assert L.mtd_fid_ws_bytes(0) == 0 and L.mtd_fid_ws_bytes(-3) == 0
    assert L.mtd_fid_stats(p(x), 4, 0, p(mu), p(s), None, None) == EINVAL
    assert L.mtd_fid_stats(p(x), 1, 8, p(mu), p(s), None, None) == EINVAL
    assert L.mtd_fid_stats(None, 4, 8, p(mu), p(s), None, None) == EINVAL
    assert L.mtd_fid_stats(p(x), 4, 8, None, p(s), None, None) == EINVAL
    assert L.mtd_fid_stats(p(x), 4, 8, p(mu), None, None, None) == EINVAL
    assert L.mtd_fid_gemm(p(s), p(s), p(s), 0, 1.0, 0.0, None) == EINVAL
    assert L.mtd_fid_gemm(None, p(s), p(s), 8, 1.0, 0.0, None) == EINVAL
    assert L.mtd_fid_gemm(p(s), p(s), None, 8, 1.0, 0.0, None) == EINVAL
    assert L.mtd_fid_residual(p(s), p(s), 1.0, 0, p(out), p(ws), None) == EINVAL
    assert L.mtd_fid_residual(p(s), None, 1.0, 8, p(out), p(ws), None) == EINVAL
    assert L.mtd_fid_residual(p(s), p(s), 1.0, 8, p(out), None, None) == EINVAL
    good = [p(mu), p(s), p(mu), p(s), 8, 0.0, 100, p(out), p(it), p(ws), None]
    for i, v in ((4, 0), (6, 0), (6, -1), (0, None), (1, None), (2, None), (3, None), (7, None), (8, None), (9, None)):
        bad = list(good)
        bad[i] = v
        assert L.mtd_fid_distance(*bad) == EINVAL, i
    assert L.mtd_fid_distance(*good) == 0
    torch.cuda.synchronize()
    assert out.tolist()[3] == 1.0


# ------------------------------------------------------------------------------------------------------------- engine
def test_test_loop_with_and_without_the_extractor(hip_lib, tmp_path):
    from mtd_gan_amd import engine, kernels as K, metrics as M
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    torch.manual_seed(3)
    m = MTD_GAN_Method().cuda()
    m.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    xs, ys = orc.synthetic_ldct(3, seed=9, size=64)
    loader = [dict(n_20=xs[i:i + 1], n_100=ys[i:i + 1], path_n_20=[f"L000_000{i}.dcm"], path_n_100=[f"L000_000{i}.dcm"]) for i in range(3)]
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(17)
    w, bias = torch.randn(40, 3, 1, 1, generator=g).cuda(), torch.randn(40, generator=g).cuda()
    calls = []

    def extractor(t):                                    # a fixed random 1x1 conv (+ ReLU) and a mean pool to D = 40
        calls.append(tuple(t.shape))
        return [F.relu(F.conv2d(t, w, bias)).mean(dim=(2, 3), keepdim=True)]

    plain = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, str(tmp_path / "plain"))
    pixel_keys = ["L1_loss"] + [f"{who}_{name}" for name in ("rmse", "psnr", "ssim") for who in ("input", "gt", "pred")]
    assert list(plain.keys()) == pixel_keys
    m.fid_features = None
    assert list(engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, None).keys()) == pixel_keys

    m.fid_features = extractor
    full = engine.test_MTD_GAN_Ours(m, torch.nn.L1Loss(), loader, dev, str(tmp_path / "fid"))
    assert list(full.keys()) == pixel_keys + ["input_fid", "gt_fid", "pred_fid"]
    assert all(full[k] == plain[k] for k in pixel_keys)
    assert open(tmp_path / "fid" / "pred_results.csv").read() == open(tmp_path / "plain" / "pred_results.csv").read()
    assert calls == [(1, 3, 64, 64)] * 9
    with torch.no_grad():
        pred = torch.cat([K.clip01(m.Generator(xs[i:i + 1].cuda()).contiguous()) for i in range(3)])
    per_slice = [M.compute_feat(xs[i:i + 1].cuda(), ys[i:i + 1].cuda(), pred[i:i + 1], extractor=extractor) for i in range(3)]       # as the loop does
    feats = [torch.cat([s[k] for s in per_slice]) for k in range(3)]
    assert all(tuple(f.shape) == (3, 40) for f in feats)
    triple = M.compute_FID(*feats)
    perm = torch.randperm(40, generator=torch.Generator().manual_seed(1))
    st = R.statistics(feats[1].cpu())
    st_p = R.statistics(feats[1].cpu()[:, perm])
    for who, f, v in zip(("input", "gt", "pred"), feats, triple):
        assert full[f"{who}_fid"] == round(v.item(), 7), who
        sf = st if who == "gt" else R.statistics(f.cpu())
        ref = R.distance(sf, st)
        ref_p = R.distance(st_p if who == "gt" else R.statistics(f.cpu()[:, perm]), st_p)
        tol = max(100 * abs(ref["fid"] - ref_p["fid"]), 1e-12 * R.base(sf, st))
        got = M.fid_distance64(M.fid_statistics(f), M.fid_statistics(feats[1])).item()
        print(f"test loop {who}_fid: hip {got:.15e} restatement {ref['fid']:.15e} |diff| {abs(got - ref['fid']):.2e} tol {tol:.2e}")
        assert abs(got - ref["fid"]) <= tol
        assert abs(v.item() - float(np.float32(ref["fid"]))) <= float(np.spacing(np.abs(np.float32(ref["fid"]))))
    assert full["pred_fid"] > 0.0
