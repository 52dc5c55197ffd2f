"""KID on the device (csrc/kid.hip, metrics.kid_distance64 / compute_KID, the test loop's opt-in model.test_kid) against the
reference's own numbers (tests/golden/kid_cases.npz: score within tol, variance within vtol, both measured at pin time) and,
named sum by named sum, against the float64 restatement of tests/_kid_ref.py.

The bound of a named sum is worked out, not measured.  u = 2^-53.  Every feature is >= 0, gamma > 0 and coef0 >= 0, so every
kernel value and every term of every sum is >= 0 and errors are relative to the sum of the terms.  Two float64 evaluations, in
whatever order, of: the dot product of D terms differ by at most 2 D u of it; t = gamma dot + coef0 by (2 D + 4) u; t^degree
by degree (2 D + 6) u; a sum of n such values by 2 n u more, n <= m^2 + m; a product of two such sums, or the square of one,
by twice that.  Hence E = (2 degree (2 D + 6) + 4 (m^2 + m) + 16) u, relative to `mag`: the sum of the magnitudes that went
into the part, the diagonal that a Kt_* sum leaves out included (the reference subtracts it from a sum that holds it).
mmd2, the zetas and var_est are sums of products of at most two parts with exact factors: 4 E of the sum of the magnitudes of
their terms."""
import pytest
import torch
import torch.nn.functional as F

import _kid_ref as R
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu
EINVAL = -1
U = 2.0 ** -53
SENTINEL = -7.0
ENTRIES = R.entries()
_CACHE = {}


def _features(index):
    if index not in _CACHE:
        _CACHE[index] = R.case_features(R.CASES[index], index)
    return _CACHE[index]


def _kwargs(case):
    kw = dict(case["opts"])
    if case["subsets"] is not None:
        kw.update(average=True, n_subsets=case["subsets"][0], subset_size=case["subsets"][1])
    return kw


def _check_parts(table, ref, case, D, m, has_var, label):
    """Every named sum of every subset against the restatement."""
    E = (2 * R.options(case, D)["degree"] * (2 * D + 6) + 4 * (m * m + m) + 16) * U
    worst = 0.0
    for s, q in enumerate(ref["parts"]):
        for j, name in enumerate(R.PARTS):
            if not has_var and name in ("zeta1_est", "zeta2_est", "var_est"):
                assert table[s][j] == 0.0
                continue
            bound = (1 if name in R.SUM_PARTS else 4) * E * q["mag"][name]
            diff = abs(table[s][j] - q[name])
            worst = max(worst, diff / bound if bound > 0 else (0.0 if diff == 0 else float("inf")))
            assert diff <= bound, (label, s, name, table[s][j], q[name], diff, bound)
    print(f"{label}: named sums, worst |diff| / bound = {worst:.3e} (E = {E:.2e})")


@pytest.mark.parametrize("entry", range(len(ENTRIES)))
def test_against_the_reference(hip_lib, entry):
    from mtd_gan_amd import metrics as M
    _, rows = R.golden()
    row = rows[entry]
    index, same = ENTRIES[entry]
    case = R.CASES[index]
    a, b = _features(index)
    assert R.crc(a, b) == row["crc"], "the seeded features differ from those the fixture was computed on"
    p = b if same else a
    ref = R.kid(p, b, case, ret_var=row["has_var"])
    S, m = ref["subsets"][0].shape
    pd, bd = p.cuda(), b.cuda()
    td = pd if same else bd                                # KID(t, t): one buffer for both sets
    runs = []
    for _ in range(2):
        if case["seed"] is not None:
            torch.manual_seed(case["seed"])
        runs.append(M.kid_distance64(pd, td, ret_var=row["has_var"], parts=True, **_kwargs(case)))
    got = runs[0]
    score, var, table = (got[0], got[1], got[2]) if row["has_var"] else (got[0], torch.zeros((), dtype=torch.float64), got[1])
    assert score.is_cuda and score.dim() == 0 and score.dtype == torch.float64 and tuple(table.shape) == (S, len(R.PARTS))
    label = f"#{index} N=({p.shape[0]}, {b.shape[0]}) D={case['D']} {case['opts'] or ''} {case['subsets'] or ''} same={same}"
    print(f"{label}: hip {score.item():.15e} reference {row['mmd2_64']:.15e} |diff| {abs(score.item() - row['mmd2_64']):.2e} tol {row['tol']:.2e}; "
          f"var {var.item():.6e} / {row['var_64']:.6e} |diff| {abs(var.item() - row['var_64']):.2e} vtol {row['vtol']:.2e}")
    assert abs(score.item() - row["mmd2_64"]) <= row["tol"]
    assert abs(var.item() - row["var_64"]) <= row["vtol"]
    assert abs(score.item() - ref["mmd2"]) <= row["tol"] and abs(var.item() - ref["var"]) <= row["vtol"]
    _check_parts(table.tolist(), ref, case, case["D"], m, row["has_var"], label)
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1]))          # two calls, the same bits
    if same and case["subsets"] is None:
        assert torch.equal(table[:, 0], table[:, 1])        # Kt_XX_sum and Kt_YY_sum: the same operands through the same instructions
        assert torch.equal(table[:, 3], table[:, 4]) and torch.equal(table[:, 8], table[:, 9]) and torch.equal(table[:, 11], table[:, 12])
    if not row["has_var"]:
        only = M.kid_distance64(pd, td, **_kwargs(case))
        assert torch.is_tensor(only) and torch.equal(only, score)
    elif not case["opts"] and case["seed"] is None:         # (whole sets, no draw matters) the score does not depend on ret_var; the float32 triple's form
        assert torch.equal(M.kid_distance64(pd, td), score)
        triple = M.compute_KID(pd, bd, pd)
        assert len(triple) == 3 and all(t.is_cuda and t.dim() == 0 and t.dtype == torch.float32 for t in triple)
        assert torch.equal(triple[0], score.float()) and torch.equal(triple[2], score.float())


def test_explicit_subsets_and_the_seeded_draw_give_the_same_bits(hip_lib):
    from mtd_gan_amd import metrics as M
    index = len(R.WHOLE) + len(R.OPTIONS)
    case = R.CASES[index]
    a, b = (t.cuda() for t in _features(index))
    S, m = case["subsets"]
    torch.manual_seed(case["seed"])
    seeded = M.kid_distance64(a, b, average=True, n_subsets=S, subset_size=m, ret_var=True, parts=True)
    torch.manual_seed(case["seed"])
    pi, ti = R.draw(a.shape[0], b.shape[0], m, S)
    torch.manual_seed(999)
    explicit = M.kid_distance64(a, b, subsets=(pi, ti.to(torch.int32)), ret_var=True, parts=True)
    assert all(torch.equal(x, y) for x, y in zip(seeded, explicit))
    torch.manual_seed(case["seed"] + 1)
    assert not torch.equal(M.kid_distance64(a, b, average=True, n_subsets=S, subset_size=m), seeded[0])
    # average=False with the longer target: the predicted set whole and sorted, the target's subset as drawn
    torch.manual_seed(4)
    whole = M.kid_distance64(a, b, ret_var=True)
    torch.manual_seed(4)
    torch.randperm(a.shape[0])
    ti = torch.randperm(b.shape[0])[:a.shape[0]]
    assert all(torch.equal(x, y) for x, y in zip(whole, M.kid_distance64(a, b, subsets=(torch.arange(a.shape[0])[None], ti[None]), ret_var=True)))


def test_a_subset_does_not_depend_on_its_place_or_on_S(hip_lib):
    from mtd_gan_amd import metrics as M
    index = len(R.WHOLE) + len(R.OPTIONS) + 1               # S = 3, m = 64
    a, b = (t.cuda() for t in _features(index))
    torch.manual_seed(21)
    pi, ti = R.draw(a.shape[0], b.shape[0], 64, 3)
    _, _, all3 = M.kid_distance64(a, b, subsets=(pi, ti), ret_var=True, parts=True)
    order = [2, 0, 1]
    _, _, moved = M.kid_distance64(a, b, subsets=(pi[order], ti[order]), ret_var=True, parts=True)
    assert torch.equal(moved, all3[order])
    for s in range(3):
        score, var, alone = M.kid_distance64(a, b, subsets=(pi[s:s + 1], ti[s:s + 1]), ret_var=True, parts=True)
        assert torch.equal(alone[0], all3[s])
        assert score.item() == all3[s, 19].item() and var.item() == all3[s, 20].item()
    assert not torch.equal(all3[0], all3[1])


def _raw_call(lib, X, Y, xi, yi, m, S, out, parts, ws, degree=3, gamma=None, coef0=1.0, mmd_est=0, want_var=1, var_at_m=None, Nx=None, Ny=None, D=None):
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    D = X.shape[1] if D is None else D
    return lib.mtd_kid(p(X), X.shape[0] if Nx is None else Nx, p(Y), Y.shape[0] if Ny is None else Ny, D, p(xi), p(yi), m, S, degree,
                       1.0 / max(D, 1) if gamma is None else gamma, coef0, mmd_est, want_var, m if var_at_m is None else var_at_m, p(out), p(parts), p(ws), None)


@pytest.mark.parametrize("N,D,S,m", [(65, 17, 1, 65), (150, 33, 4, 50), (130, 33, 2, 130)])
def test_nothing_is_written_outside_out_parts_and_the_workspace(hip_lib, N, D, S, m):
    from mtd_gan_amd import metrics as M
    x = R.F.features(N, D, 0, seed=70 + N)
    y = R.F.features(N, D, 0, seed=71 + N)
    xbuf = torch.full((N + 1, D), float("nan"))
    xbuf[:N] = x
    xd, yd = xbuf.cuda(), y.cuda()                          # a guard row of NaN behind X
    torch.manual_seed(8)
    pi, ti = R.draw(N, N, m, S)
    xi, yi = pi.to(torch.int32).cuda(), ti.to(torch.int32).cuda()
    nws = hip_lib.mtd_kid_ws_bytes(m, S)
    assert nws == S * 3 * ((m + 63) // 64) ** 2 * 132 * 8
    pad = 512
    out = torch.full((2 + 2 * S + pad,), SENTINEL, dtype=torch.float64, device="cuda")
    parts = torch.full((S * M.KID_PARTS + pad,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = torch.full((nws // 8 + 2 * pad,), SENTINEL, dtype=torch.float64, device="cuda")
    assert _raw_call(hip_lib, xd[:N], yd, xi, yi, m, S, out[pad // 2:], parts[pad // 2:], ws[pad:], var_at_m=N) == 0
    torch.cuda.synchronize()
    h = pad // 2
    assert (out[:h] == SENTINEL).all() and (out[h + 2 + 2 * S:] == SENTINEL).all()
    assert (parts[:h] == SENTINEL).all() and (parts[h + S * M.KID_PARTS:] == SENTINEL).all()
    assert (ws[:pad] == SENTINEL).all() and (ws[pad + nws // 8:] == SENTINEL).all()
    assert torch.isnan(xd[N]).all() and torch.equal(xd[:N].cpu(), x)
    want = M.kid_distance64(xd[:N], yd, subsets=(pi, ti), ret_var=True, parts=True)
    assert torch.equal(out[h:h + 2], torch.stack(want[:2])) and torch.equal(parts[h:h + S * M.KID_PARTS].view(S, -1), want[2])
    assert torch.equal(out[h + 2:h + 2 + 2 * S].view(S, 2), want[2][:, 19:21])
    # parts is optional
    out2 = torch.full((2 + 2 * S,), SENTINEL, dtype=torch.float64, device="cuda")
    assert _raw_call(hip_lib, xd[:N], yd, xi, yi, m, S, out2, None, ws[pad:], var_at_m=N) == 0
    assert torch.equal(out2, out[h:h + 2 + 2 * S])


def test_every_refusal_launches_nothing(hip_lib):
    L = hip_lib
    x, y = torch.rand(6, 4, device="cuda"), torch.rand(5, 4, device="cuda")
    idx = torch.arange(3, dtype=torch.int32, device="cuda").repeat(2, 1).contiguous()
    out = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    parts = torch.full((64,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = torch.full((L.mtd_kid_ws_bytes(3, 2) // 8,), SENTINEL, dtype=torch.float64, device="cuda")
    assert L.mtd_kid_ws_bytes(1, 1) == 0 and L.mtd_kid_ws_bytes(3, 0) == 0 and L.mtd_kid_ws_bytes(3, 21846) == 0 and L.mtd_kid_ws_bytes(-4, 1) == 0
    assert L.mtd_kid_ws_bytes(3, 21845) > 0
    good = dict(X=x, Y=y, xi=idx, yi=idx, m=3, S=2, out=out, parts=parts, ws=ws)
    bad = [dict(X=None), dict(Y=None), dict(xi=None), dict(yi=None), dict(out=None), dict(ws=None),
           dict(m=1), dict(m=2, want_var=1), dict(D=0), dict(degree=0), dict(degree=9), dict(S=0), dict(S=21846),
           dict(m=6), dict(m=6, Ny=6, Nx=5), dict(mmd_est=3), dict(var_at_m=1)]
    for change in bad:
        kw = dict(good, **change)
        X, Y = kw.pop("X"), kw.pop("Y")
        if X is None or Y is None:                          # (the helper reads the sizes from the tensors)
            p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
            rc = L.mtd_kid(p(X), 6, p(Y), 5, 4, idx.data_ptr(), idx.data_ptr(), 3, 2, 3, 0.25, 1.0, 0, 1, 3, out.data_ptr(), parts.data_ptr(), ws.data_ptr(), None)
        else:
            rc = _raw_call(L, X, Y, kw.pop("xi"), kw.pop("yi"), kw.pop("m"), kw.pop("S"), kw.pop("out"), kw.pop("parts"), kw.pop("ws"), **kw)
        assert rc == EINVAL, change
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (parts == SENTINEL).all() and (ws == SENTINEL).all()      # nothing ran
    assert _raw_call(L, x, y, idx, idx, 3, 2, out, parts, ws) == 0
    torch.cuda.synchronize()
    assert (out[:6] != SENTINEL).all() and (out[6:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("per_slice", [False, True])
def test_test_loop(hip_lib, tmp_path, per_slice):
    from mtd_gan_amd import engine, metrics as M
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    torch.manual_seed(3)
    m = MTD_GAN_Method().cuda()
    m.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    xs, ys = orc.synthetic_ldct(4, seed=9, size=64)
    step = 2 if per_slice else 1
    loader = [dict(n_20=xs[i:i + step], n_100=ys[i:i + step], path_n_20=[f"L000_000{i + j}.dcm" for j in range(step)],
                   path_n_100=[f"L000_000{i + j}.dcm" for j in range(step)]) for i in range(0, 4, step)]
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(17)
    w, bias = torch.randn(40, 3, 1, 1, generator=g).cuda(), torch.randn(40, generator=g).cuda()
    seen = []

    def extractor(t):                                    # a fixed random 1x1 conv (+ ReLU) and a mean pool to D = 40
        f = F.relu(F.conv2d(t, w, bias)).mean(dim=(2, 3), keepdim=True)
        seen.append(f.flatten(1).float())
        return [f]

    if per_slice:
        m.test_per_slice = True
    l1 = torch.nn.L1Loss()
    m.fid_features = extractor
    base = engine.test_MTD_GAN_Ours(m, l1, loader, dev, str(tmp_path / "base"))
    assert list(base.keys())[-3:] == ["input_fid", "gt_fid", "pred_fid"]
    for off in (False, None, {}):
        m.test_kid = off
        again = engine.test_MTD_GAN_Ours(m, l1, loader, dev, str(tmp_path / "off"))
        assert list(again.keys()) == list(base.keys()) and again == base
        assert open(tmp_path / "off" / "pred_results.csv").read() == open(tmp_path / "base" / "pred_results.csv").read()

    for cfg, names in ((True, ("kid",)), (dict(ret_var=True, degree=2), ("kid", "kid_var"))):
        m.test_kid = cfg
        del seen[:]
        full = engine.test_MTD_GAN_Ours(m, l1, loader, dev, str(tmp_path / "on"))
        new = [f"{who}_{n}" for n in names for who in ("input", "gt", "pred")]
        assert list(full.keys()) == list(base.keys()) + new
        assert all(full[k] == base[k] for k in base)
        assert open(tmp_path / "on" / "pred_results.csv").read() == open(tmp_path / "base" / "pred_results.csv").read()
        feats = [torch.cat(seen[k::3]) for k in range(3)]                # the loop's own feature rows: input, gt, pred per batch
        assert all(tuple(f.shape) == (4, 40) for f in feats)
        kw = {} if cfg is True else cfg
        triple = M.compute_KID(*feats, **kw)
        for j, who in enumerate(("input", "gt", "pred")):
            vals = triple[j] if len(names) == 2 else (triple[j],)
            for n, v in zip(names, vals):
                assert v.dtype == torch.float32 and full[f"{who}_{n}"] == round(v.item(), 7), (who, n)
            ref = R.kid(feats[j].cpu(), feats[1].cpu(), dict(R.CASES[0], opts=kw and dict(degree=2)), ret_var=len(names) == 2)
            got = M.kid_distance64(feats[j], feats[1], **dict(kw, ret_var=False)).item()
            print(f"test loop {who}_kid: hip {got:.15e} restatement {ref['mmd2']:.15e} |diff| {abs(got - ref['mmd2']):.2e}")
            assert abs(got - ref["mmd2"]) <= 4 * (2 * 3 * 86 + 4 * 20 + 16) * U * ref["parts"][0]["mag"]["mmd2"]
        assert full["pred_kid"] != full["gt_kid"]

    m.test_kid = True
    m.fid_features = None
    with pytest.raises(ValueError, match="fid_features"):
        engine.test_MTD_GAN_Ours(m, l1, loader, dev, None)
