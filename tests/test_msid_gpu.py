"""MSID and the Inception Score on the device (csrc/msid.hip, metrics.msid_descriptor64 / msid_distance64 / inception_score64, the
test loop's opt-in model.test_msid / model.test_is) against the reference's own numbers (tests/golden/msid_is_cases.npz:
descriptors, scores and Inception Scores within the tolerances measured at pin time) and, stage by stage, against the float64
restatement of tests/_msid_ref.py.

The bound of a distance is worked out, not measured.  u = 2^-53.  Two float64 evaluations, in whatever order, of the dot product
of D terms differ by at most 2 D u of sum |x_i y_i| <= (dd_i + dd_j) / 2; dd_j carries D u of itself from its own sum; the
product by 2 is exact and the subtraction rounds once more: (2 D + 4) u of dd_i + dd_j + 2 |dot| covers both sides.  The
neighbour sets and the CSR are compared exactly (the pin tool asserts a relative gap of more than 1e-6 at the k-th neighbour).
T is compared within the relabelling bound stored with the fixture on the sets that run all m steps; on the sets that break early
the rows of T after the break are noise-determined, and the two traces are compared instead, each within what the descriptor's
stored bound allows it alone: tol div / 1e6 for the exp row and tol div exp(ts) / 1e6 for the identity row."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _msid_ref as R
import mtdgan_oracle as orc

pytestmark = pytest.mark.gpu
EINVAL = -1
U = 2.0 ** -53
SENTINEL = -7.0
_CACHE = {}


def _ref(index):
    """The restatement of a case, computed once and left unchanged."""
    if index not in _CACHE:
        case = R.CASES[index]
        p, t = R.case_features(case)
        _CACHE[index] = (p, t, R.msid(case))
    return _CACHE[index]


def _kwargs(case, mode=True):
    kw = dict(case["opts"])
    if not mode:
        kw.pop("msid_mode", None)
    if case["ts"] is not None:
        kw["ts"] = R.case_ts(case)
    return kw


def _ws(lib, *sizes):
    n = lib.mtd_msid_ws_bytes(*sizes)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device="cuda")


def _csr_of(parts):
    rowptr = parts["rowptr"].cpu().numpy().astype(np.int64)
    return rowptr, parts["col"].cpu().numpy().astype(np.int64)[:rowptr[-1]]


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_against_the_reference(hip_lib, index):
    from mtd_gan_amd import metrics as M
    _, z = R.golden()
    case, o = R.CASES[index], R.options(R.CASES[index])
    p, t, ref = _ref(index)
    assert R.crc(p, t) == int(z["crc"][index]), "the seeded features differ from those the fixture was computed on"
    pd, td = p.cuda(), t.cuda()
    np.random.seed(case["seed"])
    score = M.msid_distance64(pd, td, **_kwargs(case))
    assert score.is_cuda and score.dim() == 0 and score.dtype == torch.float64
    print(f"#{index}: hip {score.item():.15e} reference {z['score64'][index]:.15e} |diff| {abs(score.item() - z['score64'][index]):.2e} tol {z['stol'][index]:.2e}")
    assert abs(score.item() - z["score64"][index]) <= z["stol"][index]
    assert abs(score.item() - ref["score"]) <= z["stol"][index]
    explicit = M.msid_distance64(pd, td, starting_vectors=ref["start"], **_kwargs(case))
    assert torch.equal(explicit, score)                     # the seeded draw (predicted set first) and the supplied vectors: the same bits
    ts = R.case_ts(case)
    for side, (xd, key) in enumerate(((pd, "pred"), (td, "targ"))):
        want, tol = ref[key], z["dtol"][index, side]
        runs = [M.msid_descriptor64(xd, starting_vectors=ref["start"][side], parts=True, **_kwargs(case, mode=False)) for _ in range(2)]
        desc, parts = runs[0]
        assert desc.is_cuda and desc.dtype == torch.float64 and tuple(desc.shape) == (len(ts),)
        got = desc.cpu().numpy()
        diff = np.abs(got - z[f"desc_{index}_{side}"]).max()
        print(f"#{index}.{side}: descriptor max |diff| to the reference {diff:.2e} tol {tol:.2e}")
        assert diff <= tol and np.abs(got - want["desc"]).max() <= tol
        # neighbours: the same sets (self dropped, as the graph drops it); CSR: equal, columns rising
        nbr = parts["nbr"].cpu().numpy()
        assert nbr.shape == want["nbr"].shape
        for i in range(nbr.shape[0]):
            assert set(nbr[i]) - {i} == set(want["nbr"][i]) - {i}, i
        assert all(nbr[i, 0] == i for i in range(nbr.shape[0]))      # self is strictly the nearest
        rowptr, col = _csr_of(parts)
        wr, wc = R.csr(want["A"])
        assert np.array_equal(rowptr, wr) and np.array_equal(col, wc)
        T = parts["T"].cpu().numpy()
        tr = parts["traces"].cpu().numpy()
        if want["filled"] == o["m"]:
            worst = np.abs(T - want["T"]).max()
            print(f"#{index}.{side}: T max |diff| {worst:.2e} bound {z['ttol'][index, side]:.2e}")
            assert worst <= z["ttol"][index, side]
        tab = want["tables"]
        for row, bound in ((0, tol * tab[2] / 1e6), (1, tol * tab[2] * tab[0] / 1e6)):
            worst = (np.abs(tr[row] - want["traces"][row]) / bound).max()
            print(f"#{index}.{side}: trace row {row} worst |diff| / bound = {worst:.2e} (filled {want['filled']} of {o['m']})")
            assert worst <= 1.0
        assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in ("nbr", "rowptr", "T", "traces"))
        only = M.msid_descriptor64(xd, starting_vectors=torch.from_numpy(ref["start"][side]), **_kwargs(case, mode=False))
        assert torch.is_tensor(only) and torch.equal(only, desc)


@pytest.mark.parametrize("index,row0,rows", [(3, 0, 65), (3, 64, 1), (4, 60, 70), (13, 0, 64), (0, 0, 7)])
def test_distances(hip_lib, index, row0, rows):
    p, _, _ = _ref(index)
    N, D = p.shape
    want, mag = R.distances(p.numpy())
    pad = 256
    buf = torch.full((rows * N + 2 * pad,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = _ws(hip_lib, N, D, R.options(R.CASES[index])["k"], 2, 1, 1)
    assert hip_lib.mtd_msid_distances(p.cuda().data_ptr(), N, D, row0, rows, buf[pad:].data_ptr(), ws.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (buf[:pad] == SENTINEL).all() and (buf[pad + rows * N:] == SENTINEL).all()
    got = buf[pad:pad + rows * N].view(rows, N).cpu().numpy()
    ratio = np.abs(got - want[row0:row0 + rows]) / ((2 * D + 4) * U * mag[row0:row0 + rows])
    print(f"#{index} rows {row0}..{row0 + rows} of N={N} D={D}: worst |diff| / bound = {ratio.max():.3e}")
    assert ratio.max() <= 1.0


def test_the_stages_one_by_one(hip_lib):
    """Each stage called on its own gives the bits of the chained call; V on request: its first row is the normalised start and
    its filled rows are orthonormal."""
    from mtd_gan_amd import metrics as M
    L, index = hip_lib, 3
    case, o = R.CASES[index], R.options(R.CASES[index])
    p, _, ref = _ref(index)
    N, D = p.shape
    k, m, nv = o["k"], o["m"], o["niters"]
    ts = R.case_ts(case)
    nts = len(ts)
    xd = p.cuda()
    desc, parts = M.msid_descriptor64(xd, starting_vectors=ref["start"][0], parts=True, **_kwargs(case, mode=False))
    ws = _ws(L, N, D, k, m, nv, nts)
    nbr = torch.full((N, k + 1), -9, dtype=torch.int32, device="cuda")
    assert L.mtd_msid_neighbours(xd.data_ptr(), N, D, k, nbr.data_ptr(), ws.data_ptr(), None) == 0
    assert torch.equal(nbr, parts["nbr"])
    rowptr = torch.full((N + 1,), -9, dtype=torch.int32, device="cuda")
    col = torch.full((2 * N * (k + 1),), -9, dtype=torch.int32, device="cuda")
    assert L.mtd_msid_graph(nbr.data_ptr(), N, k, rowptr.data_ptr(), col.data_ptr(), ws.data_ptr(), None) == 0
    nnz = int(rowptr[-1])
    assert torch.equal(rowptr, parts["rowptr"]) and torch.equal(col[:nnz], parts["col"][:nnz]) and (col[nnz:] == -9).all()
    deg = (rowptr[1:] - rowptr[:-1]).cpu().numpy()
    assert deg.min() >= k and deg.max() > k + 1 and np.array_equal(deg, ref["pred"]["A"].sum(axis=1).astype(np.int64))      # a hub: no fixed-width list
    start = torch.from_numpy(ref["start"][0]).cuda()
    T = torch.full((nv, m, m), SENTINEL, dtype=torch.float64, device="cuda")
    V = torch.full((m, N, nv), SENTINEL, dtype=torch.float64, device="cuda")
    assert L.mtd_msid_lanczos(rowptr.data_ptr(), col.data_ptr(), col.numel(), N, start.data_ptr(), nv, m, 1, T.data_ptr(), V.data_ptr(), ws.data_ptr(), None) == 0
    assert torch.equal(T, parts["T"])
    Vh, sv = V.cpu().numpy(), ref["start"][0]
    assert np.abs(Vh[0] - sv / np.linalg.norm(sv, axis=0)).max() <= (N + 4) * U    # a sum of N squares in another order, a root, a division; |v| <= 1
    gram = np.einsum("anv,bnv->vab", Vh, Vh)
    assert np.abs(gram - np.eye(m)).max() <= 1e-5                                  # msid.py's own orthogonality tolerance
    # m = 3: two steps, each dividing a residual that carries a few N u of rounding by a beta of more than 0.1 (asserted)
    assert T.cpu().numpy()[:, [0, 1], [1, 2]].min() > 0.1 and np.abs(np.transpose(Vh, (1, 0, 2)) - ref["pred"]["V"]).max() <= 64 * N * U * 100
    tsd = torch.from_numpy(ts.astype(np.float64)).cuda()
    traces = torch.full((2, nts), SENTINEL, dtype=torch.float64, device="cuda")
    assert L.mtd_msid_quadrature(T.data_ptr(), nv, m, N, tsd.data_ptr(), nts, traces.data_ptr(), ws.data_ptr(), None) == 0
    assert torch.equal(traces, parts["traces"])
    tab = torch.from_numpy(ref["pred"]["tables"]).cuda()
    out = torch.full((nts,), SENTINEL, dtype=torch.float64, device="cuda")
    assert L.mtd_msid_combine(traces.data_ptr(), tab.data_ptr(), nts, out.data_ptr(), None) == 0
    assert torch.equal(out, desc)
    # the distance of two descriptors, both modes, on descriptors with the extreme at either end; a NaN is handed on
    a, b = desc.clone(), desc.clone()
    b[0] += 3.0
    b[-1] -= 5.0
    c = torch.from_numpy(ref["pred"]["c"]).cuda()
    res = torch.full((3,), SENTINEL, dtype=torch.float64, device="cuda")
    assert L.mtd_msid_distance(a.data_ptr(), b.data_ptr(), c.data_ptr(), nts, 0, res[1:].data_ptr(), None) == 0
    assert res[1].item() == max(float(c[0]) * abs(float(a[0] - b[0])), float(c[-1]) * abs(float(a[-1] - b[-1]))) and res[0] == SENTINEL and res[2] == SENTINEL
    assert L.mtd_msid_distance(a.data_ptr(), b.data_ptr(), None, nts, 1, res[1:].data_ptr(), None) == 0
    assert abs(res[1].item() - np.sqrt(float(a[0] - b[0]) ** 2 + float(a[-1] - b[-1]) ** 2)) <= 4 * U * 6 and res[2] == SENTINEL
    b[nts // 2] = float("nan")
    assert L.mtd_msid_distance(a.data_ptr(), b.data_ptr(), c.data_ptr(), nts, 0, res[1:].data_ptr(), None) == 0
    assert torch.isnan(res[1])


def test_relabelling_past_the_panel_and_chunk_thresholds(hip_lib):
    """N = 8256: 19 panels of 448 rows, the last one partial, and -- past N = 8192 -- Lanczos chunks of 128 rows, the last one of 64.
    No host reference at this size: the descriptor of the relabelled set (rows and starting vectors permuted together) is the same
    quantity in another summation order, within the floor the pin tool gives every descriptor, 1e-12 max|descriptor|.  A pair's
    distance has the same bits wherever its tile lies (the depth loop's order is fixed), so the graph is the same graph."""
    from mtd_gan_amd import metrics as M
    N, D, k, m, nv = 8256, 8, 2, 3, 5
    assert hip_lib.mtd_msid_panel_rows(N) == 448
    g = torch.Generator().manual_seed(41)
    x = torch.randn(N, D, generator=g)
    sv = torch.randn(N, nv, generator=g, dtype=torch.float64)
    perm = torch.randperm(N, generator=g)
    kw = dict(k=k, m=m, niters=nv, ts=np.array([0.1, 1.0, 10.0]))
    d0, p0 = M.msid_descriptor64(x.cuda(), starting_vectors=sv, parts=True, **kw)
    d1, p1 = M.msid_descriptor64(x[perm].contiguous().cuda(), starting_vectors=sv[perm].contiguous(), parts=True, **kw)
    rowptr, col = _csr_of(p0)
    rq, cq = _csr_of(p1)
    deg = np.diff(rowptr)
    assert deg.min() >= k and np.array_equal(np.diff(rq), deg[perm.numpy()])
    row_of = np.repeat(np.arange(N), deg)
    assert all(np.all(np.diff(col[rowptr[i]:rowptr[i + 1]]) > 0) for i in range(0, N, 97))          # rising columns
    assert set(zip(row_of.tolist(), col.tolist())) == set(zip(col.tolist(), row_of.tolist()))       # symmetric, and no self-loops
    assert not np.any(row_of == col)
    pn = perm.numpy()
    assert set(zip(pn[np.repeat(np.arange(N), np.diff(rq))].tolist(), pn[cq].tolist())) == set(zip(row_of.tolist(), col.tolist()))
    a, b = d0.cpu().numpy(), d1.cpu().numpy()
    print(f"N={N}: relabelled descriptor max |diff| {np.abs(a - b).max():.2e} bound {1e-12 * np.abs(a).max():.2e}")
    assert np.isfinite(a).all() and np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


def test_zero_rows_of_T_give_eigenvalue_zero_with_first_component_zero(hip_lib):
    """The quadrature on a T whose rows after an early break are zero: what np.linalg.eigh gives (msid.py:194-199)."""
    L, nv, m, n = hip_lib, 3, 6, 11
    T = np.zeros((nv, m, m))
    rng = np.random.RandomState(5)
    for v, filled in enumerate((2, 4, 6)):
        d, e = 2.0 + rng.rand(filled), 0.5 * rng.rand(filled - 1)        # eigenvalues in (1, 4)
        T[v, :filled, :filled] = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    ts = np.array([0.1, 1.0, 7.0])
    want = R.traces(T, ts, n)
    Td, tsd = torch.from_numpy(T).cuda(), torch.from_numpy(ts).cuda()
    out = torch.full((2 * 3 + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = _ws(L, 64, 4, 5, m, nv, 3)
    assert L.mtd_msid_quadrature(Td.data_ptr(), nv, m, n, tsd.data_ptr(), 3, out[1:].data_ptr(), ws.data_ptr(), None) == 0
    got = out[1:7].view(2, 3).cpu().numpy()
    assert out[0] == SENTINEL and out[7] == SENTINEL
    # e1^T f(-t T) e1 of a backward-stable eigensolver is exact for T + E, |E| <= c m u |T|, |T| <= 4, and moves by at most t |E|
    # for f = exp (eigenvalues > 0) and f = identity alike; c = 32 for either side
    assert np.abs(got - want).max() <= 64 * m * U * 7.0 * 4.0 * n


def test_nothing_is_written_outside_the_outputs(hip_lib):
    from mtd_gan_amd import metrics as M
    L, index = hip_lib, 1
    case, o = R.CASES[index], R.options(R.CASES[index])
    p, _, ref = _ref(index)
    N, D = p.shape
    k, m, nv = o["k"], o["m"], o["niters"]
    ts = R.case_ts(case)
    nts, pad = len(ts), 128
    xbuf = torch.full((N + 1, D), float("nan"))
    xbuf[:N] = p
    xd = xbuf.cuda()                                       # a guard row of NaN behind X
    want, parts = M.msid_descriptor64(xd[:N], starting_vectors=ref["start"][0], parts=True, **_kwargs(case, mode=False))
    host = torch.from_numpy(np.concatenate([ts.astype(np.float64), ref["pred"]["tables"].reshape(-1)])).cuda()
    start = torch.from_numpy(ref["start"][0]).cuda()
    sizes = dict(nbr=N * (k + 1), rowptr=N + 1, col=2 * N * (k + 1), T=nv * m * m, traces=2 * nts, desc=nts)
    bufs = {n: torch.full((s + 2 * pad,), -9 if n in ("nbr", "rowptr", "col") else SENTINEL, dtype=torch.int32 if n in ("nbr", "rowptr", "col") else torch.float64,
                          device="cuda") for n, s in sizes.items()}
    nws = L.mtd_msid_ws_bytes(N, D, k, m, nv, nts)
    ws = torch.full((nws // 8 + 2 * pad,), SENTINEL, dtype=torch.float64, device="cuda")
    ptr = {n: b[pad:].data_ptr() for n, b in bufs.items()}
    assert L.mtd_msid_descriptor(xd.data_ptr(), N, D, k, m, nv, 1, start.data_ptr(), host.data_ptr(), host[nts:].data_ptr(), nts, ptr["nbr"], ptr["rowptr"],
                                 ptr["col"], ptr["T"], ptr["traces"], ptr["desc"], ws[pad:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    for n, b in bufs.items():
        guard = -9 if b.dtype == torch.int32 else SENTINEL
        assert (b[:pad] == guard).all() and (b[pad + sizes[n]:] == guard).all(), n
    assert (ws[:pad] == SENTINEL).all() and (ws[pad + nws // 8:] == SENTINEL).all()
    desc = bufs["desc"][pad:pad + nts]
    assert (desc != SENTINEL).all() and torch.equal(desc, want)                # a sentinel-filled output of len(ts) is fully overwritten
    assert torch.equal(bufs["T"][pad:pad + sizes["T"]].view(nv, m, m), parts["T"])
    assert torch.isnan(xd[N]).all() and torch.equal(xd[:N].cpu(), p)


def test_every_refusal_launches_nothing(hip_lib):
    L = hip_lib
    N, D, k, m, nv, nts = 12, 4, 5, 4, 3, 2
    x = torch.rand(N, D, device="cuda")
    ints = torch.full((N * (k + 1) + N + 1 + 2 * N * (k + 1),), -9, dtype=torch.int32, device="cuda")
    nbr, rowptr, col = ints[:N * (k + 1)], ints[N * (k + 1):N * (k + 1) + N + 1], ints[N * (k + 1) + N + 1:]
    dbl = torch.full((nv * m * m + 2 * nts + nts,), SENTINEL, dtype=torch.float64, device="cuda")
    T, traces, desc = dbl[:nv * m * m], dbl[nv * m * m:nv * m * m + 2 * nts], dbl[nv * m * m + 2 * nts:]
    start = torch.rand(N, nv, dtype=torch.float64, device="cuda")
    tab = torch.ones(4 * nts, dtype=torch.float64, device="cuda")
    ws = torch.full((L.mtd_msid_ws_bytes(N, D, k, m, nv, nts) // 8,), SENTINEL, dtype=torch.float64, device="cuda")

    def call(**ch):
        a = dict(X=x.data_ptr(), N=N, D=D, k=k, m=m, nv=nv, start=start.data_ptr(), ts=tab.data_ptr(), tables=tab[nts:].data_ptr(), nts=nts,
                 nbr=nbr.data_ptr(), rowptr=rowptr.data_ptr(), col=col.data_ptr(), T=T.data_ptr(), traces=traces.data_ptr(), desc=desc.data_ptr(), ws=ws.data_ptr())
        a.update(ch)
        return L.mtd_msid_descriptor(a["X"], a["N"], a["D"], a["k"], a["m"], a["nv"], 1, a["start"], a["ts"], a["tables"], a["nts"], a["nbr"], a["rowptr"],
                                     a["col"], a["T"], a["traces"], a["desc"], a["ws"], None)
    for ch in [dict(X=None), dict(start=None), dict(ts=None), dict(tables=None), dict(nbr=None), dict(rowptr=None), dict(col=None), dict(T=None),
               dict(traces=None), dict(desc=None), dict(ws=None), dict(N=6), dict(N=32769), dict(D=0), dict(k=0), dict(k=64), dict(m=1), dict(m=33),
               dict(nv=0), dict(nv=4097), dict(nts=0)]:
        assert call(**ch) == EINVAL, ch
    assert L.mtd_msid_distances(x.data_ptr(), N, D, 8, 5, dbl.data_ptr(), ws.data_ptr(), None) == EINVAL      # rows past the set
    assert L.mtd_msid_lanczos(rowptr.data_ptr(), col.data_ptr(), -1, N, start.data_ptr(), nv, m, 1, T.data_ptr(), None, ws.data_ptr(), None) == EINVAL
    assert L.mtd_msid_distance(desc.data_ptr(), desc.data_ptr(), None, nts, 0, dbl.data_ptr(), None) == EINVAL    # 'max' without c
    assert L.mtd_msid_distance(desc.data_ptr(), desc.data_ptr(), tab.data_ptr(), nts, 2, dbl.data_ptr(), None) == EINVAL
    assert L.mtd_inception_score(x.data_ptr(), N, D, 13, dbl.data_ptr(), ws.data_ptr(), None) == EINVAL
    assert L.mtd_inception_score(x.data_ptr(), N, D, 0, dbl.data_ptr(), ws.data_ptr(), None) == EINVAL
    torch.cuda.synchronize()
    assert (ints == -9).all() and (dbl == SENTINEL).all() and (ws == SENTINEL).all()      # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert (desc != SENTINEL).all() and (nbr >= 0).all()


# ------------------------------------------------------------------------------------------------------------- Inception Score
@pytest.mark.parametrize("index", range(len(R.IS_CASES)))
def test_inception_score(hip_lib, index):
    from mtd_gan_amd import metrics as M
    _, z = R.golden()
    N, D, S, _ = R.IS_CASES[index]
    x = R.is_features(index)
    assert R.crc(x) == int(z["is_crc"][index])
    xd = x.cuda()
    mean, std = M.inception_score64(xd, S)
    assert mean.is_cuda and mean.dim() == 0 and mean.dtype == torch.float64 and std.dtype == torch.float64
    want = R.inception_score(x.numpy(), S)
    print(f"IS #{index} N={N} D={D} S={S}: hip {mean.item():.15e} +- {std.item():.6e} reference {z['is_val'][index, 0]:.15e} +- {z['is_val'][index, 1]:.6e} "
          f"tol {z['is_tol'][index, 0]:.1e}")
    assert abs(mean.item() - z["is_val"][index, 0]) <= z["is_tol"][index, 0] and abs(mean.item() - want[0]) <= z["is_tol"][index, 0]
    if S == 1:
        assert torch.isnan(std)
    else:
        assert abs(std.item() - z["is_val"][index, 1]) <= z["is_tol"][index, 1] and abs(std.item() - want[1]) <= z["is_tol"][index, 1]
    again = M.inception_score64(xd, S)
    assert torch.equal(again[0], mean) and (S == 1 or torch.equal(again[1], std))
    # the raw call: the split scores behind the pair, nothing outside out or the workspace
    pad, nws = 64, hip_lib.mtd_is_ws_bytes(N, D, S)
    out = torch.full((2 + S + 2 * pad,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = torch.full((nws // 8 + 2 * pad,), SENTINEL, dtype=torch.float64, device="cuda")
    assert hip_lib.mtd_inception_score(xd.data_ptr(), N, D, S, out[pad:].data_ptr(), ws[pad:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (out[:pad] == SENTINEL).all() and (out[pad + 2 + S:] == SENTINEL).all() and (ws[:pad] == SENTINEL).all() and (ws[pad + nws // 8:] == SENTINEL).all()
    assert torch.equal(out[pad], mean)
    assert np.abs(out[pad + 2:pad + 2 + S].cpu().numpy() - want[2]).max() <= z["is_tol"][index, 0]
    if index + 1 < len(R.IS_CASES):
        yd = R.is_features(index + 1).cuda()
        S2 = min(S, R.IS_CASES[index + 1][2])
        for j, how in enumerate(("l1", "l2")):
            d = M.is_distance64(xd, yd, num_splits=S2, distance=how)
            assert d.dim() == 0 and d.dtype == torch.float64 and abs(d.item() - z["is_dist"][index, j]) <= z["is_tol"][index, 0] + z["is_tol"][index + 1, 0]


def test_softmax_of_large_logits_and_zero_probabilities(hip_lib):
    """The maximum is subtracted (logits of 800 overflow exp otherwise) and a zero p_yx contributes 0."""
    from mtd_gan_amd import metrics as M
    x = torch.zeros(8, 5)
    x[:, 0] = 800.0
    x[4:, 0], x[4:, 1] = -800.0, 800.0
    mean, std = M.inception_score64(x.cuda(), 2)
    assert mean.item() == 1.0 and std.item() == 0.0          # each split is one class with probability exactly 1
    mean, _ = M.inception_score64(x.cuda(), 1)
    assert abs(mean.item() - 2.0) <= 32 * U                  # two equally likely classes, each row certain: exp(log 2)


# ------------------------------------------------------------------------------------------------------------- triples, engine
def test_the_triples(hip_lib):
    from mtd_gan_amd import metrics as M
    case = R.CASES[2]
    p, t, ref = _ref(2)
    a, b = p.cuda(), t.cuda()
    np.random.seed(31)
    triple = M.compute_MSID(a, b, a)
    assert len(triple) == 3 and all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in triple)
    np.random.seed(31)
    each = [M.msid_distance64(f, b) for f in (a, b, a)]      # three calls, each drawing anew, in the order input, gt, pred
    assert all(torch.equal(v, e.float()) for v, e in zip(triple, each))
    assert each[1].item() > 0 and not torch.equal(each[0], each[2])      # the target's descriptor is not shared: fresh vectors every time
    tri = M.compute_IS(a, b, a, num_splits=4)
    assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in tri)
    assert tri[1].item() == 0.0 and torch.equal(tri[0], tri[2]) and torch.equal(tri[0], M.is_distance64(a, b, num_splits=4).float())


def test_test_loop(hip_lib, tmp_path):
    from mtd_gan_amd import engine, metrics as M
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    torch.manual_seed(3)
    m = MTD_GAN_Method().cuda()
    m.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    xs, ys = orc.synthetic_ldct(16, seed=9, size=64)
    loader = [dict(n_20=xs[i:i + 8], n_100=ys[i:i + 8], path_n_20=[f"L000_000{i + j}.dcm" for j in range(8)],
                   path_n_100=[f"L000_000{i + j}.dcm" for j in range(8)]) for i in range(0, 16, 8)]      # two batches
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(17)
    w, bias = torch.randn(40, 3, 1, 1, generator=g).cuda(), torch.randn(40, generator=g).cuda()
    seen = []

    def extractor(t):                                    # a fixed random 1x1 conv (+ ReLU) and a mean pool to D = 40
        f = F.relu(F.conv2d(t, w, bias)).mean(dim=(2, 3), keepdim=True)
        seen.append(f.flatten(1).float())
        return [f]

    m.test_per_slice = True
    l1 = torch.nn.L1Loss()
    m.fid_features = extractor
    base = engine.test_MTD_GAN_Ours(m, l1, loader, dev, str(tmp_path / "base"))
    assert list(base.keys())[-3:] == ["input_fid", "gt_fid", "pred_fid"]                # the default run's keys are unchanged
    m.test_msid, m.test_is = False, None
    again = engine.test_MTD_GAN_Ours(m, l1, loader, dev, str(tmp_path / "off"))
    assert list(again.keys()) == list(base.keys()) and again == base
    assert open(tmp_path / "off" / "pred_results.csv").read() == open(tmp_path / "base" / "pred_results.csv").read()

    m.test_kid, m.test_msid, m.test_is = True, dict(k=3, niters=20), dict(num_splits=2)
    del seen[:]
    np.random.seed(77)
    full = engine.test_MTD_GAN_Ours(m, l1, loader, dev, str(tmp_path / "on"))
    new = [f"{who}_{n}" for n in ("kid", "msid", "is") for who in ("input", "gt", "pred")]
    assert list(full.keys()) == list(base.keys()) + new
    assert all(full[k] == base[k] for k in base)
    assert open(tmp_path / "on" / "pred_results.csv").read() == open(tmp_path / "base" / "pred_results.csv").read()
    feats = [torch.cat(seen[k::3]) for k in range(3)]
    assert all(tuple(f.shape) == (16, 40) for f in feats)
    np.random.seed(77)
    for name, triple in (("msid", M.compute_MSID(*feats, k=3, niters=20)), ("is", M.compute_IS(*feats, num_splits=2))):
        for who, v in zip(("input", "gt", "pred"), triple):
            assert v.dtype == torch.float32 and full[f"{who}_{name}"] == round(v.item(), 7), (who, name)
    assert full["gt_is"] == 0.0 and full["gt_msid"] > 0.0
    m.test_kid = None
    m.test_is = None
    m.test_msid = True
    m.fid_features = None
    with pytest.raises(ValueError, match="fid_features"):
        engine.test_MTD_GAN_Ours(m, l1, loader, dev, None)
