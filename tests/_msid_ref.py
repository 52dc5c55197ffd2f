"""Float64 numpy restatement of the Multi-Scale Intrinsic Distance (reference module/piq/msid.py) and of the Inception Score
(module/piq/isc.py), stage by stage and without scipy: the neighbour table, the symmetric graph and its CSR, the Laplacian,
_lanczos_m with its reorthogonalisation passes and its break, the quadrature, the temperature tables in the dtype `ts` arrives
in, the descriptor and the score -- what the GPU tests compare against, pinned to the reference's own numbers by
tests/test_msid_cpu.py through tests/golden/msid_is_cases.npz (tools/pin_msid.py).  Also the case tables; the features come
from the seeded recipe of tests/_fid_ref.py and are regenerated, not stored."""
import json
import os

import numpy as np
import torch

import _fid_ref as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msid_is_cases.npz")
EPSILON, NORMALIZATION, ORTHTOL = 1e-6, 1e6, 1e-5
DEFAULTS = dict(k=5, m=10, niters=100, rademacher=False, normalized_laplacian=True, normalize="empty", msid_mode="max")


def _case(Np, Nt, D, seed, ts=None, **opts):
    """ts: None (piq's float32 logspace) or 'f64x5' (five float64 temperatures)."""
    return dict(Np=Np, Nt=Nt, D=D, seed=seed, ts=ts, opts=opts)


CASES = [
    _case(7, 8, 16, 1),                                   # k = 5 on 7 rows: a complete graph, the Krylov space ends at step 2
    _case(9, 9, 24, 2, niters=16),
    _case(40, 40, 96, 3),
    _case(65, 65, 33, 4, k=2, m=3, niters=33),            # one past a 64-row tile, odd counts
    _case(130, 300, 64, 5),                               # unequal sets: the float32 `sub` does not cancel
    _case(40, 40, 48, 6, m=2),
    _case(40, 40, 48, 7, rademacher=True),
    _case(40, 40, 48, 8, normalized_laplacian=False),
    _case(40, 50, 48, 9, normalize="complete"),
    _case(40, 50, 48, 10, normalize="er"),
    _case(40, 50, 48, 11, normalize="none"),
    _case(40, 40, 48, 12, msid_mode="l2"),
    _case(130, 300, 64, 5, ts="f64x5"),                   # the features of case 4
    _case(64, 64, 2048, 13),                              # the depth loop of the distance product
]
UNEQUAL, UNEQUAL_F64 = 4, 12
# (N, D, num_splits, seed); each also gives IS(pred, target) distances between neighbours in the table
IS_CASES = [(40, 10, 10, 1), (65, 33, 4, 2), (130, 96, 1, 3), (300, 64, 10, 4), (12, 1000, 3, 5)]
IS_SCALE = 3.0


def options(case):
    o = dict(DEFAULTS)
    o.update(case["opts"])
    return o


def case_ts(case):
    if case["ts"] is None:
        return torch.logspace(-1, 1, 256).numpy()
    return np.array([0.1, 0.5, 1.0, 3.0, 10.0], dtype=np.float64)


def case_features(case):
    """(predicted, target) fp32 feature sets of a case, as torch tensors."""
    s = case["seed"]
    return F.features(case["Np"], case["D"], 0, 5000 + 2 * s), F.features(case["Nt"], case["D"], 0, 5001 + 2 * s)


def is_features(index):
    N, D, _, seed = IS_CASES[index]
    return (F.features(N, D, 0, 7000 + seed) * IS_SCALE).contiguous()


def crc(*tensors):
    return F.crc(*tensors)


# ----------------------------------------------------------------------------------------------------------------- graph
def distances(X):
    """msid.py:29-32 for every row: dist[i][j] = dd[j] - 2 Xi . Xj, and the magnitude dd_i + dd_j + 2 |Xi . Xj| that a float64
    evaluation's error is relative to."""
    X = np.asarray(X, dtype=np.float64)
    dd = np.sum(X * X, axis=1)
    dot = X @ X.T
    return dd[None, :] - 2 * dot, dd[:, None] + dd[None, :] + 2 * np.abs(dot)


def neighbours(X, k):
    """(N, k + 1) ints: per row the k + 1 smallest distances' indices in rising (distance, index) order, and the smallest relative
    gap between the (k + 1)-th and (k + 2)-th distance of a row (np.argpartition leaves ties open: the pin tool asserts the gap)."""
    dist, mag = distances(X)
    n = dist.shape[0]
    nbr = np.zeros((n, k + 1), dtype=np.int64)
    gap = np.inf
    for i in range(n):
        order = np.lexsort((np.arange(n), dist[i]))
        nbr[i] = order[:k + 1]
        if n > k + 1:
            a, b = order[k], order[k + 1]
            gap = min(gap, (dist[i, b] - dist[i, a]) / max(mag[i, a], mag[i, b]))
    return nbr, gap


def self_is_nearest(X):
    dist, _ = distances(X)
    n = dist.shape[0]
    off = dist + np.where(np.eye(n, dtype=bool), np.inf, 0.0)
    return bool(np.all(np.diag(dist) < off.min(axis=1)))


def adjacency(nbr, union=True, keep_self=False):
    """msid.py:31-37, 235-237 as a dense 0/1 matrix.  The two switches plant a defect for the pin tool's checks."""
    n = nbr.shape[0]
    A = np.zeros((n, n))
    for i in range(n):
        for j in nbr[i]:
            if j != i or keep_self:
                A[i, j] = 1.0
    if union:
        A = ((A + A.T) > 0).astype(np.float64)
    return A


def csr(A):
    rowptr = np.concatenate([[0], np.cumsum((A != 0).sum(axis=1))]).astype(np.int64)
    col = np.concatenate([np.nonzero(A[i])[0] for i in range(A.shape[0])]).astype(np.int64)
    return rowptr, col


def laplacian(A, normalized=True):
    """msid.py:40-46."""
    row_sum = A.sum(axis=1)
    if not normalized:
        return np.diag(row_sum) - A
    s = 1 / np.sqrt(row_sum)
    return np.eye(A.shape[0]) - (s[:, None] * A) * s[None, :]


# ----------------------------------------------------------------------------------------------------------------- Lanczos
def lanczos(L, m, start):
    """msid.py:49-135 on a dense L with the starting vectors given: (T (nv, m, m), V (n, m, nv), the number of basis rows filled,
    the number of extra reorthogonalisation passes)."""
    sv = np.array(start, dtype=np.float64)
    n, nv = sv.shape
    V = np.zeros((n, m, nv))
    T = np.zeros((nv, m, m))
    sv = sv / np.linalg.norm(sv, axis=0)
    V[:, 0, :] = sv
    w = L.dot(sv)
    alpha = np.einsum("ij,ij->j", w, sv)
    w -= alpha[None, :] * sv
    beta = np.sqrt(np.einsum("ij,ij->j", w, w))
    T[:, 0, 0] = alpha
    T[:, 0, 1] = beta
    T[:, 1, 0] = beta
    w = w / beta[None, :]
    V[:, 1, :] = w
    filled, passes = 2, 0
    for i in range(1, m):
        old, cur = V[:, i - 1, :], V[:, i, :]
        w = L.dot(cur)
        w -= beta[None, :] * old
        alpha = np.einsum("ij,ij->j", w, cur)
        T[:, i, i] = alpha
        if i < m - 1:
            w -= alpha[None, :] * cur
            t = np.einsum("ijk,ik->jk", V, w)
            w -= np.einsum("ijk,jk->ik", V, t)
            beta = np.sqrt(np.einsum("ij,ij->j", w, w))
            w = w / beta[None, :]
            T[:, i, i + 1] = beta
            T[:, i + 1, i] = beta
            innerprod = np.einsum("ijk,ik->jk", V, w)
            reortho = False
            for _ in range(100):
                if not (innerprod > ORTHTOL).sum():
                    reortho = True
                    break
                t = np.einsum("ijk,ik->jk", V, w)
                w -= np.einsum("ijk,jk->ik", V, t)
                w = w / np.linalg.norm(w, axis=0)[None, :]
                innerprod = np.einsum("ijk,ik->jk", V, w)
                passes += 1
            V[:, i + 1, :] = w
            filled = i + 2
            if (np.abs(beta) > 1e-6).sum() == 0 or not reortho:
                break
    return T, V, filled, passes


def traces(T, ts, n):
    """msid.py:193-199 with fs = [exp, identity]: (2, len(ts)).  ts in its own dtype: np.outer upcasts."""
    nv, m, _ = T.shape
    eigvals, eigvecs = np.linalg.eigh(T)
    sq = np.power(eigvecs[:, 0, :], 2)
    out = np.zeros((2, len(ts)))
    for i, f in enumerate((np.exp, lambda x: x)):
        fe = f(-np.outer(ts, eigvals)).reshape(ts.shape[0], nv, m)
        out[i] = n * (fe * sq).sum(-1).mean(-1)
    return out


def tables(ts, n, k, normalize):
    """What depends on (ts, n, k) alone, by the reference's own numpy expressions in the dtype of ts, as float64:
    (3, len(ts)) = exp(ts), sub (msid.py:218-219), the divisor of _normalize_msid; and c (msid.py:389)."""
    ts = np.asarray(ts)
    expts = np.exp(ts)
    sub = -ts * n / np.exp(ts)
    if normalize == "empty":
        div = np.full(ts.shape, n, dtype=np.float64)
    elif normalize == "complete":
        div = 1 + (n - 1) * np.exp(-(1 + 1 / (n - 1)) * ts)
    elif normalize == "er":
        xs = np.linspace(0, 1, n)
        er_spectrum = 4 / np.sqrt(k) * xs + 1 - 2 / np.sqrt(k)
        div = np.exp(-np.outer(ts, er_spectrum)).sum(-1) + EPSILON
    elif normalize == "none" or normalize is None:
        div = np.ones(ts.shape, dtype=np.float64)
    else:
        raise ValueError("Unknown normalization parameter!")
    c = np.exp(-2 * (ts + 1 / ts))
    return np.stack([expts.astype(np.float64), sub.astype(np.float64), np.asarray(div, dtype=np.float64)]), c.astype(np.float64)


def combine(tr, tab):
    return ((tr[0] - tr[1] / tab[0]) + tab[1]) / tab[2] * NORMALIZATION


def draw(n, niters, rademacher):
    sv = np.random.randn(n, niters)
    return np.sign(sv) if rademacher else sv


def descriptor(X, ts, start, k=5, m=10, normalized_laplacian=True, normalize="empty", union=True, keep_self=False, **_):
    """A dict of every stage of one descriptor on the starting vectors `start`."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    nbr, gap = neighbours(X, k)
    A = adjacency(nbr, union=union, keep_self=keep_self)
    T, V, filled, passes = lanczos(laplacian(A, normalized_laplacian), m, start)
    tr = traces(T, ts, n)
    tab, c = tables(ts, n, k, normalize)
    return dict(nbr=nbr, gap=gap, A=A, T=T, V=V, filled=filled, passes=passes, traces=tr, tables=tab, c=c, desc=combine(tr, tab))


def score(dp, dt, c, mode):
    if mode == "l2":
        return float(np.linalg.norm(dp - dt))
    return float(np.amax(c * np.abs(dp - dt)))


def msid(case, p=None, t=None):
    """The case end to end after np.random.seed(seed of the case): the predicted set's vectors are drawn first."""
    o = options(case)
    if p is None:
        p, t = (x.numpy() for x in case_features(case))
    ts = case_ts(case)
    np.random.seed(case["seed"])
    sp = draw(p.shape[0], o["niters"], o["rademacher"])
    st = draw(t.shape[0], o["niters"], o["rademacher"])
    a, b = descriptor(p, ts, sp, **o), descriptor(t, ts, st, **o)
    return dict(pred=a, targ=b, start=(sp, st), score=score(a["desc"], b["desc"], a["c"], o["msid_mode"]))


# ----------------------------------------------------------------------------------------------------------------- IS
def inception_score(X, num_splits=10):
    """isc.py:20-55 on float64 copies: (mean, unbiased std, the split scores)."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    e = np.exp(X - X.max(axis=1, keepdims=True))
    probas = e / e.sum(axis=1, keepdims=True)
    R = N // num_splits
    parts = []
    for i in range(num_splits):
        sub = probas[i * R:(i + 1) * R]
        p_y = sub.mean(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            kl = np.where(sub > 0, sub * np.log(sub) - sub * np.log(p_y)[None, :], 0.0).sum(axis=1)
        parts.append(np.exp(kl.mean()))
    parts = np.array(parts)
    with np.errstate(divide="ignore", invalid="ignore"):
        std = np.sqrt(((parts - parts.mean()) ** 2).sum() / np.float64(num_splits - 1))
    return float(parts.mean()), float(std), parts


def golden():
    z = np.load(GOLDEN)
    return json.loads(str(z["meta"])), z
