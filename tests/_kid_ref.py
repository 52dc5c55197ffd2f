"""Plain-torch float64 restatement of the Kernel Inception Distance (reference module/piq/kid.py): the polynomial kernel, the
named sums of _mmd2_and_variance, the three estimators, the variance estimate, the subset draws and their mean -- what the GPU
tests compare against, pinned to the reference's own numbers by tests/test_kid_cpu.py through tests/golden/kid_cases.npz
(tools/pin_kid.py).  Also the case table; the features come from the seeded recipe of tests/_fid_ref.py."""
import json
import os

import numpy as np
import torch

import _fid_ref as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kid_cases.npz")
MMD_ESTS = ("unbiased", "biased", "u-statistic")
# the order of mtd_kid's `parts` (include/mtdgan_hip.h)
PARTS = ("Kt_XX_sum", "Kt_YY_sum", "K_XY_sum", "sum_diag_X", "sum_diag_Y", "trace_XY", "sum_diag2_X", "sum_diag2_Y",
         "Kt_XX_2_sum", "Kt_YY_2_sum", "K_XY_2_sum", "sqn_Kt_XX_sums", "sqn_Kt_YY_sums", "sqn_K_XY_sums_1", "sqn_K_XY_sums_0",
         "dot_XX_XY", "dot_YY_YX", "zeta1_est", "zeta2_est", "mmd2", "var_est")
SUM_PARTS = PARTS[:17]          # sums of products of kernel values: positive wherever every kernel value is


def _case(Np, Nt, D, decay=0, subsets=None, seed=None, same=True, **opts):
    """subsets: None (the whole predicted set, average=False) or (S, m) (average=True).  opts: degree, gamma, coef0, mmd_est,
    var_at_m where they differ from kid.py's defaults.  same: the case also runs as KID(target, target)."""
    return dict(Np=Np, Nt=Nt, D=D, decay=decay, subsets=subsets, seed=seed, same=same, opts=opts)


WHOLE = [_case(2, 2, 1), _case(3, 3, 1), _case(5, 5, 7), _case(63, 63, 15), _case(64, 64, 16), _case(65, 65, 17), _case(130, 130, 33),
         _case(200, 200, 520), _case(211, 211, 2048), _case(96, 96, 96, decay=3)]
OPTION_SETS = [dict(degree=1), dict(degree=2), dict(degree=5), dict(gamma=0.5), dict(coef0=0.0), dict(coef0=2.5),
               dict(mmd_est="unbiased"), dict(mmd_est="biased"), dict(mmd_est="u-statistic"), dict(var_at_m=40)]
OPTIONS = [_case(N, N, D, same=False, **o) for (N, D) in ((65, 17), (130, 33)) for o in OPTION_SETS]
SUBSETS = [_case(130, 150, 33, subsets=(4, 50), seed=11), _case(130, 150, 33, subsets=(3, 64), seed=12),
           _case(130, 150, 33, subsets=None, seed=13)]
CASES = WHOLE + OPTIONS + SUBSETS
PRED_SCALE = 1.5                # the predicted set is another distribution than the target: its features are 1.5 x the recipe's


def case_features(case, index):
    """(predicted, target) fp32 feature sets of case number `index` (its place in CASES)."""
    p = F.features(case["Np"], case["D"], case["decay"], 3000 + 2 * index)
    t = F.features(case["Nt"], case["D"], case["decay"], 3001 + 2 * index)
    return (p * PRED_SCALE).contiguous(), t          # one correctly rounded fp32 product per element: the same bits everywhere


def crc(*tensors):
    return F.crc(*tensors)


def entries():
    """The fixture's entries in order: (index into CASES, same)."""
    return [(i, same) for i, c in enumerate(CASES) for same in ((False, True) if c["same"] else (False,))]


def options(case, D):
    o = dict(degree=3, gamma=None, coef0=1.0, mmd_est="unbiased", var_at_m=None)
    o.update(case["opts"])
    if o["gamma"] is None:
        o["gamma"] = 1.0 / D
    return o


def polynomial_kernel(A, B, degree, gamma, coef0):
    """kid.py:46-50 on float64 copies; an integer degree."""
    K = A.double() @ B.double().t()
    K = K * gamma + coef0
    return K.pow(int(degree))


def _sqn(t):
    f = t.flatten()
    return f.dot(f)


def parts_of(X, Y, degree=3, gamma=None, coef0=1.0, mmd_est="unbiased", var_at_m=None, ret_var=True, swap_xy_sums=False, keep_diag=False):
    """kid.py:53-140 on m rows X and m rows Y: a dict of python floats under the names of PARTS.  The last two arguments plant
    a defect for the pin tool's checks (the K_XY row and column sums exchanged; the diagonal left in Kt_XX_sums)."""
    m, D = X.shape
    assert Y.shape == X.shape and mmd_est in MMD_ESTS
    gamma = 1.0 / D if gamma is None else gamma
    var_at_m = m if var_at_m is None else var_at_m
    K_XX, K_YY, K_XY = (polynomial_kernel(a, b, degree, gamma, coef0) for a, b in ((X, X), (Y, Y), (X, Y)))
    diag_X, diag_Y = torch.diagonal(K_XX), torch.diagonal(K_YY)
    p = dict(sum_diag_X=diag_X.sum(), sum_diag_Y=diag_Y.sum(), sum_diag2_X=_sqn(diag_X), sum_diag2_Y=_sqn(diag_Y), trace_XY=torch.trace(K_XY))
    Kt_XX_sums = K_XX.sum(dim=1) - (0 if keep_diag else diag_X)
    Kt_YY_sums = K_YY.sum(dim=1) - diag_Y
    K_XY_sums_0, K_XY_sums_1 = K_XY.sum(dim=0), K_XY.sum(dim=1)
    if swap_xy_sums:
        K_XY_sums_0, K_XY_sums_1 = K_XY_sums_1, K_XY_sums_0
    p.update(Kt_XX_sum=Kt_XX_sums.sum(), Kt_YY_sum=Kt_YY_sums.sum(), K_XY_sum=K_XY_sums_0.sum())
    if mmd_est == "biased":
        mmd2 = (p["Kt_XX_sum"] + p["sum_diag_X"]) / (m * m) + (p["Kt_YY_sum"] + p["sum_diag_Y"]) / (m * m) - 2 * p["K_XY_sum"] / (m * m)
    else:
        mmd2 = (p["Kt_XX_sum"] + p["Kt_YY_sum"]) / (m * (m - 1))
        if mmd_est == "unbiased":
            mmd2 = mmd2 - 2 * p["K_XY_sum"] / (m * m)
        else:
            mmd2 = mmd2 - 2 * (p["K_XY_sum"] - p["trace_XY"]) / (m * (m - 1))
    p.update(Kt_XX_2_sum=_sqn(K_XX) - p["sum_diag2_X"], Kt_YY_2_sum=_sqn(K_YY) - p["sum_diag2_Y"], K_XY_2_sum=_sqn(K_XY),
             sqn_Kt_XX_sums=_sqn(Kt_XX_sums), sqn_Kt_YY_sums=_sqn(Kt_YY_sums), sqn_K_XY_sums_1=_sqn(K_XY_sums_1), sqn_K_XY_sums_0=_sqn(K_XY_sums_0),
             dot_XX_XY=Kt_XX_sums.dot(K_XY_sums_1), dot_YY_YX=Kt_YY_sums.dot(K_XY_sums_0), mmd2=mmd2)
    # mag: for every sum the sum of the magnitudes that went into it -- the diagonal that a Kt_* sum leaves out included, since
    # the reference subtracts it from a sum that holds it; what the error of any float64 evaluation is relative to
    full_XX, full_YY = K_XX.sum(dim=1), K_YY.sum(dim=1)
    mag = dict(p, Kt_XX_sum=full_XX.sum(), Kt_YY_sum=full_YY.sum(), Kt_XX_2_sum=_sqn(K_XX), Kt_YY_2_sum=_sqn(K_YY), sqn_Kt_XX_sums=_sqn(full_XX),
               sqn_Kt_YY_sums=_sqn(full_YY), dot_XX_XY=full_XX.dot(K_XY_sums_1), dot_YY_YX=full_YY.dot(K_XY_sums_0))
    p = {k: float(v) for k, v in p.items()}
    mag = {k: abs(float(v)) for k, v in mag.items() if k != "mmd2"}
    base_of = lambda q: (abs(q["Kt_XX_sum"]) + abs(q["Kt_YY_sum"])) / (m * (m - 1)) + 2 * abs(q["K_XY_sum"]) / (m * m)      # noqa: E731
    p.update(zeta1_est=0.0, zeta2_est=0.0, var_est=0.0, base=base_of(p), vbase=0.0)
    mag.update(zeta1_est=0.0, zeta2_est=0.0, var_est=0.0, mmd2=base_of(mag) + (mag["sum_diag_X"] + mag["sum_diag_Y"] + 2 * mag["trace_XY"]) / (m * (m - 1)))
    if ret_var:
        m1, m2 = m - 1, m - 2
        s2 = p["Kt_XX_sum"] ** 2 + p["Kt_YY_sum"] ** 2
        dots = p["dot_XX_XY"] + p["dot_YY_YX"]
        sums = (p["Kt_XX_sum"] + p["Kt_YY_sum"]) * p["K_XY_sum"]
        z1 = [1 / (m * m1 * m2) * (p["sqn_Kt_XX_sums"] - p["Kt_XX_2_sum"] + p["sqn_Kt_YY_sums"] - p["Kt_YY_2_sum"]),
              -1 / (m * m1) ** 2 * s2,
              1 / (m * m * m1) * (p["sqn_K_XY_sums_1"] + p["sqn_K_XY_sums_0"] - 2 * p["K_XY_2_sum"]),
              -2 / m ** 4 * p["K_XY_sum"] ** 2,
              -2 / (m * m * m1) * dots,
              2 / (m ** 3 * m1) * sums]
        z2 = [1 / (m * m1) * (p["Kt_XX_2_sum"] + p["Kt_YY_2_sum"]),
              -1 / (m * m1) ** 2 * s2,
              2 / (m * m) * p["K_XY_2_sum"],
              -2 / m ** 4 * p["K_XY_sum"] ** 2,
              -4 / (m * m * m1) * dots,
              4 / (m ** 3 * m1) * sums]
        w1, w2 = 4 * (var_at_m - 2) / (var_at_m * (var_at_m - 1)), 2 / (var_at_m * (var_at_m - 1))
        p["zeta1_est"], p["zeta2_est"] = sum(z1[1:], z1[0]), sum(z2[1:], z2[0])          # left to right, as kid.py writes them
        p["var_est"] = w1 * p["zeta1_est"] + w2 * p["zeta2_est"]

        def sizes(q):
            """The terms of zeta1_est and zeta2_est in absolute value, the sums inside the brackets too, each with its factor."""
            qs2, qd, qs = q["Kt_XX_sum"] ** 2 + q["Kt_YY_sum"] ** 2, q["dot_XX_XY"] + q["dot_YY_YX"], (q["Kt_XX_sum"] + q["Kt_YY_sum"]) * q["K_XY_sum"]
            common = 1 / (m * m1) ** 2 * qs2 + 2 / m ** 4 * q["K_XY_sum"] ** 2
            a1 = (1 / (m * m1 * m2) * (q["sqn_Kt_XX_sums"] + q["Kt_XX_2_sum"] + q["sqn_Kt_YY_sums"] + q["Kt_YY_2_sum"]) + common
                  + 1 / (m * m * m1) * (q["sqn_K_XY_sums_1"] + q["sqn_K_XY_sums_0"] + 2 * q["K_XY_2_sum"]) + 2 / (m * m * m1) * qd + 2 / (m ** 3 * m1) * qs)
            a2 = 1 / (m * m1) * (q["Kt_XX_2_sum"] + q["Kt_YY_2_sum"]) + common + 2 / (m * m) * q["K_XY_2_sum"] + 4 / (m * m * m1) * qd + 4 / (m ** 3 * m1) * qs
            return a1, a2
        a1, a2 = sizes({k: abs(v) for k, v in p.items()})
        p["vbase"] = abs(w1) * a1 + abs(w2) * a2
        mag["zeta1_est"], mag["zeta2_est"] = sizes(mag)
        mag["var_est"] = abs(w1) * mag["zeta1_est"] + abs(w2) * mag["zeta2_est"]
    p["mag"] = mag
    return p


def draw(Np, Nt, m, S):
    """The subsets as kid.py:230-232 draws them from torch's global CPU generator -- per subset first randperm(Np)[:m], then
    randperm(Nt)[:m] -- as two (S, m) int64 tensors.  Where a subset is the whole set its indices are taken in sorted order (the
    draw is still made, so the generator stays in step)."""
    pi, ti = [], []
    for _ in range(S):
        a = torch.randperm(Np)[:m]
        b = torch.randperm(Nt)[:m]
        pi.append(torch.arange(Np) if m == Np else a)
        ti.append(torch.arange(Nt) if m == Nt else b)
    return torch.stack(pi), torch.stack(ti)


def subset_shape(case, n_pred):
    """(S, m) of a case on a predicted set of n_pred rows: kid.py:199-204,224-227."""
    return case["subsets"] if case["subsets"] is not None else (1, n_pred)


def kid(pred, targ, case, ret_var=True, subsets=None):
    """dict(mmd2, var, base, vbase, parts=[per-subset dicts]) of the case on (pred, targ): seeds the global generator with the
    case's seed (where it has one) and draws, unless `subsets` is given; var_at_m = min(N_pred, N_targ) unless the case sets it."""
    o = options(case, pred.shape[1])
    S, m = subset_shape(case, pred.shape[0])
    if subsets is None:
        if case["seed"] is not None:
            torch.manual_seed(case["seed"])
        subsets = draw(pred.shape[0], targ.shape[0], m, S)
    if o["var_at_m"] is None:
        o["var_at_m"] = min(pred.shape[0], targ.shape[0])
    rv = ret_var and m >= 3
    per = [parts_of(pred[pi], targ[ti], ret_var=rv, **o) for pi, ti in zip(*subsets)]
    mean = lambda k: float(torch.tensor([q[k] for q in per], dtype=torch.float64).mean())      # noqa: E731
    return dict(mmd2=mean("mmd2"), var=mean("var_est"), base=mean("base"), vbase=mean("vbase"), parts=per, subsets=subsets)


def golden():
    """(meta, rows): the fixture as a list of dicts in the order of entries()."""
    z = np.load(GOLDEN)
    n = len(z["mmd2_64"])
    return json.loads(str(z["meta"])), [dict(index=int(z["index"][i]), same=bool(z["same"][i]), mmd2_64=float(z["mmd2_64"][i]), var_64=float(z["var_64"][i]),
                                            mmd2_32=np.float32(z["mmd2_32"][i]), var_32=np.float32(z["var_32"][i]), base=float(z["base"][i]),
                                            vbase=float(z["vbase"][i]), tol=float(z["tol"][i]), vtol=float(z["vtol"][i]), crc=int(z["crc"][i]),
                                            has_var=bool(z["has_var"][i]), has_32=bool(z["has_32"][i])) for i in range(n)]
