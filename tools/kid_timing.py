"""Time of KID's device work at the workload's feature dimension, D = 2048, on features from the seeded recipe of
tests/_fid_ref.py: N = 211 and N = 1000 on the whole sets, and N = 5000 with average=True at piq's defaults (50 subsets of
1000), each with and without the variance estimate, beside the same computation in torch float64 ops (mm, pow, sums: what a
user of piq on .double() features would run) on the same GPU in the same process and on the same subsets.  One JSON line per
item: the median over --repeats calls, after --warmup calls, of the host clock around one call that ends in a device
synchronise (a call time: it contains the host's draw of the subsets and the launches), the float64 flop count of the three
Gram products (3 . 2 m^2 D per subset) and the TFLOP/s they give, and the two values side by side.

    python tools/kid_timing.py [--repeats 5] [--warmup 1] [--D 2048] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = (dict(name="N211_whole", N=211, kw={}), dict(name="N1000_whole", N=1000, kw={}),
           dict(name="N5000_50x1000", N=5000, kw=dict(average=True, n_subsets=50, subset_size=1000)))


def timed(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--D", type=int, default=2048)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import metrics as M
    import _fid_ref as F
    import _kid_ref as R
    assert torch.cuda.is_available(), "kid_timing needs the GPU"
    dev = torch.device("cuda:0")
    D = a.D
    lines = []

    def torch_kid(p, t, pi, ti, ret_var):
        """kid.py on the device in float64 ops, on the given subsets."""
        vals = []
        for i, j in zip(pi, ti):
            x, y = p[i].double(), t[j].double()
            m = x.shape[0]
            kern = lambda u, v: (torch.mm(u, v.t()) * (1.0 / D) + 1.0).pow(3)      # noqa: E731
            K_XX, K_YY, K_XY = kern(x, x), kern(y, y), kern(x, y)
            dX, dY = torch.diagonal(K_XX), torch.diagonal(K_YY)
            sX, sY, s0, s1 = K_XX.sum(dim=1) - dX, K_YY.sum(dim=1) - dY, K_XY.sum(dim=0), K_XY.sum(dim=1)
            SX, SY, SXY = sX.sum(), sY.sum(), s0.sum()
            mmd2 = (SX + SY) / (m * (m - 1)) - 2 * SXY / (m * m)
            if not ret_var:
                vals.append(torch.stack([mmd2, torch.zeros_like(mmd2)]))
                continue
            sqn = lambda v: v.flatten().dot(v.flatten())      # noqa: E731
            X2, Y2, XY2 = sqn(K_XX) - sqn(dX), sqn(K_YY) - sqn(dY), sqn(K_XY)
            dots = sX.dot(s1) + sY.dot(s0)
            m1, m2 = m - 1, m - 2
            z1 = (1 / (m * m1 * m2) * (sqn(sX) - X2 + sqn(sY) - Y2) - 1 / (m * m1) ** 2 * (SX ** 2 + SY ** 2)
                  + 1 / (m * m * m1) * (sqn(s1) + sqn(s0) - 2 * XY2) - 2 / m ** 4 * SXY ** 2 - 2 / (m * m * m1) * dots + 2 / (m ** 3 * m1) * (SX + SY) * SXY)
            z2 = (1 / (m * m1) * (X2 + Y2) - 1 / (m * m1) ** 2 * (SX ** 2 + SY ** 2) + 2 / (m * m) * XY2 - 2 / m ** 4 * SXY ** 2
                  - 4 / (m * m * m1) * dots + 4 / (m ** 3 * m1) * (SX + SY) * SXY)
            v = min(p.shape[0], t.shape[0])
            vals.append(torch.stack([mmd2, 4 * (v - 2) / (v * (v - 1)) * z1 + 2 / (v * (v - 1)) * z2]))
        return torch.stack(vals).mean(dim=0)

    with torch.no_grad():
        for cfg in CONFIGS:
            N = cfg["N"]
            p, t = (F.features(N, D, 0, seed=5000 + k).to(dev) for k in range(2))
            p = p * 1.5
            S, m = (cfg["kw"]["n_subsets"], cfg["kw"]["subset_size"]) if cfg["kw"] else (1, N)
            torch.manual_seed(31)
            pi, ti = R.draw(N, N, m, S)
            pid, tid = pi.to(dev), ti.to(dev)
            flops = 3 * 2.0 * m * m * D * S
            for ret_var in (False, True):
                def hip():
                    torch.manual_seed(31)
                    return M.kid_distance64(p, t, ret_var=ret_var, **cfg["kw"])
                got = hip()
                got = [v.item() for v in (got if ret_var else (got,))]
                ref = torch_kid(p, t, pid, tid, ret_var).tolist()
                meds = {}
                for impl, fn in (("hip", hip), ("torch_f64", lambda: torch_kid(p, t, pid, tid, ret_var))):
                    ts = sorted(timed(torch, fn, a.warmup, a.repeats))
                    med = statistics.median(ts)
                    meds[impl] = med
                    rec = dict(item=cfg["name"], impl=impl, N=N, D=D, subsets=S, m=m, ret_var=ret_var, repeats=a.repeats, ms=round(med, 4),
                               ms_min=round(ts[0], 4), ms_max=round(ts[-1], 4), gflop=round(flops / 1e9, 3), tflops_f64=round(flops / med / 1e9, 3),
                               values=got if impl == "hip" else ref[:len(got)])
                    line = json.dumps(rec)
                    print(line, flush=True)
                    lines.append(line)
                line = json.dumps(dict(item=cfg["name"], ret_var=ret_var, torch_over_hip_time=round(meds["torch_f64"] / meds["hip"], 3),
                                       value_diff=[abs(x - y) for x, y in zip(got, ref)]))
                print(line, flush=True)
                lines.append(line)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
