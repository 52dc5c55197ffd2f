"""Time of the FID statistic's device work at the workload's size, D = 2048 features of N = 512 samples from the
seeded recipe of tests/_fid_ref.py: the statistics, one float64 product, one Newton-Schulz round and a whole compute_FID, each
beside the same arithmetic in torch float64 ops on the same device with the reference's host read of err in every round
(module/piq/fid.py:51-59) -- what a user would otherwise run.  One JSON line per item: median ms per call over --repeats timed
groups of --inner calls enqueued back to back, each group bracketed by device synchronisation on the host clock (a call rate:
it contains what the host and the launches cost wherever those set the pace), the executed float64 flop count (2 N D^2 per
covariance, 2 D^3 per product, the rounds the iteration actually ran) and the TFLOP/s they give.

    python tools/fid_timing.py [--repeats 7] [--inner 3] [--warmup 2] [--D 2048] [--N 512] [--out FILE]
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


def timed(torch, fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / inner)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="calls enqueued back to back per timed group")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--D", type=int, default=2048)
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import _lib, kernels as K, metrics as M
    import _fid_ref as R
    assert torch.cuda.is_available(), "fid_timing needs the GPU"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    D, N = a.D, a.N
    lines = []

    def emit(rec, ts, flops):
        v = sorted(ts)
        med = statistics.median(v)
        rec.update(D=D, N=N, repeats=a.repeats, inner=a.inner, ms=round(med, 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4),
                   gflop=round(flops / 1e9, 3), tflops_f64=round(flops / med / 1e9, 3))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        return med

    def torch_stats(x):
        x = x.double()
        mu = x.mean(dim=0)
        xc = x - mu
        return mu, (xc.t() @ xc) / (x.shape[0] - 1)

    def torch_rounds(A, rounds=None):
        """fid.py:42-61 in torch ops on the device; rounds=None: until its stop, with the host read of err in every round."""
        norm = A.norm()
        Y = A / norm
        eye = torch.eye(D, dtype=A.dtype, device=A.device)
        Z = eye.clone()
        n = 0
        for _ in range(rounds or R.MAX_ITERS):
            T = 0.5 * (3.0 * eye - Z @ Y)
            Y, Z = Y @ T, T @ Z
            S = Y * torch.sqrt(norm)
            err = (A - S @ S).norm() / norm
            n += 1
            if err.item() <= R.ATOL and rounds is None:
                break
        return S, n

    def torch_fid(p, t):
        (m1, s1), (m2, s2) = torch_stats(p), torch_stats(t)
        S, n = torch_rounds(s1 @ s2)
        if not torch.isfinite(S).all():
            eye = torch.eye(D, dtype=s1.dtype, device=s1.device) * R.EPS
            S, n = torch_rounds((s1 + eye) @ (s2 + eye))
        d = m1 - m2
        return (d.dot(d) + torch.trace(s1) + torch.trace(s2) - 2 * torch.trace(S)).float(), n

    with torch.no_grad():
        inp, tgt, prd = (R.features(N, D, 3, seed=4000 + i).to(dev) for i in range(3))
        # ---- statistics
        f_stats = 2.0 * N * D * D
        emit({"item": "statistics", "impl": "hip"}, timed(torch, lambda: M.fid_statistics(tgt), a.warmup, a.repeats, a.inner * 10), f_stats)
        emit({"item": "statistics", "impl": "torch_f64"}, timed(torch, lambda: torch_stats(tgt), a.warmup, a.repeats, a.inner * 10), f_stats)
        # ---- one product
        sa, sb = M.fid_statistics(inp), M.fid_statistics(tgt)
        out = torch.empty_like(sa[1])
        f_mm = 2.0 * D ** 3
        hip_mm = emit({"item": "product", "impl": "hip"},
                      timed(torch, lambda: L.mtd_fid_gemm(sa[1].data_ptr(), sb[1].data_ptr(), out.data_ptr(), D, 1.0, 0.0, K.stream_ptr()),
                            a.warmup, a.repeats, a.inner * 4), f_mm)
        torch_mm = emit({"item": "product", "impl": "torch_f64"}, timed(torch, lambda: torch.mm(sa[1], sb[1], out=out), a.warmup, a.repeats, a.inner * 4), f_mm)
        # ---- one round: the difference of a 5-round and a 1-round solve, over 4 (the iteration needs more than 5 rounds here)
        res, its = torch.empty(4, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        ws = K.workspace(L.mtd_fid_ws_bytes(D), dev)

        def hip_solve(rounds):
            _lib.check(L.mtd_fid_distance(sa[0].data_ptr(), sa[1].data_ptr(), sb[0].data_ptr(), sb[1].data_ptr(), D, 0.0, rounds, res.data_ptr(),
                                          its.data_ptr(), ws.data_ptr(), K.stream_ptr()), "mtd_fid_distance")
        hip_solve(R.MAX_ITERS)
        full_rounds = its.item()
        assert full_rounds > 5, full_rounds
        A = sa[1] @ sb[1]
        f_round = 4 * f_mm
        h1, h5 = (statistics.median(timed(torch, lambda r=r: hip_solve(r), a.warmup, a.repeats, a.inner)) for r in (1, 5))
        t1, t5 = (statistics.median(timed(torch, lambda r=r: torch_rounds(A, r), a.warmup, a.repeats, a.inner)) for r in (1, 5))
        emit({"item": "newton_schulz_round", "impl": "hip", "method": "(5 rounds - 1 round) / 4"}, [(h5 - h1) / 4], f_round)
        emit({"item": "newton_schulz_round", "impl": "torch_f64", "method": "(5 rounds - 1 round) / 4, host read of err per round"}, [(t5 - t1) / 4], f_round)
        # ---- a whole compute_FID: three solves; the reference's flow computes both statistics of every pair
        rounds_hip = []
        for p in (inp, tgt, prd):
            _, it = M._fid_solve(*M.fid_statistics(p), *M.fid_statistics(tgt), 0.0)
            rounds_hip.append(it.item())
        got = [t.item() for t in M.compute_FID(inp, tgt, prd)]
        ref = [torch_fid(p, tgt) for p in (inp, tgt, prd)]
        rounds_torch = [n for _, n in ref]
        f_hip = 3 * f_stats + sum((1 + 4 * r) * f_mm for r in rounds_hip)
        f_torch = 6 * f_stats + sum((1 + 4 * r) * f_mm for r in rounds_torch)
        hip_all = emit({"item": "compute_FID", "impl": "hip", "rounds": rounds_hip, "values": got},
                       timed(torch, lambda: M.compute_FID(inp, tgt, prd), 1, a.repeats, 1), f_hip)
        torch_all = emit({"item": "compute_FID", "impl": "torch_f64", "rounds": rounds_torch, "values": [v.item() for v, _ in ref]},
                         timed(torch, lambda: [torch_fid(p, tgt) for p in (inp, tgt, prd)], 1, a.repeats, 1), f_torch)
        line = json.dumps({"item": "ratios", "product_hip_over_torch_rate": round(torch_mm / hip_mm, 3),
                           "compute_FID_torch_over_hip_time": round(torch_all / hip_all, 3)})
        print(line, flush=True)
        lines.append(line)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
