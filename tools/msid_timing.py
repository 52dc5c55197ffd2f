"""Time of one MSID descriptor's device work at the workload's feature dimension, D = 2048, at piq's default
options (k = 5, m = 10, 100 starting vectors, 256 temperatures), on features from the seeded recipe of tests/_fid_ref.py at
N = 1000 and N = 5000: per stage (neighbours, graph, Lanczos, quadrature + combine: each stage call between two device
synchronises) and the whole metrics.msid_descriptor64 call; next to it the same descriptor on the host by the float64
restatement of tests/_msid_ref.py INCLUDING the device-to-host copy of the feature rows -- what a test loop that keeps its
features on the device would pay to use a host implementation (the restatement works on dense N x N matrices where piq uses
scipy's sparse ones; it is the host path this repository can run, not piq's own time).  One JSON line per item: the median over
--repeats calls after --warmup calls of the host clock around work that ends in a device synchronise, and the largest
difference of the two descriptors.

    python tools/msid_timing.py [--repeats 3] [--warmup 1] [--D 2048] [--sizes 1000,5000] [--out FILE]
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
    return sorted(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--D", type=int, default=2048)
    ap.add_argument("--sizes", default="1000,5000")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import _lib, kernels as K, metrics as M
    import _fid_ref as F
    import _msid_ref as R
    assert torch.cuda.is_available(), "msid_timing needs the GPU"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    D, k, m, nv = a.D, 5, 10, 100
    ts = torch.logspace(-1, 1, 256).numpy()
    nts = len(ts)
    lines = []

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    with torch.no_grad():
        for N in (int(s) for s in a.sizes.split(",")):
            x = F.features(N, D, 0, seed=6000 + N).to(dev)
            start_np = np.random.RandomState(N).randn(N, nv)
            start = torch.from_numpy(start_np).to(dev)
            tables, _ = M.msid_tables(ts, N, k, "empty")
            tab = torch.from_numpy(np.concatenate([ts.astype(np.float64), tables.reshape(-1)])).to(dev)
            nbr = torch.empty((N, k + 1), dtype=torch.int32, device=dev)
            rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
            col = torch.empty(2 * N * (k + 1), dtype=torch.int32, device=dev)
            T = torch.empty((nv, m, m), dtype=torch.float64, device=dev)
            traces = torch.empty((2, nts), dtype=torch.float64, device=dev)
            desc = torch.empty(nts, dtype=torch.float64, device=dev)
            ws = K.workspace(L.mtd_msid_ws_bytes(N, D, k, m, nv, nts), dev)
            sp = K.stream_ptr()

            def quad():
                _lib.check(L.mtd_msid_quadrature(T.data_ptr(), nv, m, N, tab.data_ptr(), nts, traces.data_ptr(), ws.data_ptr(), sp), "quadrature")
                _lib.check(L.mtd_msid_combine(traces.data_ptr(), tab[nts:].data_ptr(), nts, desc.data_ptr(), sp), "combine")
            stages = (
                ("neighbours", lambda: _lib.check(L.mtd_msid_neighbours(x.data_ptr(), N, D, k, nbr.data_ptr(), ws.data_ptr(), sp), "neighbours")),
                ("graph", lambda: _lib.check(L.mtd_msid_graph(nbr.data_ptr(), N, k, rowptr.data_ptr(), col.data_ptr(), ws.data_ptr(), sp), "graph")),
                ("lanczos", lambda: _lib.check(L.mtd_msid_lanczos(rowptr.data_ptr(), col.data_ptr(), col.numel(), N, start.data_ptr(), nv, m, 1, T.data_ptr(),
                                                                  None, ws.data_ptr(), sp), "lanczos")),
                ("quadrature_combine", quad))
            for name, fn in stages:
                t = timed(torch, fn, a.warmup, a.repeats)
                emit(item=f"N{N}", stage=name, impl="hip", N=N, D=D, k=k, m=m, niters=nv, nts=nts, repeats=a.repeats, ms=round(statistics.median(t), 4),
                     ms_min=round(t[0], 4), ms_max=round(t[-1], 4))
            deg = (rowptr[1:] - rowptr[:-1])
            t = timed(torch, lambda: M.msid_descriptor64(x, starting_vectors=start), a.warmup, a.repeats)
            hip_ms = statistics.median(t)
            got = M.msid_descriptor64(x, starting_vectors=start).cpu().numpy()
            emit(item=f"N{N}", stage="descriptor", impl="hip", N=N, D=D, repeats=a.repeats, ms=round(hip_ms, 4), ms_min=round(t[0], 4), ms_max=round(t[-1], 4),
                 nnz=int(rowptr[-1]), max_degree=int(deg.max()))

            def host():
                rows = x.cpu().numpy()                         # the device-to-host copy a host implementation needs
                return R.descriptor(rows, ts, start_np, k=k, m=m)["desc"]
            reps = max(1, a.repeats if N <= 1000 else 1)
            t = timed(torch, host, 0, reps)
            host_ms = statistics.median(t)
            t0 = time.perf_counter()
            x.cpu()
            copy_ms = (time.perf_counter() - t0) * 1e3
            emit(item=f"N{N}", stage="descriptor", impl="host_float64_restatement_with_copy", N=N, D=D, repeats=reps, ms=round(host_ms, 4),
                 copy_ms=round(copy_ms, 4), host_over_hip_time=round(host_ms / hip_ms, 3), max_abs_diff=float(np.abs(host() - got).max()))
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
