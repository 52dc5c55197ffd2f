"""No-grad generator inference of 8 whole slices with fp32 and with binary16 activation storage (ResFFT_Generator.activation_dtype,
DESIGN 3.3), the two modes ALTERNATING call by call in one process so that both see the same clocks, the same allocator state and
the same neighbours.  One JSON line per mode and size: ms per 8 slices (median and minimum of --repeats timed calls, each bracketed
by device synchronisation), the spread of the repeats, and binary16's ratio to fp32.

    python tools/half_inference_timing.py [--repeats 15] [--warmup 3] [--sizes 512,256,128] [--slices 8] [--out FILE]
    python tools/half_inference_timing.py --once float16 --sizes 512      # one warmed call of one mode (for a kernel trace)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--sizes", default="512,256,128")
    ap.add_argument("--once", default=None, choices=["float32", "float16"], help="warm up, then ONE call of this mode per size; no timing")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd.arch.Ours.networks import ResFFT_Generator
    from mtd_gan_amd.data import synthetic_ldct
    dev = torch.device("cuda:0")
    torch.manual_seed(2024)                                   # the inference512 workload's generator (bench_workloads.py)
    G = ResFFT_Generator(1, 32, 10, 3, 1).to(dev).eval()
    modes = [("float32", torch.float32), ("float16", torch.float16)]
    lines = []
    for s in a.sizes.split(","):
        S = int(s)
        x, _ = synthetic_ldct(a.slices, seed=1234, size=S)
        x = x.to(dev)
        ts = {name: [] for name, _ in modes}
        with torch.no_grad():
            if a.once:
                G.activation_dtype = dict(modes)[a.once]
                for _ in range(a.warmup + 1):
                    G(x)
                torch.cuda.synchronize()
                continue
            for _ in range(a.warmup):
                for _name, dt in modes:
                    G.activation_dtype = dt
                    G(x)
            torch.cuda.synchronize()
            for _ in range(a.repeats):
                for name, dt in modes:
                    G.activation_dtype = dt
                    t0 = time.perf_counter()
                    G(x)
                    torch.cuda.synchronize()
                    ts[name].append((time.perf_counter() - t0) * 1e3)
        med = {name: statistics.median(v) for name, v in ts.items()}
        for name, _ in modes:
            v = sorted(ts[name])
            rec = {"activation_dtype": name, "S": S, "slices": a.slices, "repeats": a.repeats, "ms": round(med[name], 3),
                   "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3), "ms_p25": round(v[len(v) // 4], 3), "ms_p75": round(v[(3 * len(v)) // 4], 3),
                   "vs_float32": round(med[name] / med["float32"], 4)}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
