"""No-grad generator inference of 8 slices per size over a table of slice sizes (ResFFT_Generator.allow_any_size: the general-length
spectral path for every size but the 512 x 512 baseline, which is the inference512 workload of bench.py).  One JSON line per size:
ms per 8 slices (median of --repeats timed calls, each bracketed by device synchronisation) and ns per pixel.

    python tools/any_size_timing.py [--repeats 7] [--warmup 3] [--sizes 512x512,384x512,...] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(512, 512), (384, 512), (480, 480), (500, 512), (509, 509), (437, 389), (100, 77)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--sizes", default=",".join(f"{h}x{w}" for h, w in SIZES))
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd.arch.Ours.networks import ResFFT_Generator
    from mtd_gan_amd.data import synthetic_ldct
    dev = torch.device("cuda:0")
    torch.manual_seed(2024)                                   # the inference512 workload's generator (bench_workloads.py)
    G = ResFFT_Generator(1, 32, 10, 3, 1).to(dev).eval()
    G.allow_any_size = True
    base = None
    lines = []
    for s in a.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        x, _ = synthetic_ldct(a.slices, seed=1234, size=max(H, W))
        x = x[:, :, :H, :W].contiguous().to(dev)
        with torch.no_grad():
            for _ in range(a.warmup):
                G(x)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                G(x)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
        ms = statistics.median(ts)
        ns_px = ms * 1e6 / (a.slices * H * W)
        if (H, W) == (512, 512):
            base = ns_px
        rec = {"H": H, "W": W, "slices": a.slices, "ms": round(ms, 3), "ms_min": round(min(ts), 3), "ns_per_pixel": round(ns_px, 4),
               "vs_512_per_pixel": round(ns_px / base, 3) if base else None}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
