"""Time of the perceptual metrics' device work on whole slices: the VGG-19 feature stack on the stacked (input,
target, prediction) images of 1 and 8 slices, and the per-patch Gram-matrix launch (mtd_patch_gram_l1) of each of the five
levels.  One JSON line per item: median ms per call over --repeats timed groups of --inner calls enqueued back to back, each
group bracketed by device synchronisation on the host clock (so the figure is the rate at which the calls complete in stream
order: it contains what the host and the launches cost whenever those, not the kernel, set the pace -- a call rate, not a kernel
trace), the executed flop count (the conv helpers' own count, Winograd savings taken off; 2 * patches * 256 * C^2 per Gram
matrix over the tile pairs the kernel computes, two matrices per launch) and the TFLOP/s they give, beside the 157.3 TFLOP/s
fp32-MFMA peak.

    python tools/perceptual_metrics_timing.py [--repeats 15] [--inner 20] [--warmup 3] [--size 512] [--slices 1,8] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TFLOPS = 157.3


def seeded_vgg19_state(torch, seed=0):
    """He-normal stand-in for the torchvision checkpoint (timing does not depend on the values)."""
    from mtd_gan_amd.metrics import _VGG19_CONVS
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, cin, cout in _VGG19_CONVS:
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"features.{idx}.bias"] = torch.randn(cout, generator=g) * 0.05
    return sd


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
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20, help="calls enqueued back to back per timed group")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--slices", default="1,8")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import kernels as K, metrics as M
    from mtd_gan_amd.data import synthetic_ldct
    dev = torch.device("cuda:0")
    vgg = M.VGG19Features(seeded_vgg19_state(torch))
    lines = []

    def emit(rec, ts, flops):
        v = sorted(ts)
        med = statistics.median(v)
        rec.update(S=a.size, repeats=a.repeats, inner=a.inner, ms=round(med, 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4),
                   gflop=round(flops / 1e9, 3), tflops=round(flops / med / 1e9, 2), of_fp32_mfma_peak=round(flops / med / 1e9 / PEAK_TFLOPS, 4))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    with torch.no_grad():
        for n in (int(s) for s in a.slices.split(",")):
            x, y = synthetic_ldct(n, seed=1234, size=a.size)
            stacked = torch.cat([y, x, (0.5 * (x + y))]).to(dev)
            K.FLOP_COUNT = {}
            maps = vgg(stacked)
            torch.cuda.synchronize()
            counted, K.FLOP_COUNT = K.FLOP_COUNT, None
            flops = sum(v for k, v in counted.items() if k in ("conv_mfma", "conv_valu"))
            emit({"item": "vgg19_stack", "slices": n, "images": 3 * n}, timed(torch, lambda: vgg(stacked), a.warmup, a.repeats, a.inner), flops)
            for lvl, m in enumerate(maps):
                B, h, w, Cc = m.shape
                fx, fy = m[n:2 * n], m[:n]
                nt = Cc // 64
                flops = 2.0 * 2 * n * (h // 16) * (w // 16) * 256 * 64 * 64 * (nt * (nt + 1) // 2)
                out = torch.empty(1, dtype=torch.float64, device=dev)
                emit({"item": f"patch_gram_l1_level{lvl + 1}", "slices": n, "map": [n, h, w, Cc]},
                     timed(torch, lambda: M.patch_gram_l1(fx, fy, out=out), a.warmup, a.repeats, a.inner), flops)
            del maps
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
