"""The discriminator step (d_loss + WeightMethods(m).backward) per task weighting at 32 patches, the methods ALTERNATING repeat by
repeat in one process so that all see the same clocks, allocator state and neighbours.  One JSON line per method: ms per D step
(median and minimum of --repeats timed steps, each bracketed by device synchronisation) and the ratio to pcgrad in the same run.

    python tools/weight_method_timing.py [--repeats 15] [--warmup 3] [--batch 32] [--methods pcgrad,ls,...] [--out FILE]

The yardstick is pcgrad's line from the commit before these methods existed (run with --methods pcgrad there).
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KW = dict(stl=dict(main_task=0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--methods", default="pcgrad,ls,scaleinvls,stl,uw,rlw,dwa,cagrad")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    from mtd_gan_amd.data import synthetic_ldct
    from mtd_gan_amd.module.weight_methods import WeightMethods
    dev = torch.device("cuda:0")
    torch.manual_seed(2024)
    random.seed(2024)
    model = MTD_GAN_Method().to(dev).train()
    D = model.Discriminator
    x, y = (t.to(dev) for t in synthetic_ldct(a.batch, seed=1234))
    names = a.methods.split(",")
    wms = {m: WeightMethods(m, n_tasks=3, device=dev, **KW.get(m, {})) for m in names}
    lists = dict(shared_parameters=list(D.shared_parameters()), task_specific_parameters=list(D.task_specific_parameters()),
                 last_shared_parameters=list(D.last_shared_parameters()))

    def step(m):
        D.zero_grad()
        losses, _ = model.d_loss(x, y)
        wms[m].backward(losses=losses, **lists)
    for _ in range(a.warmup):
        for m in names:
            step(m)
    torch.cuda.synchronize()
    ts = {m: [] for m in names}
    for _ in range(a.repeats):
        for m in names:
            t0 = time.perf_counter()
            step(m)
            torch.cuda.synchronize()
            ts[m].append((time.perf_counter() - t0) * 1e3)
    med = {m: statistics.median(v) for m, v in ts.items()}
    lines = []
    for m in names:
        v = sorted(ts[m])
        rec = {"method": m, "batch": a.batch, "repeats": a.repeats, "d_step_ms": round(med[m], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3),
               "ms_p25": round(v[len(v) // 4], 3), "ms_p75": round(v[(3 * len(v)) // 4], 3),
               "vs_pcgrad": round(med[m] / med["pcgrad"], 4) if "pcgrad" in med else None}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
