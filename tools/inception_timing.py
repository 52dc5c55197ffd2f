"""Time of FID's feature network as the test loop runs it: 8 slices of 512 x 512, three image sets (input, target,
prediction) per slice, one single-channel image per call (metrics.compute_feat) -- 24 network passes.  Two lines:
metrics.InceptionV3Features on the HIP kernels, and the plain-torch restatement the tests compare with (tests/_inception_ref.py:
conv2d / batch_norm / relu, fp32, on x.repeat(1, 3, 1, 1)) on the same GPU in the same process, with the same seeded weights.
Median ms per slice (three passes) over --repeats timed loops, each bracketed by device synchronisation on the host clock (a call
rate: it contains what the host and the launches cost), and the largest difference of the two feature sets.  Not a bench line and no
threshold: both numbers are written down.

    python tools/inception_timing.py [--repeats 5] [--warmup 1] [--slices 8] [--size 512] [--out profiles/inception_timing.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inception_timing.jsonl"), help="the JSON lines are appended to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import metrics as M
    import _inception_ref as R
    assert torch.cuda.is_available(), "inception_timing needs the GPU"
    dev = torch.device("cuda:0")
    sd = R.seeded_state_dict(0)
    net = M.InceptionV3Features(sd)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    g = torch.Generator().manual_seed(8)
    sets = [torch.rand(a.slices, 1, a.size, a.size, generator=g).to(dev) for _ in range(3)]

    def hip_loop():
        return [M.compute_feat(*(s[i:i + 1] for s in sets), extractor=net) for i in range(a.slices)]

    def torch_loop():
        return [M.compute_feat(*(s[i:i + 1] for s in sets), extractor=lambda t: R.features(sd_dev, t)) for i in range(a.slices)]

    lines = []
    feats = {}
    with torch.no_grad():
        for impl, loop in (("hip", hip_loop), ("torch_f32", torch_loop)):
            for _ in range(a.warmup):
                feats[impl] = loop()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                feats[impl] = loop()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / a.slices)
            v = sorted(ts)
            lines.append(json.dumps({"item": "inception_features", "impl": impl, "slices": a.slices, "size": a.size, "passes_per_slice": 3,
                                     "repeats": a.repeats, "ms_per_slice": round(statistics.median(v), 3), "ms_min": round(v[0], 3),
                                     "ms_max": round(v[-1], 3)}))
            print(lines[-1], flush=True)
        diff = max((h - t).abs().max().item() for hs, tsl in zip(feats["hip"], feats["torch_f32"]) for h, t in zip(hs, tsl))
        scale = max(t.abs().max().item() for tsl in feats["torch_f32"] for t in tsl)
        lines.append(json.dumps({"item": "inception_features", "max_abs_diff_hip_vs_torch_f32": diff, "max_abs_feature": scale}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
