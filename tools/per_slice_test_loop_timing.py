"""Time of engine.test_MTD_GAN_Ours per slice on 16 slices of 512 x 512, for the two ways to get per-slice rows:
(a) a loader of 16 batches of 1 on the default path -- the baseline: code as it was before `model.test_per_slice` -- and (b) a
loader of 2 batches of 8 with `model.test_per_slice = True`, in the same process, in three configurations: pixel metrics only,
+ VGG-19 (PL, TML), + VGG-19 + InceptionV3 (FID).  The generator is MTD_GAN_Method's with the seeded fill of the tests; the
feature networks are seeded as tools/perceptual_metrics_timing.py and tools/inception_timing.py build theirs.  Host clock around
a whole loop (save_dir=None) with a device synchronise before and after, one untimed warm-up loop, median of --repeats loops:
a loop rate, which contains what the host, the launches and the device -> host reads cost.  One JSON line per configuration and
loader shape with ms per slice, one with the ratio (a) / (b) and the largest difference of the two result dicts.  Not a bench
line and no threshold: the numbers are written down.

    python tools/per_slice_test_loop_timing.py [--repeats 5] [--slices 16] [--batch 8] [--size 512] [--out profiles/per_slice_test_loop_timing.jsonl]
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_slice_test_loop_timing.jsonl"), help="the JSON lines are appended to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import engine, metrics as M
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    from mtd_gan_amd.data import synthetic_ldct
    import _inception_ref as RI
    import mtdgan_oracle as orc
    from perceptual_metrics_timing import seeded_vgg19_state
    assert torch.cuda.is_available(), "per_slice_test_loop_timing needs the GPU"
    assert a.slices % a.batch == 0
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    model = MTD_GAN_Method().to(dev)
    model.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    vgg = M.VGG19Features(seeded_vgg19_state(torch))
    inception = M.InceptionV3Features(RI.seeded_state_dict(0))
    x, y = (t.to(dev) for t in synthetic_ldct(a.slices, seed=1234, size=a.size))

    def loader(per_batch):
        return [dict(n_20=x[i:i + per_batch], n_100=y[i:i + per_batch]) for i in range(0, a.slices, per_batch)]

    shapes = (("batches_of_1_default", loader(1), False), (f"batches_of_{a.batch}_per_slice", loader(a.batch), True))
    l1 = torch.nn.L1Loss()
    lines = []
    for config, use_vgg, use_fid in (("pixel", False, False), ("pixel+vgg", True, False), ("pixel+vgg+inception", True, True)):
        model.perceptual_vgg = vgg if use_vgg else None
        model.fid_features = inception if use_fid else None
        ms, results = {}, {}
        for name, ld, per_slice in shapes:
            model.test_per_slice = per_slice
            results[name] = engine.test_MTD_GAN_Ours(model, l1, ld, dev, None)            # the untimed warm-up loop
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                engine.test_MTD_GAN_Ours(model, l1, ld, dev, None)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3 / a.slices)
            ms[name] = statistics.median(ts)
            lines.append(json.dumps({"item": "test_loop", "config": config, "loader": name, "slices": a.slices, "size": a.size, "repeats": a.repeats,
                                     "ms_per_slice": round(ms[name], 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}))
            print(lines[-1], flush=True)
        (na, ra), (nb, rb) = results.items()
        assert list(ra.keys()) == list(rb.keys())
        lines.append(json.dumps({"item": "test_loop", "config": config, "ratio_default_over_per_slice": round(ms[na] / ms[nb], 3),
                                 "max_abs_diff_of_results": max(abs(ra[k] - rb[k]) for k in ra),
                                 "key_of_max_diff": max(ra, key=lambda k: abs(ra[k] - rb[k]))}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
