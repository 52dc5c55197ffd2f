"""Time of FSIM per slice on 512 x 512 slices, B = 1 and B = 8: metrics.fsim_each (the HIP kernels of
csrc/fsim.hip: the three image sets against the target in one call) beside the same metric as torch float32 ops on the same GPU
in the same process (tests/_fsim_ref.py, the restatement of piq's function with torch.fft, once per image set as a user of piq
would call it), and the whole engine.test_MTD_GAN_Ours loop under `model.test_per_slice` with and without `model.test_fsim`.
Host clock around each call with a device synchronise before and after, one untimed warm-up call, median of --repeats calls: a
rate that contains the launches and, for the loop, the device -> host reads.  Every step that uses the GPU is a child process of
its own under its own time limit; a step that fails or runs out of time ends the tool, and nothing more is started.  One JSON
line per item.  Not a bench line and no threshold: the numbers are written down.

    python tools/fsim_timing.py [--repeats 5] [--size 512] [--out profiles/fsim_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
STEPS = (("each_1", 240), ("each_8", 240), ("loop", 420))          # (step, its time limit in seconds)


def step(a):
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import engine, metrics as M
    from mtd_gan_amd.data import synthetic_ldct
    import _fsim_ref as R
    assert torch.cuda.is_available(), "fsim_timing needs the GPU"
    dev = torch.device("cuda:0")

    def timed(fn, per):
        fn()                                                   # the untimed warm-up call
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / per)
        return dict(ms_per_slice=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))

    def emit(**kw):
        print("FSIM_TIMING " + json.dumps(dict(kw, size=a.size, repeats=a.repeats)), flush=True)

    if a.step.startswith("each_"):
        B = int(a.step.split("_")[1])
        x, y = (t.to(dev) for t in synthetic_ldct(B, seed=1234, size=a.size))
        pred = (0.5 * (x + y)).contiguous()
        hip = timed(lambda: M.fsim_each(x, y, pred), B)

        def torch_ops():
            with torch.no_grad():
                return [R.fsim(src, y)[0] for src in (x, y, pred)]
        ops = timed(torch_ops, B)
        got = M.fsim_each(x, y, pred).cpu()
        want = torch.stack([s.double().cpu() for s in torch_ops()])
        emit(item="fsim_each", B=B, hip=hip, torch_float32_ops=ops, ratio_torch_over_hip=round(ops["ms_per_slice"] / hip["ms_per_slice"], 2),
             max_abs_diff=float((got - want).abs().max()))
        return
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    import mtdgan_oracle as orc
    torch.manual_seed(3)
    model = MTD_GAN_Method().to(dev)
    model.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    model.test_per_slice = True
    x, y = (t.to(dev) for t in synthetic_ldct(a.slices, seed=1234, size=a.size))
    loader = [dict(n_20=x[i:i + 8], n_100=y[i:i + 8]) for i in range(0, a.slices, 8)]
    l1 = torch.nn.L1Loss()
    loop = {}
    for tag, setting in (("without_test_fsim", None), ("with_test_fsim", True)):
        model.test_fsim = setting
        loop[tag] = timed(lambda: engine.test_MTD_GAN_Ours(model, l1, loader, dev, None), a.slices)
        emit(item="test_loop_per_slice", config=tag, slices=a.slices, batch=8, **loop[tag])
    emit(item="test_loop_per_slice", added_ms_per_slice=round(loop["with_test_fsim"]["ms_per_slice"] - loop["without_test_fsim"]["ms_per_slice"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsim_timing.jsonl"), help="the JSON lines are written to this file (replacing it)")
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step is not None:
        return step(a)
    lines = []
    for name, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--repeats", str(a.repeats), "--size", str(a.size), "--slices", str(a.slices)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"fsim_timing: step {name} did not finish in {limit} s; nothing more is started")
        found = [ln[len("FSIM_TIMING "):] for ln in done.stdout.splitlines() if ln.startswith("FSIM_TIMING ")]
        print("\n".join(found), flush=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout)
            sys.exit(f"fsim_timing: step {name} ended with status {done.returncode}; nothing more is started")
        lines += found
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
