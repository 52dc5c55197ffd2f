"""Time of BRISQUE and total variation per slice on 512 x 512 slices, B = 1 and B = 8: metrics.brisque_each (774
seeded support vectors) / metrics.tv_each (the HIP kernels of csrc/brisque.hip: the three image sets in one call) beside the same
statistics as torch float32 ops on the same GPU in the same process (tests/_brisque_ref.py, the restatement of piq's functions,
once per image set as a user of piq would call them), and the whole engine.test_MTD_GAN_Ours loop under `model.test_per_slice`
without either (three runs: the figure to set beside the loop before this feature), with each and with both.  Host clock around
each call with a device synchronise before and after, one untimed warm-up call, median of --repeats calls: a rate that contains
the launches and, for the loop, the device -> host reads.  Every step that uses the GPU is a child process of its own under its
own time limit; a step that fails or runs out of time ends the tool, and nothing more is started.  One JSON line per item.  Not
a bench line and no threshold: the numbers are written down.

    python tools/brisque_tv_timing.py [--repeats 5] [--size 512] [--out profiles/brisque_tv_timing.jsonl]
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
TAG = "BRISQUE_TV_TIMING "


def step(a):
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import engine, metrics as M
    from mtd_gan_amd.data import synthetic_ldct
    import _brisque_ref as R
    assert torch.cuda.is_available(), "brisque_tv_timing needs the GPU"
    dev = torch.device("cuda:0")
    coef, sv = R.seeded_svm(774, 11)
    table = M.brisque_weights((coef, sv)).to(dev)

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
        print(TAG + json.dumps(dict(kw, size=a.size, repeats=a.repeats)), flush=True)

    if a.step.startswith("each_"):
        B = int(a.step.split("_")[1])
        x, y = (t.to(dev) for t in synthetic_ldct(B, seed=1234, size=a.size))
        pred = (0.5 * (x + y)).contiguous()
        c32, s32 = coef.float().to(dev), sv.float().to(dev)
        for name, each, ref in (("brisque_each", lambda *s: M.brisque_each(*s, weights=table), lambda s: R.brisque(s, c32, s32)[0]),
                                ("tv_each", M.tv_each, R.total_variation)):
            hip = timed(lambda: each(x, y, pred), B)

            def torch_ops():
                with torch.no_grad():
                    return [ref(src) for src in (x, y, pred)]
            ops = timed(torch_ops, B)
            got = each(x, y, pred).cpu()
            want = torch.stack([s.double().cpu() for s in torch_ops()])
            emit(item=name, B=B, hip=hip, torch_float32_ops=ops, ratio_torch_over_hip=round(ops["ms_per_slice"] / hip["ms_per_slice"], 2),
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
    for tag, bq, tv in (("without", None, None), ("without_run_2", None, None), ("without_run_3", None, None), ("with_test_brisque", table, None),
                        ("with_test_tv", None, True), ("with_both", table, True)):
        model.test_brisque, model.test_tv = bq, tv
        loop[tag] = timed(lambda: engine.test_MTD_GAN_Ours(model, l1, loader, dev, None), a.slices)
        emit(item="test_loop_per_slice", config=tag, slices=a.slices, batch=8, **loop[tag])
    emit(item="test_loop_per_slice", **{f"added_ms_per_slice_{tag}": round(loop[tag]["ms_per_slice"] - loop["without"]["ms_per_slice"], 4)
                                        for tag in ("with_test_brisque", "with_test_tv", "with_both")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "brisque_tv_timing.jsonl"), help="the JSON lines are written to this file (replacing it)")
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
            sys.exit(f"brisque_tv_timing: step {name} did not finish in {limit} s; nothing more is started")
        found = [ln[len(TAG):] for ln in done.stdout.splitlines() if ln.startswith(TAG)]
        print("\n".join(found), flush=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout)
            sys.exit(f"brisque_tv_timing: step {name} ended with status {done.returncode}; nothing more is started")
        lines += found
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
