"""Sliding-window inference of 8 slices of 512 x 512 with the generator on 64 x 64 windows (inferers.sliding_window_inference,
DESIGN 3.6) at overlap 0.3 / 0.5 / 0.9 and sw_batch_size 32 / 256, next to whole-slice inference in the same process, and
next to the same loop written in torch ops (slicing, torch.stack, `acc[..., y:y+rh, x:x+rw] += m * pred`).

The figure this tool is for is the share of a call spent OUTSIDE the predictor.  Per setting, three things are timed in turn,
repeat by repeat, so that all see the same clocks and neighbours (host clock around work that ends in a device synchronise):
    hip     the whole call with the device gather / blend / finish;
    torch   the whole call with the torch-ops loop (its weight-sum map is computed once, outside the timed region: the loop
            pays for window slicing, stacking and the accumulation only);
    pred    the predictor alone on the same chunk sizes, from a buffer that is already there.
outside = 1 - pred / whole call, from the medians.

    python tools/sliding_window_timing.py [--overlaps 0.3,0.5,0.9] [--batches 32,256] [--repeats 5] [--warmup 1] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--overlaps", default="0.3,0.5,0.9")
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--mode", default="gaussian", choices=["constant", "gaussian"])
    ap.add_argument("--out", default=None, help="also append the table to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd.arch.Ours.networks import ResFFT_Generator
    from mtd_gan_amd.data import synthetic_ldct
    from mtd_gan_amd.inferers import importance_map, sliding_window_inference, window_starts
    if not torch.cuda.is_available():
        raise SystemExit("sliding_window_timing.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.manual_seed(2024)                                   # the inference512 workload's generator (bench_workloads.py)
    G = ResFFT_Generator(1, 32, 10, 3, 1).to(dev).eval()
    roi = (64, 64)
    x, _ = synthetic_ldct(a.slices, seed=1234, size=a.size)
    x = x.to(dev)
    imap = importance_map(roi, a.mode, 0.125).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def plan(overlap):
        ys, xs = window_starts(a.size, roi[0], overlap), window_starts(a.size, roi[1], overlap)
        return [(b, y, xx) for b in range(a.slices) for y in ys for xx in xs]

    def weight_sum(wins):
        ws = torch.zeros(1, 1, a.size, a.size, device=dev)
        for b, y, xx in wins:
            if b == 0:
                ws[..., y:y + roi[0], xx:xx + roi[1]] += imap
        return ws

    def torch_loop(wins, sb, ws):
        acc = torch.zeros_like(x)
        for i in range(0, len(wins), sb):
            chunk = wins[i:i + sb]
            w = torch.stack([x[b, :, y:y + roi[0], xx:xx + roi[1]] for b, y, xx in chunk])
            p = G(w)
            for j, (b, y, xx) in enumerate(chunk):
                acc[b, :, y:y + roi[0], xx:xx + roi[1]] += imap * p[j]
        return acc / ws

    def predictor_only(n_windows, sb, buf):
        for i in range(0, n_windows, sb):
            G(buf[:min(sb, n_windows - i)])

    lines = [f"# {a.slices} slices of {a.size} x {a.size}, roi 64 x 64, mode {a.mode}; ms per call, median of {a.repeats} "
             f"(min-max); outside = 1 - pred / call"]
    with torch.no_grad():
        for _ in range(a.warmup + 1):
            G(x)
        whole = sorted(timed(lambda: G(x))[0] for _ in range(max(a.repeats, 5)))
        lines.append(f"whole-slice G(x): {statistics.median(whole):.2f} ms ({whole[0]:.2f}-{whole[-1]:.2f})")
        lines.append("overlap  sw_batch  windows  chunks |    hip ms (min-max)       outside |  torch ms (min-max)       outside |"
                     "   pred ms | hip/whole | max|hip-torch|")
        print("\n".join(lines), flush=True)
        for ov in (float(v) for v in a.overlaps.split(",")):
            wins = plan(ov)
            ws = weight_sum(wins)
            for sb in (int(v) for v in a.batches.split(",")):
                buf = torch.stack([x[b, :, y:y + 64, xx:xx + 64] for b, y, xx in wins[:sb]])
                runs = {"hip": lambda: sliding_window_inference(x, roi, sb, G, overlap=ov, mode=a.mode),
                        "torch": lambda: torch_loop(wins, sb, ws),
                        "pred": lambda: predictor_only(len(wins), sb, buf)}
                ts = {k: [] for k in runs}
                last = {}
                for r in range(a.warmup + a.repeats):
                    for k, fn in runs.items():
                        t, last[k] = timed(fn)
                        if r >= a.warmup:
                            ts[k].append(t)
                med = {k: statistics.median(v) for k, v in ts.items()}
                diff = (last["hip"] - last["torch"]).abs().max().item()
                span = lambda k: f"({min(ts[k]):.1f}-{max(ts[k]):.1f})"
                line = (f"{ov:7.1f}  {sb:8d}  {len(wins):7d}  {-(-len(wins) // sb):6d} | {med['hip']:9.2f} {span('hip'):>16s} "
                        f"{1 - med['pred'] / med['hip']:8.1%} | {med['torch']:9.2f} {span('torch'):>16s} {1 - med['pred'] / med['torch']:8.1%} | "
                        f"{med['pred']:9.2f} | {med['hip'] / statistics.median(whole):9.1f} | {diff:.2e}")
                print(line, flush=True)
                lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
