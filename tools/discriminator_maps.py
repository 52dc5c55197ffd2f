"""The multi-task discriminator over whole slices (inferers.sliding_window_inference_multi): synthetic slices go
through the generator window by window, the clipped result through Multi_Task_Discriminator_Skip on 64 x 64 windows, and the
pixel-level realness map (seg), the restoration (rec, clipped) and the blended image-level scores (cls_map) of every slice are
written as 8-bit PNGs through image_io (`--png-dir`).

With `--out FILE` one JSON line of timings is appended, by tools/sliding_window_timing.py's method (host clock around work that
ends in a device synchronise, an untimed warm-up, the settings timed in turn repeat by repeat, medians):
    call_ms            the whole sliding_window_inference_multi call with three outputs and the score map;
    pred_ms            the discriminator alone on the same chunk sizes, from a buffer that is already there;
    outside_share      1 - pred_ms / call_ms: the share of a call spent outside the predictor;
    blend_finish_multi_ms / blend_finish_single_ms
                       blend + finish of the recorded predictions of all chunks: one multi launch per chunk and one finish
                       for the three planes, beside three single-plane sequences (mtd_sw_blend per chunk and mtd_sw_finish,
                       the score expanded to the window's shape beforehand, outside the timed region), in the same process;
                       a timed window holds --inner such sequences back to back (one is a few tenths of a millisecond) and the
                       figure is the window over --inner;
    planes_bit_equal   whether the two gave the same bits.
No threshold is set here: the numbers are written down.

    python tools/discriminator_maps.py [--slices 4] [--size 512] [--overlap 0.5] [--sw-batch 64] [--mode gaussian]
                                       [--png-dir DIR] [--repeats 5] [--warmup 1] [--inner 50] [--out profiles/discriminator_maps_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--overlap", type=float, default=0.5)
    ap.add_argument("--sw-batch", type=int, default=64)
    ap.add_argument("--mode", default="gaussian", choices=["constant", "gaussian"])
    ap.add_argument("--png-dir", default=None, help="write <slice>_{seg,rec,cls_map}.png here")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inner", type=int, default=50, help="blend + finish sequences per timed window")
    ap.add_argument("--out", default=None, help="append the timing record (one JSON line) to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import image_io
    from mtd_gan_amd import kernels as K
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    from mtd_gan_amd.data import synthetic_ldct
    from mtd_gan_amd.inferers import _device_map, sliding_window_inference, sliding_window_inference_multi, window_interval
    import mtdgan_oracle as orc
    if not torch.cuda.is_available():
        raise SystemExit("discriminator_maps.py runs and measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    model = MTD_GAN_Method().to(dev)
    model.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    model.Discriminator.load_state_dict(orc.seeded_fill(orc.d_state_shapes(), seed=11))
    G, D = model.Generator.eval(), model.Discriminator.eval()
    roi, sb = (64, 64), a.sw_batch
    names = ("cls", "seg", "rec")
    x = synthetic_ldct(a.slices, seed=1234, size=a.size)[0].to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    with torch.no_grad():
        fake = sliding_window_inference(x, roi, sb, G, overlap=a.overlap, mode=a.mode, clip=True)
        call = lambda: sliding_window_inference_multi(fake, roi, sb, D, overlap=a.overlap, mode=a.mode, score_map=True, clip=("rec",))
        maps = call()
        if a.png_dir:
            os.makedirs(a.png_dir, exist_ok=True)
            writer = image_io.PngWriter()
            for name in ("seg", "rec", "cls_map"):
                rows = image_io.gray_png_rows(maps[name][:, 0], depth=8).cpu().numpy()
                for k in range(a.slices):
                    writer.submit(os.path.join(a.png_dir, f"slice_{k}_{name}.png"), rows[k], a.size, a.size, 8)
            writer.close()
            print(f"wrote {3 * a.slices} PNGs to {a.png_dir}", flush=True)
        if not a.out:
            return
        # ---- the timing record
        B, ny, nx = maps["cls"].shape
        total = B * ny * nx
        sizes = [min(sb, total - w0) for w0 in range(0, total, sb)]
        buf = torch.rand(min(sb, total), 1, *roi, device=dev)
        chunks = []                                                   # every chunk's recorded outputs, contiguous

        def recording(w):
            out = D(w)
            chunks.append(tuple(o.detach().contiguous() for o in out))
            return out
        sliding_window_inference_multi(fake, roi, sb, recording, overlap=a.overlap, mode=a.mode)
        expanded = [c[0].reshape(-1, 1, 1, 1).expand(-1, 1, *roi).contiguous() for c in chunks]
        scores = [c[0].reshape(-1).contiguous() for c in chunks]
        iv = (window_interval(a.size, roi[0], a.overlap), window_interval(a.size, roi[1], a.overlap))
        imap = _device_map(roi, a.mode, 0.125, dev)
        new = lambda: torch.zeros(B, 1, a.size, a.size, device=dev)

        def predictor_only():
            for n in sizes:
                D(buf[:n])

        def blend_multi():
            accs = [new(), new(), new()]
            for i, (w0, n) in enumerate(zip(range(0, total, sb), sizes)):
                K.sw_blend_multi([chunks[i][1], chunks[i][2], scores[i]], [False, False, True], imap, accs, roi, iv, w0, n)
            return K.sw_finish_multi(accs, imap, roi, iv, [False, True, False])

        def blend_single():
            outs = []
            for plane, clip in ((1, False), (2, True), (None, False)):
                acc = new()
                for i, (w0, n) in enumerate(zip(range(0, total, sb), sizes)):
                    K.sw_blend(expanded[i] if plane is None else chunks[i][plane], imap, acc, roi, iv, w0, n)
                outs.append(K.sw_finish(acc, imap, roi, iv, clip=clip))
            return outs

        def many(fn):
            def run():
                for _ in range(a.inner - 1):
                    fn()
                return fn()
            return run

        runs = {"call": call, "pred": predictor_only, "multi": many(blend_multi), "single": many(blend_single)}
        ts, last = {k: [] for k in runs}, {}
        # two rounds of alternation, so that the call and the predictor have each other as neighbours and not the much lighter
        # blend sequences (with all four in one round the call, which then follows them, read 1 ms = 3 % longer)
        for group in (("call", "pred"), ("multi", "single")):
            for r in range(a.warmup + a.repeats):
                for k in group:
                    t, last[k] = timed(runs[k])
                    if r >= a.warmup:
                        ts[k].append(t / a.inner if k in ("multi", "single") else t)
        med = {k: statistics.median(v) for k, v in ts.items()}
        equal = all(torch.equal(m, s) for m, s in zip(last["multi"], last["single"]))
        same_as_call = all(torch.equal(last["call"][n], m) for n, m in zip(("seg", "rec", "cls_map"), last["multi"]))
        rec = {"item": "discriminator_maps", "slices": a.slices, "size": a.size, "roi": list(roi), "overlap": a.overlap, "sw_batch": sb,
               "mode": a.mode, "windows": total, "chunks": len(sizes), "repeats": a.repeats, "inner": a.inner,
               "call_ms": round(med["call"], 3), "call_ms_min": round(min(ts["call"]), 3), "call_ms_max": round(max(ts["call"]), 3),
               "pred_ms": round(med["pred"], 3), "outside_share": round(1 - med["pred"] / med["call"], 4),
               "blend_finish_multi_ms": round(med["multi"], 4), "blend_finish_multi_ms_min": round(min(ts["multi"]), 4),
               "blend_finish_single_ms": round(med["single"], 4), "blend_finish_single_ms_min": round(min(ts["single"]), 4),
               "planes_bit_equal": bool(equal), "replay_equals_call": bool(same_as_call), "outputs": list(names) + ["cls_map"]}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
