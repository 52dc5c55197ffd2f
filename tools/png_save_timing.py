"""Time of engine.test_MTD_GAN_Ours per slice on 16 slices of 512 x 512 with and without the slice PNGs, in one
process: (off) the loop as it is without `model.test_save_png`; (on8 / on16) with it, depth 8 and depth 16 -- scanlines quantised
on the device, zlib on the writer threads; (imsave) the loop without the switch whose loader calls plt.imsave(..., cmap="gray")
on input, target and prediction of every slice right after the loop has finished with the batch, serially on the loop's thread,
which is what the reference does (engine.py:157-159; the prediction is computed beforehand, so only `.cpu()` and imsave are
added).  Two loader shapes: 16 batches of 1 on the default path and 2 batches of 8 with `model.test_per_slice`.  Pixel metrics only,
seeded generator as in the tests.  Host clock around a whole loop, files included (the writer is joined inside the loop's
function), with a device synchronise before and after; one untimed warm-up loop, median of --repeats loops.  For the `on` settings
the line also carries the time the loop's thread spent blocked on the writer (in submit when 4 x threads images are queued, and in
close) and its share of the loop.  One JSON line per setting and loader shape; no threshold: the numbers are written down.

    python tools/png_save_timing.py [--repeats 5] [--slices 16] [--batch 8] [--size 512] [--threads N] [--level 6] [--no-imsave] [--out profiles/png_save_timing.jsonl]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--threads", type=int, default=0, help="writer threads (0: image_io.default_threads())")
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--no-imsave", action="store_true", help="leave the plt.imsave setting out (145 ms per slice)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_save_timing.jsonl"), help="the JSON lines are appended to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import engine, image_io
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    from mtd_gan_amd.data import synthetic_ldct
    import mtdgan_oracle as orc
    assert torch.cuda.is_available(), "png_save_timing needs the GPU"
    assert a.slices % a.batch == 0
    try:
        if a.no_imsave:
            raise ImportError
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        plt = None
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    model = MTD_GAN_Method().to(dev)
    model.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    model.Generator.eval()
    x, y = (t.to(dev) for t in synthetic_ldct(a.slices, seed=1234, size=a.size))
    threads = a.threads or image_io.default_threads()
    writers = []
    init = image_io.PngWriter.__init__

    def recording_init(self, *args, **kw):
        init(self, *args, **kw)
        writers.append(self)
    image_io.PngWriter.__init__ = recording_init
    work = tempfile.mkdtemp(prefix="png_save_timing_")

    def batches(per_batch):
        return [dict(n_20=x[i:i + per_batch], n_100=y[i:i + per_batch], path_n_20=[f"L000_{k:04d}.dcm" for k in range(i, i + per_batch)],
                     path_n_100=[f"L000_{k:04d}.dcm" for k in range(i, i + per_batch)]) for i in range(0, a.slices, per_batch)]

    class ImsaveLoader:
        """Yields the batches; when the loop comes back for the next one, saves the three images of every slice of the last."""

        def __init__(self, ld, preds, d):
            self.ld, self.preds, self.d = ld, preds, d

        def __iter__(self):
            for b, p in zip(self.ld, self.preds):
                yield b
                for i, name in enumerate(b["path_n_20"]):
                    for t, names in ((b["n_20"], 0), (b["n_100"], 1), (p, 2)):
                        plt.imsave(os.path.join(self.d, image_io.png_names(name, name)[names]), t[i].squeeze().cpu().numpy(), cmap="gray")

    l1 = torch.nn.L1Loss()
    lines = []
    try:
        for shape, per_batch, per_slice in (("batches_of_1_default", 1, False), (f"batches_of_{a.batch}_per_slice", a.batch, True)):
            ld = batches(per_batch)
            model.test_per_slice = per_slice
            with torch.no_grad():
                preds = [model.Generator(b["n_20"]) for b in ld]
            settings = [("off", None, ld), ("on8", dict(depth=8, level=a.level, threads=threads), ld),
                        ("on16", dict(depth=16, level=a.level, threads=threads), ld)]
            if plt is not None:
                settings.append(("imsave", None, None))
            for setting, cfg, loader in settings:
                d = os.path.join(work, f"{shape}_{setting}")
                os.makedirs(d, exist_ok=True)
                if loader is None:
                    loader = ImsaveLoader(ld, preds, d)
                model.test_save_png = cfg
                ts, waits = [], []
                for rep in range(a.repeats + 1):                                           # the first loop is the untimed warm-up
                    del writers[:]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    engine.test_MTD_GAN_Ours(model, l1, loader, dev, d)
                    torch.cuda.synchronize()
                    if rep:
                        ts.append((time.perf_counter() - t0) * 1e3 / a.slices)
                        waits.append(sum(w.waited for w in writers) * 1e3 / a.slices)
                files = [f for f in os.listdir(d) if f.endswith(".png")]
                line = {"item": "png_save", "loader": shape, "setting": setting, "slices": a.slices, "size": a.size, "repeats": a.repeats,
                        "ms_per_slice": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                        "png_files": len(files), "png_bytes_per_slice": sum(os.path.getsize(os.path.join(d, f)) for f in files) // a.slices}
                if cfg is not None:
                    line.update(threads=threads, level=a.level, writer_wait_ms_per_slice=round(statistics.median(waits), 3),
                                writer_wait_share=round(statistics.median(waits) / statistics.median(ts), 3))
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
    finally:
        image_io.PngWriter.__init__ = init
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
