"""Times of the stored-pixel ends of an evaluation run on 512 x 512 slices, in one process.  Host clock around work
that ends in a device synchronise, one untimed warm-up, median of --repeats (>= 7) runs; one JSON line per item, no threshold:
the numbers are written down.
  (a) input, per slice PAIR (quarter and full dose) at 1, 8 and 64 slices:
        host    today's route: the numpy restatement of get_pixels_hu (tests/_dicom_ref.py) per slice on one host thread, the
                copy of the int16 HU to the device, window_slices
        fused   the copy of the stored words to the device and one dicom_io.stored_to_window launch per dose level
        (both also without their copy: `*_no_copy`)
  (b) dicom_io.denoise_series on 64 host slices in chunks of --batch, pipelined against pipelined=False, and the floor: the
      generator alone on the same chunks, windowed input already on the device; `outside_generator` is 1 - floor / call.
  (c) achieved bytes per second of the three kernels at 64 slices, --launches launches between two synchronises, from the bytes
      the kernel must move: stored_to_hu 4 per pixel, stored_to_window 6 (8 with the HU output), window_to_stored 6 (8 with
      outside="input").  (100 to 134 MB per launch: part of it can stay in the 256 MiB Infinity Cache between launches.)

    python tools/dicom_domain_timing.py [--repeats 7] [--size 512] [--batch 8] [--launches 20] [--out profiles/dicom_domain_timing.jsonl]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dicom_domain_timing.jsonl"), help="the JSON lines are appended to this file")
    a = ap.parse_args()
    assert a.repeats >= 7
    import numpy as np
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import dicom_io
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    from mtd_gan_amd.create_datasets import Mayo
    import _dicom_ref as D
    import mtdgan_oracle as orc
    assert torch.cuda.is_available(), "dicom_domain_timing needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    G = MTD_GAN_Method().to(dev).Generator
    G.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    G.eval()
    N = 64
    lo, hi = (t.numpy() for t in Mayo.synthetic_hu_slices(N, size=a.size, seed=11))
    pair = (1, -1024)                                                    # the Mayo files' own pair: stored = HU + 1024
    lo_w, hi_w = (lo.astype(np.int32) + 1024).astype(np.int16), (hi.astype(np.int32) + 1024).astype(np.int16)
    lines = []

    def timed(f):
        ts = []
        for rep in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if rep:
                ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    def emit(**line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    # ------------------------------------------------------------------------------------------------------------ (a)
    for n in (1, 8, 64):
        tab = dicom_io.rescale_table(pair, n, dev)
        words = [lo_w[:n], hi_w[:n]]
        on_dev = [torch.from_numpy(w).to(dev) for w in words]
        hu_dev = [torch.from_numpy(D.stored_to_hu(w, pair)).to(dev) for w in words]
        for w, h in zip(on_dev, hu_dev):
            assert torch.equal(dicom_io.stored_to_window(w, tab), Mayo.window_slices(h))

        def host(copy=True):
            for w, h in zip(words, hu_dev):
                hu = np.stack([D.stored_to_hu(w[s:s + 1], pair)[0] for s in range(n)])      # per slice, as a loader does it
                Mayo.window_slices(torch.from_numpy(hu).to(dev) if copy else h)

        def fused(copy=True):
            for w, d in zip(words, on_dev):
                dicom_io.stored_to_window(torch.from_numpy(w).to(dev) if copy else d, tab)

        def host_numpy_only():
            for w in words:
                for s in range(n):
                    D.stored_to_hu(w[s:s + 1], pair)

        for name, f in (("host", host), ("fused", fused), ("host_numpy_only", host_numpy_only), ("host_no_copy_no_numpy", lambda: [Mayo.window_slices(h) for h in hu_dev]),
                        ("fused_no_copy", lambda: fused(False))):
            med, mn, mx = timed(f)
            emit(item="dicom_input", route=name, slices=n, size=a.size, repeats=a.repeats, ms_per_slice_pair=round(med / n, 4),
                 ms_min=round(mn / n, 4), ms_max=round(mx / n, 4))

    # ------------------------------------------------------------------------------------------------------------ (b)
    kw = dict(a_min=-160.0, a_max=240.0, batch=a.batch)
    ref = dicom_io.denoise_series(G, lo_w, pair, pipelined=False, **kw)
    assert np.array_equal(dicom_io.denoise_series(G, lo_w, pair, pipelined=True, **kw), ref)
    xs = [dicom_io.stored_to_window(torch.from_numpy(lo_w[i:i + a.batch]).to(dev), pair)[:, None] for i in range(0, N, a.batch)]

    def floor():
        with torch.no_grad():
            for x in xs:
                G(x)
    res = {name: timed(f) for name, f in (("generator_only", floor), ("pipelined", lambda: dicom_io.denoise_series(G, lo_w, pair, pipelined=True, **kw)),
                                          ("unpipelined", lambda: dicom_io.denoise_series(G, lo_w, pair, pipelined=False, **kw)))}
    for name, (med, mn, mx) in res.items():
        emit(item="denoise_series", route=name, slices=N, size=a.size, batch=a.batch, repeats=a.repeats, ms_per_slice=round(med / N, 4),
             ms_min=round(mn / N, 4), ms_max=round(mx / N, 4), outside_generator=round(1.0 - res["generator_only"][0] / med, 4))

    # ------------------------------------------------------------------------------------------------------------ (c)
    tab = dicom_io.rescale_table(pair, N, dev)
    s = torch.from_numpy(lo_w).to(dev)
    v = dicom_io.stored_to_window(s, tab)
    out_f, out_i = torch.empty_like(v), torch.empty_like(s)
    px = s.numel()
    # (the library itself, on buffers made once: a launch is shorter than the checks of the public functions)
    from mtd_gan_amd import _lib, kernels as K
    L, st = _lib.lib(), K.stream_ptr()
    S_, H_, W_ = s.shape
    ps, pt, pv, pf, pi = s.data_ptr(), tab.data_ptr(), v.data_ptr(), out_f.data_ptr(), out_i.data_ptr()
    kernels = (("stored_to_hu", 4, lambda: L.mtd_stored_to_hu(ps, S_, H_, W_, pt, pi, st)),
               ("stored_to_window", 6, lambda: L.mtd_stored_to_window(ps, S_, H_, W_, pt, -160.0, 240.0, pf, None, st)),
               ("stored_to_window+hu", 8, lambda: L.mtd_stored_to_window(ps, S_, H_, W_, pt, -160.0, 240.0, pf, pi, st)),
               ("window_to_stored", 6, lambda: L.mtd_window_to_stored(pv, S_, H_, W_, pt, -160.0, 240.0, 1, 0, 0, None, pi, st)),
               ("window_to_stored+input", 8, lambda: L.mtd_window_to_stored(pv, S_, H_, W_, pt, -160.0, 240.0, 1, 0, 1, ps, pi, st)))
    assert all(f() == 0 for _, _, f in kernels)
    for name, bpp, f in kernels:
        med, mn, mx = timed(lambda: [f() for _ in range(a.launches)])
        emit(item="dicom_kernel", kernel=name, slices=N, size=a.size, launches=a.launches, repeats=a.repeats, bytes_per_pixel=bpp,
             us_per_launch=round(med * 1e3 / a.launches, 2), tb_per_s=round(px * bpp * a.launches / (med * 1e-3) / 1e12, 3),
             tb_per_s_best=round(px * bpp * a.launches / (mn * 1e-3) / 1e12, 3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
