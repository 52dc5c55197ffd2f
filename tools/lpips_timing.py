"""Time of LPIPS and DISTS per slice on 512 x 512 slices, B = 1 and B = 8, the three image sets against the target:
metrics.lpips_each / dists_each (VGG-16 on the HIP conv kernels, the reductions of csrc/lpips.hip) beside the same metrics as torch
float32 ops on the same GPU in the same process (tests/_lpips_ref.py, the restatement of piq's classes, once per image set as a
user of piq would call them).  The network pass and the reductions are also timed apart: the reductions on maps computed
beforehand, with the bytes of the maps they read over the time.  Then the whole engine.test_MTD_GAN_Ours loop under
`model.test_per_slice` with and without the two options.  Host clock around each call with a device synchronise before and after,
one untimed warm-up call, median of --repeats calls: a rate that contains the launches and, for the loop, the device -> host
reads.  Seeded weights (the real checkpoints are the caller's).  One JSON line per item.  Not a bench line and no threshold: the
numbers are written down.

    python tools/lpips_timing.py [--repeats 5] [--size 512] [--out profiles/lpips_timing.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_timing.jsonl"), help="the JSON lines are appended to this file")
    a = ap.parse_args()
    import torch
    import mtd_gan_amd  # noqa: F401
    from mtd_gan_amd import engine, metrics as M
    from mtd_gan_amd.arch.Ours.networks import MTD_GAN_Method
    from mtd_gan_amd.data import synthetic_ldct
    import _lpips_ref as R
    import mtdgan_oracle as orc
    assert torch.cuda.is_available(), "lpips_timing needs the GPU"
    dev = torch.device("cuda:0")
    lines = []

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
        lines.append(json.dumps(dict(kw, size=a.size, repeats=a.repeats)))
        print(lines[-1], flush=True)

    sd, lw, dw = R.seeded_state_dict(), R.seeded_lpips_weights(), R.seeded_dists_weights()
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    lw_dev = [w.to(dev) for w in lw]
    dw_dev = {k: v.to(dev) for k, v in dw.items()}
    vgg = M.VGG16Features(sd)
    ltab, dtab = M.lpips_weights(lw).to(dev), M.dists_weights(dw).to(dev)

    for B in (1, 8):
        x, y = (t.to(dev) for t in synthetic_ldct(B, seed=1234, size=a.size))
        pred = (0.5 * (x + y)).contiguous()
        stacked = torch.cat([y, x, pred])
        for pool in ("max", "l2"):
            emit(item="vgg16_features", pool=pool, B=B, images=3 * B, hip=timed(lambda: vgg(stacked, pool=pool), B))

        # the reductions alone, on maps computed beforehand
        maps = vgg(stacked, pool="max")
        read = sum(3 * m[:B].numel() * 4 for m in maps)

        def lpips_reductions():
            sums = torch.zeros((3, B, 5), dtype=torch.float64, device=dev)
            c0 = 0
            for lvl, m in enumerate(maps):
                Cc = m.shape[3]
                M.lpips_level_each(m[:B], m[B:2 * B], m[2 * B:], ltab[c0:c0 + Cc], "mse", out=sums.view(-1)[lvl:], out_stride=5, other_stride=2 * B * 5)
                c0 += Cc
            return sums
        hip = timed(lpips_reductions, B)
        nchw = [m.permute(0, 3, 1, 2).contiguous() for m in maps]

        def lpips_reductions_torch():
            with torch.no_grad():
                return [[R.lpips_level(f[k * B:(k + 1) * B], f[:B], w.flatten()) for f, w in zip(nchw, lw_dev)] for k in (1, 2)]
        ops = timed(lpips_reductions_torch, B)
        emit(item="lpips_reductions", B=B, hip=hip, torch_float32_ops=ops, map_bytes_read_per_slice=read // B,
             hip_gb_per_s=round(read / B / (hip["ms_per_slice"] * 1e-3) / 1e9, 1), ratio_torch_over_hip=round(ops["ms_per_slice"] / hip["ms_per_slice"], 2))
        del nchw
        maps = [stacked.reshape(3 * B, a.size, a.size, 1)] + vgg(stacked, pool="l2")
        read = sum(3 * m[:B].numel() * 4 for m in maps)

        def dists_reductions():
            tables = [M.channel_moments_each(m[:B], m[B:2 * B], m[2 * B:]) for m in maps]
            return M.dists_finish(tables, [m.shape[1] * m.shape[2] for m in maps], dtab, self_row=1)
        hip = timed(dists_reductions, B)
        nchw = [m.permute(0, 3, 1, 2).contiguous() for m in maps]

        def dists_reductions_torch():
            with torch.no_grad():
                out = []
                for k in (1, 2):
                    tables = [R.moments(f[:B], f[k * B:(k + 1) * B]) for f in nchw]
                    out.append(R.dists_finish(tables, [f.shape[2] * f.shape[3] for f in nchw], dw_dev["alpha"], dw_dev["beta"])[0])
                return out
        ops = timed(dists_reductions_torch, B)
        emit(item="dists_reductions", B=B, hip=hip, torch_float32_ops=ops, map_bytes_read_per_slice=read // B,
             hip_gb_per_s=round(read / B / (hip["ms_per_slice"] * 1e-3) / 1e9, 1), ratio_torch_over_hip=round(ops["ms_per_slice"] / hip["ms_per_slice"], 2))
        del nchw, maps

        # the whole metrics
        for name, fn, ref in (("lpips_each", lambda: M.lpips_each(x, y, pred, vgg=vgg, weights=ltab),
                               lambda: [R.lpips(sd_dev, lw_dev, s, y, "mse", torch.float32)[0] for s in (x, y, pred)]),
                              ("dists_each", lambda: M.dists_each(x, y, pred, vgg=vgg, weights=dtab),
                               lambda: [R.dists(sd_dev, dw_dev, s, y, torch.float32)[0] for s in (x, y, pred)])):
            def torch_ops():
                with torch.no_grad():
                    return ref()
            hip, ops = timed(fn, B), timed(torch_ops, B)
            got = fn().cpu()
            want = torch.stack([s.double().cpu() for s in torch_ops()])
            emit(item=name, B=B, hip=hip, torch_float32_ops=ops, ratio_torch_over_hip=round(ops["ms_per_slice"] / hip["ms_per_slice"], 2),
                 max_abs_diff=float((got - want).abs().max()), largest_score=float(got.max()))
        del stacked
        torch.cuda.empty_cache()

    torch.manual_seed(3)
    model = MTD_GAN_Method().to(dev)
    model.Generator.load_state_dict(orc.seeded_fill(orc.g_param_shapes(), seed=7))
    model.test_per_slice = True
    model.perceptual_vgg16 = vgg
    x, y = (t.to(dev) for t in synthetic_ldct(a.slices, seed=1234, size=a.size))
    loader = [dict(n_20=x[i:i + 8], n_100=y[i:i + 8]) for i in range(0, a.slices, 8)]
    l1 = torch.nn.L1Loss()
    loop = {}
    for tag, lp, di in (("without", None, None), ("with_test_lpips", ltab, None), ("with_test_dists", None, dtab), ("with_both", ltab, dtab)):
        model.test_lpips, model.test_dists = lp, di
        loop[tag] = timed(lambda: engine.test_MTD_GAN_Ours(model, l1, loader, dev, None), a.slices)
        emit(item="test_loop_per_slice", config=tag, slices=a.slices, batch=8, **loop[tag])
    emit(item="test_loop_per_slice", added_ms_per_slice={k: round(v["ms_per_slice"] - loop["without"]["ms_per_slice"], 4) for k, v in loop.items() if k != "without"})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
