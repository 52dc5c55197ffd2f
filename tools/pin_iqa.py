"""Golden data for MS-SSIM, VIFp and GMSD (tests/test_iqa_{cpu,gpu}.py).  TEST INFRASTRUCTURE: needs the reference checkout that
oracle/_refboot.py points at; it is not needed to run the tests.

    python tools/pin_iqa.py

Writes tests/golden/iqa_piq.npz: for every case of tests/_iqa_ref.CASES and each of (input, target, pred) against the target,
what the reference's module/piq/{ssim,vif,gmsd}.py themselves compute on the seeded inputs of _iqa_ref.case_inputs (regenerated
by the tests, not stored; their CRC-32 is): the per-image scores and stage values once in float32 -- the public functions as
the reference's users call them -- and once in float64.  vif_p and gmsd keep float64 inputs as they are; multi_scale_ssim casts
to float32, so its float64 values come from ssim._multi_scale_ssim, called as the public function calls it with the cast
left out.  The stage values are read off the reference while it runs: the (SSIM mean, cs mean) pairs that _ssim_per_channel
returns per level, the per-image sums vif_p takes per scale, the mean gmsd takes of its GMS map (its variance is score^2).

Asserted, so that a fixture which breaks it cannot be written: every per-level MS-SSIM value is above 0.5 (the relu is inactive
and the powers are well conditioned) and every VIFp den is above 0."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refboot  # noqa: E402
import _iqa_ref as R  # noqa: E402


class TorchSpy:
    """Stands in for the name `torch` in one reference module: everything is torch's, and the results of sum / mean over
    dim=[1, 2, 3] are also appended to `log`."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _logged(self, fn, x, *args, **kw):
        out = fn(x, *args, **kw)
        if "dim" in kw:
            self.log.append(out.detach().flatten().clone())
        return out

    def sum(self, x, *args, **kw):
        return self._logged(torch.sum, x, *args, **kw)

    def mean(self, x, *args, **kw):
        return self._logged(torch.mean, x, *args, **kw)


def load_reference():
    _refboot.boot()
    sys.modules["module.piq"].__path__ = [os.path.join(_refboot.REF, "module", "piq")]
    import module.piq.gmsd as gmsd
    import module.piq.ssim as ssim
    import module.piq.vif as vif
    return ssim, vif, gmsd


def run_ms_ssim(ssim, a, b, dtype):
    levels = []
    real = ssim._ssim_per_channel

    def spy(*args, **kw):
        ssim_val, cs = real(*args, **kw)
        levels.extend([cs.detach().flatten().clone(), ssim_val.detach().flatten().clone()])
        return ssim_val, cs
    ssim._ssim_per_channel = spy
    try:
        if dtype == torch.float32:
            score = ssim.multi_scale_ssim(a, b, data_range=1.0, reduction="none")
        else:
            y = b.to(dtype)
            score = ssim._multi_scale_ssim(x=a.to(dtype), y=y, data_range=1.0, kernel=ssim.gaussian_filter(11, 1.5).repeat(1, 1, 1, 1).to(y),
                                           scale_weights_tensor=torch.tensor(list(R.MS_WEIGHTS)).to(y), k1=0.01, k2=0.03)
    finally:
        ssim._ssim_per_channel = real
    assert score.dtype == dtype and len(levels) == 10
    return score.flatten(), torch.stack(levels, dim=1)


def run_vif(vif, a, b, dtype):
    spy = TorchSpy()
    vif.torch = spy
    try:
        score = vif.vif_p(a.to(dtype), b.to(dtype), sigma_n_sq=2.0, data_range=1.0, reduction="none")
    finally:
        vif.torch = torch
    assert score.dtype == dtype and len(spy.log) == 8
    return score.flatten(), torch.stack(spy.log, dim=1)


def run_gmsd(gmsd, a, b, dtype):
    spy = TorchSpy()
    gmsd.torch = spy
    try:
        score = gmsd.gmsd(a.to(dtype), b.to(dtype), reduction="none", data_range=1.0)
    finally:
        gmsd.torch = torch
    assert score.dtype == dtype and len(spy.log) == 1
    score = score.flatten()
    return score, torch.stack([spy.log[0], score * score], dim=1)


def main():
    torch.set_num_threads(8)
    ssim, vif, gmsd = load_reference()
    run = {"ms_ssim": lambda *a: run_ms_ssim(ssim, *a), "vif": lambda *a: run_vif(vif, *a), "gmsd": lambda *a: run_gmsd(gmsd, *a)}
    arrays = {}
    spread = {m: 0.0 for m in R.METRICS}
    for index, (metrics, B, H, W) in enumerate(R.CASES):
        x, y, pred = R.case_inputs(index)
        arrays[f"crc_{index}"] = np.array(R.crc(x, y, pred), dtype=np.int64)
        for m in metrics:
            got = {}
            for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
                per_source = [run[m](src, y, dtype) for src in (x, y, pred)]
                got[tag] = (torch.stack([s for s, _ in per_source]), torch.stack([p for _, p in per_source]))      # (3, B), (3, B, n)
                arrays[f"{m}_{index}_score{tag}"] = got[tag][0].numpy()
                arrays[f"{m}_{index}_parts{tag}"] = got[tag][1].numpy()
            s32, s64 = got["32"][0].double(), got["64"][0]
            rel = ((s32 - s64).abs() / s64.abs().clamp_min(1e-300))[s64 != 0]
            spread[m] = max(spread[m], float(rel.max()))
            p64 = got["64"][1]
            if m == "ms_ssim":
                lv = torch.cat([p64[..., 0:8:2], p64[..., 9:10]], dim=-1)
                assert (lv > 0.5).all(), (index, lv)
            if m == "vif":
                assert (p64[..., 1::2] > 0).all(), (index, p64)
            print(f"  case {index} {m} {B}x{H}x{W}: float64 {s64.flatten().tolist()} largest float32 distance {float(rel.max()):.3e}")
    meta = dict(recipe="tests/_iqa_ref.case_inputs", cases=[[list(m), B, H, W] for m, B, H, W in R.CASES], sigma_n_sq=2.0,
                spread={m: spread[m] for m in R.METRICS})
    print("  largest relative distance float32 -> float64 of the reference's scores:", spread)
    np.savez_compressed(R.GOLDEN, meta=np.array(json.dumps(meta)), **arrays)
    print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
