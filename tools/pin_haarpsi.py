"""Golden data for HaarPSI (tests/test_haarpsi_{cpu,gpu}.py).  TEST INFRASTRUCTURE: needs the reference checkout that
oracle/_refboot.py points at; it is not needed to run the tests.

    python tools/pin_haarpsi.py

Writes tests/golden/haarpsi_piq.npz: for every case of tests/_haarpsi_ref.CASES and each of (input, target, pred) against the
target, what the reference's module/piq/haarpsi.py itself computes on the seeded inputs of _haarpsi_ref.case_inputs (regenerated
by the tests, not stored; their CRC-32 is): the per-image scores once in float32 -- the public function as the reference's users
call it -- and once in float64, and in both the four part sums, read off the reference while it runs: a stand-in for the name
`torch` in its module keeps the weights (the result of its torch.max) and the similarity map (the result of its last
torch.cat), and the sums per orientation are taken from those two tensors with the reference's own expression.  `meta` holds
the largest relative distance float32 -> float64 of the reference's own scores and of its own part sums: the bounds of
tests/test_haarpsi_gpu.py.

Asserted, so that a fixture which breaks it cannot be written: den > 1 on every row (eps cannot matter), and the part sums add
up to the sums the reference itself takes."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refboot  # noqa: E402
import _haarpsi_ref as R  # noqa: E402


class TorchSpy:
    """Stands in for the name `torch` in the reference's haarpsi module: everything is torch's; the result of max (the weights),
    of the last cat (the similarity map) and of sum over dim=[1, 2, 3] (the denominator) are kept."""

    def __init__(self):
        self.weights = self.sim = self.den = None

    def __getattr__(self, name):
        return getattr(torch, name)

    def max(self, *args, **kw):
        self.weights = torch.max(*args, **kw)
        return self.weights

    def cat(self, *args, **kw):
        self.sim = torch.cat(*args, **kw)
        return self.sim

    def sum(self, x, *args, **kw):
        out = torch.sum(x, *args, **kw)
        if "dim" in kw:
            self.den = out.detach().clone()
        return out


def load_reference():
    _refboot.boot()
    sys.modules["module.piq"].__path__ = [os.path.join(_refboot.REF, "module", "piq")]
    import module.piq.haarpsi as haarpsi
    return haarpsi


def run(mod, a, b, dtype, subsample, c, alpha):
    spy = TorchSpy()
    mod.torch = spy
    try:
        score = mod.haarpsi(a.to(dtype), b.to(dtype), reduction="none", data_range=1.0, subsample=subsample, c=c, alpha=alpha)
    finally:
        mod.torch = torch
    w, sim = spy.weights, spy.sim
    assert score.dtype == dtype and w.dtype == dtype and w.shape == sim.shape and w.shape[1] == 2
    weighted = (sim * alpha).sigmoid() * w                                  # the reference's expression, per orientation here
    num, den = weighted.sum(dim=[2, 3]), w.sum(dim=[2, 3])
    assert torch.allclose(den.sum(dim=1), spy.den, rtol=1e-5 if dtype == torch.float32 else 1e-13, atol=0)
    return score.flatten(), torch.stack([num[:, 0], den[:, 0], num[:, 1], den[:, 1]], dim=1)


def _spread(v32, v64):
    v32, v64 = v32.double(), v64.double()
    return float(((v32 - v64).abs() / v64.abs().clamp_min(1e-300))[v64 != 0].max())


def main():
    torch.set_num_threads(8)
    mod = load_reference()
    arrays = {}
    spread = {"score": 0.0, "parts": 0.0}
    for index, (B, H, W, subsample, c, alpha) in enumerate(R.CASES):
        x, y, pred = R.case_inputs(index)
        arrays[f"crc_{index}"] = np.array(R.crc(x, y, pred), dtype=np.int64)
        got = {}
        for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
            per_source = [run(mod, src, y, dtype, subsample, c, alpha) for src in (x, y, pred)]
            got[tag] = (torch.stack([s for s, _ in per_source]), torch.stack([p for _, p in per_source]))       # (3, B), (3, B, 4)
            arrays[f"score{tag}_{index}"] = got[tag][0].numpy()
            arrays[f"parts{tag}_{index}"] = got[tag][1].numpy()
        assert (got["64"][1][..., 1::2] > 1).all() and (got["32"][1][..., 1::2] > 1).all(), (index, got["64"][1])
        d = (_spread(got["32"][0], got["64"][0]), _spread(got["32"][1], got["64"][1]))
        spread["score"], spread["parts"] = max(spread["score"], d[0]), max(spread["parts"], d[1])
        print(f"  case {index} {B}x{H}x{W} subsample={subsample} c={c} alpha={alpha}: float64 {got['64'][0].tolist()} "
              f"largest float32 distance score {d[0]:.3e} parts {d[1]:.3e} smallest den {float(got['64'][1][..., 1::2].min()):.4g}")
    meta = dict(recipe="tests/_haarpsi_ref.case_inputs", cases=[list(cs) for cs in R.CASES], spread=spread)
    print("  largest relative distance float32 -> float64 of the reference's own values:", spread)
    np.savez_compressed(R.GOLDEN, meta=np.array(json.dumps(meta)), **arrays)
    print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
