"""Float64 restatement of the reference's multi-output sliding-window loop (module/sliding_window.py:25-126,
sliding_window_inference_three_output, and its four siblings), written out here and not taken from the package: the window
plan, the importance map, the chunk loop with `if window_data.sum(): cls_list.append(cls_prob)`, the weighted sums and the
division.  Shared by test_sw_multi_cpu.py (against the reference's own functions and the committed fixture) and
test_sw_multi_gpu.py (against the device)."""
import math
import os

import numpy as np
import torch

U = 2.0 ** -24
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_multi_cases.npz")

# name -> (shape, roi, overlap, sw_batch_size, modes, input kind); the fixture holds, per case, the input and the fp32 outputs
# of the reference's three_output under toy_predictor ("empty": cls only, for sw_batch_size 3 and 4, image 1 all zero)
FIXTURE_CASES = {
    "odd_roi": ((1, 1, 41, 47), (30, 30), 0.5, 3, ("constant", "gaussian"), "signed"),       # rw % 4 != 0: the scalar gather path
    "empty": ((2, 1, 80, 99), (64, 64), 0.3, 3, ("constant",), "empty"),
}


def case_input(shape, kind, seed):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(seed))
    if kind == "signed":
        return x - 0.25
    x[1:] = 0.0           # "empty": values >= 0, every image but the first all zero
    return x


def toy_predictor(w):
    """(cls, seg, rec) of a chunk in exact elementwise arithmetic (one rounding per operation, the same on the CPU and on the
    device); the flips make a wrong window offset visible, and cls reads two fixed pixels of its window."""
    return 3 * w[:, :, 0, 0] + w[:, :, 5, 7], 2 * w + w.flip(-1), w.flip(-2) - 0.5 * w


class Recorder:
    """Wraps a predictor and keeps every chunk's outputs as the device produced them (as test_sliding_window_gpu._Recorder)."""

    def __init__(self, fn):
        self.fn, self.chunks = fn, []

    def __call__(self, w):
        out = self.fn(w)
        self.chunks.append(tuple(o.detach().cpu() for o in (out if isinstance(out, (tuple, list)) else (out,))))
        return out

    def predictions(self, names):
        return {n: torch.cat([c[i] for c in self.chunks]) for i, n in enumerate(names)}


def starts(size, roi, overlap):
    iv = roi if size == roi else (int(roi * (1 - overlap)) or 1)
    n = math.ceil((size - roi) / iv) + 1
    return [min(d * iv, size - roi) for d in range(n)]


def map64(roi, mode, sigma_scale=0.125):
    if mode == "constant":
        return torch.ones(roi, dtype=torch.float64)
    axes = []
    for n in roi:
        t = torch.arange(n, dtype=torch.float64) - (n - 1) / 2.0
        axes.append(torch.exp(-t * t / (2.0 * (n * sigma_scale) ** 2)))
    m = torch.outer(axes[0], axes[1])
    return m.clamp(min=max(m[m != 0].min().item(), 1e-3))


def restate(x, roi, sw_batch_size, overlap, mode, names=("cls", "seg", "rec"), predictor=toy_predictor, recorded=None):
    """The reference's loop over x (CPU fp32 (B, 1, H, W)) in float64.  The predictor runs on each fp32 chunk, or, with
    `recorded` (name -> all windows' outputs in plan order), the recorded outputs stand in for it.  Returns a dict:
    every map name -> float64 (B, 1, H, W); "cls" -> what the reference returns, the (kept, 1) concatenation over the chunks
    with a nonzero sum; "scores" -> every window's score (total,); "cls_map" -> the scores blended as window scalars;
    "kept" -> the kept windows' indices; "k" -> most windows on one pixel; "maxabs" -> name -> max |prediction|."""
    B, _, H, W = x.shape
    ys, xs = starts(H, roi[0], overlap), starts(W, roi[1], overlap)
    plan = [(b, y, xx) for b in range(B) for y in ys for xx in xs]
    m = map64(roi, mode)
    planes = [n for n in names if n != "cls"] + (["cls_map"] if "cls" in names else [])
    num = {n: torch.zeros(B, 1, H, W, dtype=torch.float64) for n in planes}
    den = torch.zeros(B, 1, H, W, dtype=torch.float64)
    cnt = torch.zeros(H, W)
    maxabs = {n: 0.0 for n in planes}
    cls_list, scores, kept = [], [], []
    for g in range(0, len(plan), sw_batch_size):
        chunk = plan[g:g + sw_batch_size]
        window_data = torch.cat([x[b:b + 1, :, y:y + roi[0], xx:xx + roi[1]] for b, y, xx in chunk])
        if recorded is None:
            out = predictor(window_data)
            out = dict(zip(names, out if isinstance(out, (tuple, list)) else (out,)))
        else:
            out = {n: recorded[n][g:g + len(chunk)] for n in names}
        if "cls" in names:
            cls = out["cls"].reshape(len(chunk), 1)
            scores.append(cls.reshape(-1))
            if window_data.sum():
                cls_list.append(cls)
                kept.extend(range(g, g + len(chunk)))
        for j, (b, y, xx) in enumerate(chunk):
            where = (b, 0, slice(y, y + roi[0]), slice(xx, xx + roi[1]))
            for n in planes:
                p = out["cls"].reshape(-1)[j].double() * torch.ones(roi, dtype=torch.float64) if n == "cls_map" else out[n][j, 0].double()
                num[n][where] += m * p
                maxabs[n] = max(maxabs[n], p.abs().max().item())
            den[where] += m
            if b == 0:
                cnt[y:y + roi[0], xx:xx + roi[1]] += 1
    res = {n: num[n] / den for n in planes}
    if "cls" in names:
        res["cls"] = torch.cat(cls_list) if cls_list else torch.zeros(0, 1)
        res["scores"] = torch.cat(scores)
    res.update(kept=kept, k=int(cnt.max().item()), maxabs=maxabs, counts=(len(ys), len(xs)))
    return res


def bound(k, maxabs):
    """Of an fp32 blend against the float64 one: 2 (k + 2) u max|pred| (test_sliding_window_gpu.test_blend_against_float64)."""
    return 2 * (k + 2) * U * maxabs


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}
