"""Sliding-window inference for the patch-trained models: the reference evaluates them with monai's
`sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, overlap, mode=...)` (engine.py:345, 378, 835); this is
the same call on the device.  Windows are cut out of the slices by one gather launch per chunk and the predictions are blended
back by one launch per chunk (csrc/sliding_window.hip): the host loop is gather, predictor, blend.  Semantics restate monai's
documented behaviour (monai is not a dependency; parity with monai itself is unpinned).  There is no fallback:
what the kernels do not take is refused by name."""
import math

import torch

MODES = ("constant", "gaussian")


def _pair(roi_size):
    if isinstance(roi_size, int):
        return (roi_size, roi_size)
    roi = tuple(int(r) for r in roi_size)
    if len(roi) != 2:
        raise ValueError(f"sliding_window_inference: roi_size is an int or a pair (rh, rw), got {roi_size!r}")
    return roi


def _check_overlap(overlap):
    if isinstance(overlap, (tuple, list)) or not 0.0 <= float(overlap) < 1.0:
        raise ValueError(f"sliding_window_inference: overlap is one number in [0, 1), got {overlap!r}")


def window_interval(size, roi, overlap):
    """Distance between consecutive window starts along one axis: int(roi * (1 - overlap)), at least 1; roi when the axis
    holds exactly one window."""
    _check_overlap(overlap)
    if roi < 1 or size < roi:
        raise ValueError(f"sliding_window_inference: 1 <= roi <= size along every axis, got roi {roi} on {size} "
                         "(inputs smaller than the roi are not padded here)")
    if size == roi:
        return roi
    return int(roi * (1 - overlap)) or 1


def window_starts(size, roi, overlap):
    """Window starts along one axis of length `size`: n = ceil((size - roi) / interval) + 1 windows at
    min(d * interval, size - roi) -- the last one is pulled back so that it ends at the border."""
    iv = window_interval(size, roi, overlap)
    n = -(-(size - roi) // iv) + 1
    return [min(d * iv, size - roi) for d in range(n)]


def importance_map(roi_size, mode="constant", sigma_scale=0.125):
    """(rh, rw) fp32 CPU tensor of blending weights.  "constant": ones.  "gaussian": per axis of length n,
    exp(-t^2 / (2 sigma^2)) with sigma = n * sigma_scale and t = -(n-1)/2 .. (n-1)/2, as an outer product, then clamped from
    below at max(its smallest non-zero entry, 1e-3) (so the clamped map is no longer an outer product near its corners).
    Evaluated in float64 and rounded once."""
    rh, rw = _pair(roi_size)
    if mode == "constant":
        return torch.ones(rh, rw, dtype=torch.float32)
    if mode != "gaussian":
        raise ValueError(f"sliding_window_inference: mode is one of {MODES}, got {mode!r}")
    if not sigma_scale > 0:
        raise ValueError(f"sliding_window_inference: sigma_scale > 0, got {sigma_scale!r}")
    axes = []
    for n in (rh, rw):
        t = torch.arange(n, dtype=torch.float64) - (n - 1) / 2.0
        axes.append(torch.exp(-t * t / (2.0 * (n * sigma_scale) ** 2)))
    m = torch.outer(axes[0], axes[1]).float()
    floor = max(m[m != 0].min().item(), 1e-3)
    return m.clamp_(min=floor)


_maps = {}


def _device_map(roi, mode, sigma_scale, device):
    key = (roi, mode, float(sigma_scale), device)
    m = _maps.get(key)
    if m is None:
        m = _maps[key] = importance_map(roi, mode, sigma_scale).to(device)
    return m


def _check_prediction(pred, windows):
    if not torch.is_tensor(pred) or pred.shape != windows.shape or pred.dtype != windows.dtype or pred.device != windows.device:
        got = f"{tuple(pred.shape)} {pred.dtype} on {pred.device}" if torch.is_tensor(pred) else type(pred).__name__
        raise ValueError(f"sliding_window_inference: predictor maps a {tuple(windows.shape)} {windows.dtype} chunk to a tensor of the "
                         f"same shape, dtype and device, got {got}")


@torch.no_grad()
def sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, mode="constant", sigma_scale=0.125, *,
                             clip=False):
    """predictor over every roi_size window of `inputs`, blended: out[p] = sum_w m(p - s_w) pred_w(p - s_w) / sum_w m(p - s_w)
    over the windows w (start s_w) that cover pixel p, m the importance map of `mode`.

    inputs: CUDA fp32 (B, 1, H, W).  roi_size: int or (rh, rw), rh <= H and rw <= W.  The B * ny * nx windows (images
    outermost, then rows of windows, then columns) are cut into consecutive chunks of sw_batch_size -- a chunk may span two
    images, the last may be short -- and predictor maps each (n, 1, rh, rw) chunk to an fp32 tensor of the same shape.
    overlap in [0, 1).  clip=True (keyword only, not in monai's signature) clips the result to [0, 1] in the same launch that
    divides.  Returns fp32 (B, 1, H, W); the same inputs give the same bits, whatever sw_batch_size is, as long as the
    predictor treats the windows of a chunk independently."""
    from . import kernels as K
    # what is asked for is checked before where the tensor lives, so that every refusal names its own cause
    if not torch.is_tensor(inputs) or inputs.dim() != 4:
        raise ValueError("sliding_window_inference: inputs is a (B, 1, H, W) tensor, got "
                         f"{tuple(inputs.shape) if torch.is_tensor(inputs) else type(inputs).__name__}")
    B, C, H, W = inputs.shape
    if C != 1:
        raise NotImplementedError(f"sliding_window_inference: single-channel inputs (B, 1, H, W), got {tuple(inputs.shape)}")
    if inputs.dtype != torch.float32:
        raise NotImplementedError(f"sliding_window_inference: inputs is torch.float32, got {inputs.dtype}")
    if mode not in MODES:
        raise ValueError(f"sliding_window_inference: mode is one of {MODES}, got {mode!r}")
    if not isinstance(sw_batch_size, int) or sw_batch_size < 1:
        raise ValueError(f"sliding_window_inference: sw_batch_size is a positive int, got {sw_batch_size!r}")
    if B < 1:
        raise ValueError(f"sliding_window_inference: at least one image, got {tuple(inputs.shape)}")
    roi = _pair(roi_size)
    intervals = (window_interval(H, roi[0], overlap), window_interval(W, roi[1], overlap))
    ny, nx = (math.ceil((s - r) / iv) + 1 for s, r, iv in zip((H, W), roi, intervals))
    total = B * ny * nx
    if not inputs.is_cuda:
        raise NotImplementedError(f"sliding_window_inference runs on MI355X HIP kernels only: inputs is a CUDA tensor, got one on "
                                  f"{inputs.device} (there is no CPU fallback)")
    x = inputs.detach().contiguous()
    imap = _device_map(roi, mode, sigma_scale, x.device)
    chunk = min(sw_batch_size, total)
    windows = torch.empty(chunk, 1, roi[0], roi[1], dtype=torch.float32, device=x.device)
    acc = torch.zeros(B, 1, H, W, dtype=torch.float32, device=x.device)
    for w0 in range(0, total, chunk):
        n = min(chunk, total - w0)
        K.sw_gather(x, roi, intervals, w0, n, windows)
        pred = predictor(windows[:n])
        _check_prediction(pred, windows[:n])
        K.sw_blend(pred.detach().contiguous(), imap, acc, roi, intervals, w0, n)
    return K.sw_finish(acc, imap, roi, intervals, clip=clip)
