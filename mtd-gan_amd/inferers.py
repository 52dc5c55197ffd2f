"""Sliding-window inference for the patch-trained models: the reference evaluates them with monai's
`sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, overlap, mode=...)` (engine.py:345, 378, 835); this is
the same call on the device.  Windows are cut out of the slices by one gather launch per chunk and the predictions are blended
back by one launch per chunk (csrc/sliding_window.hip): the host loop is gather, predictor, blend.  Semantics restate monai's
documented behaviour (monai is not a dependency; parity with monai itself is unpinned).  There is no fallback:
what the kernels do not take is refused by name.  `sliding_window_inference_multi` is the same loop around a predictor with
several outputs (the multi-task discriminator over a whole slice, the reference's module/sliding_window.py)."""
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


def _plan(who, inputs, roi_size, sw_batch_size, overlap, mode):
    """The argument checks and the window plan shared by the public calls: (roi, intervals, (ny, nx))."""
    # what is asked for is checked before where the tensor lives, so that every refusal names its own cause
    if not torch.is_tensor(inputs) or inputs.dim() != 4:
        raise ValueError(f"{who}: inputs is a (B, 1, H, W) tensor, got "
                         f"{tuple(inputs.shape) if torch.is_tensor(inputs) else type(inputs).__name__}")
    B, C, H, W = inputs.shape
    if C != 1:
        raise NotImplementedError(f"{who}: single-channel inputs (B, 1, H, W), got {tuple(inputs.shape)}")
    if inputs.dtype != torch.float32:
        raise NotImplementedError(f"{who}: inputs is torch.float32, got {inputs.dtype}")
    if mode not in MODES:
        raise ValueError(f"{who}: mode is one of {MODES}, got {mode!r}")
    if not isinstance(sw_batch_size, int) or sw_batch_size < 1:
        raise ValueError(f"{who}: sw_batch_size is a positive int, got {sw_batch_size!r}")
    if B < 1:
        raise ValueError(f"{who}: at least one image, got {tuple(inputs.shape)}")
    roi = _pair(roi_size)
    intervals = (window_interval(H, roi[0], overlap), window_interval(W, roi[1], overlap))
    counts = tuple(math.ceil((s - r) / iv) + 1 for s, r, iv in zip((H, W), roi, intervals))
    if not inputs.is_cuda:
        raise NotImplementedError(f"{who} runs on MI355X HIP kernels only: inputs is a CUDA tensor, got one on "
                                  f"{inputs.device} (there is no CPU fallback)")
    return roi, intervals, counts


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
    roi, intervals, (ny, nx) = _plan("sliding_window_inference", inputs, roi_size, sw_batch_size, overlap, mode)
    B, _, H, W = inputs.shape
    total = B * ny * nx
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


MAX_PLANES = 4          # kernels.SW_MAX_PLANES: what one blend / finish launch takes


def _check_outputs(outputs, score_map, clip):
    """(names, blended plane names, clip flags per plane) of a sliding_window_inference_multi call, or the refusal."""
    who = "sliding_window_inference_multi"
    names = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not names or any(not isinstance(n, str) for n in names) or len(set(names)) != len(names) or "cls_map" in names:
        raise ValueError(f"{who}: outputs is a tuple of distinct names, \"cls\" for the per-window score and any other name (but "
                         f"\"cls_map\") for a map, got {outputs!r}")
    if score_map and "cls" not in names:
        raise ValueError(f"{who}: score_map=True blends the \"cls\" output, and outputs has none: {names!r}")
    planes = [n for n in names if n != "cls"] + (["cls_map"] if score_map else [])
    if len(planes) > MAX_PLANES:
        raise NotImplementedError(f"{who}: one launch blends at most {MAX_PLANES} planes (maps, and the score map), got {planes}")
    clip = (clip,) if isinstance(clip, str) else tuple(clip)
    unknown = [c for c in clip if c not in planes]
    if unknown:
        raise ValueError(f"{who}: clip names blended maps, one of {planes}, got {unknown}")
    return names, planes, [p in clip for p in planes]


def _check_predictions(pred, windows, names):
    """The predictor's answer as a list with one tensor per name, or the refusal: "cls" entries are (n, 1) or (n,), every other
    entry has the chunk's shape; all fp32 on the chunk's device."""
    who = "sliding_window_inference_multi"
    if torch.is_tensor(pred) and len(names) == 1:
        pred = (pred,)
    if not isinstance(pred, (tuple, list)) or len(pred) != len(names):
        got = f"{len(pred)} entries" if isinstance(pred, (tuple, list)) else type(pred).__name__
        raise ValueError(f"{who}: predictor returns one tensor per output name {names!r}, got {got}")
    n = windows.shape[0]
    for name, p in zip(names, pred):
        shapes = ((n, 1), (n,)) if name == "cls" else (tuple(windows.shape),)
        if not torch.is_tensor(p) or tuple(p.shape) not in shapes or p.dtype != windows.dtype or p.device != windows.device:
            got = f"{tuple(p.shape)} {p.dtype} on {p.device}" if torch.is_tensor(p) else type(p).__name__
            raise ValueError(f"{who}: predictor output {name!r} of a {tuple(windows.shape)} chunk is a {windows.dtype} tensor of shape "
                             f"{' or '.join(str(s) for s in shapes)} on {windows.device}, got {got}")
    return list(pred)


def kept_windows(flags, sw_batch_size):
    """Indices of the windows whose scores the reference keeps: those of every chunk of sw_batch_size consecutive windows that
    holds at least one nonzero window (flags: one 0 / 1 entry per window, on the host)."""
    flags = [bool(f) for f in flags]
    keep = []
    for w0 in range(0, len(flags), sw_batch_size):
        if any(flags[w0:w0 + sw_batch_size]):
            keep.extend(range(w0, min(w0 + sw_batch_size, len(flags))))
    return keep


@torch.no_grad()
def sliding_window_inference_multi(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, mode="constant", sigma_scale=0.125, *,
                                   outputs=("cls", "seg", "rec"), score_map=False, clip=(), drop_empty_chunks=False):
    """sliding_window_inference around a predictor with several outputs -- the multi-task discriminator over a whole slice, as
    the reference's module/sliding_window.py runs it.  Same plan, window order, chunking and importance map, same refusals.

    predictor(chunk) returns one tensor per name in `outputs`, in that order (a bare tensor for one name): the "cls" entry is
    (n, 1) or (n,), the score of each window; every other name is a map of the chunk's shape (n, 1, rh, rw).
    Returns a dict: every map name -> its (B, 1, H, W) blend (the names in `clip` clipped to [0, 1] in the launch that divides);
    "cls" -> (B, ny, nx), every window's score in plan order; with score_map=True also "cls_map" -> (B, 1, H, W), the scores
    blended as if each filled its window.  All maps of a chunk are blended by one launch and finished by one launch, each with
    the bits of the single-output call on that map; with only "cls" asked for nothing is blended.

    drop_empty_chunks=True is the reference's `if window_data.sum(): cls_list.append(cls_prob)`: "cls" becomes the (kept, 1)
    concatenation of the scores of the chunks that hold a nonzero window, so it depends on sw_batch_size as the reference's
    does ((0, 1) when every chunk is empty, where the reference fails in torch.concat).  The flags are written by the gather
    launch; choosing the rows costs one device-to-host read after the last chunk (the default costs none).  Difference: the
    reference tests the chunk's SUM, this tests for ANY nonzero element; the two agree whenever a chunk holds no values of
    both signs that cancel, so for slices scaled to [0, 1]."""
    from . import kernels as K
    who = "sliding_window_inference_multi"
    names, planes, clips = _check_outputs(outputs, score_map, clip)
    roi, intervals, (ny, nx) = _plan(who, inputs, roi_size, sw_batch_size, overlap, mode)
    B, _, H, W = inputs.shape
    total = B * ny * nx
    x = inputs.detach().contiguous()
    dev = x.device
    imap = _device_map(roi, mode, sigma_scale, dev) if planes else None
    chunk = min(sw_batch_size, total)
    windows = torch.empty(chunk, 1, roi[0], roi[1], dtype=torch.float32, device=dev)
    accs = [torch.zeros(B, 1, H, W, dtype=torch.float32, device=dev) for _ in planes]
    scores = torch.empty(total, dtype=torch.float32, device=dev) if "cls" in names else None
    flags = torch.empty(total, dtype=torch.uint8, device=dev) if drop_empty_chunks and scores is not None else None
    scalar = [p == "cls_map" for p in planes]
    for w0 in range(0, total, chunk):
        n = min(chunk, total - w0)
        if flags is not None:
            K.sw_gather_flags(x, roi, intervals, w0, n, windows, flags[w0:w0 + n])
        else:
            K.sw_gather(x, roi, intervals, w0, n, windows)
        pred = dict(zip(names, _check_predictions(predictor(windows[:n]), windows[:n], names)))
        if scores is not None:
            scores[w0:w0 + n].copy_(pred["cls"].detach().reshape(n))
        if planes:
            K.sw_blend_multi([scores[w0:w0 + n] if p == "cls_map" else pred[p].detach().contiguous() for p in planes], scalar, imap,
                             accs, roi, intervals, w0, n)
    if planes:
        K.sw_finish_multi(accs, imap, roi, intervals, clips)
    out = dict(zip(planes, accs))
    if flags is not None:
        keep = kept_windows(flags.cpu().tolist(), chunk)
        out["cls"] = scores[torch.tensor(keep, dtype=torch.long).to(dev)].reshape(-1, 1)
    elif scores is not None:
        out["cls"] = scores.reshape(B, ny, nx)
    return out
