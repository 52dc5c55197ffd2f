"""The two ends of an evaluation run in the units of the DICOM files (include/mtdgan_hip.h: mtd_stored_to_hu,
mtd_stored_to_window, mtd_window_to_stored).  A series enters as the stored pixel values of its files with one (RescaleSlope,
RescaleIntercept) pair per slice and leaves the same way: the reference's get_pixels_hu (create_datasets/Mayo.py:19-43) and
dicom_denormalize + save_dicom (utils.py:167-194), which it runs in numpy on the host, as elementwise HIP kernels that give the
reference's integers.  Reading and writing the files themselves stays the caller's (pydicom; `pydicom_writer` is the one helper).
CUDA tensors only, no CPU fallback; `denoise_series` alone also takes a host array, which it stages itself."""
import os

import numpy as np
import torch

from . import _lib
from . import kernels as K

A_MIN, A_MAX = -160.0, 240.0                  # the training window (create_datasets/Mayo.py:119)
HU_MIN, HU_MAX = -1024.0, 3072.0              # the reference's dicom_normalize / dicom_denormalize pair (utils.py:167)
ROUNDING = {"trunc": 0, "nearest": 1}
OUTSIDE = {"clip": 0, "input": 1}


def rescale_table(rescale, S, device):
    """(S, 2) float64 (slope, intercept) rows on `device`, from S pairs or one pair for all slices (a sequence, a numpy array
    or a tensor; a float64 CUDA tensor of the right shape is passed through)."""
    if isinstance(rescale, torch.Tensor):
        t = rescale.detach()
        if t.is_cuda and t.dtype != torch.float64:
            raise RuntimeError(f"rescale: a CUDA table must be float64 (slope, intercept) pairs, got {t.dtype}")
        t = t.to(torch.float64)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(rescale, dtype=np.float64)))
    if t.dim() == 1 and t.numel() == 2:
        t = t.reshape(1, 2).expand(S, 2)
    if t.dim() != 2 or tuple(t.shape) != (S, 2):
        raise ValueError(f"rescale: expected ({S}, 2) (slope, intercept) pairs or one pair, got {tuple(t.shape)}")
    return t.contiguous().to(device)


def _slices(t, who, dtypes, what):
    """Checks a (S, H, W) / (S, 1, H, W) CUDA tensor; returns it contiguous with (S, H, W)."""
    if isinstance(t, torch.Tensor) and t.dtype not in dtypes:
        raise RuntimeError(f"{who}: HIP path needs a CUDA tensor of {what}, got {t.dtype}")
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: HIP path needs a CUDA tensor of {what} (no CPU fallback)")
    if not (t.dim() == 3 or (t.dim() == 4 and t.shape[1] == 1)) or min(t.shape) < 1:
        raise ValueError(f"{who}: expected (S, H, W) or (S, 1, H, W) with S, H, W >= 1, got {tuple(t.shape)}")
    S, H, W = t.shape[0], t.shape[-2], t.shape[-1]
    if S * H * W >= 1 << 31:
        raise ValueError(f"{who}: one call takes fewer than 2^31 pixels; pass fewer slices")
    return t.contiguous(), (S, H, W)


_STORED = (torch.int16, torch.uint16)


def stored_to_hu(stored, rescale):
    """stored: int16 or uint16 CUDA tensor (S, H, W) or (S, 1, H, W) of stored pixel values; rescale: see rescale_table.
    Returns get_pixels_hu's int16 Hounsfield units in the same shape -- the input of create_datasets.Mayo.window_patches and
    window_slices."""
    stored, (S, H, W) = _slices(stored, "stored_to_hu", _STORED, "int16 or uint16 stored pixel values")
    tab = rescale_table(rescale, S, stored.device)
    hu = torch.empty(stored.shape, dtype=torch.int16, device=stored.device)
    K.check(_lib.lib().mtd_stored_to_hu(stored.data_ptr(), S, H, W, tab.data_ptr(), hu.data_ptr(), K.stream_ptr()), "mtd_stored_to_hu")
    return hu


def stored_to_window(stored, rescale, a_min=A_MIN, a_max=A_MAX, return_hu=False, out=None):
    """One launch from stored pixel values to the generator's input: clip((HU - a_min) / (a_max - a_min), 0, 1) in float32, the
    bits of window_slices(stored_to_hu(stored, rescale), a_min, a_max).  return_hu: also the int16 HU, (window, hu)."""
    stored, (S, H, W) = _slices(stored, "stored_to_window", _STORED, "int16 or uint16 stored pixel values")
    if not a_max > a_min:
        raise ValueError(f"stored_to_window: a_max must exceed a_min, got {a_min!r}, {a_max!r}")
    tab = rescale_table(rescale, S, stored.device)
    if out is None:
        out = torch.empty(stored.shape, dtype=torch.float32, device=stored.device)
    hu = torch.empty(stored.shape, dtype=torch.int16, device=stored.device) if return_hu else None
    K.check(_lib.lib().mtd_stored_to_window(stored.data_ptr(), S, H, W, tab.data_ptr(), a_min, a_max, out.data_ptr(),
                                            hu.data_ptr() if return_hu else None, K.stream_ptr()), "mtd_stored_to_window")
    return (out, hu) if return_hu else out


def window_to_stored(v, rescale, a_min, a_max, *, clip=True, rounding="trunc", outside="clip", reference=None, out=None):
    """v: float32 CUDA tensor (S, H, W) or (S, 1, H, W) of windowed values.  Returns the int16 stored pixel values save_dicom
    writes for dicom_denormalize(v, a_min, a_max), in v's shape (a_min = -1024, a_max = 3072 is the reference's pair; the bounds
    are taken as float32).  clip: v is clipped to [0, 1] first.  rounding "trunc": toward zero, the reference; "nearest": ties
    to even.  outside "clip": nothing more, the reference; "input": where the HU of `reference` (the input series' stored
    values, same shape and rescale) lies outside [a_min, a_max], the input's word is written: a network fed a windowed slice
    knows nothing of air and bone, and the window bounds in their place ruin the file for a viewer.  Values beyond int16
    saturate."""
    if rounding not in ROUNDING:
        raise ValueError(f"window_to_stored: rounding must be 'trunc' or 'nearest', got {rounding!r}")
    if outside not in OUTSIDE:
        raise ValueError(f"window_to_stored: outside must be 'clip' or 'input', got {outside!r}")
    if outside == "input" and reference is None:
        raise ValueError("window_to_stored: outside='input' needs reference=, the stored pixel values of the input series")
    if not a_max > a_min:
        raise ValueError(f"window_to_stored: a_max must exceed a_min, got {a_min!r}, {a_max!r}")
    v, (S, H, W) = _slices(v, "window_to_stored", (torch.float32,), "float32 windowed values")
    ref = None
    if outside == "input":
        ref, shape = _slices(reference, "window_to_stored: reference", _STORED, "int16 or uint16 stored pixel values")
        if shape != (S, H, W):
            raise ValueError(f"window_to_stored: reference holds {shape} slices, v {(S, H, W)}")
    tab = rescale_table(rescale, S, v.device)
    if out is None:
        out = torch.empty(v.shape, dtype=torch.int16, device=v.device)
    K.check(_lib.lib().mtd_window_to_stored(v.data_ptr(), S, H, W, tab.data_ptr(), a_min, a_max, 1 if clip else 0, ROUNDING[rounding],
                                            OUTSIDE[outside], ref.data_ptr() if ref is not None else None, out.data_ptr(),
                                            K.stream_ptr()), "mtd_window_to_stored")
    return out


def _chunk(generator, stored, tab, a_min, a_max, outside, rounding, out):
    """One chunk on the current stream: stored (m, H, W) -> generator((m, 1, H, W)) -> out (m, H, W), all on the device."""
    x = stored_to_window(stored, tab, a_min, a_max)
    pred = generator(x[:, None])
    if pred.shape != x[:, None].shape:
        raise ValueError(f"denoise_series: the generator returned {tuple(pred.shape)} for {tuple(x[:, None].shape)}")
    window_to_stored(pred.float(), tab, a_min, a_max, clip=True, rounding=rounding, outside=outside, reference=stored, out=out)


def denoise_series(generator, stored, rescale, *, a_min, a_max, batch=8, outside="input", rounding="trunc", out=None, pipelined=False):
    """A whole series, stored pixel values in and stored pixel values out.  stored: int16 or uint16 (S, H, W) or (S, 1, H, W), a
    CUDA tensor or a host array (numpy or CPU tensor); rescale: see rescale_table.  Chunks of `batch` slices go through
    stored_to_window, generator(x) under torch.no_grad() -- in whatever mode its attributes select (allow_any_size,
    activation_dtype, sliding_window) -- and window_to_stored(clip=True, outside=, rounding=, reference=the chunk).  Returns int16
    in the shape of `stored` where `stored` lives (numpy for numpy), or `out` (int16, that shape, on that side) when given.
    A host series is copied chunk by chunk with plain copies on the current stream.  pipelined=True stages it through two pinned
    buffers each way instead: chunk c + 1 is copied to the device on a second stream while the generator runs on chunk c, and
    results return on a third; the streams are ordered with events only, the host waits on events of finished copies, never on
    the device.  Same integers either way; measured on 64 slices of 512 x 512 the two take the same time (2.57 against 2.58 ms
    per slice, inside their spread, 5 % above the generator alone either way), so the simpler one is the default.  A device series needs no staging and runs on the current stream either way."""
    if rounding not in ROUNDING or outside not in OUTSIDE:
        raise ValueError(f"denoise_series: rounding 'trunc' | 'nearest' and outside 'clip' | 'input', got {rounding!r}, {outside!r}")
    if not a_max > a_min:
        raise ValueError(f"denoise_series: a_max must exceed a_min, got {a_min!r}, {a_max!r}")
    if int(batch) < 1:
        raise ValueError(f"denoise_series: batch must be at least 1, got {batch!r}")
    batch = int(batch)
    as_numpy = isinstance(stored, np.ndarray)
    src = torch.from_numpy(np.ascontiguousarray(stored)) if as_numpy else stored
    if not isinstance(src, torch.Tensor) or src.dtype not in _STORED:
        raise RuntimeError(f"denoise_series: stored must hold int16 or uint16 stored pixel values, got {getattr(src, 'dtype', type(src))}")
    if not (src.dim() == 3 or (src.dim() == 4 and src.shape[1] == 1)) or min(src.shape) < 1:
        raise ValueError(f"denoise_series: expected (S, H, W) or (S, 1, H, W) with S, H, W >= 1, got {tuple(src.shape)}")
    S, H, W = src.shape[0], src.shape[-2], src.shape[-1]
    flat = src.contiguous().reshape(S, H, W)
    if out is None:
        res = torch.empty((S, H, W), dtype=torch.int16, device=src.device)
    else:
        o = torch.from_numpy(out) if isinstance(out, np.ndarray) else out
        if not isinstance(o, torch.Tensor) or o.dtype != torch.int16 or o.shape != src.shape or o.device != src.device or not o.is_contiguous():
            raise ValueError("denoise_series: out must be contiguous int16 of stored's shape, on the side where stored lives")
        res = o.reshape(S, H, W)
    if not torch.cuda.is_available():
        raise RuntimeError("denoise_series: HIP path needs a GPU (no CPU fallback)")
    dev = src.device if src.is_cuda else torch.device("cuda", torch.cuda.current_device())
    chunks = [(i, min(i + batch, S)) for i in range(0, S, batch)]
    with torch.no_grad(), torch.cuda.device(dev):
        tab = rescale_table(rescale, S, dev)
        if src.is_cuda:
            for i0, i1 in chunks:
                _chunk(generator, flat[i0:i1], tab[i0:i1], a_min, a_max, outside, rounding, res[i0:i1])
        elif not pipelined:
            for i0, i1 in chunks:
                o = torch.empty((i1 - i0, H, W), dtype=torch.int16, device=dev)
                _chunk(generator, flat[i0:i1].to(dev), tab[i0:i1], a_min, a_max, outside, rounding, o)
                res[i0:i1].copy_(o)
        else:
            _pipelined(generator, flat, tab, chunks, a_min, a_max, outside, rounding, res, dev)
    if out is not None:
        return out
    res = res.reshape(src.shape)
    return res.numpy() if as_numpy else res


def _pipelined(generator, flat, tab, chunks, a_min, a_max, outside, rounding, res, dev):
    """Host series, double-buffered.  Buffer c % 2 of each kind serves chunk c; what orders its reuse:
      pin_in   the host waits for chunk c - 2's upload (copied[b]) before it refills the buffer
      dev_in   the upload stream waits for chunk c - 2's kernels (used[b]: they read it as input and as reference)
      dev_out  the main stream waits for chunk c - 2's download (landed[b]) before window_to_stored rewrites it
      pin_out  the host has taken chunk c - 2's result out of it (collect) before chunk c's download is enqueued."""
    m, H, W = chunks[0][1] - chunks[0][0], flat.shape[1], flat.shape[2]
    main = torch.cuda.current_stream(dev)
    up, down = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    pin_in = [torch.empty((m, H, W), dtype=flat.dtype, pin_memory=True) for _ in range(2)]
    pin_out = [torch.empty((m, H, W), dtype=torch.int16, pin_memory=True) for _ in range(2)]
    dev_in = [torch.empty((m, H, W), dtype=flat.dtype, device=dev) for _ in range(2)]
    dev_out = [torch.empty((m, H, W), dtype=torch.int16, device=dev) for _ in range(2)]
    copied, used, ready, landed = ([torch.cuda.Event() for _ in range(2)] for _ in range(4))

    def stage(c):
        b, (i0, i1) = c % 2, chunks[c]
        if c >= 2:
            copied[b].synchronize()
        pin_in[b][:i1 - i0].copy_(flat[i0:i1])
        if c >= 2:
            up.wait_event(used[b])
        else:
            up.wait_stream(main)            # (the buffers were allocated on the main stream)
        with torch.cuda.stream(up):
            dev_in[b][:i1 - i0].copy_(pin_in[b][:i1 - i0], non_blocking=True)
            copied[b].record(up)

    def collect(c):
        b, (i0, i1) = c % 2, chunks[c]
        landed[b].synchronize()
        res[i0:i1].copy_(pin_out[b][:i1 - i0])

    stage(0)
    for c, (i0, i1) in enumerate(chunks):
        b, n = c % 2, i1 - i0
        main.wait_event(copied[b])
        if c >= 2:
            main.wait_event(landed[b])
        _chunk(generator, dev_in[b][:n], tab[i0:i1], a_min, a_max, outside, rounding, dev_out[b][:n])
        used[b].record(main)
        down.wait_event(used[b])
        with torch.cuda.stream(down):
            pin_out[b][:n].copy_(dev_out[b][:n], non_blocking=True)
            landed[b].record(down)
        if c + 1 < len(chunks):
            stage(c + 1)                    # host copy and upload of the next chunk, under this chunk's generator call
        if c >= 1:
            collect(c - 1)
    collect(len(chunks) - 1)
    main.wait_stream(up)                    # the caller's stream is ordered after everything the side streams touched
    main.wait_stream(down)


def pydicom_writer(dcm_dir):
    """A sink for `model.test_save_dcm` (engine.test_MTD_GAN_Ours) that does with the file what the reference's save_dicom does
    (utils.py:179-194): read the original, replace PixelData with the int16 array's bytes, save under the same name in dcm_dir.
    pydicom is the caller's dependency and is imported here, when the writer is made."""
    try:
        import pydicom
    except ImportError as e:
        raise RuntimeError("dicom_io.pydicom_writer needs the pydicom package, which is not installed; pass any other "
                           "callable(path_n_20, stored_int16_2d, k) as the sink to write the slices yourself") from e
    os.makedirs(dcm_dir, exist_ok=True)

    def write(path_n_20, stored, k):
        if path_n_20 is None:
            raise ValueError(f"pydicom_writer: slice {k} has no path_n_20 to read the original file from")
        dcm = pydicom.dcmread(path_n_20)
        dcm.PixelData = np.ascontiguousarray(stored, dtype=np.int16).tobytes()
        dcm.save_as(os.path.join(dcm_dir, os.path.basename(str(path_n_20))))

    return write
