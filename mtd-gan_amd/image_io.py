"""The test loop's slice images (reference engine.py:157-159: three `plt.imsave(..., cmap="gray")` per slice).
The device turns float32 slices into PNG scanlines (`gray_png_rows`, include/mtdgan_hip.h: mtd_gray_png_rows), the bytes cross to
the host once, and zlib -- which releases the GIL -- compresses them on a small pool of threads beside the loop (`PngWriter`).
The files are 8- or 16-bit GREYSCALE PNGs (colour type 0), a deliberate deviation from imsave, which writes RGBA with
R = G = B and A = 255: the same grey levels in a quarter of the bytes.  Standard library and numpy only on the host side; no
CPU fallback for the quantisation."""
import os
import struct
import threading
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _options
from . import kernels as K

# matplotlib's gray colormap after its bytes=True conversion, (lut * 255).astype(uint8): NOT the identity -- 24 entries are one
# below their index (33, 37, 41, ...), since k / 255 * 255 falls just short of k there.
GRAY_LUT = (np.linspace(0, 1, 256) * 255).astype(np.uint8)
_lut_on = {}


def _device_lut(device):
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    t = _lut_on.get(key)
    if t is None:
        t = _lut_on[key] = torch.from_numpy(GRAY_LUT.copy()).to(device)
    return t


def row_bytes(W, depth):
    """Bytes of one scanline: the filter byte and W samples."""
    return 1 + W * depth // 8


def gray_png_rows(images, depth=8):
    """images: (n, H, W) float32 CUDA tensor.  Returns the (n, H, 1 + W * depth / 8) uint8 CUDA tensor of PNG scanlines, byte 0 of
    every row the filter type 0.  depth 8 stretches every image over its own finite limits as imsave(cmap="gray") does
    (non-finite pixels: 0; a constant image: level 0); depth 16 is round-half-even(clamp(x, 0, 1) * 65535), big-endian, with no
    stretch, so a windowed value is recoverable to 1 / 65535."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise RuntimeError("gray_png_rows: HIP path needs a float32 CUDA tensor (no CPU fallback)")
    if images.dtype != torch.float32:
        raise RuntimeError(f"gray_png_rows: HIP path needs a float32 CUDA tensor, got {images.dtype}")
    if images.dim() != 3 or min(images.shape) < 1:
        raise ValueError(f"gray_png_rows: expected (n, H, W) with n, H, W >= 1, got {tuple(images.shape)}")
    if depth not in (8, 16):
        raise ValueError(f"gray_png_rows: depth must be 8 or 16, got {depth!r}")
    n, H, W = images.shape
    if n * H * row_bytes(W, depth) >= 1 << 31:
        raise ValueError("gray_png_rows: the scanlines of one call must stay below 2 GiB; pass fewer images")
    images = images.contiguous()
    out = torch.empty((n, H, row_bytes(W, depth)), dtype=torch.uint8, device=images.device)
    return K.gray_png_rows(images, depth, _device_lut(images.device) if depth == 8 else None, out)


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def encode_png(rows, H, W, depth, level=6):
    """rows: H * (1 + W * depth / 8) bytes of scanlines (anything with the buffer protocol).  Returns the PNG file: signature,
    IHDR (colour type 0, no interlace), one IDAT of zlib.compress(rows, level), IEND."""
    if depth not in (8, 16):
        raise ValueError(f"encode_png: depth must be 8 or 16, got {depth!r}")
    view = memoryview(rows).cast("B")
    if H < 1 or W < 1 or len(view) != H * row_bytes(W, depth):
        raise ValueError(f"encode_png: {len(view)} bytes are not {H} rows of 1 + {W} * {depth // 8}")
    ihdr = struct.pack(">IIBBBBB", W, H, depth, 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(view, level)) + _chunk(b"IEND", b"")


def default_threads():
    """The process's own thread budget (_options.thread_budget: OMP_NUM_THREADS and the like, at most 32), else 4: never
    os.cpu_count(), which shows the whole machine whatever share of it the process may use."""
    return _options.thread_budget(4)


class PngWriter:
    """Compresses and writes PNGs on `threads` worker threads.  `submit` hands one image over and returns at once, unless
    4 * threads images are already waiting: then it blocks until a worker is free, so that a loop faster than the writers is
    slowed to their rate instead of piling up host buffers.  `close()` joins the workers and re-raises the first error any
    of them met (an unwritable path, for instance); `waited` is the time this thread spent blocked in submit and close."""

    def __init__(self, threads=None, level=6):
        self.threads = int(threads) if threads else default_threads()
        if self.threads < 1:
            raise ValueError("PngWriter: threads must be at least 1")
        self.level = int(level)
        self.waited = 0.0
        self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="mtd-png")
        self._room = threading.BoundedSemaphore(4 * self.threads)
        self._lock = threading.Lock()
        self._error = None
        self._closed = False

    def _work(self, path, host_rows, H, W, depth):
        try:
            data = encode_png(host_rows, H, W, depth, self.level)
            with open(path, "wb") as f:
                f.write(data)
        except BaseException as e:      # kept for close()
            with self._lock:
                if self._error is None:
                    self._error = e
        finally:
            self._room.release()

    def submit(self, path, host_rows, H, W, depth):
        """host_rows: the H scanlines of one image in host memory; it must stay unchanged until close()."""
        if self._closed:
            raise RuntimeError("PngWriter.submit after close()")
        t0 = time.perf_counter()
        self._room.acquire()
        self.waited += time.perf_counter() - t0
        self._pool.submit(self._work, path, host_rows, H, W, depth)

    def close(self):
        if self._closed:
            return
        self._closed = True
        t0 = time.perf_counter()
        self._pool.shutdown(wait=True)
        self.waited += time.perf_counter() - t0
        if self._error is not None:
            raise self._error


def png_names(path_n_20=None, path_n_100=None, k=0):
    """The three file names of one slice (input, target, prediction).  With paths: the reference's stem, path.split('_')[-1]
    without its extension, plus `_gt_n_20.png`, `_gt_n_100.png` (from path_n_100) and `_pred_n_100.png` -- for `.dcm` paths
    exactly engine.py:157-159's names.  NOTE that these names drop everything before the last underscore, the patient
    directory included, so slices of different patients with the same instance number collide in one save_dir; the
    reference has the same collision and the names are kept for compatibility.  Without paths: `slice_{k}_...`, k counting
    slices as pred_results.csv does."""
    def stem(p):
        return os.path.splitext(str(p).split("_")[-1])[0]
    if path_n_20 is None:
        s20 = s100 = f"slice_{k}"
    else:
        s20 = stem(path_n_20)
        s100 = stem(path_n_100) if path_n_100 is not None else s20
    return s20 + "_gt_n_20.png", s100 + "_gt_n_100.png", s20 + "_pred_n_100.png"
