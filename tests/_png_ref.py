"""numpy restatement of the two quantisation modes of mtd_gray_png_rows (include/mtdgan_hip.h) and a minimal PNG
decoder (zlib, filter 0, greyscale 8 / 16): what the PNG tests compare against.  Needs neither PIL nor matplotlib."""
import struct
import zlib

import numpy as np

LUT = (np.linspace(0, 1, 256) * 255).astype(np.uint8)      # matplotlib's gray table after its bytes=True conversion


def levels8(a, lut=LUT):
    """One (H, W) float32 image -> (H, W) uint8, as matplotlib 3.10's imsave(cmap="gray") under numpy 2 maps it:
    Normalize.__call__ subtracts vmin and divides by vmax - vmin IN PLACE with float64 scalars, so each of the two results is
    formed in float64 and rounded to float32 once, and the divisor itself is never rounded to float32; Colormap.__call__ then
    multiplies by 256 in float32, moves 256 to 255, truncates, and sends t < 0 / t >= 256 to the two ends of the table.
    Beyond matplotlib: the limits are those of the FINITE pixels, and a non-finite pixel is level 0."""
    a = np.asarray(a, dtype=np.float32)
    finite = np.isfinite(a)
    out = np.zeros(a.shape, dtype=np.uint8)
    if not finite.any():
        return out
    vmin, vmax = np.float64(a[finite].min()), np.float64(a[finite].max())
    if vmin == vmax:
        out[finite] = lut[0]
        return out
    with np.errstate(all="ignore"):
        r = (a.astype(np.float64) - vmin).astype(np.float32)
        r = (r.astype(np.float64) / (vmax - vmin)).astype(np.float32)
        t = r * np.float32(256)
        t[t == 256] = 255
        k = np.where(finite, t, 0).astype(np.int64)
    k[t < 0] = 0
    k[t >= 256] = 255
    out[finite] = lut[k[finite]]
    return out


def levels16(a):
    """(H, W) float32 -> (H, W) uint16: round-half-even(clamp(x, 0, 1) * 65535) in float32; a non-finite pixel is 0."""
    a = np.asarray(a, dtype=np.float32)
    finite = np.isfinite(a)
    v = np.rint(np.clip(np.where(finite, a, 0), np.float32(0), np.float32(1)).astype(np.float32) * np.float32(65535))
    return np.where(finite, v, 0).astype(np.uint16)


def rows(images, depth, lut=LUT):
    """(n, H, W) float32 -> (n, H, 1 + W * depth / 8) uint8 scanlines with filter byte 0, most significant byte first."""
    images = np.asarray(images, dtype=np.float32)
    n, H, W = images.shape
    out = np.zeros((n, H, 1 + W * depth // 8), dtype=np.uint8)
    for i in range(n):
        if depth == 8:
            out[i, :, 1:] = levels8(images[i], lut)
        else:
            out[i, :, 1:] = levels16(images[i]).astype(">u2").view(np.uint8).reshape(H, 2 * W)
    return out


def decode_png(data):
    """A greyscale, non-interlaced PNG whose rows all use filter 0 -> (array (H, W) uint8 | uint16, depth).  Checks the
    signature, every chunk's CRC, the chunk order and the length of the inflated data."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    pos, chunks = 8, []
    while pos < len(data):
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, tag
        chunks.append((tag, body))
        pos += 12 + length
    assert pos == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b""), [t for t, _ in chunks]
    W, H, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (colour, compression, filt, interlace) == (0, 0, 0, 0) and depth in (8, 16), chunks[0][1]
    raw = zlib.decompress(b"".join(body for tag, body in chunks if tag == b"IDAT"))
    stride = 1 + W * depth // 8
    assert len(raw) == H * stride, (len(raw), H, stride)
    lines = np.frombuffer(raw, dtype=np.uint8).reshape(H, stride)
    assert (lines[:, 0] == 0).all(), "row filter"
    if depth == 8:
        return lines[:, 1:].copy(), depth
    return lines[:, 1:].copy().view(">u2").astype(np.uint16).reshape(H, W), depth
