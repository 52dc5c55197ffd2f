"""numpy restatement of the three kernels of csrc/dicom_domain.hip (include/mtdgan_hip.h), written from their
description: stored DICOM pixel values -> Hounsfield units -> window, and back.  Integers throughout, so everything that is
compared with it is compared for equality.  tests/golden/dicom_domain.npz holds what the reference's own get_pixels_hu and
dicom_denormalize + save_dicom gave on the same inputs (tools/pin_dicom_domain.py)."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dicom_domain.npz")


def sat16(x):
    """Cast to int16 that saturates; NaN -> 0.  Equal to the plain cast wherever that one is defined."""
    x = np.asarray(x)
    return np.where(np.isnan(x), 0, np.clip(x, -32768, 32767)).astype(np.int16)


def pairs(rescale, S):
    r = np.asarray(rescale, dtype=np.float64)
    return np.broadcast_to(r.reshape(1, 2), (S, 2)) if r.size == 2 else r.reshape(S, 2)


def stored_to_hu(stored, rescale):
    """stored: (S, ...) int16 or uint16; rescale: (S, 2) or one (slope, intercept) pair."""
    stored = np.asarray(stored)
    out = np.empty(stored.shape, dtype=np.int16)
    for s, (slope, icpt) in enumerate(pairs(rescale, stored.shape[0])):
        p = stored[s].view(np.int16).copy() if stored.dtype == np.uint16 else stored[s].astype(np.int16)
        p[p == -2000] = 0
        if slope != 1:
            p = sat16(np.trunc(slope * p.astype(np.float64)))
        out[s] = (p.astype(np.int32) + int(sat16(np.trunc(icpt)))).astype(np.uint16).view(np.int16)      # 16-bit wrap-around
    return out


def window(hu, a_min=-160.0, a_max=240.0):
    a_min, a_max = np.float32(a_min), np.float32(a_max)
    v = (hu.astype(np.float32) - a_min) / (a_max - a_min)
    return np.fmin(np.fmax(v, np.float32(0)), np.float32(1))


def window_to_stored(v, rescale, a_min, a_max, clip=True, rounding="trunc", outside="clip", reference=None):
    v = np.asarray(v, dtype=np.float32)
    a_min, a_max = np.float32(a_min), np.float32(a_max)
    cast = {"trunc": np.trunc, "nearest": np.rint}[rounding]          # np.rint: ties to even
    out = np.empty(v.shape, dtype=np.int16)
    R = pairs(rescale, v.shape[0])
    for s, (slope, icpt) in enumerate(R):
        x = np.fmin(np.fmax(v[s], np.float32(0)), np.float32(1)) if clip else v[s]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            hu = (a_max - a_min) * x
            hu = hu + a_min
            t = hu - np.float32(icpt)
            q = sat16(cast(t))
            if slope != 1:
                q = sat16(cast(q.astype(np.float32) / np.float32(slope)))
        out[s] = q
    if outside == "input":
        ref = np.asarray(reference)
        words = ref.view(np.int16) if ref.dtype == np.uint16 else ref.astype(np.int16)
        h = stored_to_hu(ref, R).astype(np.float32)
        out = np.where((h < a_min) | (h > a_max), words, out)
    return out


def load():
    """-> (meta dict, the archive)"""
    z = np.load(GOLD)
    return json.loads(str(z["meta"])), z
