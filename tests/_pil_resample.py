"""Numpy restatement of what the pseudo-label generator (reference src/scripts/sam_pl_gen_dav2.py) asks of Pillow and numpy, written from
Pillow's Resample.c / Geometry.c and independent of hip_ext/labels.py:

  * resize_bicubic_u8   Image.resize(size, Image.BICUBIC) on 8-bit pixels: ImagingResample's two integer passes
  * nearest_index / resize_nearest   Image.resize(size, Image.NEAREST)
  * cast_u16            numpy's float32 -> uint16 astype on x86-64 ("wrap") and the clamped alternative ("clip")
  * combine             lines 115-117 and 121 of the script: paste, * 65535, cast, nearest resize to the label size

test_pil_resample_cpu.py pins the first two against the installed Pillow byte for byte; the GPU tests compare the kernels with these.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _bicubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def coeffs(n_in, n_out):
    """(bounds int32 [n_out, 2] = (xmin, n), kk int32 [n_out, ksize], ksize): precompute_coeffs + normalize_coeffs_8bpc, every step in double."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        n = xmax - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, kk, ksize


def _pass(img, n_out, axis):
    """One pass along ``axis`` (0 = vertical, 1 = horizontal) of uint8 [h, w, c]: acc = 2^21 + sum k * pixel in int32, clip8(acc >> 22)."""
    bounds, kk, _ = coeffs(img.shape[axis], n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for xx in range(n_out):
        xmin, n = bounds[xx]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[xx, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31       # Pillow accumulates in int
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_bicubic_u8(img, size_hw):
    """uint8 [h, w] or [h, w, c] -> [ho, wo(, c)]: horizontal pass, rounded to uint8, then the vertical pass; an axis that keeps its size is skipped."""
    ho, wo = size_hw
    a = img[..., None] if img.ndim == 2 else img
    if a.shape[1] != wo:
        a = _pass(a, wo, 1)
    if a.shape[0] != ho:
        a = _pass(a, ho, 0)
    a = np.ascontiguousarray(a)
    return a[..., 0] if img.ndim == 2 else a


def nearest_index(n_in, n_out):
    """Source index per output index: min((int)floor((d + 0.5) * (n_in / n_out)), n_in - 1) in double."""
    s = n_in / n_out
    return np.array([min(int(math.floor((d + 0.5) * s)), n_in - 1) for d in range(n_out)], np.int64)


def resize_nearest(img, size_hw):
    ho, wo = size_hw
    return np.ascontiguousarray(img[nearest_index(img.shape[0], ho)][:, nearest_index(img.shape[1], wo)])


def cast_u16(t, overflow="wrap"):
    """float32 array -> uint16.  wrap: what ``t.astype(np.uint16)`` gives on x86-64 (cvttss2si to int32, the low 16 bits kept): NaN and
    |t| >= 2^31 give 0.  clip: truncation after clamping to [0, 65535], NaN gives 0.  Written without astype on out-of-range values."""
    t = np.asarray(t, np.float32)
    if overflow == "clip":
        safe = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(65535)))
        return np.trunc(safe).astype(np.int64).astype(np.uint16)
    assert overflow == "wrap", overflow
    ok = np.isfinite(t) & (np.abs(t) < np.float32(2.0 ** 31))
    i = np.trunc(np.where(ok, t, np.float32(0))).astype(np.int64)
    return (i & 0xFFFF).astype(np.uint16)


def combine(whole, occ, whole_mask, scale, shift, label_size=None, overflow="wrap"):
    """whole, occ fp32 [h, w]; whole_mask bool / uint8 [h, w]; scale, shift fp32 scalars.  Returns (label uint16 [ho, wo], combined fp32 [h, w],
    out_of_range int): combined = mask ? (whole * scale) + shift : occ with the product rounded to fp32 first; t = combined * 65535.f;
    the cast; the nearest gather to label_size (None: no resize).  out_of_range counts the GATHERED pixels with t outside [0, 65536) or NaN."""
    whole, occ = np.asarray(whole, np.float32), np.asarray(occ, np.float32)
    scale, shift = np.float32(scale), np.float32(shift)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (whole * scale).astype(np.float32)
        combined = np.where(np.asarray(whole_mask) != 0, (prod + shift).astype(np.float32), occ).astype(np.float32)
        t = (combined * np.float32(65535.0)).astype(np.float32)
    u16 = cast_u16(t, overflow)
    bad = ~((t >= 0) & (t < 65536))
    if label_size is not None:
        hw = (label_size, label_size) if np.isscalar(label_size) else tuple(label_size)
        u16, bad = resize_nearest(u16, hw), resize_nearest(bad, hw)
    return u16, combined, int(bad.sum())
