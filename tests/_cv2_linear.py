"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the OpenCV / ATen resizes of the reference's infer.py preparation:
cv2.resize(img, (W, H)) on an 8-bit image (default INTER_LINEAR, infer.py:17), cv2.resize(..., interpolation=INTER_NEAREST) (infer.py:77, 113)
and ATen's nearest rule behind torchvision Resize(NEAREST) / F.interpolate(mode="nearest") (infer.py:83-87).

OpenCV's generic 8-bit linear path (imgproc/src/resize.cpp, resizeGeneric_ with HResizeLinear / VResizeLinear<uchar, int, short>), per axis:
  scale = 1.0 / ((double)n_out / n_in);  f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s
  s < 0: s = 0, f = 0;   s >= n_in - 1: s = n_in - 1, f = 0;   second tap min(s + 1, n_in - 1)
  short coefficients on an 11-bit scale: a0 = cvRound((1.f - f) * 2048.f), a1 = cvRound(f * 2048.f)  (fp32 products, half to even)
  horizontal, int32:  h = S[x0] * a0 + S[x1] * a1
  vertical:           out = ((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2)
  exception: a source exactly twice the destination on BOTH axes is resized as INTER_AREA, the 2 x 2 mean (a + b + c + d + 2) >> 2.
cv2 is not available where the tests run, so this restatement is pinned by hand-derived values (tests/test_amodal_infer_cpu.py), not by cv2's
own output.  The product never imports this module: the kernels (ada_photo_prep_fwd, ada_mask_prep_fwd, ada_nearest_resize_fwd) are compared
with it on the GPU.
"""
import numpy as np

INTER_NEAREST = 0
INTER_LINEAR = 1


def linear_taps(n_in, n_out):
    """One axis: (first tap [n_out], second tap [n_out], a0 [n_out], a1 [n_out]) with int32 coefficients."""
    scale = 1.0 / (n_out / n_in)
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    low, high = s < 0, s >= n_in - 1
    s = np.where(low, 0, np.where(high, n_in - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int32)
    a1 = np.rint(f * np.float32(2048)).astype(np.int32)
    return s, np.minimum(s + 1, n_in - 1), a0, a1


def resize_linear_u8(src, dsize):
    """cv2.resize(src, dsize=(W, H)) for a uint8 image [h, w] or [h, w, C] (default interpolation, INTER_LINEAR)."""
    src = np.asarray(src)
    if src.dtype != np.uint8:
        raise TypeError(f"only the 8-bit path is restated, got {src.dtype}")
    wo, ho = int(dsize[0]), int(dsize[1])
    hi, wi = src.shape[:2]
    s = (src if src.ndim == 3 else src[:, :, None]).astype(np.int32)
    if wi == 2 * wo and hi == 2 * ho:
        out = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    else:
        x0, x1, ax0, ax1 = linear_taps(wi, wo)
        y0, y1, ay0, ay1 = linear_taps(hi, ho)
        h = s[:, x0] * ax0[None, :, None] + s[:, x1] * ax1[None, :, None]            # [hi, wo, C] int32
        out = (((ay0[:, None, None] * (h[y0] >> 4)) >> 16) + ((ay1[:, None, None] * (h[y1] >> 4)) >> 16) + 2) >> 2
    out = np.clip(out, 0, 255).astype(np.uint8)
    return out if src.ndim == 3 else out[:, :, 0]


def cv2_nearest_index(n_in, n_out):
    """cv2.resize(INTER_NEAREST): sx = min((int)floor(dx * ifx), n_in - 1), ifx = 1.0 / ((double)n_out / n_in)."""
    ifx = 1.0 / (n_out / n_in)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float64) * ifx).astype(np.int64), n_in - 1)


def resize_nearest(src, dsize):
    """cv2.resize(src, dsize=(W, H), interpolation=INTER_NEAREST) on [h, w] or [h, w, C] of any dtype."""
    src = np.asarray(src)
    wo, ho = int(dsize[0]), int(dsize[1])
    return src[cv2_nearest_index(src.shape[0], ho)][:, cv2_nearest_index(src.shape[1], wo)]


def aten_nearest_index(n_in, n_out):
    """ATen's nearest rule: scale = (float)n_in / n_out, src = min((int)floorf(dst * scale), n_in - 1), all fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def aten_nearest(src, ho, wo):
    """F.interpolate(mode="nearest") / torchvision Resize(NEAREST) on the two leading axes of [h, w, ...]."""
    src = np.asarray(src)
    return src[aten_nearest_index(src.shape[0], ho)][:, aten_nearest_index(src.shape[1], wo)]


def photo_inputs(img_u8, size):
    """The two network inputs of infer.py from a uint8 BGR(A) photo, channel order kept: (cv2 linear resize / 255, ATen nearest of img / 255),
    both fp32 [3, size, size]."""
    img = np.ascontiguousarray(np.asarray(img_u8)[..., :3])
    raw = resize_linear_u8(img, (size, size)).astype(np.float32) / np.float32(255)
    near = aten_nearest(img, size, size).astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(raw.transpose(2, 0, 1)), np.ascontiguousarray(near.transpose(2, 0, 1))
