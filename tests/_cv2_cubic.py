"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the two OpenCV calls of the reference's image2tensor (RAW/dpt.py:210-214):
cv2.cvtColor(img, COLOR_BGR2RGB) and cv2.resize(img, (W, H), interpolation=INTER_CUBIC) on the float64 image that `/ 255.0` makes.

OpenCV's float path (imgproc/src/resize.cpp, resizeGeneric_ with HResizeCubic / VResizeCubic<double, double, float>):
  scale_x = 1 / ((double)W / w);  fx = (float)((dx + 0.5) * scale_x - 0.5), sx = floor(fx), fx -= sx   (the same for y)
  taps sx - 1 .. sx + 2, indices clamped to the image (fx is not reset at the border for cubic)
  fp32 coefficients of interpolateCubic (A = -0.75), float64 sums: horizontal pass first, then vertical; no clamping, no antialiasing
  dsize == the source size: a plain copy.
cv2 is not available where the tests run, so this restatement is pinned by hand-derived values (tests/test_infer_image_cpu.py), not by
cv2's own output.  The product never imports this module: the prep kernel (ada_image_prep_fwd) is compared with it on the GPU, and
tools/make_infer_image_golden.py hands it to the real reference as its cv2.resize.
"""
import numpy as np

INTER_CUBIC = 2
COLOR_BGR2RGB = 4


def cvt_color(img, code):
    """cv2.cvtColor(img, COLOR_BGR2RGB): channels reversed; a 4-channel BGRA image loses its alpha."""
    if code != COLOR_BGR2RGB:
        raise NotImplementedError(f"cvtColor code {code}")
    if img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError(f"cvtColor(BGR2RGB) needs [h, w, 3 | 4], got {img.shape}")
    return np.ascontiguousarray(img[..., 2::-1])


def cubic_coeffs(x):
    """interpolateCubic of OpenCV, in fp32 with every operation rounded on its own: x (fp32, in [0, 1)) -> [..., 4] fp32."""
    f = np.float32
    x = np.asarray(x, dtype=np.float32)
    A = f(-0.75)
    x1 = x + f(1)
    c0 = ((A * x1 - f(5) * A) * x1 + f(8) * A) * x1 - f(4) * A
    c1 = ((A + f(2)) * x - (A + f(3))) * x * x + f(1)
    y = f(1) - x
    c2 = ((A + f(2)) * y - (A + f(3))) * y * y + f(1)
    c3 = f(1) - c0 - c1 - c2
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.float32)


def taps(n_in, n_out):
    """Source indices [n_out, 4] (clamped) and fp32 coefficients [n_out, 4] of one axis."""
    scale = 1.0 / (n_out / n_in)
    fx = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = fx - sx.astype(np.float32)
    idx = np.clip(sx[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, cubic_coeffs(fx)


def resize(src, dsize, interpolation=INTER_CUBIC):
    """cv2.resize(src, dsize=(W, H), interpolation=INTER_CUBIC) for a float64 image [h, w] or [h, w, C]."""
    if interpolation != INTER_CUBIC:
        raise NotImplementedError(f"interpolation {interpolation}")
    src = np.asarray(src)
    if src.dtype != np.float64:
        raise TypeError(f"only the float64 path is restated, got {src.dtype}")
    wo, ho = int(dsize[0]), int(dsize[1])
    hi, wi = src.shape[:2]
    if (ho, wo) == (hi, wi):
        return src.copy()
    s = src if src.ndim == 3 else src[:, :, None]
    xi, xc = taps(wi, wo)
    yi, yc = taps(hi, ho)
    xc, yc = xc.astype(np.float64), yc.astype(np.float64)
    h = s[:, xi[:, 0]] * xc[None, :, 0, None]
    for j in range(1, 4):
        h = h + s[:, xi[:, j]] * xc[None, :, j, None]
    out = h[yi[:, 0]] * yc[:, 0, None, None]
    for k in range(1, 4):
        out = out + h[yi[:, k]] * yc[:, k, None, None]
    return out if src.ndim == 3 else out[:, :, 0]


def image2tensor(img_u8, H, W, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """The reference's host preparation of a uint8 BGR(A) image for an H x W network input, as fp32 [3, H, W] (RAW/dpt.py:210-214 with
    NormalizeImage + PrepareForNet, RAW/util/transform.py:124-158)."""
    rgb = cvt_color(img_u8, COLOR_BGR2RGB) / 255.0
    r = resize(rgb, (W, H))
    r = (r - np.asarray(mean)) / np.asarray(std)
    return np.ascontiguousarray(r.transpose(2, 0, 1)).astype(np.float32)
