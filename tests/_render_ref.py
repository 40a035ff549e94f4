"""TEST INFRASTRUCTURE ONLY -- numpy restatement of ada_depth_render_fwd (include/ada_hip.h), written from its rules and not from the product's
helpers: it renders at the SOURCE size in the reference's order (normalise, colour, overlay, outline) and gathers last, as cv2.resize(INTER_NEAREST)
after the rendering does (reference infer.py:106-119); the kernel gathers first.

  source   sx = min((int)floor(dx * ifx), wi - 1), ifx = 1.0 / (wo / wi) in double; the same for y
  t        (d - lo) / span in fp32, clipped to [0, 1], NaN kept;  lo, span = fp32(vmin), fp32(float(vmax) - float(vmin))  or per image from minmax
  colour   lut[min(int(t * 256), 255)], NaN -> (0, 0, 0)
  overlay  mask == 0 and alpha != 0: uint8((1.0 - alpha) * c + alpha * 200.0) in float64, truncated
  outline  edge = inside & ~(all four neighbours inside), neighbours past the image = the border pixel; painted when an in-image edge pixel lies
           within L1 distance thickness - 1
  u16      uint16(t * 65535) in fp32, truncated, NaN -> 0; no mask, no outline
"""
import numpy as np


def nearest_index(n_in, n_out):
    inv = 1.0 / (n_out / n_in)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float64) * inv).astype(np.int64), n_in - 1)


def normalise(depth, minmax=None, vmin=0.0, vmax=1.0):
    d = np.asarray(depth, dtype=np.float32)
    if minmax is None:
        lo = np.float32(vmin)
        span = np.float32(float(vmax) - float(vmin))
    else:
        mm = np.asarray(minmax, dtype=np.float32)
        lo = mm[:, 0][:, None, None]
        span = (mm[:, 1] - mm[:, 0])[:, None, None]
    with np.errstate(all="ignore"):
        t = ((d - lo).astype(np.float32) / span).astype(np.float32)
    return np.where(t < 0, np.float32(0), np.where(t > 1, np.float32(1), t)).astype(np.float32)


def edge_map(inside):
    """[B, H, W] bool -> the pixels of the outline at thickness 1."""
    p = np.pad(inside, ((0, 0), (1, 1), (1, 1)), mode="edge")
    return inside & ~(p[:, :-2, 1:-1] & p[:, 2:, 1:-1] & p[:, 1:-1, :-2] & p[:, 1:-1, 2:])


def painted_map(inside, thickness):
    """Union of the edge map shifted by every (dv, du) with |dv| + |du| <= thickness - 1, zeros shifted in."""
    edge = edge_map(inside)
    B, H, W = edge.shape
    r = thickness - 1
    q = np.pad(edge, ((0, 0), (r, r), (r, r)))
    out = np.zeros_like(edge)
    for dv in range(-r, r + 1):
        for du in range(-(r - abs(dv)), r - abs(dv) + 1):
            out |= q[:, r + dv:r + dv + H, r + du:r + du + W]
    return out


def render_ref(depth, lut, ho, wo, minmax=None, vmin=0.0, vmax=1.0, mask=None, thickness=2, outline_rgb=0, alpha=0.0, bgr=False):
    """The arguments of hip_ext.depth_render as numpy arrays.  Returns (uint8 [B, ho, wo, 3], uint16 [B, ho, wo])."""
    assert 1 <= thickness <= 4
    lut = np.asarray(lut, dtype=np.uint8).reshape(256, 3)
    t = normalise(depth, minmax, vmin, vmax)
    B, hi, wi = t.shape
    nan = np.isnan(t)
    tz = np.where(nan, np.float32(0), t)
    idx = np.minimum((tz * np.float32(256)).astype(np.int64), 255)
    rgb = lut[idx]
    rgb[nan] = 0
    if mask is not None:
        mask = np.asarray(mask, dtype=np.float32)
        if alpha != 0:
            sel = mask == 0
            rgb[sel] = ((1.0 - alpha) * rgb[sel].astype(np.float64) + alpha * 200.0).astype(np.uint8)
        colour = np.array([(outline_rgb >> 16) & 255, (outline_rgb >> 8) & 255, outline_rgb & 255], dtype=np.uint8)
        rgb[painted_map(mask > 0, thickness)] = colour
    u16 = (tz * np.float32(65535)).astype(np.uint16)
    sy, sx = nearest_index(hi, ho), nearest_index(wi, wo)
    rgb = rgb[:, sy][:, :, sx]
    if bgr:
        rgb = rgb[..., ::-1]
    return np.ascontiguousarray(rgb), np.ascontiguousarray(u16[:, sy][:, :, sx])
