"""Input preparation and depth read-out of the raw model's ``infer_image`` / ``image2tensor`` (reference RAW/dpt.py:186-221), on the device.

The reference prepares a decoded BGR photo on the host with OpenCV and numpy (RAW/util/transform.py:5-158); here the photo is copied to the
device as uint8 and one kernel does BGR -> RGB, / 255, cv2's INTER_CUBIC resize and the ImageNet normalisation (ada_image_prep_fwd), and
another resizes the depth map back to the photo (ada_depth_resize_fwd).  Only the network size is decided on the host.

The two-model pipeline of infer.py prepares its photo differently (reference infer.py:17-18, 83-91): no BGR -> RGB, a square size x size squash,
cv2's 8-bit INTER_LINEAR for the base network and torchvision's nearest for the amodal one, and nearest-resized masks.  photo_to_inputs,
masks_to_tensor and resize_nearest do that on the device (ada_photo_prep_fwd, ada_mask_prep_fwd, ada_nearest_resize_fwd).

colorize is the reference's depth-to-picture function (src/scripts/colorize_depth.py:18-84 and four more scripts): the 2nd / 95th percentile of the
valid pixels (hip_ext.quantile, ada_quantile_fwd), the colour map and the background colour in one kernel (ada_depth_colorize_fwd), RGBA bytes out.

render_depth is the other end of infer.py (reference infer.py:106-119): colour map, highlight_target, the nearest resize to the photo's size and the
channel flip in one kernel (ada_depth_render_fwd), uint8 pixels out.  The outline it paints is the tree's stand-in (src/util/image_util.py
draw_mask_outline), not cv2.findContours / drawContours: there is no cv2 here to pin those against.
"""
from __future__ import annotations

import numpy as np
import torch

from . import HipExtError, depth_colorize, depth_render, depth_resize, image_prep, mask_prep, nearest_resize, photo_prep
from ._staging import DeviceCache, as_int, check_planar, resolve_device, stage_hwc, stage_planar, with_index

PIXEL_MEAN = (0.485, 0.456, 0.406)
PIXEL_STD = (0.229, 0.224, 0.225)


def network_size(h: int, w: int, input_size: int = 518, multiple: int = 14) -> tuple:
    """(H, W) the reference resizes an h x w photo to: Resize(width=height=input_size, keep_aspect_ratio=True, ensure_multiple_of=multiple,
    resize_method="lower_bound").get_size (RAW/util/transform.py:51-107) -- the same float64 expressions in the same order, np.round
    (half to even: 160 x 208 at input_size 70 scales the width to 91 = 6.5 * 14, which becomes 84, not 98)."""
    def constrain(x, min_val):
        y = int(np.round(x / multiple) * multiple)
        if y < min_val:
            y = int(np.ceil(x / multiple) * multiple)
        return y

    scale_height = input_size / h
    scale_width = input_size / w
    if scale_width > scale_height:
        scale_height = scale_width
    else:
        scale_width = scale_height
    return constrain(scale_height * h, input_size), constrain(scale_width * w, input_size)


def _check_image(img):
    """uint8 [h, w, 3 | 4] (numpy array or torch tensor), else TypeError / ValueError.  Unlike the reference, which divides any dtype by 255,
    only 8-bit images are accepted."""
    if isinstance(img, np.ndarray):
        dtype_ok = img.dtype == np.uint8
    elif isinstance(img, torch.Tensor):
        dtype_ok = img.dtype == torch.uint8
    else:
        raise TypeError(f"image: expected a numpy array or a torch tensor, got {type(img).__name__}")
    if not dtype_ok:
        raise TypeError(f"image: expected uint8 pixels, got {img.dtype}")
    if img.ndim != 3 or img.shape[2] not in (3, 4) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"image: expected [h, w, 3] BGR or [h, w, 4] BGRA, got shape {tuple(img.shape)}")


def _stage_image(img, device, who):
    """The checked photo as a uint8 [h, w, c] tensor on ``device`` with packed pixels: numpy is copied, a device tensor is read in place at its
    own row stride (made contiguous only when its pixels are not packed).  Returns (tensor, device)."""
    _check_image(img)
    device = resolve_device(who, device, current=False)      # the caller names the device: the model's
    return stage_hwc(who, img, device), device


def image_to_tensor(img, input_size: int = 518, device=None):
    """``img``: uint8 BGR [h, w, 3] or BGRA [h, w, 4] (alpha ignored) -- a numpy array (copied to ``device``; a non-contiguous one is made
    contiguous first) or a torch tensor on ``device`` (read in place, rows at their own stride: a crop of a decoded frame costs no copy).
    Returns (fp32 [1, 3, H, W] ImageNet-normalised RGB on ``device``, (h, w)), H x W = network_size(h, w, input_size): the reference's
    image2tensor (RAW/dpt.py:196-221)."""
    src, device = _stage_image(img, device, "image_to_tensor")
    h, w, c = src.shape
    H, W = network_size(h, w, input_size)
    out = torch.empty(1, 3, H, W, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        image_prep(src, 1, h, w, c, src.stride(0), h * src.stride(0), H, W, PIXEL_MEAN, PIXEL_STD, out)
    return out, (h, w)


def _check_size(size, who) -> int:
    s = as_int(size)
    if s is None or s < 14 or s % 14:
        raise ValueError(f"{who}: size must be a positive multiple of 14 (the patch size), got {size!r}")
    return s


def photo_to_inputs(img, size: int = 518, device=None):
    """The two network inputs of the amodal pipeline from one decoded photo (reference infer.py:17-18, 83-85).  ``img`` as for image_to_tensor
    (same checks, same staging, same errors).  Returns (rgb_raw, rgb, (h, w)), both fp32 [1, 3, size, size] in [0, 1] on ``device``:
    rgb_raw = cv2.resize(img, (size, size)) / 255 (8-bit INTER_LINEAR) for the base-depth network, rgb = Resize(NEAREST)(img / 255) for the
    amodal one.  The channel order of the photo is KEPT (B, G, R planes for a cv2.imread photo), as the reference keeps it on this path."""
    size = _check_size(size, "photo_to_inputs")
    src, device = _stage_image(img, device, "photo_to_inputs")
    h, w, c = src.shape
    rgb_raw = torch.empty(1, 3, size, size, dtype=torch.float32, device=device)
    rgb = torch.empty(1, 3, size, size, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        photo_prep(src, h, w, c, src.stride(0), size, size, raw_out=rgb_raw, near_out=rgb)
    return rgb_raw, rgb, (h, w)


def masks_to_tensor(masks, size: int, device, guide: bool = False):
    """``masks``: uint8 or bool [h, w] or [K, h, w] (numpy array, copied; or a torch tensor on ``device``, read in place when its rows are
    packed); any non-zero value is inside.  Returns mask01 fp32 0/1 [K, 1, size, size] on ``device``: F.interpolate(mode="nearest") > 0, the
    mask of reference infer.py:86-87.  guide=True: (mask01, 2 * mask01 - 1), the second being the network's guide_mask (infer.py:91)."""
    check_planar("masks", masks, (torch.uint8, torch.bool))
    size = _check_size(size, "masks_to_tensor")
    device = resolve_device("masks_to_tensor", device, current=False)
    src = stage_planar("masks_to_tensor", masks, device, "masks", limits=False)
    K, h, w = src.shape
    mask01 = torch.empty(K, 1, size, size, dtype=torch.float32, device=device)
    pm1 = torch.empty_like(mask01) if guide else None
    with torch.cuda.device(device):
        mask_prep(src, K, h, w, src.stride(1), src.stride(0), size, size, mask01, pm1)
    return (mask01, pm1) if guide else mask01


def resize_depth(depth: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """fp32 [B, H, W] on the device -> fp32 [B, h, w]: F.interpolate(depth[:, None], (h, w), mode="bilinear", align_corners=True)[:, 0]
    (RAW/dpt.py:192)."""
    if depth.dim() != 3 or depth.dtype != torch.float32:
        raise HipExtError(f"resize_depth: expected fp32 [B, H, W], got {depth.dtype} {tuple(depth.shape)}")
    depth = depth.contiguous()
    out = torch.empty(depth.shape[0], h, w, dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        depth_resize(depth, out)
    return out


def resize_nearest(depth: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """fp32 [B, H, W] on the device -> fp32 [B, h, w] with cv2.resize(INTER_NEAREST)'s rule, the resize the reference returns its rendering to the
    photo's size with (infer.py:77, 113)."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3 or depth.dtype != torch.float32:
        raise HipExtError(f"resize_nearest: expected fp32 [B, H, W], got {getattr(depth, 'dtype', type(depth).__name__)} {tuple(getattr(depth, 'shape', ()))}")
    hw = as_int(h), as_int(w)
    if None in hw or min(hw) < 1:
        raise ValueError(f"resize_nearest: the target size must be two positive integers, got {h!r} x {w!r}")
    h, w = hw
    depth = depth.contiguous()
    out = torch.empty(depth.shape[0], h, w, dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        nearest_resize(depth, out)
    return out


_LUTS = DeviceCache(64)      # (name, device[, "rgba"]) -> uint8 table on the device


def _colormap(who, cmap):
    import matplotlib
    cm = matplotlib.colormaps[cmap]
    if cm.N != 256:
        raise ValueError(f"{who}: colour map {cmap!r} has {cm.N} entries, the renderer needs 256")
    return cm


def colormap_lut(cmap: str = "Spectral_r", device=None) -> torch.Tensor:
    """The 256 colours of a matplotlib colour map as uint8 [256, 3] (R, G, B) on ``device``: (cmap(i)[:3] * 255).astype(uint8), the table
    ada_depth_render_fwd indexes with min((int)(t * 256), 255).  Cached per (name, device).  A map that does not have 256 entries is refused:
    the index rule assumes them."""
    cm = _colormap("colormap_lut", cmap)
    device = with_index("cpu" if device is None else device)
    return _LUTS.get((cmap, device), lambda: torch.from_numpy(np.ascontiguousarray((cm(np.arange(256))[:, :3] * 255).astype(np.uint8))).to(device))


def colormap_lut_rgba(cmap: str = "turbo_r", device=None) -> torch.Tensor:
    """The 256 colours of a matplotlib colour map as uint8 [256, 4] (R, G, B, A) on ``device``: cmap(arange(256), bytes=True), the table
    ada_depth_colorize_fwd indexes.  Cached per (name, device); a map without 256 entries is refused, as by colormap_lut."""
    cm = _colormap("colormap_lut_rgba", cmap)
    device = with_index("cpu" if device is None else device)
    return _LUTS.get((cmap, device, "rgba"), lambda: torch.from_numpy(np.ascontiguousarray(cm(np.arange(256), bytes=True))).to(device))


def colorize(value, vmin=None, vmax=None, cmap="turbo_r", invalid_val=-99, invalid_mask=None, background_color=(128, 128, 128, 255), gamma_corrected=False,
             value_transform=None, vminp=2, vmaxp=95):
    """The reference's colorize() on the device: fp32 depth maps [B, H, W] (or one [H, W]) -> uint8 [B, H, W, 4] R, G, B, A on the device.  A bound left
    None is its percentile (``vminp`` / ``vmaxp``) over the image's valid pixels -- those outside ``invalid_mask`` (uint8 / bool, non-zero = invalid) when
    given, else those != ``invalid_val`` -- taken on the device (hip_ext.quantile.percentile_range); t = (value - vmin) / (vmax - vmin) in double
    (value * 0 where the bounds are equal) through ``cmap`` as matplotlib's cmap(t, bytes=True); invalid pixels get ``background_color``.  The result is
    the reference's on the map as float64.  Nothing is read back, the launches depend on the shape alone.  ``gamma_corrected`` and ``value_transform``
    are not built."""
    who = "colorize"
    if gamma_corrected:
        raise NotImplementedError(f"{who}: gamma_corrected is not built on the device (np.power(img / 255, 2.2) in double per byte; none of the reference's call sites sets it)")
    if value_transform is not None:
        raise NotImplementedError(f"{who}: value_transform is an arbitrary host callable on the normalised map; it cannot run inside the device kernel")
    if not isinstance(value, torch.Tensor) or value.dtype != torch.float32 or value.dim() not in (2, 3) or value.numel() == 0:
        raise HipExtError(f"{who}: expected fp32 [B, H, W] or [H, W], got {getattr(value, 'dtype', type(value).__name__)} {tuple(getattr(value, 'shape', ()))}")
    if not value.is_cuda:
        raise HipExtError(f"{who}: value on {value.device}, expected a HIP device (the HIP path has no CPU fallback)")
    if value.dim() == 2:
        value = value[None]
        invalid_mask = invalid_mask[None] if isinstance(invalid_mask, torch.Tensor) and invalid_mask.dim() == 2 else invalid_mask
    value = value.contiguous()
    B, H, W = value.shape
    dev = value.device
    bg = tuple(as_int(v) for v in background_color) if isinstance(background_color, (tuple, list)) and len(background_color) == 4 else (None,)
    if None in bg or not all(0 <= v <= 255 for v in bg):
        raise ValueError(f"{who}: background_color must be four bytes (R, G, B, A), got {background_color!r}")
    mask = None
    if invalid_mask is not None:
        from .quantile import _as_mask
        mask = _as_mask(invalid_mask, value, who, "invalid_mask")
    range64 = None
    if vmin is None or vmax is None:
        from .quantile import percentile_range
        range64, _ = percentile_range(value, vminp, vmaxp, invalid_val=invalid_val, invalid_mask=mask)
        if vmin is not None:
            range64[:, 0] = float(vmin)
        if vmax is not None:
            range64[:, 1] = float(vmax)
    lut = colormap_lut_rgba(cmap, dev)
    out = torch.empty(B, H, W, 4, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        depth_colorize(value, lut, out, range64=range64, vmin=0.0 if vmin is None else float(vmin), vmax=1.0 if vmax is None else float(vmax),
                       invalid_mask=mask, invalid_val=float(invalid_val), background=bg)
    return out


def render_depth(depth, masks=None, out_size=None, cmap="Spectral_r", vmin=0.0, vmax=1.0, minmax=None, thickness=2, outline=(0, 0, 0), alpha=0.0,
                 bgr=True, u16=False):
    """fp32 depth maps [B, H, W] on the device -> uint8 [B, h, w, 3] on the device, the pictures of reference infer.py:106-119:
    ((d - vmin) / (vmax - vmin)).clip(0, 1) through the colour map ``cmap``; with ``masks`` (fp32 [B, H, W], > 0 inside) highlight_target's
    overlay (``alpha``, towards grey 200 outside the mask) and outline (``thickness`` 1..4, ``outline`` = (R, G, B) bytes; the stand-in of
    src/util/image_util.py, not cv2's contours); cv2.resize(INTER_NEAREST) to ``out_size`` = (h, w) (None: H x W); B, G, R bytes with ``bgr``.
    ``minmax``: device fp32 [B, 2] (hip_ext.minmax) used per image instead of vmin / vmax.  u16=True: (rendering, uint16 [B, h, w]), the
    16-bit map of infer.py:107-108.  Nothing is read back to the host."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3 or depth.dtype != torch.float32:
        raise HipExtError(f"render_depth: expected fp32 [B, H, W], got {getattr(depth, 'dtype', type(depth).__name__)} {tuple(getattr(depth, 'shape', ()))}")
    if not depth.is_cuda:
        raise HipExtError(f"render_depth: depth on {depth.device}, expected a HIP device (the HIP path has no CPU fallback)")
    B, H, W = depth.shape
    if masks is not None and (not isinstance(masks, torch.Tensor) or masks.dtype != torch.float32 or masks.shape != depth.shape or masks.device != depth.device):
        raise HipExtError(f"render_depth: masks must be fp32 {tuple(depth.shape)} on {depth.device}, got "
                          f"{getattr(masks, 'dtype', type(masks).__name__)} {tuple(getattr(masks, 'shape', ()))}")
    if minmax is not None and (not isinstance(minmax, torch.Tensor) or minmax.dtype != torch.float32 or tuple(minmax.shape) != (B, 2)
                               or minmax.device != depth.device):
        raise HipExtError(f"render_depth: minmax must be fp32 [{B}, 2] on {depth.device}, got "
                          f"{getattr(minmax, 'dtype', type(minmax).__name__)} {tuple(getattr(minmax, 'shape', ()))}")
    if out_size is None:
        h, w = H, W
    else:
        hw = tuple(as_int(v) for v in out_size) if isinstance(out_size, (tuple, list)) and len(out_size) == 2 else (None, None)
        if None in hw or min(hw) < 1:
            raise ValueError(f"render_depth: out_size must be None or two positive integers (h, w), got {out_size!r}")
        h, w = hw
    t = as_int(thickness)
    if t is None or not 1 <= t <= 4:
        raise ValueError(f"render_depth: thickness must be 1..4, got {thickness!r}")
    rgb = tuple(as_int(v) for v in outline) if isinstance(outline, (tuple, list)) and len(outline) == 3 else (None,)
    if None in rgb or not all(0 <= v <= 255 for v in rgb):
        raise ValueError(f"render_depth: outline must be three bytes (R, G, B), got {outline!r}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"render_depth: alpha must lie in [0, 1], got {alpha!r}")
    if minmax is None and float(vmax) == float(vmin):
        raise ValueError(f"render_depth: vmax == vmin ({vmin!r}): nothing to normalise by")
    lut = colormap_lut(cmap, depth.device)
    out = torch.empty(B, h, w, 3, dtype=torch.uint8, device=depth.device)
    out16 = torch.empty(B, h, w, dtype=torch.uint16, device=depth.device) if u16 else None
    with torch.cuda.device(depth.device):
        depth_render(depth.contiguous(), lut, h, w, out, out16, minmax=None if minmax is None else minmax.contiguous(), vmin=vmin, vmax=vmax,
                     mask=None if masks is None else masks.contiguous(), thickness=t, outline_rgb=(rgb[0] << 16) | (rgb[1] << 8) | rgb[2],
                     alpha=float(alpha), bgr=bgr)
    return (out, out16) if u16 else out
