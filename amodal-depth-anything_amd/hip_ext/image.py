"""Input preparation and depth read-out of the raw model's ``infer_image`` / ``image2tensor`` (reference RAW/dpt.py:186-221), on the device.

The reference prepares a decoded BGR photo on the host with OpenCV and numpy (RAW/util/transform.py:5-158); here the photo is copied to the
device as uint8 and one kernel does BGR -> RGB, / 255, cv2's INTER_CUBIC resize and the ImageNet normalisation (ada_image_prep_fwd), and
another resizes the depth map back to the photo (ada_depth_resize_fwd).  Only the network size is decided on the host.
"""
from __future__ import annotations

import numpy as np
import torch

from . import HipExtError, depth_resize, image_prep

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


def image_to_tensor(img, input_size: int = 518, device=None):
    """``img``: uint8 BGR [h, w, 3] or BGRA [h, w, 4] (alpha ignored) -- a numpy array (copied to ``device``; a non-contiguous one is made
    contiguous first) or a torch tensor on ``device`` (read in place, rows at their own stride: a crop of a decoded frame costs no copy).
    Returns (fp32 [1, 3, H, W] ImageNet-normalised RGB on ``device``, (h, w)), H x W = network_size(h, w, input_size): the reference's
    image2tensor (RAW/dpt.py:196-221)."""
    _check_image(img)
    device = torch.device(device) if device is not None else None
    if device is None or device.type != "cuda":
        raise HipExtError(f"image_to_tensor: target device {device} is not a HIP device (the HIP path has no CPU fallback)")
    if isinstance(img, np.ndarray):
        src = torch.from_numpy(np.ascontiguousarray(img)).to(device)
    else:
        if img.device != device:
            raise HipExtError(f"image_to_tensor: image on {img.device}, expected it on the HIP device {device}")
        c = img.shape[2]
        packed = img.stride(2) == 1 and img.stride(1) == c and img.stride(0) >= img.shape[1] * c
        src = img if packed else img.contiguous()
    h, w, c = src.shape
    H, W = network_size(h, w, input_size)
    out = torch.empty(1, 3, H, W, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        image_prep(src, 1, h, w, c, src.stride(0), h * src.stride(0), H, W, PIXEL_MEAN, PIXEL_STD, out)
    return out, (h, w)


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
