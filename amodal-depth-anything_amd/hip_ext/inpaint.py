"""Hole filling on the device: a pixel without a sample gets a value from the pixels that have one (csrc/ada_inpaint.hip; the contract is
include/ada_hip.h's "Hole filling" section, restated in numpy by tests/_inpaint_ref.py).  The reference has no such operation, and a rendered view
(hip_ext.geometry.render_mesh) or a map with objects taken out is full of holes; callers went to the host and to scipy.

Two forms.  ``nearest_valid`` / ``fill_nearest``: the exact Euclidean feature transform -- every pixel learns the flat position r * w + c of the nearest
valid pixel of its image, ties to the smallest flat position -- and the copy of the value found there.  ``fill_smooth``: the push-pull fill, a pyramid
of masked 2 x 2 means and a bilinear interpolation back down, in float32 with every operation rounded on its own.  Both leave valid pixels bit for bit
as they were; neither looks at the geometry of what it fills: this is interpolation, not a learned completion.

``valid`` is uint8 or bool [h, w] / [B, h, w], non-zero = the pixel has a sample; one mask serves all channels of an image.  ``x`` is fp32 or uint8
[h, w], [B, h, w] or [B, C, h, w], or a uint8 image [h, w, 3] / [B, h, w, 3]; numpy arrays (copied to the device) or device tensors; [h, w] in gives
[h, w] out.  uint8 is filled as fp32 planes and rounded half to even back to uint8.  There is no CPU fallback: a CPU tensor or a non-HIP target raises
HipExtError.  Nothing is read back.
"""
from __future__ import annotations

import numpy as np
import torch

from . import HipExtError, fill_gather, nearest_valid_fwd, push_pull
from ._staging import _to_device, check_planar, resolve_device, stage_planar

MAX_SIDE = 32767      # squared distances are exact in 32 bits


def _check_valid(who, valid):
    """Whether a checked ``valid`` is [h, w]."""
    if not isinstance(valid, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{who}: valid must be a numpy array or a torch tensor, got {type(valid).__name__}")
    try:
        single = check_planar(who, valid, (torch.uint8, torch.bool), "valid must be")
    except TypeError as e:
        raise ValueError(str(e)) from None
    if max(valid.shape[-2:]) > MAX_SIDE or (valid.ndim == 3 and valid.shape[0] > 65535):
        raise ValueError(f"{who}: valid: h and w must stay within {MAX_SIDE} and the batch within 65535, got shape {tuple(valid.shape)}")
    return single


def _stage_valid(who, valid, device):
    return stage_planar(who, valid, device, "valid").contiguous()      # these kernels take no pitch: a crop is packed here


def _layout(who, x, vshape):
    """How ``x`` relates to a ``valid`` of shape ``vshape`` ([h, w] or [B, h, w]): 'planar' (valid's own shape), 'planes' ([B, C, h, w]) or 'hwc'
    ([h, w, 3] / [B, h, w, 3], uint8 only).  ValueError for anything else, before any device is looked at."""
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{who}: x must be a numpy array or a torch tensor, got {type(x).__name__}")
    kind = str(x.dtype).replace("torch.", "")
    if kind not in ("float32", "uint8"):
        raise ValueError(f"{who}: x must be float32 or uint8, got {x.dtype}")
    xs, vs = tuple(x.shape), tuple(vshape)
    if min(xs, default=0) < 1:
        raise ValueError(f"{who}: x of shape {xs} is empty")
    if xs == vs:
        return "planar"
    if kind == "uint8" and xs == vs + (3,):
        return "hwc"
    if len(vs) == 3 and len(xs) == 4 and (xs[0],) + xs[2:] == vs:
        return "planes"
    raise ValueError(f"{who}: x of shape {xs} ({kind}) for valid of shape {vs}: expected valid's shape, [B, C, h, w] for valid [B, h, w], or a uint8 image "
                     f"with a last axis of 3")


def _stage_planes(who, x, layout, device):
    """x as a contiguous fp32 device tensor [B, C, h, w]."""
    t = _to_device(who, x, device, "x")
    if layout == "planar":
        t = t[None, None] if t.dim() == 2 else t[:, None]
    elif layout == "hwc":
        t = (t[None] if t.dim() == 3 else t).permute(0, 3, 1, 2)
    return t.to(torch.float32).contiguous()


def _restore(planes, layout, single, as_u8):
    """The filled planes in x's own layout and type."""
    if as_u8:
        planes = torch.round(planes).to(torch.uint8)      # half to even; a filled value lies within the range of the samples, so within 0 .. 255
    if layout == "planar":
        return planes[0, 0] if single else planes[:, 0]
    if layout == "hwc":
        out = planes.permute(0, 2, 3, 1).contiguous()
        return out[0] if single else out
    return planes


@torch.no_grad()
def nearest_valid(valid, return_distance=False, device=None):
    """int32 [B, h, w] on the device ([h, w] in, [h, w] out): for every pixel the flat position r * w + c of the valid pixel of the same image nearest in
    Euclidean distance.  A valid pixel maps to itself; among equally near pixels the smallest flat position wins (scipy's own choice there is an artefact
    of its implementation and is not followed); an image without a valid pixel gives -1 everywhere.  ``return_distance=True`` also returns the fp64
    distances: scipy.ndimage.distance_transform_edt(valid == 0) wherever an image has a valid pixel, +inf where it has none (as
    hip_ext.edges.distance_transform_edt)."""
    who = "nearest_valid"
    single = _check_valid(who, valid)
    device = resolve_device(who, device, valid)
    with torch.cuda.device(device):
        v = _stage_valid(who, valid, device)
        index = torch.empty(v.shape, dtype=torch.int32, device=device)
        dist2 = torch.empty_like(index) if return_distance else None
        nearest_valid_fwd(v, index, dist2)
        dist = None
        if return_distance:
            dist = torch.where(index >= 0, dist2.to(torch.float64).sqrt(), float("inf"))      # exact integers below 2^31: the correctly rounded root
    if single:
        index, dist = index[0], (dist[0] if return_distance else None)
    return (index, dist) if return_distance else index


def _fill(who, x, valid, empty, device, smooth):
    single = _check_valid(who, valid)
    layout = _layout(who, x, valid.shape)
    empty = float(empty)
    device = resolve_device(who, device, x, valid)
    as_u8 = str(x.dtype).endswith("uint8")
    with torch.cuda.device(device):
        v = _stage_valid(who, valid, device)
        planes = _stage_planes(who, x, layout, device)
        out = torch.empty_like(planes)
        if smooth:
            push_pull(planes, v, out, empty)
        else:
            index = torch.empty(v.shape, dtype=torch.int32, device=device)
            nearest_valid_fwd(v, index)
            fill_gather(planes, v, index, out, empty)
        return _restore(out, layout, single, as_u8)


@torch.no_grad()
def fill_nearest(x, valid, empty=0.0, device=None):
    """x with every invalid pixel replaced by the value of its nearest valid pixel (nearest_valid's, ties included), all channels from the same pixel;
    ``empty`` where an image has no valid pixel.  Values are copied bit for bit, so on uint8 this is a pure copy of bytes."""
    return _fill("fill_nearest", x, valid, empty, device, smooth=False)


@torch.no_grad()
def fill_smooth(x, valid, empty=0.0, device=None):
    """x with every invalid pixel replaced by the push-pull fill of the valid ones: masked 2 x 2 means up a pyramid whose levels halve (rounding up) to
    1 x 1, then, top down, every still empty pixel takes the bilinear value (half-pixel centres, clamped borders) of the level above.  float32, each
    operation rounded on its own -- tests/_inpaint_ref.py gives the same bits.  What lies under an invalid pixel, NaN and inf included, never reaches a
    result; ``empty`` where an image has no valid pixel.  Every filled value lies within the range of the valid samples up to rounding."""
    return _fill("fill_smooth", x, valid, empty, device, smooth=True)


__all__ = ["nearest_valid", "fill_nearest", "fill_smooth", "HipExtError"]
