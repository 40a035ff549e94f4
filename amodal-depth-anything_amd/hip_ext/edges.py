"""The edge front end of the reference's evaluation on the device: skimage's Canny detector as ``extract_edges`` calls it (reference
src/util/metric.py:181-219: ``canny(float32 image, sigma, mask=None)``, mode 'constant', thresholds 0.1 / 0.2), scipy's exact Euclidean distance
transform (metric.py:242, 245) and the sums behind EdgeAcc / EdgeComp / soft_edge_error (metric.py:247-256, 317-328).  The reference copies every
map to the host and runs the detector there; here nothing leaves HBM (csrc/ada_edges.hip, include/ada_hip.h).

The arithmetic follows the host's storage discipline stage by stage -- DESIGN.md, "Edge metrics".  The one thing computed here, on the host, is the
Gaussian's tap weights, in double and in scipy's order, so that the kernel multiplies by the very numbers scipy would.

Maps are fp32 [h, w] or [B, h, w], a numpy array (copied to the device) or a device tensor.  There is no CPU fallback: a CPU tensor or a non-HIP target
raises HipExtError.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import (CANNY_MAX_RADIUS, CANNY_PRE_LOG, CANNY_PRE_LOG15, CANNY_PRE_NONE, SOFT_EDGE_MAX_RADIUS, HipExtError, canny_front, canny_hysteresis, edge_metric_sums,
               edt, soft_edge)
from ._staging import DeviceCache, check_planar, resolve_device, stage_planar

_PRE = {None: CANNY_PRE_NONE, "none": CANNY_PRE_NONE, "log": CANNY_PRE_LOG, "log1.5": CANNY_PRE_LOG15}

CannyStages = namedtuple("CannyStages", "edges pre smoothed isobel jsobel magnitude low_masked")
CannyStages.__doc__ = """Device tensors of canny(..., stages=True): edges uint8 0 / 1 [B, h, w] and the detector's fp32 stage maps [B, h, w]: the pre-transformed
image, the normalised Gaussian, ndi.sobel along axis 0 and axis 1, the magnitude, and the magnitude after non-maximum suppression."""


def gaussian_weights(sigma: float) -> np.ndarray:
    """fp64 [2 r + 1], r = int(4 sigma + 0.5): scipy.ndimage's _gaussian_kernel1d(sigma, 0, r), step for step in double."""
    sigma = float(sigma)
    if not sigma > 0.0:
        raise ValueError(f"gaussian_weights: sigma must be positive, got {sigma!r}")
    radius = int(4.0 * sigma + 0.5)
    if radius > CANNY_MAX_RADIUS:
        raise ValueError(f"gaussian_weights: sigma {sigma} needs a radius of {radius}, the kernel holds up to {CANNY_MAX_RADIUS} (sigma <= 4)")
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    return phi / phi.sum()


_WEIGHTS = DeviceCache(16)      # (sigma, device) -> fp64 device tensor


def _device_weights(sigma, device):
    return _WEIGHTS.get((float(sigma), device), lambda: torch.from_numpy(gaussian_weights(sigma)).to(device))


def _stage(x, device, who, name, dtypes):
    """The checked map as a contiguous device tensor [B, h, w] of dtypes[0] (bool is viewed as uint8) and whether the caller gave [h, w]."""
    single = check_planar(who, x, dtypes, f"{name}: expected")
    device = resolve_device(who, device, x)
    return stage_planar(who, x, device, name).contiguous(), single      # these kernels take no pitch


def _same(who, name, t, ref):
    if t.shape != ref.shape or t.device != ref.device:
        raise HipExtError(f"{who}: {name} is {tuple(t.shape)} on {t.device}, expected {tuple(ref.shape)} on {ref.device}")


@torch.no_grad()
def canny(image, sigma=1.0, low_threshold=0.1, high_threshold=0.2, pre=None, stages=False, device=None):
    """skimage.feature.canny(image, sigma, low_threshold, high_threshold) of a float32 image (mask=None, mode='constant'): uint8 0 / 1 [B, h, w] on the
    device ([h, w] in, [h, w] out).  ``pre``: None / 'none', 'log' (the reference's to_log) or 'log1.5' (extract_edges' default branch), applied inside
    the kernel.  The thresholds are compared in float32, as skimage compares them.  ``stages=True`` returns CannyStages.  Nothing is read back."""
    who = "canny"
    if pre not in _PRE:
        raise ValueError(f"{who}: pre must be None, 'none', 'log' or 'log1.5', got {pre!r}")
    low, high = float(low_threshold), float(high_threshold)
    if not low <= high:
        raise ValueError(f"{who}: low_threshold {low} must not exceed high_threshold {high}")
    if low == 0.0:
        low = 1e-14      # skimage's own substitute, so that a magnitude of 0 never passes
    img, single = _stage(image, device, who, "image", (torch.float32,))
    with torch.cuda.device(img.device):
        weights = _device_weights(sigma, img.device)
        low_masked = torch.empty_like(img)
        extra = [torch.empty_like(img) for _ in range(5)] if stages else [None] * 5
        canny_front(img, weights, low, low_masked, _PRE[pre], *extra)
        edges = torch.empty(img.shape, dtype=torch.uint8, device=img.device)
        canny_hysteresis(low_masked, high, edges)
    if stages:
        out = CannyStages(edges, *extra, low_masked)
        return CannyStages(*(t[0] for t in out)) if single else out
    return edges[0] if single else edges


@torch.no_grad()
def distance_transform_edt(edges, device=None):
    """scipy.ndimage.distance_transform_edt(np.logical_not(edges)): fp64 [B, h, w] on the device, the exact Euclidean distance of every pixel to the nearest
    non-zero pixel of ``edges`` (uint8 or bool).  An image without any edge pixel gives +inf everywhere: scipy's output for that input is an artefact of its
    implementation, not a documented value."""
    e, single = _stage(edges, device, "distance_transform_edt", "edges", (torch.uint8, torch.bool))
    with torch.cuda.device(e.device):
        out = torch.empty(e.shape, dtype=torch.float64, device=e.device)
        edt(e, out)
    return out[0] if single else out


@torch.no_grad()
def edge_sums(pred_edges, gt_edges, valid, d_target, d_pred, th_acc=10.0):
    """fp64 [B, 4] (hip_ext.EDGE_N_BDE, EDGE_SUM_DT, EDGE_N_GT, EDGE_SUM_DP): the sums behind EdgeAcc / EdgeComp.  Edge maps uint8 / bool, ``valid`` uint8 /
    bool or None, distance maps fp64, all [B, h, w] (or [h, w]) on one HIP device."""
    who = "edge_sums"
    pe, _ = _stage(pred_edges, None, who, "pred_edges", (torch.uint8, torch.bool))
    ge, _ = _stage(gt_edges, pe.device, who, "gt_edges", (torch.uint8, torch.bool))
    dt, _ = _stage(d_target, pe.device, who, "d_target", (torch.float64,))
    dp, _ = _stage(d_pred, pe.device, who, "d_pred", (torch.float64,))
    v = None if valid is None else _stage(valid, pe.device, who, "valid", (torch.uint8, torch.bool))[0]
    for name, t in (("gt_edges", ge), ("d_target", dt), ("d_pred", dp), ("valid", v)):
        if t is not None:
            _same(who, name, t, pe)
    with torch.cuda.device(pe.device):
        sums = torch.empty(pe.shape[0], 4, dtype=torch.float64, device=pe.device)
        edge_metric_sums(pe, ge, v, dt, dp, float(th_acc), sums)
    return sums


@torch.no_grad()
def soft_edge_sums(pred, gt, valid, radius=1):
    """fp64 [B, 2]: the number of valid pixels and the sum over them of min over the (2 radius + 1)^2 shifts of |shift(gt) - pred| (the reference's
    soft_edge_error before its mean).  pred, gt fp32, ``valid`` uint8 / bool or None, [B, h, w] (or [h, w]) on one HIP device."""
    who = "soft_edge_sums"
    r = int(radius)
    if r != radius or r < 0 or r > SOFT_EDGE_MAX_RADIUS:
        raise ValueError(f"{who}: radius must be an integer in 0 .. {SOFT_EDGE_MAX_RADIUS}, got {radius!r}")
    p, _ = _stage(pred, None, who, "pred", (torch.float32,))
    g, _ = _stage(gt, p.device, who, "gt", (torch.float32,))
    v = None if valid is None else _stage(valid, p.device, who, "valid", (torch.uint8, torch.bool))[0]
    for name, t in (("gt", g), ("valid", v)):
        if t is not None:
            _same(who, name, t, p)
    with torch.cuda.device(p.device):
        sums = torch.empty(p.shape[0], 2, dtype=torch.float64, device=p.device)
        soft_edge(p, g, v, r, sums)
    return sums
