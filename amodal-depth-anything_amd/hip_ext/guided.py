"""Guided filter and guided joint up-sampling on the device (He, Sun, Tang; csrc/ada_guided.hip; the contract is include/ada_hip.h's "Guided filter"
section, restated in numpy by tests/_guided_ref.py).  A map is fitted, window by window, as a linear function of a guide image -- the photo -- and the
fit is applied to the guide: smoothing that keeps the guide's edges, and, with the fit made at the map's size and applied at the photo's, the way from
depth at the network's size to depth at the photo's size whose edges lie where the photo's lie.  The reference has no such operation: it resizes with
cv2's nearest rule.

``p`` is fp32 [h, w] or [B, h, w].  ``guide`` is uint8 or fp32, [gh, gw] or [gh, gw, C] for a single map and [B, gh, gw] or [B, gh, gw, C] for a
batch, C = 1 or 3, pixels as a photo arrives (HWC).  ``radius`` is an integer 0 .. GUIDED_MAX_RADIUS; the window is (2 radius + 1)^2, clipped by the
image and normalised by the number of voting samples.  ``eps`` > 0 is in [0, 1]^2 units for a uint8 guide (it is multiplied by 255^2) and in the
guide's own units for an fp32 one.  ``valid`` (uint8 / bool, p's shape) lets only its non-zero samples vote, and a NaN never votes.  Where no fit
reaches, the output is ``fill`` (NaN by default).  Everything is computed in fp64 and rounded to fp32 once.

numpy arrays (copied to the device) or device tensors; [h, w] in gives [H, W] out.  There is no CPU fallback: a CPU tensor or a non-HIP target raises
HipExtError.  Nothing is read back.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import GUIDED_MAX_RADIUS, HipExtError, guided_apply_fwd, guided_coeff_fwd
from ._staging import _to_device, as_int, check_planar, resolve_device, stage_planar


def _radius(who, radius):
    r = as_int(radius)
    if r is None or not 0 <= r <= GUIDED_MAX_RADIUS:
        raise ValueError(f"{who}: radius must be an integer in 0 .. {GUIDED_MAX_RADIUS}, got {radius!r}")
    return r


def _eps(who, eps, guide):
    """eps in raw guide units: times 255^2 for a uint8 guide."""
    try:
        e = float(eps)
    except (TypeError, ValueError):
        e = float("nan")
    if isinstance(eps, bool) or not (math.isfinite(e) and e > 0):
        raise ValueError(f"{who}: eps must be a finite positive number, got {eps!r}")
    return e * 65025.0 if str(guide.dtype).endswith("uint8") else e


def _check_guide(who, guide, lead):
    """(gh, gw, C) of a guide whose leading axes must equal ``lead`` (() for a single map, (B,) for a batch); no device is looked at."""
    if not isinstance(guide, (np.ndarray, torch.Tensor)):
        raise TypeError(f"{who}: guide: expected a numpy array or a torch tensor, got {type(guide).__name__}")
    if str(guide.dtype).replace("torch.", "") not in ("uint8", "float32"):
        raise HipExtError(f"{who}: guide: expected uint8 or float32, got {guide.dtype} (the HIP path has kernels for these types only)")
    shape = tuple(guide.shape)
    n = len(lead)
    if len(shape) not in (n + 2, n + 3) or shape[:n] != tuple(lead) or min(shape, default=0) < 1:
        raise ValueError(f"{who}: guide of shape {shape} for a map with leading axes {tuple(lead)}: expected [gh, gw] or [gh, gw, C] behind them")
    gh, gw = shape[n], shape[n + 1]
    C = shape[n + 2] if len(shape) == n + 3 else 1
    if C not in (1, 3):
        raise ValueError(f"{who}: the guide has 1 or 3 channels, got {C}")
    return gh, gw, C


def _stage_guide(who, guide, device, batch, gh, gw, C):
    return _to_device(who, guide, device, "guide").reshape(batch, gh, gw, C).contiguous()      # the kernels take no pitch: a crop is packed here


def _check_fit(who, p, guide, radius, eps, valid):
    """Everything of a fit that needs no device: (whether p is [h, w], radius, raw eps, (gh, gw, C))."""
    single = check_planar(who, p, (torch.float32,), "p: expected")
    r = _radius(who, radius)
    g = _check_guide(who, guide, tuple(p.shape[:-2]))
    e = _eps(who, eps, guide)
    if g[0] < p.shape[-2] or g[1] < p.shape[-1]:
        raise ValueError(f"{who}: the guide ({g[0]} x {g[1]}) must not be smaller than the map ({p.shape[-2]} x {p.shape[-1]})")
    if valid is not None:
        check_planar(who, valid, (torch.uint8, torch.bool), "valid: expected")
        if tuple(valid.shape) != tuple(p.shape):
            raise ValueError(f"{who}: valid of shape {tuple(valid.shape)} for p of shape {tuple(p.shape)}")
    return single, r, e, g


def _fit(who, p, guide, r, e, g, valid, device):
    """(coeff [B, h, w, C + 1], covered [B, h, w], the staged guide) on ``device``."""
    ps = stage_planar(who, p, device, "p").contiguous()
    vs = None if valid is None else stage_planar(who, valid, device, "valid").contiguous()
    B, h, w = ps.shape
    gs = _stage_guide(who, guide, device, B, *g)
    coeff = torch.empty(B, h, w, g[2] + 1, dtype=torch.float64, device=device)
    covered = torch.empty(B, h, w, dtype=torch.uint8, device=device)
    guided_coeff_fwd(ps, gs, r, e, coeff, covered, valid=vs)
    return coeff, covered, gs


def _apply(coeff, covered, gs, fill):
    out = torch.empty(gs.shape[:3], dtype=torch.float32, device=gs.device)
    guided_apply_fwd(coeff, covered, gs, out, fill=float("nan") if fill is None else float(fill))
    return out


def _run(who, p, guide, radius, eps, valid, fill, return_covered, device, same_size=False):
    """Both halves in one call."""
    single, r, e, g = _check_fit(who, p, guide, radius, eps, valid)
    if same_size and g[:2] != tuple(p.shape[-2:]):
        raise ValueError(f"{who}: the guide must have p's size {tuple(p.shape[-2:])}, got {g[:2]} (guided_upsample takes a larger one)")
    device = resolve_device(who, device, p, guide, valid)
    with torch.cuda.device(device):
        coeff, covered, gs = _fit(who, p, guide, r, e, g, valid, device)
        out = _apply(coeff, covered, gs, fill)
    if single:
        out, covered = out[0], covered[0]
    return (out, covered) if return_covered else out


@torch.no_grad()
def guided_coefficients(p, guide, radius, eps, valid=None, device=None):
    """The first half: (coeff, covered) of the fit of ``p`` in the guide's samples at p's positions -- coeff fp64 [h, w, C + 1] / [B, h, w, C + 1], the
    window means of (a_0 .. a_{C-1}, b); covered uint8, 1 where at least one window of the pixel's neighbourhood had a voting sample.  One fit can be
    applied to several guides of one size ratio with guided_apply."""
    who = "guided_coefficients"
    single, r, e, g = _check_fit(who, p, guide, radius, eps, valid)
    device = resolve_device(who, device, p, guide, valid)
    with torch.cuda.device(device):
        coeff, covered, _ = _fit(who, p, guide, r, e, g, valid, device)
    return (coeff[0], covered[0]) if single else (coeff, covered)


@torch.no_grad()
def guided_apply(coeff, covered, guide, fill=None, device=None):
    """The second half: q = a . I + b at the guide's size, fp32 [H, W] / [B, H, W], with (a, b) interpolated bilinearly (half-pixel centres) from
    guided_coefficients' tables.  Taps that are not covered get weight 0 and the rest are renormalised; ``fill`` (NaN by default) where none is."""
    who = "guided_apply"
    if not isinstance(coeff, torch.Tensor) or coeff.dtype != torch.float64 or coeff.dim() not in (3, 4):
        raise HipExtError(f"{who}: coeff must be guided_coefficients' fp64 device tensor [h, w, C + 1] or [B, h, w, C + 1]")
    single = coeff.dim() == 3
    if not isinstance(covered, torch.Tensor) or covered.dtype not in (torch.uint8, torch.bool) or tuple(covered.shape) != tuple(coeff.shape[:-1]):
        raise ValueError(f"{who}: covered must be uint8 of shape {tuple(coeff.shape[:-1])}, got {tuple(getattr(covered, 'shape', ()))}")
    gh, gw, C = _check_guide(who, guide, tuple(coeff.shape[:-3]))
    if coeff.shape[-1] != C + 1:
        raise ValueError(f"{who}: coefficients of a {coeff.shape[-1] - 1}-channel guide applied to a guide of {C} channels")
    if gh < coeff.shape[-3] or gw < coeff.shape[-2]:
        raise ValueError(f"{who}: the guide ({gh} x {gw}) must not be smaller than the map ({coeff.shape[-3]} x {coeff.shape[-2]})")
    device = resolve_device(who, device, coeff, guide)
    with torch.cuda.device(device):
        cs = (coeff[None] if single else coeff).contiguous()
        ms = stage_planar(who, covered, device, "covered").contiguous()
        out = _apply(cs, ms, _stage_guide(who, guide, device, cs.shape[0], gh, gw, C), fill)
    return out[0] if single else out


@torch.no_grad()
def guided_upsample(p, guide, radius, eps, valid=None, fill=None, return_covered=False, device=None):
    """``p`` at the network's size taken to the size of ``guide``, the photo, with the photo's edges (the fast guided filter): the fit is made at p's
    size against the guide sub-sampled at p's positions and applied to the full guide.  The guide must be at least p's size on both axes.
    ``return_covered=True`` also returns ``covered`` (uint8, p's shape): 0 where no window within reach had a voting sample."""
    return _run("guided_upsample", p, guide, radius, eps, valid, fill, return_covered, device)


@torch.no_grad()
def guided_filter(p, guide, radius, eps, valid=None, fill=None, device=None):
    """The guided filter proper: ``guide`` has p's size and the result is p smoothed over (2 radius + 1)^2 windows except across the guide's edges
    (eps sets what counts as one: a window whose guide variance is far below eps is averaged, one far above keeps its structure)."""
    return _run("guided_filter", p, guide, radius, eps, valid, fill, False, device, same_size=True)


__all__ = ["guided_filter", "guided_upsample", "guided_coefficients", "guided_apply", "HipExtError"]
