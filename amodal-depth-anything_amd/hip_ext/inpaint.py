"""Hole filling on the device: a pixel without a sample gets a value from the pixels that have one (csrc/ada_inpaint.hip; the contract is
include/ada_hip.h's "Hole filling" section, restated in numpy by tests/_inpaint_ref.py).  The reference has no such operation, and a rendered view
(hip_ext.geometry.render_mesh) or a map with objects taken out is full of holes; callers went to the host and to scipy.

Two forms.  ``nearest_valid`` / ``fill_nearest``: the exact Euclidean feature transform -- every pixel learns the flat position r * w + c of the nearest
valid pixel of its image, ties to the smallest flat position -- and the copy of the value found there.  ``fill_smooth``: the push-pull fill, a pyramid
of masked 2 x 2 means and a bilinear interpolation back down, in float32 with every operation rounded on its own.  Both leave valid pixels bit for bit
as they were; neither looks at the geometry of what it fills: this is interpolation, not a learned completion.

A third form has an equation behind it.  ``fill_harmonic``: the membrane solve (csrc/ada_membrane.hip; include/ada_hip.h, "Membrane solve", restated by
tests/_membrane_ref.py) -- every unknown pixel of a ``domain`` becomes the mean of its 4-neighbours inside the domain, by conjugate gradients in fp64.  It
respects a domain boundary, which the push-pull fill cannot, and it carries a gradient field: ``blend_seamless`` clones one map into another by
extending the difference of the two over the pasted region and adding the source back.

``valid`` is uint8 or bool [h, w] / [B, h, w], non-zero = the pixel has a sample; one mask serves all channels of an image.  ``x`` is fp32 or uint8
[h, w], [B, h, w] or [B, C, h, w], or a uint8 image [h, w, 3] / [B, h, w, 3]; numpy arrays (copied to the device) or device tensors; [h, w] in gives
[h, w] out.  uint8 is filled as fp32 planes and rounded half to even back to uint8.  There is no CPU fallback: a CPU tensor or a non-HIP target raises
HipExtError.  Nothing is read back.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import HipExtError, fill_gather, membrane_begin, membrane_end, membrane_iterate, membrane_workspace_bytes, nearest_valid_fwd, push_pull
from ._staging import _to_device, as_int, check_planar, resolve_device, stage_planar

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


# ---- the membrane solve ------------------------------------------------------------------------------------------------------------------------

GUESSES = ("smooth", "zero")


def default_max_iter(h, w):
    """The cap on conjugate-gradient steps when ``max_iter`` is None: 12 (h + w) + 200.  The step count of this problem grows with the graph distance an
    unknown pixel can have from the known ones, which h + w bounds on a full grid; the counts measured on the device ("Membrane solve") stay
    below 3 (h + w) for every mask kind of the tests, a single known pixel in the whole image included, at tol 1e-9."""
    return 12 * (int(h) + int(w)) + 200


def _check_solver(who, tol, max_iter, check_every, guess):
    """The solver's options, before any device is looked at: (tol, max_iter or None, check_every or None)."""
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.floating, np.integer)) or not math.isfinite(float(tol)) or float(tol) <= 0.0:
        raise ValueError(f"{who}: tol must be a finite positive number, got {tol!r}")
    counts = []
    for name, v in (("max_iter", max_iter), ("check_every", check_every)):
        n = None if v is None else as_int(v)
        if v is not None and (n is None or n < 1 or n > 2 ** 31 - 1):
            raise ValueError(f"{who}: {name} must be None or a positive integer, got {v!r}")
        counts.append(n)
    if guess not in GUESSES:
        raise ValueError(f"{who}: guess must be one of {GUESSES}, got {guess!r}")
    return float(tol), counts[0], counts[1]


def _check_same_mask(who, name, m, valid):
    if m is None:
        return
    if not isinstance(m, (np.ndarray, torch.Tensor)) or str(m.dtype).replace("torch.", "") not in ("uint8", "bool"):
        raise ValueError(f"{who}: {name} must be a uint8 or bool numpy array or torch tensor, got {getattr(m, 'dtype', type(m).__name__)}")
    if tuple(m.shape) != tuple(valid.shape):
        raise ValueError(f"{who}: {name} of shape {tuple(m.shape)} for a mask of shape {tuple(valid.shape)}")


def _reached(known, domain):
    """bool [B, h, w]: the pixels of ``domain`` whose 4-connected component holds a known pixel -- the labelling of hip_ext.masks and one flag per label,
    scattered and gathered on the device; nothing is read back."""
    from . import masks as _masks
    B, h, w = known.shape
    labels = _masks.connected_components(domain.to(torch.uint8), connectivity=4, stats=False).labels.reshape(B, -1).long()
    flags = torch.zeros((B, h * w + 1), dtype=torch.uint8, device=known.device)
    flags.scatter_reduce_(1, labels, known.reshape(B, -1).to(torch.uint8), "amax", include_self=True)
    flags[:, 0] = 0      # label 0 is what lies outside the domain
    return flags.gather(1, labels).reshape(B, h, w).bool()


def _membrane(who, planes, known, domain, minus, empty, tol, max_iter, check_every, guess):
    """The solve behind fill_harmonic and blend_seamless on staged tensors: planes fp32 [B, C, h, w], known / domain bool [B, h, w] (domain may be None),
    minus fp32 like planes or None (then also added back).  Returns (out fp32, unreached bool [B, h, w], (residual, iterations, converged) [B, C])."""
    B, C, h, w = planes.shape
    device = planes.device
    if domain is None:
        domain = torch.ones((B, h, w), dtype=torch.bool, device=device)
    known = known & domain
    reached = _reached(known, domain)
    k8, d8 = known.to(torch.uint8), reached.to(torch.uint8)      # an unreached component is a singular block: it stays out of the solve
    start = None
    if guess == "smooth":
        start = torch.empty_like(planes)
        data = planes if minus is None else torch.where(known[:, None], planes - minus, 0.0)
        push_pull(data.contiguous(), k8, start, 0.0)
    cap = default_max_iter(h, w) if max_iter is None else max_iter
    ws = torch.empty((membrane_workspace_bytes(B, C, h, w) + 7) // 8, dtype=torch.int64, device=device)
    membrane_begin(planes, k8, ws, domain=d8, guess=start, minus=minus, tol=tol)
    if check_every is None:
        membrane_iterate(planes, ws, cap)
    else:
        frozen = torch.empty(B * C, dtype=torch.uint8, device=device)
        done = 0
        while done < cap:
            n = min(check_every, cap - done)
            membrane_iterate(planes, ws, n, frozen=frozen)
            done += n
            if bool(frozen.cpu().all()):      # the one small copy; frozen planes do not change, so stopping here changes no byte
                break
    out = torch.empty_like(planes)
    residual = torch.empty(B * C, dtype=torch.float64, device=device)
    iterations = torch.empty(B * C, dtype=torch.int32, device=device)
    converged = torch.empty(B * C, dtype=torch.uint8, device=device)
    membrane_end(planes, ws, residual, iterations, converged, out=out, plus=minus)
    unreached = domain & ~reached & ~known
    fill = torch.full_like(planes, empty) if minus is None else (minus.double() + empty).float()
    out = torch.where(unreached[:, None], fill, out)
    return out, unreached, (residual.view(B, C), iterations.view(B, C), converged.view(B, C))


def _restore_clamped(planes, layout, single, as_u8):
    if as_u8:
        planes = planes.clamp(0.0, 255.0)      # a cloned gradient may leave the range of a byte
    return _restore(planes, layout, single, as_u8)


def _info(info, layout, single):
    if layout == "planar":
        return tuple(t[0, 0] if single else t[:, 0] for t in info)
    return tuple(t[0] if single and layout == "hwc" else t for t in info)


def _stage_mask(who, m, device, name):
    return None if m is None else (stage_planar(who, m, device, name).contiguous() != 0)


@torch.no_grad()
def fill_harmonic(x, valid, domain=None, empty=0.0, tol=1e-9, max_iter=None, check_every=None, guess="smooth", return_info=False, device=None):
    """x with every pixel of ``domain`` that is not valid replaced by the harmonic extension of the valid ones: u_p = the mean of u over the 4-neighbours
    of p that lie in the domain (an edge that leaves the image or the domain does not exist), by conjugate gradients in fp64, rounded to fp32 once.
    ``domain`` (a mask like ``valid``; None: every pixel) bounds what is filled and what a value may flow through; valid pixels and pixels outside the
    domain keep x bit for bit, and ``valid`` counts only inside the domain.  A 4-connected component of the domain without a valid pixel takes ``empty``.
    What lies under a pixel that is not valid, NaN and inf included, never reaches a result.

    ``tol``: the max norm of the residual, in the units of x, at which a plane stops.  ``max_iter``: the cap on steps (None: default_max_iter(h, w)).
    ``check_every=None`` issues exactly the cap's launches whatever the data (no host read; legal inside a stream capture; planes that are done idle);
    ``check_every=N`` reads the planes' done flags every N steps and stops issuing once all are set -- the same bytes either way.  ``guess``: 'smooth'
    starts from fill_smooth's values, 'zero' from 0.  ``return_info=True`` adds (residual fp64, iterations int32, converged uint8) per plane, on the
    device: the true residual's max norm, the steps taken, and whether the residual is within tol."""
    who = "fill_harmonic"
    single = _check_valid(who, valid)
    layout = _layout(who, x, valid.shape)
    _check_same_mask(who, "domain", domain, valid)
    tol, max_iter, check_every = _check_solver(who, tol, max_iter, check_every, guess)
    empty = float(empty)
    device = resolve_device(who, device, x, valid)
    as_u8 = str(x.dtype).endswith("uint8")
    with torch.cuda.device(device):
        known = _stage_mask(who, valid, device, "valid")
        dom = _stage_mask(who, domain, device, "domain")
        planes = _stage_planes(who, x, layout, device)
        out, _, info = _membrane(who, planes, known, dom, None, empty, tol, max_iter, check_every, guess)
        out = _restore_clamped(out, layout, single, as_u8)
    return (out, _info(info, layout, single)) if return_info else out


@torch.no_grad()
def blend_seamless(src, dst, mask, known=None, domain=None, tol=1e-9, max_iter=None, check_every=None, guess="smooth", return_info=False, device=None):
    """``src`` cloned into ``dst`` inside ``mask`` without a seam (Perez et al.'s cloning in its membrane form): the result is src + c, where the correction
    c is the harmonic extension of dst - src from the known pixels, so inside the mask it has src's gradients and on the known pixels it meets dst.  By
    default every pixel outside ``mask`` is known.  With ``known`` (a mask) only those pixels pin the correction, and ``domain`` (default mask | known)
    bounds where it may flow; it is met with mask | known.  Known pixels and pixels outside mask | known carry dst bit for bit; a part of the mask that no
    known pixel reaches takes c = 0, the plain paste.  The difference and the sum are formed in fp64 inside the solve.  src and dst: one shape and type,
    any input kind of fill_harmonic; the solver's options are fill_harmonic's."""
    who = "blend_seamless"
    single = _check_valid(who, mask)
    layout = _layout(who, dst, mask.shape)
    if not isinstance(src, (np.ndarray, torch.Tensor)) or tuple(src.shape) != tuple(dst.shape) or str(src.dtype).replace("torch.", "") != str(dst.dtype).replace("torch.", ""):
        raise ValueError(f"{who}: src must have dst's shape {tuple(dst.shape)} and type {dst.dtype}, got {tuple(getattr(src, 'shape', ()))} "
                         f"{getattr(src, 'dtype', type(src).__name__)}")
    _check_same_mask(who, "known", known, mask)
    _check_same_mask(who, "domain", domain, mask)
    tol, max_iter, check_every = _check_solver(who, tol, max_iter, check_every, guess)
    device = resolve_device(who, device, dst, src, mask)
    as_u8 = str(dst.dtype).endswith("uint8")
    with torch.cuda.device(device):
        m = _stage_mask(who, mask, device, "mask")
        k = ~m if known is None else _stage_mask(who, known, device, "known")
        d = (m | k) if domain is None else (_stage_mask(who, domain, device, "domain") & (m | k))
        s, t = _stage_planes(who, src, layout, device), _stage_planes(who, dst, layout, device)
        out, _, info = _membrane(who, t, k, d, s, 0.0, tol, max_iter, check_every, guess)
        out = _restore_clamped(out, layout, single, as_u8)
    return (out, _info(info, layout, single)) if return_info else out


__all__ = ["nearest_valid", "fill_nearest", "fill_smooth", "fill_harmonic", "blend_seamless", "default_max_iter", "HipExtError"]
