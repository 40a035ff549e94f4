"""Rank filters on the device: the windowed order statistic of the valid samples -- median, minimum (erosion), maximum (dilation), integer percents
(csrc/ada_filters.hip; the contract is include/ada_hip.h's "Rank filters" section, restated in numpy by tests/_filters_ref.py).  The reference has no
such operation: its median_filter_blend (app.py:267, infer.py:30) runs cv2.blur, and callers who wanted a median went to the host and to scipy.

A window is ``size`` x ``size`` or (kh, kw), both odd.  Borders: 'mirror' (reflect-101: scipy's 'mirror', cv2's default), 'nearest' (clamp: scipy's
'nearest', the border of cv2's median) and 'ignore' (positions outside the image do not vote).  ``valid`` (uint8 / bool, x's shape) lets only its
non-zero samples vote, and an fp32 NaN never votes -- a filter for maps with holes.  Where nothing votes the output is ``fill`` (NaN for fp32, 0 for
uint8 by default).  The output is always one of the input values; with every sample voting, median_filter is scipy.ndimage.median_filter.

Maps are fp32 or uint8 [h, w] or [B, h, w], a numpy array (copied to the device) or a device tensor; [h, w] in gives [h, w] out.  There is no CPU
fallback: a CPU tensor or a non-HIP target raises HipExtError.  Nothing is read back.
"""
from __future__ import annotations

import torch

from . import (BORDER_IGNORE, BORDER_MIRROR, BORDER_NEAREST, FILTER_MAX_EXTREME, FILTER_MAX_WINDOW, RANK_MAX, RANK_MEDIAN, RANK_MIN, HipExtError,
               extreme_filter_fwd, rank_filter_fwd)
from ._staging import as_int, check_planar, resolve_device, stage_planar

_BORDERS = {"mirror": BORDER_MIRROR, "nearest": BORDER_NEAREST, "ignore": BORDER_IGNORE}
_RANKS = {"min": RANK_MIN, "median": RANK_MEDIAN, "max": RANK_MAX}


def _window(who, size):
    """(kh, kw) of ``size``: an odd positive integer or a pair of them."""
    pair = (size, size) if as_int(size) is not None else size
    try:
        kh, kw = (as_int(v) for v in pair)
    except (TypeError, ValueError):
        kh = kw = None
    if kh is None or kw is None or kh < 1 or kw < 1 or kh % 2 == 0 or kw % 2 == 0:
        raise ValueError(f"{who}: size must be an odd positive integer or a pair (kh, kw) of them, got {size!r}")
    return kh, kw


def _rank(who, rank):
    if isinstance(rank, str):
        if rank not in _RANKS:
            raise ValueError(f"{who}: rank must be 'min', 'median', 'max' or an integer percent 0 .. 100, got {rank!r}")
        return _RANKS[rank]
    p = as_int(rank)
    if p is None or not 0 <= p <= 100:
        raise ValueError(f"{who}: rank must be 'min', 'median', 'max' or an integer percent 0 .. 100, got {rank!r}")
    return p


def _planar(who, x, dtypes, name):
    """check_planar, a wrong dtype reported as the device layer reports it: HipExtError, since no kernel exists for it."""
    if hasattr(x, "dtype") and hasattr(x, "ndim"):
        names = [str(d).replace("torch.", "") for d in dtypes]
        if str(x.dtype).replace("torch.", "") not in names:
            raise HipExtError(f"{who}: {name}: expected {' or '.join(names)}, got {x.dtype} (the HIP path has kernels for these types only)")
    return check_planar(who, x, dtypes, f"{name}: expected")


def _check_call(who, x, size, rank, border, valid, fill):
    """Everything of a call that needs no device: (kh, kw, rank code, border code, fill, whether x is [h, w]).  The extremes take the separable
    kernels and their limit; every other rank takes the general kernel's."""
    single = _planar(who, x, (torch.float32, torch.uint8), "x")
    kh, kw = _window(who, size)
    code = _rank(who, rank)
    if border not in _BORDERS:
        raise ValueError(f"{who}: border must be 'mirror', 'nearest' or 'ignore', got {border!r}")
    if code in (RANK_MIN, RANK_MAX):
        if max(kh, kw) > FILTER_MAX_EXTREME:
            raise ValueError(f"{who}: a minimum / maximum window holds at most {FILTER_MAX_EXTREME} samples on a side, got {kh} x {kw}")
    elif kh * kw > FILTER_MAX_WINDOW:
        raise ValueError(f"{who}: a median / percent window holds at most {FILTER_MAX_WINDOW} samples (9 x 9, 3 x 27, ...), got {kh} x {kw}")
    if valid is not None:
        _planar(who, valid, (torch.uint8, torch.bool), "valid")
        if tuple(valid.shape) != tuple(x.shape):
            raise ValueError(f"{who}: valid of shape {tuple(valid.shape)} for x of shape {tuple(x.shape)}")
    is_u8 = str(x.dtype).endswith("uint8")
    if fill is None:
        fill = 0 if is_u8 else float("nan")
    elif is_u8:
        if as_int(fill) is None or not 0 <= as_int(fill) <= 255:
            raise ValueError(f"{who}: the fill of a uint8 map must be an integer in 0 .. 255, got {fill!r}")
    else:
        fill = float(fill)
    return kh, kw, code, _BORDERS[border], fill, single


@torch.no_grad()
def rank_filter(x, size, rank="median", border="mirror", valid=None, fill=None, return_count=False, device=None):
    """The ``rank``-th order statistic of the valid samples of every window: of the n voting samples sorted ascending, 'min' takes s[0], 'max' s[n - 1],
    'median' s[n // 2] (scipy's upper median) and an integer percent p takes s[p (n - 1) // 100].  x fp32 or uint8 [h, w] / [B, h, w]; the result has
    x's type and shape.  ``return_count=True`` also returns n, int32 of x's shape.  Limits: kh kw <= 81 for 'median' and percents, kh, kw <= 63 for
    'min' / 'max' (which run separably, rows then columns)."""
    who = "rank_filter"
    kh, kw, code, bcode, fill, single = _check_call(who, x, size, rank, border, valid, fill)
    device = resolve_device(who, device, x, valid)
    with torch.cuda.device(device):
        xs = stage_planar(who, x, device, "x").contiguous()      # these kernels take no pitch
        vs = None if valid is None else stage_planar(who, valid, device, "valid").contiguous()
        out = torch.empty_like(xs)
        count = torch.empty(xs.shape, dtype=torch.int32, device=device) if return_count else None
        run = extreme_filter_fwd if code in (RANK_MIN, RANK_MAX) else rank_filter_fwd
        run(xs, kh, kw, code, bcode, out, valid=vs, fill=fill, count=count)
    if single:
        out, count = out[0], (count[0] if return_count else None)
    return (out, count) if return_count else out


def median_filter(x, size, border="mirror", valid=None, fill=None, return_count=False, device=None):
    """rank_filter(rank='median'): scipy.ndimage.median_filter(x, size, mode=border) when every sample votes."""
    return rank_filter(x, size, "median", border, valid, fill, return_count, device)


def minimum_filter(x, size, border="mirror", valid=None, fill=None, return_count=False, device=None):
    """rank_filter(rank='min'), separably; with border='ignore' grey erosion by a rectangle, the image's outside never lowering a result."""
    return rank_filter(x, size, "min", border, valid, fill, return_count, device)


def maximum_filter(x, size, border="mirror", valid=None, fill=None, return_count=False, device=None):
    """rank_filter(rank='max'), separably; with border='ignore' grey dilation by a rectangle."""
    return rank_filter(x, size, "max", border, valid, fill, return_count, device)


__all__ = ["rank_filter", "median_filter", "minimum_filter", "maximum_filter", "HipExtError"]
