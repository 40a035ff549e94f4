"""What the reference's demo (app.py) does to a MASK before the networks see it, on the device: connected components, their statistics, the area
filter of ``remove_small_noise`` (app.py:283-293) and the prompt points of ``get_points_from_components`` (app.py:77-99).  The reference runs
cv2.connectedComponents / connectedComponentsWithStats on the host; here the mask never leaves HBM (csrc/ada_masks.hip).

Morphology by a square: ``erode`` / ``dilate`` / ``opening`` / ``closing`` (cv2.erode, cv2.dilate, MORPH_OPEN, MORPH_CLOSE with their default border, under
which the image's outside never decides a pixel) are the separable minimum / maximum of csrc/ada_filters.hip, and ``invisible_mask`` is the chain the
reference's demo applies to ``whole & ~visible`` (app.py:207-211).

Numbering: components are numbered 1 .. n in the raster order of their first pixels (scipy.ndimage.label's numbering).  OpenCV does not document
its numbering, so label-for-label equality with cv2 is not claimed; the cleaned mask and the set of points per component do not depend on it.

Masks are taken as hip_ext.image.masks_to_tensor takes them: uint8 or bool, [h, w] or [K, h, w], a numpy array (copied to the device) or a device
tensor (a pitched view -- a crop of a larger tensor -- is read in place).  There is no CPU fallback: a CPU tensor or a non-HIP target raises HipExtError.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import (BORDER_IGNORE, FILTER_MAX_EXTREME, RANK_MAX, RANK_MIN, extreme_filter_fwd, extreme_filter_workspace_bytes, mask_grid_points,
               mask_keep_area, mask_label, mask_stats)
from ._staging import as_int, check_planar, resolve_device, stage_planar

Components = namedtuple("Components", "labels count stats centroids")
Components.__doc__ = """Device tensors of connected_components: labels int32 [K, h, w] (0 = background), count int32 [K] (components per mask), stats int32
[K, cap + 1, 5] in cv2's column order (LEFT, TOP, WIDTH, HEIGHT, AREA; row 0 = background, rows without pixels are zero), centroids fp64 [K, cap + 1, 2] =
(sum x, sum y) / area in cv2's (x, y) order, NaN for rows without pixels.  stats / centroids are None with stats=False."""


def _connectivity(who, connectivity):
    c = as_int(connectivity)
    if c not in (4, 8):
        raise ValueError(f"{who}: connectivity must be 4 or 8, got {connectivity!r}")
    return c


def _non_negative(who, name, v, least=0):
    i = as_int(v)
    if i is None or i < least or i >= 2 ** 31:
        raise ValueError(f"{who}: {name} must be an integer >= {least}, got {v!r}")
    return i


def _stage(masks, device, who):
    """The checked masks as (uint8 device tensor [K, h, w] with packed rows, device): masks_to_tensor's staging and errors."""
    check_planar(who, masks, (torch.uint8, torch.bool))
    device = resolve_device(who, device, masks)
    return stage_planar(who, masks, device, "masks"), device


def _label(src, connectivity):
    K, h, w = src.shape
    labels = torch.empty(K, h, w, dtype=torch.int32, device=src.device)
    count = torch.empty(K, dtype=torch.int32, device=src.device)
    mask_label(src, K, h, w, src.stride(1), src.stride(0), connectivity, labels, count)
    return labels, count


def _stats(labels, cap):
    K = labels.shape[0]
    stats = torch.empty(K, cap + 1, 5, dtype=torch.int32, device=labels.device)
    sums = torch.empty(K, cap + 1, 2, dtype=torch.int64, device=labels.device)
    mask_stats(labels, cap, stats, sums)
    return stats, sums


@torch.no_grad()
def connected_components(masks, connectivity=8, stats=True, max_labels=None, device=None) -> Components:
    """cv2.connectedComponentsWithStats on the device (the numbering: module docstring).  ``max_labels=None``: the component counts are read back once
    and the statistics are sized exactly (cap = the largest count).  An explicit ``max_labels`` is the capacity: no host read, components numbered
    above it are left out of the statistics, and ``count > max_labels`` is how the caller sees that.  ``stats=False``: labels and count only, no host read."""
    who = "connected_components"
    connectivity = _connectivity(who, connectivity)
    cap = None if max_labels is None else _non_negative(who, "max_labels", max_labels)
    src, device = _stage(masks, device, who)
    with torch.cuda.device(device):
        labels, count = _label(src, connectivity)
        if not stats:
            return Components(labels, count, None, None)
        if cap is None:
            cap = int(count.max().item())
        st, sums = _stats(labels, cap)
        centroids = sums.double() / st[:, :, 4:5].double()      # 0 / 0 = NaN for rows without pixels
    return Components(labels, count, st, centroids)


@torch.no_grad()
def remove_small_noise(masks, min_area=500, connectivity=4, device=None) -> torch.Tensor:
    """The reference's remove_small_noise (app.py:283-293): uint8 0 / 1 [K, h, w] on the device, the pixels of the components of at least ``min_area``
    pixels (``area >= min_area``).  Exact for any number of components; nothing is read back to the host."""
    who = "remove_small_noise"
    connectivity = _connectivity(who, connectivity)
    min_area = _non_negative(who, "min_area", min_area)
    src, device = _stage(masks, device, who)
    with torch.cuda.device(device):
        labels, _ = _label(src, connectivity)
        out = torch.empty(labels.shape, dtype=torch.uint8, device=device)
        mask_keep_area(labels, min_area, out_u8=out)
    return out


@torch.no_grad()
def points_from_components(masks, small_component_thresh=100, grid_step=10, connectivity=8, device=None) -> list:
    """The reference's get_points_from_components (app.py:77-99): per mask an int32 [P, 2] device tensor of (x, y) prompt points, component by
    component in label order.  A component of fewer than ``small_component_thresh`` pixels gives (sum x // area, sum y // area); a larger one gives the
    points of the grid range(top, bottom, grid_step) x range(left, right, grid_step) of its bounding box that lie inside it, in raster order -- the ranges
    exclude the box's last row and column, as the reference's do, so a large component one pixel wide gives none.  [0, 2] stands for the reference's
    empty array.

    The integer quotient equals the reference's int(centroid), the truncated double s / a: s and a are integers below 2^40.  When the exact quotient is
    not an integer it lies at least 1 / a below the next integer n, and half a unit in the last place of a double near n is at most n 2^-53; since
    a n <= s + a < 2^41, 1 / a > n 2^-53, so the correctly rounded quotient stays below n and truncates to the same integer.  A centroid may lie
    outside its component, as in the reference."""
    who = "points_from_components"
    connectivity = _connectivity(who, connectivity)
    thresh = _non_negative(who, "small_component_thresh", small_component_thresh)
    step = _non_negative(who, "grid_step", grid_step, least=1)
    src, device = _stage(masks, device, who)
    out = []
    with torch.cuda.device(device):
        labels, count = _label(src, connectivity)
        counts = count.tolist()
        st, sums = _stats(labels, max(counts))
        hit = torch.empty_like(labels)
        mask_grid_points(labels, st, thresh, step, hit)
        for k, n in enumerate(counts):
            area = st[k, 1:n + 1, 4].long()
            small = torch.nonzero(area < thresh)[:, 0]                     # label - 1, ascending
            small_pts = sums[k, 1:n + 1][small] // area[small, None]       # (x, y)
            yx = torch.nonzero(hit[k])                                     # raster order
            large_lab = hit[k][yx[:, 0], yx[:, 1]].long()
            keys = torch.cat([small + 1, large_lab])
            pts = torch.cat([small_pts, yx.flip(1)])
            order = torch.sort(keys, stable=True)[1]                       # by label; the grid points of one component keep their raster order
            out.append(pts[order].to(torch.int32).reshape(-1, 2))
    return out


def _square(who, size, iterations):
    k, it = as_int(size), as_int(iterations)
    if k is None or k < 1 or k % 2 == 0 or k > FILTER_MAX_EXTREME:
        raise ValueError(f"{who}: size must be an odd integer in 1 .. {FILTER_MAX_EXTREME}, got {size!r}")
    if it is None or it < 0:
        raise ValueError(f"{who}: iterations must be an integer >= 0, got {iterations!r}")
    return k, it


def _morph(who, masks, steps, size, iterations, device):
    """uint8 0 / 1 [K, h, w] (or [h, w]): the binarised masks after ``iterations`` minimum (RANK_MIN) or maximum (RANK_MAX) filters per entry of ``steps``
    by a size x size square under BORDER_IGNORE.  The passes ping-pong between two buffers and share one workspace."""
    k, it = _square(who, size, iterations)
    single = check_planar(who, masks, (torch.uint8, torch.bool))
    src, device = _stage(masks, device, who)
    with torch.cuda.device(device):
        cur = (src != 0).to(torch.uint8)      # non-zero counts as 1; a fresh packed buffer, the caller's mask is never written
        nxt = torch.empty_like(cur)
        ws = torch.empty((extreme_filter_workspace_bytes(*cur.shape) + 7) // 8, dtype=torch.int64, device=device)
        for rank in steps:
            for _ in range(it):
                extreme_filter_fwd(cur, k, k, rank, BORDER_IGNORE, nxt, workspace=ws)
                cur, nxt = nxt, cur
    return cur[0] if single else cur


@torch.no_grad()
def erode(masks, size=3, iterations=1, device=None) -> torch.Tensor:
    """cv2.erode(mask, ones((size, size)), iterations=iterations) with cv2's default border: uint8 0 / 1 on the device, 1 where every pixel of the
    size x size square that lies inside the image is non-zero (scipy's binary_erosion with border_value=1)."""
    return _morph("erode", masks, (RANK_MIN,), size, iterations, device)


@torch.no_grad()
def dilate(masks, size=3, iterations=1, device=None) -> torch.Tensor:
    """cv2.dilate(mask, ones((size, size)), iterations=iterations): uint8 0 / 1 on the device, 1 where any pixel of the square is non-zero (scipy's
    binary_dilation with border_value=0)."""
    return _morph("dilate", masks, (RANK_MAX,), size, iterations, device)


@torch.no_grad()
def opening(masks, size=3, iterations=1, device=None) -> torch.Tensor:
    """cv2.morphologyEx(mask, MORPH_OPEN, ones((size, size)), iterations=iterations): ``iterations`` erosions, then as many dilations.  Not scipy's
    binary_opening, whose erosion takes the image's outside as 0."""
    return _morph("opening", masks, (RANK_MIN, RANK_MAX), size, iterations, device)


@torch.no_grad()
def closing(masks, size=3, iterations=1, device=None) -> torch.Tensor:
    """cv2.morphologyEx(mask, MORPH_CLOSE, ones((size, size)), iterations=iterations): ``iterations`` dilations, then as many erosions -- pinholes and
    hairline gaps narrower than the square close.  Not scipy's binary_closing, whose erosion takes the image's outside as 0."""
    return _morph("closing", masks, (RANK_MAX, RANK_MIN), size, iterations, device)


@torch.no_grad()
def invisible_mask(visible, whole, min_area=None, erode=None, close=None, connectivity=4) -> torch.Tensor:
    """The occluded part of an object: ``whole & ~visible`` (the dataset's definition, sam_amodal_dataset.py:42), uint8 0 / 1 on the device, then the
    clean-up chain of the reference's demo (app.py:207-211) in its order: remove_small_noise(min_area, connectivity), erosion by an ``erode`` square,
    closing by a ``close`` square.  A step whose argument is None does not run.  visible, whole: masks of one shape, non-zero = set."""
    who = "invisible_mask"
    single = check_planar(who, whole, (torch.uint8, torch.bool))
    check_planar(who, visible, (torch.uint8, torch.bool))
    if tuple(visible.shape) != tuple(whole.shape):
        raise ValueError(f"{who}: visible {tuple(visible.shape)} and whole {tuple(whole.shape)} differ in shape")
    connectivity = _connectivity(who, connectivity)
    wh, device = _stage(whole, None, who)
    vis, _ = _stage(visible, device, who)
    with torch.cuda.device(device):
        out = ((wh != 0) & (vis == 0)).to(torch.uint8)
    if min_area is not None:
        out = remove_small_noise(out, min_area=min_area, connectivity=connectivity, device=device)
    if erode is not None:
        out = _morph(who, out, (RANK_MIN,), erode, 1, device)      # the argument shadows erode()
    if close is not None:
        out = _morph(who, out, (RANK_MAX, RANK_MIN), close, 1, device)
    return out[0] if single else out
