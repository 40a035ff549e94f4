"""Depth maps to geometry on the device: what the reference does on the host in numpy (src/models/amodalsynthdrive/zoedepth/utils/geometry.py:
get_intrinsics, depth_to_points, create_triangles) with the maps left in HBM (csrc/ada_geometry.hip), up to the layered meshes of an amodal result.

Meshes are also looked at here: render_mesh / render_meshes / render_layers rasterise them from a camera into a depth map, a colour image and a
map of the triangle and the mesh each pixel shows (csrc/ada_raster.hip).  The reference hands its meshes to a third-party renderer, so that arithmetic is
this library's own: include/ada_hip.h states it and tests/_raster_ref.py restates it in numpy.

Exact against the reference: the points of the default pose (R = None, t = None) for any pinhole K without skew, bit for bit in float64, and the
triangle list, order included (int32 here, int64 there).  A general pose differs from numpy's stacked matmul in the last ulps, within
2 gamma_4 (sum_j |R_ij| |q_j| + |t_i|) (include/ada_hip.h).  This library's own: the inverse-depth mode z = 1 / (a depth + b), vertex validity
(z finite and > 0), the ratio rule z_max <= max_ratio z_min of a kept triangle, the vertex compaction, and zero triangles for a grid one pixel wide
with a mask (the reference raises there).

Depth maps are fp32, [h, w] or [B, h, w], numpy arrays (copied to the device) or device tensors; masks are uint8 or bool as hip_ext.masks takes them
(a pitched crop of a larger tensor is read in place).  There is no CPU fallback: a CPU tensor or a non-HIP target raises HipExtError.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import (HipExtError, RASTER_OUT_NORMALISED, RASTER_OUT_W, RASTER_OUT_Z, depth_points, mesh_adaptive, mesh_adaptive_workspace_bytes, mesh_compact,
               mesh_project, mesh_raster, mesh_raster_workspace_bytes, mesh_triangles)
from . import inpaint as _inpaint
from . import masks as _masks
from ._staging import as_int, check_planar, from_numpy, resolve_device, stage_planar

Mesh = namedtuple("Mesh", "points triangles vertex_count triangle_count colors")
Mesh.__doc__ = """One image's mesh on the device: points [vertex_count, 3] (fp32 or fp64), triangles int32 [triangle_count, 3] indexing them, the two counts as
Python ints, colors uint8 [vertex_count, 3] (R, G, B) or None."""

Layers = namedtuple("Layers", "scene objects")
Layers.__doc__ = """amodal_layers: the scene Mesh (the base depth over every pixel) and a list of K object Meshes (each blended map over its amodal mask)."""

View = namedtuple("View", "depth index owner color")
View.__doc__ = """A rendered view on the device: depth fp32 [h, w], index int32 [h, w] (the triangle each pixel shows, -1 for background), owner int32 [h, w]
(the position of that triangle's mesh among the rendered ones, -1 for background), color uint8 [h, w, 3] (R, G, B) or None."""

MAX_PIXELS = 2 ** 30


def get_intrinsics(h, w, fov_deg=55.0) -> np.ndarray:
    """The reference's pinhole camera as a float64 3 x 3: focal length 0.5 w / tan(fov / 2) on both axes, principal point (w / 2, h / 2)."""
    f = 0.5 * w / np.tan(0.5 * fov_deg * np.pi / 180.0)
    return np.array([[f, 0.0, 0.5 * w], [0.0, f, 0.5 * h], [0.0, 0.0, 1.0]], dtype=np.float64)


def _grid(who, h, w):
    hw = as_int(h), as_int(w)
    if None in hw or min(hw) < 1:
        raise ValueError(f"{who}: h and w must be positive integers, got {h!r} x {w!r}")
    if hw[0] * hw[1] >= MAX_PIXELS:
        raise ValueError(f"{who}: h * w must stay below 2^30, got {hw[0]} x {hw[1]}")
    return hw


def _check_planar(who, x, dtypes, name):
    """Shape and type of a depth or mask argument, before any device is looked at: whether it is [h, w]."""
    was2d = check_planar(who, x, dtypes, f"{name} must be")
    if not was2d and x.shape[0] > 65535:
        raise ValueError(f"{who}: {name}: at most 65535 per call, got {x.shape[0]}")
    return was2d


def _check_depth(who, depth):
    """(h, w, was_2d) of a checked depth argument."""
    was2d = _check_planar(who, depth, (torch.float32,), "depth")
    return _grid(who, depth.shape[-2], depth.shape[-1]) + (was2d,)


def _check_mask(who, mask):
    return _check_planar(who, mask, (torch.uint8, torch.bool), "mask")


def _stage_depth(who, depth, device):
    return stage_planar(who, depth, device, "depth").contiguous()      # the kernels take no pitch for a depth map


def _stage_mask(who, mask, device):
    """uint8 device tensor [B, h, w] whose rows are packed and whose pitches the kernel can walk: a crop stays a view."""
    return stage_planar(who, mask, device, "mask")


def _camera(who, h, w, R, t, K, fov_deg):
    K = get_intrinsics(h, w, fov_deg) if K is None else np.asarray(K, dtype=np.float64)
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64).reshape(-1)
    if K.shape != (3, 3) or R.shape != (3, 3) or t.shape != (3,):
        raise ValueError(f"{who}: K and R must be 3 x 3 and t must hold 3 values, got {K.shape}, {R.shape}, {t.shape}")
    return list(np.linalg.inv(K).reshape(-1)) + list(R.reshape(-1)) + list(t)


def _inverse(who, inverse):
    if inverse is None:
        return None
    try:
        a, b = (float(v) for v in inverse)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: inverse must be None or a pair (a, b), got {inverse!r}") from None
    return a, b


def _ratio(who, max_ratio, depth):
    if max_ratio is None:
        return 0.0
    r = float(max_ratio)
    if r != r:
        raise ValueError(f"{who}: max_ratio is NaN")
    if r > 0 and depth is None:
        raise ValueError(f"{who}: max_ratio needs the depth map")
    return r


@torch.no_grad()
def depth_to_points(depth, R=None, t=None, K=None, fov_deg=55.0, inverse=None, dtype=torch.float64, return_valid=False, device=None):
    """The reference's depth_to_points on the device: depth fp32 [h, w] or [B, h, w] -> points [h, w, 3] / [B, h, w, 3] of ``dtype`` (torch.float64, the
    reference's, or torch.float32 = the float64 result rounded once).  K defaults to get_intrinsics(h, w, fov_deg); its inverse is taken with
    np.linalg.inv in float64, as the reference takes it.  ``inverse=(a, b)``: z = 1 / (a depth + b) instead of z = depth.  A vertex whose z is not finite
    is NaN in all three coordinates; ``return_valid=True`` also returns uint8 [.., h, w], 1 where z is finite and > 0.  Nothing is read back."""
    who = "depth_to_points"
    h, w, was2d = _check_depth(who, depth)
    if dtype not in (torch.float64, torch.float32):
        raise ValueError(f"{who}: dtype must be torch.float64 or torch.float32, got {dtype!r}")
    cam = _camera(who, h, w, R, t, K, fov_deg)
    inverse = _inverse(who, inverse)
    device = resolve_device(who, device, depth)
    with torch.cuda.device(device):
        d = _stage_depth(who, depth, device)
        out = torch.empty(d.shape + (3,), dtype=dtype, device=device)
        valid = torch.empty(d.shape, dtype=torch.uint8, device=device) if return_valid else None
        depth_points(d, cam, out_f64=out if dtype == torch.float64 else None, out_f32=out if dtype == torch.float32 else None, valid=valid, inverse=inverse)
    if was2d:
        out, valid = out[0], (valid[0] if return_valid else None)
    return (out, valid) if return_valid else out


def _triangles(B, h, w, m, d, inverse, ratio, capacity, device):
    tri = torch.empty(B, capacity, 3, dtype=torch.int32, device=device)
    count = torch.empty(B, dtype=torch.int32, device=device)
    mesh_triangles(B, h, w, tri, count, mask=m, row_pitch=0 if m is None else m.stride(1), image_stride=0 if m is None else m.stride(0), depth=d,
                   inverse=inverse, max_ratio=ratio)
    return tri, count


@torch.no_grad()
def create_triangles(h, w, mask=None, depth=None, inverse=None, max_ratio=None, capacity=None, device=None):
    """The reference's create_triangles on the device: of the two triangles per pixel cell, (tl, bl, tr) then (br, tr, bl) in raster order, those whose
    three vertices are all inside ``mask`` (None: every vertex).  With ``depth`` (fp32, the mask's shape) the three must also be valid vertices
    (z finite and > 0, ``inverse`` as in depth_to_points), and with ``max_ratio`` > 0 additionally z_max <= max_ratio z_min -- this library's cut
    of the sheet of stretched triangles that would join an occluder to what lies behind it.  A grid one pixel wide has no triangle.

    ``capacity=None``: the counts are read back once (the one host read) and the result is a list of exactly sized int32 [n_b, 3] device tensors, or
    one tensor when the mask (or, without one, the depth) is 2-D or both are None.  An explicit ``capacity``: (triangles int32 [B, capacity, 3],
    count int32 [B]) with no host read; the first min(count, capacity) rows are filled and count > capacity is how the caller sees an overflow."""
    who = "create_triangles"
    h, w = _grid(who, h, w)
    cap = None
    if capacity is not None:
        cap = as_int(capacity)
        if cap is None or cap < 0 or cap >= 2 ** 31:
            raise ValueError(f"{who}: capacity must be an integer >= 0, got {capacity!r}")
    single = True
    if mask is not None:
        single = _check_mask(who, mask)
        if tuple(mask.shape[-2:]) != (h, w):
            raise ValueError(f"{who}: mask of shape {tuple(mask.shape)} for a {h} x {w} grid")
    if depth is not None:
        dh, dw, d2 = _check_depth(who, depth)
        if (dh, dw) != (h, w):
            raise ValueError(f"{who}: depth of shape {tuple(depth.shape)} for a {h} x {w} grid")
        if mask is None:
            single = d2
        elif d2 != single or (not d2 and depth.shape[0] != mask.shape[0]):
            raise ValueError(f"{who}: mask {tuple(mask.shape)} and depth {tuple(depth.shape)} differ in shape")
    inverse = _inverse(who, inverse)
    ratio = _ratio(who, max_ratio, depth)
    device = resolve_device(who, device, mask, depth)
    with torch.cuda.device(device):
        m = None if mask is None else _stage_mask(who, mask, device)
        d = None if depth is None else _stage_depth(who, depth, device)
        B = m.shape[0] if m is not None else d.shape[0] if d is not None else 1
        if cap is not None:
            return _triangles(B, h, w, m, d, inverse, ratio, cap, device)
        counts = _triangles(B, h, w, m, d, inverse, ratio, 0, device)[1].tolist()      # the one host read
        tri = _triangles(B, h, w, m, d, inverse, ratio, max(counts), device)[0]
        out = [tri[b, :n] for b, n in enumerate(counts)]
    return out[0] if single else out


def _tolerance(who, max_error):
    if max_error is None:
        return None
    try:
        tau = float(max_error)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: max_error must be None or a number, got {max_error!r}") from None
    if not (0.0 <= tau < float("inf")):
        raise ValueError(f"{who}: max_error must be finite and >= 0, got {max_error!r}")
    return tau


@torch.no_grad()
def adaptive_triangles(depth, mask=None, inverse=None, max_ratio=None, max_error=0.01, capacity=None, return_error=False, device=None):
    """An adaptive triangle list over a depth map in place of create_triangles' two triangles per cell: a right-triangulated irregular network (the
    binary tree of right isosceles triangles of terrain meshes), refined until the relative error of the disparity at every hypotenuse midpoint is
    at most ``max_error`` -- the disparity is ``a depth + b`` with ``inverse=(a, b)`` and 1 / depth otherwise; a plane in space is linear in it.  The
    mesh is conforming (no T-junction, no crack), wound as create_triangles winds, indexes the same h w vertices (so it feeds mesh_compact and
    render_mesh unchanged) and keeps only triangles whose finest cover passes create_triangles' tests: inside ``mask``, z finite and > 0,
    z_max <= ``max_ratio`` z_min.  ``max_error=None``: the finest mesh, every such leaf.  Rows come in the tree's heap order, the same bytes every
    run; include/ada_hip.h has the contract.  A map whose sides are not 2^k + 1 is refined along its right and bottom borders (a 12 x 19 plane: 82
    triangles where a 17 x 17 one has 2): the tree spans the enclosing power-of-two square and the vertices outside the map force it.

    depth: fp32 [h, w] or [B, h, w], h, w >= 2, at most 16385 on a side; mask: uint8 / bool of that shape or None.  ``capacity=None``: the counts are
    read back once and the result is a list of exactly sized int32 [n_b, 3] device tensors, or one tensor for a 2-D depth.  An explicit ``capacity``:
    (triangles int32 [B, capacity, 3], count int32 [B]) with no host read, as create_triangles.  ``return_error=True`` appends the error map E, fp64
    [h, w] / [B, h, w] (+inf where a triangle must split whatever the tolerance): E depends on the tolerance not at all, so a sweep reuses it."""
    who = "adaptive_triangles"
    h, w, single = _check_depth(who, depth)
    if min(h, w) < 2:
        raise ValueError(f"{who}: h and w must be at least 2, got {h} x {w}")
    cap = None
    if capacity is not None:
        cap = as_int(capacity)
        if cap is None or cap < 0 or cap >= 2 ** 31:
            raise ValueError(f"{who}: capacity must be an integer >= 0, got {capacity!r}")
    if mask is not None:
        m2 = _check_mask(who, mask)
        if tuple(mask.shape) != tuple(depth.shape) or m2 != single:
            raise ValueError(f"{who}: mask {tuple(mask.shape)} and depth {tuple(depth.shape)} differ in shape")
    inverse = _inverse(who, inverse)
    ratio = _ratio(who, max_ratio, depth)
    tau = _tolerance(who, max_error)
    device = resolve_device(who, device, depth, mask)
    with torch.cuda.device(device):
        m = None if mask is None else _stage_mask(who, mask, device)
        d = _stage_depth(who, depth, device)
        B = d.shape[0]
        ws = torch.empty((mesh_adaptive_workspace_bytes(h, w) + 15) // 16 * 2, dtype=torch.int64, device=device)
        count = torch.empty(B, dtype=torch.int32, device=device)
        kw = dict(mask=m, row_pitch=0 if m is None else m.stride(1), image_stride=0 if m is None else m.stride(0), inverse=inverse, max_ratio=ratio,
                  max_error=tau, workspace=ws)
        if cap is not None:
            tri = torch.empty(B, cap, 3, dtype=torch.int32, device=device)
            err = torch.empty(B, h, w, dtype=torch.float64, device=device) if return_error else None
            mesh_adaptive(B, h, w, d, tri, count, error=err, **kw)
            return (tri, count, err) if return_error else (tri, count)
        err = torch.empty(B, h, w, dtype=torch.float64, device=device) if tau is not None or return_error else None      # the finest mesh needs no E
        mesh_adaptive(B, h, w, d, torch.empty(B, 0, 3, dtype=torch.int32, device=device), count, error=err, **kw)
        counts = count.tolist()      # the one host read
        tri = torch.empty(B, max(counts), 3, dtype=torch.int32, device=device)
        mesh_adaptive(B, h, w, d, tri, count, error=err, error_ready=err is not None, **kw)      # the error map is the first call's
        out = [tri[b, :n] for b, n in enumerate(counts)]
    out = out[0] if single else out
    return (out, err[0] if single else err) if return_error else out


def _stage_colors(who, colors, h, w, device):
    if colors is None:
        return None
    if isinstance(colors, np.ndarray):
        colors = from_numpy(colors).to(device)
    if not isinstance(colors, torch.Tensor) or colors.dtype != torch.uint8 or tuple(colors.shape) != (h, w, 3):
        raise ValueError(f"{who}: colors must be uint8 [{h}, {w}, 3], got {getattr(colors, 'dtype', type(colors).__name__)} {tuple(getattr(colors, 'shape', ()))}")
    if colors.device != device:
        raise HipExtError(f"{who}: colors on {colors.device}, expected them on the HIP device {device}")
    return colors.contiguous().reshape(1, h * w, 3)


@torch.no_grad()
def depth_to_mesh(depth, mask=None, colors=None, compact=True, R=None, t=None, K=None, fov_deg=55.0, inverse=None, max_ratio=None,
                  dtype=torch.float32, max_error=None, median=None, device=None) -> Mesh:
    """One depth map fp32 [h, w] -> a Mesh: depth_to_points, then create_triangles over ``mask`` (uint8 / bool [h, w] or None) with the validity and ratio
    rules applied from the same map.  ``colors``: uint8 [h, w, 3] per vertex, or None.  ``compact=True`` keeps only the vertices a triangle uses, in
    raster order, and renumbers the triangles; False keeps all h w points (invalid ones NaN or behind the camera, used by no triangle).
    ``max_error``: None is create_triangles' two triangles per cell; a number takes adaptive_triangles' mesh for that tolerance on the relative disparity
    error instead (h, w >= 2) -- far fewer triangles over flat ground, the same cover, and with compact only the vertices it uses.
    ``median``: None, or an odd window K (or (kh, kw)) -- the depth inside the mask is first replaced by
    hip_ext.filters.median_filter(depth, K, border='nearest', valid=mask), the remedy for the flying pixels of an occlusion border, which the ratio
    rule cuts into holes but which otherwise stand as spikes; only samples inside the mask vote, pixels outside it keep their own value, and points and
    triangles (regular or adaptive) are built from the filtered map.
    Host reads: the triangle count, and with compact the vertex count."""
    who = "depth_to_mesh"
    h, w, was2d = _check_depth(who, depth)
    if not was2d:
        raise ValueError(f"{who}: one map [h, w] per call, got shape {tuple(depth.shape)}")
    if mask is not None and (not _check_mask(who, mask) or tuple(mask.shape) != (h, w)):
        raise ValueError(f"{who}: mask must be [{h}, {w}], got shape {tuple(mask.shape)}")
    device = resolve_device(who, device, depth, mask)
    with torch.cuda.device(device):
        d = _stage_depth(who, depth, device)[0]
        if median is not None:
            from .filters import median_filter
            m = None if mask is None else _stage_mask(who, mask, device)[0]
            filtered = median_filter(d, median, border="nearest", valid=m, device=device)
            d = filtered if m is None else torch.where(m != 0, filtered, d)
        col = _stage_colors(who, colors, h, w, device)
        points = depth_to_points(d, R=R, t=t, K=K, fov_deg=fov_deg, inverse=inverse, dtype=dtype, device=device).reshape(1, h * w, 3)
        if max_error is None:
            tri = create_triangles(h, w, mask=mask, depth=d, inverse=inverse, max_ratio=max_ratio, device=device)
        else:
            tri = adaptive_triangles(d, mask=mask, inverse=inverse, max_ratio=max_ratio, max_error=max_error, device=device)
        n_tri = tri.shape[0]
        if not compact:
            return Mesh(points[0], tri, h * w, n_tri, None if col is None else col[0])
        tri = tri.contiguous()[None]
        count = torch.full((1,), n_tri, dtype=torch.int32, device=device)
        vcap = min(h * w, 3 * n_tri)
        p_out = torch.empty(1, vcap, 3, dtype=dtype, device=device)
        c_out = None if col is None else torch.empty(1, vcap, 3, dtype=torch.uint8, device=device)
        v_count = torch.empty(1, dtype=torch.int32, device=device)
        mesh_compact(tri, count, h, w, points, p_out, v_count, colors=col, colors_out=c_out)
        n_v = int(v_count.item())
    return Mesh(p_out[0, :n_v], tri[0], n_v, n_tri, None if c_out is None else c_out[0, :n_v])


@torch.no_grad()
def amodal_layers(result, image=None, near=1.0, far=10.0, fov_deg=55.0, max_ratio=None, max_error=None, median=None) -> Layers:
    """The layered geometry of an AmodalResult (hip_ext.pipeline.amodal_infer_image): the scene Mesh from ``result.base`` over every pixel and one Mesh per
    object from ``result.blended[k]`` over ``result.masks[k] > 0`` -- the occluded object reconstructed behind its occluder.

    The maps are normalised inverse depth in [0, 1]; this library's choice of metric is z = 1 / (a v + b) with a = 1 / near - 1 / far, b = 1 / far:
    v = 1 lies at ``near``, v = 0 at ``far``.  The reference fixes no such mapping.  With far = inf the pixel at v = 0 (``base`` contains one exactly) has
    no finite z: it is an invalid vertex and belongs to no triangle.  ``image``: the photo, uint8 [h, w, 3] in B, G, R order, brought to the maps' size by
    hip_ext.image.resize_nearest's rule, gives the vertex colours (stored R, G, B).  An all-zero mask gives an empty Mesh.  base and blended must have one
    size (call amodal_infer_image with the same out_size for both, its default).  ``max_error``: depth_to_mesh's, for every layer -- the error is then
    measured on the networks' own output, in which the disparity is linear.  ``median``: depth_to_mesh's, for every layer: each object's map is filtered
    among the samples of its own mask."""
    who = "amodal_layers"
    base, blended, masks = result.base, result.blended, result.masks
    for name, v in (("base", base), ("blended", blended), ("masks", masks)):
        if not isinstance(v, torch.Tensor) or not v.is_cuda:
            raise HipExtError(f"{who}: result.{name} must be a tensor on a HIP device (the HIP path has no CPU fallback)")
    if base.dim() != 2 or blended.dim() != 3 or tuple(blended.shape[1:]) != tuple(base.shape):
        raise ValueError(f"{who}: base [h, w] and blended [K, h, w] of one size expected, got {tuple(base.shape)} and {tuple(blended.shape)}")
    h, w = base.shape
    if not (near > 0 and far > near):
        raise ValueError(f"{who}: 0 < near < far expected, got near={near!r} far={far!r}")
    inverse = (1.0 / near - 1.0 / far, 1.0 / far)
    with torch.cuda.device(base.device):
        if tuple(masks.shape[1:]) != (h, w):
            from .image import resize_nearest
            masks = resize_nearest(masks.float().contiguous(), h, w)
        colors = None
        if image is not None:
            from .image import resize_nearest
            img = from_numpy(image) if isinstance(image, np.ndarray) else image
            if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] < 3:
                raise ValueError(f"{who}: image must be uint8 [h, w, 3] in B, G, R order")
            planes = img.to(base.device)[:, :, :3].permute(2, 0, 1).float().contiguous()
            colors = resize_nearest(planes, h, w).flip(0).permute(1, 2, 0).to(torch.uint8).contiguous()      # R, G, B
        kw = dict(colors=colors, fov_deg=fov_deg, inverse=inverse, max_ratio=max_ratio, max_error=max_error, median=median)
        scene = depth_to_mesh(base.float(), **kw)
        objects = [depth_to_mesh(blended[k].float(), mask=(masks[k] > 0), **kw) for k in range(blended.shape[0])]
    return Layers(scene, objects)


_OUT_MODES = {"w": RASTER_OUT_W, "z": RASTER_OUT_Z, "normalised": RASTER_OUT_NORMALISED}
_OUT_FILL = {"w": 0.0, "z": float("inf"), "normalised": 0.0}      # background: infinitely far


def look_at_pose(yaw_deg=0.0, pitch_deg=0.0, shift=(0.0, 0.0, 0.0), pivot_z=None):
    """(R, t), float64 numpy, of a camera that orbits about the point c = (0, 0, pivot_z) on the optical axis, for render_mesh's ``R``, ``t`` (the
    reference's "to the target viewpoint" convention, q = R p + t).  Points are in the reference's convention (what depth_to_points returns): x to the
    left, y up, z forward.  R = Rx(pitch) Ry(yaw), right-handed rotations about +x and +y; t = c - R c + shift, so with a zero ``shift`` the pivot
    stays where it is and otherwise moves by ``shift``.  ``pivot_z=None`` turns the camera about its own centre."""
    yaw, pitch = np.deg2rad(np.float64(yaw_deg)), np.deg2rad(np.float64(pitch_deg))
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]], dtype=np.float64)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]], dtype=np.float64)
    R = Rx @ Ry
    shift = np.asarray(shift, dtype=np.float64).reshape(-1)
    if shift.shape != (3,):
        raise ValueError(f"look_at_pose: shift must hold 3 values, got {shift.shape}")
    c = np.array([0.0, 0.0, 0.0 if pivot_z is None else float(pivot_z)], dtype=np.float64)
    return R, c - R @ c + shift


def _view_camera(who, h, w, K, fov_deg, R, t):
    """16 host doubles fx, fy, cx, cy, R, t and whether a pose is applied."""
    K = get_intrinsics(h, w, fov_deg) if K is None else np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"{who}: K must be 3 x 3, got {K.shape}")
    if not np.all(np.isfinite(K)) or K[0, 1] != 0 or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1:
        raise ValueError(f"{who}: K must be a finite pinhole matrix without skew, [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]")
    pose = R is not None or t is not None
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64).reshape(-1)
    if R.shape != (3, 3) or t.shape != (3,):
        raise ValueError(f"{who}: R must be 3 x 3 and t must hold 3 values, got {R.shape}, {t.shape}")
    return [K[0, 0], K[1, 1], K[0, 2], K[1, 2]] + list(R.reshape(-1)) + list(t), pose


def _view_out(who, out, inverse, fill):
    if out not in _OUT_MODES:
        raise ValueError(f"{who}: out must be 'z', 'w' or 'normalised', got {out!r}")
    inverse = _inverse(who, inverse)
    if out == "normalised":
        if inverse is None:
            raise ValueError(f"{who}: out='normalised' needs inverse=(a, b)")
        if not (inverse[0] == inverse[0] and inverse[1] == inverse[1] and inverse[0] != 0.0):
            raise ValueError(f"{who}: inverse=(a, b) needs a != 0 and no NaN, got {inverse!r}")
    return _OUT_MODES[out], (inverse if out == "normalised" else None), _OUT_FILL[out] if fill is None else float(fill)


def _fill_color(who, fill_color):
    try:
        rgb = [int(c) for c in fill_color]
    except (TypeError, ValueError):
        rgb = []
    if len(rgb) != 3 or min(rgb) < 0 or max(rgb) > 255:
        raise ValueError(f"{who}: fill_color must hold three values in 0 .. 255, got {fill_color!r}")
    return tuple(rgb)


def _check_part(who, points, triangles, colors):
    """Types and shapes of one mesh's arrays, before any device is looked at."""
    for name, a, kinds, what in (("points", points, ("float32", "float64"), "float32 or float64"), ("triangles", triangles, ("int32",), "int32"),
                                 ("colors", colors, ("uint8",), "uint8")):
        if a is None and name == "colors":
            continue
        if not isinstance(a, (np.ndarray, torch.Tensor)):
            raise TypeError(f"{who}: {name} must be a numpy array or a torch tensor, got {type(a).__name__}")
        if str(a.dtype).replace("torch.", "") not in kinds or a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{who}: {name} must be {what} [n, 3], got {a.dtype} {tuple(a.shape)}")
    if colors is not None and colors.shape[0] != points.shape[0]:
        raise ValueError(f"{who}: {colors.shape[0]} colors for {points.shape[0]} points")
    if points.shape[0] >= 2 ** 31 or triangles.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: at most 2^31 - 1 points and triangles")


def _stage_part(who, a, device):
    if isinstance(a, np.ndarray):
        return from_numpy(a).to(device)
    if a.device != device:
        raise HipExtError(f"{who}: a mesh tensor on {a.device}, expected it on the HIP device {device}")
    return a.contiguous()


@torch.no_grad()
def _render(who, parts, labels, h, w, K, fov_deg, R, t, out, inverse, fill, fill_color, device):
    """parts: (points, triangles, colors) per mesh; labels: the owner value of each."""
    h, w = _grid(who, h, w)
    cam, pose = _view_camera(who, h, w, K, fov_deg, R, t)
    mode, ab, fill = _view_out(who, out, inverse, fill)
    rgb = _fill_color(who, fill_color)
    if not parts:
        raise ValueError(f"{who}: nothing to render")
    for p in parts:
        _check_part(who, *p)
    if len({str(p[0].dtype).replace("torch.", "") for p in parts}) > 1:
        raise ValueError(f"{who}: the meshes' points must share one type")
    with_color = all(p[2] is not None for p in parts)      # colours are rendered when every mesh has them
    device = resolve_device(who, device, *[a for p in parts for a in p])
    with torch.cuda.device(device):
        staged = [tuple(None if a is None else _stage_part(who, a, device) for a in p) for p in parts]
        if len(staged) == 1:
            points, tri, col = staged[0]
        else:
            starts = np.cumsum([0] + [p[0].shape[0] for p in staged])
            points = torch.cat([p[0] for p in staged])
            tri = torch.cat([p[1] + int(s) for p, s in zip(staged, starts)])
            col = torch.cat([p[2] for p in staged]) if with_color else None
        V, T = points.shape[0], tri.shape[0]
        x = torch.empty(V, dtype=torch.int32, device=device)
        y = torch.empty(V, dtype=torch.int32, device=device)
        wv = torch.empty(V, dtype=torch.float64, device=device)
        mesh_project(points, cam, x, y, wv, pose=pose)
        depth = torch.empty(h, w, dtype=torch.float32, device=device)
        index = torch.empty(h, w, dtype=torch.int32, device=device)
        color = torch.empty(h, w, 3, dtype=torch.uint8, device=device) if with_color else None
        ws = torch.empty((mesh_raster_workspace_bytes(h, w, T) + 15) // 16 * 2, dtype=torch.int64, device=device)
        mesh_raster(x, y, wv, tri, h, w, depth, index, colors=col, color=color, mode=mode, inverse=ab, fill=fill, fill_color=rgb, workspace=ws)
        owner = torch.full_like(index, -1)      # scalar comparisons only: no host array crosses, so a stream capture may hold the whole call
        start = 0
        for p, label in zip(staged, labels):
            end = start + p[1].shape[0]
            if end > start:
                owner = torch.where((index >= start) & (index < end), int(label), owner)
            start = end
    return View(depth, index, owner, color)


def _mesh_arrays(who, mesh_or_points, triangles, colors):
    if isinstance(mesh_or_points, Mesh):
        if triangles is not None or colors is not None:
            raise ValueError(f"{who}: a Mesh carries its own triangles and colors")
        return mesh_or_points.points, mesh_or_points.triangles, mesh_or_points.colors
    if triangles is None:
        raise ValueError(f"{who}: points need triangles")
    return mesh_or_points, triangles, colors


def render_mesh(mesh_or_points, h, w, triangles=None, colors=None, K=None, fov_deg=55.0, R=None, t=None, out="z", inverse=None, fill=None,
                fill_color=(128, 128, 128), device=None) -> View:
    """A Mesh, or points [V, 3] (fp32 / fp64) with triangles int32 [T, 3] and optional colors uint8 [V, 3], seen by a pinhole camera ``K`` (default
    get_intrinsics(h, w, fov_deg); no skew) on an h x w target whose samples sit at integer pixel coordinates -- the grid depth_to_points unprojects
    from, so the identity view of a depth_to_mesh result gives the map back.  ``R``, ``t``: the pose "to the target viewpoint", q = R p + t (see
    look_at_pose); both None: q = p exactly.  A z-buffer with inclusive edges, the nearest surface wins and the lowest triangle index wins a tie
    (include/ada_hip.h has the arithmetic); no clipping: a triangle with a vertex behind the camera or beyond +-16384 pixels is dropped.

    ``out``: 'z' depth, 'w' = 1 / z, or 'normalised' = (w - b) / a for ``inverse=(a, b)``, the convention of depth_to_points and amodal_layers --
    that map goes into hip_ext.image.render_depth / colorize unchanged.  Background takes ``fill`` (default: inf for 'z', 0 otherwise) and
    ``fill_color``.  View.color is None without vertex colours; View.owner is 0 on the mesh.  Nothing is read back."""
    who = "render_mesh"
    part = _mesh_arrays(who, mesh_or_points, triangles, colors)
    return _render(who, [part], [0], h, w, K, fov_deg, R, t, out, inverse, fill, fill_color, device)


def render_meshes(meshes, h, w, K=None, fov_deg=55.0, R=None, t=None, out="z", inverse=None, fill=None, fill_color=(128, 128, 128), device=None) -> View:
    """Several Meshes into one buffer, as render_mesh: View.owner is the position in ``meshes`` of the mesh whose triangle won, View.index counts the
    triangles through the meshes in order.  Colours are rendered when every mesh has them.  An empty Mesh is legal and owns nothing."""
    who = "render_meshes"
    meshes = list(meshes)
    for m in meshes:
        if not isinstance(m, Mesh):
            raise TypeError(f"{who}: a list of Mesh expected, got {type(m).__name__}")
    return _render(who, [(m.points, m.triangles, m.colors) for m in meshes], range(len(meshes)), h, w, K, fov_deg, R, t, out, inverse, fill, fill_color, device)


def render_layers(layers, h, w, objects=None, scene=True, near=1.0, far=10.0, out="normalised", K=None, fov_deg=55.0, R=None, t=None, fill=None,
                  fill_color=(128, 128, 128), device=None) -> View:
    """The scene mesh (``scene=True``) and the object meshes ``objects`` (indices into layers.objects; None: all) of an amodal_layers result in one view.
    View.owner is 0 for the scene and k + 1 for object k, whichever are shown.  ``near`` / ``far`` / ``fov_deg`` are what amodal_layers was called with:
    the default ``out='normalised'`` maps depth back to the networks' normalised inverse depth with them, and 'z' / 'w' are metric."""
    who = "render_layers"
    if not isinstance(layers, Layers):
        raise TypeError(f"{who}: a Layers expected, got {type(layers).__name__}")
    if not (near > 0 and far > near):
        raise ValueError(f"{who}: 0 < near < far expected, got near={near!r} far={far!r}")
    chosen = list(range(len(layers.objects))) if objects is None else [as_int(k) for k in objects]
    if any(k is None or not 0 <= k < len(layers.objects) for k in chosen):
        raise ValueError(f"{who}: objects must index the {len(layers.objects)} object meshes, got {objects!r}")
    meshes = ([layers.scene] if scene else []) + [layers.objects[k] for k in chosen]
    labels = ([0] if scene else []) + [k + 1 for k in chosen]
    inverse = (1.0 / near - 1.0 / far, 1.0 / far)
    return _render(who, [(m.points, m.triangles, m.colors) for m in meshes], labels, h, w, K, fov_deg, R, t, out, inverse, fill, fill_color, device)


_FILLS = ("smooth", "nearest", "harmonic")


def _fill_fn(who, method):
    if method not in _FILLS:
        raise ValueError(f"{who}: method must be 'smooth', 'nearest' or 'harmonic', got {method!r}")
    return {"smooth": _inpaint.fill_smooth, "nearest": _inpaint.fill_nearest, "harmonic": _inpaint.fill_harmonic}[method]


@torch.no_grad()
def fill_view(view, method="smooth") -> View:
    """The view with its holes filled: the pixels no triangle covered (``view.owner < 0``) get depth, and colour where ``view.color`` is not None, from
    the pixels a triangle covered -- hip_ext.inpaint.fill_smooth (``method='smooth'``, the push-pull fill) or fill_nearest (``'nearest'``, the value of
    the nearest covered pixel) or fill_harmonic (``'harmonic'``, the membrane solve: every hole pixel the mean of its neighbours).  Covered pixels keep their bits; ``index`` and ``owner`` are returned unchanged, so the caller still sees which pixels
    were holes.  A view without any covered pixel comes back unchanged.  The fill interpolates what is seen and knows nothing of the geometry behind a
    hole.  Nothing is read back: the empty view is kept by a select on the device."""
    who = "fill_view"
    if not isinstance(view, View):
        raise TypeError(f"{who}: a View expected, got {type(view).__name__}")
    fill = _fill_fn(who, method)
    valid = view.owner >= 0
    some = valid.any()
    depth = torch.where(some, fill(view.depth, valid), view.depth)
    color = None if view.color is None else torch.where(some, fill(view.color, valid), view.color)
    return View(depth, view.index, view.owner, color)


@torch.no_grad()
def remove_objects(depth, masks, image=None, grow=1, method="smooth", device=None):
    """(depth_filled, image_filled or None): the depth map, and the photo when given, with the objects under ``masks`` taken out.  The union of ``masks``
    (uint8 / bool [K, h, w] or [h, w], non-zero = object) is dilated ``grow`` times with hip_ext.masks.dilate(size=3) (``grow=0``: not at all), marked
    invalid and filled from the rest with hip_ext.inpaint.fill_smooth / fill_nearest / fill_harmonic (``method``).  Pixels outside the grown union keep their bits.
    ``depth``: fp32 [h, w]; ``image``: uint8 [h, w, 3] or None.  Through depth_to_mesh the result is a background layer to render behind amodal_layers'
    objects.  This is geometry-blind interpolation of the surroundings, not a learned completion: what stood behind the objects is not recovered."""
    who = "remove_objects"
    fill = _fill_fn(who, method)
    h, w, was2d = _check_depth(who, depth)
    if not was2d:
        raise ValueError(f"{who}: depth must be [h, w], got shape {tuple(depth.shape)}")
    _check_mask(who, masks)
    if tuple(masks.shape[-2:]) != (h, w):
        raise ValueError(f"{who}: masks of shape {tuple(masks.shape)} for a depth map of shape {(h, w)}")
    if image is not None and (not isinstance(image, (np.ndarray, torch.Tensor)) or str(image.dtype).replace("torch.", "") != "uint8"
                              or tuple(image.shape) != (h, w, 3)):
        raise ValueError(f"{who}: image must be uint8 [{h}, {w}, 3], got {getattr(image, 'dtype', type(image).__name__)} {tuple(getattr(image, 'shape', ()))}")
    g = as_int(grow)
    if g is None or g < 0:
        raise ValueError(f"{who}: grow must be a non-negative integer, got {grow!r}")
    device = resolve_device(who, device, depth, masks, image)
    with torch.cuda.device(device):
        m = _stage_mask(who, masks, device)
        union = (m != 0).any(dim=0).to(torch.uint8)
        if g > 0:
            union = _masks.dilate(union, size=3, iterations=g, device=device)
        valid = union == 0
        d = fill(_stage_depth(who, depth, device)[0], valid, device=device)
        img = None if image is None else fill(image, valid, device=device)
    return d, img


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def write_ply(path, mesh_or_points, triangles=None, colors=None):
    """A binary little-endian PLY from a Mesh, or from points [n, 3] (fp32 -> float, fp64 -> double) with optional triangles [m, 3] and colours uint8
    [n, 3] (red, green, blue).  Written with numpy on the host: the one place the data leaves the device."""
    if isinstance(mesh_or_points, Mesh):
        if triangles is not None or colors is not None:
            raise ValueError("write_ply: a Mesh carries its own triangles and colors")
        points, triangles, colors = mesh_or_points.points, mesh_or_points.triangles, mesh_or_points.colors
    else:
        points = mesh_or_points
    pts = _host(points)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.dtype not in (np.float32, np.float64):
        raise ValueError(f"write_ply: points must be float32 or float64 [n, 3], got {pts.dtype} {pts.shape}")
    kind = "float" if pts.dtype == np.float32 else "double"
    fields = [("x", "<" + pts.dtype.str[1:]), ("y", "<" + pts.dtype.str[1:]), ("z", "<" + pts.dtype.str[1:])]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {pts.shape[0]}"] + [f"property {kind} {c}" for c in "xyz"]
    col = None
    if colors is not None:
        col = _host(colors)
        if col.dtype != np.uint8 or col.shape != pts.shape:
            raise ValueError(f"write_ply: colors must be uint8 {pts.shape}, got {col.dtype} {col.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += [f"property uchar {c}" for c in ("red", "green", "blue")]
    vert = np.empty(pts.shape[0], dtype=fields)
    for i, c in enumerate("xyz"):
        vert[c] = pts[:, i]
    if col is not None:
        for i, c in enumerate(("red", "green", "blue")):
            vert[c] = col[:, i]
    face = None
    if triangles is not None:
        tri = _host(triangles)
        if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu":
            raise ValueError(f"write_ply: triangles must be integers [m, 3], got {tri.dtype} {tri.shape}")
        if tri.size and (tri.min() < 0 or tri.max() >= pts.shape[0]):
            raise ValueError("write_ply: a triangle indexes a vertex that is not there")
        face = np.empty(tri.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
        face["n"] = 3
        face["v"] = tri
        header += [f"element face {tri.shape[0]}", "property list uchar int vertex_indices"]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vert.tobytes())
        if face is not None:
            f.write(face.tobytes())
