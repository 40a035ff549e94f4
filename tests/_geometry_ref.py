"""Numpy restatements of the depth-to-geometry stage, in this project's own words: what csrc/ada_geometry.hip must compute.  The CPU suite pins them to
goldens written from the real reference (tests/golden/geometry/cases.npz, tools/make_geometry_golden.py); the GPU suite compares the kernels with them."""
from collections import namedtuple

import numpy as np

Mesh = namedtuple("Mesh", "points triangles vertex_count triangle_count colors")
Layers = namedtuple("Layers", "scene objects")

GAMMA4 = 4 * 2.0 ** -53 / (1 - 4 * 2.0 ** -53)


def intrinsics(h, w, fov_deg=55.0):
    f = 0.5 * w / np.tan(0.5 * fov_deg * np.pi / 180.0)
    return np.array([[f, 0.0, 0.5 * w], [0.0, f, 0.5 * h], [0.0, 0.0, 1.0]])


def z_of(depth, inverse=None):
    """float64 z of an fp32 map: the map itself, or 1 / (a d + b) with every operation rounded once."""
    d = np.asarray(depth)
    assert d.dtype == np.float32
    z = d.astype(np.float64)
    if inverse is not None:
        a, b = np.float64(inverse[0]), np.float64(inverse[1])
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            z = 1.0 / (a * z + b)
    return z


def valid_of(z):
    return np.isfinite(z) & (z > 0)


def points_from_z(z, Kinv, R=None, t=None):
    """z float64 [..., h, w] -> float64 [..., h, w, 3]; numpy evaluates each elementwise product and sum with one rounding, there is no FMA here."""
    h, w = z.shape[-2:]
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = [((z * Kinv[i, 0]) * x + (z * Kinv[i, 1]) * y) + (z * Kinv[i, 2]) * 1.0 for i in range(3)]
        q = [-p[0], -p[1], p[2]]
        r = [((R[i, 0] * q[0] + R[i, 1] * q[1]) + R[i, 2] * q[2]) + t[i] for i in range(3)]
    out = np.stack(r, axis=-1)
    out[~np.isfinite(z)] = np.nan
    return out


def points(depth, R=None, t=None, K=None, fov_deg=55.0, inverse=None):
    z = z_of(depth, inverse)
    h, w = z.shape[-2:]
    K = intrinsics(h, w, fov_deg) if K is None else np.asarray(K, dtype=np.float64)
    return points_from_z(z, np.linalg.inv(K), R, t)


def pose_bound(depth, R, t, K=None, fov_deg=55.0, inverse=None):
    """2 gamma_4 (sum_j |R_ij| |q_j| + |t_i|) per coordinate, q the default-pose points (exact on both sides)."""
    q = np.abs(points(depth, K=K, fov_deg=fov_deg, inverse=inverse))
    return 2 * GAMMA4 * (q @ np.abs(np.asarray(R, dtype=np.float64)).T + np.abs(np.asarray(t, dtype=np.float64)))


def triangles(h, w, mask=None, depth=None, inverse=None, max_ratio=None):
    """int32 [n, 3]: per pixel cell in raster order (tl, bl, tr) then (br, tr, bl), kept by the mask, validity and ratio rules."""
    if h < 2 or w < 2:
        return np.zeros((0, 3), np.int32)
    inside = np.ones((h, w), bool) if mask is None else np.asarray(mask).reshape(h, w) != 0
    if depth is not None:
        z = z_of(depth, inverse).reshape(h, w)
        inside = inside & valid_of(z)
    corner = lambda a: (a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:])      # tl, tr, bl, br of every cell
    tl, tr, bl, br = corner(inside)
    first, second = tl & bl & tr, br & tr & bl
    if depth is not None and max_ratio is not None and max_ratio > 0:
        ztl, ztr, zbl, zbr = corner(z)
        with np.errstate(invalid="ignore", over="ignore"):
            first = first & (np.maximum(np.maximum(ztl, zbl), ztr) <= np.float64(max_ratio) * np.minimum(np.minimum(ztl, zbl), ztr))
            second = second & (np.maximum(np.maximum(zbr, ztr), zbl) <= np.float64(max_ratio) * np.minimum(np.minimum(zbr, ztr), zbl))
    kept = np.flatnonzero(np.stack([first, second], -1).reshape(-1))      # candidate numbers: 2 cell + (0 | 1), raster order of the cells
    cell, which = kept // 2, kept % 2
    v = (cell // (w - 1)) * w + cell % (w - 1)                               # the cell's top-left vertex
    a = np.where(which == 0, v, v + w + 1)
    b = np.where(which == 0, v + w, v + 1)
    c = np.where(which == 0, v + 1, v + w)
    return np.stack([a, b, c], 1).astype(np.int32)


def compact(tri, pts, colors=None):
    """(points of the used vertices in raster order, remapped triangles, vertex count, their colours)."""
    pts = np.asarray(pts).reshape(-1, 3)
    used = np.zeros(pts.shape[0], bool)
    used[tri.reshape(-1)] = True
    new = np.cumsum(used) - 1
    cols = None if colors is None else np.asarray(colors).reshape(-1, 3)[used]
    return pts[used], new[tri].astype(np.int32).reshape(-1, 3), int(used.sum()), cols


def depth_to_mesh(depth, mask=None, colors=None, compact_vertices=True, inverse=None, max_ratio=None, fov_deg=55.0, dtype=np.float32, **pose):
    depth = np.asarray(depth, dtype=np.float32)
    h, w = depth.shape
    pts = points(depth, fov_deg=fov_deg, inverse=inverse, **pose).astype(dtype).reshape(-1, 3)
    tri = triangles(h, w, mask, depth, inverse, max_ratio)
    cols = None if colors is None else np.asarray(colors).reshape(-1, 3)
    if not compact_vertices:
        return Mesh(pts, tri, h * w, tri.shape[0], cols)
    p, t, n, c = compact(tri, pts, cols)
    return Mesh(p, t, n, tri.shape[0], c)


def nearest_resize(a, h, w):
    """cv2's INTER_NEAREST source index rule along both axes of [..., hi, wi]."""
    hi, wi = a.shape[-2:]
    sy = np.minimum(np.floor(np.arange(h) * (1.0 / (h / hi))).astype(int), hi - 1)
    sx = np.minimum(np.floor(np.arange(w) * (1.0 / (w / wi))).astype(int), wi - 1)
    return a[..., sy[:, None], sx[None, :]]


def amodal_layers(base, blended, masks, image=None, near=1.0, far=10.0, fov_deg=55.0, max_ratio=None):
    inverse = (1.0 / near - 1.0 / far, 1.0 / far)
    h, w = base.shape
    colors = None
    if image is not None:
        colors = np.ascontiguousarray(nearest_resize(np.asarray(image)[:, :, :3].transpose(2, 0, 1), h, w)[::-1].transpose(1, 2, 0))
    kw = dict(colors=colors, inverse=inverse, max_ratio=max_ratio, fov_deg=fov_deg)
    return Layers(depth_to_mesh(base, **kw), [depth_to_mesh(blended[k], mask=masks[k] > 0, **kw) for k in range(blended.shape[0])])
