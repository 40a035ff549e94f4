"""A plain-numpy restatement of the rasteriser's contract (include/ada_hip.h, "Meshes seen from a camera"), in this project's own words: what
csrc/ada_raster.hip must compute.  Brute force: every triangle at every sample, int64 edge functions, fp64 with the stated operation order (numpy rounds
each elementwise product, sum and quotient once; there is no FMA here).  Never imported by the product."""
from collections import namedtuple

import numpy as np

View = namedtuple("View", "depth index owner color")

GUARD = 16384.0
SUB = 256
FILL = {"w": 0.0, "z": np.inf, "normalised": 0.0}


def intrinsics(h, w, fov_deg=55.0):
    f = 0.5 * w / np.tan(0.5 * fov_deg * np.pi / 180.0)
    return np.array([[f, 0.0, 0.5 * w], [0.0, f, 0.5 * h], [0.0, 0.0, 1.0]])


def look_at_pose(yaw_deg=0.0, pitch_deg=0.0, shift=(0.0, 0.0, 0.0), pivot_z=None):
    yaw, pitch = np.deg2rad(np.float64(yaw_deg)), np.deg2rad(np.float64(pitch_deg))
    Ry = np.array([[np.cos(yaw), 0.0, np.sin(yaw)], [0.0, 1.0, 0.0], [-np.sin(yaw), 0.0, np.cos(yaw)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(pitch), -np.sin(pitch)], [0.0, np.sin(pitch), np.cos(pitch)]])
    R = Rx @ Ry
    c = np.array([0.0, 0.0, 0.0 if pivot_z is None else float(pivot_z)])
    return R, c - R @ c + np.asarray(shift, dtype=np.float64)


def snap(u):
    """A coordinate in pixels -> 1/256-pixel units, round half to even."""
    return np.rint(np.float64(256.0) * np.asarray(u, dtype=np.float64)).astype(np.int64)


def project(points, K, R=None, t=None):
    """points [V, 3] (fp32 or fp64) -> X, Y int64 [V], w fp64 [V], valid bool [V]; X = Y = 0 and w = 0 where not valid."""
    p = np.asarray(points).astype(np.float64).reshape(-1, 3)
    K = np.asarray(K, dtype=np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        if R is None and t is None:
            q = [px, py, pz]
        else:
            R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
            t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64).reshape(3)
            q = [((R[i, 0] * px + R[i, 1] * py) + R[i, 2] * pz) + t[i] for i in range(3)]
        valid = np.isfinite(q[0]) & np.isfinite(q[1]) & np.isfinite(q[2]) & (q[2] >= 2.0 ** -64) & (q[2] <= 2.0 ** 64)
        qz = np.where(valid, q[2], 1.0)
        u = fx * ((-q[0]) / qz) + cx
        v = fy * ((-q[1]) / qz) + cy
        valid = valid & (np.abs(u) <= GUARD) & (np.abs(v) <= GUARD)      # False for NaN
        w = np.where(valid, 1.0 / qz, 0.0)
    X = np.where(valid, np.rint(256.0 * np.where(valid, u, 0.0)), 0.0).astype(np.int64)
    Y = np.where(valid, np.rint(256.0 * np.where(valid, v, 0.0)), 0.0).astype(np.int64)
    return X, Y, w, valid


def kept(tri, X, Y, valid):
    """bool [T]: the triangles the rule does not drop, and their signed areas A int64 [T] (0 where an index is out of range)."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    V = X.shape[0]
    inside = np.all((tri >= 0) & (tri < V), axis=1)
    safe = np.where(inside[:, None], tri, 0)
    ok = inside & (np.all(valid[safe], axis=1) if V else np.zeros(tri.shape[0], bool))
    if V:
        X0, X1, X2, Y0, Y1, Y2 = X[safe[:, 0]], X[safe[:, 1]], X[safe[:, 2]], Y[safe[:, 0]], Y[safe[:, 1]], Y[safe[:, 2]]
        A = np.where(ok, (X1 - X0) * (Y2 - Y0) - (X2 - X0) * (Y1 - Y0), 0)
    else:
        A = np.zeros(tri.shape[0], np.int64)
    return ok & (A != 0), A


def edges(X, Y, ix, A, Sx, Sy):
    """The three edge functions of one triangle at the samples (int64 arrays), signed so that inside is >= 0."""
    X0, X1, X2, Y0, Y1, Y2 = X[ix[0]], X[ix[1]], X[ix[2]], Y[ix[0]], Y[ix[1]], Y[ix[2]]
    e0 = (X2 - X1) * (Sy - Y1) - (Y2 - Y1) * (Sx - X1)
    e1 = (X0 - X2) * (Sy - Y2) - (Y0 - Y2) * (Sx - X2)
    e2 = A - e0 - e1
    if A < 0:
        e0, e1, e2, A = -e0, -e1, -e2, -A
    return e0, e1, e2, A


def rasterize(X, Y, w, valid, tri, h, width, colors=None, out="z", inverse=None, fill=None, fill_color=(128, 128, 128)):
    """Vertex records and triangles -> (depth fp32 [h, width], index int32, color uint8 [h, width, 3] or None, w fp64 of the winner, NaN on background)."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    keep, areas = kept(tri, X, Y, valid)
    Sy, Sx = np.meshgrid(np.arange(h, dtype=np.int64) * SUB, np.arange(width, dtype=np.int64) * SUB, indexing="ij")
    best32 = np.full((h, width), -1.0, np.float32)      # every candidate's float32(w) is > 0
    best64 = np.full((h, width), np.nan)
    index = np.full((h, width), -1, np.int32)
    chan = np.zeros((h, width, 3))
    for k in np.flatnonzero(keep):      # ascending ids and a strict comparison: the lowest id keeps a tie
        ix = tri[k]
        e0, e1, e2, A = edges(X, Y, ix, int(areas[k]), Sx, Sy)
        cover = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
        if not cover.any():
            continue
        w0, w1, w2 = w[ix[0]], w[ix[1]], w[ix[2]]
        wi = w0 + ((e1.astype(np.float64) * (w1 - w0) + e2.astype(np.float64) * (w2 - w0)) / np.float64(A))
        w32 = wi.astype(np.float32)      # round to nearest even
        win = cover & (w32 > best32)
        best32[win], best64[win], index[win] = w32[win], wi[win], k
        if colors is not None and win.any():
            n0, n1, n2 = e0.astype(np.float64) * w0, e1.astype(np.float64) * w1, e2.astype(np.float64) * w2
            den = (n0 + n1) + n2
            c = np.asarray(colors).reshape(-1, 3).astype(np.float64)
            for ch in range(3):
                with np.errstate(all="ignore"):
                    v = ((n0 * c[ix[0], ch] + n1 * c[ix[1], ch]) + n2 * c[ix[2], ch]) / den
                chan[..., ch][win] = v[win]
    hit = index >= 0
    with np.errstate(all="ignore"):
        if out == "w":
            d = best64
        elif out == "z":
            d = 1.0 / best64
        elif out == "normalised":
            a, b = np.float64(inverse[0]), np.float64(inverse[1])
            d = (best64 - b) / a
        else:
            raise ValueError(out)
        depth = np.where(hit, d, np.nan).astype(np.float32)      # one rounding
    depth[~hit] = np.float32(FILL[out] if fill is None else fill)
    color = None
    if colors is not None:
        color = np.minimum(255.0, np.floor(chan + 0.5)).astype(np.uint8)
        color[~hit] = np.asarray(fill_color, dtype=np.uint8)
    return depth, index, color, best64


def render(points, tri, h, width, colors=None, K=None, fov_deg=55.0, R=None, t=None, out="z", inverse=None, fill=None, fill_color=(128, 128, 128)):
    """render_mesh: a View whose owner is 0 on the mesh and -1 on the background."""
    K = intrinsics(h, width, fov_deg) if K is None else K
    X, Y, w, valid = project(points, K, R, t)
    depth, index, color, _ = rasterize(X, Y, w, valid, tri, h, width, colors, out, inverse, fill, fill_color)
    return View(depth, index, np.where(index >= 0, 0, -1).astype(np.int32), color)


def render_many(meshes, labels, h, width, **kw):
    """render_meshes / render_layers: meshes = [(points, triangles, colors)], owner = the label of the winner's mesh."""
    with_color = len(meshes) > 0 and all(m[2] is not None for m in meshes)
    starts = np.cumsum([0] + [np.asarray(m[0]).reshape(-1, 3).shape[0] for m in meshes])
    ends = np.cumsum([np.asarray(m[1]).reshape(-1, 3).shape[0] for m in meshes])
    points = np.concatenate([np.asarray(m[0]).reshape(-1, 3) for m in meshes])
    tri = np.concatenate([np.asarray(m[1]).reshape(-1, 3).astype(np.int64) + s for m, s in zip(meshes, starts)])
    colors = np.concatenate([np.asarray(m[2]).reshape(-1, 3) for m in meshes]) if with_color else None
    v = render(points, tri, h, width, colors=colors, **kw)
    which = np.searchsorted(ends, v.index, side="right").clip(max=len(meshes) - 1)
    owner = np.where(v.index >= 0, np.asarray(labels, dtype=np.int32)[which], -1).astype(np.int32)
    return View(v.depth, v.index, owner, v.color)
