"""A plain-numpy restatement of the adaptive mesh's contract (include/ada_hip.h, "Adaptive depth-map meshes"), in this project's own words: what
csrc/ada_adaptive.hip must compute.  Brute force over the WHOLE virtual grid, level by level in heap order, fp64 with the stated operation order (numpy
rounds each elementwise product, sum, difference and quotient once; there is no FMA here).  Never imported by the product."""
import numpy as np


def grid_side(h, w):
    """N: the smallest power of two >= max(h, w) - 1."""
    N = 1
    while N < max(h, w) - 1:
        N *= 2
    return N


def tree_levels(N):
    """[(a, b, c)] per level, each int64 [n, 2] (row, column) in heap order: level 0 holds the roots 2 and 3, the last one the 2 N^2 leaves."""
    a = np.array([[N, N], [0, 0]], dtype=np.int64)
    b = np.array([[0, 0], [N, N]], dtype=np.int64)
    c = np.array([[N, 0], [0, N]], dtype=np.int64)
    out = [(a, b, c)]
    for _ in range(2 * (int(N).bit_length() - 1)):
        m = (a + b) // 2
        # children of t: 2 t = (c, a, m), 2 t + 1 = (b, c, m)
        a, b, c = (np.stack([c, b], axis=1).reshape(-1, 2), np.stack([a, c], axis=1).reshape(-1, 2), np.stack([m, m], axis=1).reshape(-1, 2))
        out.append((a, b, c))
    return out


def disparity(depth, inverse=None):
    d = np.asarray(depth, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if inverse is None:
            return np.float64(1.0) / d
        return np.float64(inverse[0]) * d + np.float64(inverse[1])


def z_values(depth, inverse=None):
    d = np.asarray(depth, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return d if inverse is None else np.float64(1.0) / disparity(depth, inverse)


def _virtual(x, N, fill):
    out = np.full((N + 1, N + 1), fill, dtype=x.dtype)
    out[:x.shape[0], :x.shape[1]] = x
    return out


def _at(grid, p):
    return grid[p[:, 0], p[:, 1]]


def _keepable(ok, z, ratio, a, b, c):
    keep = _at(ok, a) & _at(ok, b) & _at(ok, c)
    if ratio is not None and ratio > 0:
        za, zb, zc = _at(z, a), _at(z, b), _at(z, c)
        with np.errstate(all="ignore"):
            keep &= np.maximum(np.maximum(za, zb), zc) <= np.float64(ratio) * np.minimum(np.minimum(za, zb), zc)
    return keep


def build(depth, mask=None, inverse=None, max_ratio=None):
    """(levels, E over the virtual grid, keepable flags of the leaves)."""
    depth = np.asarray(depth, dtype=np.float32)
    h, w = depth.shape
    assert h >= 2 and w >= 2
    N = grid_side(h, w)
    lv = tree_levels(N)
    z = z_values(depth, inverse)
    ok = np.isfinite(z) & (z > 0)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    ok = _virtual(ok, N, False)      # an absent vertex fails
    z = _virtual(np.where(ok[:h, :w], z, 1.0), N, 1.0)
    om = _virtual(disparity(depth, inverse), N, 1.0)
    leaf_keep = _keepable(ok, z, max_ratio, *lv[-1])
    E = np.zeros((N + 1, N + 1), dtype=np.float64)
    for l in range(len(lv) - 2, -1, -1):
        a, b, c = lv[l]
        m = (a + b) // 2
        if l == len(lv) - 2:
            child = np.where(leaf_keep[0::2] & leaf_keep[1::2], 0.0, np.inf)
        else:
            child = np.maximum(_at(E, (c + a) // 2), _at(E, (b + c) // 2))
        fin = np.isfinite(child)      # then every vertex of T is valid: the quotient is defined
        wa, wb, wm = (np.where(fin, _at(om, p), 1.0) for p in (a, b, m))
        with np.errstate(all="ignore"):
            dev = np.abs(np.float64(0.5) * (wa + wb) - wm) / wm
        F = np.where(fin, np.maximum(dev, child), np.inf)
        np.maximum.at(E, (m[:, 0], m[:, 1]), F)
    return lv, E, leaf_keep


def emit(lv, E, leaf_keep, w, max_error):
    """int32 [n, 3]: the rows for the tolerance ``max_error`` (None: every keepable leaf), ascending heap index."""
    rows = []
    for l, (a, b, c) in enumerate(lv):
        if l == 0 or max_error is None:
            split = np.ones(a.shape[0], dtype=bool)
        else:
            split = _at(E, c) > max_error      # c is the parent's hypotenuse midpoint
        if l == len(lv) - 1:
            keep = split & leaf_keep
        elif max_error is None:
            keep = np.zeros(a.shape[0], dtype=bool)
        else:
            keep = split & (_at(E, (a + b) // 2) <= max_error)
        ids = np.stack([p[:, 0] * w + p[:, 1] for p in (a, b, c)], axis=1)
        rows.append(ids[keep])
    return np.concatenate(rows).astype(np.int32).reshape(-1, 3)


def adaptive_triangles(depth, mask=None, inverse=None, max_ratio=None, max_error=0.01, return_error=False):
    """hip_ext.geometry.adaptive_triangles for one map: triangles int32 [n, 3] and, with ``return_error``, E fp64 [h, w]."""
    depth = np.asarray(depth, dtype=np.float32)
    h, w = depth.shape
    lv, E, leaf_keep = build(depth, mask, inverse, max_ratio)
    tri = emit(lv, E, leaf_keep, w, max_error)
    return (tri, E[:h, :w].copy()) if return_error else tri


def sweep(depth, taus, mask=None, inverse=None, max_ratio=None):
    """{tau: triangles} and E [h, w] from one error map."""
    depth = np.asarray(depth, dtype=np.float32)
    h, w = depth.shape
    lv, E, leaf_keep = build(depth, mask, inverse, max_ratio)
    return {t: emit(lv, E, leaf_keep, w, t) for t in taus}, E[:h, :w].copy()
