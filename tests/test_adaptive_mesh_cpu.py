"""CPU: tests/_adaptive_ref.py, the numpy restatement of the adaptive mesh's contract (include/ada_hip.h), pinned by hand-derived cases and by the
properties every such mesh has: conforming, same cover as the finest mesh, one winding, monotone in the tolerance, nested, and a bounded deviation."""
import numpy as np
import pytest

import _adaptive_ref as A

TAUS = (0.0, 0.01, 0.05, 0.2, None)
SHAPES = ((9, 9), (17, 17), (12, 19), (5, 33))


def _plane_depth(h, w, o0=0.5, oi=0.01, oj=0.02):
    """A map whose disparity 1 / depth is (nearly) linear; with these dyadic-free coefficients not exactly, so tolerances > 0 are what flattens it."""
    i, j = np.mgrid[:h, :w]
    return (1.0 / (o0 + oi * i + oj * j)).astype(np.float32)


def _exact_plane_inverse(h, w):
    """depth and inverse=(a, b) whose disparity a depth + b is linear in (i, j) EXACTLY (small integers): the deviation term is 0 everywhere."""
    i, j = np.mgrid[:h, :w]
    return (8 + 2 * i + 3 * j).astype(np.float32), (0.25, 1.0)


def _scene(h, w, seed):
    """Smooth ramp, a step edge and a bump: something to refine."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[:h, :w]
    d = 2.0 + 0.03 * i + 0.02 * j + 0.3 * np.sin(i / 3.0) * np.cos(j / 4.0)
    d[:, w // 2:] += 1.5
    d += 0.01 * rng.standard_normal((h, w))
    return d.astype(np.float32)


def _mask(h, w):
    m = np.ones((h, w), dtype=np.uint8)
    m[h // 3:h // 3 + 2, w // 4:w // 4 + 3] = 0
    m[0, w - 1] = 0
    return m


def _coords(tri, w):
    tri = np.asarray(tri, dtype=np.int64)
    return np.stack([tri // w, tri % w], axis=-1)      # [n, 3, (i, j)]


def _twice_area(p):
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def _assert_conforming(tri, w):
    """No vertex of the mesh lies strictly inside an edge of a triangle."""
    p = _coords(tri, w)
    verts = {tuple(v) for v in p.reshape(-1, 2)}
    for t in p:
        for k in range(3):
            (i0, j0), (i1, j1) = t[k], t[(k + 1) % 3]
            n = max(abs(i1 - i0), abs(j1 - j0))      # the edges are axis-aligned or diagonal: n lattice steps
            di, dj = (i1 - i0) // n, (j1 - j0) // n
            for s in range(1, n):
                assert (i0 + s * di, j0 + s * dj) not in verts, (t, k, s)


def _cells(tri, w, h):
    """Twice the area of every unit cell half that the mesh covers, as a raster: [h - 1, w - 1, 2] of covered (sub-cell sampling at the four quarter
    points of a cell, which no RTIN edge passes through)."""
    p = _coords(tri, w).astype(np.float64)
    cover = np.zeros((h - 1, w - 1, 4), dtype=np.int32)
    offs = ((0.25, 0.5), (0.75, 0.5), (0.5, 0.25), (0.5, 0.75))
    for t in p:
        i0, i1 = int(t[:, 0].min()), int(t[:, 0].max())
        j0, j1 = int(t[:, 1].min()), int(t[:, 1].max())
        ii, jj = np.mgrid[i0:i1, j0:j1]
        for k, (oi, oj) in enumerate(offs):
            y, x = ii + oi, jj + oj
            s = []
            for e in range(3):
                (ya, xa), (yb, xb) = t[e], t[(e + 1) % 3]
                s.append((yb - ya) * (x - xa) - (xb - xa) * (y - ya))
            inside = ((s[0] > 0) & (s[1] > 0) & (s[2] > 0)) | ((s[0] < 0) & (s[1] < 0) & (s[2] < 0))
            cover[i0:i1, j0:j1, k] += inside
    return cover


# ---------------------------------------------------------------- hand-derived cases
def test_plane_on_3x3_is_the_two_roots():
    d, inv = _exact_plane_inverse(3, 3)
    tri, E = A.adaptive_triangles(d, inverse=inv, max_error=0.0, return_error=True)
    assert tri.dtype == np.int32 and tri.tolist() == [[8, 0, 6], [0, 8, 2]]
    assert np.array_equal(E, np.zeros((3, 3)))


def test_raised_centre_on_3x3_gives_the_four_level_1_triangles():
    d = np.ones((3, 3), dtype=np.float32)
    d[1, 1] = 2.0      # omega 0.5 at the centre, 1 elsewhere: |1 - 0.5| / 0.5 = 1 at the centre, 0 at the edge midpoints
    tri, E = A.adaptive_triangles(d, max_error=0.5, return_error=True)
    want_E = np.zeros((3, 3))
    want_E[1, 1] = 1.0
    assert np.array_equal(E, want_E)
    # heap 4 = left of root 2 = (c, a, m) = ((2,0), (2,2), (1,1)); 5 = (b, c, m) = ((0,0), (2,0), (1,1)); 6 = ((0,2), (0,0), (1,1)); 7 = ((2,2), (0,2), (1,1))
    assert tri.tolist() == [[6, 8, 4], [0, 6, 4], [2, 0, 4], [8, 2, 4]]
    assert A.adaptive_triangles(d, max_error=1.0).tolist() == [[8, 0, 6], [0, 8, 2]]      # E <= tau is inclusive


def test_one_masked_corner_on_3x3():
    d, inv = _exact_plane_inverse(3, 3)
    m = np.ones((3, 3), dtype=np.uint8)
    m[0, 2] = 0      # vertex 2: the leaves that touch it go, and everything above them splits
    tri, E = A.adaptive_triangles(d, mask=m, inverse=inv, max_error=0.0, return_error=True)
    # E = +inf at (0, 1) and (1, 2) (the leaf parents beside the corner) and at the centre above them; root 2's side stays whole below level 1
    want_E = np.zeros((3, 3))
    want_E[0, 1] = want_E[1, 2] = want_E[1, 1] = np.inf
    assert np.array_equal(E, want_E)
    # level 1: 4 and 5 (E at (2, 1) and (1, 0) is 0); level 2 (leaves) under 6 and 7: 12 = ((1,1), (0,2), (0,1)) dropped, 13 = ((0,0), (1,1), (0,1)),
    # 14 = ((1,1), (2,2), (1,2)), 15 = ((0,2), (1,1), (1,2)) dropped
    assert tri.tolist() == [[6, 8, 4], [0, 6, 4], [0, 4, 1], [4, 8, 5]]


def test_absent_vertices_3x2():
    d = np.ones((3, 2), dtype=np.float32)      # N = 2: column 2 is absent
    tri, E = A.adaptive_triangles(d, max_error=0.0, return_error=True)
    assert np.array_equal(E[:, 0], [0.0, 0.0, 0.0]) and np.array_equal(E[:, 1], [np.inf, np.inf, np.inf])
    # ids i * 2 + j.  Level 1: 5 = ((0,0), (2,0), (1,1)) only (E[(1, 0)] = 0); leaves under 4 = ((2,0), (2,2), (1,1)): 8 = ((1,1), (2,0), (2,1)) kept,
    # 9 touches (2, 2); under 6 = ((0,2), (0,0), (1,1)): 12 touches (0, 2), 13 = ((0,0), (1,1), (0,1)) kept; under 7: both touch column 2
    assert tri.tolist() == [[0, 4, 3], [3, 4, 5], [0, 3, 1]]
    # every keepable leaf: 8, then 5's children 10 = (c, a, m) = ((1,1), (0,0), (1,0)) and 11 = (b, c, m) = ((2,0), (1,1), (1,0)), then 13
    assert A.adaptive_triangles(d, max_error=None).tolist() == [[3, 4, 5], [3, 0, 2], [4, 3, 2], [0, 3, 1]]


def test_2x2_is_the_two_root_leaves():
    d = np.ones((2, 2), dtype=np.float32)
    assert A.adaptive_triangles(d, max_error=0.0).tolist() == [[3, 0, 2], [0, 3, 1]]
    d[1, 0] = np.nan
    assert A.adaptive_triangles(d, max_error=None).tolist() == [[0, 3, 1]]


def test_plane_counts():
    d, inv = _exact_plane_inverse(17, 17)
    assert A.adaptive_triangles(d, inverse=inv, max_error=0.0).shape[0] == 2
    d, inv = _exact_plane_inverse(12, 19)      # refined along the border by the absent vertices
    assert A.adaptive_triangles(d, inverse=inv, max_error=0.0).shape[0] == 82


# ---------------------------------------------------------------- properties
CASES = [dict(), dict(mask=True), dict(max_ratio=1.3), dict(inverse=(0.9, 0.1)), dict(mask=True, max_ratio=1.3, inverse=(0.9, 0.1))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", range(len(CASES)))
def test_properties(shape, case):
    h, w = shape
    kw = dict(CASES[case])
    d = _scene(h, w, 7 * case + h)
    if "inverse" in kw:
        d = np.clip(d / d.max(), 0.0, 1.0).astype(np.float32)
    if kw.pop("mask", False):
        kw["mask"] = _mask(h, w)
    meshes, E = A.sweep(d, TAUS, **kw)
    assert not np.isnan(E).any() and (E >= 0).all()
    finest = meshes[None]
    if "mask" not in kw and "max_ratio" not in kw:
        assert finest.shape[0] == 2 * (h - 1) * (w - 1)
    cover0 = _cells(finest, w, h)
    assert cover0.max() <= 1
    om = A.disparity(d, kw.get("inverse"))
    levels = 2 * (A.grid_side(h, w).bit_length() - 1) + 1
    order = sorted((t for t in TAUS if t is not None))
    prev = None
    for tau in [None] + order:
        tri = meshes[tau]
        p = _coords(tri, w)
        assert tri.shape[0] == 0 or (tri.min() >= 0 and tri.max() < h * w)
        assert (_twice_area(p) > 0).all()      # create_triangles' (tl, bl, tr) has +1 in (row, column) coordinates
        _assert_conforming(tri, w)
        cover = _cells(tri, w, h)
        assert np.array_equal(cover, cover0), tau      # the same cover as the finest mesh, nothing twice
        if prev is not None:
            assert tri.shape[0] <= prev.shape[0]      # non-increasing in tau
            # nested: every triangle of the finer mesh lies inside one triangle of the coarser one -- the coarser one's are unions of the finer one's
            owner = -np.ones((h - 1, w - 1, 4), dtype=np.int64)
            for k in range(tri.shape[0]):
                c = _cells(tri[k:k + 1], w, h) > 0
                owner[c] = k
            for k in range(prev.shape[0]):
                c = _cells(prev[k:k + 1], w, h) > 0
                assert len(set(owner[c].tolist())) == 1
        prev = tri
        if tau is None:
            continue
        # the deviation cap: |omega_lin - omega| <= (levels - 1) tau max(omega) at every grid vertex inside a triangle
        cap = (levels - 1) * tau * om[np.isfinite(om)].max()
        for t in p:
            i0, i1, j0, j1 = t[:, 0].min(), t[:, 0].max(), t[:, 1].min(), t[:, 1].max()
            ii, jj = np.mgrid[i0:i1 + 1, j0:j1 + 1]
            A2 = float(_twice_area(t[None])[0])
            l0 = ((t[2, 0] - t[1, 0]) * (jj - t[1, 1]) - (t[2, 1] - t[1, 1]) * (ii - t[1, 0])) / A2      # the weight of a vertex: the area opposite it
            l1 = ((t[0, 0] - t[2, 0]) * (jj - t[2, 1]) - (t[0, 1] - t[2, 1]) * (ii - t[2, 0])) / A2
            l2 = 1.0 - l0 - l1
            inside = (l0 >= -1e-9) & (l1 >= -1e-9) & (l2 >= -1e-9)
            lin = l0 * om[t[0, 0], t[0, 1]] + l1 * om[t[1, 0], t[1, 1]] + l2 * om[t[2, 0], t[2, 1]]
            dev = np.abs(lin - om[i0:i1 + 1, j0:j1 + 1])[inside]
            assert dev.max() <= cap + 1e-12, (tau, dev.max(), cap)
