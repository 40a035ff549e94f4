"""Plain numpy / Python restatement of what hip_ext.masks computes, for the tests (no scipy, no cv2: neither has to exist where the GPU tests run).

    label(mask, connectivity)            two-pass union-find labelling, components numbered 1..n in the raster order of their first pixel
    stats(labels, cap)                   cv2.connectedComponentsWithStats' (LEFT, TOP, WIDTH, HEIGHT, AREA) rows and the (sum x, sum y) rows
    keep_area(mask, min_area, conn)      reference app.py:283-293, remove_small_noise: components of at least min_area pixels
    points(mask, thresh, step, conn)     reference app.py:81-97, get_points_from_components, over label()'s numbering

cv2's own numbering of the components is not documented; the point list depends on it only through the ORDER of the components, which here is the
raster order of their first pixels (scipy.ndimage.label's numbering, pinned in test_mask_components_cpu.py)."""
import numpy as np


def label(mask, connectivity=8):
    """int32 labels [h, w] (0 = background) and the component count.  Any non-zero element is inside."""
    if connectivity not in (4, 8):
        raise ValueError(connectivity)
    m = np.asarray(mask) != 0
    h, w = m.shape
    parent = list(range(h * w))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)      # the root is the component's first pixel in raster order

    earlier = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for y in range(h):
        for x in range(w):
            if not m[y, x]:
                continue
            for dy, dx in earlier:
                yy, xx = y + dy, x + dx
                if 0 <= yy and 0 <= xx < w and m[yy, xx]:
                    union(y * w + x, yy * w + xx)
    out = np.zeros((h, w), dtype=np.int32)
    number = {}
    for y in range(h):
        for x in range(w):
            if m[y, x]:
                r = find(y * w + x)
                if r not in number:            # first met at its first pixel: r == y * w + x
                    number[r] = len(number) + 1
                out[y, x] = number[r]
    return out, len(number)


def stats(labels, cap):
    """(stats int32 [cap + 1, 5], sums int64 [cap + 1, 2]) of labels 0..cap; pixels with a larger label are ignored; a row without pixels is zero."""
    labels = np.asarray(labels)
    h, w = labels.shape
    ys, xs = np.divmod(np.arange(h * w, dtype=np.int64), w)
    lab = labels.ravel().astype(np.int64)
    ok = (lab >= 0) & (lab <= cap)
    lab, ys, xs = lab[ok], ys[ok], xs[ok]
    area = np.bincount(lab, minlength=cap + 1).astype(np.int64)
    lo_x, lo_y = np.full(cap + 1, w, np.int64), np.full(cap + 1, h, np.int64)
    hi_x, hi_y = np.full(cap + 1, -1, np.int64), np.full(cap + 1, -1, np.int64)
    np.minimum.at(lo_x, lab, xs)
    np.minimum.at(lo_y, lab, ys)
    np.maximum.at(hi_x, lab, xs)
    np.maximum.at(hi_y, lab, ys)
    sums = np.zeros((cap + 1, 2), dtype=np.int64)
    np.add.at(sums[:, 0], lab, xs)
    np.add.at(sums[:, 1], lab, ys)
    st = np.stack([lo_x, lo_y, hi_x - lo_x + 1, hi_y - lo_y + 1, area], axis=1)
    st[area == 0] = 0
    return st.astype(np.int32), sums


def keep_area(mask, min_area=500, connectivity=4):
    """uint8 0 / 1: the pixels of the components with area >= min_area."""
    lab, n = label(mask, connectivity)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = area >= min_area
    keep[0] = False
    return keep[lab].astype(np.uint8)


def points(mask, small_component_thresh=100, grid_step=10, connectivity=8):
    """int32 [P, 2] of (x, y); [0, 2] when there is none."""
    lab, n = label(mask, connectivity)
    selected = []
    for i in range(1, n + 1):
        ys, xs = np.nonzero(lab == i)
        area = ys.size
        if area < small_component_thresh:
            # int(centroid): the centroid is sum / area in double and non-negative, int() truncates
            selected.append([int(xs.sum() / area), int(ys.sum() / area)])
        else:
            min_x, max_x, min_y, max_y = xs.min(), xs.max(), ys.min(), ys.max()
            for y in range(min_y, max_y, grid_step):
                for x in range(min_x, max_x, grid_step):
                    if lab[y, x] == i:
                        selected.append([x, y])
    return np.asarray(selected, dtype=np.int32).reshape(-1, 2)


# ---- the mask contents the GPU tests share --------------------------------------------------------------------------------------------------

def serpentine(n):
    """n x n: even rows full, joined at alternating ends through the odd rows: one long winding component."""
    m = np.zeros((n, n), dtype=np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, n - 1, 2)):
        m[y, n - 1 if k % 2 == 0 else 0] = 1
    return m


def checkerboard(h, w):
    yy, xx = np.mgrid[:h, :w]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def diagonal_blocks(n, c, anti=False):
    """Two blocks touching only diagonally: rows/columns [c - 3, c] and [c + 1, c + 4] (mirrored left-right for the anti-diagonal twin)."""
    m = np.zeros((n, n), dtype=np.uint8)
    m[c - 3:c + 1, c - 3:c + 1] = 1
    m[c + 1:c + 5, c + 1:c + 5] = 1
    return np.ascontiguousarray(m[:, ::-1]) if anti else m


def comb(h, w):
    """Teeth in every other column, joined only by the last row."""
    m = np.zeros((h, w), dtype=np.uint8)
    m[:, 0::2] = 1
    m[h - 1] = 1
    return m


def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[:h, :w]
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1.0).astype(np.uint8)


def random_mask(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)
