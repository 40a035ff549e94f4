"""The rank-filter contract of include/ada_hip.h restated in numpy, by brute force: gather every sample of every window, sort, pick.

Samples of output pixel (y, x): the positions (y + dy, x + dx), |dy| <= kh // 2, |dx| <= kw // 2, each axis mapped by the border rule ('mirror':
reflect-101 with the index reduced modulo the period 2 n - 2, index 0 for n == 1; 'nearest': clamped; 'ignore': dropped when outside).  A mapped position
votes when ``valid`` is None or non-zero there and the value is not NaN; duplicates vote once each.  Of the n voting samples sorted ascending the result is
s[0] ('min'), s[n - 1] ('max'), s[n // 2] ('median') or s[p (n - 1) // 100] (an integer percent p); ``fill`` where n == 0.

Nothing here is shared with the implementation: no keys, no separable passes, no selection -- np.sort over the stacked samples (NaN marks a sample that
does not vote and sorts last; fp32 and uint8 are exact in float64), and for windows too large to stack a running np.fmin / np.fmax over the positions.
"""
import numpy as np

BORDERS = ("mirror", "nearest", "ignore")
STACK_LIMIT = 81      # windows up to this many samples are stacked and sorted


def window(size):
    kh, kw = (size, size) if np.ndim(size) == 0 else size
    return int(kh), int(kw)


def map_index(i, n, border):
    """Image indices of the positions ``i`` along an axis of n samples; -1 = dropped."""
    i = np.asarray(i, dtype=np.int64)
    if border == "ignore":
        return np.where((i >= 0) & (i < n), i, -1)
    if border == "nearest":
        return np.clip(i, 0, n - 1)
    assert border == "mirror", border
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def rank_index(n, rank):
    """r(n) for an array of counts n >= 1, in integers."""
    n = np.asarray(n, dtype=np.int64)
    if rank == "min":
        return np.zeros_like(n)
    if rank == "max":
        return n - 1
    if rank == "median":
        return n // 2
    p = int(rank)
    assert 0 <= p <= 100, rank
    return (p * (n - 1)) // 100


def planes(x, size, border, valid=None):
    """Yields, per window position, (values float64 [B, h, w] with NaN where the sample does not vote)."""
    kh, kw = window(size)
    assert kh % 2 == 1 and kw % 2 == 1
    B, h, w = x.shape
    xf = x.astype(np.float64)
    votes = ~np.isnan(xf) if valid is None else (~np.isnan(xf) & (valid != 0))
    xf = np.where(votes, xf, np.nan)
    for dy in range(-(kh // 2), kh // 2 + 1):
        ys = map_index(np.arange(h) + dy, h, border)
        for dx in range(-(kw // 2), kw // 2 + 1):
            xs = map_index(np.arange(w) + dx, w, border)
            plane = xf[:, np.maximum(ys, 0)[:, None], np.maximum(xs, 0)[None, :]]
            plane[:, ys < 0, :] = np.nan
            plane[:, :, xs < 0] = np.nan
            yield plane


def sorted_windows(x, size, border, valid=None):
    """(s float64 [kh kw, B, h, w] ascending with the non-voting samples (NaN) last, n int32 [B, h, w]) of a [B, h, w] map."""
    s = np.sort(np.stack(list(planes(x, size, border, valid))), axis=0)
    return s, (~np.isnan(s)).sum(axis=0).astype(np.int32)


def pick(s, n, rank, dtype, fill=None):
    """The contract's result from sorted_windows' output, in ``dtype``."""
    if fill is None:
        fill = np.nan if np.dtype(dtype) == np.float32 else 0
    r = rank_index(np.maximum(n, 1), rank)
    val = np.take_along_axis(s, r[None], axis=0)[0]
    out = np.where(n > 0, val, np.float64(fill))
    with np.errstate(invalid="ignore"):
        return out.astype(dtype)


def extremes(x, size, border, valid=None):
    """(minimum float64, maximum float64, n int32), NaN where n == 0: a running fmin / fmax over the window's positions, any window size."""
    lo = hi = n = None
    for plane in planes(x, size, border, valid):
        v = ~np.isnan(plane)
        if lo is None:
            lo, hi, n = plane.copy(), plane.copy(), v.astype(np.int32)
        else:
            lo, hi, n = np.fmin(lo, plane), np.fmax(hi, plane), n + v
    return lo, hi, n


def rank_filter(x, size, rank="median", border="mirror", valid=None, fill=None):
    """(out of x's dtype and shape, count int32): x fp32 or uint8, [h, w] or [B, h, w]."""
    x = np.asarray(x)
    single = x.ndim == 2
    x3 = x[None] if single else x
    v3 = None if valid is None else (np.asarray(valid)[None] if single else np.asarray(valid))
    kh, kw = window(size)
    if kh * kw <= STACK_LIMIT:
        s, n = sorted_windows(x3, size, border, v3)
        out = pick(s, n, rank, x.dtype, fill)
    else:
        assert rank in ("min", "max"), "only the extremes are defined for windows this large"
        lo, hi, n = extremes(x3, size, border, v3)
        if fill is None:
            fill = np.nan if x.dtype == np.float32 else 0
        with np.errstate(invalid="ignore"):
            out = np.where(n > 0, lo if rank == "min" else hi, np.float64(fill)).astype(x.dtype)
    return (out[0], n[0]) if single else (out, n)


def _binary(masks, size, steps, iterations):
    cur = (np.asarray(masks) != 0).astype(np.uint8)
    for rank in steps:
        for _ in range(iterations):
            cur = rank_filter(cur, size, rank, "ignore")[0]
    return cur


def erode(masks, size=3, iterations=1):
    return _binary(masks, size, ("min",), iterations)


def dilate(masks, size=3, iterations=1):
    return _binary(masks, size, ("max",), iterations)


def opening(masks, size=3, iterations=1):
    return _binary(masks, size, ("min", "max"), iterations)


def closing(masks, size=3, iterations=1):
    return _binary(masks, size, ("max", "min"), iterations)
