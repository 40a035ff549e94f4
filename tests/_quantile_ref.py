"""Sort-based numpy restatements of what hip_ext.quantile, hip_ext.image.colorize and src.util.depth_transform compute on the device.

Each one is pinned on the CPU (tests/test_quantile_cpu.py): the two quantile rules against np.percentile / torch.quantile bit for bit, the colour rule
against matplotlib's cmap(t, bytes=True), colorize and the normalizer against goldens written by the reference's own functions
(tools/make_golden_quantile.py).  The GPU tests compare the device against these.
"""
from fractions import Fraction

import numpy as np

F32 = np.float32


def population(x, valid=None, exclude_value=None, positive_only=False):
    """The elements of ``x`` (any shape, fp32) that ada_quantile_fwd includes, as a 1-D fp32 array."""
    x = np.asarray(x, dtype=F32).reshape(-1)
    keep = np.ones(x.shape, bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    with np.errstate(invalid="ignore"):
        if exclude_value is not None:
            keep &= x.astype(np.float64) != np.float64(exclude_value)      # in double: fp32(0.1) is not 0.1
        if positive_only:
            keep &= x > 0
    return x[keep]


def quantile_numpy(pop, q):
    """np.percentile(pop.astype(float64), 100 q) ('linear') restated on a sorted copy: fp64 rank, fp64 lerp, each operation rounded on its own."""
    pop = np.asarray(pop, dtype=F32).reshape(-1)
    if pop.size == 0 or np.isnan(pop).any():
        return np.float64(np.nan)
    s = np.sort(pop).astype(np.float64)
    cnt = s.size
    v = np.float64(cnt - 1) * np.float64(q)
    j = int(np.floor(v))
    g = v - np.floor(v)
    a, b = s[j], s[min(j + 1, cnt - 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return np.float64(b - d * (1 - g) if g >= 0.5 else a + d * g)


def _round_f32(fr):
    """The fp32 nearest to the exact rational ``fr`` (ties to even); fr != 0 and within fp32's range."""
    c = F32(float(fr))
    best = None
    for cand in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - fr)
        even = (int(cand.view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, cand, even)
    return best[1]


def fmaf(a, b, c):
    """fp32 a * b + c with ONE rounding, as the hardware's fused multiply-add: exact rational arithmetic for finite operands."""
    a, b, c = F32(a), F32(b), F32(c)
    with np.errstate(invalid="ignore", over="ignore"):
        plain = F32(F32(a * b) + c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return plain
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        return plain        # the sign of an exact zero follows the plain sum
    return _round_f32(exact)


def quantile_torch(pop, q, fused=True):
    """torch.quantile(pop, float32(q)) on the CPU restated: fp32 rank, neighbours at its floor and ceil, ATen's lerp -- whose CPU kernel fuses the product into
    the sum (fmadd) while hi - lo and 1 - w are rounded on their own.  fused=False: the product rounded before the sum, what a build without FMA would
    compute; it is NOT what torch.quantile returns where these tests run (test_quantile_cpu.py keeps the count of draws on which the two differ)."""
    pop = np.asarray(pop, dtype=F32).reshape(-1)
    if pop.size == 0 or np.isnan(pop).any():
        return F32(np.nan)
    s = np.sort(pop)
    r = F32(q) * F32(s.size - 1)
    lo, hi = s[int(np.floor(r))], s[int(np.ceil(r))]
    w = F32(r - np.floor(r))
    with np.errstate(invalid="ignore", over="ignore"):
        d = F32(hi - lo)
        if not fused:
            return F32(lo + F32(w * d)) if w < F32(0.5) else F32(hi - F32(d * F32(F32(1) - w)))
        if w < F32(0.5):
            return fmaf(w, d, lo)
        return fmaf(-d, F32(F32(1) - w), hi)


def colour_index(t):
    """The table entry matplotlib's cmap(t, bytes=True) shows for t in double: min(int(t * 256), 255), below 0 entry 0, from 1 on entry 255; -1 for NaN."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        idx = np.where(t < 0, 0, np.where(t >= 1, 255, np.minimum((np.where(np.isfinite(t), t, 0.0) * 256).astype(np.int64), 255)))
    return np.where(np.isnan(t), -1, idx)


def rgba_lut(cmap):
    import matplotlib
    return np.ascontiguousarray(matplotlib.colormaps[cmap](np.arange(256), bytes=True))


def colorize(value, vmin=None, vmax=None, cmap="turbo_r", invalid_val=-99, invalid_mask=None, background_color=(128, 128, 128, 255), vminp=2, vmaxp=95):
    """The reference's colorize() (src/scripts/colorize_depth.py:18-84) on one fp32 map [H, W] promoted to float64: uint8 [H, W, 4]."""
    value = np.asarray(value, dtype=F32)
    v = value.astype(np.float64)
    invalid = (v == invalid_val) if invalid_mask is None else np.asarray(invalid_mask) != 0
    pop = value[~invalid]
    vmin = quantile_numpy(pop, vminp / 100) if vmin is None else np.float64(vmin)
    vmax = quantile_numpy(pop, vmaxp / 100) if vmax is None else np.float64(vmax)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (v - vmin) / (vmax - vmin) if vmin != vmax else v * 0.0
    idx = colour_index(t)
    lut = rgba_lut(cmap)
    out = np.where((idx < 0)[..., None], np.zeros(4, np.uint8), lut[np.maximum(idx, 0)])
    out[invalid] = np.asarray(background_color, dtype=np.uint8)
    return np.ascontiguousarray(out.astype(np.uint8))


def range_map(depth, lo, hi, scale, shift, clip=None):
    """((depth - lo) / (hi - lo)) * scale + shift in fp32, every operation rounded; ``clip`` = (lo, hi) clamps, NaN stays NaN."""
    depth = np.asarray(depth, dtype=F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        out = (depth - F32(lo)) / F32(F32(hi) - F32(lo))
        out = out * F32(scale)
        out = out + F32(shift)
        if clip is not None:
            out = np.where(out < F32(clip[0]), F32(clip[0]), np.where(out > F32(clip[1]), F32(clip[1]), out))
    return out.astype(F32)


def normalizer_range(depth, valid=None, min_max_quantile=0.02):
    """(near, far) of ScaleShiftDepthNormalizer: torch.quantile at fp32(q) and fp32(1.0 - q) over valid & depth > 0 of the whole array."""
    pop = population(depth, valid, positive_only=True)
    return quantile_torch(pop, F32(min_max_quantile)), quantile_torch(pop, F32(1.0 - min_max_quantile))


def normalize(depth, valid=None, norm_min=-1.0, norm_max=1.0, min_max_quantile=0.02, clip=True, per_image=False):
    """ScaleShiftDepthNormalizer.__call__ (src/util/depth_transform.py:73-96) in fp32 numpy; per_image: dim 0 is a batch of independent maps."""
    depth = np.asarray(depth, dtype=F32)
    if per_image:
        return np.stack([normalize(depth[i], None if valid is None else valid[i], norm_min, norm_max, min_max_quantile, clip) for i in range(depth.shape[0])])
    lo, hi = normalizer_range(depth, valid, min_max_quantile)
    return range_map(depth, lo, hi, norm_max - norm_min, norm_min, (norm_min, norm_max) if clip else None)
