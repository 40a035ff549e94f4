"""Plain numpy restatement of what hip_ext.edges and the edge metrics of src/util/metric.py compute, for the tests (no scipy, no skimage: neither has to
exist where the GPU tests run).  test_edges_cpu.py pins it against scipy.ndimage where scipy exists.

    correlate1d(a, weights, axis, mode)     scipy's 1-D correlation: fp64 accumulation in scipy's order (centre tap, then the symmetric or antisymmetric
                                            pairs from the outermost inwards), stored in the array's dtype
    gaussian / smooth / sobel / magnitude   the stages of skimage.feature.canny on a float32 image (mode 'constant', mask=None)
    nms / hysteresis / canny / stages       the bilinear non-maximum suppression, the double threshold over _components_ref.label, the detector
    edt                                     brute-force exact Euclidean distance transform: integer squared distances, one fp64 square root
    edge_acc_comp / soft_edge_error         the semantics of reference src/util/metric.py:238-256 and :303-328, restated independently
    margins / tau / undecided               how far every decision of the detector is from flipping, and the rounding allowance it is compared with
    scene / SEEDS                           the synthetic depth scenes of the end-to-end tests and the seeds whose scenes have no undecided pixel

skimage is not installed where this was written.  ``nms`` and ``canny`` restate the algorithm of skimage 0.19 - 0.24 (skimage/feature/_canny.py and
_canny_cy.pyx: _preprocess with the bleed-over normalisation, ndi.sobel, _nonmaximum_suppression_bilinear, ndi.label hysteresis); the test that pins
them against skimage.feature.canny is skipped without skimage, so the restatement of the suppression is UNPINNED until the suite runs somewhere skimage
exists.  One thing to look at first should that pin fail: the suppression's weight is divided in fp64 here and in the kernel; if skimage rounds the
quotient of its two float32 values to float32, the difference (2^-24 relative) can flip only pixels that ``undecided`` already reports.  Everything that rests on scipy alone (correlate1d, gaussian, sobel, label, edt) is pinned bit for bit.

One documented difference from scipy: ``edt`` of a map without any edge pixel is +inf everywhere (scipy's output there is an artefact of its
implementation)."""
import numpy as np

import _components_ref as C

EPS32 = np.finfo(np.float32).eps


# ---- scipy.ndimage's 1-D correlation ----------------------------------------------------------------------------------------------------------

def correlate1d(a, weights, axis, mode):
    """scipy.ndimage.correlate1d for an odd, symmetric or antisymmetric ``weights``; mode 'constant' (zeros) or 'reflect' (d c b a | a b c d)."""
    a = np.asarray(a)
    w = np.asarray(weights, dtype=np.float64)
    r = len(w) // 2
    assert len(w) == 2 * r + 1
    sym = all(w[r + k] == w[r - k] for k in range(1, r + 1))
    anti = all(w[r + k] == -w[r - k] for k in range(1, r + 1))
    assert sym or anti, "only the two forms scipy special-cases are restated"
    x = np.moveaxis(a, axis, -1).astype(np.float64)
    n = x.shape[-1]
    pad = [(0, 0)] * (x.ndim - 1) + [(r, r)]
    xp = np.pad(x, pad, mode="constant") if mode == "constant" else np.pad(x, pad, mode="symmetric")
    t = xp[..., r:r + n] * w[r]
    for k in range(r, 0, -1):                       # scipy: for jj in -size1 .. -1:  tmp += (iline[jj] +- iline[-jj]) * fw[jj]
        left, right = xp[..., r - k:r - k + n], xp[..., r + k:r + k + n]
        t = t + ((left + right) if sym else (left - right)) * w[r - k]
    return np.moveaxis(t.astype(a.dtype), -1, axis)


def gaussian_weights(sigma):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, int(4 sigma + 0.5))."""
    sigma = float(sigma)
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def gaussian(image, sigma):
    """scipy.ndimage.gaussian_filter(image, sigma, mode='constant'): axis 0, then axis 1, each pass stored in the image's dtype."""
    w = gaussian_weights(sigma)
    return correlate1d(correlate1d(image, w, 0, "constant"), w, 1, "constant")


def smooth(image, sigma):
    """skimage's _preprocess with mode 'constant' and no mask: the Gaussian divided by (the Gaussian of a map of ones + eps)."""
    bleed = gaussian(np.ones(image.shape, dtype=image.dtype), sigma) + np.finfo(image.dtype).eps
    out = gaussian(image, sigma)
    out /= bleed
    return out


def sobel(a, axis):
    """scipy.ndimage.sobel(a, axis) with its default mode 'reflect'."""
    out = correlate1d(a, [-1.0, 0.0, 1.0], axis, "reflect")
    for other in range(a.ndim):
        if other != axis:
            out = correlate1d(out, [1.0, 2.0, 1.0], other, "reflect")
    return out


def magnitude(isobel, jsobel):
    m = isobel * isobel
    m += jsobel * jsobel
    np.sqrt(m, out=m)
    return m


# ---- skimage's bilinear non-maximum suppression -----------------------------------------------------------------------------------------------

def _shifted(m, dy, dx):
    """out[y, x] = m[y + dy, x + dx] (anything outside: 0; never used off the border ring)."""
    p = np.pad(m, 1, mode="constant")
    h, w = m.shape
    return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def _nms_parts(isobel, jsobel, mag, low):
    """Everything the suppression decides with: (eligible, plus, minus, mag64, abs_i, abs_j).  ``plus`` / ``minus``: the interpolated neighbours in fp64."""
    h, w = mag.shape
    eroded = np.zeros((h, w), dtype=bool)
    eroded[1:-1, 1:-1] = True
    eligible = eroded & (mag >= np.float32(low))
    down, up, left, right = isobel <= 0, isobel >= 0, jsobel <= 0, jsobel >= 0
    cond1 = (up & right) | (down & left)
    cond2 = (down & right) | (up & left)
    eligible &= cond1 | cond2
    ai, aj = np.abs(isobel).astype(np.float64), np.abs(jsobel).astype(np.float64)
    m64 = mag.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        w_ji, w_ij = aj / ai, ai / aj
    case_a = cond1 & (ai > aj)
    case_b = cond1 & ~(ai > aj)
    case_c = ~cond1 & cond2 & (ai < aj)
    wgt = np.where(case_a, w_ji, np.where(case_b, w_ij, np.where(case_c, w_ij, w_ji)))

    def pick(a, b, c, d):
        return np.where(case_a, _shifted(m64, *a), np.where(case_b, _shifted(m64, *b), np.where(case_c, _shifted(m64, *c), _shifted(m64, *d))))
    n11 = pick((1, 0), (0, 1), (0, 1), (-1, 0))
    n12 = pick((1, 1), (1, 1), (-1, 1), (-1, 1))
    n21 = pick((-1, 0), (0, -1), (0, -1), (1, 0))
    n22 = pick((-1, -1), (-1, -1), (1, -1), (1, -1))
    with np.errstate(invalid="ignore"):
        plus = n12 * wgt + n11 * (1.0 - wgt)
        minus = n22 * wgt + n21 * (1.0 - wgt)
    return eligible, plus, minus, m64, ai, aj


def nms(isobel, jsobel, mag, low):
    """skimage's _nonmaximum_suppression_bilinear with eroded_mask = everything off the one-pixel border ring: the magnitude where kept, else 0."""
    eligible, plus, minus, m64, _, _ = _nms_parts(isobel, jsobel, mag, low)
    with np.errstate(invalid="ignore"):
        keep = eligible & (plus <= m64) & (minus <= m64)
    return np.where(keep, mag, np.float32(0)).astype(mag.dtype)


def hysteresis(low_masked, high):
    """canny's double threshold: the 8-connected components of low_masked > 0 that hold a pixel with low_masked >= high (uint8 0 / 1)."""
    labels, count = C.label(low_masked > 0, 8)
    good = np.zeros(count + 1, dtype=bool)
    good[np.unique(labels[(low_masked > 0) & (low_masked >= np.float32(high))])] = True
    good[0] = False
    return good[labels].astype(np.uint8)


def stages(image, sigma=1.0, low=0.1, high=0.2):
    """Every stage of skimage.feature.canny(image float32, sigma, low, high): dict of smoothed, isobel, jsobel, magnitude, low_masked, edges."""
    image = np.ascontiguousarray(image)
    assert image.dtype == np.float32 and image.ndim == 2
    s = smooth(image, sigma)
    js, is_ = sobel(s, 1), sobel(s, 0)
    m = magnitude(is_, js)
    lm = nms(is_, js, m, low)
    return dict(smoothed=s, isobel=is_, jsobel=js, magnitude=m, low_masked=lm, edges=hysteresis(lm, high))


def canny(image, sigma=1.0, low=0.1, high=0.2):
    return stages(image, sigma, low, high)["edges"]


def to_log(d):
    """The reference's to_log on a float32 array, the logarithm evaluated in fp64 and rounded once."""
    d = np.asarray(d, dtype=np.float32)
    lg = np.log(np.maximum(d, EPS32).astype(np.float64)).astype(np.float32)
    return ((d > 0) * lg).astype(np.float32)


def to_log15(d):
    """extract_edges' default branch: log((d > 0) * max(d, eps)) / log(1.5), the division in float32; -inf where d <= 0."""
    d = np.asarray(d, dtype=np.float32)
    v = ((d > 0) * np.maximum(d, EPS32)).astype(np.float32)
    with np.errstate(divide="ignore"):
        lg = np.log(v.astype(np.float64)).astype(np.float32)
    return lg / np.float32(np.log(1.5))


# ---- distance transform and the metrics -------------------------------------------------------------------------------------------------------

def edt(edges):
    """scipy.ndimage.distance_transform_edt(np.logical_not(edges)) by brute force; +inf everywhere when there is no edge pixel."""
    e = np.asarray(edges) != 0
    h, w = e.shape
    ys, xs = np.nonzero(e)
    if ys.size == 0:
        return np.full((h, w), np.inf)
    py, px = np.divmod(np.arange(h * w, dtype=np.int64), w)
    best = np.empty(h * w, dtype=np.int64)
    step = max(1, (1 << 22) // ys.size)
    for i in range(0, h * w, step):
        dy = py[i:i + step, None] - ys[None, :]
        dx = px[i:i + step, None] - xs[None, :]
        best[i:i + step] = (dy * dy + dx * dx).min(axis=1)
    return np.sqrt(best.astype(np.float64)).reshape(h, w)


def edge_acc_comp(pred_edges, gt_edges, valid, th_acc=10, th_comp=10):
    """(EdgeAcc, EdgeComp) with the semantics of metric.py:238-256, over this module's edt.  The distance maps come from the edge maps as detected;
    only then are the invalid pixels dropped.  EdgeAcc is the mean distance to the ground-truth edges over the valid predicted edge pixels closer
    than th_acc; EdgeComp the mean distance to the predicted edges over ALL valid ground-truth edge pixels.  Without a close predicted edge pixel
    both are their thresholds; with one but no valid ground-truth edge pixel EdgeComp is the empty mean, NaN."""
    p, g, ok = np.asarray(pred_edges) != 0, np.asarray(gt_edges) != 0, np.asarray(valid) != 0
    to_gt, to_pred = edt(g), edt(p)
    close = p & ok & (to_gt < th_acc)
    g_ok = g & ok
    if not close.any():
        return float(th_acc), float(th_comp)
    acc = to_gt[close].sum() / np.count_nonzero(close)
    n_gt = np.count_nonzero(g_ok)
    comp = to_pred[g_ok].sum() / n_gt if n_gt else float("nan")
    return float(acc), float(comp)


def soft_edge_error(pred, gt, valid, radius=1):
    """(the float32 per-pixel map with the semantics of metric.py:303-324, its fp64 mean over the valid pixels -- NaN without one): per pixel the
    smallest |gt[y + dy, x + dx] - pred[y, x]| over |dy|, |dx| <= radius, a neighbour outside the map counting as 0.  Restated over a zero-padded
    copy of gt and its (2 r + 1)^2 windows; the difference and the absolute value stay in float32, NaN propagates through the minimum."""
    pred, gt = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    h, w = gt.shape
    padded = np.pad(gt, radius, mode="constant") if radius else gt
    see = np.full((h, w), np.inf, dtype=np.float32)
    for oy in range(2 * radius + 1):
        for ox in range(2 * radius + 1):
            see = np.minimum(see, np.abs(padded[oy:oy + h, ox:ox + w] - pred))
    sel = see[np.asarray(valid) != 0].astype(np.float64)
    return see, (float(sel.sum() / sel.size) if sel.size else float("nan"))


# ---- how far the detector's decisions are from flipping ---------------------------------------------------------------------------------------

def margins(image, sigma=1.0, low=0.1, high=0.2):
    """Per pixel, the smallest distance of any decision the detector takes there from flipping (inf where it takes none: the border ring):
    |magnitude - low|; where the suppression goes on, ||isobel| - |jsobel|| (the sector) and |interpolated - magnitude| for each side that is
    evaluated (the second only when the first passed); |magnitude - high| for kept pixels."""
    st = stages(image, sigma, low, high)
    is_, js, m = st["isobel"], st["jsobel"], st["magnitude"]
    eligible, plus, minus, m64, ai, aj = _nms_parts(is_, js, m, low)
    h, w = m.shape
    out = np.full((h, w), np.inf)
    inner = np.zeros((h, w), dtype=bool)
    inner[1:-1, 1:-1] = True
    out[inner] = np.abs(m64 - float(np.float32(low)))[inner]
    with np.errstate(invalid="ignore"):
        d_plus, d_minus = np.abs(plus - m64), np.abs(minus - m64)
        first = eligible & (plus <= m64)
    for sel, val in ((eligible, np.abs(ai - aj)), (eligible, d_plus), (first, d_minus), (st["low_masked"] > 0, np.abs(m64 - float(np.float32(high))))):
        val = np.where(np.isnan(val), 0.0, val)
        out[sel] = np.minimum(out[sel], val[sel])
    return out


def tau(image):
    """The rounding allowance of a magnitude: a smoothed value one fp32 ulp off passes through Sobel's gain of 8 in each derivative and sqrt(2) in the
    magnitude, about 12 ulps of the image's scale; as much again for the magnitude's own three roundings; rounded up to 32."""
    return 32.0 * float(EPS32) * max(1.0, float(np.abs(image).max()))


def undecided(image, sigma=1.0, low=0.1, high=0.2):
    """bool map: the pixels where some decision sits within tau of flipping."""
    return margins(image, sigma, low, high) < tau(image)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------

def scene(seed, h, w):
    """A float32 depth map in [0.05, 0.95]: a ramp plus a sine plus three discs of constant depth plus 0.004 of noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    ang = rng.uniform(0, 2 * np.pi)
    d = 0.5 + 0.3 * ((xx / max(w - 1, 1) - 0.5) * np.cos(ang) + (yy / max(h - 1, 1) - 0.5) * np.sin(ang))
    d += 0.06 * np.sin(2 * np.pi * (rng.uniform(0.5, 2.0) * xx / w + rng.uniform(0.5, 2.0) * yy / h) + rng.uniform(0, 2 * np.pi))
    for _ in range(3):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        rad = rng.uniform(min(h, w) / 8.0, min(h, w) / 3.0)
        d[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = rng.uniform(0.05, 0.95)
    d += 0.004 * rng.standard_normal((h, w))
    return np.clip(d, 0.05, 0.95).astype(np.float32)


# seeds whose scene, after to_log, has NO undecided pixel and at least 30 edge pixels (asserted in test_edges_cpu.py); three per shape
SEEDS = {(33, 41): (0, 1, 2), (47, 61): (0, 1, 4)}
