"""fp64 numpy restatement of include/ada_hip.h's "Guided filter" section: the oracle of tests/test_guided_cpu.py and tests/test_gpu_guided.py.

coefficients() walks every window directly and solves with numpy.linalg.solve; coefficients_prefix() is a second restatement on prefix sums (integral
images) and one batched solve.  apply() spells the source coordinate, the tap order, the weights and the final sum exactly as the contract does, so from
given coefficients it is reproduced bit for bit.  Nothing here knows how the kernels order their sums."""
import numpy as np


def votes(p, valid=None):
    v = ~np.isnan(p)
    return v if valid is None else v & (np.asarray(valid) != 0)


def sample_guide(guide, h, w):
    """fp64 [B, h, w, C]: the guide's sample of every map pixel, I[((2 y + 1) gh) // (2 h), ((2 x + 1) gw) // (2 w)]."""
    g = np.asarray(guide)
    gh, gw = g.shape[1:3]
    ys = ((2 * np.arange(h) + 1) * gh) // (2 * h)
    xs = ((2 * np.arange(w) + 1) * gw) // (2 * w)
    return g[:, ys][:, :, xs].astype(np.float64)


def _mean_fits(ab, has, r):
    B, h, w, _ = ab.shape
    coeff = np.zeros_like(ab)
    covered = np.zeros((B, h, w), np.uint8)
    for b in range(B):
        for y in range(h):
            ys = slice(max(y - r, 0), min(y + r, h - 1) + 1)
            for x in range(w):
                xs = slice(max(x - r, 0), min(x + r, w - 1) + 1)
                m = has[b, ys, xs]
                n = int(m.sum())
                if n:
                    coeff[b, y, x] = ab[b, ys, xs][m].sum(axis=0) / n
                    covered[b, y, x] = 1
    return coeff, covered


def coefficients(p, guide, r, eps, valid=None):
    """(coeff fp64 [B, h, w, C + 1], covered uint8 [B, h, w]) by direct windows.  p fp32 [B, h, w]; guide uint8 / fp32 [B, gh, gw, C]; eps in raw units."""
    p = np.asarray(p)
    B, h, w = p.shape
    I = sample_guide(guide, h, w)
    C = I.shape[-1]
    vote = votes(p, valid)
    pd = p.astype(np.float64)
    ab = np.zeros((B, h, w, C + 1))
    has = np.zeros((B, h, w), bool)
    for b in range(B):
        for y in range(h):
            ys = slice(max(y - r, 0), min(y + r, h - 1) + 1)
            for x in range(w):
                xs = slice(max(x - r, 0), min(x + r, w - 1) + 1)
                v = vote[b, ys, xs]
                n = int(v.sum())
                if not n:
                    continue
                Iv, pv = I[b, ys, xs][v], pd[b, ys, xs][v]
                mI, mp = Iv.sum(axis=0) / n, pv.sum() / n
                cov = (Iv[:, :, None] * Iv[:, None, :]).sum(axis=0) / n - np.outer(mI, mI)
                cp = (Iv * pv[:, None]).sum(axis=0) / n - mI * mp
                a = np.linalg.solve(cov + eps * np.eye(C), cp)
                ab[b, y, x, :C], ab[b, y, x, C] = a, mp - a @ mI
                has[b, y, x] = True
    return _mean_fits(ab, has, r)


def _box(planes, r):
    """Window sums of [B, h, w, M] planes over the clipped (2 r + 1)^2 windows, by prefix sums."""
    B, h, w, M = planes.shape
    S = np.zeros((B, h + 1, w + 1, M))
    S[:, 1:, 1:] = planes.cumsum(axis=1).cumsum(axis=2)
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r, h - 1) + 1
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r, w - 1) + 1
    return S[:, y1][:, :, x1] - S[:, y0][:, :, x1] - S[:, y1][:, :, x0] + S[:, y0][:, :, x0]


def coefficients_prefix(p, guide, r, eps, valid=None):
    """coefficients() restated on prefix sums and one batched solve."""
    p = np.asarray(p)
    B, h, w = p.shape
    I = sample_guide(guide, h, w)
    C = I.shape[-1]
    vote = votes(p, valid)
    Iv = np.where(vote[..., None], I, 0.0)
    pv = np.where(vote, p.astype(np.float64), 0.0)
    n = _box(vote[..., None].astype(np.float64), r)[..., 0]
    has = n > 0.5
    nn = np.where(has, n, 1.0)
    mI = _box(Iv, r) / nn[..., None]
    mp = _box(pv[..., None], r)[..., 0] / nn
    cov = _box((Iv[..., :, None] * Iv[..., None, :]).reshape(B, h, w, C * C), r).reshape(B, h, w, C, C) / nn[..., None, None] - mI[..., :, None] * mI[..., None, :]
    cp = _box(Iv * pv[..., None], r) / nn[..., None] - mI * mp[..., None]
    a = np.linalg.solve(cov + eps * np.eye(C), cp[..., None])[..., 0]
    ab = np.concatenate([a, (mp - (a * mI).sum(axis=-1))[..., None]], axis=-1)
    ab = np.where(has[..., None], ab, 0.0)
    m = _box(has[..., None].astype(np.float64), r)[..., 0]
    covered = m > 0.5
    coeff = np.where(covered[..., None], _box(ab, r) / np.where(covered, m, 1.0)[..., None], 0.0)
    return coeff, covered.astype(np.uint8)


def source(n_out, n_in):
    """Source coordinates of the outputs 0 .. n_out - 1 on an axis of n_in samples: the contract's expression, verbatim."""
    X = np.arange(n_out).astype(np.float64)
    s = ((X + 0.5) * n_in) / n_out - 0.5
    return np.clip(s, 0.0, float(n_in - 1))


def apply(coeff, covered, guide, fill=np.nan):
    """fp32 [B, H, W]: the apply pass from given coefficients, bit for bit."""
    coeff, covered, g = np.asarray(coeff), np.asarray(covered) != 0, np.asarray(guide)
    B, h, w, C1 = coeff.shape
    H, W, C = g.shape[1:]
    assert C1 == C + 1 and H >= h and W >= w
    sy, sx = source(H, h), source(W, w)
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    fy, fx = (sy - y0)[:, None], (sx - x0)[None, :]
    taps = [(y0, x0, (1.0 - fy) * (1.0 - fx)), (y0, x1, (1.0 - fy) * fx), (y1, x0, fy * (1.0 - fx)), (y1, x1, fy * fx)]
    acc = np.zeros((B, H, W, C1))
    wsum = np.zeros((B, H, W))
    dropped = np.zeros((B, H, W), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for ty, tx, wt in taps:
            wt = np.broadcast_to(wt, (H, W))
            cov = covered[:, ty][:, :, tx]
            use = (wt > 0.0) & cov
            dropped |= (wt > 0.0) & ~cov
            wsum = wsum + np.where(use, wt, 0.0)
            acc = acc + np.where(use[..., None], wt[..., None] * coeff[:, ty][:, :, tx], 0.0)
        renorm = dropped & (wsum > 0.0)
        acc = np.where(renorm[..., None], acc / np.where(renorm, wsum, 1.0)[..., None], acc)
        gd = g.astype(np.float64)
        v = acc[..., 0] * gd[..., 0]
        for c in range(1, C):
            v = v + acc[..., c] * gd[..., c]
        v = v + acc[..., C]
        return np.where(wsum > 0.0, v.astype(np.float32), np.float32(fill)).astype(np.float32)


def guided(p, guide, r, eps, valid=None, fill=np.nan, fit=coefficients):
    """(q fp32 [B, H, W], covered uint8 [B, h, w]): both passes."""
    coeff, covered = fit(p, guide, r, eps, valid)
    return apply(coeff, covered, guide, fill), covered


def raw_eps(eps, guide):
    """A user's eps in the guide's raw units: times 255^2 for a uint8 guide."""
    return eps * 65025.0 if np.asarray(guide).dtype == np.uint8 else eps


def bound(q_ref, p):
    """The contract's tolerance: one fp32 spacing at max(|q_ref|, max |p|) -- both sides round one fp64 value that differs in summation order alone."""
    p = np.asarray(p)
    pmax = np.max(np.abs(p[np.isfinite(p)]), initial=0.0)
    with np.errstate(invalid="ignore"):
        return np.spacing(np.maximum(np.abs(np.nan_to_num(q_ref, nan=0.0)), pmax).astype(np.float32))


def assert_close(q, q_ref, p, what=""):
    """|q - q_ref| <= bound everywhere, NaN (fill) positions identical; no pixel is left out."""
    q, q_ref = np.asarray(q), np.asarray(q_ref)
    assert q.shape == q_ref.shape and q.dtype == np.float32, (what, q.shape, q_ref.shape, q.dtype)
    assert np.array_equal(np.isnan(q), np.isnan(q_ref)), f"{what}: fill positions differ"
    ok = ~np.isnan(q_ref)
    err = np.abs(q.astype(np.float64) - q_ref.astype(np.float64))[ok]
    lim = bound(q_ref, p)[ok].astype(np.float64)
    worst = float((err / lim).max()) if err.size else 0.0
    print(f"{what}: max |q - q_ref| = {float(err.max()) if err.size else 0.0:.3e}, worst error / bound = {worst:.3f}")
    assert (err <= lim).all(), f"{what}: {int((err > lim).sum())} pixels beyond the bound, worst {worst:.3f} x"
