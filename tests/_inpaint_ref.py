"""numpy restatement of the hole-filling contract (include/ada_hip.h, "Hole filling"; DESIGN.md, "Hole filling"): the nearest valid pixel by brute force
with the tie rule, the copy of its value, and the push-pull fill in np.float32 with the contract's operation order.  Slow on purpose: nothing here
shares a line of reasoning with csrc/ada_inpaint.hip's two-pass transform."""
import numpy as np

NONE = 0x7fffffff
F = np.float32


def _batched(a, nd):
    a = np.asarray(a)
    return (a[None], True) if a.ndim == nd - 1 else (a, False)


def nearest_valid_ref(valid):
    """valid [h, w] or [B, h, w], non-zero = valid -> (index int32, dist2 int32) of that shape: the flat position r * w + c of the nearest valid pixel and the
    exact squared distance; among equally near pixels the smallest flat position (argmin returns the first of the candidates, listed in flat order);
    -1 and 0x7fffffff for an image without a valid pixel."""
    v, single = _batched(valid, 3)
    B, h, w = v.shape
    index = np.full((B, h, w), -1, np.int32)
    dist2 = np.full((B, h, w), NONE, np.int32)
    rr, cc = np.mgrid[0:h, 0:w]
    rr, cc = rr.reshape(-1).astype(np.int64), cc.reshape(-1).astype(np.int64)
    for b in range(B):
        cand = np.flatnonzero(v[b].reshape(-1) != 0)      # ascending flat positions
        if cand.size == 0:
            continue
        cr, ccol = cand // w, cand % w
        for p0 in range(0, h * w, 4096):      # blocks of pixels: the distance table stays small
            p = slice(p0, min(p0 + 4096, h * w))
            d = (rr[p, None] - cr[None]) ** 2 + (cc[p, None] - ccol[None]) ** 2
            k = np.argmin(d, axis=1)
            index[b].reshape(-1)[p] = cand[k]
            dist2[b].reshape(-1)[p] = d[np.arange(d.shape[0]), k]
    return (index[0], dist2[0]) if single else (index, dist2)


def _planes(x, valid):
    """(x as [B, C, h, w], valid as [B, h, w], restore): x [h, w] / [B, h, w] with valid of the same shape, or [B, C, h, w] with valid [B, h, w]."""
    x, valid = np.asarray(x), np.asarray(valid)
    if x.shape == valid.shape:
        if x.ndim == 2:
            return x[None, None], valid[None], lambda o: o[0, 0]
        return x[:, None], valid, lambda o: o[:, 0]
    assert x.ndim == 4 and valid.ndim == 3 and (x.shape[0],) + x.shape[2:] == valid.shape, (x.shape, valid.shape)
    return x, valid, lambda o: o


def fill_nearest_ref(x, valid, empty=0.0):
    """x with every invalid pixel replaced by the value at nearest_valid_ref's position (a copy: x's dtype and bits), ``empty`` where there is none."""
    xp, v, restore = _planes(x, valid)
    B, C, h, w = xp.shape
    index, _ = nearest_valid_ref(v)
    out = xp.copy()
    for b in range(B):
        hole = v[b].reshape(-1) == 0
        idx = index[b].reshape(-1)
        for c in range(C):
            src, dst = xp[b, c].reshape(-1), out[b, c].reshape(-1)
            dst[hole] = np.where(idx[hole] >= 0, src[np.maximum(idx[hole], 0)], np.asarray(empty).astype(xp.dtype))
    return restore(out)


def _pull(v, m):
    """One level up: v float32 [C, h, w], m bool [h, w] -> (v', m') at ceil(h / 2) x ceil(w / 2)."""
    C, h, w = v.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    vp = np.zeros((C, 2 * ho, 2 * wo), F)
    mp = np.zeros((2 * ho, 2 * wo), bool)      # children outside the level: m = 0
    vp[:, :h, :w] = np.where(m[None], v, F(0))
    mp[:h, :w] = m
    s00, s01, s10, s11 = vp[:, 0::2, 0::2], vp[:, 0::2, 1::2], vp[:, 1::2, 0::2], vp[:, 1::2, 1::2]      # zero where m = 0
    n = mp[0::2, 0::2].astype(np.int32) + mp[0::2, 1::2] + mp[1::2, 0::2] + mp[1::2, 1::2]
    total = ((s00 + s01) + s10) + s11
    assert total.dtype == F
    with np.errstate(divide="ignore", invalid="ignore"):
        q = total / np.maximum(n, 1).astype(F)[None]
    return np.where(n[None] > 0, q, F(0)).astype(F), n > 0


def _push(v, m, up):
    """One level down: the pixels of v (float32 [C, h, w]) with m = 0 take the bilinear value of ``up`` (the pushed level above)."""
    C, h, w = v.shape
    hu, wu = up.shape[1:]
    i, j = np.arange(h), np.arange(w)
    I, J = i >> 1, j >> 1
    I2 = np.clip(I + np.where(i & 1, 1, -1), 0, hu - 1)
    J2 = np.clip(J + np.where(j & 1, 1, -1), 0, wu - 1)
    a, b = up[:, I][:, :, J], up[:, I][:, :, J2]
    c, d = up[:, I2][:, :, J], up[:, I2][:, :, J2]
    with np.errstate(invalid="ignore", over="ignore"):
        r = (((F(9) * a + F(3) * b) + F(3) * c) + d) * F(0.0625)
    assert r.dtype == F
    return np.where(m[None], v, r)


def push_pull_ref(x, valid, empty=0.0):
    """The push-pull fill in np.float32, the contract's order of operations.  x float32 [h, w] / [B, h, w] / [B, C, h, w]; one mask per image."""
    xp, vm, restore = _planes(x, valid)
    assert xp.dtype == F, xp.dtype
    B, C, h, w = xp.shape
    out = np.empty_like(xp)
    for b in range(B):
        m0 = vm[b] != 0
        v0 = np.where(m0[None], xp[b], F(0))      # a select: the value under an invalid pixel never enters
        vs, ms = [v0], [m0]
        while vs[-1].shape[1:] != (1, 1):
            v, m = _pull(vs[-1], ms[-1])
            vs.append(v)
            ms.append(m)
        top = np.where(ms[-1][None], vs[-1], F(empty)).astype(F)
        for l in range(len(vs) - 2, -1, -1):
            top = _push(vs[l], ms[l], top)
        out[b] = np.where(m0[None], xp[b], top)      # valid pixels: x itself, bit for bit
    return restore(out)


def fill_smooth_u8_ref(x, valid, empty=0.0):
    """The uint8 wrapper: planes as float32, push_pull_ref, np.rint (half to even) back to uint8.  x uint8 [h, w] / [B, h, w] / [B, C, h, w] or an image
    [h, w, 3] / [B, h, w, 3] with valid [h, w] / [B, h, w]."""
    x, valid = np.asarray(x), np.asarray(valid)
    hwc = x.shape == valid.shape + (3,)
    if hwc:
        xs = x[None] if x.ndim == 3 else x
        vs = valid[None] if valid.ndim == 2 else valid
        o = np.rint(push_pull_ref(np.ascontiguousarray(xs.transpose(0, 3, 1, 2)).astype(F), vs, empty)).astype(np.uint8).transpose(0, 2, 3, 1)
        return o[0] if x.ndim == 3 else o
    return np.rint(push_pull_ref(x.astype(F), valid, empty)).astype(np.uint8)
