"""Restatement of the sampling rules of the resize kernels, and the geometry sets their sweeps walk ("Geometry sweeps").

numpy only: no GPU, no library call.  The rules are ATen's -- upsample_bilinear2d(align_corners=True) and upsample_bicubic2d(align_corners=False) -- and the
contract the kernels' comments state: coordinates and weights are fp32, evaluated by the expressions below and by no others, because the kernels stage
source patches whose size the host derives from the very same fp32 expressions.  tests/test_resize_ref_cpu.py anchors this file to ATen on the CPU;
tests/test_gpu_resize_geometry.py compares the kernels with it.  The blends are done in float64, so what a comparison sees of this file's own
rounding is the weights' -- which are the kernels' weights."""
import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# align-corners bilinear
# ---------------------------------------------------------------------------------------------------------------------------------
def scale(n_in, n_out):
    """(n_in - 1) / (n_out - 1) as one fp32 division, 0 for a single output."""
    return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0.0)


def taps(n_in, n_out):
    """(i0, i1, w0, w1) per output index: f = s * i in fp32, i0 = int(f), i1 = i0 + (i0 < n_in - 1), w1 = f - i0, w0 = 1 - w1 (fp32)."""
    f = scale(n_in, n_out) * np.arange(n_out, dtype=F32)
    assert f.dtype == F32
    i0 = f.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    w1 = f - i0.astype(F32)
    w0 = F32(1.0) - w1
    assert w0.dtype == F32 and w1.dtype == F32 and int(i1.max()) <= n_in - 1 and int(i0.min()) >= 0
    return i0, i1, w0, w1


def _blend(x, ty, tx):
    y0, y1, wy0, wy1 = ty
    x0, x1, wx0, wx1 = tx
    wy0, wy1 = wy0.astype(np.float64)[None, :, None, None], wy1.astype(np.float64)[None, :, None, None]
    wx0, wx1 = wx0.astype(np.float64)[None, None, :, None], wx1.astype(np.float64)[None, None, :, None]
    top, bot = x[:, y0], x[:, y1]
    return wy0 * (wx0 * top[:, :, x0] + wx1 * top[:, :, x1]) + wy1 * (wx0 * bot[:, :, x0] + wx1 * bot[:, :, x1])


def bilinear(x_nhwc, ho, wo):
    """[B, hi, wi, C] -> float64 [B, ho, wo, C]:  wy0 (wx0 v00 + wx1 v01) + wy1 (wx0 v10 + wx1 v11)  with the fp32 weights of taps(), blended in float64."""
    x = np.asarray(x_nhwc, dtype=np.float64)
    return _blend(x, taps(x.shape[1], ho), taps(x.shape[2], wo))


def bilinear_mag(x_nhwc, ho, wo):
    """The same expression on |x| (the weights are non-negative): the magnitude a rounding bound scales with."""
    return bilinear(np.abs(np.asarray(x_nhwc, dtype=np.float64)), ho, wo)


# ---------------------------------------------------------------------------------------------------------------------------------
# bicubic resample of the position table (align_corners=False, A = -0.75)
# ---------------------------------------------------------------------------------------------------------------------------------
def _cubic_axis(n_in, n_out, scale_factor):
    """Clamped tap indices [n_out, 4] and fp32 coefficients [n_out, 4]: source coordinate (dst + 0.5) * (1 / scale_factor) - 0.5, not clamped.

    The coordinate is ONE fused multiply-add, rounded to fp32 once: that is what ATen's CPU build evaluates (its compiler contracts the expression;
    with the product rounded separately this file misses ATen's fp32 result on 36 of the 444 grids of tests/test_resize_ref_cpu.py, by up to 2.8
    times the tolerance, fused on none) and what the device compiler makes of the kernel's expression.  A coordinate near 37 has an fp32 spacing of
    4e-6, and the cubic's slope on a Gaussian table is of order one: the choice is visible at the project's 3e-6 tolerance."""
    inv = F32(1.0 / float(scale_factor))                  # the reciprocal in double, narrowed once
    dst = np.arange(n_out, dtype=F32) + F32(0.5)          # exact
    f = (dst.astype(np.float64) * np.float64(inv) - 0.5).astype(F32)      # the product of two fp32 and the subtraction are exact in float64
    fl = np.floor(f)
    t = f - fl
    assert f.dtype == F32 and t.dtype == F32
    A = F32(-0.75)
    one = F32(1.0)

    def near(x):          # |x| <= 1
        return ((A + F32(2.0)) * x - (A + F32(3.0))) * x * x + one

    def far(x):           # 1 < |x| < 2
        return ((A * x - F32(5.0) * A) * x + F32(8.0) * A) * x - F32(4.0) * A
    coef = np.stack([far(t + one), near(t), near(one - t), far((one - t) + one)], axis=1)
    assert coef.dtype == F32
    idx = np.clip(fl.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], 0, n_in - 1)
    return idx, coef


def bicubic_pos(pos, sq, ph, pw, scale_h, scale_w):
    """pos [1 + sq sq, dim] -> float64 [1 + ph pw, dim]: row 0 copied, the sq x sq grid resampled to ph x pw.  Coordinates and coefficients fp32, sums float64."""
    pos = np.asarray(pos)
    dim = pos.shape[1]
    grid = pos[1:].astype(np.float64).reshape(sq, sq, dim)
    iy, cy = _cubic_axis(sq, ph, scale_h)
    ix, cx = _cubic_axis(sq, pw, scale_w)
    rows = np.einsum("xl,yxld->yxd", cx.astype(np.float64), grid[:, ix])               # [sq, pw, dim]: along x first, as the kernel and ATen do
    out = np.einsum("yk,ykxd->yxd", cy.astype(np.float64), rows[iy])
    return np.concatenate([pos[:1].astype(np.float64), out.reshape(ph * pw, dim)], axis=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# host rules restated: the source patch a tile may touch
# ---------------------------------------------------------------------------------------------------------------------------------
BT_TH, BT_TW = 8, 16          # output tile of the LDS-tiled bilinear kernel (rows, columns)
TS_TH, TS_TW = 8, 16          # output tile of the tap-sum kernel; its patch also covers a one-pixel halo


def _itrunc(s, i):
    return int(F32(s) * F32(i))


def bilinear_origin(s, t0):
    return _itrunc(s, t0)


def bilinear_extent(n_in, n_out, tile):
    """ada_bilinear_fwd's extent(): over the tiles, (upper tap of the tile's last output, clamped) - (lower tap of its first output) + 1."""
    s, best = scale(n_in, n_out), 1
    for t0 in range(0, n_out, tile):
        last = min(t0 + tile - 1, n_out - 1)
        best = max(best, min(_itrunc(s, last) + 1, n_in - 1) - _itrunc(s, t0) + 1)
    return best


def tapsum_origin(s, t0):
    return _itrunc(s, max(t0 - 1, 0))


def tapsum_extent(n_in, n_out, tile):
    """ada_tapsum_resize_fwd's extent(): the same with the halo, outputs max(t0 - 1, 0) .. min(t0 + tile, n_out - 1)."""
    s, best = scale(n_in, n_out), 1
    for t0 in range(0, n_out, tile):
        last = min(t0 + tile, n_out - 1)
        best = max(best, min(_itrunc(s, last) + 1, n_in - 1) - tapsum_origin(s, t0) + 1)
    return best


def bilinear_is_tiled(channels, batch, hi, wi, ho, wo):
    """The dispatch predicate of ada_bilinear_fwd: channel chunks of 128, no down-sampling, at least one full tile each way, patch of at most 128 pixels (64 KiB)."""
    patch = bilinear_extent(hi, ho, BT_TH) * bilinear_extent(wi, wo, BT_TW)
    return (channels % 128 == 0 and scale(hi, ho) <= F32(1.0) and scale(wi, wo) <= F32(1.0) and ho >= BT_TH and wo >= BT_TW and patch * 512 <= 65536
            and batch * (channels // 128) <= 65535)


def tail_accepts(hi, ho):
    """ada_dpt_tail_fwd's vertical rule (10 halo rows within 8 source rows, 5 within 5): every ho >= 1.5 hi passes it."""
    s = scale(hi, ho)
    return _itrunc(s, 9) + 2 <= 7 and _itrunc(s, 4) + 2 <= 4


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry sets
# ---------------------------------------------------------------------------------------------------------------------------------
MODEL_P = range(1, 75)          # patch grids up to a 1036-pixel side


def _model_pairs():
    seen = []
    for p in MODEL_P:
        for pair in (((p - 1) // 2 + 1, p), (p, 2 * p), (2 * p, 4 * p), (4 * p, 8 * p), (8 * p, 14 * p)):
            if pair not in seen:
                seen.append(pair)
    return tuple(seen)


MODEL_PAIRS = _model_pairs()                                                                    # every per-axis resize the head does for a grid of p patches
TAIL_MODEL_PAIRS = tuple((8 * p, 14 * p) for p in MODEL_P)
UP_PAIRS = tuple((a, b) for a in range(1, 25) for b in range(a, 65))                            # n_in == 1, scale exactly 1 and (1, 1) included
DOWN_PAIRS = tuple((a, b) for a in range(2, 25) for b in range(1, a))                           # the per-pixel kernel alone accepts these
PAIR_SETS = {"model": MODEL_PAIRS, "up": UP_PAIRS, "down": DOWN_PAIRS}
POS_GRIDS = {"p_by_3": tuple((p, 3) for p in MODEL_P), "3_by_p": tuple((3, p) for p in MODEL_P), "p_by_p": tuple((p, p) for p in MODEL_P)}
POS_SQ = (16, 37)
