"""Anchors tests/_resize_ref.py -- the restatement the GPU geometry sweeps compare the resize kernels with -- to ATen on the CPU, on every pair of the
three geometry sets, and checks the host's patch-extent rules against the restated taps for every tile of every pair.  No GPU, no HIP library.

Bounds (derived, none measured), for integer inputs in [-8, 8] on a map [1, n, m, 2]:

fp32.  ATen evaluates  wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d)  in fp32, or in its channels-last form four weight products times four values: along
       any one path from an input to the output at most n = 5 roundings (weight product, product with the value, three additions); the weights
       themselves are the restated ones, bit for bit.  Allowed: (n + 1) 2^-24 mag, mag the same expression on |x|.
fp64.  The restated coordinate f = fl(fl((a-1)/(b-1)) i) carries two relative roundings of 2^-24: |delta| <= 2 2^-24 (n_in - 1).  The interpolant is
       continuous and piecewise linear in the coordinate with slope at most D, the largest difference of adjacent pixels along that axis, so it moves
       by at most delta D per axis; w0 = 1 - w1 is one more rounding of at most 2^-25, times |x| <= 8, per axis.
       Allowed: 2 2^-24 ((hi - 1) Dy + (wi - 1) Dx) + 2 2^-25 max|x|, plus fp64's own 2^-50 mag."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _resize_ref as R

U24 = 2.0 ** -24
FIXED = (2, 3)               # the other axis: the smallest pair that still interpolates
ATEN_ROUNDINGS = 5


def _ints(shape, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float64)


def _shape(pair, axis):
    (hi, ho), (wi, wo) = (pair, FIXED) if axis == "y" else (FIXED, pair)
    return hi, wi, ho, wo


def _aten(x_nhwc, ho, wo, dtype):
    t = torch.from_numpy(x_nhwc).permute(0, 3, 1, 2).contiguous().to(dtype)
    return F.interpolate(t, size=(ho, wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).double().numpy()


def _where(bad):
    return tuple(int(v) for v in np.argwhere(bad)[0])


@pytest.mark.parametrize("axis", ["y", "x"])
@pytest.mark.parametrize("pairs", sorted(R.PAIR_SETS))
def test_bilinear_restatement_agrees_with_aten_fp32(pairs, axis):
    for k, pair in enumerate(R.PAIR_SETS[pairs]):
        hi, wi, ho, wo = _shape(pair, axis)
        x = _ints((1, hi, wi, 2), 100 + k)
        ref, mag = R.bilinear(x, ho, wo), R.bilinear_mag(x, ho, wo)
        err = np.abs(_aten(x, ho, wo, torch.float32) - ref)
        bad = err > (ATEN_ROUNDINGS + 1) * U24 * mag
        assert not bad.any(), f"{pair} along {axis}: ATen fp32 and the restatement differ at {_where(bad)} by {err.max():.3e} (taps {R.taps(*pair)})"


@pytest.mark.parametrize("axis", ["y", "x"])
@pytest.mark.parametrize("pairs", sorted(R.PAIR_SETS))
def test_bilinear_restatement_agrees_with_aten_fp64(pairs, axis):
    for k, pair in enumerate(R.PAIR_SETS[pairs]):
        hi, wi, ho, wo = _shape(pair, axis)
        x = _ints((1, hi, wi, 2), 100 + k)
        dy = float(np.abs(np.diff(x, axis=1)).max()) if hi > 1 else 0.0
        dx = float(np.abs(np.diff(x, axis=2)).max()) if wi > 1 else 0.0
        lim = 2 * U24 * ((hi - 1) * dy + (wi - 1) * dx) + 2 * 2.0 ** -25 * 8.0 + 2.0 ** -50 * 8.0
        err = np.abs(_aten(x, ho, wo, torch.float64) - R.bilinear(x, ho, wo))
        assert float(err.max()) <= lim, f"{pair} along {axis}: fp64 ATen and the restatement differ by {err.max():.3e} > {lim:.3e} at {_where(err > lim)}"


@functools.lru_cache(maxsize=None)
def _pos(sq, dim=4):
    g = torch.Generator().manual_seed(601)
    return torch.randn(1 + sq * sq, dim, generator=g)


@pytest.mark.parametrize("grids", sorted(R.POS_GRIDS))
@pytest.mark.parametrize("sq", R.POS_SQ)
def test_bicubic_restatement_agrees_with_aten(sq, grids):
    pos = _pos(sq)
    grid = pos[1:].reshape(1, sq, sq, -1).permute(0, 3, 1, 2)
    for ph, pw in R.POS_GRIDS[grids]:
        sh, sw = (ph + 0.1) / sq, (pw + 0.1) / sq
        ref = F.interpolate(grid, scale_factor=(sh, sw), mode="bicubic", antialias=False)
        assert ref.shape[-2:] == (ph, pw)
        ref = torch.cat([pos[:1], ref.permute(0, 2, 3, 1).reshape(ph * pw, -1)], 0).double().numpy()
        got = R.bicubic_pos(pos.numpy(), sq, ph, pw, sh, sw)
        assert np.array_equal(got[0], pos[0].double().numpy())
        err = np.abs(got - ref)
        bad = err > 3e-6 + 1e-5 * np.abs(ref)
        assert not bad.any(), f"sq {sq} grid {ph} x {pw}: {int(bad.sum())} elements off, max {err.max():.3e}, first at {_where(bad)}"


# ---------------------------------------------------------------------------------------------------------------------------------
# host extent against the restated taps
# ---------------------------------------------------------------------------------------------------------------------------------
def extent_misses(n_in, n_out, tile, kind, slack=0):
    """Tiles (t0, output index, tap) of one pair whose restated taps fall outside [origin, origin + extent + slack) of the staged patch."""
    i0, i1, _, _ = R.taps(n_in, n_out)
    s = R.scale(n_in, n_out)
    if kind == "bilinear":
        ext = R.bilinear_extent(n_in, n_out, tile) + slack
        span = lambda t0: (R.bilinear_origin(s, t0), range(t0, min(t0 + tile, n_out)))                      # noqa: E731
    else:
        ext = R.tapsum_extent(n_in, n_out, tile) + slack
        span = lambda t0: (R.tapsum_origin(s, t0), range(max(t0 - 1, 0), min(t0 + tile + 1, n_out)))      # noqa: E731  (the halo; rows outside the image read the origin)
    out = []
    for t0 in range(0, n_out, tile):
        origin, idx = span(t0)
        assert 0 <= origin <= n_in - 1
        for i in idx:
            for tap in (int(i0[i]), int(i1[i])):
                if not origin <= tap < origin + ext:
                    out.append((t0, i, tap))
    return out


EXTENT_RULES = [("bilinear", R.BT_TH), ("bilinear", R.BT_TW), ("tapsum", R.TS_TH), ("tapsum", R.TS_TW)]


@pytest.mark.parametrize("kind,tile", EXTENT_RULES)
@pytest.mark.parametrize("pairs", sorted(R.PAIR_SETS))
def test_host_extent_covers_every_tap_of_every_tile(pairs, kind, tile):
    """The device reads a tap at (tap - origin) inside the staged patch: a tap outside [origin, origin + extent) would be another pixel's bytes."""
    for pair in R.PAIR_SETS[pairs]:
        miss = extent_misses(*pair, tile, kind)
        assert not miss, f"{kind} extent, tile {tile}, pair {pair}: (tile origin, output, tap) outside the staged patch: {miss[:4]}"


def test_extent_check_sees_an_extent_one_too_small():
    """Sensitivity, without running a wrong kernel: with the restated extent perturbed by -1 the check above reports pairs in every set it walks."""
    for kind, tile in EXTENT_RULES:
        for name in ("model", "up"):
            hit = sum(1 for pair in R.PAIR_SETS[name] if extent_misses(*pair, tile, kind, slack=-1))
            print(f"{kind} extent - 1, tile {tile}, {name}: {hit} of {len(R.PAIR_SETS[name])} pairs reported")
            assert hit > len(R.PAIR_SETS[name]) // 2
    # and the fp32 evaluation is part of the rule: a host that computed the taps in double would place some of them one pixel away from the device's
    for name in ("model", "up"):
        moved = [(a, b) for a, b in R.PAIR_SETS[name] if b > 1 and (np.floor((a - 1) / (b - 1) * np.arange(b)).astype(np.int64) != R.taps(a, b)[0]).any()]
        print(f"lower tap in double != lower tap in fp32, {name}: {len(moved)} of {len(R.PAIR_SETS[name])} pairs, e.g. {moved[:3]}")
        assert moved


@pytest.mark.parametrize("pairs", ["model", "up"])
def test_tail_row_window_holds_the_halo_rows_of_every_accepted_pair(pairs):
    """ada_dpt_tail_fwd: a producer thread keeps 5 source rows, starting at the lower tap of its first halo row, for its 5 halo rows (two groups per 10-row
    halo of an 8-row tile): every tap of an accepted pair must lie in that window, and every ho >= 1.5 hi must be accepted."""
    for hi, ho in R.PAIR_SETS[pairs] + (R.TAIL_MODEL_PAIRS if pairs == "model" else ()):
        ok = R.tail_accepts(hi, ho)
        assert ok or 2 * ho < 3 * hi, f"{hi} -> {ho} is an up-sampling by >= 1.5 that the rule refuses"
        if not ok:
            continue
        i0, i1, _, _ = R.taps(hi, ho)
        for t0 in range(0, ho, 8):
            for half in (0, 1):
                first = t0 - 1 + 5 * half
                origin = int(i0[min(max(first, 0), ho - 1)])
                for y in range(max(first, 0), min(first + 5, ho)):
                    assert origin <= i0[y] <= origin + 3 and i1[y] <= origin + 4, f"{hi} -> {ho}: halo row {y} of tile {t0} taps {i0[y]}, {i1[y]} outside rows {origin} .. {origin + 4}"


def test_geometry_sets():
    assert len(R.UP_PAIRS) == 1260 and (1, 1) in R.UP_PAIRS and (1, 64) in R.UP_PAIRS and (24, 24) in R.UP_PAIRS
    assert len(R.DOWN_PAIRS) == 276 and (2, 1) in R.DOWN_PAIRS and all(b < a for a, b in R.DOWN_PAIRS)
    for p in (1, 37, 74):
        for pair in (((p - 1) // 2 + 1, p), (p, 2 * p), (2 * p, 4 * p), (4 * p, 8 * p), (8 * p, 14 * p)):
            assert pair in R.MODEL_PAIRS
    assert len(set(R.MODEL_PAIRS)) == len(R.MODEL_PAIRS) and max(b for _, b in R.MODEL_PAIRS) == 1036
    # most of the model's scales round in fp32: the bit-for-bit tests, which need (b - 1) = 2^k (a - 1), cannot reach them
    assert sum(1 for a, b in R.MODEL_PAIRS if a > 1 and (b - 1) % (a - 1) != 0) > len(R.MODEL_PAIRS) // 2
