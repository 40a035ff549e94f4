"""CPU: the numpy restatement of the rank-filter contract (tests/_filters_ref.py) against scipy on the identities the contract names, the rank rule on
hand-made windows, and the argument validation of hip_ext.filters / hip_ext.masks that needs no device."""
import numpy as np
import pytest
import scipy.ndimage as ndi

import _filters_ref as F

SHAPES = [(1, 1), (2, 7), (5, 3), (9, 11)]
SIZES = [3, 5, 7]


def _map(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 9, shape) / 4.0 - 1.0).astype(np.float32)      # quarter-integers: ties dominate


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("size", SIZES)
def test_median_is_scipys_under_mirror_and_nearest(shape, size):
    x = _map(shape, 1)
    for border in ("mirror", "nearest"):
        out, n = F.rank_filter(x, size, "median", border)
        assert np.array_equal(out, ndi.median_filter(x, size=size, mode=border)), border
        assert (n == size * size).all()
    xu = (x * 4 + 4).astype(np.uint8) * 28
    assert np.array_equal(F.rank_filter(xu, size, "median", "mirror")[0], ndi.median_filter(xu, size=size, mode="mirror"))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("size", SIZES)
def test_extremes_under_ignore_are_scipys_with_an_infinite_constant(shape, size):
    x = _map(shape, 2)
    assert np.array_equal(F.rank_filter(x, size, "min", "ignore")[0], ndi.minimum_filter(x, size=size, mode="constant", cval=np.inf))
    assert np.array_equal(F.rank_filter(x, size, "max", "ignore")[0], ndi.maximum_filter(x, size=size, mode="constant", cval=-np.inf))
    lo, hi, n = F.extremes(x[None], size, "ignore")      # the running form used for windows too large to stack
    assert np.array_equal(lo[0], F.rank_filter(x, size, "min", "ignore")[0]) and np.array_equal(hi[0], F.rank_filter(x, size, "max", "ignore")[0])
    assert np.array_equal(n[0], F.rank_filter(x, size, "min", "ignore")[1])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("size", SIZES)
def test_binary_morphology_is_scipys_explicit_composition(shape, size):
    rng = np.random.default_rng(3)
    ones = np.ones((size, size), bool)
    for density in (0.1, 0.5, 0.9):
        m = (rng.random(shape) < density).astype(np.uint8)
        for it in (1, 2):
            er = ndi.binary_erosion(m, structure=ones, border_value=1, iterations=it)
            di = ndi.binary_dilation(m, structure=ones, border_value=0, iterations=it)
            assert np.array_equal(F.erode(m, size, it), er) and np.array_equal(F.dilate(m, size, it), di)
            assert np.array_equal(F.opening(m, size, it), ndi.binary_dilation(er, structure=ones, border_value=0, iterations=it))
            assert np.array_equal(F.closing(m, size, it), ndi.binary_erosion(di, structure=ones, border_value=1, iterations=it))


def test_scipys_own_closing_is_not_the_composition_under_ignore():
    m = np.ones((5, 5), np.uint8)
    assert F.closing(m, 3).all() and not ndi.binary_closing(m, structure=np.ones((3, 3), bool)).all()      # scipy erodes against an outside of 0


def test_rank_rule_on_hand_made_windows():
    x = np.array([[5.0, 1.0, 4.0, 2.0]], np.float32)
    size = (1, 7)      # under 'ignore' every pixel's window holds the whole row
    for votes, med, p50 in (([1, 0, 0, 0], 5, 5), ([1, 1, 0, 0], 5, 1), ([1, 1, 1, 0], 4, 4), ([1, 1, 1, 1], 4, 2)):
        v = np.array([votes], np.uint8)
        s = np.sort(x[0, np.array(votes, bool)])
        n = len(s)
        out, cnt = F.rank_filter(x, size, "median", "ignore", valid=v)
        assert (cnt == n).all() and (out == med).all() and med == s[n // 2]
        assert (F.rank_filter(x, size, 0, "ignore", valid=v)[0] == s[0]).all() and (F.rank_filter(x, size, "min", "ignore", valid=v)[0] == s[0]).all()
        assert (F.rank_filter(x, size, 100, "ignore", valid=v)[0] == s[-1]).all() and (F.rank_filter(x, size, "max", "ignore", valid=v)[0] == s[-1]).all()
        assert (F.rank_filter(x, size, 50, "ignore", valid=v)[0] == p50).all() and p50 == s[(50 * (n - 1)) // 100]
    assert list(F.rank_index(np.arange(1, 6), 25)) == [0, 0, 0, 0, 1] and list(F.rank_index(np.arange(1, 6), "median")) == [0, 1, 1, 2, 2]


def test_fill_count_nan_and_mirror_of_a_window_wider_than_the_image():
    x = np.array([[1.0, np.nan, 3.0]], np.float32)
    out, n = F.rank_filter(x, 1, "median", "mirror")
    assert list(n[0]) == [1, 0, 1] and out[0, 0] == 1 and np.isnan(out[0, 1]) and out[0, 2] == 3
    assert F.rank_filter(x, 1, "median", "mirror", fill=-7.0)[0][0, 1] == -7
    assert (F.rank_filter(np.array([[1, 2, 3]], np.uint8), 3, "max", "ignore", valid=np.zeros((1, 3), np.uint8))[0] == 0).all()
    assert list(F.map_index(np.arange(-9, 10), 3, "mirror")) == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert list(F.map_index(np.arange(-3, 4), 1, "mirror")) == [0] * 7 and list(F.map_index(np.arange(-2, 5), 3, "nearest")) == [0, 0, 0, 1, 2, 2, 2]
    assert list(F.map_index(np.arange(-1, 4), 3, "ignore")) == [-1, 0, 1, 2, -1]
    inf = np.array([[np.inf, -np.inf, 0.0, -0.0, 1e-42]], np.float32)
    assert np.array_equal(F.rank_filter(inf, (1, 9), "min", "ignore")[0], np.full((1, 5), -np.inf, np.float32))
    assert np.array_equal(F.rank_filter(inf, (1, 9), "median", "ignore")[0], np.zeros((1, 5), np.float32))      # -inf, the two zeros, the denormal, +inf: s[2] is a zero
    assert np.array_equal(F.rank_filter(inf, (1, 9), 75, "ignore")[0], np.full((1, 5), 1e-42, np.float32))      # s[75 * 4 // 100] = s[3]


def test_python_layer_rejects_bad_arguments_before_any_device_is_needed():
    from hip_ext import FILTER_MAX_EXTREME, FILTER_MAX_WINDOW, filters, masks
    assert (FILTER_MAX_WINDOW, FILTER_MAX_EXTREME) == (81, 63)
    x = np.zeros((12, 12), np.float32)
    for size in (4, (3, 2), 0, -3, (3,), "3", 3.0):
        with pytest.raises(ValueError, match="size"):
            filters.rank_filter(x, size)
    for size in ((9, 11), (3, 29), 11, (83, 1)):
        with pytest.raises(ValueError, match="at most 81"):
            filters.median_filter(x, size)
        with pytest.raises(ValueError, match="at most 81"):
            filters.rank_filter(x, size, 50)
    for size in (65, (1, 65), (65, 3)):
        with pytest.raises(ValueError, match="at most 63"):
            filters.minimum_filter(x, size)
        with pytest.raises(ValueError, match="at most 63"):
            filters.maximum_filter(x, size)
    for rank in (-1, 101, "mean", 50.0, None):
        with pytest.raises(ValueError, match="rank"):
            filters.rank_filter(x, 3, rank)
    with pytest.raises(ValueError, match="valid of shape"):
        filters.median_filter(x, 3, valid=np.ones((12, 11), np.uint8))
    with pytest.raises(ValueError, match="valid of shape"):
        filters.median_filter(x, 3, valid=np.ones((1, 12, 12), np.uint8))
    for border in ("reflect", "constant", None, 0):
        with pytest.raises(ValueError, match="border"):
            filters.median_filter(x, 3, border=border)
    with pytest.raises(ValueError, match="fill"):
        filters.median_filter(x.astype(np.uint8), 3, fill=256)
    m = np.zeros((5, 5), np.uint8)
    for fn in (masks.erode, masks.dilate, masks.opening, masks.closing):
        for size in (2, 65, 0):
            with pytest.raises(ValueError, match="size"):
                fn(m, size=size)
        with pytest.raises(ValueError, match="iterations"):
            fn(m, iterations=-1)
    with pytest.raises(ValueError, match="differ in shape"):
        masks.invisible_mask(m, np.zeros((5, 6), np.uint8))


def test_exports_constants_and_header_section():
    import os
    import hip_ext
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ada_hip.h")).read()
    for name in ("ada_rank_filter_fwd", "ada_extreme_filter_fwd"):
        assert name in hip_ext.EXPORTS and f"int {name}(" in header and hasattr(hip_ext.load(), name)
    assert (hip_ext.BORDER_MIRROR, hip_ext.BORDER_NEAREST, hip_ext.BORDER_IGNORE) == (0, 1, 2)
    assert hip_ext.FILTER_TILE_W * hip_ext.FILTER_TILE_H == 256 and hip_ext.FILTER_COL_TILE_H % hip_ext.FILTER_TILE_H == 0
    assert hip_ext.extreme_filter_workspace_bytes(3, 5, 7) == 5 * 3 * 5 * 7
