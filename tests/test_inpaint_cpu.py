"""CPU: the numpy restatement of the hole-filling contract (tests/_inpaint_ref.py) against scipy's exact distance transform and against the properties the
contract states, the argument checks of hip_ext.inpaint that need no device, and the new surface (exports, constants, the command line)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

import _inpaint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "amodal-depth-anything_amd")
F = np.float32


def random_mask(h, w, p, seed):
    v = (np.random.default_rng(seed).random((h, w)) < p).astype(np.uint8)
    v[(seed * 7) % h, (seed * 11) % w] = 1      # never empty: scipy's output for that input is an artefact
    return v


def quarter_map(shape, seed):
    """Quarter-integers in a range of nine (the values of test_gpu_filters.make_map): sums and means of a few of them are exact or tie."""
    return (np.random.default_rng(seed).integers(0, 9, shape) / 4.0 - 1.0).astype(F)


def check_index_properties(valid, index, dist2):
    """The three properties of a returned index: it is a valid pixel, it lies at the returned distance, and no valid pixel with a smaller flat
    position lies at that distance."""
    h, w = valid.shape
    flat = valid.reshape(-1) != 0
    idx = index.reshape(-1).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < h * w and flat[idx].all()
    rr, cc = np.divmod(np.arange(h * w, dtype=np.int64), w)
    ir, ic = np.divmod(idx, w)
    assert np.array_equal((rr - ir) ** 2 + (cc - ic) ** 2, dist2.reshape(-1).astype(np.int64))
    cr, ccol = np.divmod(np.flatnonzero(flat), w)
    for p0 in range(0, h * w, 2048):
        p = slice(p0, min(p0 + 2048, h * w))
        d = (rr[p, None] - cr[None]) ** 2 + (cc[p, None] - ccol[None]) ** 2
        first = np.flatnonzero(flat)[np.argmax(d == dist2.reshape(-1)[p, None].astype(np.int64), axis=1)]      # the smallest flat position at that distance
        assert (d >= dist2.reshape(-1)[p, None]).all()
        assert np.array_equal(first, idx[p])


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("hw", [(40, 57), (1, 33), (29, 1), (17, 16)], ids=str)
def test_restatement_distances_equal_scipy(hw, p):
    valid = random_mask(*hw, p, seed=hw[0] * 100 + hw[1] + int(p * 10))
    index, dist2 = R.nearest_valid_ref(valid)
    want = np.rint(ndimage.distance_transform_edt(valid == 0) ** 2).astype(np.int64)
    assert np.array_equal(dist2.astype(np.int64), want)
    check_index_properties(valid, index, dist2)


def test_restatement_tie_rule_and_empty_image():
    v = np.zeros((3, 3), np.uint8)      # two corners: their bisector is the diagonal
    v[0, 2] = v[2, 0] = 1
    index, dist2 = R.nearest_valid_ref(v)
    assert [index[k, k] for k in range(3)] == [2, 2, 2] and [dist2[k, k] for k in range(3)] == [4, 2, 4]      # ties along the diagonal go to the smaller flat position
    assert index[0, 2] == 2 and index[2, 0] == 6 and dist2[0, 2] == 0
    index, dist2 = R.nearest_valid_ref(np.zeros((2, 3, 4), np.uint8))
    assert (index == -1).all() and (dist2 == 0x7fffffff).all() and index.dtype == np.int32 and dist2.dtype == np.int32


def test_fill_nearest_ref_copies_bits():
    x = quarter_map((2, 3, 6, 7), 3)
    x[0, 0, 0, 0] = -0.0
    valid = np.stack([random_mask(6, 7, 0.3, 1), np.zeros((6, 7), np.uint8)])
    valid[0, 0, 0] = 1
    out = R.fill_nearest_ref(x, valid, empty=-7.5)
    index, _ = R.nearest_valid_ref(valid)
    assert np.array_equal(out[0].view(np.int32), x[0].reshape(3, -1)[:, index[0].reshape(-1)].reshape(3, 6, 7).view(np.int32))
    assert (out[1] == F(-7.5)).all()
    u8 = (np.arange(42).reshape(6, 7) * 5).astype(np.uint8)
    assert np.array_equal(R.fill_nearest_ref(u8, valid[0]), u8.reshape(-1)[index[0].reshape(-1)].reshape(6, 7))


SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 5), (33, 65), (9, 70)]


@pytest.mark.parametrize("hw", SHAPES, ids=str)
def test_push_pull_exact_cases(hw):
    h, w = hw
    x = quarter_map((1, 2, h, w), h * 31 + w)
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)      # noqa: E731
    # all valid: x bit for bit (a -0.0 included)
    x[0, 0, 0, 0] = -0.0
    assert np.array_equal(bits(R.push_pull_ref(x, np.ones((1, h, w), np.uint8))), bits(x))
    # none valid: empty everywhere
    assert np.array_equal(bits(R.push_pull_ref(x, np.zeros((1, h, w), np.uint8), empty=-3.25)), bits(np.full_like(x, -3.25)))
    # a constant field under any mask: the constant exactly
    mask = random_mask(h, w, 0.3, h + w)[None]
    assert np.array_equal(bits(R.push_pull_ref(np.full((1, 2, h, w), 2.0, F), mask)), bits(np.full((1, 2, h, w), 2.0, F)))
    # one valid pixel: its value everywhere
    one = np.zeros((1, h, w), np.uint8)
    one[0, h // 2, w - 1] = 1
    y = quarter_map((1, 2, h, w), 5)
    y[0, :, h // 2, w - 1] = (1.75, -0.5)
    out = R.push_pull_ref(y, one)
    assert (out[0, 0] == F(1.75)).all() and (out[0, 1] == F(-0.5)).all()
    # what lies under an invalid pixel changes nothing
    z = quarter_map((1, 2, h, w), 6)
    want = R.push_pull_ref(z, mask)
    dirty = z.copy()
    hole = np.flatnonzero(mask.reshape(-1) == 0)
    for c in range(2):
        for k, bad in zip(hole[:3], (np.nan, np.inf, -np.inf)):
            dirty[0, c].reshape(-1)[k] = bad
    with np.errstate(invalid="ignore"):
        got = R.push_pull_ref(dirty, mask)
    assert np.array_equal(bits(got), bits(want))
    # every output within [min, max] of the valid samples; for quarter-integers without any allowance beyond one ulp of the fp32 result
    for c in range(2):
        vals = z[0, c][mask[0] != 0].astype(np.float64)
        o = want[0, c].astype(np.float64)
        ulp = np.spacing(np.abs(want[0, c])).astype(np.float64)
        assert (o + ulp >= vals.min()).all() and (o - ulp <= vals.max()).all()


def test_push_pull_shapes_and_u8():
    h, w = 6, 9
    x, v = quarter_map((h, w), 1), random_mask(h, w, 0.5, 2)
    a = R.push_pull_ref(x, v)
    b = R.push_pull_ref(x[None], v[None])
    c = R.push_pull_ref(np.stack([x, x])[None], v[None])
    assert a.shape == (h, w) and np.array_equal(a, b[0]) and np.array_equal(a, c[0, 0]) and np.array_equal(a, c[0, 1])
    img = np.random.default_rng(0).integers(0, 256, (h, w, 3)).astype(np.uint8)
    out = R.fill_smooth_u8_ref(img, v)
    assert out.shape == img.shape and out.dtype == np.uint8 and np.array_equal(out[v != 0], img[v != 0])
    for k in range(3):
        assert np.array_equal(out[..., k], R.fill_smooth_u8_ref(img[..., k], v))


# ---- hip_ext.inpaint: what needs no device -----------------------------------------------------------------------------------------------------

def test_cpu_tensor_raises_hip_ext_error():
    import hip_ext
    from hip_ext import inpaint
    v, x = torch.ones(4, 5, dtype=torch.uint8), torch.zeros(4, 5)
    with pytest.raises(hip_ext.HipExtError, match="HIP device"):
        inpaint.nearest_valid(v)
    for fn in (inpaint.fill_nearest, inpaint.fill_smooth):
        with pytest.raises(hip_ext.HipExtError, match="HIP device"):
            fn(x, v)
        with pytest.raises(hip_ext.HipExtError, match="HIP device"):
            fn(x.numpy(), v.numpy(), device="cpu")


def test_bad_shapes_and_dtypes_raise_value_error():
    from hip_ext import inpaint
    v = np.ones((4, 5), np.uint8)
    with pytest.raises(ValueError, match="nearest_valid"):
        inpaint.nearest_valid(np.ones((4, 5), np.float32))
    with pytest.raises(ValueError, match="nearest_valid"):
        inpaint.nearest_valid(np.ones((2, 3, 4, 5), np.uint8))
    with pytest.raises(ValueError, match="nearest_valid"):
        inpaint.nearest_valid(np.ones((0, 5), np.uint8))
    with pytest.raises(ValueError, match="nearest_valid"):
        inpaint.nearest_valid(np.ones((1, 32768), np.uint8))
    for name in ("fill_nearest", "fill_smooth"):
        fn = getattr(inpaint, name)
        for x, valid in ((np.zeros((4, 6), F), v), (np.zeros((4, 5), np.float64), v), (np.zeros((4, 5, 3), F), v), (np.zeros((3, 4, 5), F), v),
                         (np.zeros((2, 3, 4, 5), F), np.ones((1, 4, 5), np.uint8)), (np.zeros((4, 5), F), np.ones((4, 5), np.int32)),
                         (np.zeros((4, 5, 4), np.uint8), v), ([[0.0]], v)):
            with pytest.raises(ValueError, match=name):
                fn(x, valid)
        with pytest.raises(ValueError, match=name):
            fn(torch.zeros(4, 5, dtype=torch.float16), torch.ones(4, 5, dtype=torch.uint8))


def test_geometry_argument_checks():
    from hip_ext import geometry
    with pytest.raises(TypeError, match="fill_view"):
        geometry.fill_view(np.zeros((3, 3), F))
    view = geometry.View(torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32), None)
    with pytest.raises(ValueError, match="fill_view"):
        geometry.fill_view(view, method="poisson")
    d, m = np.ones((4, 5), F), np.ones((2, 4, 5), np.uint8)
    for kwargs in ({"method": "poisson"}, {"grow": -1}, {"grow": 1.5}, {"image": np.zeros((4, 5), np.uint8)}, {"image": np.zeros((4, 5, 3), F)}):
        with pytest.raises(ValueError, match="remove_objects"):
            geometry.remove_objects(d, m, **kwargs)
    with pytest.raises(ValueError, match="remove_objects"):
        geometry.remove_objects(d, np.ones((4, 6), np.uint8))
    with pytest.raises(ValueError, match="remove_objects"):
        geometry.remove_objects(d[None], m)
    assert "not a learned completion" in geometry.remove_objects.__doc__


def test_surface_exports_constants_and_build_lists():
    import hip_ext
    header = open(os.path.join(ROOT, "include", "ada_hip.h")).read()
    for name in ("ada_nearest_valid_workspace_bytes", "ada_nearest_valid_fwd", "ada_fill_gather_fwd", "ada_push_pull_workspace_bytes", "ada_push_pull_fwd"):
        assert name in hip_ext.EXPORTS and re.search(rf"\bint {name}\(", header), name
    assert hip_ext.INPAINT_CHUNK == 1024 and re.search(r"#define\s+ADA_INPAINT_CHUNK\s+1024\b", header)
    for name in ("nearest_valid_fwd", "fill_gather", "push_pull", "nearest_valid_workspace_bytes", "push_pull_workspace_bytes"):
        assert callable(getattr(hip_ext, name)), name
    sys.path.insert(0, os.path.join(PKG, "csrc"))
    try:
        import build as B
    finally:
        sys.path.pop(0)
    assert "ada_inpaint.hip" in B.SOURCES and "ada_inpaint.hip" in B.NO_SCRATCH and B.PER_FILE_FLAGS["ada_inpaint.hip"] == ["-ffp-contract=off"]


def test_workspace_queries_without_a_device():
    import hip_ext
    assert hip_ext.nearest_valid_workspace_bytes(2, 33, 65) == 4 * 2 * 33 * 65
    levels = [(17, 33), (9, 17), (5, 9), (3, 5), (2, 3), (1, 2), (1, 1)]
    assert hip_ext.push_pull_workspace_bytes(2, 3, 33, 65) == 2 * (4 * 3 + 1) * sum(a * b for a, b in levels)
    assert hip_ext.push_pull_workspace_bytes(1, 1, 1, 1) == 0
    with pytest.raises(hip_ext.HipExtError, match="32767"):
        hip_ext.push_pull_workspace_bytes(1, 1, 32768, 4)
    with pytest.raises(hip_ext.HipExtError, match="bad shape"):
        hip_ext.nearest_valid_workspace_bytes(1, 0, 4)


def test_depth_to_view_help_lists_fill_holes():
    out = subprocess.run([sys.executable, "-m", "src.scripts.depth_to_view", "--help"], cwd=PKG, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--fill_holes" in out.stdout and "nearest" in out.stdout and "smooth" in out.stdout
