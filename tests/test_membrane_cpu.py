"""CPU: the numpy / scipy restatement of the membrane-solve contract (tests/_membrane_ref.py) against facts about discrete harmonic functions, the
argument checks of the new wrappers that run before any device is looked at, and the new surface (exports, constants, the command line)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _membrane_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "amodal-depth-anything_amd")


def quarter_map(shape, seed):
    return np.random.default_rng(seed).integers(0, 9, shape) / 4.0 - 1.0


def l_domain(n):
    d = np.zeros((n, n), np.uint8)
    d[:, : n // 3] = 1
    d[-(n // 3):, :] = 1
    return d


@pytest.mark.parametrize("seed", range(4))
def test_a_constant_field_gives_the_constant(seed):
    rng = np.random.default_rng(seed)
    h, w = 17, 23
    known = rng.random((h, w)) < 0.1
    domain = rng.random((h, w)) < 0.8
    got = R.fill(np.full((h, w), 2.75), known, domain, empty=-9.0)
    k, d = R.masks(known, domain, (h, w))
    reached = d & ~R.unreached(k, d)
    assert np.abs(got[reached] - 2.75).max() < 1e-13
    assert (got[R.unreached(k, d) & ~k] == -9.0).all() and (got[~d] == 2.75).all()


def test_an_affine_field_is_discretely_harmonic():
    h, w = 20, 31
    yy, xx = np.mgrid[0:h, 0:w]
    x = 0.5 * yy - 0.25 * xx + 3.0
    border = (yy == 0) | (yy == h - 1) | (xx == 0) | (xx == w - 1)
    hidden = np.where(border, x, np.nan)      # what lies under an unknown pixel is never read
    got = R.fill(hidden, border)
    assert np.abs(got - x).max() < 1e-12
    A, b, unk = R.system(hidden, border)
    assert unk.sum() == (h - 2) * (w - 2) and R.residual(A, b, x[unk]) < 1e-13
    assert (A != A.T).nnz == 0 and (A.diagonal() == 4).all()


@pytest.mark.parametrize("seed", range(3))
def test_maximum_principle(seed):
    h, w = 24, 19
    x = quarter_map((h, w), seed)
    known = np.random.default_rng(seed + 10).random((h, w)) < 0.07
    known[3, 4] = True
    got = R.fill(x, known, l_domain(24)[:, :19], empty=0.0)
    k, d = R.masks(known, l_domain(24)[:, :19], (h, w))
    unk = d & ~k & ~R.unreached(k, d)
    lab, n = R.ndimage.label(d, structure=R.CROSS)
    for c in range(1, n + 1):      # per component: the extension stays within the range of its own known values
        comp = lab == c
        if (comp & k).any() and (comp & unk).any():
            lo, hi = x[comp & k].min(), x[comp & k].max()
            assert got[comp & unk].min() >= lo - 1e-12 and got[comp & unk].max() <= hi + 1e-12


def test_unreached_components_get_empty_and_known_outside_the_domain_is_ignored():
    h, w = 9, 14
    domain = np.zeros((h, w), np.uint8)
    domain[1:8, 1:6] = 1
    domain[1:8, 8:13] = 7      # a second component, 4-separated from the first
    known = np.zeros((h, w), np.uint8)
    known[2, 2] = known[6, 4] = 1
    known[4, 6] = known[0, 0] = 1      # outside the domain: counts for nothing
    x = quarter_map((h, w), 5)
    un = R.unreached(known, domain)
    assert un[1:8, 8:13].all() and not un[1:8, 1:6].any() and not un[domain == 0].any()
    got = R.fill(x, known, domain, empty=-3.5)
    assert (got[1:8, 8:13] == -3.5).all() and (got[domain == 0] == x[domain == 0]).all()
    x2 = x.copy()
    x2[4, 6] = 1e6
    x2[0, 0] = np.nan
    assert np.array_equal(R.fill(x2, known, domain, empty=-3.5)[domain != 0], got[domain != 0])
    diag = np.zeros((4, 4), np.uint8)      # diagonal neighbours are not connected
    diag[0, 0] = diag[1, 1] = 1
    kd = np.zeros((4, 4), np.uint8)
    kd[0, 0] = 1
    assert R.unreached(kd, diag)[1, 1] and not R.unreached(kd, diag)[0, 0]


def test_kappa_is_the_norm_of_the_inverse_and_cg_reaches_the_direct_solve():
    x = quarter_map((12, 15), 3)
    known = np.random.default_rng(4).random((12, 15)) < 0.1
    known[0, 0] = True
    A, b, _ = R.system(x, known)
    inv = np.linalg.inv(A.toarray())
    assert inv.min() > -1e-14 and abs(R.kappa(A) - np.abs(inv).sum(axis=1).max()) < 1e-10
    ref = R.solve_direct(A, b)
    u, steps = R.cg(A, b, np.zeros(b.size), 1e-9, 10000)
    assert 0 < steps < 10000 and R.residual(A, b, u) <= 2e-9
    assert np.abs(u - ref).max() <= R.kappa(A) * (R.residual(A, b, u) + R.residual(A, b, ref) + 32 * 2.0 ** -53 * np.abs(x).max())
    assert R.cg(A, b, ref, 1e-9, 10000)[1] == 0


def test_seamless_with_equal_maps_returns_the_map_and_equals_the_poisson_solve():
    h, w = 16, 21
    rng = np.random.default_rng(8)
    dst, src = quarter_map((h, w), 1), quarter_map((h, w), 2)
    mask = np.zeros((h, w), np.uint8)
    mask[4:12, 5:17] = 1
    assert np.array_equal(R.seamless(dst, dst, mask), dst)
    got = R.seamless(src, dst, mask)
    assert np.array_equal(got[mask == 0], dst[mask == 0])
    # the Poisson system with the source's own Laplacian on the right: A u = b(dst on the known pixels) + (A g - b(g on the known pixels))
    known = mask == 0
    A, b_dst, unk = R.system(dst, known)
    _, b_src, _ = R.system(src, known)
    u = R.solve_direct(A, b_dst + (A @ src[unk] - b_src))
    assert np.abs(got[unk] - u).max() < 1e-11
    # a partial known set: the rest of the outside keeps dst and pins nothing
    part = known & (rng.random((h, w)) < 0.5)
    part[3, 5] = True
    got = R.seamless(src, dst, mask, known=part)
    outside = (mask == 0) & ~part
    assert np.array_equal(got[outside], dst[outside]) and np.array_equal(got[part], dst[part])


# ---- argument checks that need no device -------------------------------------------------------------------------------------------------------

def test_fill_harmonic_and_blend_seamless_validate_before_any_device():
    from hip_ext import inpaint
    x, v = np.zeros((4, 5), np.float32), np.ones((4, 5), np.uint8)
    for bad in (0.0, -1e-9, float("nan"), float("inf"), "1e-9", None, True):
        with pytest.raises(ValueError, match="tol"):
            inpaint.fill_harmonic(x, v, tol=bad, device="cpu")
    for bad in (0, -3, 2.5, "7", True, 2 ** 31):
        with pytest.raises(ValueError, match="max_iter"):
            inpaint.fill_harmonic(x, v, max_iter=bad, device="cpu")
        with pytest.raises(ValueError, match="check_every"):
            inpaint.blend_seamless(x, x, v, check_every=bad, device="cpu")
    with pytest.raises(ValueError, match="guess"):
        inpaint.fill_harmonic(x, v, guess="nearest", device="cpu")
    with pytest.raises(ValueError, match="domain"):
        inpaint.fill_harmonic(x, v, domain=np.ones((5, 4), np.uint8), device="cpu")
    with pytest.raises(ValueError, match="domain"):
        inpaint.fill_harmonic(x, v, domain=np.ones((4, 5), np.float32), device="cpu")
    with pytest.raises(ValueError, match="x of shape"):
        inpaint.fill_harmonic(np.zeros((4, 6), np.float32), v, device="cpu")
    with pytest.raises(ValueError, match="src must have dst's shape"):
        inpaint.blend_seamless(np.zeros((5, 4), np.float32), x, v, device="cpu")
    with pytest.raises(ValueError, match="src must have dst's shape"):
        inpaint.blend_seamless(np.zeros((4, 5), np.uint8), x, v, device="cpu")
    with pytest.raises(ValueError, match="known"):
        inpaint.blend_seamless(x, x, v, known=np.ones((4, 4), np.uint8), device="cpu")
    with pytest.raises(inpaint.HipExtError, match="HIP device"):      # everything valid: only now is the device looked at
        inpaint.fill_harmonic(x, v, device="cpu")
    with pytest.raises(inpaint.HipExtError, match="HIP device"):
        inpaint.blend_seamless(x, x, v, device="cpu")
    assert inpaint.default_max_iter(518, 518) == 12 * 1036 + 200


def test_amodal_infer_image_validates_blend_before_any_device():
    from hip_ext.pipeline import amodal_infer_image
    img, m = np.zeros((8, 8, 3), np.uint8), np.ones((8, 8), np.uint8)
    with pytest.raises(ValueError, match="blend must be"):
        amodal_infer_image(None, None, img, m, blend="poisson")
    with pytest.raises(ValueError, match="needs visible_masks"):
        amodal_infer_image(None, None, img, m, blend="seamless")
    with pytest.raises(ValueError, match="tol"):
        amodal_infer_image(None, None, img, m, visible_masks=m, blend="seamless", seam_tol=0.0)
    with pytest.raises(ValueError, match="max_iter"):
        amodal_infer_image(None, None, img, m, visible_masks=m, blend="seamless", seam_max_iter=0)
    with pytest.raises(TypeError):      # keyword-only
        amodal_infer_image(None, None, img, m, None, 518, None, True, False, None, 4, None, None, "seamless")


def test_fill_methods_of_geometry_name_the_harmonic_fill():
    from hip_ext import geometry
    with pytest.raises(ValueError, match="'smooth', 'nearest' or 'harmonic'"):
        geometry.remove_objects(np.zeros((4, 4), np.float32), np.zeros((4, 4), np.uint8), method="poisson")
    assert geometry._fill_fn("t", "harmonic") is geometry._inpaint.fill_harmonic


def test_new_exports_and_constants_are_declared_in_the_header():
    import hip_ext
    text = open(os.path.join(ROOT, "include", "ada_hip.h")).read()
    names = ["ada_membrane_workspace_bytes", "ada_membrane_begin_fwd", "ada_membrane_iterate_fwd", "ada_membrane_end_fwd"]
    for n in names:
        assert n in hip_ext.PROTOTYPES and re.search(r"\bint\s+" + n + r"\s*\(", text), n
    first = hip_ext.EXPORTS.index(names[0])
    assert list(hip_ext.EXPORTS[first:first + 4]) == names and hip_ext.EXPORTS[first - 1] == "ada_push_pull_fwd"      # additions under ABI 10, beside the other fills
    assert hip_ext.ABI_VERSION == 10
    for c in ("MEMBRANE_TILE_H", "MEMBRANE_TILE_W"):
        assert int(re.search(r"#define\s+ADA_" + c + r"\s+(\d+)", text).group(1)) == getattr(hip_ext, c)
    for w in ("membrane_workspace_bytes", "membrane_begin", "membrane_iterate", "membrane_end"):
        assert callable(getattr(hip_ext, w))
    build = open(os.path.join(PKG, "csrc", "build.py")).read()
    assert build.count('"ada_membrane.hip"') >= 2      # SOURCES and NO_SCRATCH


def test_depth_to_view_help_lists_the_harmonic_fill():
    out = subprocess.run([sys.executable, os.path.join(PKG, "src", "scripts", "depth_to_view.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "harmonic" in out.stdout
