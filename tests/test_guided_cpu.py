"""CPU: the guided filter's restatement (tests/_guided_ref.py) against a second one on prefix sums, its fixed points, and everything of the feature that
needs no device: the exports and constants under ABI 10, the build tables, the refusals of hip_ext.guided (raised before any device call: this machine
has none, so a call that reached the device layer would raise HipExtError instead), the new keywords of amodal_infer_image and the scripts' --guided."""
import importlib.util
import inspect
import os
import sys

import numpy as np
import pytest

import _guided_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "amodal-depth-anything_amd")
H, W = 37, 45


def scene(dtype, C, seed=0):
    """p with a step, a ramp and NaNs, a valid mask with a hole, a guide with a flat band that follows the step only partly."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    p = (1.0 + 0.02 * yy + 0.5 * (xx > 20) + 0.05 * rng.standard_normal((H, W))).astype(np.float32)
    p[rng.random((H, W)) < 0.03] = np.nan
    valid = np.ones((H, W), np.uint8)
    valid[5:12, 30:40] = 0
    g = rng.random((H, W, C)) * 0.3 + 0.6 * (xx > 22)[..., None]
    g[14:20] = 0.25                                                     # a flat band: zero variance, a = 0 up to eps
    guide = np.round(g * 255).astype(np.uint8) if dtype == np.uint8 else g.astype(np.float32)
    return p[None], valid[None], guide[None]


@pytest.mark.parametrize("dtype,C,r", [(np.uint8, 3, 1), (np.uint8, 3, 4), (np.uint8, 3, 8), (np.uint8, 3, 16), (np.float32, 3, 4), (np.float32, 3, 16),
                                       (np.uint8, 1, 8), (np.float32, 1, 4)])
@pytest.mark.parametrize("eps", [1e-2, 1e-8])
def test_direct_windows_agree_with_prefix_sums(dtype, C, r, eps):
    p, valid, guide = scene(dtype, C)
    e = R.raw_eps(eps, guide)
    q, cov = R.guided(p, guide, r, e, valid)
    q2, cov2 = R.guided(p, guide, r, e, valid, fit=R.coefficients_prefix)
    assert np.array_equal(cov, cov2)
    R.assert_close(q2, q, p, f"prefix sums {dtype.__name__} C={C} r={r} eps={eps}")


def test_grey_photo_as_three_equal_channels():
    """B = G = R makes Cov(I, I) rank one: the solve leans on eps alone in two directions."""
    p, valid, guide = scene(np.uint8, 1)
    grey = np.repeat(guide, 3, axis=-1)
    for eps in (1e-6, 1e-8):
        e = R.raw_eps(eps, grey)
        q3, _ = R.guided(p, grey, 4, e, valid)
        q3p, _ = R.guided(p, grey, 4, e, valid, fit=R.coefficients_prefix)
        R.assert_close(q3p, q3, p, f"grey eps={eps}")


def test_fixed_points():
    p, valid, guide = scene(np.uint8, 3)
    e = R.raw_eps(1e-4, guide)
    const = np.full_like(p, 2.75)
    q, cov = R.guided(const, guide, 4, e)
    assert cov.all()
    R.assert_close(q, const, const, "constant p")
    clean = np.nan_to_num(p, nan=1.5)
    q0, _ = R.guided(clean, guide, 0, e)
    R.assert_close(q0, clean, clean, "r = 0")
    qa, ca = R.guided(p, guide, 4, e, np.ones_like(valid))
    qb, cb = R.guided(p, guide, 4, e, None)
    assert np.array_equal(qa, qb, equal_nan=True) and np.array_equal(ca, cb)


def test_holes_fill_and_up_sampling_geometry():
    p, valid, guide = scene(np.uint8, 3)
    with pytest.raises(AssertionError):
        R.apply(np.zeros((1, H, W, 4)), np.ones((1, H, W), np.uint8), np.zeros((1, 90, 44, 3), np.uint8))      # the guide must cover both axes
    valid = valid.copy()
    valid[0, 24:, :20] = 0                                                          # a hole larger than two windows of r = 2
    q, cov = R.guided(p, guide, 2, R.raw_eps(1e-4, guide), valid, fill=-7.0)
    assert 0 < (cov == 0).sum() < 0.15 * cov.size
    assert ((q == -7.0) == (cov[0] == 0)).all()                                    # same size: the single tap
    # source coordinates: identity, exact 2x, and clamped ends
    assert np.array_equal(R.source(9, 9), np.arange(9.0))
    assert np.array_equal(R.source(8, 4), [0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3.0])
    assert np.array_equal(R.source(9, 1), np.zeros(9))
    assert np.array_equal(R.sample_guide(np.arange(8.0).reshape(1, 1, 8, 1), 1, 4)[0, 0, :, 0], [1, 3, 5, 7])


def test_exports_constants_and_build_tables():
    import hip_ext
    names = ["ada_guided_workspace_bytes", "ada_guided_coeff_fwd", "ada_guided_apply_fwd"]
    assert list(hip_ext.EXPORTS[-3:]) == names                                      # appended after the last existing declaration
    assert hip_ext.ABI_VERSION == 10 and hip_ext.load().ada_abi_version() == 10
    assert (hip_ext.GUIDED_MAX_RADIUS, hip_ext.GUIDED_TILE_W, hip_ext.GUIDED_APPLY_PX) == (31, 256, 4)
    header = open(os.path.join(ROOT, "include", "ada_hip.h")).read()
    assert all(f"int {n}(" in header for n in names) and "#define ADA_GUIDED_MAX_RADIUS 31" in header
    for fn in ("guided_coeff_fwd", "guided_apply_fwd", "guided_workspace_bytes"):
        assert callable(getattr(hip_ext, fn))
    spec = importlib.util.spec_from_file_location("ada_csrc_build_guided", os.path.join(PKG, "csrc", "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert "ada_guided.hip" in B.SOURCES and "ada_guided.hip" in B.NO_SCRATCH and B.PER_FILE_FLAGS["ada_guided.hip"] == ["-ffp-contract=off"]
    assert hip_ext.guided_workspace_bytes(2, 5, 7, 3) == 8 * 2 * 5 * 7 * 19 and hip_ext.guided_workspace_bytes(1, 5, 7, 1) == 8 * 5 * 7 * 8
    with pytest.raises(hip_ext.HipExtError):
        hip_ext.guided_workspace_bytes(1, 5, 7, 2)


def test_library_refuses_bad_arguments_before_any_launch():
    """The exports check everything before their first launch, so the refusals are visible without a device (the pointers are never followed)."""
    import ctypes

    import hip_ext
    lib = hip_ext.load()
    buf = ctypes.create_string_buffer(1 << 16)
    ptr = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16

    def coeff(h=4, w=5, gh=4, gw=5, C=3, r=2, eps=1.0, ws=1 << 15, dt=hip_ext.DT_U8):
        return lib.ada_guided_coeff_fwd(ptr, None, ptr, dt, 1, h, w, gh, gw, C, r, eps, ptr, ptr, ptr, ws, None)

    for bad in (dict(r=-1), dict(r=32), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(C=2), dict(C=4), dict(gh=3),
                dict(gw=4), dict(ws=8 * 4 * 5 * 19 - 1), dict(dt=hip_ext.DT_F16), dict(h=0)):
        assert coeff(**bad) == hip_ext.EINVAL, bad
    assert lib.ada_guided_apply_fwd(ptr, ptr, ptr, hip_ext.DT_U8, 1, 4, 5, 3, 5, 3, 0.0, ptr, None) == hip_ext.EINVAL
    assert lib.ada_guided_apply_fwd(ptr, ptr, ptr, hip_ext.DT_U8, 1, 4, 5, 4, 5, 2, 0.0, ptr, None) == hip_ext.EINVAL
    assert lib.ada_guided_apply_fwd(None, ptr, ptr, hip_ext.DT_U8, 1, 4, 5, 4, 5, 3, 0.0, ptr, None) == hip_ext.EINVAL


def test_python_layer_refuses_before_any_device_call():
    import hip_ext
    from hip_ext import guided as G
    p = np.ones((6, 8), np.float32)
    g3 = np.zeros((6, 8, 3), np.uint8)
    for fn in (G.guided_filter, G.guided_upsample, G.guided_coefficients):
        for radius in (-1, 32, 2.0, 2.5, True, None, "3", (3, 3)):
            with pytest.raises(ValueError, match="radius"):
                fn(p, g3, radius, 1e-3)
        for eps in (0, 0.0, -1e-3, float("inf"), float("nan"), None, True):
            with pytest.raises(ValueError, match="eps"):
                fn(p, g3, 2, eps)
        with pytest.raises(ValueError, match="1 or 3 channels"):
            fn(p, np.zeros((6, 8, 2), np.uint8), 2, 1e-3)
        with pytest.raises(ValueError, match="guide of shape"):
            fn(p, np.zeros((1, 6, 8, 3), np.uint8), 2, 1e-3)                          # a batched guide for a single map
        with pytest.raises(ValueError, match="guide of shape"):
            fn(p[None], g3, 2, 1e-3)
        with pytest.raises(ValueError, match="valid of shape"):
            fn(p, g3, 2, 1e-3, valid=np.ones((6, 7), np.uint8))
        with pytest.raises(TypeError, match="p: expected float32"):
            fn(p.astype(np.float64), g3, 2, 1e-3)
        with pytest.raises(hip_ext.HipExtError, match="uint8 or float32"):
            fn(p, g3.astype(np.float64), 2, 1e-3)
        with pytest.raises(ValueError, match="smaller than the map"):
            fn(p, np.zeros((5, 9, 3), np.uint8), 2, 1e-3)
    with pytest.raises(ValueError, match="must have p's size"):
        G.guided_filter(p, np.zeros((12, 16, 3), np.uint8), 2, 1e-3)
    # a legal call gets as far as the device layer, which this machine does not have
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(hip_ext.HipExtError, match="no CPU fallback"):
            G.guided_upsample(p, np.zeros((12, 16, 3), np.uint8), 2, 1e-3)
    assert G._eps("t", 1e-3, g3) == 1e-3 * 65025.0 and G._eps("t", 1e-3, g3.astype(np.float32)) == 1e-3


def test_amodal_infer_image_keywords():
    from hip_ext.pipeline import amodal_infer_image
    params = inspect.signature(amodal_infer_image).parameters
    assert list(params)[-3:] == ["upsample", "guided_radius", "guided_eps"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("upsample", "guided_radius", "guided_eps"))
    assert (params["upsample"].default, params["guided_radius"].default, params["guided_eps"].default) == ("nearest", 8, 1e-3)
    assert "must not guide" in amodal_infer_image.__doc__
    import torch
    model = torch.nn.Linear(1, 1)
    img, mask = np.zeros((20, 30, 3), np.uint8), np.ones((20, 30), np.uint8)
    with pytest.raises(ValueError, match="upsample must be"):
        amodal_infer_image(model, model, img, mask, size=14, upsample="bilinear")
    with pytest.raises(ValueError, match="radius"):
        amodal_infer_image(model, model, img, mask, size=14, out_size="image", upsample="guided", guided_radius=40)
    with pytest.raises(ValueError, match="eps"):
        amodal_infer_image(model, model, img, mask, size=14, out_size="image", upsample="guided", guided_eps=0)
    with pytest.raises(ValueError, match="photo's size"):
        amodal_infer_image(model, model, img, mask, size=14, out_size=(40, 60), upsample="guided")
    with pytest.raises(ValueError, match="at least as large"):
        amodal_infer_image(model, model, img, mask, size=28, out_size="image", upsample="guided")


def test_scripts_parse_guided(tmp_path):
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from PIL import Image
    from src.scripts import depth_to_mesh as M
    from src.scripts import depth_to_view as V
    for mod in (M, V):
        ap = mod.build_parser()
        assert ap.parse_args(["d.npy", "o"]).guided is None
        assert ap.parse_args(["d.npy", "o", "--image", "p.png", "--guided", "8", "1e-3"]).guided == [8.0, 1e-3]
        with pytest.raises(SystemExit):
            ap.parse_args(["d.npy", "o", "--guided", "8"])
    assert inspect.signature(M.mesh_file).parameters["guided"].default is None and inspect.signature(V.view_file).parameters["guided"].default is None
    depth, photo = str(tmp_path / "d.npy"), str(tmp_path / "p.png")
    np.save(depth, np.ones((6, 8), np.float32))
    Image.fromarray(np.zeros((12, 16, 3), np.uint8)).save(photo)
    with pytest.raises(ValueError, match="photo of shape"):
        M.mesh_file(depth, str(tmp_path / "o.ply"), image=photo)                    # without --guided a photo of another size is refused, as before
    with pytest.raises(ValueError, match="needs --image"):
        M.mesh_file(depth, str(tmp_path / "o.ply"), guided=(2, 1e-3))
    with pytest.raises(ValueError, match="needs --image"):
        V.view_file(depth, str(tmp_path / "o.png"), guided=(2, 1e-3))
    assert M.read_photo(photo, (6, 8), guided=(2, 1e-3)).shape == (12, 16, 3)
    with pytest.raises(ValueError, match="at least as large"):
        M.read_photo(photo, (13, 8), guided=(2, 1e-3))
    mask = np.arange(6 * 8).reshape(6, 8).astype(np.uint8)
    up = M.resize_mask_nearest(mask, (12, 16))
    assert up.shape == (12, 16) and np.array_equal(up[::2, ::2], mask) and np.array_equal(up[1::2, 1::2], mask)
    with pytest.raises(ValueError, match="integer"):
        M.guided_depth(np.ones((6, 8), np.float32), None, np.zeros((12, 16, 3), np.uint8), (2.5, 1e-3))
