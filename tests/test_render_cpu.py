"""CPU: what pins the on-device rendering (ada_depth_render_fwd, hip_ext.image.render_depth) without a GPU.  The numpy restatement of the kernel
(tests/_render_ref.py) against matplotlib (the table and the index rule), against the CLI's own host composition (colorize_depth_maps ->
highlight_target -> cv2's nearest resize -> flip) and against outline vectors derived by hand; the new export; the launcher's and the host API's
argument errors.  The GPU file compares the kernel with the same restatement bit for bit."""
import ctypes
import os
import subprocess
import sys

import matplotlib
import numpy as np
import pytest
import torch

import _cv2_linear as L
from _render_ref import edge_map, painted_map, render_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORT = "ada_depth_render_fwd"


def _lut(cmap="Spectral_r"):
    from hip_ext.image import colormap_lut
    return colormap_lut(cmap).numpy()


def test_lut_and_index_rule_reproduce_matplotlib():
    """lut[min(int(t * 256), 255)] with lut[i] = (cmap(i)[:3] * 255).astype(uint8) is (cmap(clip(x))[..., :3] * 255).astype(uint8): 200 000 random
    fp32 values in [0, 1), the ends, the first table boundary and its predecessor, values the clip acts on, NaN."""
    cm = matplotlib.colormaps["Spectral_r"]
    lut = _lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert np.array_equal(lut, (cm(np.arange(256))[:, :3] * 255).astype(np.uint8))
    rng = np.random.default_rng(0)
    one = np.float32(1)
    special = np.array([0, 1, np.nextafter(one, np.float32(0)), 1 / 256, np.nextafter(np.float32(1 / 256), np.float32(0)), -0.5, 1.5, 255 / 256,
                        np.nextafter(np.float32(255 / 256), np.float32(0)), np.inf, -np.inf], dtype=np.float32)
    x = np.concatenate([rng.random(200_000, dtype=np.float32), special])
    got, _ = render_ref(x[None, None], lut, 1, x.size)
    want = (cm(x.clip(0, 1))[..., :3] * 255).astype(np.uint8)
    assert np.array_equal(got[0, 0], want)
    got_nan, u16 = render_ref(np.full((1, 1, 2), np.nan, np.float32), lut, 1, 2)
    assert got_nan.tolist() == [[[[0, 0, 0], [0, 0, 0]]]] and u16.tolist() == [[[0, 0]]]
    assert (cm(np.array([np.nan]))[..., :3] * 255).astype(np.uint8).tolist() == [[0, 0, 0]]


def _scene(seed):
    rng = np.random.default_rng(seed)
    depth = (rng.random((48, 64), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)       # some values on both sides of the clip
    yy, xx = np.mgrid[0:48, 0:64]
    blob = (((yy - 20) / 11.0) ** 2 + ((xx - 30) / 17.0) ** 2 <= 1) | ((yy > 40) & (xx < 9))   # an ellipse and a patch on two borders
    return depth, blob


@pytest.mark.parametrize("alpha", [0.0, 0.3])
@pytest.mark.parametrize("out_hw", [(48, 64), (60, 80), (23, 31), (131, 97)])
def test_restatement_equals_the_cli_host_composition(alpha, out_hw):
    """colorize_depth_maps -> infer.highlight_target -> cv2's INTER_NEAREST (tests/_cv2_linear.py) -> [:, :, [2, 1, 0]], what infer.py does on the
    host (with cv2's own index rule for the resize): equal bytes."""
    import infer
    from src.util.image_util import chw2hwc, colorize_depth_maps
    depth, blob = _scene(3)
    mask255 = blob.astype(np.uint8) * 255
    colored = (colorize_depth_maps(depth, 0, 1, cmap="Spectral_r").squeeze() * 255).astype(np.uint8)
    host = infer.highlight_target(chw2hwc(colored), mask255, alpha=alpha)
    want = L.resize_nearest(host, (out_hw[1], out_hw[0]))[:, :, [2, 1, 0]]
    got, _ = render_ref(depth[None], _lut(), out_hw[0], out_hw[1], mask=blob[None].astype(np.float32), thickness=2, outline_rgb=0, alpha=alpha, bgr=True)
    assert np.array_equal(got[0], want)
    # and without a mask: the raw rendering
    want_raw = L.resize_nearest(chw2hwc(colored), (out_hw[1], out_hw[0]))[:, :, [2, 1, 0]]
    assert np.array_equal(render_ref(depth[None], _lut(), out_hw[0], out_hw[1], bgr=True)[0][0], want_raw)


def _painted(mask, thickness):
    """Pixels the restatement paints, through the whole function: a grey table, a red outline, same size out."""
    lut = np.full((256, 3), 9, np.uint8)
    out, _ = render_ref(np.full((1,) + mask.shape, 0.5, np.float32), lut, *mask.shape, mask=mask[None].astype(np.float32), thickness=thickness,
                        outline_rgb=0xFF0000)
    red = (out[0] == np.array([255, 0, 0], np.uint8)).all(-1)
    assert ((out[0] == 9).all(-1) | red).all()
    return {(int(v), int(u)) for v, u in zip(*np.nonzero(red))}


def _ball(v, u, r):
    return {(v + dv, u + du) for dv in range(-r, r + 1) for du in range(-r, r + 1) if abs(dv) + abs(du) <= r}


def test_outline_vectors_derived_by_hand():
    # one pixel at (3, 3) of 7 x 7: inside, all four neighbours outside -> it is the only edge.  thickness t paints its L1 ball of radius t - 1:
    # 1, 5 and 13 pixels.
    m = np.zeros((7, 7), bool)
    m[3, 3] = True
    assert _painted(m, 1) == {(3, 3)}
    assert _painted(m, 2) == {(3, 3), (2, 3), (4, 3), (3, 2), (3, 4)}
    assert _painted(m, 3) == _ball(3, 3, 2) and len(_ball(3, 3, 2)) == 13
    # a 3 x 3 block on rows / columns 2..4: the centre (3, 3) has four inside neighbours -> no edge; the other eight each touch the outside.
    # thickness 1: the ring of eight.  thickness 2: the centre is one step from (2, 3) -> painted; outside the block the three pixels along each
    # side are one step away, the diagonal corners (1, 1) ... are two steps from (2, 2) -> not painted: 9 + 4 * 3 = 21.
    m = np.zeros((7, 7), bool)
    m[2:5, 2:5] = True
    ring = {(v, u) for v in range(2, 5) for u in range(2, 5)} - {(3, 3)}
    assert _painted(m, 1) == ring
    t2 = ring | {(3, 3)} | {(1, u) for u in (2, 3, 4)} | {(5, u) for u in (2, 3, 4)} | {(v, 1) for v in (2, 3, 4)} | {(v, 5) for v in (2, 3, 4)}
    assert _painted(m, 2) == t2 and len(t2) == 21
    # a 3 x 3 block in the top-left corner of 6 x 6.  Neighbours past the image repeat the border pixel, so (0, 0), (0, 1), (1, 0) see only inside
    # pixels (their missing neighbours are themselves) and (1, 1) is interior: no edge on the two border sides.  (0, 2), (1, 2): right neighbour
    # outside; (2, 0), (2, 1), (2, 2): lower neighbour outside.
    m = np.zeros((6, 6), bool)
    m[0:3, 0:3] = True
    e = {(0, 2), (1, 2), (2, 0), (2, 1), (2, 2)}
    assert _painted(m, 1) == e
    # thickness 2: one step from those, inside the image only (nothing wraps, nothing is replicated): every pixel of rows 0..3 x columns 0..3
    # except (0, 0) [two steps from (0, 2) and (2, 0)] and (3, 3) [two steps from (2, 2)].
    assert _painted(m, 2) == {(v, u) for v in range(4) for u in range(4)} - {(0, 0), (3, 3)}
    # a mask that fills the image has no outside neighbour anywhere; an empty one has no inside pixel
    assert _painted(np.ones((5, 4), bool), 1) == set() and _painted(np.ones((5, 4), bool), 4) == set()
    assert _painted(np.zeros((5, 4), bool), 3) == set()
    # the two helpers on their own, batch axis in front
    assert edge_map(np.ones((2, 3, 3), bool)).sum() == 0 and painted_map(np.zeros((1, 2, 2), bool), 4).sum() == 0


def test_outline_equals_the_tree_stand_in_at_every_thickness():
    """draw_mask_outline (src/util/image_util.py) iterates a zero-padded cross thickness - 1 times; the L1-ball form of the restatement is the same set."""
    from src.util.image_util import draw_mask_outline
    _, blob = _scene(5)
    blob[0:7, 50:64] = True
    for thickness in (1, 2, 3, 4):
        img = np.zeros((48, 64, 3), np.uint8)
        want = (draw_mask_outline(img, blob.astype(np.uint8) * 255, thickness=thickness, color=(255, 255, 255)) == 255).all(-1)
        assert np.array_equal(painted_map(blob[None], thickness)[0], want), thickness


def test_overlay_bytes():
    """(uint8)((1 - alpha) * c + alpha * 200) in double, truncated: c = 9, alpha = 0.3 -> 0.7 * 9 + 60 = 66.3 -> 66; inside the mask and with
    alpha = 0 the byte stays 9.  A NaN pixel is black before the overlay: 0.7 * 0 + 60 -> 60."""
    lut = np.full((256, 3), 9, np.uint8)
    depth = np.array([[[0.5, 0.5, np.nan, 0.5]]], np.float32)
    mask = np.array([[[0, 1, 0, 1]]], np.float32)         # the inside pixels are edges: painted
    out, _ = render_ref(depth, lut, 1, 4, mask=mask, thickness=1, outline_rgb=0x010203, alpha=0.3)
    assert out[0, 0].tolist() == [[66, 66, 66], [1, 2, 3], [60, 60, 60], [1, 2, 3]]
    out, _ = render_ref(depth, lut, 1, 4, mask=mask, thickness=1, outline_rgb=0x010203, alpha=0.0, bgr=True)
    assert out[0, 0].tolist() == [[9, 9, 9], [3, 2, 1], [0, 0, 0], [3, 2, 1]]


def test_normalisation_corners_and_u16():
    lut = _lut()
    nan, inf = np.nan, np.inf
    d = np.array([[[0.25, -1.0, 2.0, nan, inf, -inf, 1.0, 0.0]]], np.float32)
    out, u16 = render_ref(d, lut, 1, 8)
    # t = 0.25, 0, 1, NaN, 1, 0, 1, 0: table entries 64, 0, 255, black, 255, 0, 255, 0; 0.25 * 65535 = 16383.75 -> 16383
    assert [o.tolist() for o in out[0, 0]] == [lut[i].tolist() if i is not None else [0, 0, 0] for i in (64, 0, 255, None, 255, 0, 255, 0)]
    assert u16[0, 0].tolist() == [16383, 0, 65535, 0, 65535, 0, 65535, 0]
    # negative values under a negative vmin: (-1 - -2) / 4 = 0.25
    out2, u2 = render_ref(np.array([[[-1.0, -2.0, 2.0, -3.0]]], np.float32), lut, 1, 4, vmin=-2.0, vmax=2.0)
    assert [o.tolist() for o in out2[0, 0]] == [lut[i].tolist() for i in (64, 0, 255, 0)] and u2[0, 0].tolist() == [16383, 0, 65535, 0]
    # minmax per image against the same numbers given as vmin / vmax (2 and 6 are exact in fp32)
    rng = np.random.default_rng(1)
    m = (rng.random((2, 5, 7), dtype=np.float32) * 4 + 2).astype(np.float32)
    m[:, 0, 0], m[:, 0, 1] = 2, 6
    a = render_ref(m, lut, 9, 11, minmax=np.array([[2, 6], [2, 6]], np.float32))
    b = render_ref(m, lut, 9, 11, vmin=2.0, vmax=6.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].max() == 65535 and a[1].min() == 0
    # a constant map with its own min / max: 0 / 0 = NaN everywhere -> black, 0
    c = np.full((1, 3, 4), 0.7, np.float32)
    out3, u3 = render_ref(c, lut, 3, 4, minmax=np.array([[0.7, 0.7]], np.float32))
    assert not out3.any() and not u3.any()


def test_new_export_and_abi_version():
    import hip_ext
    assert NEW_EXPORT in hip_ext.EXPORTS and hip_ext.ABI_VERSION == 10
    lib = hip_ext.load()
    assert lib.ada_abi_version() == 10 and hasattr(lib, NEW_EXPORT)
    header = open(os.path.join(ROOT, "include", "ada_hip.h")).read()
    assert "#define ADA_ABI_VERSION 10" in header and f"int {NEW_EXPORT}(" in header
    assert hasattr(ctypes.CDLL(hip_ext.library_path(bf16=True)), NEW_EXPORT)
    assert callable(hip_ext.depth_render)


def _call(lib, depth, lut, out, out16, batch=1, hi=4, wi=4, ho=4, wo=4, thickness=2, alpha=0.0, outline=0):
    return lib.ada_depth_render_fwd(depth, batch, hi, wi, None, 0.0, 1.0, lut, None, thickness, outline, alpha, ho, wo, 0, out, out16, None)


def test_launcher_rejects_bad_arguments_before_any_launch():
    """ADA_EINVAL with a message, no device needed: every call fails validation before the launch."""
    import hip_ext
    lib = hip_ext.load()
    p = ctypes.c_void_p(64)       # never dereferenced
    assert _call(lib, None, p, p, p) == -1 and b"null" in lib.ada_last_error()
    assert _call(lib, p, None, p, p) == -1 and b"null" in lib.ada_last_error()
    assert _call(lib, p, p, None, None) == -1 and b"both outputs" in lib.ada_last_error()
    for t in (0, 5, -1):
        assert _call(lib, p, p, p, None, thickness=t) == -1 and b"thickness" in lib.ada_last_error()
    for kw in (dict(batch=0), dict(hi=0), dict(wi=-1), dict(ho=0), dict(wo=0), dict(wo=-4)):
        assert _call(lib, p, p, p, None, **kw) == -1 and b"bad shape" in lib.ada_last_error(), kw
    for a in (-0.1, 1.5, float("nan")):
        assert _call(lib, p, p, p, None, alpha=a) == -1 and b"alpha" in lib.ada_last_error()
    assert _call(lib, p, p, p, None, outline=0x1000000) == -1 and b"outline" in lib.ada_last_error()


def test_host_api_errors_without_a_gpu():
    import hip_ext
    from hip_ext.image import colormap_lut, render_depth
    depth = torch.zeros(1, 4, 4)
    with pytest.raises(hip_ext.HipExtError, match="HIP device"):
        render_depth(depth)
    with pytest.raises(hip_ext.HipExtError, match="fp32"):
        render_depth(depth.double())
    with pytest.raises(hip_ext.HipExtError, match="fp32"):
        render_depth(torch.zeros(4, 4))
    with pytest.raises(hip_ext.HipExtError, match="fp32"):
        render_depth(np.zeros((1, 4, 4), np.float32))
    lut = torch.zeros(256, 3, dtype=torch.uint8)
    with pytest.raises(hip_ext.HipExtError, match="HIP device"):
        hip_ext.depth_render(depth, lut, 4, 4, torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(hip_ext.HipExtError, match="at least 48 elements"):
        hip_ext.depth_render(depth, lut, 4, 4, torch.zeros(1, 3, 4, 3, dtype=torch.uint8))
    with pytest.raises(hip_ext.HipExtError, match="contiguous"):
        hip_ext.depth_render(torch.zeros(1, 4, 8)[:, :, ::2], lut, 4, 4, torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    assert matplotlib.colormaps["tab10"].N == 10
    with pytest.raises(ValueError, match="256"):
        colormap_lut("tab10")
    assert colormap_lut("Spectral_r") is colormap_lut("Spectral_r")         # cached per (name, device)
    assert colormap_lut("viridis").shape == (256, 3)


def test_result_types():
    from hip_ext.pipeline import AmodalRendered, AmodalResult
    assert AmodalResult._fields == ("base", "amodal", "blended", "masks", "scale_shift")
    assert AmodalRendered._fields == AmodalResult._fields + ("raw_rendered", "amodal_rendered")


def test_cli_device_render_needs_device_prep(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--input_image_path", str(tmp_path / "a.png"), "--input_mask_path",
                        str(tmp_path / "m.png"), "--output_folder", str(tmp_path / "out"), "--device_render"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--device_render needs --device_prep" in r.stderr
    assert not (tmp_path / "out").exists()
