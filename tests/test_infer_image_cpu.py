"""CPU: the raw model's infer_image / image2tensor (reference RAW/dpt.py:186-221).  The host-side size rule against the reference's own
Resize.get_size (tests/golden/infer_image/sizes.json), the numpy restatement of cv2's float INTER_CUBIC path that the GPU tests hold the
prep kernel to (tests/_cv2_cubic.py; cv2 itself is not available), the method surface of the reference class, and the refusals that need
no device."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import _cv2_cubic as C
from _cases import GOLDEN_DIR

IMG_DIR = os.path.join(GOLDEN_DIR, "infer_image")


def test_network_size_matches_the_reference_get_size():
    from hip_ext.image import network_size
    rows = json.load(open(os.path.join(IMG_DIR, "sizes.json")))
    assert len(rows) > 2000
    bad = [r for r in rows if network_size(r[0], r[1], r[2]) != (r[3], r[4])]
    assert not bad, bad[:10]
    # the half-way ties round to even (np.round): 208 * 70 / 160 = 91 = 6.5 * 14 -> 84, not 98; 150 * 518 / 100 = 777 = 55.5 * 14 -> 784
    assert [160, 208, 70, 70, 84] in rows and network_size(160, 208, 70) == (70, 84)
    assert [100, 150, 518, 518, 784] in rows and network_size(100, 150, 518) == (518, 784)


def test_cubic_restatement_row_of_four_to_eight_hand_derived():
    """[0, 1, 2, 3] resized 4 -> 8: scale_x = 1 / (8 / 4) = 0.5, fx = (dx + 0.5) * 0.5 - 0.5 = -0.25, 0.25, 0.75, 1.25, ...
    so every output pixel sits at fraction x = 0.75 or 0.25 of its interval, and interpolateCubic (A = -0.75) gives, exactly in fp32,
      x = 0.75:  c0 = ((A 1.75 - 5A) 1.75 + 8A) 1.75 - 4A = ((-1.3125 + 3.75) 1.75 - 6) 1.75 + 3 = -0.03515625
                 c1 = ((A + 2) 0.75 - (A + 3)) 0.75^2 + 1 = (0.9375 - 2.25) 0.5625 + 1 = 0.26171875
                 c2 = ((A + 2) 0.25 - (A + 3)) 0.25^2 + 1 = (0.3125 - 2.25) 0.0625 + 1 = 0.87890625
                 c3 = 1 - c0 - c1 - c2 = -0.10546875
      x = 0.25:  the same four in reverse order (-0.10546875, 0.87890625, 0.26171875, -0.03515625).
    dx = 0: sx = floor(-0.25) = -1, taps -2, -1, 0, 1 clamp to pixels 0, 0, 0, 1 -> c3 * 1 = -0.10546875: the edge is REPLICATED (a zero
            border would give the same here, but a reset fx = 0 would give 0) and the result is NOT clamped to the input's range;
    dx = 1: sx = 0, x = 0.25, taps 0, 0, 1, 2 -> 0.26171875 - 2 * 0.03515625 = 0.19140625;
    dx = 2: sx = 0, x = 0.75, taps 0, 0, 1, 2 -> 0.87890625 - 2 * 0.10546875 = 0.66796875;
    dx = 3: sx = 1, x = 0.25, taps 0, 1, 2, 3 -> 0.87890625 + 2 * 0.26171875 - 3 * 0.03515625 = 1.296875;
    dx = 4..7 mirror dx = 3..0 about 1.5 (the row is symmetric about its centre under x -> 3 - x)."""
    out = C.resize(np.array([[0.0, 1.0, 2.0, 3.0]]), (8, 1))
    expect = [-0.10546875, 0.19140625, 0.66796875, 1.296875, 1.703125, 2.33203125, 2.80859375, 3.10546875]
    np.testing.assert_array_equal(out, np.array([expect]))
    np.testing.assert_array_equal(C.cubic_coeffs(np.float32(0.75)), np.float32([-0.03515625, 0.26171875, 0.87890625, -0.10546875]))
    np.testing.assert_array_equal(C.cubic_coeffs(np.float32(0.25)), np.float32([-0.10546875, 0.87890625, 0.26171875, -0.03515625]))


def test_cubic_restatement_constant_single_pixel_and_identity():
    # a constant image stays constant (up to the fp32 rounding of c3 = 1 - c0 - c1 - c2: the coefficients sum to 1 within 2^-23)
    for dsize in ((20, 5), (4, 3), (61, 200)):
        out = C.resize(np.full((7, 9, 3), 0.3), dsize)
        assert out.shape == (dsize[1], dsize[0], 3) and np.abs(out - 0.3).max() <= 1e-7
    # a 1-pixel source: every tap clamps to the one pixel
    px = np.array([[[0.2, 0.5, 0.9]]])
    for dsize in ((14, 14), (28, 14), (3, 1)):
        out = C.resize(px, dsize)
        assert np.abs(out - px).max() <= 1e-7
    # same size: the identity (cv2 copies; the coefficients at x = 0 are exactly (0, 1, 0, 0) as well)
    img = np.random.default_rng(0).random((13, 17, 3))
    np.testing.assert_array_equal(C.resize(img, (17, 13)), img)
    np.testing.assert_array_equal(C.cubic_coeffs(np.float32(0.0)), np.float32([0, 1, 0, 0]))
    idx, coef = C.taps(17, 17)
    np.testing.assert_array_equal(coef, np.tile(np.float32([0, 1, 0, 0]), (17, 1)))
    np.testing.assert_array_equal(idx[:, 1], np.arange(17))
    # BGR -> RGB, and BGRA loses its alpha
    bgra = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    np.testing.assert_array_equal(C.cvt_color(bgra, C.COLOR_BGR2RGB), bgra[..., [2, 1, 0]])
    np.testing.assert_array_equal(C.cvt_color(bgra[..., :3], C.COLOR_BGR2RGB), bgra[..., [2, 1, 0]])


def test_raw_model_has_the_reference_surface():
    from src.models.amodalsynthdrive.depth_anything_v2_raw.dpt import DepthAnythingV2
    surface = json.load(open(os.path.join(IMG_DIR, "surface.json")))
    assert {"forward", "infer_image", "image2tensor"} <= set(surface)
    for name, params in surface.items():
        fn = getattr(DepthAnythingV2, name, None)
        assert callable(fn), name
        mine = [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in inspect.signature(fn).parameters.values()]
        assert mine[:len(params)] == params, (name, mine, params)     # the reference's parameters first, same names and defaults


def _cpu_model():
    from src.models.amodalsynthdrive.depth_anything_v2_raw.dpt import DepthAnythingV2
    return DepthAnythingV2(encoder="vits", features=64, out_channels=(48, 96, 192, 384)).eval()


def test_infer_image_on_a_cpu_model_refuses():
    import hip_ext
    m = _cpu_model()
    img = np.zeros((20, 30, 3), dtype=np.uint8)
    with pytest.raises(hip_ext.HipExtError, match="HIP device"):
        m.infer_image(img)
    with pytest.raises(hip_ext.HipExtError, match="HIP device"):
        m.image2tensor(img, 70)


def test_image_type_and_shape_are_checked():
    m = _cpu_model()
    with pytest.raises(TypeError):
        m.infer_image(np.zeros((20, 30, 3), dtype=np.uint16))
    with pytest.raises(TypeError):
        m.infer_image(torch.zeros(20, 30, 3))
    with pytest.raises(TypeError):
        m.infer_image([[0, 0, 0]])
    for shape in ((20, 30), (20, 30, 1), (20, 30, 5), (1, 20, 30, 3), (0, 30, 3)):
        with pytest.raises(ValueError):
            m.infer_image(np.zeros(shape, dtype=np.uint8))
