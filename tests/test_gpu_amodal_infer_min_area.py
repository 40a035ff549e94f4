"""GPU: amodal_infer_image(min_area=...) -- the demo's remove_small_noise (reference app.py:283-293) applied to the amodal masks, as given and at their
own resolution, before the preparation.  min_area=None is byte for byte the call without the argument; min_area=N is byte for byte the call on masks
cleaned on the host by the numpy restatement (tests/_components_ref.py)."""
import numpy as np
import pytest
import torch

import _components_ref as R
from _cases import build_product_model, synth_state_dict

pytestmark = pytest.mark.gpu

RAW_CASE = dict(kind="raw", encoder="vits", features=64, out_channels=[48, 96, 192, 384])
AM_CASE = dict(kind="amodal", encoder="vits", guide_type="mask+observation", loss="entire_target_object")
FIELDS = ("base", "amodal", "blended", "masks", "scale_shift")
S = 126


@pytest.fixture(scope="module")
def models(hip):
    raw = build_product_model(RAW_CASE)
    raw.load_state_dict(synth_state_dict(raw), strict=True)
    am = build_product_model(AM_CASE)
    am.load_state_dict(synth_state_dict(am), strict=True)
    return raw.cuda(), am.cuda()


@pytest.fixture(scope="module")
def scene():
    h, w = 90, 120
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.clip(128 + 100 * np.sin(yy[..., None] * 0.07 + xx[..., None] * np.array([0.05, 0.11, 0.02])) + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
    masks = np.zeros((3, h, w), np.uint8)
    masks[0] = (((yy - 40) / 25.0) ** 2 + ((xx - 70) / 30.0) ** 2 <= 1) * 255
    masks[2, :35, 80:] = 255                                                     # [1] stays empty
    visible = np.zeros_like(masks)
    visible[0] = masks[0] * (xx < 75)
    visible[1, 50:80, 10:50] = 1
    visible[2, :20, 90:] = 255
    specked = masks.copy()
    specked[0, 2:5, 3:6] = 255                   # 9 pixels
    specked[0, 80, 100] = 1                      # a singleton
    specked[1, 10:17, 10:17] = 255               # 49 pixels in the otherwise empty mask
    specked[1, 60:70, 60:65] = 255               # 50 pixels: kept at min_area = 50
    specked[2, 60:62, 5:30] = 200                # 50 pixels, kept
    specked[2, 80, ::2] = 1                      # 60 singletons
    specked[2, 35:37, 79] = 255                  # two pixels hanging on the rectangle's corner (34, 80) by a diagonal only
    return np.ascontiguousarray(img), masks, visible, specked


def _same(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f


def test_min_area_none_is_the_call_without_the_argument(hip, models, scene):
    from hip_ext.pipeline import amodal_infer_image
    raw, am = models
    img, masks, visible, specked = scene
    for kw in (dict(), dict(visible_masks=visible), dict(out_size="image")):
        plain = amodal_infer_image(raw, am, img, specked, size=S, **kw)
        none = amodal_infer_image(raw, am, img, specked, size=S, min_area=None, **kw)
        _same(plain, none)


@pytest.mark.parametrize("conn", [4, 8])
def test_min_area_equals_the_call_on_masks_cleaned_on_the_host(hip, models, scene, conn):
    from hip_ext.pipeline import amodal_infer_image
    raw, am = models
    img, masks, visible, specked = scene
    cleaned = np.stack([R.keep_area(m, 50, conn) for m in specked])
    assert cleaned.sum() < (specked > 0).sum() and cleaned[1].sum() == 50 and cleaned[2, 60:62, 5:30].all() and not cleaned[2, 80].any()
    assert bool(cleaned[2, 35, 79]) == (conn == 8)                               # the speck at the rectangle's corner hangs on it under 8 only
    want = amodal_infer_image(raw, am, img, cleaned, visible_masks=visible, size=S)
    got = amodal_infer_image(raw, am, img, specked, visible_masks=visible, size=S, min_area=50, min_area_connectivity=conn)
    _same(want, got)
    dirty = amodal_infer_image(raw, am, img, specked, visible_masks=visible, size=S)
    assert not torch.equal(dirty.masks, got.masks)                               # the specks do reach the network without the filter
    # masks on the device, bool, and a single [h, w] mask take the same path
    on_dev = amodal_infer_image(raw, am, img, torch.from_numpy(specked > 0).cuda(), visible_masks=visible, size=S, min_area=50, min_area_connectivity=conn)
    _same(want, on_dev)
    one = amodal_infer_image(raw, am, img, specked[2], size=S, min_area=50, min_area_connectivity=conn)
    one_want = amodal_infer_image(raw, am, img, cleaned[2], size=S)
    _same(one_want, one)
