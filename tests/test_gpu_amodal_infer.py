"""GPU: the amodal infer_image (reference infer.py:16-119, alignment of app.py:214-216, 249-265) through the C ABI and the host API.
The preparation kernels (ada_photo_prep_fwd, ada_mask_prep_fwd, ada_nearest_resize_fwd) bit for bit against the numpy restatement of
OpenCV's / ATen's integer and index arithmetic (tests/_cv2_linear.py), ada_blend_ex against ada_blend_fwd and against what the real
reference's linear_regression_predict / median_filter_blend returned (tests/golden/amodal_infer/, tools/make_amodal_infer_golden.py),
amodal_infer_image end to end against the same kernels called one by one, and the CLI's two opt-in flags."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import _cv2_linear as L
from _cases import GOLDEN_DIR, build_product_model, synth_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX_DIR = os.path.join(GOLDEN_DIR, "amodal_infer")
FIXTURES = sorted(f[:-4] for f in os.listdir(FIX_DIR) if f.endswith(".npz"))
RAW_CASE = dict(kind="raw", encoder="vits", features=64, out_channels=[48, 96, 192, 384])
AM_CASE = dict(kind="amodal", encoder="vits", guide_type="mask+observation", loss="entire_target_object")


def _photo(h, w, c=3, seed=0):
    """uint8 BGR(A): smooth colour, fine noise (every grey level and every rounding case of the 11-bit coefficients) and a hard-edged rectangle."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.4 * np.sin(yy[..., None] * rng.uniform(0.01, 0.2, 3) + xx[..., None] * rng.uniform(0.01, 0.2, 3))
    img = np.clip(base * 255 + rng.normal(0, 30, (h, w, 3)), 0, 255)
    img[h // 3: 2 * h // 3 + 1, w // 4: w // 2 + 1] = (255, 0, 240)
    img = img.astype(np.uint8)
    if c == 4:
        img = np.concatenate([img, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=2)
    return np.ascontiguousarray(img)


def _photo_prep(hip, dev, size, raw=True, near=True):
    h, w, c = dev.shape
    r = torch.full((3, size, size), -7.0, device="cuda") if raw else None
    n = torch.full((3, size, size), -7.0, device="cuda") if near else None
    hip.photo_prep(dev, h, w, c, dev.stride(0), size, size, raw_out=r, near_out=n)
    torch.cuda.synchronize()
    return r, n


def _assert_photo(got_raw, got_near, img, size):
    want_raw, want_near = L.photo_inputs(img, size)
    if got_raw is not None:
        ints = L.resize_linear_u8(np.ascontiguousarray(img[..., :3]), (size, size)).transpose(2, 0, 1)
        assert np.array_equal((got_raw.cpu() * 255).numpy(), ints.astype(np.float32)), "raw_out * 255 is not the restated integers"
        assert torch.equal(got_raw.cpu(), torch.from_numpy(want_raw))
    if got_near is not None:
        assert torch.equal(got_near.cpu(), torch.from_numpy(want_near))


@pytest.mark.parametrize("hw,size,c", [((37, 53), 70, 3), ((53, 37), 126, 3), ((1, 1), 14, 3), ((1, 5), 28, 3), ((140, 140), 70, 3),
                                       ((140, 141), 70, 3), ((33, 47), 518, 3), ((1080, 1920), 518, 3), ((45, 61), 84, 4)])
def test_photo_prep_is_bit_identical_to_the_cv2_and_aten_restatements(hip, hw, size, c):
    img = _photo(*hw, c=c, seed=hw[0] * 7 + hw[1])
    raw, near = _photo_prep(hip, torch.from_numpy(img).cuda(), size)
    _assert_photo(raw, near, img, size)


def test_photo_prep_reads_a_pitched_crop_in_place_and_each_output_alone(hip):
    frame = _photo(200, 300, seed=11)
    dev = torch.from_numpy(frame).cuda()
    crop = dev[17:150, 31:250]                     # row pitch 300 * 3 bytes, offset start
    assert not crop.is_contiguous()
    crop_np = np.ascontiguousarray(frame[17:150, 31:250])
    raw, near = _photo_prep(hip, crop, 98)
    _assert_photo(raw, near, crop_np, 98)
    raw_only, none = _photo_prep(hip, crop, 98, near=False)
    assert none is None and torch.equal(raw_only, raw)
    none, near_only = _photo_prep(hip, crop, 98, raw=False)
    assert none is None and torch.equal(near_only, near)
    # the host API stages the same crop without a copy and gives the same planes
    from hip_ext.image import photo_to_inputs
    a, b, hw = photo_to_inputs(crop, 98, crop.device)
    assert hw == (133, 219) and a.shape == b.shape == (1, 3, 98, 98) and torch.equal(a[0], raw) and torch.equal(b[0], near)


def _masks(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    ell = (((yy - h * 0.45) / (h * 0.3)) ** 2 + ((xx - w * 0.55) / (w * 0.25)) ** 2 <= 1).astype(np.uint8) * 255
    full = np.full((h, w), 255, np.uint8)
    full[::3, ::5] = 1
    full[1::4, 2::7] = 128
    return np.stack([ell, np.zeros((h, w), np.uint8), full])


@pytest.mark.parametrize("hw,size", [((37, 53), 70), ((700, 518), 518)])
def test_mask_prep_matches_aten_nearest(hip, hw, size):
    from hip_ext.image import masks_to_tensor
    m = _masks(*hw)
    want = (F.interpolate(torch.from_numpy(m).float()[:, None], size=(size, size), mode="nearest") > 0).float()
    got01, got_pm1 = masks_to_tensor(m, size, "cuda", guide=True)
    assert got01.shape == (3, 1, size, size)
    assert torch.equal(got01.cpu(), want)
    assert torch.equal(got_pm1, 2 * got01 - 1)
    dev = got01.device
    assert torch.equal(masks_to_tensor(torch.from_numpy(m > 0).cuda(), size, dev), got01)              # bool, on the device
    assert torch.equal(masks_to_tensor(m[0], size, "cuda"), got01[:1])                                  # [h, w]
    big = torch.zeros(3, hw[0] + 5, hw[1] + 9, dtype=torch.uint8, device="cuda")                          # pitched rows, strided masks
    big[:, 2:2 + hw[0], 4:4 + hw[1]] = torch.from_numpy(m).cuda()
    assert torch.equal(masks_to_tensor(big[:, 2:2 + hw[0], 4:4 + hw[1]], size, dev), got01)


@pytest.mark.parametrize("hw,HW", [((70, 70), (37, 53)), ((518, 518), (1080, 1920)), ((5, 7), (5, 7))])
def test_nearest_resize_matches_the_cv2_rule(hip, hw, HW):
    from hip_ext.image import resize_nearest
    x = torch.randn(2, *hw, generator=torch.Generator().manual_seed(hw[0]))
    got = resize_nearest(x.cuda(), *HW).cpu()
    want = np.stack([L.resize_nearest(x[b].numpy(), (HW[1], HW[0])) for b in range(2)])
    assert got.shape == (2, *HW) and np.array_equal(got.numpy(), want)


def test_blend_ex_without_alignment_is_ada_blend_fwd(hip):
    g = torch.Generator().manual_seed(3)
    am, base = torch.rand(2, 61, 83, generator=g).cuda(), torch.rand(2, 61, 83, generator=g).cuda()
    mask = torch.zeros(2, 61, 83)
    mask[0, 10:40, 20:70] = 1
    mask[1, :25, 60:] = 1
    mask = mask.cuda()
    a, b = torch.empty_like(am), torch.empty_like(am)
    hip.blend(am, base, mask, a)
    hip.blend_ex(am, base, mask, b, None)
    assert torch.equal(a, b)
    one = torch.tensor([[1.0, 0.0], [1.0, 0.0]], device="cuda")       # the aligned kernel with the identity fit: same values
    hip.blend_ex(am, base, mask, b, one)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", FIXTURES)
def test_blend_ex_matches_the_reference_fit_and_blend(hip, name):
    """Bounds: the blend within atol = 1e-5 of the reference's, as the existing pipeline test asks; the aligned map within
    max|ref32 - ref64| + 4 * 2^-23 of the float64 evaluation -- the reference's own fp32 distance from it plus four fp32 roundings at
    magnitude <= 1 (scale, shift, product, sum; half an ulp of 1 each would be 2 * 2^-23: a factor two of slack, no more)."""
    from hip_ext.pipeline import fit_scale_shift
    z = np.load(os.path.join(FIX_DIR, name + ".npz"))
    am, base = torch.from_numpy(z["amodal"]).cuda()[None], torch.from_numpy(z["base"]).cuda()[None]
    mask, vis = torch.from_numpy(z["mask"]).float().cuda()[None], torch.from_numpy(z["visible"]).float().cuda()[None]
    ss = fit_scale_shift(am, base, vis)
    assert ss.shape == (1, 2) and ss.dtype == torch.float32
    out = torch.empty_like(am)
    hip.blend_ex(am, base, mask, out, ss)
    err_blend = float((out[0].cpu() - torch.from_numpy(z["ref_blend"])).abs().max())
    aligned = torch.empty_like(am)
    hip.blend_ex(am, base, torch.ones_like(am), aligned, ss)       # everything inside: the aligned map (its outer ring is blurred: zero-padded mask sum < 9)
    ref64 = torch.from_numpy(z["ref64"])
    err64 = float((aligned[0].cpu().double() - ref64)[1:-1, 1:-1].abs().max())
    bound64 = float((torch.from_numpy(z["ref_aligned"]).double() - ref64).abs().max()) + 4 * 2.0 ** -23
    print(f"{name}: scale, shift = {ss[0].tolist()}, blend err {err_blend:.3e} (1e-5), aligned vs float64 {err64:.3e} (bound {bound64:.3e})")
    assert err_blend <= 1e-5
    assert err64 <= bound64


class _Counted(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.calls = inner, []

    def forward(self, x, **kw):
        self.calls.append(tuple(x.shape))
        return self.inner(x, **kw)


@pytest.fixture(scope="module")
def models(hip):
    raw = build_product_model(RAW_CASE)
    raw.load_state_dict(synth_state_dict(raw), strict=True)
    am = build_product_model(AM_CASE)
    am.load_state_dict(synth_state_dict(am), strict=True)
    return raw.cuda(), am.cuda()


@pytest.fixture(scope="module")
def scene():
    img = _photo(90, 120, seed=5)
    masks = np.zeros((3, 90, 120), np.uint8)
    yy, xx = np.mgrid[0:90, 0:120]
    masks[0] = (((yy - 40) / 25.0) ** 2 + ((xx - 70) / 30.0) ** 2 <= 1) * 255
    masks[2, :35, 80:] = 255                                                     # [1] stays empty
    visible = np.zeros_like(masks)
    visible[0] = masks[0] * (xx < 75)
    visible[1, 50:80, 10:50] = 1
    visible[2, :20, 90:] = 255
    return img, masks, visible


def test_amodal_infer_image_equals_the_kernels_called_one_by_one(hip, models, scene):
    from hip_ext.pipeline import amodal_depth_pipeline, amodal_infer_image
    raw, am = models
    img, masks, _ = scene
    S = 126
    counted = _Counted(raw)
    res = amodal_infer_image(counted, am, img, masks, size=S)
    assert counted.calls == [(1, 3, S, S)], f"the base network ran {len(counted.calls)} times: {counted.calls}"
    assert res.base.shape == (S, S) and res.amodal.shape == res.blended.shape == res.masks.shape == (3, S, S) and res.scale_shift is None
    assert all(t.dtype == torch.float32 and t.is_cuda for t in (res.base, res.amodal, res.blended, res.masks))
    # inputs prepared by the restatements on the host
    raw_np, near_np = L.photo_inputs(img, S)
    rgb_raw, rgb = torch.from_numpy(raw_np)[None].cuda(), torch.from_numpy(near_np)[None].cuda()
    m01 = torch.from_numpy(np.stack([L.aten_nearest(m, S, S) for m in masks]) > 0).float()[:, None].cuda()
    assert torch.equal(res.masks, m01[:, 0])
    base1 = amodal_depth_pipeline(raw, am, rgb, m01[:1], rgb_raw=rgb_raw)[0][0]
    assert torch.equal(res.base, base1)
    with torch.no_grad():
        pred = am(rgb.expand(3, -1, -1, -1).contiguous(), guide_rgb=None, guide_mask=m01 * 2 - 1,
                  observation=(base1 * 2 - 1)[None, None].expand(3, -1, -1, -1).contiguous()).reshape(3, S, S).contiguous()
    assert torch.equal(res.amodal, pred)
    want = torch.empty_like(pred)
    hip.blend(pred, base1[None].expand(3, -1, -1).contiguous(), m01[:, 0].contiguous(), want)
    assert torch.equal(res.blended, want)
    assert torch.equal(res.blended[1], res.base), "an empty amodal mask must leave the base depth untouched"
    assert not torch.equal(res.blended[0], res.base)
    # out_size="image": the photo's shape, the restated cv2 nearest resize of the S x S result
    res_img = amodal_infer_image(raw, am, img, masks, size=S, out_size="image")
    assert res_img.base.shape == (90, 120) and res_img.blended.shape == (3, 90, 120) and res_img.amodal.shape == (3, S, S)
    assert np.array_equal(res_img.base.cpu().numpy(), L.resize_nearest(res.base.cpu().numpy(), (120, 90)))
    for k in range(3):
        assert np.array_equal(res_img.blended[k].cpu().numpy(), L.resize_nearest(res.blended[k].cpu().numpy(), (120, 90)))
    res_hw = amodal_infer_image(raw, am, img, masks, size=S, out_size=(33, 47))
    assert np.array_equal(res_hw.blended[2].cpu().numpy(), L.resize_nearest(res.blended[2].cpu().numpy(), (47, 33)))


def test_amodal_infer_image_alignment_and_its_error(hip, models, scene):
    from hip_ext.pipeline import amodal_infer_image
    raw, am = models
    img, masks, visible = scene
    S = 126
    res = amodal_infer_image(raw, am, img, masks, visible_masks=visible, size=S)
    assert res.scale_shift.shape == (3, 2) and bool(torch.isfinite(res.scale_shift).all())
    # the fit against float64 numpy on the same maps, and the paste applies it
    pred, base = res.amodal.cpu().double().numpy(), res.base.cpu().double().numpy()
    for k in range(3):
        v = L.aten_nearest(visible[k], S, S) > 0
        scale, shift = np.polyfit(pred[k][v], base[v], 1)
        assert np.allclose(res.scale_shift[k].cpu().numpy(), [scale, shift], rtol=1e-5, atol=1e-6), (k, res.scale_shift[k].tolist(), scale, shift)
    inside = res.masks[0] > 0
    inner = F.avg_pool2d(res.masks[:1, None], 3, 1, 1)[0, 0] == 1                 # away from the blurred border
    ss = res.scale_shift[0]
    assert bool(inside.any()) and torch.equal(res.blended[0][inner], (res.amodal[0] * ss[0] + ss[1])[inner])
    assert torch.equal(res.blended[1], res.base)
    # one empty visible mask: the reference's error with check=True, NaN for that entry only with check=False
    broken = visible.copy()
    broken[1] = 0
    with pytest.raises(ValueError, match="Denominator in slope calculation is zero."):
        amodal_infer_image(raw, am, img, masks, visible_masks=broken, size=S)
    res_nan = amodal_infer_image(raw, am, img, masks, visible_masks=broken, size=S, check=False)
    nan = torch.isnan(res_nan.scale_shift).cpu()
    assert nan.tolist() == [[False, False], [True, True], [False, False]]
    assert torch.equal(res_nan.scale_shift[[0, 2]], res.scale_shift[[0, 2]]) and torch.equal(res_nan.blended[[0, 2]], res.blended[[0, 2]])


def _write_cli_inputs(tmp_path):
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:60, 0:80]
    img = np.stack([(np.sin(xx / 17.0) * 0.5 + 0.5) * 255, (np.cos(yy / 11.0) * 0.5 + 0.5) * 255, (xx + yy) / 140.0 * 255], -1)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    Image.fromarray(img).save(tmp_path / "img.png")
    m = np.zeros((64, 64), dtype=np.uint8)
    m[20:50, 10:40] = 255
    Image.fromarray(m).save(tmp_path / "img_mask.png")
    v = np.zeros((64, 64), dtype=np.uint8)
    v[20:50, 10:25] = 255
    Image.fromarray(v).save(tmp_path / "img_visible.png")


def _cli(tmp_path, out, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--input_image_path", str(tmp_path / "img.png"),
                        "--input_mask_path", str(tmp_path / "img_mask.png"), "--output_folder", str(tmp_path / out),
                        "--raw_encoder", "vits", "--amodal_encoder", "vits", *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return [tmp_path / out / f"img_{s}.png" for s in ("raw_depth_rendered", "amodal_depth_rendered")]


def test_cli_device_prep_writes_both_renders(hip, tmp_path):
    _write_cli_inputs(tmp_path)
    files = _cli(tmp_path, "out", "--device_prep", "--visible_mask_path", str(tmp_path / "img_visible.png"))
    for f in files:
        assert f.exists() and Image.open(f).size == (80, 60) and Image.open(f).mode == "RGB"
    raw_png, agg_png = (np.asarray(Image.open(f)) for f in files)
    assert raw_png.std() > 0 and not np.array_equal(raw_png, agg_png)


def test_cli_without_the_flags_is_the_earlier_pipeline_byte_for_byte(hip, tmp_path):
    """The default CLI against the composition it had before the flags existed, restated here from infer.py's unchanged helpers
    (_on_device_pipeline on host-prepared inputs, host mask resize, colour map, outline, nearest resize): the PNG files are equal bytes.

    What carries the guarantee: both sides call the tree's own _on_device_pipeline, highlight_target, colorize_depth_maps, resize_nearest and
    imwrite_bgr, so a change to one of those helpers would move both sides together and go unseen here.  The test pins how the default CLI
    composes them (no new step, no new flag taken by default); that the helpers themselves compute what they computed is pinned by the tests
    they already have (test_on_device_pipeline_matches_host_composition, the image_util and CLI tests), and they must stay unchanged for this
    test to mean "as before".  A stored hash of earlier PNGs would not survive a change of GPU or library version."""
    import warnings
    sys.path.insert(0, ROOT)
    import infer
    from src.util.image_util import chw2hwc, colorize_depth_maps, imread_bgr, imwrite_bgr, resize_nearest
    _write_cli_inputs(tmp_path)
    files = _cli(tmp_path, "out")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        raw, am = infer.load_models("cuda", None, None, "vits", "vits")
    image_bgr = imread_bgr(str(tmp_path / "img.png"))
    amodal_mask = np.asarray(Image.open(tmp_path / "img_mask.png")) > 0
    base_depth, depth_agg = infer._on_device_pipeline(image_bgr, amodal_mask, raw, am, "cuda")
    raw_colored = (colorize_depth_maps(base_depth.numpy(), 0, 1, cmap="Spectral_r").squeeze() * 255).astype(np.uint8)
    raw_hwc = resize_nearest(chw2hwc(raw_colored), 80, 60)
    mask518 = (F.interpolate(torch.tensor(amodal_mask).float()[None, None], (518, 518)).squeeze().numpy() > 0).astype(np.uint8) * 255
    agg_colored = (colorize_depth_maps(depth_agg.numpy(), 0, 1, cmap="Spectral_r").squeeze() * 255).astype(np.uint8)
    agg_hwc = resize_nearest(infer.highlight_target(chw2hwc(agg_colored), mask518), 80, 60)
    os.makedirs(tmp_path / "want")
    for f, arr in zip(files, (raw_hwc, agg_hwc)):
        want = tmp_path / "want" / f.name
        imwrite_bgr(str(want), arr[:, :, [2, 1, 0]])
        assert f.read_bytes() == want.read_bytes(), f.name
