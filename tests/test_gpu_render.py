"""GPU: the on-device rendering (ada_depth_render_fwd, reference infer.py:106-119) through the C ABI, hip_ext.image.render_depth,
amodal_infer_image(render=True) and the CLI's --device_render, bit for bit against the numpy restatement of the kernel (tests/_render_ref.py, which
tests/test_render_cpu.py pins to matplotlib, to the CLI's host composition and to hand-derived outlines).  Every output is an integer: no tolerance.
Output widths that are multiples of 4 take the four-pixels-per-thread kernel with dword stores, the others one pixel per thread; both are covered."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

from _cases import build_product_model, synth_state_dict
from _render_ref import render_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_CASE = dict(kind="raw", encoder="vits", features=64, out_channels=[48, 96, 192, 384])
AM_CASE = dict(kind="amodal", encoder="vits", guide_type="mask+observation", loss="entire_target_object")
FILL8, FILL16 = 0xAB, 0xABCD


@pytest.fixture(scope="module")
def lut(hip):
    from hip_ext.image import colormap_lut
    return colormap_lut("Spectral_r", "cuda")


def _depth(b, h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((b, h, w), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)      # both sides of the clip


def _blob(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy - h * 0.45) / (h * 0.3 + 0.5)) ** 2 + ((xx - w * 0.55) / (w * 0.25 + 0.5)) ** 2 <= 1) | ((yy >= h - 2) & (xx < w // 3))).astype(np.float32)


def _run(hip, lut, depth, ho, wo, minmax=None, mask=None, want_out=True, want_u16=True, **kw):
    """Launches into buffers one row too long and pre-filled; checks that nothing past [B, ho, wo(, 3)] changed.  Returns (out, u16) as numpy."""
    B = depth.shape[0]
    d = torch.from_numpy(depth).cuda()
    m = None if mask is None else torch.from_numpy(mask).cuda()
    mm = None if minmax is None else (minmax if isinstance(minmax, torch.Tensor) else torch.from_numpy(minmax).cuda())
    out = torch.full((B * ho + 1, wo, 3), FILL8, dtype=torch.uint8, device="cuda") if want_out else None
    u16 = torch.from_numpy(np.full((B * ho + 1, wo), FILL16, np.uint16)).cuda() if want_u16 else None
    hip.depth_render(d, lut, ho, wo, out, u16, minmax=mm, mask=m, **kw)
    torch.cuda.current_stream().synchronize()
    res = []
    for t, fill in ((out, FILL8), (u16, FILL16)):
        if t is None:
            res.append(None)
            continue
        a = t.cpu().numpy()
        assert (a[B * ho:] == fill).all(), "the kernel wrote past its output"
        res.append(a[:B * ho].reshape((B, ho, wo) + a.shape[2:]))
    return res


def _check(hip, lut, depth, ho, wo, minmax=None, mask=None, **kw):
    got, got16 = _run(hip, lut, depth, ho, wo, minmax=minmax, mask=mask, **kw)
    mm = minmax.cpu().numpy() if isinstance(minmax, torch.Tensor) else minmax
    want, want16 = render_ref(depth, lut.cpu().numpy(), ho, wo, minmax=mm, mask=mask, **kw)
    bad = np.nonzero((got != want).any(-1))
    assert np.array_equal(got, want), f"{len(bad[0])} pixels differ, first at {[int(i[0]) for i in bad]}"
    assert np.array_equal(got16, want16)
    return got, got16


SIZES = [((14, 14), (14, 14)), ((37, 53), (60, 80)), ((48, 64), (23, 31)), ((1, 1), (5, 7)), ((5, 1), (1, 9)), ((9, 3), (4, 1)), ((9, 3), (4, 2)),
         ((9, 3), (4, 3)), ((9, 3), (4, 5)), ((9, 3), (4, 4)), ((9, 3), (3, 8)), ((37, 53), (6, 260)), ((70, 70), (1080, 1920))]


@pytest.mark.parametrize("src,dst", SIZES)
def test_render_is_bit_identical_to_the_restatement(hip, lut, src, dst):
    depth = _depth(2, *src, seed=src[0] * 131 + dst[1])
    mask = np.stack([_blob(*src), 1 - _blob(*src)])
    _check(hip, lut, depth, *dst, mask=mask, thickness=2, outline_rgb=0, alpha=0.3, bgr=True)
    _check(hip, lut, depth, *dst)                                    # no mask: the raw rendering, R, G, B


def _five_masks(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    single = np.zeros((h, w), np.float32)
    single[h // 2, w // 3] = 1
    border = ((yy < h // 3) & (xx > w // 2)).astype(np.float32)
    return np.stack([np.zeros((h, w), np.float32), np.ones((h, w), np.float32), single, border, ((yy + xx) % 2).astype(np.float32)])


@pytest.mark.parametrize("dst", [(60, 80), (23, 31)])
def test_five_masks_every_thickness_alpha_and_channel_order(hip, lut, dst):
    depth = _depth(5, 37, 53, seed=7)
    masks = _five_masks(37, 53)
    outs = {}
    for thickness in (1, 2, 3, 4):
        for alpha in (0.0, 0.3):
            for bgr in (False, True):
                outs[thickness, alpha, bgr], _ = _check(hip, lut, depth, *dst, mask=masks, thickness=thickness, outline_rgb=0x0AC81E, alpha=alpha, bgr=bgr)
    # the empty and the full mask have no outline; the overlay covers the empty one and leaves the full one alone
    plain, _ = _run(hip, lut, depth, *dst)
    assert np.array_equal(outs[4, 0.0, False][:2], plain[:2]) and np.array_equal(outs[2, 0.3, False][1], plain[1])
    assert not np.array_equal(outs[2, 0.3, False][0], plain[0])
    assert np.array_equal(outs[3, 0.3, True], outs[3, 0.3, False][..., ::-1])
    assert (outs[2, 0.0, False][2] == np.array([0x0A, 0xC8, 0x1E], np.uint8)).all(-1).any()


def test_minmax_on_the_device_against_host_numbers(hip, lut):
    depth = (_depth(3, 29, 41, seed=2).clip(0, 1) * 4 + 2).astype(np.float32)
    depth[:, 0, 0], depth[:, 0, 1] = 2.0, 6.0                      # min and max exact in fp32, the same for every image
    mm = torch.empty(3, 2, device="cuda")
    hip.minmax(torch.from_numpy(depth).cuda(), mm)
    assert mm.cpu().tolist() == [[2.0, 6.0]] * 3
    a = _check(hip, lut, depth, 50, 64, minmax=mm)
    b = _check(hip, lut, depth, 50, 64, vmin=2.0, vmax=6.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    other = np.array([[2, 6], [0, 10], [3, 4]], np.float32)         # per image
    c = _check(hip, lut, depth, 50, 63, minmax=other)
    assert np.array_equal(c[0][0], _run(hip, lut, depth, 50, 63, vmin=2.0, vmax=6.0)[0][0]) and not np.array_equal(c[0][1], c[0][0])


def test_nan_inf_and_a_constant_image(hip, lut):
    depth = _depth(2, 21, 33, seed=4)
    depth[0, 3:9, 4:20] = np.nan
    depth[0, 10:12, :] = np.inf
    depth[0, 15, 5:9] = -np.inf
    depth[1] = 0.7
    mask = np.stack([_blob(21, 33), _blob(21, 33)])
    for dst in ((40, 48), (40, 49)):
        _check(hip, lut, depth, *dst, mask=mask, thickness=2, outline_rgb=0xFFFFFF, alpha=0.3)
        mm = torch.empty(2, 2, device="cuda")
        hip.minmax(torch.from_numpy(depth[1:]).cuda().expand(2, -1, -1).contiguous(), mm)
        got, got16 = _check(hip, lut, np.stack([depth[1], depth[1]]), *dst, minmax=mm)      # span == 0: NaN -> all black
        assert not got.any() and not got16.any()


def test_each_output_alone_equals_both_together(hip, lut):
    depth, mask = _depth(2, 37, 53, seed=9), np.stack([_blob(37, 53)] * 2)
    for dst in ((60, 80), (23, 31)):
        kw = dict(mask=mask, thickness=3, outline_rgb=0x102030, alpha=0.3, bgr=True)
        both = _check(hip, lut, depth, *dst, **kw)
        only8, none = _run(hip, lut, depth, *dst, want_u16=False, **kw)
        assert none is None and np.array_equal(only8, both[0])
        none, only16 = _run(hip, lut, depth, *dst, want_out=False, **kw)
        assert none is None and np.array_equal(only16, both[1])


def test_misaligned_outputs_take_the_one_pixel_kernel_and_give_the_same_bytes(hip, lut):
    """wo % 4 == 0 with an output pointer that is not dword aligned: the launcher must fall back to byte stores."""
    depth, mask = _depth(1, 37, 53, seed=11), _blob(37, 53)[None]
    d, m = torch.from_numpy(depth).cuda(), torch.from_numpy(mask).cuda()
    want, want16 = render_ref(depth, lut.cpu().numpy(), 60, 80, mask=mask, thickness=2, alpha=0.3, bgr=True)
    buf = torch.full((60 * 80 * 3 + 8,), FILL8, dtype=torch.uint8, device="cuda")
    buf16 = torch.from_numpy(np.full(60 * 80 + 4, FILL16, np.uint16)).cuda()
    hip.depth_render(d, lut, 60, 80, buf[1:], buf16[1:], mask=m, thickness=2, alpha=0.3, bgr=True)
    torch.cuda.synchronize()
    got, got16 = buf.cpu().numpy(), buf16.cpu().numpy()
    assert np.array_equal(got[1:1 + want.size], want.ravel()) and got[0] == FILL8 and (got[1 + want.size:] == FILL8).all()
    assert np.array_equal(got16[1:1 + want16.size], want16.ravel()) and got16[0] == FILL16 and (got16[1 + want16.size:] == FILL16).all()


def test_non_default_stream(hip, lut):
    depth, mask = _depth(2, 48, 64, seed=13), np.stack([_blob(48, 64)] * 2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for dst in ((60, 80), (23, 31)):
            _check(hip, lut, depth, *dst, mask=mask, thickness=2, outline_rgb=0, alpha=0.3, bgr=True)
    s.synchronize()


def test_render_depth_against_the_raw_wrapper(hip, lut):
    from hip_ext.image import render_depth
    depth, mask = _depth(2, 37, 53, seed=17), np.stack([_blob(37, 53), 1 - _blob(37, 53)])
    d, m = torch.from_numpy(depth).cuda(), torch.from_numpy(mask).cuda()
    got = render_depth(d, m, out_size=(60, 80), alpha=0.3, outline=(1, 2, 3), thickness=3)
    assert got.shape == (2, 60, 80, 3) and got.dtype == torch.uint8 and got.is_cuda
    want, _ = _run(hip, lut, depth, 60, 80, mask=mask, thickness=3, outline_rgb=0x010203, alpha=0.3, bgr=True)
    assert np.array_equal(got.cpu().numpy(), want)
    # defaults: no mask, the source size, B, G, R; u16 beside it; minmax; another colour map
    got, got16 = render_depth(d, u16=True)
    want, want16 = render_ref(depth, lut.cpu().numpy(), 37, 53, bgr=True)
    assert got16.dtype == torch.uint16 and np.array_equal(got.cpu().numpy(), want) and np.array_equal(got16.cpu().numpy(), want16)
    mm = torch.tensor([[0.0, 2.0], [-1.0, 1.0]], device="cuda")
    from hip_ext.image import colormap_lut
    got = render_depth(d, minmax=mm, cmap="viridis", bgr=False, out_size=(np.int64(9), 31))
    assert np.array_equal(got.cpu().numpy(), render_ref(depth, colormap_lut("viridis").numpy(), 9, 31, minmax=mm.cpu().numpy())[0])
    assert np.array_equal(render_depth(d, vmin=-1, vmax=3, bgr=False).cpu().numpy(), render_ref(depth, lut.cpu().numpy(), 37, 53, vmin=-1, vmax=3)[0])
    for kw in (dict(out_size=(0, 5)), dict(out_size=(5.0, 5)), dict(out_size="image"), dict(thickness=0), dict(thickness=5), dict(thickness=2.0),
               dict(outline=(0, 0, 256)), dict(outline=(0, 0)), dict(outline=(0.5, 0, 0)), dict(vmin=1.0, vmax=1.0), dict(alpha=1.5), dict(cmap="tab10")):
        with pytest.raises(ValueError):
            render_depth(d, m, **kw)
    for bad_mask in (m[:1], m.double(), m.cpu()):
        with pytest.raises(hip.HipExtError):
            render_depth(d, bad_mask)
    with pytest.raises(hip.HipExtError):
        render_depth(d, minmax=mm[:1])


@pytest.fixture(scope="module")
def models(hip):
    raw = build_product_model(RAW_CASE)
    raw.load_state_dict(synth_state_dict(raw), strict=True)
    am = build_product_model(AM_CASE)
    am.load_state_dict(synth_state_dict(am), strict=True)
    return raw.cuda(), am.cuda()


def _photo_and_masks():
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:60, 0:80]
    img = np.stack([(np.sin(xx / 17.0) * 0.5 + 0.5) * 255, (np.cos(yy / 11.0) * 0.5 + 0.5) * 255, (xx + yy) / 140.0 * 255], -1)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    masks = np.zeros((2, 60, 80), np.uint8)
    masks[0, 20:50, 10:40] = 255
    masks[1] = (((yy - 25) / 14.0) ** 2 + ((xx - 55) / 20.0) ** 2 <= 1) * 255
    return np.ascontiguousarray(img), masks


@pytest.mark.parametrize("out_size", ["image", None])
def test_amodal_infer_image_render(hip, models, out_size):
    from hip_ext.image import render_depth
    from hip_ext.pipeline import AmodalRendered, AmodalResult, amodal_infer_image
    raw, am = models
    img, masks = _photo_and_masks()
    S = 70
    plain = amodal_infer_image(raw, am, img, masks, size=S, out_size=out_size)
    net = plain if out_size is None else amodal_infer_image(raw, am, img, masks, size=S)       # the network-size maps
    res = amodal_infer_image(raw, am, img, masks, size=S, out_size=out_size, render=True)
    assert type(plain) is AmodalResult and type(res) is AmodalRendered and len(res) == 7
    for name in AmodalResult._fields[:4]:
        assert torch.equal(getattr(res, name), getattr(plain, name)), name
    assert res.scale_shift is None and plain.scale_shift is None
    hw = (60, 80) if out_size == "image" else (S, S)
    assert res.raw_rendered.shape == hw + (3,) and res.amodal_rendered.shape == (2,) + hw + (3,)
    assert res.raw_rendered.dtype == res.amodal_rendered.dtype == torch.uint8 and res.raw_rendered.is_cuda
    assert torch.equal(res.raw_rendered, render_depth(net.base[None], out_size=hw)[0])
    assert torch.equal(res.amodal_rendered, render_depth(net.blended, net.masks, out_size=hw))
    black = (res.amodal_rendered == 0).all(-1)
    assert bool(black[0].any()) and not bool((res.raw_rendered == 0).all(-1).any())          # the outline is there, and only there


def test_cli_device_render_writes_the_restated_pictures(hip, tmp_path):
    """Both PNGs exist at the photo's size and decode to the restatement applied to the maps of the same call made here."""
    sys.path.insert(0, ROOT)
    import infer
    from hip_ext.pipeline import amodal_infer_image
    img, masks = _photo_and_masks()
    Image.fromarray(img).save(tmp_path / "img.png")
    Image.fromarray(masks[0]).save(tmp_path / "img_mask.png")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--input_image_path", str(tmp_path / "img.png"), "--input_mask_path",
                        str(tmp_path / "img_mask.png"), "--output_folder", str(tmp_path / "out"), "--raw_encoder", "vits", "--amodal_encoder", "vits",
                        "--device_prep", "--device_render"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    files = [tmp_path / "out" / f"img_{s}.png" for s in ("raw_depth_rendered", "amodal_depth_rendered")]
    for f in files:
        assert f.exists() and Image.open(f).size == (80, 60) and Image.open(f).mode == "RGB"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        raw, am = infer.load_models("cuda", None, None, "vits", "vits")
    image_bgr = infer.imread_bgr(str(tmp_path / "img.png"))
    res = amodal_infer_image(raw, am, image_bgr, infer._read_mask(str(tmp_path / "img_mask.png")), size=518)
    table = np.asarray(__import__("matplotlib").colormaps["Spectral_r"](np.arange(256))[:, :3] * 255).astype(np.uint8)
    want_raw, _ = render_ref(res.base[None].cpu().numpy(), table, 60, 80)                        # the PNG holds R, G, B
    want_agg, _ = render_ref(res.blended.cpu().numpy(), table, 60, 80, mask=res.masks.cpu().numpy(), thickness=2, outline_rgb=0, alpha=0.0)
    assert np.array_equal(np.asarray(Image.open(files[0])), want_raw[0])
    assert np.array_equal(np.asarray(Image.open(files[1])), want_agg[0])
    assert not np.array_equal(want_raw[0], want_agg[0])
