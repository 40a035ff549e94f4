"""The device quantiles (ada_quantile_fwd), colorize (ada_depth_colorize_fwd), the range map (ada_range_map_fwd) and the normalizer built on them against
the restatements of tests/_quantile_ref.py, which tests/test_quantile_cpu.py pins to np.percentile / torch.quantile / matplotlib / the reference's goldens.
Every comparison is exact: np.array_equal with NaN positions equal (np.array_equal holds -0 == +0, the one sign the kernel leaves unspecified)."""
import functools

import numpy as np
import pytest
import torch

import _quantile_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
NUMPY_Q = (0.02, 0.95, 0.5, 0.333)
TORCH_Q = (float(F32(0.02)), float(F32(0.98)))


def _exact(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    nan = np.isnan(want) if want.dtype.kind == "f" else np.zeros(want.shape, bool)
    if want.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), nan), (got, want)
    assert np.array_equal(got[~nan], want[~nan]), (got, want)


def _device(hip, x, qs, valid=None, exclude_value=None, positive_only=False, method="numpy"):
    from hip_ext.quantile import quantiles
    res = quantiles(torch.from_numpy(np.ascontiguousarray(x)).cuda(), list(qs), valid=None if valid is None else torch.from_numpy(np.ascontiguousarray(valid)).cuda(),
                    exclude_value=exclude_value, positive_only=positive_only, method=method)
    assert res.values.dtype == torch.float64 and res.count.dtype == torch.int64
    return res.values.cpu().numpy(), res.count.cpu().numpy()


def _reference(x, qs, valid=None, exclude_value=None, positive_only=False, method="numpy"):
    vals, cnt = [], []
    for b in range(x.shape[0]):
        pop = R.population(x[b], None if valid is None else valid[b], exclude_value, positive_only)
        cnt.append(pop.size)
        if method == "numpy":
            vals.append([R.quantile_numpy(pop, q) for q in qs])
        else:
            vals.append([np.float64(R.quantile_torch(pop, F32(q))) for q in qs])
    return np.array(vals, np.float64).reshape(x.shape[0], len(qs)), np.array(cnt, np.int64)


def _check(hip, x, valid=None, exclude_value=None, positive_only=False, methods=("numpy", "torch"), qs=None):
    for method in methods:
        q = qs or (NUMPY_Q if method == "numpy" else TORCH_Q)
        got, cnt = _device(hip, x, q, valid, exclude_value, positive_only, method)
        want, wcnt = _reference(x, q, valid, exclude_value, positive_only, method)
        _exact(cnt, wcnt)
        _exact(got, want)


def _sizes(hip):
    c = hip.QUANTILE_CHUNK
    return (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, c - 1, c + 1, 3 * c + 1)


def test_every_size_one_image(hip):
    rng = np.random.default_rng(1)
    for n in _sizes(hip):
        _check(hip, rng.standard_normal((1, n)).astype(F32))


def test_every_size_batches_with_different_populations(hip):
    """Batch A: [data / mask, the same data / another mask, an empty population]; batch B: [a single element, the same data / a mask, everything]."""
    rng = np.random.default_rng(2)
    for n in _sizes(hip):
        d, e, f = (rng.standard_normal(n).astype(F32) for _ in range(3))
        m0, m1 = rng.random(n) < 0.7, rng.random(n) < 0.4
        single = np.zeros(n, bool)
        single[rng.integers(n)] = True
        _check(hip, np.stack([d, d, e]), np.stack([m0, m1, np.zeros(n, bool)]))
        _check(hip, np.stack([e, e, f]), np.stack([single, m1, np.ones(n, bool)]))


def _from_bits(bits):
    return np.asarray(bits, np.uint32).view(F32)


@functools.lru_cache(None)
def _hard_contents(n):
    rng = np.random.default_rng(n)
    first = _from_bits(np.arange(256, dtype=np.uint32) << 24)                 # 256 leading digits; all finite (0x7f000000, 0xff000000 included)
    out = {
        "last_digit_only": _from_bits(0x40490F00 + rng.integers(0, 256, n).astype(np.uint32)),
        "first_digit_only": first[rng.integers(0, 256, n)],
        "constant": np.full(n, -7.5, F32),
        "two_valued": rng.choice(np.array([0.0, 0.62], F32), n, p=[0.87, 0.13]),
        "mixed_signs": rng.choice(np.array([-np.inf, -3.0, -1.4e-45, -0.0, 0.0, 1.4e-45, 2.8e-45, 1e-39, 2.5, np.inf], F32), n),
        "heavy_ties": np.concatenate([np.full(n * 2 // 5, 1.0, F32), np.full(n - 2 * (n * 2 // 5), 1.0000001, F32), np.full(n * 2 // 5, 3.0, F32)])[rng.permutation(n)],
    }
    return out


@pytest.mark.parametrize("name", ["last_digit_only", "first_digit_only", "constant", "two_valued", "mixed_signs", "heavy_ties"])
def test_contents_a_radix_select_gets_wrong(hip, name):
    c = hip.QUANTILE_CHUNK
    for n in (2 * c, c + 1):
        x = _hard_contents(n)[name]
        rng = np.random.default_rng(7)
        batch = np.stack([x, x])
        valid = np.stack([np.ones(n, bool), rng.random(n) < 0.5])
        _check(hip, batch, valid, qs=(0.0, 0.4, 0.5, 1.0), methods=("numpy",))
        _check(hip, batch, valid, qs=(0.0, 0.6, 0.8, 1.0), methods=("numpy",))
        _check(hip, batch, valid, methods=("torch",))


def test_rank_on_a_bucket_boundary(hip):
    """256 distinct leading digits once each: every rank k / 255 is the one element of bucket k."""
    x = _from_bits(np.arange(256, dtype=np.uint32) << 24)[np.random.default_rng(3).permutation(256)][None]
    _check(hip, x, qs=(0 / 255, 1 / 255, 254 / 255, 255 / 255))
    _check(hip, x, qs=(127 / 255, 128 / 255, 0.5, 129 / 255))


def test_every_flag(hip):
    rng = np.random.default_rng(4)
    n = hip.QUANTILE_CHUNK + 77
    x = rng.standard_normal((2, n)).astype(F32)
    x[rng.random((2, n)) < 0.2] = -99
    x[rng.random((2, n)) < 0.1] = 0.0
    valid = rng.random((2, n)) < 0.8
    for v in (None, valid):
        for ex in (None, -99.0):
            for pos in (False, True):
                _check(hip, x, v, ex, pos)


def test_nan_included_and_excluded(hip):
    rng = np.random.default_rng(5)
    n = 1025
    x = np.abs(rng.standard_normal((3, n))).astype(F32) + F32(0.5)
    x[0, 17] = np.nan
    x[1, 900] = np.nan
    valid = np.ones((3, n), bool)
    valid[1, 900] = False                      # image 0 includes its NaN, image 1 masks it out, image 2 has none
    _check(hip, x, valid)
    got, cnt = _device(hip, x, NUMPY_Q, valid)
    assert np.isnan(got[0]).all() and not np.isnan(got[1:]).any() and list(cnt) == [n, n - 1, n]
    _check(hip, x, None, None, True)           # x > 0 drops both NaNs
    x[2, 3] = -99
    _check(hip, x, valid, -99.0)               # NaN != -99: still included in image 0


def test_out_f32_is_out_rounded_and_518(hip):
    from hip_ext.quantile import percentile_range
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((1, 518, 518)) * 3 + 10).astype(F32)
    x[0, :40] = -99
    r64, r32 = percentile_range(torch.from_numpy(x).cuda())
    assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and tuple(r64.shape) == tuple(r32.shape) == (1, 2)
    pop = R.population(x, exclude_value=-99)
    want = np.array([[R.quantile_numpy(pop, 2 / 100), R.quantile_numpy(pop, 95 / 100)]])
    _exact(r64.cpu().numpy(), want)
    _exact(r32.cpu().numpy(), want.astype(F32))
    _check(hip, x.reshape(1, -1), methods=("torch",))
    m = rng.random(x.shape) < 0.3
    r64m, _ = percentile_range(torch.from_numpy(x).cuda(), 5, 50, invalid_mask=torch.from_numpy(m).cuda())
    popm = x[~m]
    _exact(r64m.cpu().numpy(), np.array([[R.quantile_numpy(popm, 5 / 100), R.quantile_numpy(popm, 50 / 100)]]))


CMAP_CASES = {
    "invalid_mask": dict(mask=True),
    "invalid_val": dict(holes=True),
    "explicit": dict(vmin=2.5, vmax=6.25, cmap="Spectral_r", holes=True),
    "equal_bounds": dict(vmin=3.0, vmax=3.0),
    "nan_pixel": dict(vmin=2.0, vmax=8.0, nan=True),
    "nan_pixel_percentile": dict(nan=True),
    "everything_invalid": dict(all_invalid=True),
    "one_bound": dict(vmax=7.0, vminp=5, background_color=(1, 2, 3, 4)),
}


def _colorize_inputs(shape, case, seed):
    rng = np.random.default_rng(seed)
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    imgs, masks = [], []
    for b in range(2):
        d = (2.0 + 0.05 * x + 0.03 * y + rng.standard_normal((h, w)) * 0.25 * (b + 1)).astype(F32)
        d[y + x > 0.8 * (h + w)] = 9.5
        if case.get("holes"):
            d[rng.random((h, w)) < 0.1] = -99
        if case.get("nan"):
            d[3, 4 + b] = np.nan
        if case.get("all_invalid"):
            d[:] = -99
        imgs.append(d)
        masks.append(rng.random((h, w)) < 0.3)
    return np.stack(imgs), (np.stack(masks) if case.get("mask") else None)


@pytest.mark.parametrize("shape", [(37, 53), (64, 64), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_colorize_bytes_equal_the_restatement(hip, shape):
    from hip_ext.image import colorize
    for i, (name, case) in enumerate(CMAP_CASES.items()):
        value, mask = _colorize_inputs(shape, case, 10 + i)
        kw = {k: v for k, v in case.items() if k in ("vmin", "vmax", "cmap", "vminp", "vmaxp", "background_color")}
        got = colorize(torch.from_numpy(value).cuda(), invalid_mask=None if mask is None else torch.from_numpy(mask).cuda(), **kw)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2,) + shape + (4,) and got.is_cuda
        want = np.stack([R.colorize(value[b], invalid_mask=None if mask is None else mask[b], **kw) for b in range(2)])
        assert np.array_equal(got.cpu().numpy(), want), name
    one = colorize(torch.from_numpy(value[0]).cuda(), **kw)               # a single [H, W] map
    assert np.array_equal(one.cpu().numpy()[0], want[0])


def test_capture_replays_follow_contents_and_mask(hip):
    from hip_ext.image import colorize
    from hip_ext.quantile import percentile_range
    rng = np.random.default_rng(8)
    shape = (2, 130, 70)

    def draw(frac):
        return (rng.standard_normal(shape) * 2 + 5).astype(F32), rng.random(shape) < frac

    v0, m0 = draw(0.2)
    value, mask = torch.from_numpy(v0).cuda(), torch.from_numpy(m0).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up: tables, allocator
        percentile_range(value, invalid_mask=mask)
        colorize(value, invalid_mask=mask)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r64, r32 = percentile_range(value, invalid_mask=mask)
        img = colorize(value, invalid_mask=mask)
    for frac in (0.6, 0.05):                               # new contents AND a new mask: the population count changes
        v1, m1 = draw(frac)
        value.copy_(torch.from_numpy(v1))
        mask.copy_(torch.from_numpy(m1))
        graph.replay()
        torch.cuda.synchronize()
        e64, e32 = percentile_range(value, invalid_mask=mask)
        eimg = colorize(value, invalid_mask=mask)
        _exact(r64.cpu().numpy(), e64.cpu().numpy())
        _exact(r32.cpu().numpy(), e32.cpu().numpy())
        assert torch.equal(img, eimg)
        want = np.array([[R.quantile_numpy(v1[b][~m1[b]], 0.02), R.quantile_numpy(v1[b][~m1[b]], 0.95)] for b in range(2)])
        _exact(r64.cpu().numpy(), want)
        assert np.array_equal(img.cpu().numpy(), np.stack([R.colorize(v1[b], invalid_mask=m1[b]) for b in range(2)]))


@pytest.mark.parametrize("norm", [(-1.0, 1.0), (0.0, 1.0)], ids=["pm1", "unit"])
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
def test_range_map_is_the_torch_cpu_expression(hip, norm, clip):
    rng = np.random.default_rng(9)
    d = torch.from_numpy((rng.standard_normal((3, 33, 47)) * 4 + 3).astype(F32))
    d[0, 0, 0], d[1, 2, 3] = float("nan"), float("inf")
    rng32 = torch.tensor([[0.5, 7.25], [-1.0, 0.1], [2.0, 2.0]], dtype=torch.float32)     # the last image: lo == hi
    lo, hi = rng32[:, 0].view(3, 1, 1), rng32[:, 1].view(3, 1, 1)
    want = (d - lo) / (hi - lo) * (norm[1] - norm[0]) + norm[0]
    if clip:
        want = torch.clip(want, norm[0], norm[1])
    out = torch.empty(3, 33, 47, dtype=torch.float32, device="cuda")
    hip.range_map(d.cuda(), rng32.cuda(), out, scale=norm[1] - norm[0], shift=norm[0], clip=norm if clip else None)
    _exact(out.cpu().numpy(), want.numpy())


def test_normalizer_quantiles_and_map(hip):
    import types
    from src.util.depth_transform import get_depth_normalizer
    rng = np.random.default_rng(11)
    d = (np.abs(rng.standard_normal((3, 45, 61))) * np.array([1.0, 0.3, 5.0]).reshape(3, 1, 1) + 0.2).astype(F32)
    d[rng.random(d.shape) < 0.05] = 0.0
    d[rng.random(d.shape) < 0.05] = -2.0
    valid = rng.random(d.shape) < 0.85
    dd, vv = torch.from_numpy(d).cuda(), torch.from_numpy(valid).cuda()
    for cfg in (dict(norm_min=-1.0, norm_max=1.0, min_max_quantile=0.02, clip=True), dict(norm_min=0.0, norm_max=1.0, min_max_quantile=0.1, clip=False)):
        norm = get_depth_normalizer(types.SimpleNamespace(type="scale_shift_depth", **cfg))
        qs = torch.tensor([norm.min_quantile, norm.max_quantile])
        for v_np, v_dev in ((valid, vv), (None, None)):
            sel = (valid if v_np is not None else np.ones(d.shape, bool)) & (d > 0)
            # reference meaning: one population
            _exact(norm.quantile_range(dd, v_dev).cpu().numpy(), torch.quantile(torch.from_numpy(d[sel]), qs).numpy()[None])
            _exact(norm(dd, v_dev).cpu().numpy(), R.normalize(d, v_np, **cfg))
            # per image
            want_q = np.stack([torch.quantile(torch.from_numpy(d[b][sel[b]]), qs).numpy() for b in range(3)])
            _exact(norm.quantile_range(dd, v_dev, per_image=True).cpu().numpy(), want_q)
            _exact(norm(dd, v_dev, per_image=True).cpu().numpy(), R.normalize(d, v_np, per_image=True, **cfg))
    assert norm(dd, vv, clip=True).max().item() <= 1.0


def test_render_depth_takes_the_percentile_range(hip):
    from hip_ext.image import render_depth
    from hip_ext.quantile import percentile_range
    rng = np.random.default_rng(12)
    d = torch.from_numpy((rng.standard_normal((1, 70, 90)) * 2 + 5).astype(F32)).cuda()
    _, r32 = percentile_range(d)
    lo, hi = (float(v) for v in r32[0].cpu())
    a = render_depth(d, minmax=r32)
    b = render_depth(d, vmin=lo, vmax=hi)
    assert a.dtype == torch.uint8 and torch.equal(a, b)
    assert not torch.equal(a, render_depth(d, vmin=float(d.min()), vmax=float(d.max())))


def test_colorize_depth_command_line(hip, tmp_path):
    """16-bit PNG and .npy in a folder -> PNGs whose R, G, B equal the restatement's (the alpha channel is dropped, as the reference's script does)."""
    from PIL import Image
    from src.scripts import colorize_depth as C
    rng = np.random.default_rng(13)
    d16 = (rng.random((37, 53)) * 40000 + 500).astype(np.uint16)
    d16[rng.random(d16.shape) < 0.1] = 0
    f32 = (rng.standard_normal((41, 23)) * 2 + 5).astype(F32)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(d16).save(src / "a.png")
    np.save(src / "b.npy", f32)
    assert C.main([str(src), str(dst), "--cmap", "magma_r", "--vminp", "5", "--vmaxp", "90", "--invalid_val", "0"]) == 0
    for name, depth in (("a", d16.astype(F32)), ("b", f32)):
        got = np.asarray(Image.open(dst / f"{name}.png"))
        want = R.colorize(depth, cmap="magma_r", invalid_val=0, vminp=5, vmaxp=90)[:, :, :3]
        assert got.shape == want.shape and np.array_equal(got, want), name


def test_invalid_val_that_fp32_cannot_hold_is_one_rule_for_range_and_paint(hip):
    """invalid_val = 0.1: pixels holding fp32(0.1) are neither left out of the percentiles nor painted (both compare in double); fp32(0.1) itself excludes them."""
    from hip_ext.image import colorize
    from hip_ext.quantile import percentile_range
    rng = np.random.default_rng(14)
    v = (rng.random((2, 37, 53)) * 3).astype(F32)
    v[rng.random(v.shape) < 0.3] = F32(0.1)
    dev = torch.from_numpy(v).cuda()
    for inv in (0.1, float(F32(0.1))):
        got = colorize(dev, invalid_val=inv).cpu().numpy()
        assert np.array_equal(got, np.stack([R.colorize(v[b], invalid_val=inv) for b in range(2)])), inv
        r64, _ = percentile_range(dev, invalid_val=inv)
        pops = [R.population(v[b], exclude_value=inv) for b in range(2)]
        _exact(r64.cpu().numpy(), np.array([[R.quantile_numpy(p, 0.02), R.quantile_numpy(p, 0.95)] for p in pops]))
    assert pops[0].size < v[0].size


@pytest.fixture(scope="module")
def small_models(hip):
    from _cases import build_product_model, synth_state_dict
    raw = build_product_model(dict(kind="raw", encoder="vits", features=64, out_channels=[48, 96, 192, 384]))
    raw.load_state_dict(synth_state_dict(raw), strict=True)
    am = build_product_model(dict(kind="amodal", encoder="vits", guide_type="mask+observation", loss="entire_target_object"))
    am.load_state_dict(synth_state_dict(am), strict=True)
    return raw.cuda(), am.cuda()


def test_amodal_infer_image_render_percentiles(hip, small_models):
    """render_percentiles=(lo, hi): each picture is render_depth between the percentiles of its own map; None: byte-identical to the call without it."""
    from hip_ext.image import render_depth
    from hip_ext.pipeline import amodal_infer_image
    from hip_ext.quantile import percentile_range
    raw, am = small_models
    rng = np.random.default_rng(15)
    yy, xx = np.mgrid[0:60, 0:80]
    img = np.clip(np.stack([xx * 3.0, yy * 4.0, (xx + yy) * 1.5], -1) + rng.normal(0, 6, (60, 80, 3)), 0, 255).astype(np.uint8)
    masks = np.zeros((2, 60, 80), np.uint8)
    masks[0, 20:50, 10:40] = 255
    masks[1, 5:30, 45:75] = 255
    S = 70
    net = amodal_infer_image(raw, am, img, masks, size=S)
    plain = amodal_infer_image(raw, am, img, masks, size=S, out_size="image", render=True)
    none = amodal_infer_image(raw, am, img, masks, size=S, out_size="image", render=True, render_percentiles=None)
    assert torch.equal(plain.raw_rendered, none.raw_rendered) and torch.equal(plain.amodal_rendered, none.amodal_rendered)
    res = amodal_infer_image(raw, am, img, masks, size=S, out_size="image", render=True, render_percentiles=(2, 95))
    for name in ("base", "amodal", "blended", "masks"):
        assert torch.equal(getattr(res, name), getattr(plain, name)), name
    base = net.base[None].contiguous()
    r_base = percentile_range(base, 2, 95, invalid_val=None)[1]
    r_blend = percentile_range(net.blended, 2, 95, invalid_val=None)[1]
    assert torch.equal(res.raw_rendered, render_depth(base, out_size=(60, 80), minmax=r_base)[0])
    assert torch.equal(res.amodal_rendered, render_depth(net.blended, net.masks, out_size=(60, 80), minmax=r_blend))
    assert not torch.equal(res.raw_rendered, plain.raw_rendered)
    b = net.base.cpu().numpy()
    _exact(r_base.cpu().numpy(), np.array([[R.quantile_numpy(b, 0.02), R.quantile_numpy(b, 0.95)]]).astype(F32))


def test_infer_cli_render_percentiles(hip, tmp_path):
    """infer_single_image(device_render=True, render_percentiles=...) writes the pictures of amodal_infer_image(render_percentiles=...); without it the default ones."""
    import os
    import sys
    import warnings
    from PIL import Image
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import infer
    from hip_ext.pipeline import amodal_infer_image
    rng = np.random.default_rng(16)
    img = rng.integers(0, 255, (40, 56, 3), dtype=np.uint8)
    mask = np.zeros((40, 56), np.uint8)
    mask[10:30, 12:40] = 255
    Image.fromarray(img).save(tmp_path / "p.png")
    Image.fromarray(mask).save(tmp_path / "p_mask.png")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        raw, am = infer.load_models("cuda", None, None, "vits", "vits")
    args = (str(tmp_path / "p.png"), str(tmp_path / "p_mask.png"))
    bgr, m = infer.imread_bgr(args[0]), infer._read_mask(args[1])
    for pct in (None, (2.0, 95.0)):
        out = tmp_path / ("default" if pct is None else "pct")
        raw_out, agg_out = infer.infer_single_image(*args, str(out), raw, am, "cuda", device_prep=True, device_render=True, render_percentiles=pct)
        want = amodal_infer_image(raw, am, bgr, m, size=518, out_size="image", render=True, **({} if pct is None else {"render_percentiles": pct}))
        assert np.array_equal(raw_out, want.raw_rendered.cpu().numpy()) and np.array_equal(agg_out, want.amodal_rendered[0].cpu().numpy())
        assert (out / "p_raw_depth_rendered.png").exists() and (out / "p_amodal_depth_rendered.png").exists()
