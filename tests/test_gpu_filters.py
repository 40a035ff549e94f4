"""GPU: the rank filters of csrc/ada_filters.hip against the numpy restatement of their contract (tests/_filters_ref.py), exactly: values with
np.array_equal where a sample voted, the fill where none did, the counts exactly.  Then what is built on them: the morphology of hip_ext.masks against
scipy's explicit compositions, depth_to_mesh(median=...) and amodal_infer_image(close=...) against the same calls on maps filtered on the host.

The general kernel's workgroup owns FILTER_TILE_H x FILTER_TILE_W = 4 x 64 outputs, the extremes' column pass FILTER_COL_TILE_H = 16 rows: the shapes
below sit one under, on and one over each of them."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import _components_ref as C
import _filters_ref as F

pytestmark = pytest.mark.gpu

TILE_W, TILE_H, COL_TILE_H = 64, 4, 16
SMALL = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (1, 2, 3), (1, 5, 5), (1, TILE_H - 1, TILE_W - 1), (1, TILE_H, TILE_W), (1, TILE_H + 1, TILE_W + 1),
         (1, COL_TILE_H - 1, TILE_W + 1), (1, COL_TILE_H, TILE_W - 1), (1, COL_TILE_H + 1, TILE_W)]
LARGE = [(1, 71, 131), (3, 9, 70)]
RANK_SIZES = [3, 5, 7, 9, (3, 27), (27, 3)]
EXTREME_SIZES = [3, 31, 63, (1, 63), (63, 1), (3, 9)]
VALIDS = ["none", "random", "single", "empty", "checker"]
PERCENTS = [0, 25, 50, 100]
SPECIALS = [np.inf, -np.inf, -0.0, np.nan, 1e-42]


def make_map(shape, dtype, seed):
    """Values from a range of nine, so ties dominate: quarter-integers (fp32, with cells of +inf, -inf, -0.0, NaN and a denormal planted) or bytes."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 9, shape)
    if dtype == np.uint8:
        return (q * 31).astype(np.uint8)
    x = (q / 4.0 - 1.0).astype(np.float32)
    flat = x.reshape(shape[0], -1)
    for b in range(shape[0]):
        cells = rng.permutation(flat.shape[1])[:len(SPECIALS)] if flat.shape[1] >= 12 else []
        for c, v in zip(cells, SPECIALS):
            flat[b, c] = v
    return x


def make_valid(kind, shape, seed):
    """None, or uint8 [B, h, w], different per image: random at 60 %, one valid pixel, none, a checkerboard."""
    rng = np.random.default_rng(seed + 1000)
    B, h, w = shape
    if kind == "none":
        return None
    if kind == "random":
        return (rng.random(shape) < 0.6).astype(np.uint8) * 3      # any non-zero value votes
    if kind == "single":
        v = np.zeros(shape, np.uint8)
        for b in range(B):
            v[b, rng.integers(h), rng.integers(w)] = 1
        return v
    if kind == "empty":
        return np.zeros(shape, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([((yy + xx + b) % 2).astype(np.uint8) for b in range(B)])


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _run(hip, kernel, x, v, size, rank, border, fill):
    """(out, count) as numpy from one launch of the general ('rank') or the separable ('extreme') kernel on device tensors."""
    kh, kw = F.window(size)
    out = torch.empty_like(x)
    count = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    code = {"min": hip.RANK_MIN, "median": hip.RANK_MEDIAN, "max": hip.RANK_MAX}.get(rank, rank)
    b = {"mirror": hip.BORDER_MIRROR, "nearest": hip.BORDER_NEAREST, "ignore": hip.BORDER_IGNORE}[border]
    (hip.rank_filter_fwd if kernel == "rank" else hip.extreme_filter_fwd)(x, kh, kw, code, b, out, valid=v, fill=fill, count=count)
    return out.cpu().numpy(), count.cpu().numpy()


def _assert_same(got, cnt, want, n, fill, what):
    assert np.array_equal(cnt, n), f"{what}: counts differ at {np.argwhere(cnt != n)[:4].tolist()}"
    voted = n > 0
    assert np.array_equal(got[voted], want[voted]), f"{what}: values differ at {np.argwhere(voted & (got != want))[:4].tolist()}"
    assert not np.isnan(got[voted]).any(), what
    empty = got[~voted]
    assert np.isnan(empty).all() if fill != fill else (empty == fill).all(), f"{what}: fill"


def _sweep_general(hip, shapes, dtype, border, valids, ranks, seed):
    fill = float("nan") if dtype == np.float32 else 7
    for shape in shapes:
        x = make_map(shape, dtype, seed)
        xd = _dev(x)
        for kind in valids:
            v = make_valid(kind, shape, seed)
            vd = _dev(v)
            for size in RANK_SIZES:
                s, n = F.sorted_windows(x, size, border, v)      # one sort serves every rank
                for rank in ranks:
                    got, cnt = _run(hip, "rank", xd, vd, size, rank, border, fill)
                    _assert_same(got, cnt, F.pick(s, n, rank, dtype, fill), n, fill, f"{shape} {size} {kind} {rank} {border}")


@pytest.mark.parametrize("border", F.BORDERS)
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_general_kernel_every_rank_small_shapes(hip, dtype, border):
    _sweep_general(hip, SMALL, dtype, border, VALIDS, ["min", "median", "max"] + PERCENTS, 11)


@pytest.mark.parametrize("border", F.BORDERS)
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_general_kernel_odd_shape_and_batch(hip, dtype, border):
    _sweep_general(hip, LARGE, dtype, border, ["none", "random"], ["median", 25], 12)


@pytest.mark.parametrize("border", F.BORDERS)
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_separable_extremes(hip, dtype, border):
    fill = -3.0 if dtype == np.float32 else 0
    squares = [(1, 1, 1), (1, 5, 5), (1, TILE_H + 1, TILE_W + 1), (1, COL_TILE_H + 1, TILE_W)] + LARGE      # the brute-force reference of 31 x 31 and 63 x 63 walks
    for shape in SMALL + LARGE:                                                                             # thousands of positions: fewer maps for these two
        x = make_map(shape, dtype, 13)
        xd = _dev(x)
        for kind in (VALIDS if shape not in LARGE else ["none", "random"]):
            v = make_valid(kind, shape, 13)
            vd = _dev(v)
            for size in EXTREME_SIZES:
                if size in (31, 63) and (shape not in squares or kind not in ("none", "random")):
                    continue
                lo, hi, n = F.extremes(x, size, border, v)
                for rank, ref in (("min", lo), ("max", hi)):
                    with np.errstate(invalid="ignore"):
                        want = np.where(n > 0, ref, fill).astype(dtype)
                    got, cnt = _run(hip, "extreme", xd, vd, size, rank, border, fill)
                    _assert_same(got, cnt, want, n, fill, f"{shape} {size} {kind} {rank} {border}")


def test_both_kernels_agree_on_the_extremes_and_runs_repeat(hip):
    for dtype in (np.float32, np.uint8):
        x = make_map((3, 33, 70), dtype, 14)
        v = make_valid("random", x.shape, 14)
        xd, vd = _dev(x), _dev(v)
        for border in F.BORDERS:
            for size in (3, 9, (3, 27)):
                for rank in ("min", "max"):
                    a, na = _run(hip, "rank", xd, vd, size, rank, border, 0.0)
                    b, nb = _run(hip, "extreme", xd, vd, size, rank, border, 0.0)
                    assert a.tobytes() == b.tobytes() and na.tobytes() == nb.tobytes(), (dtype, border, size, rank)
                    b2, nb2 = _run(hip, "extreme", xd, vd, size, rank, border, 0.0)
                    assert b.tobytes() == b2.tobytes() and nb.tobytes() == nb2.tobytes()
                m1, n1 = _run(hip, "rank", xd, vd, size, "median", border, 0.0)
                m2, n2 = _run(hip, "rank", xd, vd, size, "median", border, 0.0)
                assert m1.tobytes() == m2.tobytes() and n1.tobytes() == n2.tobytes()      # the same call twice: the same bytes


def test_public_functions(hip):
    from hip_ext import filters
    x = make_map((1, 21, 37), np.float32, 15)[0]
    v = make_valid("random", (1, 21, 37), 15)[0]
    for fn, rank in ((filters.median_filter, "median"), (filters.minimum_filter, "min"), (filters.maximum_filter, "max")):
        want, n = F.rank_filter(x, 5, rank, "mirror", valid=v)
        out, cnt = fn(x, 5, valid=v, return_count=True)      # numpy in, [h, w] in -> [h, w] out, the defaults: 'mirror', NaN fill
        assert out.shape == (21, 37) and out.is_cuda and out.dtype == torch.float32 and cnt.dtype == torch.int32
        _assert_same(out.cpu().numpy(), cnt.cpu().numpy(), want, n, float("nan"), rank)
        assert not isinstance(fn(x, 5), tuple)
    xd, vb = torch.from_numpy(x).cuda(), torch.from_numpy(v > 0).cuda()      # device tensors, a bool validity map, a [B, h, w] batch of crops
    want, n = F.rank_filter(x[:, 3:30], (3, 7), 30, "ignore", valid=v[:, 3:30], fill=-1.0)
    out, cnt = filters.rank_filter(xd[:, 3:30][None], (3, 7), 30, "ignore", valid=vb[:, 3:30][None], fill=-1.0, return_count=True)
    assert out.shape == (1, 21, 27)
    _assert_same(out[0].cpu().numpy(), cnt[0].cpu().numpy(), want, n, -1.0, "crop")
    xu = make_map((2, 9, 11), np.uint8, 16)
    assert np.array_equal(filters.median_filter(xu, 3).cpu().numpy(), np.stack([ndi.median_filter(m, size=3, mode="mirror") for m in xu]))
    assert np.array_equal(filters.median_filter(xu, 3, border="nearest").cpu().numpy(), np.stack([ndi.median_filter(m, size=3, mode="nearest") for m in xu]))
    none_vote = filters.median_filter(xu, 3, valid=np.zeros_like(xu))
    assert none_vote.dtype == torch.uint8 and not none_vote.any()      # the uint8 default fill


def test_launches_are_legal_inside_a_stream_capture(hip):
    x = _dev(make_map((2, 19, 70), np.float32, 17))
    out_m, out_e = torch.empty_like(x), torch.empty_like(x)
    ws = torch.empty(hip.extreme_filter_workspace_bytes(*x.shape), dtype=torch.uint8, device="cuda")
    want_m, _ = _run(hip, "rank", x, None, 5, "median", "mirror", 0.0)
    want_e, _ = _run(hip, "extreme", x, None, 31, "max", "nearest", 0.0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):      # a launch that read anything back would fail the capture
        hip.rank_filter_fwd(x, 5, 5, hip.RANK_MEDIAN, hip.BORDER_MIRROR, out_m)
        hip.extreme_filter_fwd(x, 31, 31, hip.RANK_MAX, hip.BORDER_NEAREST, out_e, workspace=ws)
    g.replay()
    torch.cuda.synchronize()
    assert out_m.cpu().numpy().tobytes() == want_m.tobytes() and out_e.cpu().numpy().tobytes() == want_e.tobytes()


def test_refusals(hip):
    from hip_ext import filters, masks
    x = torch.zeros(8, 8)
    with pytest.raises(hip.HipExtError, match="not a HIP device"):
        filters.median_filter(x, 3)
    with pytest.raises(hip.HipExtError):
        masks.erode(torch.zeros(8, 8, dtype=torch.uint8), 3)
    for bad in (np.zeros((8, 8), np.float64), torch.zeros(8, 8, dtype=torch.float16, device="cuda"), np.zeros((8, 8), np.int32)):
        with pytest.raises(hip.HipExtError, match="expected float32 or uint8"):
            filters.median_filter(bad, 3)
    with pytest.raises(hip.HipExtError, match="valid"):
        filters.median_filter(np.zeros((8, 8), np.float32), 3, valid=np.ones((8, 8), np.float32))
    # the C entry points refuse an out-of-limit window themselves, before any launch: the output keeps its bytes
    xd = torch.ones(1, 8, 8, device="cuda")
    out = torch.full_like(xd, 5.0)
    ws = torch.empty(hip.extreme_filter_workspace_bytes(1, 8, 8), dtype=torch.uint8, device="cuda")
    lib, s = hip.load(), torch.cuda.current_stream().cuda_stream
    common = (xd.data_ptr(), None, hip.DT_F32, 1, 8, 8)
    for kh, kw, rank in ((9, 11, hip.RANK_MEDIAN), (1, 83, 50), (2, 3, hip.RANK_MEDIAN), (3, 3, 104)):
        assert lib.ada_rank_filter_fwd(*common, kh, kw, rank, hip.BORDER_MIRROR, 0.0, out.data_ptr(), None, s) == hip.EINVAL
    for kh, kw, rank in ((65, 3, hip.RANK_MIN), (3, 65, hip.RANK_MAX), (3, 3, hip.RANK_MEDIAN), (4, 3, hip.RANK_MIN)):
        assert lib.ada_extreme_filter_fwd(*common, kh, kw, rank, hip.BORDER_IGNORE, 0.0, out.data_ptr(), None, ws.data_ptr(), ws.numel(), s) == hip.EINVAL
    assert lib.ada_extreme_filter_fwd(*common, 3, 3, hip.RANK_MIN, hip.BORDER_IGNORE, 0.0, out.data_ptr(), None, ws.data_ptr(), ws.numel() - 1, s) == hip.EINVAL
    assert lib.ada_rank_filter_fwd(*common, 3, 3, hip.RANK_MEDIAN, 3, 0.0, out.data_ptr(), None, s) == hip.EINVAL
    assert b"window" in lib.ada_last_error() or b"border" in lib.ada_last_error()
    torch.cuda.synchronize()
    assert (out == 5.0).all()
    with pytest.raises(hip.HipExtError, match="ada_rank_filter_fwd"):
        hip.rank_filter_fwd(xd, 9, 11, hip.RANK_MEDIAN, hip.BORDER_MIRROR, out)


# --- morphology -------------------------------------------------------------------------------------------------------------------------------

def _scipy_morph(m, size, it):
    ones = np.ones((size, size), bool)
    er = ndi.binary_erosion(m, structure=ones, border_value=1, iterations=it)
    di = ndi.binary_dilation(m, structure=ones, border_value=0, iterations=it)
    return dict(erode=er, dilate=di, opening=ndi.binary_dilation(er, structure=ones, border_value=0, iterations=it),
                closing=ndi.binary_erosion(di, structure=ones, border_value=1, iterations=it))


@pytest.mark.parametrize("size", [3, 5])
@pytest.mark.parametrize("iterations", [1, 2])
def test_morphology_is_scipys_explicit_composition(hip, size, iterations):
    from hip_ext import masks
    rng = np.random.default_rng(21)
    cases = [(rng.random((37, 70)) < d).astype(np.uint8) * 255 for d in (0.1, 0.5, 0.9)] + [np.ones((1, 1), np.uint8), np.zeros((1, 1), np.uint8)]
    for m in cases:
        want = _scipy_morph(m > 0, size, iterations)
        for name in ("erode", "dilate", "opening", "closing"):
            got = getattr(masks, name)(m, size=size, iterations=iterations)
            assert got.dtype == torch.uint8 and got.shape == m.shape and got.is_cuda
            assert np.array_equal(got.cpu().numpy(), want[name].astype(np.uint8)), (name, m.shape, float(m.mean()))
    batch = np.stack(cases[:3])      # [K, h, w], bool, on the device: the same rows
    got = masks.closing(torch.from_numpy(batch > 0).cuda(), size=size, iterations=iterations).cpu().numpy()
    assert np.array_equal(got, np.stack([_scipy_morph(m > 0, size, iterations)["closing"] for m in batch]).astype(np.uint8))
    assert np.array_equal(masks.dilate(cases[0], size=size, iterations=0).cpu().numpy(), (cases[0] > 0).astype(np.uint8))


def test_invisible_mask_is_the_reference_chain(hip):
    from hip_ext import masks
    rng = np.random.default_rng(22)
    yy, xx = np.mgrid[0:60, 0:90]
    whole = ((((yy - 30) / 22.0) ** 2 + ((xx - 45) / 35.0) ** 2 <= 1) & (rng.random((60, 90)) < 0.97)).astype(np.uint8) * 255      # a disc with pinholes
    whole[2:4, 80:83] = 255                                                                                                        # and a speck
    visible = (whole > 0) & (xx < 40) | (rng.random((60, 90)) < 0.02)
    plain = (whole > 0) & ~visible
    assert np.array_equal(masks.invisible_mask(visible, whole).cpu().numpy(), plain.astype(np.uint8))
    for conn in (4, 8):
        kept = C.keep_area(plain.astype(np.uint8), 20, conn) > 0
        assert kept.sum() < plain.sum()
        eroded = ndi.binary_erosion(kept, structure=np.ones((3, 3), bool), border_value=1)
        closed = ndi.binary_erosion(ndi.binary_dilation(eroded, structure=np.ones((5, 5), bool), border_value=0), structure=np.ones((5, 5), bool), border_value=1)
        got = masks.invisible_mask(torch.from_numpy(visible).cuda(), torch.from_numpy(whole).cuda(), min_area=20, erode=3, close=5, connectivity=conn)
        assert np.array_equal(got.cpu().numpy(), closed.astype(np.uint8)), conn
        only_close = ndi.binary_erosion(ndi.binary_dilation(plain, structure=np.ones((3, 3), bool), border_value=0), structure=np.ones((3, 3), bool), border_value=1)
        assert np.array_equal(masks.invisible_mask(visible, whole, close=3, connectivity=conn).cpu().numpy(), only_close.astype(np.uint8))


# --- consumers --------------------------------------------------------------------------------------------------------------------------------

def _same_mesh(a, b):
    assert a.vertex_count == b.vertex_count and a.triangle_count == b.triangle_count
    assert a.points.cpu().numpy().tobytes() == b.points.cpu().numpy().tobytes() and torch.equal(a.triangles, b.triangles)


@pytest.mark.parametrize("max_error", [None, 0.02], ids=["regular", "adaptive"])
def test_depth_to_mesh_median_equals_the_mesh_of_the_map_filtered_on_the_host(hip, max_error):
    from hip_ext import geometry
    h, w = 33, 40
    yy, xx = np.mgrid[0:h, 0:w]
    depth = (2.0 + 0.01 * xx + 0.02 * yy).astype(np.float32)
    depth[16, 20] = 9.0                                # a one-pixel spike inside the mask
    depth[5, 5] = 0.25                                 # and one outside it, which must survive untouched
    mask = ((yy > 8) & (yy < 30) & (xx > 6) & (xx < 36)).astype(np.uint8)
    mask[20, 25] = 0
    ref = F.rank_filter(depth, 3, "median", "nearest", valid=mask)[0]
    host = np.where(mask > 0, ref, depth)
    assert host[16, 20] < 3 and host[5, 5] == np.float32(0.25) and not np.array_equal(host, depth)
    for m in (mask, None):
        hm = host if m is not None else F.rank_filter(depth, 3, "median", "nearest")[0]
        kw = dict(mask=m, max_ratio=1.5, max_error=max_error)
        got = geometry.depth_to_mesh(depth, median=3, **kw)
        _same_mesh(got, geometry.depth_to_mesh(hm, **kw))
        plain = geometry.depth_to_mesh(depth, **kw)
        _same_mesh(geometry.depth_to_mesh(depth, median=None, **kw), plain)
        assert got.points.cpu().numpy().tobytes() != plain.points.cpu().numpy().tobytes() or got.triangle_count != plain.triangle_count
    on_dev = geometry.depth_to_mesh(torch.from_numpy(depth).cuda(), mask=torch.from_numpy(mask > 0).cuda(), median=(3, 3), max_ratio=1.5, max_error=max_error)
    _same_mesh(on_dev, geometry.depth_to_mesh(host, mask=mask, max_ratio=1.5, max_error=max_error))


RAW_CASE = dict(kind="raw", encoder="vits", features=64, out_channels=[48, 96, 192, 384])
AM_CASE = dict(kind="amodal", encoder="vits", guide_type="mask+observation", loss="entire_target_object")
FIELDS = ("base", "amodal", "blended", "masks", "scale_shift")
S = 126


@pytest.fixture(scope="module")
def models(hip):
    from _cases import build_product_model, synth_state_dict
    raw = build_product_model(RAW_CASE)
    raw.load_state_dict(synth_state_dict(raw), strict=True)
    am = build_product_model(AM_CASE)
    am.load_state_dict(synth_state_dict(am), strict=True)
    return raw.cuda(), am.cuda()


def _same_result(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f


def test_amodal_infer_image_close(hip, models):
    from hip_ext.pipeline import amodal_infer_image
    from hip_ext.geometry import amodal_layers
    raw, am = models
    h, w = 90, 120
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.ascontiguousarray(np.clip(128 + 100 * np.sin(yy[..., None] * 0.07 + xx[..., None] * np.array([0.05, 0.11, 0.02])) + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8))
    masks = np.zeros((2, h, w), np.uint8)
    masks[0] = ((((yy - 40) / 25.0) ** 2 + ((xx - 70) / 30.0) ** 2 <= 1) & (rng.random((h, w)) < 0.95)) * 255      # pinholes
    masks[1, :35, 80:] = 255
    masks[1, :35, 100] = 0                                                                                        # a hairline gap
    closed = np.stack([F.closing(m, 3) for m in masks])
    assert closed.sum() > (masks > 0).sum() and closed[1, :35, 100].all()
    for kw in (dict(), dict(out_size="image")):
        plain = amodal_infer_image(raw, am, img, masks, size=S, **kw)
        _same_result(plain, amodal_infer_image(raw, am, img, masks, size=S, close=None, **kw))
        got = amodal_infer_image(raw, am, img, masks, size=S, close=3, **kw)
        _same_result(got, amodal_infer_image(raw, am, img, closed, size=S, **kw))
        assert not torch.equal(plain.masks, got.masks)
    # min_area runs before close, and the layers' median is depth_to_mesh's
    specked = masks.copy()
    specked[0, 2, 3] = 255
    cleaned = np.stack([F.closing(C.keep_area(m, 5, 4), 3) for m in specked])
    _same_result(amodal_infer_image(raw, am, img, specked, size=S, min_area=5, close=3), amodal_infer_image(raw, am, img, cleaned, size=S))
    layers, filtered = amodal_layers(got), amodal_layers(got, median=3)
    _same_mesh(amodal_layers(got, median=None).objects[0], layers.objects[0])
    assert filtered.scene.triangle_count == layers.scene.triangle_count and not torch.equal(filtered.scene.points, layers.scene.points)
