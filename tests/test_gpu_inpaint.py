"""GPU: hole filling on the device (csrc/ada_inpaint.hip, hip_ext/inpaint.py) against the numpy restatement of its contract (tests/_inpaint_ref.py),
under np.array_equal everywhere -- indices and squared distances as integers, every float compared as its int32 bits -- and what is built on it:
hip_ext.geometry.fill_view / remove_objects and ``depth_to_view --fill_holes``.

Shapes sit one under, on and one over the constants of the kernels: the 256 columns of a workgroup, the INPAINT_CHUNK columns of the row pass's LDS
stage, the halvings of the pyramid (odd and even sides, one pixel high / wide).  Masks differ per image of a batch.  Values are quarter-integers in a
range of nine, so ties and exact sums dominate; NaN and +-inf are planted only under invalid pixels, where they must change nothing."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import _inpaint_ref as R
import hip_ext as HIP
from test_inpaint_cpu import check_index_properties

pytestmark = pytest.mark.gpu

F = np.float32
CHUNK = HIP.INPAINT_CHUNK
SHAPES = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (1, 2, 3), (1, 5, 5), (2, 33, 65), (3, 9, 70), (1, 3, CHUNK + 6), (1, 130, 5)]
EDGES = [(1, 2, 255), (1, 2, 256), (1, 2, 257), (1, 2, CHUNK - 1), (1, 2, CHUNK), (1, 2, CHUNK + 1)]      # a workgroup's columns, the row pass's LDS stage
KINDS = ["random", "single", "none", "all", "checker", "ring", "disc", "pair"]


def one_mask(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "random":
        return (rng.random((h, w)) < 0.6).astype(np.uint8) * 3      # any non-zero value counts
    if kind == "single":
        v = np.zeros((h, w), np.uint8)
        v[rng.integers(h), rng.integers(w)] = 255
        return v
    if kind == "none":
        return np.zeros((h, w), np.uint8)
    if kind == "all":
        return np.ones((h, w), np.uint8)
    if kind == "checker":
        return ((yy + xx + seed) % 2).astype(np.uint8)
    if kind == "ring":      # valid only on the border
        return ((yy == 0) | (yy == h - 1) | (xx == 0) | (xx == w - 1)).astype(np.uint8)
    if kind == "disc":      # a centred disc of invalid pixels
        r = max(min(h, w) / 3.0, 0.75)
        return (((yy - (h - 1) / 2.0) ** 2 + (xx - (w - 1) / 2.0) ** 2) > r * r).astype(np.uint8)
    assert kind == "pair"      # two valid pixels symmetric about the centre: ties along the whole bisector
    v = np.zeros((h, w), np.uint8)
    r, c = h // 4, w // 5
    v[r, c] = v[h - 1 - r, w - 1 - c] = 1
    return v


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """(valid [B, h, w], x fp32 [B, 3, h, w] with NaN / inf under holes, clean x, bytes [B, 3, h, w]): image b takes the kind b places on in KINDS."""
    B, h, w = shape
    k0 = KINDS.index(kind)
    seed = (B * 131 + h) * 1031 + w + k0
    valid = np.stack([one_mask(KINDS[(k0 + b) % len(KINDS)], h, w, seed + b) for b in range(B)])
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 9, (B, 3, h, w))
    clean = (q / 4.0 - 1.0).astype(F)
    clean[:, :, 0, 0] = -0.0      # compared as bits wherever (0, 0) is valid
    x = clean.copy()
    for b in range(B):
        holes = np.flatnonzero(valid[b].reshape(-1) == 0)
        for c in range(3):
            for p, bad in zip(rng.permutation(holes)[:3], (np.nan, np.inf, -np.inf)):
                x[b, c].reshape(-1)[p] = bad
    for a in (valid, x, clean):
        a.setflags(write=False)
    u8 = (q * 31).astype(np.uint8)
    u8.setflags(write=False)
    return valid, x, clean, u8


@functools.lru_cache(maxsize=None)
def nearest_ref(shape, kind):
    return R.nearest_valid_ref(case(shape, kind)[0])


@functools.lru_cache(maxsize=None)
def smooth_ref(shape, kind):
    valid, _, clean, _ = case(shape, kind)
    return R.push_pull_ref(clean, valid, empty=-2.5)


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()      # a copy: the cached cases are read-only


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


CASES = [(s, k) for s in SHAPES for k in KINDS] + [(s, k) for s in EDGES for k in ("random", "pair")]


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_nearest_valid_equals_brute_force(hip, shape, kind):
    from hip_ext import inpaint
    valid = case(shape, kind)[0]
    want_i, want_d = nearest_ref(shape, kind)
    index, dist = inpaint.nearest_valid(dev(valid), return_distance=True)
    assert index.dtype == torch.int32 and dist.dtype == torch.float64 and tuple(index.shape) == shape
    assert np.array_equal(host(index), want_i)
    with np.errstate(invalid="ignore"):
        want_dist = np.where(want_i >= 0, np.sqrt(want_d.astype(np.float64)), np.inf)
    assert np.array_equal(host(dist), want_dist)
    for b in range(shape[0]):
        if valid[b].any():
            assert np.array_equal(host(dist[b]), ndimage.distance_transform_edt(valid[b] == 0))
    d2 = torch.empty(shape, dtype=torch.int32, device="cuda")
    i2 = torch.empty(shape, dtype=torch.int32, device="cuda")
    hip.nearest_valid_fwd(dev((valid != 0).astype(np.uint8)), i2, d2)
    assert np.array_equal(host(d2), want_d) and np.array_equal(host(i2), want_i)


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_fill_nearest_equals_restatement(hip, shape, kind):
    from hip_ext import inpaint
    valid, x, _, u8 = case(shape, kind)
    got = host(inpaint.fill_nearest(dev(x), dev(valid), empty=-2.5))
    want = R.fill_nearest_ref(x, valid, empty=-2.5)
    assert got.dtype == F and np.array_equal(bits(got), bits(want))
    keep = np.broadcast_to(valid[:, None] != 0, x.shape)
    assert np.array_equal(bits(got)[keep], bits(x)[keep])      # -0.0 stays -0.0
    got8 = host(inpaint.fill_nearest(dev(u8), dev(valid), empty=7))
    assert got8.dtype == np.uint8 and np.array_equal(got8, R.fill_nearest_ref(u8, valid, empty=7))
    one = host(inpaint.fill_nearest(dev(x[:, 0]), dev(valid), empty=-2.5))      # [B, h, w]
    assert np.array_equal(bits(one), bits(want[:, 0]))


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_fill_smooth_equals_restatement_bit_for_bit(hip, shape, kind):
    from hip_ext import inpaint
    valid, x, clean, u8 = case(shape, kind)
    want = smooth_ref(shape, kind)
    got3 = host(inpaint.fill_smooth(dev(x), dev(valid), empty=-2.5))      # C = 3, NaN / inf under the holes
    assert got3.dtype == F and np.array_equal(bits(got3), bits(want))
    got1 = host(inpaint.fill_smooth(dev(x[:, 1]), dev(valid), empty=-2.5))      # C = 1 as [B, h, w]
    assert np.array_equal(bits(got1), bits(want[:, 1]))
    keep = np.broadcast_to(valid[:, None] != 0, x.shape)
    assert np.array_equal(bits(got3)[keep], bits(clean)[keep])
    got8 = host(inpaint.fill_smooth(dev(u8), dev(valid), empty=9))
    assert got8.dtype == np.uint8 and np.array_equal(got8, R.fill_smooth_u8_ref(u8, valid, empty=9))


def test_nearest_valid_on_a_larger_map_against_scipy(hip):
    from hip_ext import inpaint
    h, w = 130, 257
    valid = (np.random.default_rng(130257).random((1, h, w)) < 0.02).astype(np.uint8)
    index = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
    dist2 = torch.empty_like(index)
    hip.nearest_valid_fwd(dev(valid), index, dist2)
    index, dist2 = host(index)[0], host(dist2)[0]
    assert np.array_equal(dist2.astype(np.int64), np.rint(ndimage.distance_transform_edt(valid[0] == 0) ** 2).astype(np.int64))
    check_index_properties(valid[0], index, dist2)
    _, dist = inpaint.nearest_valid(valid[0], return_distance=True)      # numpy in, [h, w] in -> [h, w] out
    assert tuple(dist.shape) == (h, w) and np.array_equal(host(dist), ndimage.distance_transform_edt(valid[0] == 0))


def test_input_forms_images_and_numpy(hip):
    from hip_ext import inpaint
    shape, kind = (2, 33, 65), "random"
    valid, x, clean, u8 = case(shape, kind)
    img = np.ascontiguousarray(u8.transpose(0, 2, 3, 1))      # [B, h, w, 3]
    for fn, ref in ((inpaint.fill_smooth, R.fill_smooth_u8_ref(u8, valid)), (inpaint.fill_nearest, R.fill_nearest_ref(u8, valid))):
        got = fn(img, valid)      # numpy in: copied to the current device
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(host(got), ref.transpose(0, 2, 3, 1))
        one = fn(dev(img[1]), dev(valid[1]).bool())      # [h, w, 3] with a bool mask
        assert tuple(one.shape) == img[1].shape and np.array_equal(host(one), ref[1].transpose(1, 2, 0))
    got = inpaint.fill_smooth(x[0, 0], valid[0], empty=-2.5)      # [h, w] in, [h, w] out
    assert tuple(got.shape) == shape[1:] and np.array_equal(bits(host(got)), bits(smooth_ref(shape, kind)[0, 0]))
    idx = inpaint.nearest_valid(valid[1])
    assert tuple(idx.shape) == shape[1:] and np.array_equal(host(idx), nearest_ref(shape, kind)[0][1])
    with pytest.raises(hip.HipExtError, match="HIP device"):
        inpaint.fill_smooth(torch.from_numpy(clean.copy()), dev(valid))


def test_a_pitched_crop_gives_what_its_copy_gives(hip):
    """The kernels take no pitch: the wrapper packs a crop itself, and the caller's tensor is neither required to be packed nor written."""
    from hip_ext import inpaint
    shape, kind = (2, 33, 65), "random"
    valid, x, _, _ = case(shape, kind)
    big_v = torch.full((2, 40, 80), 1, dtype=torch.uint8, device="cuda")
    big_x = torch.full((2, 3, 40, 80), 99.0, dtype=torch.float32, device="cuda")
    big_v[:, 3:36, 5:70] = dev(valid)
    big_x[:, :, 3:36, 5:70] = dev(x)
    crop_v, crop_x = big_v[:, 3:36, 5:70], big_x[:, :, 3:36, 5:70]
    assert not crop_v.is_contiguous() and not crop_x.is_contiguous()
    before = big_v.clone()
    idx, dist = inpaint.nearest_valid(crop_v, return_distance=True)
    idx_c, dist_c = inpaint.nearest_valid(crop_v.contiguous(), return_distance=True)
    assert torch.equal(idx, idx_c) and torch.equal(dist, dist_c) and np.array_equal(host(idx), nearest_ref(shape, kind)[0])
    for fn in (inpaint.fill_nearest, inpaint.fill_smooth):
        a, b = fn(crop_x, crop_v, empty=-2.5), fn(crop_x.contiguous(), crop_v.contiguous(), empty=-2.5)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert np.array_equal(bits(host(inpaint.fill_smooth(crop_x, crop_v, empty=-2.5))), bits(smooth_ref(shape, kind)))
    assert torch.equal(big_v, before)


# ---- the workspace contract, in the manner of test_gpu_workspace_contract.py -------------------------------------------------------------------

G = 4096
GUARD, POISON = 0x5A, 0xA5


def guarded(need, fill):
    """``need`` bytes filled with ``fill`` between two bands of G guard bytes; check() asserts the bands untouched."""
    buf = torch.full((G + need + G,), GUARD, dtype=torch.uint8, device="cuda")
    ws = buf[G:G + need]
    ws.fill_(fill)

    def check(what):
        torch.cuda.synchronize()
        assert bool((buf[:G] == GUARD).all()) and bool((buf[G + need:] == GUARD).all()), f"{what}: guard bytes around the {need}-byte workspace overwritten"
    return ws, check


def poisoned(shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), POISON, dtype=torch.uint8, device="cuda").view(dtype).view(*shape)


def states(hip, what, need, call, busier):
    """call(ws) on exactly ``need`` bytes pre-filled with 0x00, with 0xFF and with what ``busier(ws)`` left: byte-identical outputs, intact guards, and a
    workspace one byte short refused.  Returns the first run's outputs."""
    runs = []
    for state in ("0x00", "0xff", "used"):
        ws, check = guarded(need, 0xFF if state == "0xff" else 0x00)
        if state == "used":
            busier(ws)
        outs = call(ws)
        check(f"{what}: workspace pre-filled {state}")
        runs.append([o.clone() for o in outs])
    for outs in runs[1:]:
        for a, b in zip(runs[0], outs):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{what}: the result depends on what the workspace held"
    short, check = guarded(need - 1, 0x00)
    with pytest.raises(hip.HipExtError, match="workspace"):
        call(short)
    check(f"{what}: the refused call")
    return runs[0]


@pytest.mark.parametrize("shape", [(2, 33, 65), (1, 3, CHUNK + 6), (1, 130, 5), (1, 1, 7)], ids=str)
def test_workspace_contract(hip, shape):
    B, h, w = shape
    valid, x, _, _ = case(shape, "random")
    dv, dx = dev((valid != 0).astype(np.uint8)), dev(x)
    full, other = torch.ones_like(dv), dev(np.full(x.shape, 1e30, F))      # the busier call: every pixel valid, other values at every level
    need = hip.nearest_valid_workspace_bytes(B, h, w)
    assert need == 4 * B * h * w

    def nearest(ws, v=dv):
        index, dist2 = poisoned(shape, torch.int32), poisoned(shape, torch.int32)
        hip.nearest_valid_fwd(v, index, dist2, workspace=ws)
        return index, dist2
    index, dist2 = states(hip, f"nearest_valid_fwd {shape}", need, nearest, lambda ws: nearest(ws, full))
    want_i, want_d = nearest_ref(shape, "random")
    assert np.array_equal(host(index), want_i) and np.array_equal(host(dist2), want_d)

    for C in (1, 3):
        need = hip.push_pull_workspace_bytes(B, C, h, w)
        px, hh, ww = 0, h, w
        while (hh, ww) != (1, 1):
            hh, ww = (hh + 1) // 2, (ww + 1) // 2
            px += hh * ww
        assert need == B * px * (4 * C + 1) > 0
        xs = dx[:, :C].contiguous()

        def smooth(ws, v=dv, data=xs):
            out = poisoned(data.shape, torch.float32)
            hip.push_pull(data, v, out, empty=-2.5, workspace=ws)
            return (out,)
        out, = states(hip, f"push_pull {shape} C={C}", need, smooth, lambda ws: smooth(ws, full, other[:, :C].contiguous()))
        assert np.array_equal(bits(host(out)), bits(smooth_ref(shape, "random")[:, :C]))

    out = poisoned(x.shape, torch.float32)      # the gather takes no workspace: every element of out is written
    hip.fill_gather(dx, dv, index, out, empty=-2.5)
    assert np.array_equal(bits(host(out)), bits(R.fill_nearest_ref(x, valid, empty=-2.5)))


def test_a_one_pixel_image_needs_no_workspace(hip):
    assert hip.push_pull_workspace_bytes(3, 2, 1, 1) == 0
    x = dev(np.array([1.5, -0.0, 3.0, 4.0, np.nan, np.inf], F).reshape(3, 2, 1, 1))
    v = dev(np.array([1, 1, 0], np.uint8).reshape(3, 1, 1))
    out = poisoned((3, 2, 1, 1), torch.float32)
    hip.push_pull(x, v, out, empty=-2.5)
    assert np.array_equal(bits(host(out)).reshape(-1), bits(np.array([1.5, -0.0, 3.0, 4.0, -2.5, -2.5], F)))


def test_fills_inside_a_stream_capture(hip):
    from hip_ext import inpaint
    shape = (2, 33, 65)
    valid, x, _, _ = case(shape, "random")
    dv, dx = dev(valid), dev(x)
    run = lambda: (inpaint.fill_smooth(dx, dv, empty=-2.5), inpaint.fill_nearest(dx, dv, empty=-2.5))      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        smooth, nearest = run()
    dv.copy_(dev(case(shape, "disc")[0]))
    graph.replay()
    torch.cuda.synchronize()
    dv.copy_(dev(valid))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(smooth)), bits(smooth_ref(shape, "random")))
    assert np.array_equal(bits(host(nearest)), bits(R.fill_nearest_ref(x, valid, empty=-2.5)))


# ---- what is built on the fills ----------------------------------------------------------------------------------------------------------------

def ramp_view(geometry, with_color=True):
    """A 24 x 32 ramp with a rectangle masked out, meshed and rendered from the default pose: the rectangle's interior is a hole of the view."""
    h, w = 24, 32
    yy, xx = np.mgrid[0:h, 0:w]
    depth = (2.0 + 0.05 * xx + 0.02 * yy).astype(F)
    mask = np.ones((h, w), np.uint8)
    mask[6:15, 9:22] = 0
    photo = np.random.default_rng(2432).integers(0, 256, (h, w, 3), dtype=np.uint8)
    mesh = geometry.depth_to_mesh(depth, mask=mask, colors=photo if with_color else None)
    return geometry.render_mesh(mesh, h, w, out="w"), depth


@pytest.mark.parametrize("method", ["smooth", "nearest"])
def test_fill_view(hip, method):
    from hip_ext import geometry, inpaint
    view, _ = ramp_view(geometry)
    hole = host(view.owner) < 0
    assert 50 < hole.sum() < hole.size // 2 and view.color is not None
    filled = geometry.fill_view(view, method=method)
    assert isinstance(filled, geometry.View) and filled.index is view.index and filled.owner is view.owner
    fill = inpaint.fill_smooth if method == "smooth" else inpaint.fill_nearest
    valid = view.owner >= 0
    assert np.array_equal(bits(host(filled.depth)), bits(host(fill(view.depth, valid))))
    assert np.array_equal(host(filled.color), host(fill(view.color, valid)))
    assert np.array_equal(bits(host(filled.depth))[~hole], bits(host(view.depth))[~hole]) and np.array_equal(host(filled.color)[~hole], host(view.color)[~hole])
    want = (R.push_pull_ref if method == "smooth" else R.fill_nearest_ref)(host(view.depth), (~hole).astype(np.uint8))
    assert np.array_equal(bits(host(filled.depth)), bits(want))
    assert (host(filled.depth)[hole] > 0).all()      # no hole keeps the background's 0
    plain, _ = ramp_view(geometry, with_color=False)
    assert geometry.fill_view(plain, method=method).color is None


def test_fill_view_leaves_an_empty_view_unchanged(hip):
    from hip_ext import geometry
    depth = np.full((24, 32), 3.0, F)
    mesh = geometry.depth_to_mesh(depth, mask=np.zeros((24, 32), np.uint8), colors=np.full((24, 32, 3), 200, np.uint8))
    assert mesh.triangle_count == 0
    view = geometry.render_meshes([mesh], 24, 32, fill=9.0, fill_color=(1, 2, 3))
    assert bool((view.owner < 0).all())
    for method in ("smooth", "nearest"):
        got = geometry.fill_view(view, method=method)
        assert np.array_equal(bits(host(got.depth)), bits(host(view.depth))) and np.array_equal(host(got.color), host(view.color))
        assert torch.equal(got.index, view.index) and torch.equal(got.owner, view.owner)


def test_remove_objects(hip):
    from hip_ext import geometry, inpaint
    h, w = 40, 48
    rng = np.random.default_rng(4048)
    depth = (rng.integers(0, 9, (h, w)) / 4.0 + 1.0).astype(F)
    image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    masks = np.zeros((2, h, w), np.uint8)
    masks[0, 5:14, 7:20] = 255
    masks[1, 20:33, 30:48] = 1      # touches the border
    grown = ndimage.binary_dilation(masks.any(axis=0), structure=np.ones((3, 3)))
    valid = (~grown).astype(np.uint8)
    for method, fill, ref in (("smooth", inpaint.fill_smooth, R.push_pull_ref), ("nearest", inpaint.fill_nearest, R.fill_nearest_ref)):
        d, img = geometry.remove_objects(depth, masks, image=image, grow=1, method=method)
        assert tuple(d.shape) == (h, w) and tuple(img.shape) == (h, w, 3) and img.dtype == torch.uint8
        assert np.array_equal(bits(host(d)), bits(host(fill(depth, valid)))) and np.array_equal(bits(host(d)), bits(ref(depth, valid)))
        assert np.array_equal(host(img), host(fill(image, valid)))
        assert np.array_equal(bits(host(d))[~grown], bits(depth)[~grown]) and np.array_equal(host(img)[~grown], image[~grown])
    d0, none = geometry.remove_objects(dev(depth), dev(masks[0]).bool(), grow=0)      # one mask [h, w], no dilation, no photo
    assert none is None and np.array_equal(bits(host(d0)), bits(R.push_pull_ref(depth, (masks[0] == 0).astype(np.uint8))))
    d2, _ = geometry.remove_objects(depth, masks, grow=2)
    grown2 = ndimage.binary_dilation(masks.any(axis=0), structure=np.ones((3, 3)), iterations=2)
    assert np.array_equal(bits(host(d2)), bits(R.push_pull_ref(depth, (~grown2).astype(np.uint8))))


def test_depth_to_view_fill_holes(hip, tmp_path):
    from PIL import Image
    from hip_ext import geometry
    from hip_ext import image as hip_image
    from src.scripts import depth_to_view as S
    h, w = 24, 32
    rng = np.random.default_rng(2432)
    depth16 = (np.where(np.arange(w)[None, :] < w // 2, 2000, 6000) + rng.integers(-50, 50, (h, w))).astype(np.uint16)
    Image.fromarray(depth16).save(tmp_path / "d.png")
    args = [str(tmp_path / "d.png"), "--max_ratio", "2", "--yaw", "12"]
    assert S.main(args[:1] + [str(tmp_path / "plain.png")] + args[1:]) == 0
    assert S.main(args[:1] + [str(tmp_path / "filled.png")] + args[1:] + ["--fill_holes", "smooth"]) == 0
    assert S.main(args[:1] + [str(tmp_path / "near.png")] + args[1:] + ["--fill_holes", "nearest"]) == 0
    plain, filled, near = (np.asarray(Image.open(tmp_path / f"{n}.png")) for n in ("plain", "filled", "near"))
    # the plain run is what it was before the option existed: the same call composed from render_mesh and colorize
    depth = depth16.astype(F)
    mesh = geometry.depth_to_mesh(depth, max_ratio=2.0)
    Rm, t = geometry.look_at_pose(12.0, 0.0, (0.0, 0.0, 0.0), pivot_z=S.pivot_depth(depth))
    view = geometry.render_mesh(mesh, h, w, R=Rm, t=t, out="w", fill=S.INVALID)
    want = host(hip_image.colorize(view.depth, invalid_val=S.INVALID)[0, :, :, :3])
    assert plain.dtype == np.uint8 and np.array_equal(plain, want)
    hole = host(view.owner) < 0
    background = (plain == 128).all(axis=2)
    assert hole.sum() > 10 and background[hole].all()
    for pic, method in ((filled, "smooth"), (near, "nearest")):
        assert pic.shape == plain.shape and not (pic == 128).all(axis=2)[hole].any()
        want = host(hip_image.colorize(geometry.fill_view(view, method).depth, invalid_val=S.INVALID)[0, :, :, :3])
        assert np.array_equal(pic, want)
    # with a photo the holes take the photo's colours
    photo = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    Image.fromarray(photo).save(tmp_path / "p.png")
    assert S.main(args[:1] + [str(tmp_path / "c.png")] + args[1:] + ["--image", str(tmp_path / "p.png"), "--fill_holes", "nearest"]) == 0
    mesh = geometry.depth_to_mesh(depth, colors=photo, max_ratio=2.0)
    view = geometry.render_mesh(mesh, h, w, R=Rm, t=t, out="w", fill=S.INVALID)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "c.png")), host(geometry.fill_view(view, "nearest").color))
