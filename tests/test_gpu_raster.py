"""GPU: the rasteriser (csrc/ada_raster.hip through hip_ext.geometry.render_mesh / render_meshes / render_layers) against the numpy restatement of its
contract, tests/_raster_ref.py, which test_raster_cpu.py pins to hand-derived cases and to matplotlib.tri.  Every comparison is zero tolerance: index
equal, depth equal bit for bit, color and owner equal.  Never one device path against another.  No case feeds a triangle index outside [0, V) to the
device: that rule is checked in the restatement only."""
import functools
import types

import numpy as np
import pytest
import torch

import _geometry_ref as G_REF
import _raster_ref as R

pytestmark = pytest.mark.gpu

UNIT_K = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def points_of(uvz):
    """Vertices given as (u, v, z) in pixels -> points that the camera UNIT_K sees there (exactly so when z is a power of two)."""
    uvz = np.asarray(uvz, dtype=np.float64).reshape(-1, 3)
    return np.stack([-uvz[:, 0] * uvz[:, 2], -uvz[:, 1] * uvz[:, 2], uvz[:, 2]], 1)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(view):
    return R.View(*(None if a is None else a.cpu().numpy() for a in view))


def render(points, tri, h, w, colors=None, **kw):
    from hip_ext import geometry as G
    return host(G.render_mesh(dev(points), h, w, triangles=dev(np.asarray(tri, dtype=np.int32).reshape(-1, 3)), colors=dev(colors), **kw))


def assert_same(got, want):
    assert got.index.dtype == np.int32 and got.depth.dtype == np.float32 and got.owner.dtype == np.int32
    assert got.index.shape == want.index.shape and np.array_equal(got.index, want.index)
    assert np.array_equal(got.depth.view(np.int32), want.depth.view(np.int32))
    assert np.array_equal(got.owner, want.owner)
    assert (got.color is None) == (want.color is None)
    if want.color is not None:
        assert got.color.dtype == np.uint8 and np.array_equal(got.color, want.color)


def check(points, tri, h, w, colors=None, **kw):
    got = render(points, tri, h, w, colors, **kw)
    want = R.render(points, np.asarray(tri).reshape(-1, 3), h, w, colors=colors, **kw)
    assert_same(got, want)
    return got


# ------------------------------------------------------------------ the hand-derived cases of test_raster_cpu.py
@pytest.mark.parametrize("winding", [(0, 1, 2), (0, 2, 1)])
def test_one_triangle_on_samples(hip, winding):
    got = check(points_of([(1, 1, 2.0), (6, 1, 2.0), (1, 6, 2.0)]), [winding], 8, 8, K=UNIT_K)
    assert ["".join("#" if v == 0 else "." for v in row) for row in got.index] == [
        "........", ".######.", ".#####..", ".####...", ".###....", ".##.....", ".#......", "........"]
    assert np.all(got.depth[got.index == 0] == np.float32(2.0))


def test_a_shared_edge_goes_to_the_lower_index(hip):
    pts = points_of([(1, 1, 2.0), (5, 1, 2.0), (1, 5, 2.0), (5, 5, 2.0)])
    tri = np.array([[0, 2, 1], [3, 1, 2]])
    a, b = check(pts, tri, 8, 8, K=UNIT_K), check(pts, tri[::-1], 8, 8, K=UNIT_K)
    diagonal = (np.add.outer(np.arange(8), np.arange(8)) == 6) & (a.index >= 0)
    assert diagonal.sum() == 5 and np.all(a.index[diagonal] == 0) and np.all(b.index[diagonal] == 0)
    assert np.array_equal(a.depth.view(np.int32), b.depth.view(np.int32))


def test_snapping_half_to_even(hip):
    from hip_ext import geometry as G  # noqa: F401
    pts = dev(np.array([[-2.498, -(4 + 1 / 512), 1.0], [-(5 + 3 / 512), 0.25, 1.0], [0.0, 0.0, -1.0]]))
    x, y = torch.empty(3, dtype=torch.int32, device="cuda"), torch.empty(3, dtype=torch.int32, device="cuda")
    w = torch.empty(3, dtype=torch.float64, device="cuda")
    hip.mesh_project(pts, [1.0, 1.0, 0.0, 0.0] + list(np.eye(3).reshape(-1)) + [0.0] * 3, x, y, w)
    assert x.tolist() == [639, 1282, 0] and y.tolist() == [1024, -64, 0] and w.tolist() == [1.0, 1.0, 0.0]


# ------------------------------------------------------------------ target shapes, each with a mesh that crosses every border
def crossing_mesh(h, w, seed, n=24):
    rng = np.random.default_rng(seed)
    uvz = np.stack([rng.uniform(-0.4 * w - 2, 1.4 * w + 2, 3 * n), rng.uniform(-0.4 * h - 2, 1.4 * h + 2, 3 * n), np.exp(rng.uniform(np.log(0.5), np.log(20), 3 * n))], 1)
    cover = [(-3.3, -2.1, 30.0), (2.5 * w + 4, -2.7, 25.0), (-3.9, 2.5 * h + 4, 35.0)]      # behind everything, over every border
    pts = points_of(np.concatenate([uvz, cover]))
    tri = np.concatenate([rng.permutation(3 * n).reshape(n, 3), [[3 * n, 3 * n + 1, 3 * n + 2]]])
    colors = rng.integers(0, 256, (3 * n + 3, 3), dtype=np.uint8)
    return pts, tri, colors


@pytest.mark.parametrize("hw", [(1, 1), (1, 9), (9, 1), (70, 50), (5, 257), (3, 600)])
def test_target_shapes(hip, hw):
    h, w = hw
    pts, tri, colors = crossing_mesh(h, w, seed=h * 1000 + w)
    got = check(pts, tri, h, w, colors, K=UNIT_K, out="w")
    assert (got.index >= 0).all() and len(np.unique(got.index)) > (1 if h * w > 1 else 0)


# ------------------------------------------------------------------ 200 random triangles over 48 x 40
@functools.lru_cache(maxsize=None)
def random_case():
    rng = np.random.default_rng(200)
    n = 200
    uvz = np.stack([rng.uniform(-8, 56, 3 * n), rng.uniform(-8, 48, 3 * n), np.exp(rng.uniform(np.log(0.5), np.log(20), 3 * n))], 1)
    pts = points_of(uvz)
    tri = np.arange(3 * n).reshape(n, 3)
    colors = rng.integers(0, 256, (3 * n, 3), dtype=np.uint8)
    want = {out: R.render(pts, tri, 40, 48, colors=colors, K=UNIT_K, out=out, inverse=(0.9, 0.1)) for out in ("z", "w", "normalised")}
    for v in want.values():
        v.depth.setflags(write=False), v.index.setflags(write=False), v.color.setflags(write=False)
    return pts, tri, colors, want


@pytest.mark.parametrize("out", ["z", "w", "normalised"])
def test_random_triangles_in_every_depth_mode(hip, out):
    pts, tri, colors, want = random_case()
    assert pts.dtype == np.float64
    assert_same(render(pts, tri, 40, 48, colors, K=UNIT_K, out=out, inverse=(0.9, 0.1)), want[out])
    assert (want[out].index >= 0).mean() > 0.9


def test_random_triangles_fp32_points_and_no_colours(hip):
    pts, tri, _, _ = random_case()
    p32 = pts.astype(np.float32)
    got = check(p32, tri, 40, 48, K=UNIT_K, fill=-5.0)
    assert got.color is None


def test_reproducible_and_independent_of_the_list_order(hip):
    pts, tri, colors, want = random_case()
    a = render(pts, tri, 40, 48, colors, K=UNIT_K)
    b = render(pts, tri, 40, 48, colors, K=UNIT_K)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    perm = np.random.default_rng(7).permutation(tri.shape[0])
    c = render(pts, tri[perm], 40, 48, colors, K=UNIT_K)
    assert_same(c, R.render(pts, tri[perm], 40, 48, colors=colors, K=UNIT_K))
    assert np.array_equal(c.depth.view(np.int32), a.depth.view(np.int32)) and np.array_equal(c.color, a.color)
    hit = a.index >= 0
    assert np.array_equal(c.index >= 0, hit) and np.array_equal(perm[c.index[hit]], a.index[hit])


# ------------------------------------------------------------------ the small / large split
def box_triangle(j0, i0, nx, ny, z):
    """A right triangle whose box holds exactly the samples j0 .. j0 + nx - 1, i0 .. i0 + ny - 1 (a quarter pixel of margin on each side)."""
    return [(j0 - 0.25, i0 - 0.25, z), (j0 + nx - 0.75, i0 - 0.25, z), (j0 - 0.25, i0 + ny - 0.75, z)]


def factor(n, max_x, max_y):
    for nx in range(min(max_x, n), 0, -1):
        if n % nx == 0 and n // nx <= max_y:
            return nx, n // nx
    raise AssertionError(f"no {n}-sample box fits {max_y} x {max_x}")


def test_boxes_at_both_thresholds(hip):
    h, w = 250, 40
    small, block = hip.RASTER_SMALL_MAX, hip.RASTER_WAVE_MAX
    verts, tri = [], []
    for k, n in enumerate((small - 1, small, small + 1, block - 1, block, block + 1, small, small + 1)):
        nx, ny = factor(n, w - 2, h - 2)
        if k >= 6:      # the same counts reached by clipping at the target's corner: the box is the screen-clipped one
            verts += [(w - nx - 0.25, h - ny - 0.25, 2.0 + k), (w + 40.0, h - ny - 0.25, 2.0 + k), (w - nx - 0.25, h + 60.0, 2.0 + k)]
        else:
            verts += box_triangle(1, 1, nx, ny, 2.0 + k)
        tri.append([3 * k, 3 * k + 1, 3 * k + 2])
    pts = points_of(verts)
    for order in (tri, tri[::-1]):
        got = check(pts, order, h, w, K=UNIT_K)
        assert len(np.unique(got.index)) >= 4
    for k in range(len(tri)):      # and each alone, so that no nearer triangle hides a miss
        got = check(pts, [tri[k]], h, w, K=UNIT_K)
        assert (got.index == 0).sum() > 0


def test_one_and_many_whole_target_triangles(hip):
    cover = lambda h, w, z: [(-1.5, -1.25, z), (2.0 * w + 3, -1.25, z), (-1.5, 2.0 * h + 3, z)]
    h, w = 70, 50
    got = check(points_of(cover(h, w, 4.0)), [[0, 1, 2]], h, w, K=UNIT_K)
    assert (got.index == 0).all()
    tri = [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(64)]
    got = check(points_of(sum((cover(h, w, 70.0 - k) for k in range(64)), [])), tri, h, w, K=UNIT_K)      # distinct depths, the nearest last in the list
    assert (got.index == 63).all()
    h, w = 130, 90      # larger than the one-wave class as well: a few, and more than the walking launch has teams
    assert h * w > hip.RASTER_WAVE_MAX
    for n in (4, hip.RASTER_WALK_BLOCKS // hip.RASTER_WALK_SHARE + 3):
        tri = [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(n)]
        got = check(points_of(sum((cover(h, w, 2.0 * n - k) for k in range(n)), [])), tri, h, w, K=UNIT_K)
        assert (got.index == n - 1).all()


def test_a_mesh_mixing_small_and_large_triangles(hip):
    h, w = 130, 90
    rng = np.random.default_rng(13090)
    gh, gw = 40, 30
    depth = rng.uniform(2.0, 3.0, (gh, gw)).astype(np.float32)
    y, x = np.mgrid[0:gh, 0:gw]
    grid = np.stack([3.0 * x.reshape(-1) + 1.3, 3.2 * y.reshape(-1) + 0.7, depth.reshape(-1).astype(np.float64)], 1)      # boxes of 9 .. 16 samples
    big = [(-5.0, -5.0, 6.0), (200.0, -4.0, 5.0), (-6.0, 300.0, 7.0), (95.0, 140.0, 2.5), (-10.0, 120.0, 2.4), (80.0, -20.0, 2.6),      # two of the large class
           (10.2, 20.1, 1.5), (60.7, 22.3, 1.6), (30.1, 80.9, 1.4), (50.5, 100.5, 1.2), (85.0, 101.0, 1.3), (52.0, 128.0, 1.25)]    # two of the middle class
    pts = points_of(np.concatenate([grid, big]))
    n = gh * gw
    tri = np.concatenate([G_REF.triangles(gh, gw), [[n, n + 1, n + 2], [n + 3, n + 4, n + 5], [n + 6, n + 7, n + 8], [n + 9, n + 10, n + 11]]])
    tri = tri[rng.permutation(tri.shape[0])]
    colors = rng.integers(0, 256, (n + 12, 3), dtype=np.uint8)
    got = check(pts, tri, h, w, colors, K=UNIT_K, out="w")
    assert len(np.unique(got.index)) > 1000


# ------------------------------------------------------------------ depth ties
def test_depth_ties_go_to_the_lowest_id(hip):
    a, b = [(1, 1, 2.0), (9, 1, 2.0), (1, 9, 2.0)], [(3, 0, 2.0), (11, 2, 2.0), (2, 8, 2.0)]      # coplanar (z = 2), overlapping
    for verts in (a + b, b + a):
        got = check(points_of(verts), [[0, 1, 2], [3, 4, 5]], 12, 12, K=UNIT_K)
        both = (R.render(points_of(verts[:3]), [[0, 1, 2]], 12, 12, K=UNIT_K).index == 0) & (R.render(points_of(verts[3:]), [[0, 1, 2]], 12, 12, K=UNIT_K).index == 0)
        assert both.sum() > 5 and np.all(got.index[both] == 0)
    # fp64 w that differ, float32(w) that do not: still the lowest id, also when the other one is nearer in fp64
    near = 2.0 / (1.0 + 2.0 ** -30)
    assert 1.0 / near > 0.5 and np.float32(1.0 / near) == np.float32(0.5)
    b = [(u, v, near) for u, v, _ in b]
    for verts in (a + b, b + a):
        got = check(points_of(verts), [[0, 1, 2], [3, 4, 5]], 12, 12, K=UNIT_K, out="w")
        both = (R.render(points_of(verts[:3]), [[0, 1, 2]], 12, 12, K=UNIT_K).index == 0) & (R.render(points_of(verts[3:]), [[0, 1, 2]], 12, 12, K=UNIT_K).index == 0)
        assert both.sum() > 5 and np.all(got.index[both] == 0)


# ------------------------------------------------------------------ identity round trip through the product
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_identity_view_of_depth_to_mesh_gives_the_map_and_the_colours_back(hip, compact, dtype):
    from hip_ext import geometry as G
    h, w = 37, 61
    rng = np.random.default_rng(3761)
    depth = rng.uniform(0.5, 9.0, size=(h, w)).astype(np.float32)
    colors = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mesh = G.depth_to_mesh(depth, colors=colors, compact=compact, dtype=dtype)
    view = G.render_mesh(mesh, h, w)
    got = host(view)
    assert (got.index >= 0).all() and (got.owner == 0).all()
    ulps = np.abs(got.depth.view(np.int32).astype(np.int64) - depth.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, ulps.max()
    assert np.array_equal(got.color, colors)
    want = R.render(mesh.points.cpu().numpy(), mesh.triangles.cpu().numpy(), h, w, colors=mesh.colors.cpu().numpy())
    assert_same(got, want)


# ------------------------------------------------------------------ a moved camera
def test_a_moved_camera_matches_the_restatement_and_opens_holes_behind_the_step(hip):
    from hip_ext import geometry as G
    h, w = 24, 32
    rng = np.random.default_rng(2432)
    depth = (np.where(np.arange(w)[None, :] < w // 2, 2.0, 6.0) + rng.uniform(-0.05, 0.05, (h, w))).astype(np.float32)
    colors = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mesh = G.depth_to_mesh(depth, colors=colors, max_ratio=2.0, dtype=torch.float64)
    assert mesh.triangle_count == 2 * (h - 1) * (w - 2)
    Rm, t = G.look_at_pose(yaw_deg=12, shift=(0.2, 0, 0), pivot_z=3.0)
    got = host(G.render_mesh(mesh, h, w, R=Rm, t=t))
    want = R.render(mesh.points.cpu().numpy(), mesh.triangles.cpu().numpy(), h, w, colors=mesh.colors.cpu().numpy(), R=Rm, t=t)
    assert_same(got, want)
    assert (got.index[2:-2, 2:-2] < 0).any() and (got.index >= 0).mean() > 0.5
    still = host(G.render_mesh(mesh, h, w))
    assert (still.index[:, : w // 2] >= 0).all() and (still.index[:, w // 2 + 1:] >= 0).all()


# ------------------------------------------------------------------ render_meshes / render_layers
@functools.lru_cache(maxsize=None)
def layers_case():
    from hip_ext import geometry as G
    h, w = 20, 28
    rng = np.random.default_rng(2028)
    base = rng.uniform(0.05, 0.3, (h, w)).astype(np.float32)
    blended = np.stack([rng.uniform(0.5, 0.6, (h, w)), rng.uniform(0.7, 0.8, (h, w)), rng.uniform(0.9, 1.0, (h, w))]).astype(np.float32)
    masks = np.zeros((3, h, w), np.float32)
    masks[0, 3:15, 4:18] = 1.0
    masks[1, 8:18, 12:25] = 1.0      # overlaps object 0 and lies in front of it; object 2's mask is empty
    photo = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    result = types.SimpleNamespace(base=dev(base), blended=dev(blended), masks=dev(masks))
    layers = G.amodal_layers(result, image=photo, near=1.0, far=10.0)
    to_host = lambda m: (m.points.cpu().numpy(), m.triangles.cpu().numpy(), m.colors.cpu().numpy())
    return layers, to_host(layers.scene), [to_host(m) for m in layers.objects], base, masks


def test_render_layers_owner_map_and_hiding_an_object(hip):
    from hip_ext import geometry as G
    layers, scene, objects, base, masks = layers_case()
    h, w = base.shape
    ab = (1.0 - 0.1, 0.1)
    assert layers.objects[2].triangle_count == 0 and layers.objects[2].vertex_count == 0
    full = host(G.render_layers(layers, h, w))
    assert_same(full, R.render_many([scene] + objects, [0, 1, 2, 3], h, w, out="normalised", inverse=ab))
    assert set(np.unique(full.owner)) == {0, 1, 2} and full.color is not None
    # on the identity view each pixel shows the nearest layer that has it, at the value that layer's map holds there (within the two roundings of the mapping)
    assert (full.owner[9:14, 13:17] == 2).all() and (full.owner[4:7, 5:11] == 1).all() and (full.owner[0, :] == 0).all()
    assert np.max(np.abs(full.depth[full.owner == 0] - base[full.owner == 0])) < 1e-6
    hidden = host(G.render_layers(layers, h, w, objects=[0, 2]))
    assert_same(hidden, R.render_many([scene, objects[0], objects[2]], [0, 1, 3], h, w, out="normalised", inverse=ab))
    was_two = full.owner == 2
    assert was_two.any() and set(np.unique(hidden.owner[was_two])) == {0, 1}
    alone = host(G.render_layers(layers, h, w, objects=[1], scene=False, out="z"))
    assert_same(alone, R.render_many([objects[1]], [2], h, w, out="z", inverse=ab))
    assert set(np.unique(alone.owner)) == {-1, 2} and np.isinf(alone.depth[alone.owner < 0]).all()


def test_render_meshes_owner_is_the_position_in_the_list(hip):
    from hip_ext import geometry as G
    layers, scene, objects, base, _ = layers_case()
    h, w = base.shape
    Rm, t = G.look_at_pose(yaw_deg=-9, pitch_deg=4, pivot_z=2.0)
    meshes = [layers.objects[2], layers.objects[1], layers.scene, layers.objects[0]]      # an empty Mesh first
    got = host(G.render_meshes(meshes, h + 5, w + 3, fov_deg=55.0, R=Rm, t=t, out="w"))
    want = R.render_many([objects[2], objects[1], scene, objects[0]], [0, 1, 2, 3], h + 5, w + 3, R=Rm, t=t, out="w")
    assert_same(got, want)
    assert set(np.unique(got.owner)) == {-1, 1, 2, 3}
    empty = host(G.render_meshes([layers.objects[2]], 6, 7, fill=9.0, fill_color=(1, 2, 3)))
    assert (empty.index == -1).all() and (empty.owner == -1).all() and (empty.depth == 9.0).all() and (empty.color == [1, 2, 3]).all()


def test_the_view_feeds_render_depth_unchanged(hip):
    from hip_ext import geometry as G
    from hip_ext import image as I
    layers, _, _, base, _ = layers_case()
    h, w = base.shape
    view = G.render_layers(layers, h, w)
    pic = I.render_depth(view.depth[None])
    assert pic.dtype == torch.uint8 and tuple(pic.shape) == (1, h, w, 3)


# ------------------------------------------------------------------ stream capture
def test_render_mesh_inside_a_stream_capture(hip):
    from hip_ext import geometry as G
    pts0, tri, colors, _ = random_case()
    pts1 = points_of(np.stack([np.random.default_rng(1).uniform(-8, 56, 600), np.random.default_rng(2).uniform(-8, 48, 600),
                               np.random.default_rng(3).uniform(0.5, 20, 600)], 1))
    p, t, c = dev(pts0), dev(tri.astype(np.int32)), dev(colors)
    run = lambda: G.render_mesh(p, 40, 48, triangles=t, colors=c, K=UNIT_K)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        view = run()
    for pts in (pts1, pts0):
        p.copy_(torch.from_numpy(pts))
        graph.replay()
        torch.cuda.synchronize()
        got = host(view)
        assert_same(got, host(run()))
        assert_same(got, R.render(pts, tri, 40, 48, colors=colors, K=UNIT_K))


# ------------------------------------------------------------------ the command line
def test_depth_to_view_writes_the_restated_picture(hip, tmp_path):
    from PIL import Image
    from src.scripts import depth_to_view as S
    h, w = 24, 32
    rng = np.random.default_rng(2432)
    depth = (np.where(np.arange(w)[None, :] < w // 2, 2.0, 6.0) + rng.uniform(-0.05, 0.05, (h, w))).astype(np.float32)
    photo = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    np.save(tmp_path / "d.npy", depth)
    Image.fromarray(photo).save(tmp_path / "p.png")
    assert S.main([str(tmp_path / "d.npy"), str(tmp_path / "view.png"), "--image", str(tmp_path / "p.png"), "--max_ratio", "2", "--yaw", "12",
                   "--shift", "0.2", "0", "0"]) == 0
    mesh = G_REF.depth_to_mesh(depth, colors=photo, max_ratio=2.0, dtype=np.float32)
    Rm, t = R.look_at_pose(yaw_deg=12, shift=(0.2, 0, 0), pivot_z=S.pivot_depth(depth))
    want = R.render(mesh.points, mesh.triangles, h, w, colors=mesh.colors, R=Rm, t=t)
    got = np.asarray(Image.open(tmp_path / "view.png"))
    assert got.dtype == np.uint8 and np.array_equal(got, want.color) and (want.index < 0).any()
    assert (got[want.index < 0] == 128).all()
    # without a photo: the view's depth through colorize, at another size
    assert S.main([str(tmp_path / "d.npy"), str(tmp_path / "depth.png"), "--size", "30", "40", "--yaw", "-8"]) == 0
    pic = np.asarray(Image.open(tmp_path / "depth.png"))
    assert pic.shape == (30, 40, 3) and pic.dtype == np.uint8 and len(np.unique(pic.reshape(-1, 3), axis=0)) > 10
