"""CPU: the numpy restatement of the rasteriser's contract (tests/_raster_ref.py) pinned to hand-derived cases and cross-checked with matplotlib.tri, an
independent implementation of point location and linear interpolation on a triangulation; and everything of the feature that needs no device: the ABI
surface, the build lists, the argument checks, look_at_pose and the command line."""
import os
import re

import numpy as np
import pytest
import torch

import _geometry_ref as G_REF
import _raster_ref as R
import hip_ext
from hip_ext import geometry as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("ada_mesh_project_fwd", "ada_mesh_raster_fwd")


def records(uvz):
    """Vertices given as (u, v, z) in pixels -> the vertex records, snapped."""
    uvz = np.asarray(uvz, dtype=np.float64).reshape(-1, 3)
    return R.snap(uvz[:, 0]), R.snap(uvz[:, 1]), 1.0 / uvz[:, 2], np.ones(uvz.shape[0], bool)


def picture(index, of=0):
    return ["".join("#" if v == of else "." for v in row) for row in index]


# ------------------------------------------------------------------ hand-derived pins
# vertices (u, v) = (1, 1), (6, 1), (1, 6): the samples with u >= 1, v >= 1, u + v <= 7 -- the three vertices and every sample on the three edges included
ONE_TRIANGLE = ["........",
                ".######.",
                ".#####..",
                ".####...",
                ".###....",
                ".##.....",
                ".#......",
                "........"]


@pytest.mark.parametrize("winding", [(0, 1, 2), (0, 2, 1), (2, 0, 1)])
def test_one_triangle_on_samples_covers_its_edges_and_vertices_in_both_windings(winding):
    X, Y, w, valid = records([(1, 1, 2.0), (6, 1, 2.0), (1, 6, 2.0)])
    depth, index, _, _ = R.rasterize(X, Y, w, valid, [winding], 8, 8)
    assert picture(index) == ONE_TRIANGLE
    assert np.all(depth[index == 0] == np.float32(2.0)) and np.all(np.isinf(depth[index < 0]))


# the square (1, 1) .. (5, 5) cut along u + v = 6: triangle 0 has the corner (1, 1), triangle 1 the corner (5, 5); the diagonal's five samples are in both
SHARED_FIRST = ["........",
                ".#####..",
                ".####...",
                ".###....",
                ".##.....",
                ".#......",
                "........",
                "........"]
SHARED_SECOND = ["........",
                 "........",
                 ".....#..",
                 "....##..",
                 "...###..",
                 "..####..",
                 "........",
                 "........"]


def test_a_shared_edge_goes_to_the_lower_index_and_swapping_swaps_the_ids():
    X, Y, w, valid = records([(1, 1, 2.0), (5, 1, 2.0), (1, 5, 2.0), (5, 5, 2.0)])
    tri = np.array([[0, 2, 1], [3, 1, 2]])
    depth, index, _, _ = R.rasterize(X, Y, w, valid, tri, 8, 8)
    assert picture(index, 0) == SHARED_FIRST and picture(index, 1) == SHARED_SECOND
    depth2, index2, _, _ = R.rasterize(X, Y, w, valid, tri[::-1], 8, 8)
    diagonal = np.add.outer(np.arange(8), np.arange(8)) == 6
    assert np.all(index[diagonal & (index >= 0)] == 0) and np.all(index2[diagonal & (index2 >= 0)] == 0)
    off = ~diagonal & (index >= 0)
    assert np.array_equal(index2[off], 1 - index[off]) and np.array_equal((index >= 0), (index2 >= 0))
    assert np.array_equal(depth, depth2)


def test_snapping_rounds_to_the_nearest_256th_half_to_even():
    assert R.snap(2.498) == 639                                  # 639.488
    assert R.snap(3 + 1 / 512) == 768 and R.snap(3 + 3 / 512) == 770 and R.snap(-(3 + 1 / 512)) == -768      # exact halves
    K = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    X, Y, w, valid = R.project(np.array([[-2.498, -(4 + 1 / 512), 1.0], [-(5 + 3 / 512), 0.25, 1.0]]), K)
    assert X.tolist() == [639, 1282] and Y.tolist() == [1024, -64] and w.tolist() == [1.0, 1.0] and valid.all()


def test_inverse_depth_is_interpolated_and_the_nearest_surface_wins():
    # a big far triangle (z = 4) under a small near one (z = 2); listed far-first and near-first
    X, Y, w, valid = records([(0, 0, 4.0), (7, 0, 4.0), (0, 7, 4.0), (1, 1, 2.0), (3, 1, 2.0), (1, 3, 2.0)])
    for tri, near in (([[0, 1, 2], [3, 4, 5]], 1), ([[3, 4, 5], [0, 1, 2]], 0)):
        depth, index, _, _ = R.rasterize(X, Y, w, valid, tri, 8, 8, out="w")
        assert index[1, 1] == near and index[2, 2] == near and index[3, 3] == 1 - near and index[7, 7] == -1
        assert depth[1, 1] == np.float32(0.5) and depth[3, 3] == np.float32(0.25) and depth[7, 7] == 0.0
    # w, not z, is linear on the screen: halfway between z = 1 and z = 3 lies w = 2 / 3
    X, Y, w, valid = records([(0, 0, 1.0), (4, 0, 3.0), (0, 4, 1.0)])
    depth, _, _, w64 = R.rasterize(X, Y, w, valid, [[0, 1, 2]], 8, 8, out="z")
    assert abs(w64[0, 2] - 2 / 3) < 1e-15 and depth[0, 2] == np.float32(1.0 / w64[0, 2])


def test_colours_are_perspective_correct_and_rounded_half_up():
    X, Y, w, valid = records([(0, 0, 1.0), (4, 0, 3.0), (0, 4, 1.0)])
    colors = np.array([[0, 10, 255], [200, 10, 255], [0, 10, 255]], np.uint8)
    _, index, color, _ = R.rasterize(X, Y, w, valid, [[0, 1, 2]], 8, 8, colors=colors, fill_color=(1, 2, 3))
    # at u = 2: e0 = e1 (equal screen weights), n0 = 1, n1 = 1 / 3: the red channel is 200 (1/3) / (4/3) = 50, not the screen-space 100
    assert color[0, 2].tolist() == [50, 10, 255] and color[0, 0].tolist() == [0, 10, 255] and color[0, 4].tolist() == [200, 10, 255]
    assert color[7, 7].tolist() == [1, 2, 3] and index[7, 7] == -1


# ------------------------------------------------------------------ matplotlib.tri
def test_the_restatement_agrees_with_matplotlib_tri_on_a_warped_grid():
    from matplotlib.tri import LinearTriInterpolator, Triangulation
    gh, gw, H, W = 12, 16, 96, 128
    tri = G_REF.triangles(gh, gw)
    y, x = (a.reshape(-1).astype(np.float64) for a in np.mgrid[0:gh, 0:gw])
    z = 3 + 0.5 * np.sin(0.7 * x) + 0.3 * np.cos(0.9 * y)
    u = 7.3 * x + 0.21 * y + 0.37 + 0.05 * z
    v = 7.1 * y - 0.13 * x + 0.61 + 0.03 * z
    X, Y = R.snap(u), R.snap(v)
    w = 1.0 / z
    depth, index, _, w64 = R.rasterize(X, Y, w, np.ones(x.size, bool), tri, H, W, out="w")
    tr = Triangulation(X / 256.0, Y / 256.0, tri)      # the snapped coordinates: exact in float64
    sy, sx = (a.astype(np.float64) for a in np.mgrid[0:H, 0:W])
    # samples within 1 / 64 pixel of any edge are left out: there a point-location routine in floating point may name either neighbour
    near = np.zeros((H, W), bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        for k in range(tri.shape[0]):
            ax, ay, bx, by = X[tri[k, a]] / 256.0, Y[tri[k, a]] / 256.0, X[tri[k, b]] / 256.0, Y[tri[k, b]] / 256.0
            dx, dy = bx - ax, by - ay
            s = np.clip(((sx - ax) * dx + (sy - ay) * dy) / (dx * dx + dy * dy), 0.0, 1.0)
            near |= np.hypot(sx - (ax + s * dx), sy - (ay + s * dy)) < 1.0 / 64
    assert near.mean() <= 0.02, near.mean()
    found = tr.get_trifinder()(sx, sy)
    assert np.array_equal(found[~near], index[~near]) and (index < 0).any() and (index >= 0).sum() > 5000
    interp = LinearTriInterpolator(tr, w)(sx, sy)
    inside = ~near & (index >= 0)
    assert not np.ma.getmaskarray(interp)[inside].any()
    assert np.max(np.abs(np.asarray(interp)[inside] - w64[inside]) / w64[inside]) <= 1e-12


# ------------------------------------------------------------------ identity round trip
def test_the_identity_view_of_a_depth_mesh_gives_the_map_back():
    h, w = 37, 61
    depth = np.random.default_rng(3761).uniform(0.5, 9.0, size=(h, w)).astype(np.float32)
    pts = G_REF.points(depth)      # the reference's formula, float64
    view = R.render(pts.reshape(-1, 3), G_REF.triangles(h, w), h, w, K=G_REF.intrinsics(h, w))
    assert (view.index >= 0).all() and (view.owner == 0).all()
    ulps = np.abs(view.depth.view(np.int32).astype(np.int64) - depth.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, ulps.max()


# ------------------------------------------------------------------ dropped triangles
def test_dropped_triangles_leave_the_target_empty():
    K = R.intrinsics(8, 8)
    good = [[-0.5, -0.5, 2.0], [0.5, -0.5, 2.0], [-0.5, 0.5, 2.0]]
    bad = {"behind": [0.0, 0.0, -1.0], "at the camera": [0.0, 0.0, 0.0], "nan": [np.nan, 0.0, 2.0], "inf": [0.0, 0.0, np.inf],
           "guard band": [-2.0 * 16385 / K[0, 0], 0.0, 2.0], "too near": [0.0, 0.0, 2.0 ** -65], "too far": [0.0, 0.0, 2.0 ** 65]}
    ok = R.render(np.array(good), [[0, 1, 2]], 8, 8, K=K)
    assert (ok.index == 0).any()
    for name, vertex in bad.items():
        pts = np.array(good + [vertex])
        assert R.project(pts, K)[3].tolist() == [True, True, True, False], name
        view = R.render(pts, [[0, 1, 3]], 8, 8, K=K)
        assert (view.index == -1).all() and np.isinf(view.depth).all(), name
        both = R.render(pts, [[0, 1, 3], [0, 1, 2]], 8, 8, K=K)      # the kept one keeps its own id
        assert np.array_equal(both.index >= 0, ok.index >= 0) and set(np.unique(both.index)) == {-1, 1}, name
    edge = np.array(good + [[-2.0 * 16384 / K[0, 0] + 2.0 * 4.0 / K[0, 0], 0.0, 2.0]])      # u = 16384 exactly is still inside the band
    assert R.project(edge, K)[3].all() and R.project(edge, K)[0][3] == 256 * 16384
    for tri in ([[0, 1, 1]], [[0, 0, 0]], [[0, 1, 3]], [[0, 1, -1]], [[0, 1, 2 ** 31 - 1]]):      # no area; a vertex index that is not there
        pts = np.array(good)
        assert (R.render(pts, tri, 8, 8, K=K).index == -1).all(), tri
    collinear = np.array([[-0.5, 0.0, 2.0], [0.0, 0.0, 2.0], [0.5, 0.0, 2.0]])
    assert (R.render(collinear, [[0, 1, 2]], 8, 8, K=K).index == -1).all()


def test_pose_arithmetic_and_its_absence():
    pts = np.random.default_rng(5).uniform(-1, 1, (50, 3)) + [0, 0, 3.0]
    K = R.intrinsics(20, 30)
    a = R.project(pts, K)
    b = R.project(pts, K, R=np.eye(3), t=np.zeros(3))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    Rm, t = R.look_at_pose(yaw_deg=12, shift=(0.2, 0, 0), pivot_z=3.0)
    q = pts @ Rm.T + t
    c = R.project(pts, K, R=Rm, t=t)
    assert np.max(np.abs(c[0] / 256.0 - (K[0, 0] * (-q[:, 0] / q[:, 2]) + K[0, 2]))) < 1 / 256


# ------------------------------------------------------------------ plumbing
def test_exports_header_and_abi():
    for name in NEW_EXPORTS:
        assert name in hip_ext.EXPORTS
    header = open(os.path.join(ROOT, "include", "ada_hip.h")).read()
    assert re.search(r"#define ADA_ABI_VERSION 10\b", header) and hip_ext.ABI_VERSION == 10
    for name in NEW_EXPORTS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
    for macro, value in (("ADA_RASTER_SMALL_MAX", hip_ext.RASTER_SMALL_MAX), ("ADA_RASTER_WAVE_MAX", hip_ext.RASTER_WAVE_MAX),
                         ("ADA_RASTER_TILE_W", hip_ext.RASTER_TILE_W), ("ADA_RASTER_TILE_H", hip_ext.RASTER_TILE_H),
                         ("ADA_RASTER_WALK_BLOCKS", hip_ext.RASTER_WALK_BLOCKS), ("ADA_RASTER_WALK_SHARE", hip_ext.RASTER_WALK_SHARE),
                         ("ADA_RASTER_OUT_W", hip_ext.RASTER_OUT_W),
                         ("ADA_RASTER_OUT_Z", hip_ext.RASTER_OUT_Z), ("ADA_RASTER_OUT_NORMALISED", hip_ext.RASTER_OUT_NORMALISED)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert hip_ext.mesh_raster_workspace_bytes(3, 3, 5) == 8 * 10 + 16 + 20 and hip_ext.mesh_raster_workspace_bytes(2, 4, 0) == 8 * 8 + 16


def test_the_build_lists_the_file_without_contraction_and_without_scratch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_ada_build", os.path.join(ROOT, "amodal-depth-anything_amd", "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "ada_raster.hip" in build.SOURCES and "ada_raster.hip" in build.NO_SCRATCH
    assert "-ffp-contract=off" in build.PER_FILE_FLAGS["ada_raster.hip"]
    assert os.path.exists(os.path.join(ROOT, "amodal-depth-anything_amd", "csrc", "ada_raster.hip"))


def test_argument_validation():
    pts = torch.zeros(3, 3)
    tri = torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(G.HipExtError):
        G.render_mesh(pts, 8, 8, triangles=tri)                              # CPU tensors: no fallback
    with pytest.raises(G.HipExtError):
        G.render_meshes([G.Mesh(pts, tri, 3, 1, None)], 8, 8)
    with pytest.raises(ValueError):
        G.render_mesh(pts, 8, 8)                                             # points without triangles
    with pytest.raises(ValueError):
        G.render_mesh(pts, 0, 8, triangles=tri)
    with pytest.raises(ValueError):
        G.render_mesh(pts, 2 ** 15, 2 ** 15, triangles=tri)                  # h w >= 2^30
    with pytest.raises(ValueError):
        G.render_mesh(pts, 8, 8, triangles=tri, K=[[10.0, 0.5, 4.0], [0.0, 10.0, 4.0], [0.0, 0.0, 1.0]])      # skew
    with pytest.raises(ValueError):
        G.render_mesh(pts, 8, 8, triangles=tri, K=np.eye(4))
    with pytest.raises(ValueError):
        G.render_mesh(pts, 8, 8, triangles=tri, out="normalised")            # needs inverse
    with pytest.raises(ValueError):
        G.render_mesh(pts, 8, 8, triangles=tri, out="normalised", inverse=(0.0, 1.0))
    with pytest.raises(ValueError):
        G.render_mesh(pts, 8, 8, triangles=tri, out="depth")
    with pytest.raises(ValueError):
        G.render_mesh(pts, 8, 8, triangles=tri.long())
    with pytest.raises(ValueError):
        G.render_mesh(torch.zeros(3, 2), 8, 8, triangles=tri)
    with pytest.raises(ValueError):
        G.render_mesh(pts, 8, 8, triangles=tri, colors=torch.zeros(2, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        G.render_mesh(pts, 8, 8, triangles=tri, R=np.eye(2))
    with pytest.raises(ValueError):
        G.render_mesh(pts, 8, 8, triangles=tri, fill_color=(0, 0, 256))
    with pytest.raises(ValueError):
        G.render_mesh(G.Mesh(pts, tri, 3, 1, None), 8, 8, triangles=tri)     # a Mesh carries its own
    with pytest.raises(TypeError):
        G.render_meshes([pts], 8, 8)
    layers = G.Layers(G.Mesh(pts, tri, 3, 1, None), [])
    with pytest.raises(ValueError):
        G.render_layers(layers, 8, 8, objects=[0])
    with pytest.raises(ValueError):
        G.render_layers(layers, 8, 8, scene=False)
    with pytest.raises(ValueError):
        G.render_layers(layers, 8, 8, near=2.0, far=1.0)
    with pytest.raises(G.HipExtError):
        G.render_layers(layers, 8, 8)
    assert G.View._fields == ("depth", "index", "owner", "color")


@pytest.mark.parametrize("kw", [dict(yaw_deg=12), dict(pitch_deg=-7.5), dict(yaw_deg=31, pitch_deg=18, pivot_z=2.5), dict(yaw_deg=-170, pivot_z=4.0)])
def test_look_at_pose_is_a_rotation_that_leaves_the_pivot_fixed(kw):
    Rm, t = G.look_at_pose(**kw)
    assert Rm.dtype == np.float64 and t.dtype == np.float64 and Rm.shape == (3, 3) and t.shape == (3,)
    assert np.max(np.abs(Rm.T @ Rm - np.eye(3))) <= 1e-15 and abs(np.linalg.det(Rm) - 1) <= 1e-15
    c = np.array([0.0, 0.0, kw.get("pivot_z", 0.0)])
    assert np.max(np.abs(Rm @ c + t - c)) <= 1e-15
    R2, t2 = G.look_at_pose(shift=(0.2, -0.1, 0.3), **kw)
    assert np.array_equal(R2, Rm) and np.max(np.abs(t2 - t - [0.2, -0.1, 0.3])) <= 1e-15
    R3, t3 = R.look_at_pose(**kw)
    assert np.array_equal(R3, Rm) and np.array_equal(t3, t)


def test_look_at_pose_defaults_to_no_motion():
    Rm, t = G.look_at_pose()
    assert np.array_equal(Rm, np.eye(3)) and np.array_equal(t, np.zeros(3))
    with pytest.raises(ValueError):
        G.look_at_pose(shift=(1, 2))


def test_the_command_line_parses_and_reads(tmp_path):
    from PIL import Image
    from src.scripts import depth_to_view as S
    args = S.build_parser().parse_args(["d.png", "o.png", "--inverse", "1", "10", "--max_ratio", "2", "--yaw", "12", "--pitch", "-3", "--shift", "0.2", "0", "-1",
                                        "--size", "40", "60", "--image", "p.png", "--mask", "m.png", "--fov", "60"])
    assert (args.input, args.output, args.inverse, args.max_ratio, args.yaw, args.pitch) == ("d.png", "o.png", [1.0, 10.0], 2.0, 12.0, -3.0)
    assert (list(args.shift), args.size, args.image, args.mask, args.fov) == ([0.2, 0.0, -1.0], [40, 60], "p.png", "m.png", 60.0)
    d = S.build_parser().parse_args(["d.npy", "o.png"])
    assert (d.inverse, d.max_ratio, d.yaw, d.pitch, tuple(d.shift), d.size, d.image, d.mask, d.fov) == (None, None, 0.0, 0.0, (0.0, 0.0, 0.0), None, None, None, 55.0)
    assert S.inverse_pair(None) is None and S.inverse_pair((1.0, 10.0)) == (1.0 - 0.1, 0.1)
    with pytest.raises(ValueError):
        S.inverse_pair((10.0, 1.0))
    u16 = (np.arange(12, dtype=np.uint16).reshape(3, 4) * 5000)
    Image.fromarray(u16).save(tmp_path / "d.png")
    got = S.read_depth(str(tmp_path / "d.png"), normalise=True)
    assert got.dtype == np.float32 and np.array_equal(got, (u16.astype(np.float64) / 65535.0).astype(np.float32))
    assert S.pivot_depth(np.array([[1.0, 2.0, 3.0, np.nan, -1.0]], np.float32)) == 2.0
    assert S.pivot_depth(np.array([[0.0, 1.0]], np.float32), (0.9, 0.1)) == np.median([10.0, 1.0])
    with pytest.raises(G.HipExtError):      # the reader ran; the device path has no CPU fallback
        S.view_file(str(tmp_path / "d.png"), str(tmp_path / "o.png"), inverse=(1.0, 10.0), device="cpu")
