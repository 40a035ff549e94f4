"""GPU: the adaptive mesh kernels (csrc/ada_adaptive.hip) behind hip_ext.geometry.adaptive_triangles against the numpy restatement of their contract,
tests/_adaptive_ref.py, which test_adaptive_mesh_cpu.py pins.  Every comparison is zero tolerance: the triangle rows and their order, the count, and the
error map E bit for bit (+inf included)."""
import numpy as np
import pytest
import torch

import _adaptive_ref as A

pytestmark = pytest.mark.gpu

SHAPES = ((2, 2), (3, 2), (2, 9), (9, 9), (17, 17), (12, 19), (5, 33), (70, 53), (130, 131))
TAUS = (0.0, 1e-3, 0.05, 1.0, None)
POISON = -77


def _depth(h, w, seed, bad=True):
    """Smooth ramps, a step edge, a little roughness; with ``bad`` a NaN, an inf, a zero and a negative value inside."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[:h, :w]
    d = 2.0 + 0.03 * i + 0.02 * j + 0.3 * np.sin(i / 3.0) * np.cos(j / 4.0)
    d[:, w // 2:] += 1.5
    d += 0.01 * rng.standard_normal((h, w))
    d = d.astype(np.float32)
    if bad and h * w > 20:
        for k, v in enumerate((np.nan, np.inf, 0.0, -1.0)):
            d[(3 * k + 1) % h, (5 * k + 2) % w] = v
    return d


def _hole(h, w):
    m = np.ones((h, w), dtype=np.uint8)
    m[h // 3:h // 3 + 2, w // 4:w // 4 + 3] = 0
    m[0, w - 1] = 0
    return m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_REFS = {}


def _ref(h, w, name):
    """(depth, keyword arguments of the restatement, {tau: triangles}, E) of a named variant, computed once and never modified."""
    key = (h, w, name)
    if key not in _REFS:
        d = _depth(h, w, 11 * h + w)
        kw = {}
        if "mask" in name:
            kw["mask"] = _hole(h, w)
        if "ratio" in name:
            kw["max_ratio"] = 1.25
        if "inverse" in name:
            d = np.where(np.isfinite(d), np.clip(d / 6.0, -1.0, 1.0), d).astype(np.float32)
            kw["inverse"] = (0.9, 0.1)
        tri, E = A.sweep(d, TAUS, **kw)
        for a in list(tri.values()) + [d, E]:
            a.setflags(write=False)
        _REFS[key] = (d, kw, tri, E)
    return _REFS[key]


def _check(G, d, kw, want, E, mask_arg=None):
    dev = torch.from_numpy(np.array(d)).cuda()
    args = {k: v for k, v in kw.items() if k != "mask"}
    if "mask" in kw:
        args["mask"] = mask_arg if mask_arg is not None else torch.from_numpy(np.array(kw["mask"])).cuda()
    for tau in TAUS:
        tri, err = G.adaptive_triangles(dev, max_error=tau, return_error=True, **args)
        assert tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3
        got = tri.cpu().numpy()
        assert got.shape == want[tau].shape, (tau, got.shape, want[tau].shape)      # the count
        assert np.array_equal(got, want[tau]), tau
        assert np.array_equal(_bits(err.cpu().numpy()), _bits(E)), tau


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_triangles_count_and_error_map_equal_the_restatement(hip, shape):
    from hip_ext import geometry as G
    h, w = shape
    for name in ("plain", "mask", "ratio", "inverse", "mask+ratio+inverse"):
        d, kw, want, E = _ref(h, w, name)
        _check(G, d, kw, want, E)


def test_more_sums_than_one_step_of_the_scan(hip):
    """417 x 993: 13 x 31 cells of 32, 806 subtrees under N = 1024, 10 + 11 * 806 = 8 876 sums, more than the 1024 * 8 of one step of the scan: the
    leaf-level sums of the whole last row of cells get their offsets from the carry, and max_error = 0.0 emits every leaf there."""
    import os
    import re
    from hip_ext import geometry as G
    h, w = 417, 993
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amodal-depth-anything_amd", "csrc", "ada_adaptive.hip")
    step = 1024 * int(re.search(r"constexpr int AD_SCAN_ITEMS = (\d+);", open(src).read()).group(1))
    cell, log_n = hip.ADAPT_CELL, int(np.ceil(np.log2(max(h, w) - 1)))
    lb, levels = 2 * (log_n - int(np.log2(cell))), 2 * log_n + 1
    n_sub = 2 * -(-(h - 1) // cell) * -(-(w - 1) // cell)
    assert (cell, log_n, n_sub) == (32, 10, 806) and lb + (levels - lb) * n_sub > step
    d, kw, want, E = _ref(h, w, "plain")
    _check(G, d, kw, want, E)


@pytest.mark.parametrize("shape", ((3, 2), (12, 19), (70, 53)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_forms(hip, shape):
    """bool, a numpy mask, and a pitched crop of a larger tensor read in place."""
    from hip_ext import geometry as G
    h, w = shape
    d, kw, want, E = _ref(h, w, "mask+ratio")
    m = np.array(kw["mask"])
    _check(G, d, kw, want, E, mask_arg=torch.from_numpy(m.astype(bool)).cuda())
    _check(G, d, kw, want, E, mask_arg=m)
    big = torch.full((h + 5, w + 9), 1, dtype=torch.uint8, device="cuda")
    big[2:2 + h, 4:4 + w] = torch.from_numpy(m).cuda()
    crop = big[2:2 + h, 4:4 + w]
    assert not crop.is_contiguous()
    _check(G, d, kw, want, E, mask_arg=crop)


def test_numpy_depth_and_clean_maps(hip):
    from hip_ext import geometry as G
    for h, w in ((17, 17), (33, 34)):
        d = _depth(h, w, 5, bad=False)
        want, E = A.sweep(d, TAUS)
        for tau in TAUS:
            got = G.adaptive_triangles(d, max_error=tau)
            assert np.array_equal(got.cpu().numpy(), want[tau])
        assert want[None].shape[0] == 2 * (h - 1) * (w - 1)
    i, j = np.mgrid[:17, :17]
    plane = (8 + 2 * i + 3 * j).astype(np.float32)      # a depth + b linear in (i, j) exactly
    assert G.adaptive_triangles(plane, inverse=(0.25, 1.0), max_error=0.0).cpu().numpy().tolist() == [[288, 0, 272], [0, 288, 16]]
    assert G.adaptive_triangles(plane[:12, :], inverse=(0.25, 1.0), max_error=0.0).shape[0] == A.adaptive_triangles(plane[:12, :], inverse=(0.25, 1.0), max_error=0.0).shape[0]


@pytest.mark.parametrize("shape", ((17, 17), (70, 53)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_explicit_capacity(hip, shape):
    from hip_ext import geometry as G
    h, w = shape
    d, kw, want, E = _ref(h, w, "mask+ratio+inverse")
    dev, m = torch.from_numpy(np.array(d)).cuda(), torch.from_numpy(np.array(kw["mask"])).cuda()
    args = dict(mask=m, max_ratio=kw["max_ratio"], inverse=kw["inverse"])
    for tau in (0.05, None):
        n = want[tau].shape[0]
        assert n > 4
        for cap in (n, n + 3, n - 2, 0):
            tri, count, err = G.adaptive_triangles(dev, max_error=tau, capacity=cap, return_error=True, **args)
            assert tuple(tri.shape) == (1, cap, 3) and tuple(count.shape) == (1,) and count.dtype == torch.int32
            assert count.item() == n      # the true number, also beyond the capacity: the overflow signal
            assert np.array_equal(tri[0, :min(n, cap)].cpu().numpy(), want[tau][:min(n, cap)])
            assert np.array_equal(_bits(err[0].cpu().numpy()), _bits(E))
    # rows from count on are untouched
    n = want[0.05].shape[0]
    import hip_ext
    tri = torch.full((1, n + 5, 3), POISON, dtype=torch.int32, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    hip_ext.mesh_adaptive(1, h, w, dev[None], tri, count, mask=m, row_pitch=m.stride(0), image_stride=0, inverse=kw["inverse"], max_ratio=kw["max_ratio"],
                          max_error=0.05)
    assert count.item() == n and np.array_equal(tri[0, :n].cpu().numpy(), want[0.05]) and bool((tri[0, n:] == POISON).all())


def test_batch_and_two_runs_give_the_same_bytes(hip):
    from hip_ext import geometry as G
    h, w = 130, 131
    maps = np.stack([_depth(h, w, s) for s in (1, 2, 3)])
    masks = np.stack([_hole(h, w), np.ones((h, w), np.uint8), _hole(h, w)[::-1].copy()])
    dev, m = torch.from_numpy(maps).cuda(), torch.from_numpy(masks).cuda()
    one = G.adaptive_triangles(dev, mask=m, max_ratio=1.3, max_error=0.01, return_error=True)
    two = G.adaptive_triangles(dev, mask=m, max_ratio=1.3, max_error=0.01, return_error=True)
    assert isinstance(one[0], list) and len(one[0]) == 3 and tuple(one[1].shape) == (3, h, w)
    assert torch.equal(one[1].view(torch.int64), two[1].view(torch.int64))
    for b in range(3):
        assert torch.equal(one[0][b], two[0][b])
        want, E = A.adaptive_triangles(maps[b], mask=masks[b], max_ratio=1.3, max_error=0.01, return_error=True)
        assert np.array_equal(one[0][b].cpu().numpy(), want) and np.array_equal(_bits(one[1][b].cpu().numpy()), _bits(E))
    cap = max(t.shape[0] for t in one[0])
    tri, count = G.adaptive_triangles(dev, mask=m, max_ratio=1.3, max_error=0.01, capacity=cap)
    assert count.tolist() == [t.shape[0] for t in one[0]]
    for b in range(3):
        assert torch.equal(tri[b, :count[b]], one[0][b])


def test_stream_capture_with_a_capacity(hip):
    import hip_ext
    h, w = 70, 53
    cap = 2 * (h - 1) * (w - 1)
    depth = torch.from_numpy(_depth(h, w, 0)[None]).cuda()
    tri = torch.empty(1, cap, 3, dtype=torch.int32, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    err = torch.empty(1, h, w, dtype=torch.float64, device="cuda")
    ws = torch.empty((hip_ext.mesh_adaptive_workspace_bytes(h, w) + 15) // 16 * 2, dtype=torch.int64, device="cuda")

    def run():
        hip_ext.mesh_adaptive(1, h, w, depth, tri, count, max_ratio=1.5, max_error=0.02, error=err, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for s in (1, 2):
        d1 = _depth(h, w, s)
        depth.copy_(torch.from_numpy(d1[None]))
        tri.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        want, E = A.adaptive_triangles(d1, max_ratio=1.5, max_error=0.02, return_error=True)
        n = want.shape[0]
        assert count.item() == n and 0 < n < cap
        assert np.array_equal(tri[0, :n].cpu().numpy(), want) and bool((tri[0, n:] == POISON).all())
        assert np.array_equal(_bits(err[0].cpu().numpy()), _bits(E))


def test_depth_to_mesh_with_a_tolerance(hip):
    from hip_ext import geometry as G
    h, w = 70, 53
    d = _depth(h, w, 4)
    m = _hole(h, w)
    dev = torch.from_numpy(d).cuda()
    colors = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(h, w, 3)).astype(np.uint8)).cuda()
    full = G.depth_to_mesh(dev, mask=m, max_ratio=1.3)
    today = G.depth_to_mesh(dev, mask=m, max_ratio=1.3, max_error=None)      # None is today's path
    assert full.triangle_count == today.triangle_count and torch.equal(full.triangles, today.triangles) and torch.equal(full.points, today.points)
    finest = G.depth_to_mesh(dev, mask=m, max_ratio=1.3, max_error=0.0, colors=colors)
    seen0 = G.render_mesh(finest, h, w).index.cpu().numpy() >= 0
    # today's mesh cuts its cells along the other diagonal, but around this map's hole, step and invalid pixels every vertex a triangle of one mesh
    # uses is used by a triangle of the other: the identity view samples at the vertices, so the two cover the same pixels
    assert seen0.any() and not seen0.all() and np.array_equal(seen0, G.render_mesh(today, h, w).index.cpu().numpy() >= 0)
    last = finest.triangle_count
    for tau in (1e-3, 0.05, 1.0):
        mesh = G.depth_to_mesh(dev, mask=m, max_ratio=1.3, max_error=tau, colors=colors)
        want = A.adaptive_triangles(d, mask=m, max_ratio=1.3, max_error=tau)
        assert isinstance(mesh, G.Mesh) and mesh.triangle_count == want.shape[0] <= last
        last = mesh.triangle_count
        tri = mesh.triangles.cpu().numpy()
        used = np.unique(want)
        assert mesh.vertex_count == used.size == tuple(mesh.points.shape)[0] == tuple(mesh.colors.shape)[0]
        assert tri.min() == 0 and tri.max() == mesh.vertex_count - 1      # only kept vertices, all of them
        assert np.array_equal(used[tri], want)      # the compaction renumbers in raster order
        loose = G.depth_to_mesh(dev, mask=m, max_ratio=1.3, max_error=tau, compact=False)
        assert np.array_equal(loose.triangles.cpu().numpy(), want) and loose.vertex_count == h * w
        assert torch.equal(loose.points[torch.from_numpy(used).cuda()], mesh.points)
        # the union of the triangles is the finest mesh's and the rasteriser's edges are inclusive integers: the same pixels are covered
        seen = G.render_mesh(mesh, h, w).index.cpu().numpy() >= 0
        assert np.array_equal(seen, seen0), tau
    assert last < finest.triangle_count // 4


def test_amodal_layers_with_a_tolerance(hip):
    from hip_ext import geometry as G
    from hip_ext.pipeline import AmodalResult
    h, w = 56, 70
    rng = np.random.default_rng(8)
    base = (0.15 + 0.7 * np.arange(w)[None, :] / w + 0.002 * rng.random((h, w))).astype(np.float32)
    masks = np.zeros((2, h, w), np.float32)
    ii, jj = np.mgrid[:h, :w]
    masks[0] = (((ii - h / 2) / (h / 3)) ** 2 + ((jj - w / 2) / (w / 4)) ** 2 <= 1.0).astype(np.float32)
    blended = np.stack([np.where(masks[0] > 0, np.float32(0.8) * base + np.float32(0.1), base), base]).astype(np.float32)
    res = AmodalResult(torch.from_numpy(base).cuda(), None, torch.from_numpy(blended).cuda(), torch.from_numpy(masks).cuda(), None)
    today, none = G.amodal_layers(res, max_ratio=1.1), G.amodal_layers(res, max_ratio=1.1, max_error=None)
    for a, b in zip([today.scene] + today.objects, [none.scene] + none.objects):
        assert torch.equal(a.triangles, b.triangles) and torch.equal(a.points, b.points)
    near, far, tau = 1.0, 10.0, 0.02
    inverse = (1.0 / near - 1.0 / far, 1.0 / far)
    got = G.amodal_layers(res, max_ratio=1.1, max_error=tau)
    assert len(got.objects) == 2
    for mesh, d, m in ((got.scene, base, None), (got.objects[0], blended[0], masks[0] > 0), (got.objects[1], blended[1], masks[1] > 0)):
        want = A.adaptive_triangles(d, mask=m, inverse=inverse, max_ratio=1.1, max_error=tau)
        used = np.unique(want)
        assert mesh.triangle_count == want.shape[0] and mesh.vertex_count == used.size
        if want.shape[0]:
            assert np.array_equal(used[mesh.triangles.cpu().numpy()], want)
    assert got.objects[1].triangle_count == 0 and 0 < got.objects[0].triangle_count < got.scene.triangle_count < today.scene.triangle_count // 4


def test_command_lines_take_a_tolerance(hip, tmp_path):
    """depth_to_mesh --max_error writes the restatement's (conforming) mesh as a PLY; depth_to_view --max_error renders it."""
    from PIL import Image

    from src.scripts import depth_to_mesh as S
    from src.scripts import depth_to_view as V
    rng = np.random.default_rng(17)
    h, w = 37, 53
    v = (20000 + 30000 * np.arange(w)[None, :] / w + 40 * rng.random((h, w))).astype(np.uint16)
    src, dst, png = str(tmp_path / "depth.png"), str(tmp_path / "out" / "mesh.ply"), str(tmp_path / "view.png")
    Image.fromarray(v).save(src)
    assert S.main([src, dst, "--inverse", "1", "10", "--max_ratio", "2", "--max_error", "0.01"]) == 0
    depth = (v.astype(np.float64) / 65535.0).astype(np.float32)
    want = A.adaptive_triangles(depth, inverse=(1.0 / 1 - 1.0 / 10, 1.0 / 10), max_ratio=2.0, max_error=0.01)
    used = np.unique(want)
    head = open(dst, "rb").read(400).split(b"end_header")[0].decode()
    assert f"element vertex {used.size}\n" in head and f"element face {want.shape[0]}\n" in head
    assert 0 < want.shape[0] < 2 * (h - 1) * (w - 1) // 4
    mesh = S.mesh_file(src, dst, inverse=(1.0, 10.0), max_ratio=2.0, max_error=0.01)
    assert np.array_equal(used[mesh.triangles.cpu().numpy()], want)
    assert V.main([src, png, "--inverse", "1", "10", "--max_ratio", "2", "--max_error", "0.01", "--yaw", "5"]) == 0
    a = np.asarray(Image.open(png))
    assert a.shape == (h, w, 3) and len(np.unique(a.reshape(-1, 3), axis=0)) > 16      # a rendered surface, not one flat fill


def test_arguments_are_checked(hip):
    from hip_ext import geometry as G
    d = torch.ones(9, 9, device="cuda")
    for bad in (-0.1, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="max_error"):
            G.adaptive_triangles(d, max_error=bad)
    with pytest.raises(ValueError, match="at least 2"):
        G.adaptive_triangles(torch.ones(1, 9, device="cuda"), max_error=0.1)
    with pytest.raises(ValueError, match="differ in shape"):
        G.adaptive_triangles(d, mask=torch.ones(9, 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="capacity"):
        G.adaptive_triangles(d, capacity=-1)
    with pytest.raises(hip.HipExtError, match="no CPU fallback"):
        G.adaptive_triangles(torch.ones(9, 9))
    with pytest.raises(hip.HipExtError, match="beyond"):
        hip.mesh_adaptive_workspace_bytes(2, 16386 + 1)
