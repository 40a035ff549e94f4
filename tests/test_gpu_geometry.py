"""GPU: depth maps to points, masked triangles and compacted meshes on the device (csrc/ada_geometry.hip through hip_ext.geometry) against the goldens
written from the real reference (tests/golden/geometry/cases.npz) and the numpy restatement tests/_geometry_ref.py, which test_geometry_cpu.py pins to
those goldens.  Never one device path against another.  Points of the default pose and every integer output: np.array_equal.  A general pose: the
derived bound 2 gamma_4 (sum_j |R_ij| |q_j| + |t_i|) against the reference, no looser."""
import os

import numpy as np
import pytest
import torch

import _geometry_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "geometry", "cases.npz"))
GOLDEN_SHAPES = [tuple(int(v) for v in s) for s in GOLDEN["shapes"]]
POISON = -7777777


def _depth(h, w, seed, lo=0.5, hi=20.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=(h, w)).astype(np.float32)


def _mask(h, w, seed, density=0.7):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def _ellipse(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return ((((y - 0.52 * h) / (0.37 * h)) ** 2 + ((x - 0.45 * w) / (0.31 * w)) ** 2) <= 1.0).astype(np.uint8)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ------------------------------------------------------------------ points
@pytest.mark.parametrize("hw", GOLDEN_SHAPES)
def test_points_default_pose_equal_the_reference_bit_for_bit(hip, hw):
    from hip_ext import geometry as G
    name = "%dx%d" % hw
    depth, want = GOLDEN[name + "_depth"], GOLDEN[name + "_points"]
    p64 = G.depth_to_points(depth)
    assert p64.dtype == torch.float64 and _same(p64.cpu().numpy(), want)
    p32, valid = G.depth_to_points(torch.from_numpy(depth).cuda(), dtype=torch.float32, return_valid=True)
    assert _same(p32.cpu().numpy(), want.astype(np.float32)) and valid.dtype == torch.uint8 and bool(valid.all())


@pytest.mark.parametrize("hw", [(64, 64), (130, 257), (3, 1030)])
def test_points_default_pose_equal_the_restatement(hip, hw):
    from hip_ext import geometry as G
    depth = _depth(*hw, seed=hw[1])
    want = R.points(depth)
    assert _same(G.depth_to_points(depth).cpu().numpy(), want)
    assert _same(G.depth_to_points(depth, dtype=torch.float32).cpu().numpy(), want.astype(np.float32))
    K = np.array([[311.5, 0.0, 100.25], [0.0, 297.0, 60.5], [0.0, 0.0, 1.0]])      # any pinhole camera without skew
    assert _same(G.depth_to_points(depth, K=K).cpu().numpy(), R.points(depth, K=K))
    assert _same(G.depth_to_points(depth, fov_deg=70.0).cpu().numpy(), R.points(depth, fov_deg=70.0))


def test_points_batch_of_three_distinct_maps(hip):
    from hip_ext import geometry as G
    depth = np.stack([_depth(37, 61, seed=s, hi=5.0 + 20 * s) for s in range(3)])
    got = G.depth_to_points(depth)
    assert got.shape == (3, 37, 61, 3) and _same(got.cpu().numpy(), np.stack([R.points(d) for d in depth]))


def _special(h, w, seed):
    d = _depth(h, w, seed)
    flat = d.reshape(-1)
    picks = np.random.default_rng(seed + 1).choice(h * w, size=12, replace=False)
    flat[picks] = np.array([0.0, -0.0, -1.5, -1e30, np.inf, -np.inf, np.nan, 1e-40, 3e38, np.inf, np.nan, -2.0], np.float32)
    return d


@pytest.mark.parametrize("inverse", [None, (0.9, 0.1), (1.0, 0.0), (1.0, -2.0)])
def test_points_nan_pattern_and_validity_at_zero_negative_infinite_and_nan_depth(hip, inverse):
    from hip_ext import geometry as G
    d = _special(37, 61, 3)
    d[0, 0] = 0.0      # with (1, 0): a v + b = 0, z = inf
    d[5, 5] = 2.0      # with (1, -2): a v + b = 0
    want, z = R.points(d, inverse=inverse), R.z_of(d, inverse)
    for dtype in (torch.float64, torch.float32):
        got, valid = G.depth_to_points(d, inverse=inverse, dtype=dtype, return_valid=True)
        got = got.cpu().numpy()
        with np.errstate(over="ignore"):
            assert _same(got, want.astype(got.dtype))
        assert np.array_equal(np.isnan(got).all(-1), ~np.isfinite(z)) and np.array_equal(np.isnan(got).any(-1), ~np.isfinite(z))
        assert np.array_equal(valid.cpu().numpy(), R.valid_of(z).astype(np.uint8))
    assert (~np.isfinite(z)).sum() >= 2 and (np.isfinite(z) & (z <= 0)).sum() >= 2


def test_points_inverse_mode_equals_the_reference_applied_to_the_converted_map(hip):
    from hip_ext import geometry as G
    a, b = (float(v) for v in GOLDEN["inv_ab"])
    assert _same(G.depth_to_points(GOLDEN["inv_depth"], inverse=(a, b)).cpu().numpy(), GOLDEN["inv_points"])


@pytest.mark.parametrize("i", [0, 1])
def test_points_general_pose_within_the_derived_bound_of_the_reference(hip, i):
    from hip_ext import geometry as G
    h, w = (int(v) for v in GOLDEN[f"pose{i}_shape"])
    depth, Rm, t = GOLDEN[f"{h}x{w}_depth"], GOLDEN[f"pose{i}_R"], GOLDEN[f"pose{i}_t"]
    got = G.depth_to_points(depth, R=Rm, t=t).cpu().numpy()
    err, bound = np.abs(got - GOLDEN[f"pose{i}_points"]), R.pose_bound(depth, Rm, t)
    print(f"general pose {h}x{w}: max |ours - reference| / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert _same(got, R.points(depth, Rm, t))      # and the restatement's stated order of operations exactly


def test_points_general_pose_larger_shape(hip):
    from hip_ext import geometry as G
    rng = np.random.default_rng(77)
    depth, Rm, t = _depth(130, 257, 9), np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.uniform(-3, 3, 3)
    got = G.depth_to_points(depth, R=Rm, t=t).cpu().numpy()
    # numpy's own stacked matmul from the identical q, as the reference forms it
    q = R.points(depth)
    ref = (Rm[None, None] @ q[..., None])[..., 0] + t
    assert (np.abs(got - ref) <= R.pose_bound(depth, Rm, t)).all()
    assert _same(got, R.points(depth, Rm, t))


# ------------------------------------------------------------------ triangles
def _check_tri(G, h, w, mask=None, depth=None, inverse=None, max_ratio=None):
    got = G.create_triangles(h, w, mask=mask, depth=depth, inverse=inverse, max_ratio=max_ratio)
    want = R.triangles(h, w, mask, depth, inverse, max_ratio)
    assert got.dtype == torch.int32 and _same(got.cpu().numpy(), want), (h, w, tuple(got.shape), want.shape)
    return want.shape[0]


@pytest.mark.parametrize("hw", GOLDEN_SHAPES)
def test_triangles_equal_the_reference_order_included(hip, hw):
    from hip_ext import geometry as G
    name = "%dx%d" % hw
    got = G.create_triangles(*hw, mask=GOLDEN[name + "_mask"])
    assert np.array_equal(got.cpu().numpy().astype(np.int64), GOLDEN[name + "_tri"].astype(np.int64)) and got.shape[1] == 3
    got = G.create_triangles(*hw)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), GOLDEN[name + "_tri_all"].astype(np.int64)) and got.shape[1] == 3


@pytest.mark.parametrize("hw", [(37, 61), (70, 130)])
def test_triangles_mask_contents(hip, hw):
    from hip_ext import geometry as G
    h, w = hw
    y, x = np.mgrid[0:h, 0:w]
    last = np.zeros((h, w), np.uint8)
    last[-2:, -2:] = 1
    first = np.zeros((h, w), np.uint8)
    first[:2, :2] = 1
    assert _check_tri(G, h, w, np.ones((h, w), np.uint8)) == 2 * (h - 1) * (w - 1)
    assert _check_tri(G, h, w, np.zeros((h, w), np.uint8)) == 0
    assert _check_tri(G, h, w, ((y + x) % 2).astype(np.uint8)) == 0
    assert _check_tri(G, h, w, _mask(h, w, 1) * np.uint8(255)) > 100
    assert _check_tri(G, h, w, last) == 2
    assert _check_tri(G, h, w, first) == 2
    assert _check_tri(G, h, w, _mask(h, w, 2).astype(bool)) > 100


def _edge_shapes(hip):
    """(h, w) whose cell counts sit just below, at and just above each chunk constant of the kernels, as the binding exports them."""
    out = []
    for c in (hip.GEOM_WAVE, hip.GEOM_CHUNK):
        out += [(2, c), (2, c + 1), (2, c + 2), (3, c // 2 + 1)]                 # c - 1, c, c + 1 cells in one row; c cells in two rows
    side = int(round((hip.GEOM_CHUNK * hip.GEOM_SCAN_BLOCK) ** 0.5))             # one scan step covers CHUNK * SCAN_BLOCK cells
    assert side * side == hip.GEOM_CHUNK * hip.GEOM_SCAN_BLOCK
    out += [(side + 1, side), (side + 1, side + 1), (side + 1, side + 2)]
    return out


def test_triangles_at_every_chunk_edge(hip):
    from hip_ext import geometry as G
    assert (hip.GEOM_WAVE, hip.GEOM_CHUNK, hip.GEOM_SCAN_BLOCK) == (64, 1024, 1024)
    for h, w in _edge_shapes(hip):
        density = 0.9 if h * w < 10 ** 5 else 0.75
        m = _mask(h, w, h + w, density)
        m[-2:, -2:] = 1         # the very last candidates are kept
        assert _check_tri(G, h, w, m) > 2, (h, w)


def test_triangles_beyond_the_reciprocal_division(hip):
    """At 2^24 cells and more the cell's row comes from an integer division, below from a float reciprocal: one grid past the threshold."""
    from hip_ext import geometry as G
    h, w = 4098, 4097
    assert (h - 1) * (w - 1) >= 2 ** 24
    m = np.zeros((h, w), np.uint8)
    m[:3, :5] = 1
    m[2000:2040, 4000:] = 1
    m[-3:, -70:] = 1
    m[-40:, :2] = 1
    m[4095:4098, 1000:1100] = _mask(3, 100, 5, 0.8)
    assert _check_tri(G, h, w, m) > 5000


def test_triangles_518_ellipse(hip):
    from hip_ext import geometry as G
    assert _check_tri(G, 518, 518, _ellipse(518, 518)) > 10 ** 5


def test_triangles_batch_of_three_masks(hip):
    from hip_ext import geometry as G
    h, w = 70, 130
    masks = np.stack([_mask(h, w, 4, 0.9), np.zeros((h, w), np.uint8), _ellipse(h, w)])
    got = G.create_triangles(h, w, mask=masks)
    want = [R.triangles(h, w, m) for m in masks]
    assert isinstance(got, list) and [g.shape[0] for g in got] == [t.shape[0] for t in want] and want[1].shape[0] == 0
    assert all(_same(g.cpu().numpy(), t) for g, t in zip(got, want))
    tri, count = G.create_triangles(h, w, mask=masks, capacity=max(t.shape[0] for t in want))
    assert count.dtype == torch.int32 and count.tolist() == [t.shape[0] for t in want]
    assert all(_same(tri[b, :t.shape[0]].cpu().numpy(), t) for b, t in enumerate(want))


def test_triangles_mask_is_a_pitched_crop_read_in_place(hip):
    from hip_ext import geometry as G
    big = torch.from_numpy(np.stack([_mask(90, 150, s, 0.8) for s in (1, 2)])).cuda()
    crop = big[:, 7:77, 11:141]
    assert not crop.is_contiguous()
    got = G.create_triangles(70, 130, mask=crop)
    for b in range(2):
        assert _same(got[b].cpu().numpy(), R.triangles(70, 130, crop[b].cpu().numpy()))
    assert _same(G.create_triangles(70, 130, mask=crop[1]).cpu().numpy(), R.triangles(70, 130, crop[1].cpu().numpy()))


def _raw_triangles(hip, masks, capacity, depth=None, inverse=None, max_ratio=0.0, guard=4096):
    """hip_ext.mesh_triangles into a poisoned buffer with a guard region behind it: (buffer [B, capacity, 3], count, guard)."""
    B, h, w = masks.shape
    flat = torch.full((B * capacity * 3 + guard,), POISON, dtype=torch.int32, device="cuda")
    tri = flat[:B * capacity * 3].view(B, capacity, 3)
    count = torch.full((B,), POISON, dtype=torch.int32, device="cuda")
    m = torch.from_numpy(masks).cuda()
    d = None if depth is None else torch.from_numpy(depth).cuda()
    hip.mesh_triangles(B, h, w, tri, count, mask=m, row_pitch=w, image_stride=h * w, depth=d, inverse=inverse, max_ratio=max_ratio)
    return tri, count, flat[B * capacity * 3:]


@pytest.mark.parametrize("capacity", [0, 1, 1000, 4097])
def test_triangles_overflow_keeps_the_first_rows_the_true_count_and_the_guard(hip, capacity):
    h, w = 70, 130
    masks = np.stack([_mask(h, w, 8, 0.9), _ellipse(h, w), _mask(h, w, 9, 0.3)])
    want = [R.triangles(h, w, m) for m in masks]
    assert want[0].shape[0] > 4097 > want[2].shape[0] > 1
    tri, count, guard = _raw_triangles(hip, masks, capacity)
    assert count.tolist() == [t.shape[0] for t in want]
    assert bool((guard == POISON).all())
    tri = tri.cpu().numpy()
    for b, t in enumerate(want):
        n = min(capacity, t.shape[0])
        assert np.array_equal(tri[b, :n], t[:n]) and (tri[b, n:] == POISON).all(), b      # rows from count on are untouched


def _ratio_map(h, w, seed):
    """A positive map with steps: many triangles on either side of the ratio rule, and cells whose z_max is exactly 2 z_min."""
    d = _depth(h, w, seed, 1.0, 1.2)
    d[:, w // 2:] *= np.float32(2.5)
    d[h // 3, :] *= np.float32(1.9)
    d[2:6, 2:6] = np.float32(1.5)
    d[3, 3], d[4, 4] = np.float32(3.0), np.float32(0.75)     # 3.0 == 2 * 1.5 and 1.5 == 2 * 0.75: kept at max_ratio = 2
    return d


@pytest.mark.parametrize("inverse", [None, (0.9, 0.1), (1.0, 0.0)])
def test_triangles_validity_and_ratio_rules(hip, inverse):
    from hip_ext import geometry as G
    h, w = 70, 130
    d = _ratio_map(h, w, 21)
    flat = d.reshape(-1)
    flat[np.random.default_rng(3).choice(h * w, 40, replace=False)] = np.tile(np.array([0.0, -1.0, np.inf, np.nan], np.float32), 10)
    if inverse is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(np.isfinite(d) & (d > 0), np.float32(1.0) / d, d).astype(np.float32)      # inverse depth in (0, 1]; the specials stay
    m = _mask(h, w, 22, 0.9)
    n_valid = _check_tri(G, h, w, None, d, inverse)
    n_masked = _check_tri(G, h, w, m, d, inverse)
    n_2 = _check_tri(G, h, w, m, d, inverse, 2.0)
    n_11 = _check_tri(G, h, w, m, d, inverse, 1.1)
    assert _check_tri(G, h, w, m, d, inverse, 0.0) == n_masked and _check_tri(G, h, w, m, d, inverse, -1.0) == n_masked
    assert 2 * (h - 1) * (w - 1) > n_valid > n_masked > n_2 > n_11 > 0


def test_triangle_with_z_max_exactly_at_the_ratio_is_kept(hip):
    from hip_ext import geometry as G
    d = np.full((6, 6), 1.5, np.float32)
    d[3, 3], d[1, 4] = 3.0, 0.75
    want = R.triangles(6, 6, depth=d, max_ratio=2.0)
    assert want.shape[0] == 50 and _same(G.create_triangles(6, 6, depth=d, max_ratio=2.0).cpu().numpy(), want)
    below = np.nextafter(np.float64(2.0), 0.0)
    assert _check_tri(G, 6, 6, None, d, None, below) == 50 - 12
    assert R.triangles(2, 2, depth=np.array([[1, 2], [2, 4]], np.float32), max_ratio=2.0).shape[0] == 2
    assert _check_tri(G, 2, 2, None, np.array([[1, 2], [2, 4]], np.float32), None, 2.0) == 2


# ------------------------------------------------------------------ compaction
def _compact_case(hip, masks, capacity, dtype, colors=True, vertex_capacity=None):
    """triangles (possibly overflowed) -> hip_ext.mesh_compact, against the restatement image by image."""
    B, h, w = masks.shape
    rng = np.random.default_rng(B * 100 + capacity)
    depth = np.stack([_depth(h, w, 30 + b) for b in range(B)])
    pts = np.stack([R.points(d) for d in depth]).astype(dtype).reshape(B, h * w, 3)
    cols = rng.integers(0, 256, size=(B, h * w, 3)).astype(np.uint8) if colors else None
    tri, count, guard = _raw_triangles(hip, masks, capacity)
    want_tri = [R.triangles(h, w, m)[:capacity] for m in masks]
    want = [R.compact(t, pts[b], None if cols is None else cols[b]) for b, t in enumerate(want_tri)]
    vcap = max(c[2] for c in want) + 3 if vertex_capacity is None else vertex_capacity
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    p_out = torch.full((B, vcap, 3), -5.0, dtype=tdt, device="cuda")
    c_out = torch.full((B, vcap, 3), 9, dtype=torch.uint8, device="cuda") if colors else None
    v_count = torch.full((B,), POISON, dtype=torch.int32, device="cuda")
    hip.mesh_compact(tri, count, h, w, torch.from_numpy(pts).cuda(), p_out, v_count, colors=None if cols is None else torch.from_numpy(cols).cuda(),
                     colors_out=c_out)
    assert v_count.tolist() == [c[2] for c in want] and bool((guard == POISON).all())
    tri, p_out = tri.cpu().numpy(), p_out.cpu().numpy()
    for b, (p, t, n, c) in enumerate(want):
        k = min(n, vcap)
        assert np.array_equal(tri[b, :t.shape[0]], t) and (tri[b, t.shape[0]:] == POISON).all(), b
        assert _same(p_out[b, :k], p[:k]) and (p_out[b, k:] == -5.0).all(), b
        if colors:
            co = c_out[b].cpu().numpy()
            assert np.array_equal(co[:k], c[:k]) and (co[k:] == 9).all(), b
    return [c[2] for c in want]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_compaction_points_triangles_counts_and_colours(hip, dtype):
    h, w = 70, 130
    masks = np.stack([_mask(h, w, 12, 0.8), _ellipse(h, w), np.ones((h, w), np.uint8)])
    n = _compact_case(hip, masks, 2 * (h - 1) * (w - 1), dtype)
    assert n[2] == h * w and 0 < n[1] < n[0] < h * w
    _compact_case(hip, masks, 2 * (h - 1) * (w - 1), dtype, colors=False)


def test_compaction_across_the_chunk_edges(hip):
    for h, w in [(2, hip.GEOM_CHUNK // 2), (2, hip.GEOM_CHUNK // 2 + 1), (33, 31), (32, 32), (3, 11)]:      # h w = CHUNK, CHUNK + 2, CHUNK - 1, CHUNK, 33
        _compact_case(hip, np.stack([_mask(h, w, h * w, 0.85), np.ones((h, w), np.uint8)]), 2 * (h - 1) * (w - 1), np.float32)


def test_compaction_after_an_overflowed_triangle_call(hip):
    h, w = 70, 130
    masks = np.stack([_mask(h, w, 12, 0.8), _ellipse(h, w), _mask(h, w, 9, 0.3)])
    n = _compact_case(hip, masks, 1000, np.float64)
    assert all(0 < v <= 3000 for v in n)


def test_compaction_vertex_capacity_overflow_reports_the_true_count(hip):
    h, w = 37, 61
    _compact_case(hip, np.stack([_mask(h, w, 1, 0.9), _ellipse(h, w)]), 2 * (h - 1) * (w - 1), np.float32, vertex_capacity=100)


def test_compaction_of_an_empty_triangle_list(hip):
    h, w = 37, 61
    y, x = np.mgrid[0:h, 0:w]
    n = _compact_case(hip, np.stack([np.zeros((h, w), np.uint8), ((y + x) % 2).astype(np.uint8)]), 64, np.float32)
    assert n == [0, 0]
    n = _compact_case(hip, np.ones((1, 1, 9), np.uint8), 0, np.float64, vertex_capacity=0)      # a grid one pixel high, no capacity at all
    assert n == [0]


def test_depth_to_mesh_equals_the_restatement(hip):
    from hip_ext import geometry as G
    h, w = 70, 130
    d = _ratio_map(h, w, 5)
    d[10, 10] = np.nan
    m = _ellipse(h, w)
    cols = np.random.default_rng(1).integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    for compact in (True, False):
        got = G.depth_to_mesh(d, mask=m, colors=cols, compact=compact, max_ratio=2.0)
        want = R.depth_to_mesh(d, m, cols, compact, max_ratio=2.0)
        assert (got.vertex_count, got.triangle_count) == (want.vertex_count, want.triangle_count) and got.triangle_count > 0
        assert _same(got.points.cpu().numpy(), want.points) and _same(got.triangles.cpu().numpy(), want.triangles)
        assert _same(got.colors.cpu().numpy(), want.colors)
    got = G.depth_to_mesh(d, mask=m, dtype=torch.float64, inverse=(0.9, 0.1))
    want = R.depth_to_mesh(d, m, inverse=(0.9, 0.1), dtype=np.float64)
    assert got.colors is None and _same(got.points.cpu().numpy(), want.points) and _same(got.triangles.cpu().numpy(), want.triangles)


# ------------------------------------------------------------------ determinism, capture
def test_two_runs_give_byte_identical_buffers(hip):
    h, w = 257, 300
    masks = np.stack([_mask(h, w, 40, 0.7), _mask(h, w, 41, 0.6)])
    depth = np.stack([_ratio_map(h, w, 42), _ratio_map(h, w, 43)])
    runs = []
    for _ in range(2):
        tri, count, _g = _raw_triangles(hip, masks, 90000, depth=depth, max_ratio=2.0)
        pts = torch.from_numpy(np.stack([R.points(d) for d in depth]).reshape(2, h * w, 3)).cuda()
        p_out = torch.zeros(2, h * w, 3, dtype=torch.float64, device="cuda")
        v_count = torch.zeros(2, dtype=torch.int32, device="cuda")
        hip.mesh_compact(tri, count, h, w, pts, p_out, v_count)
        runs.append([t.cpu().numpy().tobytes() for t in (tri, count, p_out, v_count)])
    assert runs[0] == runs[1]
    assert all(0 < c for c in count.tolist())


def test_capture_replays_with_a_new_mask_and_depth(hip):
    """A straight-line capture of the triangle and compaction calls; replayed after new contents were copied in, it gives the new contents' result."""
    h, w, cap = 70, 130, 20000
    draw = lambda s: (_mask(h, w, s, 0.5 + 0.1 * s), _ratio_map(h, w, 50 + s))
    m0, d0 = draw(0)
    mask, depth = torch.from_numpy(m0[None]).cuda(), torch.from_numpy(d0[None]).cuda()
    pts = torch.empty(1, h * w, 3, dtype=torch.float32, device="cuda")
    tri = torch.empty(1, cap, 3, dtype=torch.int32, device="cuda")
    count, v_count = torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    p_out = torch.empty(1, h * w, 3, dtype=torch.float32, device="cuda")
    ws_t = torch.empty(hip.mesh_triangles_workspace_bytes(1, h, w) // 4, dtype=torch.int32, device="cuda")
    ws_c = torch.empty(hip.mesh_compact_workspace_bytes(1, h, w) // 4, dtype=torch.int32, device="cuda")
    from hip_ext import geometry as G
    cam = G._camera("test", h, w, None, None, None, 55.0)

    def run():
        hip.depth_points(depth, cam, out_f32=pts.view(1, h, w, 3))
        hip.mesh_triangles(1, h, w, tri, count, mask=mask, row_pitch=w, image_stride=h * w, depth=depth, max_ratio=2.0, workspace=ws_t)
        hip.mesh_compact(tri, count, h, w, pts, p_out, v_count, workspace=ws_c)

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
        m1, d1 = draw(s)
        mask.copy_(torch.from_numpy(m1[None]))
        depth.copy_(torch.from_numpy(d1[None]))
        tri.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        want = R.depth_to_mesh(d1, m1, max_ratio=2.0)
        assert (count.item(), v_count.item()) == (want.triangle_count, want.vertex_count) and 0 < want.triangle_count < cap
        assert _same(tri[0, :want.triangle_count].cpu().numpy(), want.triangles) and bool((tri[0, want.triangle_count:] == POISON).all())
        assert _same(p_out[0, :want.vertex_count].cpu().numpy(), want.points)


# ------------------------------------------------------------------ amodal_layers
def test_amodal_layers_of_a_synthetic_result(hip):
    from hip_ext import geometry as G
    from hip_ext.pipeline import AmodalResult
    h, w = 56, 70
    rng = np.random.default_rng(8)
    base = (0.15 + 0.7 * np.arange(w)[None, :] / w + 0.05 * rng.random((h, w))).astype(np.float32)      # a slope with some roughness
    base[5, 7], base[30, 40] = 0.0, 1.0                       # a min-max normalised map holds both exactly
    masks = np.zeros((2, h, w), np.float32)
    masks[0] = _ellipse(h, w)
    blended = np.stack([np.where(masks[0] > 0, np.float32(0.8) * base + np.float32(0.1), base), base]).astype(np.float32)
    image = rng.integers(0, 256, size=(2 * h, 3 * w, 3)).astype(np.uint8)
    res = AmodalResult(torch.from_numpy(base).cuda(), None, torch.from_numpy(blended).cuda(), torch.from_numpy(masks).cuda(), None)

    def same_mesh(got, want):
        assert (got.vertex_count, got.triangle_count) == (want.vertex_count, want.triangle_count)
        assert _same(got.points.cpu().numpy(), want.points) and _same(got.triangles.cpu().numpy(), want.triangles)
        assert (got.colors is None) == (want.colors is None) and (got.colors is None or _same(got.colors.cpu().numpy(), want.colors))

    for kw in (dict(), dict(image=image, max_ratio=1.1), dict(near=1.0, far=float("inf"))):
        got = G.amodal_layers(res, **kw)
        want = R.amodal_layers(base, blended, masks, **kw)
        same_mesh(got.scene, want.scene)
        assert len(got.objects) == 2
        for g, t in zip(got.objects, want.objects):
            same_mesh(g, t)
        empty = got.objects[1]                                   # the all-zero mask
        assert (empty.vertex_count, empty.triangle_count) == (0, 0) and tuple(empty.points.shape) == (0, 3) and tuple(empty.triangles.shape) == (0, 3)
        assert 0 < got.objects[0].triangle_count < got.scene.triangle_count
    # with far = inf the pixel at base == 0 has no finite z: an invalid vertex, in no triangle -- the finite-far scene uses every vertex
    assert G.amodal_layers(res).scene.vertex_count == h * w
    scene = G.depth_to_mesh(res.base, inverse=(1.0, 0.0), compact=False)
    valid = G.depth_to_points(res.base, inverse=(1.0, 0.0), return_valid=True)[1].cpu().numpy()
    assert valid[5, 7] == 0 and valid.sum() == h * w - 1
    assert not bool((scene.triangles == 5 * w + 7).any()) and bool(torch.isnan(scene.points[5 * w + 7]).all())
    assert G.amodal_layers(res, near=1.0, far=float("inf")).scene.vertex_count == h * w - 1


# ------------------------------------------------------------------ command line
def test_depth_to_mesh_command_line_on_the_device(hip, tmp_path):
    """A 16-bit inverse-depth PNG, a mask and a photo in, a PLY out whose vertices, triangles and colours equal the restatement's."""
    from PIL import Image

    import test_geometry_cpu as C
    from src.scripts import depth_to_mesh as S
    rng = np.random.default_rng(17)
    h, w = 37, 53
    v = (20000 + 30000 * np.arange(w)[None, :] / w + 1500 * rng.random((h, w))).astype(np.uint16)
    v[19, 24] = 0                                      # far behind its neighbours, inside the mask: the ratio rule cuts its six triangles
    mask = _ellipse(h, w) * np.uint8(255)
    photo = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    Image.fromarray(v).save(tmp_path / "d.png")
    Image.fromarray(mask).save(tmp_path / "m.png")
    Image.fromarray(photo).save(tmp_path / "p.png")
    args = [str(tmp_path / "d.png"), str(tmp_path / "o.ply"), "--mask", str(tmp_path / "m.png"), "--image", str(tmp_path / "p.png"),
            "--inverse", "0.5", "20", "--max_ratio", "1.2", "--fov", "62.5"]
    assert S.main(args) == 0
    depth = (v.astype(np.float64) / 65535.0).astype(np.float32)
    want = R.depth_to_mesh(depth, mask > 0, photo, inverse=(1.0 / 0.5 - 1.0 / 20, 1.0 / 20), max_ratio=1.2, fov_deg=62.5)
    p, t, c = C._read_ply(tmp_path / "o.ply")
    assert want.triangle_count == R.triangles(h, w, mask).shape[0] - 6 and 0 < want.vertex_count < h * w
    assert _same(p, want.points) and _same(t, want.triangles) and _same(c, want.colors)
