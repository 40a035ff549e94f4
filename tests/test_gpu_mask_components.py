"""GPU: connected components of masks on the device (csrc/ada_masks.hip through hip_ext.masks) against the numpy restatement
tests/_components_ref.py, which test_mask_components_cpu.py pins against scipy.ndimage.  Integer work: every comparison is np.array_equal.
The shapes straddle the kernels' 32 x 32 tile, 1024-pixel chunk and 64-pixel strip; the contents are the ones a union-find can get wrong --
long winding chains, thousands of single-pixel components, pairs that touch only diagonally across every tile corner, joins in the last row."""
import functools

import numpy as np
import pytest
import torch

import _components_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 67), (67, 1), (37, 53), (64, 64), (65, 65), (130, 70), (257, 129)]
DENSITIES = (0.3, 0.5, 0.59, 0.7)


@functools.lru_cache(maxsize=None)
def _ref_label_cached(key, conn):
    return R.label(_MASKS[key], conn)


_MASKS = {}


def _ref_label(mask, conn):
    key = (mask.shape, mask.tobytes())
    _MASKS[key] = mask
    return _ref_label_cached(key, conn)


def _contents(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    mixed = R.random_mask(h, w, 0.55, h + w) * rng.choice(np.array([1, 128, 255], np.uint8), size=(h, w))
    return [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)] + [R.random_mask(h, w, d, h * 31 + w + i) for i, d in enumerate(DENSITIES)] + [mixed]


def _check_labels(M, masks, conn):
    """One call on the stack ``masks`` [K, h, w]; labels and counts against the restatement of every mask."""
    comp = M.connected_components(np.stack(masks), connectivity=conn, stats=False)
    assert comp.labels.dtype == torch.int32 and comp.count.dtype == torch.int32 and comp.stats is None and comp.centroids is None
    labels, count = comp.labels.cpu().numpy(), comp.count.cpu().numpy()
    for k, m in enumerate(masks):
        want, n = _ref_label(m, conn)
        assert count[k] == n, (k, conn, int(count[k]), n)
        assert np.array_equal(labels[k], want), (k, conn, int((labels[k] != want).sum()))


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("hw", SHAPES)
def test_labels_equal_the_restatement_on_constant_random_and_mixed_byte_masks(hip, hw, conn):
    from hip_ext import masks as M
    _check_labels(M, _contents(*hw), conn)


@pytest.mark.parametrize("conn", [4, 8])
def test_labels_at_518(hip, conn):
    from hip_ext import masks as M
    _check_labels(M, [R.random_mask(518, 518, 0.59, 7), R.ellipse(518, 518, 280, 230, 120, 150)], conn)


def _chunk_scan_step():
    """Chunk counts that one step of the labelling's scan takes: 1024 threads times the items per thread that csrc/ada_masks.hip instantiates."""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amodal-depth-anything_amd", "csrc", "ada_masks.hip")
    return 1024 * int(re.search(r"constexpr int CC_SCAN_ITEMS = (\d+);", open(src).read()).group(1))


@pytest.mark.parametrize("steps,more", ((1, -1), (1, 0), (1, 1), (2, 1)), ids=("step-1", "step", "step+1", "2step+1"))
def test_labels_where_the_chunk_scan_carries_between_steps(hip, steps, more):
    """A row of 1024 pixels is one chunk of the root count, so the rows are the sums of the scan: one short of a step, a step, one more (the first
    carry) and two steps and one (a carry into a carry).  Isolated pixels only -- a seeded half of the lattice [::2, ::2], each its own component under
    either connectivity -- so a chunk's count differs from its neighbours' and the labels are the running count of the mask in raster order."""
    from hip_ext import masks as M
    h, w = steps * _chunk_scan_step() + more, 1024
    mask = np.zeros((h, w), np.uint8)
    mask[::2, ::2] = np.random.default_rng(h).random(((h + 1) // 2, w // 2)) < 0.5
    want = np.cumsum(mask.ravel(), dtype=np.int64).reshape(h, w) * mask
    per_chunk = mask.sum(axis=1)
    assert per_chunk.min() < per_chunk.max() and int(want.max()) == int(mask.sum()) < 2 ** 31
    for conn in (4, 8):
        comp = M.connected_components(mask, connectivity=conn, stats=False)
        assert comp.count.tolist() == [int(mask.sum())], conn
        assert np.array_equal(comp.labels[0].cpu().numpy(), want), conn


@pytest.mark.parametrize("conn", [4, 8])
def test_labels_of_the_structured_masks(hip, conn):
    from hip_ext import masks as M
    comp = M.connected_components(R.serpentine(65), connectivity=conn, stats=False)
    assert comp.count.tolist() == [1] and int((comp.labels == 1).sum()) == 2177
    _check_labels(M, [R.serpentine(65)], conn)
    _check_labels(M, [R.serpentine(130)], conn)                     # the long chain: 65 rows of 130 joined end to end
    board = R.checkerboard(66, 130)
    _check_labels(M, [board, 1 - board], conn)
    assert M.connected_components(board, connectivity=conn, stats=False).count.tolist() == [4290 if conn == 4 else 1]
    eye = np.eye(67, dtype=np.uint8)
    _check_labels(M, [eye, np.ascontiguousarray(eye[:, ::-1])], conn)
    assert M.connected_components(eye, connectivity=conn, stats=False).count.tolist() == [67 if conn == 4 else 1]
    blocks = [R.diagonal_blocks(70, c, anti) for c in (7, 15, 31, 63) for anti in (False, True)]
    _check_labels(M, blocks, conn)
    assert M.connected_components(np.stack(blocks), connectivity=conn, stats=False).count.tolist() == [2 if conn == 4 else 1] * 8
    _check_labels(M, [R.comb(67, 131), np.ascontiguousarray(R.comb(67, 131)[::-1])], conn)


def test_a_batch_of_different_masks_and_a_pitched_crop_read_in_place(hip):
    from hip_ext import masks as M
    h, w = 70, 97
    masks = [R.random_mask(h, w, 0.59, 3), R.serpentine(97)[:h], R.checkerboard(h, w)]
    for conn in (4, 8):
        _check_labels(M, masks, conn)
    big = torch.zeros(3, h + 9, w + 30, dtype=torch.uint8, device="cuda")
    big[:, 4:4 + h, 11:11 + w] = torch.from_numpy(np.stack(masks)).cuda() * 255
    big[:, :4] = 1                                                   # whatever surrounds the crop must not leak in
    big[:, :, :11] = 1
    big[:, 4 + h:] = 1
    big[:, :, 11 + w:] = 1
    crop = big[:, 4:4 + h, 11:11 + w]
    assert not crop.is_contiguous()
    for conn in (4, 8):
        got = M.connected_components(crop, connectivity=conn, stats=False)
        one = M.connected_components(crop[1], connectivity=conn, stats=False)       # [h, w], a pitched view too
        boolean = M.connected_components(crop > 0, connectivity=conn, stats=False)
        for k, m in enumerate(masks):
            assert np.array_equal(got.labels[k].cpu().numpy(), _ref_label(m, conn)[0])
        assert torch.equal(one.labels[0], got.labels[1]) and torch.equal(boolean.labels, got.labels) and torch.equal(boolean.count, got.count)


def test_stats_sums_centroids_and_the_background_row(hip):
    from hip_ext import masks as M
    masks = [R.random_mask(130, 70, 0.5, 11), R.ellipse(130, 70, 60, 30, 40, 25), np.ones((130, 70), np.uint8), np.zeros((130, 70), np.uint8)]
    for conn in (4, 8):
        comp = M.connected_components(np.stack(masks), connectivity=conn)
        counts = comp.count.tolist()
        cap = max(counts)
        assert comp.stats.shape == (4, cap + 1, 5) and comp.stats.dtype == torch.int32
        assert comp.centroids.shape == (4, cap + 1, 2) and comp.centroids.dtype == torch.float64
        for k, m in enumerate(masks):
            lab, n = _ref_label(m, conn)
            st, sums = R.stats(lab, cap)
            assert counts[k] == n and np.array_equal(comp.stats[k].cpu().numpy(), st), (k, conn)
            cen = comp.centroids[k].cpu().numpy()
            has = st[:, 4] > 0
            assert np.array_equal(cen[has], sums[has] / st[has, 4:5].astype(np.float64)) and np.isnan(cen[~has]).all()
        assert comp.stats[2, 0].tolist() == [0, 0, 0, 0, 0]                 # an empty background: all zeros by this library's definition
        assert comp.stats[2, 1].tolist() == [0, 0, 70, 130, 130 * 70]
        assert comp.stats[3, 0].tolist() == [0, 0, 70, 130, 130 * 70]       # an empty mask: the background is everything


@pytest.mark.parametrize("conn", [4, 8])
def test_stats_where_labels_alternate_along_a_row(hip, conn):
    """The run walker keeps the background and the two most recent components per 64-pixel strip and merges a wave's strips by label: a checkerboard
    (two labels alternating under 8, a new label every other pixel under 4), noise around one giant component, a comb and a serpentine, several
    strips per row and several rows per wave."""
    from hip_ext import masks as M
    h, w = 67, 257
    masks = [R.checkerboard(h, w), R.random_mask(h, w, 0.59, 17), R.comb(h, w), R.serpentine(257)[:h], R.random_mask(h, w, 0.3, 18)]
    comp = M.connected_components(np.stack(masks), connectivity=conn)
    cap = int(comp.count.max())
    for k, m in enumerate(masks):
        lab, n = _ref_label(m, conn)
        st, sums = R.stats(lab, cap)
        assert int(comp.count[k]) == n and np.array_equal(comp.stats[k].cpu().numpy(), st), (k, conn)
        has = st[:, 4] > 0
        assert np.array_equal(comp.centroids[k].cpu().numpy()[has], sums[has] / st[has, 4:5].astype(np.float64)), (k, conn)
        for min_area in (1, 2, 30):
            assert np.array_equal(M.remove_small_noise(m, min_area=min_area, connectivity=conn)[0].cpu().numpy(), R.keep_area(m, min_area, conn)), (k, conn, min_area)


def test_stats_below_capacity_keep_the_count_true_and_write_nothing_past_their_rows(hip):
    import hip_ext
    from hip_ext import masks as M
    m = R.random_mask(65, 65, 0.3, 5)
    lab, n = _ref_label(m, 8)
    cap = 7
    assert n > 3 * cap
    comp = M.connected_components(m, connectivity=8, max_labels=cap)
    st, sums = R.stats(lab, cap)
    assert comp.count.tolist() == [n] and comp.stats.shape == (1, cap + 1, 5)
    assert np.array_equal(comp.stats[0].cpu().numpy(), st)
    # the raw exports on guarded buffers: rows 0..cap are written, the words behind them keep the sentinel
    guard_i = torch.full(((cap + 1) * 5 + 64,), -77, dtype=torch.int32, device="cuda")
    guard_l = torch.full(((cap + 1) * 2 + 64,), -77, dtype=torch.int64, device="cuda")
    hip_ext.mask_stats(comp.labels, cap, guard_i[:(cap + 1) * 5].view(1, cap + 1, 5), guard_l[:(cap + 1) * 2].view(1, cap + 1, 2))
    assert np.array_equal(guard_i[:(cap + 1) * 5].view(cap + 1, 5).cpu().numpy(), st) and np.array_equal(guard_l[:(cap + 1) * 2].view(cap + 1, 2).cpu().numpy(), sums)
    assert bool((guard_i[(cap + 1) * 5:] == -77).all()) and bool((guard_l[(cap + 1) * 2:] == -77).all())
    zero = M.connected_components(m, connectivity=8, max_labels=0)
    assert zero.stats.shape == (1, 1, 5) and zero.stats[0, 0].tolist() == st[0].tolist() and zero.count.tolist() == [n]


def test_remove_small_noise_keeps_exactly_min_area(hip):
    from hip_ext import masks as M
    m = np.zeros((70, 97), np.uint8)
    m[3:8, 4:14] = 255                   # 50 pixels
    m[20:27, 30:37] = 1                  # 49 pixels
    m[40, 50] = 1                        # two specks touching diagonally: one component of 2 under 8, two of 1 under 4
    m[41, 51] = 1
    m[60:62, 90:97] = 7                  # 14 pixels at the border
    for conn in (4, 8):
        got = M.remove_small_noise(m, min_area=50, connectivity=conn)
        assert got.dtype == torch.uint8 and got.shape == (1, 70, 97)
        want = np.zeros_like(m)
        want[3:8, 4:14] = 1
        assert np.array_equal(got[0].cpu().numpy(), want) and np.array_equal(want, R.keep_area(m, 50, conn))
        assert np.array_equal(M.remove_small_noise(m, min_area=49, connectivity=conn)[0].cpu().numpy(), R.keep_area(m, 49, conn))
    two8 = M.remove_small_noise(m, min_area=2, connectivity=8)[0].cpu().numpy()
    two4 = M.remove_small_noise(m, min_area=2, connectivity=4)[0].cpu().numpy()
    assert two8[40, 50] == 1 and two8[41, 51] == 1 and two4[40, 50] == 0 and two4[41, 51] == 0
    assert np.array_equal(two8, R.keep_area(m, 2, 8)) and np.array_equal(two4, R.keep_area(m, 2, 4))
    assert np.array_equal(M.remove_small_noise(m, min_area=0)[0].cpu().numpy(), (m > 0).astype(np.uint8))
    # any number of components: a checkerboard's 4290 singletons and a noisy stack, defaults of the reference (500, 4-connectivity)
    board = R.checkerboard(66, 130)
    assert not bool(M.remove_small_noise(board, min_area=2, connectivity=4).any())
    assert np.array_equal(M.remove_small_noise(board, min_area=2, connectivity=8)[0].cpu().numpy(), board)
    noisy = np.stack([R.random_mask(257, 129, d, 40 + i) for i, d in enumerate(DENSITIES)])
    got = M.remove_small_noise(noisy).cpu().numpy()
    for k in range(4):
        assert np.array_equal(got[k], R.keep_area(noisy[k])), k


def _points_cases():
    ell = R.ellipse(518, 518, 280, 230, 120, 150)             # semi-axes 150 (x) / 120 (y) at (x, y) = (230, 280)
    hundred = np.zeros((40, 60), np.uint8)
    hundred[5:15, 7:17] = 1                                     # exactly 100 pixels: large (the test is <); 99 beside it: small
    hundred[20:29, 30:41] = 1
    narrow = np.zeros((80, 60), np.uint8)
    narrow[10:70, 20:27] = 1                                    # 420 pixels, bounding box 7 wide: one grid column
    line = np.zeros((170, 40), np.uint8)
    line[10:160, 21] = 1                                        # 150 pixels, one wide: no point at all
    cshape = np.zeros((30, 30), np.uint8)
    cshape[5:16, 5:16] = 1
    cshape[7:14, 7:16] = 0                                      # a C of 58 pixels: its centroid falls in the hole
    mixed = R.random_mask(130, 70, 0.45, 77)
    return dict(ellipse=ell, hundred=hundred, narrow=narrow, line=line, cshape=cshape, twins=_same_centroid(), mixed=mixed, empty=np.zeros((33, 65), np.uint8))


def _same_centroid():
    """A 3-pixel bar with centroid (21, 10) and, around it without touching under 8-connectivity, a hollow frame whose centroid is (21, 10) too."""
    m = np.zeros((30, 40), np.uint8)
    m[10, 20:23] = 1
    m[7, 18:25] = 1
    m[13, 18:25] = 1
    m[7:14, 18] = 1
    m[7:14, 24] = 1
    return m


def test_points_from_components_equal_the_transcribed_rule(hip):
    from hip_ext import masks as M
    cases = _points_cases()
    for name, m in cases.items():
        got = M.points_from_components(m)
        assert len(got) == 1 and got[0].dtype == torch.int32 and got[0].dim() == 2 and got[0].shape[1] == 2 and got[0].is_cuda, name
        want = R.points(m)
        assert np.array_equal(got[0].cpu().numpy(), want), (name, got[0].shape, want.shape)
    assert R.points(cases["ellipse"]).shape == (557, 2)
    assert R.points(cases["line"]).shape == (0, 2) and R.points(cases["empty"]).shape == (0, 2)
    assert tuple(M.points_from_components(cases["empty"])[0].shape) == (0, 2)
    hundred = R.points(cases["hundred"]).tolist()
    assert hundred == [[7, 5]] + [[35, 24]], hundred                        # 100 pixels: one grid point (range(5, 14, 10) x range(7, 16, 10)); 99: the centroid
    assert R.points(cases["narrow"]).tolist() == [[20, y] for y in range(10, 69, 10)]
    c = R.points(cases["cshape"]).tolist()
    assert len(c) == 1 and cases["cshape"][c[0][1], c[0][0]] == 0             # the centroid lies outside its component
    assert R.points(cases["twins"]).tolist() == [[21, 10], [21, 10]]          # both emitted, frame first (its first pixel comes first)
    # other thresholds / steps / connectivity, and a stack with different point counts per mask
    for kw in (dict(small_component_thresh=5, grid_step=3, connectivity=4), dict(small_component_thresh=1, grid_step=1), dict(small_component_thresh=40, grid_step=7)):
        got = M.points_from_components(cases["mixed"], **kw)[0].cpu().numpy()
        assert np.array_equal(got, R.points(cases["mixed"], **kw)), kw
    stack = np.stack([cases["hundred"], np.zeros((40, 60), np.uint8), R.random_mask(40, 60, 0.5, 9)])
    got = M.points_from_components(stack)
    assert [tuple(g.shape) for g in got] == [R.points(s).shape for s in stack]
    for g, s in zip(got, stack):
        assert np.array_equal(g.cpu().numpy(), R.points(s))


def test_same_bytes_twice_on_a_side_stream_and_from_a_captured_graph(hip):
    import hip_ext
    from hip_ext import masks as M
    masks = np.stack([R.random_mask(257, 129, 0.59, 21), R.serpentine(257)[:, :129], R.checkerboard(257, 129)])
    dev = torch.from_numpy(masks).cuda()
    first = M.connected_components(dev, connectivity=8)
    again = M.connected_components(dev, connectivity=8)
    for a, b in zip(first[:3], again[:3]):
        assert torch.equal(a, b)
    clean = M.remove_small_noise(dev, min_area=30)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = M.connected_components(dev, connectivity=8)
        clean_side = M.remove_small_noise(dev, min_area=30)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(on_side.labels, first.labels) and torch.equal(on_side.count, first.count) and torch.equal(on_side.stats, first.stats)
    assert torch.equal(clean_side, clean)
    # the raw label call inside a stream capture: no host read, no allocation by the library; the replay gives the eager labels
    K, h, w = dev.shape
    labels = torch.zeros(K, h, w, dtype=torch.int32, device="cuda")
    count = torch.zeros(K, dtype=torch.int32, device="cuda")
    ws = torch.empty(hip_ext.mask_label_workspace_bytes(K, h, w) // 4, dtype=torch.int32, device="cuda")
    with torch.cuda.stream(side):
        hip_ext.mask_label(dev, K, h, w, dev.stride(1), dev.stride(0), 8, labels, count, ws)       # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip_ext.mask_label(dev, K, h, w, dev.stride(1), dev.stride(0), 8, labels, count, ws)
        cleaned = M.remove_small_noise(dev, min_area=30)
    labels.fill_(-5)
    count.fill_(-5)
    cleaned.fill_(9)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(labels, first.labels) and torch.equal(count, first.count) and torch.equal(cleaned, clean)


def test_raw_exports_reject_bad_arguments(hip):
    import hip_ext
    dev = torch.ones(1, 8, 8, dtype=torch.uint8, device="cuda")
    labels = torch.zeros(1, 8, 8, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(hip_ext.HipExtError, match="connectivity 6"):
        hip_ext.mask_label(dev, 1, 8, 8, 8, 64, 6, labels, count)
    small = torch.empty(16, dtype=torch.int32, device="cuda")
    with pytest.raises(hip_ext.HipExtError, match="workspace needs"):
        hip_ext.mask_label(dev, 1, 8, 8, 8, 64, 8, labels, count, small)
    with pytest.raises(hip_ext.HipExtError, match="workspace needs"):
        hip_ext.mask_keep_area(labels, 3, out_u8=torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"), workspace=small[:8])
    with pytest.raises(hip_ext.HipExtError, match="both None"):
        hip_ext.mask_keep_area(labels, 3)
    stats = torch.zeros(1, 2, 5, dtype=torch.int32, device="cuda")
    with pytest.raises(hip_ext.HipExtError, match="grid_step 0"):
        hip_ext.mask_grid_points(labels, stats, 100, 0, torch.zeros_like(labels))
    f32 = torch.zeros(1, 8, 8, dtype=torch.float32, device="cuda")
    hip_ext.mask_label(dev, 1, 8, 8, 8, 64, 4, labels, count)
    hip_ext.mask_keep_area(labels, 64, out_f32=f32)                       # the fp32 output alone: 0 / 1
    assert count.tolist() == [1] and bool((f32 == 1).all())
    hip_ext.mask_keep_area(labels, 65, out_f32=f32)
    assert bool((f32 == 0).all())
