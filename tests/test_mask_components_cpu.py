"""CPU: the numpy restatement the GPU mask-component tests compare against (tests/_components_ref.py) is pinned against scipy.ndimage -- labels
identical INCLUDING the numbering (raster order of each component's first pixel) -- and the host surface of hip_ext.masks: the four exports under
ABI 10, no CPU fallback, argument validation."""
import os
import re

import numpy as np
import pytest
import torch

import _components_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ada_hip.h")
NEW_EXPORTS = ("ada_mask_label_fwd", "ada_mask_stats_fwd", "ada_mask_keep_area_fwd", "ada_mask_grid_points_fwd")
DENSITIES = (0.3, 0.5, 0.59, 0.7)
STRUCTURE = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1], [1, 1, 1], [1, 1, 1]]}


def _random_cases(n):
    rng = np.random.default_rng(2024)
    for k in range(n):
        h, w = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        yield k, R.random_mask(h, w, DENSITIES[k % 4], 1000 + k)


def test_restatement_labels_equal_scipy_including_the_numbering():
    ndi = pytest.importorskip("scipy.ndimage")
    checked = 0
    for k, m in _random_cases(240):
        for conn in (4, 8):
            want, n_want = ndi.label(m, structure=STRUCTURE[conn])
            got, n_got = R.label(m, conn)
            assert n_got == n_want and np.array_equal(got, want), (k, m.shape, conn)
            checked += 1
    assert checked >= 400


def test_restatement_stats_sums_and_filter_equal_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for k, m in _random_cases(60):
        for conn in (4, 8):
            lab, n = R.label(m, conn)
            st, sums = R.stats(lab, n)
            yy, xx = np.mgrid[:m.shape[0], :m.shape[1]]
            for i, sl in enumerate(ndi.find_objects(lab), start=1):
                assert tuple(st[i, :4]) == (sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start)
            idx = np.arange(1, n + 1)
            assert np.array_equal(st[1:, 4], ndi.sum(np.ones_like(lab), lab, idx).astype(np.int64))
            assert np.array_equal(sums[1:, 0], ndi.sum(xx, lab, idx).astype(np.int64)) and np.array_equal(sums[1:, 1], ndi.sum(yy, lab, idx).astype(np.int64))
            assert st[0, 4] == int((lab == 0).sum()) and st[:, 4].sum() == lab.size
            area = np.concatenate([[0], st[1:, 4]])
            assert np.array_equal(R.keep_area(m, 5, conn), ((area >= 5)[lab] & (lab > 0)).astype(np.uint8))


def test_restatement_counts_of_the_structured_masks():
    s = R.serpentine(65)
    assert int(s.sum()) == 2177 and R.label(s, 4)[1] == 1 and R.label(s, 8)[1] == 1
    c = R.checkerboard(66, 130)
    assert R.label(c, 4)[1] == 4290 and R.label(c, 8)[1] == 1
    d = np.eye(37, dtype=np.uint8)
    assert R.label(d, 8)[1] == 1 and R.label(d, 4)[1] == 37
    for c0 in (7, 15, 31, 63):
        for anti in (False, True):
            blocks = R.diagonal_blocks(70, c0, anti)
            assert R.label(blocks, 8)[1] == 1 and R.label(blocks, 4)[1] == 2
    assert R.label(R.comb(40, 67), 4)[1] == 1
    assert R.label(np.zeros((5, 7), np.uint8), 8) [1] == 0


def test_restatement_point_rule_on_hand_checked_masks():
    m = np.zeros((40, 60), np.uint8)
    m[2:5, 3:6] = 1                      # 9 pixels: small, centroid (4, 3)
    m[10:30, 10:45] = 1                  # 700 pixels: grid rows 10, 20 (29 excluded), columns 10, 20, 30, 40
    want = [[4, 3]] + [[x, y] for y in (10, 20) for x in (10, 20, 30, 40)]
    assert R.points(m).tolist() == want
    line = np.zeros((160, 9), np.uint8)
    line[5:155, 4] = 1                   # 150 pixels, one wide: range(4, 4, step) is empty
    assert R.points(line).shape == (0, 2)
    assert R.points(np.zeros((8, 8), np.uint8)).shape == (0, 2) and R.points(np.zeros((8, 8), np.uint8)).dtype == np.int32


def test_header_declares_the_four_exports_under_abi_10():
    import hip_ext
    header = open(HEADER).read()
    assert re.search(r"#define\s+ADA_ABI_VERSION\s+10\b", header) and hip_ext.ABI_VERSION == 10
    for name in NEW_EXPORTS:
        assert name in hip_ext.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    lib = hip_ext.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    build_py = open(os.path.join(ROOT, "amodal-depth-anything_amd", "csrc", "build.py")).read()
    no_scratch = re.search(r"^NO_SCRATCH\s*=\s*\{([^}]*)\}", build_py, flags=re.M).group(1)
    assert '"ada_masks.hip"' in no_scratch and '"ada_masks.hip"' in re.search(r"^SOURCES\s*=\s*\[([^\]]*)\]", build_py, flags=re.M).group(1)


def test_cpu_inputs_raise_hipexterror():
    from hip_ext import HipExtError
    from hip_ext import masks as M
    m = np.zeros((6, 7), np.uint8)
    for call in (lambda x, **kw: M.connected_components(x, **kw), lambda x, **kw: M.remove_small_noise(x, **kw),
                 lambda x, **kw: M.points_from_components(x, **kw)):
        with pytest.raises(HipExtError, match="no CPU fallback"):
            call(m, device="cpu")
        with pytest.raises(HipExtError, match="no CPU fallback"):
            call(torch.from_numpy(m))
        with pytest.raises(HipExtError, match="no CPU fallback"):
            call(torch.from_numpy(m > 0))
    if not torch.cuda.is_available():
        with pytest.raises(HipExtError, match="no CPU fallback"):
            M.remove_small_noise(m)
    import hip_ext
    with pytest.raises(HipExtError):
        hip_ext.mask_stats(torch.zeros(1, 4, 4, dtype=torch.int32), 3, torch.zeros(1, 4, 5, dtype=torch.int32), torch.zeros(1, 4, 2, dtype=torch.int64))


def test_argument_validation():
    from hip_ext import masks as M
    m = np.zeros((6, 7), np.uint8)
    for bad in (6, 0, "8", 4.0, True, None):
        with pytest.raises(ValueError, match="connectivity"):
            M.connected_components(m, connectivity=bad, device="cpu")
        with pytest.raises(ValueError, match="connectivity"):
            M.remove_small_noise(m, connectivity=bad, device="cpu")
        with pytest.raises(ValueError, match="connectivity"):
            M.points_from_components(m, connectivity=bad, device="cpu")
    with pytest.raises(ValueError, match="max_labels"):
        M.connected_components(m, max_labels=-1, device="cpu")
    with pytest.raises(ValueError, match="min_area"):
        M.remove_small_noise(m, min_area=-3, device="cpu")
    with pytest.raises(ValueError, match="min_area"):
        M.remove_small_noise(m, min_area=2.5, device="cpu")
    with pytest.raises(ValueError, match="grid_step"):
        M.points_from_components(m, grid_step=0, device="cpu")
    with pytest.raises(ValueError, match="small_component_thresh"):
        M.points_from_components(m, small_component_thresh=-1, device="cpu")
    with pytest.raises(TypeError, match="uint8 or bool"):
        M.connected_components(m.astype(np.float32), device="cpu")
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        M.remove_small_noise([[0, 1]], device="cpu")
    for shape in ((7,), (2, 3, 4, 5), (0, 5)):
        with pytest.raises(ValueError, match="expected"):
            M.connected_components(np.zeros(shape, np.uint8), device="cpu")


def test_amodal_infer_image_takes_min_area_and_defaults_to_none():
    import inspect
    from hip_ext.pipeline import amodal_infer_image
    p = inspect.signature(amodal_infer_image).parameters
    assert p["min_area"].default is None and p["min_area_connectivity"].default == 4
