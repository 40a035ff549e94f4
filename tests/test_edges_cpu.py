"""CPU side of the edge metrics: tests/_edges_ref.py (the plain-numpy restatement the GPU tests compare with) pinned against scipy.ndimage bit for
bit and against skimage.feature.canny where skimage exists, the reference's metric formulas on hand-derivable cases, the scenes of the end-to-end test,
and the surface the feature adds (exports, header, build flags, metric names, the runner's flag)."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import _edges_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "amodal-depth-anything_amd")
NEW_EXPORTS = ("ada_canny_fwd", "ada_canny_hysteresis_fwd", "ada_edt_fwd", "ada_edge_metric_fwd", "ada_soft_edge_fwd")
SHAPES = ((1, 1), (2, 2), (3, 3), (1, 67), (67, 1), (5, 4), (33, 41))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the restatement against scipy ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", (0.7, 1.0, 2.5))
def test_gaussian_is_scipys_bit_for_bit(sigma):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    for shape in SHAPES:
        a = (rng.standard_normal(shape) * 3).astype(np.float32)
        assert np.array_equal(_bits(ndi.gaussian_filter(a, sigma, mode="constant")), _bits(R.gaussian(a, sigma))), shape
    from hip_ext.edges import gaussian_weights
    assert np.array_equal(gaussian_weights(sigma), R.gaussian_weights(sigma))      # the weights the kernel is handed are the restatement's


def test_sobel_is_scipys_bit_for_bit_and_its_sign():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    for shape in SHAPES:
        a = (rng.standard_normal(shape) * 3).astype(np.float32)
        for axis in (0, 1):
            assert np.array_equal(_bits(ndi.sobel(a, axis=axis)), _bits(R.sobel(a, axis))), (shape, axis)
    ramp = np.tile(np.arange(5, dtype=np.float32), (5, 1))      # grows along axis 1: the derivative is positive, 2 * 4 in the interior
    assert R.sobel(ramp, 1)[2, 2] == 8.0 and ndi.sobel(ramp, axis=1)[2, 2] == 8.0 and R.sobel(ramp, 0)[2, 2] == 0.0


def test_hysteresis_labelling_and_edt_are_scipys():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for shape in SHAPES:
        lm = np.where(rng.random(shape) < 0.4, rng.uniform(0.05, 0.3, shape), 0).astype(np.float32)
        labels, count = ndi.label(lm > 0, np.ones((3, 3), bool))
        good = np.zeros(count + 1, bool)
        good[np.unique(labels[(lm > 0) & (lm >= np.float32(0.2))])] = True
        good[0] = False
        assert np.array_equal(good[labels].astype(np.uint8), R.hysteresis(lm, 0.2)), shape
        for density in (0.02, 0.3, 1.0):
            e = rng.random(shape) < density
            if e.any():
                assert np.array_equal(ndi.distance_transform_edt(~e), R.edt(e)), (shape, density)
    assert np.isinf(R.edt(np.zeros((3, 4), bool))).all()


def test_canny_is_skimages():
    """Skipped where skimage is missing -- until it has run somewhere, the restatement of the suppression is unpinned (tests/_edges_ref.py)."""
    feature = pytest.importorskip("skimage.feature")
    for shape, seeds in R.SEEDS.items():
        for seed in seeds:
            img = R.to_log(R.scene(seed, *shape))
            for sigma in (0.7, 1.0, 2.5):
                assert np.array_equal(feature.canny(img, sigma=sigma), R.canny(img, sigma).astype(bool)), (shape, seed, sigma)


# ---- the metric formulas ----------------------------------------------------------------------------------------------------------------------

def test_edge_acc_comp_by_hand():
    h, w = 24, 30
    pred, gt = np.zeros((h, w), bool), np.zeros((h, w), bool)
    pred[:, 10] = True
    gt[:, 13] = True
    valid = np.ones((h, w), bool)
    assert R.edge_acc_comp(pred, gt, valid) == (3.0, 3.0)                          # two parallel lines three pixels apart
    assert R.edge_acc_comp(np.zeros((h, w), bool), gt, valid) == (10.0, 10.0)      # empty prediction: both fall back
    assert R.edge_acc_comp(pred, gt, valid, 7, 9) == (3.0, 3.0) and R.edge_acc_comp(np.zeros((h, w), bool), gt, valid, 7, 9) == (7.0, 9.0)
    v = valid.copy()
    v[:, 13] = False                                                               # every ground-truth edge invalid: the empty mean
    acc, comp = R.edge_acc_comp(pred, gt, v)
    assert acc == 3.0 and math.isnan(comp)
    assert R.edge_acc_comp(pred, np.zeros((h, w), bool), valid) == (10.0, 10.0)    # no ground-truth edge: D_target = inf, nothing is close
    far = np.zeros((h, w), bool)
    far[:, 25] = True
    assert R.edge_acc_comp(pred, far, valid) == (10.0, 10.0)                       # 15 pixels apart: beyond the threshold


def test_soft_edge_error_by_hand():
    gt = np.zeros((6, 7), np.float32)
    gt[:, 3:] = 1.0
    pred = np.zeros((6, 7), np.float32)
    pred[:, 4:] = 1.0                                                              # the step one pixel off
    valid = np.ones((6, 7), bool)
    see0, m0 = R.soft_edge_error(pred, gt, valid, 0)
    assert see0.dtype == np.float32 and see0.sum() == 6.0 and m0 == 6.0 / 42.0
    see1, m1 = R.soft_edge_error(pred, gt, valid, 1)
    # radius 1 forgives the shift: every pixel finds its own value among its neighbours in gt
    assert see1.dtype == np.float32 and m1 == 0.0
    assert math.isnan(R.soft_edge_error(pred, gt, np.zeros((6, 7), bool), 1)[1])
    _, m5 = R.soft_edge_error(pred, gt, valid, 9)                                  # wider than the map: every shift exists, zeros everywhere outside
    assert m5 == 0.0


def test_step_ridge_is_kept_whole():
    img = np.zeros((12, 14), np.float32)
    img[:, 7:] = 1.0
    st = R.stages(img)
    assert (st["low_masked"][1:-1, 6] > 0).all() and (st["low_masked"][1:-1, 7] > 0).all()      # equal magnitudes on both sides: `<=` keeps both
    assert np.array_equal(st["magnitude"][1:-1, 6], st["magnitude"][1:-1, 7])
    assert not R.canny(np.full((9, 9), 0.5, np.float32)).any()                                # a constant: bleed-over only, no edge


# ---- the scenes of the end-to-end comparison --------------------------------------------------------------------------------------------------

def test_seeds_have_no_undecided_pixel():
    assert set(R.SEEDS) == {(33, 41), (47, 61)}
    for shape, seeds in R.SEEDS.items():
        assert len(seeds) == 3
        for seed in seeds:
            img = R.to_log(R.scene(seed, *shape))
            assert not R.undecided(img).any(), (shape, seed)
            assert int(R.canny(img).sum()) >= 30, (shape, seed)
    assert R.tau(np.zeros((2, 2), np.float32)) == 32 * 2.0 ** -23 and R.tau(np.full((2, 2), -4.0, np.float32)) == 128 * 2.0 ** -23


# ---- surface ----------------------------------------------------------------------------------------------------------------------------------

def test_exports_header_and_abi():
    import hip_ext
    header = open(os.path.join(ROOT, "include", "ada_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in hip_ext.EXPORTS, name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert hip_ext.ABI_VERSION == 10 and re.search(r"#define ADA_ABI_VERSION 10\b", header)
    assert hip_ext.CANNY_MAX_RADIUS == int(re.search(r"#define ADA_CANNY_MAX_RADIUS (\d+)", header).group(1))
    assert hip_ext.SOFT_EDGE_MAX_RADIUS == int(re.search(r"#define ADA_SOFT_EDGE_MAX_RADIUS (\d+)", header).group(1))
    assert hip_ext.EDGE_SUM_BLOCKS == int(re.search(r"#define ADA_EDGE_SUM_BLOCKS (\d+)", header).group(1))
    for wrapper in ("canny_front", "canny_hysteresis", "edt", "edge_metric_sums", "soft_edge", "canny_hysteresis_workspace_bytes", "edt_workspace_bytes"):
        assert callable(getattr(hip_ext, wrapper)), wrapper


def test_build_lists_the_new_source():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ada_csrc_build_edges", os.path.join(PKG, "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "ada_edges.hip" in mod.SOURCES and "ada_edges.hip" in mod.NO_SCRATCH
    assert "-ffp-contract=off" in mod.PER_FILE_FLAGS["ada_edges.hip"]
    assert os.path.exists(os.path.join(PKG, "csrc", "ada_edges.hip"))


def test_metric_module_offers_the_references_names():
    from src.util import metric
    for name in ("eps", "to_log", "to_inv", "extract_edges", "edge_metrics", "EdgeAcc", "EdgeComp", "soft_edge_error"):
        assert name in metric.__all__ and callable(getattr(metric, name)), name
    assert "Not built" not in metric.__doc__
    sig = inspect.signature(metric.EdgeAcc)
    assert list(sig.parameters) == ["pred", "gt", "valid_mask", "th_edges_acc", "th_edges_comp"] and sig.parameters["th_edges_acc"].default == 10
    assert list(inspect.signature(metric.extract_edges).parameters) == ["depth", "preprocess", "sigma", "mask", "use_canny"]
    assert inspect.signature(metric.soft_edge_error).parameters["radius"].default == 1
    import torch
    d = torch.tensor([[0.0, 1.0], [-2.0, 4.0]])
    assert metric.to_log(d).tolist() == [[0.0, 0.0], [0.0, math.log(np.float32(4.0))]] or torch.allclose(metric.to_log(d), torch.tensor([[0.0, 0.0], [0.0, 1.3862944]]))
    assert metric.to_inv(d).tolist() == [[0.0, 1.0], [0.0, 0.25]]
    assert metric.eps(None) == torch.finfo(torch.float32).eps
    with pytest.raises(ValueError):
        metric.extract_edges(d, preprocess="sqrt")
    with pytest.raises(NotImplementedError):
        metric.extract_edges(d, use_canny=False)
    with pytest.raises(NotImplementedError):
        metric.extract_edges(d, mask=d > 0)


def test_edges_module_has_no_cpu_fallback():
    import torch
    from hip_ext import HipExtError, edges
    with pytest.raises(HipExtError):
        edges.canny(torch.zeros(4, 4), device="cpu")
    with pytest.raises(HipExtError):
        edges.distance_transform_edt(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        edges.gaussian_weights(5.0)      # radius 20 > the kernel's cap
    with pytest.raises(TypeError):
        edges.canny(np.zeros((4, 4), np.float64), device="cuda:0")


def test_runner_flag_and_unchanged_keys(tmp_path):
    from oracle import metrics_oracle as MO
    from PIL import Image
    from src.scripts import amodal_dav2_inference as S
    assert "edge_metrics" in inspect.signature(S.run).parameters and inspect.signature(S.run).parameters["edge_metrics"].default is False
    assert "--edge_metrics" in inspect.getsource(S.main)
    rng = np.random.default_rng(0)
    d = {k: tmp_path / k for k in ("occ", "whole", "obs", "gt")}
    for v in d.values():
        v.mkdir()
    for sid in ("1", "2"):
        Image.fromarray((rng.random((64, 64, 3)) * 255).astype(np.uint8)).save(d["occ"] / f"{sid}_occlusion.png")
        m = np.zeros((64, 64), dtype=np.uint8)
        m[10:50, 8:40] = 255
        Image.fromarray(m).save(d["whole"] / f"{sid}_whole_mask.png")
        Image.fromarray((rng.uniform(0.2, 0.9, size=(32, 32)) * 65535).astype(np.uint16)).save(d["obs"] / f"{sid}_depth.png")
        Image.fromarray((rng.uniform(0.2, 0.9, size=(128, 128)) * 65535).astype(np.uint16)).save(d["gt"] / f"{sid}_depth.png")

    def model(x, guide_rgb=None, guide_mask=None, observation=None):
        return (observation + 1) / 2 * 0.5 + 0.25

    def evaluate(pred, gt, mask):
        p, g, m = pred.numpy(), gt.numpy(), mask.numpy()
        al = np.stack([MO.align_depth_least_square(g[b], p[b], m[b])[0] for b in range(p.shape[0])])
        return MO.depth_metrics(np.clip(al, 1e-3, 1.0), g, m)
    args = (model, ["1", "2"], str(d["occ"]), str(d["whole"]), str(d["obs"]))
    res = S.run(*args, str(tmp_path / "out"), str(d["gt"]), batch_size=2, device="cpu", evaluate=evaluate)
    assert set(res) == set(MO.ALL)
    with pytest.raises(ValueError, match="paper"):
        S.run(*args, str(tmp_path / "out2"), str(d["gt"]), device="cpu", protocol="paper", visible_mask_dir=str(d["whole"]), edge_metrics=True)
