"""GPU: the paper's evaluation protocol on the device (ada_protocol_fit_fwd / ada_protocol_eval_fwd behind hip_ext.protocol_fit / protocol_eval and
src/util/validation.py) against the reference's own results (tests/golden/protocol/cases.npz), exact arithmetic on dyadic inputs, bit
reproducibility, and the fp64 restatement (tests/_protocol_ref.py) on the shapes at which the kernels take another path: one chunk is
ADA_PROTOCOL_CHUNK = 4096 pixels, and the 16-byte / 4-byte loads need h * w % 4 == 0."""
import math

import numpy as np
import pytest
import torch

import _protocol_ref as PR

pytestmark = pytest.mark.gpu
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)


@pytest.fixture(scope="module")
def V(hip):
    from src.util import validation
    return validation


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_rows(hip, pred, gt, obs, whole, visible, region, valid, eps=1e-5, fit=None):
    """(fit rows, sums) as fp64 numpy from the two wrappers; ``fit`` replaces the computed rows in the second call."""
    p = _cuda(pred)
    rows = hip.protocol_fit(p, _cuda(obs), _cuda(visible), _cuda(whole))
    sums = hip.protocol_eval(p, _cuda(gt), _cuda(region), _cuda(valid), rows if fit is None else _cuda(fit), eps=eps)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), sums.cpu().numpy()


def _scene(B, h, w, seed, pred_hw=None, region_share=1.0):
    """Seeded maps: gt in (0.1, 0.9) with 10 % holes, an observation near it, a prediction that is an affine image of the gt plus noise (or, at another
    size, noise alone), a rectangular object whose upper part is visible, speckled."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.1, 0.9, (B, h, w)).astype(np.float32)
    gt[rng.uniform(size=gt.shape) < 0.1] = 0.0
    obs = (gt + rng.normal(0, 0.01, gt.shape)).astype(np.float32)
    if pred_hw is None:
        pred = np.maximum((gt - 0.05) / 1.5 + rng.normal(0, 0.01, gt.shape), 0.01).astype(np.float32)
    else:
        pred = rng.uniform(0.05, 0.95, (B, *pred_hw)).astype(np.float32)
    whole = np.zeros((B, h, w), bool)
    whole[:, h // 6:h - h // 6, w // 8:w - w // 8] = True
    visible = whole & (np.arange(h)[None, :, None] < h * 0.55) & (rng.uniform(size=gt.shape) < 0.9)
    invisible = whole & ~visible & (rng.uniform(size=gt.shape) < region_share)
    return dict(pred=pred, gt=gt, obs=obs, whole=whole, visible=visible, invisible=invisible, valid=gt > 0)


def _ambiguous(pred, gt, region, scale, shift, eps):
    """Pixels of the region whose ratio lies within 1e-5 (relative) of a delta threshold, raw or aligned: the fp32 quotient of the device may fall
    on the other side of the threshold there."""
    p = PR.resize_nearest(np.asarray(pred, np.float64), *gt.shape)[region]
    g = gt.astype(np.float64)[region] + eps
    n = 0
    for pp in (p + eps, p * scale + shift + eps):
        with np.errstate(all="ignore"):
            r = np.maximum(pp / g, g / pp)
        n += sum(int((np.abs(r / t - 1) < 1e-5).sum()) for t in THRESHOLDS)
    return n


def _check_against_restatement(V, hip, s, eps=1e-5, use_valid=True):
    """Every image of the scene: fit and the twenty metrics against the fp64 restatement.  Tolerances: the ones the goldens are held to (fp32
    per-pixel terms summed in fp64); a delta metric may additionally differ by one pixel's share per ambiguous pixel (see _ambiguous)."""
    valid = s["valid"] if use_valid else None
    rows, sums = _device_rows(hip, s["pred"], s["gt"], s["obs"], s["whole"], s["visible"], s["invisible"], valid, eps)
    got = V.samples_from_rows(torch.from_numpy(rows), torch.from_numpy(sums))
    for b, r in enumerate(got):
        want = PR.evaluate_sample(s["pred"][b], s["gt"][b], s["obs"][b], s["whole"][b], s["visible"][b], s["invisible"][b], None if valid is None else valid[b], eps)
        assert r.scale == pytest.approx(want.scale, rel=1e-5) and r.shift == pytest.approx(want.shift, rel=1e-5, abs=1e-6)
        assert (r.bucket, r.n_visible, r.n_whole) == (want.bucket, want.n_visible, want.n_whole)
        region = s["invisible"][b] & (valid[b] if valid is not None else True)
        assert sums[b, 0, hip.EVAL_N] == sums[b, 1, hip.EVAL_N] == region.sum()
        slack = _ambiguous(s["pred"][b], s["gt"][b], region, want.scale, want.shift, eps) / max(1, int(region.sum()))
        for name_row, g_, w_ in (("raw", r.raw, want.raw), ("aligned", r.aligned, want.aligned)):
            for m in V.METRICS:
                if math.isnan(w_[m]):
                    assert math.isnan(g_[m]), (b, name_row, m)
                else:
                    assert g_[m] == pytest.approx(w_[m], rel=2e-5, abs=1e-7 + (slack if m.startswith("delta") else 0.0)), (b, name_row, m)
    return got


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the reference's own results
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(V, hip):
    samples, rec = PR.load_golden()
    results = [V.evaluate_batch(_cuda(s["pred"][None]), _cuda(s["gt"][None]), _cuda(s["obs"][None]), _cuda(s["whole"][None]), _cuda(s["visible"][None]),
                                _cuda(s["invisible"][None]), _cuda(s["valid"][None]))[0] for s in samples]
    return samples, rec, results


def test_golden_fits(golden):
    _, rec, results = golden
    np.testing.assert_allclose([r.scale for r in results], rec["scale"], rtol=1e-5)
    np.testing.assert_allclose([r.shift for r in results], rec["shift"], rtol=1e-5, atol=1e-6)


def test_golden_nan_pattern_of_every_sample(golden, V):
    _, rec, results = golden
    for i, r in enumerate(results):
        for row, values in enumerate((r.raw, r.aligned)):
            got = [math.isnan(values[m]) for m in V.METRICS]
            assert got == [bool(x) for x in np.isnan(rec["values"][i, row])], (i, row, got)


def test_golden_groups_and_counts(golden, V):
    _, rec, results = golden
    tracker = V.ValidationTracker()
    for r in results:
        tracker.update(r)
    means, counts = tracker.result(), tracker.counts()
    for gi, g in enumerate(V.GROUPS):
        for j, m in enumerate(V.METRICS):
            assert counts[g][m] == int(rec["counts"][gi, j]), (g, m)
            assert means[g][m] == pytest.approx(float(rec["means"][gi, j]), rel=2e-5, abs=1e-7), (g, m)


def test_validate_single_dataset_returns_the_golden_dict(golden, V):
    samples, rec, _ = golden
    batches, model, calls = PR.golden_loader(samples)
    res = V.validate_single_dataset(model, batches, "cuda")
    assert len(calls) == len(samples) and all(c[1] == -1.0 and c[2] == 1.0 and -1.0 <= c[3] <= c[4] <= 1.0 for c in calls)
    assert list(res) == list(V.GROUPS)
    for gi, g in enumerate(V.GROUPS):
        for j, m in enumerate(V.METRICS):
            assert res[g][m] == pytest.approx(float(rec["means"][gi, j]), rel=2e-5, abs=1e-7), (g, m)


def test_evaluate_batch_defaults_invisible_to_whole_and_not_visible(golden, V):
    samples, _, results = golden
    s = samples[1]
    assert np.array_equal(s["invisible"], s["whole"] & ~s["visible"])
    r = V.evaluate_batch(_cuda(s["pred"][None]), _cuda(s["gt"][None]), _cuda(s["obs"][None]), _cuda(s["whole"][None]), _cuda(s["visible"][None]), None, _cuda(s["valid"][None]))[0]
    assert r == results[1]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact arithmetic: pred, obs, gt = k / 64, eps = 2^-7, the fit set by hand to (2, 0.25) -- every term and every sum is exact in fp32 / fp64
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _dyadic_scene(B, h, w, seed):
    rng = np.random.default_rng(seed)
    k = lambda: rng.integers(1, 65, (B, h, w)).astype(np.float32) / 64.0      # noqa: E731
    s = dict(pred=k(), gt=k(), obs=k())
    s["whole"] = rng.uniform(size=(B, h, w)) < 0.7
    s["visible"] = s["whole"] & (rng.uniform(size=(B, h, w)) < 0.5)
    s["invisible"] = s["whole"] & ~s["visible"]
    s["valid"] = rng.uniform(size=(B, h, w)) < 0.8
    return s


@pytest.mark.parametrize("shape", [(3, 37, 53), (2, 64, 68)])      # scalar loads in one chunk; vector loads, two chunks
def test_exact_sums_on_dyadic_inputs(hip, shape):
    B, h, w = shape
    s = _dyadic_scene(B, h, w, seed=h)
    eps = 2.0 ** -7
    fit = np.zeros((B, hip.FIT_NCOL))
    fit[:, hip.FIT_SCALE], fit[:, hip.FIT_SHIFT] = 2.0, 0.25
    rows, sums = _device_rows(hip, s["pred"], s["gt"], s["obs"], s["whole"], s["visible"], s["invisible"], s["valid"], eps, fit=fit)
    p64, g64, o64 = (s[k].astype(np.float64) for k in ("pred", "gt", "obs"))
    for b in range(B):
        v = s["visible"][b]
        want = {hip.FIT_N: v.sum(), hip.FIT_SUM_P: p64[b][v].sum(), hip.FIT_SUM_O: o64[b][v].sum(), hip.FIT_SUM_PP: (p64[b][v] ** 2).sum(),
                hip.FIT_SUM_PO: (p64[b][v] * o64[b][v]).sum(), hip.FIT_MIN_P: p64[b][v].min(), hip.FIT_MAX_P: p64[b][v].max(),
                hip.FIT_N_VISIBLE: v.sum(), hip.FIT_N_WHOLE: s["whole"][b].sum()}
        for col, val in want.items():
            assert rows[b, col].tobytes() == np.float64(val).tobytes(), (b, col, rows[b, col], val)
        m = s["invisible"][b] & s["valid"][b]
        g = g64[b][m] + eps
        for r, p in enumerate((p64[b][m] + eps, p64[b][m] * 2.0 + 0.25 + eps)):
            assert np.array_equal(p.astype(np.float32).astype(np.float64), p)                      # the fp32 values of the kernel are these, exactly
            want = {hip.EVAL_N: m.sum(), hip.EVAL_SUM_P: p.sum(), hip.EVAL_SUM_G: g.sum(), hip.EVAL_SUM_PP: (p * p).sum(), hip.EVAL_SUM_PG: (p * g).sum(),
                    hip.EVAL_SQ: ((p - g) ** 2).sum()}
            for col, val in want.items():
                assert sums[b, r, col].tobytes() == np.float64(val).tobytes(), (b, r, col, sums[b, r, col], val)
            ratio = np.maximum(p / g, g / p)
            assert min(float(np.abs(ratio - t).min()) for t in THRESHOLDS) >= 1e-6                 # shown on the CPU first: no ratio near a threshold
            for col, t in zip((hip.EVAL_D1, hip.EVAL_D2, hip.EVAL_D3), THRESHOLDS):
                assert sums[b, r, col] == float((ratio < t).sum()), (b, r, col)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pred_hw", [((5, 37, 53), None), ((5, 72, 116), None), ((5, 37, 53), (28, 42))])      # 1 chunk scalar; 3 chunks vector; gathered
def test_bit_reproducible_and_independent_of_the_batch(hip, shape, pred_hw):
    s = _scene(*shape, seed=11, pred_hw=pred_hw)
    args = [s[k] for k in ("pred", "gt", "obs", "whole", "visible", "invisible", "valid")]
    rows, sums = _device_rows(hip, *args)
    rows2, sums2 = _device_rows(hip, *args)
    assert rows.tobytes() == rows2.tobytes() and sums.tobytes() == sums2.tobytes()
    assert np.isfinite(sums[:, 0, :hip.EVAL_SUM_PG + 1]).all() and (sums[:, 0, hip.EVAL_N] > 0).all()
    for b in range(shape[0]):
        r1, s1 = _device_rows(hip, *[a[b:b + 1] for a in args])
        assert r1.tobytes() == rows[b:b + 1].tobytes() and s1.tobytes() == sums[b:b + 1].tobytes(), b


# ---------------------------------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pred_hw", [((2, 5, 7), None), ((2, 37, 53), None), ((2, 37, 53), (28, 42)), ((2, 37, 53), (74, 74)), ((1, 64, 68), (28, 42))])
def test_small_shapes_against_the_restatement(V, hip, shape, pred_hw):
    s = _scene(*shape, seed=sum(shape), pred_hw=pred_hw)
    if shape[1:] == (5, 7):      # 35 pixels: a hand-made object, every pixel valid
        s["gt"] = np.maximum(s["gt"], 0.2).astype(np.float32)
        s["valid"] = s["gt"] > 0
        s["whole"][:] = False
        s["whole"][:, 1:5, 1:6] = True
        s["visible"] = s["whole"] & (np.arange(5)[None, :, None] < 3)
        s["invisible"] = s["whole"] & ~s["visible"]
    _check_against_restatement(V, hip, s)


def test_full_size_batch_against_the_restatement(V, hip):
    got = _check_against_restatement(V, hip, _scene(2, 518, 518, seed=518, region_share=0.25))
    assert {r.bucket for r in got} <= {"easy", "mid", "diff"}


def test_valid_none_counts_every_pixel_of_the_region(V, hip):
    s = _scene(2, 37, 53, seed=5)
    s["gt"] = np.maximum(s["gt"], 0.05).astype(np.float32)      # no holes: without a valid mask a gt of 0 would be evaluated as eps
    _check_against_restatement(V, hip, s, use_valid=False)


def test_all_zero_masks(V, hip):
    s = _scene(2, 37, 53, seed=6)
    for k in ("whole", "visible", "invisible"):
        s[k] = np.zeros_like(s[k])
    rows, sums = _device_rows(hip, s["pred"], s["gt"], s["obs"], s["whole"], s["visible"], s["invisible"], s["valid"])
    assert (rows[:, [hip.FIT_N, hip.FIT_N_VISIBLE, hip.FIT_N_WHOLE, hip.FIT_SCALE, hip.FIT_SHIFT]] == 0).all()
    assert (rows[:, hip.FIT_MIN_P] == np.inf).all() and (rows[:, hip.FIT_MAX_P] == -np.inf).all()
    assert (sums == 0).all()
    for r in V.samples_from_rows(torch.from_numpy(rows), torch.from_numpy(sums)):
        assert r.bucket == "diff" and all(math.isnan(v) for v in list(r.raw.values()) + list(r.aligned.values()))


def test_degenerate_fits_get_the_minimum_norm_answer(hip):
    s = _scene(3, 37, 53, seed=8)
    s["visible"][0] = False                                      # no support
    s["pred"][1][s["visible"][1]] = 0.375                        # rank one
    rows, _ = _device_rows(hip, s["pred"], s["gt"], s["obs"], s["whole"], s["visible"], s["invisible"], s["valid"])
    assert rows[0, hip.FIT_SCALE] == 0 and rows[0, hip.FIT_SHIFT] == 0
    for b in (1, 2):
        scale, shift = PR.fit(s["pred"][b], s["obs"][b], s["visible"][b])      # numpy.linalg.lstsq in fp64
        assert rows[b, hip.FIT_SCALE] == pytest.approx(scale, rel=1e-9) and rows[b, hip.FIT_SHIFT] == pytest.approx(shift, rel=1e-9, abs=1e-12)
    obar = s["obs"][1].astype(np.float64)[s["visible"][1]].mean()
    assert rows[1, hip.FIT_SCALE] == pytest.approx(0.375 * obar / (0.375 ** 2 + 1), rel=1e-12)
    assert rows[1, hip.FIT_SHIFT] == pytest.approx(obar / (0.375 ** 2 + 1), rel=1e-12)


def test_negative_aligned_values_poison_exactly_the_log_sums(hip):
    s = _scene(1, 37, 53, seed=9)
    fit = np.zeros((1, hip.FIT_NCOL))
    fit[:, hip.FIT_SCALE], fit[:, hip.FIT_SHIFT] = 1.0, -0.5     # most aligned values are negative
    _, sums = _device_rows(hip, s["pred"], s["gt"], s["obs"], s["whole"], s["visible"], s["invisible"], s["valid"], fit=fit)
    log_cols = [hip.EVAL_LOG_SQ, hip.EVAL_LOG, hip.EVAL_LOG10_ABS]
    others = [c for c in range(hip.EVAL_NSUM) if c not in log_cols]
    assert np.isnan(sums[0, 1, log_cols]).all() and np.isfinite(sums[0, 1, others]).all() and np.isfinite(sums[0, 0]).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the wrappers refuse what the kernels cannot take
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_cpu_tensors_wrong_dtypes_and_a_small_workspace(hip):
    s = _scene(2, 37, 53, seed=10)
    pred, gt, obs, whole, visible, region, valid = (_cuda(s[k]) for k in ("pred", "gt", "obs", "whole", "visible", "invisible", "valid"))
    fit = hip.protocol_fit(pred, obs, visible, whole)
    E = hip.HipExtError
    with pytest.raises(E, match="no CPU fallback"):
        hip.protocol_fit(pred.cpu(), obs, visible, whole)
    with pytest.raises(E, match="no CPU fallback"):
        hip.protocol_eval(pred, gt.cpu(), region, valid, fit)
    with pytest.raises(E, match="dtype"):
        hip.protocol_fit(pred.double(), obs, visible, whole)
    with pytest.raises(E, match="dtype"):
        hip.protocol_fit(pred, obs, visible.float(), whole)
    with pytest.raises(E, match="dtype"):
        hip.protocol_eval(pred, gt, region, valid, fit.float())
    with pytest.raises(E, match="the other maps"):
        hip.protocol_fit(pred, obs, visible[:, :30].contiguous(), whole)
    with pytest.raises(E, match="fit must be"):
        hip.protocol_eval(pred, gt, region, valid, fit[:1])
    need = hip.protocol_workspace_bytes(2, 37, 53)
    assert need == 2 * 1 * hip.PROTOCOL_WS_DOUBLES * 8
    small = torch.empty(need - 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(E, match="workspace"):
        hip.protocol_fit(pred, obs, visible, whole, workspace=small)
    with pytest.raises(E, match="workspace"):
        hip.protocol_eval(pred, gt, region, valid, fit, workspace=small)
    exact = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert torch.equal(hip.protocol_fit(pred, obs, visible, whole, workspace=exact), fit)
