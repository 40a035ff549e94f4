"""GPU: the evaluation sums of csrc/ada_eval.hip (hip.depth_eval, behind src/util/metric.py) over their value domain, against tests/_glue_ref.py:
eval_terms_ref (the reference's fp32 per-pixel rules) for everything that must be exact -- threshold ties, counts, dyadic sums, where NaN and inf
appear -- and eval_terms_fp64 (float64 terms) for the rest, within a tolerance measured on the CPU between those two ("Glue and
evaluation value domain")."""
import numpy as np
import pytest
import torch

import _glue_ref as G
from _exact import assert_exact_budget

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _eval(hip, pred, gt, mask=None, clip=None):
    s = hip.depth_eval(pred.to(DEV).contiguous(), gt.to(DEV).contiguous(), None if mask is None else mask.to(DEV).contiguous(), clip=clip)
    return s.cpu()[:, :15]


@pytest.fixture(scope="module")
def metric(hip):
    from src.util import metric
    return metric


def check_against_references(got, pred, gt, mask, clip, what):
    """NaN and +-inf exactly where eval_terms_ref has them; every finite sum within eval_tolerance of eval_terms_fp64.  Returns the two figures the
    issue asks for per sum: |ref32 - ref64| and |got - ref64|, relative to |ref64|."""
    r32 = G.eval_terms_ref(pred, gt, mask, clip=clip)
    r64, mag, logs = G.eval_terms_fp64(pred, gt, mask, clip=clip, with_abs=True)
    assert torch.equal(torch.isnan(r32), torch.isnan(r64)) and torch.equal(torch.isnan(got), torch.isnan(r32)), \
        f"{what}: NaN sums {[(b, G.NAMES[k]) for b, k in torch.isnan(got).nonzero().tolist()]}, reference {[(b, G.NAMES[k]) for b, k in torch.isnan(r32).nonzero().tolist()]}"
    inf = torch.isinf(r32)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], r32[inf]), f"{what}: infinities differ"
    fin = torch.isfinite(r64)
    tol = G.eval_tolerance(r32, r64, mag, logs, pred[0].numel())
    err = (got - r64).abs()
    bad = fin & ~(err <= tol)
    assert not bool(bad.any()), f"{what}: " + "; ".join(f"image {b} {G.NAMES[k]}: |got - fp64| {float(err[b, k]):.3e} > {float(tol[b, k]):.3e}" for b, k in bad.nonzero().tolist())
    den = r64.abs().clamp_min(1e-300)
    z = torch.zeros_like(r64)
    return torch.where(fin, (r32 - r64).abs() / den, z).max(0).values, torch.where(fin, err / den, z).max(0).values


# ---------------------------------------------------------------------------------------------------------------------------------
# threshold ties
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("t", G.THRESHOLDS)
def test_threshold_ties_counted_by_the_ieee_division(hip, metric, t, use_mask):
    """pred = t gt exactly, one ulp above, one ulp below, and mirrored: D1, D2, D3 are the reference rule's counts exactly (tests/test_glue_ref_cpu.py shows
    that a reciprocal-and-multiply miscounts these very inputs by dozens to hundreds)."""
    pred, gt = G.tie_image(t)
    mask = (torch.rand(pred.shape, generator=torch.Generator().manual_seed(3)) > 0.4) if use_mask else None
    want = G.eval_terms_ref(pred, gt, mask)
    got = _eval(hip, pred, gt, mask)
    counts = [G.N, G.D1, G.D2, G.D3]
    assert got[0, counts].tolist() == want[0, counts].tolist(), (t, got[0, counts].tolist(), want[0, counts].tolist())
    if not use_mask:
        assert want[0, G.N] == 9 * 4096 and want[0, G.D1 + G.THRESHOLDS.index(t)] == 5 * 4096
        one_image = lambda x: x.reshape(1, -1, 3).to(DEV)      # noqa: E731  (the metrics take the last two axes as the image)
        every = torch.ones(1, 3 * 4096, 3, dtype=torch.bool, device=DEV)
        for i, fn in enumerate((metric.delta1_acc, metric.delta2_acc, metric.delta3_acc)):
            assert float(fn(one_image(pred), one_image(gt), every)) == float(want[0, G.D1 + i] / want[0, G.N])


# ---------------------------------------------------------------------------------------------------------------------------------
# shapes and masks: the sums that no addition may round
# ---------------------------------------------------------------------------------------------------------------------------------
EVAL_SHAPES = [(1, 1, 1), (3, 1, 7), (2, 5, 255), (1, 1031, 1033)]          # one pixel; under one wave; odd; the smallest map above 512 * 2048 pixels (the workgroup cap)
MASK_KINDS = ["none", "uint8_0_255", "bool", "all_false", "first_only", "last_only"]


def _mask(kind, shape, seed):
    if kind == "none":
        return None
    m = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) > 0.35
    if kind == "uint8_0_255":
        return m.to(torch.uint8) * 255
    if kind == "bool":
        return m
    m = torch.zeros(shape, dtype=torch.bool)
    if kind == "first_only":
        m.view(shape[0], -1)[:, 0] = True
    elif kind == "last_only":
        m.view(shape[0], -1)[:, -1] = True
    return m


@pytest.mark.parametrize("shape", EVAL_SHAPES)
def test_linear_sums_are_exact_on_dyadic_maps(hip, metric, shape):
    """pred, gt = k / q: the terms of N are ones, those of SUM_P and SUM_G multiples of 1 / q, those of SUM_PP, SUM_PG and SQ of 1 / q^2, and each sum
    stays below 2^24 of its units (far inside float64's 2^53), so the sums equal float64 bit for bit in whatever order the per-thread partials, the
    shuffles and the atomics add them."""
    n = shape[1] * shape[2]
    kmax, q = (3, 4) if n > 2 ** 16 else (64, 64)
    g = torch.Generator().manual_seed(n)
    pred = torch.randint(1, kmax + 1, shape, generator=g).float() / q
    gt = torch.randint(1, kmax + 1, shape, generator=g).float() / q
    t32, t64 = G.eval_pixel_terms(pred, gt), G.eval_pixel_terms(pred, gt, dtype=torch.float64)
    units = {G.N: 1.0, G.SUM_P: 1.0 / q, G.SUM_G: 1.0 / q, G.SUM_PP: 1.0 / (q * q), G.SUM_PG: 1.0 / (q * q), G.SQ: 1.0 / (q * q)}
    for k, unit in units.items():
        total = t64[k].abs().flatten(1).sum(1)
        assert_exact_budget(unit=unit, mag=total, ref=torch.cat([total, t64[k].flatten()]), what=f"{G.NAMES[k]} {shape}")
    for kind in MASK_KINDS:
        mask = _mask(kind, shape, seed=n + 1)
        got = _eval(hip, pred, gt, mask)
        w64, w32 = G.eval_masked_sums(t64, mask), G.eval_masked_sums(t32, mask)
        for k in G.LINEAR:
            assert torch.equal(got[:, k], w64[:, k]), (kind, G.NAMES[k], got[:, k].tolist(), w64[:, k].tolist())
        assert torch.equal(got[:, G.SQ], w32[:, G.SQ]), (kind, got[:, G.SQ].tolist(), w32[:, G.SQ].tolist())
        for k in (G.D1, G.D2, G.D3):
            assert torch.equal(got[:, k], w32[:, k]), (kind, G.NAMES[k])
        if kind == "all_false":
            assert torch.equal(got, torch.zeros(shape[0], 15, dtype=torch.float64))
            m = metric.depth_metrics(pred.to(DEV), gt.to(DEV), mask.to(DEV))          # 0 / 0, as the reference's own expressions give
            assert all(bool(torch.isnan(v)) for v in m.values()), {k: float(v) for k, v in m.items()}
        elif kind in ("first_only", "last_only"):
            assert got[:, G.N].tolist() == [1.0] * shape[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# value domain
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.EVAL_FAMILIES)
def test_value_domain_against_fp64_terms(hip, name):
    pred, gt, mask = G.eval_family(name)
    clip = G.EVAL_CLIP.get(name)
    got = _eval(hip, pred, gt, mask, clip)
    assert bool(torch.isfinite(got).all())
    cpu, dev = check_against_references(got, pred, gt, mask, clip, name)
    print(f"{name}: relative to the float64-term sums -- fp32 terms on the CPU / the kernel: " +
          ", ".join(f"{G.NAMES[k]} {float(cpu[k]):.1e} / {float(dev[k]):.1e}" for k in range(15) if float(cpu[k]) or float(dev[k])))


# ---------------------------------------------------------------------------------------------------------------------------------
# constant log difference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", G.CONST_LOG_N)
def test_constant_log_difference_has_no_variance(hip, metric, n):
    """A region of n pixels with one log difference dl: silog_rmse = 100 sqrt(sum dl^2 / n - (sum dl)^2 / n^2) is 0.  With the square taken in fp32 the
    difference of the two terms is that square's rounding error, of either sign: NaN for about half of these cases (tests/test_glue_ref_cpu.py) and
    up to 2.4e-2 |dl| otherwise.  Squared in float64 what remains is float64 rounding of the n-term sums, at most 4 n 2^-53 dl^2."""
    for c_pred, c_gt in G.const_log_pairs():
        g = torch.Generator().manual_seed(n)
        pred, gt = torch.rand(1, 20, 20, generator=g) + 0.5, torch.rand(1, 20, 20, generator=g) + 0.5
        mask = torch.zeros(1, 400, dtype=torch.bool)
        mask[0, :n] = True
        mask = mask.view(1, 20, 20)
        pred[mask], gt[mask] = c_pred, c_gt
        dl = abs(float(np.log(np.float64(np.float32(c_pred))) - np.log(np.float64(np.float32(c_gt)))))
        silog = float(metric.silog_rmse(pred.to(DEV), gt.to(DEV), mask.to(DEV)))
        s = _eval(hip, pred, gt, mask)[0]
        var = float(s[G.LOG_SQ] / s[G.N] - (s[G.LOG] / s[G.N]) ** 2)
        what = f"c_pred {c_pred!r} c_gt {c_gt!r} n {n}: silog_rmse {silog!r}, rmse_log^2 - mean(dl)^2 {var!r}, |dl| {dl!r}"
        assert s[G.N] == n and abs(float(s[G.LOG])) / n == pytest.approx(dl, abs=1e-5), what
        assert np.isfinite(silog) and 0.0 <= silog <= 1e-3 * dl, what
        assert np.isfinite(var) and 100 * abs(var) ** 0.5 <= 1e-3 * dl, what
        if n == 1:
            assert silog == 0.0 and var == 0.0, what


# ---------------------------------------------------------------------------------------------------------------------------------
# NaN, non-positive predictions, zero ground truth
# ---------------------------------------------------------------------------------------------------------------------------------
def _maps(seed, B=3, H=9, W=31):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, H, W, generator=g) * 0.9 + 0.05
    pred = gt * (0.8 + 0.5 * torch.rand(B, H, W, generator=g))
    mask = torch.rand(B, H, W, generator=g) > 0.3
    return pred, gt, mask


P_SUMS = [G.SUM_P, G.SUM_PP, G.SUM_PG, G.ABS_REL, G.SQ_REL, G.SQ, G.LOG_SQ, G.LOG, G.LOG10_ABS, G.INV_SQ]          # every sum whose term is NaN for a NaN prediction


@pytest.mark.parametrize("clip", [(1e-3, 1.0), None])
def test_nan_prediction_inside_the_mask_is_reported(hip, clip):
    """torch.clamp and np.clip propagate NaN: a NaN prediction under the mask makes every sum that depends on the prediction NaN for its image (the three
    counts see `NaN < t` = False, as the reference's do), clipped or not; the other images of the batch are untouched."""
    pred, gt, mask = _maps(1)
    clean = _eval(hip, pred, gt, mask, clip)
    mask[1, 4, 17], mask[2, 0, 0] = True, False
    base = _eval(hip, pred, gt, mask, clip)
    pred[1, 4, 17] = NAN          # inside the mask of image 1
    pred[2, 0, 0] = NAN           # outside the mask of image 2: changes nothing
    got = _eval(hip, pred, gt, mask, clip)
    check_against_references(got, pred, gt, mask, clip, f"NaN under clip {clip}")
    assert bool(torch.isnan(got[1, P_SUMS]).all()) and bool(torch.isfinite(got[1, [G.N, G.SUM_G, G.D1, G.D2, G.D3]]).all())
    assert torch.equal(got[[0, 2]], base[[0, 2]]) and torch.equal(got[0], clean[0]) and bool(torch.isfinite(got[[0, 2]]).all())
    assert torch.equal(got[1, [G.N, G.SUM_G]], base[1, [G.N, G.SUM_G]])


def test_non_positive_prediction_without_clip(hip):
    """log of 0 is -inf and of a negative number NaN: the log sums say so exactly where the reference's fp32 rules do; the linear sums stay finite."""
    pred, gt, mask = _maps(2)
    mask[0, 3, 3] = mask[1, 5, 30] = True
    pred[0, 3, 3] = 0.0
    pred[1, 5, 30] = -0.25
    got = _eval(hip, pred, gt, mask)
    check_against_references(got, pred, gt, mask, None, "non-positive prediction")
    assert got[0, G.LOG] == -np.inf and got[0, G.LOG_SQ] == np.inf and got[0, G.LOG10_ABS] == np.inf and got[0, G.INV_SQ] == np.inf
    assert bool(torch.isnan(got[1, list(G.LOG_SUMS)]).all()) and bool(torch.isfinite(got[1, G.INV_SQ]))
    assert bool(torch.isfinite(got[:, list(G.LINEAR) + [G.ABS_REL, G.SQ_REL, G.SQ]]).all()) and bool(torch.isfinite(got[2]).all())


def test_zero_ground_truth_under_the_mask(hip):
    pred, gt, mask = _maps(3)
    mask[1, 2, 2] = True
    gt[1, 2, 2] = 0.0
    got = _eval(hip, pred, gt, mask)
    check_against_references(got, pred, gt, mask, None, "gt = 0")
    assert got[1, [G.ABS_REL, G.SQ_REL, G.LOG_SQ, G.LOG, G.LOG10_ABS, G.INV_SQ]].tolist() == [np.inf] * 6
    assert bool(torch.isfinite(got[[0, 2]]).all()) and bool(torch.isfinite(got[1, list(G.LINEAR) + [G.SQ, G.D1, G.D2, G.D3]]).all())
