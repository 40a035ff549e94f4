"""Premises of tests/test_gpu_glue_edges.py and tests/test_gpu_eval_values.py, checked without a GPU: the restatements of tests/_glue_ref.py agree
with independent formulations, the exact families are exact, the threshold ties can see a lost IEEE division and the constant-log-difference
family can see an fp32 square ("Glue and evaluation value domain")."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _glue_ref as G
from _exact import assert_exact_budget

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ---------------------------------------------------------------------------------------------------------------------------------
# blend
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.BLEND_SHAPES)
def test_blend_ref_against_host_helper_and_avg_pool(shape):
    """blend_ref adds nine terms in float64, rounds the sum to fp32 and divides by 9 in fp32: two roundings.  infer.median_filter_blend (float64 sum,
    float64 quotient, one rounding) and F.avg_pool2d in float64 (rounded once here) are the exact mean rounded once, up to float64's own error.  So
    |difference| <= (2 + 1) * 2^-24 * |mean| <= 3 * 2^-24 * max|blended| on the blurred pixels, and identical values everywhere else."""
    import infer
    H, W = shape
    names, amodal, base, masks = G.blend_case(H, W, exact=False)
    out, border, blended = G.blend_parts(amodal, base, masks)
    pooled = F.avg_pool2d(F.pad(blended.double()[:, None], (1, 1, 1, 1), mode="reflect"), 3, stride=1)[:, 0].float()
    want_pool = torch.where(border, pooled, blended)
    for b, name in enumerate(names):
        bound = 3 * G.U * float(blended[b].abs().max())
        # the helper, like the reference, box-sums the mask's own values and is only ever handed 0 / 1 masks (infer.py divides the byte mask by 255);
        # the kernel and blend_ref count mask > 0, the same rule on that domain, so the 255 / 0.5 family reaches the helper binarised
        host = infer.median_filter_blend(amodal[b], base[b].clone(), (masks[b] > 0).float().numpy())
        for other, what in ((host, "median_filter_blend"), (want_pool[b], "avg_pool2d")):
            err = (out[b].double() - other.double()).abs()
            assert float(err[border[b]].max() if bool(border[b].any()) else 0.0) <= bound, (name, what, float(err.max()), bound)
            assert torch.equal(out[b][~border[b]], other[~border[b]]), (name, what)
    # what the families are for: the border is empty only for the empty mask, and the full mask still blurs the image's frame
    i_empty, i_full = names.index("empty"), names.index("full")
    assert not bool(border[i_empty].any()) and torch.equal(out[i_empty], base[i_empty])
    frame = torch.ones(H, W, dtype=torch.bool)
    frame[1:H - 1, 1:W - 1] = False
    assert torch.equal(border[i_full], frame)
    assert all(bool(border[b].any()) for b in range(len(names)) if b != i_empty)


@pytest.mark.parametrize("pair", G.BLEND_SCALE_SHIFTS)
@pytest.mark.parametrize("shape", G.BLEND_SHAPES)
def test_blend_exact_family_is_exact(shape, pair):
    """Values k / 1024 in [0, 1), scale and shift multiples of 2^-4: the aligned paste is a multiple of 2^-14 and the nine-term sum stays far below
    2^24 units -- no fp32 summation order rounds, and the only rounding left is the correctly rounded quotient."""
    H, W = shape
    names, amodal, base, masks = G.blend_case(H, W, exact=True)
    ss = G.scale_shift_tensor(pair, len(names))
    if pair is not None:
        assert all(v * 16 == int(v * 16) for v in pair)
    out, border, blended = G.blend_parts(amodal, base, masks, ss)
    pasted64 = amodal.double() * (pair[0] if pair else 1.0) + (pair[1] if pair else 0.0)
    blended64 = torch.where(masks > 0, pasted64, base.double())
    assert torch.equal(blended.double(), blended64), "the aligned paste rounds"
    total64 = sum(F.pad(blended64[:, None], (1, 1, 1, 1), mode="reflect")[:, 0][:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    assert_exact_budget(unit=2.0 ** -14, mag=G.blur_mag(blended), ref=torch.cat([total64.flatten(), blended64.flatten()]), what=f"blend {shape} {pair}")
    # ... so an fp32 sum in the kernel's order (row by row) and in the opposite order are the float64 sum
    pad32 = F.pad(blended[:, None], (1, 1, 1, 1), mode="reflect")[:, 0]
    taps = [pad32[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]
    for order in (taps, taps[::-1]):
        s = torch.zeros_like(blended)
        for tap in order:
            s = s + tap
        assert torch.equal(s.double(), total64)
    assert torch.equal(out[border], (total64.float() / 9)[border])


# ---------------------------------------------------------------------------------------------------------------------------------
# tile blend
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", G.TILE_GEOMETRIES)
def test_tile_blend_ref_properties_and_exact_family(geom):
    th, tw, H, W, overlap, ramp = geom
    assert ramp == min(max(1, overlap), min(th, tw) // 2)          # what tiled_apply hands the kernel
    origins = G.tile_geometry_origins(th, tw, H, W, overlap)
    T = len(origins)
    tiles = G.tile_values(2, T, th, tw, exact=True, seed=5)
    out, cover, acc, wsum = G.tile_blend_parts(tiles, origins, H, W, ramp)
    assert int(cover.min()) >= 1, "the origins of tile_origins cover the image"
    assert origins[-1] == (H - th, W - tw)          # the last tile is end-aligned
    # a pixel under a single tile keeps that tile's value; a constant field stays constant
    single = cover == 1
    if bool(single.any()):
        pasted = torch.full((2, H, W), float("nan"))
        for t, (oy, ox) in enumerate(origins):
            pasted[:, oy:oy + th, ox:ox + tw] = tiles[:, t]
        if ramp & (ramp - 1) == 0:
            assert torch.equal(out[:, single], pasted[:, single])
        else:          # fp32(ramp * fp32(1 / ramp)) need not be 1: the product, the quotient and the final rounding remain
            assert float((out[:, single] - pasted[:, single]).abs().max()) <= 3 * G.U * float(tiles.abs().max())
    const = G.tile_blend_ref(torch.full((1, T, th, tw), 0.37), origins, H, W, ramp)
    assert float((const / np.float32(0.37) - 1).abs().max()) <= 2.0 ** -23
    if ramp & (ramp - 1) == 0:
        # weights are multiples of 1 / ramp^2, values of 2^-10: products, acc and wsum are exact in fp32
        unit = 2.0 ** -10 / (ramp * ramp)
        w = torch.from_numpy(G.feather(th, ramp)[:, None].astype(np.float64) * G.feather(tw, ramp)[None, :].astype(np.float64))
        assert torch.equal(w.float().double(), w) and torch.equal(w * ramp * ramp, (w * ramp * ramp).round())
        mag = torch.zeros(2, H, W, dtype=torch.float64)
        for t, (oy, ox) in enumerate(origins):
            mag[:, oy:oy + th, ox:ox + tw] += w * tiles[:, t].double().abs()
        assert_exact_budget(unit=unit, mag=torch.maximum(mag, wsum.expand_as(mag)), ref=torch.cat([acc.flatten(), wsum.flatten()]), what=f"tile blend {geom}")
        # fp32 accumulation, tiles first to last and last to first, is the float64 accumulation
        for order in (range(T), reversed(range(T))):
            a32, w32 = torch.zeros(2, H, W), torch.zeros(H, W)
            for t in order:
                oy, ox = origins[t]
                a32[:, oy:oy + th, ox:ox + tw] += w.float() * tiles[:, t]
                w32[oy:oy + th, ox:ox + tw] += w.float()
            assert torch.equal(a32.double(), acc) and torch.equal(w32.double(), wsum)
            assert torch.equal(a32 / w32, out)          # and the fp32 quotient of exact operands is the float64 quotient rounded once


def test_tile_blend_ref_uncovered_pixel_is_nan():
    tiles = G.tile_values(1, 1, 8, 8, exact=True, seed=6)
    out, cover, _, _ = G.tile_blend_parts(tiles, [(0, 0)], 8, 12, 4)
    assert torch.equal(torch.isnan(out[0]), cover == 0) and int((cover == 0).sum()) == 32
    assert torch.equal(out[0, :, :8], tiles[0, 0])


# ---------------------------------------------------------------------------------------------------------------------------------
# min / max, normalisation
# ---------------------------------------------------------------------------------------------------------------------------------
def test_minmax_and_normalize_ref_propagate_nan():
    x = torch.tensor([[1.0, float("nan"), 3.0], [2.0, 5.0, -1.0], [float("inf"), float("inf"), float("inf")]])
    mm = G.minmax_ref(x)
    assert torch.isnan(mm[0]).all() and mm[1].tolist() == [-1.0, 5.0] and mm[2].tolist() == [float("inf"), float("inf")]
    norm, obs = G.normalize_ref(x, mm)
    assert torch.isnan(norm[0]).all() and torch.isnan(obs[0]).all()
    assert norm[1].tolist() == [0.5, 1.0, 0.0] and obs[1].tolist() == [0.0, 1.0, -1.0]
    const = torch.full((1, 4), 0.25)
    assert torch.isnan(G.normalize_ref(const, G.minmax_ref(const))[0]).all()          # 0 / 0, as the reference's own expression gives


# ---------------------------------------------------------------------------------------------------------------------------------
# evaluation sums
# ---------------------------------------------------------------------------------------------------------------------------------
def test_eval_terms_reproduce_the_metrics_oracle():
    """The 15 sums, combined as src/util/metric.py combines them, are the reference-pinned fp64 oracle's metrics."""
    from oracle import metrics_oracle as MO
    rng = np.random.default_rng(1)
    gt = rng.uniform(0.5, 10.0, size=(3, 17, 23)).astype(np.float32)
    pred = (gt * rng.uniform(0.7, 1.4, size=gt.shape)).astype(np.float32)
    mask = rng.uniform(size=gt.shape) > 0.3
    want = MO.depth_metrics(pred, gt, mask)
    s = G.eval_terms_fp64(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(mask))
    n = s[:, G.N]
    got = {"abs_relative_difference": (s[:, G.ABS_REL] / n).mean(), "squared_relative_difference": (s[:, G.SQ_REL] / n).mean(),
           "rmse_linear": (s[:, G.SQ] / n).sqrt().mean(), "rmse_log": (s[:, G.LOG_SQ] / n).sqrt().mean(), "log10": s[:, G.LOG10_ABS].sum() / n.sum(),
           "delta1_acc": (s[:, G.D1] / n).mean(), "delta2_acc": (s[:, G.D2] / n).mean(), "delta3_acc": (s[:, G.D3] / n).mean(),
           "i_rmse": (s[:, G.INV_SQ] / n).sqrt().mean(), "silog_rmse": (s[:, G.LOG_SQ] / n - s[:, G.LOG] ** 2 / n ** 2).mean().sqrt() * 100}
    for k, v in want.items():
        assert float(got[k]) == pytest.approx(v, rel=1e-12), k
    assert torch.equal(s[:, G.SUM_PG], (torch.from_numpy(pred).double() * torch.from_numpy(gt).double() * torch.from_numpy(mask)).flatten(1).sum(1))


def test_eval_terms_clip_and_mask_rules():
    nan = float("nan")
    pred = torch.tensor([[nan, 2.0, 0.5, 5.0]])
    gt = torch.tensor([[1.0, 1.0, 1.0, 1.0]])
    s = G.eval_terms_ref(pred, gt, torch.tensor([[0, 1, 255, 1]], dtype=torch.uint8), clip=(1e-3, 1.0))
    assert s[0, G.N] == 3 and s[0, G.SUM_P] == 1.0 + 0.5 + 1.0          # NaN outside the mask: nothing; 2 and 5 clipped to 1
    s = G.eval_terms_ref(pred, gt, None, clip=(1e-3, 1.0))
    assert s[0, G.N] == 4 and torch.isnan(s[0, G.SUM_P]) and s[0, G.SUM_G] == 4          # torch.clamp propagates NaN


@pytest.mark.parametrize("t", G.THRESHOLDS)
def test_threshold_ties_discriminate_a_lost_division(t):
    """max(p / g, g / p) < t with p = t g exactly: the IEEE quotient is t, not under the threshold; one ulp up neither, one ulp down under it.  A
    reciprocal-and-multiply rounds twice and lands under t on part of the ties (and not under it on part of the ulp-below cases)."""
    assert float(np.float32(t)) == t
    f = G.tie_family(t)
    for name, (pred, gt) in f.items():
        assert pred.shape == (3, 4096)
        ref = G.under_threshold_ref(pred, gt, t)
        assert ref.sum(1).tolist() == [0, 0, 4096], (name, ref.sum(1).tolist())
        rec = G.under_threshold_reciprocal(pred, gt, t)
        wrong = (rec != ref).sum(1).tolist()
        print(f"t = {t} {name}: p * (1 / g) decides differently on {wrong[0]} ties, {wrong[1]} ulp-above and {wrong[2]} ulp-below cases of 4096")
        assert wrong[0] >= 50, (name, wrong)
    pred, gt = G.tie_image(t)
    assert pred.shape == (1, 3, 4096, 3)
    s = G.eval_terms_ref(pred, gt)
    # column pred = gt: always under.  The two tie columns: rows "ulp below" under t itself; all three rows under every larger threshold, none under a smaller one.
    want = [4096 * 3 + 2 * 4096 * (3 if thr > t else 1 if thr == t else 0) for thr in G.THRESHOLDS]
    assert s[0, [G.D1, G.D2, G.D3]].tolist() == want and s[0, G.N] == 9 * 4096


def emulate_parent_variance(c_pred, c_gt, n):
    """S_LOG_SQ / n - S_LOG^2 / n^2 as the kernel before the fix accumulated it: dl in fp32, its square rounded to fp32, n-fold float64 addition."""
    dl = np.log(np.float32(c_pred)) - np.log(np.float32(c_gt))
    assert dl.dtype == np.float32
    sq = np.float64(dl * dl)
    s_sq = s = np.float64(0.0)
    for _ in range(n):
        s_sq += sq
        s += np.float64(dl)
    return s_sq / n - s * s / (n * n), float(dl)


def test_constant_log_difference_family_discriminates_an_fp32_square():
    cases = G.const_log_cases()
    assert len(cases) == 72 and all(0.01 <= min(a, b) and max(a, b) <= 50 for a, b, _ in cases)
    var = [emulate_parent_variance(*c) for c in cases]
    negative = sum(v < 0 for v, _ in var)
    worst = max(abs(v) ** 0.5 / abs(dl) for v, dl in var)
    print(f"fp32 square: variance negative in {negative} of {len(cases)} cases; sqrt|variance| up to {worst:.2e} |dl|")
    assert negative >= len(cases) // 4
    # squared in float64 the same sums give a variance of at most a few float64 roundings of dl^2, and exactly 0 for one pixel
    for cp, cg, n in cases:
        dl = np.float64(np.log(np.float32(cp)) - np.log(np.float32(cg)))
        s_sq = s = np.float64(0.0)
        for _ in range(n):
            s_sq += dl * dl
            s += dl
        v = s_sq / n - s * s / (n * n)
        assert abs(v) <= 4 * n * 2.0 ** -53 * dl * dl and (n > 1 or v == 0.0), (cp, cg, n, v)


@pytest.mark.parametrize("name", G.EVAL_FAMILIES)
def test_value_domain_fp32_terms_against_fp64(name):
    """The figures behind the GPU tolerance: relative error of fp32 per-pixel terms (eval_terms_ref) against float64 terms (eval_terms_fp64), per sum."""
    pred, gt, mask = G.eval_family(name)
    clip = G.EVAL_CLIP.get(name)
    r32 = G.eval_terms_ref(pred, gt, mask, clip=clip)
    r64, mag, logs = G.eval_terms_fp64(pred, gt, mask, clip=clip, with_abs=True)
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all())
    rel = torch.where(r32 == r64, torch.zeros_like(r64), (r32 - r64).abs() / r64.abs()).max(0).values
    print(f"{name}: fp32 terms against float64 terms, relative difference of the sums: " + ", ".join(f"{G.NAMES[k]} {float(rel[k]):.1e}" for k in range(15) if float(rel[k])))
    for k in G.LINEAR + (G.D1, G.D2, G.D3):
        assert torch.equal(r32[:, k], r64[:, k]), G.NAMES[k]          # values of fp32 maps and counts: nothing to round (no threshold tie in these families)
    if name == "identical":
        assert torch.equal(r32[:, G.ABS_REL:G.LOG10_ABS + 1], torch.zeros(2, 6, dtype=torch.float64)) and torch.equal(r32[:, G.D1], r32[:, G.N])
