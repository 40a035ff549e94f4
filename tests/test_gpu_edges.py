"""hip_ext.edges and the edge metrics of src/util/metric.py on the device against tests/_edges_ref.py (plain numpy, pinned against scipy.ndimage in
test_edges_cpu.py).  Stage by stage: the pre-transform, the detector's front end (smoothed map within one fp32 ulp, the suppressed magnitude at every
pixel whose decisions are not within rounding distance of flipping), hysteresis, the distance transform and the sums bit for bit or within the bound
of their summation, then the public functions end to end on scenes without any undecided pixel, and the dataset runner's flag."""
import functools
import math

import numpy as np
import pytest
import torch

import _components_ref as C
import _edges_ref as R

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (2, 2), (3, 3), (1, 67), (67, 1), (5, 4), (33, 41), (47, 61), (64, 64), (65, 65), (31, 97))
EPS32 = float(np.finfo(np.float32).eps)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _within_one_ulp(got, want):
    """|got - want| <= one fp32 ulp of want (exact where want is 0 or infinite)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    fin = np.isfinite(want)
    ok = np.where(fin, np.abs(got.astype(np.float64) - np.where(fin, want, 0).astype(np.float64)) <= np.spacing(np.abs(np.where(fin, want, 0))).astype(np.float64),
                  got == want)
    return bool(ok.all())


@functools.lru_cache(maxsize=None)
def _case(shape, seed=0, sigma=1.0):
    """(log map float32, the restatement's stages, the undecided pixels): computed once, shared, never written to."""
    img = R.to_log(R.scene(seed + 100 * shape[0] + shape[1], *shape))
    st = R.stages(img, sigma)
    und = R.undecided(img, sigma)
    for a in (img, und, *st.values()):
        a.setflags(write=False)
    return img, st, und


def _check_front(img_batch, sigma, refs):
    """One device call over the batch; per image the conditions of the front end."""
    from hip_ext import edges as E
    for img, st, und in refs:
        assert und.mean() <= 0.01, "the restatement itself leaves more than 1 % of this scene undecided"
    got = E.canny(_dev(np.stack(img_batch)), sigma=sigma, stages=True)
    for b, (img, st, und) in enumerate(refs):
        assert np.array_equal(got.pre[b].cpu().numpy(), img)                                  # the identity pre-transform
        assert _within_one_ulp(got.smoothed[b].cpu().numpy(), st["smoothed"])
        lm, want = got.low_masked[b].cpu().numpy(), st["low_masked"]
        decided = ~und
        assert np.array_equal((lm > 0)[decided], (want > 0)[decided])
        assert (np.abs(lm.astype(np.float64) - want.astype(np.float64))[decided] <= R.tau(img)).all()
        ring = np.ones(img.shape, bool)
        ring[1:-1, 1:-1] = False
        assert not lm[ring].any()


# ---- 1. the pre-transform ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ("log", "log1.5"))
def test_pre_transform(hip, mode):
    """The device log map against np.log in fp64 rounded to fp32, within one fp32 ulp.  Where d <= 0: mode 'log' (to_log) gives zeros; mode 'log1.5' gives
    -inf, NOT zeros.  That is deliberate: the formula of extract_edges' default branch, log((d > 0) * max(d, eps)) / log(1.5), takes the logarithm of 0
    there, the reference does the same, and the kernel follows the formula; the expectation below is the formula's value, not an oversight."""
    from hip_ext import edges as E
    rng = np.random.default_rng(5)
    d = np.concatenate([rng.uniform(1e-4, 1.0, 2000), rng.uniform(1.0, 80.0, 500), np.float64(10.0) ** rng.uniform(-12, 6, 400), [0.0, -0.0, -1.0, -1e-9, 1e-8, 1.0, EPS32]])
    d = d.astype(np.float32)[:2900].reshape(50, 58)
    d[0, :7] = [0.0, -0.0, -1.0, -1e-9, 1e-8, 1.0, EPS32]
    got = E.canny(_dev(d), pre=mode, stages=True).pre.cpu().numpy()
    want = R.to_log(d) if mode == "log" else R.to_log15(d)
    assert _within_one_ulp(got, want)
    if mode == "log":
        assert (got[d <= 0] == 0).all() and (d <= 0).sum() >= 3
    else:      # the reference's default branch takes the logarithm of 0 there
        assert np.isneginf(got[d <= 0]).all()


# ---- 2. the front end -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_front_end(hip, shape):
    ref = _case(shape)
    _check_front([ref[0]], 1.0, [ref])


def test_front_end_batch_of_three_scenes(hip):
    refs = [_case((33, 41), seed) for seed in (0, 1, 2)]
    _check_front([r[0] for r in refs], 1.0, refs)


@pytest.mark.parametrize("sigma", (0.7, 2.5))
def test_front_end_other_sigmas(hip, sigma):
    ref = _case((47, 61), 0, sigma)
    _check_front([ref[0]], sigma, [ref])


def test_front_end_constant_and_step(hip):
    from hip_ext import edges as E
    for value in (0.0, 0.5, -3.25):
        img = np.full((40, 37), value, np.float32)
        got = E.canny(_dev(img), stages=True)
        assert _within_one_ulp(got.smoothed.cpu().numpy(), R.smooth(img, 1.0))      # bleed-over only
        assert not got.low_masked.any() and not got.edges.any()
    img = np.zeros((45, 70), np.float32)
    img[:, 33:] = 1.0                                    # the ridge straddles the tile border at column 32
    st = R.stages(img)
    got = E.canny(_dev(img), stages=True)
    lm = got.low_masked.cpu().numpy()
    assert (st["low_masked"][1:-1, 32] > 0).all() and (st["low_masked"][1:-1, 33] > 0).all()
    assert np.array_equal(lm > 0, st["low_masked"] > 0)      # two columns of exactly equal magnitudes: `<=` keeps the ridge whole
    assert np.abs(lm.astype(np.float64) - st["low_masked"]).max() <= R.tau(img)
    assert np.array_equal(got.edges.cpu().numpy(), st["edges"])


def test_front_end_rejects_a_radius_above_the_cap(hip):
    import hip_ext as H
    img = torch.zeros(1, 8, 8, device="cuda")
    with pytest.raises(H.HipExtError):
        H.canny_front(img, torch.full((2 * (H.CANNY_MAX_RADIUS + 1) + 1,), 0.1, dtype=torch.float64, device="cuda"), 0.1, torch.empty_like(img))


# ---- 3. hysteresis ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hysteresis_maps():
    rng = np.random.default_rng(7)
    maps = {}
    for shape in SHAPES:
        maps[f"random {shape}"] = np.where(rng.random(shape) < 0.3, rng.uniform(0.05, 0.3, shape), 0).astype(np.float32)
    chain = C.serpentine(65).astype(np.float32) * np.float32(0.1)
    chain[64, 64] = 0.5                                  # one strong pixel at the far end ([0, 0] is the other) of one long winding weak chain
    maps["chain"] = chain
    for anti in (False, True):
        blocks = np.zeros((70, 70), np.float32)
        blocks[28:32, 28:32] = 0.1                       # weak, touching the strong block only diagonally across the tile corner (31, 31) - (32, 32)
        blocks[32:36, 32:36] = 0.4
        blocks[5:9, 40:44] = 0.15                        # weak and alone
        maps[f"diagonal anti={anti}"] = np.ascontiguousarray(blocks[:, ::-1]) if anti else blocks
    maps["no strong pixel"] = np.where(rng.random((40, 50)) < 0.4, np.float32(0.12), 0).astype(np.float32)
    maps["exactly high"] = np.where(rng.random((40, 50)) < 0.2, np.float32(0.2), 0).astype(np.float32)
    maps["empty"] = np.zeros((33, 35), np.float32)
    return maps


def test_hysteresis(hip):
    import hip_ext as H
    for name, lm in _hysteresis_maps().items():
        t = _dev(lm[None])
        out = torch.empty(t.shape, dtype=torch.uint8, device="cuda")
        H.canny_hysteresis(t, 0.2, out)
        assert np.array_equal(out[0].cpu().numpy(), R.hysteresis(lm, 0.2)), name
    assert R.hysteresis(_hysteresis_maps()["chain"], 0.2).sum() == C.serpentine(65).sum()
    # a batch: images do not see each other's labels
    a, b = _hysteresis_maps()["chain"], _hysteresis_maps()["random (65, 65)"]
    t = _dev(np.stack([a, b, a]))
    out = torch.empty(t.shape, dtype=torch.uint8, device="cuda")
    H.canny_hysteresis(t, 0.2, out)
    for k, lm in enumerate((a, b, a)):
        assert np.array_equal(out[k].cpu().numpy(), R.hysteresis(lm, 0.2))


# ---- 4. the distance transform ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES + ((2, 1500), (1100, 3)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_distance_transform(hip, shape):
    from hip_ext import edges as E
    rng = np.random.default_rng(11)
    h, w = shape
    one = np.zeros(shape, np.uint8)
    one[h - 1, w - 1] = 1                                # a far corner: every row chunk of a long row sees it
    maps = [one, (rng.random(shape) < 0.01).astype(np.uint8), (rng.random(shape) < 0.3).astype(np.uint8), np.ones(shape, np.uint8), np.zeros(shape, np.uint8)]
    got = E.distance_transform_edt(_dev(np.stack(maps))).cpu().numpy()
    assert got.dtype == np.float64
    for k, m in enumerate(maps):
        assert np.array_equal(got[k], R.edt(m)), k
    assert np.isinf(got[4]).all() and not got[3].any()
    assert np.array_equal(E.distance_transform_edt(_dev(maps[2].astype(bool))).cpu().numpy(), got[2])      # [h, w] in, [h, w] out; bool accepted


# ---- 5. sums and metrics ----------------------------------------------------------------------------------------------------------------------

def _close(got, want, n_terms):
    return got == want or abs(got - want) <= n_terms * 2.0 ** -52 * abs(want)


@pytest.mark.parametrize("shape", ((5, 4), (47, 61), (65, 65)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_sums(hip, shape):
    from hip_ext import edges as E
    import hip_ext as H
    from src.util import metric
    rng = np.random.default_rng(13)
    pe, ge = (rng.random(shape) < 0.05).astype(np.uint8), (rng.random(shape) < 0.05).astype(np.uint8)
    pe[0, 0] = ge[-1, -1] = 1
    ge[0, 0] = 0
    dt, dp = R.edt(ge), R.edt(pe)
    valids = [np.zeros(shape, np.uint8), np.ones(shape, np.uint8), (rng.random(shape) < 0.6).astype(np.uint8)]
    B = len(valids)
    stack = lambda a: _dev(np.stack([a] * B))      # noqa: E731
    for th in (10.0, 3.0):
        s = E.edge_sums(stack(pe), stack(ge), _dev(np.stack(valids)), stack(dt), stack(dp), th).cpu().numpy()
        m = metric._edge_from_sums(torch.from_numpy(s).cuda(), th, th + 1)
        for b, v in enumerate(valids):
            bde = (pe > 0) & (v > 0) & (dt < th)
            gsel = (ge > 0) & (v > 0)
            assert s[b, H.EDGE_N_BDE] == bde.sum() and s[b, H.EDGE_N_GT] == gsel.sum()
            assert _close(s[b, H.EDGE_SUM_DT], math.fsum(dt[bde]), max(int(bde.sum()), 1))
            assert _close(s[b, H.EDGE_SUM_DP], math.fsum(dp[gsel]), max(int(gsel.sum()), 1))
            acc, comp = float(m["EdgeAcc"][b]), float(m["EdgeComp"][b])
            if not bde.sum():
                assert acc == th and comp == th + 1                         # the fallback
            else:
                assert _close(acc, math.fsum(dt[bde]) / bde.sum(), int(bde.sum()) + 1)
                assert _close(comp, math.fsum(dp[gsel]) / gsel.sum(), int(gsel.sum()) + 1)
    # close predicted edges, every ground-truth edge invalid: 0 / 0
    v = (ge == 0).astype(np.uint8)
    s = E.edge_sums(_dev(pe), _dev(ge), _dev(v), _dev(dt), _dev(dp), 1e9)
    m = metric._edge_from_sums(s)
    assert float(s[0, H.EDGE_N_BDE]) > 0 and float(s[0, H.EDGE_N_GT]) == 0 and math.isnan(float(m["EdgeComp"][0])) and not math.isnan(float(m["EdgeAcc"][0]))
    # no valid mask at all = every pixel
    assert torch.equal(E.edge_sums(_dev(pe), _dev(ge), None, _dev(dt), _dev(dp)), E.edge_sums(_dev(pe), _dev(ge), _dev(np.ones(shape, np.uint8)), _dev(dt), _dev(dp)))


@pytest.mark.parametrize("shape", ((5, 2), (2, 5), (33, 41), (65, 65)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("radius", (0, 1, 3))
def test_soft_edge_error(hip, shape, radius):
    from hip_ext import edges as E
    from src.util import metric
    rng = np.random.default_rng(17)
    pred, gt = rng.uniform(0.05, 1.0, shape).astype(np.float32), rng.uniform(0.05, 1.0, shape).astype(np.float32)
    valids = [np.zeros(shape, np.uint8), np.ones(shape, np.uint8), (rng.random(shape) < 0.6).astype(np.uint8)]
    s = E.soft_edge_sums(_dev(np.stack([pred] * 3)), _dev(np.stack([gt] * 3)), _dev(np.stack(valids)), radius).cpu().numpy()
    for b, v in enumerate(valids):
        see, mean = R.soft_edge_error(pred, gt, v, radius)
        n = int(v.sum())
        assert s[b, 0] == n
        assert _close(s[b, 1], math.fsum(see[v > 0].astype(np.float64)), max(n, 1))
        got = float(metric.soft_edge_error(_dev(pred), _dev(gt), _dev(v.astype(bool)), radius))
        assert (math.isnan(got) and math.isnan(mean)) if n == 0 else _close(got, mean, n + 1)


def test_soft_edge_radius_cap(hip):
    import hip_ext as H
    from hip_ext import edges as E
    x = torch.zeros(1, 4, 4, device="cuda")
    with pytest.raises(ValueError):
        E.soft_edge_sums(x, x, None, H.SOFT_EDGE_MAX_RADIUS + 1)
    with pytest.raises(H.HipExtError):
        H.soft_edge(x, x, None, H.SOFT_EDGE_MAX_RADIUS + 1, torch.empty(1, 2, dtype=torch.float64, device="cuda"))


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", tuple(R.SEEDS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_end_to_end_on_decided_scenes(hip, shape):
    from src.util import metric
    rng = np.random.default_rng(19)
    seeds = R.SEEDS[shape]
    depth = [R.scene(s, *shape) for s in seeds]
    edges = [R.canny(R.to_log(d)) for d in depth]
    for d, e in zip(depth, edges):
        got = metric.extract_edges(_dev(d), preprocess="log")
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), e.astype(bool)) and e.sum() >= 30
    batch = metric.extract_edges(_dev(np.stack(depth))[:, None], preprocess="log")          # [B, 1, H, W] squeezes to a batch
    assert np.array_equal(batch.cpu().numpy(), np.stack(edges).astype(bool))
    gts = depth[1:] + depth[:1]
    gt_edges = edges[1:] + edges[:1]
    valid = [(rng.random(shape) < 0.8) for _ in seeds]
    both = metric.edge_metrics(_dev(np.stack(depth)), _dev(np.stack(gts)), _dev(np.stack(valid)))
    assert both["EdgeAcc"].dtype == torch.float64 and both["EdgeAcc"].shape == (3,)
    for k in range(3):
        p, g, v = _dev(depth[k]), _dev(gts[k]), _dev(valid[k])
        acc, comp = metric.EdgeAcc(p[None, None], g[None, None], v[None, None]), metric.EdgeComp(p, g, v)
        assert acc.dim() == 0 and acc.dtype == torch.float64 and acc.is_cuda
        one = metric.edge_metrics(p, g, v)
        # the batch against the single calls, bit for bit
        assert float(acc) == float(one["EdgeAcc"][0]) == float(both["EdgeAcc"][k]) and float(comp) == float(one["EdgeComp"][0]) == float(both["EdgeComp"][k])
        want_acc, want_comp = R.edge_acc_comp(edges[k], gt_edges[k], valid[k])
        # each metric's own number of terms, plus one for the division
        n_bde = int((edges[k].astype(bool) & valid[k] & (R.edt(gt_edges[k]) < 10)).sum())
        n_gt = int((gt_edges[k].astype(bool) & valid[k]).sum())
        assert _close(float(acc), want_acc, n_bde + 1) and _close(float(comp), want_comp, n_gt + 1), (k, float(acc), want_acc, float(comp), want_comp)
        assert 0 < want_acc < 10 and 0 < want_comp


def test_extract_edges_other_preprocessing(hip):
    from src.util import metric
    shape = (33, 41)
    d = R.scene(R.SEEDS[shape][0], *shape)
    assert not R.undecided(R.to_log15(d)).any()
    want = R.canny(R.to_log15(d)).astype(bool)
    for pre in (None, "none"):      # the reference's default branch: log(d) / log(1.5)
        assert np.array_equal(metric.extract_edges(_dev(d), preprocess=pre).cpu().numpy(), want) and want.sum() >= 30
    inv = metric.extract_edges(_dev(d), preprocess="inv")
    assert inv.dtype == torch.bool and inv.shape == shape and inv.any()


# ---- 7. the runner ----------------------------------------------------------------------------------------------------------------------------

def test_runner_edge_metrics(hip, tmp_path):
    from PIL import Image
    from oracle import metrics_oracle as MO
    from src.scripts import amodal_dav2_inference as S
    from src.util import alignment, metric
    rng = np.random.default_rng(0)
    ids = ["21", "22"]
    d = {k: tmp_path / k for k in ("occ", "whole", "obs", "gt")}
    for v in d.values():
        v.mkdir()
    for sid in ids:
        Image.fromarray((rng.random((64, 64, 3)) * 255).astype(np.uint8)).save(d["occ"] / f"{sid}_occlusion.png")
        m = np.zeros((64, 64), dtype=np.uint8)
        m[10:50, 8:40] = 255
        Image.fromarray(m).save(d["whole"] / f"{sid}_whole_mask.png")
        Image.fromarray((rng.uniform(0.2, 0.9, size=(32, 32)) * 65535).astype(np.uint16)).save(d["obs"] / f"{sid}_depth.png")
        Image.fromarray((rng.uniform(0.2, 0.9, size=(128, 128)) * 65535).astype(np.uint16)).save(d["gt"] / f"{sid}_depth.png")
    seen = []

    def model(x, guide_rgb=None, guide_mask=None, observation=None):      # a stand-in network: the runner's plumbing is what is under test
        out = (observation + 1) / 2 * 0.5 + 0.25 + 0.05 * x[:, :1]
        seen.append(out)
        return out
    args = (model, ids, str(d["occ"]), str(d["whole"]), str(d["obs"]))
    plain = S.run(*args, str(tmp_path / "o1"), str(d["gt"]), batch_size=2, device="cuda")
    got = S.run(*args, str(tmp_path / "o2"), str(d["gt"]), batch_size=2, device="cuda", edge_metrics=True)
    assert set(plain) == set(MO.ALL) and set(got) == set(MO.ALL) | {"EdgeAcc", "EdgeComp", "soft_edge_error"}
    for k in MO.ALL:      # the other metrics are untouched by the flag (their sums come from fp64 atomics: equal up to the order of the additions)
        assert got[k] == pytest.approx(plain[k], rel=1e-12), k
    want = {"EdgeAcc": 0.0, "EdgeComp": 0.0, "soft_edge_error": 0.0}
    pred = seen[-1].reshape(2, 518, 518).float()
    for b, sid in enumerate(ids):
        s = S.load_sample(sid, str(d["occ"]), str(d["whole"]), str(d["obs"]), str(d["gt"]))
        gt = s["gt_depth"].cuda().reshape(518, 518)
        valid = s["whole_mask"].cuda().reshape(518, 518) & (gt > 0)
        ss = alignment.scale_shift_least_square(gt[None], pred[b:b + 1], valid[None]).float()
        aligned = (pred[b] * ss[0, 0] + ss[0, 1]).clamp(1e-3, 1.0)
        want["EdgeAcc"] += float(metric.EdgeAcc(aligned, gt, valid)) / 2
        want["EdgeComp"] += float(metric.EdgeComp(aligned, gt, valid)) / 2
        want["soft_edge_error"] += float(metric.soft_edge_error(aligned, gt, valid)) / 2
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-12), k
    assert 0 < got["EdgeAcc"] <= 10 and got["soft_edge_error"] > 0
    with pytest.raises(ValueError, match="paper"):
        S.run(*args, str(tmp_path / "o3"), str(d["gt"]), device="cuda", protocol="paper", visible_mask_dir=str(d["whole"]), edge_metrics=True)
