"""CPU: the host side of the paper's evaluation protocol (src/util/validation.py, the dataset runner's --protocol paper) and its fp64
restatement (tests/_protocol_ref.py) against what the reference's own validate_single_dataset returned (tests/golden/protocol/cases.npz)."""
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F
from PIL import Image

import _protocol_ref as PR
from src.scripts import amodal_dav2_inference as R
from src.util import validation as V


@pytest.fixture(scope="module")
def golden():
    samples, rec = PR.load_golden()
    results = [PR.evaluate_sample(s["pred"], s["gt"], s["obs"], s["whole"], s["visible"], s["invisible"], s["valid"]) for s in samples]
    return samples, rec, results


def test_golden_dataset_holds_the_cases_it_was_built_for(golden):
    samples, rec, _ = golden
    assert 12 <= len(samples) <= 16 and {s["gt"].shape for s in samples} == {(37, 53), (74, 74)}
    ratios = [(int(s["visible"].sum()), int(s["whole"].sum())) for s in samples]
    assert {V.bucket_of(*r) for r in ratios} == {"easy", "mid", "diff"}
    assert (300, 400) in ratios and (200, 400) in ratios                              # exactly 0.75 and exactly 0.5
    nan = np.isnan(rec["values"])                                                     # [sample, raw | aligned, metric]
    assert any(nan[i].all() and not (s["invisible"] & s["valid"]).any() for i, s in enumerate(samples))      # empty region
    log_based = np.array([m in ("rmse_log", "log10", "silog_rmse") for m in V.METRICS])
    assert any((nan[i, 1] == log_based).all() and not nan[i, 0].any() for i in range(len(samples)))          # negative aligned values
    assert any(not s["visible"].any() for s in samples)                               # empty visible mask
    assert any(s["visible"].any() and np.ptp(s["pred"][s["visible"]]) == 0 for s in samples if s["pred"].shape == s["gt"].shape)
    assert any(s["pred"].shape == (28, 42) and s["gt"].shape == (37, 53) for s in samples)
    assert any((s["gt"] == 0).any() for s in samples)                                 # holes
    for s in samples:
        code = s["gt"].astype(np.float64) * 65535
        assert np.array_equal(s["valid"], s["gt"] > 0) and float(np.abs(code - np.round(code)).max()) < 1e-2      # gt on the 1 / 65535 grid


def test_restatement_reproduces_the_reference(golden):
    samples, rec, results = golden
    np.testing.assert_allclose([r.scale for r in results], rec["scale"], rtol=1e-5)
    np.testing.assert_allclose([r.shift for r in results], rec["shift"], rtol=1e-5, atol=1e-6)
    tracker = V.ValidationTracker()
    for i, r in enumerate(results):
        for row, values in enumerate((r.raw, r.aligned)):
            for j, m in enumerate(V.METRICS):
                assert math.isnan(values[m]) == bool(np.isnan(rec["values"][i, row, j])), (i, row, m)
        tracker.update(r)
    means, counts = tracker.result(), tracker.counts()
    for gi, g in enumerate(V.GROUPS):
        for j, m in enumerate(V.METRICS):
            assert counts[g][m] == int(rec["counts"][gi, j]), (g, m)
            assert means[g][m] == pytest.approx(float(rec["means"][gi, j]), rel=2e-5, abs=1e-7), (g, m)


def test_bucket_boundaries_and_nan():
    assert V.bucket_of(301, 400) == "easy" and V.bucket_of(300, 400) == "mid"          # > 0.75, not >=
    assert V.bucket_of(201, 400) == "mid" and V.bucket_of(200, 400) == "diff"
    assert V.bucket_of(0, 400) == "diff" and V.bucket_of(400, 400) == "easy"
    assert V.bucket_of(0, 0) == "diff"                                                # 0 / 0 is NaN: every comparison false
    assert V.bucket_of(5, 0) == "easy"                                                # inf
    # the ratio is a float32 quotient, as torch's int / int
    nv, nw = 3 * 2 ** 24 + 1, 2 ** 26                                                 # above 0.75 in exact arithmetic, 0.75 once nv is a float32
    assert float(torch.tensor(nv) / torch.tensor(nw)) == 0.75 and V.bucket_of(nv, nw) == "mid"


def test_tracker_skips_nan_per_metric():
    nan = float("nan")
    base = {m: 1.0 for m in V.METRICS}
    t = V.ValidationTracker()
    t.update(V.SampleResult(dict(base), dict(base, rmse_log=nan, log10=nan, silog_rmse=nan), 1.0, 0.0, "mid", 3, 5))
    t.update(V.SampleResult({m: 3.0 for m in V.METRICS}, {m: 5.0 for m in V.METRICS}, 1.0, 0.0, "easy", 4, 5))
    t.update(V.SampleResult({m: nan for m in V.METRICS}, {m: nan for m in V.METRICS}, 0.0, 0.0, "diff", 0, 5))
    res, cnt = t.result(), t.counts()
    assert set(res) == set(V.GROUPS) and all(set(res[g]) == set(V.METRICS) for g in V.GROUPS)
    assert cnt["overall"]["rmse_log"] == 2 and res["overall"]["rmse_log"] == 2.0
    assert cnt["align_overall"]["rmse_log"] == 1 and res["align_overall"]["rmse_log"] == 5.0
    assert cnt["align_overall"]["rmse_linear"] == 2 and res["align_overall"]["rmse_linear"] == 3.0
    assert cnt["align_mid"]["log10"] == 0 and res["align_mid"]["log10"] == 0.0 and cnt["align_mid"]["i_rmse"] == 1
    assert all(c == 0 for g in ("diff", "align_diff") for c in cnt[g].values())
    vec = t.state_vector()
    assert len(vec) == 2 * len(V.GROUPS) * len(V.METRICS)
    u = V.ValidationTracker()
    u.load_state_vector([2 * v for v in vec])                                          # two ranks with the same share
    assert u.result() == res and u.counts()["overall"]["rmse_log"] == 4


@pytest.mark.parametrize("n_in,n_out", [(518, 53), (53, 518), (28, 37), (42, 53), (74, 37), (37, 74), (7, 7), (1, 5), (5, 1), (518, 517)])
def test_nearest_index_rule_is_atens(n_in, n_out):
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
    want = F.interpolate(src, size=(1, n_out), mode="nearest").view(-1).long().numpy()
    assert np.array_equal(PR.nearest_index(n_out, n_in), want)
    want_rows = F.interpolate(src.view(1, 1, n_in, 1), size=(n_out, 1), mode="nearest").view(-1).long().numpy()
    assert np.array_equal(PR.nearest_index(n_out, n_in), want_rows)


def test_restatement_resizes_like_interpolate():
    g = torch.Generator().manual_seed(0)
    p = torch.rand(2, 28, 42, generator=g)
    want = F.interpolate(p[:, None], size=(37, 53), mode="nearest")[:, 0].numpy()
    assert np.array_equal(PR.resize_nearest(p.numpy(), 37, 53), want)


def test_validate_single_dataset_host_glue_returns_the_golden_dict(golden):
    """The drop-in's glue (batch keys, guide ranges, tracker) with the restatement as the evaluator; the device evaluator is tested on the GPU."""
    samples, rec, _ = golden
    batches, model, calls = PR.golden_loader(samples)
    res = V.validate_single_dataset(model, batches, "cpu", evaluate=PR.evaluate_batch)
    assert len(calls) == len(samples) and all(c[0] <= 1.0 and c[1] == -1.0 and c[2] == 1.0 and -1.0 <= c[3] <= c[4] <= 1.0 for c in calls)
    assert list(res) == list(V.GROUPS)
    for gi, g in enumerate(V.GROUPS):
        for j, m in enumerate(V.METRICS):
            assert res[g][m] == pytest.approx(float(rec["means"][gi, j]), rel=2e-5, abs=1e-7), (g, m)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------------------------------
IDS = ["101", "102", "103", "104", "105"]


def _make_tree(tmp, ids):
    rng = np.random.default_rng(7)
    d = {k: tmp / k for k in ("occ", "whole", "obs", "gt", "vis")}
    for v in d.values():
        v.mkdir()
    for n, sid in enumerate(ids):
        Image.fromarray((rng.random((64, 64, 3)) * 255).astype(np.uint8)).save(d["occ"] / f"{sid}_occlusion.png")
        m = np.zeros((64, 64), dtype=np.uint8); m[10:50, 8:40] = 255
        Image.fromarray(m).save(d["whole"] / f"{sid}_whole_mask.png")
        v = np.zeros((64, 64), dtype=np.uint8); v[10:10 + (36, 24, 10, 30, 20)[n % 5], 8:40] = 255          # 0.9, 0.6, 0.25, 0.75, 0.5 of the object
        Image.fromarray(v).save(d["vis"] / f"{sid}_visible_mask.png")
        Image.fromarray((rng.uniform(0.2, 0.9, size=(32, 32)) * 65535).astype(np.uint16)).save(d["obs"] / f"{sid}_depth.png")
        gt = (rng.uniform(0.2, 0.9, size=(128, 128)) * 65535).astype(np.uint16)
        gt[rng.uniform(size=gt.shape) < 0.05] = 0
        Image.fromarray(gt).save(d["gt"] / f"{sid}_depth.png")
    return {k: str(v) for k, v in d.items()}


def _model(x, guide_rgb=None, guide_mask=None, observation=None):
    return (observation + 1) / 2 * 0.5 + 0.2 + 0.05 * x[:, :1]


def _run(tree, ids, out, **kw):
    return R.run(_model, ids, tree["occ"], tree["whole"], tree["obs"], out, tree["gt"], batch_size=2, device="cpu", evaluate=PR.evaluate_batch,
                 protocol="paper", visible_mask_dir=tree["vis"], **kw)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, tree, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, json.dumps([_run(tree, IDS, out + "/five"), _run(tree, IDS[:1], out + "/one")])))
    finally:
        dist.destroy_process_group()


def test_runner_paper_protocol_sharded_equals_unsharded(tmp_path):
    """--protocol paper over 2 gloo ranks: 5 samples (shards of 3 and 2) and 1 sample (one rank's shard is empty) give the unsharded JSON on
    every rank -- counts exactly, means up to the order of the fp64 additions."""
    tree = _make_tree(tmp_path, IDS)
    single = [_run(tree, IDS, str(tmp_path / "s5")), _run(tree, IDS[:1], str(tmp_path / "s1"))]
    assert list(single[0]) == list(V.GROUPS) + ["counts"]
    assert [single[0]["counts"][g]["abs_relative_difference"] for g in ("easy", "mid", "diff", "overall")] == [1, 2, 2, 5]
    assert single[0]["counts"]["align_overall"]["delta1_acc"] == 5 and single[1]["counts"]["overall"]["rmse_log"] == 1
    assert 0 < single[0]["align_overall"]["abs_relative_difference"] < 2
    json.loads(json.dumps(single))                                                    # what main() writes to metrics.json
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, tree, str(tmp_path / "sharded"))) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert sorted(os.listdir(tmp_path / "sharded" / "five" / "amodal_depth")) == [f"{i}_depth.png" for i in IDS]
    for r in (0, 1):
        for got, want in zip(json.loads(res[r]), single):
            assert got["counts"] == want["counts"]
            for g in V.GROUPS:
                for m in V.METRICS:
                    assert got[g][m] == pytest.approx(want[g][m], rel=1e-12, abs=0), (r, g, m)


def test_runner_legacy_default_is_untouched(tmp_path):
    """Without --protocol the runner evaluates as before: one flat dict of means, the evaluator called per sample with (pred, gt, mask)."""
    tree = _make_tree(tmp_path, IDS[:2])
    seen = []

    def evaluate(pred, gt, mask):
        seen.append((tuple(pred.shape), bool(mask.any())))
        return {"m": float(pred.mean())}
    res = R.run(_model, IDS[:2], tree["occ"], tree["whole"], tree["obs"], str(tmp_path / "o"), tree["gt"], batch_size=2, device="cpu", evaluate=evaluate)
    assert set(res) == {"m"} and seen == [((1, 518, 518), True)] * 2
    with pytest.raises(ValueError):
        R.run(_model, IDS[:2], tree["occ"], tree["whole"], tree["obs"], str(tmp_path / "o"), tree["gt"], device="cpu", protocol="paper")
