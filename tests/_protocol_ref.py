"""TEST INFRASTRUCTURE ONLY -- fp64 numpy restatement of the paper's evaluation protocol (reference: src/trainer/discriminative_trainer.py:496-613),
built on oracle.metrics_oracle: nearest resize of the prediction, least-squares fit onto the observation over the visible mask
(numpy.linalg.lstsq: minimum norm where the system is rank deficient), the ten metrics over ``invisible & valid`` of the raw and the aligned
prediction with + eps on both sides, the bucket.  Pinned against the reference's own method by tests/golden/protocol/cases.npz
(tools/make_protocol_golden.py).  ``evaluate_batch`` has the signature and the return type of src.util.validation.evaluate_batch, so it can stand
in for it where there is no device."""
import os
import warnings

import numpy as np

from oracle import metrics_oracle as MO
from src.util.validation import GROUPS, METRICS, SampleResult, bucket_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "protocol", "cases.npz")
assert tuple(MO.ALL) == tuple(METRICS)


def nearest_index(out_size, in_size):
    """ATen's legacy nearest rule: min(floorf(dst * ((float)in / out)), in - 1), the arithmetic in float32."""
    scale = np.float32(in_size) / np.float32(out_size)
    return np.minimum(np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64), in_size - 1)


def resize_nearest(pred, h, w):
    pred = np.asarray(pred)
    return pred[..., nearest_index(h, pred.shape[-2]), :][..., nearest_index(w, pred.shape[-1])]


def fit(pred, obs, visible):
    """(scale, shift) of one image in fp64; lstsq's minimum-norm answer without support or with a constant prediction."""
    m = np.asarray(visible) != 0
    p, o = np.asarray(pred, np.float64)[m], np.asarray(obs, np.float64)[m]
    if p.size == 0:
        return 0.0, 0.0
    (scale, shift), *_ = np.linalg.lstsq(np.stack([p, np.ones_like(p)], 1), o, rcond=None)
    return float(scale), float(shift)


def evaluate_sample(pred, gt, obs, whole, visible, invisible=None, valid=None, eps=1e-5):
    gt = np.asarray(gt, np.float64)
    h, w = gt.shape
    p = resize_nearest(np.asarray(pred, np.float64), h, w)
    whole, visible = np.asarray(whole) != 0, np.asarray(visible) != 0
    region = (whole & ~visible) if invisible is None else (np.asarray(invisible) != 0)
    if valid is not None:
        region = region & (np.asarray(valid) != 0)
    scale, shift = fit(p, obs, visible)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        raw = MO.depth_metrics(p + eps, gt + eps, region)
        aligned = MO.depth_metrics(p * scale + shift + eps, gt + eps, region)
    nv, nw = int(visible.sum()), int(whole.sum())
    return SampleResult(raw, aligned, scale, shift, bucket_of(nv, nw), nv, nw)


def evaluate_batch(pred, gt, observation, whole, visible, invisible=None, valid=None, eps=1e-5):
    """Tensors (any device) or arrays [B, ...] in, a list of SampleResult out."""
    def arr(t):
        if t is None:
            return None
        a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        return a[:, 0] if a.ndim == 4 else a
    pred, gt, observation, whole, visible, invisible, valid = (arr(t) for t in (pred, gt, observation, whole, visible, invisible, valid))
    return [evaluate_sample(pred[b], gt[b], observation[b], whole[b], visible[b], None if invisible is None else invisible[b],
                            None if valid is None else valid[b], eps) for b in range(gt.shape[0])]


def load_golden():
    """-> (samples, recorded): samples a list of dicts (pred, gt, obs fp32; whole, visible, invisible, valid bool), recorded the reference's results."""
    g = np.load(GOLDEN)
    samples = []
    for i in range(int(g["n"])):
        s = {k: g[f"s{i}.{k}"] for k in ("whole", "visible", "invisible", "valid")}
        s["pred"] = (g[f"s{i}.pred16"] / 65536.0).astype(np.float32)
        s["gt"] = (g[f"s{i}.gt16"] / 65535.0).astype(np.float32)
        s["obs"] = (g[f"s{i}.obs16"] / 65535.0).astype(np.float32)
        samples.append(s)
    assert tuple(g["metrics"]) == tuple(METRICS) and tuple(g["groups"]) == tuple(GROUPS)
    return samples, {k: g[k] for k in ("means", "counts", "scale", "shift", "values")}


def golden_loader(samples):
    """The samples as the batches the reference's loader yields (batch size 1) and a stand-in model that returns their predictions in order."""
    import torch

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a))[None, None]
    batches = []
    for s in samples:
        h, w = s["gt"].shape
        batches.append(dict(rgb_int=torch.zeros(1, 3, h, w), guide_rgb_norm=torch.zeros(1, 3, h, w), guide=t(s["whole"]), depth_observation=t(s["obs"]),
                            depth_gt=t(s["gt"]), valid_mask_raw=t(s["valid"]), visible_mask=t(s["visible"]), invisible_mask=t(s["invisible"])))
    calls = []

    def model(rgb, guide_rgb=None, guide_mask=None, observation=None):
        calls.append((float(rgb.max()), float(guide_mask.min()), float(guide_mask.max()), float(observation.min()), float(observation.max())))
        return torch.from_numpy(samples[len(calls) - 1]["pred"])[None, None].to(rgb.device)
    return batches, model, calls
