"""The paper's evaluation protocol on the device: the reference trainer's ``validate_single_dataset``
(``src/trainer/discriminative_trainer.py:471-670``) and its stand-alone twin ``src/scripts/pix2gestalt_eval.py:200-303``.

Per sample the reference
  * resizes the prediction to the ground truth's size with ``F.interpolate(mode='nearest')``,
  * fits it onto the depth OBSERVATION over the VISIBLE mask (``align_depth_least_square``),
  * evaluates every metric over the INVISIBLE part of the object (``invisible & valid``), once on the raw and once on the aligned
    prediction, both with ``+ 1e-5`` on prediction and ground truth,
  * files the sample under easy / mid / diff by the ratio of visible to whole-object pixels (> 0.75, > 0.5, else),
  * and skips a metric whose value is NaN -- for that metric only.
Here a batch costs two library calls (``ada_protocol_fit_fwd``, ``ada_protocol_eval_fwd``: the nearest gather, the fit and every sum on the
device, without atomics) and one read of a ``[B, 12 + 32]`` fp64 block; the bucket, the ten metrics of a sample and the running means are host
arithmetic on those numbers.  There is no CPU fallback.
"""
from typing import Callable, Dict, Iterable, List, NamedTuple, Optional

import numpy as np
import torch

import hip_ext as H
from src.util import metric
from src.util.metric import MetricTracker

__all__ = ["METRICS", "GROUPS", "SampleResult", "bucket_of", "samples_from_rows", "evaluate_batch", "ValidationTracker", "validate_single_dataset"]

METRICS = ("abs_relative_difference", "squared_relative_difference", "rmse_linear", "rmse_log", "log10", "delta1_acc", "delta2_acc", "delta3_acc",
           "i_rmse", "silog_rmse")
GROUPS = ("easy", "mid", "diff", "overall", "align_easy", "align_mid", "align_diff", "align_overall")


class SampleResult(NamedTuple):
    raw: Dict[str, float]        # metric name -> value of the raw prediction over the region (NaN where the reference's would be)
    aligned: Dict[str, float]    # the same for the aligned prediction
    scale: float
    shift: float
    bucket: str                  # "easy" | "mid" | "diff"
    n_visible: int
    n_whole: int


def bucket_of(n_visible, n_whole) -> str:
    """The reference's difficulty bucket (discriminative_trainer.py:558-568): the ratio of two pixel counts in float32; > 0.75 easy, > 0.5 mid,
    anything else -- a NaN from 0 / 0 included -- diff."""
    with np.errstate(all="ignore"):
        ratio = np.float32(float(n_visible)) / np.float32(float(n_whole))
    return "easy" if ratio > 0.75 else "mid" if ratio > 0.5 else "diff"


def samples_from_rows(fit: torch.Tensor, sums: torch.Tensor) -> List[SampleResult]:
    """fit fp64 [B, FIT_NCOL], sums fp64 [B, 2, EVAL_NSUM] on the host -> one SampleResult per image (metric._from_sums on one-image batches: the
    reference evaluates with batch size 1)."""
    out = []
    for b in range(fit.shape[0]):
        raw, aligned = ({k: float(v) for k, v in metric._from_sums(sums[b, r][None]).items()} for r in (0, 1))
        nv, nw = int(fit[b, H.FIT_N_VISIBLE]), int(fit[b, H.FIT_N_WHOLE])
        out.append(SampleResult(raw, aligned, float(fit[b, H.FIT_SCALE]), float(fit[b, H.FIT_SHIFT]), bucket_of(nv, nw), nv, nw))
    return out


def _maps(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3:
        raise ValueError(f"{name}: expected [B, H, W] or [B, 1, H, W], got {tuple(t.shape)}")
    return t


def _mask(t: torch.Tensor, name: str) -> torch.Tensor:
    t = _maps(t, name)
    if t.dtype not in (torch.bool, torch.uint8):
        t = t != 0
    return t.contiguous()


def evaluate_batch(pred, gt, observation, whole, visible, invisible=None, valid=None, eps: float = 1e-5) -> List[SampleResult]:
    """One batch by the protocol.  ``pred`` fp32 [B, hp, wp] (any size: gathered to the ground truth's by the nearest rule inside the kernels);
    ``gt`` / ``observation`` [B, h, w]; ``whole`` / ``visible`` / ``invisible`` / ``valid`` masks [B, h, w] (non-zero = inside).  ``invisible``
    defaults to ``whole & ~visible`` (pix2gestalt_eval.py:281); the metrics are summed over ``invisible & valid``.  Two launches, one host read."""
    pred = _maps(pred, "pred").contiguous().float()
    gt = _maps(gt, "gt").contiguous().float()
    observation = _maps(observation, "observation").contiguous().float()
    whole, visible = _mask(whole, "whole"), _mask(visible, "visible")
    if invisible is None:
        invisible = (whole != 0) & (visible == 0)
    invisible = _mask(invisible, "invisible")
    valid = None if valid is None else _mask(valid, "valid")
    B, h, w = gt.shape
    ws = torch.empty(H.protocol_workspace_bytes(B, h, w) // 8, dtype=torch.float64, device=pred.device)
    fit = H.protocol_fit(pred, observation, visible, whole, workspace=ws)
    sums = H.protocol_eval(pred, gt, invisible, valid, fit, eps=eps, workspace=ws)
    host = torch.cat([fit, sums.reshape(B, -1)], dim=1).cpu()          # the one read
    return samples_from_rows(host[:, :H.FIT_NCOL], host[:, H.FIT_NCOL:].reshape(B, 2, H.EVAL_NSUM))


class ValidationTracker:
    """The reference's eight MetricTrackers (discriminative_trainer.py:92-99) and its update rule (:595-613): a value goes to ``overall`` and to the
    sample's bucket unless it is NaN, metric by metric; the aligned values go to the ``align_`` twins."""

    def __init__(self, metrics: Iterable[str] = METRICS):
        self.metrics = tuple(metrics)
        self.trackers = {g: MetricTracker(*self.metrics) for g in GROUPS}

    def reset(self):
        for t in self.trackers.values():
            t.reset()

    def update(self, sample: SampleResult):
        for prefix, values in (("", sample.raw), ("align_", sample.aligned)):
            for name in self.metrics:
                v = values[name]
                if v != v:      # NaN: skipped for this metric only
                    continue
                self.trackers[prefix + "overall"].update(name, v)
                self.trackers[prefix + sample.bucket].update(name, v)

    def result(self) -> Dict[str, Dict[str, float]]:
        return {g: self.trackers[g].result() for g in GROUPS}

    def counts(self) -> Dict[str, Dict[str, int]]:
        return {g: {m: int(self.trackers[g]._counts[m]) for m in self.metrics} for g in GROUPS}

    # ranks combine one fixed-length fp64 vector: (total, count) of every (group, metric), in GROUPS x metrics order
    def state_vector(self) -> List[float]:
        return [x for g in GROUPS for m in self.metrics for x in (self.trackers[g]._total[m], float(self.trackers[g]._counts[m]))]

    def load_state_vector(self, vec):
        it = iter(float(v) for v in vec)
        for g in GROUPS:
            for m in self.metrics:
                self.trackers[g]._total[m] = next(it)
                self.trackers[g]._counts[m] = int(round(next(it)))


def validate_single_dataset(model: Callable, data_loader, device, metrics: Iterable[str] = METRICS, eps: float = 1e-5,
                            evaluate: Optional[Callable] = None) -> Dict[str, Dict[str, float]]:
    """Drop-in for the reference trainer's method: consumes its batch keys (``rgb_int, guide, guide_rgb_norm, depth_observation, depth_gt,
    valid_mask_raw, visible_mask, invisible_mask``; any batch size), feeds the model the image / 255 and both guides mapped to [-1, 1], and returns
    the reference's dict of eight groups.  ``evaluate`` replaces evaluate_batch (tests without a device)."""
    evaluate = evaluate or evaluate_batch
    tracker = ValidationTracker(metrics)
    if hasattr(model, "eval"):
        model.eval()
    with torch.no_grad():
        for batch in data_loader:
            rgb = batch["rgb_int"].to(device) / 255.0
            pred = model(rgb, guide_rgb=batch["guide_rgb_norm"].float().to(device), guide_mask=batch["guide"].float().to(device) * 2 - 1,
                         observation=batch["depth_observation"].float().to(device) * 2 - 1)
            on = lambda k: _maps(batch[k], k).to(device)      # noqa: E731
            for s in evaluate(_maps(pred, "pred"), on("depth_gt"), on("depth_observation"), on("guide"), on("visible_mask"), on("invisible_mask"),
                              on("valid_mask_raw"), eps):
                tracker.update(s)
    return tracker.result()
