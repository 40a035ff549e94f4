"""Depth metrics of the reference's evaluation (``src/util/metric.py:37-160``) on the device.

Same function names, arguments and reductions as the reference -- per-image masked mean, then the mean over the batch
(``log10``: mean over every valid pixel of the batch; ``silog_rmse``: sqrt of the batch mean, times 100) -- but every
function reads its per-image sums from ONE pass of ``ada_depth_eval_fwd`` over the maps instead of building a full-size
temporary per metric on the host.  ``depth_metrics`` returns all of them from a single pass.  Inputs are ``[B, H, W]``
(or ``[B, 1, H, W]``) tensors on a HIP device; there is no CPU fallback.

The edge metrics (``extract_edges``, ``EdgeAcc`` / ``EdgeComp`` / ``soft_edge_error``, metric.py:181-328) sit on skimage's Canny detector and
scipy's Euclidean distance transform in the reference, on the host and twice per sample; here they run on the device (``hip_ext.edges``,
csrc/ada_edges.hip), following the host's float32 stage storage so that the edge maps are the reference's wherever no decision of the detector sits
within rounding distance of flipping ("Edge metrics").  ``edge_metrics`` returns EdgeAcc and EdgeComp from ONE detector run per map.

Deliberate difference: when the ground truth has no edge pixel the device distance transform is ``+inf`` everywhere, so no predicted edge counts as
close (``n_bde == 0``) and both metrics take their fallback threshold.  scipy's distance map for an input without any background pixel is an
artefact of its implementation, not a documented value, and is not reproduced.
"""
from typing import Dict, Optional

import torch

import hip_ext as H

__all__ = ["MetricTracker", "depth_metrics", "abs_relative_difference", "squared_relative_difference", "rmse_linear", "rmse_log",
           "log10", "threshold_percentage", "delta1_acc", "delta2_acc", "delta3_acc", "i_rmse", "silog_rmse",
           "eps", "to_log", "to_inv", "extract_edges", "edge_metrics", "EdgeAcc", "EdgeComp", "soft_edge_error"]


class MetricTracker:
    """Running averages per key (metric.py:13-34; same ``update`` / ``avg`` / ``result`` / ``reset`` behaviour, no pandas)."""

    def __init__(self, *keys, writer=None):
        self.writer = writer
        self._keys = list(keys)
        self.reset()

    def reset(self):
        self._total = {k: 0.0 for k in self._keys}
        self._counts = {k: 0 for k in self._keys}

    def update(self, key, value, n=1):
        if self.writer is not None:
            self.writer.add_scalar(key, value)
        if key not in self._total:
            raise KeyError(key)
        self._total[key] += float(value) * n
        self._counts[key] += n

    def avg(self, key):
        return self._total[key] / self._counts[key] if self._counts[key] else 0.0

    def result(self) -> Dict[str, float]:
        return {k: self.avg(k) for k in self._keys}


def _sums(output: torch.Tensor, target: torch.Tensor, valid_mask: Optional[torch.Tensor]) -> torch.Tensor:
    if output.shape != target.shape:
        raise ValueError(f"prediction {tuple(output.shape)} and target {tuple(target.shape)} differ in shape")
    if output.dim() < 2:
        raise ValueError("depth maps need at least [H, W]")
    hw = output.shape[-2:]
    o = output.reshape(-1, *hw).contiguous().float()
    t = target.reshape(-1, *hw).contiguous().float()
    m = None
    if valid_mask is not None:
        m = valid_mask.expand_as(output).reshape(-1, *hw).contiguous()
        if m.dtype not in (torch.bool, torch.uint8):
            m = m != 0
    return H.depth_eval(o, t, m)


def _per_image(sums: torch.Tensor, idx: int) -> torch.Tensor:
    return sums[:, idx] / sums[:, H.EVAL_N]


def _from_sums(s: torch.Tensor) -> Dict[str, torch.Tensor]:
    n = s[:, H.EVAL_N]
    first = s[:, H.EVAL_LOG_SQ] / n
    second = (s[:, H.EVAL_LOG] ** 2) / (n * n)
    return {
        "abs_relative_difference": _per_image(s, H.EVAL_ABS_REL).mean(),
        "squared_relative_difference": _per_image(s, H.EVAL_SQ_REL).mean(),
        "rmse_linear": torch.sqrt(_per_image(s, H.EVAL_SQ)).mean(),
        "rmse_log": torch.sqrt(first).mean(),
        "log10": s[:, H.EVAL_LOG10_ABS].sum() / n.sum(),
        "delta1_acc": _per_image(s, H.EVAL_D1).mean(),
        "delta2_acc": _per_image(s, H.EVAL_D2).mean(),
        "delta3_acc": _per_image(s, H.EVAL_D3).mean(),
        "i_rmse": torch.sqrt(_per_image(s, H.EVAL_INV_SQ)).mean(),
        # a variance: where every valid pixel has the same log difference the two fp64 terms differ by their last bits, of either sign (NaN stays NaN)
        "silog_rmse": torch.sqrt(torch.mean(torch.clamp(first - second, min=0.0))) * 100,
    }


def depth_metrics(output, target, valid_mask=None) -> Dict[str, torch.Tensor]:
    """Every metric of this module from one pass over the maps (0-dim fp64 tensors on the device)."""
    return _from_sums(_sums(output, target, valid_mask))


def abs_relative_difference(output, target, valid_mask=None):   # metric.py:37-48
    return _per_image(_sums(output, target, valid_mask), H.EVAL_ABS_REL).mean()


def squared_relative_difference(output, target, valid_mask=None):   # metric.py:51-64
    return _per_image(_sums(output, target, valid_mask), H.EVAL_SQ_REL).mean()


def rmse_linear(output, target, valid_mask=None):   # metric.py:67-79
    return torch.sqrt(_per_image(_sums(output, target, valid_mask), H.EVAL_SQ)).mean()


def rmse_log(output, target, valid_mask=None):   # metric.py:82-92
    return torch.sqrt(_per_image(_sums(output, target, valid_mask), H.EVAL_LOG_SQ)).mean()


def log10(output, target, valid_mask=None):   # metric.py:95-102
    s = _sums(output, target, valid_mask)
    return s[:, H.EVAL_LOG10_ABS].sum() / s[:, H.EVAL_N].sum()


def threshold_percentage(output, target, threshold_val, valid_mask=None):   # metric.py:106-120
    idx = {1.25: H.EVAL_D1, 1.25 ** 2: H.EVAL_D2, 1.25 ** 3: H.EVAL_D3}.get(threshold_val)
    if idx is None:
        raise ValueError("threshold_percentage: the device pass counts the thresholds 1.25, 1.25**2 and 1.25**3")
    return _per_image(_sums(output, target, valid_mask), idx).mean()


def delta1_acc(pred, gt, valid_mask):   # metric.py:123-124
    return threshold_percentage(pred, gt, 1.25, valid_mask)


def delta2_acc(pred, gt, valid_mask):   # metric.py:127-128
    return threshold_percentage(pred, gt, 1.25 ** 2, valid_mask)


def delta3_acc(pred, gt, valid_mask):   # metric.py:131-132
    return threshold_percentage(pred, gt, 1.25 ** 3, valid_mask)


def i_rmse(output, target, valid_mask=None):   # metric.py:135-147
    return torch.sqrt(_per_image(_sums(output, target, valid_mask), H.EVAL_INV_SQ)).mean()


def silog_rmse(depth_pred, depth_gt, valid_mask=None):   # metric.py:150-163
    return _from_sums(_sums(depth_pred, depth_gt, valid_mask))["silog_rmse"]


# ---- edge metrics (metric.py:164-328) -------------------------------------------------------------------------------------------------------

def eps(x):   # same contract as metric.py:164-167
    """Machine epsilon of ``x``'s dtype; of float32 when ``x`` is None."""
    return torch.finfo(torch.float32 if x is None else x.dtype).eps


def _positive_floor(depth):
    """(tensor, tensor clamped from below at its dtype's epsilon, positive mask) -- what to_log and to_inv share."""
    d = torch.as_tensor(depth)
    return d, torch.clamp(d, min=eps(d)), d > 0


def to_log(depth):   # same contract as metric.py:169-173
    """Linear depth to log depth: log(max(depth, eps)) times the 0 / 1 mask of positive depth (torch ops on ``depth``'s device)."""
    _, floored, positive = _positive_floor(depth)
    return torch.log(floored) * positive


def to_inv(depth):   # same contract as metric.py:175-179
    """Linear depth to disparity: the 0 / 1 mask of positive depth over max(depth, eps) (torch ops on ``depth``'s device)."""
    _, floored, positive = _positive_floor(depth)
    return positive / floored


def _maps(x, name):
    """``x`` squeezed to [H, W] or [B, H, W], and whether it was a single map."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor on a HIP device, got {type(x).__name__}")
    x = x.squeeze()
    if x.dim() not in (2, 3):
        raise ValueError(f"{name}: expected something that squeezes to [H, W] or [B, H, W], got {tuple(x.shape)}")
    return (x[None], True) if x.dim() == 2 else (x, False)


def _valid(valid_mask, like, single):
    v = valid_mask.squeeze()
    v = v[None] if single and v.dim() == 2 else v
    if v.shape != like.shape:
        raise ValueError(f"valid_mask {tuple(valid_mask.shape)} does not match the maps {tuple(like.shape)}")
    return (v if v.dtype in (torch.bool, torch.uint8) else v != 0).contiguous()


def extract_edges(depth, preprocess=None, sigma=1, mask=None, use_canny=True):   # metric.py:181-219
    """Canny edges of a depth map as the reference detects them: bool [H, W] (or [B, H, W] for a batch) on the device.  ``preprocess``: 'log' is to_log;
    'none' / None is the reference's default branch, log(depth) / log(1.5); 'inv' is to_inv shifted and scaled to [0, 1] per image.  A ``mask`` is not
    supported (no call site of the reference passes one), nor is ``use_canny=False`` (the reference raises there too)."""
    if preprocess not in {'log', 'inv', 'none', None}:
        raise ValueError(f"extract_edges: preprocess must be 'log', 'inv', 'none' or None, got {preprocess!r}")
    if mask is not None:
        raise NotImplementedError("extract_edges: a mask of valid pixels is not supported on the device")
    if not use_canny:
        raise NotImplementedError("extract_edges: only the Canny detector exists (use_canny=False is not implemented in the reference either)")
    from hip_ext import edges as E
    d, single = _maps(depth, "extract_edges")
    d = d.float()
    if preprocess == 'inv':
        d = to_inv(d)
        d = d - d.amin(dim=(1, 2), keepdim=True)
        d = d / d.amax(dim=(1, 2), keepdim=True)
        pre = None
    else:
        pre = 'log' if preprocess == 'log' else 'log1.5'
    e = E.canny(d.contiguous(), sigma=sigma, pre=pre).view(torch.bool)
    return e[0] if single else e


def _edge_sums(pred, gt, valid_mask, th_edges_acc):
    from hip_ext import edges as E
    p, single = _maps(pred, "pred")
    g, _ = _maps(gt, "gt")
    if p.shape != g.shape:
        raise ValueError(f"prediction {tuple(p.shape)} and target {tuple(g.shape)} differ in shape")
    v = _valid(valid_mask, p, single)
    pe = E.canny(p.float().contiguous(), pre='log')
    ge = E.canny(g.float().contiguous(), pre='log')
    # both distance maps are taken BEFORE the invalid pixels are cleared from the edge maps (metric.py:242-248)
    return E.edge_sums(pe, ge, v, E.distance_transform_edt(ge), E.distance_transform_edt(pe), th_edges_acc)


def edge_metrics(pred, gt, valid_mask, th_edges_acc=10, th_edges_comp=10) -> Dict[str, torch.Tensor]:
    """EdgeAcc and EdgeComp per image (fp64 [B] on the device) from one detector run per map.  The reference's quirks are kept: both metrics test
    ``D_target < th_edges_acc``; EdgeComp averages ``D_pred`` over every valid ground-truth edge pixel; both fall back to their threshold when no
    predicted edge is close (``n_bde == 0``); close predicted edges without any valid ground-truth edge give 0 / 0 = NaN, as numpy's empty mean does."""
    return _edge_from_sums(_edge_sums(pred, gt, valid_mask, th_edges_acc), th_edges_acc, th_edges_comp)


def _edge_from_sums(s: torch.Tensor, th_edges_acc=10, th_edges_comp=10) -> Dict[str, torch.Tensor]:
    """metric.py:253-256 from the rows of ada_edge_metric_fwd."""
    some = s[:, H.EDGE_N_BDE] > 0
    acc = torch.where(some, s[:, H.EDGE_SUM_DT] / s[:, H.EDGE_N_BDE], torch.full_like(s[:, 0], float(th_edges_acc)))
    comp = torch.where(some, s[:, H.EDGE_SUM_DP] / s[:, H.EDGE_N_GT], torch.full_like(s[:, 0], float(th_edges_comp)))
    return {"EdgeAcc": acc, "EdgeComp": comp}


def _one(t):
    if t.numel() != 1:
        raise ValueError(f"the per-sample edge metrics take one map, got a batch of {t.numel()}; use edge_metrics")
    return t[0]


def EdgeAcc(pred, gt, valid_mask, th_edges_acc=10, th_edges_comp=10):   # metric.py:221-259
    return _one(edge_metrics(pred, gt, valid_mask, th_edges_acc, th_edges_comp)["EdgeAcc"])


def EdgeComp(pred, gt, valid_mask, th_edges_acc=10, th_edges_comp=10):   # metric.py:261-300
    return _one(edge_metrics(pred, gt, valid_mask, th_edges_acc, th_edges_comp)["EdgeComp"])


def soft_edge_error(pred, gt, valid_mask, radius=1):   # metric.py:317-328
    """Mean over the valid pixels of min over the (2 radius + 1)^2 shifts of |shift(gt) - pred| (0-dim fp64; NaN without a valid pixel)."""
    from hip_ext import edges as E
    p, single = _maps(pred, "pred")
    g, _ = _maps(gt, "gt")
    if p.shape != g.shape:
        raise ValueError(f"prediction {tuple(p.shape)} and target {tuple(g.shape)} differ in shape")
    s = E.soft_edge_sums(p.float().contiguous(), g.float().contiguous(), _valid(valid_mask, p, single), radius)
    return _one(s[:, 1] / s[:, 0])
