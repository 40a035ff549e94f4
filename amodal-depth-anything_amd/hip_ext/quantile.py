"""Exact per-image quantiles of depth maps on the device: what the reference takes with ``np.percentile`` (colorize(), src/scripts/colorize_depth.py:55-56)
and ``torch.quantile`` (ScaleShiftDepthNormalizer, src/util/depth_transform.py:81-84), without a sort and without a host read.

One kernel sequence (ada_quantile_fwd, an 8-bit radix select on the floats' order-preserving keys) serves both: ``method="numpy"`` reproduces
``np.percentile(x.astype(float64)[population], 100 * q)`` ('linear'), ``method="torch"`` reproduces ``torch.quantile(x[population], float32(q))`` on a
CPU with FMA (ATen's lerp is an fmadd there; include/ada_hip.h), bit for bit.  The population is chosen on the device too, so a changed mask changes nothing about the launches: the calls are capturable.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import (Q_EXCLUDE_VALUE, Q_NUMPY, Q_POSITIVE_ONLY, Q_TORCH, QUANTILE_MAX_Q, HipExtError, quantile_select, quantile_workspace_bytes)
from ._args import _u8

_METHODS = {"numpy": Q_NUMPY, "torch": Q_TORCH}

Quantiles = namedtuple("Quantiles", "values count")
Quantiles.__doc__ = """Device tensors of quantiles(): values fp64 [B, Q] (NaN for an empty population or one that holds a NaN), count int64 [B] (the
population's size)."""


def _as_mask(mask, like, who, name):
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool) or mask.shape != like.shape or mask.device != like.device:
        raise HipExtError(f"{who}: {name} must be uint8 or bool {tuple(like.shape)} on {like.device}, got "
                          f"{getattr(mask, 'dtype', type(mask).__name__)} {tuple(getattr(mask, 'shape', ()))}")
    return _u8(mask.contiguous())


def _check_map(x, who, name="x"):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() < 1 or x.numel() == 0:
        raise HipExtError(f"{who}: {name} must be a non-empty fp32 [B, ...] tensor, got {getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    if not x.is_cuda:
        raise HipExtError(f"{who}: {name} on {x.device}, expected a HIP device (the HIP path has no CPU fallback)")
    return x.contiguous()


def _run(x, qs, valid, flags, exclude_value, mode, want_f32):
    """Every group of up to QUANTILE_MAX_Q quantiles is one call; returns (fp64 [B, Q], fp32 [B, Q] or None, int64 [B])."""
    B, dev = x.shape[0], x.device
    values = torch.empty(B, len(qs), dtype=torch.float64, device=dev)
    values32 = torch.empty(B, len(qs), dtype=torch.float32, device=dev) if want_f32 else None
    count = torch.empty(B, dtype=torch.int64, device=dev)
    ws = torch.empty(quantile_workspace_bytes(B) // 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for i in range(0, len(qs), QUANTILE_MAX_Q):
            part = qs[i:i + QUANTILE_MAX_Q]
            whole = len(part) == len(qs)
            out = values if whole else torch.empty(B, len(part), dtype=torch.float64, device=dev)
            out32 = values32 if whole or not want_f32 else torch.empty(B, len(part), dtype=torch.float32, device=dev)
            quantile_select(x, part, out, out_f32=out32, count=count, valid=valid, mode=mode, flags=flags, exclude_value=exclude_value, workspace=ws)
            if not whole:
                values[:, i:i + len(part)] = out
                if want_f32:
                    values32[:, i:i + len(part)] = out32
    return values, values32, count


def quantiles(x, q, valid=None, exclude_value=None, positive_only=False, method="numpy") -> Quantiles:
    """The quantiles ``q`` (fractions in [0, 1]; a number or a sequence) of every image of ``x`` (fp32 [B, ...] on a HIP device), each image over its own
    population: the elements where ``valid`` (uint8 / bool of x's shape) is non-zero, that differ from ``exclude_value`` (compared in double) and, with ``positive_only``, are
    > 0.  ``method``: "numpy" = np.percentile's 'linear' on the values as float64; "torch" = torch.quantile (CPU build with FMA) on fp32 with q rounded to fp32.
    Nothing is read back; there is no CPU fallback (HipExtError)."""
    who = "quantiles"
    if method not in _METHODS:
        raise ValueError(f"{who}: method must be 'numpy' or 'torch', got {method!r}")
    qs = [float(v) for v in (q if isinstance(q, (list, tuple)) else torch.as_tensor(q, dtype=torch.float64).reshape(-1).tolist())]
    if not qs or not all(0.0 <= v <= 1.0 for v in qs):
        raise ValueError(f"{who}: q must be one or more fractions in [0, 1], got {q!r}")
    x = _check_map(x, who)
    valid = None if valid is None else _as_mask(valid, x, who, "valid")
    flags = (Q_EXCLUDE_VALUE if exclude_value is not None else 0) | (Q_POSITIVE_ONLY if positive_only else 0)
    values, _, count = _run(x, qs, valid, flags, 0.0 if exclude_value is None else float(exclude_value), _METHODS[method], False)
    return Quantiles(values, count)


def percentile_range(depth, vminp=2, vmaxp=95, invalid_val=-99, invalid_mask=None):
    """The colour range of the reference's colorize(): (np.percentile(value[mask], vminp), np.percentile(value[mask], vmaxp)) per image of ``depth`` (fp32
    [B, ...] on a HIP device), mask = ~invalid_mask when given (uint8 / bool, non-zero = invalid), else value != invalid_val (compared in double, as colorize paints; None: every
    pixel counts).  Returns (fp64 [B, 2],
    fp32 [B, 2]) on the device; the second is the form render_depth(minmax=...) and hip_ext.normalize read.  Nothing is read back."""
    who = "percentile_range"
    ps = (float(vminp), float(vmaxp))
    if not all(0.0 <= p <= 100.0 for p in ps):
        raise ValueError(f"{who}: percentiles must lie in [0, 100], got {vminp!r}, {vmaxp!r}")
    depth = _check_map(depth, who, "depth")
    if invalid_mask is not None:
        valid, flags, excl = _as_mask(invalid_mask, depth, who, "invalid_mask") == 0, 0, 0.0
        valid = valid.view(torch.uint8)
    else:
        valid, flags, excl = None, (0 if invalid_val is None else Q_EXCLUDE_VALUE), (0.0 if invalid_val is None else float(invalid_val))
    values, values32, _ = _run(depth, [p / 100.0 for p in ps], valid, flags, excl, Q_NUMPY, True)
    return values, values32
