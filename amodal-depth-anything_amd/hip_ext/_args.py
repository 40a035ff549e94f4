"""The tensor-argument checks of the wrappers in hip_ext/__init__.py: what a kernel is handed is on a HIP device, of the stated dtype, shape and
packing, and on one device.  Every check raises HipExtError before anything is launched; none of them copies or computes."""
from __future__ import annotations

from typing import Optional

import torch

from ._abi import HipExtError


def _dev(t: torch.Tensor, name: str, dtype=None) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipExtError(f"{name}: expected a tensor on a HIP device (the HIP path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise HipExtError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t.data_ptr()


def _opt(t: Optional[torch.Tensor], name: str, dtype=None):
    return None if t is None else _dev(t, name, dtype)


def _u8(t):
    """The bool -> uint8 rule: a bool tensor holds one byte per element, 0 / 1, so it is viewed, never copied.  The view keeps the strides: a caller
    whose kernel reads packed bytes checks contiguity (or packs) itself, before or after."""
    return t.view(torch.uint8) if isinstance(t, torch.Tensor) and t.dtype == torch.bool else t


def _same_device(who, ref_name, ref, **tensors):
    """Every tensor given (None skipped) is on ``ref``'s device.  Called by every wrapper that takes more than one tensor except the launches that
    hip_ext.engine issues per layer or per forward from buffers it allocated on one device itself, where the model's latency is the host's launch
    rate: igemm, attention, layernorm, patchify, pos_embed_resize, write_cls, bilinear, dpt_tail, tapsum_resize, depth_stats, token_diversity,
    ladder_select, count_saturated."""
    for name, t in tensors.items():
        if t is not None and t.device != ref.device:
            raise HipExtError(f"{who}: {name} on {t.device}, {ref_name} on {ref.device}")


def _sized(who, name, t, shape, dtype):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise HipExtError(f"{who}: {name} must be a contiguous {tuple(shape)} tensor, got {tuple(getattr(t, 'shape', ()))}")
    return _dev(t, name, dtype)


def _like(who, name, t, ref, dtype, optional=False):
    """Device pointer of ``t``, which has ``ref``'s shape and device (None for an absent optional one)."""
    if t is None and optional:
        return None
    p = _sized(who, name, t, tuple(ref.shape), dtype)
    _same_device(who, "expected", ref, **{name: t})
    return p


def _maps3(who, first, name="image", dtype=torch.float32):
    """Shape of a non-empty contiguous [B, h, w] device tensor of ``dtype``."""
    if not isinstance(first, torch.Tensor) or first.dim() != 3 or not first.is_contiguous() or first.numel() == 0:
        raise HipExtError(f"{who}: {name} must be a non-empty contiguous [B, h, w] tensor, got {tuple(getattr(first, 'shape', ()))}")
    _dev(first, name, dtype)
    return tuple(first.shape)


def _bytes_of(who, workspace, need, device):
    """(workspace, its size in bytes): any contiguous tensor on ``device``, allocated with ``need`` bytes when None.  The kernels see bytes and
    check the size themselves, so the dtype it is allocated in means nothing."""
    if workspace is None:
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or not workspace.is_contiguous() or workspace.device != device:
        raise HipExtError(f"{who}: workspace must be a contiguous tensor on {device}")
    return workspace, workspace.numel() * workspace.element_size()


def _check_src_extent(who, src, need):
    """``src`` (uint8, possibly a strided view) must have ``need`` bytes from its first element to the end of its storage: the kernels read
    (hi - 1) * row_pitch + a row's bytes (per image) from that pointer, whatever the view's own shape says."""
    if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8:
        return      # _dev reports it
    have = src.untyped_storage().nbytes() - src.storage_offset()
    if min(need, have) < 0 or have < need:
        raise HipExtError(f"{who}: src holds {have} bytes from its first pixel, the given sizes and pitches read {need}")
