"""ADIW pseudo-labels on the device: the counterpart of the reference's ``src/scripts/sam_pl_gen_dav2.py`` below its file handling.

Per sample the reference runs the raw ViT-G on the un-occluded photo and on the occluded composite, min-max normalises both maps (lines 74, 88), fits
the first onto the second by least squares over the visible mask (101-106), pastes the fitted map inside the whole mask (115-116), quantises to 16 bits
(117) and saves a 512 x 512 PNG (121) -- one image at a time through host Pillow, numpy and a host lstsq.  Here a batch of P pairs is prepared, run as
ONE network batch of 2 P, fitted, combined and quantised without leaving HBM; only uint16 [P, 512, 512] comes back.

Everything the reference prepares goes through Pillow: ``Image.open(fp).convert('RGB').resize((518, 518))`` is Pillow's antialiased BICUBIC convolution on
8-bit pixels, and the masks take the same resize before ``> 0``.  A label is only reproducible if those bytes are, so ``pil_resize`` reproduces Pillow's
integer arithmetic bit for bit (ada_pil_resize_u8_fwd); the coefficient tables are computed here, on the host, in double, as Pillow computes them.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from . import (FIT_SCALE, FIT_SHIFT, LABEL_CLIP, LABEL_WRAP, PIL_BICUBIC, PIL_NEAREST, HipExtError, label_combine, minmax, normalize, pil_resize_u8,
               protocol_fit)
from ._args import _u8
from ._staging import DeviceCache, as_int, check_planar, resolve_device, stage_hwc, stage_planar

_PRECISION_BITS = 22      # Pillow's Resample.c: 32 - 8 - 2
_FILTERS = {"bicubic": PIL_BICUBIC, "nearest": PIL_NEAREST}
_OVERFLOW = {"wrap": LABEL_WRAP, "clip": LABEL_CLIP}


def pil_coeffs(n_in: int, n_out: int):
    """(bounds int32 [n_out, 2] = (xmin, n), kk int32 [n_out, ksize], ksize): the BICUBIC tables of Pillow's precompute_coeffs and
    normalize_coeffs_8bpc for one axis, every step in double in Pillow's order (include/ada_hip.h lists the rules)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"pil_coeffs: sizes must be positive, got {n_in} -> {n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # (int): truncation towards zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    a = -0.5
    w = np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1, np.where(t < 2.0, (((t - 5) * t + 8) * t - 4) * a, 0.0))
    w = np.where(x < n[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                        # accumulated in index order; the zeros past n add nothing
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    q = np.where(w < 0, -0.5 + w * (1 << _PRECISION_BITS), 0.5 + w * (1 << _PRECISION_BITS)).astype(np.int64)
    return np.stack([xmin, n], axis=1).astype(np.int32), np.ascontiguousarray(q.astype(np.int32)), ksize


_TABLES = DeviceCache(64)      # (n_in, n_out, device) -> (bounds, kk, ksize) on the device


def _device_tables(n_in, n_out, device):
    def make():
        bounds, kk, ksize = pil_coeffs(n_in, n_out)
        return torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize
    return _TABLES.get((n_in, n_out, device), make)


def _stage(img, device, who):
    """The checked pixels as (uint8 device tensor, K, h, w, channels, row pitch, image stride, kind) with kind in {"l", "rgb", "stack"}: numpy is
    copied, a device tensor is read in place at its own strides when its pixels are packed ([h, w], [h, w, 3] or [K, h, w])."""
    single = check_planar(who, img, (torch.uint8,), shapes="[h, w], [h, w, 3] or [K, h, w]")
    device = resolve_device(who, device, img)
    if img.ndim == 3 and img.shape[2] == 3:          # [h, w, 3]: a last axis of three is RGB, never a stack of masks three pixels wide
        src = stage_hwc(who, img, device)
        h, w, _ = src.shape
        return src, 1, h, w, 3, src.stride(0), h * src.stride(0), "rgb"
    src = stage_planar(who, img, device, "image", limits=False)
    K, h, w = src.shape
    return src, K, h, w, 1, src.stride(1), src.stride(0), "l" if single else "stack"


def _resize_into(staged, ho, wo, filt, device, out_u8=None, out_f32=None, out_mask=None):
    src, K, h, w, c, pitch, istride, _ = staged
    tx = ty = tmp = None
    if filt == PIL_BICUBIC:
        tx = _device_tables(w, wo, device) if w != wo else None
        ty = _device_tables(h, ho, device) if h != ho else None
        if tx is not None and ty is not None:
            tmp = torch.empty(K * h * wo * c, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        pil_resize_u8(src, K, h, w, c, pitch, istride, ho, wo, filt, tx, ty, tmp, out_u8=out_u8, out_f32=out_f32, out_mask=out_mask)


def _check_hw(size_hw, who):
    hw = tuple(as_int(v) for v in size_hw) if isinstance(size_hw, (tuple, list)) and len(size_hw) == 2 else (None, None)
    if None in hw or min(hw) < 1:
        raise ValueError(f"{who}: the target size must be two positive integers (h, w), got {size_hw!r}")
    return hw


def pil_resize(img, size_hw, resample: str = "bicubic", out: str = "u8", device=None):
    """Pillow's ``Image.resize((w, h), BICUBIC | NEAREST)`` of 8-bit pixels on the device, byte for byte.  ``img``: uint8 [h, w] (mode L), [h, w, 3] (RGB; a
    last axis of 3 always means RGB) or [K, h, w] (K mode-L images) -- a numpy array (copied to ``device``) or a device tensor, read in place at its own
    row stride (a crop costs no copy).  ``size_hw`` = (h, w).  Returns, on the device:
        out="u8"     Pillow's bytes: uint8 [h, w], [h, w, 3] or [K, h, w]
        out="float"  bytes / 255 as fp32: [h, w], planar [3, h, w] (R, G, B planes kept) or [K, h, w] -- np.array(im) / 255 cast to float32
        out="mask"   uint8 0 / 1 = bytes > 0, mode L only
    There is no CPU fallback: a non-HIP device raises HipExtError; TypeError / ValueError as hip_ext.image's staging."""
    who = "pil_resize"
    if resample not in _FILTERS:
        raise ValueError(f"{who}: resample must be 'bicubic' or 'nearest', got {resample!r}")
    if out not in ("u8", "float", "mask"):
        raise ValueError(f"{who}: out must be 'u8', 'float' or 'mask', got {out!r}")
    ho, wo = _check_hw(size_hw, who)
    staged = _stage(img, device, who)
    src, K, _, _, c, _, _, kind = staged
    if out == "mask" and c != 1:
        raise ValueError(f"{who}: out='mask' takes mode-L images ([h, w] or [K, h, w]), got an RGB image")
    dev = src.device
    if out == "u8":
        res = torch.empty((K, ho, wo, c), dtype=torch.uint8, device=dev)
        _resize_into(staged, ho, wo, _FILTERS[resample], dev, out_u8=res)
        res = res[0] if kind == "rgb" else res[..., 0]
    elif out == "float":
        res = torch.empty((K, c, ho, wo), dtype=torch.float32, device=dev)
        _resize_into(staged, ho, wo, _FILTERS[resample], dev, out_f32=res)
        res = res[0] if kind == "rgb" else res[:, 0]
    else:
        res = torch.empty((K, ho, wo), dtype=torch.uint8, device=dev)
        _resize_into(staged, ho, wo, _FILTERS[resample], dev, out_mask=res)
    return res[0] if kind == "l" else res


PseudoLabel = namedtuple("PseudoLabel", "label combined whole_norm occ_norm scale_shift out_of_range")
PseudoLabel.__doc__ = """Device tensors of label_from_depths: label uint16 [P, L, L] (the 16-bit map the reference saves), combined fp32 [P, S, S] (the
paste before quantising), whole_norm / occ_norm fp32 [P, S, S] (the min-max normalised maps), scale_shift fp32 [P, 2] (the fit of whole_norm onto
occ_norm over the visible mask), out_of_range int64 [P] (label pixels whose value * 65535 left [0, 65536) or was NaN)."""


def _norm(depth):
    mm = torch.empty(depth.shape[0], 2, dtype=torch.float32, device=depth.device)
    minmax(depth, mm)
    out = torch.empty_like(depth)
    normalize(depth, mm, norm=out)
    return out


@torch.no_grad()
def label_from_depths(whole_depth, occ_depth, visible_u8, whole_u8, label_size=512, overflow: str = "wrap") -> PseudoLabel:
    """The reference's lines 74, 88, 101-106, 115-117 and 121 on the device.  ``whole_depth`` / ``occ_depth``: fp32 [P, S, S], the raw network's outputs for
    the un-occluded photo and the occluded composite; ``visible_u8`` / ``whole_u8``: uint8 (or bool) [P, S, S], non-zero inside.  Steps: min-max
    normalise both (ada_minmax_fwd, ada_normalize_fwd); least-squares (scale, shift) of whole_norm onto occ_norm over the visible mask
    (ada_protocol_fit_fwd: numpy.linalg.lstsq's minimum-norm answers for an empty or constant support), rounded to fp32; paste whole_norm * scale +
    shift inside the whole mask, * 65535, cast, Pillow's NEAREST resize to ``label_size`` (ada_label_combine_fwd).  ``label_size=None`` keeps S.
    ``overflow``: "wrap" is the reference's cast (numpy's astype(np.uint16) on x86-64: values outside [0, 65536) wrap, NaN gives 0), "clip" clamps.
    Nothing is read back to the host."""
    who = "label_from_depths"
    if overflow not in _OVERFLOW:
        raise ValueError(f"{who}: overflow must be 'wrap' or 'clip', got {overflow!r}")
    for name, t in (("whole_depth", whole_depth), ("occ_depth", occ_depth)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != torch.float32 or not t.is_cuda:
            raise HipExtError(f"{who}: {name} must be fp32 [P, S, S] on a HIP device, got {getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
    if occ_depth.shape != whole_depth.shape or occ_depth.device != whole_depth.device:
        raise HipExtError(f"{who}: occ_depth {tuple(occ_depth.shape)} on {occ_depth.device} does not match whole_depth {tuple(whole_depth.shape)} on {whole_depth.device}")
    P, h, w = whole_depth.shape
    masks = []
    for name, m in (("visible_u8", visible_u8), ("whole_u8", whole_u8)):
        if not isinstance(m, torch.Tensor) or m.dtype not in (torch.uint8, torch.bool) or m.shape != whole_depth.shape or m.device != whole_depth.device:
            raise HipExtError(f"{who}: {name} must be uint8 {tuple(whole_depth.shape)} on {whole_depth.device}, got "
                              f"{getattr(m, 'dtype', type(m).__name__)} {tuple(getattr(m, 'shape', ()))}")
        masks.append(_u8(m.contiguous()))
    visible, whole_mask = masks
    if label_size is None:
        ho, wo = h, w
    else:
        ho = wo = as_int(label_size)
        if ho is None or ho < 1:
            raise ValueError(f"{who}: label_size must be None or a positive integer, got {label_size!r}")
    dev = whole_depth.device
    with torch.cuda.device(dev):
        whole_norm, occ_norm = _norm(whole_depth.contiguous()), _norm(occ_depth.contiguous())
        fit = protocol_fit(whole_norm, occ_norm, visible, whole_mask)
        scale_shift = fit[:, FIT_SCALE:FIT_SHIFT + 1].float().contiguous()
        label = torch.empty(P, ho, wo, dtype=torch.uint16, device=dev)
        combined = torch.empty_like(whole_norm)
        rows = torch.empty(P, ho, dtype=torch.int32, device=dev)
        label_combine(whole_norm, occ_norm, whole_mask, scale_shift, label, combined, rows, _OVERFLOW[overflow])
    return PseudoLabel(label, combined, whole_norm, occ_norm, scale_shift, rows.sum(dim=1))


def _per_item(mask_resample, P, who):
    """mask_resample as P pairs (visible, whole) of filter names: one name for all, or per item a name or a pair."""
    items = [mask_resample] * P if isinstance(mask_resample, str) else list(mask_resample)
    if len(items) != P:
        raise ValueError(f"{who}: mask_resample has {len(items)} entries for {P} pairs")
    pairs = [(m, m) if isinstance(m, str) else tuple(m) for m in items]
    for pair in pairs:
        if len(pair) != 2 or any(m not in _FILTERS for m in pair):
            raise ValueError(f"{who}: mask_resample entries must be 'bicubic' or 'nearest' (or a pair of them), got {pair!r}")
    return pairs


@torch.no_grad()
def pseudo_label_pairs(model_raw, whole_images, occ_images, visible_masks, whole_masks, size: int = 518, label_size=512, overflow: str = "wrap",
                       mask_resample="bicubic") -> PseudoLabel:
    """P occlusion pairs in, their ADIW pseudo-labels out.  ``whole_images`` / ``occ_images``: lists of P decoded RGB photos, uint8 [h, w, 3] (what
    ``Image.open(fp).convert('RGB')`` decodes; sizes may differ per item); ``visible_masks`` / ``whole_masks``: lists of P mode-L masks, uint8 [h, w].
    Each item is prepared with pil_resize to ``size`` x ``size`` (the reference's load_im and lines 93-98), ONE ``model_raw(x, normalise_input=True)``
    call runs on the [2 P, 3, size, size] batch (the un-occluded photos first), then label_from_depths.  ``mask_resample``: "bicubic" (Pillow's default
    for mode L) or "nearest" (what Pillow uses for masks whose file mode is 1 or P); one name, or per pair a name or a (visible, whole) pair."""
    from .image import _check_size
    who = "pseudo_label_pairs"
    size = _check_size(size, who)
    P = len(whole_images)
    if P < 1 or not (len(occ_images) == len(visible_masks) == len(whole_masks) == P):
        raise ValueError(f"{who}: {P} photos, {len(occ_images)} composites, {len(visible_masks)} visible and {len(whole_masks)} whole masks: one of each per pair")
    resample = _per_item(mask_resample, P, who)
    device = resolve_device(who, next(model_raw.parameters()).device)
    x = torch.empty(2 * P, 3, size, size, dtype=torch.float32, device=device)
    masks = torch.empty(2, P, size, size, dtype=torch.uint8, device=device)
    for i in range(P):
        for j, img in ((i, whole_images[i]), (P + i, occ_images[i])):
            staged = _stage(img, device, who)
            if staged[-1] != "rgb":
                raise ValueError(f"{who}: photos must be RGB [h, w, 3], got shape {tuple(img.shape)}")
            _resize_into(staged, size, size, PIL_BICUBIC, device, out_f32=x[j])
        for j, m in enumerate((visible_masks[i], whole_masks[i])):
            staged = _stage(m, device, who)
            if staged[-1] != "l":
                raise ValueError(f"{who}: masks must be mode L [h, w], got shape {tuple(m.shape)}")
            _resize_into(staged, size, size, _FILTERS[resample[i][j]], device, out_mask=masks[j, i])
    with torch.cuda.device(device):
        depth = model_raw(x, normalise_input=True).reshape(2 * P, size, size).contiguous()
    return label_from_depths(depth[:P], depth[P:], masks[0], masks[1], label_size=label_size, overflow=overflow)
