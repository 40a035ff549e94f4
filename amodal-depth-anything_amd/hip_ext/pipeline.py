"""The two-model amodal-depth pipeline of infer.py kept on the device.

    base = raw Depth-Anything-V2(normalised rgb)            reference infer.py:16-20
    norm = (base - min) / (max - min)   per image           infer.py:22          ada_minmax_fwd + ada_normalize_fwd
    pred = AmodalDAv2(rgb, mask*2-1, norm*2-1)              infer.py:88-93
    out  = paste pred inside the mask, 3x3 box blur on the mask border      infer.py:30-44   ada_blend_fwd

The reference moves `base` to the host, normalises it in numpy, sends it back, and blends on the host again; here the
maps never leave HBM and the only host traffic is the final result.

amodal_infer_image is the whole call, photo and masks in: the preparation of infer.py:17-18, 83-91 on the device (hip_ext.image), the base
network ONCE per photo, the amodal network as one batch over the K masks, optionally the demo's least-squares alignment over each
object's visible part (reference app.py:214-216, 249-265), the blend, and optionally the nearest resize back to the photo's size.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import (EVAL_N, EVAL_SUM_G, EVAL_SUM_P, EVAL_SUM_PG, EVAL_SUM_PP, HipExtError, blend, blend_ex, depth_eval, minmax,
               normalize)


@torch.no_grad()
def amodal_depth_pipeline(model_raw, amodal_model, rgb: torch.Tensor, mask01: torch.Tensor, rgb_raw: torch.Tensor = None):
    """rgb: [B,3,H,W] fp32 in [0,1] on the HIP device, the image fed to the amodal network; rgb_raw: the image fed to the
    base-depth network (the reference resizes that one bilinearly and the other with nearest: infer.py:17,84) -- defaults
    to rgb.  mask01: [B,1,H,W] fp32 0/1.  Returns (base_norm [B,H,W], amodal_pred [B,H,W], blended [B,H,W]) on the device."""
    if not rgb.is_cuda:
        raise HipExtError("amodal_depth_pipeline: inputs must live on a HIP device")
    B, _, H, W = rgb.shape
    src = rgb if rgb_raw is None else rgb_raw
    # the caller-side ImageNet normalisation of infer.py:19 runs inside the raw model's patchify kernel (normalise_input): no extra pass
    base = model_raw(src.contiguous(), normalise_input=True).contiguous()     # [B,H,W] >= 0
    mm = torch.empty(B, 2, dtype=torch.float32, device=rgb.device)
    minmax(base, mm)
    base_norm = torch.empty_like(base)
    obs = torch.empty(B, 1, H, W, dtype=torch.float32, device=rgb.device)
    normalize(base, mm, norm=base_norm, obs=obs)
    mask01 = mask01.float().contiguous()
    pred = amodal_model(rgb, guide_rgb=None, guide_mask=mask01 * 2 - 1, observation=obs).reshape(B, H, W).contiguous()
    out = torch.empty_like(base_norm)
    blend(pred, base_norm, mask01.reshape(B, H, W).contiguous(), out)
    return base_norm, pred, out


AmodalResult = namedtuple("AmodalResult", "base amodal blended masks scale_shift")
AmodalResult.__doc__ = """fp32 device tensors of amodal_infer_image: base [S, S] (min-max normalised base depth), amodal [K, S, S] (the network's
prediction, before any alignment), blended [K, S, S], masks [K, S, S] (0 / 1 at the network size), scale_shift [K, 2] or None.  With out_size,
base and blended are [h, w] / [K, h, w]."""


AmodalRendered = namedtuple("AmodalRendered", AmodalResult._fields + ("raw_rendered", "amodal_rendered"))
AmodalRendered.__doc__ = """amodal_infer_image(render=True): the five fields of AmodalResult, then the pictures of reference infer.py:106-119 as uint8 device tensors
in B, G, R order at out_size (the network size when out_size is None): raw_rendered [h, w, 3] (the base depth, no mask) and amodal_rendered
[K, h, w, 3] (the blended depth with highlight_target's outline and overlay)."""


def fit_scale_shift(amodal: torch.Tensor, base: torch.Tensor, visible: torch.Tensor) -> torch.Tensor:
    """Least-squares (scale, shift) per image with amodal * scale + shift ~ base over visible > 0 (reference app.py:249-261,
    linear_regression_predict): fp32 [K, 2] on the device, no host read.  From the fp64 sums of ada_depth_eval_fwd:
    scale = (S_PG - S_P S_G / N) / (S_PP - S_P^2 / N), shift = (S_G - scale S_P) / N.  An image with no visible pixel or a zero
    denominator gets NaN (N = 0: 0 / 0; denominator 0: masked explicitly, the reference raises there)."""
    if amodal.shape != base.shape or amodal.shape != visible.shape or amodal.dim() != 3:
        raise HipExtError(f"fit_scale_shift: [K, H, W] tensors of one shape required, got {tuple(amodal.shape)} {tuple(base.shape)} {tuple(visible.shape)}")
    vis = (visible > 0).contiguous()
    s = depth_eval(amodal.contiguous(), base.contiguous(), mask=vis)
    n, sp, sg, spp, spg = s[:, EVAL_N], s[:, EVAL_SUM_P], s[:, EVAL_SUM_G], s[:, EVAL_SUM_PP], s[:, EVAL_SUM_PG]
    den = spp - sp * sp / n
    scale = (spg - sp * sg / n) / den
    scale = torch.where(den == 0, torch.full_like(scale, float("nan")), scale)
    shift = (sg - scale * sp) / n
    return torch.stack([scale, shift], dim=1).float().contiguous()


@torch.no_grad()
def amodal_infer_image(model_raw, amodal_model, image, masks, visible_masks=None, size: int = 518, out_size=None, check: bool = True,
                       render: bool = False, min_area=None, min_area_connectivity: int = 4, render_percentiles=None, close=None, *,
                       blend: str = "paste", seam_tol: float = 1e-9, seam_max_iter=None, upsample: str = "nearest", guided_radius: int = 8,
                       guided_eps: float = 1e-3):
    """The reference's infer.py call on the device: a decoded uint8 BGR(A) photo [h, w, 3 | 4] and K amodal masks (uint8 / bool [h, w] or
    [K, h, w]) in, an AmodalResult out.  The base network runs once (B = 1), the amodal network once as a batch of K.

    visible_masks (same layout as masks, K entries): fit the amodal prediction to the base depth over each object's visible part before the
    paste (fit_scale_shift; the reference's demo, app.py:214-216).  check=True reads scale_shift back once, at the very end, and raises
    ValueError("Denominator in slope calculation is zero.") for an empty visible mask or a zero / non-finite denominator (app.py:257-258);
    check=False leaves NaN in scale_shift (and in that image's paste) instead.
    out_size: None (size x size), (h, w) or "image" (the photo's size): base and blended go through cv2's INTER_NEAREST rule (infer.py:77, 113).
    An all-zero amodal mask is legal: its blended map equals base.
    render=True: an AmodalRendered -- the same five fields plus the two pictures of infer.py:106-119 (hip_ext.image.render_depth: Spectral_r, the
    outline and overlay of highlight_target on the amodal ones, B, G, R), rendered from the network-size maps straight to out_size.
    min_area: when given, the AMODAL masks are first cleaned as given, at their own resolution, by hip_ext.masks.remove_small_noise (the demo's
    filter, app.py:283-293: components of fewer than min_area pixels under min_area_connectivity go) -- specks of a segmenter's mask would otherwise be
    guidance for the network and receive pasted depth.  The visible masks are not touched.  None: nothing runs, the call is exactly the one without it.
    render_percentiles: (lo, hi) in [0, 100] -- with render=True each picture is coloured between these percentiles of its own map (colorize()'s range,
    hip_ext.quantile.percentile_range, taken on the device) instead of between 0 and 1.  None: the pictures are exactly the ones without it.
    close: when given, the AMODAL masks are closed by a close x close square (hip_ext.masks.closing, the MORPH_CLOSE of app.py:211), at their own
    resolution, after the min_area step -- a segmenter's pinholes and hairline gaps would otherwise be guidance for the network and keep the base depth
    in the paste.  None: nothing runs, the call is exactly the one without it.
    upsample: how base and blended reach out_size.  "nearest" (the default) is the rule above, bit for bit the call without the keyword.  "guided"
    takes ``base`` there with the photo as guide (hip_ext.guided.guided_upsample, radius guided_radius at the network size, guided_eps in [0, 1]^2
    units): its depth edges lie where the photo's edges lie and not on the staircase of the nearest rule.  out_size must then be "image" or the photo's
    own size, and the photo at least the network's size.  ``blended`` takes the guided base OUTSIDE the nearest-resized amodal mask and keeps the
    nearest-resized blended values INSIDE it: a hidden surface has no edges in the photo, so the photo must not guide it.  The pictures of render=True
    are not affected.  Without an out_size nothing is resized and the keyword changes nothing.
    blend: how the prediction enters ``blended``.  "paste" (the default) is the paste and border blur above, bit for bit the call without the keyword.
    "seamless" needs visible_masks and adds a spatially varying correction instead of a seam: per object, with pred' = pred * scale + shift, the
    difference base - pred' on the object's visible part (visible and inside the amodal mask) is extended harmonically under the occluder, over the amodal
    mask and no further (hip_ext.inpaint's membrane solve, fp64, stopped at seam_tol / seam_max_iter as fill_harmonic's tol / max_iter), and
    blended = pred' + correction inside the mask, base bit for bit on the visible part and outside the mask; there is no border blur.  A part of the mask
    that no visible pixel reaches keeps the plain paste.  scale_shift, check, render, out_size and upsample act on the new ``blended`` as before."""
    from ._staging import as_int
    from .image import _check_size, masks_to_tensor, photo_to_inputs, render_depth, resize_nearest
    size = _check_size(size, "amodal_infer_image")
    if not (out_size is None or (isinstance(out_size, str) and out_size == "image")
            or (isinstance(out_size, (tuple, list)) and len(out_size) == 2 and all((as_int(v) or 0) > 0 for v in out_size))):
        raise ValueError(f"amodal_infer_image: out_size must be None, 'image' or (h, w), got {out_size!r}")
    if upsample not in ("nearest", "guided"):
        raise ValueError(f"amodal_infer_image: upsample must be 'nearest' or 'guided', got {upsample!r}")
    if blend not in ("paste", "seamless"):
        raise ValueError(f"amodal_infer_image: blend must be 'paste' or 'seamless', got {blend!r}")
    if blend == "seamless":
        from .inpaint import _check_solver
        if visible_masks is None:
            raise ValueError("amodal_infer_image: blend='seamless' needs visible_masks: the correction is pinned to each object's visible part (pinning it "
                             "to the pixels outside the amodal mask would tie the object to its occluders)")
        seam_tol, seam_max_iter, _ = _check_solver("amodal_infer_image", seam_tol, seam_max_iter, None, "smooth")
    guided = upsample == "guided" and out_size is not None
    if guided:
        from .guided import _eps, _radius
        _radius("amodal_infer_image", guided_radius), _eps("amodal_infer_image", guided_eps, torch.empty(0, dtype=torch.uint8))
        photo = tuple(getattr(image, "shape", ()))[:2]
        if out_size != "image" and tuple(as_int(v) for v in out_size) != photo:
            raise ValueError(f"amodal_infer_image: upsample='guided' takes the photo as guide: out_size must be 'image' or the photo's size {photo}, got {out_size!r}")
        if len(photo) == 2 and min(photo) < size:
            raise ValueError(f"amodal_infer_image: upsample='guided' needs a photo at least as large as the network size {size}, got {photo}")
    device = next(amodal_model.parameters()).device
    rgb_raw, rgb, (h, w) = photo_to_inputs(image, size, device)
    if min_area is not None:
        from .masks import remove_small_noise
        masks = remove_small_noise(masks, min_area=min_area, connectivity=min_area_connectivity, device=device)
    if close is not None:
        from .masks import closing
        masks = closing(masks, size=close, device=device)
    mask01, guide = masks_to_tensor(masks, size, device, guide=True)
    K, S = mask01.shape[0], size
    visible = None
    if visible_masks is not None:
        visible = masks_to_tensor(visible_masks, size, device)
        if visible.shape[0] != K:
            raise ValueError(f"amodal_infer_image: {visible.shape[0]} visible masks for {K} amodal masks")
    with torch.cuda.device(device):
        # the caller-side ImageNet normalisation of infer.py:19 runs inside the raw model's patchify kernel, as in amodal_depth_pipeline
        base = model_raw(rgb_raw, normalise_input=True).contiguous()              # [1, S, S]: once per photo, whatever K
        mm = torch.empty(1, 2, dtype=torch.float32, device=device)
        minmax(base, mm)
        base_norm = torch.empty_like(base)
        obs = torch.empty(1, 1, S, S, dtype=torch.float32, device=device)
        normalize(base, mm, norm=base_norm, obs=obs)
        pred = amodal_model(rgb.expand(K, -1, -1, -1), guide_rgb=None, guide_mask=guide, observation=obs.expand(K, -1, -1, -1)).reshape(K, S, S).contiguous()
        base_k = base_norm.expand(K, -1, -1).contiguous()
        m = mask01.reshape(K, S, S)
        scale_shift = fit_scale_shift(pred, base_k, visible.reshape(K, S, S)) if visible is not None else None
        if blend == "seamless":
            from .inpaint import _membrane
            aligned = pred * scale_shift[:, 0, None, None] + scale_shift[:, 1, None, None]      # fp32, product and sum rounded on their own, as ada_blend_ex
            inside = m > 0
            known = (visible.reshape(K, S, S) > 0) & inside
            every = None if torch.cuda.is_current_stream_capturing() else 64      # outside a capture: stop issuing steps once every object is done
            blended = _membrane("amodal_infer_image", base_k[:, None], known, inside, aligned[:, None].contiguous(), 0.0, seam_tol, seam_max_iter, every,
                                "smooth")[0][:, 0].contiguous()
        else:
            blended = torch.empty_like(pred)
            blend_ex(pred, base_k, m, blended, scale_shift)
        base_out = base_norm
        target = None if out_size is None else ((h, w) if out_size == "image" else tuple(out_size))
        if render and render_percentiles is not None:
            from .quantile import percentile_range
            lo_p, hi_p = render_percentiles
            raw_rendered = render_depth(base_norm, out_size=target, minmax=percentile_range(base_norm, lo_p, hi_p, invalid_val=None)[1])
            amodal_rendered = render_depth(blended, m, out_size=target, minmax=percentile_range(blended, lo_p, hi_p, invalid_val=None)[1])
        elif render:
            raw_rendered = render_depth(base_norm, out_size=target)
            amodal_rendered = render_depth(blended, m, out_size=target)
        if guided:
            from .guided import guided_upsample
            base_out = guided_upsample(base_norm, image[None, ..., :3], guided_radius, guided_eps, device=device)
            inside = resize_nearest(m.contiguous(), *target) > 0
            blended = torch.where(inside, resize_nearest(blended, *target), base_out)
        elif target is not None:
            base_out, blended = resize_nearest(base_norm, *target), resize_nearest(blended, *target)
    if check and scale_shift is not None and not bool(torch.isfinite(scale_shift.cpu()).all()):
        raise ValueError("Denominator in slope calculation is zero.")
    if render:
        return AmodalRendered(base_out[0], pred, blended, m, scale_shift, raw_rendered[0], amodal_rendered)
    return AmodalResult(base_out[0], pred, blended, m, scale_shift)
