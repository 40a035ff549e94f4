"""The depth normalizers every dataset of the reference's evaluation is built with (``src/util/depth_transform.py``), on the device.

``ScaleShiftDepthNormalizer`` takes the 2 % / 98 % quantiles of the valid, positive depths with ``torch.quantile`` and maps them linearly onto
[norm_min, norm_max].  Here that is a composition of two device calls with no host read between them: the exact quantiles
(``hip_ext.quantile.quantiles(method="torch", positive_only=True)``, ada_quantile_fwd) and the scale-and-shift (ada_range_map_fwd), so the call sequence is
fixed by the shape and can be captured.  The quantiles equal ``torch.quantile`` on a CPU with FMA bit for bit (include/ada_hip.h, ADA_Q_TORCH), the map equals the torch expression evaluated
in fp32 on the CPU.  The surface is the reference's; ``per_image=True`` is the one addition.
"""
import logging

import torch

import hip_ext as H
from hip_ext.quantile import quantiles

__all__ = ["get_depth_normalizer", "DepthNormalizerBase", "ScaleShiftDepthNormalizer", "SAMNormalizer"]


def get_depth_normalizer(cfg_normalizer):
    """``cfg_normalizer``: any object with the reference's attributes (``type``, and for "scale_shift_depth" ``norm_min``, ``norm_max``,
    ``min_max_quantile``, ``clip``); None gives the identity."""
    if cfg_normalizer is None:
        return _identity
    kind = cfg_normalizer.type
    if kind == "scale_shift_depth":
        c = cfg_normalizer
        return ScaleShiftDepthNormalizer(norm_min=c.norm_min, norm_max=c.norm_max, min_max_quantile=c.min_max_quantile, clip=c.clip)
    if kind == "sam_depth":
        return SAMNormalizer()
    raise NotImplementedError(f"get_depth_normalizer: unknown normalizer type {kind!r} ('scale_shift_depth', 'sam_depth')")


def _identity(x):
    return x


class DepthNormalizerBase:
    """What every normalizer answers: ``is_absolute`` (metric depth or relative), ``far_plane_at_max`` (does far map to ``norm_max``), calling it on a
    depth tensor, and ``denormalize`` for the way back.  Abstract: it cannot be constructed or called."""

    is_absolute = None
    far_plane_at_max = None

    def __init__(self, norm_min=-1.0, norm_max=1.0):
        raise NotImplementedError(f"{type(self).__name__} is abstract: use get_depth_normalizer")

    def __call__(self, depth, valid_mask=None, clip=None):
        raise NotImplementedError(f"{type(self).__name__} does not normalise")

    def denormalize(self, depth_norm, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} does not denormalise")


class ScaleShiftDepthNormalizer(DepthNormalizerBase):
    """d' = (d - near) / (far - near) * (norm_max - norm_min) + norm_min, near / far = the ``min_max_quantile`` and 1 - ``min_max_quantile`` quantiles of
    the depths that are valid and > 0.  Relative depth, far at ``norm_max``."""

    is_absolute = False
    far_plane_at_max = True

    def __init__(self, norm_min=-1.0, norm_max=1.0, min_max_quantile=0.02, clip=True):
        self.norm_min, self.norm_max = norm_min, norm_max
        self.norm_range = norm_max - norm_min
        self.min_quantile, self.max_quantile = min_max_quantile, 1.0 - min_max_quantile      # 1.0 - q in double, rounded to fp32 only at the call
        self.clip = clip

    def quantile_range(self, depth_linear, valid_mask=None, per_image=False):
        """(near, far) as torch.quantile gives them: fp32 [B, 2] on the device, B = 1 unless ``per_image`` (then dim 0 of ``depth_linear``)."""
        if not isinstance(depth_linear, torch.Tensor) or depth_linear.dtype != torch.float32 or not depth_linear.is_cuda or depth_linear.numel() == 0:
            raise H.HipExtError(f"ScaleShiftDepthNormalizer: depth must be a non-empty fp32 tensor on a HIP device (the HIP path has no CPU fallback), got "
                                f"{getattr(depth_linear, 'dtype', type(depth_linear).__name__)} on {getattr(depth_linear, 'device', None)}")
        x = depth_linear.contiguous()
        x = x if per_image else x.reshape(1, -1)
        if valid_mask is not None:
            valid_mask = valid_mask.contiguous().reshape(x.shape)
        # the reference hands torch.quantile an fp32 tensor of the two fractions: they are rounded before the rank is computed
        qs = [float(torch.tensor(q, dtype=torch.float32)) for q in (self.min_quantile, self.max_quantile)]
        return quantiles(x, qs, valid=valid_mask, positive_only=True, method="torch").values.float()

    def __call__(self, depth_linear, valid_mask=None, clip=None, per_image=False):
        """The reference's meaning: the whole tensor is one population.  ``per_image=True`` treats dim 0 as a batch of independent maps.  ``clip`` None
        takes the constructor's."""
        do_clip = self.clip if clip is None else clip
        rng = self.quantile_range(depth_linear, valid_mask, per_image)
        x = depth_linear.contiguous()
        out = torch.empty_like(x)
        view = (lambda t: t) if per_image else (lambda t: t.view(1, -1))
        with torch.cuda.device(x.device):
            H.range_map(view(x), rng, view(out), scale=self.norm_range, shift=self.norm_min, clip=(self.norm_min, self.norm_max) if do_clip else None)
        return out

    def scale_back(self, depth_norm):
        """[norm_min, norm_max] -> [0, 1]; any tensor, any device (plain torch arithmetic)."""
        return (depth_norm - self.norm_min) / self.norm_range

    def denormalize(self, depth_norm, **kwargs):
        """Near and far were taken from the sample and are not kept: only the way back to [0, 1] exists (a warning says so)."""
        logging.warning("%s.denormalize: the sample's near / far planes are not stored, returning scale_back()", type(self).__name__)
        return self.scale_back(depth_norm)


class SAMNormalizer(DepthNormalizerBase):
    """The pseudo labels on SAM lie in [0, 1] already: the identity, both ways."""

    def __init__(self):
        self.norm_min, self.norm_max = 0.0, 1.0

    def __call__(self, depth_linear, valid_mask=None, clip=None):
        return depth_linear

    def denormalize(self, depth_norm, **kwargs):
        return depth_norm
