"""Host inputs of the domain modules (image, labels, masks, geometry, edges): which device a call targets, a numpy array or a tensor as a checked,
packed device tensor, and a small cache of device tables.  There is no CPU fallback: a CPU tensor or a non-HIP target raises HipExtError."""
from __future__ import annotations

import operator
from collections import OrderedDict

import numpy as np
import torch

from ._abi import HipExtError
from ._args import _u8


def as_int(v):
    """Any integer type (int, a numpy integer, a 0-d integer tensor) as a Python int; None for anything else, bool included."""
    if isinstance(v, bool):
        return None
    try:
        return operator.index(v)
    except TypeError:
        return None


def with_index(device) -> torch.device:
    """torch.device(device), a bare "cuda" naming the current device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def resolve_device(who, device, *arrays, current=True) -> torch.device:
    """The HIP device a call targets: ``device``, else the device of the first tensor among ``arrays``, else the current device.  ``current=False``
    never consults the current device: a target must be given, and is returned as given."""
    for a in arrays:
        if device is None and isinstance(a, torch.Tensor):
            device = a.device
    if device is None and current and torch.cuda.is_available():
        device = "cuda"
    device = torch.device(device) if device is not None else None
    if device is None or device.type != "cuda":
        raise HipExtError(f"{who}: target device {device} is not a HIP device (the HIP path has no CPU fallback)")
    return with_index(device) if current else device


def from_numpy(a) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy())      # a decoded image is a read-only view; the tensor only feeds a copy to the device


def _to_device(who, x, device, name):
    if isinstance(x, np.ndarray):
        return from_numpy(x).to(device)
    if x.device != device:
        raise HipExtError(f"{who}: {name} on {x.device}, expected on the HIP device {device}")
    return x


def check_planar(who, x, dtypes, label="expected", shapes="[h, w] or [n, h, w]"):
    """Type, dtype (one of the torch ``dtypes``) and shape (2 or 3 axes, none empty; ``shapes`` is what the message calls them) of a planar
    argument, before any device is looked at: TypeError / ValueError whose text starts "{who}: {label}".  Returns whether it has 2 axes."""
    names = [str(d).replace("torch.", "") for d in dtypes]
    if isinstance(x, np.ndarray):
        ok = x.dtype in tuple(np.dtype(n) for n in names)
    elif isinstance(x, torch.Tensor):
        ok = x.dtype in dtypes
    else:
        raise TypeError(f"{who}: {label} a numpy array or a torch tensor, got {type(x).__name__}")
    if not ok:
        raise TypeError(f"{who}: {label} {' or '.join(names)}, got {x.dtype}")
    if x.ndim not in (2, 3) or min(x.shape) < 1:
        raise ValueError(f"{who}: {label} {shapes}, got shape {tuple(x.shape)}")
    return x.ndim == 2


def stage_planar(who, x, device, name, limits=True) -> torch.Tensor:
    """A checked planar argument on ``device`` as [n, h, w] with packed rows: numpy is copied, a device tensor is read in place at its own pitches (a
    crop of a larger tensor stays a view) and made contiguous only when its rows are not packed.  bool is viewed as uint8.  ``limits``: h * w < 2^31
    and n <= 65535 are required here (ValueError); False leaves the sizes to the kernel."""
    t = _to_device(who, x, device, name)
    if t.dim() == 2:
        t = t[None]
    n, h, w = t.shape
    if limits and (h * w >= 2 ** 31 or n > 65535):
        raise ValueError(f"{who}: h * w must stay below 2^31 and n within 65535, got {tuple(t.shape)}")
    if not (t.stride(2) == 1 and t.stride(1) >= w and (n == 1 or t.stride(0) >= (h - 1) * t.stride(1) + w)):
        t = t.contiguous()
    return _u8(t)


def stage_hwc(who, img, device, name="image") -> torch.Tensor:
    """Checked uint8 pixels [h, w, c] on ``device``: numpy is copied, a device tensor is read in place at its own row stride and made contiguous only
    when its pixels are not packed."""
    t = _to_device(who, img, device, name)
    c = t.shape[2]
    return t if t.stride(2) == 1 and t.stride(1) == c and t.stride(0) >= t.shape[1] * c else t.contiguous()


class DeviceCache:
    """key -> value built once by ``make()``, the ``max_entries`` most recently used kept."""

    def __init__(self, max_entries):
        self.max_entries = max_entries
        self._entries = OrderedDict()

    def get(self, key, make):
        if key in self._entries:
            self._entries.move_to_end(key)
        else:
            self._entries[key] = make()
            while len(self._entries) > self.max_entries:
                self._entries.popitem(last=False)
        return self._entries[key]
