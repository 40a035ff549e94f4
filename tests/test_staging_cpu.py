"""CPU: hip_ext._staging, the host-input helpers of the domain modules -- the target device is a HIP device or the call raises, the planar check
raises the pinned exception types before any device is looked at, and DeviceCache keeps the most recently used entries."""
import numpy as np
import pytest
import torch

import hip_ext
from hip_ext import _staging as S


def test_resolve_device_without_a_gpu_and_without_a_target_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # the same on a machine that has one
    with pytest.raises(hip_ext.HipExtError, match="not a HIP device"):
        S.resolve_device("who", None)
    with pytest.raises(hip_ext.HipExtError, match="not a HIP device"):
        S.resolve_device("who", None, np.zeros((2, 2), np.uint8), None)


def test_resolve_device_refuses_a_cpu_target_and_a_cpu_tensor():
    with pytest.raises(hip_ext.HipExtError, match="not a HIP device"):
        S.resolve_device("who", "cpu")
    with pytest.raises(hip_ext.HipExtError, match="not a HIP device"):
        S.resolve_device("who", torch.device("cpu"), torch.zeros(2, 2))
    with pytest.raises(hip_ext.HipExtError, match="who: target device cpu is not a HIP device .*no CPU fallback"):
        S.resolve_device("who", None, None, torch.zeros(2, 2))          # the first tensor names the device
    with pytest.raises(hip_ext.HipExtError, match="target device None"):
        S.resolve_device("who", None, current=False)                    # no target and no fallback asked for
    assert S.resolve_device("who", "cuda:1", current=False) == torch.device("cuda", 1)      # a given target is taken as given, no device is touched
    assert S.with_index("cpu") == torch.device("cpu") and S.with_index("cuda:3") == torch.device("cuda", 3)


def test_check_planar_types_and_shapes():
    kinds = (torch.uint8, torch.bool)
    assert S.check_planar("f", np.zeros((3, 4), np.uint8), kinds) is True and S.check_planar("f", torch.zeros(2, 3, 4, dtype=torch.bool), kinds) is False
    with pytest.raises(TypeError, match="f: mask must be a numpy array or a torch tensor, got list"):
        S.check_planar("f", [[1]], kinds, "mask must be")
    with pytest.raises(TypeError, match="f: expected uint8 or bool, got float32"):
        S.check_planar("f", np.zeros((3, 4), np.float32), kinds)
    with pytest.raises(TypeError, match="f: x: expected float32, got torch.float64"):
        S.check_planar("f", torch.zeros(3, 4, dtype=torch.float64), (torch.float32,), "x: expected")
    for bad in (np.zeros(4, np.uint8), np.zeros((1, 2, 3, 4), np.uint8), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError, match="got shape"):
            S.check_planar("f", bad, kinds)


def test_as_int_takes_integers_only():
    assert S.as_int(7) == 7 and S.as_int(np.int64(7)) == 7 and S.as_int(torch.tensor(7)) == 7
    assert S.as_int(True) is None and S.as_int(7.0) is None and S.as_int("7") is None and S.as_int(None) is None


def test_device_cache_evicts_the_oldest_entry_and_a_hit_refreshes():
    cache, made = S.DeviceCache(2), []

    def make(k):
        def f():
            made.append(k)
            return torch.full((2,), k)
        return f
    a = cache.get("a", make(1))
    assert cache.get("a", make(9)) is a and made == [1]               # a hit returns the cached tensor and builds nothing
    cache.get("b", make(2))
    cache.get("c", make(3))                                           # "a" is the oldest: evicted
    assert list(cache._entries) == ["b", "c"]
    cache.get("b", make(9))                                           # a hit refreshes "b" ...
    cache.get("d", make(4))                                           # ... so "c" goes
    assert list(cache._entries) == ["b", "d"] and made == [1, 2, 3, 4]
    assert torch.equal(cache.get("a", make(5)), torch.full((2,), 5)) and made[-1] == 5      # an evicted key is built again


def test_the_modules_caches_are_bounded():
    from hip_ext import edges, image, labels
    assert (labels._TABLES.max_entries, edges._WEIGHTS.max_entries) == (64, 16) and image._LUTS.max_entries >= 16
    lut = image.colormap_lut("Spectral_r")
    assert image.colormap_lut("Spectral_r") is lut and lut.device.type == "cpu" and tuple(lut.shape) == (256, 3)
