"""CPU: the host side of the precision ladder's device mode -- hip_ext.ladder.stats_from_host against the arithmetic it replaced inside
DepthEngine._image_stats (restated here), the NaN rule the device kernel is held to, the new export's declaration and binding, and the module attribute."""
import inspect
import os
import re

import pytest
import torch

import hip_ext
from hip_ext.ladder import ladder_decide, stats_from_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS, GROUPS, GROUPS_IN = 8, 12, 10


def _stat_buf(seed, B, spread=10):
    g = torch.Generator().manual_seed(seed)
    n = B * (CHUNKS + GROUPS + GROUPS_IN) * 2
    return ((0.5 + torch.rand(n, generator=g)) * torch.exp2(torch.randint(-spread, spread, (n,), generator=g).float())).float()


def _inline(host, B, D, has_r, has_div, has_in, lad):
    """DepthEngine._image_stats' arithmetic as it stood before the helper (STAT_CHUNKS = 8), word for word."""
    nst, ndv = B * CHUNKS * 2, B * ((D + 63) // 64) * 2
    st = host[:nst].view(B, CHUNKS, 2).sum(1)
    r = st[:, 1] / st[:, 0].clamp_min(1e-300) if has_r else torch.zeros(B, dtype=torch.float64)
    flat = torch.zeros(B, dtype=torch.bool)
    tap_div = in_div = None
    if has_div:
        dv = host[nst:nst + ndv].view(B, -1, 2).sum(1)
        tap_div = dv[:, 0] / dv[:, 1].clamp_min(1e-300)
        flat = tap_div < lad["div"]
    if has_in:
        di = host[nst + ndv:].view(B, -1, 2).sum(1)
        in_div = di[:, 0] / di[:, 1].clamp_min(1e-300)
        flat = flat | (in_div < lad.get("div_in", 1e-4))
    return r, flat, tap_div, in_div


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype == torch.bool:
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0).view(torch.int64), torch.nan_to_num(b, nan=0.0).view(torch.int64))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("spread", [10, 40])      # 2^20: every sum exact;  2^80: rounded sums -- the helper must still be the inline arithmetic, bit for bit
def test_helper_is_the_inline_arithmetic(B, spread):
    buf = _stat_buf(21 + B, B, spread)
    buf[:B * CHUNKS * 2].view(B, CHUNKS, 2)[0, 3, 0] = float("nan")
    if B > 1:
        buf[:B * CHUNKS * 2].view(B, CHUNKS, 2)[1, :, 0] = 0.0
    host = buf.double()
    D = GROUPS * 64
    for has_r in (True, False):
        for has_div in (True, False):
            for has_in in (True, False):
                lad = dict(div=0.7, div_in=0.9)
                want = _inline(host, B, D, has_r, has_div, has_in, lad)
                got = stats_from_host(host, B, CHUNKS, GROUPS, has_r, lad["div"] if has_div else None, has_in, lad["div_in"])
                assert all(_same(a, b) for a, b in zip(got, want)), (has_r, has_div, has_in, got, want)
    got = stats_from_host(host, B, CHUNKS, GROUPS, True, 0.0, True)      # div = 0: no tap trigger;  div_in defaults to 1e-4
    want = _inline(host, B, D, True, False, True, {})
    assert all(_same(a, b) for a, b in zip(got, want))


def test_nan_statistics_stay_on_the_first_rung():
    """The rule the device kernel restates with a comparison instead of fmax: clamp_min lets a NaN through, and a NaN exceeds no threshold."""
    B = 3
    buf = _stat_buf(5, B)
    sums = buf[:B * CHUNKS * 2].view(B, CHUNKS, 2)
    sums[0, 2, 0] = float("nan")          # S0 NaN, S1 a finite count
    sums[1, :, 0] = 0.0                   # S0 = 0: r = S1 / 1e-300
    r, flat, _, _ = stats_from_host(buf.double(), B, CHUNKS, GROUPS, True, None, False)
    assert torch.isnan(r[0]) and float(r[1]) > 1e290 and not flat.any()
    lad = dict(make=None, make3=None, r=0.5, r3=2.0)
    rung = ladder_decide(r, flat, lad, 1, 0.02)
    assert rung[0] == 1 and rung[1] == 3
    assert float(torch.tensor([float("nan")], dtype=torch.float64).clamp_min(1e-300).isnan().sum()) == 1


def test_export_is_declared_bound_and_built():
    assert "ada_ladder_select_fwd" in hip_ext.EXPORTS and hip_ext.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "ada_hip.h")).read()
    m = re.search(r"\bint\s+ada_ladder_select_fwd\s*\(([^;]*)\)\s*;", header)
    assert m, "ada_ladder_select_fwd is not declared in ada_hip.h"
    lib = hip_ext.load()
    assert len(lib.ada_ladder_select_fwd.argtypes) == len(m.group(1).split(",")) == 22
    build_py = open(os.path.join(ROOT, "amodal-depth-anything_amd", "csrc", "build.py")).read()
    assert '"ada_ladder.hip"' in build_py and "-ffast-math" not in build_py and "-Ofast" not in build_py      # the fp64 division must stay the correctly rounded one
    assert callable(hip_ext.ladder_select)


def test_ladder_select_has_no_cpu_fallback():
    B, n = 2, 8
    sums = torch.zeros(B, CHUNKS, 2)
    with pytest.raises(hip_ext.HipExtError, match="HIP device"):
        hip_ext.ladder_select(sums, None, None, 0.5, 0.9, 0.0, 1e-4, True, True, True, torch.zeros(B, n), None, None,
                              torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.float64), torch.zeros(4, dtype=torch.int64))


def test_module_attribute_and_engine_parameter():
    from hip_ext.engine import DepthEngine
    from src.models.amodalsynthdrive.depth_anything_v2.dpt import DepthAnythingV2 as Amodal, _EngineMixin
    from src.models.amodalsynthdrive.depth_anything_v2_raw.dpt import DepthAnythingV2 as Raw
    assert _EngineMixin.ladder_on_device is False and Amodal.ladder_on_device is False and Raw.ladder_on_device is False
    assert inspect.signature(DepthEngine.forward).parameters["on_device"].default is False
    assert callable(DepthEngine.device_ladder_report)
    # the attribute is read at the forward, not when the engine is stamped
    src = inspect.getsource(_EngineMixin._engine)
    assert "ladder_on_device" not in src and "ladder_on_device" in inspect.getsource(_EngineMixin._run)
