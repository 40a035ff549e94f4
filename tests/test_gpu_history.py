"""GPU: a forward is a function of its input -- never of what the engine's Workspace (hip_ext/engine.py) held before the call.

The Workspace of a shape is allocated once with torch.zeros and reused by every later forward of that shape: the zero borders of the 3x3 convolutions'
operand maps are written once, the pad columns behind a logical width never, and several fp32 buffers share storage by lifetime (zf / rnx, r / ipf,
oc1 over r[0] | s[0]).  Every test here runs an input A, then inputs chosen to leave as much behind as an input can (another seed of checkerboards, a
10^4-fold image whose operand stores saturate, an all-NaN image), then A again, and holds the two results of A -- and the bytes of every buffer of the
Workspace behind them -- to each other bit for bit.  The forked head (chains 1-3 on side streams) is held to the serial head the same way, a replayed
graph to plain launches, and a rebuilt Workspace (LRU eviction) to the first one.  No tolerance anywhere; what a fresh result must be is pinned to the
oracle by test_gpu_model.py and test_gpu_fuzz.py on the same models."""
import copy

import numpy as np
import pytest
import torch

from _cases import build_product_model, case_inputs, load_golden, synth_state_dict
from src.util.synth_weights import make_inputs

pytestmark = pytest.mark.gpu

RAW_VITS = dict(kind="raw", encoder="vits", features=64, out_channels=[48, 96, 192, 384])
# family -> (golden fixture whose weights (and, where the shape is kept, inputs) are used, overrides of its case, module attributes)
FAMILIES = {
    "amodal_vits_mask_b1": ("vits_g_mask", {}, {}),
    "amodal_vits_observation_b3": ("vits_g_observation", dict(B=3), {}),
    "amodal_vitb_b1": ("vitb_518", dict(H=126, W=154, B=1, seed=71), {}),
    "amodal_vitb_b3": ("vitb_518", dict(H=98, W=154, B=3, seed=72), {}),
    "amodal_vitb_b1_two_launch_tail": ("vitb_518", dict(H=126, W=154, B=1, seed=71), {}),
    "raw_vits": ("raw_vits_126x154_w1", {}, {}),
    "raw_vits_single": ("raw_vits_126x154_w1", {}, dict(head_precision="single")),
    "raw_vits_clstoken": ("raw_vits_clstoken", {}, {}),
    "raw_vits_bn": ("raw_vits_bn", {}, {}),
}
# Buffers left out of the Workspace comparison of a family, by name, at most two per family: name -> the kernel that rewrites all of what any later
# launch reads, and why the rest may differ.  The output comparison has no exceptions.
LEFT_OUT = {name: {} for name in FAMILIES}


def workspace_bytes(ws):
    """{name: uint8 view} of every tensor a Workspace holds, tensors inside lists and dicts included; entries over the same memory (same data_ptr and
    size: zf / rnx, r[i] / ipf[i]) once.  Bytes, so that a NaN equals itself."""
    out, seen = {}, set()

    def add(name, v):
        if isinstance(v, torch.Tensor):
            key = (v.data_ptr(), v.numel() * v.element_size())
            if key not in seen:
                seen.add(key)
                out[name] = v.contiguous().view(torch.uint8)
        elif isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                add(f"{name}[{i}]", e)
        elif isinstance(v, dict):
            for k, e in v.items():
                add(f"{name}[{k}]", e)
    for name, v in sorted(vars(ws).items()):
        add(name, v)
    return out


def snapshot(ws):
    torch.cuda.synchronize()
    return {name: t.clone() for name, t in workspace_bytes(ws).items()}


def _where(ws, name, byte):
    """The element of a buffer that holds flat byte ``byte``, in the buffer's own shape: (image, row, column, channel) of a zero-bordered operand map,
    (row, column) of a row buffer -- with what that says about where it lies."""
    t = ws
    for part in name.replace("]", "").split("["):
        t = t[int(part) if part.isdigit() else part] if isinstance(t, (list, dict)) else getattr(t, part)
    idx = tuple(int(v) for v in np.unravel_index(byte // t.element_size(), tuple(t.shape)))
    note = ""
    if t.dim() == 4:
        border = idx[1] in (0, t.shape[1] - 1) or idx[2] in (0, t.shape[2] - 1)
        note = " -- on the zero BORDER" if border else " -- interior pixel (a high channel index is a pad column)"
    return f"{name} {tuple(t.shape)} {t.dtype}: first differing byte {byte} = element {idx}{note}"


def assert_same_workspace(ws, before, what, left_out=()):
    torch.cuda.synchronize()
    now = workspace_bytes(ws)
    assert set(now) == set(before), (what, sorted(set(now) ^ set(before)))
    bad = []
    for name, t in now.items():
        if name in left_out or torch.equal(t, before[name]):
            continue
        diff = torch.nonzero(t.reshape(-1) != before[name].reshape(-1))
        bad.append(_where(ws, name, int(diff[0])) + f"; {diff.numel()} bytes differ")
    for line in bad:
        print(f"{what}: {line}")
    assert not bad, f"{what}: the Workspace depends on the call before -- " + " | ".join(bad)


def hostile(case, a):
    """Three inputs of A's shape that leave as much behind as an input can: (i) checkerboards of another seed, (ii) A's image times 10^4 with the mask
    inverted -- finite, the operand stores saturate (test_mlp_hidden_saturation_is_finite_and_observable: safe) -- and (iii) NaN everywhere."""
    x, grgb, mask, obs = a
    checker = list(t.cuda() for t in make_inputs(x.shape[0], x.shape[-2], x.shape[-1], seed=case.get("seed", 0) + 977, style="checker"))
    if case["kind"] == "raw":      # the raw model takes the ImageNet-normalised image (case_inputs)
        checker[0] = (checker[0] - x.new_tensor((0.485, 0.456, 0.406)).view(-1, 1, 1)) / x.new_tensor((0.229, 0.224, 0.225)).view(-1, 1, 1)
    nan = lambda t: torch.full_like(t, float("nan"))      # noqa: E731
    return {"checker": tuple(checker), "x1e4": (x * 1e4, grgb, -mask, obs), "nan": (nan(x), nan(grgb), nan(mask), nan(obs))}


class _Family:
    def __init__(self, name):
        fixture, over, attrs = FAMILIES[name]
        _, meta = load_golden(fixture)
        self.name, self.case = name, dict(meta["case"], **over)
        model = build_product_model(self.case)
        model.load_state_dict(synth_state_dict(model, meta), strict=True)
        self.model = model.cuda()
        self.mixin = self.model if self.case["kind"] == "raw" else self.model.encoder
        self.mixin.precision_ladder = False
        for k, v in attrs.items():
            setattr(self.mixin, k, v)
        self.a = tuple(t.cuda() for t in case_inputs(self.case))
        self.key = (self.case["B"], self.case["H"], self.case["W"], str(self.a[0].device))

    def __call__(self, ins):
        x, grgb, mask, obs = ins
        with torch.no_grad():
            if self.case["kind"] == "raw":
                return self.model(x)
            return self.model(x, guide_rgb=grgb, guide_mask=mask, observation=obs)

    def fresh(self):
        """The engine with no Workspace and no graph: the next forward allocates a new, zeroed Workspace (what a new model has) without paying for
        another pack of the weights."""
        eng = self.mixin._engine()
        torch.cuda.synchronize()
        eng._ws.clear()
        eng._ws_hi.clear()
        eng._graphs.clear()
        return eng

    def check_paths(self, eng, E):
        """The launches the family is named for are on the path."""
        w = eng.w
        if self.name.startswith("amodal_vitb"):
            ws = eng._ws[self.key]
            assert set(w.sp) == {0, 1} and w.oc1c is not None and ws.fused_tail == ("two_launch" not in self.name), (set(w.sp), w.oc1c is None, ws.fused_tail)
            assert (ws.fin is None) == ws.fused_tail
        elif self.name.startswith("amodal_vits"):
            assert w.split_head and w.amodal_head
        elif self.name == "raw_vits_single":
            assert set(w.sp) == {0, 1} and not w.amodal_head and set(eng._ws[self.key].spf) == {0, 1}
        elif self.name == "raw_vits_clstoken":
            assert w.readout and len(eng._ws[self.key].taps_ro) == 4
        elif self.name == "raw_vits_bn":
            assert any(k.endswith("bn1.running_var") for k in self.model.state_dict())


@pytest.fixture(scope="module")
def families(hip):
    """name -> _Family, each model built once for the module."""
    built = {}

    def get(name):
        base = name.replace("_two_launch_tail", "")      # the same model; FUSED_TAIL is read when a Workspace is built (_modes, _Family.fresh)
        if base not in built:
            built[base] = _Family(base)
        fam = copy.copy(built[base])
        fam.name = name
        return fam
    yield get
    built.clear()
    torch.cuda.empty_cache()


def _modes(monkeypatch, name, graph="0", streams=None):
    from hip_ext import engine as E
    monkeypatch.setattr(E, "GRAPH_MODE", graph)
    monkeypatch.setattr(E, "FUSED_TAIL", "two_launch" not in name)
    if streams is not None:
        monkeypatch.setattr(E, "HEAD_STREAMS", streams)
    return E


# ---- 1. fresh, after B, after B again ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FAMILIES))
def test_same_bits_after_hostile_inputs(families, monkeypatch, name):
    """out1 = f(A) on a new Workspace; then, for each hostile B, f(B) and out2 = f(A): out2 is out1, and every buffer of the Workspace holds after out2
    what it held after out1, byte for byte.  Ladder off, plain launches.  An all-NaN B is run, not refused (what it returns is not this test's
    business: the saturating operand stores do not carry every NaN through), and nothing of it survives."""
    E = _modes(monkeypatch, name)
    fam = families(name)
    eng = fam.fresh()
    out1 = fam(fam.a).clone()
    assert fam.mixin._engine() is eng and eng.ladder is None and list(eng._ws) == [fam.key]
    fam.check_paths(eng, E)
    ws = eng._ws[fam.key]
    before = snapshot(ws)
    assert torch.isfinite(out1).all()
    assert len(LEFT_OUT[name]) <= 2
    for label, b in hostile(fam.case, fam.a).items():
        out_b = fam(b).clone()
        assert not torch.equal(out_b, out1), label
        out2 = fam(fam.a)
        assert eng._ws[fam.key] is ws
        same = torch.equal(out1, out2)
        if not same:
            diff = torch.nonzero((out1 != out2).reshape(-1))
            idx = tuple(int(v) for v in np.unravel_index(int(diff[0]), tuple(out1.shape)))
            print(f"{name} after {label}: {diff.numel()} output elements differ, the first at {idx}: {float(out1[idx])!r} -> {float(out2[idx])!r}")
        assert_same_workspace(ws, before, f"{name} after {label}", LEFT_OUT[name])
        assert same, f"{name}: f(A) after {label} is not f(A) on a fresh workspace"


# ---- 2. the ladder on: host mode and device mode ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vitb_ladder(hip):
    """vitb_518's weights (sigmoid ViT-B: all three rungs) at 126 x 154 with the ladder on, and two single images whose first-rung ratios r lie far apart:
    the fixture's noise image and the darkest of its dimmed copies (a darker image has a lower map and a larger r)."""
    _, meta = load_golden("vitb_518")
    case = dict(meta["case"], H=126, W=154, B=1, seed=73)
    model = build_product_model(case)
    model.load_state_dict(synth_state_dict(model, meta), strict=True)
    model = model.cuda()
    x, grgb, mask, obs = (t.cuda() for t in case_inputs(case))
    enc = model.encoder

    def run(xv):
        with torch.no_grad():
            return model(xv, guide_rgb=None, guide_mask=mask, observation=obs).clone()
    run(x)
    eng = enc._engine()
    assert eng.ladder is not None and "make" in eng.ladder and "make3" in eng.ladder and enc.ladder_calibration is not None
    calibrated = dict(r=eng.ladder["r"], r3=eng.ladder["r3"])
    eng.ladder["r"] = eng.ladder["r3"] = float("inf")      # the first-rung ratios themselves: nothing escalates while they are read
    eng._start_rung, e0, ratios = 1, eng.escalated, {}
    for dim in (1.0, 0.5, 0.25, 0.0625):
        run(x * dim)
        assert eng.escalated == e0 and enc._engine() is eng, "a diversity trigger fired on a noise image"
        ratios[dim] = float(eng.last_ratio[0])
    print(f"vitb 126x154: first-rung r by brightness {ratios}; calibrated thresholds {calibrated}")
    yield model, enc, eng, run, x, ratios
    enc.ladder_on_device = False


def _clearly(lo, hi, thr, g):
    """test_gpu_model._mixed_thresholds' "clearly": twice the guard band on either side of the threshold."""
    return lo * (1 + 2 * g) < thr and thr * (1 + 2 * g) < hi


@pytest.mark.parametrize("rung", [2, 3])
@pytest.mark.parametrize("device_mode", [False, True], ids=["host", "device"])
def test_ladder_on_same_bits_after_a_call_that_escalates(vitb_ladder, monkeypatch, rung, device_mode):
    """A stays on the first rung, B goes to the second (third) rung -- the thresholds are placed between their ratios, both clearly outside the guard band
    -- so B's call flips the engine's start rung, fills the head-only workspaces of _ws_hi (the third-rung engine's Workspace) and, in host mode, the
    next call of A runs that rung first and falls back.  f(A) before and after are the same bits; then the roles swapped: A escalates, B does not."""
    from hip_ext import engine as E
    monkeypatch.setattr(E, "GRAPH_MODE", "0")
    model, enc, eng, run, x, ratios = vitb_ladder
    g = E.LADDER_GUARD
    dim = max(ratios, key=ratios.get)
    r_lo, r_hi = ratios[1.0], ratios[dim]
    thr = (r_lo * r_hi) ** 0.5
    assert dim != 1.0 and _clearly(r_lo, r_hi, thr, g), (ratios, thr, g)
    eng.ladder["r"], eng.ladder["r3"] = (thr, float("inf")) if rung == 2 else (thr, thr)
    stays, goes = x, x * dim
    enc.ladder_on_device = device_mode
    try:
        for a, b, a_rung, b_rung in ((stays, goes, 1, rung), (goes, stays, rung, 1)):
            eng._start_rung = 1
            counts = lambda: (eng.escalated, eng.escalated3, eng.second_rung_first_calls + eng.third_rung_first_calls, eng._start_rung)      # noqa: E731
            c0 = counts()
            first = run(a)
            c1 = counts()
            other = run(b)
            c2 = counts()
            again = run(a)
            c3 = counts()
            if device_mode:      # nothing is decided in Python: the books stand still, the device names the rung
                rep = eng.device_ladder_report()
                assert rep["rungs"].tolist() == [a_rung] and c0 == c1 == c2 == c3, (rep, c0, c3)
            else:                # (escalated, escalated3, calls that ran another rung first) per call, and the start rung each call leaves: B's flips it
                step = lambda p, q, k, start: (p[0] - q[0], p[1] - q[1], p[2] - q[2], p[3]) == (int(k >= 2), int(k == 3), int(start != 1), k)      # noqa: E731
                assert step(c1, c0, a_rung, 1) and step(c2, c1, b_rung, a_rung) and step(c3, c2, a_rung, b_rung), (c0, c1, c2, c3)
            assert enc._engine() is eng
            assert not torch.equal(first, other)
            assert torch.equal(first, again), f"rung {a_rung} image after a rung {b_rung} image: other bits"
        if not device_mode:
            assert len(eng._ws_hi) >= 1 and (rung == 2 or eng._eng3 is not None)
    finally:
        enc.ladder_on_device = False
        eng._start_rung = 1


# ---- 3. forked equals serial ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FAMILIES))
def test_forked_head_equals_serial_head(families, monkeypatch, name):
    """HEAD_STREAMS "0" (every chain on the caller's stream) against "1" (chains 1-3 on three side streams over the same aliased buffers): serial,
    forked, serial, forked on one model, one input and one Workspace -- the same output and the same Workspace bytes all four times."""
    fam = families(name)
    _modes(monkeypatch, name, streams="0")
    eng = fam.fresh()
    out = fam(fam.a).clone()
    ws = eng._ws[fam.key]
    before = snapshot(ws)
    for i, streams in enumerate(("1", "0", "1")):
        _modes(monkeypatch, name, streams=streams)
        got = fam(fam.a)
        what = f"{name}: run {i + 2} (HEAD_STREAMS = {streams})"
        assert_same_workspace(ws, before, what)
        assert torch.equal(out, got), f"{what}: other bits than the serial head"
    assert eng._ws[fam.key] is ws and len(eng._streams) == 1


# ---- 4. graph replay after B ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["amodal_vits_mask_b1", "raw_vits"])
def test_graph_replay_after_hostile_inputs(families, monkeypatch, name):
    """One ViT-S image under GRAPH_MODE "auto": the shape is captured on its second sighting; replay(A), replay(B), replay(A) for every hostile B --
    every replay of A is the eager result."""
    fam = families(name)
    E = _modes(monkeypatch, name)
    eng = fam.fresh()
    out1 = fam(fam.a).clone()
    _modes(monkeypatch, name, graph="auto")
    assert torch.equal(fam(fam.a), out1)                                   # first sighting: plain launches
    assert not any(isinstance(g, E._GraphedForward) for g in eng._graphs.values())
    assert torch.equal(fam(fam.a), out1), "replay(A) right after the capture"
    assert [isinstance(g, E._GraphedForward) for g in eng._graphs.values()] == [True], "the forward was not captured"
    for label, b in hostile(fam.case, fam.a).items():
        assert not torch.equal(fam(b), out1), label
        assert torch.equal(fam(fam.a), out1), f"{name}: replay(A) after replay({label})"


# ---- 5. eviction ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["amodal_vits_mask_b1", "amodal_vitb_b1"])
def test_rebuilt_workspace_after_eviction(families, monkeypatch, name):
    """MAX_WORKSPACES = 2: A at its shape, three other shapes (the first Workspace is dropped and its memory handed out again), then A: the rebuilt
    Workspace gives the first one's bits."""
    fam = families(name)
    E = _modes(monkeypatch, name)
    monkeypatch.setattr(E, "MAX_WORKSPACES", 2)
    eng = fam.fresh()
    out1 = fam(fam.a).clone()
    first = eng._ws[fam.key]
    for i, (h, w) in enumerate(((140, 140), (154, 126), (112, 168))):
        other = dict(fam.case, H=h, W=w)
        b = hostile(other, tuple(t.cuda() for t in case_inputs(other, seed=10 + i)))["x1e4" if i else "nan"]
        fam(b)
    assert fam.key not in eng._ws and len(eng._ws) == 2
    del first
    out2 = fam(fam.a)
    assert fam.key in eng._ws
    assert torch.equal(out1, out2)
