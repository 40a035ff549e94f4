"""GPU: the precision ladder in its DEVICE mode (module.ladder_on_device; hip_ext.engine.DepthEngine._ladder_device; ada_ladder_select_fwd).

Kernel, without a model: rung and r against hip_ext.ladder.ladder_decide fed by hip_ext.ladder.stats_from_host from a host copy of the same statistics buffer,
every row of the output against the source its rung names, bit for bit.  The crafted chunk sums spread over 2^20 in magnitude: a sum of up to 16 fp32 terms
(24 bits each) then needs at most 24 + 20 + 4 = 48 bits and is exact in fp64 in ANY order -- the host's torch sum and the device's index-order sum must agree,
whatever order this torch build picks.  Model: a captured and replayed device-mode forward returns the eager ladder's bits; a mixed batch carries, image by image,
the rows of the rung its statistics name; the replayed output is inside the project's one tolerance."""
import math

import pytest
import torch

from _cases import build_product_model, case_inputs, fixture_model, load_golden, rel_l1, synth_state_dict
from src.util.synth_weights import make_inputs
from test_gpu_model import TOL

pytestmark = pytest.mark.gpu

B5 = 5
CHUNKS, GROUPS, GROUPS_IN = 8, 12, 10
INF = float("inf")


# ---- kernel, no model ---------------------------------------------------------------------------------------------------------------

def _stat_buf(seed, B=B5):
    """A Workspace.stat_buf look-alike: [B, CHUNKS, 2 | B, GROUPS, 2 | B, GROUPS_IN, 2] fp32, positive, magnitudes spread over 2^20."""
    g = torch.Generator().manual_seed(seed)
    n = B * (CHUNKS + GROUPS + GROUPS_IN) * 2
    buf = (0.5 + torch.rand(n, generator=g)) * torch.exp2(torch.randint(-10, 10, (n,), generator=g).float())
    return buf.float()


def _views(buf, B=B5):
    a, b = B * CHUNKS * 2, B * (CHUNKS + GROUPS) * 2
    return buf[:a].view(B, CHUNKS, 2), buf[a:b].view(B, GROUPS, 2), buf[b:].view(B, GROUPS_IN, 2)


def _pattern(source, B, n):
    """fp32 [B, n] whose word (b, i) is the bit pattern source << 28 | b << 24 | i: distinct per (source, image, index)."""
    w = (source << 28) | (torch.arange(B, dtype=torch.int64).view(B, 1) << 24) | torch.arange(n, dtype=torch.int64).view(1, n)
    return w.to(torch.int32).view(torch.float32).contiguous()


def _host(buf, B, has2, has3, has_r, thr, thr3, div, div_in, use_div, use_in):
    """(rung, r, flat, tap_div, in_div) as the HOST decides them from a host copy of the buffer."""
    from hip_ext.ladder import ladder_decide, stats_from_host
    host = buf.cpu().double()
    if not use_in:      # stats_from_host reads everything behind the tap block as the input block
        host = host[:B * (CHUNKS + GROUPS) * 2]
    r, flat, tap_div, in_div = stats_from_host(host, B, CHUNKS, GROUPS, has_r, div if use_div else None, use_in, div_in)
    lad = {}
    if has2:
        lad.update(make=None, r=thr)
    if has3:
        lad.update(make3=None, r3=thr3)
    return ladder_decide(r, flat, lad, 1, 0.02), r, flat, tap_div, in_div


def _run_select(hip, buf, n, *, has2=True, has3=True, has_r=True, use_div=True, use_in=True, give2=True, give3=True, thr=None, thr3=None,
                div=None, div_in=None, calls=1, B=B5):
    """Runs hip_ext.ladder_select ``calls`` times on crafted rows and checks everything against the host.  Thresholds default to values between the images'
    statistics, so that every rung occurs.  Returns the host's rung vector."""
    h0 = _host(buf, B, True, True, True, INF, INF, INF, INF, True, True)
    r_all, td_all, id_all = h0[1], h0[3], h0[4]
    srt = torch.sort(r_all).values
    thr = float((srt[0] + srt[1]) / 2) if thr is None else thr                 # the lowest r stays; ...
    thr3 = float((srt[-2] + srt[-1]) / 2) if thr3 is None else thr3             # ... the highest goes to the third rung
    div = float(torch.sort(td_all).values[0] * 1.0001) if div is None else div   # the least diverse tap is flat
    div_in = float(torch.sort(id_all).values[0] * 1.0001) if div_in is None else div_in
    rung_h, r_h, flat_h, _, _ = _host(buf, B, has2, has3, has_r, thr, thr3, div, div_in, use_div, use_in)
    dev = "cuda"
    d = buf.to(dev)
    sums, sdiv, sin = _views(d, B)
    out0, s2, s3 = (_pattern(k, B, n) for k in (1, 2, 3))
    out = out0.to(dev)
    src2, src3 = (s2.to(dev) if give2 else None), (s3.to(dev) if give3 else None)
    rung = torch.full((B,), -7, dtype=torch.int32, device=dev)
    ratio = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    for _ in range(calls):
        hip.ladder_select(sums if has_r else None, sdiv if use_div else None, sin if use_in else None, thr, thr3, div, div_in, has2, has3, has_r,
                          out, src2, src3, rung, ratio, counts)
    torch.cuda.synchronize()
    what = f"n={n} has2={has2} has3={has3} has_r={has_r} div={use_div} in={use_in} src2={give2} src3={give3}"
    assert torch.equal(rung.cpu().long(), rung_h), (what, rung.cpu().tolist(), rung_h.tolist(), r_h.tolist(), flat_h.tolist())
    r_d = ratio.cpu()      # bit for bit; a NaN for a NaN (its payload says nothing)
    assert torch.equal(torch.isnan(r_d), torch.isnan(r_h)) and torch.equal(torch.nan_to_num(r_d, nan=0.0).view(torch.int64), torch.nan_to_num(r_h, nan=0.0).view(torch.int64)), \
        (what, r_d.tolist(), r_h.tolist())
    want, unserved = out0.clone(), 0
    for b in range(B):
        k = int(rung_h[b])
        src = (s3 if give3 else s2 if give2 else None) if k == 3 else (s2 if give2 else None) if k == 2 else None
        unserved += (k == 3 and not give3) or (k == 2 and not give2)
        if src is not None:
            want[b] = src[b]
    got = out.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (what, [b for b in range(B) if not torch.equal(got[b].view(torch.int32), want[b].view(torch.int32))])
    for b in range(B):      # (part of the line above; said on its own: rows of first-rung images are not touched)
        if int(rung_h[b]) == 1:
            assert torch.equal(got[b].view(torch.int32), out0[b].view(torch.int32)), (what, b)
    n2, n3 = int((rung_h >= 2).sum()), int((rung_h == 3).sum())
    assert counts.cpu().tolist() == [calls, calls * n2, calls * n3, calls * unserved], (what, counts.cpu().tolist(), n2, n3, unserved)
    return rung_h


@pytest.mark.parametrize("n", [1, 3, 4, 77, 19404])
def test_select_rows_rungs_and_counts(hip, n):
    """Every row size of the issue (19404 = 126 x 154; 1, 3 and 77 have a word tail, and rows that begin off a 16-byte boundary), every rung in the batch, two
    calls: rung, r, rows and twice the host's counts."""
    rung = _run_select(hip, _stat_buf(11), n, calls=2)
    assert set(rung.tolist()) == {1, 2, 3}, rung.tolist()      # a condition of the test: the defaults spread the images over the rungs


@pytest.mark.parametrize("n", [77, 19404])
def test_select_sweeps_flags_and_missing_sources(hip, n):
    """has2 / has3 / has_r, absent statistics blocks, absent sources: the decision is ladder_decide's for that ladder; an image whose source is absent takes the
    best there is (rung 3 without src3: src2; else its row stays) and is counted as unserved while its rung still reads what it decided."""
    buf = _stat_buf(12)
    seen3_without_src3 = False
    for has2 in (True, False):
        for has3 in (True, False):
            for has_r in (True, False):
                for use_div, use_in in ((True, True), (False, True), (True, False), (False, False)):
                    rung = _run_select(hip, buf, n, has2=has2, has3=has3, has_r=has_r, use_div=use_div, use_in=use_in)
                    assert has2 or 2 not in rung.tolist()
                    assert has3 or 3 not in rung.tolist()
    for give2, give3 in ((True, False), (False, True), (False, False)):
        rung = _run_select(hip, buf, n, give2=give2, give3=give3, calls=2)
        seen3_without_src3 |= (not give3) and 3 in rung.tolist() and 2 in rung.tolist()
    assert seen3_without_src3
    # a ladder without a second rung (the raw models): rung 3 without src3 and src2 leaves the row
    _run_select(hip, buf, n, has2=False, give2=False, give3=False)
    _run_select(hip, buf, n, has2=False, give2=False, give3=True)


def test_select_ties_go_the_hosts_way(hip):
    """A threshold EQUAL to an image's statistic does not fire (r > thr, div > tap_div are strict); the next fp64 towards the statistic does."""
    buf = _stat_buf(13)
    _, r, _, td, idv = _host(buf, B5, True, True, True, INF, INF, INF, INF, True, True)
    b = 2
    rb, tdb, idb = float(r[b]), float(td[b]), float(idv[b])
    # r against thr: a ladder with a second rung only, no diversity trigger
    kw = dict(has3=False, use_div=False, use_in=False)
    assert int(_run_select(hip, buf, 77, thr=rb, **kw)[b]) == 1
    assert int(_run_select(hip, buf, 77, thr=math.nextafter(rb, 0.0), **kw)[b]) == 2
    # r against thr3
    kw = dict(has2=False, use_div=False, use_in=False)
    assert int(_run_select(hip, buf, 77, thr3=rb, **kw)[b]) == 1
    assert int(_run_select(hip, buf, 77, thr3=math.nextafter(rb, 0.0), **kw)[b]) == 3
    # the diversities: flat is `statistic < threshold`
    kw = dict(has_r=False, use_in=False)
    assert int(_run_select(hip, buf, 77, div=tdb, **kw)[b]) == 1
    assert int(_run_select(hip, buf, 77, div=math.nextafter(tdb, INF), **kw)[b]) == 3
    kw = dict(has_r=False, use_div=False)
    assert int(_run_select(hip, buf, 77, div_in=idb, **kw)[b]) == 1
    assert int(_run_select(hip, buf, 77, div_in=math.nextafter(idb, INF), **kw)[b]) == 3


def test_select_nan_and_zero_statistics_go_the_hosts_way(hip):
    """torch's clamp_min lets a NaN through, fmax would not: an image whose sum S0 is NaN and whose S1 is a finite count (a ReLU head with a NaN in its map) has
    r = NaN, which exceeds no threshold -- first rung on the host, and on the device.  Both NaN likewise; S0 = 0 divides by the clamp (r = S1 / 1e-300)."""
    buf = _stat_buf(14)
    sums, sdiv, sin = _views(buf)
    sums[0, 3, 0] = float("nan")                       # image 0: S0 NaN, S1 finite
    sums[1, 2, 0], sums[1, 5, 1] = float("nan"), float("nan")      # image 1: both NaN
    sums[2, :, 0] = 0.0                                # image 2: S0 = 0, S1 > 0
    sums[3] = 0.0                                      # image 3: 0 / clamp(0) = 0
    sdiv[4, 1, 1] = float("nan")                       # image 4: a NaN diversity is not flat
    kw = dict(use_in=False, div=1e-30, thr=0.5, thr3=1e6)      # no image is flat by its finite tap diversity
    rung = _run_select(hip, buf, 77, **kw)
    assert rung.tolist()[:4] == [1, 1, 3, 1], rung.tolist()
    rung = _run_select(hip, buf, 77, has3=False, **kw)
    assert rung.tolist()[:4] == [1, 1, 2, 1], rung.tolist()


def test_select_refuses_what_it_cannot_check(hip):
    out = torch.zeros(2, 8, device="cuda")
    rung, ratio, counts = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    sums = torch.zeros(2, CHUNKS, 2, device="cuda")
    with pytest.raises(hip.HipExtError, match="as large as out"):
        hip.ladder_select(sums, None, None, 0.5, 0.9, 0.0, 1e-4, True, True, True, out, torch.zeros(2, 4, device="cuda"), None, rung, ratio, counts)
    with pytest.raises(hip.HipExtError, match="aliases"):
        hip.ladder_select(sums, None, None, 0.5, 0.9, 0.0, 1e-4, True, True, True, out, out, None, rung, ratio, counts)
    with pytest.raises(hip.HipExtError, match="rung"):
        hip.ladder_select(sums, None, None, 0.5, 0.9, 0.0, 1e-4, True, True, True, out, None, None, rung[:1], ratio, counts)


# ---- the models ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vitb_low(hip):
    """The pinned capture test's model: vitb_518_m20's weights, final bias - 1.5 (well into the second rung's range at 126 x 154 too), on the device."""
    _, meta = load_golden("vitb_518_m20")
    case = dict(meta["case"], H=126, W=154)
    model = build_product_model(case)
    model.load_state_dict(synth_state_dict(model, meta), strict=True)
    model = model.cuda()
    with torch.no_grad():
        model.encoder.depth_head.scratch.output_conv2[2].bias.sub_(1.5)
    return model, case


def _on_side_stream(fn):
    """A warm-up outside the capture, as the pinned test makes it."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        out = fn().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return out


def _capture_equals_eager(mixin, run, want_rung, mode=True):
    """eager default mode -> device mode: one eager warm-up, capture, replay.  ``want_rung`` None: the rung the eager ladder's books name.
    Returns (eager, replayed, engine, rung)."""
    mixin.ladder_on_device = False
    eng = mixin._engine()      # (packs and calibrates on first use; the books of an engine other tests have used start where they stand)
    eng._start_rung = 1
    esc0, esc30, rep0 = eng.escalated, eng.escalated3, eng.device_ladder_report() or dict(calls=0, escalated=0, escalated3=0, unserved=0)
    eager = _on_side_stream(run)
    assert mixin._engine() is eng
    esc, esc3 = eng.escalated, eng.escalated3
    assert mixin.ladder_calibration is not None and esc - esc0 == 1, (esc, esc3, eng.last_ratio, eng.ladder)
    if want_rung is None:
        want_rung = 3 if esc3 - esc30 == 1 else 2
    assert esc3 - esc30 == int(want_rung == 3), (esc, esc3, eng.last_ratio, eng.ladder)
    mixin.ladder_on_device = mode
    try:
        warm = _on_side_stream(run)
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g):      # the capture is the proof that no host read is left: a synchronising call inside it raises
            captured = run()
        captured.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        replayed = captured.clone()
        assert mixin._engine() is eng and (eng.escalated, eng.escalated3) == (esc, esc3)      # the host-side books do not move in device mode
        rep = eng.device_ladder_report()
        assert rep["rungs"].tolist() == [want_rung], rep
        delta = {k: rep[k] - rep0[k] for k in ("calls", "escalated", "escalated3", "unserved")}      # warm-up, the capture's own launches do not run, replay: 2
        assert delta == dict(calls=2, escalated=2, escalated3=2 * int(want_rung == 3), unserved=0), (delta, rep)
        assert torch.equal(warm, eager)
        assert torch.equal(replayed, eager)
    finally:
        mixin.ladder_on_device = False
    mixin.precision_ladder = False
    try:
        with torch.no_grad():
            off = run().clone()
    finally:
        mixin.precision_ladder = None
    assert not torch.equal(replayed, off)
    return eager, replayed, eng, want_rung


def test_captured_device_ladder_equals_eager_pinned_recipe(vitb_low, monkeypatch):
    """The pinned capture test's recipe (vitb_518_m20's weights at 126 x 154, final bias - 1.5) with ladder_on_device = True: the replay of the caller's graph
    returns the eager ladder's bits, not the first rung's, and the device names the rung the eager ladder's books name (at this operating point r = 0.90 lies
    above BOTH calibrated thresholds: the eager ladder takes the image to the third rung)."""
    from hip_ext import engine as E
    monkeypatch.setattr(E, "GRAPH_MODE", "0")
    model, case = vitb_low
    x, grgb, mask, obs = (t.cuda() for t in case_inputs(case))
    _, _, eng, rung = _capture_equals_eager(model.encoder, lambda: model(x, guide_rgb=None, guide_mask=mask, observation=obs), None)
    print(f"captured device-mode forward == eager ladder: rung {rung} (r = {float(eng.last_ratio_dev[0]):.3f} against {eng.ladder['r']:.3f} / {eng.ladder['r3']:.3f})")


def test_captured_device_ladder_equals_eager_second_rung(vitb_low, monkeypatch):
    """The same model with its final bias moved to where the image's r lies between the two calibrated thresholds: the second rung (the head alone, re-run from
    the first rung's taps), captured and replayed."""
    from hip_ext import engine as E
    monkeypatch.setattr(E, "GRAPH_MODE", "0")
    model, case = vitb_low
    x, grgb, mask, obs = (t.cuda() for t in case_inputs(case))
    enc = model.encoder
    bias = enc.depth_head.scratch.output_conv2[2].bias
    b0 = bias.detach().clone()

    def run():
        return model(x, guide_rgb=None, guide_mask=mask, observation=obs)
    try:
        tried = []
        for back in (1.5, 1.25, 1.0, 0.75, 0.5, 0.25, 1.75, 2.0):      # b0 is the fixture's bias - 1.5: back towards it until r is clearly between the thresholds
            with torch.no_grad():
                bias.copy_(b0 + back)
                run()
            eng = enc._engine()
            r, lad = float(eng.last_ratio[0]), eng.ladder
            tried.append((back, round(r, 4)))
            if lad["r"] * 1.05 < r < lad["r3"] * 0.95:
                break
        assert lad["r"] * 1.05 < r < lad["r3"] * 0.95, (tried, lad["r"], lad["r3"])
        _, _, eng, _ = _capture_equals_eager(enc, run, 2)
        print(f"second rung captured: final bias + {back}, r = {float(eng.last_ratio_dev[0]):.3f} against {eng.ladder['r']:.3f} / {eng.ladder['r3']:.3f}")
    finally:
        with torch.no_grad():
            bias.copy_(b0)


def test_captured_device_ladder_equals_eager_flat_image(hip, monkeypatch):
    """vitb_126x154_zeros_m03: an all-zero input -- the diversity triggers send it to the third rung, the whole forward in split precision."""
    from hip_ext import engine as E
    monkeypatch.setattr(E, "GRAPH_MODE", "0")
    _, meta = load_golden("vitb_126x154_zeros_m03")
    case = meta["case"]
    model = build_product_model(case)
    model.load_state_dict(synth_state_dict(model, meta), strict=True)
    model = model.cuda()
    x, grgb, mask, obs = (t.cuda() for t in case_inputs(case))
    _capture_equals_eager(model.encoder, lambda: model(x, guide_rgb=None, guide_mask=mask, observation=obs), 3)


def test_captured_device_ladder_equals_eager_raw_model(hip, monkeypatch):
    """A raw model (rungs 1 and 3 only) on an un-centred map: the r trigger sends the image to the third rung.  raw_vitb_518_unc's weights at 126 x 154 -- the
    smallest raw model with an r trigger: raw ViT-S runs everything in split precision on its first rung already and its calibrated threshold is inf."""
    from hip_ext import engine as E
    monkeypatch.setattr(E, "GRAPH_MODE", "0")
    _, meta = load_golden("raw_vitb_518_unc")
    case = dict(meta["case"], H=126, W=154)
    model = build_product_model(case)
    model.load_state_dict(synth_state_dict(model, meta), strict=True)
    model = model.cuda()
    x = case_inputs(case)[0].cuda()
    bias = model.depth_head.scratch.output_conv2[2].bias
    b0 = bias.detach().clone()
    for shift in (0.0, 0.5, 1.0, 1.5, 2.0, 2.5):      # as test_third_rung_first_returns_the_same_bits: down until the image is clearly above the calibrated threshold
        with torch.no_grad():
            bias.copy_(b0 - shift)
            model(x)
        eng = model._engine()
        if float(eng.last_ratio[0]) > eng.ladder["r3"] * 1.05 and eng.last_input_diversity[0] > 1e-3:
            break
    assert "make" not in eng.ladder and float(eng.last_ratio[0]) > eng.ladder["r3"] * 1.05 and eng.last_input_diversity[0] > 1e-3, (shift, eng.last_ratio, eng.ladder)
    _capture_equals_eager(model, lambda: model(x), 3)


def test_device_ladder_under_capture_without_warm_up_is_refused(vitb_low, monkeypatch):
    """Inside a capture nothing can be packed or allocated: device mode at a shape it has not run at raises, naming the warm-up, before its first launch -- the
    capture goes on and its graph replays."""
    from hip_ext import engine as E
    from hip_ext import HipExtError
    monkeypatch.setattr(E, "GRAPH_MODE", "0")
    model, case = vitb_low
    x, grgb, mask, obs = (t[..., :126, :126].contiguous().cuda() for t in case_inputs(case))      # a shape no other test of this module runs
    enc = model.encoder

    def run():
        return model(x, guide_rgb=None, guide_mask=mask, observation=obs)
    _on_side_stream(run)                                # the DEFAULT mode's warm-up: engine, calibration, first- and second-rung workspaces
    y = torch.ones(8, device="cuda")
    enc.ladder_on_device = True
    try:
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g):
            z = y * 2
            with pytest.raises(HipExtError, match="warm up"):
                run()
            assert torch.cuda.is_current_stream_capturing()
        y.fill_(3.0)
        g.replay()
        torch.cuda.synchronize()
        assert not torch.cuda.is_current_stream_capturing() and z.tolist() == [6.0] * 8
        with torch.no_grad():
            first = run().clone()                       # and outside a capture the same call simply works
        enc.ladder_on_device = False
        with torch.no_grad():
            assert torch.equal(first, run())
    finally:
        enc.ladder_on_device = False


def test_mixed_batch_carries_each_images_rung(vitb_low, monkeypatch):
    """ViT-B, 4 x 126 x 154: two noise images, one image-like, one all-zero.  With the thresholds placed between the three first-rung ratios the device rungs are
    {1, 2, 3, 3}, and every image's rows are the rows of that rung run over the WHOLE batch; "head" mode gives the rung-3 images the second rung's rows and
    counts them as unserved."""
    from hip_ext import engine as E
    monkeypatch.setattr(E, "GRAPH_MODE", "0")
    model, case = vitb_low
    H, W = case["H"], case["W"]
    parts = [make_inputs(2, H, W, 0, style="noise"), make_inputs(1, H, W, 1, style="structured"), make_inputs(1, H, W, 0, style="zeros")]
    x, mask, obs = (torch.cat([p[i] for p in parts], 0).cuda() for i in (0, 2, 3))
    x[1] *= 0.25                                        # a darker noise image: a lower map, a larger r
    enc = model.encoder

    def run():
        with torch.no_grad():
            return model(x, guide_rgb=None, guide_mask=mask, observation=obs).clone()
    run()
    eng = enc._engine()
    seen = {}
    plain_forward = eng.forward

    def spy(x_, g_, n_=None, **kw):      # what the module hands to the engine
        seen.update(x=x_, g=g_, n=n_)
        return plain_forward(x_, g_, n_, **kw)
    eng.forward = spy
    keep = {k: eng.ladder[k] for k in ("r", "r3")}
    try:
        eng._start_rung = 1
        run()
        rr = [float(v) for v in eng.last_ratio[:3]]      # the first rung ran first: its own r
        lo, mid, hi = sorted(range(3), key=lambda i: rr[i])
        assert rr[lo] < rr[mid] < rr[hi], rr
        eng.ladder["r"], eng.ladder["r3"] = (rr[lo] + rr[mid]) / 2, (rr[mid] + rr[hi]) / 2
        want = [0, 0, 0, 3]
        want[lo], want[mid], want[hi] = 1, 2, 3
        enc.ladder_on_device = True
        out_dev = run()
        rep = eng.device_ladder_report()
        assert rep["rungs"].tolist() == want and sorted(want) == [1, 2, 3, 3], (rep, rr, eng.ladder)
        assert [float(v) for v in rep["ratio"][:3]] == rr
        xe, ge, ne = seen["x"], seen["g"], seen["n"]
        with torch.no_grad():
            o1 = eng._forward(xe, ge, ne).clone()
            ws = eng.workspace(4, H, W, xe.device)
            o2 = eng._head_for(ws, 4, None, eng._second_weights()).clone()
            o3 = eng._third_engine().forward(xe, ge, ne).clone()
        whole = {1: o1, 2: o2, 3: o3}
        for b in range(4):
            assert torch.equal(out_dev[b], whole[want[b]][b].view_as(out_dev[b])), (b, want[b])
            for k in (1, 2, 3):      # (and of no other rung: the rungs differ on every image)
                assert k == want[b] or not torch.equal(out_dev[b], whole[k][b].view_as(out_dev[b])), (b, k)
        enc.ladder_on_device = False
        eng._start_rung = 1
        n23, n3 = eng.escalated, eng.escalated3
        out_eager = run()
        assert (eng.escalated - n23, eng.escalated3 - n3) == (3, 2)
        for b in (lo, mid):
            assert torch.equal(out_dev[b], out_eager[b]), b
        same3 = [bool(torch.equal(out_dev[b], out_eager[b])) for b in (hi, 3)]
        print(f"mixed batch: r = {[round(v, 4) for v in rr]}, rungs {want}; third-rung rows of the whole batch == those of the eager ladder's two-image subset: {same3}")
        before = rep
        enc.ladder_on_device = "head"
        out_head = run()
        rep = eng.device_ladder_report()
        assert rep["rungs"].tolist() == want and rep["unserved"] - before["unserved"] == 2 and rep["escalated3"] - before["escalated3"] == 2, (rep, before)
        for b in range(4):
            assert torch.equal(out_head[b], (o1 if want[b] == 1 else o2)[b].view_as(out_head[b])), b
    finally:
        enc.ladder_on_device = False
        eng.ladder.update(keep)
        del eng.forward
        eng._start_rung = 1


@pytest.mark.parametrize("name", ["vitb_518_m20", "vitl_518_m10", "vitb_126x154_zeros_m03"])
def test_captured_device_ladder_is_inside_the_contract(hip, monkeypatch, name):
    """The fixtures whose first-rung output is outside the bar, at their golden sizes, through a captured and replayed device-mode forward: inside the project's
    one tolerance (test_gpu_model.TOL)."""
    from hip_ext import engine as E
    monkeypatch.setattr(E, "GRAPH_MODE", "0")
    gold, meta = load_golden(name)
    case = meta["case"]
    model = fixture_model(meta)
    x, grgb, mask, obs = (t.cuda() for t in case_inputs(case))
    enc = model.encoder

    def run():
        return model(x, guide_rgb=grgb, guide_mask=mask, observation=obs)
    enc.ladder_on_device = True
    try:
        _on_side_stream(run)
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g):
            captured = run()
        captured.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        out = captured.cpu()
        rep = enc._engine().device_ladder_report()
    finally:
        enc.ladder_on_device = False
    st = case["stride"]
    err = rel_l1(out[..., ::st, ::st], gold)
    print(f"{name}: captured device-mode forward, rungs {rep['rungs'].tolist()}, rel-L1 vs reference golden = {err:.3e}")
    assert min(rep["rungs"].tolist()) >= 2 and rep["unserved"] == 0, rep
    assert err <= TOL, f"{name}: rel-L1 {err:.3e} > {TOL}"
    del g, captured
    torch.cuda.empty_cache()


def test_toggling_device_mode_does_not_repack(vitb_low):
    model, case = vitb_low
    x, grgb, mask, obs = (t.cuda() for t in case_inputs(case))
    enc = model.encoder
    with torch.no_grad():
        model(x, guide_rgb=None, guide_mask=mask, observation=obs)
    eng, stamp = enc._engine(), enc._engine_stamp
    try:
        for mode in (True, "head", False):
            enc.ladder_on_device = mode
            assert enc._engine() is eng and enc._engine_stamp == stamp, mode
        enc.ladder_on_device = "tail"
        with pytest.raises(Exception, match="on_device"), torch.no_grad():
            model(x, guide_rgb=None, guide_mask=mask, observation=obs)
    finally:
        enc.ladder_on_device = False


def test_pipeline_in_device_mode_returns_the_default_modes_bits(vitb_low):
    """amodal_depth_pipeline with BOTH models in device mode (a raw ViT-S base network: rungs 1 and 3; the amodal ViT-B on a low-mean map: second rung)."""
    from hip_ext.pipeline import amodal_depth_pipeline
    am, case = vitb_low
    raw_case = dict(kind="raw", encoder="vits", features=64, out_channels=[48, 96, 192, 384])
    raw = build_product_model(raw_case)
    raw.load_state_dict(synth_state_dict(raw), strict=True)
    raw = raw.cuda()
    g = torch.Generator().manual_seed(7)
    rgb = torch.rand(1, 3, case["H"], case["W"], generator=g).cuda()
    mask = torch.zeros(1, 1, case["H"], case["W"])
    mask[0, :, 20:80, 30:100] = 1
    mask = mask.cuda()
    want = [t.clone() for t in amodal_depth_pipeline(raw, am, rgb, mask)]
    eng = am.encoder._engine()
    assert float(eng.last_ratio[0]) > eng.ladder["r"], (eng.last_ratio, eng.ladder)      # a low-mean map: the ladder has work to do
    am.encoder.ladder_on_device = raw.ladder_on_device = True
    try:
        for _ in range(2):      # (the second call of the ViT-S base network replays its own graph: device mode follows the replay)
            got = amodal_depth_pipeline(raw, am, rgb, mask)
            for a, b in zip(got, want):
                assert torch.equal(a, b)
        assert int(eng.device_ladder_report()["rungs"][0]) >= 2 and raw._engine().device_ladder_report() is not None
    finally:
        am.encoder.ladder_on_device = False
