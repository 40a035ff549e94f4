"""GPU: the guided filter and guided up-sampling (csrc/ada_guided.hip, hip_ext/guided.py) against the fp64 numpy restatement tests/_guided_ref.py.

Tolerance (derived, include/ada_hip.h "Guided filter"): device and restatement both work in fp64 and differ in summation order alone, so their fp32
results agree except at a rounding boundary: |q - q_ref| <= spacing_fp32(max(|q_ref|, max |p|)) at every pixel, none left out; ``covered`` and every
``fill`` pixel are compared exactly, and the apply pass from given coefficients bit for bit.  Map widths: 257 is one more than the row passes' tile
(GUIDED_TILE_W), 1025 guide pixels one more than the apply pass's (GUIDED_TILE_W threads x GUIDED_APPLY_PX)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import _guided_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
U8 = np.uint8


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def hole_box(h, w, r):
    """One hole larger than two windows (side 4 r + 3, clipped by the map; 2 for r = 0): its innermost 3 x 3 pixels (r = 0: all four) get no fit."""
    side = 4 * r + 3 if r else 2
    y0, x0 = max((h - side) // 2, 0), max((w - side) // 2, 0)
    return slice(y0, min(y0 + side, h)), slice(x0, min(x0 + side, w))


@functools.lru_cache(maxsize=None)
def case(shape, C, dtype, kind, r, out_hw=None, seed=0):
    """(p fp32 [B, h, w], valid or None, guide [B, H, W, C]) -- depth-like values in 1 .. 3.5.  kind: 'random'; 'band' (a flat band in the guide);
    'grey' (C = 3 stored as three equal channels); 'step' (p with a step and NaNs); 'hole' (valid with one hole larger than two windows)."""
    B, h, w = shape
    H, W = out_hw or (h, w)
    rng = np.random.default_rng(seed + 7 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    p = (1.5 + yy / max(h, 1) + 0.5 * xx / max(w, 1) + 0.05 * rng.standard_normal((B, h, w))).astype(F)
    YY, XX = np.mgrid[0:H, 0:W]
    g = 0.2 + 0.3 * rng.random((B, H, W, C)) + 0.4 * (XX > 0.45 * W)[None, ..., None]
    if kind == "grey":
        g = np.repeat(g[..., :1], C, axis=-1)
    if kind == "band":
        if H >= 8:
            g[:, H // 3:H // 3 + H // 4] = 0.25
        else:
            g[:, :, W // 2:W // 2 + max(W // 5, 1)] = 0.25
    valid = None
    if kind == "step":
        p = p + (0.75 * (xx > 0.5 * w)).astype(F)
        p[rng.random((B, h, w)) < 0.04] = np.nan
    if kind == "hole":
        valid = np.ones((B, h, w), U8)
        valid[(slice(None),) + hole_box(h, w, r)] = 0
        p[valid == 0] = 1e30                                   # what lies under an invalid sample never reaches a result
    guide = np.round(g * 255).astype(U8) if dtype == "u8" else g.astype(F)
    return p, valid, np.ascontiguousarray(guide)


@functools.lru_cache(maxsize=None)
def reference(shape, C, dtype, kind, r, eps, out_hw=None, fill=None):
    p, valid, guide = case(shape, C, dtype, kind, r, out_hw)
    coeff, covered = R.coefficients(p, guide, r, R.raw_eps(eps, guide), valid)
    return coeff, covered, R.apply(coeff, covered, guide, np.nan if fill is None else fill)


def finite_p(p, valid):
    return p if valid is None else np.where(valid != 0, p, np.nan)


SAME_SIZE = [
    # shape, C, dtype, kind, r, eps
    ((1, 1, 1), 1, "u8", "random", 0, 1e-2), ((1, 1, 1), 3, "f32", "random", 31, 1e-8), ((1, 1, 1), 3, "u8", "step", 4, 1e-4),
    ((1, 3, 70), 3, "u8", "random", 4, 1e-4), ((1, 3, 70), 1, "f32", "hole", 4, 1e-2), ((1, 3, 70), 3, "f32", "band", 31, 1e-6), ((1, 3, 70), 1, "u8", "step", 1, 1e-8),
    ((2, 33, 65), 3, "u8", "random", 1, 1e-2), ((2, 33, 65), 3, "u8", "grey", 4, 1e-6), ((2, 33, 65), 3, "u8", "grey", 4, 1e-8), ((2, 33, 65), 3, "f32", "grey", 1, 1e-8),
    ((2, 33, 65), 1, "u8", "hole", 4, 1e-4), ((2, 33, 65), 3, "f32", "hole", 1, 1e-6), ((2, 33, 65), 3, "f32", "step", 31, 1e-4), ((2, 33, 65), 1, "f32", "band", 0, 1e-2),
    ((2, 33, 65), 3, "u8", "hole", 0, 1e-8),
    ((1, 17, 129), 3, "u8", "band", 4, 1e-8), ((1, 17, 129), 1, "f32", "random", 31, 1e-6), ((1, 17, 129), 3, "f32", "hole", 4, 1e-2), ((1, 17, 129), 1, "u8", "step", 1, 1e-4),
    ((1, 5, 257), 3, "u8", "hole", 31, 1e-4), ((1, 5, 257), 1, "f32", "step", 4, 1e-8), ((1, 5, 257), 3, "f32", "random", 1, 1e-2), ((1, 5, 257), 1, "u8", "band", 31, 1e-6),
]


def test_the_cases_cover_what_they_should():
    for values, col in (({0, 1, 4, 31}, 4), ({1, 3}, 1), ({"u8", "f32"}, 2), ({1e-2, 1e-4, 1e-6, 1e-8}, 5), ({"random", "band", "grey", "step", "hole"}, 3)):
        assert {c[col] for c in SAME_SIZE} == values
    assert {c[0] for c in SAME_SIZE} == {(1, 1, 1), (1, 3, 70), (2, 33, 65), (1, 17, 129), (1, 5, 257)}
    assert {c[5] for c in SAME_SIZE if c[3] == "grey" and c[1] == 3} == {1e-6, 1e-8}
    assert ((1, 3, 70), 4) in {(c[0], c[4]) for c in SAME_SIZE}                    # h < r


@pytest.mark.parametrize("shape,C,dtype,kind,r,eps", SAME_SIZE, ids=lambda v: str(v).replace(" ", ""))
def test_filter_equals_restatement(hip, shape, C, dtype, kind, r, eps):
    from hip_ext import guided as G
    p, valid, guide = case(shape, C, dtype, kind, r)
    _, covered_ref, q_ref = reference(shape, C, dtype, kind, r, eps)
    if kind == "hole":
        share = float((covered_ref == 0).mean())
        assert 0 < share <= 0.15, share
    gd = guide[..., 0] if C == 1 and r % 2 else guide                              # a one-channel guide with or without its last axis
    q, covered = G.guided_upsample(dev(p), dev(gd), r, eps, valid=None if valid is None else dev(valid), return_covered=True)
    assert q.shape == p.shape and covered.dtype == torch.uint8
    assert np.array_equal(host(covered), covered_ref)
    R.assert_close(host(q), q_ref, finite_p(p, valid), f"filter {shape} C={C} {dtype} {kind} r={r} eps={eps}")
    q2 = G.guided_filter(dev(p), dev(gd), r, eps, valid=None if valid is None else dev(valid))
    assert torch.equal(q.view(torch.int32), q2.view(torch.int32))                   # two consecutive calls: the same bits


GEOMETRIES = [
    # map shape, guide size, C, dtype, kind, r, eps
    ((2, 33, 65), (66, 130), 3, "u8", "hole", 4, 1e-4),           # exact 2x
    ((1, 37, 41), (90, 61), 3, "u8", "hole", 2, 1e-6),
    ((1, 37, 41), (90, 61), 1, "f32", "step", 4, 1e-4),
    ((1, 5, 7), (64, 200), 3, "f32", "hole", 0, 1e-2),
    ((1, 5, 7), (64, 200), 1, "u8", "random", 1, 1e-8),
    ((1, 1, 1), (9, 9), 3, "u8", "random", 4, 1e-4),
    ((1, 3, 257), (4, 1025), 3, "u8", "hole", 1, 1e-4),
    ((1, 3, 257), (6, 1028), 1, "f32", "band", 31, 1e-6),
]


@pytest.mark.parametrize("shape,out_hw,C,dtype,kind,r,eps", GEOMETRIES, ids=lambda v: str(v).replace(" ", ""))
def test_upsample_equals_restatement(hip, shape, out_hw, C, dtype, kind, r, eps):
    from hip_ext import guided as G
    p, valid, guide = case(shape, C, dtype, kind, r, out_hw)
    coeff_ref, covered_ref, q_ref = reference(shape, C, dtype, kind, r, eps, out_hw)
    dv = None if valid is None else dev(valid)
    q, covered = G.guided_upsample(dev(p), dev(guide), r, eps, valid=dv, return_covered=True)
    assert tuple(q.shape) == (shape[0],) + out_hw
    assert np.array_equal(host(covered), covered_ref)
    if kind == "hole":
        share = float((covered_ref == 0).mean())
        assert 0 < share <= 0.15 and np.isnan(q_ref).any(), share
    R.assert_close(host(q), q_ref, finite_p(p, valid), f"upsample {shape}->{out_hw} C={C} {dtype} {kind} r={r} eps={eps}")
    # the two halves give the same bits as the whole, and a given fill lands exactly where NaN did
    coeff, cov2 = G.guided_coefficients(dev(p), dev(guide), r, eps, valid=dv)
    assert coeff.dtype == torch.float64 and tuple(coeff.shape) == shape + (C + 1,) and torch.equal(cov2, covered)
    q2 = G.guided_apply(coeff, cov2, dev(guide), fill=-7.0)
    assert np.array_equal(host(q2) == -7.0, np.isnan(q_ref))
    keep = ~np.isnan(q_ref)
    assert np.array_equal(host(q2).view(np.int32)[keep], host(q).view(np.int32)[keep])
    # the apply pass alone, from the restatement's coefficients: bit for bit, renormalised taps and fill included
    q3 = G.guided_apply(dev(coeff_ref), dev(covered_ref), dev(guide))
    assert np.array_equal(np.isnan(host(q3)), ~keep) and np.array_equal(host(q3).view(np.int32)[keep], q_ref.view(np.int32)[keep])


def test_renormalised_taps_occur():
    """The hole cases of GEOMETRIES do exercise the renormalisation: some output has a covered and an uncovered tap of positive weight."""
    shape, out_hw, C, dtype, kind, r, eps = GEOMETRIES[1]
    coeff, covered, q = reference(shape, C, dtype, kind, r, eps, out_hw)
    _, _, guide = case(shape, C, dtype, kind, r, out_hw)
    plain = R.apply(coeff, np.ones_like(covered), guide)
    differ = ~np.isnan(q) & (q != plain)
    assert differ.any() and np.isnan(q).any()


def test_nothing_votes_gives_fill_everywhere(hip):
    from hip_ext import guided as G
    p, _, guide = case((1, 5, 7), 3, "u8", "random", 1, (64, 200))
    q, covered = G.guided_upsample(dev(p), dev(guide), 1, 1e-3, valid=torch.zeros(1, 5, 7, dtype=torch.bool, device="cuda"), fill=2.5, return_covered=True)
    assert not bool(covered.any()) and bool((q == 2.5).all())
    q = G.guided_filter(np.full((1, 1, 1), np.nan, F), np.zeros((1, 1, 1, 1), U8), 0, 1e-3)
    assert bool(torch.isnan(q).all())


def test_input_forms(hip):
    """numpy and device inputs, [h, w] and [1, h, w], and pitched crops give what their contiguous copies give; the caller's tensors are not written."""
    from hip_ext import guided as G
    shape, out_hw, C, dtype, kind, r, eps = GEOMETRIES[1]
    p, valid, guide = case(shape, C, dtype, kind, r, out_hw)
    want = G.guided_upsample(dev(p), dev(guide), r, eps, valid=dev(valid))
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))      # noqa: E731
    assert same(want, G.guided_upsample(p, guide, r, eps, valid=valid))
    assert same(want, G.guided_upsample(dev(p), guide, r, eps, valid=valid != 0))
    one = G.guided_upsample(p[0], guide[0], r, eps, valid=dev(valid[0]).bool())
    assert one.shape == out_hw and same(want[0], one)
    big_p = torch.full((1, 50, 60), 9.0, device="cuda")
    big_v = torch.ones((1, 50, 60), dtype=torch.uint8, device="cuda")
    big_g = torch.full((1, 100, 80, 4), 7, dtype=torch.uint8, device="cuda")
    big_p[:, 3:40, 5:46], big_v[:, 3:40, 5:46], big_g[:, 2:92, 9:70, :3] = dev(p), dev(valid), dev(guide)
    crops = big_p[:, 3:40, 5:46], big_g[:, 2:92, 9:70, :3], big_v[:, 3:40, 5:46]
    assert not any(c.is_contiguous() for c in crops)
    before = [t.clone() for t in (big_p, big_v, big_g)]
    assert same(want, G.guided_upsample(crops[0], crops[1], r, eps, valid=crops[2]))
    assert all(torch.equal(a, b) for a, b in zip(before, (big_p, big_v, big_g)))
    with pytest.raises(hip.HipExtError, match="no CPU fallback|HIP device"):
        G.guided_upsample(torch.from_numpy(p), torch.from_numpy(guide), r, eps)


# ---- the workspace contract, in the manner of test_gpu_workspace_contract.py -------------------------------------------------------------------

GUARD_BYTES = 4096
GUARD, POISON = 0x5A, 0xA5


def guarded(need, fill):
    """``need`` bytes filled with ``fill`` between two bands of guard bytes; check() asserts the bands untouched."""
    buf = torch.full((GUARD_BYTES + need + GUARD_BYTES,), GUARD, dtype=torch.uint8, device="cuda")
    ws = buf[GUARD_BYTES:GUARD_BYTES + need]
    ws.fill_(fill)

    def check(what):
        torch.cuda.synchronize()
        assert bool((buf[:GUARD_BYTES] == GUARD).all()) and bool((buf[GUARD_BYTES + need:] == GUARD).all()), f"{what}: guard bytes around the workspace overwritten"
    return ws, check


def poisoned(shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), POISON, dtype=torch.uint8, device="cuda").view(dtype).view(*shape)


@pytest.mark.parametrize("shape,C,dtype,kind,r,eps", [SAME_SIZE[11], SAME_SIZE[12], SAME_SIZE[20]], ids=lambda v: str(v).replace(" ", ""))
def test_workspace_contract(hip, shape, C, dtype, kind, r, eps):
    """Exactly the bytes asked for, pre-filled with 0x00, with 0xFF and left over from a busier call (every sample voting, other values): the same bytes
    out, guard bands intact, every element of both outputs written, and a workspace one byte short refused before any launch."""
    B, h, w = shape
    p, valid, guide = case(shape, C, dtype, kind, r)
    coeff_ref, covered_ref, q_ref = reference(shape, C, dtype, kind, r, eps)
    dp, dv, dg = dev(p), dev(valid), dev(guide)
    need = hip.guided_workspace_bytes(B, h, w, C)
    assert need == 8 * B * h * w * ((5 if C == 1 else 14) + C + 2)
    e = R.raw_eps(eps, guide)

    def fit(ws, pp=dp, vv=dv):
        coeff, covered = poisoned(shape + (C + 1,), torch.float64), poisoned(shape, torch.uint8)
        hip.guided_coeff_fwd(pp, dg, r, e, coeff, covered, valid=vv, workspace=ws)
        return coeff, covered
    runs = []
    for state in ("0x00", "0xff", "used"):
        ws, check = guarded(need, 0xFF if state == "0xff" else 0x00)
        if state == "used":
            fit(ws, torch.full_like(dp, 1e30), None)
        outs = fit(ws)
        check(f"workspace pre-filled {state}")
        runs.append(outs)
    for outs in runs[1:]:
        for a, b in zip(runs[0], outs):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "the result depends on what the workspace held"
    short, check = guarded(need - 1, 0x00)
    with pytest.raises(hip.HipExtError, match="workspace"):
        fit(short)
    check("the refused call")
    coeff, covered = runs[0]
    assert np.array_equal(host(covered), covered_ref)
    out = poisoned(q_ref.shape, torch.float32)
    hip.guided_apply_fwd(coeff, covered, dg, out)
    R.assert_close(host(out), q_ref, finite_p(p, valid), f"workspace {shape}")
    for bad in (dict(radius=32), dict(radius=-1), dict(eps=0.0), dict(eps=float("inf"))):
        with pytest.raises(hip.HipExtError, match="radius|eps"):
            hip.guided_coeff_fwd(dp, dg, bad.get("radius", r), bad.get("eps", e), coeff, covered, valid=dv)


def test_both_passes_inside_a_stream_capture(hip):
    from hip_ext import guided as G
    shape, out_hw, C, dtype, kind, r, eps = GEOMETRIES[1]
    p, valid, guide = case(shape, C, dtype, kind, r, out_hw)
    other = case(shape, C, dtype, "step", r, out_hw)[0]
    dp, dv, dg = dev(p), dev(valid), dev(guide)
    eager = G.guided_upsample(dp, dg, r, eps, valid=dv)
    run = lambda: G.guided_upsample(dp, dg, r, eps, valid=dv)      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    dp.copy_(dev(other))
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out.view(torch.int32), eager.view(torch.int32))
    dp.copy_(dev(p))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))


# ---- where it is used ------------------------------------------------------------------------------------------------------------------------

RAW_CASE = dict(kind="raw", encoder="vits", features=64, out_channels=[48, 96, 192, 384])
AM_CASE = dict(kind="amodal", encoder="vits", guide_type="mask+observation", loss="entire_target_object")
FIELDS = ("base", "amodal", "blended", "masks", "scale_shift")
S = 70


def test_amodal_infer_image_guided(hip):
    from _cases import build_product_model, synth_state_dict
    from hip_ext.guided import guided_upsample
    from hip_ext.image import resize_nearest
    from hip_ext.pipeline import amodal_infer_image
    raw, am = build_product_model(RAW_CASE), build_product_model(AM_CASE)
    raw.load_state_dict(synth_state_dict(raw), strict=True)
    am.load_state_dict(synth_state_dict(am), strict=True)
    raw, am = raw.cuda(), am.cuda()
    h, w = 96, 128
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.clip(128 + 100 * np.sin(yy[..., None] * 0.07 + xx[..., None] * np.array([0.05, 0.11, 0.02])) + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(U8)
    masks = np.zeros((2, h, w), U8)
    masks[0] = (((yy - 40) / 25.0) ** 2 + ((xx - 70) / 30.0) ** 2 <= 1) * 255
    masks[1, :35, 80:] = 255
    net = amodal_infer_image(raw, am, img, masks, size=S)
    near = amodal_infer_image(raw, am, img, masks, size=S, out_size="image")
    same = amodal_infer_image(raw, am, img, masks, size=S, out_size="image", upsample="nearest")
    for f in FIELDS:
        x, y = getattr(near, f), getattr(same, f)
        assert (x is None) == (y is None) and (x is None or (x.dtype == y.dtype and x.shape == y.shape and host(x).tobytes() == host(y).tobytes())), f
    got = amodal_infer_image(raw, am, img, masks, size=S, out_size=(h, w), upsample="guided", guided_radius=4, guided_eps=1e-2)
    want_base = guided_upsample(net.base, img, 4, 1e-2)
    assert got.base.shape == (h, w) and torch.equal(got.base.view(torch.int32), want_base.view(torch.int32))
    assert not torch.equal(got.base, near.base) and bool(torch.isfinite(got.base).all())
    inside = resize_nearest(net.masks.contiguous(), h, w) > 0
    assert bool(inside.any()) and not bool(inside.all())
    assert torch.equal(got.blended[inside], near.blended[inside])
    assert torch.equal(got.blended[~inside], want_base.expand(2, -1, -1)[~inside])
    for f in ("amodal", "masks"):
        assert torch.equal(getattr(got, f), getattr(net, f)), f
    # without an out_size nothing is resized: the keyword changes nothing
    plain = amodal_infer_image(raw, am, img, masks, size=S, upsample="guided")
    assert torch.equal(plain.base, net.base) and torch.equal(plain.blended, net.blended)


def test_depth_to_mesh_guided_writes_the_photos_vertex_count(hip, tmp_path):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amodal-depth-anything_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from PIL import Image
    from src.scripts import depth_to_mesh as M
    p, _, guide = case((1, 20, 24), 3, "u8", "random", 2, (40, 48))
    depth, photo, same_photo, ply = (str(tmp_path / n) for n in ("d.npy", "p.png", "s.png", "o.ply"))
    np.save(depth, p[0])
    Image.fromarray(guide[0]).save(photo)
    Image.fromarray(guide[0, ::2, ::2].copy()).save(same_photo)
    assert M.main([depth, ply, "--image", photo, "--guided", "2", "1e-3"]) == 0
    header = open(ply, "rb").read(400).decode("ascii", "replace")
    assert "element vertex 1920" in header, header
    mesh = M.mesh_file(depth, ply, image=same_photo, guided=(2, 1e-3))
    assert mesh.vertex_count == 480
    with pytest.raises(ValueError, match="photo of shape"):
        M.mesh_file(depth, ply, image=photo)
