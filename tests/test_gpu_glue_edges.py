"""GPU: the glue kernels of csrc/ada_pipeline.hip -- minmax, normalize, blend / blend_aligned, tile_blend -- at their edges, against the plain
restatements of tests/_glue_ref.py (whose premises tests/test_glue_ref_cpu.py checks without a GPU): bit for bit where the arithmetic allows it,
within bounds counted from the roundings elsewhere ("Glue and evaluation value domain")."""
import pytest
import torch

import _glue_ref as G
from _exact import assert_bits, assert_exact_budget

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------------------------
# minmax: one workgroup of 16 waves per image, lane l of wave w reads the indices 64 w + l + 1024 pass
# ---------------------------------------------------------------------------------------------------------------------------------
MINMAX_N = [1, 63, 64, 1023, 1024, 1025, 4097]


def _minmax(hip, x):
    out = torch.full((x.shape[0], 2), 123.0, device=DEV)
    hip.minmax(x.to(DEV), out)
    return out.cpu()


def _placements(n):
    """Index 0, index n - 1, and lane 17 of each of the 16 waves in each pass over the image."""
    return sorted({0, n - 1} | {i for i in (64 * w + 17 + 1024 * p for p in range((n + 1023) // 1024) for w in range(16)) if i < n})


@pytest.mark.parametrize("n", MINMAX_N)
def test_minmax_unique_extremes_at_every_wave_and_pass(hip, n):
    """Every image of the batch carries its unique minimum at one swept index and its unique maximum at another: one launch per n."""
    places = _placements(n)
    B = len(places)
    x = torch.rand(B, n, generator=torch.Generator().manual_seed(n)) * 2 - 1
    for b, i in enumerate(places):
        x[b, i] = -5.0 - b
        if n > 1:
            x[b, places[(b + 1) % B]] = 7.0 + b
    want = G.minmax_ref(x)
    if n > 1:
        assert torch.equal(want[:, 0], -5.0 - torch.arange(B)) and torch.equal(want[:, 1], 7.0 + torch.arange(B))
    assert torch.equal(_minmax(hip, x), want)


@pytest.mark.parametrize("n", MINMAX_N)
def test_minmax_infinities_and_nan(hip, n):
    g = torch.Generator().manual_seed(100 + n)
    # +-inf: as values among finite ones, and as every value of an image (the minimum of an all-inf image is inf)
    x = torch.randn(3, n, generator=g)
    x[0, n // 2] = INF
    x[1, n - 1] = -INF
    x[2] = INF
    want = G.minmax_ref(x)
    assert want[2].tolist() == [INF, INF] and want[0, 1] == INF and want[1, 0] == -INF
    assert torch.equal(_minmax(hip, x), want)
    # one NaN inside an otherwise finite image: (NaN, NaN) for that image only -- at the first, a middle and the last index
    for i in sorted({0, n // 2, n - 1}):
        x = torch.randn(3, n, generator=g)
        x[1, i] = NAN
        got, want = _minmax(hip, x), G.minmax_ref(x)
        assert torch.isnan(want[1]).all() and torch.isfinite(want[[0, 2]]).all()
        G.assert_same(got, want, f"minmax n={n}, NaN at {i}")
    x = torch.randn(3, n, generator=g)
    x[0] = NAN
    x[2, 0] = -INF
    x[2, n - 1] = NAN          # a NaN beside an infinity is still the result
    G.assert_same(_minmax(hip, x), G.minmax_ref(x), f"minmax n={n}, all-NaN image")


# ---------------------------------------------------------------------------------------------------------------------------------
# normalize: 256 pixels per workgroup
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", ["norm", "obs", "both"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70 * 70])
def test_normalize_bit_for_bit(hip, n, outputs):
    """(d - lo) / (hi - lo) and v * 2 - 1 are correctly rounded operations (the doubling exact): bit for bit.  Image 0 Gaussian, image 1 constant (0 / 0 =
    NaN everywhere, as is every one-pixel image), then the same maps with a NaN min / max pair."""
    d = torch.randn(2, n, generator=torch.Generator().manual_seed(n)) * 3
    d[1] = 0.625
    for own, mm in ((True, G.minmax_ref(d)), (False, torch.tensor([[NAN, NAN], [0.0, 1.0]]))):
        want_norm, want_obs = G.normalize_ref(d, mm)
        assert bool(torch.isnan(want_norm[1 if own else 0]).all()) and (own or torch.equal(want_norm[1], d[1]))
        norm = torch.full((2, n), 9.0, device=DEV) if outputs != "obs" else None
        obs = torch.full((2, 1, n), 9.0, device=DEV) if outputs != "norm" else None
        hip.normalize(d.to(DEV), mm.to(DEV), norm=norm, obs=obs)
        if norm is not None:
            G.assert_same(norm, want_norm, f"norm n={n}")
        if obs is not None:
            G.assert_same(obs[:, 0], want_obs, f"obs n={n}")
    if n > 1:
        assert bool(torch.isfinite(G.normalize_ref(d, G.minmax_ref(d))[0][0]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# blend / blend_ex: 256 columns per workgroup, one image of the batch per mask family
# ---------------------------------------------------------------------------------------------------------------------------------
def _blend(hip, amodal, base, masks, ss, ex):
    out = torch.full(tuple(amodal.shape), NAN, device=DEV)
    if ex:
        hip.blend_ex(amodal.to(DEV), base.to(DEV), masks.to(DEV), out, scale_shift=None if ss is None else ss.to(DEV))
    else:
        hip.blend(amodal.to(DEV), base.to(DEV), masks.to(DEV), out)
    return out.cpu()


@pytest.mark.parametrize("pair", G.BLEND_SCALE_SHIFTS)
@pytest.mark.parametrize("shape", G.BLEND_SHAPES)
def test_blend_exact_family_bit_for_bit(hip, shape, pair):
    H, W = shape
    names, amodal, base, masks = G.blend_case(H, W, exact=True)
    ss = G.scale_shift_tensor(pair, len(names))
    want, border, blended = G.blend_parts(amodal, base, masks, ss)
    assert_exact_budget(unit=2.0 ** -14, mag=G.blur_mag(blended), ref=blended.double(), what=f"blend {shape} {pair}")
    got = _blend(hip, amodal, base, masks, ss, ex=True)
    for b, name in enumerate(names):
        assert_bits(got[b], want[b], f"blend_ex {shape} {pair} mask {name}")
    if pair is None:
        plain = _blend(hip, amodal, base, masks, None, ex=False)
        assert_bits(plain, got, f"blend against blend_ex(scale_shift=None) {shape}")
        assert_bits(plain[names.index("empty")], base[names.index("empty")], "empty mask")


@pytest.mark.parametrize("pair", G.BLEND_SCALE_SHIFTS)
@pytest.mark.parametrize("shape", G.BLEND_SHAPES)
def test_blend_gaussian_within_counted_roundings(hip, shape, pair):
    """Blurred pixels: eight fp32 additions whose partial sums are at most k max|blended| (2 + ... + 9 = 44 half-ulps of max|blended|, 4.9 after the
    division by 9), one quotient, and the restatement's own two roundings -- under 10 * 2^-24 * max|blended|, the issue's bound.  Every other pixel is
    a copy (with scale_shift: the restatement's product and sum, rounded separately): bit for bit."""
    H, W = shape
    names, amodal, base, masks = G.blend_case(H, W, exact=False)
    ss = G.scale_shift_tensor(pair, len(names))
    want, border, blended = G.blend_parts(amodal, base, masks, ss)
    got = _blend(hip, amodal, base, masks, ss, ex=True)
    worst = 0.0
    for b, name in enumerate(names):
        bound = 10 * G.U * float(blended[b].abs().max())
        err = (got[b].double() - want[b].double()).abs()
        if bool(border[b].any()):
            worst = max(worst, float(err[border[b]].max()) / bound)
            assert float(err[border[b]].max()) <= bound, (name, float(err[border[b]].max()), bound)
        keep = ~border[b]
        assert_bits(got[b][keep], want[b][keep], f"blend_ex {shape} {pair} mask {name}, pixels off the border")
    print(f"blend {shape} {pair}: worst |got - ref| / bound on blurred pixels = {worst:.3f}")
    if pair is None:
        assert_bits(_blend(hip, amodal, base, masks, None, ex=False), got, f"blend against blend_ex(scale_shift=None) {shape}")


# ---------------------------------------------------------------------------------------------------------------------------------
# tile_blend
# ---------------------------------------------------------------------------------------------------------------------------------
def _tile_blend(hip, tiles, origins, H, W, ramp):
    oy = torch.tensor([o[0] for o in origins], dtype=torch.int32, device=DEV)
    ox = torch.tensor([o[1] for o in origins], dtype=torch.int32, device=DEV)
    out = torch.full((tiles.shape[0], H, W), NAN, device=DEV)          # every pixel must be written
    hip.tile_blend(tiles.to(DEV).contiguous(), oy, ox, H, W, ramp, out)
    return out.cpu()


@pytest.mark.parametrize("geom", G.TILE_GEOMETRIES)
def test_tile_blend_geometries(hip, geom):
    th, tw, H, W, overlap, ramp = geom
    origins = G.tile_geometry_origins(th, tw, H, W, overlap)
    T = len(origins)
    # exact family: bit for bit when the ramp is a power of two (weights, acc and wsum exact: tests/test_glue_ref_cpu.py)
    tiles = G.tile_values(2, T, th, tw, exact=True, seed=5)
    want, cover, _, _ = G.tile_blend_parts(tiles, origins, H, W, ramp)
    got = _tile_blend(hip, tiles, origins, H, W, ramp)
    assert bool(torch.isfinite(got).all()), "a pixel was not written"
    if ramp & (ramp - 1) == 0:
        assert_bits(got, want, f"tile blend {geom}, exact family")
    # Gaussian values: (2 T + 2) * 2^-24 * max|tile| with T the number of tiles over the pixel (counted in tile_blend_parts' docstring)
    for values in ([tiles] if ramp & (ramp - 1) else []) + [G.tile_values(2, T, th, tw, exact=False, seed=6)]:
        want = G.tile_blend_ref(values, origins, H, W, ramp)
        got = _tile_blend(hip, values, origins, H, W, ramp)
        bound = (2 * cover + 2).double() * G.U * float(values.abs().max())
        ratio = ((got.double() - want.double()).abs() / bound).max()
        print(f"tile blend {geom}: up to {int(cover.max())} tiles per pixel, worst |got - ref| / bound = {float(ratio):.3f}")
        assert bool(torch.isfinite(got).all()) and float(ratio) <= 1.0
    # a constant field stays constant
    got = _tile_blend(hip, torch.full((1, T, th, tw), 0.37), origins, H, W, ramp)
    assert float((got.double() / float(torch.tensor(0.37)) - 1).abs().max()) <= 2.0 ** -23


def test_tile_blend_two_identical_origins(hip):
    """Two tiles on the same place: equal weights, the mean of the two -- exact on the exact family."""
    tiles = G.tile_values(2, 2, 8, 8, exact=True, seed=8)
    origins = [(0, 0), (0, 0)]
    want, cover, _, _ = G.tile_blend_parts(tiles, origins, 8, 8, 4)
    assert int(cover.min()) == 2 and torch.equal(want.double(), (tiles[:, 0].double() + tiles[:, 1].double()) / 2)
    assert_bits(_tile_blend(hip, tiles, origins, 8, 8, 4), want, "two identical origins")


def test_tile_blend_uncovered_pixel_is_nan(hip):
    """Documented behaviour, not refused by the library (the origins live on the device): a pixel no tile covers is 0 / 0 = NaN, its neighbours are not."""
    tiles = G.tile_values(1, 2, 8, 8, exact=True, seed=6)
    origins = [(0, 0), (8, 12)]
    want, cover, _, _ = G.tile_blend_parts(tiles, origins, 16, 300, 4)
    got = _tile_blend(hip, tiles, origins, 16, 300, 4)
    assert torch.equal(torch.isnan(got[0]), cover == 0) and int((cover > 0).sum()) == 128
    G.assert_same(got, want, "uncovered pixels")
