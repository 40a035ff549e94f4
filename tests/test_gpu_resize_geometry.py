"""Geometry sweeps of the resize kernels ("Geometry sweeps"): every (n_in, n_out) of tests/_resize_ref.py's pair sets along one axis, the other
axis fixed at the smallest size that still selects the kernel, once along y and once along x, every output element compared with the restated sampling
rule.  What is checked is WHICH taps a kernel reads and with which weights: the host sizes the staged source patch from fp32 expressions the device
re-evaluates, and an off-by-one between the two does not fault -- it returns a neighbour's value for a few pixels.

Inputs are small integers, so a wrong tap moves an output by O(1) while the bounds below are O(1e-6).  All bounds are derived, none measured: an fp32
kernel may differ from the float64 blend of the same fp32 weights by (n + 1) 2^-24 mag, n the roundings on the longest path from an input to the output
(counted at each test), mag the same expression on absolute values.

One test is a few hundred to 1260 small launches; on an MI355X each takes 0.04 - 1.4 s (the slowest: tiled up-y 1.4, tiled up-x 1.1, tap-sum 128 channels 1.2,
tail up 0.9), the 35 tests together about 16 s.  A test prints how many pairs it ran and how many the library refused."""
import time

import numpy as np
import pytest
import torch

import _resize_ref as R
from test_gpu_kernels import _pack3

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -7.0
U24 = 2.0 ** -24


def _op_unit(op):
    """Half an ulp, relative, of the operand type."""
    return 2.0 ** -11 if op == torch.float16 else 2.0 ** -8


def _shape(pair, axis, fixed_y, fixed_x):
    (hi, ho), (wi, wo) = (pair, fixed_x) if axis == "y" else (fixed_y, pair)
    return hi, wi, ho, wo


def _ints(shape, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float32)


def _taps_at(shape, y, x):
    hi, wi, ho, wo = shape
    (y0, y1, wy0, wy1), (x0, x1, wx0, wx1) = R.taps(hi, ho), R.taps(wi, wo)
    return (f"rows {int(y0[y])}, {int(y1[y])} with weights {float(wy0[y])!r}, {float(wy1[y])!r}; "
            f"columns {int(x0[x])}, {int(x1[x])} with weights {float(wx0[x])!r}, {float(wx1[x])!r}")


def _check(kernel, axis, pair, shape, got, ref, lim):
    """got, ref, lim: [B, ho, wo, ...] numpy arrays or device tensors.  NaN counts as a miss."""
    bad = ~(abs(got - ref) <= lim)
    if not bool(bad.any()):
        return
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t      # noqa: E731
    bad, got, ref, lim = to_np(bad), to_np(got), to_np(ref), to_np(lim)
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    hi, wi, ho, wo = shape
    raise AssertionError(f"{kernel}, sweep along {axis}, pair {pair[0]} -> {pair[1]} ({hi} x {wi} -> {ho} x {wo}): {int(bad.sum())} of {bad.size} outputs beyond the bound; "
                         f"first at (b, y, x, ...) = {at}: got {float(got[at])!r}, want {float(ref[at])!r} (bound {float(np.broadcast_to(lim, bad.shape)[at]):.3e}); "
                         f"the restatement expects {_taps_at(shape, at[1], at[2])}")


def _report(what, t0, ran, refused=0, why=""):
    print(f"{what}: {ran} pairs ran, {refused} refused{(' (' + why + ')') if refused else ''}, {time.time() - t0:.1f} s")


# =====================================================================================================================
# ada_bilinear_fwd, per-pixel kernel
# =====================================================================================================================
# roundings from an input to the output of  ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d):  product, sum, product, sum (a contraction only removes one)
N_BILINEAR = 4


@pytest.mark.parametrize("axis", ["y", "x"])
@pytest.mark.parametrize("pairs", ["model", "up", "down"])
def test_bilinear_per_pixel_sweep(hip, pairs, axis):
    """C = 4 never takes the LDS-tiled path.  fp32 output with ld = C + 4 and one spare row: the guard columns and the guard row come back untouched."""
    B, C = 2, 4
    ld, t0 = C + 4, time.time()
    for k, pair in enumerate(R.PAIR_SETS[pairs]):
        shape = hi, wi, ho, wo = _shape(pair, axis, (2, 3), (2, 3))
        assert not R.bilinear_is_tiled(C, B, hi, wi, ho, wo)
        x = _ints((B, hi, wi, C), -8, 8, 1000 + k)
        out = torch.full((B * ho * wo + 1, ld), GUARD, device=DEV)
        hip.bilinear(torch.from_numpy(x).reshape(-1, C).to(DEV), C, B, hi, wi, ho, wo, C, out_f32=out, ld_f32=ld)
        o = out.cpu().numpy()
        assert (o[:-1, C:] == GUARD).all() and (o[-1] == GUARD).all(), f"per-pixel bilinear, {axis}, {pair}: guard values behind C / behind the last row overwritten"
        _check("ada_bilinear_fwd (per-pixel)", axis, pair, shape, o[:-1, :C].reshape(B, ho, wo, C).astype(np.float64), R.bilinear(x, ho, wo),
               (N_BILINEAR + 1) * U24 * R.bilinear_mag(x, ho, wo))
    _report(f"per-pixel bilinear, {pairs} along {axis}", t0, len(R.PAIR_SETS[pairs]))


# =====================================================================================================================
# ada_bilinear_fwd, LDS-tiled kernel
# =====================================================================================================================
def _dev_taps(t):
    i0, i1, w0, w1 = t
    return (torch.from_numpy(i0).to(DEV), torch.from_numpy(i1).to(DEV), torch.from_numpy(w0.astype(np.float64)).to(DEV), torch.from_numpy(w1.astype(np.float64)).to(DEV))


def _blend_dev(x64, ty, tx):
    """R.bilinear's expression, operation for operation, in float64 on the device: the tiled sweeps compare up to 2 M elements per pair (asserted equal,
    bit for bit, to R.bilinear on the small pairs of every sweep)."""
    y0, y1, wy0, wy1 = _dev_taps(ty)
    x0, x1, wx0, wx1 = _dev_taps(tx)
    wy0, wy1 = wy0[None, :, None, None], wy1[None, :, None, None]
    wx0, wx1 = wx0[None, None, :, None], wx1[None, None, :, None]
    top, bot = x64[:, y0], x64[:, y1]
    return wy0 * (wx0 * top[:, :, x0] + wx1 * top[:, :, x1]) + wy1 * (wx0 * bot[:, :, x0] + wx1 * bot[:, :, x1])


def _tiled_pairs(pairs, axis):
    return [p for p in R.PAIR_SETS[pairs] if p[1] >= (R.BT_TH if axis == "y" else R.BT_TW)]


def _tiled_case(hip, axis, pair, C, k, forms):
    B = 1
    shape = hi, wi, ho, wo = _shape(pair, axis, (4, 8), (8, 16))
    # the dispatch predicate of ada_bilinear_fwd, restated: a silent fall-back to the per-pixel kernel must not pass for coverage
    assert R.bilinear_is_tiled(C, B, hi, wi, ho, wo), f"{pair} along {axis} with {C} channels would not take the LDS-tiled kernel"
    g = torch.Generator(device=DEV).manual_seed(2000 + k)
    x = torch.randint(-8, 9, (B, hi, wi, C), device=DEV, generator=g).float()
    ty, tx = R.taps(hi, ho), R.taps(wi, wo)
    ref, mag = _blend_dev(x.double(), ty, tx), _blend_dev(x.double().abs(), ty, tx)
    if ho * wo <= 1024:
        assert np.array_equal(ref.cpu().numpy(), R.bilinear(x.cpu().numpy(), ho, wo)), "the device blend is not the restatement's"
    kernel = f"ada_bilinear_fwd (LDS-tiled, {C} channels)"
    out = torch.full((B * ho * wo, C), GUARD, device=DEV)
    if not forms:
        hip.bilinear(x.reshape(-1, C), C, B, hi, wi, ho, wo, C, out_f32=out, ld_f32=C)
        _check(kernel, axis, pair, shape, out.view(B, ho, wo, C).double(), ref, (N_BILINEAR + 1) * U24 * mag)
        return
    # + add (one more rounding), fp32 copy, and the ReLU'd [hi | lo] operand copy inside a zero-bordered grid
    op, u = hip.operand_dtype(), _op_unit(hip.operand_dtype())
    add = torch.randint(-8, 9, (B * ho * wo, C), device=DEV, generator=g).float()
    oo = torch.zeros(B, ho + 2, wo + 2, 2 * C, dtype=op, device=DEV)
    hip.bilinear(x.reshape(-1, C), C, B, hi, wi, ho, wo, C, add=add, ld_add=C, out_f32=out, ld_f32=C, out_op=oo, ld_op=2 * C, map_op=hip.MAP_PAD, relu=True, split_seg=C)
    v = ref + add.view(B, ho, wo, C).double()
    lim = (N_BILINEAR + 2) * U24 * (mag + add.view(B, ho, wo, C).double().abs())
    _check(kernel + ", fp32 copy with add", axis, pair, shape, out.view(B, ho, wo, C).double(), v, lim)
    # hi = rne(relu(v32)), lo = rne(relu(v32) - hi):  |hi - relu(v)| <= lim + u (|v| + lim) + sub;  |hi + lo - relu(v)| <= lim + u^2 (|v| + lim) + sub, with
    # sub = 2^-25, half the spacing of fp16's subnormals (below 2^-14 a rounding is absolute, not relative; bf16 has fp32's exponent range)
    sub = 2.0 ** -25 if op == torch.float16 else 0.0
    vr = v.clamp_min(0)
    inner = oo[:, 1:-1, 1:-1].double()
    _check(kernel + ", operand copy hi", axis, pair, shape, inner[..., :C], vr, lim + u * (vr + lim) + sub)
    _check(kernel + ", operand copy hi + lo", axis, pair, shape, inner[..., :C] + inner[..., C:], vr, lim + u * u * (vr + lim) + sub)
    border = oo.clone()
    border[:, 1:-1, 1:-1] = 0
    assert float(border.float().abs().max()) == 0.0, f"{kernel}, {axis}, {pair}: border of the padded grid written"


@pytest.mark.parametrize("axis,pairs,C,forms", [("y", "model", 128, False), ("y", "up", 128, False), ("x", "model", 128, False), ("x", "up", 128, False),
                                                ("x", "model", 256, False), ("x", "model", 128, True)])
def test_bilinear_tiled_sweep(hip, axis, pairs, C, forms):
    """y: wi = 8 -> wo = 16 fixed; x: hi = 4 -> ho = 8 fixed (one tile the other way).  Pairs below one tile (n_out < 8 rows / 16 columns) belong to the
    per-pixel kernel and are walked there."""
    t0 = time.time()
    cases = _tiled_pairs(pairs, axis)
    for k, pair in enumerate(cases):
        _tiled_case(hip, axis, pair, C, k, forms)
    torch.cuda.synchronize()
    _report(f"LDS-tiled bilinear, {C} channels{' with add / ReLU / [hi | lo] padded' if forms else ''}, {pairs} along {axis}", t0, len(cases))


def test_bilinear_tiled_weights_come_from_the_rounded_coordinate(hip):
    """Regression, found by the sweeps above on every pair with a source of more than a few pixels: the tiled kernel's fy - y0 was contracted with
    fy = sy * y into fma(sy, y, -y0), so its weights came from the UNROUNDED coordinate while the per-pixel kernel, ATen and the host's patch arithmetic
    use the rounded one.  The first half needs no kernel: at 296 -> 592 the contracted weights miss the bound, i.e. the sweep does see such a kernel."""
    pair, axis = (296, 592), "x"
    hi, wi, ho, wo = _shape(pair, axis, (4, 8), (8, 16))
    x = _ints((1, hi, wi, 128), -8, 8, 77)
    x64 = x.astype(np.float64)
    y0, y1, wy0, wy1 = R.taps(hi, ho)
    i0, i1, _, _ = R.taps(wi, wo)
    lx1 = (np.float64(R.scale(wi, wo)) * np.arange(wo) - i0).astype(np.float32)            # product and difference exact in float64, rounded once: the fma
    lx0 = np.float32(1.0) - lx1
    rows = wy0.astype(np.float64)[None, :, None, None] * x64[:, y0] + wy1.astype(np.float64)[None, :, None, None] * x64[:, y1]
    contracted = lx0.astype(np.float64)[None, None, :, None] * rows[:, :, i0] + lx1.astype(np.float64)[None, None, :, None] * rows[:, :, i1]
    lim = (N_BILINEAR + 1) * U24 * R.bilinear_mag(x, ho, wo)
    worst = float((np.abs(contracted - R.bilinear(x, ho, wo)) / np.maximum(lim, 1e-30)).max())
    assert worst > 10.0, f"contracted weights stay within {worst:.1f} bounds at {pair}: the sweep could not tell them apart"
    _tiled_case(hip, axis, pair, 128, 77, False)
    _tiled_case(hip, "y", pair, 128, 78, False)


# =====================================================================================================================
# ada_tapsum_resize_fwd
# =====================================================================================================================
# roundings from a tap-map value to the output: the corner weight ly * lx (1), its product with the value (1), the four-corner sum (3), the nine taps
# accumulated (9), the bias (1).  Integer tap maps are exact in the operand type: the same bound holds for operand-typed maps.
N_TAPSUM = 15
TS_CIN = 4


def _tapsum_pairs(C, pairs, axis):
    if C == 64:
        return list(R.PAIR_SETS[pairs])
    tile = R.TS_TH if axis == "y" else R.TS_TW
    return [p for p in R.PAIR_SETS[pairs] if p[1] % tile != 0]


def _conv3(p, w):
    """p [ho + 2, wo + 2, Cin] zero-padded, w [Co, Cin, 3, 3] -> [ho, wo, Co] in float64."""
    ho, wo = p.shape[0] - 2, p.shape[1] - 2
    out = np.zeros((ho, wo, w.shape[0]))
    for dy in range(3):
        for dx in range(3):
            out += p[dy:dy + ho, dx:dx + wo] @ w[:, :, dy, dx].T
    return out


@pytest.mark.parametrize("C,pairs,axis", [(64, "model", "y"), (64, "model", "x"), (64, "up", "y"), (64, "up", "x"),
                                          (32, "model", "y"), (32, "model", "x"), (128, "model", "y"), (128, "model", "x")])
def test_tapsum_resize_sweep(hip, C, pairs, axis):
    """Integer tap maps T[:, t C + co] = W_t u built on the host (as tests/_exact.py tapsum_family does), fp32 and operand-typed, against
    conv3x3(bilinear(u)) in float64 with the restated weights; mag is that expression on |W| and |u|.  The other axis is 2 -> 4.  32 and 128 channels
    walk the model pairs whose n_out is no multiple of the tile (8 rows / 16 columns): the masked edge, the case that once went wrong."""
    op, t0 = hip.operand_dtype(), time.time()
    w1 = _ints((C, TS_CIN, 3, 3), -1, 1, 72).astype(np.float64)
    b1 = _ints((C,), -4096, 4096, 73) / np.float32(64.0)
    wt = w1.transpose(2, 3, 0, 1).reshape(9 * C, TS_CIN)          # row t C + co, t = dy * 3 + dx
    bias = torch.from_numpy(b1).to(DEV)
    cases = _tapsum_pairs(C, pairs, axis)
    for k, pair in enumerate(cases):
        shape = hi, wi, ho, wo = _shape(pair, axis, (2, 4), (2, 4))
        u = _ints((1, hi, wi, TS_CIN), -2, 2, 3000 + k)
        T = (u.reshape(-1, TS_CIN).astype(np.float64) @ wt.T).astype(np.float32)
        assert np.abs(T).max() <= 256                                # integers: exact in fp16 and in bf16
        ref = _conv3(np.pad(R.bilinear(u, ho, wo)[0], ((1, 1), (1, 1), (0, 0))), w1) + b1.astype(np.float64)
        mag = _conv3(np.pad(R.bilinear_mag(u, ho, wo)[0], ((1, 1), (1, 1), (0, 0))), np.abs(w1)) + np.abs(b1.astype(np.float64))
        Tdev = torch.from_numpy(T).to(DEV)
        for tmap in (torch.float32, op):
            out = torch.full((ho * wo, C), float("nan"), device=DEV)
            hip.tapsum_resize(Tdev.to(tmap), 9 * C, 1, hi, wi, ho, wo, C, bias, out, C)
            _check(f"ada_tapsum_resize_fwd ({C} channels, {tmap} tap maps)", axis, pair, shape, out.cpu().numpy().astype(np.float64).reshape(1, ho, wo, C), ref[None],
                   (N_TAPSUM + 1) * U24 * mag[None])
    _report(f"tap-sum resize, {C} channels, {pairs} along {axis}, fp32 and operand-typed maps", t0, len(cases))


# =====================================================================================================================
# ada_dpt_tail_fwd
# =====================================================================================================================
TAIL_REASON = "needs ho >= 1.5 hi"


def _tail_channels(cp):
    """A few channels spread over the staging lanes of a 64-channel unit (first, middle, last), and both units of cp = 128."""
    return (0, 17, 63) + ((64, 127) if cp == 128 else ())


@pytest.mark.parametrize("cp,pairs,axis", [(64, "model", "y"), (64, "model", "x"), (64, "up", "y"), (64, "up", "x"),
                                           (128, "model", "y"), (128, "model", "x"), (128, "up", "y"), (128, "up", "x")])
def test_dpt_tail_sweep(hip, cp, pairs, axis):
    """8 p -> 14 p for p = 1 .. 74 ("model") and the pairs of UP_PAIRS the kernel's vertical rule accepts; y with wi = 4 -> wo = 7, x with hi = 4 -> ho = 7.
    Along y every pair of UP_PAIRS goes to the library: it must refuse exactly those the restated rule refuses, as ADA_EUNSUPPORTED naming the rule.

    Integers in [-4, 4] on the channels of _tail_channels, zero elsewhere; dyadic weights, bias and tail_w (tests/_exact.py dpt_tail_family's ranges); act none.
    Bound:  (n + 1) 2^-24 mag + u sum_n |tail_w[n]| sum |w| |up|,  u = half an operand ulp (the interpolated halo is staged in the operand type; the exact
    |up| -- not its magnitude -- because the term bounds one rounding of the value itself), and n = 4 (interpolation) + 9 nch - 1 (the non-zero products of
    the convolution, which are exact; zeros add exactly) + 1 (bias) + 2 (tail_w, the sum of the two column halves) + 4 (row reduction) + 1 (tail_b)."""
    op, t0 = hip.operand_dtype(), time.time()
    u_op = _op_unit(op)
    ch = list(_tail_channels(cp))
    n = 4 + 9 * len(ch) - 1 + 1 + 2 + 4 + 1
    w = _ints((32, cp, 3, 3), -16, 16, 82) / np.float32(32.0)
    b = (_ints((32,), -256, 256, 83) / np.float32(32.0)).astype(np.float64)
    tw = (_ints((32,), -4, 4, 84) / np.float32(4.0)).astype(np.float64)
    tb = 0.25
    ws = w[:, ch].astype(np.float64)
    wp = _pack3(torch.from_numpy(w), cp, op).to(DEV)
    bdev, twdev = torch.from_numpy(b.astype(np.float32)).to(DEV), torch.from_numpy(tw.astype(np.float32)).to(DEV)
    cases = list(R.TAIL_MODEL_PAIRS) if pairs == "model" else list(R.UP_PAIRS)
    ran = refused = 0
    for k, pair in enumerate(cases):
        accepted = R.tail_accepts(*pair)
        assert accepted or 2 * pair[1] < 3 * pair[0], f"{pair}: an up-sampling by >= 1.5 that the restated rule refuses"
        if axis == "x" and not accepted:
            continue                                                  # the pair set is the one the rule accepts; the rule itself is vertical
        shape = hi, wi, ho, wo = _shape(pair, axis, (4, 7), (4, 7))
        xs = _ints((1, hi, wi, len(ch)), -4, 4, 4000 + k)
        x = np.zeros((hi * wi, cp), dtype=np.float32)
        x[:, ch] = xs.reshape(-1, len(ch))
        out = torch.full((1, ho, wo), float("nan"), device=DEV)
        try:
            hip.dpt_tail(torch.from_numpy(x).to(DEV), cp, 1, hi, wi, ho, wo, cp, wp, bdev, twdev, tb, hip.ACT_NONE, out)
        except hip.HipExtError as e:
            assert not accepted, f"{pair}: refused though the restated rule accepts it: {e}"
            assert "rc=-2" in str(e) and TAIL_REASON in str(e), f"{pair}: refused, but not as ADA_EUNSUPPORTED naming the vertical rule: {e}"
            refused += 1
            continue
        assert accepted, f"{pair}: ran though the restated vertical rule refuses it"
        pad = ((1, 1), (1, 1), (0, 0))
        up = R.bilinear(xs, ho, wo)[0]
        v = _conv3(np.pad(up, pad), ws) + b
        vm = _conv3(np.pad(R.bilinear_mag(xs, ho, wo)[0], pad), np.abs(ws))
        vu = _conv3(np.pad(np.abs(up), pad), np.abs(ws))
        ref = np.maximum(v, 0.0) @ tw + tb
        lim = (n + 1) * U24 * ((vm + np.abs(b)) @ np.abs(tw) + abs(tb)) + u_op * (vu @ np.abs(tw))
        _check(f"ada_dpt_tail_fwd (cp = {cp})", axis, pair, shape, out.cpu().numpy().astype(np.float64), ref[None], lim[None])
        ran += 1
    _report(f"fused tail, cp = {cp}, {pairs} along {axis}", t0, ran, refused, "ADA_EUNSUPPORTED: " + TAIL_REASON)
    assert ran > 0 and (refused > 0) == (pairs == "up" and axis == "y")


# =====================================================================================================================
# ada_pos_embed_resize
# =====================================================================================================================
@pytest.mark.parametrize("grids", sorted(R.POS_GRIDS))
@pytest.mark.parametrize("sq", R.POS_SQ)
def test_pos_embed_resize_sweep(hip, sq, grids):
    """dim = 4, the scales the model passes, against bicubic_pos at the tolerance of test_pos_embed_bicubic_resize_matches_aten; row 0 bit for bit."""
    t0, dim = time.time(), 4
    pos = torch.randn(1 + sq * sq, dim, generator=torch.Generator().manual_seed(601))
    pdev = pos.to(DEV)
    for ph, pw in R.POS_GRIDS[grids]:
        sh, sw = (ph + 0.1) / sq, (pw + 0.1) / sq
        out = torch.full((1 + ph * pw, dim), float("nan"), device=DEV)
        hip.pos_embed_resize(pdev, sq, dim, ph, pw, sh, sw, out)
        got = out.cpu().numpy()
        ref = R.bicubic_pos(pos.numpy(), sq, ph, pw, sh, sw)
        assert np.array_equal(got[0].view(np.int32), pos[0].numpy().view(np.int32)), f"ada_pos_embed_resize, sq {sq}, grid {ph} x {pw}: row 0 is not a copy"
        bad = ~(np.abs(got - ref) <= 3e-6 + 1e-5 * np.abs(ref))
        if bad.any():
            tok, c = (int(v) for v in np.argwhere(bad)[0])
            oy, ox = (tok - 1) // pw, (tok - 1) % pw
            iy, cy = R._cubic_axis(sq, ph, sh)
            ix, cx = R._cubic_axis(sq, pw, sw)
            raise AssertionError(f"ada_pos_embed_resize, sq {sq}, grid {ph} x {pw}: {int(bad.sum())} of {bad.size} beyond 3e-6 + 1e-5 |ref|, worst {np.nanmax(np.abs(got - ref)):.3e}; first at "
                                 f"token {tok} (y {oy}, x {ox}) channel {c}: got {got[tok, c]!r}, want {ref[tok, c]!r}; the restatement expects rows {iy[oy].tolist()} x "
                                 f"{cy[oy].tolist()}, columns {ix[ox].tolist()} x {cx[ox].tolist()}")
    _report(f"position table, sq {sq}, {grids}", t0, len(R.POS_GRIDS[grids]))
