"""Plain restatements of the glue kernels (csrc/ada_pipeline.hip) and of the evaluation sums (csrc/ada_eval.hip) in numpy and torch on the CPU, with
the input families that tests/test_glue_ref_cpu.py (premises, no GPU) and tests/test_gpu_glue_edges.py / tests/test_gpu_eval_values.py (the kernels)
share ("Glue and evaluation value domain").

Nothing here is derived from the kernels: every function restates the reference's rule (infer.py:22,30-44,92; src/util/metric.py:37-161) or, for the
tile blend, the formula of the kernel's header comment, with the roundings written out so that the tests can count them."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # half an fp32 ulp, relative: the error of one correctly rounded fp32 operation


# ---------------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------------
def assert_same(got, want, what=""):
    """NaN in the same places, and the same fp32 bits everywhere else (the sign of a zero and the payload of a NaN aside)."""
    from _exact import assert_bits
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} against {tuple(want.shape)}"
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN at {int(gn.sum())} places, the reference has {int(wn.sum())} ({int((gn != wn).sum())} differ)"
    z = torch.zeros((), dtype=got.dtype)
    assert_bits(torch.where(gn, z, got), torch.where(wn, z, want), what)


# ---------------------------------------------------------------------------------------------------------------------------------
# min / max and normalisation (reference infer.py:22, 92)
# ---------------------------------------------------------------------------------------------------------------------------------
def minmax_ref(x):
    """[B, ...] fp32 -> [B, 2] = (amin, amax) per image; torch's reductions propagate NaN as depth_raw.min() / .max() do."""
    f = x.reshape(x.shape[0], -1)
    return torch.stack([torch.amin(f, dim=1), torch.amax(f, dim=1)], dim=1)


def normalize_ref(d, minmax):
    """(norm, obs): fp32 (d - lo) / (hi - lo), then norm * 2 - 1, each a separate correctly rounded fp32 operation (the doubling is exact, so a
    fused multiply-add gives the same bits).  A constant image is 0 / 0 = NaN."""
    B = d.shape[0]
    shape = (B,) + (1,) * (d.dim() - 1)
    lo, hi = minmax[:, 0].reshape(shape), minmax[:, 1].reshape(shape)
    num = d - lo
    den = hi - lo
    norm = num / den
    dbl = norm * 2
    return norm, dbl - 1


# ---------------------------------------------------------------------------------------------------------------------------------
# paste + border blur (reference infer.py:30-44)
# ---------------------------------------------------------------------------------------------------------------------------------
def blend_parts(amodal, base, mask, scale_shift=None):
    """(out, border, blended) for [B, H, W] fp32 maps.  Paste where mask > 0 (with scale_shift [B, 2]: fp32(fp32(a * scale) + shift), two operations);
    border = 0 < zero-padded 3x3 box sum of (mask > 0) < 9; on the border the 3x3 mean of `blended` under BORDER_REFLECT_101: the nine terms added
    in float64, the sum rounded to fp32, the quotient fp32 / 9."""
    B = amodal.shape[0]
    inside = mask > 0
    pasted = amodal
    if scale_shift is not None:
        prod = amodal * scale_shift[:, 0].reshape(B, 1, 1)
        pasted = prod + scale_shift[:, 1].reshape(B, 1, 1)
    blended = torch.where(inside, pasted, base)
    box = F.conv2d(inside.float()[:, None], torch.ones(1, 1, 3, 3), padding=1)[:, 0]
    border = (box > 0) & (box < 9)
    H, W = blended.shape[-2:]
    padded = F.pad(blended.double()[:, None], (1, 1, 1, 1), mode="reflect")[:, 0]          # torch's "reflect" does not repeat the edge: reflect-101
    total = torch.zeros_like(blended, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            total = total + padded[:, dy:dy + H, dx:dx + W]
    blur = total.float() / 9
    return torch.where(border, blur, blended), border, blended


def blend_ref(amodal, base, mask, scale_shift=None):
    return blend_parts(amodal, base, mask, scale_shift)[0]


def blur_mag(blended):
    """Sum of |blended| over each reflect-padded 3x3 window, float64 (the budget of the nine-term sum)."""
    H, W = blended.shape[-2:]
    padded = F.pad(blended.double().abs()[:, None], (1, 1, 1, 1), mode="reflect")[:, 0]
    return sum(padded[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))


BLEND_SHAPES = [(2, 2), (2, 300), (37, 53), (3, 257), (40, 513)]          # the smallest legal size, one row pair across the x-block seam, odd, two and three x-blocks
BLEND_SCALE_SHIFTS = [None, (1.25, 0.5), (0.8125, -0.1875)]              # multiples of 2^-4; neither scale is a power of two, so the product rounds on Gaussian values


def mask_families(H, W):
    """name -> [H, W] fp32 mask: every family of the issue that fits the shape."""
    z = lambda: torch.zeros(H, W)      # noqa: E731
    out = {"empty": z(), "full": torch.ones(H, W)}
    my, mx = H // 2, W // 2
    for name, (y, x) in {"corner_tl": (0, 0), "corner_tr": (0, W - 1), "corner_bl": (H - 1, 0), "corner_br": (H - 1, W - 1), "edge_t": (0, mx), "edge_b": (H - 1, mx),
                         "edge_l": (my, 0), "edge_r": (my, W - 1), "interior": (my, mx)}.items():
        m = z()
        m[y, x] = 1
        out["pixel_" + name] = m
    hy, hx = max(1, H // 3), max(1, W // 3)
    ymid, xmid = slice(hy, max(hy + 1, H - hy)), slice(hx, max(hx + 1, W - hx))          # free of both borders where the shape has three rows / columns
    for name, (ys, xs) in {"top": (slice(0, hy), xmid), "bottom": (slice(H - hy, H), xmid), "left": (ymid, slice(0, hx)), "right": (ymid, slice(W - hx, W))}.items():
        m = z()
        m[ys, xs] = 1
        out["rect_" + name] = m
    m = z()          # a frame: one mask that touches all four borders and leaves the middle free
    m[0, :] = m[H - 1, :] = 1
    m[:, 0] = m[:, W - 1] = 1
    out["rect_all_four"] = m
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out["checkerboard"] = ((yy + xx) % 2).float()
    if W > 257:
        for c in (255, 256):          # the last column of the first x-block, the first of the second
            m = z()
            m[:, c] = 1
            out[f"line_col{c}"] = m
        m = z()
        m[my, 250:262] = 1
        out["line_across_seam"] = m
    m = z()          # any value > 0 is inside: 255 (a byte mask) and 0.5; a negative value is outside
    m[:, : max(1, W // 2)] = 255.0
    m[0, W - 1] = 0.5
    m[H - 1, W - 1] = -1.0
    out["values_255_half"] = m
    return out


@functools.lru_cache(maxsize=None)
def blend_case(H, W, exact):
    """(names, amodal, base, masks) with one image per mask family: exact = multiples of 2^-10 in [0, 1), otherwise Gaussian * 3."""
    fam = mask_families(H, W)
    names = list(fam)
    B = len(names)
    g = torch.Generator().manual_seed(1000 * H + W + (7 if exact else 0))
    if exact:
        amodal = torch.randint(0, 1024, (B, H, W), generator=g).float() / 1024.0
        base = torch.randint(0, 1024, (B, H, W), generator=g).float() / 1024.0
    else:
        amodal = torch.randn(B, H, W, generator=g) * 3
        base = torch.randn(B, H, W, generator=g) * 3
    return names, amodal, base, torch.stack([fam[k] for k in names])


def scale_shift_tensor(pair, B):
    return None if pair is None else torch.tensor([pair], dtype=torch.float32).repeat(B, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# tile blend (the formula of tile_blend_kernel's header comment)
# ---------------------------------------------------------------------------------------------------------------------------------
def feather(n, ramp):
    """w(i, n) = fp32(min(i + 1, n - i, ramp)) * fp32(1 / ramp), an fp32 product, i = 0 .. n - 1."""
    i = np.arange(n)
    inv = np.float32(1.0) / np.float32(ramp)
    return np.minimum(np.minimum(i + 1, n - i), ramp).astype(np.float32) * inv


def tile_blend_parts(tiles, origins, H, W, ramp):
    """tiles [B, T, th, tw] fp32, origins [(oy, ox)] * T -> (out fp32 [B, H, W], cover int [H, W], acc float64, wsum float64).

    out = sum_t w_t tile_t / sum_t w_t with w_t = fp32(wy * wx) and every product w_t * tile_t rounded to fp32; the two sums are float64 and the
    quotient is taken in float64 and rounded once.  Counted against this, a kernel that adds in fp32 makes, per pixel covered by T tiles: its T
    products (rounded here too, or not at all under an fma: at most 2^-24 * w_t * max|tile| each, 2^-24 * wsum * max|tile| together), T - 1 additions
    into acc (each at most 2^-24 * wsum * max|tile|), T - 1 additions into wsum (each 2^-24 relative), one quotient, and this function's final
    rounding: (1 + 2 (T - 1) + 1 + 1) * 2^-24 * max|tile| = (2 T + 1) * 2^-24 * max|tile| <= (2 T + 2) * 2^-24 * max|tile| after the division by wsum.
    A pixel that no tile covers is 0 / 0 = NaN."""
    B, T, th, tw = tiles.shape
    assert T == len(origins)
    w = torch.from_numpy(feather(th, ramp)[:, None] * feather(tw, ramp)[None, :])          # fp32 product
    acc = torch.zeros(B, H, W, dtype=torch.float64)
    wsum = torch.zeros(H, W, dtype=torch.float64)
    cover = torch.zeros(H, W, dtype=torch.int64)
    for t, (oy, ox) in enumerate(origins):
        acc[:, oy:oy + th, ox:ox + tw] += (w * tiles[:, t]).double()                          # fp32 product, float64 sum
        wsum[oy:oy + th, ox:ox + tw] += w.double()
        cover[oy:oy + th, ox:ox + tw] += 1
    return (acc / wsum).float(), cover, acc, wsum


def tile_blend_ref(tiles, origins, H, W, ramp):
    return tile_blend_parts(tiles, origins, H, W, ramp)[0]


# (tile h, tile w, image h, image w, overlap handed to tile_origins, ramp handed to the kernel = min(max(1, overlap), tile / 2) as tiled_apply passes it)
TILE_GEOMETRIES = [(8, 8, 8, 8, 4, 4),              # a single tile
                   (16, 16, 24, 40, 8, 8),          # ramp = tile / 2: no flat interior, four-tile corners everywhere
                   (16, 32, 40, 300, 0, 1),         # abutting tiles, ramp 1; the end-aligned last tile overlaps by 8 rows / 20 columns
                   (28, 42, 61, 100, 14, 14),       # ramp not a power of two; up to three tiles along an axis where the end-aligned tile lands
                   (32, 32, 48, 530, 16, 16)]       # two x-block seams


def tile_geometry_origins(th, tw, H, W, overlap):
    from hip_ext.tiling import tile_origins
    return [(y, x) for y in tile_origins(H, th, overlap) for x in tile_origins(W, tw, overlap)]


def tile_values(B, T, th, tw, exact, seed):
    g = torch.Generator().manual_seed(seed)
    if exact:
        return torch.randint(0, 1024, (B, T, th, tw), generator=g).float() / 1024.0
    return torch.randn(B, T, th, tw, generator=g) * 3


# ---------------------------------------------------------------------------------------------------------------------------------
# evaluation sums (reference src/util/metric.py:37-161, src/util/alignment.py)
# ---------------------------------------------------------------------------------------------------------------------------------
N, SUM_P, SUM_G, SUM_PP, SUM_PG, ABS_REL, SQ_REL, SQ, LOG_SQ, LOG, LOG10_ABS, D1, D2, D3, INV_SQ = range(15)          # ADA_EVAL_* of include/ada_hip.h
NAMES = ["N", "SUM_P", "SUM_G", "SUM_PP", "SUM_PG", "ABS_REL", "SQ_REL", "SQ", "LOG_SQ", "LOG", "LOG10_ABS", "D1", "D2", "D3", "INV_SQ"]
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)          # 1.25, 1.5625, 1.953125: exact in fp32
LINEAR = (N, SUM_P, SUM_G, SUM_PP, SUM_PG)
LOG_SUMS = (LOG_SQ, LOG, LOG10_ABS)


def _prepare(pred, gt, mask, scale_shift, clip, dtype):
    """The prediction the metrics see: fp32 pred * scale + shift (two operations) and torch.clamp, which propagates NaN, then the terms' type."""
    B = pred.shape[0]
    p = pred.float()
    if scale_shift is not None:
        shape = (B,) + (1,) * (pred.dim() - 1)
        p = p * scale_shift[:, 0].reshape(shape)
        p = p + scale_shift[:, 1].reshape(shape)
    if clip is not None:
        p = torch.clamp(p, float(np.float32(clip[0])), float(np.float32(clip[1])))
    m = torch.ones_like(p, dtype=torch.bool) if mask is None else (mask != 0)
    return p.to(dtype), gt.float().to(dtype), m


def _terms(p, g):
    """The 15 per-pixel terms in the type of p and g, written as the reference's functions write them (as float64 tensors, unmasked)."""
    d = p - g
    dl = torch.log(p) - torch.log(g)
    ratio = torch.max(p / g, g / p)
    di = 1.0 / p - 1.0 / g
    one, zero = torch.ones_like(p), torch.zeros_like(p)
    t = [one, p, g,
         p.double() * p.double(), p.double() * g.double(),                                    # the alignment's normal equations: products of fp32 values, exact in float64
         torch.abs(d) / g,                                                                   # abs_relative_difference
         torch.pow(torch.abs(d), 2) / g,                                                     # squared_relative_difference
         torch.pow(d, 2),                                                                    # rmse_linear
         torch.pow(dl, 2),                                                                   # rmse_log, silog_rmse
         dl,                                                                                 # silog_rmse
         torch.abs(torch.log10(p) - torch.log10(g))]                                         # log10
    t += [torch.where(ratio < thr, one, zero) for thr in THRESHOLDS]                         # threshold_percentage
    t += [torch.pow(di, 2)]                                                                  # i_rmse
    return [x.double() for x in t]


def _sum(terms, m):
    """[B, 15]: float64 sums over the mask; 0 outside it, as the reference's `x[~valid_mask] = 0` leaves it."""
    B = m.shape[0]
    return torch.stack([torch.where(m, x, torch.zeros_like(x)).reshape(B, -1).sum(1) for x in terms], dim=1)


def eval_pixel_terms(pred, gt, scale_shift=None, clip=None, dtype=torch.float32):
    """The unmasked per-pixel terms (a list of 15 float64 tensors), for tests that sum one pair of maps under several masks: eval_masked_sums."""
    p, g, _ = _prepare(pred, gt, None, scale_shift, clip, dtype)
    return _terms(p, g)


def eval_masked_sums(terms, mask):
    return _sum(terms, torch.ones_like(terms[0], dtype=torch.bool) if mask is None else (mask != 0))


def eval_terms_ref(pred, gt, mask=None, scale_shift=None, clip=None):
    """[B, 15] float64: every per-pixel term by the reference's fp32 rules (torch fp32 CPU operations), summed in float64."""
    p, g, m = _prepare(pred, gt, mask, scale_shift, clip, torch.float32)
    return _sum(_terms(p, g), m)


def eval_terms_fp64(pred, gt, mask=None, scale_shift=None, clip=None, with_abs=False):
    """The same with every term in float64: the high-precision reference.  with_abs: also the per-image float64 sums of |term| (the scale of the float64
    accumulation's own error) and of |log p| + |log g| weighted as each log sum's error propagates (see eval_tolerance)."""
    p, g, m = _prepare(pred, gt, mask, scale_shift, clip, torch.float64)
    terms = _terms(p, g)
    B = pred.shape[0]
    s = _sum(terms, m)
    if not with_abs:
        return s
    mag = _sum([x.abs() for x in terms], m)
    z = torch.zeros_like(p)
    la = torch.where(m, torch.log(p).abs() + torch.log(g).abs(), z)
    dl = torch.where(m, (torch.log(p) - torch.log(g)).abs(), z)
    la = torch.where(torch.isfinite(la), la, z)
    dl = torch.where(torch.isfinite(dl), dl, z)
    logs = torch.zeros(B, 15, dtype=torch.float64)
    logs[:, LOG] = la.reshape(B, -1).sum(1)
    logs[:, LOG10_ABS] = la.reshape(B, -1).sum(1) * float(np.log10(np.e))
    logs[:, LOG_SQ] = (2 * dl * la).reshape(B, -1).sum(1)
    return s, mag, logs


def eval_tolerance(ref32, ref64, mag, logs, n_pixels):
    """What the kernel may differ from eval_terms_fp64 by, per sum [B, 15]:

      4 |eval_terms_ref - eval_terms_fp64|      four times what fp32 terms cost on the CPU, neither side being the code under test;
      + 2^-21 sum (|log p| + |log g|)           for LOG (times log10 e for LOG10_ABS, and d(dl^2) = 2 |dl| d(dl) for LOG_SQ): __logf is v_log_f32 times ln 2,
                                                one ulp of log2 p and one product, where torch.log is correctly rounded;
      + n 2^-53 sum |term|                      the float64 accumulation itself, in whatever order the workgroups' atomics land (n - 1 additions, each
                                                within 2^-53 of a partial sum that sum |term| bounds) -- without it two float64 sums of the same terms in
                                                two orders could not be compared at all.
    The counts N, D1, D2, D3 get none of it: they are integers."""
    tol = 4 * (ref32 - ref64).abs() + 2.0 ** -21 * logs + n_pixels * 2.0 ** -53 * mag
    for k in (N, D1, D2, D3):
        tol[:, k] = 0
    return tol


# threshold ties -------------------------------------------------------------------------------------------------------------------
TIE_K = (2 ** 12, 2 ** 13)          # g = k / 1024 for the 4096 k of the top binade of [2^10, 2^13): g in [4, 8)


def _ulp_step(x, up):
    return torch.from_numpy(np.nextafter(x.numpy(), np.float32(np.inf if up else -np.inf)))


@functools.lru_cache(maxsize=None)
def tie_family(t):
    """For the threshold t: dict of fp32 [3, 4096] pairs (row 0 the tie, row 1 the moved value one ulp up, row 2 one ulp down).
    direct: gt = k / 1024, pred = t * gt;   mirrored: pred = k / 1024, gt = t * pred."""
    k = torch.arange(*TIE_K, dtype=torch.float64)
    base64 = k / 1024.0
    moved64 = base64 * t
    base, moved = base64.float(), moved64.float()
    assert torch.equal(base.double(), base64) and torch.equal(moved.double(), moved64), "t * k / 1024 is not exact in fp32"
    rows = torch.stack([moved, _ulp_step(moved, True), _ulp_step(moved, False)])
    fixed = base.expand(3, -1).contiguous()
    return dict(direct=(rows, fixed), mirrored=(fixed, rows))          # (pred, gt)


def tie_image(t):
    """(pred, gt) fp32 [1, 3, 4096, 3]: per row of tie_family the columns direct, mirrored, and pred = gt (ratio exactly 1, under every threshold)."""
    f = tie_family(t)
    pred = torch.stack([f["direct"][0], f["mirrored"][0], f["direct"][1]], dim=2)
    gt = torch.stack([f["direct"][1], f["mirrored"][1], f["direct"][1]], dim=2)
    return pred[None].contiguous(), gt[None].contiguous()


def under_threshold_ref(pred, gt, t):
    """The reference's rule (metric.py:104-110): torch.max(p / g, g / p) < t on fp32 CPU tensors."""
    return torch.max(pred / gt, gt / pred) < t


def under_threshold_reciprocal(pred, gt, t):
    """What a reciprocal-and-multiply would decide: p * fp32(1 / g), g * fp32(1 / p)."""
    return torch.max(pred * (1.0 / gt), gt * (1.0 / pred)) < t


# constant log difference ----------------------------------------------------------------------------------------------------------
CONST_LOG_N = (1, 2, 3, 7, 64, 300)


@functools.lru_cache(maxsize=None)
def const_log_pairs():
    """12 seeded fp32 pairs (c_pred, c_gt), log-uniform in [0.01, 50]."""
    rng = np.random.default_rng(20240)
    v = np.exp(rng.uniform(np.log(0.01), np.log(50.0), size=(12, 2))).astype(np.float32)
    return [(float(a), float(b)) for a, b in v]


def const_log_cases():
    return [(cp, cg, n) for (cp, cg) in const_log_pairs() for n in CONST_LOG_N]


# value-domain families -------------------------------------------------------------------------------------------------------------
EVAL_FAMILIES = ("normalised_good", "normalised_gross", "metric_80", "identical", "double")
EVAL_CLIP = {"normalised_good": (1e-3, 1.0), "normalised_gross": (1e-3, 1.0)}          # the runner's default clip; the other families are evaluated unclipped


@functools.lru_cache(maxsize=None)
def eval_family(name, B=2, H=61, W=300):
    """(pred, gt, mask) fp32 / fp32 / bool [B, H, W]; 18300 pixels per image: nine workgroups of the evaluation kernel."""
    rng = np.random.default_rng(EVAL_FAMILIES.index(name) + 77)
    shape = (B, H, W)
    if name.startswith("normalised"):
        gt = rng.uniform(1e-3, 1.0, size=shape)
        pred = gt * (1 + 1e-3 * rng.choice([-1.0, 1.0], size=shape)) if name == "normalised_good" else rng.uniform(-0.2, 1.3, size=shape)          # gross: beyond both clip bounds
    else:
        gt = rng.uniform(0.5, 80.0, size=shape)
        pred = {"metric_80": gt * rng.uniform(0.6, 1.6, size=shape) + rng.normal(0, 0.3, size=shape), "identical": gt, "double": None}[name]
    gt = gt.astype(np.float32)
    pred = 2 * gt if name == "double" else np.asarray(pred).astype(np.float32)
    if name == "metric_80":
        pred = np.maximum(pred, np.float32(0.05))
    mask = rng.uniform(size=shape) > 0.3
    return torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(mask)
