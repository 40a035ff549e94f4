"""The reference side of tests/test_gpu_layernorm_values.py, checked without a GPU: ref64 against torch in float64 and against tests/_exact.py's
un-shuffle restatement, the premises of the exact family, and -- the reason these tests exist -- an fp32 numpy emulation of layernorm_kernel's
arithmetic (lane layout, float4 inner sums, xor butterfly, two passes) that must stay inside budget() on every value family, with five mutants of
it that must not: one-pass variance, eps outside the root, eps omitted, eps fixed at 1e-5, variance over dim - 1.  Four of the five pass the
tolerance of test_layernorm_plain on Gaussian rows: the old inputs could not see them."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _exact as X
import _layernorm_ref as L

ROWS = 21
MUTANTS = ("one_pass", "eps_outside_root", "eps_omitted", "eps_1e-5", "dim_minus_1")


# ---------------------------------------------------------------------------------------------------------------------------------
# ref64 is LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), f"{what}: {err:.3e} apart in float64"


@pytest.mark.parametrize("dim", L.DIMS)
def test_ref64_is_torch_layer_norm_in_float64(dim):
    x = L.family("gauss", 3 * 11, dim)
    (w, b), (w2, b2) = L.gain_bias(dim), L.gain_bias(dim, 1)
    ln = lambda rows, g, o: F.layer_norm(rows.double(), (dim,), g.double(), o.double(), float(np.float32(L.EPS)))
    _same(L.ref64(x, dim, w, b, L.EPS, 33).f32, ln(x, w, b), "plain rows")
    for relu in (1, 2):
        r = L.ref64(x, dim, w, b, L.EPS, 33, relu=relu)
        _same(r.op, ln(x, w, b).clamp_min(0), f"relu = {relu}, operand copy")
        _same(r.f32, ln(x, w, b).clamp_min(0) if relu == 1 else ln(x, w, b), f"relu = {relu}, fp32 copy")
    for skip in (0, 1, 3):
        r = L.ref64(x, dim, w, b, L.EPS, 3 * (11 - skip), group_in=11, skip=skip)
        _same(r.f32, ln(x.view(3, 11, dim)[:, skip:].reshape(-1, dim), w, b), f"group_in = 11, skip = {skip}")
    for group, skip in ((0, 0), (11, 1), (11, 2)):
        r = L.ref64(x, dim, w, b, L.EPS, 33, w2=w2, b2=b2, out2_group=group, out2_skip=skip)
        _same(r.f32, ln(x, w, b), "main output beside a second one")
        _same(r.out2, ln(x.view(3, 11, dim)[:, skip:].reshape(-1, dim), w2, b2), f"second output, group {group} skip {skip}")
    # a wide input row: only the first dim columns of each are read (the class-token read: ld_in = N dim)
    wide = L.family("gauss", 3, 5 * dim)
    _same(L.ref64(wide, dim, w, b, L.EPS, 3).f32, ln(wide[:, :dim], w, b), "class-token rows")


@pytest.mark.parametrize("s,dim,H,W_", X.UNSHUFFLE_CASES)
def test_ref64_unshuffle_is_the_exact_suites_restatement_normalised(s, dim, H, W_):
    f = X.unshuffle_family(s, dim, H, W_)
    w, b = L.gain_bias(dim)
    rows = 2 * f["fh"] * f["fw"]
    r = L.ref64(f["inp"], dim, w, b, L.EPS, rows, unshuffle_s=s, grid=(f["fh"], f["fw"]), tap_bias=f["tapb"])
    assert torch.equal(r.rows, f["ref"].reshape(rows, dim)), "the gathered rows differ from tests/_exact.py unshuffle_family (dyadic inputs: exact in float64)"
    _same(r.f32, F.layer_norm(f["ref"].reshape(rows, dim), (dim,), w.double(), b.double(), float(np.float32(L.EPS))), "normalised un-shuffle")
    ring = L.ring_taps(f["fh"], f["fw"]).sum(-1)
    assert int(ring.max()) == 5 and int(ring[1:-1, 1:-1].max()) == 0 and int(ring[0, 1]) == 3, "ring: 5 taps at a corner, 3 on an edge, none inside"
    assert torch.equal(r.ntap.view(2, f["fh"], f["fw"])[0].long(), ring)
    plain = L.ref64(f["inp"], dim, w, b, L.EPS, rows, unshuffle_s=s, grid=(f["fh"], f["fw"]))
    inner = r.ntap.view(-1) == 0
    assert torch.equal(plain.f32[inner], r.f32[inner]) and not torch.equal(plain.f32[~inner], r.f32[~inner]), "tap_bias must change the ring rows and only them"


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact family's premises, in float64 and integers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", L.DIMS)
def test_exact_family_premises(dim):
    f = L.exact_family(dim)
    x = f.x.double()
    a, m = f.a, f.m
    assert torch.equal(torch.log2(a), torch.log2(a).round()) and float((m / a).abs().max()) <= 1024 and torch.equal(m / a, (m / a).round())
    k = x / a                                                     # every entry an integer multiple of its row's power of two
    assert torch.equal(k, k.round()) and float(k.abs().sum(1).max()) < X.LIMIT, "partial sums leave fp32's significand"
    assert torch.equal(k.sum(1, keepdim=True), dim * m / a) and int((f.sign > 0).sum(1).min()) == dim // 2 == int((f.sign > 0).sum(1).max())
    mean = x.sum(1, keepdim=True) / dim
    assert torch.equal(mean, m) and torch.equal(mean.float().double(), mean)
    d = x - mean
    assert torch.equal(d, f.sign * a)
    var = (d * d).sum(1, keepdim=True) / dim
    assert torch.equal(var, a * a) and float((d * d / (a * a)).sum(1).max()) < X.LIMIT
    rstd32 = 1.0 / torch.sqrt(var.float())                         # fp32, correctly rounded: exact on powers of four
    assert torch.equal(rstd32.double(), 1.0 / a)
    y32 = (d.float() * rstd32) * f.w + f.b                         # the kernel's expression in fp32, and the same with the last two fused
    assert torch.equal(y32.double(), f.ref) and torch.equal(torch.addcmul(f.b, d.float() * rstd32, f.w).double(), f.ref)
    q = f.ref * 1024.0
    assert torch.equal(q, q.round()) and float(q.abs().max()) <= 6144, "outputs are multiples of 2^-10 within 13 bits"
    _same(L.ref64(f.x, dim, f.w, f.b, 0.0, f.x.shape[0]).f32, f.ref, "ref64 on the exact family")
    for op in X.OP_TYPES:                                          # the operand copy really rounds, and [hi | lo] holds the value whole
        share, _, trunc = X.rounding_census(f.ref, op)
        assert share >= 0.10 and trunc > 0.05, f"{op}: {share:.1%} of the outputs need rounding, truncation differs on {trunc:.1%}"
        hi, lo = X.split_ref(f.ref, op)
        assert torch.equal(hi.double() + lo.double(), f.ref), f"{op}: hi + lo != v"
    # three fp32 summation orders equal fp64: forwards, backwards, and the kernel's (below)
    x32 = f.x.numpy()
    assert np.array_equal(np.cumsum(x32, 1, dtype=np.float32)[:, -1].astype(np.float64), (dim * m).view(-1).numpy())
    assert np.array_equal(np.cumsum(x32[:, ::-1], 1, dtype=np.float32)[:, -1].astype(np.float64), (dim * m).view(-1).numpy())
    assert np.array_equal(_emulate(x32, f.w.numpy(), f.b.numpy(), 0.0).astype(np.float64), f.ref.numpy()), "the emulated kernel is not exact on the exact family"


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation of layernorm_kernel<LPR> and its mutants
# ---------------------------------------------------------------------------------------------------------------------------------
def _row_sum(t):
    """t [R, dim] fp32 terms -> [R, 1] fp32 in the kernel's order: lane l of the row's LPR lanes owns float4 chunks l, l + LPR, ..., adds each as
    (x + y) + (z + w) onto its running sum, then the lanes meet in an xor butterfly (row_sum<LPR>)."""
    R, dim = t.shape
    lpr, nch = L.lanes_per_row(dim), dim // 4
    per = math.ceil(nch / lpr)
    c = t.reshape(R, nch, 4)
    c = (c[:, :, 0] + c[:, :, 1]) + (c[:, :, 2] + c[:, :, 3])
    c = np.concatenate([c, np.zeros((R, per * lpr - nch), np.float32)], 1).reshape(R, per, lpr)      # chunk lane + LPR i at [i, lane]; dead chunks add nothing
    s = np.zeros((R, lpr), np.float32)
    for i in range(per):
        s = s + c[:, i]
    lane = np.arange(lpr)
    m = lpr // 2
    while m:
        s = s + s[:, lane ^ m]
        m //= 2
    assert s.dtype == np.float32
    return s[:, :1]


def _emulate(x, w, b, eps, mutant=None):
    x, w, b = x.astype(np.float32), w.astype(np.float32), b.astype(np.float32)
    dim = x.shape[1]
    n, eps = np.float32(dim), np.float32(eps)
    with np.errstate(all="ignore"):
        mean = _row_sum(x) / n
        d = x - mean
        if mutant == "one_pass":
            var = _row_sum(x * x) / n - mean * mean
        elif mutant == "dim_minus_1":
            var = _row_sum(d * d) / np.float32(dim - 1)
        else:
            var = _row_sum(d * d) / n
        one = np.float32(1.0)
        if mutant == "eps_outside_root":
            rstd = one / (np.sqrt(var) + eps)
        elif mutant == "eps_omitted":
            rstd = one / np.sqrt(var)
        elif mutant == "eps_1e-5":
            rstd = one / np.sqrt(var + np.float32(1e-5))
        else:
            rstd = one / np.sqrt(var + eps)
        y = d * rstd * w + b
    assert y.dtype == np.float32
    return y


def _ratio(name, dim, mutant=None):
    """Largest |emulation - ref64| / budget over the family's rows; a non-finite output counts as infinitely far."""
    x = L.family(name, ROWS, dim)
    w, b = L.gain_bias(dim)
    r = L.ref64(x, dim, w, b, L.EPS, ROWS)
    y = torch.from_numpy(_emulate(x.numpy(), w.numpy(), b.numpy(), L.EPS, mutant)).double()
    q = (y - r.f32).abs() / L.budget(r, w, r.f32)
    return float(torch.where(torch.isfinite(y), q, torch.full_like(q, float("inf"))).max())


def test_butterfly_emulation_sums_every_element_once():
    for dim in (4, 48, 512, 516, 1536):
        t = np.zeros((dim, dim), np.float32)
        t[np.arange(dim), np.arange(dim)] = np.arange(1, dim + 1)
        assert np.array_equal(_row_sum(t)[:, 0], np.arange(1, dim + 1, dtype=np.float32)), dim
    assert [L.chain_adds(d) for d in L.DIMS] == [8, 28, 36, 18, 22, 30] and L.chain_adds(4) == 8 and L.chain_adds(1028) == 26


@pytest.mark.parametrize("dim", L.DIMS)
def test_two_pass_emulation_stays_inside_the_budget(dim):
    for name in L.FAMILIES:
        q = _ratio(name, dim)
        print(f"two-pass emulation {name} dim {dim}: worst error / budget = {q:.3f}")
        assert q <= 1.0, f"{name} dim {dim}: the kernel's own arithmetic leaves the budget ({q:.3f})"


def test_value_families_have_the_expected_results():
    for dim in L.DIMS:
        w, b = L.gain_bias(dim)
        x = L.family("constant", ROWS, dim)
        assert np.array_equal(_emulate(x.numpy(), w.numpy(), b.numpy(), L.EPS), np.broadcast_to(b.numpy(), (ROWS, dim))), "constant rows: out == bias bit for bit"
        _same(L.ref64(x, dim, w, b, L.EPS, ROWS).f32, b.double().expand(ROWS, dim), "constant rows in ref64")
        r = L.ref64(L.family("tiny", ROWS, dim), dim, w, b, L.EPS, ROWS)
        rms = float(r.yhat.pow(2).mean().sqrt())
        assert 0.05 < rms < 0.2, f"tiny rows: normalised values of order 0.1, got rms {rms:.3f}"
        for name, lo, hi in (("offset_1e2", 50, 200), ("offset_1e3", 500, 2000), ("offset_1e5", 5e4, 2e5)):
            q = L.ref64(L.family(name, ROWS, dim), dim, w, b, L.EPS, ROWS)
            ratio = float((q.mean.abs() / q.sig).median())
            assert lo < ratio < hi, f"{name}: mean / sigma = {ratio:.3g}"


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_is_rejected_by_the_budget_and_was_invisible_before(mutant):
    worst = {(name, dim): _ratio(name, dim, mutant) for name in L.FAMILIES for dim in L.DIMS}
    (name, dim), q = max(worst.items(), key=lambda kv: kv[1])
    print(f"{mutant}: worst error / budget = {q:.3g} on {name} dim {dim}; per family: " +
          ", ".join(f"{n} {max(worst[n, d] for d in L.DIMS):.3g}" for n in L.FAMILIES))
    assert q >= 4.0, f"{mutant}: no family sees it (worst {q:.3g} of the budget)"
    if mutant == "dim_minus_1":
        return
    for dim in L.DIMS:                     # test_layernorm_plain's inputs and tolerance: atol 2e-5, rtol 1e-5 against fp32 torch
        x = L.family("gauss", ROWS, dim)
        w, b = L.gain_bias(dim)
        ref = F.layer_norm(x, (dim,), w, b, L.EPS)
        y = torch.from_numpy(_emulate(x.numpy(), w.numpy(), b.numpy(), L.EPS, mutant))
        assert bool(((y - ref).abs() <= 2e-5 + 1e-5 * ref.abs()).all()), f"{mutant} dim {dim}: the old tolerance on Gaussian rows does see it"
