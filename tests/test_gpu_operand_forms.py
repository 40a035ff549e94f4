"""hip_ext.operands against the kernels: for every legal (weight form, activation form) pair the REAL producer writes the activation from an fp32 matrix
(ada_layernorm_ex, identity, told ``ActForm.split_seg``), ``pack`` lays out the weights, and ada_igemm runs with ``walk``'s arguments -- as a plain GEMM and as
a 3x3 convolution over a zero-bordered grid.  Inputs are exact (tests/_exact.py's budget: every product and partial sum a multiple of the unit below 2^24 of
it), so the result must equal the fp64 product of the pair's terms bit for bit.  The fp8 row: ``pack`` picks the scales, so the expectation is the fp64
product of the operands DECODED from the bytes, within fp32 accumulation error K 2^-24 sum|a||w|."""
import pytest
import torch
import torch.nn.functional as F

import _exact as X
from hip_ext import operands as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEG, N = 128, 64
WIDE_X, WIDE_W = list(range(3, SEG, 16)), list(range(11, SEG, 16))     # eight columns each where x / w need more bits than the operand type has


def _inputs(rows, taps, seed):
    """x [rows, SEG]: integers in [-2, 2]; +-(8 + j 2^-8), j odd, in the WIDE_X columns (12 bits: hi + lo, lo != 0).  w [N, taps, SEG]: k / 4, |k| <= 4;
    +-(1 + j 2^-11), j odd, in the WIDE_W columns.  A wide x meets a narrow w and the other way round: every product is a multiple of 2^-11, lo * lo is zero."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()      # noqa: E731
    x = ri(-2, 2, rows, SEG)
    x[:, WIDE_X] = (2 * ri(0, 1, rows, 8) - 1) * (8 + (2 * ri(0, 127, rows, 8) + 1) / 256)
    w = ri(-4, 4, N, taps, SEG) / 4
    w[..., WIDE_W] = (2 * ri(0, 1, N, taps, 8) - 1) * (1 + (2 * ri(0, 1023, N, taps, 8) + 1) / 2048)
    return x.float(), w.float()


def _produce(hip, x, act, grid=None):
    """The activation buffer as the engine's producers write it: plain rows, or the interior of a zero-bordered [1, H + 2, W + 2, width] grid."""
    op = hip.operand_dtype()
    rows, width = x.shape[0], act.width(SEG)
    if grid is None:
        buf = torch.zeros(rows, width, dtype=op, device=DEV)
        hip.layernorm(x.to(DEV), SEG, rows, SEG, None, None, 1e-6, identity=True, out_op=buf, ld_op=width, split_seg=act.split_seg(SEG))
    else:
        buf = torch.zeros(1, grid[0] + 2, grid[1] + 2, width, dtype=op, device=DEV)
        hip.layernorm(x.to(DEV), SEG, rows, SEG, None, None, 1e-6, identity=True, out_op=buf, ld_op=width, map_op=hip.MAP_PAD, map_h=grid[0], map_w=grid[1],
                      split_seg=act.split_seg(SEG))
    return buf


def _terms(p, act, x, w, op):
    """The fp64 operand pairs the walk of (p.form, act) contracts -- restated from include/ada_hip.h, not from the packer."""
    x_hi, x_lo = X.split_ref(x.double(), op)
    w_hi = w.to(op)
    w_lo = (w - w_hi.float()).to(op)
    if p.form == O.W_PLAIN:
        return [(x_hi, w_hi)]
    if p.form == O.W_SPLIT2:
        return [(x_hi, w_hi), (x_hi, w_lo)]
    assert p.form == O.W_SPLIT3 and act is O.A_HILO
    return [(x_hi, w_hi), (x_lo, w_hi), (x_hi, w_lo)]


def _f8_terms(p, buf_rows):
    """(a, w) fp64 pairs decoded from the bytes of a [rows, 2 SEG] [hi | lo8 | hi8] buffer and of [w_hi | w_hi8 | w_lo8] weights, scales from the word."""
    word = p.f8_scales
    sc = [2.0 ** (((word >> s) & 255) - 127) for s in (0, 8, 16, 24)]       # A then W byte of [f8_from, f8_mid), A then W byte of [f8_mid, period)
    a = buf_rows.cpu().contiguous().view(torch.uint8).reshape(buf_rows.shape[0], 4 * SEG)
    a_hi, a_lo8, a_hi8 = a[:, :2 * SEG].contiguous().view(torch.float16), a[:, 2 * SEG:3 * SEG].contiguous().view(torch.float8_e5m2), a[:, 3 * SEG:].contiguous().view(torch.float8_e5m2)
    b = p.t.cpu().contiguous().view(torch.uint8).reshape(*((N, p.taps) if p.taps > 1 else (N,)), 4 * SEG)
    w_hi, w_hi8, w_lo8 = b[..., :2 * SEG].contiguous().view(torch.float16), b[..., 2 * SEG:3 * SEG].contiguous().view(torch.float8_e4m3fn), b[..., 3 * SEG:].contiguous().view(torch.float8_e4m3fn)
    return [(a_hi.double(), w_hi.double()), (a_lo8.double() * sc[0], w_hi8.double() * sc[1]), (a_hi8.double() * sc[2], w_lo8.double() * sc[3])]


def _rows(hip, taps):
    """The legal pairs: all of them for plain rows; a 3x3 convolution reads whole pixels, so neither the hi half alone nor [w_hi | w_lo]."""
    pairs = [(O.W_PLAIN, O.A_PLAIN), (O.W_SPLIT3, O.A_HILO)] + ([(O.W_PLAIN, O.A_HILO), (O.W_SPLIT2, O.A_PLAIN), (O.W_SPLIT2, O.A_HILO)] if taps == 1 else [])
    if hip.operand_dtype() == torch.float16:      # the [hi | lo8 | hi8] form and the fp8 correction terms exist for fp16 operands only
        pairs += [(O.W_F8, O.A_HILO8)] + ([(O.W_PLAIN, O.A_HILO8), (O.W_SPLIT2, O.A_HILO8)] if taps == 1 else [])
    return pairs


def _check(out, terms, contract, K, what, exact):
    ref = sum(contract(a, w) for a, w in terms)
    mag = sum(contract(a.abs(), w.abs()) for a, w in terms)
    if not exact:
        err = float(((out.double().cpu() - ref).abs() / (K * 2.0 ** -24 * mag).clamp_min(1e-300)).max())
        print(f"{what}: worst |out - ref| = {err:.3f} of the bound K 2^-24 sum|a||w| (K = {K})")
        assert err <= 1.0, what
    else:
        X.assert_exact_budget(mag=mag, unit=2.0 ** -11, ref=ref, what=what)
        X.assert_bits(out, ref, what)


def test_every_linear_row_of_the_walk_table(hip):
    op, M = hip.operand_dtype(), 64
    x, w = _inputs(M, 1, 11)
    for form, act in _rows(hip, 1):
        what = f"{form} x {act.name}"
        p = O.pack(w.reshape(N, SEG), form, op)
        buf = _produce(hip, x, act)
        kw = O.walk(p, act, buf.shape[1])
        out = torch.full((M, N), -7.0, device=DEV)
        hip.igemm(M=M, N=N, A=buf, W=p.t.to(DEV), flags=0, out_f32=out, ldo_f32=N, **kw)
        terms = _f8_terms(p, buf) if form == O.W_F8 else _terms(p, act, x, w.reshape(N, SEG), op)
        x_hi, x_lo = X.split_ref(x.double(), op)      # the producer wrote the form it was told
        X.assert_bits(buf[:, :SEG], x_hi, what + ": hi segment")
        if act is O.A_HILO:
            X.assert_bits(buf[:, SEG:], x_lo, what + ": lo segment")
        _check(out, terms, lambda a, b: a.double() @ b.double().T, kw["K"], what, exact=form != O.W_F8)


def test_every_convolution_row_of_the_walk_table(hip):
    op, (H, Wd) = hip.operand_dtype(), (4, 6)
    M = H * Wd
    x, w = _inputs(M, 9, 12)

    def conv(a, b):      # a [M, SEG] pixel rows, b [N, 9, SEG] tap-major -> [M, N]
        img = a.double().reshape(1, H, Wd, SEG).permute(0, 3, 1, 2)
        return F.conv2d(img, b.double().reshape(N, 3, 3, SEG).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(M, N)
    for form, act in _rows(hip, 9):
        what = f"3x3 {form} x {act.name}"
        p = O.pack(w.reshape(N, 9 * SEG), form, op, taps=9)
        buf = _produce(hip, x, act, (H, Wd))
        border = buf.clone()
        border[:, 1:-1, 1:-1] = 0
        assert float(border.float().abs().max()) == 0.0, what + ": border written"
        kw = O.walk(p, act, buf.shape[3])
        out = torch.full((M, N), -7.0, device=DEV)
        hip.igemm(M=M, N=N, A=buf, W=p.t.to(DEV), a_mode=hip.A_CONV3, conv=(H, Wd, H + 2, Wd + 2, 1), flags=0, out_f32=out, ldo_f32=N, **kw)
        if form == O.W_F8:
            terms = [(a, b.reshape(N, 9, SEG)) for a, b in _f8_terms(p, buf[0, 1:-1, 1:-1].reshape(M, -1))]
        else:
            terms = _terms(p, act, x, w, op)
        _check(out, terms, conv, kw["K"], what, exact=form != O.W_F8)
