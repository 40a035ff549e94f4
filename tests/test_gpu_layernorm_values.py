"""ada_layernorm_ex against its fp64 restatement, within the error its own fp32 arithmetic allows (tests/_layernorm_ref.py: ref64, budget; the premise
side is tests/test_layernorm_ref_cpu.py).  Value domain -- rows with mean / sigma up to 1e5, outlier channels, rows where eps is the whole denominator --
the exact family bit for bit, eps as an argument, every dim at which a lane or the dispatch changes, row selection, the second output on both
kernels, the padded map and the ReLU modes, the normalising un-shuffle, non-finite rows, and the argument checks.

Every output buffer is filled with GUARD and is 8 columns wider and 3 rows longer than what the launch may write, split segments are wider than dim,
and input rows carry NaN behind dim: each test ends by comparing every byte outside the expected stores with the fill."""
import pytest
import torch

import _exact as X
import _layernorm_ref as L
from _exact import assert_bits, assert_within, rne

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -7.0
ROWS = 21                                        # neither a multiple of 4 (rows per workgroup, LPR 64) nor of 16 (LPR 16): the last wave holds live and dead rows
EDGE_DIMS = (4, 8, 60, 64, 68, 252, 256, 260, 508, 512, 516, 764, 768, 1020, 1024, 1028, 1532, 1536)
EDGE_ROWS = (1, 3, 4, 5, 15, 16, 17, 65)


def _f8_seg(dim):
    return (dim + 8 + 127) // 128 * 128


def _need_f16(hip):
    if hip.operand_dtype() != torch.float16:
        pytest.skip("the [hi | lo8 | hi8] form exists for fp16 operands only")


def _inp(x, pad=8):
    """CPU [R, C] fp32 -> (device [R, C + pad] with NaN behind C, ld)."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"))
    buf[:, :x.shape[1]] = x
    return buf.to(DEV), x.shape[1] + pad


class Out:
    """A guarded output: rows x (dim, or two segments of |seg|) plus 8 columns and 3 rows of GUARD.  seg > 0: [hi | lo], seg < 0: [hi | lo8 | hi8]."""

    def __init__(self, rows, dim, dtype, seg=0):
        self.rows, self.dim, self.seg, self.width = rows, dim, seg, (2 * abs(seg) if seg else dim)
        self.buf = torch.full((rows + 3, self.width + 8), GUARD, dtype=dtype, device=DEV)
        self.ld = self.width + 8

    def spans(self):
        """Byte ranges of a row that a launch may write."""
        it, d, s = self.buf.element_size(), self.dim, abs(self.seg)
        if self.seg > 0:
            return [(0, d * it), (s * it, (s + d) * it)]
        if self.seg < 0:
            return [(0, d * it), (2 * s, 2 * s + d), (3 * s, 3 * s + d)]
        return [(0, d * it)]

    def cpu(self):
        return self.buf.cpu()

    def guards_untouched(self, what, written=None):
        """Every byte outside spans() of the `written` rows (default: the first `rows`) still holds the fill."""
        got = self.buf.cpu().contiguous().view(torch.uint8).reshape(self.buf.shape[0], -1)
        fill = torch.full(self.buf.shape, GUARD, dtype=self.buf.dtype).view(torch.uint8).reshape(self.buf.shape[0], -1)
        free = torch.ones(got.shape, dtype=torch.bool)
        rows = torch.arange(self.rows) if written is None else written
        for a, z in self.spans():
            free[rows, a:z] = False
        bad = free & (got != fill)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} guard bytes overwritten, first at (row, byte) {tuple(bad.nonzero()[0].tolist())}"
        assert int((~free).sum()) == len(rows) * sum(z - a for a, z in self.spans())


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _check_pair(of, oo, r, w, op, what, rows=None):
    """fp32 copy within budget, operand copy within budget + half an operand ulp; returns the two worst error / bound ratios."""
    rows = of.rows if rows is None else rows
    bf = L.budget(r, w, r.pre)
    got_f, got_o = of.cpu()[:rows, :of.dim].double(), oo.cpu()[:rows, :oo.dim].double()
    assert bool(torch.isfinite(got_f).all()) and bool(torch.isfinite(got_o).all()), f"{what}: non-finite output"
    assert_within(got_f, r.f32, bf, None, what + " fp32")
    assert_within(got_o, r.op, bf, op, what + " operand")
    return float(((got_f - r.f32).abs() / bf).max()), float(((got_o - r.op).abs() / (bf + X.ulp(r.op, op) / 2)).max())


def _check_forms_of(oo, v32, op, what, rows=None):
    """The operand buffer holds the split form of the fp32 values v32 (the launch's own fp32 copy), by tests/_exact.py's restatements: hi = rne(v),
    lo = rne(v - hi); lo8 = e5m2((v - hi) 2^10), hi8 = e5m2(v)."""
    rows = oo.rows if rows is None else rows
    b, d, s = oo.cpu()[:rows], oo.dim, abs(oo.seg)
    v64 = v32.cpu()[:rows].double()
    hi = rne(v64, op)
    assert_bits(b[:, :d], hi, what + " hi")
    resid = (v32.cpu()[:rows] - hi.float())                       # fp32, as split_lo4 / split_lo8 compute it (exact: Sterbenz-like, |v - hi| <= ulp / 2)
    if oo.seg > 0:
        assert_bits(b[:, s:s + d], rne(resid.double(), op), what + " lo")
    elif oo.seg < 0:
        raw = b.contiguous().view(torch.uint8).reshape(rows, -1)
        assert torch.equal(raw[:, 2 * s:2 * s + d], X.e5m2(resid * 1024.0)), what + ": lo8 bytes"
        assert torch.equal(raw[:, 3 * s:3 * s + d], X.e5m2(v32.cpu()[:rows])), what + ": hi8 bytes"


def _check_forms_ref(oo, ref, bud, op, what):
    """The same forms where no fp32 copy exists (the second output): hi within bud + ulp / 2; hi + lo within bud + half an ulp of the residual's size;
    the e5m2 bytes within bud + half an e5m2 ulp."""
    b, d, s = oo.cpu()[:oo.rows], oo.dim, abs(oo.seg)
    hi = b[:, :d].double()
    assert_within(hi, ref, bud, op, what + " hi")
    resid = (ref - hi).abs() + bud                                # no smaller than |v - hi| for any v within bud of ref
    if oo.seg > 0:
        lo = b[:, s:s + d].double()
        lim = bud + X.ulp(resid, op) / 2
        q = float(((hi + lo - ref).abs() / lim).max())
        print(f"{what} hi + lo: worst / bound = {q:.3f}")
        assert q <= 1.0, f"{what}: hi + lo leaves the bound ({q:.3f})"
    elif oo.seg < 0:
        raw = b.contiguous().view(torch.uint8).reshape(oo.rows, -1)
        lo8 = raw[:, 2 * s:2 * s + d].contiguous().view(torch.float8_e5m2).float().double() / 1024.0
        hi8 = raw[:, 3 * s:3 * s + d].contiguous().view(torch.float8_e5m2).float().double()
        q_lo = float(((hi + lo8 - ref).abs() / (bud + L.ulp_e5m2(resid * 1024.0) / 2 / 1024.0)).max())
        q_hi = float(((hi8 - ref).abs() / (bud + L.ulp_e5m2(ref.abs() + bud) / 2)).max())
        print(f"{what}: hi + lo8 worst / bound = {q_lo:.3f}, hi8 = {q_hi:.3f}")
        assert q_lo <= 1.0 and q_hi <= 1.0, f"{what}: e5m2 bytes leave the bound (lo8 {q_lo:.3f}, hi8 {q_hi:.3f})"


# =====================================================================================================================
# a. value domain
# =====================================================================================================================
@pytest.mark.parametrize("dim", L.DIMS)
@pytest.mark.parametrize("name", L.FAMILIES)
def test_value_domain(hip, name, dim):
    op = hip.operand_dtype()
    x = L.family(name, ROWS, dim)
    w, b = L.gain_bias(dim)
    r = L.ref64(x, dim, w, b, L.EPS, ROWS)
    xin, ld = _inp(x)
    of, oo = Out(ROWS, dim, torch.float32), Out(ROWS, dim, op)
    hip.layernorm(xin, ld, ROWS, dim, *_dev(w, b), L.EPS, out_op=oo.buf, ld_op=oo.ld, out_f32=of.buf, ld_f32=of.ld)
    qf, qo = _check_pair(of, oo, r, w, op, f"{name} dim {dim}")
    print(f"RATIO {name} {dim} fp32 {qf:.3f} operand {qo:.3f}")
    if name == "constant":
        assert_bits(of.cpu()[:ROWS, :dim], b.expand(ROWS, dim), "constant rows: the fp32 output is the bias")
    of.guards_untouched("fp32")
    oo.guards_untouched("operand")


# =====================================================================================================================
# b. exact
# =====================================================================================================================
@pytest.mark.parametrize("dim", L.DIMS)
def test_exact_family_bit_for_bit(hip, dim):
    op = hip.operand_dtype()
    f = L.exact_family(dim, ROWS)
    xin, ld = _inp(f.x)
    w, b = _dev(f.w, f.b)
    of, oo = Out(ROWS, dim, torch.float32), Out(ROWS, dim, op)
    hip.layernorm(xin, ld, ROWS, dim, w, b, 0.0, out_op=oo.buf, ld_op=oo.ld, out_f32=of.buf, ld_f32=of.ld)
    assert_bits(of.cpu()[:ROWS, :dim], f.ref, f"exact family dim {dim}, fp32")
    assert_bits(oo.cpu()[:ROWS, :dim], rne(f.ref, op), f"exact family dim {dim}, operand")
    seg = dim + 4
    of2, os_ = Out(ROWS, dim, torch.float32), Out(ROWS, dim, op, seg=seg)
    hip.layernorm(xin, ld, ROWS, dim, w, b, 0.0, out_op=os_.buf, ld_op=os_.ld, out_f32=of2.buf, ld_f32=of2.ld, split_seg=seg)
    assert_bits(of2.cpu()[:ROWS, :dim], f.ref, "fp32 beside [hi | lo]")
    hi, lo = X.split_ref(f.ref, op)
    got = os_.cpu()[:ROWS]
    assert_bits(got[:, :dim], hi, "[hi | lo] hi")
    assert_bits(got[:, seg:seg + dim], lo, "[hi | lo] lo")
    assert torch.equal(got[:, :dim].double() + got[:, seg:seg + dim].double(), of2.cpu()[:ROWS, :dim].double()), "hi + lo != the fp32 value"
    for o in (of, oo, of2, os_):
        o.guards_untouched(f"exact dim {dim}")


# =====================================================================================================================
# c. eps is an argument
# =====================================================================================================================
@pytest.mark.parametrize("eps", [1e-6, 1e-3, 0.5])
@pytest.mark.parametrize("dim", [384, 1024])
@pytest.mark.parametrize("name", ["tiny", "constant"])
def test_eps_is_an_argument(hip, name, dim, eps):
    op = hip.operand_dtype()
    x = L.family(name, ROWS, dim)
    w, b = L.gain_bias(dim)
    r = L.ref64(x, dim, w, b, eps, ROWS)
    xin, ld = _inp(x)
    of, oo = Out(ROWS, dim, torch.float32), Out(ROWS, dim, op)
    hip.layernorm(xin, ld, ROWS, dim, *_dev(w, b), eps, out_op=oo.buf, ld_op=oo.ld, out_f32=of.buf, ld_f32=of.ld)
    _check_pair(of, oo, r, w, op, f"{name} dim {dim} eps {eps}")
    if name == "constant":
        assert_bits(of.cpu()[:ROWS, :dim], b.expand(ROWS, dim), "constant rows: the fp32 output is the bias")
    of.guards_untouched("fp32")
    oo.guards_untouched("operand")


# =====================================================================================================================
# d. dispatch and lane edges
# =====================================================================================================================
@pytest.mark.parametrize("name", ["gauss", "offset_1e3"])
@pytest.mark.parametrize("dim", EDGE_DIMS)
def test_dispatch_and_lane_edges(hip, name, dim):
    op = hip.operand_dtype()
    top = max(EDGE_ROWS)
    x = L.family(name, top, dim)
    w, b = L.gain_bias(dim)
    xin, ld = _inp(x)
    wd, bd = _dev(w, b)
    for rows in EDGE_ROWS:                                          # the rows are independent: every count normalises a prefix of the same rows
        r = L.ref64(x, dim, w, b, L.EPS, rows)
        of, oo = Out(rows, dim, torch.float32), Out(rows, dim, op)
        hip.layernorm(xin, ld, rows, dim, wd, bd, L.EPS, out_op=oo.buf, ld_op=oo.ld, out_f32=of.buf, ld_f32=of.ld)
        _check_pair(of, oo, r, w, op, f"{name} dim {dim} rows {rows}")
        of.guards_untouched(f"fp32, dim {dim} rows {rows}")
        oo.guards_untouched(f"operand, dim {dim} rows {rows}")


# =====================================================================================================================
# e. row selection
# =====================================================================================================================
@pytest.mark.parametrize("skip", [0, 1, 3])
@pytest.mark.parametrize("dim", [128, 768])
def test_group_in_and_skip(hip, dim, skip):
    op = hip.operand_dtype()
    B, G = 3, 7
    rows = B * (G - skip)
    x = L.family("offset_1e2", B * G, dim)
    w, b = L.gain_bias(dim)
    r = L.ref64(x, dim, w, b, L.EPS, rows, group_in=G, skip=skip)
    xin, ld = _inp(x)
    of, oo = Out(rows, dim, torch.float32), Out(rows, dim, op)
    hip.layernorm(xin, ld, rows, dim, *_dev(w, b), L.EPS, group_in=G, skip=skip, out_op=oo.buf, ld_op=oo.ld, out_f32=of.buf, ld_f32=of.ld)
    _check_pair(of, oo, r, w, op, f"group_in {G} skip {skip} dim {dim}")
    of.guards_untouched("fp32")
    oo.guards_untouched("operand")


@pytest.mark.parametrize("dim", [384, 1024])
def test_class_token_read(hip, dim):
    """The engine's class-token read-out: row b is the first dim floats of a [N dim]-wide row; the other tokens are NaN here."""
    op = hip.operand_dtype()
    B, N = 3, 5
    x = L.family("massive", B, dim)
    w, b = L.gain_bias(dim)
    r = L.ref64(x, dim, w, b, L.EPS, B)
    tokens = torch.full((B, N, dim), float("nan"))
    tokens[:, 0] = x
    of, oo = Out(B, dim, torch.float32), Out(B, dim, op)
    hip.layernorm(tokens.to(DEV), N * dim, B, dim, *_dev(w, b), L.EPS, out_op=oo.buf, ld_op=oo.ld, out_f32=of.buf, ld_f32=of.ld)
    _check_pair(of, oo, r, w, op, f"class-token read dim {dim}")
    of.guards_untouched("fp32")
    oo.guards_untouched("operand")


# =====================================================================================================================
# f. second output, both kernels
# =====================================================================================================================
@pytest.mark.parametrize("form2", ["plain", "hi_lo", "f8"])
@pytest.mark.parametrize("group,skip", [(0, 0), (11, 1), (11, 2)])
@pytest.mark.parametrize("dim", [384, 768])
def test_second_output(hip, dim, group, skip, form2):
    op = hip.operand_dtype()
    if form2 == "f8":
        _need_f16(hip)
    rows = 33
    seg2 = {"plain": 0, "hi_lo": dim + 8, "f8": -_f8_seg(dim)}[form2]
    seg1 = 0 if form2 == "hi_lo" else dim + 8                    # the main output's form always differs from the second's
    x = L.family("offset_1e2", rows, dim)
    (w, b), (w2, b2) = L.gain_bias(dim), L.gain_bias(dim, 1)
    r = L.ref64(x, dim, w, b, L.EPS, rows, w2=w2, b2=b2, out2_group=group, out2_skip=skip)
    xin, ld = _inp(x)
    of, oo, o2 = Out(rows, dim, torch.float32), Out(rows, dim, op, seg=seg1), Out(len(r.keep2), dim, op, seg=seg2)
    assert o2.rows == (rows if group == 0 else 3 * (11 - skip))
    hip.layernorm(xin, ld, rows, dim, *_dev(w, b), L.EPS, out_op=oo.buf, ld_op=oo.ld, out_f32=of.buf, ld_f32=of.ld, split_seg=seg1,
                  weight2=w2.to(DEV), bias2=b2.to(DEV), out2_op=o2.buf, ld2_op=o2.ld, out2_group=group, out2_skip=skip, split_seg2=seg2)
    _check_pair(of, oo, r, w, op, f"main output beside a second one, dim {dim}")
    _check_forms_of(oo, of.cpu()[:, :dim], op, "main output")
    _check_forms_ref(o2, r.out2, L.budget(r, w2, r.pre2, rows=r.keep2), op, f"second output dim {dim} group {group} skip {skip} {form2}")
    for o in (of, oo, o2):
        o.guards_untouched(f"second output dim {dim} group {group} skip {skip} {form2}")


@pytest.mark.parametrize("dim", [384, 768])
def test_second_output_alone(hip, dim):
    """out_op and out_f32 both null: the argument check permits a launch whose only store is the second output."""
    op = hip.operand_dtype()
    rows = 22
    x = L.family("offset_1e3", rows, dim)
    (w, b), (w2, b2) = L.gain_bias(dim), L.gain_bias(dim, 1)
    r = L.ref64(x, dim, w, b, L.EPS, rows, w2=w2, b2=b2, out2_group=11, out2_skip=1)
    xin, ld = _inp(x)
    o2 = Out(len(r.keep2), dim, op, seg=dim + 8)
    hip.layernorm(xin, ld, rows, dim, *_dev(w, b), L.EPS, weight2=w2.to(DEV), bias2=b2.to(DEV), out2_op=o2.buf, ld2_op=o2.ld, out2_group=11, out2_skip=1,
                  split_seg2=dim + 8)
    _check_forms_ref(o2, r.out2, L.budget(r, w2, r.pre2, rows=r.keep2), op, f"second output alone, dim {dim}")
    o2.guards_untouched("second output alone")


# =====================================================================================================================
# g. padded map and ReLU modes
# =====================================================================================================================
@pytest.mark.parametrize("relu", [0, 1, 2])
@pytest.mark.parametrize("dim", [128, 768])
def test_padded_map_and_relu_modes(hip, dim, relu):
    op = hip.operand_dtype()
    B, H, W_ = 3, 4, 5
    rows = B * H * W_
    x = L.family("gauss", rows, dim)
    w, b = L.gain_bias(dim)
    r = L.ref64(x, dim, w, b, L.EPS, rows, relu=relu)
    assert bool((r.pre < 0).any()) and (relu == 0 or float(r.op.min()) == 0.0)
    xin, ld = _inp(x)
    of, oo = Out(rows, dim, torch.float32), Out(B * (H + 2) * (W_ + 2), dim, op)
    hip.layernorm(xin, ld, rows, dim, *_dev(w, b), L.EPS, out_op=oo.buf, ld_op=oo.ld, map_op=hip.MAP_PAD, map_h=H, map_w=W_, relu=relu,
                  out_f32=of.buf, ld_f32=of.ld)
    m = torch.arange(rows)
    inner = ((m // (H * W_)) * (H + 2) + (m % (H * W_)) // W_ + 1) * (W_ + 2) + m % W_ + 1
    bud = L.budget(r, w, r.pre)
    got_f, got_o = of.cpu()[:rows, :dim], oo.cpu()[inner][:, :dim]
    assert_within(got_f, r.f32, bud, None, f"relu {relu} fp32 copy")
    assert_within(got_o, r.op, bud, op, f"relu {relu} padded operand copy")
    if relu == 2:
        assert float(got_f.min()) < 0.0 and float(got_o.float().min()) == 0.0, "relu = 2: the fp32 copy is the pre-activation, the operand copy is clamped"
        assert_bits(got_o, rne(got_f.double().clamp_min(0), op), "relu = 2: operand copy == rne(max(fp32 copy, 0))")
    else:
        assert_bits(got_o, rne(got_f.double(), op), "operand copy == rne(fp32 copy)")
        assert (float(got_f.min()) == 0.0) == (relu == 1)
    of.guards_untouched("fp32")
    oo.guards_untouched("padded operand copy: border", written=inner)


# =====================================================================================================================
# h. normalising un-shuffle
# =====================================================================================================================
@pytest.mark.parametrize("dim", [48, 516])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_normalising_unshuffle_with_ring_subtraction(hip, s, dim):
    op = hip.operand_dtype()
    B, H, W_ = 2, 2, 3
    fh, fw = s * H, s * W_
    rows, N = B * fh * fw, s * s * dim
    g = torch.Generator().manual_seed(500 + 10 * s + dim)
    x = 3.0 * torch.randn(B * H * W_, N, generator=g) + 0.5
    tapb = 0.5 * torch.randn(N, 9, generator=g)
    w, b = L.gain_bias(dim)
    r = L.ref64(x, dim, w, b, L.EPS, rows, unshuffle_s=s, grid=(fh, fw), tap_bias=tapb)
    xin, ld = _inp(x)
    of, oo = Out(rows, dim, torch.float32), Out(rows, dim, op)
    hip.layernorm(xin, ld, rows, dim, *_dev(w, b), L.EPS, out_op=oo.buf, ld_op=oo.ld, out_f32=of.buf, ld_f32=of.ld, map_h=fh, map_w=fw, unshuffle_s=s,
                  tap_bias=tapb.to(DEV))
    bud = L.budget(r, w, r.pre)
    ring = r.ntap.view(-1) > 0
    assert int(ring.sum()) == B * (fh * fw - max(fh - 2, 0) * max(fw - 2, 0))
    got_f, got_o = of.cpu()[:rows, :dim].double(), oo.cpu()[:rows, :dim].double()
    if bool((~ring).any()):
        assert_within(got_f[~ring], r.f32[~ring], bud[~ring], None, f"s {s} dim {dim}: interior pixels (gather only), fp32")
        assert_within(got_o[~ring], r.op[~ring], bud[~ring], op, f"s {s} dim {dim}: interior pixels (gather only), operand")
    assert_within(got_f[ring], r.f32[ring], bud[ring], None, f"s {s} dim {dim}: ring pixels (tap_bias subtraction), fp32")
    assert_within(got_o[ring], r.op[ring], bud[ring], op, f"s {s} dim {dim}: ring pixels (tap_bias subtraction), operand")
    of.guards_untouched("fp32")
    oo.guards_untouched("operand")


# =====================================================================================================================
# i. non-finite rows stay in their row
# =====================================================================================================================
@pytest.mark.parametrize("dim", [128, 768])
def test_non_finite_rows_stay_in_their_row(hip, dim):
    x = L.family("gauss", ROWS, dim)
    w, b = _dev(*L.gain_bias(dim))
    bad = x.clone()
    bad[5, dim // 3] = float("nan")                                # rows 4..7 share a wave of the quarter-wave kernel, rows 8..11 the next
    bad[10, dim - 1] = float("inf")
    outs = []
    for rows_in in (x, bad):
        xin, ld = _inp(rows_in)
        of = Out(ROWS, dim, torch.float32)
        hip.layernorm(xin, ld, ROWS, dim, w, b, L.EPS, out_f32=of.buf, ld_f32=of.ld)
        of.guards_untouched("fp32")
        outs.append(of.cpu()[:ROWS, :dim])
    clean, got = outs
    assert bool(torch.isfinite(clean).all())
    assert bool(torch.isnan(got[5]).all()), "the row with a NaN is not all-NaN"
    assert bool(torch.isnan(got[10]).all()), "the row with +Inf is not all-NaN"
    others = [i for i in range(ROWS) if i not in (5, 10)]
    assert torch.equal(got[others].view(torch.int32), clean[others].view(torch.int32)), "a non-finite row changed another row's bits"


# =====================================================================================================================
# j. refusals
# =====================================================================================================================
def test_refusals_launch_nothing(hip):
    op = hip.operand_dtype()
    dim, rows = 128, 20
    big = torch.zeros(64, 4 * 1540 + 8, device=DEV)
    w, b = torch.ones(1540, device=DEV), torch.zeros(1540, device=DEV)
    tapb = torch.zeros(16 * 128, 9, device=DEV)
    of, oo, o2 = Out(64, 1540, torch.float32), Out(64, 1540, op), Out(64, 1540, op)
    base = dict(out_op=oo.buf, ld_op=oo.ld, out_f32=of.buf, ld_f32=of.ld)
    second = dict(weight2=w, bias2=b, out2_op=o2.buf, ld2_op=o2.ld)
    cases = {
        "dim 1540": ((big, 1548, rows, 1540), base),
        "dim 6": ((big, 8, rows, 6), base),
        "ld_in not divisible by 4": ((big, dim + 2, rows, dim), base),
        "ld_f32 not divisible by 4": ((big, dim, rows, dim), dict(base, ld_f32=of.ld + 2)),
        "ld_op not divisible by 4": ((big, dim, rows, dim), dict(base, ld_op=oo.ld + 2)),
        "skip == group_in": ((big, dim, rows, dim), dict(base, group_in=5, skip=5)),
        "skip > group_in": ((big, dim, rows, dim), dict(base, group_in=5, skip=7)),
        "second output with group_in": ((big, dim, rows, dim), dict(base, group_in=5, skip=1, **second)),
        "second output with unshuffle_s": ((big, 4 * dim, rows, dim), dict(base, unshuffle_s=2, map_h=2, map_w=10, **second)),
        "identity with a second output": ((big, dim, rows, dim), dict(base, identity=True, **second)),
        "tap_bias without unshuffle_s": ((big, dim, rows, dim), dict(base, tap_bias=tapb)),
        "unshuffle_s = 5": ((big, 25 * dim, 50, dim), dict(base, unshuffle_s=5, map_h=5, map_w=10)),
        "PAD grid that does not divide the rows": ((big, dim, 21, dim), dict(base, map_op=hip.MAP_PAD, map_h=4, map_w=5)),
    }
    for what, (args, kw) in cases.items():
        with pytest.raises(hip.HipExtError) as e:
            hip.layernorm(*args, w, b, L.EPS, **kw)
        assert "rc=" in str(e.value) and "rc=0" not in str(e.value), what
        assert len(hip.load().ada_last_error()) > 0, f"{what}: empty ada_last_error"
    torch.cuda.synchronize()
    for o in (of, oo, o2):
        o.guards_untouched("a refused call stored something", written=torch.arange(0))
