"""Zero-tolerance GPU tests on exactly representable inputs ("Exactness tests"; helpers and input families in tests/_exact.py).

The kernels here are linear up to the activation: with small integers and dyadic fractions every product and partial sum is exact in fp32 whatever
the summation order (assert_exact_budget, checked on the CPU alone by tests/test_exact_inputs_cpu.py), so a correct kernel returns the fp64 result bit
for bit -- and an operand-typed output is that result rounded once, to nearest even (rne).  One wrong element fails a test.  The Gaussian tests of
tests/test_gpu_kernels.py remain the check for summation-order robustness.

The first tests are the premise probe: the matrix instructions themselves must add exactly representable products without losing bits at this span.
Part C checks the non-linear epilogues (GELU, SwiGLU, the sigmoid tail) on exact pre-activations, against the activation's own derived error."""

import pytest
import torch
import torch.nn.functional as F

import _exact as X
from _exact import assert_bits, assert_exact_budget, rne, split_ref
from test_gpu_kernels import TILE_CASES, _check_tile, _pack3, _pad_nhwc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -7.0                                     # fills every output buffer: what a launch must not touch comes back as this
CFGS = TILE_CASES + [(-1, 0)]                    # every forced (tile, main loop) + the heuristic's own choice
SOME = [(-1, 0), (3, 4), (4, 4), (1, 4)]         # the tile subset of the existing split / fp8 tests, for the geometry shapes


def _op(hip):
    return hip.operand_dtype()


def _need_f16(hip):
    if hip.operand_dtype() != torch.float16:
        pytest.skip("the [hi | lo8 | hi8] form and the fp8 correction terms exist for fp16 operands only")


def _run(hip, forced_tile, cfg, variant, pipe4_ok=True, **kw):
    """pipe4_ok=False: a split, wrapped or fp8 A operand must stay on the 8-wave loop even when the generated 4-wave loop is forced (csrc/ada_igemm.hip
    use_pipe4: that loop's scalar A-offset counters assume a monotonic walk) -- the tile code must then be the plain 3."""
    if cfg >= 0:
        forced_tile(cfg, variant)
    hip.igemm(**kw)
    if cfg >= 0 and variant == 16 and not pipe4_ok:
        assert hip.debug_last_tile() == cfg, f"forced variant 16 on an operand the 4-wave loop cannot walk: tile code {hip.debug_last_tile()}, expected the 8-wave loop ({cfg})"
    elif cfg >= 0:
        _check_tile(hip, cfg, variant)


def _padded_a(A, op, pad=64):
    """[M, K] -> device [M, K + pad] operand-typed with a loud value behind K: lda > K, and nothing behind K may be read into the sum."""
    M, K = A.shape
    buf = torch.full((M, K + pad), 1000.0, dtype=op)
    buf[:, :K] = A.to(op)
    return buf.to(DEV), K + pad


def _guarded(M, N, dtype, pad_cols=8, pad_rows=3):
    """Output buffer with guard values behind N and behind M."""
    return torch.full((M + pad_rows, N + pad_cols), GUARD, dtype=dtype, device=DEV)


def _guards_untouched(buf, M, N, what):
    b = buf.float().cpu()
    assert bool((b[:M, N:] == GUARD).all()) and bool((b[M:] == GUARD).all()), f"{what}: guard values behind N / behind M were overwritten"


def _border_zero(padded, what=""):
    b = padded.clone()
    b[:, 1:-1, 1:-1] = 0
    assert float(b.float().abs().max()) == 0.0, what + ": border of the padded grid written"


def _f8_bytes(buf, seg):
    """[..., 2 seg] fp16 storage of a split_seg = -seg row -> (hi fp16 [..., seg], lo8 bytes [..., seg], hi8 bytes [..., seg])"""
    b = buf.cpu().contiguous().view(torch.uint8).reshape(*buf.shape[:-1], 4 * seg)
    return b[..., :2 * seg].contiguous().view(torch.float16), b[..., 2 * seg:3 * seg], b[..., 3 * seg:]


def _check_f8_form(buf, v64, C, seg, what):
    """hi == rne(v), lo8 == e5m2((v - hi) 2^10), hi8 == e5m2(v) (the restatement of tests/test_gpu_f8.py), byte for byte; pad bytes untouched (zero)."""
    hi, lo8, hi8 = _f8_bytes(buf, seg)
    want_hi = rne(v64, torch.float16)
    assert_bits(hi[..., :C], want_hi, what + " hi")
    resid = (v64 - want_hi.double()) * 1024.0
    assert torch.equal(resid.float().double(), resid)
    assert torch.equal(lo8[..., :C], X.e5m2(resid.float())), what + ": lo8 bytes"
    assert torch.equal(hi8[..., :C], X.e5m2(v64.float())), what + ": hi8 bytes"
    for t in (hi[..., C:], lo8[..., C:], hi8[..., C:]):
        assert t.numel() == 0 or float(t.float().abs().max()) == 0.0, what + ": pad written"


def _check_split_form(buf, v64, C, seg, op, what):
    """hi == rne(v), lo == rne(v - hi), hi + lo == v exactly; pad columns untouched (zero)."""
    b = buf.cpu()
    hi, lo = b[..., :C], b[..., seg:seg + C]
    want_hi, want_lo = split_ref(v64, op)
    assert_bits(hi, want_hi, what + " hi")
    assert_bits(lo, want_lo, what + " lo")
    assert torch.equal(hi.double() + lo.double(), v64.double()), what + ": hi + lo != v"
    for a, z in ((C, seg), (seg + C, 2 * seg)):
        if z > a:
            assert float(b[..., a:z].float().abs().max()) == 0.0, what + ": pad columns written"


# =====================================================================================================================
# Premise probe: everything below depends on it
# =====================================================================================================================
@pytest.mark.parametrize("K", [64, 8256])
def test_premise_matrix_instruction_adds_exactly(hip, K):
    """Plain igemm, M = N = 64, no bias, fp32 out: v_mfma_f32_*_f16 / _bf16 on products and partial sums that span at most 21 bits must equal fp64."""
    op = _op(hip)
    f = X.gemm_family(K, 64, 64)
    assert_exact_budget(f["A"], f["W"], unit=f["unit"], ref=f["lin"], what=f"premise K={K}")
    out = torch.full((64, 64), GUARD, device=DEV)
    hip.igemm(M=64, N=64, K=K, A=f["A"].to(op).to(DEV), lda=K, W=f["W"].to(op).to(DEV), flags=0, out_f32=out, ldo_f32=64)
    assert_bits(out, f["lin"], f"premise: plain igemm 64 x 64 x {K}")


def test_premise_f8_matrix_instruction_adds_exactly(hip):
    """The same for v_mfma_scale_f32_16x16x128_f8f6f4 behind f8_from, on hand-built bytes and a fixed scale word."""
    _need_f16(hip)
    f = X.f8_family(64, 64)
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what="premise f8")
    seg = f["seg"]
    A = X.f8_pack(f["a_hi"], f["a_lo8"], f["a_hi8"], torch.float16, torch.float8_e5m2, torch.float8_e5m2)
    W = X.f8_pack(f["w_hi"], f["w_hi8"], f["w_lo8"], torch.float16, torch.float8_e4m3fn, torch.float8_e4m3fn)
    out = torch.full((64, 64), GUARD, device=DEV)
    hip.igemm(M=64, N=64, K=2 * seg, A=A.to(DEV), lda=2 * seg, W=W.to(DEV), flags=0, out_f32=out, ldo_f32=64, f8_from=seg, f8_mid=seg + seg // 2, f8_scales=f["word"])
    assert_bits(out, f["ref"], "premise: f8_from igemm 64 x 64")


# =====================================================================================================================
# Part A -- ada_igemm, bit for bit
# =====================================================================================================================
@pytest.mark.parametrize("cfg,variant", CFGS)
@pytest.mark.parametrize("epi", ["f32_bias", "gamma_res_inplace", "op_plain", "op_gamma", "relu_op_and_f32", "bias_row_mod"])
def test_igemm_exact_epilogues(hip, forced_tile, cfg, variant, epi):
    """M = 3 * 256 + 77, N = 2 * 256 + 64, K = 320 (4 ragged tile rows, a partial last N tile, 5 k-tiles), padded lda / ldo, guards behind N and M."""
    op = _op(hip)
    f = X.gemm_family(320)
    M, N, K = X.GEMM_M, X.GEMM_N, 320
    A, lda = _padded_a(f["A"], op)
    W = f["W"].to(op).to(DEV)
    b, g = f["bias"].to(DEV), f["gamma"].to(DEV)
    lin, b64, g64 = f["lin"], f["bias"].double(), f["gamma"].double()
    assert_exact_budget(f["A"], f["W"], bias=f["bias"], gamma=f["gamma"], residual=f["res"], unit=f["unit_gamma"], what="epilogues")
    kw = dict(M=M, N=N, K=K, A=A, lda=lda, W=W)
    tag = f"tile {cfg}/{variant} {epi}"
    if epi == "f32_bias":
        out = _guarded(M, N, torch.float32)
        _run(hip, forced_tile, cfg, variant, bias=b, flags=hip.EP_BIAS, out_f32=out, ldo_f32=N + 8, **kw)
        assert_bits(out[:M, :N], lin + b64, tag)
        _guards_untouched(out, M, N, tag)
    elif epi == "gamma_res_inplace":
        x = _guarded(M, N, torch.float32)
        x[:M, :N] = f["res"].to(DEV)
        _run(hip, forced_tile, cfg, variant, bias=b, gamma=g, res=x, ldr=N + 8, flags=hip.EP_BIAS | hip.EP_GAMMA | hip.EP_RESIDUAL, out_f32=x, ldo_f32=N + 8, **kw)
        assert_bits(x[:M, :N], (lin + b64) * g64 + f["res"].double(), tag)
        _guards_untouched(x, M, N, tag)
    elif epi == "op_plain":
        out = _guarded(M, N, op)
        _run(hip, forced_tile, cfg, variant, flags=0, out_op=out, ldo_op=N + 8, **kw)
        assert_bits(out[:M, :N], rne(lin, op), tag)
        _guards_untouched(out, M, N, tag)
    elif epi == "op_gamma":
        out = _guarded(M, N, op)
        _run(hip, forced_tile, cfg, variant, bias=b, gamma=g, flags=hip.EP_BIAS | hip.EP_GAMMA, out_op=out, ldo_op=N + 8, **kw)
        assert_bits(out[:M, :N], rne((lin + b64) * g64, op), tag)
        _guards_untouched(out, M, N, tag)
    elif epi == "relu_op_and_f32":
        of, oo = _guarded(M, N, torch.float32), _guarded(M, N, op, pad_cols=4)       # ldo_op % 8 == 4: the 4-column stores
        _run(hip, forced_tile, cfg, variant, bias=b, flags=hip.EP_BIAS | hip.EP_RELU_OP, out_f32=of, ldo_f32=N + 8, out_op=oo, ldo_op=N + 4, **kw)
        assert_bits(of[:M, :N], lin + b64, tag + " f32")
        assert_bits(oo[:M, :N], rne((lin + b64).clamp_min(0), op), tag + " relu op")
        _guards_untouched(of, M, N, tag)
        _guards_untouched(oo, M, N, tag)
    else:
        rows = M // X.BIAS_GROUPS                         # 845 = 5 * 169: one bias vector per group of 169 rows
        bg = X.bias_groups()
        assert_exact_budget(f["A"], f["W"], bias=bg.abs().max(0).values, unit=f["unit"], what="bias_row_mod")
        out = _guarded(M, N, op)
        _run(hip, forced_tile, cfg, variant, bias=bg.to(DEV), bias_row_mod=rows, flags=hip.EP_BIAS, out_op=out, ldo_op=N + 8, **kw)
        assert_bits(out[:M, :N], rne(lin + bg.double().repeat_interleave(rows, dim=0), op), tag)
        _guards_untouched(out, M, N, tag)


@pytest.mark.parametrize("cfg,variant", CFGS)
def test_igemm_exact_long_k(hip, forced_tile, cfg, variant):
    """K = 8256: 129 k-tiles, the long-k main loop.  Left to itself (cfg -1) the launcher takes the generated 4-wave loop for k-loops of >= 128 k-tiles
    whenever it picks the 256 x 256 tile: asserted from the tile code."""
    op = _op(hip)
    f = X.gemm_family(8256)
    M, N, K = X.GEMM_M, X.GEMM_N, 8256
    assert_exact_budget(f["A"], f["W"], bias=f["bias"], unit=f["unit"], ref=f["lin"], what="long k")
    A, lda = _padded_a(f["A"], op)
    out = _guarded(M, N, torch.float32)
    _run(hip, forced_tile, cfg, variant, M=M, N=N, K=K, A=A, lda=lda, W=f["W"].to(op).to(DEV), bias=f["bias"].to(DEV), flags=hip.EP_BIAS, out_f32=out, ldo_f32=N + 8)
    if cfg < 0 and hip.debug_last_tile() % 100 == 3:
        assert hip.debug_last_tile() // 100 == 2, f"K = 8256 on the 256 x 256 tile did not take the 4-wave loop (tile code {hip.debug_last_tile()})"
    assert_bits(out[:M, :N], f["lin"] + f["bias"].double(), f"tile {cfg}/{variant} K=8256")
    _guards_untouched(out, M, N, "long k")


@pytest.mark.parametrize("cfg,variant", CFGS)
@pytest.mark.parametrize("form", ["hi_lo", "f8"])
def test_igemm_exact_split_output_plain(hip, forced_tile, cfg, variant, form):
    """split_seg > 0: hi == rne(v), lo == rne(v - hi), hi + lo == v.  split_seg < 0: hi, and the lo8 / hi8 bytes == e5m2((v - hi) 2^10), e5m2(v).
    Through the fp32 + operand-copy epilogue (residual: 4-column stores) and the operand-only one (8-column stores)."""
    op = _op(hip)
    if form == "f8":
        _need_f16(hip)
    f = X.gemm_family(320)
    M, N, K, seg = X.GEMM_M, X.GEMM_N, 320, X.GEMM_N + 64
    sign = 1 if form == "hi_lo" else -1
    check = (lambda buf, v, what: _check_split_form(buf, v, N, seg, op, what)) if form == "hi_lo" else (lambda buf, v, what: _check_f8_form(buf, v, N, seg, what))
    A, lda = _padded_a(f["A"], op)
    W, b = f["W"].to(op).to(DEV), f["bias"].to(DEV)
    assert_exact_budget(f["A"], f["W"], bias=f["bias"], residual=f["res"], unit=f["unit"], what="split outputs")
    kw = dict(M=M, N=N, K=K, A=A, lda=lda, W=W, bias=b)
    o = torch.zeros(M, 2 * seg, dtype=op, device=DEV)
    of = _guarded(M, N, torch.float32)
    _run(hip, forced_tile, cfg, variant, res=f["res"].to(DEV), ldr=N, flags=hip.EP_BIAS | hip.EP_RESIDUAL, out_f32=of, ldo_f32=N + 8, out_op=o, ldo_op=2 * seg, split_seg=sign * seg, **kw)
    v = f["lin"] + f["bias"].double() + f["res"].double()
    assert_bits(of[:M, :N], v, f"tile {cfg}/{variant} split {form}: fp32 copy")
    check(o, v, f"tile {cfg}/{variant} split {form}, fp32 + operand copy")
    o2 = torch.zeros(M, 2 * seg, dtype=op, device=DEV)
    _run(hip, forced_tile, cfg, variant, flags=hip.EP_BIAS | hip.EP_RELU_OP, out_op=o2, ldo_op=2 * seg, split_seg=sign * seg, **kw)
    check(o2, (f["lin"] + f["bias"].double()).clamp_min(0), f"tile {cfg}/{variant} split {form}, operand only")


@pytest.mark.parametrize("cfg,variant", SOME)
@pytest.mark.parametrize("form", ["hi_lo", "f8"])
def test_igemm_exact_split_output_pad_and_shuffle(hip, forced_tile, cfg, variant, form):
    """The split forms behind the padded and the shuffled map, at the smallest shapes of the existing tests for those maps and on their tile subset
    (heuristic, 256 x 256, 128 x 128, 128 x 64): the stores are the plain map's, which runs over every tile above; what differs is the row arithmetic."""
    op = _op(hip)
    if form == "f8":
        _need_f16(hip)
    sign = 1 if form == "hi_lo" else -1
    # PAD: 3x3 convolution writing a split, zero-bordered NHWC output + its fp32 copy
    B, C, H, W_ = 2, 64, 13, 17
    c = X.split_pad_family(B, C, H, W_)
    v = c["ref"]
    assert_exact_budget(mag=c["mag"], unit=c["unit"], ref=v, what="split pad")
    o = torch.zeros(B, H + 2, W_ + 2, 2 * C, dtype=op, device=DEV)
    of = torch.full((B * H * W_, C), GUARD, device=DEV)
    _run(hip, forced_tile, cfg, variant, M=B * H * W_, N=C, K=9 * C, A=_pad_nhwc(c["x"], C, op).to(DEV), lda=C, W=_pack3(c["w"], C, op).to(DEV), a_mode=hip.A_CONV3,
         conv=(H, W_, H + 2, W_ + 2, 1), bias=c["bias"].to(DEV), flags=hip.EP_BIAS | hip.EP_RELU_OP, out_f32=of, ldo_f32=C, out_op=o, ldo_op=2 * C, map_op=hip.MAP_PAD,
         map_h=H, map_w=W_, split_seg=sign * C)
    assert_bits(of.view(B, H, W_, C), v, f"tile {cfg} split pad: fp32 copy")
    if form == "hi_lo":
        _check_split_form(o[:, 1:-1, 1:-1], v.clamp_min(0), C, C, op, f"tile {cfg} split pad")
    else:
        _check_f8_form(o[:, 1:-1, 1:-1], v.clamp_min(0), C, C, f"tile {cfg} f8 pad")
    _border_zero(o, "split pad")
    # SHUFFLE: ConvTranspose2d k = s = 2 as a GEMM + pixel shuffle
    s_, Co, Ci, h, w_ = X.SPLIT_SHUFFLE_CASE
    segc = 64
    f = X.shuffle_family(s_, Co, Ci, h, w_)
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what="split shuffle")
    o = torch.zeros(B, s_ * h + 2, s_ * w_ + 2, 2 * segc, dtype=op, device=DEV)
    _run(hip, forced_tile, cfg, variant, M=B * h * w_, N=s_ * s_ * Co, K=f["cp"], A=f["A"].to(op).to(DEV), lda=f["cp"], W=f["Wp"].to(op).to(DEV), bias=f["bias"].to(DEV),
         flags=hip.EP_BIAS, out_op=o, ldo_op=2 * segc, map_op=hip.MAP_SHUFFLE, map_h=h, map_w=w_, shuffle_s=s_, shuffle_c=Co, split_seg=sign * segc)
    if form == "hi_lo":
        _check_split_form(o[:, 1:-1, 1:-1], f["ref"], Co, segc, op, f"tile {cfg} split shuffle")
    else:
        _check_f8_form(o[:, 1:-1, 1:-1], f["ref"], Co, segc, f"tile {cfg} f8 shuffle")
    _border_zero(o, "split shuffle")


@pytest.mark.parametrize("cfg,variant", CFGS)
def test_igemm_exact_a_dup_seg(hip, forced_tile, cfg, variant):
    """The k-walk (hi, lo, hi) of a split A operand against [w_hi | w_hi | w_lo]: x_hi w_hi + x_lo w_hi + x_hi w_lo of independent exact pieces."""
    op = _op(hip)
    M, N, seg = 300, 200, 128
    f = X.a_dup_family(M, N, seg)
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what="a_dup_seg")
    A = torch.cat([f["hi"], f["lo"]], 1).to(op).contiguous().to(DEV)
    out = _guarded(M, N, torch.float32)
    _run(hip, forced_tile, cfg, variant, pipe4_ok=False, M=M, N=N, K=3 * seg, A=A, lda=2 * seg, a_dup_seg=seg, W=f["w3"].to(op).contiguous().to(DEV), bias=f["bias"].to(DEV),
         flags=hip.EP_BIAS, out_f32=out, ldo_f32=N + 8)
    assert_bits(out[:M, :N], f["ref"], f"tile {cfg}/{variant} a_dup_seg")
    _guards_untouched(out, M, N, "a_dup_seg")


@pytest.mark.parametrize("cfg,variant", CFGS)
def test_igemm_exact_a_wrap(hip, forced_tile, cfg, variant):
    """Weight-only split: the A walk starts over at k = a_wrap against [w_hi | w_lo]: x w_hi + x w_lo of independent exact pieces."""
    op = _op(hip)
    M, N, K = 300, 200, 128
    f = X.a_wrap_family(M, N, K)
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what="a_wrap")
    A, lda = _padded_a(f["x"], op)
    out = _guarded(M, N, torch.float32)
    _run(hip, forced_tile, cfg, variant, pipe4_ok=False, M=M, N=N, K=2 * K, A=A, lda=lda, a_wrap=K, W=f["w2"].to(op).contiguous().to(DEV), bias=f["bias"].to(DEV),
         flags=hip.EP_BIAS, out_f32=out, ldo_f32=N + 8)
    assert_bits(out[:M, :N], f["ref"], f"tile {cfg}/{variant} a_wrap")
    _guards_untouched(out, M, N, "a_wrap")


@pytest.mark.parametrize("cfg,variant", CFGS)
def test_igemm_exact_f8_from(hip, forced_tile, cfg, variant):
    """Hand-built [hi | lo8 | hi8] rows against [w_hi | w_hi8 | w_lo8] with a fixed scale word: the contraction of the decoded pieces, exactly."""
    _need_f16(hip)
    M, N = 300, 200
    f = X.f8_family(M, N)
    seg = f["seg"]
    b = X.f8_bias()
    assert_exact_budget(mag=f["mag"], bias=b, unit=f["unit"], ref=f["ref"] + b.double(), what="f8_from")
    A = X.f8_pack(f["a_hi"], f["a_lo8"], f["a_hi8"], torch.float16, torch.float8_e5m2, torch.float8_e5m2)
    W = X.f8_pack(f["w_hi"], f["w_hi8"], f["w_lo8"], torch.float16, torch.float8_e4m3fn, torch.float8_e4m3fn)
    out = _guarded(M, N, torch.float32)
    _run(hip, forced_tile, cfg, variant, pipe4_ok=False, M=M, N=N, K=2 * seg, A=A.to(DEV), lda=2 * seg, W=W.to(DEV), bias=b.to(DEV), flags=hip.EP_BIAS, out_f32=out,
         ldo_f32=N + 8, f8_from=seg, f8_mid=seg + seg // 2, f8_scales=f["word"])
    assert_bits(out[:M, :N], f["ref"] + b.double(), f"tile {cfg}/{variant} f8_from")
    _guards_untouched(out, M, N, "f8_from")


# ---- geometry -------------------------------------------------------------------------------------------------------------------
SMALL_TILES = [(0, 4), (1, 4), (-1, 0)]            # the narrow tiles + the heuristic's own choice, for shapes too small for the wide tiles
WIDE_TILES = [(2, 4), (3, 4), (3, 16), (4, 4)]
CONV_RES_RUNS = [(c, t) for c in X.CONV_RES_CASES for t in SMALL_TILES] + [(X.CONV_RES_WIDE_CASE, t) for t in WIDE_TILES]


@pytest.mark.parametrize("case,tile", CONV_RES_RUNS)
def test_igemm_exact_conv3x3_padded_output_and_residual(hip, forced_tile, case, tile):
    """The padded-grid row map and the residual addresses on every tile shape: interior and edge tiles of each (the wide case: M = 272 rows)."""
    (B, C, H, W_, Co, stride), (cfg, variant) = case, tile
    op = _op(hip)
    c = X.conv_res_family(B, C, H, W_, Co, stride)
    Ho, Wo, v = c["Ho"], c["Wo"], c["ref"]
    assert_exact_budget(mag=c["mag"], unit=c["unit"], ref=v, what="conv3x3")
    of = torch.full((B * Ho * Wo, Co), GUARD, device=DEV)
    op_ = torch.zeros(B, Ho + 2, Wo + 2, Co, dtype=op, device=DEV)
    _run(hip, forced_tile, cfg, variant, M=B * Ho * Wo, N=Co, K=9 * C, A=_pad_nhwc(c["x"], C, op).to(DEV), lda=C, W=_pack3(c["w"], C, op).to(DEV), a_mode=hip.A_CONV3,
         conv=(Ho, Wo, H + 2, W_ + 2, stride), bias=c["bias"].to(DEV), res=c["res"].to(DEV), ldr=Co, flags=hip.EP_BIAS | hip.EP_RESIDUAL | hip.EP_RELU_OP,
         out_f32=of, ldo_f32=Co, out_op=op_, ldo_op=Co, map_op=hip.MAP_PAD, map_h=Ho, map_w=Wo)
    assert_bits(of, v, f"conv3x3 stride {stride} f32")
    assert_bits(op_[:, 1:-1, 1:-1].reshape(-1, Co), rne(v.clamp_min(0), op), f"conv3x3 stride {stride} relu padded")
    _border_zero(op_, "conv3x3")


@pytest.mark.parametrize("cfg,variant", SMALL_TILES)
def test_igemm_exact_token_map_with_pos(hip, forced_tile, cfg, variant):
    op = _op(hip)
    B, Np, D, K = X.TOKEN_MAP_CASE
    f = X.token_map_family(B, Np, D, K)
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what="token map")
    x = torch.full((B * (Np + 1), D), GUARD, device=DEV)
    _run(hip, forced_tile, cfg, variant, M=B * Np, N=D, K=K, A=f["A"].to(op).to(DEV), lda=K, W=f["W"].to(op).to(DEV), bias=f["bias"].to(DEV), res=f["pos"].to(DEV), ldr=D,
         res_row_mod=Np, res_row_off=1, flags=hip.EP_BIAS | hip.EP_RESIDUAL, out_f32=x, ldo_f32=D, map_f32=hip.MAP_TOKEN, map_h=Np)
    got = x.reshape(B, Np + 1, D).cpu()
    assert_bits(got[:, 1:], f["ref"], "token map")
    assert bool((got[:, 0] == GUARD).all()), "cls rows written"


@pytest.mark.parametrize("s,C,Ci,H,W_", X.SHUFFLE_CASES)
def test_igemm_exact_conv_transpose_shuffle(hip, s, C, Ci, H, W_):
    op = _op(hip)
    B = 2
    f = X.shuffle_family(s, C, Ci, H, W_)
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what="shuffle")
    out = torch.zeros(B, s * H + 2, s * W_ + 2, C, dtype=op, device=DEV)
    hip.igemm(M=B * H * W_, N=s * s * C, K=f["cp"], A=f["A"].to(op).to(DEV), lda=f["cp"], W=f["Wp"].to(op).to(DEV), bias=f["bias"].to(DEV), flags=hip.EP_BIAS,
              out_op=out, ldo_op=C, map_op=hip.MAP_SHUFFLE, map_h=H, map_w=W_, shuffle_s=s, shuffle_c=C)
    assert_bits(out[:, 1:-1, 1:-1], rne(f["ref"], op), f"conv transpose s={s}")
    _border_zero(out, "shuffle")


@pytest.mark.parametrize("s,Ci,Co,H,W_,cfg", X.SUBPIXEL_CASES)
def test_igemm_exact_subpixel_tap_walk(hip, forced_tile, s, Ci, Co, H, W_, cfg):
    """tap_cols / tap_mask: the k-loop of an N-tile walks the union of its phases' taps only.  The weights are dyadic in the taps a phase touches and
    zero elsewhere (as the packer leaves them), so the masked walk must equal the full 3x3 convolution over the coarse grid."""
    op = _op(hip)
    B = 2
    cp = (Ci + 63) // 64 * 64
    N = s * s * Co
    f = X.subpixel_family(s, Ci, Co, H, W_)
    assert sum(bin(m).count("1") for m in f["masks"]) == (36 if s == 4 else 16)
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what="sub-pixel")
    wp = torch.zeros(N, 9, cp)
    wp[..., :Ci] = f["wm"]
    out = torch.full((B * H * W_, N), GUARD, device=DEV)
    _run(hip, forced_tile, cfg, 0, M=B * H * W_, N=N, K=9 * cp, A=_pad_nhwc(f["x"], cp, op).to(DEV), lda=cp, W=wp.reshape(N, 9 * cp).to(op).to(DEV), a_mode=hip.A_CONV3,
         conv=(H, W_, H + 2, W_ + 2, 1), bias=f["bias"].to(DEV), flags=hip.EP_BIAS, out_f32=out, ldo_f32=N, tap_cols=Co, tap_mask=f["masks"])
    assert_bits(out, f["ref"], f"sub-pixel tap walk s={s} tile {cfg}")


def _tail_budget(f, what):
    assert_exact_budget(mag=f["conv_mag"], unit=f["conv_unit"], ref=f["conv"], what=what + " conv")
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what=what + " dot")


@pytest.mark.parametrize("act", ["none", "relu"])
def test_igemm_exact_tail(hip, act):
    op = _op(hip)
    f = X.tail_family(False)
    _tail_budget(f, "tail")
    x, d = f["x"], f["ref"]
    B, C, H, W_ = x.shape
    out = torch.full((B, 1, H, W_), GUARD, device=DEV)
    hip.igemm(M=B * H * W_, N=32, K=9 * C, A=_pad_nhwc(x, C, op).to(DEV), lda=C, W=_pack3(f["w"], C, op).to(DEV), a_mode=hip.A_CONV3, conv=(H, W_, H + 2, W_ + 2, 1),
              bias=f["bias"].to(DEV), flags=hip.EP_BIAS | hip.EP_TAIL, out_f32=out, ldo_f32=1, tail_w=f["tw"].to(DEV), tail_b=0.25,
              tail_act=hip.ACT_RELU if act == "relu" else hip.ACT_NONE)
    assert float((d < 0).double().mean()) > 0.1
    assert_bits(out, d.clamp_min(0) if act == "relu" else d, f"tail {act}")


def test_igemm_exact_saturation(hip):
    """One column block's exact result is > 65504, one is < -65504: fp16 stores are exactly +-65504 with lo = to_op(v - hi), and count_saturated counts
    exactly those elements; bf16 has the range: rne(v), nothing counted."""
    op = _op(hip)
    M, N, K = 300, 128, 64
    f = X.saturation_family(M, N, K)
    v = f["ref"]
    assert_exact_budget(f["A"], f["W"], unit=f["unit"], ref=v, what="saturation")
    A, W = f["A"].to(op).to(DEV), f["W"].to(op).to(DEV)
    out = torch.zeros(M, N, dtype=op, device=DEV)
    hip.igemm(M=M, N=N, K=K, A=A, lda=K, W=W, flags=0, out_op=out, ldo_op=N)
    assert_bits(out, rne(v, op), "saturating store")
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    hip.count_saturated(out, counter)
    assert int(counter.item()) == (M * 80 if op == torch.float16 else 0)
    two = torch.zeros(M, 2 * N, dtype=op, device=DEV)
    hip.igemm(M=M, N=N, K=K, A=A, lda=K, W=W, flags=0, out_op=two, ldo_op=2 * N, split_seg=N)
    hi, lo = split_ref(v, op)
    assert_bits(two[:, :N], hi, "saturating store, hi")
    assert_bits(two[:, N:], lo, "saturating store, lo = to_op(v - hi)")
    if op == torch.float16:
        assert torch.equal(two[:, :40].float().cpu(), torch.full((M, 40), 65504.0)) and torch.equal(two[:, 40:80].float().cpu(), torch.full((M, 40), -65504.0))


# =====================================================================================================================
# Part B -- kernels without a matrix instruction, bit for bit
# =====================================================================================================================
@pytest.mark.parametrize("C,hi,wi,ho,wo", X.BILINEAR_CASES)
def test_bilinear_exact(hip, C, hi, wi, ho, wo):
    """Scales 1/2, 1/4, 1/8 on integer maps.  128 channels at 19 x 19 -> 37 x 73 take the LDS-tiled kernel; 128 channels with wo = 13 < 16 are a shape
    the tiled path rejects: the per-pixel kernel on wide rows."""
    op = _op(hip)
    B = 2
    f = X.bilinear_family(C, hi, wi, ho, wo)
    add, up, v = f["add"], f["up"], f["ref"]
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=v, what="bilinear")
    xin = f["x"].permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(DEV)
    # add + fp32 + ReLU'd padded operand copy
    of = torch.full((B * ho * wo, C), GUARD, device=DEV)
    oo = torch.zeros(B, ho + 2, wo + 2, C, dtype=op, device=DEV)
    hip.bilinear(xin, C, B, hi, wi, ho, wo, C, add=add.to(DEV), ld_add=C, out_f32=of, ld_f32=C, out_op=oo, ld_op=C, map_op=hip.MAP_PAD, relu=True)
    assert_bits(of, v, "bilinear + add, f32")
    assert_bits(oo[:, 1:-1, 1:-1].reshape(-1, C), rne(v.clamp_min(0), op), "bilinear + add, relu padded")
    _border_zero(oo, "bilinear")
    # fp32 only, no add
    of2 = torch.full((B * ho * wo, C), GUARD, device=DEV)
    hip.bilinear(xin, C, B, hi, wi, ho, wo, C, out_f32=of2, ld_f32=C)
    assert_bits(of2, up, "bilinear f32 only")
    # plain operand output, [hi | lo]
    o2 = torch.zeros(B * ho * wo, 2 * C, dtype=op, device=DEV)
    hip.bilinear(xin, C, B, hi, wi, ho, wo, C, add=add.to(DEV), ld_add=C, out_op=o2, ld_op=2 * C, map_op=hip.MAP_PLAIN, split_seg=C)
    _check_split_form(o2, v, C, C, op, "bilinear split")
    if op == torch.float16:       # [hi | lo8 | hi8] into a padded grid
        o3 = torch.zeros(B, ho + 2, wo + 2, 2 * C, dtype=op, device=DEV)
        hip.bilinear(xin, C, B, hi, wi, ho, wo, C, add=add.to(DEV), ld_add=C, out_op=o3, ld_op=2 * C, map_op=hip.MAP_PAD, relu=True, split_seg=-C)
        _check_f8_form(o3[:, 1:-1, 1:-1].reshape(-1, 2 * C), v.clamp_min(0), C, C, "bilinear f8 form")
        _border_zero(o3, "bilinear f8")


@pytest.mark.parametrize("B,C,Cin,hi,wi,ho,wo", X.TAPSUM_CASES)
@pytest.mark.parametrize("tmap", ["f32", "op"])
def test_tapsum_resize_exact(hip, B, C, Cin, hi, wi, ho, wo, tmap):
    """The nine integer tap maps W_t u (built on the host: no matrix instruction) gathered by ada_tapsum_resize_fwd == conv3x3(upsample(u)) in fp64;
    wo = 33 and 65 are right-edge widths of the halo test."""
    op = _op(hip)
    f = X.tapsum_family(B, C, Cin, hi, wi, ho, wo)
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what="tap-sum")
    Tdev = f["T"].to(op if tmap == "op" else torch.float32).contiguous().to(DEV)
    out = torch.full((B * ho * wo, C), GUARD, device=DEV)
    hip.tapsum_resize(Tdev, 9 * C, B, hi, wi, ho, wo, C, f["bias"].to(DEV), out, C)
    assert_bits(out, f["ref"], f"tap-sum resize {tmap}")


@pytest.mark.parametrize("B,C,hi,wi,ho,wo", X.DPT_TAIL_CASES)
@pytest.mark.parametrize("act", ["none", "relu"])
def test_dpt_tail_exact(hip, B, C, hi, wi, ho, wo, act):
    """x2 and x4 up-sampling of an integer map, dyadic 3x3 weights, bias and tail_w.  The last case has 594 tiles of two channel passes: every one of the
    <= 256 persistent workgroups walks several (tile, pass) units through its two halo buffers."""
    op = _op(hip)
    f = X.dpt_tail_family(B, C, hi, wi, ho, wo)
    _tail_budget(f, "fused tail")
    d = f["ref"]
    xin = f["x"].permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(DEV)
    out = torch.full((B, ho, wo), GUARD, device=DEV)
    hip.dpt_tail(xin, C, B, hi, wi, ho, wo, C, _pack3(f["w"], C, op).to(DEV), f["bias"].to(DEV), f["tw"].to(DEV), 0.25, hip.ACT_RELU if act == "relu" else hip.ACT_NONE, out)
    assert float((d < 0).double().mean()) > 0.05
    assert_bits(out, d.clamp_min(0) if act == "relu" else d, f"fused tail {act}")


@pytest.mark.parametrize("s,dim,H,W_", X.UNSHUFFLE_CASES)
def test_layernorm_identity_unshuffle_exact(hip, s, dim, H, W_):
    """ada_layernorm_ex with identity = 1: the un-shuffle pass behind a sub-pixel convolution, with tap_bias and the ring subtraction, against an fp64
    restatement of the index arithmetic.  dim = 640 takes the one-wave-per-row kernel."""
    op = _op(hip)
    B = 2
    N = s * s * dim
    f = X.unshuffle_family(s, dim, H, W_)
    fh, fw, fine = f["fh"], f["fw"], f["ref"]
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=fine, what="un-shuffle")
    inp, tapb = f["inp"].to(DEV), f["tapb"].to(DEV)
    rows = B * fh * fw
    outp = torch.zeros(B, fh + 2, fw + 2, dim, dtype=op, device=DEV)
    outf = torch.full((rows, dim), GUARD, device=DEV)
    hip.layernorm(inp, N, rows, dim, None, None, 1e-6, identity=True, relu=2, out_f32=outf, ld_f32=dim, out_op=outp, ld_op=dim, map_op=hip.MAP_PAD,
                  map_h=fh, map_w=fw, unshuffle_s=s, tap_bias=tapb)
    assert_bits(outf.view(B, fh, fw, dim), fine, "re-layout pass, fp32 copy")
    assert_bits(outp[:, 1:-1, 1:-1], rne(fine.clamp_min(0), op), "re-layout pass, ReLU'd padded operand copy")
    _border_zero(outp, "un-shuffle")
    plain = torch.full((rows, dim), GUARD, dtype=op, device=DEV)
    hip.layernorm(inp, N, rows, dim, None, None, 1e-6, identity=True, relu=0, out_op=plain, ld_op=dim, map_h=fh, map_w=fw, unshuffle_s=s, tap_bias=tapb)
    assert_bits(plain.view(B, fh, fw, dim), rne(fine, op), "re-layout pass, plain operand output")


@pytest.mark.parametrize("cg", [0, 2, 5])
@pytest.mark.parametrize("norm", [False, True])
def test_patchify_exact(hip, cg, norm):
    """Pixels k / 16384 (14 bits: the operand type rounds them), dyadic mean and power-of-two inv_std: (x - mean) * inv_std is exact in fp32."""
    op = _op(hip)
    B, H, W_ = 2, 42, 56
    f = X.patchify_family(cg, norm, B, H, W_)
    x, g, K, ref = f["x"].to(DEV), f["g"].to(DEV) if cg else None, f["K"], f["ref"]
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=ref, what="patchify")       # no sum at all: the single value, in units of 2^-14
    mean, inv_std = (X.PATCHIFY_MEAN, X.PATCHIFY_INV_STD) if norm else (None, None)
    ld = (K + 63) // 64 * 64 + 64
    out = torch.full((B * 12, ld), 7.0, dtype=op, device=DEV)
    hip.patchify(x, g, B, cg, H, W_, mean, inv_std, out, ld)
    assert_bits(out[:, :K], rne(ref, op), "patchify")
    assert float(out[:, K:].float().abs().max()) == 0.0, "columns behind K must be exactly 0"
    seg = ld
    two = torch.full((B * 12, 2 * seg), 7.0, dtype=op, device=DEV)
    hip.patchify(x, g, B, cg, H, W_, mean, inv_std, two, 2 * seg, split=True)
    _check_split_form(two, ref, K, seg, op, "patchify split")


@pytest.mark.parametrize("B,H,W_", X.DEPTH_STATS_CASES)
def test_depth_stats_exact(hip, B, H, W_):
    """s = k / 16, z = k / 4: s (1 - s) = k (16 - k) / 256 and every chunk sum are exact; each chunk's pair must equal fp64, all three activations."""
    f = X.depth_stats_family(B, H, W_)
    for m, u, r in f["budgets"]:
        assert_exact_budget(mag=m, unit=u, ref=r, what="depth stats")
    s, z, ref = f["s"], f["z"], f["ref"]
    sums = torch.full((B, X.DEPTH_STATS_CHUNKS, 2), float("nan"), device=DEV)
    hip.depth_stats(s.to(DEV), sums)
    assert_bits(sums, ref["sigmoid"], "depth stats, sigmoid")
    hip.depth_stats(z.clamp_min(0).to(DEV), sums, hip.ACT_RELU)
    assert_bits(sums, ref["relu"], "depth stats, relu")
    hip.depth_stats(z.to(DEV), sums, hip.ACT_NONE)
    assert_bits(sums, ref["none"], "depth stats, none")


@pytest.mark.parametrize("B,Np,D,ld", X.TOKEN_CASES)
def test_token_diversity_sums_exact(hip, B, Np, D, ld):
    """Integer tokens and a power-of-two token count: column means, mean squares and variances are dyadic, their 64-column sums exact."""
    op = _op(hip)
    f = X.token_family(B, Np, D, ld)
    assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what="token diversity")
    sums = torch.full((B, f["G"], 2), float("nan"), device=DEV)
    hip.token_diversity(f["t"].to(op).reshape(B * Np, ld).contiguous().to(DEV), ld, B, Np, D, sums)
    assert_bits(sums, f["ref"], "token diversity")


# =====================================================================================================================
# Part C -- non-linear epilogues at their own accuracy: exact pre-activation, |got - ref64| <= ulp_op(ref64) / 2 + e_act
# =====================================================================================================================
@pytest.mark.parametrize("cfg,variant", CFGS)
def test_igemm_gelu_on_exact_preactivation(hip, forced_tile, cfg, variant):
    op = _op(hip)
    M, N, K = X.GEMM_M, X.GEMM_N, 64
    f = X.nonlinear_family(M, N)
    assert_exact_budget(f["A"], f["W"], bias=f["bias"], unit=f["unit"], ref=f["pre"], what="gelu pre-activation")
    assert float(f["pre"].abs().max()) <= 16.0
    out = _guarded(M, N, op)
    _run(hip, forced_tile, cfg, variant, M=M, N=N, K=K, A=f["A"].to(op).to(DEV), lda=K, W=f["W"].to(op).to(DEV), bias=f["bias"].to(DEV), flags=hip.EP_BIAS | hip.EP_GELU,
         out_op=out, ldo_op=N + 8)
    ref = F.gelu(f["pre"])
    X.assert_within(out[:M, :N], ref, X.e_act_gelu(ref), op, f"gelu tile {cfg}/{variant}")
    _guards_untouched(out, M, N, "gelu")


def test_igemm_swiglu_on_exact_preactivation(hip):
    op = _op(hip)
    M, N, K = X.GEMM_M, X.GEMM_N, 64
    f = X.nonlinear_family(M, N)
    assert_exact_budget(f["A"], f["W"], bias=f["bias"], unit=f["unit"], ref=f["pre"], what="swiglu pre-activation")
    pre = f["pre"].view(M, N // 64, 2, 32)                 # columns come in (x1, x2) 32-wide groups
    assert float(pre.abs().max()) <= 16.0
    ref = (F.silu(pre[:, :, 0]) * pre[:, :, 1]).reshape(M, N // 2)
    out = _guarded(M, N // 2, op)
    hip.igemm(M=M, N=N, K=K, A=f["A"].to(op).to(DEV), lda=K, W=f["W"].to(op).to(DEV), bias=f["bias"].to(DEV), flags=hip.EP_BIAS | hip.EP_SWIGLU, out_op=out, ldo_op=N // 2 + 8)
    X.assert_within(out[:M, :N // 2], ref, X.e_act_sigmoid(ref), op, "swiglu")
    _guards_untouched(out, M, N // 2, "swiglu")


def test_igemm_sigmoid_tail_on_exact_logit(hip):
    op = _op(hip)
    f = X.tail_family(True)
    _tail_budget(f, "sigmoid tail")
    x, d = f["x"], f["ref"]
    assert float(d.abs().max()) <= 16.0 and float(d.std()) > 1.0
    B, C, H, W_ = x.shape
    out = torch.full((B, 1, H, W_), GUARD, device=DEV)
    hip.igemm(M=B * H * W_, N=32, K=9 * C, A=_pad_nhwc(x, C, op).to(DEV), lda=C, W=_pack3(f["w"], C, op).to(DEV), a_mode=hip.A_CONV3, conv=(H, W_, H + 2, W_ + 2, 1),
              bias=f["bias"].to(DEV), flags=hip.EP_BIAS | hip.EP_TAIL, out_f32=out, ldo_f32=1, tail_w=f["tw"].to(DEV), tail_b=0.25, tail_act=hip.ACT_SIGMOID)
    ref = torch.sigmoid(d)
    X.assert_within(out, ref, X.e_act_sigmoid(ref), None, "sigmoid tail")
