"""Exactly representable inputs for bit-for-bit kernel tests ("Exactness tests").

The kernels of libada_hip are linear in their operands up to the activation.  With small integers and dyadic fractions every product and every
partial sum of such a kernel is a multiple of one unit u = 2^-s, and as long as  sum |terms| / u < 2^24  each of them fits fp32's 24-bit
significand: no summation order rounds, and a correct kernel returns the fp64 result bit for bit.  What remains to round is the one conversion
to the operand type, which the tests restate with rne().

Builders return fp32 CPU tensors and assert that their values survive the operand type; assert_exact_budget is the sufficient condition above,
computed from the inputs alone (it knows nothing of the kernel); assert_bits compares raw bits.  Every input family of the GPU tests is built
here, cached, and the *_CASES lists hold the arguments the GPU tests pass: tests/test_exact_inputs_cpu.py walks the same lists, so the premise --
two fp32 summation orders equal fp64, budget, rounded share, ties -- is checked on the very tensors the kernels get."""
import functools

import torch
import torch.nn.functional as F

LIMIT = float(2 ** 24)
OP_TYPES = (torch.float16, torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------
def survives(t, op=None):
    """t (fp32 / fp64) is exactly representable in the operand type(s)."""
    for o in ((op,) if op is not None else OP_TYPES):
        back = t.float().to(o).float()
        assert torch.equal(back, t.float()), f"{int((back != t.float()).sum())} of {t.numel()} values do not survive {o}"
    return t


def ints(shape, lo, hi, seed, op=None):
    """Seeded integers in [lo, hi] as fp32 (unit 1)."""
    g = torch.Generator().manual_seed(seed)
    return survives(torch.randint(lo, hi + 1, tuple(shape), generator=g).float(), op)


def dyadic(shape, max_k, denom, seed, op=None):
    """Seeded k / denom with |k| <= max_k, denom a power of two (unit 1 / denom)."""
    assert denom & (denom - 1) == 0
    return survives(ints(shape, -max_k, max_k, seed) / float(denom), op)


def fp32_dyadic(shape, max_k, denom, seed):
    """The same for tensors the kernels read as fp32 (bias, residual, gain tables): no operand type to survive."""
    assert denom & (denom - 1) == 0
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-max_k, max_k + 1, tuple(shape), generator=g).float() / float(denom)


def choice(shape, values, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the budget
# ---------------------------------------------------------------------------------------------------------------------------------
def assert_exact_budget(a=None, w=None, *, unit, bias=None, gamma=None, residual=None, mag=None, ref=None, what=""):
    """Per output element  (sum_k |a w| + |bias|) |gamma| + |residual|  in units of `unit` must stay below 2^24, and every term must be a multiple of
    the unit: then every partial sum, in any order, is an integer below 2^24 times the unit -- exact in fp32.  a [M, K], w [N, K]; `mag` replaces
    sum_k |a w| where the contraction is not a plain matrix product (convolutions, interpolations).  `ref` (the fp64 result, or any fp64 tensor of
    intermediate values) must be integral in units of `unit`: a unit chosen too coarse would make the 2^24 condition meaningless, and shows here.
    Returns the largest budget in units."""
    if mag is None:
        mag = a.double().abs() @ w.double().abs().T
    mag = mag.double()
    if bias is not None:
        mag = mag + bias.double().abs()
    if gamma is not None:
        mag = mag * gamma.double().abs()
    if residual is not None:
        mag = mag + residual.double().abs()
    worst = float(mag.max()) / unit
    assert worst < LIMIT, f"{what}: budget {worst:.3e} units of {unit} is not below 2^24"
    if ref is not None:
        q = ref.double() / unit
        assert torch.equal(q, q.round()), f"{what}: {int((q != q.round()).sum())} reference values are not multiples of the unit {unit}"
    # the unit really is one: the smallest products / addends are multiples of it
    probe = []
    if a is not None:
        probe.append(float(a.double().abs()[a != 0].min()) * float(w.double().abs()[w != 0].min()))
    for t in (bias, residual):
        if t is not None and bool((t != 0).any()):
            probe.append(float(t.double().abs()[t != 0].min()))
    for p in probe:
        if gamma is not None:
            p = p * float(gamma.double().abs()[gamma != 0].min())
        assert (p / unit) == int(p / unit), f"{what}: {p} is not a multiple of the unit {unit}"
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# references and checks
# ---------------------------------------------------------------------------------------------------------------------------------
def rne(x64, op):
    """The fp64 reference rounded ONCE to the operand type, with the saturation at +-65504 that csrc/ada_common.h to_op applies for fp16.  (The
    reference must be exact in fp32 -- which the budget guarantees -- so that no double rounding hides in the conversion.)"""
    x32 = x64.float()
    assert torch.equal(x32.double(), x64.double()), "the fp64 reference is not exact in fp32: rne would round twice"
    if op == torch.float16:
        x32 = x32.clamp(-65504.0, 65504.0)
    return x32.to(op)


def split_ref(v64, op):
    """(hi, lo) = (rne(v), rne(v - hi)): the [hi | lo] form of a split-precision output."""
    hi = rne(v64, op)
    lo = rne(v64.double() - hi.double(), op)
    return hi, lo


def e5m2(t):
    """fp32 -> e5m2 byte codes, saturating at the largest finite code (csrc/ada_common.h bf8x4)."""
    return t.float().clamp(-57344.0, 57344.0).to(torch.float8_e5m2).view(torch.uint8)


def _raw(t):
    t = t.detach().cpu().contiguous()
    if t.dtype in (torch.float16, torch.bfloat16):
        t = torch.where(t == 0, torch.zeros_like(t), t)        # -0 and +0 are the same value
        return t.view(torch.int16)
    if t.dtype == torch.float32:
        t = torch.where(t == 0, torch.zeros_like(t), t)
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        raise TypeError("compare in the kernel's own output type")
    return t


def assert_bits(got, want, what=""):
    """torch.equal on the raw bits (the sign of a zero aside).  `want` fp64 is first narrowed to got's type, exactly or not at all."""
    got = got.detach().cpu()
    want = want.detach().cpu()
    if want.dtype == torch.float64:
        narrowed = want.to(got.dtype)
        assert torch.equal(narrowed.double(), want), f"{what}: the reference is not representable in {got.dtype}"
        want = narrowed
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    g, w = _raw(got), _raw(want)
    if torch.equal(g, w):
        return
    bad = (g != w)
    idx = bad.nonzero()
    lines = [f"{tuple(i.tolist())}: got {float(got[tuple(i)])!r} want {float(want[tuple(i)])!r}" for i in idx[:6]]
    trunc = ""
    if got.dtype in (torch.float16, torch.bfloat16) and got.is_floating_point():
        gi, wi = g[bad].int(), w[bad].int()
        finite = torch.isfinite(got[bad].float()).all()
        # sign-magnitude codes: one ulp towards zero is the magnitude code one lower, sign kept
        toward_zero = bool(finite) and bool((((wi & 0x7fff) - (gi & 0x7fff)) == 1).all()) and bool(((wi ^ gi) & 0x8000 == 0).all())
        trunc = "; every miss is 1 ulp towards zero (truncation instead of round-to-nearest-even?)" if toward_zero else "; the misses are not all 1 ulp towards zero"
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ bit for bit{trunc}\n  " + "\n  ".join(lines))


def ulp(x64, op):
    """Spacing of the operand type at |x| (subnormals included)."""
    mant, emin = (10, -14) if op == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(x64.double().abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def rounding_census(x64, op):
    """(share of the values that need rounding in the operand type, share that are exact ties, share where truncation differs from RNE)."""
    x = x64.double()
    r = x.float().to(op).double()
    inexact = r != x
    u = ulp(x, op)
    down = torch.floor(x / u) * u
    tie = inexact & ((x - down) * 2 == u)
    trunc = torch.where(x >= 0, down, torch.ceil(x / u) * u)
    return float(inexact.double().mean()), float(tie.double().mean()), float((trunc != r).double().mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# e_act: the activations' own error (derived, not measured)
# ---------------------------------------------------------------------------------------------------------------------------------
def e_act_gelu(ref64):
    """tests/test_gelu_formula_cpu.py's bound for the kernel's exp2-polynomial form."""
    return 4e-7 * ref64.double().abs().clamp_min(1.0)


def e_act_sigmoid(ref64):
    """One v_exp_f32 and one v_rcp_f32 at 1 ulp each, the argument's rounding at |x| <= 16 (~1e-6 relative in the exponential) and two multiplies: about three
    times their sum."""
    return 4e-6 * ref64.double().abs() + 1e-7


def assert_within(got, ref64, e_act, op=None, what=""):
    """|got - ref64| <= ulp_op(ref64) / 2 + e_act; the rounding term is dropped for fp32 outputs (op None)."""
    got = got.detach().cpu().double()
    lim = e_act + (ulp(ref64, op) / 2 if op is not None else 0.0)
    err = (got - ref64.double()).abs()
    bad = err > lim
    worst = float((err / lim).max())
    print(f"{what}: worst |got - ref| / bound = {worst:.3f}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} beyond ulp/2 + e_act, worst ratio {worst:.3f}"


# ---------------------------------------------------------------------------------------------------------------------------------
# input families (shared by the CPU premise test and the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------------------
GEMM_M, GEMM_N = 3 * 256 + 77, 2 * 256 + 64        # 4 ragged tile rows of 256, partial last N tile (tests/test_gpu_kernels.py, forced-tile epilogues)
GAMMAS = (0.5, -0.5, 0.75, -0.75, 1.0, -1.0, 1.5, 2.0)


@functools.lru_cache(maxsize=None)
def gemm_family(K, M=GEMM_M, N=GEMM_N):
    """A integers in [-8, 8], W = k / 64 with |k| <= 64, bias = k / 64 with |k| <= 4096, gamma in GAMMAS (quarters), residual k / 64: unit 2^-8 with gamma."""
    A = ints((M, K), -8, 8, 1000 + K)
    W = dyadic((N, K), 64, 64, 2000 + K)
    b = fp32_dyadic((N,), 4096, 64, 3000 + K)
    g = choice((N,), GAMMAS, 4000 + K)
    r = fp32_dyadic((M, N), 4096, 64, 5000 + K)
    lin = A.double() @ W.double().T
    return dict(A=A, W=W, bias=b, gamma=g, res=r, lin=lin, unit=2.0 ** -6, unit_gamma=2.0 ** -8)


@functools.lru_cache(maxsize=None)
def small_family(M, N, K, seed=0, a_max=8, w_k=64, w_denom=64, b_k=4096):
    """The same value ranges on another shape (geometry tests); a_max / w_k / w_denom shrink them where a test needs it."""
    A = ints((M, K), -a_max, a_max, 6000 + seed)
    W = dyadic((N, K), w_k, w_denom, 6100 + seed)
    b = fp32_dyadic((N,), b_k, w_denom, 6200 + seed)
    return dict(A=A, W=W, bias=b, lin=A.double() @ W.double().T, unit=1.0 / w_denom)


@functools.lru_cache(maxsize=None)
def conv_family(B, C, H, W_, Co, seed=0):
    """NCHW integer map in [-8, 8], 3x3 weights k / 64 with |k| <= 64, bias k / 64 (the GEMM family's ranges): unit 2^-6."""
    x = ints((B, C, H, W_), -8, 8, 7000 + seed)
    w = dyadic((Co, C, 3, 3), 64, 64, 7100 + seed)
    b = fp32_dyadic((Co,), 4096, 64, 7200 + seed)
    return dict(x=x, w=w, bias=b, unit=2.0 ** -6)


@functools.lru_cache(maxsize=None)
def f8_family(M, N, seg=128):
    """Hand-built [hi | lo8 | hi8] rows and [w_hi | w_hi8 | w_lo8] weights (include/ada_hip.h, f8_from) with the fixed scale word
    117 | 127 << 8 | 127 << 16 | 117 << 24:  x_hi w_hi + 2^-10 x_lo8 w_hi8 + 2^-10 x_hi8 w_lo8.  The hi part is kept small (A in [-2, 2], W = k / 8)
    so that the 2^-13 unit of the correction terms stays inside the budget.  Byte values: e5m2 integers in [-2, 2], e4m3 k / 8 with |k| <= 16."""
    a_hi = ints((M, seg), -2, 2, 8000)
    a_lo8 = ints((M, seg), -2, 2, 8001)
    a_hi8 = ints((M, seg), -2, 2, 8002)
    w_hi = dyadic((N, seg), 16, 8, 8003)
    w_hi8 = dyadic((N, seg), 16, 8, 8004)
    w_lo8 = dyadic((N, seg), 16, 8, 8005)
    for t in (a_lo8, a_hi8):
        assert torch.equal(t.to(torch.float8_e5m2).float(), t)
    for t in (w_hi8, w_lo8):
        assert torch.equal(t.to(torch.float8_e4m3fn).float(), t)
    word = 117 | (127 << 8) | (127 << 16) | (117 << 24)
    s = 2.0 ** -10
    ref = a_hi.double() @ w_hi.double().T + s * (a_lo8.double() @ w_hi8.double().T) + s * (a_hi8.double() @ w_lo8.double().T)
    mag = a_hi.abs().double() @ w_hi.abs().double().T + s * (a_lo8.abs().double() @ w_hi8.abs().double().T) + s * (a_hi8.abs().double() @ w_lo8.abs().double().T)
    return dict(a_hi=a_hi, a_lo8=a_lo8, a_hi8=a_hi8, w_hi=w_hi, w_hi8=w_hi8, w_lo8=w_lo8, word=word, ref=ref, mag=mag, unit=2.0 ** -13, seg=seg)


def f8_pack(hi, first8, second8, op, first_dtype, second_dtype):
    """[rows, seg] fp32 pieces -> [rows, 2 seg] operand-typed storage: seg operand slots, then seg bytes, then seg bytes."""
    rows, seg = hi.shape
    packed = torch.cat([hi.to(op).contiguous().view(torch.uint8).reshape(rows, 2 * seg), first8.to(first_dtype).view(torch.uint8),
                        second8.to(second_dtype).view(torch.uint8)], dim=1)
    return packed.contiguous().view(op)


@functools.lru_cache(maxsize=None)
def nonlinear_family(M, N, K=64, seed=0):
    """Pre-activations of std ~2, |x| <= 16: A in [-2, 2], W = k / 64 with |k| <= 16, bias k / 64 with |k| <= 128."""
    A = ints((M, K), -2, 2, 9000 + seed)
    W = dyadic((N, K), 16, 64, 9100 + seed)
    b = fp32_dyadic((N,), 128, 64, 9200 + seed)
    pre = A.double() @ W.double().T + b.double()
    assert float(pre.abs().max()) <= 16.0
    return dict(A=A, W=W, bias=b, pre=pre, unit=2.0 ** -6)


def bilinear_ref(x_nchw, ho, wo):
    """Align-corners bilinear in fp64; exact for integer maps when ho - 1 = 2^k (hi - 1) (the scale is dyadic)."""
    hi, wi = x_nchw.shape[-2:]
    for n_in, n_out in ((hi, ho), (wi, wo)):
        if n_in > 1:
            ratio = (n_out - 1) / (n_in - 1)
            assert ratio == int(ratio) and int(ratio) & (int(ratio) - 1) == 0, f"{n_in} -> {n_out} is not a dyadic scale"
    return F.interpolate(x_nchw.double(), size=(ho, wo), mode="bilinear", align_corners=True)


def reversed_chunks(k, chunk=64):
    """A second summation order: the k axis in chunks of 64, last chunk first."""
    idx = torch.arange(k)
    return torch.cat([idx[s:s + chunk] for s in range(0, k, chunk)][::-1])


# ---------------------------------------------------------------------------------------------------------------------------------
# Families beyond the plain GEMM.  Each returns a dict with the inputs and
#   ref     the fp64 result the kernel must return          mag / unit   the budget's magnitude (sum |terms|) and unit
#   orders  () -> fp32 evaluations in different orders       op_out       {name: fp64 values a kernel rounds to the operand type} (census)
# The *_CASES lists are the arguments the GPU tests use.
# ---------------------------------------------------------------------------------------------------------------------------------
def _mm_orders(a, w, extra=None):
    """fp32 a @ w.T plain, with k reversed in chunks of 64, and as chunk sums added last chunk first."""
    def run():
        K = a.shape[1]
        perm = reversed_chunks(K)
        acc = torch.zeros(a.shape[0], w.shape[0])
        for s0 in reversed(range(0, K, 64)):
            acc = acc + a[:, s0:s0 + 64] @ w[:, s0:s0 + 64].T
        outs = [a @ w.T, a[:, perm] @ w[:, perm].T, acc]
        return [extra(t) for t in outs] if extra is not None else outs
    return run


def _conv_orders(x, w, b, stride=1, post=None):
    def run():
        outs = [F.conv2d(x, w, b, stride=stride, padding=1), F.conv2d(x.flip(1), w.flip(1), b, stride=stride, padding=1)]
        return [post(t) for t in outs] if post is not None else outs
    return run


BIAS_GROUPS = 5          # GEMM_M = 845 = 5 * 169: one bias vector per group of 169 rows (bias_row_mod)


@functools.lru_cache(maxsize=None)
def bias_groups():
    return fp32_dyadic((BIAS_GROUPS, GEMM_N), 4096, 64, 3333)


@functools.lru_cache(maxsize=None)
def a_dup_family(M=300, N=200, seg=128):
    """(hi, lo, hi) against [w_hi | w_hi | w_lo], independent exact pieces: units 2^-6, 2^-14, 2^-10 per segment."""
    hi, lo = ints((M, seg), -8, 8, 41), dyadic((M, seg), 8, 256, 42)
    w_hi, w_lo = dyadic((N, seg), 64, 64, 43), dyadic((N, seg), 8, 1024, 44)
    b = fp32_dyadic((N,), 4096, 64, 45)
    a3, w3 = torch.cat([hi, lo, hi], 1), torch.cat([w_hi, w_hi, w_lo], 1)
    return dict(hi=hi, lo=lo, w3=w3, bias=b, ref=a3.double() @ w3.double().T + b.double(), mag=a3.double().abs() @ w3.double().abs().T + b.double().abs(),
                unit=2.0 ** -14, orders=_mm_orders(a3, w3, lambda t: t + b), op_out={})


@functools.lru_cache(maxsize=None)
def a_wrap_family(M=300, N=200, K=128):
    """x against [w_hi | w_lo] with the A walk starting over: units 2^-6 and 2^-10."""
    x = ints((M, K), -8, 8, 47)
    w_hi, w_lo = dyadic((N, K), 64, 64, 48), dyadic((N, K), 8, 1024, 49)
    b = fp32_dyadic((N,), 4096, 64, 50)
    a2, w2 = torch.cat([x, x], 1), torch.cat([w_hi, w_lo], 1)
    return dict(x=x, w2=w2, bias=b, ref=a2.double() @ w2.double().T + b.double(), mag=a2.double().abs() @ w2.double().abs().T + b.double().abs(),
                unit=2.0 ** -10, orders=_mm_orders(a2, w2, lambda t: t + b), op_out={})


@functools.lru_cache(maxsize=None)
def f8_bias():
    return fp32_dyadic((200,), 4096, 64, 46)


@functools.lru_cache(maxsize=None)
def saturation_family(M=300, N=128, K=64):
    """Column blocks whose exact result is > 65504, < -65504, and ordinary (W = k / 8).  The subject is the clamp, not the rounding: no census."""
    A = ints((M, K), 2, 4, 51)
    W = torch.zeros(N, K)
    W[:40] = 1024.0           # >= 2 * 64 * 1024 = 131072
    W[40:80] = -1024.0
    W[80:] = dyadic((N - 80, K), 64, 8, 52)
    survives(W)
    v = A.double() @ W.double().T
    assert float(v[:, :40].min()) > 65504.0 and float(v[:, 40:80].max()) < -65504.0 and float(v[:, 80:].abs().max()) < 65504.0
    return dict(A=A, W=W, ref=v, mag=A.double().abs() @ W.double().abs().T, unit=2.0 ** -3, orders=_mm_orders(A, W), op_out={})


CONV_RES_CASES = [(2, 64, 21, 17, 64, 1), (2, 128, 37, 37, 128, 2)]
CONV_RES_WIDE_CASE = (1, 64, 17, 16, 256, 1)   # M = 272, N = 256: on the 256- and 128-row tiles interior tiles and one edge tile


@functools.lru_cache(maxsize=None)
def conv_res_family(B, C, H, W_, Co, stride):
    """3x3 convolution (stride 1 / 2) + bias + fp32 residual; the ReLU'd operand copy goes to a padded grid."""
    c = conv_family(B, C, H, W_, Co, seed=10 + stride)
    Ho, Wo = (H - 1) // stride + 1, (W_ - 1) // stride + 1
    res = fp32_dyadic((B * Ho * Wo, Co), 4096, 64, 12)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Co)      # noqa: E731
    v = rows(F.conv2d(c["x"].double(), c["w"].double(), c["bias"].double(), stride=stride, padding=1)) + res.double()
    mag = rows(F.conv2d(c["x"].double().abs(), c["w"].double().abs(), c["bias"].double().abs(), stride=stride, padding=1)) + res.double().abs()
    return dict(x=c["x"], w=c["w"], bias=c["bias"], res=res, Ho=Ho, Wo=Wo, ref=v, mag=mag, unit=c["unit"],
                orders=_conv_orders(c["x"], c["w"], c["bias"], stride, lambda t: rows(t) + res), op_out={"relu(conv + residual)": v.clamp_min(0)})


@functools.lru_cache(maxsize=None)
def split_pad_family(B=2, C=64, H=13, W_=17):
    """3x3 convolution writing a split, zero-bordered output (ReLU'd) + its fp32 copy."""
    c = conv_family(B, C, H, W_, C, seed=3)
    v = F.conv2d(c["x"].double(), c["w"].double(), c["bias"].double(), padding=1).permute(0, 2, 3, 1)
    mag = F.conv2d(c["x"].double().abs(), c["w"].double().abs(), c["bias"].double().abs(), padding=1)
    return dict(x=c["x"], w=c["w"], bias=c["bias"], ref=v, mag=mag, unit=c["unit"], orders=_conv_orders(c["x"], c["w"], c["bias"], 1, lambda t: t.permute(0, 2, 3, 1)),
                op_out={"relu(conv)": v.clamp_min(0)})


TOKEN_MAP_CASE = (3, 50, 128, 192)


@functools.lru_cache(maxsize=None)
def token_map_family(B, Np, D, K):
    f = small_family(B * Np, D, K, seed=2)
    pos = fp32_dyadic((Np + 1, D), 4096, 64, 15)
    add = f["bias"].view(1, 1, D) + pos[1:].view(1, Np, D)
    ref = (f["lin"] + f["bias"].double()).reshape(B, Np, D) + pos.double()[1:]
    mag = (f["A"].double().abs() @ f["W"].double().abs().T + f["bias"].double().abs()).reshape(B, Np, D) + pos.double().abs()[1:]
    return dict(A=f["A"], W=f["W"], bias=f["bias"], pos=pos, ref=ref, mag=mag, unit=f["unit"],
                orders=_mm_orders(f["A"], f["W"], lambda t: (t + f["bias"]).reshape(B, Np, D) + pos[1:]), op_out={})


SHUFFLE_CASES = [(2, 96, 96, 7, 5), (4, 48, 48, 7, 5)]      # s, C, Ci, H, W
SPLIT_SHUFFLE_CASE = (2, 48, 64, 5, 6)


@functools.lru_cache(maxsize=None)
def shuffle_family(s, C, Ci, H, W_, B=2):
    """ConvTranspose2d k = s as a GEMM [B H W, Ci] x [s s C, Ci] + pixel shuffle; the GEMM family's value ranges."""
    x = ints((B, Ci, H, W_), -8, 8, 21)
    w = dyadic((Ci, C, s, s), 64, 64, 22)
    b = fp32_dyadic((C,), 4096, 64, 23)
    cp = (Ci + 63) // 64 * 64
    A = torch.zeros(B * H * W_, cp)
    A[:, :Ci] = x.permute(0, 2, 3, 1).reshape(-1, Ci)
    Wp = torch.zeros(s * s * C, cp)
    Wp[:, :Ci] = w.permute(2, 3, 1, 0).reshape(s * s * C, Ci)
    bp = b.repeat(s * s)
    ref = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=s).permute(0, 2, 3, 1)          # [B, s H, s W, C]
    flat = A.double() @ Wp.double().T + bp.double()
    assert torch.equal(flat.view(B, H, W_, s, s, C).permute(0, 1, 3, 2, 4, 5).reshape(B, s * H, s * W_, C), ref)
    return dict(A=A, Wp=Wp, bias=bp, cp=cp, ref=ref, flat=flat, mag=A.double().abs() @ Wp.double().abs().T + bp.double().abs(), unit=2.0 ** -6,
                orders=_mm_orders(A, Wp, lambda t: t + bp), orders_ref=flat, op_out={"conv transpose": ref})


def subpixel_masks(s):
    """tap_mask of a stride-s transposed convolution followed by a 3x3 convolution (hip_ext.functional.subpixel_merge's index arithmetic)."""
    masks = [0] * (s * s)
    for py in range(s):
        for px in range(s):
            for ty in range(3):
                for tx in range(3):
                    dy, dx = (py + ty - 1) // s, (px + tx - 1) // s
                    masks[py * s + px] |= 1 << ((dy + 1) * 3 + (dx + 1))
    return masks


SUBPIXEL_CASES = [(4, 48, 48, 7, 5, -1), (2, 96, 96, 9, 6, -1), (4, 48, 48, 7, 5, 3), (2, 96, 96, 9, 6, 1)]      # s, Ci, Co, H, W, tile cfg


@functools.lru_cache(maxsize=None)
def subpixel_family(s, Ci, Co, H, W_, B=2):
    """Masked-tap weights: dyadic in the taps a phase touches, zero elsewhere (as the packer leaves them)."""
    N = s * s * Co
    masks = subpixel_masks(s)
    x = ints((B, Ci, H, W_), -8, 8, 31)
    wm = dyadic((s * s, Co, 9, Ci), 64, 64, 32)
    keep = torch.tensor([[(m >> t) & 1 for t in range(9)] for m in masks], dtype=torch.float32)      # [phase, tap]
    wm = (wm * keep.view(s * s, 1, 9, 1)).reshape(N, 9, Ci)
    b = fp32_dyadic((N,), 4096, 64, 33)
    w4 = wm.reshape(N, 3, 3, Ci).permute(0, 3, 1, 2).contiguous()
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, N)      # noqa: E731
    return dict(x=x, wm=wm, bias=b, masks=masks, ref=rows(F.conv2d(x.double(), w4.double(), b.double(), padding=1)),
                mag=F.conv2d(x.double().abs(), w4.double().abs(), b.double().abs(), padding=1), unit=2.0 ** -6, orders=_conv_orders(x, w4, b, 1, rows), op_out={})


@functools.lru_cache(maxsize=None)
def tail_family(sigmoid):
    """conv3x3 (64 -> 32) -> ReLU -> 32 -> 1 dot -> + tail_b.  For the sigmoid the dot is kept within |d| <= 16 (part C)."""
    B, C, H, W_, Co = 1, 64, 28, 42, 32
    if sigmoid:
        x, w, b = ints((B, C, H, W_), -1, 1, 9300), dyadic((Co, C, 3, 3), 16, 64, 9301), fp32_dyadic((Co,), 64, 64, 9302)
        tw, unit = fp32_dyadic((Co,), 24, 64, 9303), 2.0 ** -12
    else:
        c = conv_family(B, C, H, W_, Co, seed=2)
        x, w, b = c["x"], c["w"], c["bias"]
        tw, unit = fp32_dyadic((Co,), 8, 8, 60), 2.0 ** -9
    v = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    d = (v.clamp_min(0) * tw.double().view(1, -1, 1, 1)).sum(1, keepdim=True) + 0.25
    mag = (v.clamp_min(0) * tw.double().abs().view(1, -1, 1, 1)).sum(1) + 0.25

    def orders():
        v32 = [F.conv2d(x, w, b, padding=1).clamp_min(0), F.conv2d(x.flip(1), w.flip(1), b, padding=1).clamp_min(0)]
        return [(v32[0] * tw.view(1, -1, 1, 1)).sum(1, keepdim=True) + 0.25, (v32[1].flip(1) * tw.flip(0).view(1, -1, 1, 1)).sum(1, keepdim=True) + 0.25]
    return dict(x=x, w=w, bias=b, tw=tw, conv=v, conv_mag=F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1), conv_unit=2.0 ** -6,
                ref=d, mag=mag, unit=unit, orders=orders, op_out={})


BILINEAR_CASES = [(64, 5, 4, 9, 13), (64, 3, 9, 17, 33), (128, 19, 19, 37, 73), (128, 5, 4, 9, 13)]      # C, hi, wi, ho, wo


@functools.lru_cache(maxsize=None)
def bilinear_family(C, hi, wi, ho, wo, B=2):
    x = ints((B, C, hi, wi), -8, 8, 61)
    add = fp32_dyadic((B * ho * wo, C), 4096, 64, 62)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)      # noqa: E731
    up = rows(bilinear_ref(x, ho, wo))
    v = up + add.double()

    def orders():
        a = F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=True)
        # the other order: columns first, then rows
        b_ = F.interpolate(F.interpolate(x, size=(hi, wo), mode="bilinear", align_corners=True), size=(ho, wo), mode="bilinear", align_corners=True)
        return [rows(a) + add, rows(b_) + add]
    return dict(x=x, add=add, up=up, ref=v, mag=rows(bilinear_ref(x.abs(), ho, wo)) + add.double().abs(), unit=2.0 ** -6, orders=orders,
                op_out={"bilinear + add": v, "relu(bilinear + add)": v.clamp_min(0)})


TAPSUM_CASES = [(2, 32, 8, 3, 9, 17, 33), (1, 64, 8, 9, 17, 17, 33), (1, 128, 4, 5, 4, 9, 13), (1, 64, 8, 9, 33, 17, 65)]      # B, C, Cin, hi, wi, ho, wo


@functools.lru_cache(maxsize=None)
def tapsum_family(B, C, Cin, hi, wi, ho, wo):
    """Integer tap maps T[:, t C + co] = W_t u on the coarse grid, built on the host; reference conv3x3(upsample(u))."""
    u = ints((B, Cin, hi, wi), -2, 2, 71)
    w1 = ints((C, Cin, 3, 3), -1, 1, 72)
    b1 = fp32_dyadic((C,), 4096, 64, 73)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)      # noqa: E731
    ref = rows(F.conv2d(bilinear_ref(u, ho, wo), w1.double(), b1.double(), padding=1))
    mag = F.conv2d(bilinear_ref(u.abs(), ho, wo), w1.double().abs(), b1.double().abs(), padding=1)
    T = torch.einsum("ocyx,bchw->bhwyxo", w1.double(), u.double()).reshape(B * hi * wi, 9 * C).float()          # column t * C + co, t = dy * 3 + dx
    survives(T)

    def orders():
        up = F.interpolate(u, size=(ho, wo), mode="bilinear", align_corners=True)
        direct = rows(F.conv2d(up, w1, b1, padding=1))
        # the kernel's own order: resample each tap map, then add the nine shifted maps
        Tm = F.interpolate(T.view(B, hi, wi, 9, C).permute(0, 3, 4, 1, 2).reshape(B, 9 * C, hi, wi), size=(ho, wo), mode="bilinear", align_corners=True).view(B, 9, C, ho, wo)
        acc = torch.zeros(B, C, ho, wo)
        P = F.pad(Tm, (1, 1, 1, 1))
        for t in range(9):
            dy, dx = t // 3, t % 3
            acc = acc + P[:, t, :, dy:dy + ho, dx:dx + wo]
        return [direct, rows(acc + b1.view(1, -1, 1, 1))]
    return dict(T=T, bias=b1, ref=ref, mag=mag, unit=2.0 ** -6, orders=orders, op_out={})


DPT_TAIL_CASES = [(2, 64, 9, 11, 17, 41), (1, 128, 8, 16, 29, 31), (6, 128, 41, 121, 81, 241)]      # B, C, hi, wi, ho, wo


@functools.lru_cache(maxsize=None)
def dpt_tail_family(B, C, hi, wi, ho, wo):
    """x2 / x4 up-sampling of an integer map (exact in the operand type the kernel stages it in), dyadic 3x3 weights, bias and tail_w."""
    x = ints((B, C, hi, wi), -4, 4, 81)
    w = dyadic((32, C, 3, 3), 16, 32, 82)
    b = fp32_dyadic((32,), 256, 32, 83)
    tw = fp32_dyadic((32,), 4, 4, 84)
    up = bilinear_ref(x, ho, wo)
    survives(up.float())
    v = F.conv2d(up, w.double(), b.double(), padding=1)
    d = (v.clamp_min(0) * tw.double().view(1, -1, 1, 1)).sum(1) + 0.25

    def orders():
        up32 = F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=True)
        a = (F.conv2d(up32, w, b, padding=1).clamp_min(0) * tw.view(1, -1, 1, 1)).sum(1) + 0.25
        r = (F.conv2d(up32.flip(1), w.flip(1), b, padding=1).clamp_min(0).flip(1) * tw.flip(0).view(1, -1, 1, 1)).sum(1) + 0.25
        return [a, r]
    return dict(x=x, w=w, bias=b, tw=tw, conv=v, conv_mag=F.conv2d(bilinear_ref(x.abs(), ho, wo), w.double().abs(), b.double().abs(), padding=1), conv_unit=2.0 ** -9,
                ref=d, mag=(v.clamp_min(0) * tw.double().abs().view(1, -1, 1, 1)).sum(1) + 0.25, unit=2.0 ** -11, orders=orders, op_out={})


UNSHUFFLE_CASES = [(4, 48, 7, 5), (2, 96, 9, 6), (2, 640, 3, 2)]      # s, dim, H, W


@functools.lru_cache(maxsize=None)
def unshuffle_family(s, dim, H, W_, B=2):
    """[coarse pixel, s s dim] fp32 input and tap_bias [s s dim, 9], dyadic; the fp64 restatement of the un-shuffle with the ring subtraction."""
    N = s * s * dim
    inp = fp32_dyadic((B * H * W_, N), 4096, 64, 91)
    tapb = fp32_dyadic((N, 9), 256, 64, 92)
    fh, fw = s * H, s * W_
    Y, Xc = torch.arange(fh), torch.arange(fw)

    def restate(inp_, tapb_, taps):
        fine = inp_.view(B, H, W_, s, s, dim).permute(0, 1, 3, 2, 4, 5).reshape(B, fh, fw, dim).clone()
        tb = tapb_.view(s, s, dim, 9)
        for t in taps:
            dy, dx = t // 3, t % 3
            miss_y = ((Y == 0) & (dy == 0)) | ((Y == fh - 1) & (dy == 2))
            miss_x = ((Xc == 0) & (dx == 0)) | ((Xc == fw - 1) & (dx == 2))
            miss = (miss_y[:, None] | miss_x[None, :]).to(inp_.dtype)                          # [fh, fw]: coarse tap t is outside the grid for this fine pixel
            fine -= miss[None, :, :, None] * tb[Y % s][:, Xc % s][:, :, :, t][None]
        return fine
    fine = restate(inp.double(), tapb.double(), range(9))
    mag = inp.double().abs().max() + tapb.double().abs().sum(1).max().expand(1)
    return dict(inp=inp, tapb=tapb, fh=fh, fw=fw, ref=fine, mag=mag, unit=2.0 ** -6, orders=lambda: [restate(inp, tapb, range(9)), restate(inp, tapb, reversed(range(9)))],
                op_out={"un-shuffled": fine, "relu(un-shuffled)": fine.clamp_min(0)})


PATCHIFY_MEAN, PATCHIFY_INV_STD = (0.5, 0.25, 0.375), (4.0, 2.0, 8.0)


@functools.lru_cache(maxsize=None)
def patchify_family(cg, norm, B=2, H=42, W_=56):
    """Pixels k / 16384 (14 bits: the operand type rounds them), guide k / 8192, dyadic mean and power-of-two inv_std: (x - mean) * inv_std is exact in fp32."""
    x = ints((B, 3, H, W_), 0, 16384, 101, op=torch.float32) / 16384.0
    g = fp32_dyadic((B, max(cg, 1), H, W_), 8192, 8192, 102)
    K = (3 + cg) * 196

    def run(x_, g_):
        mu, inv = torch.tensor(PATCHIFY_MEAN, dtype=x_.dtype).view(-1, 1, 1), torch.tensor(PATCHIFY_INV_STD, dtype=x_.dtype).view(-1, 1, 1)
        xn = (x_ - mu) * inv if norm else x_
        full = torch.cat([xn, g_], 1) if cg else xn
        return F.unfold(full, 14, stride=14).transpose(1, 2).reshape(-1, K)
    ref = run(x.double(), g.double())
    return dict(x=x, g=g, K=K, ref=ref, mag=ref.abs(), unit=2.0 ** -14, orders=lambda: [run(x, g)], op_out={"patches": ref})


DEPTH_STATS_CASES = [(2, 126, 154), (3, 14, 14)]
DEPTH_STATS_CHUNKS = 8


@functools.lru_cache(maxsize=None)
def depth_stats_family(B, H, W_):
    """s = k / 16 (sigmoid maps), z = k / 4 (ReLU / none): every chunk sum of the three activations' pairs, as the kernel cuts the chunks."""
    chunks, n = DEPTH_STATS_CHUNKS, H * W_
    s = ints((B, 1, H, W_), 0, 16, 111, op=torch.float32) / 16.0
    z = ints((B, 1, H, W_), -16, 16, 112, op=torch.float32) / 4.0
    per = (n + chunks - 1) // chunks

    def by_chunk(t, flip=False):          # [B, n] -> [B, chunks]: contiguous chunks of ceil(n / chunks) elements
        c = F.pad(t, (0, per * chunks - n)).view(B, chunks, per)
        return (c.flip(2) if flip else c).sum(2)

    def pairs(s_, z_, flip=False):
        zr = z_.clamp_min(0)
        return dict(sigmoid=torch.stack([by_chunk(s_, flip), by_chunk(s_ * (1 - s_), flip)], 2), relu=torch.stack([by_chunk(zr, flip), by_chunk((zr > 0).to(z_.dtype), flip)], 2),
                    none=torch.stack([by_chunk(z_.abs(), flip), by_chunk(torch.ones_like(z_), flip)], 2))
    s64, z64 = s.double().flatten(1), z.double().flatten(1)
    ref = pairs(s64, z64)
    # one budget per sum: (magnitude, unit, the fp64 sums) -- s in sixteenths, s (1 - s) in 1 / 256, z in quarters, counts in ones
    budgets = [(s64.sum(1), 2.0 ** -4, ref["sigmoid"][..., 0]), ((s64 * (1 - s64)).sum(1), 2.0 ** -8, ref["sigmoid"][..., 1]),
               (z64.abs().sum(1), 2.0 ** -2, torch.stack([ref["relu"][..., 0], ref["none"][..., 0]])), (torch.tensor([float(n)]), 1.0, torch.stack([ref["relu"][..., 1], ref["none"][..., 1]]))]
    allref = torch.cat([ref[k].flatten() for k in ("sigmoid", "relu", "none")])
    return dict(s=s, z=z, ref=ref, budgets=budgets, allref=allref,
                orders=lambda: [torch.cat([p[k].flatten() for k in ("sigmoid", "relu", "none")]) for p in (pairs(s.flatten(1), z.flatten(1)), pairs(s.flatten(1), z.flatten(1), True))],
                op_out={})


TOKEN_CASES = [(2, 64, 128, 256), (2, 64, 100, 128), (1, 128, 200, 200)]      # B, Np, D, ld


@functools.lru_cache(maxsize=None)
def token_family(B, Np, D, ld):
    """Integer tokens and a power-of-two token count: column means, mean squares and variances are dyadic, their 64-column sums exact."""
    assert Np & (Np - 1) == 0
    t = ints((B, Np, ld), -3, 3, 121)
    G = (D + 63) // 64
    pad = G * 64 - D

    def run(t_, flip=False):
        x = t_[:, :, :D]
        x = x.flip(1) if flip else x
        msq = (x * x).sum(1) / Np
        var = msq - (x.sum(1) / Np) ** 2
        cols = lambda v: F.pad(v, (0, pad)).view(B, G, 64)      # noqa: E731
        return torch.stack([(cols(var).flip(2) if flip else cols(var)).sum(2), (cols(msq).flip(2) if flip else cols(msq)).sum(2)], dim=2)
    ref = run(t.double())
    msq = (t.double()[:, :, :D] ** 2).sum(1) / Np
    return dict(t=t, G=G, ref=ref, mag=msq.sum(1), unit=2.0 ** -14, orders=lambda: [run(t), run(t, True)], op_out={})
