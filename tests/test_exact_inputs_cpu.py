"""The premise of tests/test_gpu_exact.py, checked on the reference alone: for every input family of tests/_exact.py, fp32 torch in two different
summation orders equals fp64 bit for bit, the budget is below 2^24, and the operand-typed outputs really exercise the rounding (>= 10 % of them
need it, exact ties are present).  A family that fails here is not used on the GPU."""
import pytest
import torch
import torch.nn.functional as F

import _exact as X


def _two_orders_equal_fp64(A, W, ref64, extra32=None, what=""):
    """fp32 A @ W.T plain and with the k axis reversed in chunks of 64 (both + extra32) against fp64."""
    K = A.shape[1]
    perm = X.reversed_chunks(K)
    plain = A @ W.T
    rev = A[:, perm] @ W[:, perm].T
    # a third order that no BLAS blocking can undo: chunk sums added last chunk first
    acc = torch.zeros_like(plain)
    for s in reversed(range(0, K, 64)):
        acc = acc + A[:, s:s + 64] @ W[:, s:s + 64].T
    for name, t in (("plain", plain), ("k reversed in chunks", rev), ("chunk sums, last first", acc)):
        if extra32 is not None:
            t = extra32(t)
        assert torch.equal(t.double(), ref64), f"{what}: fp32 ({name}) differs from fp64 on {int((t.double() != ref64).sum())} elements"


def _census(v64, what, need_ties=True):
    for op in X.OP_TYPES:
        share, ties, trunc = X.rounding_census(v64, op)
        print(f"{what} {op}: {share:.1%} of the outputs need rounding, {ties:.1%} are exact ties, truncation would differ on {trunc:.1%}")
        assert share >= 0.10, f"{what} {op}: only {share:.1%} of the outputs need rounding"
        assert trunc > 0.05, f"{what} {op}: truncation would be invisible"
        if need_ties:
            assert ties > 0, f"{what} {op}: no exact ties"
        hi, lo = X.split_ref(v64, op)
        assert torch.equal(hi.double() + lo.double(), v64.clamp(-65504.0, 65504.0) if op == torch.float16 else v64), f"{what} {op}: hi + lo != v"


@pytest.mark.parametrize("K", [64, 8256])
def test_premise_probe_family(K):
    f = X.gemm_family(K, 64, 64)
    X.assert_exact_budget(f["A"], f["W"], unit=f["unit"], ref=f["lin"], what=f"premise K={K}")
    _two_orders_equal_fp64(f["A"], f["W"], f["lin"], what=f"premise K={K}")


@pytest.mark.parametrize("K", [64, 320, 1088, 8256])
def test_gemm_family_is_order_independent(K):
    f = X.gemm_family(K) if K in (320, 8256) else X.gemm_family(K, 64, 64)
    ref = f["lin"] + f["bias"].double()
    worst = X.assert_exact_budget(f["A"], f["W"], bias=f["bias"], unit=f["unit"], what=f"gemm K={K}")
    print(f"gemm K={K}: worst budget {worst:.3e} units of 2^-6")
    _two_orders_equal_fp64(f["A"], f["W"], ref, lambda t: t + f["bias"], what=f"gemm K={K}")
    _two_orders_equal_fp64(f["A"], f["W"], f["lin"], what=f"gemm K={K}, no bias")
    if K == 320:
        _census(ref, "gemm + bias")
        _census(f["lin"], "gemm")
        _census(ref.clamp_min(0), "relu(gemm + bias)")
        X.assert_exact_budget(f["A"], f["W"], bias=f["bias"], gamma=f["gamma"], residual=f["res"], unit=f["unit_gamma"], what="gemm gamma + residual")
        full = ref * f["gamma"].double() + f["res"].double()
        _two_orders_equal_fp64(f["A"], f["W"], full, lambda t: (t + f["bias"]) * f["gamma"] + f["res"], what="gamma + residual")
        _census(ref * f["gamma"].double(), "(gemm + bias) * gamma")


def test_small_and_conv_families():
    f = X.small_family(150, 128, 192, seed=1)
    X.assert_exact_budget(f["A"], f["W"], bias=f["bias"], unit=f["unit"], what="small")
    _two_orders_equal_fp64(f["A"], f["W"], f["lin"] + f["bias"].double(), lambda t: t + f["bias"], what="small")
    _census(f["lin"] + f["bias"].double(), "small")
    c = X.conv_family(2, 64, 21, 17, 64, seed=1)
    ref = F.conv2d(c["x"].double(), c["w"].double(), c["bias"].double(), padding=1)
    mag = F.conv2d(c["x"].double().abs(), c["w"].double().abs(), c["bias"].double().abs(), padding=1)
    X.assert_exact_budget(mag=mag, unit=c["unit"], ref=ref, what="conv3x3")
    got = F.conv2d(c["x"], c["w"], c["bias"], padding=1)
    assert torch.equal(got.double(), ref)
    flipped = F.conv2d(c["x"].flip(1), c["w"].flip(1), c["bias"], padding=1)          # channels summed the other way round
    assert torch.equal(flipped.double(), ref)
    _census(ref, "conv3x3")


@pytest.mark.parametrize("M,N", [(300, 200), (64, 64)])
def test_f8_family(M, N):
    f = X.f8_family(M, N)
    worst = X.assert_exact_budget(mag=f["mag"], unit=f["unit"], ref=f["ref"], what="f8")
    print(f"f8: worst budget {worst:.3e} units of 2^-13")
    s = 2.0 ** -10
    a = torch.cat([f["a_hi"], f["a_lo8"] * s, f["a_hi8"] * s], dim=1)
    w = torch.cat([f["w_hi"], f["w_hi8"], f["w_lo8"]], dim=1)
    _two_orders_equal_fp64(a, w, f["ref"], what="f8 decoded pieces")
    # the correction terms matter: the result is not the hi product alone
    assert not torch.equal(f["ref"], f["a_hi"].double() @ f["w_hi"].double().T)


def _families():
    """Every family of tests/test_gpu_exact.py beyond the plain GEMM ones above, with the arguments the GPU tests pass (the *_CASES lists of tests/_exact.py)."""
    out = [("a_dup_seg", X.a_dup_family, ()), ("a_wrap", X.a_wrap_family, ()), ("saturation", X.saturation_family, ()),
           ("token map", X.token_map_family, X.TOKEN_MAP_CASE), ("split pad", X.split_pad_family, ()), ("split shuffle", X.shuffle_family, X.SPLIT_SHUFFLE_CASE),
           ("tail", X.tail_family, (False,)), ("sigmoid tail", X.tail_family, (True,))]
    out += [("conv + residual", X.conv_res_family, c) for c in X.CONV_RES_CASES + [X.CONV_RES_WIDE_CASE]]
    out += [("conv transpose", X.shuffle_family, c) for c in X.SHUFFLE_CASES]
    out += [("sub-pixel", X.subpixel_family, c[:5]) for c in X.SUBPIXEL_CASES[:2]]
    out += [("bilinear", X.bilinear_family, c) for c in X.BILINEAR_CASES]
    out += [("tap-sum", X.tapsum_family, c) for c in X.TAPSUM_CASES]
    out += [("fused tail", X.dpt_tail_family, c) for c in X.DPT_TAIL_CASES]
    out += [("un-shuffle", X.unshuffle_family, c) for c in X.UNSHUFFLE_CASES]
    out += [("patchify", X.patchify_family, (cg, norm)) for cg in (0, 2, 5) for norm in (False, True)]
    out += [("depth stats", X.depth_stats_family, c) for c in X.DEPTH_STATS_CASES]
    out += [("token diversity", X.token_family, c) for c in X.TOKEN_CASES]
    return out


@pytest.mark.parametrize("name,builder,args", _families(), ids=lambda v: v if isinstance(v, str) else ("-".join(str(a) for a in v) if isinstance(v, tuple) else ""))
def test_family_is_order_independent_and_exercises_rounding(name, builder, args):
    f = builder(*args)
    ref = f.get("orders_ref", f["ref"])
    ref = f["allref"] if "allref" in f else ref
    budgets = f.get("budgets") or [(f["mag"], f["unit"], ref)]
    worst = max(X.assert_exact_budget(mag=m, unit=u, ref=r, what=name) for m, u, r in budgets)
    if "conv" in f:         # two-stage families: the convolution in front of the ReLU -> 32 -> 1 dot has its own unit
        X.assert_exact_budget(mag=f["conv_mag"], unit=f["conv_unit"], ref=f["conv"], what=name + " (conv stage)")
    print(f"{name} {args}: worst budget {worst:.3e} units")
    for i, got in enumerate(f["orders"]()):
        assert got.dtype == torch.float32
        assert torch.equal(got.double(), ref), f"{name}: fp32 order {i} differs from fp64 on {int((got.double() != ref).sum())} elements"
    for what, v in f["op_out"].items():
        _census(v, f"{name} {args}: {what}")


def test_saturation_family_saturates():
    """The saturation family is about the clamp, not the rounding (its ordinary block needs none in fp16): what is asserted is that the exact result
    lies beyond +-65504 in two blocks and that lo = rne(v - hi) saturates too where v - hi does."""
    f = X.saturation_family()
    hi, lo = X.split_ref(f["ref"], torch.float16)
    assert bool((hi[:, :40] == 65504.0).all()) and bool((hi[:, 40:80] == -65504.0).all()) and bool((lo[:, :40] == 65504.0).all())
    hb, lb = X.split_ref(f["ref"], torch.bfloat16)
    assert torch.isfinite(hb.float()).all() and torch.equal(hb.double() + lb.double(), f["ref"])


def test_bias_row_groups_stay_in_budget():
    f = X.gemm_family(320)
    X.assert_exact_budget(f["A"], f["W"], bias=X.bias_groups().abs().max(0).values, unit=f["unit"], what="bias_row_mod")
    _census(f["lin"] + X.bias_groups().double().repeat_interleave(X.GEMM_M // X.BIAS_GROUPS, dim=0), "per-row-group bias")


@pytest.mark.parametrize("act", ["gelu", "silu", "sigmoid"])
def test_nonlinear_reference_alone(act):
    """fp32 torch against fp64 stays under a quarter of e_act on the inputs of part C: the bound leaves room for the kernel, not for the reference."""
    f = X.nonlinear_family(X.GEMM_M, X.GEMM_N)
    X.assert_exact_budget(f["A"], f["W"], bias=f["bias"], unit=f["unit"], what="pre-activation")
    pre = f["pre"]
    _two_orders_equal_fp64(f["A"], f["W"], pre, lambda t: t + f["bias"], what="pre-activation")
    print(f"pre-activation: std {float(pre.std()):.2f}, max {float(pre.abs().max()):.2f}")
    assert 1.5 < float(pre.std()) < 2.5 and float(pre.abs().max()) <= 16.0
    if act == "gelu":
        # fp32 in the well-conditioned form the kernel uses, max(x, 0) - |x| Phi(-|x|), with Phi from erfc.  F.gelu's own fp32 path evaluates
        # 0.5 x (1 + erf(x / sqrt 2)) and loses digits to the cancellation in 1 + erf for x < -3: 1.6 e_act on these inputs (printed below).
        # That is a property of that formula, not of fp32, and no kernel here uses it.
        x32 = pre.float()
        ref, e = F.gelu(pre), X.e_act_gelu
        got = x32.clamp_min(0) - 0.5 * x32.abs() * torch.erfc(x32.abs() * 0.7071067811865476)
        print(f"gelu: F.gelu in fp32, worst error / e_act = {float(((F.gelu(x32).double() - ref).abs() / e(ref)).max()):.3f}")
    elif act == "silu":
        half = pre.shape[1] // 2
        ref = F.silu(pre[:, :half]) * pre[:, half:]
        got = F.silu(pre[:, :half].float()) * pre[:, half:].float()
        e = X.e_act_sigmoid
    else:
        ref, got, e = torch.sigmoid(pre), torch.sigmoid(pre.float()), X.e_act_sigmoid
    ratio = float(((got.double() - ref).abs() / e(ref)).max())
    print(f"{act}: fp32 torch against fp64, worst error / e_act = {ratio:.3f}")
    assert ratio < 0.25
