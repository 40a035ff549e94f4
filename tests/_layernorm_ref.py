"""fp64 reference, value families and the derived error budget of ada_layernorm_ex (csrc/ada_elementwise.hip layernorm_kernel<16> / <64>).

ref64 restates everything the kernel does to its fp32 input -- row selection, the un-shuffle gather with the ring subtraction, biased variance with
eps inside the root, gain / bias, the three ReLU modes, the second output -- in float64.  budget is the per-element bound on |kernel - ref64| that
follows from the kernel's fp32 arithmetic; it is derived below and fitted to nothing.  CPU only: tests/test_layernorm_ref_cpu.py pins this module
against torch and tests/_exact.py, tests/test_gpu_layernorm_values.py holds the kernels to it.

The budget.  u = 2^-24 (half an fp32 ulp, relative), mean / var the exact statistics of the fp32 row, s = sqrt(var + eps), yh = (x - mean) / s.
  * Row sum: a lane adds its float4 chunks as  s += (x + y) + (z + w)  -- four additions per chunk -- and the LPR lanes of a row meet in a
    log2(LPR)-step butterfly.  No value passes through more than  D = 4 * chunks_per_lane + log2(LPR)  additions (the longest real chain is
    chunks_per_lane + 2 + log2(LPR); the count of all four is kept so that the bound does not depend on how the compiler associates them), so
    |sum~ - sum| <= D u sum|x| to first order, the division by dim adds one rounding, the subtraction x - mean~ another of size u |x - mean|:
    |d~ - d| <= (D + 2) u max|x|  for every deviation d = x - mean, up to the second term's share.
  * Through 1 / s that is the first term,  (D + 2) u max|x| / s.
  * The variance sum squares and adds deviations over the same tree (relative D + 2 in var, half of it in s), then  / dim, + eps, sqrtf, 1 / .
    (correctly rounded: the build has no fast-math flag), the deviation's own rounding, * rstd, * w: fewer than (D + 8) roundings relative to |yh|.
    The common shift of all deviations by the mean's error moves var by its square only.
  * + bias rounds once relative to the result, and the reference itself is a few fp64 ulps off:  2 u |y|.
Together   |y - y64| <= |w| [ (D + 2) u max|x| / s + |yh| (D + 8) u ] + 2 u |y64|.
Un-shuffle rows on the ring subtract up to five tap-bias values from every input first, each rounding once at no more than  M = max(|x| + sum|tb|):
the row the statistics see is off by  n_taps u M  per element, which reaches y directly, through the mean and through s:
+ |w| n_taps u M (2 + |yh|) / s.  max|x| is taken after the subtraction.
ReLU is 1-Lipschitz and exact: the bound carries over.  The operand-typed copy adds half an operand ulp (tests/_exact.py assert_within)."""
import functools
import math
from types import SimpleNamespace

import torch

U = 2.0 ** -24
DIMS = (48, 384, 512, 516, 1024, 1536)                       # LPR 16: 48, 384, 512 (the switch); LPR 64: 516 (partial last round), 1024, 1536 (the cap)
FAMILIES = ("gauss", "offset_1e2", "offset_1e3", "offset_1e5", "massive", "tiny", "constant")
EPS = 1e-6


def lanes_per_row(dim):
    return 16 if dim <= 512 else 64


def chain_adds(dim):
    """D of the module docstring."""
    lpr = lanes_per_row(dim)
    return 4 * math.ceil((dim // 4) / lpr) + int(math.log2(lpr))


def _gen(*key):
    seed = 7919
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def family(name, rows, dim):
    """[rows, dim] fp32, fixed seed per (name, rows, dim).  Callers must not write into the cached tensor."""
    g = _gen(FAMILIES.index(name), rows, dim)
    r = torch.randn(rows, dim, generator=g)
    if name == "gauss":
        x = 3.0 * r + 0.5
    elif name == "offset_1e2":
        x = 100.0 + r
    elif name == "offset_1e3":
        x = 1000.0 + r
    elif name == "offset_1e5":
        x = 1.0e4 + 0.1 * r
    elif name == "massive":
        x = r.clone()
        pos = torch.stack([torch.randperm(dim, generator=g)[:2] for _ in range(rows)])
        x[torch.arange(rows), pos[:, 0]] = 600.0
        x[torch.arange(rows), pos[:, 1]] = -350.0
    elif name == "tiny":
        x = 1.0e-4 * r
    elif name == "constant":
        x = torch.full((rows, dim), 3.25)
    else:
        raise KeyError(name)
    return x.float().contiguous()


@functools.lru_cache(maxsize=None)
def gain_bias(dim, which=0):
    """Gaussian gain and bias, as in tests/test_gpu_kernels.py test_layernorm_plain; which = 1: the second output's."""
    g = _gen(101 + which, dim)
    return torch.randn(dim, generator=g), torch.randn(dim, generator=g)


@functools.lru_cache(maxsize=None)
def exact_family(dim, rows=21):
    """Rows the kernel must normalise to the bit with eps = 0.  Row r: half the entries m + a, half m - a in a seeded shuffle, a = 2^k (k in -3..3),
    m = j a with |j| <= 2^10.  Then every partial sum is an integer below dim (2^10 + 1) < 2^24 times a, the mean is m, the deviations are +-a, the
    sum of squares dim a^2, the variance a^2, sqrtf and the division give 1 / a, and the output is +-w + b: gain k / 1024 with |k| <= 2048, bias
    j / 1024 with |j| <= 4096, so 13 bits at most -- exact in fp32, and beyond both operand types' significands (the lo segment has something to hold)."""
    g = _gen(211, dim, rows)
    a = 2.0 ** torch.randint(-3, 4, (rows, 1), generator=g).double()
    j = torch.randint(-1024, 1025, (rows, 1), generator=g).double()
    sign = torch.ones(rows, dim, dtype=torch.float64)
    sign[:, dim // 2:] = -1.0
    sign = torch.stack([row[torch.randperm(dim, generator=g)] for row in sign])
    x = (j + sign) * a
    w = torch.randint(-2048, 2049, (dim,), generator=g).double() / 1024.0
    b = torch.randint(-4096, 4097, (dim,), generator=g).double() / 1024.0
    return SimpleNamespace(x=x.float(), a=a, m=j * a, sign=sign, w=w.float(), b=b.float(), ref=sign * w + b)


def ring_taps(fh, fw):
    """[fh, fw, 9] bool: coarse tap t = 3 dy + dx falls outside the grid for fine pixel (Y, X) (the kernel's `ring` bits)."""
    Y, X = torch.arange(fh)[:, None, None], torch.arange(fw)[None, :, None]
    dy, dx = (torch.arange(9) // 3)[None, None, :], (torch.arange(9) % 3)[None, None, :]
    return ((Y == 0) & (dy == 0)) | ((Y == fh - 1) & (dy == 2)) | ((X == 0) & (dx == 0)) | ((X == fw - 1) & (dx == 2))


def gather_rows(x, dim, rows_out, *, group_in=0, skip=0, unshuffle_s=0, grid=None, tap_bias=None):
    """The fp32 rows the kernel's statistics see, in float64: (rows [rows_out, dim], n_taps [rows_out, 1], tap_mag [rows_out, 1]).
    x: fp32 [rows_in, >= dim] (only the columns the kernel reads are used).  group_in / skip: output row r reads input row
    (r // (group_in - skip)) * group_in + skip + r % (group_in - skip).  unshuffle_s = s with grid = (fh, fw): output row (b, Y, X) reads columns
    [phase dim, (phase + 1) dim) of coarse row (b, Y // s, X // s), phase = (Y % s) s + X % s, minus tap_bias[(phase, c), t] for every tap t
    that ring_taps marks."""
    x = x.double()
    r = torch.arange(rows_out)
    zero = torch.zeros(rows_out, 1, dtype=torch.float64)
    if unshuffle_s:
        s, (fh, fw) = unshuffle_s, grid
        b, rem = r // (fh * fw), r % (fh * fw)
        Y, X = rem // fw, rem % fw
        coarse = (b * (fh // s) + Y // s) * (fw // s) + X // s
        phase = (Y % s) * s + X % s
        cols = phase[:, None] * dim + torch.arange(dim)[None, :]
        rows = x[coarse[:, None], cols]
        if tap_bias is None:
            return rows, zero, zero
        miss = ring_taps(fh, fw)[Y, X].double()                                        # [rows_out, 9]
        tb = tap_bias.double()[cols]                                                   # [rows_out, dim, 9]
        mag = (rows.abs() + (tb.abs() * miss[:, None, :]).sum(-1)).amax(1, keepdim=True)
        return rows - (tb * miss[:, None, :]).sum(-1), miss.sum(1, keepdim=True), mag
    if group_in:
        per = group_in - skip
        r = (r // per) * group_in + skip + r % per
    return x[r, :dim], zero, zero


def ref64(x, dim, w, b, eps, rows_out, *, group_in=0, skip=0, relu=0, w2=None, b2=None, out2_group=0, out2_skip=0, unshuffle_s=0, grid=None, tap_bias=None):
    """ada_layernorm_ex in float64.  eps is narrowed to fp32 first, as the argument struct does.  Returns
    f32 / op: the references of the fp32 and the operand-typed copy (relu 1: both clamped, 2: the operand copy only), pre: before the ReLU,
    out2 / pre2: the second output (rows with r % out2_group < out2_skip dropped, the rest compacted; no ReLU), keep2: its source rows,
    and the statistics budget() needs."""
    rows, ntap, tapmag = gather_rows(x, dim, rows_out, group_in=group_in, skip=skip, unshuffle_s=unshuffle_s, grid=grid, tap_bias=tap_bias)
    eps = float(torch.tensor(eps, dtype=torch.float32))
    mean = rows.mean(1, keepdim=True)
    var = ((rows - mean) ** 2).mean(1, keepdim=True)
    sig = torch.sqrt(var + eps)
    yhat = (rows - mean) / sig
    pre = yhat * w.double() + b.double()
    out = SimpleNamespace(rows=rows, mean=mean, var=var, sig=sig, yhat=yhat, xmax=rows.abs().amax(1, keepdim=True), ntap=ntap, tapmag=tapmag, dim=dim,
                          pre=pre, f32=pre.clamp_min(0) if relu == 1 else pre, op=pre.clamp_min(0) if relu in (1, 2) else pre, out2=None, pre2=None, keep2=None)
    if w2 is not None:
        keep = torch.arange(rows_out)
        if out2_group:
            keep = keep[keep % out2_group >= out2_skip]
        out.keep2 = keep
        out.pre2 = out.out2 = yhat[keep] * w2.double() + b2.double()
    return out


def budget(r, w, y64, rows=None):
    """The module docstring's bound for outputs y64 = yhat w + b of reference r (rows: the subset of r's rows that y64 holds, for the second output)."""
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    D = chain_adds(r.dim)
    yh, sig = pick(r.yhat).abs(), pick(r.sig)
    t = (D + 2) * U * pick(r.xmax) / sig + yh * (D + 8) * U + pick(r.ntap) * U * pick(r.tapmag) * (2 + yh) / sig
    return w.double().abs() * t + 2 * U * y64.double().abs()


def ulp_e5m2(x64):
    """Spacing of e5m2 at |x| (2 mantissa bits, subnormals below 2^-14)."""
    e = torch.floor(torch.log2(x64.double().abs().clamp_min(2.0 ** -14))).clamp_min(-14)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 2)
