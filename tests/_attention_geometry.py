"""Inputs, expected values and an fp32 emulation for the attention geometry sweep ("Geometry sweeps: attention").

Two input families on which ANY correct softmax(q k^T) v has one derivable result, so that a test can say which key or column went where:

  R  routing.  Key j of (b, h) carries the code of (j + 997 (b heads + h)) mod 65536: its 16 bits as +-1, four times over the 64 channels; k_j = 4 code(j),
     q_i = 4 code(pi(i)) with pi a seeded permutation per (b, h) (q is the pre-scaled one: q k^T is the score in log2 units).  A score is
     16 (64 - 8 hamming) = 1024 - 128 hamming: a multiple of 128 within +-1024, exact in fp32 and as an fp16 / bf16 running maximum; key pi(i) scores 1024
     and every other key at most 896.  Every foreign weight is <= 2^-128 of the designated one, l rounds to the designated weight, every rescale is a
     power of two: the output row is V[pi(i)] BIT FOR BIT in either operand type, for any flash-style order.  V holds integers of magnitude 1 ... 7
     (exact in fp16, bf16 and e5m2), rows pairwise distinct within a launch, so a wrong row names the key that arrived.
  C  census.  q = 0: every score is exactly 0, every valid key weighs exactly 1, k (Gaussian) must not matter.  V[j, d] = [class(j) == d] with
     class = j mod 64 (launch 0) or j // 64 (launch 1; j // 128 above 4096 keys): out[i, d] = c_d / N with c_d the number of valid keys of class d.
     A key dropped, doubled or read from behind the end moves one c_d, or N, by one.  Bound (census_bound): (u + 4 2^-24) c_d / N, u = half an
     operand ulp -- one reciprocal (<= 1 ulp of fp32), one product (1/2 ulp), the factor two of slack used elsewhere in this suite, one conversion.

emulate() is a tiled online softmax in fp32 that follows the two kernels of csrc/ada_attention.hip where they differ in what rounds (mode "v3": the
running maximum kept in the operand type, l from the unrounded exponentials, keys behind the end staged by clamping; mode "mix": fp32 maximum, l from
the operand-typed P, keys behind the end read as zero) and addresses the flat qkv buffer with the kernels' strides.  MUTANTS are switchable faults of
that emulation; tests/test_attention_geometry_cpu.py shows that the case lists below catch every one of them.  Builders are cached and shared by the
CPU and the GPU file: what they return must not be modified."""
import functools

import torch

HD = 64
QBLK = 128          # query rows per workgroup
TILE = 64           # keys per tile
SALT = 997
SENTINEL = 1024.0   # behind and between everything a launch may write: no routing value (|v| <= 7) and no census value (<= 1)
OP_TYPES = (torch.float16, torch.bfloat16)
LOG2E = 1.4426950408889634

LENGTHS = tuple(range(1, 322)) + (383, 384, 385, 1370, 1409, 5330)
LAYOUTS = ((3, 5, 130), (2, 3, 257), (1, 16, 65), (5, 1, 129), (2, 6, 64), (3, 2, 200), (7, 1, 1), (1, 7, 1), (1, 3, 1))      # B, heads, N
FORM_LAYOUTS = ((3, 5, 130), (1, 1, 65), (2, 3, 257))
GAUSS_CASES = ((2, 1370, 2), (1, 64, 1), (1, 65, 3), (1, 1, 1), (3, 200, 6), (1, 129, 1), (1, 1409, 1), (1, 5330, 1))       # B, N, heads of test_attention_variants


def n_blocks(B, heads, N):
    return (N + QBLK - 1) // QBLK * B * heads


def form_cases(heads):
    """(ld_out, split_seg) of the output-form cases for a layout: the strided plain form at three strides, [hi | lo] and [hi | lo8 | hi8] at two.
    seg = D + 8 leaves pad columns behind every segment."""
    D = heads * HD
    seg = D + 8
    return [(D + 8, 0), (2 * seg, 0), (2 * seg + 16, 0), (2 * seg, seg), (2 * seg + 16, seg), (2 * seg, -seg), (2 * seg + 16, -seg)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the block remap, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def remap(bid, nblk, first_branch_only=False):
    """Launch block id -> logical block id (bh * nqb + qb): blocks are dealt round-robin to 8 XCDs, and the logical ids one XCD gets are contiguous."""
    q, r = nblk >> 3, nblk & 7
    xcd, idx = bid & 7, bid >> 3
    if xcd < r or first_branch_only:
        return xcd * (q + 1) + idx
    return r * (q + 1) + (xcd - r) * q + idx


def remap_class(nblk):
    return "nblk < 8" if nblk < 8 else ("nblk mod 8 = 0" if nblk % 8 == 0 else "nblk mod 8 != 0")


# ---------------------------------------------------------------------------------------------------------------------------------
# family R
# ---------------------------------------------------------------------------------------------------------------------------------
def code(idx):
    """int64 [...] -> [..., 64] of +-1: bit (c mod 16) of idx mod 65536 at channel c."""
    bits = ((idx.unsqueeze(-1) % 65536) >> torch.arange(16)) & 1
    return (bits * 2 - 1).float().repeat(*([1] * idx.dim()), 4)


@functools.lru_cache(maxsize=None)
def routing(B, heads, N):
    """dict(qkv fp32 [B N + 1, 3 D] with a NaN row behind the last token, perm int64 [B, heads, N], v fp32 [B, heads, N, 64], want fp32 [B N, D])."""
    D = heads * HD
    g = torch.Generator().manual_seed(100003 * B + 1009 * heads + N)
    perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B * heads)]).view(B, heads, N)
    if N > TILE:
        assert bool(((perm // TILE) != (torch.arange(N) // TILE)).any(-1).all()), "a permutation moves no key across tiles"
    mag = torch.randint(1, 8, (B, heads, N, HD), generator=g)
    sign = torch.randint(0, 2, (B, heads, N, HD), generator=g) * 2 - 1
    v = (mag * sign).float()
    salt = (SALT * torch.arange(B * heads)).view(B, heads, 1)
    k = 4.0 * code(torch.arange(N).view(1, 1, N) + salt)            # [B, heads, N, 64]
    q = 4.0 * code(perm + salt)
    to_rows = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, D)      # noqa: E731
    qkv = torch.full((B * N + 1, 3 * D), float("nan"))
    qkv[:-1] = torch.cat([to_rows(q), to_rows(k), to_rows(v)], 1)
    want = to_rows(torch.gather(v, 2, perm.unsqueeze(-1).expand(B, heads, N, HD)))
    return dict(qkv=qkv, perm=perm, v=v, want=want)


def arriving_key(case, row64):
    """Which key's V row is ``row64`` (64 values)?  (b, h, j) of the first match within the launch, or None."""
    v = case["v"]
    hit = (v == row64.float().view(1, 1, 1, HD)).all(-1).nonzero()
    return tuple(int(x) for x in hit[0]) if hit.numel() else None


def routing_failure(case, got, B, heads, N):
    """None if ``got`` [B N, D] equals the routed rows bit for bit, else the message: the first bad (b, h, row, column) and which key's row arrived."""
    want = case["want"].to(got.dtype)
    if torch.equal(got, want):
        return None
    bad = ~(got == want)               # NaN counts
    r, c = (int(x) for x in bad.nonzero()[0])
    b, i, h, col = r // N, r % N, c // HD, c % HD
    src = arriving_key(case, got[r, h * HD:(h + 1) * HD])
    pi = int(case["perm"][b, h, i])
    if src is None:
        arrived = "the row that arrived is no key's V row of this launch"
    else:
        arrived = f"the row that arrived is V of (b, h, key) = {src}" + (" (the right key: single columns are wrong)" if src == (b, h, pi) else "")
    return (f"{int(bad.sum())} of {bad.numel()} elements differ, {int(bad.any(1).sum())} of {B * N} rows; first at (b, h, row, column) = ({b}, {h}, {i}, {col}): "
            f"got {float(got[r, c])!r}, want {float(want[r, c])!r} = V[key {pi}]; {arrived}")


# ---------------------------------------------------------------------------------------------------------------------------------
# family C
# ---------------------------------------------------------------------------------------------------------------------------------
def census_class(N, which):
    j = torch.arange(N)
    if which == 0:
        return j % 64
    return j // (128 if N > 4096 else 64)


@functools.lru_cache(maxsize=None)
def census(N, which):
    """One head, one image: dict(qkv fp32 [N + 1, 192] with a NaN row behind, count int64 [64], want fp64 [64] = count / N)."""
    g = torch.Generator().manual_seed(7000 + 2 * N + which)
    cls = census_class(N, which)
    assert int(cls.max()) < HD
    qkv = torch.full((N + 1, 3 * HD), float("nan"))
    qkv[:-1, :HD] = 0.0
    qkv[:-1, HD:2 * HD] = torch.randn(N, HD, generator=g)
    qkv[:-1, 2 * HD:] = (cls.view(N, 1) == torch.arange(HD).view(1, HD)).float()
    count = torch.bincount(cls, minlength=HD)
    return dict(qkv=qkv, count=count, want=count.double() / N)


def census_bound(want, op):
    u = 2.0 ** -11 if op == torch.float16 else 2.0 ** -8
    return (u + 4.0 * 2.0 ** -24) * want


def census_error(case, got, op):
    """Largest |got - c_d / N| in units of its bound over the rows of ``got`` [N, 64]; inf where a class without keys is not exactly 0 or a value is not finite."""
    want = case["want"].view(1, HD)
    lim = census_bound(want, op)
    err = (got.double() - want).abs()
    inf = torch.full_like(err, float("inf"))
    ratio = torch.where(want > 0, err / lim.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    ratio = torch.where(torch.isfinite(got.double()), ratio, inf)
    return float(ratio.max())


def census_failure(case, got, op, N):
    ratio = census_error(case, got, op)
    if ratio <= 1.0:
        return None
    want = case["want"].view(1, HD)
    err = (got.double() - want).abs()
    bad = ~(err <= census_bound(want, op))
    r, c = (int(x) for x in bad.nonzero()[0])
    implied = float(got[r, c]) * N
    return (f"{int(bad.sum())} of {bad.numel()} elements beyond the bound (worst {ratio:.3g} x); first at (row, column) = ({r}, {c}): got {float(got[r, c])!r}, "
            f"want {int(case['count'][c])} / {N} = {float(want[0, c])!r}; got x N = {implied:.3f} keys of class {c}")


# ---------------------------------------------------------------------------------------------------------------------------------
# Gaussian inputs of tests/test_gpu_kernels.py test_attention_variants (for comparison only)
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gaussian(B, N, heads, op):
    D = heads * HD
    g = torch.Generator().manual_seed(33)
    qkv = torch.randn(B * N, 3 * D, generator=g).to(op)
    qkv[:, :D] *= 0.125 * LOG2E
    qkv = qkv.to(op)
    t = qkv.double().reshape(B, N, 3, heads, HD).permute(2, 0, 3, 1, 4)
    p = ((t[0] @ t[1].transpose(-2, -1)) / LOG2E).softmax(-1)
    ref = (p @ t[2]).transpose(1, 2).reshape(B * N, D)
    return qkv, ref


def gaussian_miss(got, ref, op):
    """(share of the elements outside the project's attention tolerance, worst error in units of it); NaN counts as outside."""
    atol, rtol = 2e-3, (1e-2 if op == torch.bfloat16 else 3e-3)
    frac = (got.double() - ref).abs() / (atol + rtol * ref.abs())
    frac = torch.where(torch.isfinite(frac), frac, torch.full_like(frac, float("inf")))
    return float((frac > 1.0).double().mean()), float(frac.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "mask_gt": "tail mask > instead of >=",
    "drop_last": "last key dropped",
    "swap_slots": "two k-slots of P swapped against V inside one 16-key step",
    "v_head0": "V taken from head 0 for every head",
    "batch_stride": "batch stride computed from N rounded up to 64",
    "no_rescale": "O not rescaled when the maximum moves",
    "remap": "block remap with the xcd < r branch used for all blocks",
}
MODES = ("v3", "mix")
RESCALE_THR = 8.0


def _online(Q, K, V, N, op, mode, mutant):
    """fp32 online softmax of N queries over the N keys in tiles of 64.  K, V [nt 64, 64]: already staged, rows behind N as the mode reads them."""
    nt = (N + TILE - 1) // TILE
    m, l, O = torch.zeros(N), torch.zeros(N), torch.zeros(N, HD)
    first_masked = N + 1 if mutant == "mask_gt" else (N - 1 if mutant == "drop_last" else N)
    for t in range(nt):
        kt, vt = K[t * TILE:(t + 1) * TILE], V[t * TILE:(t + 1) * TILE]
        s = Q @ kt.T - m[:, None]
        if t == nt - 1:
            s[:, (t * TILE + torch.arange(TILE)) >= first_masked] = float("-inf")
        mx = s.max(1).values
        mv = (mx > RESCALE_THR) | (t == 0)
        cand = m + mx
        if mode == "v3":
            cand = cand.to(op).float()
        m_new = torch.where(mv, cand, m)
        delta = m_new - m
        alpha = torch.exp2(-delta).clamp(0.0, 1.0)
        l = l * alpha
        if mutant != "no_rescale":
            O = O * alpha[:, None]
        s = s - delta[:, None]
        m = m_new
        P = torch.exp2(s)
        Pop = P.to(op).float()
        l = l + (Pop if mode == "mix" else P).sum(1)
        if mutant == "swap_slots":
            Pop = Pop.clone()
            Pop[:, [1, 2]] = Pop[:, [2, 1]]
        O = O + Pop @ vt
    return (O * (1.0 / l)[:, None]).to(op)


def emulate(qkv, B, N, heads, op, mode="mix", mutant=None):
    """qkv: [>= B N rows, 3 D] (any float type; rounded to ``op`` first).  Returns [B N, D] in ``op``; rows of a query block that no launch block maps to stay NaN."""
    assert mode in MODES and (mutant is None or mutant in MUTANTS)
    D = heads * HD
    rs = 3 * D
    nt = (N + TILE - 1) // TILE
    n_up = nt * TILE
    flat = qkv.to(op).float().flatten()
    need = (B * n_up + TILE) * rs
    if flat.numel() < need:
        flat = torch.cat([flat, torch.full((need - flat.numel(),), float("nan"))])
    nqb = (N + QBLK - 1) // QBLK
    nblk = nqb * B * heads
    covered = {remap(bid, nblk, mutant == "remap") for bid in range(nblk)}
    n_stride = n_up if mutant == "batch_stride" else N
    ch = torch.arange(HD).view(1, HD)
    rows = torch.arange(n_up)
    rows_live = torch.arange(N)
    out = torch.full((B * N, D), float("nan"), dtype=op)
    for bh in range(B * heads):
        b, h = divmod(bh, heads)
        base = b * n_stride * rs + h * HD
        Q = flat[base + rows_live.view(N, 1) * rs + ch]
        if mutant == "mask_gt":          # the rows behind N are read as the kernel reads them: clamped to the last key, or zero behind the buffer window
            krows = rows.clamp_max(N - 1) if mode == "v3" else rows
            K = flat[base + D + krows.view(-1, 1) * rs + ch]
            V = flat[base + 2 * D + krows.view(-1, 1) * rs + ch]
            if mode == "mix":
                K[N:], V[N:] = 0.0, 0.0
        else:                            # masked: what they hold cannot matter
            K, V = torch.zeros(n_up, HD), torch.zeros(n_up, HD)
            vbase = b * n_stride * rs + (0 if mutant == "v_head0" else h * HD) + 2 * D
            K[:N] = flat[base + D + rows_live.view(N, 1) * rs + ch]
            V[:N] = flat[vbase + rows_live.view(N, 1) * rs + ch]
        o = _online(Q, K, V, N, op, mode, mutant)
        for qb in range(nqb):
            if bh * nqb + qb in covered:
                r0, r1 = qb * QBLK, min(N, (qb + 1) * QBLK)
                out[b * N + r0:b * N + r1, h * HD:(h + 1) * HD] = o[r0:r1]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the case list, as (family, arguments) in the order the GPU tests run it
# ---------------------------------------------------------------------------------------------------------------------------------
def listed_cases():
    for N in LENGTHS:
        yield ("R", 1, 1, N, None)
    for B, heads, N in LAYOUTS:
        yield ("R", B, heads, N, None)
    for N in LENGTHS:
        yield ("C", 1, 1, N, 0)
        yield ("C", 1, 1, N, 1)


def emulated_failure(family, B, heads, N, which, op, mode, mutant=None):
    """The emulation's verdict on one listed case: None (passes the GPU test's own check) or the failure message."""
    if family == "R":
        case = routing(B, heads, N)
        return routing_failure(case, emulate(case["qkv"], B, N, heads, op, mode, mutant), B, heads, N)
    case = census(N, which)
    return census_failure(case, emulate(case["qkv"], 1, N, 1, op, mode, mutant), op, N)
