"""Inputs and the fp64 reference of the value-domain attention tests (tests/test_gpu_attention_values.py).

The kernels take q pre-scaled (head_dim**-0.5 * log2(e) folded in), so q k^T is the score in log2 units.  A case places an exact
offset on the scores through channel 0 alone: q[r, 0] = 16 for the "cold" rows r and k[j, 0] = off_j / 16, every other channel a small
random number.  16 and off_j / 16 are exact in fp16 and in bf16 (checked when a case is built), so the kernel sees off_j + (random part)
and a uniform offset is a pure softmax shift.  |off| <= 4096: up to there an fp32 evaluation of the reference formula itself stays far
inside the tolerance (asserted once per case below), so a kernel that keeps fp32 scores can meet it."""
import functools

import torch

LOG2E = 1.4426950408889634
TILE = 64          # keys per tile of both kernels
SEED = 71
MAX_OFF = 4096.0


def tolerance(op):
    """The project's attention tolerance (tests/test_gpu_kernels.py): atol, rtol."""
    return 2e-3, (1e-2 if op == torch.bfloat16 else 3e-3)


def uniform(off):
    return lambda n: torch.full((n,), float(off))


def two_level(first, later):
    """Tile 0 at ``first``, every later tile at ``later``."""
    return lambda n: torch.where(torch.arange(n) < TILE, float(first), float(later))


def stairs(step):
    """Tile t at ``step * t``."""
    return lambda n: (torch.arange(n) // TILE).float() * float(step)


def softmax_v(qkv, dtype):
    t = qkv.to(dtype)
    p = ((t[:, :64] @ t[:, 64:128].T) / LOG2E).softmax(-1)
    return p @ t[:, 128:]


def off_by(got, ref, op):
    """Largest error in units of the tolerance (> 1: out of tolerance); inf where ``got`` is not finite."""
    atol, rtol = tolerance(op)
    got, ref = got.double().cpu(), ref.double().cpu()
    frac = (got - ref).abs() / (atol + rtol * ref.abs())
    frac = torch.where(torch.isfinite(got), frac, torch.full_like(frac, float("inf")))
    return float(frac.max())


def build(op, n, offsets, cold, q_zero=False):
    """qkv [n, 192] in the operand type for one head: ``offsets(n)`` on the keys, seen by the rows in ``cold`` (None: every row).
    q_zero: q is zero outside channel 0, so a cold row's scores are exactly the offsets and every other row's exactly 0."""
    g = torch.Generator().manual_seed(SEED)
    qkv = torch.randn(n, 192, generator=g) * 0.3
    off = offsets(n)
    assert float(off.abs().max()) <= MAX_OFF
    if q_zero:
        qkv[:, :64] = 0.0
    qkv[:, 0] = 0.0
    qkv[:, 64] = off / 16.0
    rows = torch.arange(n) if cold is None else torch.tensor(list(cold), dtype=torch.long)
    if rows.numel():
        assert int(rows.max()) < n
        qkv[rows, 0] = 16.0
    r = qkv.to(op)
    assert torch.equal(r[:, 0].float(), qkv[:, 0]) and torch.equal(r[:, 64].float(), qkv[:, 64]), "the offsets are not exact in the operand type"
    return r


@functools.lru_cache(maxsize=None)
def case(op, n, offsets_key, cold=None, q_zero=False):
    """(qkv, fp64 reference) of a case, built once and shared by the tests that use it: neither tensor may be modified.
    offsets_key = (builder name, *arguments), e.g. ("two_level", -1024, -1000)."""
    offsets = {"uniform": uniform, "two_level": two_level, "stairs": stairs}[offsets_key[0]](*offsets_key[1:])
    qkv = build(op, n, offsets, cold, q_zero)
    ref = softmax_v(qkv, torch.float64)
    # the reference alone must sit well inside the tolerance: fp32 torch against fp64, at most 10 % of it
    frac = off_by(softmax_v(qkv, torch.float32), ref, op)
    assert frac <= 0.1, f"fp32 evaluation of the reference is {frac:.3f} of the tolerance away from fp64: the case is too hard to judge a kernel by"
    return qkv, ref


def permute_keys(qkv, seed=5):
    """The same problem with its (key, value) rows in another order (queries stay): a fixed permutation that moves keys across tiles."""
    n = qkv.shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    if n > TILE:
        assert bool(((perm // TILE) != (torch.arange(n) // TILE)).any())
    out = qkv.clone()
    out[:, 64:] = qkv[perm, 64:]
    return out
