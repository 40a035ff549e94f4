"""GPU: the value domain of the two attention kernels (5: the shipped mixed-stream kernel, 3: the alternate) -- scores far from 0 and
placed over the key tiles so that every branch of the online softmax is taken: a first tile far below 0 (the running max starts at 0),
far above, later tiles just under and far over the deferred-rescale threshold, rows of one wave on different paths, one tile only.
Every other attention test draws randn scores within a few units of 0.  Inputs and the fp64 reference: tests/_attention_ref.py.
Every output must be finite and within the attention tolerance of the reference.  (The fp16 library's store clamps to +-65504 and the
clamp turns a NaN of the kernel into -65504: there it is the comparison, not the finiteness check, that sees a NaN row.)"""
import pytest
import torch

import _attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARIANTS = [3, 5]


def _run(hip, qkv, variant):
    """The kernel's output for one head; the buffer starts as NaN so that a row nobody wrote fails like a NaN the kernel computed."""
    n = qkv.shape[0]
    out = torch.full((n, 64), float("nan"), dtype=qkv.dtype, device=DEV)
    hip.debug_set_attention_variant(variant)
    try:
        hip.attention(qkv.to(DEV), out, 1, n, 1)
        torch.cuda.synchronize()
    finally:
        hip.debug_set_attention_variant(5)
    return out.cpu()


def _check(got, ref, op, what):
    bad = ~torch.isfinite(got.float())
    assert not bad.any(), f"{what}: {int(bad.any(1).sum())} of {got.shape[0]} rows are not finite (first: row {int(bad.any(1).nonzero()[0])})"
    frac = R.off_by(got, ref, op)
    print(f"{what}: max error = {frac:.3f} of the tolerance")
    assert frac <= 1.0, f"{what}: max error is {frac:.2f} x the tolerance"


def _case_and_output(hip, variant, n, offsets_key, cold=None, q_zero=False):
    op = hip.operand_dtype()
    qkv, ref = R.case(op, n, offsets_key, cold, q_zero)
    out = _run(hip, qkv, variant)
    _check(out, ref, op, f"variant {variant} {offsets_key} vs fp64")
    return op, qkv, ref, out


def _check_shift(hip, variant, n, off, cold=None, q_zero=False):
    """Reference check + shift invariance: the same tensors with offset 0 have the same softmax rows, so the kernel's own two outputs must agree."""
    op, _, _, out = _case_and_output(hip, variant, n, ("uniform", off), cold, q_zero)
    qkv0, ref0 = R.case(op, n, ("uniform", 0), cold, q_zero)
    out0 = _run(hip, qkv0, variant)
    _check(out0, ref0, op, f"variant {variant} offset 0 vs fp64")
    _check(out, out0, op, f"variant {variant} offset {off} vs the kernel's own output at offset 0")
    return out


def _check_permuted(hip, variant, n, offsets_key):
    """Reference check in key order and with the keys moved across tiles: one reference for both."""
    op, qkv, ref, _ = _case_and_output(hip, variant, n, offsets_key)
    _check(_run(hip, R.permute_keys(qkv), variant), ref, op, f"variant {variant} {offsets_key}, keys permuted, vs fp64")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("off", [-160, -1024, -4096])
def test_uniform_low(hip, variant, off):
    """Every score of tile 0 below -128 log2 units: nothing has been accumulated at the first tile, so moving the running max from its
    initial 0 down to the tile's must not rescale anything (exp2(128) = inf in fp32, 0 * inf = NaN)."""
    _check_shift(hip, variant, 300, off)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("off", [160, 4096])
def test_uniform_high(hip, variant, off):
    """The other direction: the first rescale factor underflows to 0 and multiplies zeros."""
    _check_shift(hip, variant, 300, off)


@pytest.mark.parametrize("variant", VARIANTS)
def test_low_then_close(hip, variant):
    """Later tiles 2^4 above the first tile's max: under the deferred-rescale threshold, the max does not move and P rides at 2^4."""
    _case_and_output(hip, variant, 300, ("two_level", -1024, -1020))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("later", [-1000, 0])
def test_low_then_far(hip, variant, later):
    """Tile 1 rescales by 2^-24, and by less than 2^-128: the factor flushes to 0 and tile 0's share vanishes without a trace."""
    _check_permuted(hip, variant, 300, ("two_level", -1024, later))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rows", [(0,), (17,), tuple(range(16, 32)), (40, 100, 299)], ids=["row0", "row17", "rows16-31", "rows40-100-299"])
def test_some_rows_cold(hip, variant, rows):
    """Only some queries see the -1024: the move of the max is per lane, the row sums of queries n + 16 take their factor from another
    lane, and the cold rows share a wave (and the ragged last query block) with rows whose scores stay near 0."""
    _check_shift(hip, variant, 300, -1024, cold=rows)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("step", [7, 9])
def test_staircase(hip, variant, step):
    """The max climbs by ``step`` per tile over 5 tiles + 1 key: 7 stays under the threshold (2^8) on one tile and crosses it on the next,
    9 crosses it on every tile; P sits near its ceiling throughout."""
    _check_permuted(hip, variant, 5 * R.TILE + 1, ("stairs", step))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", [1, 37, 64])
def test_single_tile(hip, variant, n):
    """Tile 0 is also the last tile: the -inf of the masked keys meets the first-tile path."""
    _case_and_output(hip, variant, n, ("uniform", -1024))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("off", [0, -1024])
def test_all_equal(hip, variant, off):
    """q is zero outside channel 0: all scores of a row are exactly equal (0, or -1024), so every output row is the column mean of V."""
    op = hip.operand_dtype()
    cold = None if off else ()
    out = _check_shift(hip, variant, 300, off, cold=cold, q_zero=True)
    qkv, _ = R.case(op, 300, ("uniform", off), cold, True)
    mean_v = qkv[:, 128:].double().mean(0, keepdim=True).expand(300, 64)
    _check(out, mean_v, op, f"variant {variant} equal scores at {off} vs the column mean of V")


@pytest.mark.parametrize("cold", [None, tuple(range(16, 32))], ids=["uniform_low", "rows16-31"])
def test_split_output_forms_on_cold_rows(hip, cold):
    """The split forms of ada_attention_ex (the shipped kernel only), driven as test_attention_split_output_forms drives them, at -1024: the hi
    segment of [hi | lo] and of [hi | lo8 | hi8] is the plain output bit for bit, |lo| <= ulp(hi) / 2, hi + lo is no further from the fp64
    reference than hi, and the byte segments decode to the value and its residual (that test's own helper)."""
    from test_gpu_f8 import _check_bytes_against_hi_lo
    op = hip.operand_dtype()
    n, D, ld = 300, 64, 256
    seg = ld // 2
    qkv, ref = R.case(op, n, ("uniform", -1024), cold)
    plain_cpu = _run(hip, qkv, 5)
    _check(plain_cpu, ref, op, "plain output vs fp64")
    plain, q = plain_cpu.to(DEV), qkv.to(DEV)
    two = torch.zeros(n, ld, dtype=op, device=DEV)
    hip.attention(q, two, 1, n, 1, ld_out=ld, split_seg=seg)
    assert torch.equal(two[:, :D], plain)
    hi, lo = two[:, :D].float().cpu(), two[:, seg:seg + D].float().cpu()
    assert bool(torch.isfinite(lo).all())
    half_ulp = torch.finfo(op).eps / 2          # 2^-11 for fp16
    assert float(lo.abs().max()) > 0 and bool((lo.abs() <= hi.abs() * half_ulp + 6.0e-8).all())
    e_hi, e_two = float((hi.double() - ref).abs().mean()), float((hi.double() + lo.double() - ref).abs().mean())
    print(f"mean |err| of hi {e_hi:.3e}, of hi + lo {e_two:.3e}")
    assert e_two <= e_hi
    f8 = torch.zeros(n, ld, dtype=op, device=DEV)
    hip.attention(q, f8, 1, n, 1, ld_out=ld, split_seg=-seg)
    b = f8.cpu().contiguous().view(torch.uint8).reshape(n, 2 * ld)
    assert torch.equal(b[:, :2 * D].contiguous().view(op), plain_cpu)
    _check_bytes_against_hi_lo(b[:, 2 * seg:2 * seg + D], b[:, 3 * seg:3 * seg + D], hi, lo, "attention at -1024")
    assert float(two[:, D:seg].abs().max()) == 0.0 and float(two[:, seg + D:].abs().max()) == 0.0, "pad columns written"
    for a, z in ((2 * D, 2 * seg), (2 * seg + D, 3 * seg), (3 * seg + D, 4 * seg)):
        assert int(b[:, a:z].max()) == 0, "pad bytes written"
