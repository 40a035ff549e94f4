"""GPU: the geometry of the two attention kernels (5: the shipped mixed-stream kernel, 3: the alternate) -- DESIGN.md, "Geometry sweeps: attention".
Every length 1 ... 321 (every residue mod 64 at one to six key tiles, both parities of the two-tile loop, the query-block edges 128 and 256, every
count of inactive waves) plus 383 - 385, 1370, 1409 and 5330, and (batch, heads) layouts whose block counts put the XCD remap on each of its branches,
on the two input families of tests/_attention_geometry.py: routed rows must come back BIT FOR BIT (a failure names the key whose row arrived instead),
census rows within (u + 4 2^-24) c_d / N.  On every launch qkv ends in a row of NaN and the output buffer in a guard row (and guard columns where
ld_out > heads 64) that must come back untouched.  The premises and the sensitivity of this list are checked without a GPU by
tests/test_attention_geometry_cpu.py.

A test loops over its lengths itself: about 2000 tiny launches in all, a few seconds per test; each prints its launches and seconds."""
import contextlib
import time

import pytest
import torch

import _attention_geometry as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARIANTS = [3, 5]
KERNEL = {3: "attention_kernel_v3", 5: "attention_kernel_mix"}


@contextlib.contextmanager
def _variant(hip, variant):
    hip.debug_set_attention_variant(variant)
    try:
        yield
    finally:
        hip.debug_set_attention_variant(5)


def _launch(hip, qkv, B, N, heads, ld_out=0, split_seg=0):
    """One launch on a guarded pair of buffers; returns the whole output buffer [B N + 1, ld] on the CPU."""
    op = hip.operand_dtype()
    ld = ld_out or heads * G.HD
    q = qkv.to(op).to(DEV)
    out = torch.full((B * N + 1, ld), G.SENTINEL, dtype=op, device=DEV)
    hip.attention(q, out, B, N, heads, ld_out=ld_out, split_seg=split_seg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(q[-1]).all()), "the row behind qkv was written"
    return out.cpu()


def _guards(buf, rows, cols, what):
    """The guard row and the columns from ``cols`` on hold the sentinel."""
    assert bool((buf[rows:] == G.SENTINEL).all()), f"{what}: the row behind the last token was written"
    assert bool((buf[:, cols:] == G.SENTINEL).all()), f"{what}: columns behind the row's {cols} were written"


def _summarise(fails, what, ran):
    if fails:
        names = ", ".join(str(f[0]) for f in fails[:40])
        raise AssertionError(f"{what}: {len(fails)} of {ran} cases fail: {names}{' ...' if len(fails) > 40 else ''}\n  " + "\n  ".join(f"{f[0]}: {f[1]}" for f in fails[:8]))


@pytest.mark.parametrize("variant", VARIANTS)
def test_routing_every_length(hip, variant):
    t0, fails = time.time(), []
    with _variant(hip, variant):
        for N in G.LENGTHS:
            case = G.routing(1, 1, N)
            buf = _launch(hip, case["qkv"], 1, N, 1)
            _guards(buf, N, G.HD, f"variant {variant}, N = {N}")
            msg = G.routing_failure(case, buf[:N], 1, 1, N)
            if msg:
                fails.append((N, msg))
    print(f"{KERNEL[variant]}: routing over {len(G.LENGTHS)} lengths, {len(G.LENGTHS)} launches, {time.time() - t0:.1f} s")
    _summarise(fails, f"variant {variant}, routing, N", len(G.LENGTHS))


@pytest.mark.parametrize("variant", VARIANTS)
def test_census_every_length(hip, variant):
    op = hip.operand_dtype()
    t0, fails, worst, ran = time.time(), [], 0.0, 0
    with _variant(hip, variant):
        for N in G.LENGTHS:
            for which in (0, 1):
                case = G.census(N, which)
                buf = _launch(hip, case["qkv"], 1, N, 1)
                ran += 1
                _guards(buf, N, G.HD, f"variant {variant}, N = {N}, census {which}")
                ratio = G.census_error(case, buf[:N], op)
                worst = max(worst, ratio)
                if not ratio <= 1.0:
                    fails.append(((N, which), G.census_failure(case, buf[:N], op, N)))
    print(f"{KERNEL[variant]}: census over {len(G.LENGTHS)} lengths, {ran} launches, worst error = {worst:.3f} of its bound, {time.time() - t0:.1f} s")
    _summarise(fails, f"variant {variant}, census, (N, launch)", ran)


@pytest.mark.parametrize("variant", VARIANTS)
def test_routing_layouts(hip, variant):
    t0, fails = time.time(), []
    with _variant(hip, variant):
        for B, heads, N in G.LAYOUTS:
            case = G.routing(B, heads, N)
            buf = _launch(hip, case["qkv"], B, N, heads)
            _guards(buf, B * N, heads * G.HD, f"variant {variant}, (B, heads, N) = {(B, heads, N)}")
            msg = G.routing_failure(case, buf[:B * N], B, heads, N)
            if msg:
                nblk = G.n_blocks(B, heads, N)
                fails.append(((B, heads, N), f"{nblk} blocks ({G.remap_class(nblk)}): {msg}"))
    print(f"{KERNEL[variant]}: routing over {len(G.LAYOUTS)} layouts, block counts {[G.n_blocks(*lay) for lay in G.LAYOUTS]}, {time.time() - t0:.1f} s")
    _summarise(fails, f"variant {variant}, routing, (B, heads, N)", len(G.LAYOUTS))


@pytest.mark.parametrize("variant", VARIANTS)
def test_routing_output_forms(hip, variant):
    """Strided plain, [hi | lo] and [hi | lo8 | hi8] rows of routed values: the hi segment is the plain output, the residual segments are zero (the
    value is exact), the hi8 bytes are the value in e5m2 at byte h 64 + column of its segment, and nothing else in the buffer changes.  With variant 3
    selected the library runs the split forms on the mixed-stream kernel (the alternate writes the plain form only): the printed line says which ran."""
    op = hip.operand_dtype()
    t0, ran = time.time(), 0
    sent = torch.full((1,), G.SENTINEL, dtype=op).view(torch.uint8)          # the sentinel's two bytes
    with _variant(hip, variant):
        for B, heads, N in G.FORM_LAYOUTS:
            D, rows = heads * G.HD, B * N
            case = G.routing(B, heads, N)
            plain = _launch(hip, case["qkv"], B, N, heads)[:rows]
            ran += 1
            msg = G.routing_failure(case, plain, B, heads, N)
            assert msg is None, f"variant {variant}, {(B, heads, N)}, contiguous: {msg}"
            hi8_want = case["want"].to(torch.float8_e5m2).view(torch.uint8)
            for ld, split in G.form_cases(heads):
                seg = abs(split)
                kernel = KERNEL[5] if split else KERNEL[variant]
                what = f"{kernel}, (B, heads, N) = {(B, heads, N)}, ld_out {ld}, split_seg {split}"
                buf = _launch(hip, case["qkv"], B, N, heads, ld_out=ld, split_seg=split)
                ran += 1
                msg = G.routing_failure(case, buf[:rows, :D].contiguous(), B, heads, N)
                assert msg is None, f"{what}, hi segment: {msg}"
                assert torch.equal(buf[:rows, :D], plain), f"{what}: the hi segment is not the contiguous output"
                by = buf.view(torch.uint8).reshape(rows + 1, 2 * ld)
                written = torch.zeros(rows + 1, 2 * ld, dtype=torch.bool)
                written[:rows, :2 * D] = True
                if split > 0:
                    lo = buf[:rows, seg:seg + D]
                    assert bool((lo == 0).all()), f"{what}: {int((lo != 0).sum())} lo values are not zero"
                    written[:rows, 2 * seg:2 * (seg + D)] = True
                elif split < 0:
                    lo8, hi8 = by[:rows, 2 * seg:2 * seg + D], by[:rows, 3 * seg:3 * seg + D]
                    assert bool(((lo8 == 0x00) | (lo8 == 0x80)).all()), f"{what}: {int(((lo8 != 0) & (lo8 != 0x80)).sum())} lo8 bytes are not a zero"
                    if not torch.equal(hi8, hi8_want):
                        r, c = (int(x) for x in (hi8 != hi8_want).nonzero()[0])
                        raise AssertionError(f"{what}: {int((hi8 != hi8_want).sum())} hi8 bytes differ; first at row {r}, byte {c} (head {c // G.HD}, column {c % G.HD}): "
                                             f"got {int(hi8[r, c]):#04x}, want {int(hi8_want[r, c]):#04x}")
                    written[:rows, 2 * seg:2 * seg + D] = True
                    written[:rows, 3 * seg:3 * seg + D] = True
                untouched = by[~written].view(-1, 2)
                assert bool((untouched == sent.view(1, 2)).all()), f"{what}: {int((untouched != sent.view(1, 2)).any(1).sum())} guard values outside the written segments changed"
                print(f"  {what}: ok")
    print(f"variant {variant}: output forms on {len(G.FORM_LAYOUTS)} layouts, {ran} launches, {time.time() - t0:.1f} s")
