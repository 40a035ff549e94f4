"""Geometry sweep of ada_igemm's index arithmetic on the device ("Geometry sweeps"; cases and restatements in tests/_igemm_geometry.py,
judged without a GPU by tests/test_igemm_geometry_cpu.py).

Source side: the 3x3 walk's row base (two reciprocal divisions, stride 1 / 2, minimal and pitched Hp / Wp, divisor 1), the tap walk of both main
loops of the 256x256 tile, the masked tap union of an N-tile.  Destination side: MAP_PAD through pad_start / pad_step on both PadWalk users and
through the general paths, MAP_TOKEN, MAP_SHUFFLE, the split stores behind the walked address -- on every tile, at map widths on both sides of every
walk step.  Inputs are exactly representable (tests/_exact.py): every comparison is bit for bit against an fp64 convolution / product, and it is made
on the WHOLE buffer: outputs are pre-filled with NaN where the launch must write and with a sentinel in the border, the cls rows, guard columns
behind N and one whole guard image behind the last, so a stray store and a missing one both show.  Sources hold NaN in every pitch row / column and
in an extra image: a walk that leaves its window poisons the sum."""
import pytest
import torch

import _exact as X
import _igemm_geometry as G
from test_gpu_kernels import _check_tile

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ids(cases):
    return [c.id for c in cases]


def _compare(got, want, case, what):
    """Whole buffers, raw bits (bytes for the [hi | lo8 | hi8] form); the message says how many rows stayed unwritten and how many guards were hit."""
    got, want = got.cpu(), want.cpu()
    raw = got.dtype == torch.uint8
    if torch.equal(got, want) if raw else torch.equal(X._raw(got), X._raw(want)):
        return
    g, w = got.float(), want.float()
    bad = (got != want) if raw else (g != w) & ~(torch.isnan(g) & torch.isnan(w))
    rows = bad.any(1).nonzero().flatten()
    detail = "" if raw else (f"; {int((torch.isnan(g) & ~torch.isnan(w)).any(1).sum())} rows left unwritten (NaN), "
                             f"{int(((w == G.SENTINEL) & (g != G.SENTINEL)).any(1).sum())} rows with a sentinel (border / guard) overwritten")
    raise AssertionError(f"{case.id} {what}: {int(bad.sum())} of {bad.numel()} cells differ in {rows.numel()} buffer rows (first {rows[:8].tolist()}){detail}")


def _launch(hip, case, d, op):
    """One launch into freshly pre-filled buffers; returns (operand-typed buffer, fp32 buffer)."""
    maps = dict(PLAIN=hip.MAP_PLAIN, PAD=hip.MAP_PAD, TOKEN=hip.MAP_TOKEN, SHUFFLE=hip.MAP_SHUFFLE)
    kw = dict(M=case.M, N=case.N, K=case.K, A=G.a_buffer(case, d).to(op).to(DEV), lda=G.C, W=d["W"].to(op).to(DEV), bias=d["bias"].to(DEV),
              map_h=case.map_h, map_w=case.map_w)
    flags = hip.EP_BIAS
    if case.conv:
        kw.update(a_mode=hip.A_CONV3, conv=case.conv)
    if case.masked:
        kw.update(tap_cols=case.c, tap_mask=list(d["masks"]))
    if case.res:
        flags |= hip.EP_RESIDUAL
        if case.Np:
            kw.update(res=d["pos"].to(DEV), ldr=case.N, res_row_mod=case.Np, res_row_off=1)
        else:
            kw.update(res=d["res"].to(DEV), ldr=case.N)
    out_op = out_f32 = None
    if case.has_op:
        out_op = G.op_prefill(case).to(op).to(DEV)
        kw.update(out_op=out_op, ldo_op=case.ldo_op, map_op=maps[case.map_op], split_seg=case.split * case.N)
        if case.relu:
            flags |= hip.EP_RELU_OP
        if case.map_op == "SHUFFLE":
            kw.update(shuffle_s=case.s, shuffle_c=case.c)
    if case.has_f32:
        out_f32 = G.f32_prefill(case).to(DEV)
        kw.update(out_f32=out_f32, ldo_f32=case.ldo_f32, map_f32=maps[case.map_f32])
    if case.out == "tail":
        flags |= hip.EP_TAIL
        kw.update(tail_w=d["tw"].to(DEV), tail_b=0.25)
    hip.igemm(flags=flags, **kw)
    return out_op, out_f32


def _check(case, d, v, op, out_op, out_f32, what):
    if case.has_op:
        got = out_op.cpu()
        if case.split < 0:
            got = got.view(torch.uint8).reshape(got.shape[0], 2 * case.ldo_op)
        _compare(got, G.expected_op(case, v, op), case, what + " operand-typed buffer")
    if case.has_f32:
        _compare(out_f32, G.expected_f32(case, d["dot"] if case.out == "tail" else v), case, what + " fp32 buffer")


def _run(hip, forced_tile, case, unforced_too=False):
    op = hip.operand_dtype()
    if case.split < 0 and op != torch.float16:
        pytest.skip("the [hi | lo8 | hi8] form exists for fp16 operands only")
    d = G.data(case)
    v, mag = G.values(case, d)
    X.assert_exact_budget(mag=mag, unit=d["unit"], ref=v, what=case.id)
    if case.out == "tail":
        X.assert_exact_budget(mag=d["dot_mag"], unit=2.0 ** -9, ref=d["dot"], what=case.id + " dot")
    t = G.TILES[case.tile]
    forced_tile(t.cfg, t.variant)
    out_op, out_f32 = _launch(hip, case, d, op)
    if case.masked and t.variant == 16:
        assert hip.debug_last_tile() == t.cfg          # a masked walk stays on the 8-wave loop
    else:
        _check_tile(hip, t.cfg, t.variant)
    _check(case, d, v, op, out_op, out_f32, f"forced tile {case.tile}")
    if unforced_too and case.N <= 64:
        # the launcher's own choice: N <= 32 -> the 256x32 tile, N <= 64 -> the 128x64 tile (no debug hook between the caller and the defect)
        hip.debug_set_tile(-1)
        hip.debug_set_variant(0)
        out_op, out_f32 = _launch(hip, case, d, op)
        want = 0 if case.N <= 32 else 1
        assert hip.debug_last_tile() % 100 == want, f"{case.id}: unforced launch took tile code {hip.debug_last_tile()}, expected {want}"
        _check(case, d, v, op, out_op, out_f32, f"unforced (tile {want})")


PAD_OP, PAD_F32, PAD_SPLIT = G.by_family("pad_op"), G.by_family("pad_f32res"), G.by_family("pad_split")
STRIDE2, PITCHED, SHUFFLE, TOKEN, TAPS = G.by_family("stride2"), G.by_family("pitched", "tail"), G.by_family("shuffle"), G.by_family("token"), G.by_family("taps")


@pytest.mark.parametrize("case", PAD_OP, ids=_ids(PAD_OP))
def test_padded_map_operand_only(hip, forced_tile, case):
    """conv3x3 + bias + ReLU into the interior of a zero-bordered grid: the operand-only PadWalk user (step 8, 16 on the 256x32 tile) for maps at least
    a step wide, the general 8-column path below that and on ragged tiles, the 4-column path for ldo_op % 8 == 4."""
    _run(hip, forced_tile, case, unforced_too=True)


@pytest.mark.parametrize("case", PAD_F32, ids=_ids(PAD_F32))
def test_padded_map_fp32_residual_and_operand_copy(hip, forced_tile, case):
    """The same geometry with fp32 output + residual + ReLU'd operand copy: the second PadWalk user (step 4, 8 on the 256x32 tile) and the general
    4-column path."""
    _run(hip, forced_tile, case, unforced_too=True)


@pytest.mark.parametrize("case", PAD_SPLIT, ids=_ids(PAD_SPLIT))
def test_padded_map_split_stores_share_the_walked_address(hip, forced_tile, case):
    """[hi | lo] and [hi | lo8 | hi8] behind both PadWalk users, next to the steps."""
    _run(hip, forced_tile, case, unforced_too=True)


@pytest.mark.parametrize("case", STRIDE2, ids=_ids(STRIDE2))
def test_stride2_source_walk(hip, forced_tile, case):
    """Stride 2 from odd and even grids down to 1x1, minimal and pitched Hp / Wp, both main loops of the 256x256 tile, to a padded Ho x Wo grid and to fp32."""
    _run(hip, forced_tile, case)


@pytest.mark.parametrize("case", PITCHED, ids=_ids(PITCHED))
def test_stride1_pitched_source_tiny_grids(hip, forced_tile, case):
    """Stride 1 on a pitched input, Ho Wo = 1 and Wo = 1 included (divisor 1 of the reciprocal division); plain outputs on interior and ragged tiles,
    and the tail epilogue on its two tiles."""
    _run(hip, forced_tile, case)


@pytest.mark.parametrize("case", SHUFFLE, ids=_ids(SHUFFLE))
def test_shuffle_map(hip, forced_tile, case):
    """Pixel shuffle by 2 and 4 from coarse grids down to 1x1, shuffle_c 8 / 48 (8-column path) and 12 (4-column path), every tile, ragged M."""
    _run(hip, forced_tile, case)


@pytest.mark.parametrize("case", TOKEN, ids=_ids(TOKEN))
def test_token_map(hip, forced_tile, case):
    """Rows skip the cls slot of every image (Np 1, 2 and around 256: tiles straddle and meet image borders); fp32 with the row-modulo residual, and operand-only."""
    _run(hip, forced_tile, case)


@pytest.mark.parametrize("case", TAPS, ids=_ids(TAPS))
def test_masked_tap_walk(hip, forced_tile, case):
    """tap_cols / tap_mask: N-tiles that span one phase, several and all phases walk the union of their phases' taps, on grids down to 1x1."""
    _run(hip, forced_tile, case)
