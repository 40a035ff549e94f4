"""CPU tests of hip_ext/operands.py -- the packer, the (weight form, activation form) walk table -- and of the agreement between what PackedWeights tells
the producers of a head group's input, what Workspace allocates for it and what the group's contractions walk.
The kernels' side of the same: tests/test_gpu_operand_forms.py."""
import functools
import itertools

import pytest
import torch

import _cases
from hip_ext import engine as E
from hip_ext import operands as O

W_FORMS = (O.W_PLAIN, O.W_SPLIT3, O.W_SPLIT2, O.W_F8)
A_FORMS = (O.A_PLAIN, O.A_HILO, O.A_HILO8)
N = 8


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- packing: the bytes, decoded here by the layouts include/ada_hip.h states ---------------------------------------------------
@pytest.mark.parametrize("op", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("taps,k", [(1, 128), (1, 48), (1, 100), (9, 64), (9, 128), (9, 48)])
@pytest.mark.parametrize("form", W_FORMS)
def test_pack_lays_out_every_form(form, taps, k, op):
    seg = (k + 63) // 64 * 64
    g = torch.Generator().manual_seed(17 * taps + k)
    w = torch.randn(N, taps * k, generator=g) * 0.3
    w[0, 0] = 0.0
    if form == O.W_F8 and seg % 128:
        with pytest.raises(AssertionError):      # 128-element granularity of the fp8 matrix instruction
            O.pack(w, form, op, taps)
        return
    p = O.pack(w, form, op, taps)
    assert (p.form, p.seg, p.taps) == (form, seg, taps) and p.t.dtype == op and p.t.is_contiguous()
    wp = torch.zeros(N, taps, seg)
    wp[..., :k] = w.reshape(N, taps, k)
    hi = wp.to(op)                                   # rounded once to the operand type
    lo = (wp - hi.float()).to(op)                    # the rounded remainder
    slots = {O.W_PLAIN: 1, O.W_SPLIT3: 3, O.W_SPLIT2: 2, O.W_F8: 2}[form]
    assert p.t.shape == (N, taps * slots * seg)
    per_tap = p.t.reshape(N, taps, slots * seg)
    assert torch.equal(_bits(per_tap[..., :seg]), _bits(hi)), "segment 0 of every tap: w_hi"
    assert int(_bits(per_tap[..., k:seg]).abs().max()) == 0 if seg > k else True, "K is padded with zeros"
    if form == O.W_PLAIN:
        assert p.f8_scales == 0
    elif form == O.W_SPLIT3:
        assert torch.equal(_bits(per_tap[..., seg:2 * seg]), _bits(hi)) and torch.equal(_bits(per_tap[..., 2 * seg:]), _bits(lo)) and p.f8_scales == 0
    elif form == O.W_SPLIT2:
        assert torch.equal(_bits(per_tap[..., seg:]), _bits(lo)) and p.f8_scales == 0
    else:       # [w_hi: seg slots | w_hi8: seg bytes | w_lo8: seg bytes], e4m3 codes of t 2^sh with the largest magnitude of the tensor in [224, 448]
        word = p.f8_scales
        assert (word & 255) == 117 and ((word >> 16) & 255) == 127
        b = p.t.view(torch.uint8).reshape(N, taps, 4 * seg)
        for what, codes, t, byte in (("w_hi8", b[..., 2 * seg:3 * seg], hi.float(), (word >> 8) & 255), ("w_lo8", b[..., 3 * seg:], wp - hi.float(), (word >> 24) & 255)):
            sh = 127 - byte
            assert 224.0 <= float(t.abs().max()) * 2.0 ** sh <= 448.0, what
            assert torch.equal(codes, (t * 2.0 ** sh).to(torch.float8_e4m3fn).view(torch.uint8)), what
            assert int(codes[..., k:].max()) == 0 if seg > k else True


# ---- the walk table, exhaustively: every legal pair's kwargs written out, every other pair refused ------------------------------
Z = dict(a_dup_seg=0, a_wrap=0, f8_from=0, f8_mid=0, f8_scales=0)
WORD = "word"       # stands for the packed matrix's own scale word
LINEAR = {          # seg = 128, a_width = the form's own width
    (O.W_PLAIN, O.A_PLAIN): dict(Z, K=128, lda=128),
    (O.W_PLAIN, O.A_HILO): dict(Z, K=128, lda=256),
    (O.W_PLAIN, O.A_HILO8): dict(Z, K=128, lda=256),
    (O.W_SPLIT3, O.A_HILO): dict(Z, K=384, lda=256, a_dup_seg=128),
    (O.W_SPLIT2, O.A_PLAIN): dict(Z, K=256, lda=128, a_wrap=128),
    (O.W_SPLIT2, O.A_HILO): dict(Z, K=256, lda=256, a_wrap=128),
    (O.W_SPLIT2, O.A_HILO8): dict(Z, K=256, lda=256, a_wrap=128),
    (O.W_F8, O.A_HILO8): dict(Z, K=256, lda=256, f8_from=128, f8_mid=192, f8_scales=WORD),
}
CONV3 = {           # nine taps: K is per launch, lda per pixel; ada_igemm walks a tap's whole pixel (K == 9 lda for a plain operand) and cannot start over inside it
    (O.W_PLAIN, O.A_PLAIN): dict(Z, K=1152, lda=128),
    (O.W_SPLIT3, O.A_HILO): dict(Z, K=3456, lda=256, a_dup_seg=128),
    (O.W_F8, O.A_HILO8): dict(Z, K=2304, lda=256, f8_from=128, f8_mid=192, f8_scales=WORD),
}


@pytest.mark.parametrize("taps", [1, 9])
def test_walk_table_is_exactly_the_legal_pairs(taps):
    table = LINEAR if taps == 1 else CONV3
    for form, act in itertools.product(W_FORMS, A_FORMS):
        p = O.pack(torch.ones(N, taps * 128), form, torch.float16, taps)
        want = table.get((form, act))
        if want is None:
            with pytest.raises(E.HipExtError) as e:
                O.walk(p, act, act.width(128))
            assert form in str(e.value) and act.name in str(e.value), "the refusal names both forms"
            continue
        want = dict(want, f8_scales=p.f8_scales if want["f8_scales"] == WORD else 0)
        assert (p.f8_scales != 0) == (form == O.W_F8)
        assert O.walk(p, act, act.width(128)) == want, (form, act.name)
        if taps == 1:
            assert O.walk(p, act, 512) == dict(want, lda=512)     # a wider row stride (a non-split block in a split model's buffer) changes lda only
        else:
            with pytest.raises(E.HipExtError):
                O.walk(p, act, 512)                                # ... which a convolution, walking whole pixels, cannot have
        with pytest.raises(E.HipExtError):
            O.walk(p, act, act.width(128) - 64)                    # a row too narrow for the form
    assert (O.A_PLAIN.split_seg(128), O.A_HILO.split_seg(128), O.A_HILO8.split_seg(128)) == (0, 128, -128)
    assert (O.A_PLAIN.width(128), O.A_HILO.width(128), O.A_HILO8.width(128)) == (128, 256, 256)


# ---- producers and consumers of every head group agree, for every policy the product builds ------------------------------------
@functools.lru_cache(maxsize=None)
def _state_dict(kind):
    if kind == "raw":
        return _cases.schema_state_dict({"kind": "raw", "encoder": "vitb"})
    sd = _cases.schema_state_dict({"kind": "amodal", "encoder": "vitb", "guide_type": "mask+observation"})
    return {k[len("encoder."):]: v for k, v in sd.items()}


def _group_weights(w):
    """head group (or "tap") -> the packed matrices that read the group's buffer"""
    g = {"tap": list(w.proj_w), "rs0": [w.rs0_w], "rs1": [w.rs1_w], "rs3": [w.rs3_w], "oc1": [w.oc1_w], "oc2": [w.oc2_w]}
    for i in range(4):
        g[f"rn{i}"] = [w.rn_w[i]]
        g[f"rcu{i}"] = [w.fuse[i][f"u{u}c{c}_w"] for u in (1, 2) for c in (1, 2)]
        g[f"out{i}"] = [w.fuse[i]["out_w"]]
        if w.amodal_head:
            g[f"ip{i}"] = [w.ip_w[i]]
    return g


@pytest.mark.parametrize("tap_split", [False, True])
@pytest.mark.parametrize("f8", ["none", "head", "both"])
@pytest.mark.parametrize("split_head", [(), True, ("projw",), ("out1", "out2", "out3")])
@pytest.mark.parametrize("kind", ["amodal", "raw"])
def test_producers_and_consumers_agree(monkeypatch, kind, split_head, f8, tap_split):
    monkeypatch.setattr(E, "OC1_COMMUTE", False)     # (the commuted output_conv1 and the sub-pixel merge compose their weights on the device)
    monkeypatch.setattr(E, "SUBPIXEL", False)
    w = E.PackedWeights(_state_dict(kind), "vitb", guided=kind == "amodal", amodal_head=kind == "amodal", split_head=split_head, f8=f8, tap_split=tap_split, head_only=True)
    cols = E.Workspace.widths(w)
    groups = _group_weights(w)
    assert set(groups) - {"tap"} == set(E.HEAD_GROUPS) - {"proj", "projw"} - (set() if kind == "amodal" else {f"ip{i}" for i in range(4)})
    for group, packed in groups.items():
        act = w.act_form(group)
        for p in packed:
            kw = O.walk(p, act, cols[group])           # legal, or this raises
            assert kw["lda"] == cols[group] == act.width(p.seg), group
            reader = "proj" if group == "tap" else group
            if reader in w.split:                      # a split group gets the full product of the form its producers write
                assert (kw["a_dup_seg"] or kw["f8_from"]) == p.seg and bool(kw["f8_from"]) == (reader in w.f8_groups) == (act is O.A_HILO8), group
            elif group != "tap":
                assert act is O.A_PLAIN and p.form == O.W_PLAIN, group
    # the taps are split for the projects -- or kept so for the ladder's second rung, whatever reads them here
    assert (w.act_form("tap") is not O.A_PLAIN) == (tap_split or "proj" in w.split)
    assert all(p.form == (O.W_SPLIT2 if "projw" in w.split and "proj" not in w.split else w.proj_w[0].form) for p in w.proj_w)


def test_an_illegal_pair_is_refused_when_the_weights_are_packed(monkeypatch):
    monkeypatch.setattr(E, "OC1_COMMUTE", False)
    monkeypatch.setattr(E, "SUBPIXEL", False)
    with pytest.raises(E.HipExtError):     # three-term fp16 projects against taps kept [hi | lo8 | hi8] for a second rung (the bug DA2/dpt.py::_engine records)
        E.PackedWeights(_state_dict("raw"), "vitb", guided=False, amodal_head=False, split_head=("proj",), f8="none", tap_f8=True, head_only=True)
