"""Operand forms of the split-precision contractions (the kernels' side: include/ada_hip.h, ada_igemm_args): what a packed weight
matrix looks like (``pack``), what the producer of its A operand must write (``ActForm``), and how ada_igemm walks the pair (``walk``).  Host only: no launch."""
from __future__ import annotations

import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

from . import HipExtError

# weight forms, per tap of seg = r64(K) slots
W_PLAIN, W_SPLIT3, W_SPLIT2, W_F8 = "[w]", "[w_hi | w_hi | w_lo]", "[w_hi | w_lo]", "[w_hi | w_hi8 | w_lo8]"
F8_A_SCALES = 117 | (127 << 16)     # E8M0 bytes of the activation's two byte segments: lo8 = e5m2((x - x_hi) 2^10), hi8 = e5m2(x)


class ActForm(NamedTuple):
    """The form of an operand-typed activation row over segments of ``seg`` columns: what its producer is told, how wide its buffer is."""
    name: str
    sign: int
    segments: int

    def split_seg(self, seg: int) -> int:
        return self.sign * seg

    def width(self, seg: int) -> int:
        return self.segments * seg


A_PLAIN, A_HILO, A_HILO8 = ActForm("[x]", 0, 1), ActForm("[hi | lo]", 1, 2), ActForm("[hi | lo8 | hi8]", -1, 2)


def reads(form: str) -> ActForm:
    """The activation form whose full product a weight form evaluates ([w_hi | w_lo] reads a plain row twice)."""
    return {W_SPLIT3: A_HILO, W_F8: A_HILO8}.get(form, A_PLAIN)


class Packed(NamedTuple):
    """A packed weight matrix: the operand-typed [N, K_packed] tensor, its form, ``seg`` (padded K per tap), taps, the fp8 scale word (0 unless W_F8)."""
    t: torch.Tensor
    form: str
    seg: int
    taps: int = 1
    f8_scales: int = 0


def f8_weight_split(wm: torch.Tensor, op, taps: int = 1):
    """[N, taps * K] fp32 (K a multiple of 128) -> ([N, taps * 2 K] operand-typed storage, f8_scales word): per tap [w_hi | w_hi8 | w_lo8] with
    w_hi = round(w) in the operand type (K slots), then K bytes e4m3(w_hi 2^s_hi) and K bytes e4m3((w - w_hi) 2^s_lo), one power-of-two scale per
    tensor and segment chosen so that the largest magnitude lands in [224, 448].  The contraction against an activation stored [hi | lo8 | hi8]
    (split_seg = -K) evaluates x_hi w_hi + 2^-10 x_lo8 w_hi8 2^-s_hi + x_hi8 w_lo8 2^-s_lo (include/ada_hip.h, ada_igemm_args.f8_from)."""
    n = wm.shape[0]
    k = wm.shape[1] // taps
    assert wm.shape[1] == taps * k and k % 128 == 0, (wm.shape, taps)
    w = wm.reshape(n, taps, k).float()
    hi = w.to(op)
    lo = w - hi.float()

    def enc(t):
        m = float(t.abs().max())
        sh = max(-100, min(100, int(math.floor(math.log2(448.0 / m))))) if m > 0 else 0
        q = (t.float() * (2.0 ** sh)).clamp(-448.0, 448.0)
        try:
            b = q.to(torch.float8_e4m3fn).view(torch.uint8)
        except (RuntimeError, TypeError):      # no device cast for the dtype on this backend
            b = q.cpu().to(torch.float8_e4m3fn).view(torch.uint8).to(t.device)
        return b, 127 - sh
    hi8, sb_hi = enc(hi)
    lo8, sb_lo = enc(lo)
    packed = torch.cat([hi.contiguous().view(torch.uint8).reshape(n, taps, 2 * k), hi8, lo8], dim=2).reshape(n, taps * 4 * k)
    return packed.contiguous().view(op), F8_A_SCALES | (sb_hi << 8) | (sb_lo << 24)


def pack(w2d: torch.Tensor, form: str, op, taps: int = 1) -> Packed:
    """[N, taps * K] fp32, tap-major -> ``Packed``: K padded to a multiple of 64 with zeros, hi = round(w) in the operand type ``op``, lo = round(w - hi)."""
    n, k = w2d.shape[0], w2d.shape[1] // taps
    seg = (k + 63) // 64 * 64
    w = F.pad(w2d.reshape(n, taps, k), (0, seg - k))
    if form == W_F8:
        t, word = f8_weight_split(w.reshape(n, taps * seg), op, taps)
        return Packed(t, form, seg, taps, word)
    hi = w.to(op)
    if form != W_PLAIN:
        lo = (w - hi.float()).to(op)
        hi = torch.cat({W_SPLIT3: [hi, hi, lo], W_SPLIT2: [hi, lo]}[form], dim=2)
    return Packed(hi.reshape(n, -1).contiguous(), form, seg, taps)


# (weight form, activation form) -> (which of a_dup_seg / a_wrap / f8_from is set to seg, legal for 3x3 convolutions too).  Every other pair is refused.
_WALKS = {(W_PLAIN, A_PLAIN): (None, True),
          (W_PLAIN, A_HILO): (None, False), (W_PLAIN, A_HILO8): (None, False),       # a single-precision product of a split row: its hi half only
          (W_SPLIT3, A_HILO): ("a_dup_seg", True),
          (W_SPLIT2, A_PLAIN): ("a_wrap", False), (W_SPLIT2, A_HILO): ("a_wrap", False), (W_SPLIT2, A_HILO8): ("a_wrap", False),      # ... the hi half, walked twice
          (W_F8, A_HILO8): ("f8_from", True)}


def walk(p: Packed, act: ActForm, a_width: int) -> dict:
    """The ada_igemm arguments that contract rows of form ``act`` (row stride ``a_width``; per pixel for a 3x3 convolution) with the packed weights ``p``."""
    how, conv3 = _WALKS.get((p.form, act), ("", False))
    # (a convolution walks whole pixels: its row stride is the form's own width)
    if how == "" or a_width < act.width(p.seg) or (p.taps != 1 and not (conv3 and a_width == act.width(p.seg))):
        raise HipExtError(f"{p.form} weights (segments of {p.seg}, {p.taps} tap(s)) against a {act.name} operand of width {a_width}")
    kw = dict(K=p.t.shape[1], lda=a_width, a_dup_seg=0, a_wrap=0, f8_from=0, f8_mid=0, f8_scales=p.f8_scales)
    if how:
        kw[how] = p.seg
    if how == "f8_from":
        kw["f8_mid"] = p.seg + p.seg // 2
    return kw
