"""Forward engine: runs the whole Depth-Anything-V2 / Amodal-DAv2 forward pass as a fixed sequence of
libada_hip launches on the current HIP stream.

The nn.Module tree in ``src/models`` owns the fp32 parameters (reference ``state_dict`` schema); this
engine owns everything derived from them:

* ``PackedWeights`` -- operand-typed, MFMA-friendly copies made once per parameter version: linear /
  1x1 weights as [N, K]; 3x3 weights as [N, 9*Cp] (tap-major, channels padded to 64); transposed-conv
  weights as [s*s*Cout, Cin] with the bias expanded; the RGB and guidance patch-embed filters fused
  into one [D, 1024] matrix (reference DA2/dinov2.py:237-240 adds the two embeddings, so one GEMM over
  the concatenated K does both); the q rows of qkv pre-multiplied by head_dim**-0.5 * log2(e) (base-2 softmax in the attention kernel).
* ``Workspace`` -- every activation buffer for a (batch, H, W), allocated once and kept resident in HBM.

Data layout: the residual stream is fp32 [B*N, D]; every tensor that is only ever a contraction
operand is stored in the operand type (fp16 by default); DPT-head activations are NHWC, 3x3-conv
inputs carry a one-pixel zero border so the implicit-GEMM gather never branches.
"""
from __future__ import annotations

import math
import os
import threading
from collections import OrderedDict
from typing import Dict, Optional

import torch

from . import (A_CONV3, ACT_NONE, ACT_RELU, ACT_SIGMOID, EP_BIAS, EP_GAMMA, EP_GELU, EP_RELU_OP, EP_RESIDUAL,
               EP_SWIGLU, EP_TAIL, MAP_PAD, MAP_SHUFFLE, MAP_TOKEN, HipExtError)
from . import attention as k_attention
from . import bilinear as _bilinear
from . import count_saturated
from . import dpt_tail as k_dpt_tail
from . import igemm as _igemm
from . import layernorm as _layernorm
from . import debug_epoch, instrumented, operand_dtype
from . import depth_stats as k_depth_stats
from . import token_diversity as k_token_diversity
from . import ladder_select as k_ladder_select
from . import patchify as k_patchify
from . import pos_embed_resize as k_pos_embed_resize
from . import tapsum_resize as k_tapsum_resize
from . import write_cls as k_write_cls
from . import operands as O
from .ladder import ladder_curve, ladder_decide, ladder_thresholds, next_start_rung, rung_counts, stats_from_host  # noqa: F401  (ladder_curve: re-exported)
from .operands import f8_weight_split  # noqa: F401  (re-exported)

_probe = None   # list of (label, device counter) while DepthEngine.saturation_report runs, else None


def _probed(kernel, launch):
    """Wraps a launcher: while a saturation probe is active, the operand-typed output of every launch is swept by ada_debug_count_saturated."""
    def run(*a, **kw):
        launch(*a, **kw)
        t = kw.get("out_op")
        if _probe is not None and t is not None and t.is_contiguous():
            c = torch.zeros(1, dtype=torch.int64, device=t.device)
            count_saturated(t, c)
            _probe.append((f"{kernel} #{len(_probe)} {list(t.shape)}", c))
    return run


k_igemm, k_layernorm, k_bilinear = _probed("igemm", _igemm), _probed("layernorm", _layernorm), _probed("bilinear", _bilinear)

PATCH = 14
LN_EPS = 1e-6
# Contractions of the DPT head that can run in split precision (PackedWeights.split), by name: "proj" = read-out + the four 1x1 `projects`,
# "rs0" / "rs1" / "rs3" = resize_layers (ConvT 4x4, ConvT 2x2, conv3x3 stride 2), "ip<i>" = input_projection conv of level i,
# "rn<i>" = layer<i+1>_rn, "rcu<i>" = the ResidualConvUnit convs of refinenet<i+1>, "out<i>" = its 1x1 out_conv, "oc1" / "oc2" = the tail
# convs.  Level 0 is the finest grid (4x the patch grid), level 3 the coarsest.  HEAD_ALIASES name whole families.
# "projw" = the four 1x1 projects with WEIGHT-ONLY split precision ([w_hi | w_lo] against the plain LayerNorm output walked twice, ada_igemm a_wrap:
# the weight's rounding error goes, the activation's stays; 2x the MACs instead of 3x and no [hi | lo] copy of the tap).  Ignored when "proj" is set.
HEAD_GROUPS = ("proj", "projw", "rs0", "rs1", "rs3") + tuple(f"{f}{i}" for f in ("ip", "rn", "rcu", "out") for i in range(4)) + ("oc1", "oc2")
HEAD_ALIASES = {"tok": ("proj", "rs0", "rs1", "rs3"), "ip": tuple(f"ip{i}" for i in range(4)), "rn": tuple(f"rn{i}" for i in range(4)),
                "rcu": tuple(f"rcu{i}" for i in range(4)), "out": tuple(f"out{i}" for i in range(4))}
# ada_dpt_tail_fwd (resize + output_conv2 fused; the up-sampled map "fin" -- 2.2 GB at ViT-L bs=32 -- is neither allocated nor written) is the
# default tail wherever it applies (fused_tail_applies): 1.18 ms against 2.13 ms for the resize kernel + tail GEMM at ViT-L bs=32
# (profiles/r03_p_fused_tail.txt).  ADA_FUSED_TAIL=0 selects the two-launch tail everywhere (A/B, and the only path for split-precision "oc2").
FUSED_TAIL = os.environ.get("ADA_FUSED_TAIL", "1") == "1"
# Sub-pixel merge (round 4): resize_layers[0/1] (ConvTranspose 4x4 s4 / 2x2 s2, reference DA2/dpt.py:88-100,173) and the 3x3 convolution of
# input_projection[0/1] that follows with nothing in between (:153-159,178-179) run as ONE 3x3 convolution over the patch grid whose
# s*s*C output columns are the output phases (functional.subpixel_merge; ada_igemm_args.tap_cols): 36 C^2 instead of 160 C^2 MACs per patch
# at level 0, 16 C^2 instead of 40 C^2 at level 1 (39 GFLOP of 1390 per ViT-L image), one fp16 rounding of the intermediate map less, and
# the up-sampled maps L[0] / L[1] are never written.  Exact in real arithmetic, weights composed in fp64 when they are packed.
# ADA_SUBPIXEL=0 keeps the two launches (A/B; also the path of every split-precision level).
SUBPIXEL = os.environ.get("ADA_SUBPIXEL", "1") == "1"
# output_conv1 in front of its resize (round 4): path_1 = resize_x2(out_conv(RCU2(...))) (util/blocks.py:140-146, out_conv already commuted in front of
# the resize) feeds scratch.output_conv1, a 3x3 convolution (DA2/dpt.py:192-193).  A 1x1 channel mix commutes with a per-channel resample, so
#   conv3x3(resize(z)) = b + sum over the 9 taps t of  shift_t(resize(W_t z)),   z = out_conv(u):   W_t z = (W_t W_out) u + W_t b_out
# -- ONE GEMM over the 148^2 grid with N = 9 * features / 2 (0.41 TFLOP at ViT-L bs = 32 instead of out_conv 0.09 + output_conv1 1.65) whose nine
# operand-typed tap maps ada_tapsum_resize_fwd gathers (9 taps x 4 bilinear corners per output element; a tap whose position falls into the
# zero padding drops out whole, out_conv's bias included).  The up-sampled operand map p1 is never written.  ADA_OC1_COMMUTE=0: the old path.
SUBPIXEL_SPLIT = os.environ.get("ADA_SUBPIXEL_SPLIT", "1") != "0"           # A/B: 0 = two launches wherever a level's resize / first conv are split groups (round 5)
OC1_COMMUTE_SPLIT = os.environ.get("ADA_OC1_COMMUTE_SPLIT", "1") != "0"     # A/B: 0 = round 5's resize -> 3x3 conv path wherever "oc1" is a split group
STAT_CHUNKS = 8
OC1_COMMUTE = os.environ.get("ADA_OC1_COMMUTE", "1") != "0"     # operand-typed tap maps; 0: the resize -> conv path (A/B, profiles/r04_g_*; also the path of a split-precision oc1)


# fp8 correction terms (ada_igemm_args.f8_from): a split-precision product whose two small terms x_lo w_hi + x_hi w_lo run on the fp8 matrix pipe
# (v_mfma_scale_f32_16x16x128_f8f6f4, twice the fp16 rate) -- 2x the MACs' time instead of 3x.  oracle/study_fp8_correction.py: three mantissa bits
# are enough for terms that are 2^-11 of the product.  ADA_F8_CORR=0 keeps the three fp16 terms everywhere (A/B).
_F8_ENV = os.environ.get("ADA_F8_CORR", "1")     # 1 | 0 | enc | head (A/B: only the encoder's split blocks / only the head's split groups)
F8_CORR = _F8_ENV != "0"
F8_ENC, F8_HEAD = _F8_ENV in ("1", "enc"), _F8_ENV in ("1", "head")


def fused_tail_applies(half, halfp, hi, ho, split):
    """Whether ada_dpt_tail_fwd can take the tail (include/ada_hip.h): single-precision oc2, 64 or 128 (un-padded) channels, and a vertical
    scale whose 10-row halo tiles span at most 7 source row intervals -- always true for the model's 14 / 8 ratio."""
    if "oc2" in split or half != halfp or halfp // 64 > 2:
        return False
    sy = (hi - 1) / (ho - 1) if ho > 1 else 0.0
    return int(sy * 9) + 2 <= 7


VIT = {
    "vits": dict(dim=384, depth=12, heads=6, ffn="mlp"),
    "vitb": dict(dim=768, depth=12, heads=12, ffn="mlp"),
    "vitl": dict(dim=1024, depth=24, heads=16, ffn="mlp"),
    "vitg": dict(dim=1536, depth=40, heads=24, ffn="swiglu"),
}
TAPS = {"vits": [2, 5, 8, 11], "vitb": [2, 5, 8, 11], "vitl": [4, 11, 17, 23], "vitg": [9, 19, 29, 39]}
Q_PRESCALE = 0.125 * 1.4426950408889634  # head_dim**-0.5 * log2(e), head_dim = 64
MAX_ROWS = (1 << 24) - 1  # row-index limit of the kernels' fast division


def _r64(c: int) -> int:
    return (c + 63) // 64 * 64




class PackedWeights:
    """Operand-typed copies of the parameters, laid out for the kernels.  ``sd``: name -> fp32 CUDA tensor
    with the *raw* model's key names (``pretrained.*``, ``depth_head.*``)."""

    def __init__(self, sd: Dict[str, torch.Tensor], encoder: str, guided: bool, amodal_head: bool, split_head=False,
                 enc_split_blocks: int = 0, head_only: bool = False, tap_split: bool = False,
                 f8: str = "both", tap_f8: Optional[bool] = None, f8_only=None):
        op = operand_dtype()
        # head_only: the DPT head's weights only (the second rung of the precision ladder, DepthEngine._ladder, re-runs the head from the taps)
        # tap_split: the four taps are stored [hi | lo] whatever the head's own policy -- so that a split-precision head can be re-run from them
        self.head_only, self.tap_split = bool(head_only), bool(tap_split)
        cfg = VIT[encoder]
        D = cfg["dim"]
        self.encoder, self.guided, self.amodal_head = encoder, guided, amodal_head
        # split_head: contractions of the DPT head run in split precision (~fp32 operand accuracy at 3x the MACs, 2x with fp8 correction terms), PER LAYER
        # GROUP (HEAD_GROUPS; True = every group).  The forms of the weights and activations, and who decides them: DESIGN.md section 4.1.  Used where the
        # head's operand rounding is what limits parity: the unbounded-output models (raw ReLU / 'ssi' heads) and ViT-S.
        if split_head is True:
            split_head = HEAD_GROUPS
        self.split = frozenset(g for name in (split_head or ()) for g in HEAD_ALIASES.get(name, (name,)))
        unknown = self.split - set(HEAD_GROUPS)
        if unknown:
            raise HipExtError(f"unknown head layer group(s) {sorted(unknown)}; known: {HEAD_GROUPS}")
        self.split_head = bool(self.split)
        # enc_split_blocks = K: the linear layers of the FIRST K transformer blocks run in split precision.  Operand rounding noise injected
        # early is amplified by every later block (oracle study, profiles/r04_e_raw_vitg_operand_noise_by_block.txt: blocks 0-9 of ViT-G carry
        # half of the encoder's share, blocks 30-39 a fiftieth), so for the unbounded-output ViT-G model, whose encoder alone reaches
        # 0.7e-3 ... 1.05e-3 depending on the weight draw, the head's split precision is not enough.  All four linear layers of a split block take the
        # full product: the attention kernel and the GELU / SwiGLU epilogues write their outputs in the split form too (rounds 4-5 walked the plain
        # activation twice against [w_hi | w_lo]: the weight's rounding error went, the activation's stayed -- and that was what bounded the everything-split
        # engine: raw ViT-G 6.2e-4 of output error from these two activations alone against 2.9e-4 from the attention core, oracle/study_rung3_floor.py).
        self.enc_split_blocks = max(0, min(int(enc_split_blocks), cfg["depth"]))
        # ... with the two correction terms on the fp8 matrix pipe where the build has it (fp16 operands, D a multiple of 128)
        # f8: which of the two users take it -- "both" | "enc" | "head" | "none" (the caller's precision policy, DA2/dpt.py::_f8_policy)
        if f8 not in ("both", "enc", "head", "none"):
            raise HipExtError(f"PackedWeights: f8={f8!r} (both | enc | head | none)")
        self.f8_head = F8_HEAD and f8 in ("both", "head") and op == torch.float16
        self.f8_only = None if f8_only is None else frozenset(f8_only)      # head groups that may take it (None: every split group)
        self.enc_f8 = F8_ENC and f8 in ("both", "enc") and self.enc_split_blocks > 0 and op == torch.float16 and D % 128 == 0
        # the form of the taps when they are kept split: that of their reader -- this object's own "proj" group, or (tap_f8 given) the weights of
        # the ladder's second rung, which are packed later from the same state_dict
        self.tap_f8 = (self.f8_head if tap_f8 is None else (bool(tap_f8) and F8_HEAD and op == torch.float16)) and D % 128 == 0
        self.dim, self.depth, self.heads, self.ffn = D, cfg["depth"], cfg["heads"], cfg["ffn"]
        self.op = op
        # reader -> the activation form it reads (act_form).  The taps are split when the projects read them so -- or the engine keeps them for the second rung
        self.reads = {"tap": (O.A_HILO8 if self.tap_f8 else O.A_HILO) if (self.tap_split or "proj" in self.split) else O.A_PLAIN}

        def f32(name):
            return sd[name].detach().to(torch.float32).contiguous()

        self.blocks = []
        self.guide_channels = 0
        if not head_only:
            self._pack_encoder(sd, f32, D, guided)
        self._pack_head(sd, f32, D, amodal_head)
        # head groups whose producers write [hi | lo8 | hi8]
        self.f8_groups = {g for g in HEAD_GROUPS if self.reads.get(g) is O.A_HILO8}
        for p in self.proj_w + (self.ro_wx + self.ro_wc if self.readout else []):     # the one pair whose two sides are chosen apart (tap_f8): refused here, not at launch
            O.walk(p, self.reads["tap"], self.reads["tap"].width(D))

    def _form(self, group, seg, weight_only=False):
        """THE choice of a head contraction's weight form.  A split group takes the full product, its two correction terms on the fp8
        pipe where the policy (f8, f8_only) allows it and the padded channel count is a multiple of 128; ``weight_only``: [w_hi | w_lo] outside a split group."""
        if group not in self.split:
            return O.W_SPLIT2 if weight_only else O.W_PLAIN
        f8 = self.f8_head and (self.f8_only is None or group in self.f8_only) and seg % 128 == 0
        return O.W_F8 if f8 else O.W_SPLIT3

    def _pack(self, w, group, taps=1, weight_only=False) -> O.Packed:
        """[N, taps, K] (any trailing shape) fp32 weights of a contraction of ``group``, in the group's form; what its producers must write is recorded."""
        w = w.reshape(w.shape[0], -1)
        p = O.pack(w, self._form(group, _r64(w.shape[1] // taps), weight_only), self.op, taps)
        if self.reads.setdefault(group, O.reads(p.form)) is not O.reads(p.form):
            raise HipExtError(f"head group {group!r}: {p.form} weights against the {self.reads[group].name} operand of the group's other contractions")
        return p

    def act_form(self, reader) -> O.ActForm:
        """The form the producers of a contraction's A operand must write and its buffer holds.  ``reader``: a head group, "tap" (the four taps and the class
        tokens), "sp<i>" (the merged sub-pixel convolution of level i), or the index of an encoder block (its LayerNorm / attention / MLP-hidden rows)."""
        if isinstance(reader, int):
            return O.reads(self.blocks[reader]["qkv_w"].form)
        return self.reads.get(reader, O.A_PLAIN)

    def _pack_encoder(self, sd, f32, D, guided):
        p, op = "pretrained.", self.op
        w_rgb = f32(p + "patch_embed.proj.weight").reshape(D, -1)
        b_pe = f32(p + "patch_embed.proj.bias")
        if guided:
            w_g = f32(p + "patch_embed_guidance.proj.weight")
            self.guide_channels = w_g.shape[1]
            w_rgb = torch.cat([w_rgb, w_g.reshape(D, -1)], dim=1)
            b_pe = b_pe + f32(p + "patch_embed_guidance.proj.bias")
        # split-precision patch embedding: the image is the one operand whose fp16 rounding error (2.5e-4 relative) is
        # injected into every token, so it is carried as hi + lo halves and the weights likewise (0.6 % of the model's MACs instead of 0.2 %)
        self.pe_w = O.pack(w_rgb, O.W_SPLIT3, op)
        self.pe_b = b_pe.contiguous()
        self.pe_seg = self.pe_w.seg
        self.cls = f32(p + "cls_token").reshape(D)
        self.pos_native = f32(p + "pos_embed")  # [1, 1 + 37*37, D]
        self._pos_cache: Dict[tuple, torch.Tensor] = {}

        for i in range(self.depth):
            b = f"{p}blocks.{i}."
            qw, qb = f32(b + "attn.qkv.weight").clone(), f32(b + "attn.qkv.bias").clone()
            # q * head_dim**-0.5 (reference attention.py:41,53) folded into the weights, together with log2(e): the attention
            # kernel runs its softmax in base 2 (exp2 is the native transcendental), softmax_e(s) == softmax_2(s * log2 e)
            qw[:D] *= Q_PRESCALE
            qb[:D] *= Q_PRESCALE
            form = O.W_PLAIN if i >= self.enc_split_blocks else O.W_F8 if self.enc_f8 else O.W_SPLIT3

            def lin(name):
                return O.pack(name if torch.is_tensor(name) else f32(b + name), form, op)

            blk = dict(
                ln1_w=f32(b + "norm1.weight"), ln1_b=f32(b + "norm1.bias"), qkv_w=lin(qw), qkv_b=qb,
                proj_w=lin("attn.proj.weight"), proj_b=f32(b + "attn.proj.bias"), ls1=f32(b + "ls1.gamma"),
                ln2_w=f32(b + "norm2.weight"), ln2_b=f32(b + "norm2.bias"), ls2=f32(b + "ls2.gamma"),
            )
            if self.ffn == "mlp":
                blk.update(fc1_w=lin("mlp.fc1.weight"), fc1_b=f32(b + "mlp.fc1.bias"), fc2_w=lin("mlp.fc2.weight"), fc2_b=f32(b + "mlp.fc2.bias"))
                blk["hidden"] = blk["fc1_w"].t.shape[0]
            else:
                w12, b12 = f32(b + "mlp.w12.weight"), f32(b + "mlp.w12.bias")
                hid = w12.shape[0] // 2
                assert hid % 32 == 0
                # interleave x1 / x2 rows in groups of 32 so one wave's two MFMA column tiles hold the gate pair
                idx = torch.arange(hid, device=w12.device).reshape(-1, 32)
                order = torch.stack([idx, idx + hid], dim=1).reshape(-1)
                blk.update(w12_w=lin(w12[order]), w12_b=b12[order].contiguous(), w3_w=lin("mlp.w3.weight"), w3_b=f32(b + "mlp.w3.bias"))
                blk["hidden"] = hid
            self.blocks.append(blk)
        self.norm_w, self.norm_b = f32(p + "norm.weight"), f32(p + "norm.bias")

    def _pack_head(self, sd, f32, D, amodal_head):
        def conv3(w, group):  # [Co, Ci, 3, 3] -> tap-major
            return self._pack(w.permute(0, 2, 3, 1), group, taps=9)

        def convT(w, b, s_, group):  # [Ci, Co, s, s] -> [s*s*Co, Ci], bias expanded to [s*s*Co]
            return self._pack(w.permute(2, 3, 1, 0).reshape(s_ * s_ * w.shape[1], w.shape[0]), group), b.repeat(s_ * s_).contiguous()

        h = "depth_head."
        # use_clstoken read-out (reference DA2/dpt.py:110-117,164-167): Linear(2D -> D) on [patch token | class token] + GELU.  The class
        # token half is the same for every patch of an image, so it becomes a per-image bias  c_b = W_cls cls_b + b  (one tiny GEMM) and
        # the patch half runs as a D -> D GEMM per image with that bias.
        self.readout = f"{h}readout_projects.0.0.weight" in sd
        if self.readout:
            self.ro_wx, self.ro_wc, self.ro_b = [], [], []
            for i in range(4):
                wr = f32(f"{h}readout_projects.{i}.0.weight")
                self.ro_wx.append(self._pack(wr[:, :D], "proj"))
                self.ro_wc.append(self._pack(wr[:, D:], "proj"))
                self.ro_b.append(f32(f"{h}readout_projects.{i}.0.bias"))
        self.oc = [sd[f"{h}projects.{i}.weight"].shape[0] for i in range(4)]
        self.features = sd[h + "scratch.layer1_rn.weight"].shape[0]
        # "projw": weight-only split of the four projects (HEAD_GROUPS comment); "proj" (full split) takes precedence
        self.proj_w = [self._pack(f32(f"{h}projects.{i}.weight"), "proj", weight_only="projw" in self.split) for i in range(4)]
        self.proj_b = [f32(f"{h}projects.{i}.bias") for i in range(4)]
        self.rs0_w, self.rs0_b = convT(f32(h + "resize_layers.0.weight"), f32(h + "resize_layers.0.bias"), 4, "rs0")
        self.rs1_w, self.rs1_b = convT(f32(h + "resize_layers.1.weight"), f32(h + "resize_layers.1.bias"), 2, "rs1")
        self.rs3_w, self.rs3_b = conv3(f32(h + "resize_layers.3.weight"), "rs3"), f32(h + "resize_layers.3.bias")
        # level -> merged sub-pixel convolution: resize_layers[i] + input_projection[i][0] in the amodal head,
        # resize_layers[i] + scratch.layer{i+1}_rn (no bias, util/blocks.py:20-24) in the raw head
        self.sp = {}
        if SUBPIXEL:
            from .functional import subpixel_merge
            nxt = "ip" if amodal_head else "rn"
            for i, s_ in ((0, 4), (1, 2)):
                # single-precision levels -- and (round 6) a level whose transposed conv AND the 3x3 conv behind it are split groups with fp8 correction terms: the
                # merged weights take the 3x3 conv's form and `projects[i]` writes the patch-grid tensor [hi | lo8 | hi8]
                groups = {f"rs{i}", f"{nxt}{i}"}
                if groups & self.split and not (SUBPIXEL_SPLIT and groups <= self.split
                                                and all(self._form(g, _r64(self.oc[i])) == O.W_F8 for g in groups)):
                    continue
                if amodal_head:
                    w3_, b3_ = f32(f"{h}input_projection.{i}.0.weight"), f32(f"{h}input_projection.{i}.0.bias")
                else:
                    w3_, b3_ = f32(f"{h}scratch.layer{i + 1}_rn.weight"), None
                wm, bias, tapb, masks = subpixel_merge(f32(f"{h}resize_layers.{i}.weight"), f32(f"{h}resize_layers.{i}.bias"), w3_, b3_, s_)
                self.sp[i] = dict(s=s_, w=self._pack(wm, f"{nxt}{i}", taps=9), b=bias, tapb=tapb, masks=masks,
                                  taps_per_col=sum(bin(m).count("1") for m in masks) / float(s_ * s_))
                self.reads[f"sp{i}"] = O.reads(self.sp[i]["w"].form)
        if amodal_head:
            self.ip_w = [conv3(f32(f"{h}input_projection.{i}.0.weight"), f"ip{i}") for i in range(4)]
            self.ip_b = [f32(f"{h}input_projection.{i}.0.bias") for i in range(4)]
            self.ip_ln_w = [f32(f"{h}input_projection.{i}.1.weight") for i in range(4)]
            self.ip_ln_b = [f32(f"{h}input_projection.{i}.1.bias") for i in range(4)]
        s = h + "scratch."
        self.rn_w = [conv3(f32(f"{s}layer{i + 1}_rn.weight"), f"rn{i}") for i in range(4)]
        self.fuse = []
        for k in range(1, 5):
            r = f"{s}refinenet{k}."
            d = dict(out_w=self._pack(f32(r + "out_conv.weight"), f"out{k - 1}"), out_b=f32(r + "out_conv.bias"))
            for u in (1, 2):
                for c in (1, 2):
                    w, b = f32(f"{r}resConfUnit{u}.conv{c}.weight"), f32(f"{r}resConfUnit{u}.conv{c}.bias")
                    bn = f"{r}resConfUnit{u}.bn{c}."
                    if bn + "running_var" in sd:      # use_bn=True: inference BatchNorm folded into the conv (reference blocks.py:70-76)
                        from .functional import fold_batchnorm
                        w, b = fold_batchnorm(w, b, f32(bn + "weight"), f32(bn + "bias"), f32(bn + "running_mean"), f32(bn + "running_var"))
                    d[f"u{u}c{c}_w"] = conv3(w, f"rcu{k - 1}")
                    d[f"u{u}c{c}_b"] = b.contiguous()
            self.fuse.append(d)  # index k-1
        self.oc1_w, self.oc1_b = conv3(f32(s + "output_conv1.weight"), "oc1"), f32(s + "output_conv1.bias")
        self.oc1c = None     # output_conv1 composed with refinenet1.out_conv, one 1x1 per tap: [9 * half, Fp] (+ the bias each tap map carries)
        half_, Fp = self.features // 2, _r64(self.features)
        # (round 6) ... ALSO when "oc1" / "out0" are split groups with fp8 correction terms: the tap-map GEMM then reads u[0] as [hi | lo8 | hi8] against the composed
        # matrix in the fp8 form; the nine tap maps stay operand-typed.  The ladder's second rung (-2 ms of its 27) and the raw ViT-B / ViT-L heads.
        groups = {"oc1", "out0"}
        split_commute = OC1_COMMUTE_SPLIT and groups <= self.split and all(self._form(g, Fp) == O.W_F8 for g in groups) and self.features % 128 == 0
        if OC1_COMMUTE and (split_commute or not groups & self.split) and half_ in (32, 64, 128):
            from .functional import compose_f32
            w1 = f32(s + "output_conv1.weight")                                  # [half, F, 3, 3]
            wo_ = f32(s + "refinenet1.out_conv.weight").reshape(self.features, self.features)   # [F(cm), F(ci)]
            bo_ = f32(s + "refinenet1.out_conv.bias")
            wt_ = w1.permute(2, 3, 0, 1).reshape(9 * half_, self.features)       # rows (tap, co), columns cm
            # weight-only split where the groups are single-precision: rounding the COMPOSED matrix to the operand type once is not harmless -- its error acts on the
            # activation's large common-mode part coherently over all taps and positions and survives the resizes and convolutions behind it
            # (oracle study: 5.3e-4 at the output of ViT-B from this rounding alone, against 1.0e-4 / 0.9e-4 for the two factors rounded
            # separately; profiles/r04_g_output_conv1_commute.txt).  K = 2 * 256 on a GEMM that is bound by its 1.6 GB of output anyway.
            wc_ = compose_f32(wt_, wo_.t())       # the library's own GEMM in split precision (functional.compose_f32); W_t b_out is a reduction
            tap_b = (wt_.double() * bo_.double()[None, :]).sum(1).float().contiguous()
            self.oc1c = dict(w=self._pack(wc_, "out0", weight_only=True), b=tap_b)
        self.oc2_w, self.oc2_b = conv3(f32(s + "output_conv2.0.weight"), "oc2"), f32(s + "output_conv2.0.bias")
        self.tail_w = f32(s + "output_conv2.2.weight").reshape(-1).contiguous()
        self.tail_b = float(f32(s + "output_conv2.2.bias").reshape(-1)[0].item())

    def pos_embed(self, ph: int, pw: int) -> torch.Tensor:
        """[1 + ph*pw, D] fp32 position table for a ph x pw patch grid (reference DA2/dinov2.py:199-230).
        The native 37x37 square grid is used as is; anything else is a one-off bicubic resample of the
        parameter by ada_pos_embed_resize (cached per grid) -- a parameter transform like weight packing, not part of the per-image path."""
        key = (ph, pw)
        if key in self._pos_cache:
            return self._pos_cache[key]
        pos = self.pos_native
        n = pos.shape[1] - 1
        if not (ph * pw == n and ph == pw):
            sq = int(math.sqrt(n))
            # reference quirk kept on purpose: w0 is derived from x.shape[2] (image *height*) -- dinov2.py:233,209
            w0, h0 = ph + 0.1, pw + 0.1
            src = pos[0].contiguous()
            res = torch.empty(1 + ph * pw, src.shape[1], dtype=torch.float32, device=src.device)
            k_pos_embed_resize(src, sq, src.shape[1], ph, pw, float(w0) / sq, float(h0) / sq, res)
            pos = res[None]
        out = pos[0].contiguous()
        self._pos_cache[key] = out
        return out


class Workspace:
    @staticmethod
    def widths(pw_: PackedWeights) -> Dict[str, int]:
        """reader (PackedWeights.act_form) -> columns of the operand-typed buffer its contractions read: the form its producers write over the reader's segment."""
        ocp, Fp = [_r64(c) for c in pw_.oc], _r64(pw_.features)
        seg = {"tap": pw_.dim, "oc1": Fp, "oc2": _r64(pw_.features // 2)}
        for i in range(4):
            seg.update({f"rs{i}": ocp[i], f"ip{i}": ocp[i], f"rn{i}": ocp[i], f"sp{i}": ocp[i], f"rcu{i}": Fp, f"out{i}": Fp})
        return {g: pw_.act_form(g).width(s) for g, s in seg.items()}

    def __init__(self, pw_: PackedWeights, B: int, H: int, W: int, device, head_only: bool = False):
        """head_only: the buffers of the DPT head and the four taps only (the precision ladder's second rung re-runs the head from the taps)."""
        op = operand_dtype()
        self.B, self.H, self.W = B, H, W
        ph, pw = H // PATCH, W // PATCH
        self.ph, self.pw = ph, pw
        Np = ph * pw
        N = Np + 1
        D = pw_.dim
        T, P = B * N, B * Np
        Fch = pw_.features
        Fp = _r64(Fch)
        cols = self.widths(pw_)     # an op-typed head tensor is as wide as the form the contraction that READS it needs
        first = "ip" if pw_.amodal_head else "rn"     # the contraction family that reads the reassembled maps L[i]

        def z(*shape, dtype=op):
            return torch.zeros(*shape, dtype=dtype, device=device)

        if not head_only:
            self.a_pe = z(P, O.A_HILO.width(pw_.pe_seg))     # split-precision patches
            self.x = z(T, D, dtype=torch.float32)
            # LayerNorm output, attention output, MLP hidden: one buffer each for every block, in the form of block 0 (split if any block is: enc_split_blocks)
            enc = pw_.act_form(0)
            self.y = z(T, enc.width(D))
            self.qkv = z(T, 3 * D)
            self.o = z(T, enc.width(D))
            self.hd = z(T, enc.width(pw_.blocks[0]["hidden"]))
        self.taps = [z(P, cols["tap"]) for _ in range(4)]
        # the precision ladder's per-image statistics, one buffer (one host read): stat_sums = (sum s, sum s (1 - s)) of the depth map in chunks
        # (ada_depth_stats_fwd), stat_div = (sum of column variances, sum of column mean squares) of the last tap in 64-column chunks (ada_token_diversity_fwd)
        # ... and stat_in = the same pair over the PATCHIFIED INPUT (a_pe: one row per patch, pixels + guide channels): exactly zero variance when every patch of the
        # image is the same (constant images, pixel checkerboards) -- the input-side trigger of the flat-input rung
        G = (D + 63) // 64
        Gi = 0 if head_only else pw_.pe_seg // 64
        self.stat_buf = z(B * (STAT_CHUNKS + G + Gi) * 2, dtype=torch.float32)
        self.stat_sums = self.stat_buf[:B * STAT_CHUNKS * 2].view(B, STAT_CHUNKS, 2)
        self.stat_div = self.stat_buf[B * STAT_CHUNKS * 2:B * (STAT_CHUNKS + G) * 2].view(B, G, 2)
        self.stat_in = self.stat_buf[B * (STAT_CHUNKS + G) * 2:].view(B, Gi, 2) if Gi else None
        if pw_.readout:
            self.cls_op = [z(B, cols["tap"]) for _ in range(4)]                          # final-LayerNorm'd class tokens, operand-typed
            self.cls_bias = [z(B, D, dtype=torch.float32) for _ in range(4)]       # W_cls cls + b per image
            self.taps_ro = [z(P, cols["tap"]) for _ in range(4)]                         # read-out tokens (inputs of `projects`)
        # head grids
        self.grid = [(4 * ph, 4 * pw), (2 * ph, 2 * pw), (ph, pw), ((ph - 1) // 2 + 1, (pw - 1) // 2 + 1)]
        oc = pw_.oc
        ocp = [_r64(c) for c in oc]
        self.ocp, self.Fp = ocp, Fp
        # levels whose resize + first 3x3 conv run as one sub-pixel convolution: `projects[i]` writes a zero-bordered patch-grid tensor tp[i]
        # (the conv's A operand); t<i> and the up-sampled map L[i] do not exist
        self.tp = {i: z(B, ph + 2, pw + 2, cols[f"sp{i}"]) for i in pw_.sp}
        self.t0 = None if 0 in pw_.sp else z(P, cols["rs0"])
        self.t1 = None if 1 in pw_.sp else z(P, cols["rs1"])
        self.pre3 = z(B, ph + 2, pw + 2, cols["rs3"])
        self.L = [None if i in pw_.sp else z(B, g[0] + 2, g[1] + 2, cols[f"{first}{i}"]) for i, g in enumerate(self.grid)]
        if pw_.amodal_head:
            self.ipf = [z(B * g[0] * g[1], oc[i], dtype=torch.float32) for i, g in enumerate(self.grid)]
            self.L2 = [z(B, g[0] + 2, g[1] + 2, cols[f"rn{i}"]) for i, g in enumerate(self.grid)]
        self.rnx = [z(B * g[0] * g[1], Fch, dtype=torch.float32) for g in self.grid]
        # raw head: [patch, s*s*features] fp32 output of a merged resize + layer_rn convolution, re-laid out into rnx / rnr by one pass
        self.spf = {} if pw_.amodal_head else {i: z(B * self.grid[i][0] * self.grid[i][1], Fch, dtype=torch.float32) for i in pw_.sp}
        self.rnr = [z(B, g[0] + 2, g[1] + 2, cols[f"rcu{i}"]) for i, g in enumerate(self.grid)]
        self.tmpa = [z(B, g[0] + 2, g[1] + 2, cols[f"rcu{i}"]) for i, g in enumerate(self.grid)]
        # fp32 side buffers whose lifetimes do not overlap share storage (plain row buffers only: the zero-bordered operand tensors keep their own,
        # their borders are written once).  Launch order of _head: ip conv -> LN (ipf dead) ... rn convs ... per level i = 3..0:
        # RCU2(i) [reads s[i]] -> out_conv [writes zf[i]] -> RCU1(i-1) [reads rnx[i-1], writes r[i-1]] -> resize [reads zf[i], r[i-1], writes s[i-1]];
        # then resize zf[0] -> p1, output_conv1 [writes oc1].  So: zf[i] lives in rnx[i] (dead since RCU1(i) / RCU2(3)), r[i] in ipf[i] where that is
        # large enough, and oc1 (4 x the pixels, half the channels = 2 x one level-0 buffer) in the level-0 pair (r[0], s[0]).
        rows = [B * g[0] * g[1] for g in self.grid]
        lvl0 = z(2 * rows[0] * Fch, dtype=torch.float32)
        self.r = [lvl0[:rows[0] * Fch].view(rows[0], Fch)]
        self.s = [lvl0[rows[0] * Fch:].view(rows[0], Fch)]
        for i in range(1, 4):
            if pw_.amodal_head and oc[i] >= Fch:
                self.r.append(self.ipf[i].view(-1)[:rows[i] * Fch].view(rows[i], Fch))
            else:
                self.r.append(z(rows[i], Fch, dtype=torch.float32))
            self.s.append(z(rows[i], Fch, dtype=torch.float32))
        self.sr = [z(B, g[0] + 2, g[1] + 2, cols[f"rcu{i}"]) for i, g in enumerate(self.grid)]
        self.u = [z(B * g[0] * g[1], cols[f"out{i}"]) for i, g in enumerate(self.grid)]
        self.zf = self.rnx
        g0 = self.grid[0]
        self.g296 = (2 * g0[0], 2 * g0[1])
        self.p1 = None if pw_.oc1c is not None else z(B, self.g296[0] + 2, self.g296[1] + 2, cols["oc1"])
        # the nine tap maps of output_conv1 on the level-0 grid
        self.tmaps = z(rows[0], 9 * (Fch // 2)) if pw_.oc1c is not None else None
        half = Fch // 2
        self.half, self.halfp = half, _r64(half)
        self.oc1 = lvl0.view(B * self.g296[0] * self.g296[1], half)
        # fused tail (ada_dpt_tail_fwd): resize + output_conv2 in one kernel, the up-sampled map is never materialised.  Needs the
        # single-precision head and a channel count that is already a multiple of 64 (ViT-B / ViT-L heads)
        self.fused_tail = FUSED_TAIL and fused_tail_applies(half, self.halfp, self.g296[0], H, pw_.split)
        self.fin = None if self.fused_tail else z(B, H + 2, W + 2, cols["oc2"])


# Head branches on side streams (round 6): the four reassemble -> input_projection -> layerN_rn chains (DA2/dpt.py:161-187) and the
# ResidualConvUnit 1 of levels 0-2 (util/blocks.py:131-133) are independent of each other until the refinenets join them; at small batches their launches
# fill 0.04-0.7 of a round of the 256 CUs (profiles/r05_e_config2_shapes.txt), so below HEAD_STREAMS_ROWS patch rows they are issued on four HIP streams
# (fork / join with events: capturable into the forward's graph) and the coarse levels run in the CUs the fine level leaves idle.  Same kernels, same
# arguments, same bits.  ADA_HEAD_STREAMS=0 / 1: never / always.
# hip_ext.ladder.ladder_decide: relative guard band around the ladder's thresholds inside which a higher rung's r does not decide and the first rung's own r does (the rungs' maps differ by ~1e-3 of their logits)
LADDER_GUARD = float(os.environ.get("ADA_LADDER_GUARD", "0.02"))
# ADA_LADDER_STICKY=0: always run the first rung's head first (A/B)
LADDER_STICKY = os.environ.get("ADA_LADDER_STICKY", "1") != "0"
HEAD_STREAMS = os.environ.get("ADA_HEAD_STREAMS", "auto")
HEAD_STREAMS_ROWS = int(os.environ.get("ADA_HEAD_STREAMS_ROWS", str(12 * 1369)))
GRAPH_MODE = os.environ.get("ADA_GRAPH", "auto")
# "auto": graph replay for calls of up to one 518x518 image.  Measured (profiles/r02_k_hip_graph_latency_ab.txt): the forward is device-bound
# from ViT-B upwards (replay == launches within 0.5 % at B = 1..8) and host-bound only for a single ViT-S image (3.55 -> 2.62 ms).
GRAPH_AUTO_PIXELS = int(os.environ.get("ADA_GRAPH_AUTO_PIXELS", str(518 * 518)))
GRAPH_AUTO_ENCODERS = tuple(e for e in os.environ.get("ADA_GRAPH_AUTO_ENCODERS", "vits").split(",") if e)
# Bounds of the per-shape caches (LRU): a variable-resolution stream of single images must not grow device memory without limit.  A shape is
# captured only on its SECOND sighting (a one-off resolution pays no extra warm-up forward, synchronise and empty_cache).
MAX_GRAPHS = int(os.environ.get("ADA_GRAPH_CACHE", "4"))
MAX_WORKSPACES = int(os.environ.get("ADA_WORKSPACE_CACHE", "6"))


class _GraphedForward:
    """The launch sequence of DepthEngine._forward for one input shape, captured into a HIP graph.  The forward is a fixed list of
    kernel launches over a pre-allocated workspace (no host synchronisation, no data-dependent control flow), so the capture is exact;
    inputs are copied into the graph's static buffers and the result is cloned out of its pool."""

    def __init__(self, eng: "DepthEngine", x: torch.Tensor, guide: Optional[torch.Tensor], norm: Optional[bool] = None):
        dev = x.device
        self.x = x.detach().contiguous().float().clone()
        self.guide = None if guide is None else guide.detach().contiguous().float().clone()
        # The captured launches carry raw pointers into this shape's Workspace (allocated by the warm-up forward below, in the ordinary
        # allocator pool, not the graph's): the graph must keep it alive itself.  Replays never pass through DepthEngine.workspace(), so
        # the engine's LRU sees a captured shape as idle and may drop its entry -- with this reference that only removes the dict entry.
        self.ws = eng.workspace(x.shape[0], x.shape[2], x.shape[3], dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):   # warm-up outside the capture: workspace, position table, per-kernel function attributes
            eng._forward(self.x, self.guide, norm)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        # thread-local capture mode: other host threads may keep using the device (a serving process) while this one captures
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.out = eng._forward(self.x, self.guide, norm)
        if eng.workspace(x.shape[0], x.shape[2], x.shape[3], dev) is not self.ws:   # cannot happen under the engine lock; never replay a graph over foreign memory
            raise RuntimeError("workspace changed during graph capture")
        self.lock = threading.Lock()

    def __call__(self, x: torch.Tensor, guide: Optional[torch.Tensor], post=None) -> torch.Tensor:
        # the static input / output buffers are shared by every caller of this shape: copy-in, replay and copy-out are one critical section
        # (`post(ws, out, x, guide)`: the engine's precision ladder, which reads the taps this replay left in the graph's workspace)
        with self.lock:
            self.x.copy_(x)
            if self.guide is not None:
                if guide is None or guide.shape != self.guide.shape:
                    raise HipExtError(f"guide tensor of shape {tuple(self.guide.shape)} required")
                self.guide.copy_(guide)
            self.graph.replay()
            out = self.out.clone()
            return out if post is None else post(self.ws, out, x, guide)


class DepthEngine:
    """Runs one forward.  ``final_act``: 'sigmoid' | 'relu' | 'none'."""

    def __init__(self, weights: PackedWeights, final_act: str, normalise_input: bool, ladder: Optional[dict] = None):
        self.w = weights
        self.final_act = {"sigmoid": ACT_SIGMOID, "relu": ACT_RELU, "none": ACT_NONE}[final_act]
        self.normalise_input = normalise_input
        # Precision ladder of the sigmoid heads (see _ladder): dict(r=<threshold on sum s(1-s) / sum s>, make=<callable -> head-only PackedWeights
        # in split precision>) or None.  The first rung -- this engine's own weights -- must keep its taps [hi | lo] (PackedWeights.tap_split).
        # Heads without a sigmoid keep the third rung's token-diversity trigger only: dict(div=..., make3=...) (DA2/dpt.py::_flat_input_rung).
        self.ladder = ladder
        self._warned = False          # the one-time notice that images are being re-run
        self.second_rung_first_calls = 0     # calls that ran the second rung's head first (diagnostic)
        self.third_rung_first_calls = 0      # ... the third-rung engine first
        self._start_rung = 1          # which rung runs first (_ladder; hip_ext.ladder.next_start_rung): 2 after a call most of whose images left the first rung
        if self.ladder is not None and "make" in self.ladder and not weights.tap_split and "proj" not in weights.split:
            raise HipExtError("precision ladder: the engine's weights must be packed with tap_split=True")
        self._w_hi: Optional[PackedWeights] = None
        self._ws_hi: "OrderedDict[tuple, Workspace]" = OrderedDict()
        self.block_probe = None       # diagnostic hook: callable(block index, workspace) behind every transformer block (never set on the product path)
        self._eng3: Optional["DepthEngine"] = None       # third rung: an engine with every encoder block and the whole head in split precision
        self.escalated = 0            # images the ladder has re-run so far (second + third rung)
        self.escalated3 = 0           # ... of which on the third rung
        self.tap_f8 = bool(weights.tap_f8)   # the taps (and with them the second rung's products) carry fp8 correction terms
        self.last_ratio = None        # per-image sum s(1-s) / sum s of the most recent call (CPU tensor), None when the ladder is off
        self.last_diversity = None    # per-image token diversity of the last tap (see _image_stats)
        self.last_input_diversity = None   # ... and of the patchified input
        # device mode of the ladder (forward(on_device=...), _ladder_device): per image the rung and r of the most recent such call and the running
        # counts (calls, images on rung >= 2, on rung 3, unserved), all ON THE DEVICE -- read with device_ladder_report(), which is what synchronises
        self.last_rungs_dev: Optional[torch.Tensor] = None
        self.last_ratio_dev: Optional[torch.Tensor] = None
        self.ladder_counts_dev: Optional[torch.Tensor] = None
        self._dev_state: Dict[tuple, tuple] = {}     # (B, device) -> (rung int32 [B], ratio float64 [B], counts int64 [4]); never dropped: captured graphs hold their addresses
        self._ws: "OrderedDict[tuple, Workspace]" = OrderedDict()
        self._graphs: "OrderedDict[tuple, object]" = OrderedDict()   # key -> _GraphedForward | False (capture refused) | int (sightings)
        self._lock = threading.Lock()
        self._streams: Dict[str, list] = {}      # device -> the three side streams of the head's forked section

    def max_batch(self, H: int, W: int) -> int:
        if H * W > MAX_ROWS:
            raise HipExtError(f"a {H}x{W} image has more than 2^24 pixels, the row limit of one kernel launch: "
                              "use hip_ext.tiling.tiled_amodal_forward / tiled_raw_forward")
        return max(1, MAX_ROWS // (H * W))

    def workspace(self, B, H, W, device) -> Workspace:
        key = (B, H, W, str(device))
        ws = self._ws.get(key)
        if ws is None:
            while len(self._ws) >= max(1, MAX_WORKSPACES):
                self._ws.popitem(last=False)      # least recently used shape; a captured graph holds its own reference (_GraphedForward.ws)
            ws = Workspace(self.w, B, H, W, device)
            self._ws[key] = ws
        else:
            self._ws.move_to_end(key)
        return ws

    def _side_streams(self, device):
        key = str(device)
        st = self._streams.get(key)
        if st is None:
            st = self._streams[key] = [torch.cuda.Stream(device=device) for _ in range(3)]
        return st

    def saturation_report(self, x: torch.Tensor, guide: Optional[torch.Tensor]):
        """Diagnostic forward, not the hot path: runs ``_forward`` with a probe behind every launch that writes an operand-typed tensor and
        returns ``(output, report)``; ``report`` maps "<kernel> #<launch index> [rows x cols]" to the number of elements that sit at the fp16
        clamp (+-65504: to_op saturates instead of overflowing to inf) or are non-finite.  An empty report = nothing saturated.  Meant for
        real checkpoints with massive activations (the synthetic fills never get near the clamp)."""
        global _probe
        _probe = []
        try:
            out = self._forward(x, guide)
            torch.cuda.synchronize(x.device)
            rep = {label: int(c.item()) for label, c in _probe if int(c.item())}
        finally:
            _probe = None
        return out, rep

    # ---- small helpers over igemm ---------------------------------------------------------
    @staticmethod
    def _mm(A, p: O.Packed, act: O.ActForm, **kw):
        """One ada_igemm launch: the rows of ``A`` (row stride = its last dimension), written in the form ``act``, against the packed weights ``p``."""
        k_igemm(A=A, W=p.t, **O.walk(p, act, A.shape[-1]), **kw)

    @classmethod
    def _conv3(cls, src_pad, p, act, M, N, grid, stride=1, cin=None, k_alg=None, **kw):
        """3x3 conv over a zero-bordered NHWC tensor."""
        B, Hp, Wp, Cp = src_pad.shape
        cls._mm(src_pad, p, act, M=M, N=N, k_alg=k_alg if k_alg is not None else 9 * (cin or p.seg), a_mode=A_CONV3, conv=(grid[0], grid[1], Hp, Wp, stride), **kw)

    def forward(self, x: torch.Tensor, guide: Optional[torch.Tensor], normalise: Optional[bool] = None, on_device=False) -> torch.Tensor:
        """One forward.  ``normalise`` overrides the engine's default for the fused ImageNet normalisation of the input (the
        patchify kernel applies (x - mean) / std on the fly: callers holding a [0, 1] image need no separate normalise pass).  The smallest problems are bound by the host's launch rate (~230 launches per image): for those the launch
        sequence is captured once per input shape into a HIP graph and replayed, bit-identically (``ADA_GRAPH`` = auto | 1 | 0).
        ``on_device`` = False | True | "head": the precision ladder in its device mode (_ladder_device) -- every rung for the whole batch, the decision taken by a
        kernel, no host read: the only form of the ladder that runs inside a caller's stream capture.  Ignored by an engine without a ladder."""
        if not x.is_cuda:
            raise HipExtError("DepthEngine.forward: input must live on a HIP device (no CPU fallback in the product path)")
        if on_device not in (False, True, "head"):
            raise HipExtError(f"DepthEngine.forward: on_device={on_device!r} (False | True | 'head')")
        norm = self.normalise_input if normalise is None else bool(normalise)
        if on_device is not False and self.ladder is not None:
            ladder = (lambda x_, g_, first=None: self._ladder_device(x_, g_, norm, on_device, first=first))
        else:
            ladder = (lambda x_, g_, first=None: self._ladder(x_, g_, norm, first=first))
        mode = GRAPH_MODE
        # (round 6: with the head's branches on side streams the plain launches of a single ViT-B / ViT-L image are FASTER than the replay -- 2.68 / 5.27 ms against
        #  3.00 / 5.84 ms, profiles/r06_g_* -- so "auto" replays only the model that is bound by the host's launch rate: ViT-S)
        use = mode == "1" or (mode == "auto" and self.w.encoder in GRAPH_AUTO_ENCODERS and x.shape[0] * x.shape[-2] * x.shape[-1] <= GRAPH_AUTO_PIXELS)
        # replay bypasses the Python wrappers: with a KernelTimer or a tile log attached the launches must be issued one by one
        if not use or instrumented() or torch.cuda.is_current_stream_capturing():
            return ladder(x, guide)
        # the kernel variant / tile override / fused-tail switch in force at capture time are baked into the graph
        key = (tuple(x.shape), None if guide is None else tuple(guide.shape), str(x.device), debug_epoch(), FUSED_TAIL, SUBPIXEL, OC1_COMMUTE, norm)
        with self._lock:
            g = self._graphs.get(key)
            if g is not None:
                self._graphs.move_to_end(key)
            if g is None or isinstance(g, int):
                seen = (g or 0) + 1
                if mode != "1" and seen < 2:       # first sighting of this shape: plain launches, capture when it comes back
                    self._graphs[key] = seen
                    g = False
                else:
                    try:
                        g = _GraphedForward(self, x, guide, norm)
                    except RuntimeError as e:   # capture refused (e.g. an enclosing capture in another mode): same kernels, launched one by one
                        import warnings
                        warnings.warn(f"HIP-graph capture of the forward failed ({e}); this shape runs as plain launches")
                        g = False
                    self._graphs[key] = g
                while len(self._graphs) > max(1, MAX_GRAPHS):
                    self._graphs.popitem(last=False)
        if g is False:
            return ladder(x, guide)
        return g(x, guide, (lambda ws_, out_, x_, g_: ladder(x_, g_, first=(ws_, out_))) if self.ladder is not None else None)

    # ---- precision ladder: the rungs run here, every decision is hip_ext.ladder's ----------------------
    def _second_weights(self) -> PackedWeights:
        """The second rung's head-only weights, packed on first use."""
        if self._w_hi is None:
            self._w_hi = self.ladder["make"]()
        return self._w_hi

    def _third_engine(self) -> "DepthEngine":
        """The third rung: an engine of its own with every encoder block and the whole head in split precision, built on first use."""
        if self._eng3 is None:
            self._eng3 = self.ladder["make3"]()
        return self._eng3

    @staticmethod
    def _third_workspace(eng3: "DepthEngine", out: torch.Tensor) -> Workspace:
        """The workspace behind the output ``eng3.forward`` has just returned -- looked up by shape (a replayed graph of eng3 writes the one it captured, which an
        LRU eviction can have replaced under this key: ADVICE.md)."""
        return eng3.workspace(out.shape[0], out.shape[-2], out.shape[-1], out.device)

    def _image_stats(self, eng: "DepthEngine", ws: Workspace, out: torch.Tensor):
        """The ladder's per-image statistics of one rung's run -- ``out`` and the full workspace ``ws`` of ``eng`` (this engine or the third rung's) that produced it:
        one deterministic reduction each, ONE host read of (8 + D / 64 + patch width / 64) x 2 floats per image (the forward's only synchronisation).  Returns
        (r, flat, tap_div, in_div), float64 / bool CPU tensors per image:
        r -- the sensitivity of the metric mean|a - b| / mean|b| to a logit error, from the output itself (ada_depth_stats_fwd): sum s(1-s) / sum s behind a sigmoid
        (0.3-0.5 for maps that span (0, 1), -> 1 for maps near 0, where nothing is left of the sigmoid's compression), (positive outputs) / sum out behind a ReLU (a
        clipped pixel carries no error; a map that is mostly clipped with the rest just above the kink has a small denominator), N / sum |out| for bare logits; zeros
        while the ladder has no r threshold.
        tap_div -- the TOKEN DIVERSITY of the last tap (ada_token_diversity_fwd: sum of the feature columns' variances over the image's patch tokens / sum of their
        mean squares): 0.23-0.53 on noise and image-like inputs, 0.02 on constant and checkerboard images, where every patch token is the same up to its position and
        the rounding errors add coherently over positions; None without lad["div"].
        in_div -- the same over the PATCHIFIED INPUT: the raw models' last tap does not tell (synthetic raw ViT-B at 518^2: token diversity 0.18 on an all-zero
        image, 0.11 on a noise image; profiles/r05_aa_*), the input does.
        flat -- tap_div < lad["div"] or in_div < lad["div_in"].
        The sizes are ``eng``'s (whose buffers are read); the ladder and the final activation are this engine's -- the third-rung engine is built from the same
        module and has no ladder of its own (and calibrate() switches the activation of both)."""
        lad = self.ladder
        B, D = out.shape[0], eng.w.dim
        has_r = "r" in lad or "r3" in lad
        has_div = lad.get("div", 0.0) > 0.0
        has_in = ws.stat_in is not None
        if has_r:
            self._depth_sums(out, ws.stat_sums)
        if has_div:
            k_token_diversity(ws.taps[3], ws.taps[3].shape[1], B, ws.ph * ws.pw, D, ws.stat_div)
        if has_in:
            k_token_diversity(ws.a_pe, ws.a_pe.shape[1], B, ws.ph * ws.pw, eng.w.pe_seg, ws.stat_in)
        host = ws.stat_buf.cpu().double()
        return stats_from_host(host, B, STAT_CHUNKS, (D + 63) // 64, has_r, lad["div"] if has_div else None, has_in, lad.get("div_in", 1e-4))

    def _depth_sums(self, out: torch.Tensor, sums: torch.Tensor):
        """The one launch of ada_depth_stats_fwd for the ladder: (sum |f|, sum w) of every image of ``out`` in STAT_CHUNKS chunks."""
        k_depth_stats(out, sums, self.final_act)

    def _ratio_of(self, out: torch.Tensor) -> torch.Tensor:
        """r of every image of ``out`` (see _image_stats) -- one reduction + one host read.  For a head run on a SUBSET of a workspace's images (the first rung
        behind the second), whose ``out`` has fewer rows than the workspace's statistics buffer."""
        sums = torch.empty(out.shape[0], STAT_CHUNKS, 2, dtype=torch.float32, device=out.device)
        self._depth_sums(out, sums)
        st = sums.cpu().double().sum(1)
        return st[:, 1] / st[:, 0].clamp_min(1e-300)

    def _ladder(self, x: torch.Tensor, guide: Optional[torch.Tensor], norm: Optional[bool], first=None) -> torch.Tensor:
        """One forward through the precision ladder.  FIRST RUNG: this engine's own weights -- for the sigmoid ViT-B / ViT-L models the DPT
        head on single fp16 operands, counting on the sigmoid to compress the logit error it leaves (~1.2e-3 mean absolute); in the metric that error arrives
        multiplied by the image's r (_image_stats).  SECOND RUNG (lad["make"], thresholded by lad["r"]): the HEAD ONLY (27 % of the FLOPs) re-run in split precision
        from the four taps, which this engine keeps [hi | lo] for the purpose.  THIRD RUNG (lad["make3"], lad["r3"], and every flat image): the whole forward,
        encoder blocks and head, in split precision -- at the bottom of the range the second rung's own logit error (the ENCODER's operand rounding) is what shows,
        and on constant / checkerboard inputs the rounding errors add coherently in the encoder as well.  Thresholds are calibrated per checkpoint (calibrate()).

        The rung of an image is a pure function of its own results (hip_ext.ladder.ladder_decide): deterministic, independent of the rest of the batch.  Which rung
        runs FIRST is a matter of cost alone: the one most images of this engine's previous call ended on (next_start_rung; a stream of low-mean images does not pay
        12 ms of first-rung head per bs=32 step for nothing), whose r decides for every image outside a guard band around the thresholds; for the others the first
        rung is run and its r decides, exactly as if it had run first.  Every image carries the output of its rung, bit for bit, in every order.
        ``first``: the (workspace, output) of a first-rung run a graph replay has already made (_GraphedForward's ``post`` hook).  Off under stream capture (a
        caller's own HIP graph cannot hold a data-dependent branch): the first rung's output is returned, no counter moves."""
        lad = self.ladder
        capturing = torch.cuda.is_current_stream_capturing()
        start = 1
        if lad is not None and first is None and LADDER_STICKY and not capturing:
            if self._start_rung == 3 and "make3" in lad and lad.get("r3", float("inf")) < float("inf"):
                start = 3
            elif self._start_rung == 2 and "make" in lad:
                start = 2
        # 1. the start rung for the whole batch
        if start == 1:
            eng = self
            ws, out = first if first is not None else (None, self._forward(x, guide, norm))
            if lad is None or capturing:
                return out
            if ws is None:
                ws = self.workspace(out.shape[0], out.shape[-2], out.shape[-1], out.device)
        elif start == 2:
            eng = self
            ws = self._forward(x, guide, norm, head=False)
            out = self._head_for(ws, ws.B, None, self._second_weights())
        else:
            eng = self._third_engine()
            out = eng.forward(x, guide, norm)
            ws = self._third_workspace(eng, out)
        B, dev = out.shape[0], out.device

        def rows(t, idx):
            return None if t is None else t.index_select(0, idx.to(dev))
        # 2. its statistics decide every image they can
        ratio, flat, tap_div, in_div = self._image_stats(eng, ws, out)
        rung = ladder_decide(ratio, flat, lad, start, LADDER_GUARD)
        # 3. the first rung for the others.  idx1 = the batch rows of the images of the first-rung run, ASCENDING, so that row j of that run (out1, and the taps
        #    in ws1) is image idx1[j]: everything for start rung 1; the undecided images otherwise (start rung 2: their taps are rows idx1 of ws itself)
        idx1, ws1, out1 = torch.arange(B), ws, out
        if start != 1:
            idx1, out1 = torch.nonzero(rung == 0).flatten(), None
        if start != 1 and idx1.numel() > 0:
            if start == 2:      # the first-rung head over the same taps; not flat, or ladder_decide had decided them
                out1 = self._head_for(ws, B, None if idx1.numel() == B else idx1, self.w)
                r1, flat1 = self._ratio_of(out1), torch.zeros(idx1.numel(), dtype=torch.bool)
            else:               # a plain forward of the subset; r AND the diversities are those of this run
                out1 = self._forward(rows(x, idx1), rows(guide, idx1), norm)
                ws1 = self.workspace(out1.shape[0], out1.shape[-2], out1.shape[-1], dev)
                r1, flat1, d1, di1 = self._image_stats(self, ws1, out1)
                in_div[idx1] = di1
                if tap_div is not None:
                    tap_div[idx1] = d1
            ratio[idx1] = r1
            rung[idx1] = ladder_decide(r1, flat1, lad, 1, LADDER_GUARD)
        # 4. every image from the output of its rung, running only what is not in hand
        #    (order as before: third rung, second, first).  `have`: the start rung's output IS the image's; `pos`: batch row -> row of the first-rung run
        have = rung == start
        if start == 3:
            have[idx1] = False      # (run again on the subset, as the first-rung-first order does: the two runs' bits have not been compared)
        pos = torch.zeros(B, dtype=torch.int64)
        pos[idx1] = torch.arange(idx1.numel())
        need1, need2, need3 = (torch.nonzero((rung == k) & ~have).flatten() for k in (1, 2, 3))
        if need3.numel() == B:
            out = self._third_engine().forward(x, guide, norm)
        elif need3.numel() > 0:
            out.index_copy_(0, need3.to(dev), self._third_engine().forward(rows(x, need3), rows(guide, need3), norm))
        if need2.numel() > 0:       # the head re-run from the taps of the first-rung run (never from start rung 2: its rung-2 images are in hand)
            assert start != 2
            hi = self._head_for(ws1, ws1.B, None if need2.numel() == ws1.B else pos[need2], self._second_weights())
            out = hi if need2.numel() == B else out.index_copy_(0, need2.to(dev), hi)
        if need1.numel() > 0:
            out = out1 if need1.numel() == B else out.index_copy_(0, need1.to(dev), rows(out1, pos[need1]))
        # 5. the books
        n2, n3 = rung_counts(rung)
        self.escalated += n2
        self.escalated3 += n3
        self.second_rung_first_calls += int(start == 2)
        self.third_rung_first_calls += int(start == 3)
        self._start_rung = next_start_rung(rung, "make" in lad)
        self.last_ratio = ratio if ("r" in lad or "r3" in lad) else None      # per image: r1 where the first rung ran for it, else the start rung's r
        self.last_diversity, self.last_input_diversity = tap_div, in_div      # always B long: of the rung that ran first for the image
        if n2 and not self._warned:
            self._warned = True
            import warnings
            warnings.warn(f"precision ladder: {n2} of {B} image(s) re-run in split precision (second rung: head only; third: whole forward; {n3} on the third) -- "
                          f"r up to {float(ratio.max()):.3g} against thresholds {lad.get('r')} / {lad.get('r3')}; counted in DepthEngine.escalated / escalated3 "
                          "(this message appears once per engine; module.precision_ladder = False switches the ladder off)")
        return out

    def _ladder_device(self, x: torch.Tensor, guide: Optional[torch.Tensor], norm: Optional[bool], mode, first=None) -> torch.Tensor:
        """The ladder in its DEVICE mode: the data-independent form of _ladder.  The first rung for the batch, the three statistics launches
        of _image_stats, then EVERY further rung the ladder has for the whole batch -- the second rung's head from the first rung's taps, the third-rung engine's
        forward -- and one launch of ada_ladder_select_fwd, which takes ladder_decide(r, flat, lad, 1, .) per image from the statistics where they lie and pastes the
        image's rows from the output of its rung into the first rung's output, which is returned.  A fixed launch sequence with no host read: it runs inside a
        caller's stream capture, and every image carries the bits of the rung the eager ladder names for it.  The price is every rung for every image, every call.
        ``mode`` "head": rungs 1 and 2 only -- no third engine is built (no second full-batch workspace); an image that decides 3 carries the second rung's rows
        (the first's on a ladder without a second rung) and is counted as unserved.  The thresholds enter the launch by value, as ``self.ladder`` holds them now.
        Nothing is decided in Python: escalated / escalated3 / _start_rung / last_ratio do not move; rung, r and the running counts stay on the device
        (last_rungs_dev, last_ratio_dev, ladder_counts_dev; device_ladder_report() reads them).  Under capture everything must exist already: a warm-up call in
        the same mode and shape outside the capture builds the second rung's weights, the third engine, the workspaces and the device tensors.
        ``first``: as for _ladder (the engine's own graph replay captures the first rung only; the rest follows here as plain launches)."""
        lad = self.ladder
        inf = float("inf")
        B, H, W, dev = x.shape[0], x.shape[-2], x.shape[-1], x.device
        has2, has3 = "make" in lad, "make3" in lad
        has_r = "r" in lad or "r3" in lad
        has_div = lad.get("div", 0.0) > 0.0
        has_in = self.w.pe_seg // 64 > 0      # Workspace.stat_in
        run3 = mode != "head" and has3 and (lad.get("r3", inf) < inf or has_div or has_in)
        skey, wkey = (B, str(dev)), (B, H, W, str(dev))
        if torch.cuda.is_current_stream_capturing():
            missing = [what for what, there in (
                ("the first rung's workspace", wkey in self._ws),
                ("the second rung's weights and workspace", not has2 or (self._w_hi is not None and (False,) + wkey in self._ws_hi)),
                ("the third-rung engine and its workspace", not run3 or (self._eng3 is not None and wkey in self._eng3._ws)),
                ("the device-side rung / ratio / counts tensors", skey in self._dev_state)) if not there]
            if missing:
                raise HipExtError(f"precision ladder on the device under stream capture: {', '.join(missing)} not built for a {B}x3x{H}x{W} input -- warm up with one "
                                  f"forward in the same mode (ladder_on_device = {mode!r}) and shape OUTSIDE the capture (packing and allocating synchronise)")
        state = self._dev_state.get(skey)
        if state is None:      # one running count per device, shared by every batch size
            counts = next((st[2] for k, st in self._dev_state.items() if k[1] == skey[1]), None)
            state = self._dev_state[skey] = (torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.float64, device=dev),
                                             counts if counts is not None else torch.zeros(4, dtype=torch.int64, device=dev))
        rung, ratio, counts = state
        if first is None:
            out = self._forward(x, guide, norm)
            ws = self.workspace(B, H, W, dev)
        else:
            ws, out = first
        # the statistics of the first rung's run: the launches of _image_stats, without its host read
        if has_r:
            self._depth_sums(out, ws.stat_sums)
        if has_div:
            k_token_diversity(ws.taps[3], ws.taps[3].shape[1], B, ws.ph * ws.pw, self.w.dim, ws.stat_div)
        if has_in:
            k_token_diversity(ws.a_pe, ws.a_pe.shape[1], B, ws.ph * ws.pw, self.w.pe_seg, ws.stat_in)
        src2 = self._head_for(ws, B, None, self._second_weights()) if has2 else None
        src3 = self._third_engine().forward(x, guide, norm) if run3 else None
        k_ladder_select(ws.stat_sums if has_r else None, ws.stat_div if has_div else None, ws.stat_in if has_in else None,
                        lad["r"] if has2 and "r" in lad else inf, lad["r3"] if has3 and "r3" in lad else inf, lad.get("div", 0.0), lad.get("div_in", 1e-4),
                        has2, has3, has_r, out, src2, src3, rung, ratio, counts)
        self.last_rungs_dev, self.last_ratio_dev, self.ladder_counts_dev = rung, ratio, counts
        return out

    def device_ladder_report(self) -> Optional[dict]:
        """What the device mode of the ladder has left on the device, read NOW (this is the call that synchronises; after a graph replay it shows the replay's
        values): dict(rungs=int64 [B], ratio=float64 [B] -- of the most recent device-mode call (or replay) of that batch size -- and the running totals calls,
        escalated, escalated3, unserved since the engine was built).  None before the first device-mode call."""
        if self.last_rungs_dev is None:
            return None
        calls, n2, n3, unserved = (int(v) for v in self.ladder_counts_dev.cpu())
        return dict(rungs=self.last_rungs_dev.cpu().long(), ratio=self.last_ratio_dev.cpu(), calls=calls, escalated=n2, escalated3=n3, unserved=unserved)

    def _head_for(self, ws: Workspace, B: int, idx: Optional[torch.Tensor], w: PackedWeights) -> torch.Tensor:
        """The DPT head with the weights ``w`` (this engine's own = first rung, or the second rung's) for the images ``idx`` (CPU index tensor; None = all B) of the
        taps in ``ws``, on a head-only workspace of its own (cached per shape)."""
        if idx is None and w is self.w:
            return self._head(ws, B)
        Be = B if idx is None else int(idx.numel())
        dev = ws.taps[0].device
        key = (w is self.w, Be, ws.H, ws.W, str(dev))
        ws2 = self._ws_hi.get(key)
        if ws2 is None:
            while len(self._ws_hi) >= max(1, MAX_WORKSPACES):
                self._ws_hi.popitem(last=False)
            ws2 = Workspace(w, Be, ws.H, ws.W, dev, head_only=True)
            self._ws_hi[key] = ws2
        else:
            self._ws_hi.move_to_end(key)
        own = ws2.taps
        own_cls = getattr(ws2, "cls_op", None)      # use_clstoken models: the read-out also reads the final-LayerNorm'd class tokens of the first rung
        try:
            if idx is None:
                ws2.taps = ws.taps        # every image of the batch: the head reads the encoder's taps in place
                if own_cls is not None:
                    ws2.cls_op = ws.cls_op
            else:
                sel = idx.to(dev)
                for t in range(4):
                    torch.index_select(ws.taps[t].view(B, -1), 0, sel, out=own[t].view(Be, -1))
                    if own_cls is not None:
                        torch.index_select(ws.cls_op[t], 0, sel, out=own_cls[t])
            return self._head(ws2, Be, w)
        finally:
            ws2.taps = own
            if own_cls is not None:
                ws2.cls_op = own_cls

    def calibrate(self, x: torch.Tensor, guide: Optional[torch.Tensor], budget: float = 9e-4, safety: float = 1.1, flat_index: Optional[int] = None,
                  rule: str = "cross") -> dict:
        """Self-calibration of the ladder's thresholds for THIS checkpoint, on the device, with no oracle (round 6; round 5's thresholds were ~12 constants fitted
        to synthetic weights).  The calibration images ``x`` ([0, 1] RGB; ``guide`` with the model's guide channels) run through the first rung, through the second
        (head re-run from the first rung's taps, where the policy has one) and through the third-rung engine -- every encoder block and the whole head in split
        precision, 1.6-3.7e-4 from the reference where it was measured -- with the final activation switched OFF, i.e. as logits z1, z2, z3.  For a grid of bias
        shifts d (the final bias is added in fp32: moving it moves the map's operating point and nothing else) the metric of rung k against the third,
        e = mean|f(z_k + d) - f(z_3 + d)| / mean f(z_3 + d), is known together with the image's r (see _image_stats); e / r is the rung's sensitivity-normalised
        logit error eps_k.  Rule "cross" (default): a rung is left at the smallest r at which any calibration point has safety * e > budget; rule "global":
        at budget / (safety * max eps_k) -- the worst eps anywhere on the grid (round 5's hand-fitted constants, 0.42 / 0.45, are what "global" returns for the
        synthetic fills they were fitted on at budget 9e-4).  r from rung 1, r3 from rung 2 (heads without a second rung: r3 from rung 1).  ``flat_index``: a
        constant image of the batch -- left out of eps, used to place the tap-diversity threshold between it and the other images (geometric mean), or to switch that
        trigger off where the last tap does not tell them apart (outlier-dominated tokens).  Returns the numbers; the caller installs them (DA2/dpt.py)."""
        lad = self.ladder
        if lad is None or "make3" not in lad:
            raise HipExtError("calibrate: this engine has no precision ladder")
        B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
        eng3 = self._third_engine()
        act = self.final_act
        keep = (self.final_act, eng3.final_act)
        z2 = None
        try:
            self.final_act = eng3.final_act = ACT_NONE
            z1 = self._forward(x, guide, True)
            ws = self.workspace(B, H, W, x.device)
            k_token_diversity(ws.taps[3], ws.taps[3].shape[1], B, ws.ph * ws.pw, self.w.dim, ws.stat_div)
            dv = ws.stat_div.double().sum(1)
            tap_div = (dv[:, 0] / dv[:, 1].clamp_min(1e-300)).cpu()
            if "make" in lad:
                w_hi = self._second_weights()
                ws2 = Workspace(w_hi, B, H, W, x.device, head_only=True)
                ws2.taps = ws.taps
                if getattr(ws2, "cls_op", None) is not None:
                    ws2.cls_op = ws.cls_op
                z2 = self._head(ws2, B, w_hi)
            z3 = eng3._forward(x, guide, True)
        finally:
            self.final_act, eng3.final_act = keep
        use = [i for i in range(B) if i != flat_index]
        sel = torch.tensor(use, device=x.device)
        res = ladder_thresholds(z1.index_select(0, sel), None if z2 is None else z2.index_select(0, sel), z3.index_select(0, sel), act, budget, safety, rule)
        res.update(images=len(use), size=(H, W))
        if flat_index is not None:
            dmin, dflat = float(tap_div[use].min()), float(tap_div[flat_index])
            res.update(tap_diversity_images_min=dmin, tap_diversity_flat=dflat, div=math.sqrt(dmin * dflat) if dflat < 0.25 * dmin else 0.0)
        return res

    def _forward(self, x: torch.Tensor, guide: Optional[torch.Tensor], norm: Optional[bool] = None, head: bool = True):
        """The first rung: encoder + DPT head -> depth map.  ``head=False``: the encoder only -- returns the Workspace holding the four taps (_ladder, second rung first)."""
        w = self.w
        if not x.is_cuda:
            raise HipExtError("DepthEngine.forward: input must live on a HIP device (no CPU fallback in the product path)")
        B, C, H, W = x.shape
        assert C == 3
        assert H % PATCH == 0, f"Input image height {H} is not a multiple of patch height {PATCH}"
        assert W % PATCH == 0, f"Input image width {W} is not a multiple of patch width: {PATCH}"
        if w.guided:
            if guide is None or guide.shape[1] != w.guide_channels:
                raise HipExtError(f"guide tensor with {w.guide_channels} channels required")
            guide = guide.contiguous().float()
        x = x.contiguous().float()
        ws = self.workspace(B, H, W, x.device)
        D, heads = w.dim, w.heads
        ph, pw = ws.ph, ws.pw
        Np = ph * pw
        N = Np + 1
        T, P = B * N, B * Np

        # ---- tokens: patchify (+normalise) -> one GEMM over [rgb | guide] -> + bias + pos, cls row ----------
        norm = self.normalise_input if norm is None else norm
        mean = (0.485, 0.456, 0.406) if norm else None
        inv_std = (1 / 0.229, 1 / 0.224, 1 / 0.225) if norm else None
        k_patchify(x, guide if w.guided else None, B, w.guide_channels, H, W, mean, inv_std, ws.a_pe, ws.a_pe.shape[1], split=True)
        pos = w.pos_embed(ph, pw)
        self._mm(ws.a_pe, w.pe_w, O.A_HILO, M=P, N=D, k_alg=(3 + w.guide_channels) * 196, bias=w.pe_b, res=pos, ldr=D, res_row_mod=Np, res_row_off=1,
                 flags=EP_BIAS | EP_RESIDUAL, out_f32=ws.x, ldo_f32=D, map_f32=MAP_TOKEN, map_h=Np)
        k_write_cls(ws.x, B, N, D, w.cls, pos)

        # ---- transformer blocks ------------------------------------------------------------------
        taps = TAPS[w.encoder]
        tap_seg = w.act_form("tap").split_seg(D)
        ldy, ldo, ldh = ws.y.shape[1], ws.o.shape[1], ws.hd.shape[1]
        ln1_done = False    # block i's norm1 output already sits in ws.y (emitted by the tap LayerNorm of block i - 1, see below)
        for i, blk in enumerate(w.blocks):
            last = i == len(w.blocks) - 1
            act = w.act_form(i)     # of the rows this block's four linear layers read: LayerNorm output, attention output, MLP hidden
            if not ln1_done:
                k_layernorm(ws.x, D, T, D, blk["ln1_w"], blk["ln1_b"], LN_EPS, out_op=ws.y, ld_op=ldy, split_seg=act.split_seg(D))
            ln1_done = False
            self._mm(ws.y, blk["qkv_w"], act, M=T, N=3 * D, k_alg=D, bias=blk["qkv_b"], flags=EP_BIAS, out_op=ws.qkv, ldo_op=3 * D)
            k_attention(ws.qkv, ws.o, B, N, heads, ld_out=ldo if ldo != D else 0, split_seg=act.split_seg(D))
            hid = blk["hidden"]
            self._mm(ws.o, blk["proj_w"], act, M=T, N=D, k_alg=D, bias=blk["proj_b"], gamma=blk["ls1"], res=ws.x, ldr=D,
                     flags=EP_BIAS | EP_GAMMA | EP_RESIDUAL, out_f32=ws.x, ldo_f32=D)
            k_layernorm(ws.x, D, T, D, blk["ln2_w"], blk["ln2_b"], LN_EPS, out_op=ws.y, ld_op=ldy, split_seg=act.split_seg(D))
            if w.ffn == "mlp":
                self._mm(ws.y, blk["fc1_w"], act, M=T, N=hid, k_alg=D, bias=blk["fc1_b"], flags=EP_BIAS | EP_GELU, out_op=ws.hd, ldo_op=ldh, split_seg=act.split_seg(hid))
                self._mm(ws.hd, blk["fc2_w"], act, M=T, N=D, k_alg=hid, bias=blk["fc2_b"], gamma=blk["ls2"], res=ws.x, ldr=D,
                         flags=EP_BIAS | EP_GAMMA | EP_RESIDUAL, out_f32=ws.x, ldo_f32=D)
            else:
                self._mm(ws.y, blk["w12_w"], act, M=T, N=2 * hid, k_alg=D, bias=blk["w12_b"], flags=EP_BIAS | EP_SWIGLU, out_op=ws.hd, ldo_op=ldh, split_seg=act.split_seg(hid))
                self._mm(ws.hd, blk["w3_w"], act, M=T, N=D, k_alg=hid, bias=blk["w3_b"], gamma=blk["ls2"], res=ws.x, ldr=D,
                         flags=EP_BIAS | EP_GAMMA | EP_RESIDUAL, out_f32=ws.x, ldo_f32=D)
            if self.block_probe is not None:      # diagnostic (tools/stage_errors.py): the residual stream behind block i
                self.block_probe(i, ws)
            if i in taps:  # shared final LayerNorm on the tap, cls row dropped (dinov2.py:337-340)
                tap = ws.taps[taps.index(i)]
                if not last:
                    # the next block's norm1 (block.py:84) reads the very rows this LayerNorm reads: one pass over x, two outputs with the
                    # same statistics -- norm1(x) for all T rows into ws.y, norm(x) without the cls rows into the tap
                    nb = w.blocks[i + 1]
                    k_layernorm(ws.x, D, T, D, nb["ln1_w"], nb["ln1_b"], LN_EPS, out_op=ws.y, ld_op=ldy, split_seg=w.act_form(i + 1).split_seg(D), weight2=w.norm_w, bias2=w.norm_b,
                                out2_op=tap, ld2_op=tap.shape[1], out2_group=N, out2_skip=1, split_seg2=tap_seg)
                    ln1_done = True
                else:
                    k_layernorm(ws.x, D, P, D, w.norm_w, w.norm_b, LN_EPS, group_in=N, skip=1, out_op=tap, ld_op=tap.shape[1],
                                split_seg=tap_seg)
                if w.readout:   # the class token of every image (row b * N of the token matrix): input row stride N * D
                    j = taps.index(i)
                    k_layernorm(ws.x, N * D, B, D, w.norm_w, w.norm_b, LN_EPS, out_op=ws.cls_op[j], ld_op=ws.cls_op[j].shape[1],
                                split_seg=tap_seg)

        return self._head(ws, B) if head else ws

    def _head(self, ws: Workspace, B: int, w: Optional[PackedWeights] = None) -> torch.Tensor:
        w = self.w if w is None else w
        D = w.dim
        ph, pw = ws.ph, ws.pw
        P = B * ph * pw
        oc = w.oc
        Fch = w.features
        grid = ws.grid
        rows = [B * g[0] * g[1] for g in grid]

        ocp, Fp = ws.ocp, ws.Fp
        first = "ip" if w.amodal_head else "rn"     # the family of the contraction that reads the reassembled maps L[i]

        form = w.act_form     # reader -> the form of the buffer it reads: the producer's split_seg and the consumer's walk both come from it
        taps_in = ws.taps
        if w.readout:   # x = GELU(W_x x + (W_cls cls_b + b))  per image (DA2/dpt.py:164-167)
            Np = ph * pw
            for i in range(4):
                self._mm(ws.cls_op[i], w.ro_wc[i], form("tap"), M=B, N=D, k_alg=D, bias=w.ro_b[i], flags=EP_BIAS, out_f32=ws.cls_bias[i], ldo_f32=D)
                # one launch for the whole batch: the bias vector of row m is cls_bias[m // Np] (ada_igemm_args.bias_row_mod)
                self._mm(ws.taps[i], w.ro_wx[i], form("tap"), M=B * Np, N=D, k_alg=D, bias=ws.cls_bias[i], bias_row_mod=Np,
                         flags=EP_BIAS | EP_GELU, out_op=ws.taps_ro[i], ldo_op=ws.taps_ro[i].shape[1], split_seg=form("proj").split_seg(D))
            taps_in = ws.taps_ro
        # ---- per level i: reassemble (1x1 project + resize, dpt.py:171-173) -> [amodal: input_projection = conv3x3 -> channels-first LN -> ReLU,
        #      dpt.py:153-159,178-179] -> layerN_rn (blocks.py:20-24): fp32 copy for the residual adds + ReLU'd operand copy for conv1.  The four chains are
        #      independent (chain(i) below touches level-i buffers only) -----

        def project(i, out, reader, **kw):      # projects[i] of the tap into ``out``, in the form ``reader`` needs
            self._mm(taps_in[i], w.proj_w[i], form("tap"), M=P, N=oc[i], k_alg=D, bias=w.proj_b[i], flags=EP_BIAS, out_op=out, ldo_op=out.shape[-1],
                     split_seg=form(reader).split_seg(ocp[i]), **kw)

        def reassemble(i):
            if i in w.sp:     # 1x1 project -> zero-bordered patch-grid tensor; the transposed conv runs inside the sub-pixel convolution below
                project(i, ws.tp[i], f"sp{i}", map_op=MAP_PAD, map_h=ph, map_w=pw)
            elif i < 2:
                s_ = 4 if i == 0 else 2
                t = ws.t0 if i == 0 else ws.t1
                rs_w, rs_b = (w.rs0_w, w.rs0_b) if i == 0 else (w.rs1_w, w.rs1_b)
                project(i, t, f"rs{i}")
                self._mm(t, rs_w, form(f"rs{i}"), M=P, N=s_ * s_ * oc[i], k_alg=oc[i], bias=rs_b, flags=EP_BIAS,
                         out_op=ws.L[i], ldo_op=ws.L[i].shape[3], map_op=MAP_SHUFFLE, map_h=ph, map_w=pw, shuffle_s=s_, shuffle_c=oc[i], split_seg=form(f"{first}{i}").split_seg(ocp[i]))
            elif i == 2:
                project(2, ws.L[2], first + "2", map_op=MAP_PAD, map_h=ph, map_w=pw)
            else:
                project(3, ws.pre3, "rs3", map_op=MAP_PAD, map_h=ph, map_w=pw)
                self._conv3(ws.pre3, w.rs3_w, form("rs3"), rows[3], oc[3], grid[3], stride=2, cin=oc[3], bias=w.rs3_b, flags=EP_BIAS,
                            out_op=ws.L[3], ldo_op=ws.L[3].shape[3], map_op=MAP_PAD, map_h=grid[3][0], map_w=grid[3][1], split_seg=form(first + "3").split_seg(ocp[3]))

        def input_projection(i):      # amodal only
            rn_seg = form(f"rn{i}").split_seg(ocp[i])
            if i in w.sp:
                # resize_layers[i] + input_projection[i][0] as one sub-pixel convolution over the patch grid: [P, s*s*oc] fp32, column block
                # (py*s + px) = output phase; the LayerNorm reads it in fine-pixel order and takes the transposed conv's bias back out where
                # a tap falls into the zero padding (the outermost ring of the fine grid)
                sp = w.sp[i]
                ncol = sp["s"] * sp["s"] * oc[i]
                self._conv3(ws.tp[i], sp["w"], form(f"sp{i}"), P, ncol, (ph, pw), k_alg=sp["taps_per_col"] * oc[i], bias=sp["b"], flags=EP_BIAS,
                            out_f32=ws.ipf[i], ldo_f32=ncol, tap_cols=oc[i], tap_mask=sp["masks"])
                k_layernorm(ws.ipf[i], ncol, rows[i], oc[i], w.ip_ln_w[i], w.ip_ln_b[i], LN_EPS, out_op=ws.L2[i], ld_op=ws.L2[i].shape[3],
                            map_op=MAP_PAD, map_h=grid[i][0], map_w=grid[i][1], relu=True, split_seg=rn_seg, unshuffle_s=sp["s"], tap_bias=sp["tapb"])
                return
            self._conv3(ws.L[i], w.ip_w[i], form(f"ip{i}"), rows[i], oc[i], grid[i], cin=oc[i], bias=w.ip_b[i], flags=EP_BIAS, out_f32=ws.ipf[i], ldo_f32=oc[i])
            k_layernorm(ws.ipf[i], oc[i], rows[i], oc[i], w.ip_ln_w[i], w.ip_ln_b[i], LN_EPS, out_op=ws.L2[i],
                        ld_op=ws.L2[i].shape[3], map_op=MAP_PAD, map_h=grid[i][0], map_w=grid[i][1], relu=True, split_seg=rn_seg)

        def layer_rn(i):
            rcu_seg = form(f"rcu{i}").split_seg(Fp)
            if not w.amodal_head and i in w.sp:
                # raw head: resize_layers[i] + layer{i+1}_rn as one sub-pixel convolution over the patch grid, then ONE re-layout pass: fine-pixel
                # order, the transposed conv's bias taken out on the outermost ring, fp32 copy for the residual adds + ReLU'd operand copy
                sp = w.sp[i]
                ncol = sp["s"] * sp["s"] * Fch
                self._conv3(ws.tp[i], sp["w"], form(f"sp{i}"), P, ncol, (ph, pw), k_alg=sp["taps_per_col"] * oc[i], bias=sp["b"], flags=EP_BIAS,
                            out_f32=ws.spf[i], ldo_f32=ncol, tap_cols=Fch, tap_mask=sp["masks"])
                k_layernorm(ws.spf[i], ncol, rows[i], Fch, None, None, LN_EPS, identity=True, relu=2, out_f32=ws.rnx[i], ld_f32=Fch, out_op=ws.rnr[i],
                            ld_op=ws.rnr[i].shape[3], map_op=MAP_PAD, map_h=grid[i][0], map_w=grid[i][1], split_seg=rcu_seg,
                            unshuffle_s=sp["s"], tap_bias=sp["tapb"])
                return
            src = ws.L2[i] if w.amodal_head else ws.L[i]
            self._conv3(src, w.rn_w[i], form(f"rn{i}"), rows[i], Fch, grid[i], cin=oc[i], flags=EP_RELU_OP, out_f32=ws.rnx[i], ldo_f32=Fch,
                        out_op=ws.rnr[i], ldo_op=ws.rnr[i].shape[3], map_op=MAP_PAD, map_h=grid[i][0], map_w=grid[i][1], split_seg=rcu_seg)

        def rcu(i, fw, unit, src_relu_pad, src_f32, **out):
            """ResidualConvUnit (blocks.py:57-80) at grid i: conv2(relu(conv1(relu(x)))) + x."""
            g, act = grid[i], form(f"rcu{i}")
            self._conv3(src_relu_pad, fw[f"u{unit}c1_w"], act, rows[i], Fch, g, cin=Fch, bias=fw[f"u{unit}c1_b"], flags=EP_BIAS | EP_RELU_OP,
                        out_op=ws.tmpa[i], ldo_op=ws.tmpa[i].shape[3], map_op=MAP_PAD, map_h=g[0], map_w=g[1], split_seg=act.split_seg(Fp))
            self._conv3(ws.tmpa[i], fw[f"u{unit}c2_w"], act, rows[i], Fch, g, cin=Fch, bias=fw[f"u{unit}c2_b"], res=src_f32, ldr=Fch,
                        flags=EP_BIAS | EP_RESIDUAL, **out)

        def chain(i):     # everything of level i that does not depend on another level; RCU 1 of levels 0-2 (blocks.py:131-133) reads rnr / rnx of its own level only
            reassemble(i)
            if w.amodal_head:
                input_projection(i)
            layer_rn(i)
            if i < 3:
                rcu(i, w.fuse[i], 1, ws.rnr[i], ws.rnx[i], out_f32=ws.r[i], ldo_f32=Fch)

        # (r[i] lives in ipf[i] where that is large enough and zf[i] in rnx[i] -- Workspace: both are dead by the time they are overwritten INSIDE chain i / after the join)
        forked = HEAD_STREAMS == "1" or (HEAD_STREAMS == "auto" and P <= HEAD_STREAMS_ROWS)
        if forked and not instrumented():
            cur = torch.cuda.current_stream(ws.oc1.device)
            side = self._side_streams(ws.oc1.device)
            for st_ in side:
                st_.wait_stream(cur)
            chain(0)                      # the finest level -- most of the work -- stays on the caller's stream
            for i, st_ in zip((1, 2, 3), side):
                with torch.cuda.stream(st_):
                    chain(i)
            for st_ in side:
                cur.wait_stream(st_)
        else:
            for i in range(4):
                chain(i)

        # ---- refinenet4..1 (blocks.py:123-148).  out_conv is applied BEFORE the bilinear resize: both are linear and
        #      the align_corners weights sum to one, so conv1x1(resize(x)) == resize(conv1x1(x)) at a quarter of the MACs.
        s_f32, s_pad = ws.rnx[3], ws.rnr[3]
        for i in (3, 2, 1, 0):
            fw = w.fuse[i]
            rcu(i, fw, 2, s_pad, s_f32, out_op=ws.u[i], ldo_op=ws.u[i].shape[1], split_seg=form(f"out{i}").split_seg(Fp))
            if i == 0 and w.oc1c is not None:
                break     # refinenet1.out_conv is part of output_conv1's tap maps (below)
            self._mm(ws.u[i], fw["out_w"], form(f"out{i}"), M=rows[i], N=Fch, k_alg=Fch, bias=fw["out_b"], flags=EP_BIAS, out_f32=ws.zf[i], ldo_f32=Fch)
            if i > 0:
                j = i - 1
                k_bilinear(ws.zf[i], Fch, B, grid[i][0], grid[i][1], grid[j][0], grid[j][1], Fch, add=ws.r[j], ld_add=Fch,
                           out_f32=ws.s[j], ld_f32=Fch, out_op=ws.sr[j], ld_op=ws.sr[j].shape[3], map_op=MAP_PAD, relu=True, split_seg=form(f"rcu{j}").split_seg(Fp))
                s_f32, s_pad = ws.s[j], ws.sr[j]
        g2 = ws.g296
        # ---- resize x2 -> output_conv1 (dpt.py:192-193) -> resize to (14 ph, 14 pw) -> output_conv2 (3x3, ReLU, 1x1, activation) (:194-195) ----
        if w.oc1c is not None:
            ntap = 9 * ws.half
            # u[0] plain against [w_hi | w_lo], or (split group "out0") [hi | lo8 | hi8]: a full split product with fp8 correction terms
            self._mm(ws.u[0], w.oc1c["w"], form("out0"), M=rows[0], N=ntap, k_alg=Fch, bias=w.oc1c["b"], flags=EP_BIAS, out_op=ws.tmaps, ldo_op=ntap)
            k_tapsum_resize(ws.tmaps, ntap, B, grid[0][0], grid[0][1], g2[0], g2[1], ws.half, w.oc1_b, ws.oc1, ws.half)
        else:
            k_bilinear(ws.zf[0], Fch, B, grid[0][0], grid[0][1], g2[0], g2[1], Fch, out_op=ws.p1, ld_op=ws.p1.shape[3], map_op=MAP_PAD, split_seg=form("oc1").split_seg(Fp))
            self._conv3(ws.p1, w.oc1_w, form("oc1"), B * g2[0] * g2[1], ws.half, g2, cin=Fch, bias=w.oc1_b, flags=EP_BIAS, out_f32=ws.oc1, ldo_f32=ws.half)
        out = torch.empty(B, 1, ws.H, ws.W, dtype=torch.float32, device=ws.oc1.device)
        if ws.fused_tail:
            k_dpt_tail(ws.oc1, ws.half, B, g2[0], g2[1], ws.H, ws.W, ws.halfp, w.oc2_w.t, w.oc2_b, w.tail_w, w.tail_b, self.final_act, out)
            return out
        k_bilinear(ws.oc1, ws.half, B, g2[0], g2[1], ws.H, ws.W, ws.half, out_op=ws.fin, ld_op=ws.fin.shape[3], map_op=MAP_PAD, split_seg=form("oc2").split_seg(ws.halfp))
        self._conv3(ws.fin, w.oc2_w, form("oc2"), B * ws.H * ws.W, w.oc2_w.t.shape[0], (ws.H, ws.W), cin=ws.half, bias=w.oc2_b, flags=EP_BIAS | EP_TAIL,
                    out_f32=out, ldo_f32=1, tail_w=w.tail_w, tail_b=w.tail_b, tail_act=self.final_act)
        return out
