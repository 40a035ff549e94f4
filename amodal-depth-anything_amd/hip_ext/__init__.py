"""hip_ext -- ctypes binding of libada_hip.so (the C ABI declared in include/ada_hip.h).

PyTorch is used here for device memory and streams only: every wrapper hands raw device pointers,
sizes and the current HIP stream to the library.  There is NO fallback: if the shared library is
missing or a tensor is not on a HIP device the call raises -- the product path never computes on
the CPU (the fp32 CPU oracle under /oracle is test infrastructure and is never imported here).
"""
from __future__ import annotations

import ctypes
from ctypes import c_double, c_float
from typing import Optional

import torch

from ._abi import *  # noqa: F401,F403 -- _abi.__all__: the constants, EXPORTS / PROTOTYPES, IgemmArgs, LayerNormArgs, HipExtError, library_path, load, operand_dtype
from ._abi import _check, _stream
from ._args import _bytes_of, _check_src_extent, _dev, _like, _maps3, _opt, _same_device, _sized, _u8


class KernelTimer:
    """Optional per-kernel timing with HIP events recorded on the stream the kernels are launched on
    (bench.py uses it to compute the roofline fraction of the dominant kernels inside the timed region)."""

    def __init__(self):
        self.records = {}
        self.active = True     # bench.py brackets the launches of every 4th timed step only: the event records cost ~2 us of stream time each

    def start(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        return ev

    def stop(self, name, ev0, work):
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record(torch.cuda.current_stream())
        self.records.setdefault(name, []).append((ev0, ev1, float(work)))

    def summary(self):
        """name -> dict(launches, ms_total, ms_avg, work_total)  (call after a device synchronize)"""
        out = {}
        for name, recs in self.records.items():
            ms = sum(a.elapsed_time(b) for a, b, _ in recs)
            out[name] = dict(launches=len(recs), ms_total=ms, ms_avg=ms / len(recs), work_total=sum(w for _, _, w in recs))
        return out


_timer: Optional[KernelTimer] = None


def set_timer(t: Optional[KernelTimer]):
    global _timer
    _timer = t


# ------------------------------------------------------------------------------------------------
# thin wrappers (argument meaning = include/ada_hip.h)
# ------------------------------------------------------------------------------------------------
def igemm(*, M, N, K, A, lda, W, k_alg=None, a_mode=A_PLAIN, conv=None, bias=None, gamma=None, res=None, ldr=0,
          res_row_mod=0, res_row_off=0, flags=0, out_f32=None, ldo_f32=0, map_f32=MAP_PLAIN, out_op=None, ldo_op=0,
          map_op=MAP_PLAIN, map_h=0, map_w=0, shuffle_s=0, shuffle_c=0, tail_w=None, tail_b=0.0, tail_act=ACT_NONE, split_seg=0,
          a_dup_seg=0, tap_cols=0, tap_mask=None, a_wrap=0, bias_row_mod=0,
          f8_from=0, f8_mid=0, f8_scales=0):
    op = operand_dtype()
    a = IgemmArgs()
    a.M, a.N, a.K, a.a_mode = M, N, K, a_mode
    a.A, a.lda = _dev(A, "A", op), lda
    if conv is not None:
        a.Ho, a.Wo, a.Hp, a.Wp, a.stride = conv
    a.W = _dev(W, "W", op)
    a.bias = _opt(bias, "bias", torch.float32)
    a.gamma = _opt(gamma, "gamma", torch.float32)
    a.res, a.ldr = _opt(res, "res", torch.float32), ldr
    a.res_row_mod, a.res_row_off, a.flags = res_row_mod, res_row_off, flags
    a.out_f32, a.ldo_f32, a.map_f32 = _opt(out_f32, "out_f32", torch.float32), ldo_f32, map_f32
    a.out_op, a.ldo_op, a.map_op = _opt(out_op, "out_op", op), ldo_op, map_op
    a.map_h, a.map_w, a.shuffle_s, a.shuffle_c = map_h, map_w, shuffle_s, shuffle_c
    a.tail_w, a.tail_b, a.tail_act = _opt(tail_w, "tail_w", torch.float32), tail_b, tail_act
    a.split_seg = split_seg
    a.a_dup_seg = a_dup_seg
    a.a_wrap = a_wrap
    a.bias_row_mod = bias_row_mod
    a.f8_from, a.f8_mid, a.f8_scales = f8_from, f8_mid, f8_scales
    if tap_cols:
        a.tap_cols = tap_cols
        for i, m in enumerate(tap_mask):
            a.tap_mask[i] = int(m)
    if _timer is not None and _timer.active:
        ev = _timer.start()
        _check(load().ada_igemm(ctypes.byref(a), _stream()), "ada_igemm")
        _timer.stop("igemm", ev, 2.0 * M * N * (k_alg if k_alg is not None else K))  # algorithmic FLOP (MAC = 2)
    else:
        _check(load().ada_igemm(ctypes.byref(a), _stream()), "ada_igemm")
    if _tile_log is not None:
        _tile_log.append((M, N, K, load().ada_debug_last_tile()))


def attention(qkv: torch.Tensor, out: torch.Tensor, batch: int, n_tokens: int, heads: int, ld_out: int = 0, split_seg: int = 0):
    """ada_attention_fwd / ada_attention_ex: ``ld_out`` = row stride of ``out`` (0: heads * 64), ``split_seg`` != 0: the split-precision forms of the output row."""
    op = operand_dtype()
    ev = _timer.start() if (_timer is not None and _timer.active) else None
    if ld_out or split_seg:
        _check(load().ada_attention_ex(_dev(qkv, "qkv", op), _dev(out, "out", op), batch, n_tokens, heads, ld_out, split_seg, _stream()), "ada_attention_ex")
    else:
        _check(load().ada_attention_fwd(_dev(qkv, "qkv", op), _dev(out, "out", op), batch, n_tokens, heads, _stream()),
               "ada_attention_fwd")
    if ev is not None:
        _timer.stop("attention", ev, 4.0 * batch * heads * 64 * float(n_tokens) ** 2)  # QK^T + PV, MAC = 2


def layernorm(inp, ld_in, rows_out, dim, weight, bias, eps, *, group_in=0, skip=0, out_op=None, ld_op=0, map_op=MAP_PLAIN,
              map_h=0, map_w=0, relu=False, out_f32=None, ld_f32=0, split_seg=0, weight2=None, bias2=None, out2_op=None, ld2_op=0,
              out2_group=0, out2_skip=0, split_seg2=0, unshuffle_s=0, tap_bias=None, identity=False):
    """ada_layernorm_ex (include/ada_hip.h): LayerNorm rows -> op-typed / fp32 output; optionally a second op-typed output with its own gain /
    bias (out2_*), optionally reading a sub-pixel convolution's [coarse pixel, s*s*dim] output in fine-pixel order (unshuffle_s, tap_bias)."""
    op = operand_dtype()
    a = LayerNormArgs()
    a.in_, a.ld_in, a.rows_out, a.dim, a.group_in, a.skip = _dev(inp, "in", torch.float32), ld_in, rows_out, dim, group_in, skip
    a.weight, a.bias, a.eps = _opt(weight, "weight", torch.float32), _opt(bias, "bias", torch.float32), eps
    a.identity = int(identity)
    a.out_op, a.ld_op, a.map_op, a.map_h, a.map_w, a.relu = _opt(out_op, "out_op", op), ld_op, map_op, map_h, map_w, int(relu)
    a.out_f32, a.ld_f32, a.split_seg = _opt(out_f32, "out_f32", torch.float32), ld_f32, split_seg
    a.weight2, a.bias2 = _opt(weight2, "weight2", torch.float32), _opt(bias2, "bias2", torch.float32)
    a.out2_op, a.ld2_op, a.out2_group, a.out2_skip, a.split_seg2 = _opt(out2_op, "out2_op", op), ld2_op, out2_group, out2_skip, split_seg2
    a.unshuffle_s, a.tap_bias = unshuffle_s, _opt(tap_bias, "tap_bias", torch.float32)
    _check(load().ada_layernorm_ex(ctypes.byref(a), _stream()), "ada_layernorm_ex")


def patchify(x, guide, batch, cg, height, width, mean, inv_std, out, ld, split=False):
    op = operand_dtype()
    if mean is not None:
        m = (c_float * 3)(*mean)
        s = (c_float * 3)(*inv_std)
    else:
        m = s = None
    _check(load().ada_patchify(_dev(x, "x", torch.float32), _opt(guide, "guide", torch.float32), batch, cg, height, width,
                               m, s, _dev(out, "out", op), ld, int(split), _stream()), "ada_patchify")


def pos_embed_resize(pos, sq, dim, ph, pw, scale_h, scale_w, out):
    """pos fp32 [1 + sq*sq, dim] -> out fp32 [1 + ph*pw, dim] (ada_pos_embed_resize: bicubic, ATen semantics)."""
    _check(load().ada_pos_embed_resize(_dev(pos, "pos", torch.float32), sq, dim, ph, pw, float(scale_h), float(scale_w),
                                       _dev(out, "out", torch.float32), _stream()), "ada_pos_embed_resize")


def write_cls(tokens, batch, n_tokens, dim, cls, pos0):
    _check(load().ada_write_cls(_dev(tokens, "tokens", torch.float32), batch, n_tokens, dim,
                                _dev(cls, "cls", torch.float32), _dev(pos0, "pos0", torch.float32), _stream()), "ada_write_cls")


def bilinear(inp, ld_in, batch, hi, wi, ho, wo, channels, *, add=None, ld_add=0, out_f32=None, ld_f32=0, out_op=None,
             ld_op=0, map_op=MAP_PLAIN, relu=False, split_seg=0):
    op = operand_dtype()
    _check(load().ada_bilinear_fwd(_dev(inp, "in", torch.float32), ld_in, batch, hi, wi, ho, wo, channels,
                                   _opt(add, "add", torch.float32), ld_add, _opt(out_f32, "out_f32", torch.float32), ld_f32,
                                   _opt(out_op, "out_op", op), ld_op, map_op, int(relu), split_seg, _stream()), "ada_bilinear_fwd")


def dpt_tail(inp, ld_in, batch, hi, wi, ho, wo, cp, w, bias, tail_w, tail_b, tail_act, out):
    """Fused bilinear resize + output_conv2 (3x3 -> ReLU -> 1x1 -> activation), ada_dpt_tail_fwd."""
    op = operand_dtype()
    ev = _timer.start() if (_timer is not None and _timer.active) else None
    _check(load().ada_dpt_tail_fwd(_dev(inp, "in", torch.float32), ld_in, batch, hi, wi, ho, wo, cp, _dev(w, "w", op),
                                   _dev(bias, "bias", torch.float32), _dev(tail_w, "tail_w", torch.float32), tail_b, tail_act,
                                   _dev(out, "out", torch.float32), _stream()), "ada_dpt_tail_fwd")
    if ev is not None:
        _timer.stop("dpt_tail", ev, 2.0 * batch * ho * wo * 32 * 9 * cp)


def tapsum_resize(inp, ld_in, batch, hi, wi, ho, wo, channels, bias, out, ld_out):
    """conv3x3 of an align-corners up-sampling from the nine coarse tap maps (ada_tapsum_resize_fwd)."""
    ev = _timer.start() if (_timer is not None and _timer.active) else None
    if inp.dtype not in (torch.float32, operand_dtype()):
        raise HipExtError(f"tapsum_resize: tap maps must be fp32 or {operand_dtype()}, got {inp.dtype}")
    code = DT_F32 if inp.dtype == torch.float32 else (DT_F16 if inp.dtype == torch.float16 else DT_BF16)
    _check(load().ada_tapsum_resize_fwd(_dev(inp, "in"), code, ld_in, batch, hi, wi, ho, wo, channels, _opt(bias, "bias", torch.float32),
                                        _dev(out, "out", torch.float32), ld_out, _stream()), "ada_tapsum_resize_fwd")
    if ev is not None:
        _timer.stop("tapsum_resize", ev, 2.0 * 36 * batch * ho * wo * channels)


def minmax(inp, minmax_out):
    """inp: fp32 [B, ...] contiguous -> minmax_out fp32 [B, 2]."""
    B = inp.shape[0]
    pi, pm = _dev(inp, "in", torch.float32), _dev(minmax_out, "minmax", torch.float32)
    _same_device("minmax", "in", inp, minmax=minmax_out)
    _check(load().ada_minmax_fwd(pi, B, inp.numel() // B, pm, _stream()), "ada_minmax_fwd")


def depth_stats(inp, sums, act=ACT_SIGMOID):
    """inp: fp32 [B, ...] contiguous depth maps of a head that ends in `act` -> sums fp32 [B, chunks, 2], per chunk (sum s, sum s (1 - s)) for a sigmoid,
    (sum out, number of positive outputs) for a ReLU, (sum |out|, number of outputs) for none (ada_depth_stats_fwd)."""
    B = inp.shape[0]
    _check(load().ada_depth_stats_fwd(_dev(inp, "in", torch.float32), B, inp.numel() // B, sums.shape[1], int(act), _dev(sums, "sums", torch.float32), _stream()),
           "ada_depth_stats_fwd")


def token_diversity(tap, ld, batch, rows_per_image, dim, sums):
    """tap: operand-typed [batch * rows_per_image, ld] -> sums fp32 [batch, ceil(dim / 64), 2] = per column chunk (sum Var_rows, sum E_rows[t^2]) (ada_token_diversity_fwd)."""
    _check(load().ada_token_diversity_fwd(_dev(tap, "tap", operand_dtype()), ld, batch, rows_per_image, dim, _dev(sums, "sums", torch.float32), _stream()),
           "ada_token_diversity_fwd")


def ladder_select(stat_sums, stat_div, stat_in, thr, thr3, div, div_in, has2, has3, has_r, out, src2, src3, rung, ratio, counts):
    """The precision ladder's decision and paste on the device (ada_ladder_select_fwd; the rule is hip_ext.ladder.ladder_decide with ran = 1, fed by
    hip_ext.ladder.stats_from_host's arithmetic).  stat_sums fp32 [B, chunks, 2]; stat_div / stat_in fp32 [B, G, 2] or None; thresholds as Python floats
    (inf = none); out fp32 [B, ...] contiguous, updated in place; src2 / src3 fp32 of out's shape or None; rung int32 [B], ratio float64 [B] (overwritten),
    counts int64 [4] (added to: calls, images on rung >= 2, on rung 3, unserved).  No host read, no allocation: capturable."""
    B = out.shape[0]
    n = out.numel() // max(B, 1)

    def block(t, name):
        if t is None:
            return None, 0
        if t.dim() != 3 or t.shape[0] != B or t.shape[2] != 2 or not t.is_contiguous():
            raise HipExtError(f"ladder_select: {name} must be a contiguous [B={B}, n, 2] tensor, got {tuple(t.shape)}")
        return _dev(t, name, torch.float32), t.shape[1]

    def rows(t, name):
        if t is None:
            return None
        if t.numel() != out.numel() or not t.is_contiguous():
            raise HipExtError(f"ladder_select: {name} must be contiguous and as large as out ({out.numel()} elements), got {t.numel()}")
        return _dev(t, name, torch.float32)
    if not out.is_contiguous() or B < 1 or n < 1:
        raise HipExtError(f"ladder_select: out must be a non-empty contiguous [B, ...] tensor, got {tuple(out.shape)}")
    for t, name, k in ((rung, "rung", B), (ratio, "ratio", B), (counts, "counts", 4)):
        if t.numel() != k or not t.is_contiguous():
            raise HipExtError(f"ladder_select: {name} must hold {k} contiguous elements, got {tuple(t.shape)}")
    if stat_sums is None and has_r:
        raise HipExtError("ladder_select: has_r without stat_sums")
    (p_sums, chunks), (p_div, groups), (p_in, groups_in) = block(stat_sums, "stat_sums"), block(stat_div, "stat_div"), block(stat_in, "stat_in")
    _check(load().ada_ladder_select_fwd(p_sums, chunks, p_div, groups, p_in, groups_in, B, float(thr), float(thr3), float(div), float(div_in),
                                        int(bool(has2)), int(bool(has3)), int(bool(has_r)), _dev(out, "out", torch.float32), rows(src2, "src2"), rows(src3, "src3"), n,
                                        _dev(rung, "rung", torch.int32), _dev(ratio, "ratio", torch.float64), _dev(counts, "counts", torch.int64), _stream()),
           "ada_ladder_select_fwd")


def normalize(inp, minmax_in, norm=None, obs=None):
    B = inp.shape[0]
    pi, pm, pn, po = _dev(inp, "in", torch.float32), _dev(minmax_in, "minmax", torch.float32), _opt(norm, "norm", torch.float32), _opt(obs, "obs", torch.float32)
    _same_device("normalize", "in", inp, minmax=minmax_in, norm=norm, obs=obs)
    _check(load().ada_normalize_fwd(pi, pm, B, inp.numel() // B, pn, po, _stream()), "ada_normalize_fwd")


def blend(amodal, base, mask, out):
    B, H, W = amodal.shape[0], amodal.shape[-2], amodal.shape[-1]
    pa, pb, pm, po = _dev(amodal, "amodal", torch.float32), _dev(base, "base", torch.float32), _dev(mask, "mask", torch.float32), _dev(out, "out", torch.float32)
    _same_device("blend", "amodal", amodal, base=base, mask=mask, out=out)
    _check(load().ada_blend_fwd(pa, pb, pm, B, H, W, po, _stream()), "ada_blend_fwd")


def blend_ex(amodal, base, mask, out, scale_shift=None):
    """blend with an optional device fp32 [B, 2] (scale, shift): the pasted value is amodal * scale + shift (ada_blend_ex)."""
    B, H, W = amodal.shape[0], amodal.shape[-2], amodal.shape[-1]
    if scale_shift is not None and (tuple(scale_shift.shape) != (B, 2) or not scale_shift.is_contiguous()):
        raise HipExtError(f"blend_ex: scale_shift must be contiguous [{B}, 2], got {tuple(scale_shift.shape)}")
    pa, pb, pm, po = _dev(amodal, "amodal", torch.float32), _dev(base, "base", torch.float32), _dev(mask, "mask", torch.float32), _dev(out, "out", torch.float32)
    ps = _opt(scale_shift, "scale_shift", torch.float32)
    _same_device("blend_ex", "amodal", amodal, base=base, mask=mask, scale_shift=scale_shift, out=out)
    _check(load().ada_blend_ex(pa, pb, pm, ps, B, H, W, po, _stream()), "ada_blend_ex")


def tile_blend(tiles, origin_y, origin_x, height, width, ramp, out):
    """tiles fp32 [B, T, th, tw]; origin_y / origin_x int32 [T] on the device; out fp32 [B, height, width] (ada_tile_blend_fwd)."""
    B, T, th, tw = tiles.shape
    pt, py, px, po = _dev(tiles, "tiles", torch.float32), _dev(origin_y, "origin_y", torch.int32), _dev(origin_x, "origin_x", torch.int32), _dev(out, "out", torch.float32)
    _same_device("tile_blend", "tiles", tiles, origin_y=origin_y, origin_x=origin_x, out=out)
    _check(load().ada_tile_blend_fwd(pt, B, T, th, tw, py, px, height, width, ramp, po, _stream()), "ada_tile_blend_fwd")


def depth_eval(pred, gt, mask=None, scale_shift=None, clip=None) -> torch.Tensor:
    """Per-image masked evaluation sums, fp64 [B, EVAL_NSUM] (ada_depth_eval_fwd).  pred / gt: fp32 [B, ...]; mask: uint8/bool
    of the same shape or None; scale_shift: fp32 [B, 2] or None; clip: (lo, hi) or None."""
    B = pred.shape[0]
    n = pred[0].numel()
    if gt.shape != pred.shape or (mask is not None and mask.shape != pred.shape):
        raise HipExtError(f"depth_eval: shape mismatch pred {tuple(pred.shape)} gt {tuple(gt.shape)}")
    if mask is not None and mask.dtype == torch.bool and not mask.is_contiguous():
        mask = mask.to(torch.uint8)      # a packed copy: the kernel reads B * n consecutive bytes
    mask = _u8(mask)
    pp, pg, pm, ps = _dev(pred, "pred", torch.float32), _dev(gt, "gt", torch.float32), _opt(mask, "mask", torch.uint8), _opt(scale_shift, "scale_shift", torch.float32)
    _same_device("depth_eval", "pred", pred, gt=gt, mask=mask, scale_shift=scale_shift)
    sums = torch.empty(B, EVAL_NSUM, dtype=torch.float64, device=pred.device)
    lo, hi = (float(clip[0]), float(clip[1])) if clip is not None else (0.0, 0.0)
    _check(load().ada_depth_eval_fwd(pp, pg, pm, B, n, ps, lo, hi, sums.data_ptr(), _stream()), "ada_depth_eval_fwd")
    return sums


def protocol_workspace_bytes(batch: int, h: int, w: int) -> int:
    """Bytes of workspace ada_protocol_fit_fwd / ada_protocol_eval_fwd ask for (include/ada_hip.h)."""
    return batch * ((h * w + PROTOCOL_CHUNK - 1) // PROTOCOL_CHUNK) * PROTOCOL_WS_DOUBLES * 8


def _protocol_maps(who, pred, maps):
    """pred fp32 [B, hp, wp]; every (name, tensor, dtype, optional) of ``maps`` [B, h, w] with one (h, w), contiguous, on pred's device (bool masks are
    viewed as uint8).  Returns (B, hp, wp, h, w, device pointers in the order of ``maps``)."""
    B, hp, wp = _maps3(who, pred, "pred")
    shape, ptrs = None, []
    for name, t, dtype, optional in maps:
        if t is None and optional:
            ptrs.append(None)
            continue
        if dtype == torch.uint8:
            t = _u8(t)
        ptrs.append(_dev(t, name, dtype))
        if t.dim() != 3 or not t.is_contiguous() or t.shape[0] != B or t.device != pred.device:
            raise HipExtError(f"{who}: {name} must be a contiguous [{B}, h, w] tensor on {pred.device}, got {tuple(t.shape)} on {t.device}")
        shape = shape or tuple(t.shape)
        if tuple(t.shape) != shape:
            raise HipExtError(f"{who}: {name} is {tuple(t.shape)}, the other maps are {shape}")
    return B, hp, wp, shape[1], shape[2], ptrs


def protocol_fit(pred, observation, visible, whole, workspace=None) -> torch.Tensor:
    """Fit rows fp64 [B, FIT_NCOL] of the prediction (fp32 [B, hp, wp], gathered to the maps' size by ATen's nearest rule) onto ``observation`` (fp32
    [B, h, w]) over ``visible`` (uint8 / bool [B, h, w]), with the pixel counts of ``visible`` and ``whole`` (ada_protocol_fit_fwd).  ``workspace``:
    any contiguous device tensor of at least protocol_workspace_bytes(B, h, w) bytes, allocated when None."""
    B, hp, wp, h, w, (po, pv, pw) = _protocol_maps("protocol_fit", pred, (("observation", observation, torch.float32, False),
                                                                           ("visible", visible, torch.uint8, False), ("whole", whole, torch.uint8, False)))
    ws, ws_bytes = _bytes_of("protocol_fit", workspace, protocol_workspace_bytes(B, h, w), pred.device)
    fit = torch.empty(B, FIT_NCOL, dtype=torch.float64, device=pred.device)
    _check(load().ada_protocol_fit_fwd(pred.data_ptr(), hp, wp, po, pv, pw, B, h, w, fit.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "ada_protocol_fit_fwd")
    return fit


def protocol_eval(pred, gt, region, valid, fit, eps=1e-5, workspace=None) -> torch.Tensor:
    """fp64 [B, 2, EVAL_NSUM]: the EVAL_* sums over region != 0 && valid != 0 (``valid`` None: every pixel) of gt + eps against pred + eps (row 0)
    and against pred * scale + shift + eps with the fit rows' scale / shift (row 1) (ada_protocol_eval_fwd).  Shapes and workspace as protocol_fit."""
    B, hp, wp, h, w, (pg, pr, pv) = _protocol_maps("protocol_eval", pred, (("gt", gt, torch.float32, False), ("region", region, torch.uint8, False),
                                                                            ("valid", valid, torch.uint8, True)))
    if not isinstance(fit, torch.Tensor) or tuple(fit.shape) != (B, FIT_NCOL) or not fit.is_contiguous() or fit.device != pred.device:
        raise HipExtError(f"protocol_eval: fit must be a contiguous [{B}, {FIT_NCOL}] tensor on {pred.device}, got {tuple(getattr(fit, 'shape', ()))}")
    ws, ws_bytes = _bytes_of("protocol_eval", workspace, protocol_workspace_bytes(B, h, w), pred.device)
    sums = torch.empty(B, 2, EVAL_NSUM, dtype=torch.float64, device=pred.device)
    _check(load().ada_protocol_eval_fwd(pred.data_ptr(), hp, wp, pg, pr, pv, _dev(fit, "fit", torch.float64), float(eps), B, h, w, sums.data_ptr(), ws.data_ptr(),
                                        ws_bytes, _stream()), "ada_protocol_eval_fwd")
    return sums


def image_prep(src, batch, hi, wi, channels, row_pitch, image_stride, ho, wo, mean, std, out):
    """uint8 BGR(A) HWC images (rows ``row_pitch`` bytes apart, images ``image_stride`` bytes apart; ``src`` points at pixel (0, 0) of image 0) ->
    out fp32 [batch, 3, ho, wo]: RGB / 255, cv2 INTER_CUBIC resize, (v - mean) / std (ada_image_prep_fwd)."""
    m = (c_float * 3)(*mean)
    sd = (c_float * 3)(*std)
    ps, po = _dev(src, "src", torch.uint8), _dev(out, "out", torch.float32)
    _same_device("image_prep", "src", src, out=out)
    _check(load().ada_image_prep_fwd(ps, batch, hi, wi, channels, row_pitch, image_stride, ho, wo, m, sd, po, _stream()), "ada_image_prep_fwd")


def depth_resize(inp, out):
    """inp fp32 [B, hi, wi] -> out fp32 [B, ho, wo], both contiguous: bilinear, align_corners=True, ATen's arithmetic (ada_depth_resize_fwd)."""
    if not (inp.is_contiguous() and out.is_contiguous()) or inp.dim() != 3 or out.dim() != 3 or inp.shape[0] != out.shape[0]:
        raise HipExtError(f"depth_resize: contiguous [B, H, W] tensors required, got {tuple(inp.shape)} -> {tuple(out.shape)}")
    B, hi, wi = inp.shape
    pi, po = _dev(inp, "in", torch.float32), _dev(out, "out", torch.float32)
    _same_device("depth_resize", "in", inp, out=out)
    _check(load().ada_depth_resize_fwd(pi, B, hi, wi, out.shape[1], out.shape[2], po, _stream()), "ada_depth_resize_fwd")


def photo_prep(src, hi, wi, channels, row_pitch, ho, wo, raw_out=None, near_out=None):
    """One uint8 BGR(A) HWC photo (rows ``row_pitch`` bytes apart) -> raw_out / near_out fp32 [3, ho, wo] (either may be None), channel order kept:
    cv2's 8-bit INTER_LINEAR resize / 255 and ATen's nearest resize / 255 (ada_photo_prep_fwd)."""
    for name, t in (("raw_out", raw_out), ("near_out", near_out)):
        if t is not None and (t.numel() != 3 * ho * wo or not t.is_contiguous()):
            raise HipExtError(f"photo_prep: {name} must be contiguous with 3 x {ho} x {wo} elements, got {tuple(t.shape)}")
    _check_src_extent("photo_prep", src, (hi - 1) * row_pitch + wi * channels)
    ps, pr, pn = _dev(src, "src", torch.uint8), _opt(raw_out, "raw_out", torch.float32), _opt(near_out, "near_out", torch.float32)
    _same_device("photo_prep", "src", src, raw_out=raw_out, near_out=near_out)
    _check(load().ada_photo_prep_fwd(ps, hi, wi, channels, row_pitch, ho, wo, pr, pn, _stream()), "ada_photo_prep_fwd")


def mask_prep(src, batch, hi, wi, row_pitch, image_stride, ho, wo, out01, out_pm1=None):
    """uint8 masks [batch][hi][wi] (non-zero = inside) -> out01 fp32 0/1 [batch, 1, ho, wo] and optionally out_pm1 = 2 m - 1, ATen's nearest rule
    (ada_mask_prep_fwd)."""
    for name, t in (("out01", out01), ("out_pm1", out_pm1)):
        if t is not None and (t.numel() != batch * ho * wo or not t.is_contiguous()):
            raise HipExtError(f"mask_prep: {name} must be contiguous with {batch} x {ho} x {wo} elements, got {tuple(t.shape)}")
    _check_src_extent("mask_prep", src, (batch - 1) * image_stride + (hi - 1) * row_pitch + wi)
    ps, p01, pm1 = _dev(src, "src", torch.uint8), _dev(out01, "out01", torch.float32), _opt(out_pm1, "out_pm1", torch.float32)
    _same_device("mask_prep", "src", src, out01=out01, out_pm1=out_pm1)
    _check(load().ada_mask_prep_fwd(ps, batch, hi, wi, row_pitch, image_stride, ho, wo, p01, pm1, _stream()), "ada_mask_prep_fwd")


def nearest_resize(inp, out):
    """inp fp32 [B, hi, wi] -> out fp32 [B, ho, wo], both contiguous: cv2.resize(INTER_NEAREST)'s rule (ada_nearest_resize_fwd)."""
    if not (inp.is_contiguous() and out.is_contiguous()) or inp.dim() != 3 or out.dim() != 3 or inp.shape[0] != out.shape[0]:
        raise HipExtError(f"nearest_resize: contiguous [B, H, W] tensors required, got {tuple(inp.shape)} -> {tuple(out.shape)}")
    B, hi, wi = inp.shape
    pi, po = _dev(inp, "in", torch.float32), _dev(out, "out", torch.float32)
    _same_device("nearest_resize", "in", inp, out=out)
    _check(load().ada_nearest_resize_fwd(pi, B, hi, wi, out.shape[1], out.shape[2], po, _stream()), "ada_nearest_resize_fwd")


def depth_render(depth, lut, ho, wo, out=None, out_u16=None, *, minmax=None, vmin=0.0, vmax=1.0, mask=None, thickness=2, outline_rgb=0,
                 alpha=0.0, bgr=False):
    """depth fp32 [B, hi, wi] -> out uint8 [B, ho, wo, 3] and / or out_u16 uint16 [B, ho, wo] (ada_depth_render_fwd): (d - lo) / span clipped, the
    256-entry colour table ``lut`` (uint8 [256, 3], R, G, B), with ``mask`` (fp32 [B, hi, wi]) the overlay and the outline of highlight_target, the
    cv2 nearest resize to ho x wo, B, G, R bytes with ``bgr``.  lo / span come from ``minmax`` (device fp32 [B, 2]) when given, else from vmin /
    vmax.  ``outline_rgb`` is 0xRRGGBB.  Every tensor is contiguous and on one device; the output buffers may be larger than the sizes say."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3 or not depth.is_contiguous():
        raise HipExtError(f"depth_render: depth must be a contiguous [B, H, W] tensor, got {tuple(getattr(depth, 'shape', ()))}")
    B, hi, wi = depth.shape
    n = B * ho * wo
    for name, t, need in (("lut", lut, 768), ("mask", mask, depth.numel()), ("minmax", minmax, 2 * B), ("out", out, 3 * n), ("out_u16", out_u16, n)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_contiguous() or t.numel() < need:
            raise HipExtError(f"depth_render: {name} must be a contiguous tensor of at least {need} elements, got {tuple(getattr(t, 'shape', ()))}")
    _same_device("depth_render", "depth", depth, lut=lut, mask=mask, minmax=minmax, out=out, out_u16=out_u16)
    if mask is not None and mask.shape != depth.shape:
        raise HipExtError(f"depth_render: mask {tuple(mask.shape)} does not match depth {tuple(depth.shape)}")
    _check(load().ada_depth_render_fwd(_dev(depth, "depth", torch.float32), B, hi, wi, _opt(minmax, "minmax", torch.float32), float(vmin), float(vmax),
                                       _dev(lut, "lut", torch.uint8), _opt(mask, "mask", torch.float32), int(thickness), int(outline_rgb), float(alpha),
                                       int(ho), int(wo), int(bool(bgr)), _opt(out, "out", torch.uint8), _opt(out_u16, "out_u16", torch.uint16), _stream()),
           "ada_depth_render_fwd")


def pil_resize_u8(src, batch, hi, wi, channels, row_pitch, image_stride, ho, wo, filter=PIL_BICUBIC, tables_x=None, tables_y=None, tmp=None,
                  out_u8=None, out_f32=None, out_mask=None):
    """uint8 HWC images (1 or 3 channels; rows ``row_pitch`` bytes apart, images ``image_stride`` bytes apart) -> Pillow's Image.resize bytes
    ``out_u8`` [batch, ho, wo, channels], ``out_f32`` = bytes / 255 planar [batch, channels, ho, wo], ``out_mask`` uint8 = bytes > 0 [batch, ho, wo]
    (ada_pil_resize_u8_fwd).  ``tables_x`` / ``tables_y``: (bounds, kk, ksize) with device int32 tensors per resized axis for PIL_BICUBIC (None for an
    axis that keeps its size); ``tmp``: uint8 workspace of batch * hi * wo * channels bytes when both axes are resized."""
    n = batch * ho * wo
    for name, t, need in (("out_u8", out_u8, n * channels), ("out_f32", out_f32, n * channels), ("out_mask", out_mask, n)):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_contiguous() or t.numel() != need):
            raise HipExtError(f"pil_resize_u8: {name} must be a contiguous tensor of {need} elements, got {tuple(getattr(t, 'shape', ()))}")
    _check_src_extent("pil_resize_u8", src, (batch - 1) * image_stride + (hi - 1) * row_pitch + wi * channels)
    ptrs, others = [], dict(tmp=tmp, out_u8=out_u8, out_f32=out_f32, out_mask=out_mask)
    for axis, tab, n_out in (("x", tables_x, wo), ("y", tables_y, ho)):
        if tab is None:
            ptrs += [None, None, 0]
            continue
        bounds, kk, ksize = tab
        if bounds.numel() != 2 * n_out or kk.numel() != n_out * ksize or not (bounds.is_contiguous() and kk.is_contiguous()):
            raise HipExtError(f"pil_resize_u8: tables_{axis} must be contiguous [{n_out}, 2] and [{n_out}, {ksize}], got {tuple(bounds.shape)} {tuple(kk.shape)}")
        ptrs += [_dev(bounds, f"bounds_{axis}", torch.int32), _dev(kk, f"kk_{axis}", torch.int32), int(ksize)]
        others.update({f"bounds_{axis}": bounds, f"kk_{axis}": kk})
    ps, pt, pu = _dev(src, "src", torch.uint8), _opt(tmp, "tmp", torch.uint8), _opt(out_u8, "out_u8", torch.uint8)
    pf, pm = _opt(out_f32, "out_f32", torch.float32), _opt(out_mask, "out_mask", torch.uint8)
    _same_device("pil_resize_u8", "src", src, **others)
    _check(load().ada_pil_resize_u8_fwd(ps, batch, hi, wi, channels, row_pitch, image_stride, ho, wo, int(filter), *ptrs, pt, tmp.numel() if tmp is not None else 0,
                                        pu, pf, pm, _stream()), "ada_pil_resize_u8_fwd")


def label_combine(whole, occ, whole_mask, scale_shift, out_u16, out_f32=None, out_of_range=None, overflow=LABEL_WRAP):
    """whole, occ fp32 [P, h, w], whole_mask uint8 [P, h, w], scale_shift fp32 [P, 2] -> out_u16 uint16 [P, ho, wo] (Pillow's NEAREST gather of the
    quantised paste), optionally out_f32 fp32 [P, h, w] (the paste) and out_of_range int32 [P, ho] (ada_label_combine_fwd).  All contiguous, one device."""
    if not isinstance(whole, torch.Tensor) or whole.dim() != 3 or not isinstance(out_u16, torch.Tensor) or out_u16.dim() != 3 or out_u16.shape[0] != whole.shape[0]:
        raise HipExtError(f"label_combine: whole [P, h, w] and out_u16 [P, ho, wo] required, got {tuple(getattr(whole, 'shape', ()))} {tuple(getattr(out_u16, 'shape', ()))}")
    P, h, w = whole.shape
    ho, wo = out_u16.shape[1:]
    for name, t, shape in (("whole", whole, (P, h, w)), ("occ", occ, (P, h, w)), ("whole_mask", whole_mask, (P, h, w)), ("scale_shift", scale_shift, (P, 2)),
                           ("out_u16", out_u16, (P, ho, wo)), ("out_f32", out_f32, (P, h, w)), ("out_of_range", out_of_range, (P, ho))):
        if t is None and name in ("out_f32", "out_of_range"):
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or not t.is_contiguous():
            raise HipExtError(f"label_combine: {name} must be a contiguous {shape} tensor, got {tuple(getattr(t, 'shape', ()))}")
    _same_device("label_combine", "whole", whole, occ=occ, whole_mask=whole_mask, scale_shift=scale_shift, out_u16=out_u16, out_f32=out_f32, out_of_range=out_of_range)
    _check(load().ada_label_combine_fwd(_dev(whole, "whole", torch.float32), _dev(occ, "occ", torch.float32), _dev(whole_mask, "whole_mask", torch.uint8),
                                        _dev(scale_shift, "scale_shift", torch.float32), P, h, w, ho, wo, int(overflow), _dev(out_u16, "out_u16", torch.uint16),
                                        _opt(out_f32, "out_f32", torch.float32), _opt(out_of_range, "out_of_range", torch.int32), _stream()),
           "ada_label_combine_fwd")


def mask_label_workspace_bytes(batch: int, h: int, w: int) -> int:
    """Bytes of workspace ada_mask_label_fwd asks for (include/ada_hip.h)."""
    return 4 * batch * (2 * h * w + (h * w + 1023) // 1024)


def mask_keep_area_workspace_bytes(batch: int, h: int, w: int) -> int:
    """Bytes of workspace ada_mask_keep_area_fwd asks for: the areas of labels 0 .. ceil(h * w / 2) per image."""
    return 4 * batch * (h * w // 2 + 2)


def mask_label(src, batch, h, w, row_pitch, image_stride, connectivity, labels, n_labels, workspace=None):
    """uint8 masks [batch][h][w] (rows ``row_pitch`` bytes, images ``image_stride`` bytes apart; non-zero = inside) -> labels int32 [batch, h, w] (0 =
    background, components 1 .. n in the raster order of their first pixels) and n_labels int32 [batch] (ada_mask_label_fwd).  ``workspace``: any
    contiguous device tensor of at least mask_label_workspace_bytes(batch, h, w) bytes, allocated when None."""
    who = "mask_label"
    _check_src_extent(who, src, (batch - 1) * image_stride + (h - 1) * row_pitch + w)
    pl, pn = _sized(who, "labels", labels, (batch, h, w), torch.int32), _sized(who, "n_labels", n_labels, (batch,), torch.int32)
    ws, ws_bytes = _bytes_of(who, workspace, mask_label_workspace_bytes(batch, h, w), labels.device)
    ps = _dev(src, "src", torch.uint8)
    _same_device(who, "labels", labels, src=src, n_labels=n_labels)
    _check(load().ada_mask_label_fwd(ps, batch, h, w, row_pitch, image_stride, int(connectivity), pl, pn, ws.data_ptr(), ws_bytes, _stream()), "ada_mask_label_fwd")


def mask_stats(labels, max_labels, stats, sums):
    """labels int32 [K, h, w] -> stats int32 [K, max_labels + 1, 5] (LEFT, TOP, WIDTH, HEIGHT, AREA) and sums int64 [K, max_labels + 1, 2] = (sum x, sum y);
    row 0 is the background, rows without pixels are zero, labels above max_labels are ignored (ada_mask_stats_fwd)."""
    K, h, w = _maps3("mask_stats", labels, "labels", torch.int32)
    ps = _sized("mask_stats", "stats", stats, (K, max_labels + 1, 5), torch.int32)
    pm = _sized("mask_stats", "sums", sums, (K, max_labels + 1, 2), torch.int64)
    _same_device("mask_stats", "labels", labels, stats=stats, sums=sums)
    _check(load().ada_mask_stats_fwd(labels.data_ptr(), K, h, w, int(max_labels), ps, pm, _stream()), "ada_mask_stats_fwd")


def mask_keep_area(labels, min_area, out_u8=None, out_f32=None, workspace=None):
    """labels int32 [K, h, w] -> out_u8 uint8 / out_f32 fp32 0 / 1 [K, h, w] = label != 0 and area(label) >= min_area (ada_mask_keep_area_fwd)."""
    who = "mask_keep_area"
    K, h, w = _maps3(who, labels, "labels", torch.int32)
    if out_u8 is None and out_f32 is None:
        raise HipExtError(f"{who}: out_u8 and out_f32 are both None")
    pu = _like(who, "out_u8", out_u8, labels, torch.uint8, optional=True)
    pf = _like(who, "out_f32", out_f32, labels, torch.float32, optional=True)
    ws, ws_bytes = _bytes_of(who, workspace, mask_keep_area_workspace_bytes(K, h, w), labels.device)
    _check(load().ada_mask_keep_area_fwd(labels.data_ptr(), K, h, w, int(min_area), pu, pf, ws.data_ptr(), ws_bytes, _stream()), "ada_mask_keep_area_fwd")


def mask_grid_points(labels, stats, small_component_thresh, grid_step, hit):
    """labels int32 [K, h, w], stats int32 [K, cap + 1, 5] -> hit int32 [K, h, w]: the label at the grid points of the components of at least
    ``small_component_thresh`` pixels, 0 elsewhere (ada_mask_grid_points_fwd)."""
    who = "mask_grid_points"
    K, h, w = _maps3(who, labels, "labels", torch.int32)
    if not isinstance(stats, torch.Tensor) or stats.dim() != 3 or stats.shape[0] != K or stats.shape[1] < 1 or stats.shape[2] != 5 or not stats.is_contiguous():
        raise HipExtError(f"{who}: stats must be a contiguous int32 [{K}, cap + 1, 5] tensor, got {tuple(getattr(stats, 'shape', ()))}")
    ps, ph = _dev(stats, "stats", torch.int32), _like(who, "hit", hit, labels, torch.int32)
    _same_device(who, "labels", labels, stats=stats)
    _check(load().ada_mask_grid_points_fwd(labels.data_ptr(), ps, K, h, w, stats.shape[1] - 1, int(small_component_thresh), int(grid_step), ph, _stream()),
           "ada_mask_grid_points_fwd")


def quantile_workspace_bytes(batch: int) -> int:
    """Bytes of workspace ada_quantile_fwd asks for (include/ada_hip.h)."""
    return batch * QUANTILE_WS_BYTES_PER_IMAGE


def quantile_select(x, q, out, out_f32=None, count=None, valid=None, mode=Q_NUMPY, flags=0, exclude_value=0.0, workspace=None):
    """x fp32 [B, ...] contiguous -> out fp64 [B, len(q)], optionally out_f32 fp32 [B, len(q)] and count int64 [B]: the exact quantiles ``q`` (fractions
    in [0, 1], at most QUANTILE_MAX_Q) of each image's population (ada_quantile_fwd).  ``valid``: uint8 of x's shape or None; ``workspace``: any
    contiguous device tensor of at least quantile_workspace_bytes(B) bytes, allocated when None.  Nothing is read back."""
    who = "quantile_select"
    if not isinstance(x, torch.Tensor) or x.dim() < 1 or not x.is_contiguous() or x.numel() == 0:
        raise HipExtError(f"{who}: x must be a non-empty contiguous fp32 [B, ...] tensor, got {tuple(getattr(x, 'shape', ()))}")
    px = _dev(x, "x", torch.float32)
    B = x.shape[0]
    n = x.numel() // B
    qs = [float(v) for v in q]
    if not 1 <= len(qs) <= QUANTILE_MAX_Q:
        raise HipExtError(f"{who}: {len(qs)} quantiles, 1..{QUANTILE_MAX_Q} per call")
    nq = len(qs)
    po = _sized(who, "out", out, (B, nq), torch.float64)
    pf = None if out_f32 is None else _sized(who, "out_f32", out_f32, (B, nq), torch.float32)
    pc = None if count is None else _sized(who, "count", count, (B,), torch.int64)
    pv = _like(who, "valid", valid, x, torch.uint8, optional=True)
    _same_device(who, "x", x, out=out, out_f32=out_f32, count=count)
    ws, ws_bytes = _bytes_of(who, workspace, quantile_workspace_bytes(B), x.device)
    _check(load().ada_quantile_fwd(px, pv, B, n, (c_double * nq)(*qs), nq, int(mode), int(flags), float(exclude_value), po, pf, pc, ws.data_ptr(), ws_bytes,
                                   _stream()), "ada_quantile_fwd")


def mesh_triangles_workspace_bytes(batch: int, h: int, w: int) -> int:
    """Bytes of workspace ada_mesh_triangles_fwd asks for (include/ada_hip.h)."""
    return 4 * batch * max(1, ((h - 1) * (w - 1) + GEOM_CHUNK - 1) // GEOM_CHUNK)


def mesh_compact_workspace_bytes(batch: int, h: int, w: int) -> int:
    """Bytes of workspace ada_mesh_compact_fwd asks for (include/ada_hip.h)."""
    return 4 * batch * (h * w + (h * w + GEOM_CHUNK - 1) // GEOM_CHUNK)


def _z_rule(inverse):
    return (0, 0.0, 0.0) if inverse is None else (1, float(inverse[0]), float(inverse[1]))


def depth_points(depth, camera, out_f64=None, out_f32=None, valid=None, inverse=None):
    """depth fp32 [B, h, w] -> points [B, h, w, 3] as fp64 and / or fp32 and optionally valid uint8 [B, h, w] (ada_depth_points_fwd).  ``camera``: 21
    host doubles, Kinv row-major, R row-major, t.  ``inverse``: None for z = depth, (a, b) for z = 1 / (a depth + b)."""
    who = "depth_points"
    B, h, w = _maps3(who, depth, "depth")
    cam = [float(v) for v in camera]
    if len(cam) != 21:
        raise HipExtError(f"{who}: camera must hold 21 doubles (Kinv, R, t), got {len(cam)}")
    if out_f64 is None and out_f32 is None:
        raise HipExtError(f"{who}: one of out_f64 / out_f32 is needed")
    p64 = None if out_f64 is None else _sized(who, "out_f64", out_f64, (B, h, w, 3), torch.float64)
    p32 = None if out_f32 is None else _sized(who, "out_f32", out_f32, (B, h, w, 3), torch.float32)
    pv = _like(who, "valid", valid, depth, torch.uint8, optional=True)
    _same_device(who, "depth", depth, out_f64=out_f64, out_f32=out_f32)
    inv, a, b = _z_rule(inverse)
    _check(load().ada_depth_points_fwd(depth.data_ptr(), B, h, w, (c_double * 21)(*cam), inv, a, b, p64, p32, pv, _stream()), "ada_depth_points_fwd")


def mesh_triangles(batch, h, w, triangles, count, mask=None, row_pitch=0, image_stride=0, depth=None, inverse=None, max_ratio=0.0, workspace=None):
    """The kept triangles of create_triangles's candidate list, in its order (ada_mesh_triangles_fwd): triangles int32 [batch, capacity, 3] receives the
    first min(count, capacity) of each image, count int32 [batch] the true number.  ``mask``: uint8, rows ``row_pitch`` bytes and images ``image_stride``
    bytes apart (non-zero = inside) or None; ``depth``: contiguous fp32 [batch, h, w] or None, with ``inverse`` as in depth_points; ``max_ratio`` <= 0: off.
    ``workspace``: any contiguous device tensor of at least mesh_triangles_workspace_bytes(batch, h, w) bytes, allocated when None."""
    who = "mesh_triangles"
    if not isinstance(triangles, torch.Tensor) or triangles.dim() != 3 or triangles.shape[0] != batch or triangles.shape[2] != 3 or not triangles.is_contiguous():
        raise HipExtError(f"{who}: triangles must be a contiguous int32 [{batch}, capacity, 3] tensor, got {tuple(getattr(triangles, 'shape', ()))}")
    pt = _dev(triangles, "triangles", torch.int32)
    pc = _sized(who, "count", count, (batch,), torch.int32)
    pm = None
    if mask is not None:
        pm = _dev(mask, "mask", torch.uint8)
        _check_src_extent(who, mask, (batch - 1) * image_stride + (h - 1) * row_pitch + w)
    pd = None
    if depth is not None:
        if _maps3(who, depth, "depth") != (batch, h, w):
            raise HipExtError(f"{who}: depth must be [{batch}, {h}, {w}], got {tuple(depth.shape)}")
        pd = depth.data_ptr()
    _same_device(who, "triangles", triangles, count=count, mask=mask, depth=depth)
    inv, a, b = _z_rule(inverse)
    ws, ws_bytes = _bytes_of(who, workspace, mesh_triangles_workspace_bytes(batch, h, w), triangles.device)
    _check(load().ada_mesh_triangles_fwd(pm, int(row_pitch), int(image_stride), pd, inv, a, b, float(max_ratio), batch, h, w, pt, triangles.shape[1], pc,
                                         ws.data_ptr(), ws_bytes, _stream()), "ada_mesh_triangles_fwd")


def mesh_compact(triangles, count, h, w, points, points_out, vertex_count, colors=None, colors_out=None, workspace=None):
    """The vertices that the first min(count, capacity) triangles of each image use, in raster order (ada_mesh_compact_fwd): points [B, h * w, 3] (fp32 or
    fp64) -> points_out [B, vertex_capacity, 3], colors uint8 [B, h * w, 3] -> colors_out likewise, vertex_count int32 [B]; triangles int32
    [B, capacity, 3] is rewritten in place to the new numbering.  ``workspace``: at least mesh_compact_workspace_bytes(B, h, w) bytes, allocated when None."""
    who = "mesh_compact"
    if not isinstance(triangles, torch.Tensor) or triangles.dim() != 3 or triangles.shape[2] != 3 or not triangles.is_contiguous():
        raise HipExtError(f"{who}: triangles must be a contiguous int32 [B, capacity, 3] tensor, got {tuple(getattr(triangles, 'shape', ()))}")
    B, cap = triangles.shape[0], triangles.shape[1]
    pt = _dev(triangles, "triangles", torch.int32)
    pc = _sized(who, "count", count, (B,), torch.int32)
    if not isinstance(points, torch.Tensor) or points.dtype not in (torch.float32, torch.float64):
        raise HipExtError(f"{who}: points must be an fp32 or fp64 tensor")
    pp = _sized(who, "points", points, (B, h * w, 3), points.dtype)
    if not isinstance(points_out, torch.Tensor) or points_out.dim() != 3:
        raise HipExtError(f"{who}: points_out must be a [B, vertex_capacity, 3] tensor")
    vcap = points_out.shape[1]
    po = _sized(who, "points_out", points_out, (B, vcap, 3), points.dtype)
    pv = _sized(who, "vertex_count", vertex_count, (B,), torch.int32)
    if (colors is None) != (colors_out is None):
        raise HipExtError(f"{who}: colors and colors_out come together")
    pci = None if colors is None else _sized(who, "colors", colors, (B, h * w, 3), torch.uint8)
    pco = None if colors_out is None else _sized(who, "colors_out", colors_out, (B, vcap, 3), torch.uint8)
    _same_device(who, "triangles", triangles, count=count, points=points, points_out=points_out, vertex_count=vertex_count, colors=colors, colors_out=colors_out)
    ws, ws_bytes = _bytes_of(who, workspace, mesh_compact_workspace_bytes(B, h, w), triangles.device)
    _check(load().ada_mesh_compact_fwd(pt, pc, cap, B, h, w, pp, points.element_size(), pci, po, pco, vcap, pv, ws.data_ptr(), ws_bytes, _stream()),
           "ada_mesh_compact_fwd")


def mesh_raster_workspace_bytes(h: int, w: int, n_triangles: int) -> int:
    """Bytes of workspace ada_mesh_raster_fwd asks for (include/ada_hip.h)."""
    return 8 * (h * w + (h * w) % 2) + 16 + 4 * n_triangles


def mesh_project(points, camera, x, y, w, pose=False):
    """The rasteriser's vertex stage (ada_mesh_project_fwd): points [V, 3] fp32 or fp64 -> x, y int32 [V] (snapped to 1/256 pixel) and w fp64 [V] = 1 / z,
    0 for an invalid vertex.  ``camera``: 16 host doubles fx, fy, cx, cy, R row-major, t; R and t are applied only with ``pose``."""
    who = "mesh_project"
    if not isinstance(points, torch.Tensor) or points.dtype not in (torch.float32, torch.float64) or points.dim() != 2 or points.shape[1] != 3:
        raise HipExtError(f"{who}: points must be an fp32 or fp64 [V, 3] tensor")
    V = points.shape[0]
    pp = _sized(who, "points", points, (V, 3), points.dtype)
    cam = [float(v) for v in camera]
    if len(cam) != 16:
        raise HipExtError(f"{who}: camera must hold 16 doubles (fx, fy, cx, cy, R, t), got {len(cam)}")
    px, py, pw = _sized(who, "x", x, (V,), torch.int32), _sized(who, "y", y, (V,), torch.int32), _sized(who, "w", w, (V,), torch.float64)
    _same_device(who, "points", points, x=x, y=y, w=w)
    _check(load().ada_mesh_project_fwd(pp, points.element_size(), V, (c_double * 16)(*cam), 1 if pose else 0, px, py, pw, _stream()), "ada_mesh_project_fwd")


def mesh_raster(x, y, w, triangles, h, width, depth, index, colors=None, color=None, mode=RASTER_OUT_Z, inverse=None, fill=0.0, fill_color=(128, 128, 128),
                workspace=None):
    """Clear, rasterise and resolve (ada_mesh_raster_fwd): vertex records x, y int32 [V], w fp64 [V] and triangles int32 [T, 3] -> depth fp32 [h, width],
    index int32 [h, width] and, with colors uint8 [V, 3], color uint8 [h, width, 3].  ``mode``: RASTER_OUT_W / _Z / _NORMALISED, the last with
    ``inverse`` = (a, b).  ``workspace``: at least mesh_raster_workspace_bytes(h, width, T) bytes, 16-byte aligned, allocated when None."""
    who = "mesh_raster"
    if not isinstance(triangles, torch.Tensor) or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise HipExtError(f"{who}: triangles must be an int32 [T, 3] tensor, got {tuple(getattr(triangles, 'shape', ()))}")
    T = triangles.shape[0]
    pt = _sized(who, "triangles", triangles, (T, 3), torch.int32)
    if not isinstance(x, torch.Tensor) or x.dim() != 1:
        raise HipExtError(f"{who}: x must be an int32 [V] tensor")
    V = x.shape[0]
    px, py, pw = _sized(who, "x", x, (V,), torch.int32), _sized(who, "y", y, (V,), torch.int32), _sized(who, "w", w, (V,), torch.float64)
    pd, pi = _sized(who, "depth", depth, (h, width), torch.float32), _sized(who, "index", index, (h, width), torch.int32)
    if color is not None and colors is None:
        raise HipExtError(f"{who}: a color output needs the vertex colors")
    pci = None if colors is None else _sized(who, "colors", colors, (V, 3), torch.uint8)
    pco = None if color is None else _sized(who, "color", color, (h, width, 3), torch.uint8)
    _same_device(who, "depth", depth, y=y, w=w, triangles=triangles, index=index, colors=colors, color=color, x=x)
    a, b = (1.0, 0.0) if inverse is None else (float(inverse[0]), float(inverse[1]))
    rgb = [int(c) for c in fill_color]
    if len(rgb) != 3 or min(rgb) < 0 or max(rgb) > 255:
        raise HipExtError(f"{who}: fill_color must hold three values in 0 .. 255, got {fill_color!r}")
    ws, ws_bytes = _bytes_of(who, workspace, mesh_raster_workspace_bytes(h, width, T), depth.device)
    _check(load().ada_mesh_raster_fwd(px, py, pw, pci, V, pt, T, h, width, int(mode), a, b, float(fill), rgb[0] | rgb[1] << 8 | rgb[2] << 16, pd, pi, pco,
                                      ws.data_ptr(), ws_bytes, _stream()), "ada_mesh_raster_fwd")


def mesh_adaptive_workspace_bytes(h: int, w: int) -> int:
    """Bytes of workspace ada_mesh_adaptive_fwd asks for an h x w map, whatever the batch (ada_mesh_adaptive_workspace_bytes)."""
    n = ctypes.c_int64(0)
    _check(load().ada_mesh_adaptive_workspace_bytes(int(h), int(w), ctypes.byref(n)), "ada_mesh_adaptive_workspace_bytes")
    return n.value


def mesh_adaptive(batch, h, w, depth, triangles, count, mask=None, row_pitch=0, image_stride=0, inverse=None, max_ratio=0.0, max_error=None, error=None,
                  error_ready=False, workspace=None):
    """The error-bounded RTIN mesh of each depth map, rows in heap order (ada_mesh_adaptive_fwd, the contract in include/ada_hip.h): triangles int32
    [batch, capacity, 3] receives the first min(count, capacity) rows of each image, count int32 [batch] the true number.  ``depth``: contiguous fp32
    [batch, h, w], ``mask`` / ``inverse`` / ``max_ratio`` as in mesh_triangles.  ``max_error``: the tolerance on the relative disparity error, finite and
    >= 0, or None for every keepable leaf.  ``error``: optional fp64 [batch, h, w] that receives the error map E; with ``error_ready`` it holds E already (an
    earlier call on the same map, mask, inverse and max_ratio) and the error phase is skipped.  ``workspace``: at least
    mesh_adaptive_workspace_bytes(h, w) bytes, 16-byte aligned, allocated when None."""
    who = "mesh_adaptive"
    if _maps3(who, depth, "depth") != (batch, h, w):
        raise HipExtError(f"{who}: depth must be [{batch}, {h}, {w}], got {tuple(depth.shape)}")
    if not isinstance(triangles, torch.Tensor) or triangles.dim() != 3 or triangles.shape[0] != batch or triangles.shape[2] != 3 or not triangles.is_contiguous():
        raise HipExtError(f"{who}: triangles must be a contiguous int32 [{batch}, capacity, 3] tensor, got {tuple(getattr(triangles, 'shape', ()))}")
    pt = _dev(triangles, "triangles", torch.int32)
    pc = _sized(who, "count", count, (batch,), torch.int32)
    pm = None
    if mask is not None:
        pm = _dev(mask, "mask", torch.uint8)
        _check_src_extent(who, mask, (batch - 1) * image_stride + (h - 1) * row_pitch + w)
    pe = None if error is None else _sized(who, "error", error, (batch, h, w), torch.float64)
    _same_device(who, "depth", depth, triangles=triangles, count=count, mask=mask, error=error)
    inv, a, b = _z_rule(inverse)
    ws, ws_bytes = _bytes_of(who, workspace, mesh_adaptive_workspace_bytes(h, w), depth.device)
    _check(load().ada_mesh_adaptive_fwd(pm, int(row_pitch), int(image_stride), depth.data_ptr(), inv, a, b, float(max_ratio),
                                        0.0 if max_error is None else float(max_error), 1 if max_error is None else 0, batch, h, w, pt, triangles.shape[1], pc,
                                        pe, 1 if error_ready else 0, ws.data_ptr(), ws_bytes, _stream()), "ada_mesh_adaptive_fwd")


def range_map(depth, range32, out, scale=1.0, shift=0.0, clip=None):
    """out = ((depth - lo) / (hi - lo)) * scale + shift per image, clamped to ``clip`` = (lo, hi) when given; (lo, hi) of the map from ``range32``, device
    fp32 [B, 2] (ada_range_map_fwd).  depth, out: contiguous fp32 [B, ...] of one shape."""
    who = "range_map"
    if not isinstance(depth, torch.Tensor) or depth.dim() < 1 or not depth.is_contiguous() or depth.numel() == 0:
        raise HipExtError(f"{who}: depth must be a non-empty contiguous fp32 [B, ...] tensor, got {tuple(getattr(depth, 'shape', ()))}")
    B = depth.shape[0]
    pd = _dev(depth, "depth", torch.float32)
    po = _like(who, "out", out, depth, torch.float32)
    pr = _sized(who, "range32", range32, (B, 2), torch.float32)
    _same_device(who, "depth", depth, range32=range32)
    lo, hi = (float(clip[0]), float(clip[1])) if clip is not None else (0.0, 0.0)
    _check(load().ada_range_map_fwd(pd, pr, B, depth.numel() // B, float(scale), float(shift), int(clip is not None), lo, hi, po, _stream()), "ada_range_map_fwd")


def depth_colorize(value, lut, out, range64=None, vmin=0.0, vmax=1.0, invalid_mask=None, invalid_val=-99.0, background=(128, 128, 128, 255)):
    """value fp32 [B, h, w] -> out uint8 [B, h, w, 4]: the reference's colorize() below its percentiles (ada_depth_colorize_fwd).  The range is
    ``range64`` (device fp64 [B, 2]) when given, else the host numbers vmin / vmax; ``lut`` uint8 [256, 4] R, G, B, A; invalid pixels (``invalid_mask``
    uint8 [B, h, w] non-zero when given, else value == invalid_val) get ``background`` (R, G, B, A bytes).  All contiguous, one device."""
    who = "depth_colorize"
    B, h, w = _maps3(who, value, "value")
    pl = _sized(who, "lut", lut, (256, 4), torch.uint8)
    po = _sized(who, "out", out, (B, h, w, 4), torch.uint8)
    pr = None if range64 is None else _sized(who, "range64", range64, (B, 2), torch.float64)
    pm = _like(who, "invalid_mask", invalid_mask, value, torch.uint8, optional=True)
    _same_device(who, "value", value, lut=lut, out=out, range64=range64)
    r, g, b, a = (int(c) & 0xff for c in background)
    _check(load().ada_depth_colorize_fwd(value.data_ptr(), B, h, w, pr, float(vmin), float(vmax), pl, pm, float(invalid_val), r | (g << 8) | (b << 16) | (a << 24), po,
                                         _stream()), "ada_depth_colorize_fwd")


def canny_hysteresis_workspace_bytes(batch: int, h: int, w: int) -> int:
    """Bytes of workspace ada_canny_hysteresis_fwd asks for (include/ada_hip.h)."""
    hw = h * w
    return 4 * batch * hw + 4 * batch + mask_label_workspace_bytes(batch, h, w) + batch * ((hw // 2 + 2 + 3) // 4 * 4) + (batch * hw + 3) // 4 * 4


def edt_workspace_bytes(batch: int, h: int, w: int) -> int:
    """Bytes of workspace ada_edt_fwd asks for: one int32 per pixel."""
    return 4 * batch * h * w


def edge_sums_workspace_bytes(batch: int, columns: int = 4) -> int:
    """Bytes of workspace ada_edge_metric_fwd (4 columns) / ada_soft_edge_fwd (2 columns) ask for."""
    return 8 * batch * EDGE_SUM_BLOCKS * columns


def canny_front(image, weights, low_threshold, low_masked, pre=CANNY_PRE_NONE, pre_out=None, smoothed=None, isobel=None, jsobel=None, magnitude=None):
    """image fp32 [B, h, w] -> low_masked fp32 [B, h, w]: skimage's Canny detector up to the suppressed magnitude (ada_canny_fwd).  ``weights``: device
    fp64 [2 r + 1], the Gaussian's taps; ``pre``: CANNY_PRE_*; the other maps are optional fp32 stage outputs of image's shape."""
    who = "canny_front"
    B, h, w = _maps3(who, image)
    if not isinstance(weights, torch.Tensor) or weights.dim() != 1 or weights.numel() % 2 != 1 or not weights.is_contiguous() or weights.device != image.device:
        raise HipExtError(f"{who}: weights must be a contiguous fp64 [2 r + 1] tensor on {image.device}, got {tuple(getattr(weights, 'shape', ()))}")
    pw = _dev(weights, "weights", torch.float64)
    outs = [_like(who, n, t, image, torch.float32, optional=n != "low_masked") for n, t in
            (("low_masked", low_masked), ("pre_out", pre_out), ("smoothed", smoothed), ("isobel", isobel), ("jsobel", jsobel), ("magnitude", magnitude))]
    _check(load().ada_canny_fwd(image.data_ptr(), B, h, w, int(pre), pw, weights.numel() // 2, float(low_threshold), *outs, _stream()), "ada_canny_fwd")


def canny_hysteresis(low_masked, high_threshold, edges, workspace=None):
    """low_masked fp32 [B, h, w] -> edges uint8 0 / 1 [B, h, w]: the 8-connected components of low_masked > 0 that reach ``high_threshold``
    (ada_canny_hysteresis_fwd).  ``workspace``: at least canny_hysteresis_workspace_bytes(B, h, w) bytes, allocated when None."""
    who = "canny_hysteresis"
    B, h, w = _maps3(who, low_masked, "low_masked")
    pe = _like(who, "edges", edges, low_masked, torch.uint8)
    ws, ws_bytes = _bytes_of(who, workspace, canny_hysteresis_workspace_bytes(B, h, w), low_masked.device)
    _check(load().ada_canny_hysteresis_fwd(low_masked.data_ptr(), B, h, w, float(high_threshold), pe, ws.data_ptr(), ws_bytes, _stream()),
           "ada_canny_hysteresis_fwd")


def edt(edges, out, workspace=None):
    """edges uint8 [B, h, w] -> out fp64 [B, h, w]: the exact Euclidean distance to the nearest non-zero pixel, +inf where the image has none
    (ada_edt_fwd).  ``workspace``: at least edt_workspace_bytes(B, h, w) bytes, allocated when None."""
    who = "edt"
    B, h, w = _maps3(who, edges, "edges", torch.uint8)
    po = _like(who, "out", out, edges, torch.float64)
    ws, ws_bytes = _bytes_of(who, workspace, edt_workspace_bytes(B, h, w), edges.device)
    _check(load().ada_edt_fwd(edges.data_ptr(), B, h, w, po, ws.data_ptr(), ws_bytes, _stream()), "ada_edt_fwd")


def edge_metric_sums(pred_edges, gt_edges, valid, d_target, d_pred, th_acc, sums, workspace=None):
    """sums fp64 [B, 4] (EDGE_*): count and sum of d_target over pred_edges & valid & (d_target < th_acc), count and sum of d_pred over gt_edges & valid
    (ada_edge_metric_fwd).  Edge maps and ``valid`` (or None) uint8 [B, h, w], distance maps fp64 [B, h, w]."""
    who = "edge_metric_sums"
    B, h, w = _maps3(who, pred_edges, "pred_edges", torch.uint8)
    pg = _like(who, "gt_edges", gt_edges, pred_edges, torch.uint8)
    pv = _like(who, "valid", valid, pred_edges, torch.uint8, optional=True)
    pt, pp = _like(who, "d_target", d_target, pred_edges, torch.float64), _like(who, "d_pred", d_pred, pred_edges, torch.float64)
    ps = _sized(who, "sums", sums, (B, 4), torch.float64)
    _same_device(who, "pred_edges", pred_edges, sums=sums)
    ws, ws_bytes = _bytes_of(who, workspace, edge_sums_workspace_bytes(B, 4), pred_edges.device)
    _check(load().ada_edge_metric_fwd(pred_edges.data_ptr(), pg, pv, pt, pp, B, h, w, float(th_acc), ps, ws.data_ptr(), ws_bytes, _stream()),
           "ada_edge_metric_fwd")


def soft_edge(pred, gt, valid, radius, sums, workspace=None):
    """sums fp64 [B, 2]: the number of valid pixels and the sum over them of min over the (2 radius + 1)^2 shifts of |shift(gt) - pred| (ada_soft_edge_fwd).
    pred, gt fp32 [B, h, w]; ``valid`` uint8 [B, h, w] or None."""
    who = "soft_edge"
    B, h, w = _maps3(who, pred, "pred")
    pg = _like(who, "gt", gt, pred, torch.float32)
    pv = _like(who, "valid", valid, pred, torch.uint8, optional=True)
    ps = _sized(who, "sums", sums, (B, 2), torch.float64)
    _same_device(who, "pred", pred, sums=sums)
    ws, ws_bytes = _bytes_of(who, workspace, edge_sums_workspace_bytes(B, 2), pred.device)
    _check(load().ada_soft_edge_fwd(pred.data_ptr(), pg, pv, B, h, w, int(radius), ps, ws.data_ptr(), ws_bytes, _stream()), "ada_soft_edge_fwd")


def extreme_filter_workspace_bytes(batch: int, h: int, w: int) -> int:
    """Bytes of workspace ada_extreme_filter_fwd asks for: a key and a one-byte count per pixel."""
    return 5 * batch * h * w


def _filter_maps(who, x, valid, out, count):
    """(B, h, w, ADA_DT_* of x, pointers of valid / out / count) of a rank filter's maps: x fp32 or uint8 [B, h, w], out of x's type, all of one shape."""
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.uint8):
        raise HipExtError(f"{who}: x must be an fp32 or uint8 tensor, got {getattr(x, 'dtype', type(x).__name__)}")
    B, h, w = _maps3(who, x, "x", x.dtype)
    return (B, h, w, DT_F32 if x.dtype == torch.float32 else DT_U8, _like(who, "valid", valid, x, torch.uint8, optional=True),
            _like(who, "out", out, x, x.dtype), _like(who, "count", count, x, torch.int32, optional=True))


def rank_filter_fwd(x, kh, kw, rank, border, out, valid=None, fill=0.0, count=None):
    """x fp32 / uint8 [B, h, w] -> out: the rank-th order statistic of the valid samples of every kh x kw window (ada_rank_filter_fwd; kh * kw <=
    FILTER_MAX_WINDOW).  ``rank``: RANK_MIN / RANK_MEDIAN / RANK_MAX or an integer percent 0 .. 100; ``border``: BORDER_*; ``valid``: uint8 [B, h, w] or
    None; ``fill``: the output where no sample votes; ``count``: optional int32 [B, h, w], the number of voting samples."""
    who = "rank_filter_fwd"
    B, h, w, dt, pv, po, pc = _filter_maps(who, x, valid, out, count)
    _check(load().ada_rank_filter_fwd(x.data_ptr(), pv, dt, B, h, w, int(kh), int(kw), int(rank), int(border), float(fill), po, pc, _stream()), "ada_rank_filter_fwd")


def extreme_filter_fwd(x, kh, kw, rank, border, out, valid=None, fill=0.0, count=None, workspace=None):
    """rank_filter_fwd for RANK_MIN / RANK_MAX on the separable kernels (ada_extreme_filter_fwd; kh, kw <= FILTER_MAX_EXTREME).  ``workspace``: at least
    extreme_filter_workspace_bytes(B, h, w) bytes, allocated when None."""
    who = "extreme_filter_fwd"
    B, h, w, dt, pv, po, pc = _filter_maps(who, x, valid, out, count)
    ws, ws_bytes = _bytes_of(who, workspace, extreme_filter_workspace_bytes(B, h, w), x.device)
    _check(load().ada_extreme_filter_fwd(x.data_ptr(), pv, dt, B, h, w, int(kh), int(kw), int(rank), int(border), float(fill), po, pc, ws.data_ptr(), ws_bytes,
                                         _stream()), "ada_extreme_filter_fwd")


def nearest_valid_workspace_bytes(batch: int, h: int, w: int) -> int:
    """Bytes of workspace ada_nearest_valid_fwd asks for (ada_nearest_valid_workspace_bytes): one int32 per pixel."""
    n = ctypes.c_int64(0)
    _check(load().ada_nearest_valid_workspace_bytes(int(batch), int(h), int(w), ctypes.byref(n)), "ada_nearest_valid_workspace_bytes")
    return n.value


def push_pull_workspace_bytes(batch: int, channels: int, h: int, w: int) -> int:
    """Bytes of workspace ada_push_pull_fwd asks for (ada_push_pull_workspace_bytes): the pyramid above level 0, 0 for a 1 x 1 image."""
    n = ctypes.c_int64(0)
    _check(load().ada_push_pull_workspace_bytes(int(batch), int(channels), int(h), int(w), ctypes.byref(n)), "ada_push_pull_workspace_bytes")
    return n.value


def _planes4(who, x, name="x"):
    """Shape of a non-empty contiguous fp32 [B, C, h, w] device tensor."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or not x.is_contiguous() or x.numel() == 0:
        raise HipExtError(f"{who}: {name} must be a non-empty contiguous [B, C, h, w] tensor, got {tuple(getattr(x, 'shape', ()))}")
    _dev(x, name, torch.float32)
    return tuple(x.shape)


def nearest_valid_fwd(valid, index, dist2=None, workspace=None):
    """valid uint8 [B, h, w] -> index int32 [B, h, w]: the flat position of the nearest valid pixel of the same image, ties to the smallest flat position,
    -1 where the image has none (ada_nearest_valid_fwd).  ``dist2``: optional int32 [B, h, w], the exact squared distance (0x7fffffff where the image
    has none).  ``workspace``: at least nearest_valid_workspace_bytes(B, h, w) bytes, allocated when None."""
    who = "nearest_valid_fwd"
    B, h, w = _maps3(who, valid, "valid", torch.uint8)
    pi = _like(who, "index", index, valid, torch.int32)
    pd = _like(who, "dist2", dist2, valid, torch.int32, optional=True)
    ws, ws_bytes = _bytes_of(who, workspace, nearest_valid_workspace_bytes(B, h, w), valid.device)
    _check(load().ada_nearest_valid_fwd(valid.data_ptr(), B, h, w, pi, pd, ws.data_ptr(), ws_bytes, _stream()), "ada_nearest_valid_fwd")


def fill_gather(x, valid, index, out, empty=0.0):
    """out[b, c, p] = valid[b, p] ? x[b, c, p] : (index[b, p] >= 0 ? x[b, c, index[b, p]] : empty), bit for bit (ada_fill_gather_fwd).  x, out fp32
    [B, C, h, w]; valid uint8 and index int32 [B, h, w]."""
    who = "fill_gather"
    B, C, h, w = _planes4(who, x)
    po = _like(who, "out", out, x, torch.float32)
    pv = _sized(who, "valid", valid, (B, h, w), torch.uint8)
    pi = _sized(who, "index", index, (B, h, w), torch.int32)
    _same_device(who, "x", x, valid=valid, index=index)
    _check(load().ada_fill_gather_fwd(x.data_ptr(), pv, pi, B, C, h, w, float(empty), po, _stream()), "ada_fill_gather_fwd")


def push_pull(x, valid, out, empty=0.0, workspace=None):
    """x fp32 [B, C, h, w], valid uint8 [B, h, w] -> out: the push-pull fill of include/ada_hip.h's "Hole filling" section (ada_push_pull_fwd); valid
    pixels carry x bit for bit.  ``workspace``: at least push_pull_workspace_bytes(B, C, h, w) bytes, allocated when None."""
    who = "push_pull"
    B, C, h, w = _planes4(who, x)
    po = _like(who, "out", out, x, torch.float32)
    pv = _sized(who, "valid", valid, (B, h, w), torch.uint8)
    _same_device(who, "x", x, valid=valid)
    ws, ws_bytes = _bytes_of(who, workspace, push_pull_workspace_bytes(B, C, h, w), x.device)
    _check(load().ada_push_pull_fwd(x.data_ptr(), pv, B, C, h, w, float(empty), po, ws.data_ptr() if ws_bytes else None, ws_bytes, _stream()), "ada_push_pull_fwd")


def guided_workspace_bytes(batch: int, h: int, w: int, channels: int) -> int:
    """Bytes of workspace ada_guided_coeff_fwd asks for (ada_guided_workspace_bytes): the fp64 planes of the window sums and of the window fits."""
    n = ctypes.c_int64(0)
    _check(load().ada_guided_workspace_bytes(int(batch), int(h), int(w), int(channels), ctypes.byref(n)), "ada_guided_workspace_bytes")
    return n.value


def _guide4(who, guide, batch):
    """(gh, gw, C, ADA_DT_* of the guide) of a non-empty contiguous uint8 / fp32 [B, gh, gw, C] device tensor."""
    if not isinstance(guide, torch.Tensor) or guide.dtype not in (torch.float32, torch.uint8):
        raise HipExtError(f"{who}: guide must be an fp32 or uint8 tensor, got {getattr(guide, 'dtype', type(guide).__name__)}")
    if guide.dim() != 4 or guide.shape[0] != batch or not guide.is_contiguous() or guide.numel() == 0:
        raise HipExtError(f"{who}: guide must be a non-empty contiguous [{batch}, gh, gw, C] tensor, got {tuple(guide.shape)}")
    _dev(guide, "guide")
    return guide.shape[1], guide.shape[2], guide.shape[3], DT_F32 if guide.dtype == torch.float32 else DT_U8


def guided_coeff_fwd(p, guide, radius, eps, coeff, covered, valid=None, workspace=None):
    """p fp32 [B, h, w] and guide uint8 / fp32 [B, gh, gw, C] -> coeff fp64 [B, h, w, C + 1] and covered uint8 [B, h, w]: the window-averaged linear fit
    of p in the guide's samples (ada_guided_coeff_fwd; include/ada_hip.h, "Guided filter").  ``eps`` in raw guide units; ``valid``: uint8 [B, h, w] or
    None; ``workspace``: at least guided_workspace_bytes(B, h, w, C) bytes, allocated when None."""
    who = "guided_coeff_fwd"
    B, h, w = _maps3(who, p, "p")
    gh, gw, C, dt = _guide4(who, guide, B)
    pv = _like(who, "valid", valid, p, torch.uint8, optional=True)
    pc = _sized(who, "coeff", coeff, (B, h, w, C + 1), torch.float64)
    pm = _like(who, "covered", covered, p, torch.uint8)
    _same_device(who, "p", p, guide=guide, coeff=coeff)
    ws, ws_bytes = _bytes_of(who, workspace, guided_workspace_bytes(B, h, w, C), p.device)
    _check(load().ada_guided_coeff_fwd(p.data_ptr(), pv, guide.data_ptr(), dt, B, h, w, gh, gw, C, int(radius), float(eps), pc, pm, ws.data_ptr(), ws_bytes,
                                       _stream()), "ada_guided_coeff_fwd")


def guided_apply_fwd(coeff, covered, guide, out, fill=float("nan")):
    """coeff fp64 [B, h, w, C + 1], covered uint8 [B, h, w] and guide uint8 / fp32 [B, H, W, C] -> out fp32 [B, H, W]: the bilinearly interpolated
    coefficients applied to the guide, ``fill`` where no covered tap has weight (ada_guided_apply_fwd)."""
    who = "guided_apply_fwd"
    B, h, w = _maps3(who, covered, "covered", torch.uint8)
    H, W, C, dt = _guide4(who, guide, B)
    pc = _sized(who, "coeff", coeff, (B, h, w, C + 1), torch.float64)
    po = _sized(who, "out", out, (B, H, W), torch.float32)
    _same_device(who, "covered", covered, guide=guide, coeff=coeff, out=out)
    _check(load().ada_guided_apply_fwd(pc, covered.data_ptr(), guide.data_ptr(), dt, B, h, w, H, W, C, float(fill), po, _stream()), "ada_guided_apply_fwd")


def membrane_workspace_bytes(batch: int, channels: int, h: int, w: int) -> int:
    """Bytes of workspace the ada_membrane_*_fwd calls of one solve share (ada_membrane_workspace_bytes): the fp64 state of conjugate gradients."""
    n = ctypes.c_int64(0)
    _check(load().ada_membrane_workspace_bytes(int(batch), int(channels), int(h), int(w), ctypes.byref(n)), "ada_membrane_workspace_bytes")
    return n.value


def _membrane_workspace(who, workspace, x):
    B, C, h, w = _planes4(who, x)
    ws, ws_bytes = _bytes_of(who, workspace, membrane_workspace_bytes(B, C, h, w), x.device)
    return B, C, h, w, ws, ws_bytes


def membrane_begin(x, known, workspace, domain=None, guess=None, minus=None, tol=1e-9):
    """Starts a membrane solve (ada_membrane_begin_fwd; include/ada_hip.h, "Membrane solve"): x fp32 [B, C, h, w], known and the optional domain uint8
    [B, h, w]; ``guess`` (fp32 like x, None: 0) is the start on the unknown pixels; with ``minus`` (fp32 like x) the data on a known pixel is x - minus in
    fp64.  ``workspace``: a contiguous device tensor of at least membrane_workspace_bytes(B, C, h, w) bytes, which carries the solve to membrane_end."""
    who = "membrane_begin"
    if workspace is None:
        raise HipExtError(f"{who}: the workspace carries the solve from call to call and cannot be None")
    B, C, h, w, ws, ws_bytes = _membrane_workspace(who, workspace, x)
    pk = _sized(who, "known", known, (B, h, w), torch.uint8)
    pd = None if domain is None else _sized(who, "domain", domain, (B, h, w), torch.uint8)
    pg, pm = _like(who, "guess", guess, x, torch.float32, optional=True), _like(who, "minus", minus, x, torch.float32, optional=True)
    _same_device(who, "x", x, known=known, domain=domain)
    _check(load().ada_membrane_begin_fwd(x.data_ptr(), pm, pk, pd, pg, B, C, h, w, float(tol), ws.data_ptr(), ws_bytes, _stream()), "ada_membrane_begin_fwd")


def membrane_iterate(x, workspace, iterations, frozen=None):
    """Exactly ``iterations`` conjugate-gradient steps of the solve in ``workspace`` for all planes of x's shape, frozen planes idle
    (ada_membrane_iterate_fwd).  ``frozen``: optional uint8 [B * C] that receives the planes' frozen flags."""
    who = "membrane_iterate"
    if workspace is None:
        raise HipExtError(f"{who}: the workspace carries the solve from call to call and cannot be None")
    B, C, h, w, ws, ws_bytes = _membrane_workspace(who, workspace, x)
    pf = None if frozen is None else _sized(who, "frozen", frozen, (B * C,), torch.uint8)
    _same_device(who, "x", x, frozen=frozen)
    _check(load().ada_membrane_iterate_fwd(B, C, h, w, int(iterations), pf, ws.data_ptr(), ws_bytes, _stream()), "ada_membrane_iterate_fwd")


def membrane_end(x, workspace, residual, iterations, converged, out=None, out64=None, plus=None):
    """Finishes the solve in ``workspace`` (ada_membrane_end_fwd): out fp32 and / or out64 fp64 [B, C, h, w] = the solution on the unknown pixels (plus
    ``plus``, fp32 like x, when given) and x bit for bit elsewhere; per plane residual fp64 [B * C] (the true residual's max norm), iterations int32 and
    converged uint8."""
    who = "membrane_end"
    if workspace is None:
        raise HipExtError(f"{who}: the workspace carries the solve from call to call and cannot be None")
    B, C, h, w, ws, ws_bytes = _membrane_workspace(who, workspace, x)
    if out is None and out64 is None:
        raise HipExtError(f"{who}: out and out64 are both None")
    po, po64 = _like(who, "out", out, x, torch.float32, optional=True), _like(who, "out64", out64, x, torch.float64, optional=True)
    pp = _like(who, "plus", plus, x, torch.float32, optional=True)
    pr = _sized(who, "residual", residual, (B * C,), torch.float64)
    pi = _sized(who, "iterations", iterations, (B * C,), torch.int32)
    pc = _sized(who, "converged", converged, (B * C,), torch.uint8)
    _same_device(who, "x", x, residual=residual, iterations=iterations, converged=converged)
    _check(load().ada_membrane_end_fwd(x.data_ptr(), pp, B, C, h, w, po, po64, pr, pi, pc, ws.data_ptr(), ws_bytes, _stream()), "ada_membrane_end_fwd")


# --- tuning / diagnostic hooks (include/ada_hip.h, last section) ---------------------------------
TILE_NAMES = {0: "256x32", 1: "128x64", 2: "256x128", 3: "256x256", 4: "128x128"}


_tile_log = None
# bumped by every debug_set_* call: captured HIP graphs (hip_ext/engine.py) bake the kernel variant in, so they are keyed by this epoch
_debug_epoch = 0


def debug_epoch() -> int:
    return _debug_epoch


def instrumented() -> bool:
    """True while a KernelTimer or a tile log is attached: launches must then go through the Python wrappers (no graph replay)."""
    return _timer is not None or _tile_log is not None


def _bump_epoch():
    global _debug_epoch
    _debug_epoch += 1


def set_tile_log(log):
    """log: a list that receives (M, N, K, tile code) for every ada_igemm launch, or None to stop recording."""
    global _tile_log
    _tile_log = log


def debug_set_tile(cfg: int = -1):
    _bump_epoch()
    load().ada_debug_set_tile(int(cfg))


def debug_set_variant(v: int = 0):
    _bump_epoch()
    load().ada_debug_set_variant(int(v))


def debug_set_group(g: int = 0):
    _bump_epoch()
    load().ada_debug_set_group(int(g))


def debug_last_tile() -> int:
    return int(load().ada_debug_last_tile())


def debug_set_attention_variant(v: int = 5):
    _bump_epoch()
    load().ada_debug_set_attention_variant(int(v))


def count_saturated(buf: torch.Tensor, counter: torch.Tensor):
    """Adds to ``counter`` (int64 [1] on the device) the number of elements of the operand-typed tensor ``buf`` that sit at the fp16 clamp
    (+-65504) or are inf / NaN (ada_debug_count_saturated)."""
    if not buf.is_contiguous():
        raise HipExtError("count_saturated: contiguous tensor required")
    _check(load().ada_debug_count_saturated(_dev(buf, "buf", operand_dtype()), buf.numel(), _dev(counter, "counter", torch.int64), _stream()),
           "ada_debug_count_saturated")


def selftest() -> int:
    scratch = torch.zeros(1 << 18, dtype=torch.int32, device="cuda")
    return load().ada_selftest(scratch.data_ptr(), scratch.numel() * 4, _stream())
