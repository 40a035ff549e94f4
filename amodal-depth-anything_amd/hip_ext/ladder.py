"""The precision ladder's arithmetic that needs no device (pure torch): the calibration's curves and thresholds, the rung rule and the rule for the rung the
next call starts on.  DepthEngine (hip_ext.engine) runs the rungs and reads the statistics; everything it DECIDES is decided here, once, for every order in
which the rungs can run -- "which head runs first changes what a call costs, never what it returns" rests on ladder_decide alone."""
from __future__ import annotations

from typing import Optional

import torch

from . import ACT_NONE, ACT_RELU, ACT_SIGMOID, HipExtError


def ladder_curve(zk: torch.Tensor, z3: torch.Tensor, act: int):
    """The calibration's raw material (DepthEngine.calibrate; pure torch, any device): for every image [n, ...] and every shift d of the grid, (r, e) =
    (the image's sensitivity  sum w(z3 + d) / sum |f(z3 + d)|,  the metric  sum |f(zk + d) - f(z3 + d)| / sum |f(z3 + d)|  of rung k against the third),
    f / w = sigmoid / s(1-s), ReLU / [z > 0], identity / 1.  Returns R, E as [n, shifts] float64 tensors."""
    a, t = zk.flatten(1).double(), z3.flatten(1).double()
    if act == ACT_NONE:      # a shift of bare logits changes nothing but the denominator: one point per image, e = eps r exactly
        den = t.abs().sum(1).clamp_min(1e-300)
        return (t.shape[1] / den).unsqueeze(1), ((a - t).abs().sum(1) / den).unsqueeze(1)
    if act == ACT_SIGMOID:      # shifts that put the map's mean between ~0.9 and ~0.02 -- in units of the logits' own spread where that is wide, so that r reaches -> 1
        scale = t.std(dim=1, keepdim=True).clamp_min(1.0)
        grid = -t.median(dim=1, keepdim=True).values + scale * torch.linspace(-5.0, 2.0, 29, dtype=t.dtype, device=t.device)[None, :]
    else:                       # ReLU: shifts that leave 97 % ... 3 % of the map positive
        qs = torch.tensor([0.03, 0.08, 0.15, 0.25, 0.35, 0.5, 0.65, 0.75, 0.85, 0.92, 0.97], dtype=t.dtype, device=t.device)
        grid = -torch.quantile(t, qs, dim=1).t()
    R, Em = [], []
    for j in range(grid.shape[1]):
        d = grid[:, j:j + 1]
        if act == ACT_SIGMOID:
            fa, ft = torch.sigmoid(a + d), torch.sigmoid(t + d)
            wsum = (ft * (1 - ft)).sum(1)
        else:
            fa, ft = (a + d).clamp_min(0), (t + d).clamp_min(0)
            wsum = (ft > 0).double().sum(1)
        den = ft.sum(1).clamp_min(1e-300)
        R.append(wsum / den)
        Em.append((fa - ft).abs().sum(1) / den)
    return torch.stack(R, 1), torch.stack(Em, 1)


def ladder_thresholds(z1: torch.Tensor, z2: Optional[torch.Tensor], z3: torch.Tensor, act: int, budget: float, safety: float, rule: str = "cross") -> dict:
    """Thresholds of the precision ladder from the logits of the rungs on the calibration images (see DepthEngine.calibrate): per rung k the largest eps = e / r over
    the points, the `global` threshold budget / (safety eps_max) and the `cross` threshold -- the smallest r at which a calibration point has safety * e > budget (the
    rung's error AT the operating point where it would be left, not its worst anywhere; inf when no point exceeds the budget).  r from rung 1, r3 from rung 2 (no
    second rung: r3 from rung 1).  A sigmoid's r lives in (0, 1): its thresholds are capped at 0.97.  Pure torch: unit-tested on the CPU."""
    if rule not in ("cross", "global"):
        raise HipExtError(f"ladder_thresholds: rule={rule!r} (cross | global)")

    def one(zk):
        R, Em = ladder_curve(zk, z3, act)
        eps_max = float((Em / R.clamp_min(1e-300)).max())
        bad = Em * safety > budget
        return eps_max, budget / (safety * max(eps_max, 1e-30)), (float(R[bad].min()) if bool(bad.any()) else float("inf"))
    cap = (lambda v, lo: min(max(v, lo), 0.97)) if act == ACT_SIGMOID else (lambda v, lo: max(v, lo))
    pick = (lambda g, c: c if rule == "cross" else g)
    e1, g1, c1 = one(z1)
    res = dict(budget=budget, safety=safety, rule=rule, eps1=e1, r_global=g1, r_cross=c1, act={ACT_SIGMOID: "sigmoid", ACT_RELU: "relu", ACT_NONE: "none"}[act])
    if z2 is not None:
        e2, g2, c2 = one(z2)
        r = cap(pick(g1, c1), 0.02)
        res.update(eps2=e2, r3_global=g2, r3_cross=c2, r=r, r3=cap(pick(g2, c2), r))
    else:
        res.update(r3=cap(pick(g1, c1), 0.0))
    return res


def stats_from_host(host: torch.Tensor, B: int, chunks: int, groups: int, has_r: bool, div: Optional[float], has_in: bool, div_in: float = 1e-4):
    """The ladder's per-image statistics from a HOST copy of a Workspace.stat_buf (DepthEngine._image_stats reads it; ada_ladder_select_fwd does the same
    arithmetic on the device and is tested against this function).  ``host``: the buffer as a flat float64 CPU tensor, laid out [B, chunks, 2] (sum |f|, sum w) of
    the depth map | [B, groups, 2] (sum of column variances, sum of column mean squares) of the last tap | [B, rest, 2] the same of the patchified input (read only
    with ``has_in``).  ``div``: the tap-diversity threshold, None or <= 0 for none.  Returns (r, flat, tap_div, in_div): float64 / bool [B], None for a diversity
    that is not read; r = zeros without ``has_r``.  The pairs of a block are added in fp64.  torch's CPU sum picks its own order (several accumulators, by shape),
    the device adds in index order: the two are the same bits whenever the sum is exact in fp64, i.e. for n fp32 terms whose magnitudes span less than
    2^(53 - 24 - ceil(log2 n)) -- 2^26 for the eight chunks of a depth map -- and can differ by one fp64 rounding beyond that.  The
    denominators are clamped with clamp_min, which lets a NaN through: a NaN statistic compares false with every threshold."""
    nst, ndv = B * chunks * 2, B * groups * 2
    st = host[:nst].view(B, chunks, 2).sum(1)
    r = st[:, 1] / st[:, 0].clamp_min(1e-300) if has_r else torch.zeros(B, dtype=torch.float64)
    flat = torch.zeros(B, dtype=torch.bool)
    tap_div = in_div = None
    if div is not None and div > 0.0:
        dv = host[nst:nst + ndv].view(B, -1, 2).sum(1)
        tap_div = dv[:, 0] / dv[:, 1].clamp_min(1e-300)
        flat = tap_div < div
    if has_in:      # every patch of the image alike: variance over patches below 1e-4 of their mean square
        di = host[nst + ndv:].view(B, -1, 2).sum(1)
        in_div = di[:, 0] / di[:, 1].clamp_min(1e-300)
        flat = flat | (in_div < div_in)
    return r, flat, tap_div, in_div


def ladder_decide(r: torch.Tensor, flat: torch.Tensor, lad: dict, ran: int, guard: float) -> torch.Tensor:
    """THE rung rule.  ``r``: float64 [B], the per-image sensitivity read from the output of rung ``ran`` (1, 2 or 3); ``flat``: bool [B], the diversity triggers;
    ``lad``: the engine's ladder dict (keys and thresholds only: "make" / "make3" say which rungs exist, "r" / "r3" where they begin); ``guard``: the relative band
    around a threshold inside which a higher rung's r does not decide (the rungs' maps differ by ~1e-3 of their logits).  Returns int64 [B]: the image's final rung
    1 / 2 / 3 -- or, for ran != 1, 0: the FIRST rung must be run for this image and its own r decides (ladder_decide(r1, flat1, lad, 1, guard)).

    ran = 1:  3 where the third rung exists and the image is flat or r > r3;  else 2 where the second exists and the image is flat or r > r;  else 1.
    ran = 2:  0 where the image is not flat and r <= r (1 + g) or r is within g of r3;  else 3 where the third rung exists and the image is flat or r > r3 (1 + g);  else 2.
    ran = 3:  3 where the image is flat or r > r3 (1 + g);  else 0.
    An image that a higher rung decides carries what the first-rung-first order computes for it as long as the two r differ by less than the guard band."""
    inf = float("inf")
    has2, has3 = "make" in lad, "make3" in lad
    thr = lad["r"] if has2 and "r" in lad else inf
    thr3 = lad["r3"] if has3 and "r3" in lad else inf
    never = torch.zeros_like(flat)
    one, two, three, undecided = (torch.full(flat.shape, k, dtype=torch.int64) for k in (1, 2, 3, 0))
    if ran == 1:
        to3 = (flat | (r > thr3)) if has3 else never
        to2 = (flat | (r > thr)) if has2 else never
        return torch.where(to3, three, torch.where(to2, two, one))
    g = guard
    if ran == 2:
        if not has2:
            raise ValueError("ladder_decide: ran=2 on a ladder without a second rung")
        near3 = ((r / thr3 - 1.0).abs() <= g) if thr3 < inf else never
        first = ~flat & ((r <= thr * (1.0 + g)) | near3)
        to3 = (flat | (r > thr3 * (1.0 + g))) if has3 else never
        return torch.where(first, undecided, torch.where(to3, three, two))
    if ran == 3:
        if not thr3 < inf:
            raise ValueError("ladder_decide: ran=3 on a ladder without a third rung and a finite r3")
        return torch.where(flat | (r > thr3 * (1.0 + g)), three, undecided)
    raise ValueError(f"ladder_decide: ran={ran!r} (1 | 2 | 3)")


def rung_counts(rungs: torch.Tensor):
    """(images on the second rung or higher, images on the third) of a vector of final rungs: what a call adds to DepthEngine.escalated / escalated3."""
    return int((rungs >= 2).sum()), int((rungs == 3).sum())


def next_start_rung(rungs: torch.Tensor, has2: bool) -> int:
    """The rung the NEXT call runs first: the one MORE THAN HALF of this call's images ended on (a stream of such images does not pay the rungs in front of it
    for nothing), else the first."""
    B = int(rungs.numel())
    if 2 * int((rungs == 3).sum()) > B:
        return 3
    if has2 and 2 * int((rungs == 2).sum()) > B:
        return 2
    return 1
