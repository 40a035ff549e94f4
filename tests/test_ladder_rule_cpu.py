"""CPU: the precision ladder's rung rule (hip_ext.ladder.ladder_decide / next_start_rung / rung_counts: pure torch) against a literal transcription of the three
rules it replaced -- the first-rung-first, second-rung-first and third-rung-first orders of DepthEngine, one image at a time -- on a grid that reaches every cell:
r at and around both thresholds and the guard band, flat and not, every combination of rungs and thresholds a ladder can have.  No GPU, no library call."""
import itertools

import pytest
import torch

from hip_ext.ladder import ladder_decide, next_start_rung, rung_counts

INF = float("inf")
G = 0.02
MULTS = (0.5, 1 - G / 2, 1.0, 1 + G / 2, 1 + 2 * G)


# ---- the yardstick: the three old rules, per image ---------------------------------------------------------------------------------------
def old_first(r, flat, lad):
    """First rung first: the rung of an image from its first-rung r and diversity triggers."""
    trigger = ((r > lad["r"]) if ("r" in lad and "make" in lad) else False) or (flat if "make" in lad else False)
    top = (((r > lad["r3"]) if "r3" in lad else False) or flat) if "make3" in lad else False
    return 3 if top else (2 if trigger else 1)


def old_second(r2, flat, lad, g):
    """Second-rung head first: 0 = the first-rung head must run for the image (then old_second_then_first), else the rung r2 decides."""
    thr, thr3 = lad["r"], lad.get("r3", INF)
    has3 = "make3" in lad
    near3 = (abs(r2 / thr3 - 1.0) <= g) if (has3 and thr3 < INF) else False
    need1 = (not flat) and ((r2 <= thr * (1.0 + g)) or near3)
    rung = 2
    if has3 and (flat or r2 > thr3 * (1.0 + g)):
        rung = 3
    return 0 if need1 else rung


def old_second_then_first(r1, lad):
    thr, thr3 = lad["r"], lad.get("r3", INF)
    return 3 if (r1 > thr3 and "make3" in lad) else (2 if r1 > thr else 1)


def old_third(r3v, flat, lad, g):
    """Third-rung engine first: 3 = keeps its result, 0 = goes through the ordinary order (old_first on its own first-rung r AND flat)."""
    return 3 if (flat or r3v > lad["r3"] * (1.0 + g)) else 0


# ---- ladders: with and without make / make3 / "r" / "r3", thr == thr3, thr3 = inf ----------------------------------------------------------
def ladders():
    make = lambda: None     # noqa: E731  (never called: the rule reads keys and thresholds only)
    out = []
    for has2, has3, has_r, r3 in itertools.product((False, True), (False, True), (False, True), (None, 0.6, 0.4, INF)):
        lad = {}
        if has2:
            lad["make"] = make
        if has3:
            lad["make3"] = make
        if has_r:
            lad["r"] = 0.4
        if r3 is not None:
            lad["r3"] = r3
        out.append(lad)
    return out


def r_grid(lad):
    pts = {m * t for m in MULTS for t in (lad.get("r", 0.4), lad.get("r3", 0.6)) if t < INF}
    return sorted(pts | {0.0, 0.97, 5.0})


def decide(rs, flats, lad, ran):
    return ladder_decide(torch.tensor(rs, dtype=torch.float64), torch.tensor(flats, dtype=torch.bool), lad, ran, G).tolist()


def test_first_rung_rule_matches_the_old_one_in_every_cell():
    n = 0
    for lad in ladders():
        rs = r_grid(lad)
        for flat in (False, True):
            got = decide(rs, [flat] * len(rs), lad, 1)
            want = [old_first(r, flat, lad) for r in rs]
            assert got == want, (lad, flat, rs, got, want)
            n += len(rs)
    assert n > 500
    # the cells by name: no second rung -> a flat image goes to the third or stays; second rung only -> flat is rung 2; without "r" only flat and r3 act
    make = lambda: None     # noqa: E731
    assert decide([0.1, 0.5, 0.9], [True, False, False], dict(make=make, r=0.4), 1) == [2, 2, 2]
    assert decide([0.1, 0.5, 0.9], [True, False, False], dict(make3=make, r3=0.6, div_in=1e-4), 1) == [3, 1, 3]
    assert decide([0.1, 0.5, 0.9], [True, False, False], dict(make3=make), 1) == [3, 1, 1]
    assert decide([0.1, 0.5, 0.9, 0.4, 0.6], [False] * 5, dict(make=make, make3=make, r=0.4, r3=0.6), 1) == [1, 2, 3, 1, 2]
    assert decide([0.5], [False], dict(r=0.4, r3=0.45), 1) == [1]      # thresholds without rungs


def test_second_rung_rule_matches_the_old_one_in_every_cell():
    n = 0
    for lad in ladders():
        if "make" not in lad or "r" not in lad:       # the old order read lad["r"] unconditionally and was entered only with a second rung
            continue
        rs = r_grid(lad)
        for flat in (False, True):
            got = decide(rs, [flat] * len(rs), lad, 2)
            want = [old_second(r, flat, lad, G) for r in rs]
            assert got == want, (lad, flat, rs, got, want)
            assert 1 not in got and (0 not in got if flat else True)
            # ... and the images it hands to the first rung are decided as the old order decided them (never flat there)
            got1 = decide(rs, [False] * len(rs), lad, 1)
            assert got1 == [old_second_then_first(r, lad) for r in rs] == [old_first(r, False, lad) for r in rs]
            n += len(rs)
    assert n > 100
    make = lambda: None     # noqa: E731
    lad = dict(make=make, make3=make, r=0.4, r3=0.6)
    #            below   in band (below / above thr)      clear 2   near r3 (both sides)         clear 3   flat
    rs = [0.2, 0.4 * (1 - G / 2), 0.4 * (1 + G / 2), 0.5, 0.6 * (1 - G / 2), 0.6 * (1 + G / 2), 0.7, 0.2]
    assert decide(rs, [False] * 7 + [True], lad, 2) == [0, 0, 0, 2, 0, 0, 3, 3]
    assert decide([0.2, 0.5, 0.9], [False, False, True], dict(make=make, r=0.4), 2) == [0, 2, 2]     # no third rung: flat keeps the second
    with pytest.raises(ValueError):
        decide([0.5], [False], dict(make3=make, r3=0.6), 2)


def test_third_rung_rule_matches_the_old_one_in_every_cell():
    n = 0
    for lad in ladders():
        if "make3" not in lad or not lad.get("r3", INF) < INF:
            with pytest.raises(ValueError):
                decide([0.5], [False], lad, 3)
            continue
        rs = r_grid(lad)
        for flat in (False, True):
            got = decide(rs, [flat] * len(rs), lad, 3)
            assert got == [old_third(r, flat, lad, G) for r in rs], (lad, flat)
            n += len(rs)
    assert n > 100
    with pytest.raises(ValueError):
        decide([0.5], [False], dict(make=lambda: None, r=0.4), 4)


def _two_stages(lad, ran, r_start, flat_start, r1, flat1):
    """What the executor does with the rule: the start rung's r decides what it can, the first rung's r (and, behind the third rung, its flat) the rest."""
    rung = ladder_decide(torch.tensor(r_start, dtype=torch.float64), torch.tensor(flat_start), lad, ran, G)
    idx = torch.nonzero(rung == 0).flatten()
    if idx.numel():
        rung[idx] = ladder_decide(torch.tensor(r1, dtype=torch.float64)[idx], torch.tensor(flat1)[idx], lad, 1, G)
    return rung


def test_mixed_batches_through_two_stages():
    make = lambda: None     # noqa: E731
    lad = dict(make=make, make3=make, r=0.4, r3=0.6, div=0.1, div_in=1e-4)
    # second rung first; r1 within 1e-3 of r2 as on the device.  Images: clearly below -> 1; in the band, r1 below -> 1; in the band, r1 above -> 2; clear 2;
    # near r3 with r1 below r3 -> 2; near r3 with r1 above -> 3; clear 3; flat -> 3
    r2 = [0.2, 0.4 * (1 + G / 2), 0.4 * (1 + G / 2), 0.5, 0.6 * (1 + G / 2), 0.6 * (1 - G / 2), 0.8, 0.3]
    r1 = [0.2003, 0.3999, 0.4001, 0.5004, 0.5999, 0.6001, 0.8002, 0.3001]
    flat = [False] * 7 + [True]
    rung = _two_stages(lad, 2, r2, flat, r1, flat)
    assert rung.tolist() == [1, 1, 2, 2, 2, 3, 3, 3]
    want = []
    for a, b, f in zip(r2, r1, flat):
        k = old_second(a, f, lad, G)
        want.append(old_second_then_first(b, lad) if k == 0 else k)
    assert rung.tolist() == want == [old_first(b, f, lad) for b, f in zip(r1, flat)]       # = what the first-rung-first order assigns
    assert rung_counts(rung) == (6, 3) and next_start_rung(rung, True) == 1
    # third rung first: undecided images end on each of the rungs -- the third again through r1, or through the FIRST-rung run's own flat trigger
    r3v = [0.9, 0.2, 0.5, 0.6 * (1 + G / 2), 0.6 * (1 + G / 2), 0.3, 0.3]
    r1 = [0.9003, 0.2001, 0.5002, 0.5999, 0.6002, 0.3001, 0.3001]
    flat3 = [False, False, False, False, False, True, False]      # flat by the third-rung run's statistics ...
    flat1 = [False, False, False, False, False, True, True]       # ... and by the first rung's
    rung = _two_stages(lad, 3, r3v, flat3, r1, flat1)
    assert rung.tolist() == [3, 1, 2, 2, 3, 3, 3]
    want = []
    for a, f3, b, f1 in zip(r3v, flat3, r1, flat1):
        k = old_third(a, f3, lad, G)
        want.append(old_first(b, f1, lad) if k == 0 else k)
    assert rung.tolist() == want
    assert rung_counts(rung) == (6, 4) and next_start_rung(rung, True) == 3
    # a ladder without a second rung (raw / ssi / ViT-S) behind the third rung: back to the first or the third again
    lad3 = dict(make3=make, r3=0.6, div_in=1e-4)
    rung = _two_stages(lad3, 3, [0.9, 0.5, 0.605], [False] * 3, [0.9, 0.5, 0.6001], [False] * 3)
    assert rung.tolist() == [3, 1, 3] and rung_counts(rung) == (2, 2)


def test_next_start_rung_needs_more_than_half_and_follows_a_stream():
    t = lambda *v: torch.tensor(v, dtype=torch.int64)     # noqa: E731
    assert next_start_rung(t(3, 3, 1, 1), True) == 1 and next_start_rung(t(3, 3, 3, 1), True) == 3          # exactly half is not enough
    assert next_start_rung(t(2, 2, 1, 1), True) == 1 and next_start_rung(t(2, 2, 2, 1), True) == 2
    assert next_start_rung(t(3, 3, 2, 2), True) == 1 and next_start_rung(t(3, 2, 2, 2), True) == 2
    assert next_start_rung(t(2, 2, 2), False) == 1 and next_start_rung(t(3,), False) == 3 and next_start_rung(t(1,), True) == 1
    # consecutive calls of one engine: 1 -> 2 -> 3 -> 1, with the counters each call adds
    start, esc, esc3, seen = 1, 0, 0, []
    for rungs in (t(2, 2, 1), t(3, 3, 2), t(1, 1, 3), t(1, 1, 1)):
        n2, n3 = rung_counts(rungs)
        esc, esc3 = esc + n2, esc3 + n3
        start = next_start_rung(rungs, True)
        seen.append((start, esc, esc3))
    assert seen == [(2, 2, 0), (3, 5, 2), (1, 6, 3), (1, 6, 3)]
    assert rung_counts(t(1, 2, 3, 3, 0)) == (3, 2)
