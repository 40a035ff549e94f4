"""The case list of tests/test_gpu_igemm_geometry.py, judged without a GPU (tests/_igemm_geometry.py; DESIGN.md, "Geometry sweeps"): it fills the
(tile, epilogue branch, row map) grid, its padded-map families reach every tile position, every mutant of the restated index arithmetic moves an
index of a listed case, the lane-level PadWalk emulation agrees with the closed form under the fixed rule and disagrees under the present one on
exactly the 256x32 cases with 8 <= map_w <= 15, and the inputs are exact: two fp32 orders equal fp64, the budget holds on the very tensors used."""
import pytest
import torch

import _exact as X
import _igemm_geometry as G

CASES = G.cases()
PAD_FAMILIES = ("pad_op", "pad_f32res", "pad_split")


def test_case_ids_are_unique_and_cases_reach_what_they_name():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)[:6]
    print(f"{len(CASES)} cases, {len({G.data_key(c) for c in CASES})} input sets")
    for c in CASES:
        assert c.want in G.branches(c), f"{c.id}: meant for {c.want}, reaches {sorted(G.branches(c))}"
        assert c.M < 2 ** 24 and c.N % 4 == 0


def test_case_list_fills_the_tile_branch_map_grid():
    filled = {}
    for c in CASES:
        for br in G.branches(c):
            filled.setdefault((c.tile, br, c.cell_map), c.id)
    empty, wrongly_filled = [], []
    for tile in G.TILES:
        for br in G.BRANCHES:
            for mp in G.MAPS:
                reason = G.impossible(tile, br, mp)
                if reason is None and (tile, br, mp) not in filled:
                    empty.append((tile, br, mp))
                if reason is not None:
                    assert len(reason) > 20
                    if (tile, br, mp) in filled:
                        wrongly_filled.append(((tile, br, mp), filled[(tile, br, mp)]))
    assert not empty, f"cells no case reaches: {empty}"
    assert not wrongly_filled, f"cells listed as impossible that a case reaches: {wrongly_filled}"
    # every case names its cell: the named branch on the named tile and map is among the filled ones by construction; count them per branch
    print({br: sum(1 for c in CASES if c.want == br) for br in G.BRANCHES})


@pytest.mark.parametrize("family", PAD_FAMILIES)
def test_padded_families_reach_every_tile_position(family):
    for key, t in G.TILES.items():
        cs = [c for c in G.by_family(family) if c.tile == key]
        assert cs, (family, key)
        hw = lambda c: c.map_h * c.map_w      # noqa: E731
        assert any(b.startswith("interior") for c in cs for b in G.branches(c)), f"{family} tile {key}: no interior tile"
        assert all(c.M % t.BM != 0 and c.M > 2 * t.BM for c in cs), f"{family} tile {key}: a case without a ragged last tile above two tile rows"
        assert any(m0 // hw(c) != (min(m0 + t.BM, c.M) - 1) // hw(c) for c in cs for m0, _ in G.tiles_of(c)), f"{family} tile {key}: no tile straddles an image border"
        assert any(m0 % hw(c) != 0 for c in cs for m0, _ in G.tiles_of(c) if m0), f"{family} tile {key}: every tile starts on an image border"
        for step, f32 in ((t.step_op, False), (t.step_f32, True)):      # the two PadWalk users: operand-only, fp32 / residual
            ws = {c.map_w for c in cs if c.has_f32 == f32 and c.ldo_op % 8 == 0}
            if family == "pad_split" or f32 == (family == "pad_f32res"):
                assert any(w < step for w in ws) and any(w >= step for w in ws), f"{family} tile {key}: map widths {sorted(ws)} lie on one side of the step {step}"
    if family == "pad_op":
        ws = {c.map_w for c in G.by_family(family) if c.tile == "0"}
        assert {8, 9, 12, 15} <= ws and {1, 2, 3, 7, 16, 17, 31, 33} <= ws
        assert {c.map_h for c in G.by_family(family)} == {1, 2, 5}
        assert {c.ldo_op % 8 for c in G.by_family(family)} == {0, 4}


@pytest.mark.parametrize("name", list(G.MUTANTS))
def test_case_list_notices_the_mutant(name):
    rules = G.MUTANTS[name]
    hit = []
    for c in CASES:
        a, b = G.indices(c), G.indices(c, rules)
        if any(x.shape != y.shape or not torch.equal(x, y) for x, y in zip(a, b)):
            hit.append(c.id)
    print(f"{name}: moves an index of {len(hit)} of {len(CASES)} cases, e.g. {hit[:3]}")
    assert hit, f"mutant '{name}' changes no source or destination index of any listed case"


def test_pad_walk_emulation_fixed_rule_is_the_closed_form_and_present_rule_fails_on_tile_0_only():
    wrong_present = set()
    padded = [c for c in CASES if c.has_op and c.map_op == "PAD"]
    for c in padded:
        closed = G.pad_row(torch.arange(c.M), c.map_h, c.map_w)
        fixed = G.emulated_pad_rows(c, G.BASE)
        assert bool((fixed == closed[None, :]).all()), f"{c.id}: the walk with the fixed rule leaves the closed form"
        if not bool((G.emulated_pad_rows(c, G.PRESENT) == closed[None, :]).all()):
            wrong_present.add(c.id)
    predicted = {c.id for c in padded if c.tile == "0" and 8 <= c.map_w <= 15 and "interior_op" in G.branches(c, G.PRESENT)}
    claimed = {c.id for c in padded if c.tile == "0" and 8 <= c.map_w <= 15 and not c.has_f32 and not c.res and c.ldo_op % 8 == 0}
    assert predicted == claimed and len(predicted) >= 12
    assert wrong_present == predicted, f"present rule: wrong on {sorted(wrong_present ^ predicted)[:6]} beyond / short of the prediction"
    # what the misplaced stores look like: the second store of a lane (16 rows on) lags 2 padded rows per missed wrap, never ahead, never outside the images
    for c in padded:
        if c.id in predicted:
            got, closed = G.emulated_pad_rows(c, G.PRESENT)[0], G.pad_row(torch.arange(c.M), c.map_h, c.map_w)
            assert bool((got <= closed).all()) and int(got.min()) >= 0
            assert bool(((got != closed) <= ((torch.arange(c.M) % 32) >= 16)).all())


DATA_KEYS = sorted({G.data_key(c) for c in CASES}, key=str)


@pytest.mark.parametrize("key", DATA_KEYS, ids=lambda k: "-".join(str(v) for v in k).replace(" ", ""))
def test_inputs_are_exact_and_restatements_match_the_reference(key):
    d = G._data(key)
    users = [c for c in CASES if G.data_key(c) == key]
    with_res = next((c for c in users if c.res), users[0])
    v, mag = G.values(with_res, d)
    worst = X.assert_exact_budget(mag=mag, unit=d["unit"], ref=v, what=str(key))
    X.assert_exact_budget(mag=d["mag"], unit=d["unit"], ref=d["lin"], what=str(key))
    for i, got in enumerate(d["orders"]()):
        assert got.dtype == torch.float32 and torch.equal(got.reshape(d["lin"].shape).double(), d["lin"]), f"{key}: fp32 order {i} differs from fp64"
    if "dot" in d:
        X.assert_exact_budget(mag=d["dot_mag"], unit=2.0 ** -9, ref=d["dot"], what=str(key) + " tail dot")
        for got in d["dot_orders"]():
            assert torch.equal(got.double(), d["dot"])
    print(f"{key}: worst budget {worst:.3e} units, {len(users)} cases")
    for c in users:
        X.survives(d["W"])
        a = G.a_buffer(c, d)
        X.survives(torch.nan_to_num(a, nan=0.0))
        if c.conv:
            # the restated walk gathers the fp64 convolution from the NaN-guarded buffer: it reads what F.conv2d reads and nothing else
            t = G.TILES[c.tile]
            masks = d.get("masks")
            for n0 in range(0, c.N, t.BN) if masks else [0]:
                taps = G.tap_set(n0, t.BN, c.N, c.c, masks) if masks else 0x1ff
                n1 = min(n0 + t.BN, c.N) if masks else c.N
                got = G.im2col(c, a.double(), taps=taps) @ d["W"].double()[n0:n1].T + d["bias"].double()[n0:n1]
                assert torch.equal(got, d["lin"][:, n0:n1]), f"{c.id}: restated source walk differs from F.conv2d (N-tile at {n0})"
        vv = G.values(c, d)[0]
        if c.out == "tail":
            buf = G.expected_f32(c, d["dot"])
            assert torch.equal(buf[:c.M, 0].double(), d["dot"]) and bool((buf[c.M:] == G.SENTINEL).all())
            continue
        if c.has_f32:
            buf = G.expected_f32(c, vv)
            assert int(torch.isnan(buf).sum()) == 0 and int((buf != G.SENTINEL).sum()) <= c.M * c.N
            if c.map_f32 == "TOKEN":
                b3 = buf.view(c.B + 1, c.Np + 1, -1)
                assert torch.equal(b3[:c.B, 1:, :c.N].reshape(c.M, c.N).double(), vv) and bool((b3[:, 0] == G.SENTINEL).all())
        if c.has_op:
            for op in X.OP_TYPES:
                if c.split < 0 and op != torch.float16:
                    continue
                buf = G.expected_op(c, vv, op)
                if c.split < 0:
                    continue
                assert int(torch.isnan(buf.float()).sum()) == 0, f"{c.id}: the destination map leaves cells unwritten"
                want = X.rne(vv.clamp_min(0) if c.relu else vv, op)
                if c.map_op == "PAD":
                    got = buf.view(c.B + 1, c.map_h + 2, c.map_w + 2, -1)[:c.B, 1:-1, 1:-1, :c.N].reshape(c.M, c.N)
                    assert torch.equal(got, want)
                elif c.map_op == "SHUFFLE":
                    s, h, w = c.s, c.map_h, c.map_w
                    fine = buf.view(c.B + 1, s * h + 2, s * w + 2, -1)[:c.B, 1:-1, 1:-1, :c.c]
                    ref = want.view(c.B, h, w, s, s, c.c).permute(0, 1, 3, 2, 4, 5).reshape(c.B, s * h, s * w, c.c)
                    assert torch.equal(fine, ref)
