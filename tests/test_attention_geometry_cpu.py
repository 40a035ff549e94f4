"""No GPU: the premises of the attention geometry sweep (tests/_attention_geometry.py, tests/test_gpu_attention_geometry.py), on the very tensors the
GPU tests build -- the routing scores are exact, their maximum is unique, 128 log2 units clear and where pi says; V is exact and its rows distinct; the
census counts are what the classes say -- and the sensitivity of the case list: an fp32 emulation of the tiled online softmax returns the routed rows bit
for bit and the census within its bound on every listed case in both operand types, and each of seven mutants of it (a mask off by one in either
direction, a k-slot permutation P and V disagree on, a head or batch stride, a missing rescale, the block remap) fails at least one listed case.  The
same mutants are run against the Gaussian inputs of test_attention_variants for comparison (printed; profiles/attention_geometry.txt)."""
import torch

import _attention_geometry as G


def _all_routing_layouts():
    seen = []
    for fam, B, heads, N, _ in G.listed_cases():
        if fam == "R":
            seen.append((B, heads, N))
    for lay in G.FORM_LAYOUTS:
        assert lay in seen, f"output-form layout {lay} is not among the routed cases"
    return seen


def test_remap_restated_is_a_bijection():
    """Every launch block gets one logical block and every logical block is taken, for every block count 1 ... 64; one XCD's logical ids are contiguous
    (that is the point of the remap); the mutant is no bijection from 8 blocks on, except where only XCD 7 takes the other branch, whose two forms
    agree there."""
    for nblk in range(1, 65):
        ids = [G.remap(bid, nblk) for bid in range(nblk)]
        assert sorted(ids) == list(range(nblk)), f"nblk {nblk}: {ids}"
        for xcd in range(min(8, nblk)):
            mine = [G.remap(bid, nblk) for bid in range(xcd, nblk, 8)]
            assert mine == list(range(mine[0], mine[0] + len(mine))), f"nblk {nblk}, XCD {xcd}: {mine}"
        mutant = sorted(G.remap(bid, nblk, True) for bid in range(nblk))
        assert (mutant == list(range(nblk))) == (nblk < 8 or nblk % 8 == 7), f"nblk {nblk}: the mutant remap gives {mutant}"


def test_layouts_cover_the_remap_classes():
    counts = [G.n_blocks(*lay) for lay in G.LAYOUTS]
    assert counts == [30, 18, 16, 10, 12, 12, 7, 7, 3]
    classes = {G.remap_class(c) for c in counts}
    assert classes == {"nblk < 8", "nblk mod 8 = 0", "nblk mod 8 != 0"}, classes
    # both branches of the remap live in one launch: more than 8 blocks, not a multiple of 8
    assert sum(1 for c in counts if c > 8 and c % 8) >= 4


def test_lengths_cover_every_residue_parity_and_wave_count():
    L = [n for n in G.LENGTHS if n <= 321]
    assert L == list(range(1, 322))
    for tiles in range(1, 6):
        assert {n % 64 for n in L if (n + 63) // 64 == tiles} == set(range(64)), f"{tiles} tiles: not every residue"
    assert {((n - 1) % 128) // 32 for n in L} == {0, 1, 2, 3}          # active waves of the last query block - 1
    assert {128, 129, 256, 257, 384, 385, 1370, 1409, 5330} <= set(G.LENGTHS)


def test_routing_premise():
    """Scores: multiples of 32 within +-1024, the maximum at pi(i), unique, margin >= 128.  V: integers 1 ... 7 in magnitude, exact in fp16, bf16 and
    e5m2, rows pairwise distinct within the launch.  q and k exact in both operand types."""
    for B, heads, N in _all_routing_layouts():
        case = G.routing(B, heads, N)
        D = heads * G.HD
        qkv = case["qkv"]
        assert bool(torch.isnan(qkv[-1]).all()) and bool(torch.isfinite(qkv[:-1]).all())
        for op in G.OP_TYPES:
            assert torch.equal(qkv[:-1].to(op).float(), qkv[:-1])
        v = case["v"]
        assert float(v.abs().min()) >= 1.0 and float(v.abs().max()) <= 7.0 and torch.equal(v, v.round())
        assert torch.equal(v.to(torch.float8_e5m2).float(), v)
        flat_v = v.reshape(-1, G.HD)
        assert torch.unique(flat_v, dim=0).shape[0] == flat_v.shape[0], f"{(B, heads, N)}: V rows repeat"
        t = qkv[:-1].reshape(B, N, 3, heads, G.HD).permute(2, 0, 3, 1, 4)          # [3, B, heads, N, 64]
        assert torch.equal(t[2], v)
        for b in range(B):
            for h in range(heads):
                s = t[0, b, h] @ t[1, b, h].T
                s64 = t[0, b, h].double() @ t[1, b, h].double().T
                assert torch.equal(s.double(), s64)
                assert torch.equal(s % 32, torch.zeros_like(s)) and float(s.abs().max()) <= 1024.0
                top = s.max(1)
                assert torch.equal(top.indices, case["perm"][b, h]) and bool((top.values == 1024.0).all())
                if N > 1:
                    second = s.scatter(1, top.indices.view(N, 1), float("-inf")).max(1).values
                    assert float(second.max()) <= 1024.0 - 128.0, f"{(B, heads, N)} ({b}, {h}): margin {1024.0 - float(second.max())}"
        assert torch.equal(case["want"].reshape(B, N, heads, G.HD).permute(0, 2, 1, 3), torch.gather(v, 2, case["perm"].unsqueeze(-1).expand(-1, -1, -1, G.HD)))
        if B * heads > 1:      # the salt: the same position holds another code in every other (b, h), so a foreign K does not route to the same position
            k = t[1].reshape(B * heads, N, G.HD)
            assert not bool((k[0] == k[1:]).all(-1).any())


def test_census_premise():
    for N in G.LENGTHS:
        for which in (0, 1):
            case = G.census(N, which)
            qkv = case["qkv"]
            assert bool(torch.isnan(qkv[-1]).all()) and bool((qkv[:-1, :G.HD] == 0).all()) and bool(torch.isfinite(qkv[:-1]).all())
            v = qkv[:-1, 2 * G.HD:]
            assert bool(((v == 0) | (v == 1)).all()) and bool((v.sum(1) == 1).all())
            assert torch.equal(v.sum(0).long(), case["count"]) and int(case["count"].sum()) == N
            if which == 0:
                assert int(case["count"].max()) - int(case["count"].min()) <= 1
            else:      # full tiles of one class, then the tail
                per = 128 if N > 4096 else 64
                full, tail = divmod(N, per)
                assert case["count"][:full].tolist() == [per] * full and (tail == 0 or int(case["count"][full]) == tail)


def test_emulation_returns_the_derived_result_on_every_listed_case():
    worst, ran = 0.0, 0
    for op in G.OP_TYPES:
        for mode in G.MODES:
            for fam, B, heads, N, which in G.listed_cases():
                ran += 1
                if fam == "R":
                    msg = G.emulated_failure(fam, B, heads, N, which, op, mode)
                else:
                    case = G.census(N, which)
                    got = G.emulate(case["qkv"], 1, N, 1, op, mode)
                    worst = max(worst, G.census_error(case, got, op))
                    msg = G.census_failure(case, got, op, N)
                assert msg is None, f"{fam} {(B, heads, N)} launch {which}, {op}, mode {mode}: {msg}"
    print(f"emulation: {ran} runs pass; worst census error = {worst:.3f} of its bound")
    assert worst <= 1.0


def _first_caught(mutant, family, op, mode):
    for fam, B, heads, N, which in G.listed_cases():
        if fam == family and G.emulated_failure(fam, B, heads, N, which, op, mode, mutant) is not None:
            return f"(B, heads, N) = ({B}, {heads}, {N})" + (f" launch {which}" if fam == "C" else "")
    return None


def test_every_mutant_fails_a_listed_case():
    """The full table (first routed case and first census case that fails, or none in the whole list) for the fp16 "mix" emulation; for the other
    operand type and mode, that some listed case fails."""
    print("\nmutant of the emulation | first routing case that fails | first census case that fails     (fp16, mode mix)")
    for mutant, what in G.MUTANTS.items():
        r = _first_caught(mutant, "R", torch.float16, "mix")
        c = _first_caught(mutant, "C", torch.float16, "mix")
        print(f"  {what:68s} | {r or 'none of 336':30s} | {c or 'none of 654'}")
        assert r is not None or c is not None, f"mutant '{what}' passes every listed case"
    for op, mode in ((torch.float16, "v3"), (torch.bfloat16, "mix"), (torch.bfloat16, "v3")):
        for mutant, what in G.MUTANTS.items():
            caught = _first_caught(mutant, "R", op, mode) or _first_caught(mutant, "C", op, mode)
            assert caught is not None, f"mutant '{what}' passes every listed case ({op}, mode {mode})"


def test_mutants_on_the_gaussian_inputs_for_comparison():
    """What the existing tolerance (atol 2e-3, rtol 3e-3 against softmax in higher precision) sees of the same mutants on the inputs of
    test_attention_variants: share of elements out of tolerance and the worst error in units of it.  The unmutated emulation must pass there."""
    op, mode = torch.float16, "mix"
    print("\nGaussian inputs of test_attention_variants (fp16, mode mix): share of elements out of tolerance / worst error in units of the tolerance")
    print("  " + " " * 68 + " | " + " | ".join(f"{str(c):>14s}" for c in G.GAUSS_CASES))
    for mutant in (None,) + tuple(G.MUTANTS):
        cells = []
        for B, N, heads in G.GAUSS_CASES:
            qkv, ref = G.gaussian(B, N, heads, op)
            share, worst = G.gaussian_miss(G.emulate(qkv, B, N, heads, op, mode, mutant), ref, op)
            if mutant is None:
                assert share == 0.0, f"the emulation itself misses the tolerance on {(B, N, heads)}: {share:.3%}, worst {worst:.2f} x"
            cells.append(f"{share:7.2%} {worst:6.1f}" if worst != float("inf") else f"{share:7.2%}    NaN")
        print(f"  {(G.MUTANTS[mutant] if mutant else 'none (the emulation as it is)'):68s} | " + " | ".join(cells))
