"""CPU proof that the per-element bounds of the loss-head tests bite (tests/_loss_head_cases.py check, applied to the kernels by
tests/test_loss_head_gpu.py).  No kernel runs here: the kernels' arithmetic is restated in torch CPU float32, in their order of
operations, and judged by the same checker as the kernels, against the same float64 reference, on every case.

  * The constants K of the bounds are 4 x the worst ratio |restatement - reference| / F the two honest restatements reach over all
    cases, rounded up to a power of two (test_the_constants_are_four_times_the_measured_ratios prints the table that the
    helper's docstring holds and asserts that K is that number).
  * The honest restatements pass every case within a quarter of the bound (dlogits of the bf16 mode: the fp32 value before its
    rounding within a quarter of the fp32 term K F; the rounded value within the whole bound, of which bf16 round-to-nearest of
    the reference alone can take all but K F).
  * Every mutant of L.MUTANTS is rejected by at least one case; which ones is printed.  No mutant survives, no case is skipped.
"""
import functools
import math

import pytest
import torch

from tests import _loss_head_cases as L

CASES = L.cases()
IDS = [c.name for c in CASES]
ONES = dict.fromkeys(L.K, 1.0)
OUTPUT_OF = {"lse": ("row_lse", "tstats lse"), "loss": ("row_loss",), "stats0": ("stats[0]",), "dlogits": ("dlogits_f32",), "ex": ("tstats E_p[x]",)}


@functools.lru_cache(maxsize=None)
def _honest(i):
    c = CASES[i]
    return L.restate_bf16(c), L.restate_f32(c, True), L.restate_f32(c, False)


@functools.lru_cache(maxsize=None)
def _unit_ratios():
    """-> {constant: (worst ratio at K = 1 of the bf16-kernel restatement, of the fp32-twin restatement)} over all cases"""
    worst = {k: [0.0, 0.0] for k in L.K}
    for i, c in enumerate(CASES):
        b, f_exact, f_bf = _honest(i)
        rb = L.check(c, b, k=ONES, limit=math.inf)
        for k, names in OUTPUT_OF.items():
            worst[k][0] = max(worst[k][0], *(rb[n] for n in names))
        for out, exact_values in ((f_exact, True), (f_bf, False)):
            rf = L.check(c, out, fp32_mode=True, fp32_values=exact_values, k=ONES, limit=math.inf)
            for k, n in (("lse", "row_lse"), ("loss", "row_loss"), ("stats0", "stats[0]"), ("dlogits", "dlogits")):
                worst[k][1] = max(worst[k][1], rf[n])
    return worst


def test_the_constants_are_four_times_the_measured_ratios():
    print(f"{'output':<9} {'bf16-kernel restatement':>24} {'fp32-twin restatement':>22} {'4 x worst':>10} {'K':>6}")
    for k, (b, f) in _unit_ratios().items():
        four = 4 * max(b, f)
        want = 2.0 ** math.ceil(math.log2(four))
        print(f"{k:<9} {b:>24.3f} {f:>22.3f} {four:>10.2f} {L.K[k]:>6g}")
        assert math.isfinite(four) and L.K[k] == want, f"K[{k!r}] is {L.K[k]}, measured 4 x {max(b, f):.3f} -> {want}"


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_honest_restatements_stay_within_a_quarter_of_the_bound(i):
    c = CASES[i]
    b, f_exact, f_bf = _honest(i)
    rb = L.check(c, b, what="bf16-kernel restatement")
    print(f"{c.name}: bf16-kernel restatement: " + ", ".join(f"{k} {v:.3f}" for k, v in rb.items()))
    assert all(v <= 0.25 for k, v in rb.items() if k != "dlogits"), rb     # (dlogits: bf16 rounding of the reference alone reaches ~1)
    for out, exact_values in ((f_exact, True), (f_bf, False)):
        rf = L.check(c, out, fp32_mode=True, fp32_values=exact_values, what="fp32-twin restatement")
        print(f"{c.name}: fp32-twin restatement on {'fp32' if exact_values else 'bf16'} values: " + ", ".join(f"{k} {v:.3f}" for k, v in rf.items()))
        assert all(v <= 0.25 for v in rf.values()), rf


def test_the_all_ignored_batch_is_exact_zero():
    c = L.all_ignored_case()
    out = L.restate_bf16(c)
    r = L.check(c, out)
    assert out["stats"].tolist() == [0.0, 0.0] and r["stats[0]"] == 0 and r["dlogits"] == 0


@functools.lru_cache(maxsize=None)
def _rejections(mut):
    hit = []
    for c in CASES:
        try:
            L.check(c, L.restate_bf16(c, mut))
        except AssertionError as e:
            hit.append((c.name, str(e)))
    return hit


@pytest.mark.parametrize("mut", L.MUTANTS)
def test_every_mutant_is_rejected(mut):
    hit = _rejections(mut)
    print(f"{mut}: rejected by {len(hit)} of {len(CASES)} cases")
    for name, why in hit:
        print(f"  {name}: {why[why.index(name) + len(name) + 2:][:230]}")
    assert hit, f"the mutant '{mut}' passes every case"


def test_the_cases_are_the_ones_the_kernels_can_go_wrong_at():
    assert {c.V for c in CASES} == set(L.VOCABS) and all(c.ld == L.round_up(c.V, 128) and c.ld > c.V for c in CASES)
    assert {c.rows for c in CASES if c.V < 51865} == {1, 50, 600} and all(c.rows <= 8 for c in CASES if c.V >= 51865)
    assert {(c.V, c.rows) for c in CASES if c.rows == 600} == {(1000, 600), (2051, 600)}
    assert {c.eps for c in CASES} == {0.0, 0.05, 0.1} and {c.gscale for c in CASES} == {1.0, 0.25}
    assert max(c.x.numel() for c in CASES) <= 600 * 2176
    for c in CASES:
        ref = L.case_reference(c)
        assert (c.x[:, c.V:] == L.POISON).all() and c.x[:, :c.V].max() < L.POISON and torch.isfinite(c.x).all()
        if c.rows > 1:   # every kind of the vocabulary size in every multi-row case, and every tie planted where it says
            kinds = set(L.VALUE_KINDS) | {f"tie: {n}" for n, _, _ in L.tie_pairs(c.V)}
            assert set(c.kinds) <= kinds and (c.rows < len(kinds) or set(c.kinds) == kinds)
        ties = {f"tie: {n}": (a, b) for n, a, b in L.tie_pairs(c.V)}
        for r, kind in enumerate(c.kinds):
            if kind in ties:
                a, b = ties[kind]
                assert c.x[r, a] == c.x[r, b] == c.x[r, :c.V].max() and ref["argmax"][r] == a and (c.x[r, :c.V] == c.x[r, a]).sum() == 2
            if r % 7 == 6:
                assert c.targets[r] == L.IGNORE
    for V in (51865, 51866):   # the placements the tie mutants need: different threads / lanes / waves, crossed ones included
        own = {n: (L.owner(a, V), L.owner(b, V)) for n, a, b in L.tie_pairs(V)}
        assert own["columns i, i + 1 of one 8-vector"][0] == own["columns i, i + 1 of one 8-vector"][1]
        a, b = own["one in-vector position, two lanes of a wave"]
        assert a != b and a >> 6 == b >> 6
        a, b = own["two waves"]
        assert a >> 6 < b >> 6
        a, b = own["two waves, crossed"]
        assert a >> 6 > b >> 6
        a, b = own["two lanes, crossed"]
        assert a >> 6 == b >> 6 and a > b
        a, b = own["vector part and tail, one thread"]
        assert a == b
