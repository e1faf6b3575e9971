"""CPU proof that the per-element bounds of the optimizer-kernel tests bite (tests/_optim_cases.py, applied to the kernels by
tests/test_optim_gpu.py).  No kernel runs here: the arithmetic of wft_mt_adamw, wft_mt_sumsq_f32, wft_muon_momentum_mt,
wft_muon_prepare and wft_muon_apply_mt is restated in torch CPU float32, in the kernels' order of operations, and judged by the same
checkers as the kernels, against the same float64 references.

  * The constants K are 4 x the worst ratio |restatement - reference| / F the honest restatements reach over all cases, in every
    form the compiler may give a * b + c (rounded product, or an fma either way round), rounded up to a power of two:
    test_the_constants_are_four_times_the_measured_ratios prints the table that the helper's docstring holds and asserts that K is
    that number and that the docstring holds the table.  The bound of wft_muon_prepare has no constant: it is derived.
  * The honest restatements stay within a quarter of every bound, keep every sentinel and pass every exact assertion.
  * Every mutant of O.MUTANTS is rejected by at least one case; which ones is printed.
"""
import functools
import math

import pytest
import torch

from tests import _optim_cases as O

ONES = dict.fromkeys(O.K, 1.0)
INF = math.inf


def _honest_runs():
    """(checker call, restatement call) of every case and form"""
    for c in O.adam_cases():
        for f in O.FORMS:
            yield functools.partial(O.check_adam_case, c), functools.partial(O.restate_mt_adamw, c, f)
    for tb in "AB":
        for f in (0, 1):
            yield functools.partial(O.check_mt_sumsq, tb), functools.partial(O.restate_mt_sumsq, tb, f)
    for c in O.mom_cases():
        for f in (0, 1):
            for null in (True, False):
                yield functools.partial(O.check_momentum, c, null=null), functools.partial(O.restate_momentum, c, f, null=null)
    for c in O.apply_cases():
        for f in O.FORMS:
            yield functools.partial(O.check_apply, c), functools.partial(O.restate_apply, c, f)


@functools.lru_cache(maxsize=None)
def _unit_ratios():
    """{output: worst ratio at K = 1 of the honest restatements}; every exact assertion of the checkers holds on the way"""
    worst = dict.fromkeys(O.K, 0.0)
    for check, restate in _honest_runs():
        for k, v in check(restate(), k=ONES, limit=INF).items():
            if k in worst:
                worst[k] = max(worst[k], v)
    return worst


def _table():
    return [f"  {k:<9} {r:<32.3f} {4 * r:<11.2f} {O.K[k]:g}" for k, r in _unit_ratios().items()]


def test_the_constants_are_four_times_the_measured_ratios():
    print("  output    worst ratio of the restatement   4 x worst   K")
    print("\n".join(_table()))
    for k, r in _unit_ratios().items():
        want = 2.0 ** math.ceil(math.log2(4 * r))
        assert math.isfinite(r) and O.K[k] == want, f"K[{k!r}] is {O.K[k]}, measured 4 x {r:.3f} -> {want}"
    for line in _table():
        assert line.rstrip() in O.__doc__, f"the docstring of _optim_cases.py does not hold the measured line\n{line}"


def test_the_honest_restatements_stay_within_a_quarter_of_the_bound():
    for k, r in _unit_ratios().items():
        assert r <= O.K[k] / 4, (k, r)
    worst = 0.0
    for c in O.prep_cases():   # the derived bound of prepare: half an ulp of bf16 + 4u |q|, of which the rounding alone can take the half ulp
        worst = max(worst, O.check_prepare(c, O.restate_prepare(c))["X"])
    print(f"prepare: X against half an ulp of bf16 + 4u |q|: worst {worst:.4f}")
    assert worst <= 1.0
    for c in O.mom_cases():    # U of the NULL row, bf16 of a u nobody wrote: half an ulp + K F
        assert O.check_momentum(c, O.restate_momentum(c))["U of the NULL row"] <= 1.0


def test_the_exact_assertions_hold_on_the_restatement():
    """what tests/test_optim_gpu.py asserts bit for bit, on the restatement: a coefficient >= 1 (sumsq = 0 included) gives the bits
    of the launch without sumsq; a NULL gradient row gives the buf, U and partial of an all-zero gradient"""
    for tb in "AB":
        for hp in (0, 4):
            plain = O.restate_mt_adamw(O.AdamCase(tb, hp, 0))
            for clip in (2, 3):
                out = O.restate_mt_adamw(O.AdamCase(tb, hp, clip))
                assert all(torch.equal(O.bits(out[a]), O.bits(plain[a])) for a in "pmv")
    for c in O.mom_cases():
        a, b = O.restate_momentum(c, null=True), O.restate_momentum(c, null=False)
        assert all(torch.equal(O.bits(a[k]), O.bits(b[k])) for k in ("buf", "U", "partial"))


# ------------------------------------------------------------------------------------------------ mutants
def _mutant_runs(family, mut):
    """(case name, checker call, mutated restatement call) of the cases a mutant of this family is judged on"""
    if family == "adamw":
        for c in (c for c in O.adam_cases() if c.table == "B" or c.hp == 0):   # table A (400 000 elements) at the first set only
            yield c.name, functools.partial(O.check_adam_case, c), functools.partial(O.restate_mt_adamw, c, 0, mut)
    elif family == "sumsq":
        for tb in "AB":
            yield f"table {tb}", functools.partial(O.check_mt_sumsq, tb), functools.partial(O.restate_mt_sumsq, tb, 0, mut)
    elif family == "momentum":
        for c in O.mom_cases():
            yield c.name, functools.partial(O.check_momentum, c), functools.partial(O.restate_momentum, c, 0, mut)
    elif family == "prepare":
        for c in O.prep_cases():
            yield c.name, functools.partial(O.check_prepare, c), functools.partial(O.restate_prepare, c, mut)
    else:
        for c in O.apply_cases():
            yield c.name, functools.partial(O.check_apply, c), functools.partial(O.restate_apply, c, 0, mut)


ALL_MUTANTS = tuple((fam, m) for fam, muts in O.MUTANTS.items() for m in muts)


@pytest.mark.parametrize("family,mut", ALL_MUTANTS, ids=[f"{f}: {m}" for f, m in ALL_MUTANTS])
def test_every_mutant_is_rejected(family, mut):
    hit, n = [], 0
    for name, check, restate in _mutant_runs(family, mut):
        n += 1
        try:
            check(restate())
        except AssertionError as e:
            hit.append((name, str(e)))
    print(f"{family}: {mut}: rejected by {len(hit)} of {n} cases")
    for name, why in hit:
        print(f"  {name}: {why[why.index(name) + len(name) + 2:][:230]}")
    assert hit, f"the mutant '{mut}' passes every case"


def test_the_mutants_are_the_listed_ones():
    assert {f: len(m) for f, m in O.MUTANTS.items()} == {"adamw": 12, "sumsq": 4, "momentum": 6, "prepare": 6, "apply": 4}


def test_the_cases_are_the_ones_the_kernels_can_go_wrong_at():
    numels, lay = O.adam_table("A")
    assert numels == (3, 8, 1001, 65536, 65537, 70001, 2 * 65536 + 5) and O.chunk_starts(numels)[-1] == 11
    off = [tuple(lay[a].starts[t] % 4 for a in "pgmv") for t in range(7)]
    assert [sum(1 for x in o if x) for o in off] == [1, 1, 1, 0, 1, 0, 0]                      # exactly one pointer unaligned, four times,
    assert {o.index(max(o)) for o in off if any(o)} == {0, 1, 2, 3}                            # each of p, g, m, v once,
    assert {max(o) for o in off if any(o)} == {1, 2}                                           # 4 or 8 bytes off
    for a in "pgmv":                                                                           # at least 64 sentinels on every side
        ends = [0] + sorted((s, s + n) for s, n in zip(lay[a].starts, numels)) + [lay[a].length]
        flat = [ends[0]] + [x for se in ends[1:-1] for x in se] + [ends[-1]]
        assert all(flat[i + 1] - flat[i] >= O.GUARD for i in range(0, len(flat), 2))
    numels, lay = O.adam_table("B")
    assert numels == tuple(1 + i % 7 for i in range(300)) and O.chunk_starts(numels)[-1] == 300
    for tb in "AB":
        inp = O.adam_inputs(tb)
        k = inp["kind"]
        assert set(k.tolist()) == set(range(8)) and all(torch.isfinite(inp[a]).all() for a in "pgmv")
        assert (inp["g"][(k == 1) | (k == 2)] == 0).all() and (inp["m"][(k == 2) | (k == 3)] == 0).all() and (inp["v"][(k == 2) | (k == 3)] == 0).all()
        assert (inp["p"][k == 6] == 0).all() and inp["p"][k == 7].abs().min() >= 1e3 and inp["v"][k == 5].min() >= 5e3
        assert (inp["v"] >= 0).all()
    # kind 7: the update is below half an ulp of p (weight_decay 0: the reference moves p by less than 2^-25 |p|)
    ref = O.adam_reference(O.adam_inputs("A"), O.adam_scalars(O.ADAM_HP[2]))
    k7 = O.adam_inputs("A")["kind"] == 7
    assert ((ref["p"] - O.adam_inputs("A")["p"].double()).abs()[k7] < 2.0 ** -25 * 1e3).all()
    coef = [O.clip_coefficient(c)[0] if c else None for c in O.CLIPS]
    assert coef[0] is None and abs(coef[1] - 0.37) < 1e-3 and coef[2] == coef[3] == 1.0 and abs(coef[4] - 0.5) < 1e-3
    assert abs(O.f32(1e-6) / (math.sqrt(O.f32(1e-10)) + O.f32(1e-6)) - 1 / 11) < 1e-3         # the + 1e-6 is a tenth of the norm
    # sums of squares: two NULL rows and two unaligned gradients in table A, 300 partials in table B (the strided final loop)
    numels, lay = O.sumsq_table("A")
    assert len(O.SUMSQ_NULL["A"]) == 2 and sum(1 for s in lay.starts if s % 4) == 2 and len(O.chunk_list(O.B_NUMELS)) == 300 > 256
    g = O.sumsq_inputs("A")[lay.offsets[6] + O.CHUNK:lay.offsets[6] + 2 * O.CHUNK]
    assert (g == 1e4).sum() == 1 and (g == O.f32(1e-4)).sum() == O.CHUNK - 1
    # momentum: one chunk, one chunk minus one element, exactly one chunk, two chunks with a tail of 24 464
    assert [(c.numel, c.chunks) for c in O.mom_cases()[::4]] == [(5120, 1), (65535, 1), (65536, 1), (90000, 2)] and 90000 - 65536 == 24464
    # prepare: every s and every chunk count occurs, tall, wide and square shapes, partial sums exact
    pc = O.prep_cases()
    assert {c.chunks for c in pc} == {1, 2, 300} and {s for c in pc for s in c.s} == {2.25, 2.0, 2.0 ** -40, 0.0}
    assert any(c.tall for c in pc) and any(c.rows == c.cols for c in pc) and all(c.s[0] != c.s[1] for c in pc)
    for c in pc:
        for t in (0, 1):
            part = O.prep_inputs(c)["partial"][t]
            assert float(part.double().sum()) == c.s[t] == float(O.final_sum(part)) == float(part.flip(0).sum())
    # apply: ldo > cols and stride_o larger than rows x ldo
    assert all(c.frame[1] > c.cols and c.frame[0] * c.frame[1] > c.rows * c.frame[1] for c in O.apply_cases())
