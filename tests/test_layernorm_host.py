"""CPU proof that the per-element bounds of the LayerNorm tests bite (tests/_layernorm_cases.py check, applied to the kernels by
tests/test_layernorm_gpu.py).  No kernel runs here: the kernels' arithmetic is restated in torch CPU float32, in their order of
operations, and judged by the same checker as the kernels, against the same float64 reference.

  * The constants K of the bounds are 4 x the worst ratio |restatement - reference| / F the two honest restatements reach over all
    cases (every case of bf16_cases() and f32_cases(); a span (d) case masks nothing, so its restatement is the plain case's and is
    not run twice), rounded up to a power of two: test_the_constants_are_four_times_the_measured_ratios prints the table that the
    helper's docstring holds and asserts that K is that number and that the docstring holds the table.
  * The honest restatements stay within a quarter of the bound (y and dx of the bf16 mode: the fp32 value before its rounding within
    a quarter of the fp32 term K F; the rounded value within the whole bound, of which bf16 round-to-nearest of the reference alone
    can take all but K F).
  * Every mutant of N.MUTANTS is rejected by at least one case of width 264 (NQ = 2, two pieces in the last pass) up to 2051 rows;
    which ones is printed.  The mutants of the masked positions run on the span cases, the others on the plain ones.
"""
import functools
import math

import pytest
import torch

from tests import _layernorm_cases as N

BF = tuple(c for c in N.bf16_cases() if c.span != "d")
F32 = N.f32_cases()
ONES = dict.fromkeys(N.K, 1.0)
MEASURED = {"y": "y_f32", "mean": "mean", "rstd": "rstd", "dx": "dx_f32", "dgamma": "dgamma", "dbeta": "dbeta", "dxsum": "dxsum"}


def _ref_f32(c, exact):
    return N.reference({**N.inputs(c, exact), "dres": None}, c.mask)


@functools.lru_cache(maxsize=None)
def _unit_ratios():
    """-> {output: [worst ratio at K = 1 of the bf16-kernel restatement, of the fp32-twin restatement]} over all cases, and the
    worst ratio of the rounded y and dx against half an ulp of bf16 + 1 F"""
    worst = {k: [0.0, 0.0] for k in N.K}
    rounded = 0.0
    for c in BF:
        out = N.restate_bf16(c)
        ref = N.reference(N.inputs(c), c.mask)
        big = c.rows * c.cols > 1 << 20   # (the rounded y and dx, bf16 round-to-nearest of the values judged anyway: the smaller cases)
        r = N.check(c.name, ref, out, N.depth_bf16(c.rows), k=ONES, limit=math.inf, skip=("y", "dx") if big else ())
        for k, name in MEASURED.items():
            worst[k][0] = max(worst[k][0], r[name])
        rounded = max(rounded, r.get("y", 0), r.get("dx", 0))   # against half an ulp + 1 F: no looser than half an ulp + K F
    for c in F32:
        for exact in (True, False):
            r = N.check(c.name, _ref_f32(c, exact), N.restate_f32(c, exact), c.rows, fp32_mode=True, k=ONES, limit=math.inf)
            for k, v in r.items():
                worst[k][1] = max(worst[k][1], v)
    return worst, rounded


def _table():
    lines = []
    for k, (b, f) in _unit_ratios()[0].items():
        lines.append(f"  {k:<8} {b:<37.3f} {f'{f:.3f}' if k != 'dxsum' else '-':<35} {4 * max(b, f):<11.2f} {N.K[k]:g}")
    return lines


def test_the_constants_are_four_times_the_measured_ratios():
    print("  output   worst ratio bf16-kernel restatement   worst ratio fp32-twin restatement   4 x worst   K")
    print("\n".join(_table()))
    for k, (b, f) in _unit_ratios()[0].items():
        four = 4 * max(b, f)
        want = 2.0 ** math.ceil(math.log2(four))
        assert math.isfinite(four) and N.K[k] == want, f"K[{k!r}] is {N.K[k]}, measured 4 x {max(b, f):.3f} -> {want}"
    for line in _table():
        assert line.rstrip() in N.__doc__, f"the docstring of _layernorm_cases.py does not hold the measured line\n{line}"


def test_the_honest_restatements_stay_within_a_quarter_of_the_bound():
    worst, rounded = _unit_ratios()
    for k, (b, f) in worst.items():
        assert max(b, f) <= N.K[k] / 4, (k, b, f)
    print(f"rounded y and dx of the bf16-kernel restatement against half an ulp + K F: worst {rounded:.3f}")
    assert rounded <= 1.0


MUT_PLAIN = tuple(c for c in N.bf16_cases() if c.cols == 264 and c.rows <= 2051 and not c.span)
MUT_SPAN = tuple(c for c in N.bf16_cases() if c.cols == 264 and c.rows <= 2051 and c.span)
SPAN_MUTANTS = tuple(m for m in N.MUTANTS["masked positions and reduce"] if m != "short last reduce chunk skipped")


@functools.lru_cache(maxsize=None)
def _small_ref(c):
    return N.reference(N.inputs(c), c.mask)


def _rejections(mut):
    hit = []
    cases = MUT_SPAN if mut in SPAN_MUTANTS else MUT_PLAIN
    for c in cases:
        try:
            N.check(c.name, _small_ref(c), N.restate_bf16(c, mut), N.depth_bf16(c.rows))
        except AssertionError as e:
            hit.append((c.name, str(e)))
    return hit, len(cases)


def test_the_unmutated_restatement_passes_the_mutant_cases():
    for c in MUT_PLAIN + MUT_SPAN:
        N.check(c.name, _small_ref(c), N.restate_bf16(c), N.depth_bf16(c.rows))


@pytest.mark.parametrize("mut", N.ALL_MUTANTS)
def test_every_mutant_is_rejected(mut):
    hit, n = _rejections(mut)
    print(f"{mut}: rejected by {len(hit)} of {n} cases")
    for name, why in hit:
        print(f"  {name}: {why[why.index(name) + len(name) + 2:][:230]}")
    assert hit, f"the mutant '{mut}' passes every case"


def test_the_cases_are_the_ones_the_kernels_can_go_wrong_at():
    bf = N.bf16_cases()
    plain = {(c.rows, c.cols) for c in bf if not c.span}
    assert {c for _, c in plain} == set(N.WIDTHS) and {(c + 255) // 256 for c in N.WIDTHS} == set(range(1, 9))
    assert all((5, c) in plain and (1029, c) in plain for c in N.WIDTHS)
    assert all((r, c) in plain for c in N.SPAN_WIDTHS for r in (1, 3, 1024, 2051, 8197))
    for c in N.SPAN_WIDTHS:
        for r, rpb in N.SPAN_ROWS:
            got = {k.span: k.mask for k in bf if k.span and (k.rows, k.cols) == (r, c)}
            assert got == N.spans(rpb, c) and (r % rpb != 0 or rpb == 7)   # a short last batch at rows_per_batch 1500 (1029 = 147 x 7)
    # the dispatch the row counts aim at (csrc/norm.hip)
    assert N.fold_levels(1024) == (256,) and N.fold_levels(1029) == (17, 16) and N.bwd_grid(1029) == 258 and 258 - 15 * 17 == 3
    assert N.bwd_grid(2051) == 512 and 2051 - 4 * 512 == 3 and 8197 > N.FWD_WAVES_MAX
    assert {c.cols for c in F32} == set(N.F32_COLS) and {c.rows for c in F32} == set(N.F32_ROWS)
    assert {c.span for c in F32} == {"", "a", "b", "e"}
    for c in (k for k in bf if k.rows == 1029 and not k.span):   # every kind in every multi-row case, the kinds as described
        x, dy = N.inputs(c)["x"], N.inputs(c)["dy"]
        kind = (torch.arange(c.rows) + c.offset) % 8
        assert set(kind.tolist()) == set(range(8)) and torch.equal(N._bfq(x), x) and torch.equal(N._bfq(dy), dy)
        assert (x[kind == 2] == 2.5).all() and (x[kind == 5][:, -1] == 200).all() and (dy[kind == 6] >= 0).all()
        assert x[kind == 3].mean() > 250 and x[kind == 4].abs().max() < 2.0 ** -7
