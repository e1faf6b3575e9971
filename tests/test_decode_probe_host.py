"""CPU proof that the per-(row, head) bound of the decode probe tests bites (tests/test_decode_kernels_gpu.py close_per_head at
PER_HEAD_TOL = 2^-7, used on the GPU by tests/test_decode_probe_gpu.py): on the probe operands of every GPU case the fp32-softmax ->
bf16 emulation of CORRECT single-token attention passes it, and the emulation of each way csrc/decode_attn.hip's dealing can lose,
leak or double-count a key (tests/_decode_probe.py mutants) fails it on every (row, head) whose targets or decoys the fault concerns.
Only arithmetic on the CPU: no kernel runs here, right or wrong.

Neither number is measured from a kernel.  The correct emulation must stay within 2^-8 x 1.01 of each head's own largest fp64
value: one rounding of the output to bf16 (half an ulp of the largest element), which the bound doubles.  Every touched (row, head)
of every mutant must lie at least 4 x 2^-7 off: the mildest fault, a target counted twice, turns (v_a + v_b) / 2 into
(2 v_a + v_b) / 3 and moves the row by |v_a - v_b| / 6.  As built (seed 0): the targets hold >= 0.9990 of every (row, head)'s
mass, each >= 0.4995, a decoy would take >= 0.3331; the correct emulation reaches 3.86e-3 at worst; the mildest touched (row, head)
of any mutant lies 0.164 off (a split's partial merged twice), a lost target 0.46 or more.

"Touched" (tests/_decode_probe.py touched): the (row, head) pairs whose own targets or decoys the fault concerns.  A wave dropped
from a row whose two targets live in other waves removes background keys alone, 1e-3 of the row, and no bound on a bf16 output
could see it: the edge keys are dealt so that some (row, head) of the case has a target there, and the last block of the test
asserts that every mutant the form and the split have did touch one.
"""
import math

import pytest
import torch

from tests import _decode_probe as P
from tests.test_decode_kernels_gpu import PER_HEAD_TOL, close_per_head


def _ratios(got, ref, H):
    R = ref.shape[0]
    return (got.double() - ref).abs().view(R, H, 64).amax(-1) / ref.abs().view(R, H, 64).amax(-1)


@pytest.mark.parametrize("case", P.CASES, ids=P.IDS)
def test_the_per_head_bound_passes_correct_attention_and_fails_every_mutant(case):
    case_id, pre = case
    worst, lowest, names = 0.0, {}, set()
    calls = P.calls(case_id, pre)
    for i, c in enumerate(calls):
        ref = P.oracle(c)
        lists64 = P.emulate(c, dtype=torch.float64)   # the key lists restate the oracle's gathered cache
        assert (lists64 - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
        two = c.tgt[..., 0] != c.tgt[..., 1]
        _, vp = c.pools(torch.float64)
        half = torch.stack([torch.stack([vp[c.keys(r, c.tgt[r, h]), h].mean(0) for h in range(c.H)]) for r in range(c.R)])
        assert ((ref.view(c.R, c.H, 64) - half).abs().amax(-1) <= 1e-2 * half.abs().amax(-1))[two].all(), "a row is not (v_a + v_b) / 2"
        good = P.emulate(c)
        ratio = close_per_head(good, ref, PER_HEAD_TOL, f"{case_id} pre={pre} call {i}: correct fp32 -> bf16")
        worst = max(worst, ratio.max().item())
        for name, m in P.mutants(c).items():
            hit = P.touched(c, **m)
            if not hit.any():
                continue
            names.add(name)
            bad = P.emulate(c, **m)
            r = _ratios(bad, ref, c.H)[hit]
            lowest[name] = min(lowest.get(name, math.inf), r.min().item())
            with pytest.raises(AssertionError):
                close_per_head(bad, ref, PER_HEAD_TOL, name)
    mass = {k: min(c.mass[k] for c in calls) for k in calls[0].mass}
    print(f"{case_id} pre={pre}: {len(calls)} call(s) of {calls[0].R} rows at {calls[0].nsplit} split(s); targets hold >= {mass['targets']:.4f} "
          f"of every (row, head)'s mass, each >= {mass['each']:.4f}, a decoy would take >= {mass['decoy']:.4f}")
    print(f"correct emulation, worst (row, head) ratio {worst:.3e} (must be <= 2^-8 x 1.01 = {2.0 ** -8 * 1.01:.3e})")
    assert worst <= 2.0 ** -8 * 1.01
    for name in sorted(lowest):
        print(f"  {name:<52} smallest touched (row, head) ratio {lowest[name]:.3e}")
        assert lowest[name] >= P.MUTANT_MIN, f"{name}: a touched (row, head) lies only {lowest[name]:.3e} off (need {P.MUTANT_MIN:.3e})"
    # every mutant the form and the split have must have touched something
    c = calls[0]
    want = {"n + 1: the guard decoy admitted"}
    if max(max(c.lens) for c in calls) > 1:
        want |= {"target a lost", "target b lost", "n - 1"}
    if c.self_form:
        want |= {"stale cache row at len - 1, k and v", "stale cache row at len - 1, v only"}
    if any(n % P.BLOCK for c in calls for n in c.lens) and max(max(c.lens) for c in calls) > 1:
        want.add("the clamped tail counted")
    blocks = max(-(-n // P.BLOCK) for c in calls for n in c.lens)
    # (the reduced edge set of the 16-split cases — multiples of 128 and the key before — has keys in waves 0 and 3 alone; waves 1
    # and 2 run the same code at every split and meet their targets in the cases of 1, 2 and 3 splits)
    seam = P.SPEC[case_id].get("seam", P.BLOCK)
    want |= {f"wave {e // P.BLOCK % P.WAVES}'s blocks dropped" for c in calls for n in set(c.lens) for e in P.edge_keys(n, seam) if blocks > 1}
    if c.nsplit > 1:
        live = min(c.nsplit, -(-blocks // P.WAVES))
        want |= {f"split {s}'s partial dropped" for s in range(live)} | {f"split {s}'s partial merged twice" for s in range(live)}
    if c.form == "beam_self":
        want |= {"anc ignored: own slot read", "the indices of block j + stride used for block j"}
    if c.form == "beam_cross":
        want |= {"the next audio's cache read"} if c.S > 1 else set()
        want |= {"a group's queries all attend with row 0's q"} if c.group > 1 else set()
    assert want <= names, f"mutants that touched no (row, head): {sorted(want - names)}"


@pytest.mark.parametrize("pre", [False, True])
def test_the_clamp_case_meets_the_mass_conditions_and_the_bound(pre):
    c = P.clamp_case(pre)   # (the builder asserts the three mass conditions)
    ratio = close_per_head(P.emulate(c), P.oracle(c), PER_HEAD_TOL, f"clamp case pre={pre}: correct fp32 -> bf16")
    assert ratio.max().item() <= 2.0 ** -8 * 1.01
    hit = P.touched(c, **P.mutants(c)["n + 1: the guard decoy admitted"])
    assert hit.all()   # a row that runs one key over meets its decoy in every head


def test_every_case_of_the_table_is_present():
    ids = [s["id"] for s in P.SPECS]
    assert len(ids) == len(set(ids))
    seen = {(s["form"], s["nsplit"]) for s in P.SPECS}
    assert {("self", 1), ("self", 2), ("self", 3), ("cross", 1), ("cross", 2), ("cross", 3), ("cross", 16), ("beam_cross", 1),
            ("beam_cross", 3), ("beam_cross", 16), ("beam_self", 1), ("beam_self", 3)} <= seen
    assert {s["group"] for s in P.SPECS if s["form"] == "beam_cross" and s["cap"] == 500} == set(range(1, 9))
    assert {s["group"] for s in P.SPECS if s["form"] == "beam_cross" and s["cap"] == 1500} == set(range(1, 9))
    assert ("7-cross-H2-B1-Tk7700-split16", True) not in P.CASES and ("7-cross-H2-B1-Tk7700-split16", False) in P.CASES
    three = P.calls("3-self-H2-cap1100-split3", False)
    assert all(c.R <= 42 for c in three) and any(min(c.lens) <= 128 and max(c.lens) > 1024 for c in three)   # empty partials next to full ones
    assert len(P.calls("8-beamcross-H2-A1-g8-Tk7700-split16", False)) == 4
