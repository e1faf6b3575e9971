"""CPU proof that the per-element checks of the 8-bit AdamW kernel bite (tests/_adam8_cases.py, applied to wft_mt_adamw8 by
tests/test_adam8_gpu.py).  No kernel runs here: the kernel's arithmetic is restated in torch CPU float32, in its order of operations,
and judged by the same checker as the kernel, against the same float64 reference.

  * The constants K are 4 x the worst ratio |restatement - reference| / F the honest restatement reaches over all cases, in every form
    the compiler may give a * b + c, rounded up to a power of two: test_the_constants_are_four_times_the_measured_ratios prints the
    table that the helper's docstring holds and asserts that K is that number and that the docstring holds the table.
  * The checker accepts every form of every case; in stages 1 to 3 the three forms give the same codes and absmax bit for bit (the
    arithmetic is exact), so the kernel's codes are held to equality there whatever the compiler contracted.
  * At most 1e-3 of a stage-4 case's elements lie near a midpoint, and no band holds two midpoints.
  * Every mutant of A.MUTANTS is rejected by at least one case; which ones is printed.
"""
import functools
import math

import pytest
import torch

from tests import _adam8_cases as A

@functools.lru_cache(maxsize=None)
def _honest():
    """every case x form once -> (worst ratios at K = 1, [(case, form, what the checker said)], [(case, form) whose codes or absmax
    differ from form 0 in an exact stage], {case: stats of form 0})"""
    worst, refused, moved, stats = dict.fromkeys(A.K, 0.0), [], [], {}
    for c in A.all_cases():
        ref = A.reference(c)
        first = None
        for f in A.FORMS:
            out = A.restate_mt_adamw8(c, f)
            got = {a: c.lay[a].gather(out[a]) for a in ("p", "a1", "a2")}
            r = {"n1": A.ratio(got["a1"], ref["n1"], ref["F"]["n1"]), "n2": A.ratio(got["a2"], ref["n2"], ref["F"]["n2"]),
                 "p": A.ratio(got["p"], ref["p"], ref["F"]["p"]), **A.measure_x(c, out, ref)}
            for k, v in r.items():
                worst[k] = max(worst[k], v)
            try:
                st = A.check_adam8(c, out, ref=ref)
                if f == 0:
                    stats[c.name] = st
            except AssertionError as e:
                refused.append((c.name, f, str(e)))
            if c.exact is not None:
                keep = {a: out[a] for a in ("s1", "s2", "a1", "a2")}
                if first is None:
                    first = keep
                elif not all(torch.equal(A.bits(keep[a]) if a[0] == "a" else keep[a], A.bits(first[a]) if a[0] == "a" else first[a]) for a in keep):
                    moved.append((c.name, f))
    return worst, refused, moved, stats


def _table():
    return [f"  {k:<9} {r:<32.3f} {4 * r:<11.2f} {A.K[k]:g}" for k, r in _honest()[0].items()]


def test_the_constants_are_four_times_the_measured_ratios():
    print("  output    worst ratio of the restatement   4 x worst   K")
    print("\n".join(_table()))
    for k, r in _honest()[0].items():
        want = 2.0 ** math.ceil(math.log2(4 * r))
        assert math.isfinite(r) and A.K[k] == want, f"K[{k!r}] is {A.K[k]}, measured 4 x {r:.3f} -> {want}"
    for line in _table():
        assert line.rstrip() in A.__doc__, f"the docstring of _adam8_cases.py does not hold the measured line\n{line}"


def test_the_checker_accepts_every_form_of_every_case():
    _, refused, _, stats = _honest()
    for name, st in stats.items():
        print(f"{name}: " + ", ".join(f"{k} {v:.3g}" for k, v in st.items()))
    assert not refused, "\n".join(f"{n}, form {f}: {why[:300]}" for n, f, why in refused)
    assert len(stats) == len(A.all_cases()) == 4 + len(A.STAGE4)


def test_the_forms_agree_bit_for_bit_in_stages_1_to_3():
    _, _, moved, _ = _honest()
    assert not moved, f"codes or absmax depend on the contraction in {moved}"
    assert [c.stage for c in A.exact_cases()] == [1, 2, 3, 3] and all(c.exact is not None for c in A.exact_cases())


def test_few_elements_are_near_a_midpoint_and_the_float32_codes_seldom_differ():
    """the 1e-3 cap for the reference inputs alone (no restatement takes part); the restatement's codes leave the float64 ones seldom
    and never outside the band (that is test_the_checker_accepts_every_form_of_every_case)"""
    for k in range(len(A.STAGE4)):
        c = A.stage4_case(k)
        ref = A.reference(c)
        for key in ("1", "2"):
            lo, hi, near = A.code_band(ref, key, A.K["x" + key])
            share = float(near.double().mean())
            print(f"{c.name}: state{key}: {int(near.sum())} of {near.numel()} elements near a midpoint ({share:.2e})")
            assert share <= A.NEAR_CAP and bool((hi - lo <= 1).all())
            n = ref["n" + key]
            assert bool(((n == 0) | (n >= 2.0 ** -126)).all()) and bool(torch.isfinite(n).all()), "an absmax outside the normal range"
    st = _honest()[3]
    for c in A.all_cases():
        if c.stage == 4:
            total = sum(c.numels)
            assert st[c.name]["diff1"] <= 1e-3 * total and st[c.name]["diff2"] <= 1e-3 * total


# ------------------------------------------------------------------------------------------------ mutants
@functools.lru_cache(maxsize=None)
def _mutant_cases():
    """the exact stages and six stage-4 cases (table A, 345 100 elements, once; every hyper-parameter set, step and clip, and the first
    step, on table B): each with its reference"""
    cases = list(A.exact_cases()) + [A.stage4_case(k) for k in (4, 11, 12, 13, 16, 19)]
    return tuple((c, A.reference(c)) for c in cases)


@pytest.mark.parametrize("mut", A.MUTANTS)
def test_every_mutant_is_rejected(mut):
    hit, n = [], 0
    for c, ref in _mutant_cases():
        if mut == "last chunk at the full count" and c.numels == A.B_NUMELS:
            continue   # (300 chunks of 65 536 lanes each; the other tables show it)
        n += 1
        try:
            A.check_adam8(c, A.restate_mt_adamw8(c, 0, mut), ref=ref)
        except AssertionError as e:
            hit.append((c.name, str(e)))
    print(f"{mut}: rejected by {len(hit)} of {n} cases, stages {sorted({int(n[6]) for n, _ in hit})}")
    for name, why in hit:
        print(f"  {name}: {why[len(name) + 2:][:230]}")
    assert hit, f"the mutant '{mut}' passes every case"


def test_the_mutants_are_the_listed_ones():
    assert len(A.MUTANTS) == len(set(A.MUTANTS)) == 20


# ------------------------------------------------------------------------------------------------ the cases themselves
def test_stage_1_probes_get_the_codes_they_were_built_for():
    pr = A.stage1_probes()
    q1, q2 = A.real_maps()
    print(f"stage 1: {pr[1][0].numel()} probes of state1, {pr[2][0].numel()} of state2; no float32 g gives fl32(g g) equal to "
          f"{pr['unreachable'][0]} of the 255 midpoints and {pr['unreachable'][1]} of the 256 entries of qmap2")
    assert pr[1][0].numel() == 2 + 256 + 3 * 255 - 1 and pr[1][0].numel() % 8 and pr[2][0].numel() % 8 and pr[2][0].numel() <= A.BLOCK
    assert float(pr[1][0].abs().max()) == 1.0 and float(pr[2][0].abs().max()) == 1.0
    c = A.stage1_case()
    ref = A.reference(c)
    assert bool((ref["n1"] == 1).all()) and bool((ref["n2"] == 1).all())
    for which, start, n in A.stage1_probe_slices(c):
        g, want = pr[which]
        reps = -(-n // g.numel())
        assert torch.equal(c.inp["g"][start:start + n], g.repeat(reps)[:n])
        assert torch.equal(ref["code" + str(which)][start:start + n], want.repeat(reps)[:n]), f"probe set {which} at {start}"
    # what the probes hold: every entry, every midpoint and both neighbours (state1); a value below and above every midpoint (state2)
    m1 = A.midpoints(q1)
    g1 = set(pr[1][0].tolist())
    assert set(q1.tolist()) <= g1 and set(m1.tolist()) <= g1
    x2 = (pr[2][0] * pr[2][0]).tolist()
    m2 = A.midpoints(q2).tolist()
    assert all(any(x < m for x in x2) and any(x > m for x in x2) for m in m2)
    lay = c.lay
    off = [tuple(lay[a].starts[t] % (4 if a in "pg" else 8) for a in ("p", "g", "s1", "s2")) for t in range(len(c.numels))]
    assert [sum(1 for x in o if x) for o in off] == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1]
    assert [n % A.BLOCK != 0 for n in c.numels] == [s[2] for s in A.STAGE1_TENSORS]


def test_stage_2_decodes_every_code_under_differing_absmax():
    c = A.stage2_case()
    ref = A.reference(c)
    q1, _ = A.real_maps()
    t, b, i, ln = A.block_coords(c.numels)
    ex = c.exact["s1"]
    assert torch.equal(ref["code1"][ex], c.inp["s1"].long()[ex]) and torch.equal(ref["code2"], c.inp["s2"].long())
    blk = c.block_of
    for full in torch.unique(blk[ln == A.BLOCK]).tolist():
        for s in ("s1", "s2"):
            codes = c.inp[s][blk == full]
            if s == "s1" and full in (_gb(c, *A.STAGE2_ZERO), _gb(c, *A.STAGE2_NEG)) or s == "s2" and full == _gb(c, *A.STAGE2_ZERO):
                continue
            assert all(set(codes[k:k + 256].tolist()) == set(range(256)) for k in range(0, A.BLOCK, 256))
    a1, a2 = c.inp["a1"], c.inp["a2"]
    pw = set(A.STAGE2_POW)
    assert set(a1.tolist()) == pw and set(a2.tolist()) == pw and bool((a1 != a2).all())
    nb = c.nblocks
    assert bool((a1[:nb[0] - 1] != a1[1:nb[0]]).all()) and bool((a1[:nb[0] - 32] != a1[32:nb[0]]).all()) and nb[0] == 36
    z, ng = _gb(c, *A.STAGE2_ZERO), _gb(c, *A.STAGE2_NEG)
    keep = torch.ones(sum(nb), dtype=torch.bool)
    keep[z] = keep[ng] = False
    assert torch.equal(ref["n1"][keep].float(), a1[keep]) and torch.equal(ref["n2"][torch.arange(sum(nb)) != z].float(), a2[torch.arange(sum(nb)) != z])
    assert float(ref["n1"][z]) == 0 == float(ref["n2"][z]) and float(a1[z]) > 0 and float(a1[z - 1]) > 0 and float(a1[z + 1]) > 0
    assert set(ref["code1"][blk == z].tolist()) == {127} and set(ref["code2"][blk == z].tolist()) == {0} and float(q1[127]) == 0.0
    neg = c.inp["s1"][blk == ng]
    assert int(neg.min()) == 0 and int(neg.max()) == 254
    assert float(ref["n1"][ng]) == float(q1[0].abs() * a1[ng]) == float(torch.tensor(float(q1[0].abs()) * float(a1[ng]), dtype=A.F64).float())


def _gb(c, t, b):
    return sum(c.nblocks[:t]) + b


@pytest.mark.parametrize("table", "AB")
def test_stage_3_is_integer_arithmetic(table):
    c = A.stage3_case(table)
    ref = A.reference(c)
    w = c.want
    assert torch.equal(ref["code1"], w["s1"].long()) and torch.equal(ref["code2"], w["s2"].long())
    assert torch.equal(ref["n1"].float(), w["a1"]) and torch.equal(ref["n2"].float(), w["a2"])
    blk = c.block_of
    A1 = torch.log2(c.inp["a1"].double())[blk]
    assert torch.equal(ref["m"], w["s"].double() * torch.exp2(A1 - 8)) and torch.equal(ref["v"], w["w"].double() * torch.exp2(2 * A1 - 16))
    assert int(w["s"].abs().max()) == 512 and int(w["w"].max()) == 2 ** 18 and int(w["w"].min()) >= 0
    tie1, tie2 = w["s"] % 4 == 2, w["w"] % 1024 == 512
    print(f"stage 3, table {table}: {float(tie1.double().mean()):.3f} of the elements on a midpoint of the signed map, "
          f"{float(tie2.double().mean()):.3f} of the unsigned one")
    assert float(tie1.double().mean()) > 0.15 and float(tie2.double().mean()) > (0.05 if table == "A" else 0.02)
    if table == "A":
        for s in ("s1", "s2"):
            assert {0, 1, 254, 255} <= set(w[s].tolist()), s
        assert {0, 1, 254} <= set(w["s1"][tie1].tolist())   # ties next to the end codes too (a tie takes the lower code: never 255)
    # the planted lane is the only maximum of its block, for both states; it is lane 0, 8, 1 023 or 2 047 of a full block
    t, b, i, ln = A.block_coords(c.numels)
    top1, top2 = w["s"].abs() == 512, w["w"] == 2 ** 18
    assert torch.equal(top1, top2) and int(top1.sum()) == sum(c.nblocks) == len(set(blk[top1].tolist()))
    if table == "A":
        assert {0, 8, 1023, 2047} == set(i[top1 & (ln == A.BLOCK)].tolist())
    gs, _ = A.clip_coefficient(c.clip)
    assert gs == 1.0 and c.scalars[1:3] == (0.5, 0.75)


def test_the_tables_and_kinds_are_the_ones_the_kernel_can_go_wrong_at():
    assert A.A_NUMELS == (1, 7, 8, 9, 2047, 2048, 2049, 5096, 65536, 65537, 65536 + 3 * 2048 + 5, 2 * 65536 + 5)
    assert A.B_NUMELS == tuple(1 + t % 7 for t in range(300)) and sum(A.A_NUMELS) + sum(A.B_NUMELS) < 400_000
    c = A.stage4_case(0)
    lay = c.lay
    off = [tuple(lay[a].starts[t] * (4 if a in "pg" else 1) % (16 if a in "pg" else 8) for a in ("p", "g", "s1", "s2")) for t in range(12)]
    assert sum(1 for o in off if any(o)) == 6 and all(sum(1 for x in o if x) <= 1 for o in off)
    assert sorted(o for o in off if any(o)) == sorted([(4, 0, 0, 0), (0, 8, 0, 0), (0, 0, 1, 0), (0, 0, 4, 0), (0, 0, 7, 0), (0, 0, 0, 3)])
    for cc in (c, A.stage4_case(9), A.stage1_case(), A.stage2_case()):
        for a in A.ARRAYS:   # at least GUARD sentinels on every side of every array, the absmax arrays included
            la = cc.lay[a]
            ends = sorted((s, s + n) for s, n in zip(la.starts, la.numels))
            flat = [0] + [x for se in ends for x in se] + [la.length]
            assert all(flat[k + 1] - flat[k] >= A.GUARD for k in range(0, len(flat), 2)), (cc.name, a)
    cb = A.stage4_case(9)
    assert cb.numels == A.B_NUMELS and any(s % 4 for s in cb.lay["p"].starts) and any(s % 8 for s in cb.lay["s2"].starts)
    # the Latin square: every hyper-parameter set, step and clip, each pair of them once per table; the first step of either table
    sq = [s for s in A.STAGE4 if not s[4]]
    assert len({(tb, h, s) for tb, h, s, _, _ in sq}) == 18 and {cl for _, _, _, cl, _ in sq} == {0, 1, 2} and sum(s[4] for s in A.STAGE4) == 2
    assert A.HP[0] == (1e-2, 0.9, 0.98, 1e-6, 0.1) and A.HP[1] == (1e-3, 0.9, 0.999, 1e-8, 0.0) and A.STEPS == (1, 2, 1000)
    coef = [A.clip_coefficient(cl)[0] for cl in A.CLIPS]
    assert coef[0] == coef[1] == 1.0 and abs(coef[2] - 0.5) < 1e-3
    for tb in "AB":
        inp = A.stage4_inputs(tb, False)
        k = inp["kind"]
        assert set(k.tolist()) == set(range(8)) and all(torch.isfinite(inp[a]).all() for a in ("p", "g", "a1", "a2"))
        assert (inp["g"][(k == 1) | (k == 2)] == 0).all() and (inp["s1"][(k == 2) | (k == 3)] == 127).all() and (inp["s2"][(k == 2) | (k == 3)] == 0).all()
        assert (inp["p"][k == 6] == 0).all() and inp["p"][k == 7].abs().min() >= 1e3 and (inp["s2"][k == 5] == 255).all()
        assert (inp["a1"] > 0).all() and (inp["a2"] > 0).all() and inp["g"][k == 3].abs().max() < 1e-6 and inp["g"][k == 4].abs().max() > 1e3
        first = A.stage4_inputs(tb, True)
        assert not first["s1"].any() and not first["s2"].any() and not first["a1"].any() and not first["a2"].any()
    # kind 7: the update is below half an ulp of p (the case without weight decay: the reference moves p by less than 2^-25 |p|)
    c7 = A.stage4_case(4)
    assert c7.scalars[4] == 0 and c7.numels == A.A_NUMELS
    ref = A.reference(c7)
    k7 = c7.inp["kind"] == 7
    assert ((ref["p"] - c7.inp["p"].double()).abs()[k7] < 2.0 ** -25 * 1e3).all()
    # kind 3: eps rules the denominator (sqrt(v') below eps2 for most of them at eps 1e-6, step 1000)
    c3 = A.stage4_case(2)
    assert c3.scalars[3] == A.f32(1e-6)
    ref = A.reference(c3)
    k3 = c3.inp["kind"] == 3
    assert float((ref["v"][k3].sqrt() < math.sqrt(c3.scalars[6]) * c3.scalars[3]).double().mean()) > 0.9
