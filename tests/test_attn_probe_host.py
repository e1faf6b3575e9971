"""CPU proof that the per-(row, head) bound of the attention probe tests bites (tests/_attn_probe.py close_rows, used on the GPU by
tests/test_attn_probe_gpu.py): on the probe operands of every GPU case the fp32 -> bf16 emulation of CORRECT attention passes it
for o, dq, dk and dv, and the emulation under each wrong mask — a lost diagonal, an admitted key i + 1, a lost last key, an admitted
key Tk, a lost tile-edge key, a lost 32-key block, a lost 32-query dK/dV step — fails it on every row and key it touches whose
target or decoy the fault concerns.  Only arithmetic on the CPU: no kernel runs here, right or wrong.

The tolerance is measured here against the fp64 oracle, never against a kernel: TOL = 2 x the worst per-(row, head) ratio the
correct emulation reaches over all cases and the four tensors, rounded up to a power of two.  The factor 2 covers what the emulation
does not model (the kernels' fp32 summation order, hardware exp2, the one-wave-per-SIMD kernels' row constants entering through the
accumulators).  Measured over the 38 operand cases (seed 0): worst ratio 1.09e-2, in dk of a non-causal case (o 5.4e-3, dq 7.8e-3,
dv 7.1e-3 at worst; causal dk 6.7e-3), so TOL = 2^-5 = 3.125e-2; test_tol_is_twice_the_worst_emulation_ratio asserts that the
constant in _attn_probe.py is that number.  dk is the largest because dK_j sums dS_ij q_i over the rows that target key j, dS is
rounded to bf16 before that MFMA, and where the signed sum happens to come out small the roundings do not.
The condition on the mutants is not a measurement: every probed row of every mutant fails the bound in o or dq and every probed key
in dk or dv, the worst probed (row, head) of each tensor a mutant reaches lies at least 8 x TOL off (measured: 10 x TOL at the
least), and every mask mutant moves lse of its probed rows by at least ln 1.1.
"""
import functools
import math

import pytest
import torch

from tests import _attn_dispatch_cases as dispatch
from tests import _attn_probe as P
from tests.test_decode_kernels_gpu import close
from whisper_finetune.engine import lib as L

CASES = P.operand_cases()
IDS = ["B{}H{}-{}x{}-c{}-pre{}".format(*map(int, c)) for c in CASES]


def _min_over(ratio, sel):
    return ratio[sel].min().item() if sel.any() else math.inf


@functools.lru_cache(maxsize=None)
def _measure(case):
    """-> (worst ratio of the correct emulation per tensor, {mutant: min ratio over its probed rows / keys per tensor}, masses)"""
    B, H, Tq, Tk, causal, pre = case
    c = P.probe_case(B, H, Tq, Tk, causal, pre, seed=0)
    o64, lse64 = P.oracle_fwd(c)
    o, lse = P.emulate_fwd(c)
    P.close_lse(lse, lse64, "correct emulation, lse")
    dq, dk, dv = P.emulate_bwd(c, o, lse)
    ref = dict(zip(("o", "dq", "dk", "dv"), (o64, *P.oracle_bwd(c, o, lse))))
    worst = {}
    for name, got in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        worst[name] = P.close_rows(got, ref[name], P.TOL, P.FLOOR, f"correct emulation, {name}", atol=1e-6 if Tk == 1 else 0.0).max().item()
    table = {}
    for mname, (mask, drop_q) in P.mutants(c).items():
        rows, keys = P.probed(c, mask, drop_q)
        rows, keys = rows.permute(0, 2, 1), keys.permute(0, 2, 1)   # [B, T, H] as row_ratios returns
        t = {}
        got = dict(zip(("dq", "dk", "dv"), P.emulate_bwd(c, o, lse, mask, drop_q)))   # the backward alone is wrong: correct o, lse
        r = {name: P.row_ratios(got[name], ref[name])[0] for name in ("dq", "dk", "dv")}
        if mask is not None:
            got["o"], lm = P.emulate_fwd(c, mask)
            r["o"] = P.row_ratios(got["o"], ref["o"])[0]
            t["lse"] = _min_over((lm.double() - lse64).abs().permute(0, 2, 1), rows)
            t["o|dq"] = _min_over(torch.maximum(r["o"], r["dq"]), rows)
        t["dk|dv"] = _min_over(torch.maximum(r["dk"], r["dv"]), keys)
        for name, sel in (("o", rows), ("dq", rows), ("dk", keys), ("dv", keys)):
            if name in r and sel.any() and ref[name].abs().max() > 0:   # (one key: dq = dk = 0 whatever the mask)
                t[name] = (r[name][sel].min().item(), r[name][sel].max().item())
                with pytest.raises(AssertionError):   # the bound itself refuses the mutant wherever it has something probed
                    P.close_rows(got[name], ref[name], P.TOL, P.FLOOR, f"{mname}, {name}")
        t["n"] = (int(rows.sum()), int(keys.sum()))
        table[mname] = t
    return worst, table, c.mass


COLS = ("o", "dq", "dk", "dv")


def _check_mutant(mname, t):
    """Every probed row fails the bound in o or dq, every probed key in dk or dv (dq and dk alone are not decisive row by row:
    dS_ij = P_ij (dP_ij - delta_i) is 0.25 (dP_ia - dP_ib) on a row with two equal targets and vanishes where the two dP happen to
    meet); the worst probed (row, head) of every tensor the mutant reaches lies at least 8 x TOL off, so each kernel family (o: the
    forward kernels, dq: the dQ kernels, dk / dv: the dK/dV kernels) is caught decisively; lse of every probed row moves by ln 1.1."""
    for name in ("o|dq", "dk|dv"):
        if name in t:
            assert t[name] > P.TOL, f"{mname}: a probed (row, head) passes the bound in both of {name} ({t[name]:.3e})"
    for name in COLS:
        if name in t:
            assert t[name][1] >= 8 * P.TOL, f"{mname}: the worst probed (row, head) of {name} is only {t[name][1]:.3e} off (need {8 * P.TOL:.3e})"
    if "lse" in t:
        assert t["lse"] >= math.log(1.1), f"{mname}: lse of a probed row moves by only {t['lse']:.3e}"


def _cell(t, name):
    return f"{t[name][0]:8.1e}..{t[name][1]:<8.1e}" if name in t else " " * 18


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_row_bound_passes_correct_attention_and_fails_every_mutant(case):
    worst, table, mass = _measure(case)
    print(f"{case}: targets hold >= {mass['targets']:.3f} of every row's mass, each target >= {mass['each']:.3f}, "
          f"the decoy would take >= {mass['decoy']:.3f}")
    assert mass["decoy"] >= 0.1 and mass["each"] >= 0.1 and mass["targets"] >= P.MIN_TARGET_MASS
    print("correct emulation, worst (row, head) ratio: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert max(worst.values()) <= P.TOL / 2
    print(f"{'mutant: min..max ratio over its probed rows / keys':<52} {'rows/keys':>11}  " + " ".join(f"{n:<18}" for n in COLS) + " min|lse err|")
    for mname, t in table.items():
        print(f"{mname:<52} {t['n'][0]:>5}/{t['n'][1]:<5}  " + " ".join(_cell(t, n) for n in COLS) + f" {t.get('lse', math.nan):8.2e}")
        _check_mutant(mname, t)
    assert len(table) >= (2 if case[3] == 1 else 5)


def test_tol_is_twice_the_worst_emulation_ratio():
    worst = max(max(_measure(case)[0].values()) for case in CASES)
    tol = 2.0 ** math.ceil(math.log2(2 * worst))
    print(f"worst (row, head) ratio of the correct emulation over {len(CASES)} cases and o, dq, dk, dv: {worst:.3e}; "
          f"TOL = 2 x that, rounded up to a power of two = 2^{math.log2(tol):.0f} = {tol:.4e}")
    assert tol == P.TOL
    lowest = min(t[n][1] for case in CASES for t in _measure(case)[1].values() for n in COLS if n in t)
    print(f"lowest worst-probed (row, head) ratio of any mutant in any tensor it reaches: {lowest:.3e} = {lowest / P.TOL:.1f} x TOL")
    assert lowest >= 8 * P.TOL


def test_every_kernel_meets_a_causal_or_ragged_probe_and_the_table_names_the_kernels_the_plan_picks():
    h = L.load()
    for (Tq, Tk, causal), kern in P.TABLE:
        for B, H in P.GROUPS:
            assert dispatch.answers(h, (Tq, Tk, causal, B, H, 0, 0, 0, {}))[:3] == list(kern), (Tq, Tk, causal, B, H)
    for Tq, Tk, causal in P.FORCED:
        assert dispatch.answers(h, (Tq, Tk, causal, 1, 8, 7, 0, 0, {}))[:3] == [1, 8, 8]
    ragged = lambda s: s[2] or s[0] % 64 or s[1] % 64  # noqa: E731
    seen = {(i, k[i]) for s, k in P.TABLE if ragged(s) for i in range(3)} | {(i, (1, 8, 8)[i]) for s in P.FORCED if ragged(s) for i in range(3)}
    assert seen == {(0, 1), (0, 2), (1, 8), (1, 4), (2, 8), (2, 4)}


@pytest.mark.parametrize("T", [130, 448])
def test_the_tensor_wide_bound_on_randn_operands_for_the_record(T):
    """The gap this closes: causal T x T, randn operands, the existing tensor-wide close(..., 2e-2) against single-key seam faults.
    Printed for the record, like the last loop of test_attn_bounds_host.py.  Found: a fault at the 64-row seam, where a row has 65
    keys, the old bound still notices (3e-2 to 1.5e-1 of the tensor's maximum; dv of the lost diagonal excepted).  One seam on it
    does not: the diagonal lost on row 128 of 130, key 128 lost, and the diagonal lost on row 384 of 448 pass it in o, dq, dk and
    dv alike.  Asserted is only that the faults are real (they move o); what the old bound makes of them is reported."""
    c = P.randn_case(2, 4, T, T, True)
    o64, lse64 = P.oracle_fwd(c)
    o, lse = P.emulate_fwd(c)
    refs = dict(zip(("o", "dq", "dk", "dv"), (o64, *P.oracle_bwd(c, o, lse))))
    good = P.good_mask(c)
    s64 = (T - 1) // 64 * 64   # the last 64-seam: row s64 sees s64 + 1 keys
    seams = {f"diagonal dropped on row {s64}": good.clone(), f"key {s64} dropped": good.clone(),
             "diagonal dropped on rows that are multiples of 64": good.clone(), "key 64 dropped": good.clone()}
    seams[f"diagonal dropped on row {s64}"][s64, s64] = False
    seams[f"key {s64} dropped"][:, s64] = False
    r64 = torch.arange(64, T, 64)
    seams["diagonal dropped on rows that are multiples of 64"][r64, r64] = False
    seams["key 64 dropped"][:, 64] = False
    for mname, mask in seams.items():
        got = dict(zip(("o", "dq", "dk", "dv"), (P.emulate_fwd(c, mask)[0], *P.emulate_bwd(c, o, lse, mask))))
        ok = []
        for name in ("o", "dq", "dk", "dv"):
            try:
                close(got[name], refs[name], 2e-2, f"T={T}, tensor-wide 2e-2 on randn operands, {mname}, {name}")
                ok.append(name)
            except AssertionError:
                pass
        print(f"T={T} {mname}: PASSES the tensor-wide 2e-2 bound on randn operands in {ok or 'no tensor'}, fails it in "
              f"{[n for n in ('o', 'dq', 'dk', 'dv') if n not in ok] or 'no tensor'}")
        assert not torch.equal(got["o"], o)
