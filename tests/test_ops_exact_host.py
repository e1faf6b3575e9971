"""CPU twin of tests/test_ops_exact_gpu.py: no kernel runs here.  It proves what tests/_ops_exact_cases.py claims about its cases --
the conditions (a) to (c) hold for every case, seed and pass (the builders assert them; this test builds every one), the tap pattern of
the conv weights reaches every (kk, ci) slot, the float64 restatement of ConvStemFn's stride recipes equals plain float64 autograd, the
three GELU formulas of csrc/common.h and the one-byte code are exact on every integer 8..256 in CPU fp32 -- and that the comparison
the GPU test uses (`mismatch` on tensors of the engine's dtypes) rejects every mutant in every case whose operands it changes, and every
mutant in at least one case.  Prints, per family, the cases and seeds built and the mutants rejected."""
import numpy as np
import pytest
import torch

from tests import _ops_exact_cases as S

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
_BF16_OUTPUTS = ("y", "dx", "dres", "out", "logits")


def _as_engine(ref):
    """the reference in the dtypes the engine returns: activations and their gradients bf16, parameter gradients f32"""
    return {k: v.to(BF16 if k in _BF16_OUTPUTS else F32) for k, v in ref.items()}


def _rejected(clean, mutated, what):
    """-> True if the mutant changes a checked tensor (then the comparison must report it), False if it changes nothing"""
    got = _as_engine(mutated)
    if all(torch.equal(got[k], _as_engine(clean)[k]) for k in clean):
        return False
    report = S.first_mismatch(got, clean, what)
    assert report is not None and what in report and "differ, first at" in report, report
    return True


def test_mismatch_report_names_tensor_index_values_and_count():
    want = torch.arange(12, dtype=F64).view(3, 4)
    assert S.mismatch(want.to(BF16), want, "t") is None
    got = want.to(F32).clone()
    got[1, 2] += 1.0
    got[2, 3] -= 2.0
    assert S.mismatch(got, want, "case x dW0") == "case x dW0: 2 of 12 elements differ, first at (1, 2): got 7.0, want 6.0"
    assert "shape (3, 4), want (4, 3)" in S.mismatch(got, want.T, "t")
    got[0, 0] = float("nan")
    assert "3 of 12" in S.mismatch(got, want, "t")


def test_gelu_is_the_identity_on_integers_from_8_in_cpu_fp32():
    lo, hi = S.GELU_RANGE
    v = np.arange(lo, hi + 1, dtype=np.float32)
    r = S.gelu_premise_cpu(v)
    one = np.ones_like(v)
    assert np.array_equal(r["gelu"], v) and np.array_equal(r["both_g"], v)
    assert np.array_equal(r["dgelu"], one) and np.array_equal(r["both_d"], one)
    assert np.array_equal(r["code"], np.full(v.shape, 226, dtype=np.uint32)) and np.array_equal(r["decoded"], one)
    # and the restatement is a GELU: below the range it is not the identity, and its one-byte codes are those of the exact derivative
    w = np.array([-3.0, -1.0, 0.5, 1.0, 2.0, 4.0], dtype=np.float32)
    q = S.gelu_premise_cpu(w)
    x = torch.from_numpy(w).double()
    dref = 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-x * x / 2) / (2 * torch.pi) ** 0.5
    assert bool((q["gelu"] != w).all()) and bool((q["both_g"] != w).all()) and bool((q["dgelu"] != 1).all()) and bool((q["both_d"] != 1).all())
    assert q["code"].tolist() == (torch.round(200 * dref) + 26).long().tolist() == [24, 9, 199, 243, 243, 226]
    print(f"gelu premise: {hi - lo + 1} integers {lo}..{hi}: gelu_f, gelu_both_f, dgelu_f exact, code 226 -> 1.0f")


# ------------------------------------------------------------------------------------------------ ConvStemFn
@pytest.mark.parametrize("case", S.CONV_CASES, ids=str)
def test_conv_premises_and_mutants(case):
    n_mels, d, T, B = case
    for cin in (n_mels, d):
        slots = S.conv_tap_slots(d, cin)
        assert len(torch.unique(slots)) == 3 * cin, f"the tap pattern misses a (kk, ci) slot: {len(torch.unique(slots))} of {3 * cin}"
        assert all(len(set(row)) == 4 for row in slots.tolist())
    rejected = {m: 0 for m in S.CONV_MUTANTS}
    runs = 0
    for seed in S.SEEDS:
        for sign in (1.0, -1.0):
            t = S.conv_inputs(case, seed, sign)
            r = S.conv_premises(t, f"conv {case} seed {seed} w2 sign {sign}")
            assert set(t["w1"].abs().sum((1, 2)).tolist()) == {4.0} == set(t["w2"].abs().sum((1, 2)).tolist())
            assert 8 <= float(r["pre1"].min()) and float(r["pre1"].max()) <= 24
            assert 17 <= float(r["pre2"].min()) and float(r["pre2"].max()) <= 190 and float(r["out"].abs().max()) <= 190
            assert float(r["dpre1p"].abs().max()) <= 6 and float(r["dw2"].abs().max()) < 1200
            assert float(r["dpre1p"][:, 0].abs().max()) == 0 == float(r["dpre1p"][:, T + 1].abs().max())
            ref = S.conv_ref64(t)
            clean = {k: ref[k] for k in S.CONV_CHECKED}
            assert S.first_mismatch(_as_engine({k: r[k] for k in S.CONV_CHECKED}), clean, "restated") is None
            assert ref["dw1"].shape == t["w1"].shape and bool((ref["dw1"] != 0).any())
            for m in S.CONV_MUTANTS:
                mut = S.conv_restate(t, m)
                rejected[m] += _rejected(clean, {k: mut[k] for k in S.CONV_CHECKED}, f"conv {case} {m}")
            runs += 1
    print(f"ConvStemFn {case}: {len(S.SEEDS)} seeds x 2 signs of w2; mutants rejected: {rejected}")
    for m, n in rejected.items():
        assert n == (0 if case in S.CONV_NEVER.get(m, ()) else runs), (case, m, n)


def test_every_conv_mutant_is_rejected_somewhere():
    for m in S.CONV_MUTANTS:
        assert len(S.CONV_NEVER.get(m, ())) < len(S.CONV_CASES), m


# ------------------------------------------------------------------------------------------------ LinearFn
def test_linear_table_covers_the_routes():
    names = {c.name for c in S.LINEAR_CASES}
    assert len(names) == len(S.LINEAR_CASES)
    assert {c.M for c in S.LINEAR_CASES} == {37, 300}
    assert {(c.K, c.outs, max((s.rank for s in c.lora_list if s is not None), default=0)) for c in S.LINEAR_CASES} >= {
        (128, (128,), 0), (128, (128,) * 3, 8), (384, (384,) * 3, 16), (1536, (384,), 3)}
    assert any(c.n != c.npad for c in S.LINEAR_CASES) and any(c.fwd_scales == (0.25, 1.0, 1.0) for c in S.LINEAR_CASES)
    assert sum(s.rank for s in next(c for c in S.LINEAR_CASES if c.name == "lora_total_rank_80").loras) == 80
    assert {c.fused for c in S.LINEAR_CASES} == {None, True, False}


@pytest.mark.parametrize("case", S.LINEAR_CASES, ids=str)
def test_linear_premises_and_mutants(case):
    rejected = {m: 0 for m in S.LINEAR_MUTANTS}
    runs = 0
    for seed in S.SEEDS:
        for pas in S.PASSES:
            t, ref = S.linear_case(case, seed, pas)                      # asserts (a) and (b)
            for i, m in enumerate(t["mask"]):
                assert m is None or set(m.unique().tolist()) == {0.0, 2.0}
            assert bool((ref["y"][:, case.n:] == 0).all())
            for i, o in enumerate(case.outs):
                assert ref[f"dW{i}"].shape == (o, case.K)
            if pas == 0 and seed == 0:     # fp32 on the CPU, whatever order its BLAS sums in, gives the float64 bits
                w = torch.cat([t["W"][i] if case.lora_list[i] is None else
                               t["W"][i] + S.SCALING * t["B"][i] @ (t["A"][i] * (1.0 if t["mask"][i] is None else t["mask"][i]))
                               for i in range(len(case.outs))])
                y32 = t["x"] @ w.T
                y64 = t["x"].double() @ w.double().T
                assert torch.equal(y32, y64.to(F32)), case.name
            for m in S.LINEAR_MUTANTS:
                if not S.linear_mutant_applies(case, m):
                    continue
                mut, _ = S.linear_ref64(case, t, m)
                rejected[m] += _rejected(ref, mut, f"{case.name} {m}")
            runs += 1
    print(f"LinearFn {case.name}: {len(S.SEEDS)} seeds x {len(S.PASSES)} passes; mutants rejected: {({m: n for m, n in rejected.items() if n})}")
    for m, n in rejected.items():
        assert n == (runs if S.linear_mutant_applies(case, m) else 0), (case.name, m, n)


def test_every_linear_mutant_is_rejected_somewhere():
    for m in S.LINEAR_MUTANTS:
        assert any(S.linear_mutant_applies(c, m) for c in S.LINEAR_CASES), m


# ------------------------------------------------------------------------------------------------ MLP pair, fork, homes, tied logits
def test_mlp_pair_premises_and_mutants():
    shapes = S.MLP_CASES + (S.AUX8_SHAPE_OBSERVED,)
    rejected = {m: 0 for m in S.MLP_MUTANTS}
    runs = 0
    for M, d in shapes:
        for seed in (S.SEEDS if (M, d) in S.MLP_CASES else S.SEEDS[:1]):     # (the one-byte shape runs on one seed, as on the GPU)
            runs += 1
            t, ref = S.mlp_case(M, d, seed)                              # asserts (a), (b), (c)
            assert int((t["x"] != 0).sum(1).max()) <= 4 and set(t["x"].unique().tolist()) <= {-1.0, 0.0, 1.0}
            assert bool(((t["w2"] != 0).sum(1) == 8).all()) and bool(((t["w2"] != 0).sum(0) == 2).all()), "W2 must cover all 4d columns"
            pre = t["x"].double() @ t["w1"].double().T + t["b1"].double()
            assert 8 <= float(pre.min()) and float(pre.max()) <= 16
            for m in S.MLP_MUTANTS:
                rejected[m] += _rejected(ref, S.mlp_ref64(t, m)[0], f"mlp {M} x {d} {m}")
    print(f"MLP pair: {len(shapes)} shapes, {runs} (shape, seed) pairs; mutants rejected: {rejected}")
    assert all(n == runs for n in rejected.values()), rejected


def test_fork_premises_and_mutants():
    n = 0
    for case in S.FORK_CASES:
        for seed in S.SEEDS:
            for left_out in (None, 1):
                t, ref = S.fork_case(case, seed, left_out)               # asserts that every subset sum is a bf16 number
                assert ("dW1" in ref) == (left_out is None)
                _, mut = S.fork_case(case, seed, left_out, "fork_sum_misses_a_consumer")
                assert _rejected(ref, mut, f"fork {case}")
                n += 1
    print(f"fork: {len(S.FORK_CASES)} cases x {len(S.SEEDS)} seeds x (all consumers, one left out); fork_sum_misses_a_consumer rejected: {n}")


def test_grad_homes_premises_and_mutants():
    n = 0
    for case in S.HOME_CASES:
        assert case.n == case.npad                       # LinearFn asks for homes only when nothing is padded
        for seed in S.home_seeds(case):
            ts, total = S.homes_case(case, seed)
            assert len(ts) == S.HOME_PASSES and set(total) == {"dW0", "dW1", "dW2", "db0", "db2"}
            assert torch.equal(total["dW1"], sum(ref["dW1"] for _, ref in ts))
            if case.M <= 300:                            # (the mutant's sums are the last pass's products: nothing new to compute at 16384 rows)
                _, mut = S.homes_case(case, seed, "home_overwritten")
            else:
                mut = {k: (ts[-1][1][k] if k[:2] == "dW" else v) for k, v in total.items()}
            assert _rejected(total, mut, case.name)
            n += 1
    print(f"gradient homes: {len(S.HOME_CASES)} cases, {n} (case, seed) pairs x {S.HOME_PASSES} passes; home_overwritten rejected: {n}")


def test_tied_logits_premises_and_mutants():
    rejected = {m: 0 for m in S.TIED_MUTANTS}
    for rows in S.TIED_ROWS:
        for seed in S.SEEDS:
            for pas in S.PASSES:
                t, ref = S.tied_case(rows, seed, pas)
                assert ref["logits"].shape == (rows, 384) and ref["dE"].shape == (S.TIED_V, S.TIED_D)
                for m in S.TIED_MUTANTS:
                    rejected[m] += _rejected(ref, S.tied_case(rows, seed, pas, m)[1], f"tied rows {rows} {m}")
    runs = len(S.TIED_ROWS) * len(S.SEEDS) * len(S.PASSES)
    print(f"TiedLogitsFn: rows {S.TIED_ROWS} x {len(S.SEEDS)} seeds x {len(S.PASSES)} passes; mutants rejected: {rejected}")
    assert all(n == runs for n in rejected.values()), rejected
