"""CPU twin of tests/test_f32_kernels_gpu.py: no kernel runs here.  It proves what tests/_f32_cases.py claims about its cases --
operands are integers with sum |a||b| < 2^24 and give the same bits in three fp32 summation orders, the one-hot selectors reach every
k, poison sits exactly where the strides never point (the overlapping conv windows included), the conv stem's pre-activations are
>= 8 and CPU fp32 GELU is the identity / 1.0f there -- that each checker accepts the clean CPU restatement of its kernel and rejects
every planted mutant on every case where the mutant changes a bit, and that the constants written in that module's docstring are what
this test measures now.  Prints, per kernel, the cases built and the mutants rejected."""
import math

import pytest
import torch

from tests import _f32_cases as S

F32, F64 = torch.float32, torch.float64
NAN = float("nan")


def _is_int(t):
    return bool((t == t.round()).all())


# ------------------------------------------------------------------------------------------------ wft_gemm_f32
def test_gemm_shapes_cover_ragged_and_full():
    Ms, Ns, Ks = ({s[i] for s in S.GEMM_SHAPES} for i in range(3))
    assert Ms <= {1, 31, 33, 64, 65, 129} and Ns <= {1, 31, 33, 64, 65, 129} and Ks == {1, 2, 15, 16, 17, 33, 50}
    assert 64 in Ms and 64 in Ns and 16 in Ks and any(m % 64 for m in Ms) and any(n % 64 for n in Ns)
    assert 9 <= len(S.GEMM_SHAPES) <= 12
    stagings = {(c.la.strides[2] == 1, c.lb.strides[1] == 1) for c in S.gemm_cases(33, 31, 15)}
    assert stagings == {(True, True), (True, False), (False, True), (False, False)}   # what the kernel's a_kfast / b_kfast see


@pytest.mark.parametrize("shape", S.GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_premises_and_mutants(shape):
    cases = S.gemm_cases(*shape) + [c for c in S.GEMM_RECIPES if shape == S.GEMM_SHAPES[0]]
    rejected = {m: 0 for m in S.GEMM_MUTANTS}
    for case in cases:
        for seed in S.SEEDS:
            for poison in S.POISONS:
                op = S.gemm_operands(case, seed, poison)
                for flat, lay in ((op.a_flat, case.la), (op.b_flat, case.lb)):
                    assert S.untouched_is_poison(flat, lay, poison), case.name
                a, b, c0 = case.la.view(op.a_flat), case.lb.view(op.b_flat), case.lc.view(op.c_flat)
                assert _is_int(a) and _is_int(b) and float(a.abs().max()) <= 2 and float(b.abs().max()) <= 2
                assert (bool(torch.isnan(c0).all()) if case.beta == 0 else _is_int(c0)), case.name
                guard = torch.ones(op.c_flat.numel(), dtype=torch.bool)
                guard[case.lc.addresses().reshape(-1)] = False
                assert bool((op.c_flat[guard] == S.GUARD).all()) and int(guard.sum()) > 0
                want = S.gemm_expected(op)
                assert bool(torch.isfinite(case.lc.view(want)).all())
                assert S.gemm_mismatch(S.gemm_restate(op), want, case) is None, case.name     # poison never read, same bits
        # three summation orders, once per case (seed 0)
        op = S.gemm_operands(case, 0, NAN)
        prod64 = (case.la.view(op.a_flat).double() @ case.lb.view(op.b_flat).double()).to(F32)
        for s in S.fp32_sum_orders(case.la.view(op.a_flat), case.lb.view(op.b_flat)):
            assert torch.equal(s, prod64), case.name
        if case in S.GEMM_RECIPES:
            continue
        clean, want = S.gemm_restate(op), S.gemm_expected(op)
        for m in S.GEMM_MUTANTS:
            mut = S.gemm_restate(op, m)
            if S.same_bits(mut, clean):
                continue
            report = S.gemm_mismatch(mut, want, case)
            assert report is not None, (case.name, m)
            assert ("OUTSIDE" in report) == (m in ("write_row_M", "write_col_N")), report
            rejected[m] += 1
    print(f"wft_gemm_f32 {shape}: {len(cases)} cases x {len(S.SEEDS)} seeds x {len(S.POISONS)} poisons; mutants rejected: {rejected}")
    never = set()                       # the mutants that cannot change this shape
    if shape[2] % 16 == 0:
        never.add("drop_last_k_of_ragged_slab")
    if shape[2] < 2:
        never.add("swap_mfma_pair_in_A")
    if shape[0] == 1 and shape[1] == 1:
        never.add("bias_by_m")
    for m, n in rejected.items():
        assert (n == 0) == (m in never), (shape, m, n)
    assert rejected["write_row_M"] == len(S.gemm_cases(*shape)) == rejected["write_col_N"]


def test_gemm_mutants_hit_ragged_and_full_cases():
    """every mutant is rejected on at least one ragged and one full shape (drop_last_k: ragged only, by construction)"""
    for m in S.GEMM_MUTANTS:
        hit = set()
        for shape in ((64, 64, 16), (65, 64, 17), (129, 31, 50)):
            for case in S.gemm_cases(*shape):
                op = S.gemm_operands(case, 1, NAN)
                mut = S.gemm_restate(op, m)
                if not S.same_bits(mut, S.gemm_restate(op)):
                    assert S.gemm_mismatch(mut, S.gemm_expected(op), case) is not None
                    hit.add(case.ragged)
        assert hit == ({True} if m == "drop_last_k_of_ragged_slab" else {True, False}), (m, hit)


@pytest.mark.parametrize("one_hot", "BA")
def test_gather_probes_select_every_k(one_hot):
    n_cases = 0
    for shape in S.GEMM_SHAPES:
        M, N, K = shape
        for case in S.gather_cases(*shape):
            for seed in S.SEEDS:
                ops = S.gather_operands(case, seed, NAN, one_hot)
                sel = ops[0].selectors
                for b in range(S.BATCH):
                    assert set(sel[:, b].reshape(-1).tolist()) == set(range(K)), case.name
                for r, op in enumerate(ops):
                    dense = case.la.view(op.a_flat) if one_hot == "B" else case.lb.view(op.b_flat)
                    hot = case.lb.view(op.b_flat) if one_hot == "B" else case.la.view(op.a_flat)
                    assert bool((dense.abs() >= 2.0 ** -126).all()) and bool(torch.isfinite(dense).all())
                    assert bool((hot.sum(1 if one_hot == "B" else 2) == 1).all()) and set(hot.unique().tolist()) <= {0.0, 1.0}
                    logical = S.gather_expected_logical(op, one_hot, r)
                    want = S.gemm_expected(op, logical)
                    assert S.same_bits(want, S.gemm_expected(op)), case.name           # the gather IS the float64 product
                    clean = S.gemm_restate(op)
                    assert S.gemm_mismatch(clean, want, case) is None
                    if one_hot == "B" and K >= 2 and seed == 0:   # a k swapped inside an MFMA pair of A is seen by the gather
                        mut = S.gemm_restate(op, "swap_mfma_pair_in_A")
                        if not S.same_bits(mut, clean):
                            assert S.gemm_mismatch(mut, want, case) is not None
                    n_cases += 1
    print(f"wft_gemm_f32 gather probe, one-hot {one_hot}: {n_cases} operand sets")


def test_gemm_report_names_tile_and_quadrant():
    case = S.gemm_cases(129, 65, 17)[0]
    op = S.gemm_operands(case, 0, NAN)
    want = S.gemm_expected(op)
    bad = want.clone()
    case.lc.view(bad)[2, 100, 40] += 1.0
    report = S.gemm_mismatch(bad, want, case)
    assert "(batch 2, m 100, n 40)" in report and "1 elements differ" in report and "[(1, 0)]" in report and "quadrants [3]" in report


# ------------------------------------------------------------------------------------------------ ops32 functions
def test_linear_cases_are_integer_arithmetic():
    assert {c[0] for c in S.LINEAR_CASES} == {40, 72} == {c[1] for c in S.LINEAR_CASES} and {8, 3, 0} == {c[2] for c in S.LINEAR_CASES}
    for case in S.LINEAR_CASES:
        for seed in S.SEEDS:
            t, ref = S.linear_case(case, seed)
            assert all(_is_int(v) for v in t.values() if v is not None)
            assert t["mask"] is None or set(t["mask"].unique().tolist()) == {0.0, 2.0}
            assert all(_is_int(v) for v in ref.values()), case
            assert S.linear_magnitudes(t) < S.LIMIT
            assert set(ref) == {"y", "w_eff", "dx", "dw"} | ({"db"} if case[4] else set()) | ({"dA", "dB"} if case[2] else set())
    print(f"LinearFn: {len(S.LINEAR_CASES)} cases x {len(S.SEEDS)} seeds")


def test_conv_stem_premises_and_mutants():
    assert {c[0] for c in S.CONV_CASES} == {5, 8} and {c[1] for c in S.CONV_CASES} == {24, 72}
    assert {c[2] for c in S.CONV_CASES} == {6, 22, 130} and {c[3] for c in S.CONV_CASES} == {1, 3}
    rejected = {m: 0 for m in S.CONV_MUTANTS}
    for case in S.CONV_CASES:
        for seed in S.SEEDS:
            t = S.conv_inputs(case, seed)
            assert all(_is_int(v) for v in t.values())
            ref = S.conv_ref64(t)
            assert all(_is_int(v) for v in ref.values())
            assert S.conv_magnitudes(t) < S.LIMIT
            for pre in (ref["pre1"], ref["pre2"]):
                assert float(pre.min()) >= 8.0
                p32 = pre.to(F32)
                assert torch.equal(p32.double(), pre)
                assert S.same_bits(S.gelu_f32_cpu(p32), p32), "CPU fp32 GELU is not the identity on the pre-activations"
                ones = torch.ones_like(p32)
                assert S.same_bits(S.dgelu_f32_cpu(ones, p32), ones), "CPU fp32 GELU' is not 1.0f on the pre-activations"
            for m in S.CONV_MUTANTS:
                mut = S.conv_ref64(t, m)
                changed = [k for k in S.CONV_CHECKED if not torch.equal(mut[k], ref[k])]
                assert changed, (case, m)     # each conv mutant moves the forward or a gradient on every case
                rejected[m] += 1
    print(f"ConvStemFn: {len(S.CONV_CASES)} cases x {len(S.SEEDS)} seeds; mutants rejected: {rejected}")
    assert all(n == len(S.CONV_CASES) * len(S.SEEDS) for n in rejected.values())


def test_tied_logits_case_is_integer_arithmetic():
    for seed in S.SEEDS:
        t, ref, mag = S.tied_case(seed)
        assert all(_is_int(v) for v in list(t.values()) + list(ref.values())) and mag < S.LIMIT


# ------------------------------------------------------------------------------------------------ softmax
def _p_buffer(case, x):
    p, _ = S.softmax_ref64(case, x)
    buf = torch.full((case.nrows, case.ld), NAN, dtype=F32)
    buf[:, :case.cols] = p.to(F32)
    return buf


_SOFTMAX_WORST = {}


@pytest.mark.parametrize("cols", S.SOFTMAX_COLS)
def test_softmax_restatement_and_mutants(cols):
    cases = S.softmax_cases(cols)
    assert {c.nrows for c in cases} == {7, 10} and all(c.nrows % 4 for c in cases)
    if cols >= 7:
        assert {c.rpm for c in cases if c.causal} == {5, 7} and any(c.causal and c.nrows >= 2 * c.rpm for c in cases)
    rejected = {m: 0 for m in S.SOFTMAX_MUTANTS}
    worst_f = worst_b = 0.0
    for case in cases:
        floor = 2.0 ** -126 if case.kind == "span80" else 0.0
        for seed in S.SEEDS:
            x, dp = S.softmax_inputs(case, seed)
            assert bool(torch.isnan(x[:, cols:]).all()) and bool(torch.isfinite(x[:, :cols]).all())
            lim = S.softmax_lim(case)
            if case.causal:
                assert int(lim[0]) == 1 and bool((x[0, 1:cols] == S.DECOY / case.scale).all())
            if case.kind == "tie":
                t = torch.where(torch.arange(cols)[None, :] < lim[:, None], x[:, :cols], torch.tensor(-math.inf))
                assert bool(((t == t.max(1, keepdim=True).values).sum(1)[lim > 1] == 2).all())
            if case.kind == "span80":
                assert float((x[:, :cols] * case.scale).abs()[:, :1].max()) == 80.0
            clean = S.softmax_fwd_restate(case, x)
            problem, ratio = S.softmax_fwd_check(case, x, clean, floor)
            assert problem is None, (case.name, problem)
            if case.kind != "span80":
                worst_f = max(worst_f, ratio)
            p32 = _p_buffer(case, x)
            clean_b = S.softmax_bwd_restate(case, p32, dp)
            problem, ratio = S.softmax_bwd_check(case, p32, dp, clean_b, floor)
            assert problem is None, (case.name, problem)
            if case.kind != "span80":
                worst_b = max(worst_b, ratio)
            for m in S.SOFTMAX_MUTANTS:
                hit = False
                mut = S.softmax_fwd_restate(case, x, m)
                if not S.same_bits(mut, clean):
                    assert S.softmax_fwd_check(case, x, mut, floor)[0] is not None, (case.name, m, "forward")
                    hit = True
                mut = S.softmax_bwd_restate(case, p32, dp, m)
                if not S.same_bits(mut, clean_b):
                    assert S.softmax_bwd_check(case, p32, dp, mut, floor)[0] is not None, (case.name, m, "backward")
                    hit = True
                rejected[m] += hit
    _SOFTMAX_WORST[cols] = (worst_f, worst_b)
    print(f"wft_softmax_*_f32 cols {cols}: {len(cases)} cases x {len(S.SEEDS)} seeds; CPU restatement worst ratio fwd {worst_f:.3f} "
          f"bwd {worst_b:.3f}; mutants rejected: {rejected}")
    assert rejected["bwd_dot_over_ld"]      # one column: p = 1 and ds = 0 whatever the scale or the mask
    if cols >= 7:
        assert all(rejected.values()), rejected


def _matches(measured, recorded):
    return abs(measured - recorded) <= S.CPU_FIGURE_RTOL * recorded + 0.005


def test_softmax_constants_are_the_documented_ones():
    if len(_SOFTMAX_WORST) < len(S.SOFTMAX_COLS):
        for cols in S.SOFTMAX_COLS:
            test_softmax_restatement_and_mutants(cols)
    worst_f = max(v[0] for v in _SOFTMAX_WORST.values())
    worst_b = max(v[1] for v in _SOFTMAX_WORST.values())
    print(f"softmax CPU restatement: forward {worst_f:.3f}, backward {worst_b:.3f}")
    assert _matches(worst_f, S.SOFTMAX_CPU_F) and _matches(worst_b, S.SOFTMAX_CPU_B), (worst_f, worst_b)
    assert S.SOFTMAX_CF >= 4 * worst_f and S.SOFTMAX_CB >= 4 * worst_b
    assert S.SOFTMAX_CF == 20.0 and S.SOFTMAX_CB == 12.0 and f"SOFTMAX_CPU_F = 4 x {S.SOFTMAX_CPU_F:.2f}" in S.__doc__
    assert f"SOFTMAX_CPU_B = 4 x {S.SOFTMAX_CPU_B:.2f}" in S.__doc__ and "SOFTMAX_CF = 20" in S.__doc__ and "SOFTMAX_CB = 12" in S.__doc__


# ------------------------------------------------------------------------------------------------ element-wise
def test_gelu_inputs_and_constants():
    x = S.gelu_inputs()
    edges = x[:12].tolist()
    assert edges[:2] == [0.0, 0.0] and S.bits(x[:2]).tolist() == [0, -2 ** 31] and edges[2] == 2.0 ** -126 and set(map(abs, edges[4:])) == {1, 5.5, 8, 10}
    sat, _ = S.erff_saturation_points()
    c = torch.tensor(S.INV_SQRT2, dtype=F32)
    at, below = torch.tensor(sat, dtype=F32), torch.nextafter(torch.tensor(sat, dtype=F32), torch.tensor(0.0))
    assert S.erf32(at * c).item() == 1.0 and S.erf32(below * c).item() < 1.0 and 5.5 < sat < 5.6
    assert bool((x == at).any()) and bool((x == below).any()) and bool((x == -at).any()) and bool((x == S.EARLY_SATURATION).any())
    worst_f = S.gelu_fwd_ratio(x, S.gelu_f32_cpu(x))
    dy = S.gelu_dy(x.numel())
    worst_b = S.gelu_bwd_ratio(dy, x, S.dgelu_f32_cpu(dy, x))
    print(f"gelu CPU restatement: forward {worst_f:.3f}, backward {worst_b:.3f} over {x.numel()} inputs")
    assert _matches(worst_f, S.GELU_CPU_F) and _matches(worst_b, S.GELU_CPU_B), (worst_f, worst_b)
    assert S.GELU_CF >= 4 * worst_f and S.GELU_CB >= 4 * worst_b and S.GELU_CF == 6.0 and S.GELU_CB == 10.0
    assert f"GELU_CPU_F = 4 x {S.GELU_CPU_F:.2f}" in S.__doc__ and f"GELU_CPU_B = 4 x {S.GELU_CPU_B:.2f}" in S.__doc__
    assert S.bits(S.gelu_f32_cpu(x[1:2])).item() == -2 ** 31        # gelu(-0.0) = -0.0 by the fp32 formula
    # a GELU that is wrong by one part in 2^18 at one input is seen
    bad = S.gelu_f32_cpu(x).clone()
    bad[4] *= 1.0 + 2.0 ** -18      # x = 1
    assert S.gelu_fwd_ratio(x, bad) > S.GELU_CF


def test_second_grid_stride_trip_is_checked():
    assert S.BIG_N == 65535 * 256 + 300 and S.BIG_N % S.PERIOD and math.gcd(S.PERIOD, 256) == 1
    x = S.gelu_inputs()
    small = S.gelu_f32_cpu(x)
    assert S.tiled_mismatch(S.tiled(small, S.BIG_N), small, S.BIG_N) is None
    report = S.tiled_mismatch(S.second_trip_skipped(small, S.BIG_N), small, S.BIG_N)
    assert report is not None and "300 of" in report and "trip 1" in report
    print("grid-stride: 1 case, mutant second_trip_skipped rejected")


def test_axpby_forms():
    for n in S.EW_SIZES:
        x, y = S.axpby_inputs(n)
        for a, b in S.AXPBY_PAIRS:
            got = S.f32_scalar(a) * x + S.f32_scalar(b) * y                 # two roundings more than an fma: still inside
            assert S.axpby_ratio(a, x, b, y, got) <= 1.0
            fma = (S.f32_scalar(a).double() * x.double() + (S.f32_scalar(b) * y).double()).to(F32)
            assert S.axpby_ratio(a, x, b, y, fma) <= 1.0
    assert (1.0 - 1.0 / 0.9, 1.0 / 0.9) in S.AXPBY_PAIRS and (1.0, 1.0) in S.AXPBY_PAIRS


def test_colsum_cases_and_mutant():
    n = rejected = 0
    for rows in S.COLSUM_ROWS:
        for cols in S.COLSUM_COLS:
            for kind in ("int", "randn"):
                for seed in S.SEEDS:
                    x = S.colsum_input(rows, cols, kind, seed)
                    assert bool(torch.isnan(x[:, cols:]).all())
                    want = S.colsum_expected(x, cols, kind)
                    assert bool(torch.isfinite(want).all())
                    if kind == "int":
                        assert _is_int(x[:, :cols]) and float(x[:, :cols].abs().sum(0).max()) < S.LIMIT
                        assert torch.equal(want, S.colsum_expected(x, cols, "randn"))      # and in fp32 row order too
                    mut = S.colsum_expected(x, cols, kind, "colsum_ld_is_cols")
                    if rows > 1:
                        assert not S.same_bits(mut, want)
                        rejected += 1
                    n += 1
    print(f"wft_colsum_f32: {n} cases; mutant colsum_ld_is_cols rejected on {rejected}")
    assert rejected
