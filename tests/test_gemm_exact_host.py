"""CPU proof that the exact comparison of tests/test_gemm_exact_gpu.py rests on true premises and bites (tests/_gemm_exact_cases.py):
every case of the table is built for both seeds and its builder conditions hold (operands exactly bf16, every partial sum below
2^24 in any order, final values of a bf16 C representable, epilogue operands distinct from their neighbours, every k selected by the
gather probe); the fp32 sum in three orders equals the fp64 reference bit for bit; every way a tiled GEMM goes wrong, restated in
torch as a wrong reference, fails torch.equal (GELU forms: fails the derived bound); the recorded kernel kinds match the library's
public plan queries under its no-device assumption of 256 CUs; and the GELU constant in the cases module's docstring is the one
measured here against fp64.  Only arithmetic on the CPU: no kernel runs here, right or wrong.

Order independence is proved for the whole of every case by sum_k |a| |b| < 2^24 (asserted by the builders); the three explicit fp32
orders (ascending, 32-deep slabs, descending) are summed on the first, middle and last rows of each case.  The element-wise mutants
run on the last two 256-row tiles of a case (the ragged one and the full one before it, row M's poison behind them).
The slab condition is a condition, not a measurement: for every case and every 32-deep k-slab, every 16 x 16 output block changes in
at least a quarter of its elements when the slab is dropped or counted twice."""
import ctypes
import functools
import math
import re

import pytest
import torch

from tests import _gemm_exact_cases as G
from whisper_finetune.engine import lib as L

PTR = 1 << 20
NT = {c.name: c for c in G.NT_CASES}
TN = {c.name: c for c in G.TN_CASES}
ORDER_ROWS = 96    # the three-order sums run on the first, a middle and the last rows of a case


@functools.lru_cache(maxsize=4)
def _nt(name, seed):
    ops = G.nt_operands(NT[name], seed)
    return ops, G.nt_acc(ops)


def _rows(M):
    idx = sorted(set(list(range(min(M, ORDER_ROWS // 3))) + list(range(max(0, M // 2 - 16), min(M, M // 2 + 16))) + list(range(max(0, M - 32), M))))
    return torch.tensor(idx)


def _three_orders(X, Y, ref):
    """fp32 sums of X [m, K] Y [n, K]^T: ascending k, 32-deep slabs reduced separately and then added, descending k — all equal ref"""
    K = X.shape[1]
    up = torch.zeros(X.shape[0], Y.shape[0])
    down = torch.zeros_like(up)
    for k in range(K):
        up += X[:, k:k + 1] * Y[:, k][None, :]
        down += X[:, K - 1 - k:K - k] * Y[:, K - 1 - k][None, :]
    slabs = torch.zeros_like(up)
    for k0 in range(0, K, 32):
        slabs += X[:, k0:k0 + 32] @ Y[:, k0:k0 + 32].t()
    for name, got in (("ascending", up), ("32-deep slabs", slabs), ("descending", down)):
        assert got.dtype == torch.float32 and torch.equal(got.double(), ref), name


# ------------------------------------------------------------------------------------------------ builder conditions
@pytest.mark.parametrize("name", list(NT))
def test_nt_builder_conditions(name):
    c = NT[name]
    covered = {p: torch.zeros(c.K, dtype=torch.bool) for p in ("gather_b", "gather_a")}
    for seed in G.SEEDS:
        ops, acc = _nt(name, seed)
        assert G.is_bf16(ops.A) and G.is_bf16(ops.B) and acc.abs().max() < 2 ** 24
        assert torch.equal(ops.A_buf[..., :1].float(), ops.A_buf[..., :1].float())
        if not c.windows:   # the poison: rows >= M and columns K .. lda of A, columns K .. ldb of B
            assert (ops.A_buf[:, c.M:] == G.POISON).all() and (ops.A_buf[:, :, c.K:] == G.POISON).all() and ops.A_buf.shape[1] >= -(-c.M // 256) * 256
        assert (ops.B_buf[:, :, c.K:] == G.POISON).all()
        rows = _rows(c.M)
        _three_orders(ops.A[-1, rows, :], ops.B[0, :min(c.N, 512)], acc[-1, rows][:, :min(c.N, 512)])
        for fname in c.forms + c.forms256:
            form = G.FORMS[fname]
            e = G.nt_epilogue_operands(c, form, seed)
            want = G.nt_expected(form, acc, e)
            if form.exact:
                G.assert_nt_representable(form, want)
            else:
                assert torch.isfinite(want["C"]).all() and (want["bound"] >= 0).all()
        print(f"{name} seed {seed}: max|acc| = {acc.abs().max().item():.0f}")
        for probe, n_out in (("gather_b", c.N), ("gather_a", c.M * c.batch)):
            if probe == "gather_a" and c.windows:
                continue
            for r in range(G.gather_rounds(n_out, c.K)):
                covered[probe][G.gather_sel(n_out, c.K, seed, r, 3 if probe == "gather_b" else 5)] = True
    # the gather probe in one of its two forms selects every k (the other form is run as far as its rounds reach)
    assert covered["gather_b"].all()
    assert c.windows or covered["gather_a"].all()
    ops = G.nt_operands(c, 0, "gather_b")
    assert torch.equal(G.nt_acc(ops), ops.A.double()[:, :, ops.sel])


@pytest.mark.parametrize("name", list(TN))
def test_tn_builder_conditions(name):
    c = TN[name]
    for R in [c.R] + c.ragged():
        for seed in G.SEEDS if R == c.R else (0,):
            ops = G.tn_operands(c, R, seed, p_valid=c.p_valid[-1])
            assert G.is_bf16(ops.A) and G.is_bf16(ops.B)
            assert (ops.A_buf[:, R:] == G.POISON).all() and (ops.B_buf[:, R:] == G.POISON).all() and ops.A_buf.shape[1] >= R + 64
            acc = G.tn_acc(ops)
            assert acc.abs().max() < 2 ** 24 and torch.equal(acc, acc.round())
            if not c.c_f32:
                v = acc
                assert torch.equal(v.to(G.BF).double(), v) and v.abs().max() <= 256
            if R == c.R and seed == 0:
                p = torch.arange(0, c.P, max(1, c.P // 48))
                X, Y = ops.A[:, :, p].reshape(-1, len(p)).t().contiguous(), ops.B[:, :, :256].reshape(-1, min(c.Q, 256)).t().contiguous()
                _three_orders(X[:, :2048], Y[:, :2048], X[:, :2048].double() @ Y[:, :2048].double().t())
    if c.batch == 1:
        cov = torch.zeros(c.R, dtype=torch.bool)
        for seed in G.SEEDS:
            for r in range(G.gather_rounds(c.Q, c.R)):
                cov[G.gather_sel(c.Q, c.R, seed, r, 5)] = True
        assert cov.all()
        ops = G.tn_operands(c, c.R, 0, "gather_b")
        assert torch.equal(G.tn_acc(ops), ops.A.double()[0, ops.sel].t())


def test_epilogue_operands_differ_from_their_neighbours():
    G.assert_distinct_neighbours(G.bias_vec(8192))
    for b in range(3):
        G.assert_distinct_neighbours(G.residual_mat(b, 600, 600))
        G.assert_distinct_neighbours(G.aux_mat(b, 600, 600))
    assert all(G.is_bf16(torch.tensor(v)) and math.log2(abs(v)) == round(math.log2(abs(v))) for v in G.AUX_VALUES)
    assert G.is_bf16(G.col_scale_mat(8, 384))


# ------------------------------------------------------------------------------------------------ the comparison bites
def _fails_exact(got, want, what):
    with pytest.raises(AssertionError):
        G.assert_exact(got, want, 128, what)


def _fails(form, wrong, want, what, key="C"):
    """the wrong reference, rounded as the kernel would store it, fails the check the GPU test applies to this form"""
    bound = want["bound" if key == "C" else "aux_bound"]
    if bound is None:
        _fails_exact(wrong, want[key], what)
    else:
        with pytest.raises(AssertionError):
            G.assert_bounded(wrong.to(G.BF if not form.c_f32 else G.F32), want[key], bound, 128, what)


@pytest.mark.parametrize("name", list(NT))
def test_every_nt_mutant_fails(name):
    c = NT[name]
    ops, acc = _nt(name, 0)
    M, N, K = c.M, c.N, c.K
    X, Y = ops.A[-1], ops.B[0]
    frac = G.slab_delta_counts(X, Y)
    print(f"{name}: a dropped 32-deep slab moves at least {frac:.3f} of every 16 x 16 block")
    assert frac >= 0.25
    # the element-wise mutants run on the case's last rows: the ragged 256-row tile and the full one before it, row M's poison behind
    row0 = max(0, (M - 1) // 256 * 256 - 256)
    acc, X = acc[:, row0:], X[row0:]
    bi, bj, k0 = (M - row0 - 1) // 16, (N // 16) - 1, (K // 32 - 1) * 32   # the ragged corner block, the last slab
    tried = set()
    for fname in c.forms + c.forms256:
        form = G.FORMS[fname]
        e = G.nt_epilogue_operands(c, form, 0)
        e = G.Epi(e.bias, *(None if t is None else t[:, row0:] for t in (e.res, e.aux, e.base)))
        nt_expected = functools.partial(G.nt_expected, row0=row0)
        want = nt_expected(form, acc, e)
        for mname, factor in (("slab dropped", -1.0), ("slab counted twice", 1.0)):
            bad = acc.clone()
            if form.exact:     # one 16 x 16 block: the ragged corner
                bad[-1] = G.drop_slab(acc[-1], X, Y, bi, bj, k0, factor)
            else:              # a GELU form is flat where pre << 0: the fault in every block of one 16-column strip
                cols = slice(16 * bj, 16 * bj + 16)
                bad[-1][:, cols] += factor * (X[:, k0:k0 + 32].double() @ Y[cols, k0:k0 + 32].double().t())
            _fails(form, nt_expected(form, bad, e)["C"], want, f"{fname}: {mname}")
            tried.add(mname)
        if c.kind == "NT_128_SPLITK":
            for s, (a, b) in enumerate(G.nt_splits(M, N, K)):
                part = (X[:, a:b].double() @ Y[:, a:b].double().t())[None]
                _fails(form, nt_expected(form, acc - part, e)["C"], want, f"{fname}: split {s} dropped")
                _fails(form, nt_expected(form, acc + part, e)["C"], want, f"{fname}: split {s} added twice")
                tried.add("split dropped")
        muts = []
        if form.bias:
            muts += [("bias from column n+1", {"bias_shift": 1}), ("bias from the next 128-column tile", {"bias_shift": 128 % N})]
        if form.residual or form.epilogue in ("mul_aux", "dgelu"):
            muts.append(("residual / aux from row m+1", {"row_shift": 1}))
        if form.residual and form.beta != 1.0:
            muts.append(("beta read as 1", {"beta_one": True}))
        if form.res_first:
            muts.append(("residual_first ignored", {"ignore_res_first": True}))
        if form.valid is not None and M > form.valid[1]:
            muts += [("valid_rows one too many", {"valid_shift": 1}), ("valid_rows one too few", {"valid_shift": -1})]
        for mname, mut in muts:
            if mut.get("bias_shift", 1) == 0:
                continue   # N = 128: there is no next tile
            wrong = nt_expected(form, acc, e, mut)
            _fails(form, wrong["C"], want, f"{fname}: {mname}")
            if want["aux"] is not None and "bias_shift" in mut:
                if form.epilogue == "gelu":
                    _fails_exact(wrong["aux"], want["aux"], f"{fname} aux: {mname}")
                else:
                    _fails(form, wrong["aux"], want, f"{fname} aux: {mname}", key="aux")
            tried.add(mname)
        if form.colsum:   # row M (poison in A, residual and aux alike) admitted into the last tile's column sums
            accM = (G.POISON * Y.double().sum(1))[None, None, :]
            eM = G.Epi(e.bias, None if e.res is None else e.res[:, -1:].repeat(1, 2, 1), None if e.aux is None else e.aux[:, -1:].repeat(1, 2, 1))
            leak = G.nt_expected(form, accM, eM)["C"][0, 0]
            assert (leak != 0).any()
            _fails_exact(want["colsum"] + leak, want["colsum"], f"{fname}: row M admitted into the column sums")
            tried.add("row M in colsum")
    if c.kind == "NT_RANK":   # a column past the rank columns written: the product there is 0, the buffer's sentinel is not
        for pv in c.p_valid:
            nc = 16 * -(-pv // 16)
            buf = torch.full((M, N), 7.0, dtype=torch.float64)
            buf[:, :nc] = acc[0][:, :nc]
            wrong = buf.clone()
            if nc < N:
                wrong[:, nc] = 0.0
                _fails_exact(wrong, buf, f"p_valid {pv}: column {nc} written")
        tried.add("column past the rank columns")
    print(f"{name}: mutants refused: {sorted(tried)}")
    assert {"slab dropped", "slab counted twice"} <= tried


def test_every_listed_nt_mutant_is_tried_somewhere():
    """the forms of the table reach every mutant of the list (a table edit that drops the last valid_rows or colsum form fails here)"""
    forms = {f for c in G.NT_CASES for f in c.forms + c.forms256}
    F = [G.FORMS[f] for f in forms]
    assert any(f.bias == "int" for f in F) and any(f.residual and f.beta != 1 for f in F) and any(f.res_first for f in F)
    assert any(f.valid for f in F) and any(f.colsum == "fused" for f in F) and any(f.colsum == "pass" for f in F)
    assert any(c.kind == "NT_128_SPLITK" for c in G.NT_CASES) and any(c.kind == "NT_RANK" for c in G.NT_CASES)


@pytest.mark.parametrize("name", list(TN))
def test_every_tn_mutant_fails(name):
    c = TN[name]
    pv = c.p_valid[-1]
    ops = G.tn_operands(c, c.R, 0, p_valid=pv)
    acc = G.tn_acc(ops)
    X, Y = ops.A.reshape(-1, c.P).t().contiguous(), ops.B.reshape(-1, c.Q).t().contiguous()   # [P, R], [Q, R]
    live = pv if pv else c.P
    frac = G.slab_delta_counts(X[:live, :4096], Y[:, :4096]) if c.R * c.batch > 4096 else G.slab_delta_counts(X[:live], Y)
    print(f"{name}: a dropped 32-row slab moves at least {frac:.3f} of every 16 x 16 block")
    if c.R >= 32:
        assert frac >= 0.25
    _fails_exact(G.drop_slab(acc, X, Y, c.P // 16 - 1 if not pv else 0, c.Q // 16 - 1, (c.R * c.batch - 1) // 32 * 32), acc, "slab dropped")
    _fails_exact(G.drop_slab(acc, X, Y, 0, 0, 0, 1.0), acc, "slab counted twice")
    _fails_exact(G.tn_acc(ops, extra_row=True), acc, "row R admitted into the reduction")
    plan = G.tn_plan(c.R, c.P, c.Q, c.batch, c.c_f32, c.variant, pv, False, 0, c.workspace)
    if plan["nsplit"] > 1 and c.batch == 1:
        for s, (a, b) in enumerate(G.tn_splits(c.R, plan["nsplit"])):
            _fails_exact(acc - X[:, a:b].double() @ Y[:, a:b].double().t(), acc, f"split {s} dropped")
    if "block" in c.forms:
        bn, br = c.Q // 3, pv // 3 or 1
        want = G.tn_expected("block", acc, pv, block=(bn, br))
        assert want.numel() == c.Q * br
        _fails_exact(G.tn_expected("block", acc, pv, block=(bn, br), mut={"no_transpose": True})[None], want[None], "block_n output not transposed")
    if "col_scale" in c.forms:
        sc = G.col_scale_mat(3, c.Q)
        want = G.tn_expected("col_scale", acc, pv, scale=sc, scale_rows=-(-pv // 3))
        _fails_exact(G.tn_expected("col_scale", acc, pv, scale=torch.roll(sc, -1, 1), scale_rows=-(-pv // 3)), want, "column scale from column q+1")
        _fails_exact(G.tn_expected("col_scale", acc, pv, scale=sc, scale_rows=-(-pv // 3) + 1), want, "scale_rows off by one")


# ------------------------------------------------------------------------------------------------ plan pins
def _nt_args(c, form, variant, pv, splitk_ws):
    a = L.GemmArgs()
    a.A = a.B = a.C = PTR
    a.M, a.N, a.K, a.batch, a.alpha, a.beta = c.M, c.N, c.K, c.batch, form.alpha, form.beta
    a.lda, a.ldb, a.ldc = c.lda, c.K + 8, c.N + 8
    a.c_is_f32, a.accumulate, a.variant, a.p_valid = int(form.c_f32), int(form.accumulate), variant, pv
    a.epilogue = {"none": L.EPI_NONE, "gelu": L.EPI_GELU, "dgelu": L.EPI_DGELU, "gelu_grad": L.EPI_GELU_GRAD, "mul_aux": L.EPI_MUL_AUX}[form.epilogue]
    a.residual_first = int(form.res_first)
    if form.bias:
        a.bias = PTR
    if form.residual:
        a.residual, a.ldr = PTR, c.N + 8
    if form.epilogue in ("dgelu", "gelu_grad", "mul_aux") or form.aux_out:
        a.aux, a.ldaux = PTR, c.N + 8
    if form.colsum:
        a.colsum = PTR
    if form.valid:
        a.valid_rows_period, a.valid_rows = form.valid
    if splitk_ws:
        a.workspace, a.workspace_bytes = PTR, 1 << 30
    return a


def test_nt_cases_reach_their_kinds():
    h = L.load()
    seen = set()
    for c in G.NT_CASES:
        first = _nt_args(c, G.FORMS[c.forms[0]], 0, c.p_valid[0], True)
        assert (int(h.wft_gemm_nt_variant(ctypes.byref(first))), int(h.wft_gemm_nt_splitk_workspace_bytes(ctypes.byref(first)))) == c.answers, c.name
        assert G.nt_plan(c.M, c.N, c.K, c.batch, G.FORMS[c.forms[0]], 0, c.p_valid[0], c.lda)[0] == c.kind, c.name
        for fname, variant, launch, pv, kind in G.nt_runs(c):
            a = _nt_args(c, G.FORMS[fname], variant, pv, True)
            rule = G.nt_plan(c.M, c.N, c.K, c.batch, G.FORMS[fname], variant, pv, c.lda)
            got = (int(h.wft_gemm_nt_variant(ctypes.byref(a))), int(h.wft_gemm_nt_splitk_workspace_bytes(ctypes.byref(a))))
            assert got == rule[1:] and rule[0] == kind, (c.name, fname, variant, pv, got, rule)
            if fname in c.forms256:
                assert kind == "NT_256", (c.name, fname, kind)
            if fname in c.forms and variant == 0:
                assert kind == c.kind, (c.name, fname, kind)
            if G.FORMS[fname].colsum:
                assert (int(h.wft_gemm_nt_colsum_workspace_bytes(ctypes.byref(a))) > 0) == (kind in ("NT_4W", "NT_256")), (c.name, fname)
            seen.add(kind)
    assert seen == set(G.NT_KINDS)
    # ring versus two-buffer is the tile count against the CU count
    for c in G.NT_CASES:
        if c.kind in ("NT_128_RING", "NT_128_2BUF"):
            assert (-(-c.M // 128) * (c.N // 128) * c.batch <= G.NCU) == (c.kind == "NT_128_RING"), c.name


def _tn_args(c, R, pv, workspace, segs=0, reduce_form=False):
    a = L.GemmArgs()
    a.A = a.B = a.C = PTR
    a.M, a.N, a.K, a.batch, a.alpha, a.beta = c.P, c.Q, R, c.batch, 1.0, 1.0
    a.lda, a.ldb, a.ldc = c.P + 8, c.Q + 8, c.Q + 8
    a.c_is_f32, a.variant, a.p_valid = int(c.c_f32), c.variant, pv
    if reduce_form:
        a.tn_col_scale, a.tn_scale_rows = PTR, 1
    if segs:
        a.tn_seg_count = segs
        for i in range(segs):
            a.tn_seg_end[i], a.tn_seg_ptr[i] = c.P * (i + 1) // segs, PTR
    if workspace:
        a.workspace, a.workspace_bytes = PTR, 1 << 30
    return a


def test_tn_cases_reach_their_kinds():
    h = L.load()
    seen = set()
    for c in G.TN_CASES:
        segs = 3 if "seg3" in c.forms else 0
        bare, granted = _tn_args(c, c.R, c.p_valid[0], False, segs), _tn_args(c, c.R, c.p_valid[0], True, segs)
        got = (int(h.wft_gemm_tn_workspace_bytes(ctypes.byref(bare))), int(h.wft_gemm_tn_variant(ctypes.byref(bare))), int(h.wft_gemm_tn_variant(ctypes.byref(granted))))
        assert got == c.answers, (c.name, got)
        if segs:
            assert int(h.wft_gemm_tn_segments_ok(ctypes.byref(granted))) == 1
        for R in [c.R] + c.ragged():
            for pv in c.p_valid:
                for reduce_form in ((False, True) if "col_scale" in c.forms else (False,)):
                    plan = G.tn_plan(R, c.P, c.Q, c.batch, c.c_f32, c.variant, pv, reduce_form, segs, c.workspace)
                    a = _tn_args(c, R, pv, c.workspace, segs, reduce_form)
                    got = (int(h.wft_gemm_tn_workspace_bytes(ctypes.byref(a))), int(h.wft_gemm_tn_variant(ctypes.byref(a))))
                    assert got == (plan["ws_bytes"], plan["variant"]), (c.name, R, pv, got, plan)
                    if not reduce_form:
                        assert plan["kind"] == c.kind, (c.name, R, pv, plan)
                    seen.add(plan["kind"])
        assert len(c.ragged()) >= 3, c.name
    assert seen == set(G.TN_KINDS)


# ------------------------------------------------------------------------------------------------ the GELU constant
def _gelu_pres():
    """the pre-activations of the table's GELU forms (seed 0): fl32(alpha acc + bias), and the saved ones DGELU reads"""
    out = []
    for c in G.NT_CASES:
        for fname in c.forms + c.forms256:
            form = G.FORMS[fname]
            if form.exact or c.M * c.N > 9_000_000:
                continue
            e = G.nt_epilogue_operands(c, form, 0)
            out.append(e.aux[:, :c.M].reshape(-1) if form.epilogue == "dgelu" else
                       (form.alpha * _nt(c.name, 0)[1] + e.bias.double()).float().reshape(-1))
    for M, N, K in G.STREAM_CASES:
        ops, e = G.stream_operands(M, N, K, 0)
        out.append((G.nt_acc(ops) + e.bias.double()).float().reshape(-1))
    return torch.cat(out)[::5].contiguous()   # every fifth: 11 million values


def test_the_gelu_constant_is_twice_the_worst_fp32_error_and_the_docstring_says_so():
    x = _gelu_pres()
    x64 = x.double()
    w = 1.0 + x64.abs()
    g2, d2 = G.gelu_both_f32(x)
    errs = {"gelu_f": ((G.gelu_f32(x).double() - G.gelu64(x64)).abs() / w).max().item(),
            "dgelu_f": ((G.dgelu_f32(x).double() - G.dgelu64(x64)).abs() / w).max().item(),
            "gelu_both_f (gelu)": ((g2.double() - G.gelu64(x64)).abs() / w).max().item(),
            "gelu_both_f (gelu')": ((d2.double() - G.dgelu64(x64)).abs() / w).max().item()}
    worst = max(errs.values())
    c = 2.0 ** math.ceil(math.log2(2 * worst))
    print(f"{x.numel()} pre-activations in [{x.min().item():.1f}, {x.max().item():.1f}]: worst |fp32 - fp64| / (1 + |pre|) = "
          + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f"; GELU_C = 2 x {worst:.3e} rounded up = 2^{math.log2(c):.0f}")
    assert x.abs().max() > 4 and (x.abs() < 0.5).float().mean() > 0.02   # varied: the flat tails and the curved middle
    assert c == G.GELU_C
    m = re.search(r"GELU_C = 2\^(-\d+): measured.*?= ([0-9.e-]+), doubled", G.__doc__, re.S)
    assert m and 2.0 ** int(m.group(1)) == G.GELU_C and abs(float(m.group(2)) - worst) <= 0.05 * worst, (m and m.groups(), worst)
