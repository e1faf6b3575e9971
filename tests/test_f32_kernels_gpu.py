"""The fp32 parity-mode kernels of csrc/f32.hip, element by element, against the references of tests/_f32_cases.py (whose docstring
says why each check is exact or how its bound was counted; tests/test_f32_host.py proves the premises and rejects the mutants on the
CPU): wft_gemm_f32 through ops32.gemm on poisoned flat buffers, the stride recipes of ops32 through LinearFn / ConvStemFn /
TiedLogitsFn, wft_softmax_fwd_f32 / _bwd_f32, wft_gelu_*_f32, wft_axpby_f32 and wft_colsum_f32 through the C ABI, and every
WFT_CHECK_ARG refusal.  Each non-exact test prints the worst utilisation of its bound (worst ratio / constant) before it asserts.

Measured on an MI355X: every bitwise comparison holds (GEMM under all four stagings, the gather probes, the restated recipes, LinearFn,
ConvStemFn with its premise, TiedLogitsFn, colsum, the one-operand and (1, 1) axpby, the second grid-stride trip); utilisation of the
counted bounds: softmax forward 0.056 (cols 130), backward 0.213 (cols 65), GELU forward 0.146, backward 0.122.  The two-operand axpby
reaches 0.70 of u (|a x| + |b y| + |ref|): above one half, as it must be for a bound that is the plain sum of the three roundings of the
uncontracted form with no constant in front; it says nothing against the kernel.  The kernels needed no fix."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _f32_cases as S  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402
from whisper_finetune.engine import ops32  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
NAN = float("nan")
_p = ops32._p


# ------------------------------------------------------------------------------------------------ wft_gemm_f32
def _run_gemm(op):
    """the call ops32 makes, on the flat poisoned buffers; -> the whole flat C buffer"""
    case = op.case
    a, b, c = op.a_flat.to(DEV), op.b_flat.to(DEV), op.c_flat.to(DEV)
    (a_bs, a_rs, a_cs), (b_bs, b_rs, b_cs), (c_bs, ldc, c_cs) = case.la.strides, case.lb.strides, case.lc.strides
    assert c_cs == 1
    ops32.gemm(a[case.la.off:], b[case.lb.off:], M=case.M, N=case.N, K=case.K, a_strides=(a_rs, a_cs, a_bs), b_strides=(b_rs, b_cs, b_bs),
               out=c[case.lc.off:], ldc=ldc, c_bs=c_bs, batch=case.la.shape[0], bias=None if op.bias is None else op.bias.to(DEV),
               alpha=case.alpha, beta=case.beta)
    return c.cpu()


def _hold_gemm(op, want=None):
    report = S.gemm_mismatch(_run_gemm(op), S.gemm_expected(op) if want is None else want, op.case)
    assert report is None, f"poison {op.poison}: {report}"


@pytest.mark.parametrize("shape", S.GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_integer_operands_exact(shape):
    for case in S.gemm_cases(*shape):
        for seed in S.SEEDS:
            for poison in S.POISONS:
                _hold_gemm(S.gemm_operands(case, seed, poison))


@pytest.mark.parametrize("one_hot", "BA")
@pytest.mark.parametrize("shape", S.GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_gather_probe(shape, one_hot):
    for case in S.gather_cases(*shape):
        for seed in S.SEEDS:
            for r, op in enumerate(S.gather_operands(case, seed, S.POISONS[seed], one_hot)):
                _hold_gemm(op, S.gemm_expected(op, S.gather_expected_logical(op, one_hot, r)))


@pytest.mark.parametrize("case", S.GEMM_RECIPES, ids=[c.name for c in S.GEMM_RECIPES])
def test_gemm_ops32_stride_recipes_restated(case):
    for seed in S.SEEDS:
        for poison in S.POISONS:
            _hold_gemm(S.gemm_operands(case, seed, poison))


def _gemm_args(c, **over):
    a = torch.ones(64, device=DEV)
    args = L.GemmF32Args()
    args.A, args.a_rs, args.a_cs, args.a_bs = a.data_ptr(), 4, 1, 16
    args.B, args.b_rs, args.b_cs, args.b_bs = a.data_ptr(), 1, 4, 16
    args.C, args.ldc, args.c_bs = c.data_ptr(), 4, 16
    args.bias = None
    args.M, args.N, args.K, args.batch = 4, 4, 4, 1
    args.alpha, args.beta = 1.0, 0.0
    for k, v in over.items():
        setattr(args, k, v)
    return args, a


@pytest.mark.parametrize("over", [{"A": None}, {"B": None}, {"C": None}, {"M": 0}, {"N": 0}, {"K": 0}, {"batch": 0}, {"M": -1}, {"batch": 65536},
                                  {"M": 65535 * 64 + 1}], ids=str)
def test_gemm_refuses_bad_arguments(over):
    lib = L.load()
    c = torch.full((64,), S.GUARD, device=DEV)
    args, keep = _gemm_args(c, **over)
    assert lib.wft_gemm_f32(C.byref(args), L.stream_ptr()) != 0
    assert lib.wft_gemm_f32(None, L.stream_ptr()) != 0
    with pytest.raises(L.WftError):
        L.check(lib.wft_gemm_f32(C.byref(args), L.stream_ptr()), "wft_gemm_f32")
    torch.cuda.synchronize()
    assert bool((c == S.GUARD).all()), "a refused call wrote C"
    args, keep = _gemm_args(c)                      # and the same table without the override runs
    assert lib.wft_gemm_f32(C.byref(args), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((c[:16] == 4.0).all()) and bool((c[16:] == S.GUARD).all())


# ------------------------------------------------------------------------------------------------ ops32 functions
def _equal(got, ref64, what):
    got, want = got.detach().cpu(), ref64.to(F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: got {got[i].item()!r}, want {want[i].item()!r}")


@pytest.mark.parametrize("case", S.LINEAR_CASES, ids=str)
def test_linear_fn_exact(case):
    for seed in S.SEEDS:
        t, ref = S.linear_case(case, seed)
        d = {k: (None if v is None else v.to(DEV).requires_grad_(k not in ("dy", "mask"))) for k, v in t.items()}
        y = ops32.LinearFn.apply(d["x"], d["w"], d["b"], d["A"], d["B"], S.LINEAR_SCALING, d["mask"])
        y.backward(d["dy"])
        _equal(y, ref["y"], f"{case} y")
        for name, key in (("dx", "x"), ("dw", "w"), ("db", "b"), ("dA", "A"), ("dB", "B")):
            if name in ref:
                _equal(d[key].grad, ref[name], f"{case} seed {seed} {name}")


@pytest.mark.parametrize("case", S.CONV_CASES, ids=str)
def test_conv_stem_fn_exact(case):
    for seed in S.SEEDS:
        t = S.conv_inputs(case, seed)
        ref = S.conv_ref64(t)
        # the premise, on the device: GELU is the identity and its derivative 1.0f on this case's pre-activations
        for name in ("pre1", "pre2"):
            pre = ref[name].to(F32).to(DEV).requires_grad_(True)
            act = ops32.GeluFn.apply(pre)
            assert S.same_bits(act, pre.detach()), f"{case}: the PREMISE failed, not the conv: GeluFn is not the identity on {name}"
            act.backward(torch.ones_like(act))
            assert S.same_bits(pre.grad, torch.ones_like(pre.grad)), f"{case}: the PREMISE failed, not the conv: GELU' is not 1.0f on {name}"
        d = {k: v.to(DEV).requires_grad_(k in ("w1", "b1", "w2", "b2")) for k, v in t.items()}
        out = ops32.ConvStemFn.apply(d["mel"], d["w1"], d["b1"], d["w2"], d["b2"], d["pos"])
        out.backward(d["dx"])
        _equal(out, ref["out"], f"{case} seed {seed} forward")
        for name in ("w1", "b1", "w2", "b2"):
            _equal(d[name].grad, ref["d" + name], f"{case} seed {seed} d{name}")


def test_tied_logits_fn_exact():
    for seed in S.SEEDS:
        t, ref, _ = S.tied_case(seed)
        x, emb = t["x"].to(DEV).requires_grad_(True), t["emb"].to(DEV).requires_grad_(True)
        logits = ops32.TiedLogitsFn.apply(x, emb)
        logits.backward(t["dl"].to(DEV))
        _equal(logits, ref["logits"], "logits")
        _equal(x.grad, ref["dx"], "dx")
        _equal(emb.grad, ref["demb"], "demb")


# ------------------------------------------------------------------------------------------------ softmax
def _p_buffer(case, x):
    p, _ = S.softmax_ref64(case, x)
    buf = torch.full((case.nrows, case.ld), NAN, dtype=F32)
    buf[:, :case.cols] = p.to(F32)
    return buf


@pytest.mark.parametrize("cols", S.SOFTMAX_COLS)
def test_softmax_fwd_bwd_per_element(cols):
    lib = L.load()
    worst_f = worst_b = 0.0
    for case in S.softmax_cases(cols):
        floor = 2.0 ** -126 if case.kind == "span80" else 0.0
        for seed in S.SEEDS:
            x, dp = S.softmax_inputs(case, seed)
            xd = x.to(DEV)
            L.check(lib.wft_softmax_fwd_f32(_p(xd), case.nrows, cols, case.ld, case.scale, int(case.causal), case.rpm, L.stream_ptr()),
                    "wft_softmax_fwd_f32")
            problem, ratio = S.softmax_fwd_check(case, x, xd, floor)
            assert problem is None, f"{case.name} seed {seed} forward: {problem}"
            p32 = _p_buffer(case, x)
            pd, dpd = p32.to(DEV), dp.to(DEV)
            L.check(lib.wft_softmax_bwd_f32(_p(pd), _p(dpd), case.nrows, cols, case.ld, case.scale, L.stream_ptr()),
                    "wft_softmax_bwd_f32")
            problem, ratio_b = S.softmax_bwd_check(case, p32, dp, dpd, floor)
            assert problem is None, f"{case.name} seed {seed} backward: {problem}"
            if case.kind != "span80":
                worst_f, worst_b = max(worst_f, ratio), max(worst_b, ratio_b)
    print(f"softmax cols {cols}: worst utilisation forward {worst_f / S.SOFTMAX_CF:.3f} (ratio {worst_f:.2f} / {S.SOFTMAX_CF}), "
          f"backward {worst_b / S.SOFTMAX_CB:.3f} (ratio {worst_b:.2f} / {S.SOFTMAX_CB})")


def test_softmax_refuses_bad_arguments():
    lib = L.load()
    s = torch.full((4, 8), S.GUARD, device=DEV)
    st = L.stream_ptr()
    fwd_bad = [(None, 4, 8, 8, 1.0, 0, 4), (_p(s), 0, 8, 8, 1.0, 0, 4), (_p(s), 4, 0, 8, 1.0, 0, 4), (_p(s), 4, 8, 7, 1.0, 0, 4),
               (_p(s), 4, 8, 8, 1.0, 1, 0), (_p(s), -1, 8, 8, 1.0, 0, 4)]
    for a in fwd_bad:
        assert lib.wft_softmax_fwd_f32(*a, st) != 0, a
    bwd_bad = [(None, _p(s), 4, 8, 8, 1.0), (_p(s), None, 4, 8, 8, 1.0), (_p(s), _p(s), 0, 8, 8, 1.0), (_p(s), _p(s), 4, 0, 8, 1.0),
               (_p(s), _p(s), 4, 8, 7, 1.0)]
    for a in bwd_bad:
        assert lib.wft_softmax_bwd_f32(*a, st) != 0, a
    torch.cuda.synchronize()
    assert bool((s == S.GUARD).all())


# ------------------------------------------------------------------------------------------------ element-wise
def _guarded(n, fill=S.FILL):
    """an n-element device view with 8 sentinel elements behind it"""
    buf = torch.full((n + 8,), fill, dtype=F32, device=DEV)
    buf[n:] = S.GUARD
    return buf, buf[:n]


def _tail_intact(buf, n, what):
    assert bool((buf[n:] == S.GUARD).all()), f"{what}: wrote behind its {n} elements"


def test_gelu_per_element():
    lib = L.load()
    x = S.gelu_inputs()
    worst_f = worst_b = 0.0
    small = {}
    for n in S.EW_SIZES + (S.PERIOD,):
        xn, dy = S.tiled(x, n), S.gelu_dy(n)
        xd, dyd = xn.to(DEV), dy.to(DEV)
        ybuf, y = _guarded(n)
        L.check(lib.wft_gelu_fwd_f32(_p(xd), _p(y), n, L.stream_ptr()), "wft_gelu_fwd_f32")
        _tail_intact(ybuf, n, f"gelu fwd n = {n}")
        worst_f = max(worst_f, S.gelu_fwd_ratio(xn, y))
        dbuf, dx = _guarded(n)
        L.check(lib.wft_gelu_bwd_f32(_p(dyd), _p(xd), _p(dx), n, L.stream_ptr()), "wft_gelu_bwd_f32")
        _tail_intact(dbuf, n, f"gelu bwd n = {n}")
        worst_b = max(worst_b, S.gelu_bwd_ratio(dy, xn, dx))
        small[n] = (y.cpu(), dx.cpu())
    print(f"gelu: worst utilisation forward {worst_f / S.GELU_CF:.3f} (ratio {worst_f:.2f} / {S.GELU_CF}), "
          f"backward {worst_b / S.GELU_CB:.3f} (ratio {worst_b:.2f} / {S.GELU_CB})")
    assert worst_f <= S.GELU_CF and worst_b <= S.GELU_CB
    y = small[S.PERIOD][0]
    assert S.same_bits(y[:2], S.gelu_f32_cpu(x[:2])) and S.bits(y[1:2]).item() == -2 ** 31, "gelu(-0.0) lost the sign of its zero"


def test_elementwise_second_grid_stride_trip():
    """BIG_N = 65535 x 256 + 300 elements: the last 300 belong to the second trip of the grid-stride loop.  Inputs are PERIOD-periodic,
    so every output must be the PERIOD-sized run's output tiled, bit for bit (that run is judged by the tests above and below)."""
    lib = L.load()
    n, P = S.BIG_N, S.PERIOD
    reps = -(-n // P)
    pat_x, pat_dy = S.gelu_inputs().to(DEV), S.gelu_dy(P).to(DEV)
    x, dy = pat_x.repeat(reps)[:n].contiguous(), pat_dy.repeat(reps)[:n].contiguous()
    obuf, out = _guarded(n)
    small = torch.empty(P, device=DEV)

    def hold(what):
        torch.cuda.synchronize()
        _tail_intact(obuf, n, what)
        want = small.repeat(reps)[:n]
        if not torch.equal(out.view(torch.int32), want.view(torch.int32)):
            raise AssertionError(f"{what}: {S.tiled_mismatch(out.cpu(), small.cpu(), n)}")
        out.fill_(S.FILL)

    L.check(lib.wft_gelu_fwd_f32(_p(pat_x), _p(small), P, L.stream_ptr()), "wft_gelu_fwd_f32")
    L.check(lib.wft_gelu_fwd_f32(_p(x), _p(out), n, L.stream_ptr()), "wft_gelu_fwd_f32")
    hold("gelu fwd")
    L.check(lib.wft_gelu_bwd_f32(_p(pat_dy), _p(pat_x), _p(small), P, L.stream_ptr()), "wft_gelu_bwd_f32")
    L.check(lib.wft_gelu_bwd_f32(_p(dy), _p(x), _p(out), n, L.stream_ptr()), "wft_gelu_bwd_f32")
    hold("gelu bwd")
    a, b = S.AXPBY_PAIRS[1]
    L.check(lib.wft_axpby_f32(a, _p(pat_x), b, _p(pat_dy), _p(small), P, L.stream_ptr()), "wft_axpby_f32")
    L.check(lib.wft_axpby_f32(a, _p(x), b, _p(dy), _p(out), n, L.stream_ptr()), "wft_axpby_f32")
    hold("axpby")
    L.check(lib.wft_axpby_f32(a, _p(pat_x), NAN, None, _p(small), P, L.stream_ptr()), "wft_axpby_f32")
    L.check(lib.wft_axpby_f32(a, _p(x), NAN, None, _p(out), n, L.stream_ptr()), "wft_axpby_f32")
    hold("axpby, one operand")
    del x, dy, obuf, out
    torch.cuda.empty_cache()


def test_axpby_per_element():
    lib = L.load()
    worst = 0.0
    for n in S.EW_SIZES + (S.PERIOD,):
        x, y = S.axpby_inputs(n)
        xd, yd = x.to(DEV), y.to(DEV)
        for a, b in S.AXPBY_PAIRS:
            obuf, out = _guarded(n)
            L.check(lib.wft_axpby_f32(a, _p(xd), b, _p(yd), _p(out), n, L.stream_ptr()), "wft_axpby_f32")
            _tail_intact(obuf, n, f"axpby n = {n}")
            if (a, b) == (1.0, 1.0):
                assert S.same_bits(out, x + y), f"axpby (1, 1), n = {n}"
            else:
                ratio = S.axpby_ratio(a, x, b, y, out)
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"axpby ({a}, {b}), n = {n}: {ratio:.3f} of u (|a x| + |b y| + |ref|)"
            for bb in (b, NAN):      # y == NULL: b is not read, a NaN b included
                obuf, out = _guarded(n)
                L.check(lib.wft_axpby_f32(a, _p(xd), bb, None, _p(out), n, L.stream_ptr()), "wft_axpby_f32")
                _tail_intact(obuf, n, f"axpby one operand n = {n}")
                assert S.same_bits(out, S.f32_scalar(a) * x), f"axpby ({a}, y = NULL, b = {bb}), n = {n}"
    print(f"axpby: worst utilisation of u (|a x| + |b y| + |ref|): {worst:.3f}")


@pytest.mark.parametrize("rows", S.COLSUM_ROWS)
def test_colsum_per_element(rows):
    lib = L.load()
    for cols in S.COLSUM_COLS:
        for kind in ("int", "randn"):
            for seed in S.SEEDS:
                x = S.colsum_input(rows, cols, kind, seed)
                xd = x.to(DEV)
                obuf, out = _guarded(cols)
                L.check(lib.wft_colsum_f32(_p(xd), rows, cols, cols + 3, _p(out), L.stream_ptr()), "wft_colsum_f32")
                _tail_intact(obuf, cols, f"colsum {rows} x {cols}")
                assert S.same_bits(out, S.colsum_expected(x, cols, kind)), f"colsum {rows} x {cols} {kind} seed {seed}"
    x = S.colsum_input(rows, 65, "int", 0)[:, :65].contiguous()
    assert S.same_bits(ops32.colsum(x.to(DEV)), x.double().sum(0).to(F32))     # the wrapper: ld = stride(0)


def test_elementwise_refuse_bad_arguments():
    lib = L.load()
    buf = torch.full((16,), S.GUARD, device=DEV)
    p, st = _p(buf), L.stream_ptr()
    for a in ((None, p, 4), (p, None, 4), (p, p, 0), (p, p, -1)):
        assert lib.wft_gelu_fwd_f32(*a, st) != 0, a
    for a in ((None, p, p, 4), (p, None, p, 4), (p, p, None, 4), (p, p, p, 0)):
        assert lib.wft_gelu_bwd_f32(*a, st) != 0, a
    for a in ((1.0, None, 1.0, p, p, 4), (1.0, p, 1.0, p, None, 4), (1.0, p, 1.0, p, p, 0)):
        assert lib.wft_axpby_f32(*a, st) != 0, a
    for a in ((None, 2, 4, 4, p), (p, 2, 4, 4, None), (p, 0, 4, 4, p), (p, 2, 0, 4, p), (p, 2, 4, 3, p)):
        assert lib.wft_colsum_f32(*a, st) != 0, a
    torch.cuda.synchronize()
    assert bool((buf == S.GUARD).all())
    with pytest.raises(L.WftError):
        L.check(lib.wft_colsum_f32(p, 2, 4, 3, p, st), "wft_colsum_f32")
