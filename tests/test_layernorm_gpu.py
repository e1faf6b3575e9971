"""The LayerNorm kernels under the per-element bounds of tests/_layernorm_cases.py (whose docstring has the cases, the float64
reference, the bound forms and how their constants were measured; tests/test_layernorm_host.py proves on the CPU that the same
checker rejects every listed mutant of the kernels' arithmetic): K.layernorm_fwd / K.layernorm_bwd on every width and row count of
bf16_cases(), plain and under the deep-SpecAugment spans, through the host-span and the device-span entry points, in the four
want_colsum x want_params combinations, each launched twice; the two sizes at which the non-temporal variant takes over, each
against its neighbour one row smaller; wft_layernorm_fwd_f32 / wft_layernorm_bwd_f32 through the C ABI and through
ops32.LayerNormFn; the argument checks.  The reference is computed on the device in float64.  Each test prints the worst
|err| / bound it saw per output and the running worst of its case family; above 1 it fails.

Measured on an MI355X, worst |err| / bound per output and case family (the bound with the K in force; y and dx of the bf16 kernels
include the half ulp of bf16, which round-to-nearest of the reference alone can use up):
  plain:                   y 1.000, dx 1.000, mean 0.124, rstd 0.189, dgamma 0.151, dbeta 0.020, dxsum 0.185
  span (a):                y 1.000, dx 1.000, mean 0.124, rstd 0.180, dgamma 0.045, dbeta 0.017, dxsum 0.068
  span (b):                y 1.000, dx 1.000, mean 0.124, rstd 0.180, dgamma 0.039, dbeta 0.017, dxsum 0.059
  span (c):                y 1.000, dx 1.000, mean 0.124, rstd 0.180, dgamma 0.034, dbeta 0.020, dxsum 0.050
  span (d):                y 1.000, dx 1.000, mean 0.124, rstd 0.180, dgamma 0.034, dbeta 0.020, dxsum 0.064
  span (e):                y 0.000, dx 0.000, mean 0.124, rstd 0.180, dgamma 0.000, dbeta 0.000, dxsum 0.015
  threshold:               y 1.000, dx 1.000, mean 0.091, rstd 0.163, dgamma 0.000, dbeta 0.013, dxsum 0.011
  fp32 twin, fp32 values:  y 0.141, dx 0.244, mean 0.142, rstd 0.165, dgamma 0.222, dbeta 0.243
  fp32 twin, bf16 values:  y 0.075, dx 0.229, mean 0.062, rstd 0.204, dgamma 0.172, dbeta 0.015
No output of any case reaches its bound: the kernels needed no fix.  The statistics land where the CPU restatement does (mean
0.124 x 8 = 0.99 F against 0.996 F restated; fp32 twin 0.142 x 8 = 1.14 F against 1.135 F).
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _layernorm_cases as N  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402
from whisper_finetune.engine import ops32  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16
PLAIN = tuple(c for c in N.bf16_cases() if not c.span)
SPANS = tuple(c for c in N.bf16_cases() if c.span)
F32 = N.f32_cases()
NAMES = ("y", "mean", "rstd", "dx", "dgamma", "dbeta", "dxsum")
WORST = {}


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _note(family, name, r):
    w = WORST.setdefault(family, {})
    for k, v in r.items():
        w[k] = max(w.get(k, 0.0), v)
    print(f"{family} {name}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    print(f"  so far, {family}: " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b, what):
    assert len(a) == len(b)
    for name, u, v in zip(NAMES, a, b):
        assert (u is None) == (v is None) and (u is None or torch.equal(_bits(u), _bits(v))), f"{what}: {name} differs"


@functools.lru_cache(maxsize=1)
def _dev(rows, cols, offset, seed, exact=False):
    """the operands of a shape on the device: f32 (for the reference) and bf16 (for the kernels); the span cases of a shape share
    them, and with them what the reference takes from x alone"""
    d = {k: v.to(DEV) for k, v in N._inputs(rows, cols, offset, seed, exact).items()}
    if not exact:
        d.update({k + "b": d[k].to(BF16) for k in ("x", "dy", "dres")})
    return d


def _operands(c, exact=False):
    return _dev(c.rows, c.cols, c.offset, c.seed, exact)


def _launch(d, mask):
    """forward, then the backward in its four want_colsum x want_params combinations, everything twice -> (y, mean, rstd, dx,
    dgamma, dbeta, dxsum) after asserting what has to be bit-equal: the two launches of everything, dx across the four
    combinations, dgamma / dbeta and the dx sums across the two combinations that return them"""
    fwd = K.layernorm_fwd(d["xb"], d["gamma"], d["beta"], N.EPS, mask)
    again = K.layernorm_fwd(d["xb"], d["gamma"], d["beta"], N.EPS, mask)
    _same_bits((*fwd, None, None, None, None), (*again, None, None, None, None), "two forward launches")
    y, mean, rstd = fwd
    got = {}
    for colsum in (False, True):
        for params in (True, False):
            def bwd():
                r = K.layernorm_bwd(d["dyb"], d["xb"], d["gamma"], mean, rstd, d["dresb"], mask, want_colsum=colsum, want_params=params)
                assert (r[1] is None) == (not params) and (r[2] is None) == (not params) and len(r) == (4 if colsum else 3)
                return (None, None, None, *r, *(() if colsum else (None,)))
            got[colsum, params] = bwd()
            _same_bits(got[colsum, params], bwd(), f"two backward launches, want_colsum={colsum}, want_params={params}")
    full = got[True, True]
    for key, o in got.items():
        assert torch.equal(_bits(o[3]), _bits(full[3])), f"dx of want_colsum, want_params = {key} differs from (True, True)"
    _same_bits(got[False, True], (*full[:6], None), "dgamma / dbeta with and without the dx sums")
    assert torch.equal(_bits(got[True, False][6]), _bits(full[6])), "dx sums with and without dgamma / dbeta"
    return (y, mean, rstd, *full[3:])


def _as_out(t):
    return {k: (v.float() if v.dtype == BF16 else v) for k, v in zip(NAMES, t)}


@pytest.mark.parametrize("i", range(len(PLAIN)), ids=[c.name for c in PLAIN])
def test_bf16_kernels_within_the_element_bounds(i):
    c = PLAIN[i]
    d = _operands(c)
    out = _launch(d, None)
    _note("plain", c.name, N.check(c.name, N.reference(d), _as_out(out), N.depth_bf16(c.rows), what="bf16 kernels"))


@pytest.mark.parametrize("i", range(len(SPANS)), ids=[c.name for c in SPANS])
def test_bf16_kernels_under_a_span(i):
    c = SPANS[i]
    d = _operands(c)
    rpb, t0, t1, c0, c1 = c.mask
    out = _launch(d, c.mask)
    span = torch.tensor(c.mask[1:], dtype=torch.int32, device=DEV)
    _same_bits(out, _launch(d, (rpb, span)), "span in device memory against span in the arguments")
    if c.span == "d":   # both spans empty, rows_per_batch > 0: the unmasked result
        _same_bits(out, _launch(d, None), "empty spans against mask=None")
    ref = N.reference(d, c.mask)
    y, _, _, dx, dgamma, dbeta, _ = out
    if ref["masked"] is not None and c.span != "d":
        assert ref["masked"].any() and (_bits(y)[ref["masked"]] == 0).all(), "a masked y is not +0"
        assert (_bits(dgamma)[c0:c1] == 0).all() and (_bits(dbeta)[c0:c1] == 0).all(), "dgamma / dbeta of a masked column is not 0"
        t = torch.arange(c.rows, device=DEV) % rpb
        trow = (t >= t0) & (t < t1) if c.span != "e" else torch.ones_like(t, dtype=torch.bool)
        assert c.span == "c" or trow.any()
        assert torch.equal(_bits(dx)[trow], _bits(d["dresb"])[trow]), "dx of a row without gradient is not the residual gradient's bits"
    _note(c.family, c.name, N.check(c.name, ref, _as_out(out), N.depth_bf16(c.rows), what="bf16 kernels"))


@pytest.mark.parametrize("rows,cols", [(16384, 2048), (127101, 264)])
def test_the_non_temporal_variant_against_its_neighbour(rows, cols):
    """csrc/norm.hip switches to the non-temporal loads and stores (VAR 2) at rows x cols x 2 >= 64 MiB; the library does not report
    which variant ran, so the sizes sit on both sides of that constant: 16384 x 2048 and 127101 x 264 (67 109 328 bytes) run VAR 2,
    16383 x 2048 and 127100 x 264 (67 108 800 bytes) run VAR 1 forward and VAR 0 backward, on the first rows - 1 rows of the same
    tensors.  Rows are independent of the grid and of the variant: y, mean, rstd and dx of the common rows are bit-equal.  Both
    launches: three 256-row slabs (first, middle, last) against the float64 reference; dgamma, dbeta and the dx sums against
    float64 sums over all rows, chunked on the device.  Inputs are made on the device, rows of the kinds of every other case."""
    assert rows * cols * 2 >= 64 << 20 > (rows - 1) * cols * 2
    gen = torch.Generator(device=DEV).manual_seed(rows)
    gamma = 1 + 0.5 * torch.randn(cols, generator=gen, device=DEV)
    beta = torch.randn(cols, generator=gen, device=DEV)
    x, dy, dres = N.make_rows(rows, cols, 3, gen, device=DEV)
    outs = {}
    for n in (rows, rows - 1):
        d = {"x": x[:n], "dy": dy[:n], "dres": dres[:n], "gamma": gamma, "beta": beta}
        d.update({k + "b": d[k].to(BF16) for k in ("x", "dy", "dres")})
        out = outs[n] = _launch(d, None)
        res = _as_out(out)
        r = {}
        for r0, r1 in ((0, 256), (n // 2 - 128, n // 2 + 128), (n - 256, n)):
            got = N.check(f"{n}x{cols} rows {r0}..{r1}", N.reference(d, None, r0, r1), {k: res[k] for k in ("y", "mean", "rstd", "dx")}, 1,
                          rows=slice(r0, r1), what="bf16 kernels")
            r = {k: max(v, r.get(k, 0.0)) for k, v in got.items()}
        sums = None
        for r0 in range(0, n, 8192):
            part = N.reference(d, None, r0, min(r0 + 8192, n), per_row=False)
            part.pop("masked")
            sums = part if sums is None else {k: sums[k] + part[k] for k in part}
        r.update(N.check(f"{n}x{cols}", sums, {k: res[k] for k in ("dx", "dgamma", "dbeta", "dxsum")}, N.depth_bf16(n), skip=("dx",),
                         what="bf16 kernels"))
        _note("threshold", f"{n}x{cols}", r)
    big, small = outs[rows], outs[rows - 1]
    for name, a, b in zip(NAMES[:4], big, small):
        assert torch.equal(_bits(a[:rows - 1]), _bits(b)), f"{name} of the common rows differs between the two variants"


# ------------------------------------------------------------------------------------------------ fp32 twins
def _f32_abi(d, rows, cols, mask):
    h = L.load()
    arr = None if mask is None else (C.c_int32 * 5)(*mask)
    y, dx = torch.empty_like(d["x"]), torch.empty_like(d["x"])
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    dg, db = torch.empty(cols, device=DEV), torch.empty(cols, device=DEV)
    L.check(h.wft_layernorm_fwd_f32(_p(d["x"]), _p(d["gamma"]), _p(d["beta"]), _p(y), _p(mean), _p(rstd), rows, cols, N.EPS, arr, L.stream_ptr()),
            "wft_layernorm_fwd_f32")
    L.check(h.wft_layernorm_bwd_f32(_p(d["dy"]), _p(d["x"]), _p(d["gamma"]), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db), rows, cols, arr,
                                    L.stream_ptr()), "wft_layernorm_bwd_f32")
    return {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dgamma": dg, "dbeta": db}


@pytest.mark.parametrize("i", range(len(F32)), ids=[c.name for c in F32])
def test_f32_twins_within_the_element_bounds(i):
    c = F32[i]
    for exact in (True, False):
        d = dict(_operands(c, True) if exact else {k: v for k, v in _operands(c).items() if not k.endswith("b")})
        d["dres"] = None   # the fp32 mode adds the residual gradient elsewhere
        out = _f32_abi(d, c.rows, c.cols, c.mask)
        ref = N.reference(d, c.mask)
        if ref["masked"] is not None:
            assert (_bits(out["y"])[ref["masked"]] == 0).all(), "a masked y is not +0"
            assert (out["dgamma"][c.mask[3]:c.mask[4]] == 0).all() and (out["dbeta"][c.mask[3]:c.mask[4]] == 0).all()
        _note(f"fp32 twin, {'fp32' if exact else 'bf16'} values", c.name, N.check(c.name, ref, out, c.rows, fp32_mode=True, what="fp32 twins"))
        if c.rows == 50:   # the autograd function of the fp32 mode hands back the same bits
            x, g, b = (d[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
            y = ops32.LayerNormFn.apply(x.view(5, 10, c.cols), g, b, N.EPS, c.mask)
            y.backward(d["dy"].view(5, 10, c.cols))
            for name, t in (("y", y.detach().view(50, c.cols)), ("dx", x.grad), ("dgamma", g.grad), ("dbeta", b.grad)):
                assert torch.equal(_bits(t), _bits(out[name])), f"ops32.LayerNormFn: {name} differs from the C ABI's"


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("rows,cols", [(4, 4), (4, 12), (4, 2056), (0, 8)])
def test_argument_checks_raise_and_leave_the_outputs_untouched(rows, cols):
    h = L.load()
    n = max(rows, 1)
    x = torch.ones(n, cols, dtype=BF16, device=DEV)
    gamma, beta = torch.ones(cols, device=DEV), torch.zeros(cols, device=DEV)
    stats = torch.ones(n, device=DEV)
    span = torch.zeros(4, dtype=torch.int32, device=DEV)
    ws = torch.empty((512 + 16) * 3 * cols * 4, dtype=torch.uint8, device=DEV)
    for dspan in (False, True):
        y, dx = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
        mean, rstd = torch.full((n,), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)
        dg, db, dxs = (torch.full((cols,), 7.0, device=DEV) for _ in range(3))
        if dspan:
            st_f = h.wft_layernorm_fwd_dspan(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, cols, N.EPS, 7, _p(span), L.stream_ptr())
            st_b = h.wft_layernorm_bwd_dspan(_p(x), _p(x), _p(gamma), _p(stats), _p(stats), _p(x), _p(dx), _p(dg), _p(db), _p(dxs), _p(ws), rows,
                                             cols, 7, _p(span), L.stream_ptr())
        else:
            st_f = h.wft_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, cols, N.EPS, 0, 0, 0, 0, 0, L.stream_ptr())
            st_b = h.wft_layernorm_bwd(_p(x), _p(x), _p(gamma), _p(stats), _p(stats), _p(x), _p(dx), _p(dg), _p(db), _p(dxs), _p(ws), rows, cols,
                                       0, 0, 0, 0, 0, L.stream_ptr())
        for st, what in ((st_f, "wft_layernorm_fwd"), (st_b, "wft_layernorm_bwd")):
            with pytest.raises(L.WftError, match="cols must be a multiple of 8"):
                L.check(st, what)
        torch.cuda.synchronize()
        for t in (y, dx, mean, rstd, dg, db, dxs):
            assert (t == 7.0).all(), "a refused call wrote to an output"
    xs = torch.ones(rows, cols, dtype=BF16, device=DEV)
    with pytest.raises(L.WftError):
        K.layernorm_fwd(xs, gamma, beta)
    for colsum, params in ((False, True), (True, False), (False, False)):
        with pytest.raises(L.WftError):
            K.layernorm_bwd(xs, xs, gamma, torch.ones(rows, device=DEV), torch.ones(rows, device=DEV), xs, want_colsum=colsum, want_params=params)
