"""wft_gemm_nt_i8 (csrc/gemm_i8.hip) on the GPU, against the numpy restatement of tests/_i8_cases.py.

The accumulation is exact integer arithmetic, so the plain / bias / bias + residual forms are held to the reference BIT FOR BIT over
the whole case table, inside a C buffer with ldc > N and guard rows behind M whose sentinels must survive; the operands carry poison
in their pad columns.  tests/test_gemm_i8_host.py shows that each of eleven wrong kernels changes a bit of such a comparison
somewhere in the table — this is also the check of the int8 MFMA's operand lane map (an asymmetric B, distinct k-blocks).  The GELU
forms go through the kernel's erf approximation and are held to the per-element bound of _i8_cases.gelu_bound (the pre-activation is
exact: no dot-product term).  Measured on an MI355X: every exact form equal bit for bit; GELU forms, largest error / bound 0.984-0.996 (the
bound's own bf16 rounding term)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _i8_cases as I8  # noqa: E402
from tests import _q8_cases as Q8  # noqa: E402
from tests.test_kernels_gpu import DEV  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

BF16 = torch.bfloat16
TABLE = I8.table()
IDS = [t[0] for t in TABLE]
_DEV = {}


def _dev(name, case):
    """The operands of a case on the device, once per case: the full padded int8 buffers, the scales, bias, residual."""
    if name not in _DEV:
        t = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731  (a copy: the cases are read-only)
        _DEV[name] = dict(A=t(case["A"]), B=t(case["B"]), a_scale=t(case["a_scale"]), b_scale=t(case["b_scale"]), bias=t(case["bias"]),
                          res=t(case["res"]).to(BF16))
    return _DEV[name]


def _run(case, d, form, rows=None):
    """One call into a fresh sentinel-filled C buffer [M + guard, ldc] -> the whole buffer as f32 on the host."""
    M, N, Kd = case["M"] if rows is None else rows, case["N"], case["K"]
    flags = I8.FORMS[form]
    cbuf = torch.full((M + I8.GUARD_ROWS, case["ldc"]), float(I8.SENTINEL), dtype=BF16, device=DEV)
    out = K.gemm_nt_i8(d["A"][:M, :Kd], d["a_scale"][:M], d["B"][:, :Kd], d["b_scale"], bias=d["bias"] if flags["bias"] else None,
                       residual=d["res"][:M] if flags["res"] else None, epilogue=L.EPI_GELU if flags["gelu"] else L.EPI_NONE,
                       out=cbuf[:M, :N])
    assert out.data_ptr() == cbuf.data_ptr()
    torch.cuda.synchronize()
    return cbuf.float().cpu().numpy()


@pytest.mark.parametrize("entry", TABLE, ids=IDS)
def test_i8_gemm_against_the_reference(entry):
    name, kw, form = entry
    case = I8.make_case(**kw)
    d = _dev(name, case)
    M, N = case["M"], case["N"]
    flags = I8.FORMS[form]
    forms = [form] + ([f for f in I8.EXACT_FORMS if f != form] if kw.get("kind") else [])  # the two special cases: every exact form
    for f in forms:
        fl = I8.FORMS[f]
        got = _run(case, d, f)
        assert (got[M:] == I8.SENTINEL).all(), "guard rows behind M were written"
        assert (got[:, N:] == I8.SENTINEL).all(), "columns between N and ldc were written"
        if not fl["gelu"]:
            want = I8.reference(case, **fl)
            bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (name, f, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
        else:
            target, bound = I8.gelu_bound(case, bias=fl["bias"], res=fl["res"])
            ratio = float((np.abs(got[:M, :N].astype(np.float64) - target) / bound).max())
            print(f"{name}: largest |kernel - f64 gelu of the exact pre-activation| / bound = {ratio:.3f}")
            assert ratio <= 1.0, (name, ratio)
    if kw.get("kind") == "deep":
        m, n = case["tie"]
        assert got is not None and I8.reference(case, **flags)[m, n] != I8.reference(case, mutant="truncating_cvt", **flags)[m, n]


def test_row_m_does_not_depend_on_m_and_two_runs_agree():
    """Rows 0..126 of the M = 257 product are the bits of the M = 127 run on the same rows (a ragged single tile against the first
    of three); a second run of each gives the same bits."""
    kw = dict(M=257, N=384, K=320, scales="general")
    case = I8.make_case(**kw)
    d = _dev("rows-257x384x320", case)
    for form in ("bias_res", "gelu_bias_res"):
        full = _run(case, d, form)
        again = _run(case, d, form)
        assert np.array_equal(full.view(np.uint32), again.view(np.uint32)), form
        part = _run(case, d, form, rows=127)
        assert np.array_equal(part[:127, :384].view(np.uint32), full[:127, :384].view(np.uint32)), form
        assert (part[127:] == I8.SENTINEL).all() and (part[:, 384:] == I8.SENTINEL).all()
        assert np.array_equal(part.view(np.uint32), _run(case, d, form, rows=127).view(np.uint32)), form


def test_quantiser_on_an_activation_shaped_matrix():
    """The existing wft_quantize_rows_i8, unchanged, at a row count that is no multiple of 4 (its workgroup holds four rows) and
    far above a weight's: 4097 x 1280, the structured rows of _q8_cases.quantizer_rows tiled.  Bytes and scales equal the numpy
    restatement."""
    rows = np.tile(Q8.quantizer_rows(1280), (456, 1))[:4097]
    x = torch.from_numpy(rows).to(DEV).to(BF16)
    q, s = K.quantize_rows_i8(x)
    torch.cuda.synchronize()
    want_q, want_s = Q8.quantize_rows(rows)
    assert q.shape == (4097, 1280) and s.shape == (4097,)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), want_s.view(np.uint32))
    bad = np.argwhere(q.cpu().numpy() != want_q)
    assert bad.size == 0, bad[:5]


def test_quantiser_then_gemm_is_the_fake_quantised_product():
    """The path ops.linear takes: quantise x, multiply with a quantised weight — equal, bit for bit, to the reference on the
    restated quantiser's bytes and scales."""
    rng = np.random.default_rng(5)
    x = Q8.bf16_round(rng.standard_normal((45, 384), dtype=np.float32) * 2)
    w = Q8.bf16_round(rng.standard_normal((256, 384), dtype=np.float32) * 0.05)
    xq, xs = K.quantize_rows_i8(torch.from_numpy(x).to(DEV).to(BF16))
    wq, ws = K.quantize_rows_i8(torch.from_numpy(w).to(DEV).to(BF16))
    got = K.gemm_nt_i8(xq, xs, wq, ws).float().cpu().numpy()
    a, sa = Q8.quantize_rows(x)
    b, sb = Q8.quantize_rows(w)
    acc = (a.astype(np.int64) @ b.astype(np.int64).T).astype(np.float32)
    want = Q8.bf16_round((acc * (sa[:, None] * sb[None, :]).astype(np.float32)).astype(np.float32))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_refusals_reach_python_with_their_reason():
    a = torch.zeros(40, 384, dtype=torch.int8, device=DEV)
    b = torch.zeros(256, 384, dtype=torch.int8, device=DEV)
    sa, sb = torch.ones(40, device=DEV), torch.ones(256, device=DEV)
    assert K.gemm_nt_i8(a, sa, b, sb).shape == (40, 256)
    with pytest.raises(L.WftError, match="not served.*epilogue"):
        K.gemm_nt_i8(a, sa, b, sb, epilogue=L.EPI_DGELU)
    with pytest.raises(L.WftError, match="not served.*K must be a multiple of 64"):
        K.gemm_nt_i8(a[:, :96], sa, b[:, :96], sb)
    with pytest.raises(L.WftError, match="not served.*N must be a multiple of 128"):
        K.gemm_nt_i8(a, sa, b[:192], sb)
    with pytest.raises(L.WftError, match="not served.*16-byte aligned"):
        K.gemm_nt_i8(a[:, 8:72], sa, b[:, :64], sb)
    with pytest.raises(L.WftError, match="not served.*ldc"):
        K.gemm_nt_i8(a, sa, b, sb, out=torch.zeros(40, 258, dtype=BF16, device=DEV)[:, :256])
    with pytest.raises(L.WftError, match="16-byte aligned vectors"):
        K.gemm_nt_i8(a, torch.ones(41, device=DEV)[1:], b, sb)
    with pytest.raises((L.WftError, TypeError, ValueError)):
        K.gemm_nt_i8(a.to(BF16), sa, b, sb)
    assert not K.gemm_nt_i8_serves(40, 256, 96) and not K.gemm_nt_i8_serves(40, 192, 384) and K.gemm_nt_i8_serves(40, 256, 384)
    # the symbols exist in the loaded library with their restypes (a missing one is the failure on a library without the kernel)
    h = L.load()
    assert h.wft_gemm_nt_i8_ok(C.byref(K._i8_shape_args(1, 128, 64, L.EPI_NONE))) == 1
