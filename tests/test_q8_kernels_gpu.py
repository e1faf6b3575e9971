"""wft_quantize_rows_i8 (csrc/shadow.hip) and wft_gemm_nt_stream_q8 (csrc/gemm_stream.hip) on the GPU.

The quantiser is held to bit equality with its numpy float32 restatement (tests/_q8_cases.py).  The GEMM is held to bit equality
with wft_gemm_nt_stream_bf16 on Q.to(bf16) wherever the scale is a power of two (every int8 value is a bf16 value and a power of two
commutes with every rounding), and to the derived per-element bound of tests/_q8_cases.py against float64 with general scales.
Shapes: tests/_q8_cases.SHAPES, chosen against stream_plan on 256 CUs."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _q8_cases as Q8  # noqa: E402
from tests.test_kernels_gpu import DEV, close  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

BF16 = torch.bfloat16
IDS = lambda s: "x".join(map(str, s))  # noqa: E731
_CASES = {}


def _dev(case):
    """The operands of a case on the device, once per case: x bf16, Q int8, scale / bias f32, res bf16."""
    if "_dev" not in case:
        t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
        case["_dev"] = dict(x=t(case["A"]).to(BF16), Q=t(case["Q"]), scale=t(case["scale"]), bias=t(case["bias"]), res=t(case["res"]).to(BF16))
    return case["_dev"]


def _case(shape, scales="general"):
    if (shape, scales) not in _CASES:
        _CASES[(shape, scales)] = Q8.make_case(*shape, scales=scales)
    return _CASES[(shape, scales)]


def _kw(d, form, rows=slice(None)):
    kw = {}
    if form["bias"]:
        kw["bias"] = d["bias"]
    if form["gelu"]:
        kw["epilogue"] = L.EPI_GELU
    if form["res"]:
        kw["residual"] = d["res"][rows]
    return kw


def _split(x, Q):
    args, _ = K.gemm_nt_stream_q8(x, Q, torch.empty(Q.shape[0], device=DEV), _args_only=True)
    return int(L.load().wft_gemm_nt_stream_q8_workspace_bytes(C.byref(args))) // (x.shape[0] * Q.shape[0] * 4)


# ----------------------------------------------------------------------------- the quantiser
@pytest.mark.parametrize("cols", [64, 128, 1536])
def test_quantiser_is_the_restatement_bit_for_bit(cols):
    """Structured rows (zero row, lossless row, maximum in the last column, ties, ...; 9 rows: the last workgroup has three dead
    waves; 1536 columns: a second pass of the wave) inside guard-filled buffers with padded leading dimensions."""
    rows = Q8.quantizer_rows(cols)
    n = rows.shape[0]
    want_q, want_s = Q8.quantize_rows(rows)
    wbuf = torch.full((n, cols + 8), 3.0, dtype=BF16, device=DEV)
    wbuf[:, :cols] = torch.from_numpy(rows).to(DEV).to(BF16)
    qbuf = torch.full((n + 2, cols + 16), 0x55, dtype=torch.int8, device=DEV)
    sbuf = torch.full((n + 2,), -7.0, dtype=torch.float32, device=DEV)
    L.check(L.load().wft_quantize_rows_i8(wbuf.data_ptr(), n, cols, cols + 8, qbuf[1].data_ptr(), cols + 16, sbuf[1:].data_ptr(),
                                          L.stream_ptr()), "wft_quantize_rows_i8")
    torch.cuda.synchronize()
    got_q, got_s = qbuf[1:n + 1, :cols].cpu().numpy(), sbuf[1:n + 1].cpu().numpy()
    assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32)), (got_s, want_s)
    bad = np.argwhere(got_q != want_q)
    assert bad.size == 0, (bad[:5], got_q[tuple(bad[0])], want_q[tuple(bad[0])])
    assert (qbuf[0] == 0x55).all() and (qbuf[n + 1] == 0x55).all() and (qbuf[:, cols:] == 0x55).all(), "guard bytes around Q were written"
    assert sbuf[0] == -7.0 and sbuf[n + 1] == -7.0, "guard values around scale were written"
    # the wrapper, on contiguous tensors, gives the same
    q2, s2 = K.quantize_rows_i8(wbuf[:, :cols])
    assert torch.equal(q2, qbuf[1:n + 1, :cols]) and torch.equal(s2, sbuf[1:n + 1])


def test_quantiser_on_random_weight_rows_and_its_refusals():
    g = torch.Generator(device=DEV).manual_seed(5)
    w = (torch.randn(517, 384, device=DEV, generator=g) * 0.05).to(BF16)
    q, s = K.quantize_rows_i8(w)
    want_q, want_s = Q8.quantize_rows(w.float().cpu().numpy())
    assert np.array_equal(q.cpu().numpy(), want_q) and np.array_equal(s.cpu().numpy(), want_s)
    lib = L.load()
    qb, sb = torch.empty(4, 96, dtype=torch.int8, device=DEV), torch.empty(4, device=DEV)
    assert lib.wft_quantize_rows_i8(w.data_ptr(), 4, 96, 384, qb.data_ptr(), 96, sb.data_ptr(), L.stream_ptr()) == -1  # WFT_ERR_ARG: cols % 64
    assert lib.wft_quantize_rows_i8(w.data_ptr(), 4, 64, 384, qb.data_ptr(), 72, sb.data_ptr(), L.stream_ptr()) == -1  # ldq % 16
    assert "ldq" in L.last_error()


# ----------------------------------------------------------------------------- the GEMM
@pytest.mark.parametrize("shape", Q8.SHAPES, ids=IDS)
@pytest.mark.parametrize("scales", ["unit", "pow2"])
def test_q8_equals_the_bf16_kernel_on_the_converted_weights(shape, scales):
    """b_scale = 1 and b_scale[n] = 2^e(n): every form gives the bits of wft_gemm_nt_stream_bf16 on Q.to(bf16) * 2^e(n)."""
    case = _case(shape, scales)
    d = _dev(case)
    M, N, _ = shape
    wb = (d["Q"].float() * d["scale"][:, None]).to(BF16)
    assert torch.equal(wb.float(), d["Q"].float() * d["scale"][:, None])  # exact: the premise
    for name, form in Q8.FORMS.items():
        kw = _kw(d, form)
        got = K.gemm_nt_stream_q8(d["x"], d["Q"], d["scale"], **kw)
        want = K.gemm_nt_stream(d["x"], wb, **kw)
        assert got is not None and want is not None and got.shape == (M, N) and got.dtype == BF16
        assert torch.equal(got, want), (shape, scales, name, (got.float() - want.float()).abs().max().item())
    aux_q, aux_b = torch.zeros(M, N, dtype=BF16, device=DEV), torch.zeros(M, N, dtype=BF16, device=DEV)
    got = K.gemm_nt_stream_q8(d["x"], d["Q"], d["scale"], bias=d["bias"], epilogue=L.EPI_GELU, aux=aux_q)
    want = K.gemm_nt_stream(d["x"], wb, bias=d["bias"], epilogue=L.EPI_GELU, aux=aux_b)
    assert torch.equal(got, want) and torch.equal(aux_q, aux_b), "gelu + aux"
    assert torch.equal(got, K.gemm_nt_stream_q8(d["x"], d["Q"], d["scale"], bias=d["bias"], epilogue=L.EPI_GELU)), "storing aux changes C"


@pytest.mark.parametrize("shape", Q8.SHAPES, ids=IDS)
def test_q8_with_general_scales_stays_inside_the_derived_bound(shape):
    case = _case(shape)
    d = _dev(case)
    M, N, _ = shape
    split = _split(d["x"], d["Q"])
    for name, form in Q8.FORMS.items():
        aux = torch.zeros(M, N, dtype=BF16, device=DEV) if form["gelu"] else None
        got = K.gemm_nt_stream_q8(d["x"], d["Q"], d["scale"], aux=aux, **_kw(d, form)).float().cpu().numpy()
        ref, pre = Q8.gemm_ref64(case, **form)
        bound, bound_pre = Q8.gemm_bound(case, split, **form)
        ratio = float((np.abs(got - ref) / bound).max())
        print(f"{shape} {name} split={split}: largest |q8 - f64| / bound = {ratio:.3f}")
        assert ratio <= 1.0, (shape, name, ratio)
        if aux is not None:
            ratio = float((np.abs(aux.float().cpu().numpy() - pre) / bound_pre).max())
            print(f"{shape} {name}: stored pre-activation, largest error / bound = {ratio:.3f}")
            assert ratio <= 1.0, (shape, "aux", ratio)


def test_row_m_does_not_depend_on_the_batch_and_two_runs_agree():
    shape = (32, 51968, 384)
    d = _dev(_case(shape))
    for form in (Q8.FORMS["none"], Q8.FORMS["residual"], Q8.FORMS["gelu"]):
        full = K.gemm_nt_stream_q8(d["x"], d["Q"], d["scale"], **_kw(d, form))
        assert torch.equal(full, K.gemm_nt_stream_q8(d["x"], d["Q"], d["scale"], **_kw(d, form))), "two runs differ"
        for M in (17, 16, 5):
            part = K.gemm_nt_stream_q8(d["x"][:M], d["Q"], d["scale"], **_kw(d, form, slice(0, M)))
            assert torch.equal(part, full[:M]), M
        for m in (0, 15, 16, 31):
            one = K.gemm_nt_stream_q8(d["x"][m:m + 1], d["Q"], d["scale"], **_kw(d, form, slice(m, m + 1)))
            assert torch.equal(one[0], full[m]), m


@pytest.mark.parametrize("shape", [(17, 384, 1536), (5, 32768, 320)], ids=IDS)
def test_guards_around_c_and_the_workspace(shape):
    """Rows >= M of C, the columns beyond N (ldc > N) and the workspace beyond [split][M][N] keep their fill."""
    case = _case(shape)
    d = _dev(case)
    M, N, _ = shape
    cbuf = torch.full((M + 15, N + 128), 7.0, dtype=BF16, device=DEV)
    out = cbuf[:M, :N]
    args, _ = K.gemm_nt_stream_q8(d["x"], d["Q"], d["scale"], bias=d["bias"], residual=d["res"], out=out, _args_only=True)
    lib = L.load()
    need = lib.wft_gemm_nt_stream_q8_workspace_bytes(C.byref(args))
    assert need > 0 and need == lib.wft_gemm_nt_stream_workspace_bytes(C.byref(args)) and need % (M * N * 4) == 0
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    args.workspace, args.workspace_bytes = ws.data_ptr(), need
    L.check(lib.wft_gemm_nt_stream_q8(C.byref(args), d["scale"].data_ptr(), L.stream_ptr()), "wft_gemm_nt_stream_q8")
    torch.cuda.synchronize()
    assert torch.equal(out, K.gemm_nt_stream_q8(d["x"], d["Q"], d["scale"], bias=d["bias"], residual=d["res"]))
    assert (cbuf[:M, N:] == 7.0).all() and (cbuf[M:] == 7.0).all(), "columns / rows beyond C were written"
    assert (ws[need:] == 0x5A).all(), "bytes behind the workspace were written"
    args.workspace_bytes = need - 1
    assert lib.wft_gemm_nt_stream_q8(C.byref(args), d["scale"].data_ptr(), L.stream_ptr()) == -1 and "workspace" in L.last_error()


def test_refusals_name_their_reason():
    lib = L.load()
    N, Kd = 256, 384
    d = _dev(_case((16, N, Kd)))
    x33 = torch.zeros(33, Kd, dtype=BF16, device=DEV)
    qpad = torch.zeros(N, Kd + 8, dtype=torch.int8, device=DEV)
    qoff = torch.zeros(N * Kd + 16, dtype=torch.int8, device=DEV)[8:8 + N * Kd].view(N, Kd)
    calls = {
        "M = 33": (dict(a=x33, q=d["Q"]), "M must lie"),
        "K = 96": (dict(a=d["x"], q=d["Q"], K=96), "K must be a multiple of 64"),
        "ldb = K + 8": (dict(a=d["x"], q=qpad[:, :Kd]), "ldb must be a multiple of 16"),
        "misaligned B": (dict(a=d["x"], q=qoff), "16-byte aligned"),
        "unsupported epilogue": (dict(a=d["x"], q=d["Q"], epilogue=L.EPI_GELU_GRAD, aux=torch.zeros(16, N, dtype=BF16, device=DEV)), "epilogue"),
    }
    for name, (kw, reason) in calls.items():
        a, q = kw.pop("a"), kw.pop("q")
        assert K.gemm_nt_stream_q8(a, q, d["scale"], **kw) is None, name  # the wrapper: nothing launched, the caller falls back
        args = L.GemmArgs()
        args.A, args.lda, args.B, args.ldb = a.data_ptr(), a.stride(0), q.data_ptr(), q.stride(0)
        out = torch.zeros(a.shape[0], N, dtype=BF16, device=DEV)
        args.C, args.ldc = out.data_ptr(), N
        args.M, args.N, args.K, args.batch, args.alpha, args.beta = a.shape[0], N, kw.get("K", Kd), 1, 1.0, 1.0
        args.epilogue = kw.get("epilogue", L.EPI_NONE)
        if "aux" in kw:
            args.aux, args.ldaux = kw["aux"].data_ptr(), N
        assert lib.wft_gemm_nt_stream_q8_ok(C.byref(args)) == 0 and lib.wft_gemm_nt_stream_q8_workspace_bytes(C.byref(args)) == 0, name
        assert lib.wft_gemm_nt_stream_q8(C.byref(args), d["scale"].data_ptr(), L.stream_ptr()) == -3, name  # WFT_ERR_UNSUPPORTED
        msg = L.last_error()
        assert "wft_gemm_nt_stream_q8" in msg and "not served" in msg and reason in msg, (name, msg)
        assert not out.any(), name
    # a served call without scales is an argument error
    args, _ = K.gemm_nt_stream_q8(d["x"], d["Q"], d["scale"], _args_only=True)
    assert lib.wft_gemm_nt_stream_q8(C.byref(args), None, L.stream_ptr()) == -1 and "b_scale" in L.last_error()


@pytest.mark.parametrize("shape", [(16, 256, 384), (17, 384, 1536), (32, 51968, 384)], ids=IDS)
def test_the_bf16_entry_point_keeps_its_relation_to_gemm_nt(shape):
    """The reduce kernel gained a scale pointer; with NULL the bf16 entry point must compute what it computed: held against
    wft_gemm_nt_bf16 on the same operands by the bound tests/test_gemm_stream_gpu.py holds both to (1e-2 of the largest magnitude)."""
    d = _dev(_case(shape))
    wb = (d["Q"].float() * 2.0 ** -6).to(BF16)
    for name, form in Q8.FORMS.items():
        kw = _kw(d, form)
        close(K.gemm_nt_stream(d["x"], wb, **kw), K.gemm_nt(d["x"], wb, **kw).float(), 1e-2, f"{shape} {name}")
