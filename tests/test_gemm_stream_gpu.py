"""The weight-streaming small-M GEMM (csrc/gemm_stream.hip, K.gemm_nt_stream) on the projection shapes of a cached decoding step of
whisper-tiny and whisper-large-v3, M in {1, 2, 5, 8, 16, 17, 32}.

Reference: the fp32 product of the bf16 inputs (GELU: torch.nn.functional.gelu), bound = the project's own for a bf16 C
(`close(got, ref, 1e-2)` of tests/test_kernels_gpu.py: max error <= 1e-2 of the largest reference magnitude).  The largest difference to
wft_gemm_nt_bf16 on the same arguments is printed, not bounded.  Bit-level properties: two calls agree, row m at M = 32 equals the
M = 1 product of that row alone, nothing outside C's columns and the workspace is written."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_kernels_gpu import DEV, bf, close  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

TINY = [(1152, 384), (384, 384), (1536, 384), (384, 1536), (51968, 384)]
LARGE_V3 = [(3840, 1280), (1280, 1280), (5120, 1280), (1280, 5120), (51968, 1280)]
MS = [1, 2, 5, 8, 16, 17, 32]
_W = {}


def _weights(N, Kd):
    """One weight matrix per shape for the whole module (the vocabulary-sized ones are 133 MB)."""
    if (N, Kd) not in _W:
        g = torch.Generator(device=DEV).manual_seed(N * 7 + Kd)
        _W[(N, Kd)] = bf(torch.randn(N, Kd, device=DEV, generator=g) * 0.05)
    return _W[(N, Kd)]


def _operands(M, N, Kd, lda=None, seed=0):
    g = torch.Generator(device=DEV).manual_seed(1000 * M + seed)
    lda = Kd if lda is None else lda
    xbuf = bf(torch.randn(M, lda, device=DEV, generator=g))
    x = xbuf[:, :Kd]
    bias = torch.randn(N, device=DEV, generator=g) * 0.5
    res = bf(torch.randn(M, N, device=DEV, generator=g))
    return x, bias, res


def _ref(x, w, bias=None, res=None, gelu=False):
    y = x.float() @ w.float().t()
    if bias is not None:
        y = y + bias
    pre = y
    if gelu:
        y = torch.nn.functional.gelu(y)
    if res is not None:
        y = y + res.float()
    return y, pre


@pytest.mark.parametrize("N,Kd", TINY + LARGE_V3)
def test_all_forms_against_the_fp32_product(N, Kd):
    w = _weights(N, Kd)
    worst_old = 0.0
    for M in MS:
        x, bias, res = _operands(M, N, Kd)
        forms = {
            "plain": (dict(), dict()),
            "bias": (dict(bias=bias), dict(bias=bias)),
            "bias+residual": (dict(bias=bias, residual=res), dict(bias=bias, res=res)),
            "gelu": (dict(bias=bias, epilogue=L.EPI_GELU), dict(bias=bias, gelu=True)),
        }
        for name, (kw, rkw) in forms.items():
            got = K.gemm_nt_stream(x, w, **kw)
            assert got is not None and got.shape == (M, N) and got.dtype == torch.bfloat16, (name, M)
            ref, _ = _ref(x, w, **rkw)
            close(got, ref, 1e-2, f"{name} M={M} N={N} K={Kd}")
            old = K.gemm_nt(x, w, **kw)
            worst_old = max(worst_old, (got.float() - old.float()).abs().max().item())
        # GELU with the pre-activation stored
        aux = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        got = K.gemm_nt_stream(x, w, bias=bias, epilogue=L.EPI_GELU, aux=aux)
        ref, pre = _ref(x, w, bias=bias, gelu=True)
        close(got, ref, 1e-2, f"gelu+aux M={M}")
        close(aux, pre, 1e-2, f"aux M={M}")
        assert torch.equal(got, K.gemm_nt_stream(x, w, bias=bias, epilogue=L.EPI_GELU)), "storing aux changes C"
    print(f"N={N} K={Kd}: largest |stream - wft_gemm_nt_bf16| over all forms and M: {worst_old:.3e}")


def test_row_stride_larger_than_k():
    N, Kd, M = 1280, 1280, 8
    w = _weights(N, Kd)
    x, bias, res = _operands(M, N, Kd, lda=Kd + 64)
    assert x.stride(0) == Kd + 64
    got = K.gemm_nt_stream(x, w, bias=bias, residual=res)
    close(got, _ref(x, w, bias=bias, res=res)[0], 1e-2, "lda > K")
    assert torch.equal(got, K.gemm_nt_stream(x.contiguous(), w, bias=bias, residual=res))


@pytest.mark.parametrize("N,Kd", [(384, 1536), (1152, 384), (1280, 5120), (5120, 1280), (51968, 1280)])
def test_repeatable_and_row_invariant(N, Kd):
    """Row m of C at M = 32 (and at 17, 16, 5) is bit-equal to the M = 1 product of that row alone: a transcript does not depend on
    the evaluation batch it sat in."""
    w = _weights(N, Kd)
    x, bias, res = _operands(32, N, Kd)
    for kw_of in (lambda s: dict(), lambda s: dict(bias=bias, residual=res[s]), lambda s: dict(bias=bias, epilogue=L.EPI_GELU)):
        full = K.gemm_nt_stream(x, w, **kw_of(slice(0, 32)))
        assert torch.equal(full, K.gemm_nt_stream(x, w, **kw_of(slice(0, 32)))), "two calls differ"
        for M in (17, 16, 5):
            part = K.gemm_nt_stream(x[:M], w, **kw_of(slice(0, M)))
            assert torch.equal(part, full[:M]), (N, Kd, M)
        for m in (0, 3, 15, 16, 31):
            one = K.gemm_nt_stream(x[m:m + 1], w, **kw_of(slice(m, m + 1)))
            assert torch.equal(one[0], full[m]), (N, Kd, m)


def test_canaries_around_c_and_the_workspace():
    """C with ldc > N: the columns beyond N keep their value; the workspace is written in its first workspace_bytes only."""
    N, Kd, M = 1280, 1280, 17
    w = _weights(N, Kd)
    x, bias, res = _operands(M, N, Kd)
    cbuf = torch.full((M + 1, N + 128), 7.0, dtype=torch.bfloat16, device=DEV)
    out = cbuf[:M, :N]
    args, _ = K.gemm_nt_stream(x, w, bias=bias, residual=res, out=out, _args_only=True)
    need = L.load().wft_gemm_nt_stream_workspace_bytes(C.byref(args))
    assert 0 < need and args.ldc == N + 128
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    args.workspace, args.workspace_bytes = ws.data_ptr(), need
    L.check(L.load().wft_gemm_nt_stream_bf16(C.byref(args), L.stream_ptr()), "wft_gemm_nt_stream_bf16")
    torch.cuda.synchronize()
    close(out, _ref(x, w, bias=bias, res=res)[0], 1e-2, "ldc > N")
    assert (cbuf[:M, N:] == 7.0).all() and (cbuf[M] == 7.0).all(), "columns / rows beyond C were written"
    assert (ws[need:] == 0x5A).all(), "bytes behind the workspace were written"
    assert not (ws[:need] == 0x5A).all()
    # a workspace one byte short is an argument error, not a launch
    args.workspace_bytes = need - 1
    assert L.load().wft_gemm_nt_stream_bf16(C.byref(args), L.stream_ptr()) != 0
    assert "workspace" in L.last_error()


def test_unserved_calls_return_none_and_launch_nothing():
    w = _weights(1280, 1280)
    x = bf(torch.randn(33, 1280, device=DEV))
    assert K.gemm_nt_stream(x, w) is None
    assert K.gemm_nt_stream(x[:8], w, epilogue=L.EPI_GELU_GRAD, aux=torch.empty(8, 1280, dtype=torch.bfloat16, device=DEV)) is None
