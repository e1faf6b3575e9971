"""Host side of the weight-streaming small-M GEMM (csrc/gemm_stream.hip): which calls wft_gemm_nt_stream_ok serves, what the
workspace query answers, and that a refused call returns an error with a message before any device call — all without a GPU."""
import ctypes

import pytest

from whisper_finetune.engine import lib as L

# (N, K) of every projection of a cached decoding step: fused q/k/v, attention out / cross q, mlp.0, mlp.2, padded vocabulary
TINY = [(1152, 384), (384, 384), (1536, 384), (384, 1536), (51968, 384)]
LARGE_V3 = [(3840, 1280), (1280, 1280), (5120, 1280), (1280, 5120), (51968, 1280)]


def _args(M, N, K, **kw):
    a = L.GemmArgs()
    a.A = a.B = a.C = 1 << 20
    a.M, a.N, a.K, a.batch, a.alpha, a.beta = M, N, K, 1, 1.0, 1.0
    a.lda, a.ldb, a.ldc = K, K, N
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("M", [1, 8, 32])
def test_decode_step_shapes_are_served(M):
    h = L.load()
    for N, K in TINY + LARGE_V3:
        for kw in ({}, {"bias": 1 << 21}, {"bias": 1 << 21, "residual": 1 << 22, "ldr": N}, {"bias": 1 << 21, "epilogue": L.EPI_GELU},
                   {"bias": 1 << 21, "epilogue": L.EPI_GELU, "aux": 1 << 23, "ldaux": N}):
            a = _args(M, N, K, **kw)
            assert h.wft_gemm_nt_stream_ok(ctypes.byref(a)) == 1, (M, N, K, kw)
            ws = h.wft_gemm_nt_stream_workspace_bytes(ctypes.byref(a))
            # fp32 partials [split][M][N] with 1 <= split <= K / 64
            assert ws > 0 and ws % (M * N * 4) == 0 and 1 <= ws // (M * N * 4) <= K // 64, (M, N, K, ws)


def test_the_split_does_not_depend_on_m():
    """Row m of C must not depend on the batch it sat in: the number of K slices is a function of (N, K) and the chip only."""
    h = L.load()
    for N, K in TINY + LARGE_V3:
        splits = {h.wft_gemm_nt_stream_workspace_bytes(ctypes.byref(_args(M, N, K))) // (M * N * 4) for M in (1, 2, 5, 8, 16, 17, 32)}
        assert len(splits) == 1, (N, K, splits)
    # 256 CUs is what the library assumes without a device: a deep K over few column blocks is cut into many slices
    assert h.wft_gemm_nt_stream_workspace_bytes(ctypes.byref(_args(1, 1280, 5120))) // (1280 * 4) > 8


REFUSED = {
    "M above the limit": dict(M=33),
    "f32 C": dict(c_is_f32=1),
    "batch 2": dict(batch=2),
    "accumulate": dict(accumulate=1, c_is_f32=1),
    "colsum": dict(colsum=1 << 24),
    "p_valid": dict(p_valid=8),
    "valid_rows_period": dict(valid_rows_period=4, valid_rows=3),
    "DGELU": dict(epilogue=L.EPI_DGELU, aux=1 << 23, ldaux=1280),
    "MUL_AUX": dict(epilogue=L.EPI_MUL_AUX, aux=1 << 23, ldaux=1280),
    "GELU_GRAD": dict(epilogue=L.EPI_GELU_GRAD, aux=1 << 23, ldaux=1280),
    "K % 64 != 0": dict(K=1280 + 32, lda=1312, ldb=1312),
    "N % 128 != 0": dict(N=1280 + 64, ldc=1344),
    "alpha": dict(alpha=0.5),
    "residual before the epilogue": dict(residual=1 << 22, ldr=1280, residual_first=1),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_everything_else_is_refused_without_a_device(what):
    h = L.load()
    a = _args(**{**dict(M=8, N=1280, K=1280), **REFUSED[what]})
    ws = (ctypes.c_char * 64)()
    a.workspace, a.workspace_bytes = ctypes.addressof(ws), 1 << 40  # (never touched: the refusal comes first)
    assert h.wft_gemm_nt_stream_ok(ctypes.byref(a)) == 0
    assert h.wft_gemm_nt_stream_workspace_bytes(ctypes.byref(a)) == 0
    rc = h.wft_gemm_nt_stream_bf16(ctypes.byref(a), None)
    assert rc != 0
    msg = L.last_error()
    assert "wft_gemm_nt_stream_bf16" in msg and "not served" in msg, msg


def test_null_arguments_are_refused():
    h = L.load()
    assert h.wft_gemm_nt_stream_ok(None) == 0 and h.wft_gemm_nt_stream_workspace_bytes(None) == 0
    a = _args(8, 1280, 1280)
    a.B = 0
    assert h.wft_gemm_nt_stream_ok(ctypes.byref(a)) == 0 and h.wft_gemm_nt_stream_bf16(ctypes.byref(a), None) != 0


def test_the_old_dispatch_is_untouched():
    """wft_gemm_nt_variant answers what it answered on the argument sets of tests/test_abi.py, and 128 on every step shape."""
    h = L.load()
    a = _args(130500, 5120, 1280)
    assert h.wft_gemm_nt_variant(ctypes.byref(a)) == 4
    a.variant = 1
    assert h.wft_gemm_nt_variant(ctypes.byref(a)) == 256
    for N, K in TINY + LARGE_V3:
        assert h.wft_gemm_nt_variant(ctypes.byref(_args(8, N, K))) == 128
