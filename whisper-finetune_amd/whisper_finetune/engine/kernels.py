"""Tensor-level wrappers over the C ABI (no autograd here; see ops.py).

Every function takes torch CUDA tensors, checks dtype/contiguity, and enqueues the HIP
kernel on the current stream.  Shapes follow include/wft.h.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import lib as L

BF16 = torch.bfloat16
F32 = torch.float32

# bench.py sets this to a list to time every gemm_nt launch with HIP events recorded on the
# launch stream: entries are (start_event, end_event, algorithmic_flops, kernel variant 128|256, algorithmic_bytes).
PROFILE_NT = None


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _chk(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise L.WftError(f"{name}: libwft kernels need CUDA/HIP tensors (got {t.device}); there is no CPU path")


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# --------------------------------------------------------------------------- casts
def cast_bf16(src: torch.Tensor) -> torch.Tensor:
    _chk(src, F32, "src")
    src = src.contiguous()
    dst = torch.empty(src.shape, dtype=BF16, device=src.device)
    L.check(L.load().wft_cast_f32_bf16(_p(src), _p(dst), src.numel(), L.stream_ptr()), "wft_cast_f32_bf16")
    return dst


def cast_f32(src: torch.Tensor) -> torch.Tensor:
    _chk(src, BF16, "src")
    src = src.contiguous()
    dst = torch.empty(src.shape, dtype=F32, device=src.device)
    L.check(L.load().wft_cast_bf16_f32(_p(src), _p(dst), src.numel(), L.stream_ptr()), "wft_cast_bf16_f32")
    return dst


def weight_shadow(w: torch.Tensor, rows_pad: int, cols_pad: int, want_t: bool, out=None, out_t=None, fwd_scale: float = 1.0):
    """f32 [rows, cols] -> bf16 [rows_pad, cols_pad] (+ transposed [cols_pad, rows_pad]).  fwd_scale: the straight image is
    bf16(fwd_scale * w) (one rounding), the transposed one stays bf16(w) (wft.h; ops.QK_PRESCALE)."""
    _chk(w, F32, "w")
    w2 = w.reshape(w.shape[0], -1).contiguous()
    rows, cols = w2.shape
    dst = out if out is not None else torch.empty((rows_pad, cols_pad), dtype=BF16, device=w.device)
    dst_t = None
    if want_t:
        dst_t = out_t if out_t is not None else torch.empty((cols_pad, rows_pad), dtype=BF16, device=w.device)
    assert dst.stride(1) == 1 and (dst_t is None or dst_t.stride(1) == 1)
    L.check(
        L.load().wft_cast_pad_transpose_f32_bf16(_p(w2), rows, cols, _p(dst), _p(dst_t), rows_pad, cols_pad,
                                                 dst.stride(0), 0 if dst_t is None else dst_t.stride(0), float(fwd_scale), L.stream_ptr()),
        "wft_cast_pad_transpose_f32_bf16",
    )
    return dst, dst_t


def lora_merge(w, B, A, mask, scaling: float, rows_pad=None, cols_pad=None, out=None, out_t=None, out_f32=None, fwd_scale: float = 1.0):
    """W + scaling * B @ (A * mask) -> bf16 shadow `out` [rows_pad, cols_pad] (+ `out_t`) and/or f32 `out_f32` [rows, cols]."""
    for n, t in (("w", w), ("B", B), ("A", A)):
        _chk(t, F32, n)
    w2 = w.reshape(w.shape[0], -1).contiguous()
    rows, cols = w2.shape
    B, A = B.contiguous(), A.contiguous()
    r = A.shape[0]
    assert B.shape == (rows, r) and A.shape == (r, cols)
    if mask is not None:
        _chk(mask, F32, "mask")
        mask = mask.reshape(-1).contiguous()
        assert mask.numel() == cols
    if out is not None:
        rows_pad = out.shape[0] if rows_pad is None else rows_pad
        cols_pad = out.shape[1] if cols_pad is None else cols_pad
        assert out.stride(1) == 1 and (out_t is None or out_t.stride(1) == 1)
    L.check(
        L.load().wft_lora_merge(_p(w2), rows, cols, _p(B), _p(A), _p(mask), r, float(scaling), _p(out), _p(out_t),
                                rows_pad or rows, cols_pad or cols, 0 if out is None else out.stride(0),
                                0 if out_t is None else out_t.stride(0), _p(out_f32), float(fwd_scale), L.stream_ptr()),
        "wft_lora_merge",
    )
    return out, out_t, out_f32


def lora_refresh_mt(table: torch.Tensor, tile_start: torch.Tensor, n: int, total_tiles: int) -> None:
    """wft_lora_refresh_mt: lora_merge (bf16 shadow + transposed shadow) and lora_pack of every adapter in the device table
    (int64 [n, 20], see wft.h) in one launch."""
    L.check(L.load().wft_lora_refresh_mt(_p(table), _p(tile_start), int(n), int(total_tiles), L.stream_ptr()), "wft_lora_refresh_mt")


def mt_copy_f32(table: torch.Tensor) -> None:
    """wft_mt_copy_f32: every (source, destination, count) row of the device table int64 [n, 3] in one launch."""
    L.check(L.load().wft_mt_copy_f32(_p(table), int(table.shape[0]), L.stream_ptr()), "wft_mt_copy_f32")


def lora_pack(A, mask, B, scaling: float, Am, AmT, Bb, BbT, ro: int, no: int) -> None:
    """One adapter's blocks of the rank-r gradient-GEMM operands (see wft_lora_pack): A f32 [r, K], mask f32 [1, K] or None,
    B f32 [n, r] -> Am [Rpad, K] / AmT, Bb [Npad, Rpad] / BbT (bf16, zero-initialised by the caller)."""
    _chk(A, F32, "A"); _chk(B, F32, "B")
    for t, nme in ((Am, "Am"), (AmT, "AmT"), (Bb, "Bb"), (BbT, "BbT")):
        _chk(t, BF16, nme)
    r, Kd = A.shape
    n = B.shape[0]
    assert A.is_contiguous() and B.is_contiguous() and B.shape[1] == r and Am.shape[1] == Kd
    rpad, npad = Am.shape[0], Bb.shape[0]
    m = None if mask is None else mask.contiguous()
    L.check(L.load().wft_lora_pack(_p(A), _p(m), _p(B), r, Kd, n, float(scaling), _p(Am), _p(AmT), _p(Bb), _p(BbT), rpad, npad, ro, no,
                                   L.stream_ptr()), "wft_lora_pack")


def add_bf16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _chk(a, BF16, "a"); _chk(b, BF16, "b")
    a = a.contiguous(); b = b.contiguous()
    y = torch.empty_like(a)
    L.check(L.load().wft_add_bf16(_p(a), _p(b), _p(y), a.numel(), L.stream_ptr()), "wft_add_bf16")
    return y


def axpby_bf16(a: float, x: torch.Tensor, b: float = 0.0, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a*x + b*y (bf16, same shape; y optional)."""
    _chk(x, BF16, "x")
    x = x.contiguous()
    if y is not None:
        _chk(y, BF16, "y")
        y = y.contiguous()
    out = torch.empty_like(x)
    L.check(L.load().wft_axpby_bf16(float(a), _p(x), float(b), _p(y), _p(out), x.numel(), L.stream_ptr()), "wft_axpby_bf16")
    return out


def _chk_flag(t: torch.Tensor, n: int, name: str):
    """A device int32 parameter block (a stochastic-depth skip flag, a SpecAugment span): contiguous, n elements."""
    _chk(t, torch.int32, name)
    if t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous int32 tensor of {n} elements, got shape {tuple(t.shape)}")


def sd_select_fwd(skip: torch.Tensor, keep: float, x: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    """Stochastic depth with a device skip flag: *skip ? x : (1-s)*x + s*f, s = 1/keep (bf16; kept: the bits of axpby_bf16)."""
    _chk_flag(skip, 1, "skip"); _chk(x, BF16, "x"); _chk(f, BF16, "f")
    x = x.contiguous(); f = f.contiguous()
    if f.shape != x.shape:
        raise ValueError(f"sd_select_fwd: x {tuple(x.shape)} and f {tuple(f.shape)} differ")
    s = 1.0 / keep
    out = torch.empty_like(x)
    L.check(L.load().wft_sd_select_fwd_bf16(_p(skip), float(1.0 - s), _p(x), float(s), _p(f), _p(out), x.numel(), L.stream_ptr()),
            "wft_sd_select_fwd_bf16")
    return out


def sd_select_bwd(skip: torch.Tensor, keep: float, dy: torch.Tensor):
    """-> (dx, df): *skip ? (dy, 0) : ((1-s)*dy, s*dy), s = 1/keep, in one pass over dy."""
    _chk_flag(skip, 1, "skip"); _chk(dy, BF16, "dy")
    dy = dy.contiguous()
    s = 1.0 / keep
    dx = torch.empty_like(dy)
    df = torch.empty_like(dy)
    L.check(L.load().wft_sd_select_bwd_bf16(_p(skip), float(1.0 - s), float(s), _p(dy), _p(dx), _p(df), dy.numel(), L.stream_ptr()),
            "wft_sd_select_bwd_bf16")
    return dx, df


def dgelu_mul(dy: torch.Tensor, pre: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(dy, BF16, "dy"); _chk(pre, BF16, "pre")
    assert dy.is_contiguous() and pre.is_contiguous()
    out = torch.empty_like(dy) if out is None else out
    L.check(L.load().wft_dgelu_mul_bf16(_p(dy), _p(pre), _p(out), dy.numel(), L.stream_ptr()), "wft_dgelu_mul_bf16")
    return out


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """x bf16 [rows, cols] (row stride may exceed cols) -> f32 [cols]."""
    _chk(x, BF16, "x")
    assert x.dim() == 2 and x.stride(1) == 1
    rows, cols = x.shape
    if out is None:
        out = torch.empty(cols, dtype=F32, device=x.device)
        accumulate = False
    lib = L.load()
    need = lib.wft_colsum_workspace_bytes(rows, cols)
    if need > 0:  # large inputs: chunked over the whole chip, folded in a fixed order
        ws = _tn_workspace(x.device, need, slot="colsum")
        L.check(lib.wft_colsum_bf16_ws(_p(x), rows, cols, x.stride(0), _p(out), int(accumulate), ws.data_ptr(), ws.numel(), L.stream_ptr()),
                "wft_colsum_bf16_ws")
    else:
        L.check(lib.wft_colsum_bf16(_p(x), rows, cols, x.stride(0), _p(out), int(accumulate), L.stream_ptr()), "wft_colsum_bf16")
    return out


# --------------------------------------------------------------------------- layernorm
def layernorm_fwd(x, gamma, beta, eps=1e-5, mask=None):
    """x bf16 [..., cols]; mask = (rows_per_batch, t0, t1, c0, c1), (rows_per_batch, span: device int32[4] {t0, t1, c0, c1}) or None."""
    _chk(x, BF16, "x"); _chk(gamma, F32, "gamma"); _chk(beta, F32, "beta")
    x = x.contiguous()
    cols = x.shape[-1]
    rows = x.numel() // cols
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=F32, device=x.device)
    rstd = torch.empty(rows, dtype=F32, device=x.device)
    if mask is not None and len(mask) == 2:
        rpb, span = mask
        _chk_flag(span, 4, "span")
        L.check(L.load().wft_layernorm_fwd_dspan(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, cols, eps, int(rpb),
                                                 _p(span), L.stream_ptr()), "wft_layernorm_fwd_dspan")
        return y, mean, rstd
    rpb, t0, t1, c0, c1 = mask if mask is not None else (0, 0, 0, 0, 0)
    L.check(
        L.load().wft_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, cols, eps,
                                   rpb, t0, t1, c0, c1, L.stream_ptr()),
        "wft_layernorm_fwd",
    )
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dres=None, mask=None, want_colsum=False, want_params=True):
    """returns dx bf16, dgamma f32, dbeta f32 (fresh tensors, each its own allocation so that autograd can keep them as
    the .grad without a copy; None, None with want_params=False: frozen LayerNorm parameters) [, colsum(dx) f32 if want_colsum]."""
    _chk(dy, BF16, "dy"); _chk(x, BF16, "x")
    dy = dy.contiguous(); x = x.contiguous()
    if dres is not None:
        _chk(dres, BF16, "dres")
        dres = dres.contiguous()
    cols = x.shape[-1]
    rows = x.numel() // cols
    lib = L.load()
    need_ws = want_params or want_colsum
    ws = torch.empty(lib.wft_layernorm_bwd_workspace(rows, cols), dtype=torch.uint8, device=x.device) if need_ws else None
    dx = torch.empty_like(x)
    dgamma = torch.empty(cols, dtype=F32, device=x.device) if want_params else None
    dbeta = torch.empty(cols, dtype=F32, device=x.device) if want_params else None
    dxs = torch.empty(cols, dtype=F32, device=x.device) if want_colsum else None
    if mask is not None and len(mask) == 2:
        rpb, span = mask
        _chk_flag(span, 4, "span")
        L.check(lib.wft_layernorm_bwd_dspan(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx), _p(dgamma), _p(dbeta),
                                            _p(dxs), _p(ws), rows, cols, int(rpb), _p(span), L.stream_ptr()), "wft_layernorm_bwd_dspan")
    else:
        rpb, t0, t1, c0, c1 = mask if mask is not None else (0, 0, 0, 0, 0)
        L.check(
                lib.wft_layernorm_bwd(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx), _p(dgamma), _p(dbeta),
                                      _p(dxs), _p(ws), rows, cols, rpb, t0, t1, c0, c1, L.stream_ptr()),
            "wft_layernorm_bwd",
        )
    if want_colsum:
        return dx, dgamma, dbeta, dxs
    return dx, dgamma, dbeta


# --------------------------------------------------------------------------- GEMM
# Per-call launch state (wft.h: wft_gemm_args / wft_attn_args `launch_mode`, `variant`, `q_prescaled`).  libwft keeps NO mutable state;
# these Python-side hooks only choose what the wrappers below write into the argument structs.
#   VARIANT: test / A-B hook — force the 8-wave kernels ("nt", "tn": gemm_nt256 / gemm_tn256; "fwd", "dq", "dkdv": the 8-wave
#     attention kernels) where the one-wave-per-SIMD kernels would apply; `set_variant` returns the previous value.
#   LAUNCH_OVERRIDE[0]: bench tooling (bench.py ddp_mode_1gpu) — None: the caller's `launch` argument decides; 0 / 1: every call.
VARIANT = {"nt": 0, "tn": 0, "fwd": 0, "dq": 0, "dkdv": 0}
LAUNCH_OVERRIDE = [None]
LAUNCH_PERSISTENT, LAUNCH_PER_TILE = 0, 1


def set_variant(which: str, v: int) -> int:
    old = VARIANT[which]
    if v >= 0:
        VARIANT[which] = 1 if v else 0
    return old


def _launch(launch: int) -> int:
    o = LAUNCH_OVERRIDE[0]
    return int(launch) if o is None else int(o)


def _attn_variant_bits() -> int:
    return VARIANT["fwd"] | (VARIANT["dq"] << 1) | (VARIANT["dkdv"] << 2)


def gemm_nt(a, b, *, M=None, N=None, K=None, lda=None, ldb=None, out=None, out_f32=False, accumulate=False,
            bias=None, residual=None, aux=None, epilogue=L.EPI_NONE, alpha=1.0, batch=1,
            strideA=0, strideB=0, strideC=0, strideR=0, strideAux=0, ldc=None,
            valid_rows_period=0, valid_rows=0, residual_first=False, ldaux=None, ldr=None, beta=1.0, colsum=None, p_valid=0,
            launch=0, _args_only=False):
    """C[M,N] = alpha * A[M,K] @ B[N,K]^T (+bias) (epilogue) (+residual).

    a: bf16, row m at a.data_ptr() + m*lda; b: bf16 [N, K] (ldb).  Defaults take the shapes
    from 2-D contiguous tensors.  `aux`: GELU pre-activation out (EPI_GELU) / in (EPI_DGELU); gelu' out (EPI_GELU_GRAD) / in (EPI_MUL_AUX).
    p_valid (N = 128, plain bf16 product): rows >= p_valid of b are zero padding (a rank-r LoRA operand) — the load-stream
    kernel for rank-r operands, which writes ONLY columns < 16*ceil(p_valid/16) of the output (the rest stays uninitialised:
    the consumer is gemm_tn with the same p_valid).
    """
    _chk(a, BF16, "A"); _chk(b, BF16, "B")
    if M is None:
        M = a.shape[0]
    if K is None:
        K = a.shape[-1]
    if N is None:
        N = b.shape[0]
    if lda is None:
        lda = a.stride(-2) if a.dim() >= 2 else K
    if ldb is None:
        ldb = b.stride(-2)
    if out is None:
        out = torch.empty((batch * M, N) if batch > 1 else (M, N), dtype=F32 if out_f32 else BF16, device=a.device)
        if batch > 1 and strideC == 0:
            strideC = M * N
    if ldc is None:
        ldc = out.stride(-2)
    out_f32 = out.dtype == F32
    args = L.GemmArgs()
    args.A, args.lda, args.strideA = a.data_ptr(), lda, strideA
    args.B, args.ldb, args.strideB = b.data_ptr(), ldb, strideB
    args.C, args.ldc, args.strideC = out.data_ptr(), ldc, strideC
    args.c_is_f32, args.accumulate = int(out_f32), int(accumulate)
    args.bias = 0 if bias is None else bias.data_ptr()
    if residual is not None:
        _chk(residual, BF16, "residual")
        args.residual, args.ldr, args.strideR = residual.data_ptr(), (residual.stride(-2) if ldr is None else ldr), strideR
    if aux is not None and epilogue in (L.EPI_GELU_GRAD8, L.EPI_MUL_AUX8):
        # one-byte gelu' in gemm_nt4w_kernel's fragment order (wft.h): an opaque uint8 buffer of aux8_bytes(...) bytes
        _chk(aux, torch.uint8, "aux")
        args.aux, args.ldaux, args.strideAux = aux.data_ptr(), 0, 0
    elif aux is not None:
        _chk(aux, BF16, "aux")
        args.aux, args.ldaux, args.strideAux = aux.data_ptr(), (aux.stride(-2) if ldaux is None else ldaux), strideAux
    args.epilogue, args.alpha, args.beta = epilogue, alpha, beta
    args.M, args.N, args.K, args.batch = M, N, K, batch
    args.valid_rows_period, args.valid_rows = valid_rows_period, valid_rows
    args.residual_first = int(residual_first)
    args.p_valid = int(p_valid)
    args.launch_mode, args.variant = _launch(launch), VARIANT["nt"]
    if colsum is not None:  # f32 [N]: column sums of C (bias gradient of C's consumer), fused into the epilogue when possible
        _chk(colsum, F32, "colsum")
        args.colsum = colsum.data_ptr()
        _grant_workspace(args, "wft_gemm_nt_colsum_workspace_bytes", a.device, "nt_colsum")
    elif not out_f32 and batch == 1 and epilogue == L.EPI_NONE and K >= 4096 and N * M <= (1 << 21):
        # few output tiles over a deep K (the tied-embedding backward-data product of a short decoder batch): split-K partials
        _grant_workspace(args, "wft_gemm_nt_splitk_workspace_bytes", a.device, "nt_splitk")
    if _args_only:  # (paired launches: gemm_nt_rank_pair)
        return args, out
    if epilogue in (L.EPI_GELU_GRAD8, L.EPI_MUL_AUX8):
        need = L.load().wft_gemm_nt_aux8_bytes(C.byref(args))
        if need <= 0 or aux is None or aux.numel() < need:
            raise L.WftError(f"one-byte gelu' epilogue: the call is not served in that form or the buffer is too small (need {need} bytes)")
    if PROFILE_NT is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        L.check(L.load().wft_gemm_nt_bf16(C.byref(args), L.stream_ptr()), "wft_gemm_nt_bf16")
        ev1.record()
        nbytes = 2.0 * batch * (M * K + N * K + M * N * (2 if out_f32 else 1) + (M * N if residual is not None else 0) + (M * N if aux is not None else 0))
        PROFILE_NT.append((ev0, ev1, 2.0 * M * N * K * batch, L.load().wft_gemm_nt_variant(C.byref(args)), nbytes))
        return out
    L.check(L.load().wft_gemm_nt_bf16(C.byref(args), L.stream_ptr()), "wft_gemm_nt_bf16")
    return out


def _stream_args(a, b, b_dtype, query, M, N, K, lda, ldb, out, bias, residual, aux, epilogue, ldc, ldaux, ldr):
    """The wft_gemm_args of both streaming entry points -> (args, out), or None when `query` (the workspace query of the entry point)
    says the library does not serve the call."""
    _chk(a, BF16, "A"); _chk(b, b_dtype, "B")
    if M is None:
        M = a.shape[0]
    if K is None:
        K = a.shape[-1]
    if N is None:
        N = b.shape[0]
    args = L.GemmArgs()
    args.A, args.lda = a.data_ptr(), (a.stride(-2) if a.dim() >= 2 else K) if lda is None else lda
    args.B, args.ldb = b.data_ptr(), b.stride(-2) if ldb is None else ldb
    args.M, args.N, args.K, args.batch = M, N, K, 1
    args.epilogue, args.alpha, args.beta = epilogue, 1.0, 1.0
    args.bias = 0 if bias is None else bias.data_ptr()
    if residual is not None:
        _chk(residual, BF16, "residual")
        args.residual, args.ldr = residual.data_ptr(), (residual.stride(-2) if ldr is None else ldr)
    if aux is not None:
        _chk(aux, BF16, "aux")
        args.aux, args.ldaux = aux.data_ptr(), (aux.stride(-2) if ldaux is None else ldaux)
    if out is not None:
        _chk(out, BF16, "out")
        args.C, args.ldc = out.data_ptr(), out.stride(-2) if ldc is None else ldc
    else:
        args.C, args.ldc = 1 << 20, N  # (a placeholder with the alignment a fresh tensor has: nothing is allocated for a refused call)
    if _grant_workspace(args, query, a.device, "nt_stream") <= 0:
        return None
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
        args.C, args.ldc = out.data_ptr(), out.stride(-2)
    return args, out


def gemm_nt_stream(a, b, *, M=None, N=None, K=None, lda=None, ldb=None, out=None, bias=None, residual=None, aux=None,
                   epilogue=L.EPI_NONE, ldc=None, ldaux=None, ldr=None, _args_only=False):
    """C[M,N] = A[M,K] @ B[N,K]^T (+bias) (gelu) (+residual) on the weight-streaming kernel for M <= 32 (csrc/gemm_stream.hip,
    wft_gemm_nt_stream_bf16): the keywords of `gemm_nt` that apply.  Returns None — nothing launched — when the library does not
    serve the call in that form (wft_gemm_nt_stream_ok): the caller sends it to `gemm_nt`.  The fp32 partials live in a scratch
    slot of their own ("nt_stream")."""
    served = _stream_args(a, b, BF16, "wft_gemm_nt_stream_workspace_bytes", M, N, K, lda, ldb, out, bias, residual, aux, epilogue, ldc, ldaux, ldr)
    if served is None or _args_only:
        return served
    args, out = served
    L.check(L.load().wft_gemm_nt_stream_bf16(C.byref(args), L.stream_ptr()), "wft_gemm_nt_stream_bf16")
    return out


def gemm_nt_stream_q8(a, q, scale, *, M=None, N=None, K=None, lda=None, ldb=None, out=None, bias=None, residual=None, aux=None,
                      epilogue=L.EPI_NONE, ldc=None, ldaux=None, ldr=None, _args_only=False):
    """gemm_nt_stream on int8 weights: C = (A[M,K] @ Q[N,K]^T) * scale[N] (+bias) (gelu) (+residual) (wft_gemm_nt_stream_q8; q int8
    [N, K], scale f32 [N] — what `quantize_rows_i8` made of a bf16 shadow).  None — nothing launched — when wft_gemm_nt_stream_q8_ok
    does not serve the call: the caller sends it to `gemm_nt_stream` on the bf16 shadow.  The partials share the "nt_stream" slot."""
    _chk(scale, F32, "scale")
    served = _stream_args(a, q, torch.int8, "wft_gemm_nt_stream_q8_workspace_bytes", M, N, K, lda, ldb, out, bias, residual, aux, epilogue, ldc,
                          ldaux, ldr)
    if served is None or _args_only:
        return served
    args, out = served
    if scale.numel() < args.N or not scale.is_contiguous():
        raise L.WftError(f"scale: expected a contiguous f32 vector of at least N={args.N} elements, got {tuple(scale.shape)}")
    L.check(L.load().wft_gemm_nt_stream_q8(C.byref(args), _p(scale), L.stream_ptr()), "wft_gemm_nt_stream_q8")
    return out


def gemm_nt_stream_q8_serves(M: int, N: int, K: int, epilogue=L.EPI_NONE) -> bool:
    """Shapes only (wft_gemm_nt_stream_q8_ok on placeholder pointers with the alignment real operands have): would the int8 streaming
    kernel take an [M, K] x [N, K]^T product?  Asked BEFORE an int8 image is built for a group, so a product the kernel never serves
    (the prefill's cross key / value projection, M = B * n_audio_ctx) never gets one."""
    args = L.GemmArgs()
    args.A = args.B = args.C = 1 << 20
    args.lda, args.ldb, args.ldc = K, K, N
    args.M, args.N, args.K, args.batch, args.alpha, args.beta = M, N, K, 1, 1.0, 1.0
    args.epilogue = epilogue
    return bool(L.load().wft_gemm_nt_stream_q8_ok(C.byref(args)))


def _i8_shape_args(M: int, N: int, K: int, epilogue) -> "L.GemmArgs":
    args = L.GemmArgs()
    args.A = args.B = args.C = 1 << 20  # (placeholders with the alignment real operands have)
    args.lda, args.ldb, args.ldc = K, K, N
    args.M, args.N, args.K, args.batch, args.alpha, args.beta = M, N, K, 1, 1.0, 1.0
    args.epilogue = epilogue
    return args


def gemm_nt_i8(a_q, a_scale, b_q, b_scale, *, bias=None, residual=None, epilogue=L.EPI_NONE, out=None):
    """W8A8 product on the int8 matrix cores (wft_gemm_nt_i8; include/wft.h states the definition):
    C[M,N] = bf16(epi((a_q[M,K] @ b_q[N,K]^T) * (a_scale[M] x b_scale[N]) + bias) + residual); a_q / b_q int8 with unit column stride,
    the scales contiguous f32 — what `quantize_rows_i8` makes of an activation matrix and of a weight shadow.  A call the library
    does not serve raises WftError with its reason (ask `gemm_nt_i8_serves` first): there is no other kernel behind this one."""
    _chk(a_q, torch.int8, "a_q"); _chk(b_q, torch.int8, "b_q"); _chk(a_scale, F32, "a_scale"); _chk(b_scale, F32, "b_scale")
    if a_q.dim() != 2 or b_q.dim() != 2 or a_q.stride(1) != 1 or b_q.stride(1) != 1 or a_q.shape[1] != b_q.shape[1]:
        raise L.WftError(f"gemm_nt_i8: a_q [M, K] and b_q [N, K] with unit column stride, got {tuple(a_q.shape)} and {tuple(b_q.shape)}")
    M, Kd = a_q.shape
    N = b_q.shape[0]
    if a_scale.numel() < M or b_scale.numel() < N or not a_scale.is_contiguous() or not b_scale.is_contiguous():
        raise L.WftError(f"gemm_nt_i8: the scales must be contiguous f32 vectors of at least M={M} and N={N} elements")
    args = _i8_shape_args(M, N, Kd, epilogue)
    args.A, args.lda = a_q.data_ptr(), a_q.stride(0)
    args.B, args.ldb = b_q.data_ptr(), b_q.stride(0)
    if bias is not None:
        _chk(bias, F32, "bias")
        if bias.numel() < N or not bias.is_contiguous():
            raise L.WftError(f"gemm_nt_i8: bias must be a contiguous f32 vector of at least N={N} elements")
        args.bias = bias.data_ptr()
    if residual is not None:
        _chk(residual, BF16, "residual")
        if residual.dim() != 2 or residual.stride(1) != 1 or residual.shape[0] < M or residual.shape[1] < N:
            raise L.WftError(f"gemm_nt_i8: residual must cover [M={M}, N={N}] with unit column stride, got {tuple(residual.shape)}")
        args.residual, args.ldr = residual.data_ptr(), residual.stride(0)
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a_q.device)
    _chk(out, BF16, "out")
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < M or out.shape[1] < N:
        raise L.WftError(f"gemm_nt_i8: out must cover [M={M}, N={N}] with unit column stride, got {tuple(out.shape)}")
    args.C, args.ldc = out.data_ptr(), out.stride(0)
    L.check(L.load().wft_gemm_nt_i8(C.byref(args), _p(a_scale), _p(b_scale), L.stream_ptr()), "wft_gemm_nt_i8")
    return out


def gemm_nt_i8_serves(M: int, N: int, K: int, epilogue=L.EPI_NONE) -> bool:
    """Shapes only (wft_gemm_nt_i8_ok on placeholder pointers with the alignment real operands have): would the W8A8 kernel take an
    [M, K] x [N, K]^T product?  Asked before the activation is quantised and before an int8 image is built for a group."""
    return bool(L.load().wft_gemm_nt_i8_ok(C.byref(_i8_shape_args(M, N, K, epilogue))))


def quantize_rows_i8(w, out=None, scale=None):
    """bf16 [rows, cols] (row stride ldw) -> (int8 [rows, cols], f32 [rows]): per-row symmetric quantisation of a weight shadow
    (wft_quantize_rows_i8; include/wft.h states the definition).  `out` / `scale`: buffers to write in place."""
    _chk(w, BF16, "w")
    rows, cols = w.shape
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.int8, device=w.device)
    if scale is None:
        scale = torch.empty(rows, dtype=F32, device=w.device)
    _chk(out, torch.int8, "out"); _chk(scale, F32, "scale")
    if w.stride(1) != 1 or out.stride(1) != 1 or tuple(out.shape) != (rows, cols) or scale.numel() < rows or not scale.is_contiguous():
        raise L.WftError("quantize_rows_i8: w and out must be [rows, cols] with unit column stride, scale a contiguous f32 [rows]")
    L.check(L.load().wft_quantize_rows_i8(_p(w), rows, cols, w.stride(0), _p(out), out.stride(0), _p(scale), L.stream_ptr()),
            "wft_quantize_rows_i8")
    return out, scale


def gemm_nt_aux8_bytes(M: int, N: int, K: int, device, epilogue=None, colsum: bool = False) -> int:
    """Bytes of the one-byte gelu' buffer if an [M, K] x [N, K]^T product with the GELU_GRAD8 / MUL_AUX8 epilogue is served by
    gemm_nt4w_kernel (wft_gemm_nt_aux8_bytes), else 0.  Shapes only — the pointers are placeholders with the alignment real operands have."""
    args = L.GemmArgs()
    args.A = args.B = args.C = args.aux = 1 << 20
    args.lda, args.ldb, args.ldc = K, K, N
    args.M, args.N, args.K, args.batch, args.alpha, args.beta = M, N, K, 1, 1.0, 1.0
    args.epilogue = L.EPI_GELU_GRAD8 if epilogue is None else epilogue
    args.variant = VARIANT["nt"]
    if colsum:
        args.colsum = 1 << 20
    return int(L.load().wft_gemm_nt_aux8_bytes(C.byref(args)))


def gemm_tn(a, b, *, P=None, Q=None, R=None, lda=None, ldb=None, out=None, out_f32=True, accumulate=False,
            alpha=1.0, batch=1, strideA=0, strideB=0, p_valid=0, col_scale=None, scale_rows=0, block_n=0, block_r=0,
            seg_out=None, _args_only=False, _ws_slot="tn"):
    """C[P,Q] (+)= alpha * A[R,P]^T @ B[R,Q]  (weight gradients).  p_valid (P = 128 only): columns >= p_valid of A are zero
    padding (a rank-r LoRA operand): the reduction runs in the load-stream kernel for rank-r operands (gemm.hip
    gemm_tn_rank_kernel — 4-stage LDS-DMA ring, compact A, compact split-K workspace), bit-identical to the general path.
    With p_valid the kernel that sums the split-K partials can also finish the two LoRA adapter gradients (wft.h tn_col_scale /
    tn_block_n): col_scale f32 [S, Q] multiplies C[p, q] by col_scale[p // scale_rows, q] (dA = (du^T x) * mask);
    block_n / block_r return a flat f32 tensor of Q / block_n blocks [block_n, block_r], block b = the transpose of rows
    b*block_r.., columns b*block_n.. of the product (dB of adapter b as [out, r] row-major).
    seg_out: 1..4 contiguous f32 [rows_i, Q] tensors that receive consecutive row ranges of the product INSTEAD of one [P, Q]
    tensor (wft.h tn_seg_*: each parameter of a fused Linear group gets its gradient where it lives — a DDP bucket view);
    returns None if the library does not take the call in that form (the caller falls back to `out` + slicing), else seg_out."""
    _chk(a, BF16, "A"); _chk(b, BF16, "B")
    if R is None:
        R = a.shape[0]
    if P is None:
        P = a.shape[1]
    if Q is None:
        Q = b.shape[1]
    if lda is None:
        lda = a.stride(0)
    if ldb is None:
        ldb = b.stride(0)
    if seg_out is not None:
        out, ldc = seg_out[0], Q
    elif block_n:
        if out is None:
            out = torch.empty(Q * block_r, dtype=F32, device=a.device)
            accumulate = False
        ldc = Q
    else:
        if out is None:
            # col_scale form (dA of a group's adapters): the library writes p_valid rows only — a compact gradient tensor
            rows = int(p_valid) if (col_scale is not None and p_valid > 0) else P
            out = torch.empty((rows, Q), dtype=F32 if out_f32 else BF16, device=a.device)
            accumulate = False
        ldc = out.stride(0)
    args = L.GemmArgs()
    args.A, args.lda, args.strideA = a.data_ptr(), lda, strideA
    args.B, args.ldb, args.strideB = b.data_ptr(), ldb, strideB
    args.C, args.ldc, args.strideC = out.data_ptr(), ldc, 0
    args.c_is_f32, args.accumulate = int(out.dtype == F32), int(accumulate)
    args.epilogue, args.alpha = L.EPI_NONE, alpha
    args.M, args.N, args.K, args.batch = P, Q, R, batch
    args.p_valid = int(p_valid)
    if col_scale is not None:
        _chk(col_scale, F32, "col_scale")
        args.tn_col_scale, args.tn_scale_rows = col_scale.data_ptr(), int(scale_rows)
    args.tn_block_n, args.tn_block_r = int(block_n), int(block_r)
    args.variant = VARIANT["tn"]
    lib = L.load()
    if seg_out is not None:
        end = 0
        args.tn_seg_count = len(seg_out)
        for i, t in enumerate(seg_out):
            end += t.shape[0]
            args.tn_seg_end[i], args.tn_seg_ptr[i] = end, t.data_ptr()
        if not lib.wft_gemm_tn_segments_ok(C.byref(args)):
            return None
    _grant_workspace(args, "wft_gemm_tn_workspace_bytes", a.device, _ws_slot)
    if _args_only:  # (paired launches: gemm_tn_rank_pair)
        return args, out
    L.check(lib.wft_gemm_tn_bf16(C.byref(args), L.stream_ptr()), "wft_gemm_tn_bf16")
    return out if seg_out is None else seg_out


def gemm_nt_rank_pair(a0, b0, a1, b1, p_valid: int):
    """(a0 @ b0^T, a1 @ b1^T) for two rank-r operands b0, b1 ([128, K] padded buffers, p_valid data rows) in ONE launch of the
    load-stream kernel (wft_gemm_nt_rank_pair_bf16): u = x (sA*m)^T and du = dy (sB) of an adapted Linear group's backward."""
    args0, out0 = gemm_nt(a0, b0, p_valid=p_valid, _args_only=True)
    args1, out1 = gemm_nt(a1, b1, p_valid=p_valid, _args_only=True)
    L.check(L.load().wft_gemm_nt_rank_pair_bf16(C.byref(args0), C.byref(args1), L.stream_ptr()), "wft_gemm_nt_rank_pair_bf16")
    return out0, out1


def gemm_tn_rank_pair(kw0: dict, kw1: dict):
    """Two gemm_tn(**kw) products with rank-r A operands (p_valid) in ONE launch plus ONE split-K reduce launch
    (wft_gemm_tn_rank_pair_bf16): dA = (du^T x) * mask and dB = u^T dy of an adapted Linear group.  Each product has its own
    workspace."""
    args0, out0 = gemm_tn(**kw0, _args_only=True, _ws_slot="tn")
    args1, out1 = gemm_tn(**kw1, _args_only=True, _ws_slot="tn_b")
    L.check(L.load().wft_gemm_tn_rank_pair_bf16(C.byref(args0), C.byref(args1), L.stream_ptr()), "wft_gemm_tn_rank_pair_bf16")
    return out0, out1


_TN_WS = {}


def _tn_workspace(device, nbytes: int, slot: str = "tn") -> torch.Tensor:
    """Per-device scratch for deterministic split-K weight-gradient GEMMs / fused column sums (grown on demand,
    reused: all launches are ordered on one stream)."""
    key = (device.type, device.index, slot)
    ws = _TN_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 64 << 20), dtype=torch.uint8, device=device)
        _TN_WS[key] = ws
    return ws


def _grant_workspace(args, query: str, device, slot: str) -> int:
    """Ask the library's `query`(args) how much scratch the call wants and, if any, point args.workspace / workspace_bytes at the
    device's `slot`.  -> the answer (<= 0: no workspace wanted, or the call is not served in that form)."""
    need = getattr(L.load(), query)(C.byref(args))
    if need > 0:
        ws = _tn_workspace(device, need, slot=slot)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel()
    return need


# --------------------------------------------------------------------------- attention
def _attn_view(t: torch.Tensor):
    """t: [B, T, H*64-ish view] with last-dim stride 1 -> (ptr, ld, batch_stride)."""
    assert t.dim() == 3 and t.stride(2) == 1
    return t.data_ptr(), t.stride(1), t.stride(0)


def attn_fwd(q, k, v, n_head: int, causal: bool, scale: float, q_prescaled: bool = False, o=None, lse=None):
    """q [B,Tq,H*64], k/v [B,Tk,H*64] bf16 views (any row stride) -> o [B,Tq,H*64], lse [B,H,Tq].
    q_prescaled: q already carries scale * log2(e) (ops.QK_PRESCALE folded into the q projection's forward shadow).
    o / lse: optional outputs to write into (o: a bf16 [B,Tq,H*64] view of any row stride; lse: contiguous f32 [B,H,Tq])."""
    for n, t in (("q", q), ("k", k), ("v", v)):
        _chk(t, BF16, n)
    B, Tq, D = q.shape
    Tk = k.shape[1]
    assert D == n_head * 64, "head_dim must be 64"
    if o is None:
        o = torch.empty((B, Tq, D), dtype=BF16, device=q.device)
    else:
        _chk(o, BF16, "o")
        assert o.shape == (B, Tq, D)
    if lse is None:
        lse = torch.empty((B, n_head, Tq), dtype=F32, device=q.device)
    else:
        _chk(lse, F32, "lse")
        assert lse.shape == (B, n_head, Tq) and lse.is_contiguous()
    a = L.AttnArgs()
    a.q, a.ldq, a.q_bs = _attn_view(q)
    a.k, a.ldk, a.k_bs = _attn_view(k)
    a.v, a.ldv, a.v_bs = _attn_view(v)
    a.o, a.ldo, a.o_bs = _attn_view(o)
    a.lse = lse.data_ptr()
    a.B, a.H, a.Tq, a.Tk, a.causal, a.scale = B, n_head, Tq, Tk, int(causal), scale
    a.variant, a.q_prescaled = _attn_variant_bits(), int(bool(q_prescaled))
    L.check(L.load().wft_attn_fwd_bf16(C.byref(a), L.stream_ptr()), "wft_attn_fwd_bf16")
    return o, lse


def attn_bwd(q, k, v, o, lse, do, n_head: int, causal: bool, scale: float, dq=None, dk=None, dv=None, colsums=None,
             q_prescaled: bool = False, launch: int = 0):
    """colsums = (cs_q, cs_v): optional f32 [H*64] outputs, the column sums over (batch, time) of dq / dv (bias gradients).
    q_prescaled: as in attn_fwd; dq is the gradient w.r.t. the UNSCALED projection output either way."""
    B, Tq, D = q.shape
    Tk = k.shape[1]
    _chk(do, BF16, "do")
    if do.stride(2) != 1:
        do = do.contiguous()
    dq = torch.empty((B, Tq, D), dtype=BF16, device=q.device) if dq is None else dq
    dk = torch.empty((B, Tk, D), dtype=BF16, device=q.device) if dk is None else dk
    dv = torch.empty((B, Tk, D), dtype=BF16, device=q.device) if dv is None else dv
    delta = torch.empty((2, B, n_head, Tq), dtype=F32, device=q.device)  # kernel-internal workspace: [0] -rowsum(dO*O), [1] -lse/scale
    a = L.AttnArgs()
    a.q, a.ldq, a.q_bs = _attn_view(q)
    a.k, a.ldk, a.k_bs = _attn_view(k)
    a.v, a.ldv, a.v_bs = _attn_view(v)
    a.o, a.ldo, a.o_bs = _attn_view(o)
    a.lse = lse.data_ptr()
    a.B, a.H, a.Tq, a.Tk, a.causal, a.scale = B, n_head, Tq, Tk, int(causal), scale
    a.d_o, a.lddo, a.do_bs = _attn_view(do)
    a.delta = delta.data_ptr()
    a.dq, a.lddq, a.dq_bs = _attn_view(dq)
    a.dk, a.lddk, a.dk_bs = _attn_view(dk)
    a.dv, a.lddv, a.dv_bs = _attn_view(dv)
    a.variant, a.q_prescaled, a.launch_mode = _attn_variant_bits(), int(bool(q_prescaled)), _launch(launch)
    if colsums is not None:
        cs_q, cs_v = colsums
        _chk(cs_q, F32, "cs_q"); _chk(cs_v, F32, "cs_v")
        assert cs_q.numel() == D and cs_v.numel() == D and cs_q.is_contiguous() and cs_v.is_contiguous()
        ws = _tn_workspace(q.device, L.load().wft_attn_bwd_colsum_workspace_bytes(C.byref(a)), slot="attn_colsum")
        a.dq_colsum, a.dv_colsum, a.colsum_ws = cs_q.data_ptr(), cs_v.data_ptr(), ws.data_ptr()
    L.check(L.load().wft_attn_bwd_bf16(C.byref(a), L.stream_ptr()), "wft_attn_bwd_bf16")
    return dq, dk, dv


# --------------------------------------------------------------------------- greedy decoding (csrc/decode_attn.hip, csrc/decode_pick.hip)
def _attn_decode_call(a, stem: str, q, cache, n_head: int, scale: float, new_kv, lens, q_prescaled: bool, out, args_only: bool, group: int = 1):
    """What AttnDecodeArgs and AttnDecodeBeamArgs share: the layout checks, q / cache / o, the step's k / v rows with `lens`, the
    workspace slot and the call of `stem`_bf16.  The caller has set the fields of its own struct (rows, group, anc) before."""
    who = stem[4:]  # (also the workspace slot)
    _chk(q, BF16, "q"); _chk(cache, BF16, "cache")
    R, D = q.shape
    if D != n_head * 64 or cache.dim() != 3 or cache.shape[0] != R // group or cache.shape[2] != 2 * D or q.stride(1) != 1 or cache.stride(2) != 1:
        raise ValueError(f"{who}: q {tuple(q.shape)} / cache {tuple(cache.shape)} do not fit {n_head} heads of 64 at group {group}")
    o = torch.empty((R, D), dtype=BF16, device=q.device) if out is None else out
    a.q, a.ldq = q.data_ptr(), q.stride(0)
    a.k_cache, a.v_cache = cache.data_ptr(), cache.data_ptr() + 2 * D
    a.ld_cache, a.cache_bs = cache.stride(1), cache.stride(0)
    a.o, a.ldo = o.data_ptr(), o.stride(0)
    if new_kv is not None:
        k, v = new_kv
        _chk(k, BF16, "k_new"); _chk(v, BF16, "v_new")
        _chk_flag(lens, R, "lens")
        if k.shape != (R, D) or v.shape != (R, D) or k.stride() != v.stride() or k.stride(1) != 1:
            raise ValueError(f"{who}: k_new / v_new must be [rows, H*64] views with one row stride")
        a.k_new, a.v_new, a.ld_new, a.len = k.data_ptr(), v.data_ptr(), k.stride(0), lens.data_ptr()
    a.H, a.Tk, a.scale, a.q_prescaled = n_head, cache.shape[1], scale, int(bool(q_prescaled))
    _grant_workspace(a, stem + "_workspace_bytes", q.device, who)
    if args_only:  # (timing tools replay one argument struct)
        return a, o
    L.check(getattr(L.load(), stem + "_bf16")(C.byref(a), L.stream_ptr()), stem + "_bf16")
    return o


def attn_decode(q, cache, n_head: int, scale: float, *, new_kv=None, lens=None, q_prescaled: bool = False, out=None, _args_only=False):
    """Single-token attention (wft_attn_decode_bf16).  q bf16 [B, H*64] (any row stride); cache bf16 [B, Tk, 2*H*64], rows {k | v}.
    Self-attention form: new_kv = (k, v) bf16 [B, H*64] views of the step's fused projection output and lens i32 [B] — the rows
    are written to cache[b, lens[b] - 1] and attended over keys 0 .. lens[b] - 1.  Cross-attention form (neither given): all Tk
    keys, the cache is only read.  -> o bf16 [B, H*64]."""
    if (new_kv is None) != (lens is None):
        raise ValueError("attn_decode: the self-attention form needs both new_kv and lens")
    _chk(q, BF16, "q")
    a = L.AttnDecodeArgs()
    a.B = q.shape[0]
    return _attn_decode_call(a, "wft_attn_decode", q, cache, n_head, scale, new_kv, lens, q_prescaled, out, _args_only)


def decode_embed(tokens, lens, emb, pos):
    """out[b] = emb[tokens[b, lens[b] - 1]] + pos[lens[b] - 1] -> bf16 [B, d]; tokens i64 [B, n_ctx], lens i32 [B] on the device."""
    _chk(tokens, torch.int64, "tokens"); _chk(emb, F32, "emb"); _chk(pos, F32, "pos")
    B = tokens.shape[0]
    _chk_flag(lens, B, "lens")
    V, d = emb.shape
    n_ctx = pos.shape[0]
    if tokens.dim() != 2 or tokens.stride(1) != 1 or tokens.shape[1] < n_ctx or not emb.is_contiguous() or not pos.is_contiguous():
        raise ValueError("decode_embed: tokens must be [B, >= n_ctx] with contiguous rows, emb / pos contiguous")
    out = torch.empty((B, d), dtype=BF16, device=emb.device)
    L.check(L.load().wft_decode_embed(_p(tokens), tokens.stride(0), _p(lens), _p(emb), _p(pos), _p(out), B, n_ctx, d, V, L.stream_ptr()),
            "wft_decode_embed")
    return out


def _set_suppress(a, V: int, suppress, suppress_first) -> None:
    """The two suppression masks (u8 [V] or None) of DecodePickArgs / DecodeTopkArgs."""
    for name, m in (("suppress", suppress), ("suppress_first", suppress_first)):
        if m is not None:
            _chk(m, torch.uint8, name)
            if m.numel() != V or not m.is_contiguous():
                raise ValueError(f"{name}: expected a contiguous uint8 mask of {V} entries")
            setattr(a, name, m.data_ptr())


def _ts_rules(ts_rules):
    """(ts_begin, no_timestamps or None, max_initial or None) -> TsRules (None / a negative value: -1, "none")."""
    ts_begin, no_ts, max_initial = ts_rules
    ru = L.TsRules()
    ru.ts_begin = int(ts_begin)
    ru.no_timestamps = -1 if no_ts is None else int(no_ts)
    ru.max_initial = -1 if max_initial is None else int(max_initial)
    return ru


def _pick_args(logits, V: int, tokens, lens, finished, sum_logprob, unfinished, eot, max_len, suppress, suppress_first, first_len, want_pick, group=1):
    """DecodePickArgs of decode_pick / decode_sample for the R = tokens.shape[0] state rows (logits: R // group rows) -> (args, pick, lp)."""
    _chk(logits, BF16, "logits"); _chk(tokens, torch.int64, "tokens"); _chk(sum_logprob, F32, "sum_logprob")
    B = tokens.shape[0]
    assert logits.dim() == 2 and logits.stride(1) == 1 and tokens.dim() == 2 and tokens.stride(1) == 1 and logits.shape[0] * group == B
    _chk_flag(lens, B, "lens"); _chk_flag(finished, B, "finished"); _chk_flag(unfinished, 1, "unfinished")
    a = L.DecodePickArgs()
    a.logits, a.ld, a.V = logits.data_ptr(), logits.stride(0), V
    _set_suppress(a, V, suppress, suppress_first)
    if first_len is not None:
        _chk_flag(first_len, B, "first_len")
        a.first_len = first_len.data_ptr()
    a.tokens, a.ld_tokens = tokens.data_ptr(), tokens.stride(0)
    a.len, a.finished, a.sum_logprob, a.unfinished = lens.data_ptr(), finished.data_ptr(), sum_logprob.data_ptr(), unfinished.data_ptr()
    pick = lp = None
    if want_pick:
        pick = torch.empty(B, dtype=torch.int64, device=logits.device)
        lp = torch.empty(B, dtype=F32, device=logits.device)
        a.pick_out, a.logprob_out = pick.data_ptr(), lp.data_ptr()
    a.B, a.eot, a.max_len = B, int(eot), int(max_len)
    return a, pick, lp


def _pick_call(entry, ts_rules, *structs):
    """entry(*structs, stream), or with ts_rules its _ts form: the timestamp rules follow the structs."""
    if ts_rules is not None:
        entry, structs = entry + "_ts", structs + (_ts_rules(ts_rules),)
    L.check(getattr(L.load(), entry)(*map(C.byref, structs), L.stream_ptr()), entry)


def decode_pick(logits, V: int, tokens, lens, finished, sum_logprob, unfinished, *, eot: int, max_len: int, suppress=None,
                suppress_first=None, first_len=None, want_pick: bool = False, ts_rules=None):
    """Greedy pick + state update (wft_decode_pick; include/wft.h).  logits bf16 [B, ld >= V]; suppress / suppress_first u8 [V] or None.
    want_pick -> (pick i64 [B], logprob f32 [B]) as computed for EVERY row, finished or not.
    ts_rules = (ts_begin, no_timestamps or None, max_initial or None): the pick under the timestamp rules (wft_decode_pick_ts)."""
    a, pick, lp = _pick_args(logits, V, tokens, lens, finished, sum_logprob, unfinished, eot, max_len, suppress, suppress_first, first_len, want_pick)
    _pick_call("wft_decode_pick", ts_rules, a)
    return pick, lp


def decode_sample(logits, V: int, tokens, lens, finished, sum_logprob, unfinished, temperature, seed, *, group: int = 1, eot: int,
                  max_len: int, suppress=None, suppress_first=None, first_len=None, want_pick: bool = False, ts_rules=None):
    """Sampled pick + state update (wft_decode_sample; include/wft.h "Sampled decoding").  As decode_pick for the R = tokens.shape[0]
    state rows; logits bf16 [R // group, ld >= V], state row r reads logits row r // group.  temperature f32 [R] and seed i64 [R]
    (the bits of a u64) live on the device and are read by the kernel: rows with temperature <= 0 pick greedily, the others draw
    from softmax(logits / temperature) over the live columns; the log-probability is the pick's at temperature 1.
    ts_rules: as decode_pick (wft_decode_sample_ts)."""
    group = int(group)
    if group < 1 or tokens.shape[0] % group:
        raise ValueError(f"decode_sample: group={group} must be >= 1 and divide the {tokens.shape[0]} state rows")
    a, pick, lp = _pick_args(logits, V, tokens, lens, finished, sum_logprob, unfinished, eot, max_len, suppress, suppress_first, first_len, want_pick,
                             group=group)
    _chk(temperature, F32, "temperature"); _chk(seed, torch.int64, "seed")
    if temperature.numel() != a.B or seed.numel() != a.B or not temperature.is_contiguous() or not seed.is_contiguous():
        raise ValueError(f"decode_sample: temperature f32 / seed i64 must be contiguous [{a.B}]")
    s = L.SampleRules()
    s.temperature, s.seed, s.group = temperature.data_ptr(), seed.data_ptr(), group
    _pick_call("wft_decode_sample", ts_rules, a, s)
    return pick, lp


# --------------------------------------------------------------------------- beam-search decoding (csrc/decode_attn.hip, csrc/decode_beam.hip)
def attn_decode_beam(q, cache, n_head: int, scale: float, *, new_kv=None, lens=None, anc=None, group: int = 1, q_prescaled: bool = False,
                     out=None, _args_only=False):
    """Single-token attention for beams (wft_attn_decode_beam_bf16).  q bf16 [R, H*64] (any row stride).
    Self form (new_kv, lens, anc given): cache bf16 [R, Tk, 2*H*64] of slot rows; key t of row r is read at slot anc[r, t] (i32
    [R, >= Tk]), the step's k / v rows are written to cache[r, lens[r] - 1].  Cross form: cache bf16 [R // group, Tk, 2*H*64], read
    only, shared by the `group` consecutive rows of an audio.  -> o bf16 [R, H*64]."""
    _chk(q, BF16, "q"); _chk(cache, BF16, "cache")
    R = q.shape[0]
    if (new_kv is None) != (lens is None) or (anc is None) != (lens is None):
        raise ValueError("attn_decode_beam: the self form needs new_kv, lens and anc together")
    if not 1 <= int(group) <= 8 or R % int(group) or (lens is not None and group != 1):
        raise ValueError(f"attn_decode_beam: group={group} must lie in 1..8 and divide the {R} rows (1 in the self form)")
    a = L.AttnDecodeBeamArgs()
    a.R, a.group = R, int(group)
    if anc is not None:
        _chk(anc, torch.int32, "anc")
        if anc.dim() != 2 or anc.shape[0] != R or cache.dim() != 3 or anc.shape[1] < cache.shape[1] or anc.stride(1) != 1:
            raise ValueError(f"attn_decode_beam: anc must be i32 [R, >= {cache.shape[1] if cache.dim() == 3 else 'Tk'}] with contiguous rows")
        a.anc, a.ld_anc = anc.data_ptr(), anc.stride(0)
    return _attn_decode_call(a, "wft_attn_decode_beam", q, cache, n_head, scale, new_kv, lens, q_prescaled, out, _args_only, group=int(group))


def decode_topk(logits, V: int, cand_tok, cand_logp, *, lens=None, first_len=None, suppress=None, suppress_first=None, row_step: int = 1,
                ts_rules=None, tokens=None, eot: Optional[int] = None):
    """The k best continuations per logits row (wft_decode_topk).  logits bf16 [rows, ld >= V]; logits row i belongs to state row
    i * row_step of lens / first_len / cand_tok i32 [R, k] / cand_logp f32 [R, k], which receive (token, log-probability) in
    descending order, ties to the lower token.
    ts_rules = (ts_begin, no_timestamps or None, max_initial or None) with tokens i64 [R, n_ctx] and eot: the candidates under the
    timestamp rules (wft_decode_topk_ts)."""
    _chk(logits, BF16, "logits"); _chk(cand_tok, torch.int32, "cand_tok"); _chk(cand_logp, F32, "cand_logp")
    rows = logits.shape[0]
    if logits.dim() != 2 or logits.stride(1) != 1 or cand_tok.dim() != 2 or cand_tok.shape != cand_logp.shape or not cand_tok.is_contiguous() \
            or not cand_logp.is_contiguous() or row_step < 1 or (rows - 1) * row_step >= cand_tok.shape[0]:
        raise ValueError("decode_topk: logits [rows, ld], cand_tok / cand_logp contiguous [R, k] with (rows - 1) * row_step < R")
    R, k = cand_tok.shape
    a = L.DecodeTopkArgs()
    a.logits, a.ld, a.V = logits.data_ptr(), logits.stride(0), V
    _set_suppress(a, V, suppress, suppress_first)
    if lens is not None:
        _chk_flag(lens, R, "lens")
        a.len = lens.data_ptr()
    if first_len is not None:
        _chk_flag(first_len, R, "first_len")
        a.first_len = first_len.data_ptr()
    a.cand_tok, a.cand_logp = cand_tok.data_ptr(), cand_logp.data_ptr()
    a.rows, a.row_step, a.k = rows, int(row_step), k
    if ts_rules is not None:
        if tokens is None or eot is None:
            raise ValueError("decode_topk: the timestamp rules need tokens and eot")
        _chk(tokens, torch.int64, "tokens")
        if tokens.dim() != 2 or tokens.shape[0] != R or not tokens.is_contiguous():
            raise ValueError(f"decode_topk: tokens must be contiguous i64 [{R}, n_ctx]")
        ru = _ts_rules(ts_rules)
        L.check(L.load().wft_decode_topk_ts(C.byref(a), C.byref(ru), tokens.data_ptr(), tokens.shape[1], int(eot), L.stream_ptr()),
                "wft_decode_topk_ts")
        return
    L.check(L.load().wft_decode_topk(C.byref(a), L.stream_ptr()), "wft_decode_topk")


def beam_update(cand_tok, cand_logp, tokens, anc, lens, sum_logprob, done, unfinished, fin_tokens, fin_len, fin_score, fin_n, *, eot: int,
                max_len: int, first: bool = False, src_out=None):
    """One beam-search step per audio (wft_beam_update; include/wft.h).  cand_* [R, W + 1]; tokens i64 / anc i32 [R, n_ctx]; lens i32 /
    sum_logprob f32 [R]; done i32 [B], unfinished i32 [1]; fin_tokens i64 [B, C, n_ctx], fin_len i32 / fin_score f32 [B, C], fin_n i32
    [B].  Everything is updated in place."""
    _chk(cand_tok, torch.int32, "cand_tok"); _chk(cand_logp, F32, "cand_logp"); _chk(tokens, torch.int64, "tokens"); _chk(anc, torch.int32, "anc")
    _chk(sum_logprob, F32, "sum_logprob"); _chk(fin_tokens, torch.int64, "fin_tokens"); _chk(fin_score, F32, "fin_score")
    R, k = cand_tok.shape
    W, B = k - 1, done.numel()
    if W < 1 or R != B * W or fin_tokens.dim() != 3 or fin_tokens.shape[0] != B:
        raise ValueError(f"beam_update: {R} candidate rows of {k} do not fit {B} audios")
    Cn = fin_tokens.shape[1]
    ok = (cand_tok.is_contiguous() and cand_logp.is_contiguous() and cand_logp.shape == (R, k) and tokens.dim() == 2 and tokens.shape[0] == R
          and tokens.stride(1) == 1 and anc.dim() == 2 and anc.shape[0] == R and anc.stride(1) == 1 and fin_tokens.is_contiguous()
          and fin_tokens.shape[2] == tokens.stride(0) and fin_len.is_contiguous() and fin_score.is_contiguous()
          and tuple(fin_len.shape) == (B, Cn) and tuple(fin_score.shape) == (B, Cn)
          and max_len <= tokens.shape[1] and max_len <= anc.shape[1])
    if not ok:
        raise ValueError("beam_update: buffer layouts do not match (see the docstring)")
    _chk_flag(lens, R, "lens"); _chk_flag(done, B, "done"); _chk_flag(unfinished, 1, "unfinished"); _chk_flag(fin_n, B, "fin_n")
    _chk(fin_len, torch.int32, "fin_len")
    a = L.BeamUpdateArgs()
    a.cand_tok, a.cand_logp = cand_tok.data_ptr(), cand_logp.data_ptr()
    a.tokens, a.ld_tokens, a.anc, a.ld_anc = tokens.data_ptr(), tokens.stride(0), anc.data_ptr(), anc.stride(0)
    a.len, a.sum_logprob, a.done, a.unfinished = lens.data_ptr(), sum_logprob.data_ptr(), done.data_ptr(), unfinished.data_ptr()
    a.fin_tokens, a.fin_len, a.fin_score, a.fin_n = fin_tokens.data_ptr(), fin_len.data_ptr(), fin_score.data_ptr(), fin_n.data_ptr()
    if src_out is not None:
        _chk_flag(src_out, R, "src_out")
        a.src_out = src_out.data_ptr()
    a.B, a.W, a.C, a.eot, a.max_len, a.first = B, W, Cn, int(eot), int(max_len), int(bool(first))
    L.check(L.load().wft_beam_update(C.byref(a), L.stream_ptr()), "wft_beam_update")


# --------------------------------------------------------------------------- word-level alignment (csrc/align.hip)
def _host_lens(host, n: int, hi: int, name: str) -> list:
    """The host copy of a device length array: n ints inside [0, hi] — checked before any launch (the kernels clamp as well)."""
    vals = [int(v) for v in host]
    if len(vals) != n or any(v < 0 or v > hi for v in vals):
        raise ValueError(f"{name}: expected {n} lengths inside 0..{hi}, got {vals}")
    return vals


def attn_probs(q, k, heads, n_tok, n_key, n_head: int, scale: float, out, *, host_lens):
    """Alignment-head probabilities (wft_attn_probs_bf16; include/wft.h "Word-level alignment").  q bf16 [B, Tq, H*64] / k bf16
    [B, Tk, H*64] views (any row stride: the k half of the cross kv buffer in place); heads i32 [n] on the device; n_tok / n_key
    i32 [B] on the device with host_lens = (their values on the host); out f32 [B, n, Tq, Tk] view with contiguous rows (a slice of
    the [B, n_sel_total, Tq, Tk] buffer) -> out, rows >= n_tok[b] and columns >= n_key[b] untouched."""
    _chk(q, BF16, "q"); _chk(k, BF16, "k"); _chk(heads, torch.int32, "heads"); _chk(out, F32, "out")
    B, Tq, D = q.shape
    Tk = k.shape[1]
    n = heads.numel()
    if D != n_head * 64 or k.shape[0] != B or k.shape[2] != D or q.stride(2) != 1 or k.stride(2) != 1:
        raise ValueError(f"attn_probs: q {tuple(q.shape)} / k {tuple(k.shape)} do not fit {n_head} heads of 64")
    if n < 1 or not heads.is_contiguous() or tuple(out.shape) != (B, n, Tq, Tk) or out.stride(3) != 1 or out.stride(2) < Tk \
            or out.stride(1) < Tq * out.stride(2):
        raise ValueError(f"attn_probs: heads must be contiguous i32 [n >= 1] and out an f32 [{B}, n, {Tq}, {Tk}] view with contiguous rows")
    _chk_flag(n_tok, B, "n_tok"); _chk_flag(n_key, B, "n_key")
    _host_lens(host_lens[0], B, Tq, "n_tok"); _host_lens(host_lens[1], B, Tk, "n_key")
    a = L.AttnArgs()
    a.q, a.ldq, a.q_bs = _attn_view(q)
    a.k, a.ldk, a.k_bs = _attn_view(k)
    a.B, a.H, a.Tq, a.Tk, a.scale = B, n_head, Tq, Tk, scale
    L.check(L.load().wft_attn_probs_bf16(C.byref(a), _p(heads), n, _p(n_tok), _p(n_key), _p(out), out.stride(0), out.stride(1), out.stride(2),
                                         L.stream_ptr()), "wft_attn_probs_bf16")
    return out


def align_matrix(probs, n_tok, n_key, width: int = 7, out=None, *, host_lens):
    """Standardise over the tokens, median-filter along the frames, average the heads (wft_align_matrix).  probs f32 [B, n_sel, Tq, Tk]
    with contiguous rows -> matrix f32 [B, Tq, Tk]; elements at rows >= n_tok[b] or columns >= n_key[b] are not written (a fresh
    `out` is zero-filled)."""
    _chk(probs, F32, "probs")
    if probs.dim() != 4 or probs.stride(3) != 1:
        raise ValueError("align_matrix: probs must be f32 [B, n_sel, Tq, Tk] with contiguous rows")
    B, n_sel, Tq, Tk = probs.shape
    width = int(width)
    if width < 1 or width > 31 or width % 2 == 0:
        raise ValueError(f"align_matrix: the filter width must be odd and lie in 1..31, got {width}")
    if out is None:
        out = torch.zeros((B, Tq, Tk), dtype=F32, device=probs.device)
    _chk(out, F32, "out")
    if tuple(out.shape) != (B, Tq, Tk) or out.stride(2) != 1:
        raise ValueError(f"align_matrix: out must be f32 [{B}, {Tq}, {Tk}] with contiguous rows")
    _chk_flag(n_tok, B, "n_tok"); _chk_flag(n_key, B, "n_key")
    _host_lens(host_lens[0], B, Tq, "n_tok"); _host_lens(host_lens[1], B, Tk, "n_key")
    L.check(L.load().wft_align_matrix(_p(probs), probs.stride(0), probs.stride(1), probs.stride(2), _p(n_tok), _p(n_key), _p(out), out.stride(0),
                                      out.stride(1), B, n_sel, Tq, Tk, width, L.stream_ptr()), "wft_align_matrix")
    return out


def dtw(matrix, row0: int, n_rows, n_cols, *, host_lens, negate: bool = True, paths=None):
    """Dynamic time warping with the backtrace (wft_dtw_f32): per audio the path through -matrix[b, row0 : row0 + n_rows[b], : n_cols[b]]
    (negate=False: the matrix as it is).  matrix f32 [B, rows, cols] with contiguous rows; n_rows / n_cols i32 [B] on the device with
    host_lens = (their values on the host) -> (path_text i32 [B, ld], path_time i32 [B, ld], path_len i32 [B]) in forward order;
    entries beyond path_len[b] keep what `paths` = (path_text, path_time, path_len) held (fresh buffers: -1)."""
    _chk(matrix, F32, "matrix")
    if matrix.dim() != 3 or matrix.stride(2) != 1:
        raise ValueError("dtw: matrix must be f32 [B, rows, cols] with contiguous rows")
    B, R, Cn = matrix.shape
    _chk_flag(n_rows, B, "n_rows"); _chk_flag(n_cols, B, "n_cols")
    row0 = int(row0)
    if row0 < 0 or row0 >= R:
        raise ValueError(f"dtw: row0={row0} is outside the {R} matrix rows")
    rows = _host_lens(host_lens[0], B, min(R - row0, 448), "n_rows")
    cols = _host_lens(host_lens[1], B, Cn, "n_cols")
    nr, nc = max(max(rows), 1), max(max(cols), 1)
    ld = nr + nc - 1
    if paths is None:
        paths = (torch.full((B, ld), -1, dtype=torch.int32, device=matrix.device), torch.full((B, ld), -1, dtype=torch.int32, device=matrix.device),
                 torch.zeros(B, dtype=torch.int32, device=matrix.device))
    pt, pj, pl = paths
    _chk(pt, torch.int32, "path_text"); _chk(pj, torch.int32, "path_time"); _chk_flag(pl, B, "path_len")
    if pt.shape != pj.shape or pt.dim() != 2 or pt.shape[0] != B or pt.shape[1] < ld or not pt.is_contiguous() or not pj.is_contiguous():
        raise ValueError(f"dtw: path_text / path_time must be contiguous i32 [{B}, >= {ld}]")
    need = L.load().wft_dtw_workspace_bytes(B, nr, nc)
    ws = _tn_workspace(matrix.device, need, slot="dtw")
    L.check(L.load().wft_dtw_f32(_p(matrix), matrix.stride(0), matrix.stride(1), R, row0, _p(n_rows), _p(n_cols), B, nr, nc, int(bool(negate)),
                                 _p(pt), _p(pj), pt.stride(0), _p(pl), _p(ws), ws.numel(), L.stream_ptr()), "wft_dtw_f32")
    return pt, pj, pl


def word_spans(paths, bounds, n_words, token_probs, tok_off, n_rows_max: int, *, host_lens, out=None):
    """Word boundary frames and mean token probabilities from DTW paths that stay on the device (wft_word_spans).  paths =
    (path_text, path_time, path_len) as `dtw` returns them; bounds i32 [B, ld_bounds] (bounds[b, w] = the path row at which word w
    starts, n_words[b] + 1 entries per audio); n_words, tok_off i32 [B]; token_probs f32 1-D, packed over the audios; n_rows_max:
    the `n_rows_max` of the dtw call (1..448); host_lens = (n_words on the host,) -> (start_frame i32, end_frame i32, prob f32),
    each [B, ld_bounds - 1]; elements at w >= n_words[b], and every element of an audio with an empty path, keep what `out` =
    (start_frame, end_frame, prob) held (fresh buffers: -1, -1, 0)."""
    pt, pj, pl = paths
    _chk(pt, torch.int32, "path_text"); _chk(pj, torch.int32, "path_time"); _chk(bounds, torch.int32, "bounds"); _chk(token_probs, F32, "token_probs")
    if pt.dim() != 2 or pt.shape != pj.shape or pt.shape[1] < 1 or not pt.is_contiguous() or not pj.is_contiguous():
        raise ValueError("word_spans: path_text / path_time must be contiguous i32 [B, ld >= 1] of one shape")
    B = pt.shape[0]
    if bounds.dim() != 2 or bounds.shape[0] != B or bounds.shape[1] < 2 or not bounds.is_contiguous():
        raise ValueError(f"word_spans: bounds must be contiguous i32 [{B}, >= 2]")
    if token_probs.dim() != 1 or token_probs.numel() < 1 or not token_probs.is_contiguous():
        raise ValueError("word_spans: token_probs must be a contiguous f32 vector with at least one element")
    _chk_flag(pl, B, "path_len"); _chk_flag(n_words, B, "n_words"); _chk_flag(tok_off, B, "tok_off")
    n_rows_max = int(n_rows_max)
    if not 1 <= n_rows_max <= 448:
        raise ValueError(f"word_spans: n_rows_max must lie in 1..448, got {n_rows_max}")
    ld = bounds.shape[1] - 1
    _host_lens(host_lens[0], B, min(ld, n_rows_max), "n_words")
    if out is None:
        out = (torch.full((B, ld), -1, dtype=torch.int32, device=pt.device), torch.full((B, ld), -1, dtype=torch.int32, device=pt.device),
               torch.zeros((B, ld), dtype=F32, device=pt.device))
    sf, ef, pr = out
    _chk(sf, torch.int32, "start_frame"); _chk(ef, torch.int32, "end_frame"); _chk(pr, F32, "prob")
    if any(tuple(t.shape) != (B, ld) or not t.is_contiguous() for t in (sf, ef, pr)):
        raise ValueError(f"word_spans: start_frame / end_frame / prob must be contiguous [{B}, {ld}]")
    L.check(L.load().wft_word_spans(_p(pt), _p(pj), pt.stride(0), _p(pl), _p(bounds), bounds.stride(0), _p(n_words), _p(token_probs),
                                    token_probs.numel(), _p(tok_off), _p(sf), _p(ef), _p(pr), ld, B, n_rows_max, L.stream_ptr()), "wft_word_spans")
    return sf, ef, pr


# --------------------------------------------------------------------------- language detection / long-form windows (csrc/transcribe.hip)
def lang_probs(logits, V: int, lang_ids):
    """Softmax and argmax over the language columns (wft_lang_probs; include/wft.h "Language detection and long-form windows").
    logits bf16 [B, ld >= V] with contiguous rows; lang_ids: the language token ids on the HOST (a sequence or a CPU tensor),
    strictly increasing, each in [0, V), 1..1024 of them — checked here, then uploaded -> (probs f32 [B, n_lang], best i64 [B])."""
    _chk(logits, BF16, "logits")
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] < 1:
        raise ValueError("lang_probs: logits must be bf16 [B >= 1, ld] with contiguous rows")
    B, ld = logits.shape[0], logits.stride(0)
    V = int(V)
    if not 1 <= V <= logits.shape[1] or ld < V:
        raise ValueError(f"lang_probs: V={V} does not fit logits rows of {logits.shape[1]} columns")
    ids = [int(i) for i in (lang_ids.tolist() if hasattr(lang_ids, "tolist") else lang_ids)]
    if not 1 <= len(ids) <= 1024:
        raise ValueError(f"lang_probs: 1..1024 language ids expected, got {len(ids)}")
    if ids[0] < 0 or ids[-1] >= V or any(a >= b for a, b in zip(ids, ids[1:])):
        raise ValueError(f"lang_probs: language ids must be strictly increasing and lie in [0, V={V})")
    dev = logits.device
    ids_dev = upload_table(ids, torch.int32, dev)
    probs = torch.empty((B, len(ids)), dtype=F32, device=dev)
    best = torch.empty(B, dtype=torch.int64, device=dev)
    L.check(L.load().wft_lang_probs(_p(logits), ld, V, _p(ids_dev), len(ids), _p(probs), probs.stride(0), _p(best), B, L.stream_ptr()),
            "wft_lang_probs")
    return probs, best


def mel_windows(mel, mel_off, ld_frames, content_frames, audio, seek, n_mels: int, n_win: int = 3000, *, host, out=None):
    """One zero-padded window per row out of the packed long log-mels (wft_mel_windows): row r is recording audio[r] from frame
    seek[r].  mel f32 1-D (the packed buffer); mel_off i64 [A], ld_frames / content_frames i32 [A] on the device with host =
    (their values on the host); audio / seek: R ints each on the HOST, checked against those copies (audio inside [0, A), seek
    inside [0, content_frames[audio])) and uploaded -> out f32 [R, n_mels, n_win]."""
    _chk(mel, F32, "mel"); _chk(mel_off, torch.int64, "mel_off")
    n_mels, n_win = int(n_mels), int(n_win)
    if mel.dim() != 1 or not mel.is_contiguous():
        raise ValueError("mel_windows: mel must be the packed 1-D f32 buffer")
    if n_mels < 1 or n_win < 4 or n_win % 4:
        raise ValueError(f"mel_windows: n_mels must be >= 1 and n_win a positive multiple of 4, got {n_mels}, {n_win}")
    offs, lds, cfs = ([int(v) for v in h] for h in host)
    A = len(offs)
    if A < 1 or len(lds) != A or len(cfs) != A or mel_off.numel() != A or not mel_off.is_contiguous():
        raise ValueError("mel_windows: mel_off / ld_frames / content_frames and their host copies must hold one entry per recording")
    _chk_flag(ld_frames, A, "ld_frames"); _chk_flag(content_frames, A, "content_frames")
    for a in range(A):
        if lds[a] < n_win or cfs[a] != lds[a] - n_win or offs[a] < 0 or offs[a] + n_mels * lds[a] > mel.numel():
            raise ValueError(f"mel_windows: recording {a} (offset {offs[a]}, {lds[a]} frames, {cfs[a]} of content) does not fit: content_frames "
                             f"must be ld_frames - {n_win} and the recording lie inside the {mel.numel()} packed elements")
    rows, seeks = [int(v) for v in audio], [int(v) for v in seek]
    R = len(rows)
    if R < 1 or len(seeks) != R:
        raise ValueError(f"mel_windows: audio and seek must hold the same number (>= 1) of rows, got {R} and {len(seeks)}")
    for r in range(R):
        if not 0 <= rows[r] < A or not 0 <= seeks[r] < cfs[rows[r]]:
            raise ValueError(f"mel_windows: row {r} reads recording {rows[r]} at frame {seeks[r]}: outside the {A} recordings or their content frames")
    dev = mel.device
    if out is None:
        out = torch.empty((R, n_mels, n_win), dtype=F32, device=dev)
    _chk(out, F32, "out")
    if tuple(out.shape) != (R, n_mels, n_win) or not out.is_contiguous():
        raise ValueError(f"mel_windows: out must be a contiguous f32 [{R}, {n_mels}, {n_win}]")
    rs = upload_table(rows + seeks, torch.int32, dev)
    L.check(L.load().wft_mel_windows(_p(mel), _p(mel_off), _p(ld_frames), _p(content_frames), _p(rs[:R]), _p(rs[R:]), _p(out), R, A, n_mels, n_win,
                                     L.stream_ptr()), "wft_mel_windows")
    return out


# --------------------------------------------------------------------------- embedding / CE
def embed_fwd(tokens, emb, pos):
    _chk(tokens, torch.int64, "tokens"); _chk(emb, F32, "emb"); _chk(pos, F32, "pos")
    tokens = tokens.contiguous()
    B, S = tokens.shape
    V, d = emb.shape
    out = torch.empty((B, S, d), dtype=BF16, device=emb.device)
    L.check(L.load().wft_embed_fwd(_p(tokens), _p(emb), _p(pos), _p(out), B, S, d, V, L.stream_ptr()), "wft_embed_fwd")
    return out


def embed_bwd(tokens, dout, demb, dpos):
    """accumulates into demb f32 [V,d] and dpos f32 [n_ctx,d]."""
    _chk(dout, BF16, "dout")
    tokens = tokens.contiguous(); dout = dout.contiguous()
    B, S = tokens.shape
    V, d = demb.shape
    L.check(L.load().wft_embed_bwd(_p(tokens), _p(dout), _p(demb), _p(dpos), B, S, d, V, L.stream_ptr()), "wft_embed_bwd")


def ce_fwd(logits, targets, V: int, label_smoothing: float, want_argmax: bool = False):
    """logits bf16 [rows, ld>=V]; targets i64 [rows] -> (row_loss, row_lse, stats[2], argmax|None)."""
    _chk(logits, BF16, "logits"); _chk(targets, torch.int64, "targets")
    assert logits.dim() == 2 and logits.stride(1) == 1
    rows, ld = logits.shape[0], logits.stride(0)
    targets = targets.contiguous()
    dev = logits.device
    row_loss = torch.empty(rows, dtype=F32, device=dev)
    row_lse = torch.empty(rows, dtype=F32, device=dev)
    stats = torch.empty(2, dtype=F32, device=dev)
    am = torch.empty(rows, dtype=torch.int64, device=dev) if want_argmax else None
    L.check(
        L.load().wft_ce_fwd(_p(logits), ld, _p(targets), rows, V, label_smoothing, _p(row_loss), _p(row_lse), _p(stats),
                            _p(am), L.stream_ptr()),
        "wft_ce_fwd",
    )
    return row_loss, row_lse, stats, am


def ce_bwd(logits, targets, V: int, label_smoothing: float, row_lse, stats, gscale, inplace=True):
    rows, ld = logits.shape[0], logits.stride(0)
    dl = logits if inplace else torch.empty_like(logits)
    gscale = gscale.reshape(1).to(F32)
    L.check(
        L.load().wft_ce_bwd(_p(logits), ld, _p(targets.contiguous()), rows, V, label_smoothing, _p(row_lse), _p(stats),
                            _p(gscale), _p(dl), L.stream_ptr()),
        "wft_ce_bwd",
    )
    return dl


def token_stats(logits, targets, V: int):
    """logits bf16 [rows, ld>=V]; targets i64 [rows] or None -> (stats f32 [rows, 4] = lse, max, E_p[x], x_target; argmax i64)."""
    _chk(logits, BF16, "logits")
    assert logits.dim() == 2 and logits.stride(1) == 1
    rows, ld = logits.shape[0], logits.stride(0)
    out4 = torch.empty((rows, 4), dtype=F32, device=logits.device)
    am = torch.empty(rows, dtype=torch.int64, device=logits.device)
    tg = None if targets is None else targets.contiguous()
    L.check(L.load().wft_token_stats(_p(logits), ld, _p(tg), rows, V, _p(out4), _p(am), L.stream_ptr()), "wft_token_stats")
    return out4, am


# --------------------------------------------------------------------------- audio
def logmel(audio, filters, n_frames: int = 3000):
    """audio f32 [B, 160*n_frames], filters f32 [n_mels, 201] -> f32 [B, n_mels, n_frames]."""
    _chk(audio, F32, "audio"); _chk(filters, F32, "filters")
    audio = audio.contiguous(); filters = filters.contiguous()
    B, n = audio.shape
    n_mels = filters.shape[0]
    out = torch.empty((B, n_mels, n_frames), dtype=F32, device=audio.device)
    clipmax = torch.empty(B, dtype=F32, device=audio.device)
    L.check(L.load().wft_logmel(_p(audio), _p(filters), _p(out), _p(clipmax), B, n, n_mels, n_frames, L.stream_ptr()), "wft_logmel")
    return out


def specaug(mel, params, extremes=None):
    """mel f32 [B, n_mels, T]; params i32 [B, 8]; extremes i32 [B, 2] or None."""
    _chk(mel, F32, "mel"); _chk(params, torch.int32, "params")
    mel = mel.contiguous(); params = params.contiguous()
    B, n_mels, T = mel.shape
    out = torch.empty_like(mel)
    if extremes is not None:
        _chk(extremes, torch.int32, "extremes")
        extremes = extremes.contiguous()
    L.check(L.load().wft_specaug(_p(mel), _p(out), _p(params), _p(extremes), B, n_mels, T, L.stream_ptr()), "wft_specaug")
    return out


_RESAMPLE_TAPS = {}  # (o, n, device) -> the f32 [n, 2 * width] table on the device


def resample(audio, orig: int, new: int, *, out=None):
    """Sample-rate conversion orig -> new (wft_resample_f32: the polyphase form of torchaudio's default sinc_interp_hann resampler).

    audio f32 [B, n_in] on the device, rows of any stride (stride(1) == 1; what lies behind n_in in a row is never read) ->
    f32 [B, n_out], n_out = ceil(n_in * new / orig).  orig / new: positive ints, reduced here by their gcd; orig == new returns
    `audio` unchanged.  `out`: f32 [B, n_out] with stride(1) == 1 to write into (what lies behind n_out in a row is never written).
    Every argument is checked before the launch."""
    _chk(audio, F32, "audio")
    for name, v in (("orig", orig), ("new", new)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"resample: {name} must be a positive integer, got {v!r}")
    if audio.dim() != 2 or audio.shape[0] < 1 or audio.shape[1] < 1:
        raise ValueError(f"resample: audio must be [B, n_in] with B >= 1 and n_in >= 1, got {tuple(audio.shape)}")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    if o == n:
        return audio
    if audio.stride(1) != 1 or (audio.shape[0] > 1 and audio.stride(0) < audio.shape[1]):
        audio = audio.contiguous()
    B, n_in = audio.shape
    if B > 65535:
        raise ValueError(f"resample: at most 65535 rows per call, got {B}")
    n_out = -(-n_in * n // o)
    from ..data.gpu_frontend import resample_taps

    taps, _, _, width = resample_taps(o, n)
    if L.load().wft_resample_tile(o, n, width) < 4:
        raise ValueError(f"resample: the rate pair {orig} -> {new} ({2 * width} taps per output) is not supported by wft_resample_f32")
    key = (o, n, audio.device)
    if key not in _RESAMPLE_TAPS:
        _RESAMPLE_TAPS[key] = taps.to(audio.device)
    if out is None:
        out = torch.empty((B, n_out), dtype=F32, device=audio.device)
    _chk(out, F32, "out")
    if tuple(out.shape) != (B, n_out) or out.stride(1) != 1 or (B > 1 and out.stride(0) < n_out) or out.device != audio.device:
        raise ValueError(f"resample: out must be f32 [{B}, {n_out}] on {audio.device} with unit column stride and rows that do not overlap")
    ld_in = audio.stride(0) if B > 1 else max(audio.stride(0), n_in)
    ld_out = out.stride(0) if B > 1 else max(out.stride(0), n_out)
    L.check(L.load().wft_resample_f32(_p(audio), ld_in, n_in, _p(_RESAMPLE_TAPS[key]), o, n, width, _p(out), ld_out, n_out, B, L.stream_ptr()),
            "wft_resample_f32")
    return out


STRETCH_MIN_RATE, STRETCH_MAX_RATE = 0.5, 2.0
STRETCH_WORKSPACE_CAP = 1 << 30  # bytes per launch: rows are processed in chunks above it (30 s at rate 0.5: 23 MB per row)


def stretch_rates(rates, B: int):
    """One rate or one per row (numbers, a list, an array or a HOST tensor) -> float64 numpy [B]; a rate outside [0.5, 2.0]
    (or NaN) raises ValueError."""
    import numpy as np

    r = rates.detach().cpu().numpy() if torch.is_tensor(rates) else np.asarray(rates)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    if r.shape[0] == 1 and B > 1:
        r = np.repeat(r, B)
    if r.shape[0] != B:
        raise ValueError(f"time_stretch: {r.shape[0]} rates for {B} rows")
    if not bool(np.all((r >= STRETCH_MIN_RATE) & (r <= STRETCH_MAX_RATE))):
        raise ValueError(f"time_stretch: rates must lie in [{STRETCH_MIN_RATE}, {STRETCH_MAX_RATE}], got {r.tolist()}")
    return r


def time_stretch(audio, rates):
    """Phase-vocoder time stretch (wft_time_stretch_f32, include/wft.h "Time stretch").

    audio f32 [B, n] on the device (stride(1) == 1); rates: one float64 rate or one per row, HOST values inside [0.5, 2.0]
    (ValueError otherwise: they size the launch, so they are checked here and not on the device).
    -> (out f32 [B, cap], n_out i32 [B] on the device): row b holds n_out[b] = round(n / rates[b]) samples followed by zeros up to
    cap = round(n / min(rates)).  A row's bits depend on its samples, its rate and n only.  Rows go through the kernels in chunks
    so that the workspace of one launch stays below STRETCH_WORKSPACE_CAP."""
    _chk(audio, F32, "audio")
    if audio.dim() != 2 or audio.shape[0] < 1 or audio.shape[1] < 1:
        raise ValueError(f"time_stretch: audio must be [B, n] with B >= 1 and n >= 1, got {tuple(audio.shape)}")
    if audio.stride(1) != 1 or (audio.shape[0] > 1 and audio.stride(0) < audio.shape[1]):
        audio = audio.contiguous()
    B, n = audio.shape
    r = stretch_rates(rates, B)
    rate_lo = float(r.min())
    lib = L.load()
    per_row = lib.wft_time_stretch_workspace_bytes(1, n, rate_lo)
    if per_row < 0:
        raise ValueError(f"time_stretch: rows of {n} samples are not supported by wft_time_stretch_f32")
    cap = int(round(n / rate_lo))
    out = torch.zeros((B, max(cap, 1)), dtype=F32, device=audio.device)
    n_out = torch.empty(B, dtype=torch.int32, device=audio.device)
    rates_d = torch.from_numpy(r).to(audio.device)
    chunk = max(1, min(B, STRETCH_WORKSPACE_CAP // per_row))
    ws = torch.empty(chunk * per_row, dtype=torch.uint8, device=audio.device)
    ld_in = audio.stride(0) if B > 1 else max(audio.stride(0), n)
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        L.check(lib.wft_time_stretch_f32(_p(audio[b0:]), ld_in, n, _p(rates_d[b0:]), rate_lo, _p(out[b0:]), out.stride(0), _p(n_out[b0:]),
                                         _p(ws), nb * per_row, nb, L.stream_ptr()), "wft_time_stretch_f32")
    return out, n_out


def logmel_ragged(audio, n_samples, keep_frames, filters, T_out: int = 3000):
    """Log-mel of rows of different lengths (wft_logmel_ragged): audio f32 [B, ld] on the device, n_samples / keep_frames i32 [B]
    on the device (row b: n_samples[b] <= ld samples, n_samples[b] // 160 frames, the first min(keep_frames[b], frames, T_out)
    columns kept and the rest filled with their minimum), filters f32 [n_mels, 201] -> f32 [B, n_mels, T_out]."""
    _chk(audio, F32, "audio"); _chk(filters, F32, "filters")
    _chk(n_samples, torch.int32, "n_samples"); _chk(keep_frames, torch.int32, "keep_frames")
    audio = audio.contiguous(); filters = filters.contiguous()
    n_samples = n_samples.contiguous(); keep_frames = keep_frames.contiguous()
    B, ld = audio.shape
    if n_samples.shape != (B,) or keep_frames.shape != (B,):
        raise ValueError(f"logmel_ragged: n_samples and keep_frames must be [{B}], got {tuple(n_samples.shape)}, {tuple(keep_frames.shape)}")
    n_mels = filters.shape[0]
    out = torch.empty((B, n_mels, T_out), dtype=F32, device=audio.device)
    stats = torch.empty(2 * B, dtype=F32, device=audio.device)
    L.check(L.load().wft_logmel_ragged(_p(audio), ld, _p(n_samples), _p(keep_frames), _p(filters), _p(out), _p(stats), B, ld, n_mels,
                                       T_out, L.stream_ptr()), "wft_logmel_ragged")
    return out


SOS_MAX_SECTIONS = 4


def sos_coefficients(sos, B: int):
    """sos f64 [B, S, 6] or [S, 6] (one filter for every row), a host or a device tensor or an array -> float64 numpy [B, S, 6].
    ValueError: a shape other than these, S outside 1..4, a coefficient that is not finite, a0 != 1.  A device tensor is copied to
    the host for the check (it is B * S * 6 doubles)."""
    import numpy as np

    c = sos.detach().cpu().numpy() if torch.is_tensor(sos) else np.asarray(sos)
    if c.dtype != np.float64:
        raise ValueError(f"sos_filter: sos must be float64, got {c.dtype}")
    if c.ndim == 2:
        c = np.broadcast_to(c[None], (B,) + c.shape)
    if c.ndim != 3 or c.shape[0] != B or c.shape[2] != 6:
        raise ValueError(f"sos_filter: sos must be [{B}, S, 6] or [S, 6], got {tuple(c.shape)}")
    if not 1 <= c.shape[1] <= SOS_MAX_SECTIONS:
        raise ValueError(f"sos_filter: 1 to {SOS_MAX_SECTIONS} sections, got {c.shape[1]}")
    if not bool(np.all(np.isfinite(c))):
        raise ValueError("sos_filter: coefficients must be finite")
    if not bool(np.all(c[:, :, 3] == 1.0)):
        raise ValueError("sos_filter: every section must be normalised to a0 == 1")
    return np.array(c, dtype=np.float64, order="C", copy=True)  # (a broadcast view is read-only)


def sos_filter(audio, sos, n=None, *, out=None):
    """A cascade of second-order sections over every row (wft_sos_filter_f32, include/wft.h "IIR filter").

    audio f32 [B, ld] on the device (stride(1) == 1); sos f64 [B, S, 6] or [S, 6] = b0 b1 b2 a0 a1 a2 with a0 == 1, S in 1..4, on the
    host or the device; n i32 [B] on the device (row b filters its first n[b] samples, clamped to [0, ld], and is zero behind them) or
    None (every row filters all ld samples).  out: None (a new tensor), `audio` itself (in place) or an f32 [B, ld] tensor with unit
    column stride that does not overlap `audio`.  Every host-side check raises ValueError before the device is touched."""
    if not torch.is_tensor(audio) or audio.dtype != F32 or audio.dim() != 2 or audio.shape[0] < 1 or audio.shape[1] < 1:
        raise ValueError(f"sos_filter: audio must be a float32 tensor [B, n] with B >= 1 and n >= 1, got {getattr(audio, 'dtype', type(audio))} "
                         f"{tuple(getattr(audio, 'shape', ()))}")
    B, n_max = audio.shape
    if B > 65535 or n_max > (1 << 30):
        raise ValueError(f"sos_filter: at most 65535 rows of 2^30 samples per call, got {tuple(audio.shape)}")
    c = sos_coefficients(sos, B)
    S = c.shape[1]
    if n is not None:
        if not torch.is_tensor(n) or n.dtype != torch.int32 or tuple(n.shape) != (B,):
            raise ValueError(f"sos_filter: n must be an int32 tensor [{B}] or None")
    if audio.stride(1) != 1 or (B > 1 and audio.stride(0) < n_max):
        if out is audio:
            raise ValueError("sos_filter: an in-place call needs rows with unit column stride that do not overlap")
        audio = audio.contiguous()
    if out is not None and out is not audio:
        if not torch.is_tensor(out) or out.dtype != F32 or tuple(out.shape) != (B, n_max) or out.stride(1) != 1 or (B > 1 and out.stride(0) < n_max):
            raise ValueError(f"sos_filter: out must be f32 [{B}, {n_max}] with unit column stride and rows that do not overlap")
    _chk(audio, F32, "audio")  # (every ValueError above comes before the device is touched)
    if out is None:
        out = torch.empty((B, n_max), dtype=F32, device=audio.device)
    if out.device != audio.device or (n is not None and n.device != audio.device):
        raise ValueError("sos_filter: audio, out and n must live on the same GPU")
    lib = L.load()
    nbytes = lib.wft_sos_filter_workspace_bytes(B, n_max, S)
    if nbytes < 0:
        raise ValueError(f"sos_filter: {B} rows of {n_max} samples with {S} sections are not supported by wft_sos_filter_f32")
    sos_d = sos.contiguous() if (torch.is_tensor(sos) and sos.is_cuda and sos.dim() == 3 and sos.device == audio.device) else \
        torch.from_numpy(c).to(audio.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=audio.device)
    if n is not None:
        n = n.contiguous()
    ld_in = audio.stride(0) if B > 1 else max(audio.stride(0), n_max)
    ld_out = out.stride(0) if B > 1 else max(out.stride(0), n_max)
    L.check(lib.wft_sos_filter_f32(_p(audio), ld_in, _p(n), n_max, _p(sos_d), S, _p(out), ld_out, _p(ws), nbytes, B, L.stream_ptr()),
            "wft_sos_filter_f32")
    return out


def wave_fx_records(fx, B: int):
    """fx -> checked host records [B] (data/wave_fx.py RECORD_DTYPE).  fx: a numpy structured array [B] of that dtype, or the table
    f64 [B, 14] / [14] (one record for every row) as a host tensor or array.  Every refusal is a ValueError."""
    import numpy as np

    from whisper_finetune.data import wave_fx as WF

    a = fx.detach().cpu().numpy() if torch.is_tensor(fx) else np.asarray(fx)
    if a.dtype != WF.RECORD_DTYPE:
        if a.ndim == 1:
            a = np.broadcast_to(a[None], (B,) + a.shape)
        a = WF.records_from_table(np.ascontiguousarray(a))
    if a.shape != (B,):
        raise ValueError(f"wave_fx: {B} rows need {B} records, got {tuple(a.shape)}")
    return WF.check_records(np.ascontiguousarray(a))


def wave_fx(audio, fx, stage, n=None, *, out=None):
    """One stage of the wave effects over every row (wft_wave_fx_f32, include/wft.h "Wave effects").

    audio f32 [B, ld] on the device (stride(1) == 1); fx: the rows' records on the HOST (wave_fx_records states the forms); stage:
    "noise", "clip" or "level" (or L.FX_NOISE / FX_CLIP / FX_LEVEL); n i32 [B] on the device (row b covers its first n[b] samples,
    clamped to [0, ld]; out of place the output is zero behind them) or None (every row covers all ld samples).  out: None (a new
    tensor), `audio` itself (in place) or an f32 [B, ld] tensor with unit column stride that does not overlap `audio`.
    When no row is active in the stage nothing is launched: in place `audio` is returned as it is, out of place the rows are copied
    and zeroed behind n by torch.  A `shift` is a rotation and cannot be done in place: an in-place LEVEL call with shift rows runs
    into a temporary of the batch's size, which is then copied back (one extra read and write of the batch).
    Every host-side check raises ValueError before the device is touched."""
    from whisper_finetune.data import wave_fx as WF

    if not torch.is_tensor(audio) or audio.dtype != F32 or audio.dim() != 2 or audio.shape[0] < 1 or audio.shape[1] < 1:
        raise ValueError(f"wave_fx: audio must be a float32 tensor [B, n] with B >= 1 and n >= 1, got {getattr(audio, 'dtype', type(audio))} "
                         f"{tuple(getattr(audio, 'shape', ()))}")
    B, n_max = audio.shape
    if B > 65535 or n_max > (1 << 30):
        raise ValueError(f"wave_fx: at most 65535 rows of 2^30 samples per call, got {tuple(audio.shape)}")
    if isinstance(stage, str):
        if stage not in WF.STAGE_ID:
            raise ValueError(f"wave_fx: stage must be one of {WF.STAGES}, got {stage!r}")
        stage = WF.STAGE_ID[stage]
    if stage not in (L.FX_NOISE, L.FX_CLIP, L.FX_LEVEL):
        raise ValueError(f"wave_fx: unknown stage {stage!r}")
    rec = wave_fx_records(fx, B)
    if n is not None:
        if not torch.is_tensor(n) or n.dtype != torch.int32 or tuple(n.shape) != (B,):
            raise ValueError(f"wave_fx: n must be an int32 tensor [{B}] or None")
    if audio.stride(1) != 1 or (B > 1 and audio.stride(0) < n_max):
        if out is audio:
            raise ValueError("wave_fx: an in-place call needs rows with unit column stride that do not overlap")
        audio = audio.contiguous()
    if out is not None and out is not audio:
        if not torch.is_tensor(out) or out.dtype != F32 or tuple(out.shape) != (B, n_max) or out.stride(1) != 1 or (B > 1 and out.stride(0) < n_max):
            raise ValueError(f"wave_fx: out must be f32 [{B}, {n_max}] with unit column stride and rows that do not overlap")
    _chk(audio, F32, "audio")  # (every ValueError above comes before the device is touched)
    if (out is not None and out.device != audio.device) or (n is not None and n.device != audio.device):
        raise ValueError("wave_fx: audio, out and n must live on the same GPU")
    stage_name = WF.STAGES[stage]
    if not bool(WF.active_rows(rec, stage_name).any()):  # nothing to launch
        if out is audio:
            return audio
        if out is None:
            out = torch.empty((B, n_max), dtype=F32, device=audio.device)
        out.copy_(audio)
        if n is not None:
            out.masked_fill_(torch.arange(n_max, device=audio.device)[None] >= n.clamp(0, n_max)[:, None], 0.0)
        return out
    through_tmp = out is audio and stage == L.FX_LEVEL and bool((rec["level_kind"] == L.FX_SHIFT).any())
    dst = torch.empty((B, n_max), dtype=F32, device=audio.device) if (out is None or through_tmp) else out
    lib = L.load()
    nbytes = lib.wft_wave_fx_workspace_bytes(B, n_max, stage)
    if nbytes < 0:
        raise ValueError(f"wave_fx: {B} rows of {n_max} samples are not supported by wft_wave_fx_f32")
    fx_d = torch.from_numpy(rec.view("u1").reshape(B, WF.RECORD_DTYPE.itemsize).copy()).to(audio.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=audio.device)
    if n is not None:
        n = n.contiguous()
    ld_in = audio.stride(0) if B > 1 else max(audio.stride(0), n_max)
    ld_out = dst.stride(0) if B > 1 else max(dst.stride(0), n_max)
    L.check(lib.wft_wave_fx_f32(_p(audio), ld_in, _p(n), n_max, _p(fx_d), stage, _p(dst), ld_out, _p(ws), nbytes, B, L.stream_ptr()),
            "wft_wave_fx_f32")
    if through_tmp:
        if n is None:
            audio.copy_(dst)
        else:  # in place nothing behind n[b] is touched
            torch.where(torch.arange(n_max, device=audio.device)[None] < n.clamp(0, n_max)[:, None], dst, audio, out=audio)
        return audio
    return dst


def _row_values(values, B: int, who: str, what: str):
    """One value or one per row (numbers, a list, an array or a HOST tensor) -> float64 numpy [B]."""
    import numpy as np

    v = values.detach().cpu().numpy() if torch.is_tensor(values) else np.asarray(values)
    if v.dtype == object or v.dtype.kind not in "fiu":
        raise ValueError(f"{who}: {what} must be numbers, got {v.dtype}")
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.shape[0] == 1 and B > 1:
        v = np.repeat(v, B)
    if v.shape[0] != B:
        raise ValueError(f"{who}: {v.shape[0]} {what} for {B} rows")
    return np.ascontiguousarray(v)


def _rate_rows(audio, who: str):
    """The shared host-side checks of the per-row rate kernels on their input (ValueError); returns it unchanged."""
    if not torch.is_tensor(audio) or audio.dtype != F32 or audio.dim() != 2 or audio.shape[0] < 1 or audio.shape[1] < 1:
        raise ValueError(f"{who}: audio must be a float32 tensor [B, n] with B >= 1 and n >= 1, got {getattr(audio, 'dtype', type(audio))} "
                         f"{tuple(getattr(audio, 'shape', ()))}")
    if audio.shape[0] > 65535 or audio.shape[1] > (1 << 30):
        raise ValueError(f"{who}: at most 65535 rows of 2^30 samples per call, got {tuple(audio.shape)}")
    return audio


def sinc_resample_rows(audio, n_in, ratios, n_out: int):
    """Resampling by a float64 ratio of its own for every row (wft_sinc_resample_rows_f32, include/wft.h "Per-row rate conversion").

    audio f32 [B, ld] on the device (stride(1) == 1); n_in i32 [B] on the device: row b holds n_in[b] samples (clamped to [0, ld]);
    ratios: one ratio (output rate / input rate) or one per row, HOST values inside [0.5, 2.0] (ValueError otherwise: their minimum
    sizes the launch, so they are checked here and not on the device); n_out: the length of every output row.
    -> f32 [B, n_out]: row b holds min(n_out, ceil(n_in[b] * ratio[b])) resampled samples and zeros behind them.
    Every host-side check raises ValueError before the device is touched."""
    import numpy as np

    audio = _rate_rows(audio, "sinc_resample_rows")
    B, ld = audio.shape
    if isinstance(n_out, bool) or not isinstance(n_out, int) or not 1 <= n_out <= (1 << 30):
        raise ValueError(f"sinc_resample_rows: n_out must be an integer inside [1, 2^30], got {n_out!r}")
    if not torch.is_tensor(n_in) or n_in.dtype != torch.int32 or tuple(n_in.shape) != (B,):
        raise ValueError(f"sinc_resample_rows: n_in must be an int32 tensor [{B}]")
    r = _row_values(ratios, B, "sinc_resample_rows", "ratios")
    if not bool(np.all((r >= STRETCH_MIN_RATE) & (r <= STRETCH_MAX_RATE))):
        raise ValueError(f"sinc_resample_rows: ratios must lie in [{STRETCH_MIN_RATE}, {STRETCH_MAX_RATE}], got {r.tolist()}")
    _chk(audio, F32, "audio")  # (every ValueError above comes before the device is touched)
    if n_in.device != audio.device:
        raise ValueError("sinc_resample_rows: audio and n_in must live on the same GPU")
    if audio.stride(1) != 1 or (B > 1 and audio.stride(0) < ld):
        audio = audio.contiguous()
    ratio_lo = float(r.min())
    lib = L.load()
    if lib.wft_sinc_resample_rows_tile(ratio_lo) < 4:
        raise ValueError(f"sinc_resample_rows: a lowest ratio of {ratio_lo} is not supported by wft_sinc_resample_rows_f32")
    out = torch.empty((B, n_out), dtype=F32, device=audio.device)
    ratio_d = torch.from_numpy(r).to(audio.device)
    ld_in = audio.stride(0) if B > 1 else max(audio.stride(0), ld)
    L.check(lib.wft_sinc_resample_rows_f32(_p(audio), ld_in, _p(n_in.contiguous()), ld, _p(ratio_d), ratio_lo, _p(out), out.stride(0),
                                           n_out, B, L.stream_ptr()), "wft_sinc_resample_rows_f32")
    return out


def alias_rates(new_rates, B: int, sample_rate):
    """One new rate or one per row -> float64 numpy [B]; a rate is 0 ("none": the row is copied) or lies inside
    [1000, 2 * sample_rate], anything else (NaN included) raises ValueError."""
    import numpy as np

    from whisper_finetune.data.rate_fx import ALIAS_MIN_RATE

    r = _row_values(new_rates, B, "alias", "rates")
    if not bool(np.all((r == 0.0) | ((r >= ALIAS_MIN_RATE) & (r <= 2.0 * sample_rate)))):
        raise ValueError(f"alias: a new rate must be 0 (none) or lie in [{ALIAS_MIN_RATE}, {2.0 * sample_rate}], got {r.tolist()}")
    return r


def alias(audio, new_rates, n=None, sample_rate=16000):
    """audiomentations' Aliasing over every row: linear interpolation down to `new_rate` and back without a low-pass
    (wft_alias_f32, include/wft.h "Per-row rate conversion"; numpy's float64 result rounded once, bit for bit).

    audio f32 [B, ld] on the device (stride(1) == 1); new_rates: one rate in Hz or one per row, HOST values, 0 = "none" (the row is
    copied) or inside [1000, 2 * sample_rate]; n i32 [B] on the device (row b covers its first n[b] samples, clamped to [0, ld]; the
    output is zero behind them) or None (every row covers all ld samples); sample_rate: the clips' rate, a positive number.
    -> a new f32 [B, ld] tensor (the kernel does not run in place).  Every host-side check raises ValueError before the device is
    touched."""
    audio = _rate_rows(audio, "alias")
    B, n_max = audio.shape
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, float)) or not 1000 <= sample_rate <= 384000:
        raise ValueError(f"alias: sample_rate must be a number inside [1000, 384000], got {sample_rate!r}")
    r = alias_rates(new_rates, B, float(sample_rate))
    if n is not None:
        if not torch.is_tensor(n) or n.dtype != torch.int32 or tuple(n.shape) != (B,):
            raise ValueError(f"alias: n must be an int32 tensor [{B}] or None")
    _chk(audio, F32, "audio")  # (every ValueError above comes before the device is touched)
    if n is not None and n.device != audio.device:
        raise ValueError("alias: audio and n must live on the same GPU")
    if audio.stride(1) != 1 or (B > 1 and audio.stride(0) < n_max):
        audio = audio.contiguous()
    out = torch.empty((B, n_max), dtype=F32, device=audio.device)
    rate_d = torch.from_numpy(r).to(audio.device)
    if n is not None:
        n = n.contiguous()
    ld_in = audio.stride(0) if B > 1 else max(audio.stride(0), n_max)
    L.check(L.load().wft_alias_f32(_p(audio), ld_in, _p(n), n_max, _p(rate_d), float(sample_rate), _p(out), out.stride(0), B,
                                   L.stream_ptr()), "wft_alias_f32")
    return out


FIR_TAPS_MAX = 8192  # wft_fir_conv_f32's limit on taps_max


def _lengths(n, B: int, device, who: str, what: str):
    """None, or an int32 tensor [B] on `device` -> the same, contiguous (ValueError otherwise)."""
    if n is None:
        return None
    if not torch.is_tensor(n) or n.dtype != torch.int32 or tuple(n.shape) != (B,):
        raise ValueError(f"{who}: {what} must be an int32 tensor [{B}] or None")
    if n.device != device:
        raise ValueError(f"{who}: audio and {what} must live on the same GPU")
    return n.contiguous()


def fir_conv(audio, ir, n=None, n_taps=None):
    """A causal FIR over every row, each row with an impulse response of its own (wft_fir_conv_f32, include/wft.h "Office effects":
    FFT overlap-save in f32; the tail is chopped at the row's length).

    audio f32 [B, ld] on the device (stride(1) == 1); ir f32 [B, taps_max] or [taps_max] (one response for every row) on the same
    device, 1 <= taps_max <= 8192; n i32 [B] on the device (row b covers its first n[b] samples, clamped to [0, ld]; the output is zero
    behind them) or None (all ld samples); n_taps i32 [B] on the device (row b uses its first n_taps[b] taps, clamped to
    [0, taps_max]; 0 = the row is copied) or None (all taps_max).
    -> a new f32 [B, ld] tensor (the kernel cannot run in place).  Every host-side check raises ValueError before the device is
    touched."""
    audio = _rate_rows(audio, "fir_conv")
    B, n_max = audio.shape
    if not torch.is_tensor(ir) or ir.dtype != F32 or ir.dim() not in (1, 2) or ir.shape[-1] < 1 or ir.shape[-1] > FIR_TAPS_MAX or \
            (ir.dim() == 2 and ir.shape[0] != B):
        raise ValueError(f"fir_conv: ir must be a float32 tensor [{B}, taps] or [taps] with 1 <= taps <= {FIR_TAPS_MAX}, got "
                         f"{getattr(ir, 'dtype', type(ir))} {tuple(getattr(ir, 'shape', ()))}")
    taps_max = int(ir.shape[-1])
    _chk(audio, F32, "audio")  # (every ValueError above comes before the device is touched)
    if ir.device != audio.device:
        raise ValueError("fir_conv: audio and ir must live on the same GPU")
    n = _lengths(n, B, audio.device, "fir_conv", "n")
    n_taps = _lengths(n_taps, B, audio.device, "fir_conv", "n_taps")
    if ir.dim() == 1:
        ir = ir[None].expand(B, taps_max)
    if ir.stride(1) != 1 or (B > 1 and ir.stride(0) < taps_max):
        ir = ir.contiguous()
    if audio.stride(1) != 1 or (B > 1 and audio.stride(0) < n_max):
        audio = audio.contiguous()
    lib = L.load()
    nbytes = lib.wft_fir_conv_workspace_bytes(B, taps_max)
    out = torch.empty((B, n_max), dtype=F32, device=audio.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=audio.device)
    ld_in = audio.stride(0) if B > 1 else max(audio.stride(0), n_max)
    ld_ir = ir.stride(0) if B > 1 else max(ir.stride(0), taps_max)
    L.check(lib.wft_fir_conv_f32(_p(audio), ld_in, _p(n), n_max, _p(ir), ld_ir, _p(n_taps), taps_max, _p(out), out.stride(0), _p(ws),
                                 nbytes, B, L.stream_ptr()), "wft_fir_conv_f32")
    return out


def bitcrush_depths(bits, B: int):
    """One bit depth or one per row (host integers) -> int32 numpy [B]; a depth is 0 ("none": the row is copied) or lies inside
    [1, 24], anything else raises ValueError."""
    import numpy as np

    v = _row_values(bits, B, "bitcrush", "bit depths")
    if not bool(np.all((v == np.rint(v)) & (v >= 0) & (v <= 24))):  # (NaN fails)
        raise ValueError(f"bitcrush: a bit depth must be an integer inside [1, 24], or 0 (none), got {v.tolist()}")
    return v.astype(np.int32)


def bitcrush(audio, bits, n=None, *, out=None):
    """audiomentations' BitCrush over every row: round(x * q) / q with q = 2^(bits - 1) + 1 in f32 (wft_bitcrush_f32, include/wft.h
    "Office effects"; numpy's np.round(samples * q) / q bit for bit).

    audio f32 [B, ld] on the device (stride(1) == 1); bits: one depth or one per row as HOST integers inside [1, 24], 0 = "none" (the
    row is copied), or an int32 tensor [B] on the device (unchecked: the kernel copies a row whose depth lies outside [1, 24]);
    n i32 [B] on the device (row b covers its first n[b] samples; the output is zero behind them) or None.  out: None (a new
    tensor), `audio` itself (in place) or an f32 [B, ld] tensor with unit column stride that does not overlap `audio`.  Every
    host-side check raises ValueError before the device is touched."""
    audio = _rate_rows(audio, "bitcrush")
    B, n_max = audio.shape
    on_device = torch.is_tensor(bits) and bits.is_cuda
    if on_device:
        if bits.dtype != torch.int32 or tuple(bits.shape) != (B,):
            raise ValueError(f"bitcrush: device-side bits must be an int32 tensor [{B}]")
    else:
        depths = bitcrush_depths(bits, B)
    if audio.stride(1) != 1 or (B > 1 and audio.stride(0) < n_max):
        if out is audio:
            raise ValueError("bitcrush: an in-place call needs rows with unit column stride that do not overlap")
        audio = audio.contiguous()
    if out is not None and out is not audio:
        if not torch.is_tensor(out) or out.dtype != F32 or tuple(out.shape) != (B, n_max) or out.stride(1) != 1 or (B > 1 and out.stride(0) < n_max):
            raise ValueError(f"bitcrush: out must be f32 [{B}, {n_max}] with unit column stride and rows that do not overlap")
    _chk(audio, F32, "audio")  # (every ValueError above comes before the device is touched)
    if out is None:
        out = torch.empty((B, n_max), dtype=F32, device=audio.device)
    if out.device != audio.device:
        raise ValueError("bitcrush: audio and out must live on the same GPU")
    n = _lengths(n, B, audio.device, "bitcrush", "n")
    bits_d = bits.contiguous() if on_device else torch.from_numpy(depths).to(audio.device)
    if bits_d.device != audio.device:
        raise ValueError("bitcrush: audio and bits must live on the same GPU")
    ld_in = audio.stride(0) if B > 1 else max(audio.stride(0), n_max)
    ld_out = out.stride(0) if B > 1 else max(out.stride(0), n_max)
    L.check(L.load().wft_bitcrush_f32(_p(audio), ld_in, _p(n), n_max, _p(bits_d), _p(out), ld_out, B, L.stream_ptr()), "wft_bitcrush_f32")
    return out


def _mix_rows(audio, out, who: str):
    """The shared checks of loudness / bg_mix on audio and out -> audio with usable strides (ValueError before the device is touched)."""
    audio = _rate_rows(audio, who)
    B, n_max = audio.shape
    if audio.stride(1) != 1 or (B > 1 and audio.stride(0) < n_max):
        if out is audio:
            raise ValueError(f"{who}: an in-place call needs rows with unit column stride that do not overlap")
        audio = audio.contiguous()
    if out is not None and out is not audio:
        if not torch.is_tensor(out) or out.dtype != F32 or tuple(out.shape) != (B, n_max) or out.stride(1) != 1 or (B > 1 and out.stride(0) < n_max):
            raise ValueError(f"{who}: out must be f32 [{B}, {n_max}] with unit column stride and rows that do not overlap")
    return audio


def loudness(audio, sample_rate: int = 16000, target=None, n=None, *, out=None):
    """The ITU-R BS.1770 integrated loudness of every row and, with a target, the gain that brings the row to it
    (wft_loudness_f32, include/wft.h "Loudness and background noise": pyloudnorm's meter and normalize.loudness, restated).

    audio f32 [B, ld] on the device (stride(1) == 1); sample_rate: an integer multiple of 10 inside [8000, 384000]; target: None
    (measure only), or one value in LUFS or one per row as HOST numbers, NaN = "leave the row as it is" (not measured either);
    n i32 [B] on the device (row b covers its first n[b] samples) or None.  out: None (a new tensor), `audio` itself (in place) or an
    f32 [B, ld] tensor that does not overlap `audio` (ignored without a target).
    -> (out or None, stats f64 [B, 4] on the device = LUFS, relative gate, blocks over both gates, gain).  A row without a block
    over both gates, or shorter than 400 ms, reads -inf and is copied.  When no row has a target and an output is wanted nothing is
    launched.  Every host-side check raises ValueError before the device is touched."""
    import numpy as np

    from whisper_finetune.data import mix_fx as MF

    measure = target is None
    audio = _mix_rows(audio, None if measure else out, "loudness")
    B, n_max = audio.shape
    hop = MF.loudness_hop(sample_rate)
    sos = MF.k_weighting(sample_rate)
    tg = md = None
    if target is not None:
        t = _row_values(target, B, "loudness", "targets")
        on = ~np.isnan(t)
        if not bool(np.all(np.abs(t[on]) <= MF.DB_LIMIT)):
            raise ValueError(f"loudness: a target must lie inside [-{MF.DB_LIMIT}, {MF.DB_LIMIT}] LUFS (NaN: leave the row), got {t.tolist()}")
        t = np.where(on, t, 0.0)
    _chk(audio, F32, "audio")  # (every ValueError above comes before the device is touched)
    n = _lengths(n, B, audio.device, "loudness", "n")
    if not measure and out is not None and out.device != audio.device:
        raise ValueError("loudness: audio and out must live on the same GPU")
    if not measure and not bool(on.any()):  # nothing to launch
        stats = torch.tensor([[-math.inf, -math.inf, 0.0, 1.0]], dtype=torch.float64, device=audio.device).repeat(B, 1)
        if out is audio:
            return audio, stats
        if out is None:
            out = torch.empty((B, n_max), dtype=F32, device=audio.device)
        out.copy_(audio)
        if n is not None:
            out.masked_fill_(torch.arange(n_max, device=audio.device)[None] >= n.clamp(0, n_max)[:, None], 0.0)
        return out, stats
    if target is not None:
        tg = torch.from_numpy(t).to(audio.device)
        md = torch.from_numpy(on.astype(np.int32)).to(audio.device)
    lib = L.load()
    nbytes = lib.wft_loudness_workspace_bytes(B, n_max, hop)
    if nbytes < 0:
        raise ValueError(f"loudness: {B} rows of {n_max} samples at hop {hop} are not supported by wft_loudness_f32")
    if not measure and out is None:
        out = torch.empty((B, n_max), dtype=F32, device=audio.device)
    stats = torch.empty((B, 4), dtype=torch.float64, device=audio.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=audio.device)
    ld_in = audio.stride(0) if B > 1 else max(audio.stride(0), n_max)
    ld_out = 0 if measure else (out.stride(0) if B > 1 else max(out.stride(0), n_max))
    L.check(lib.wft_loudness_f32(_p(audio), ld_in, _p(n), n_max, sos.ctypes.data, hop, _p(tg), _p(md), None if measure else _p(out), ld_out,
                                 _p(stats), _p(ws), nbytes, B, L.stream_ptr()), "wft_loudness_f32")
    return (None if measure else out), stats


def bg_records(rec, B: int, lengths):
    """rec -> checked wft_bg_rec records [B] (data/mix_fx.py RECORD_DTYPE).  rec: a numpy structured array [B] of that dtype.
    lengths: the bank's entry lengths.  ValueError: a kind outside 0..2; on a row with a kind an entry outside the bank, an offset
    outside its entry, a dB value that is not finite or beyond +-200."""
    import numpy as np

    from whisper_finetune.data import mix_fx as MF

    a = np.asarray(rec)
    if a.dtype != MF.RECORD_DTYPE or a.shape != (B,):
        raise ValueError(f"bg_mix: {B} rows need {B} records of data/mix_fx.py RECORD_DTYPE, got {a.dtype} {tuple(a.shape)}")
    table = MF.none_table(B)
    table[:, 0], table[:, 1], table[:, 2], table[:, 3] = a["kind"], a["entry"], a["offset"], a["db"]
    return MF.records_from_table(MF.check_table(table, lengths))


def bg_mix(audio, bank, bank_off, rec, n=None, *, out=None, lengths=None):
    """A scaled entry of a noise bank added to every row (wft_bg_mix_f32, include/wft.h "Loudness and background noise":
    audiomentations' AddBackgroundNoise, restated).

    audio f32 [B, ld] on the device (stride(1) == 1); bank f32 [total] and bank_off i64 [K + 1] on the same device (data/mix_fx.py
    pack_bank); rec: the rows' records on the HOST (bg_records states the form; kind 0 = the row is copied); n i32 [B] on the device
    or None; lengths: the entry lengths as host integers (None: read back from bank_off, one small copy).  out: None (a new tensor),
    `audio` itself (in place) or an f32 [B, ld] tensor that does not overlap `audio`.
    -> (out, stats f64 [B, 3] on the device = clean RMS, noise RMS, scale).  When no row has a kind nothing is launched.
    Every host-side check raises ValueError before the device is touched."""
    import numpy as np

    from whisper_finetune.data import mix_fx as MF

    audio = _mix_rows(audio, out, "bg_mix")
    B, n_max = audio.shape
    if not torch.is_tensor(bank) or bank.dtype != F32 or bank.dim() != 1 or bank.numel() < 1 or not bank.is_contiguous():
        raise ValueError("bg_mix: bank must be a contiguous float32 tensor [total]")
    if not torch.is_tensor(bank_off) or bank_off.dtype != torch.int64 or bank_off.dim() != 1 or bank_off.numel() < 2 or not bank_off.is_contiguous():
        raise ValueError("bg_mix: bank_off must be a contiguous int64 tensor [K + 1]")
    K_ = bank_off.numel() - 1
    if lengths is None:
        off = bank_off.detach().cpu().numpy()
        if int(off[0]) != 0 or int(off[-1]) != bank.numel() or bool(np.any(np.diff(off) < 1)):
            raise ValueError("bg_mix: bank_off must rise from 0 to the bank's size in steps of at least 1")
        lengths = np.diff(off)
    if len(lengths) != K_:
        raise ValueError(f"bg_mix: {len(lengths)} lengths for a bank of {K_} entries")
    r = bg_records(rec, B, lengths)
    _chk(audio, F32, "audio")  # (every ValueError above comes before the device is touched)
    n = _lengths(n, B, audio.device, "bg_mix", "n")
    if bank.device != audio.device or bank_off.device != audio.device or (out is not None and out.device != audio.device):
        raise ValueError("bg_mix: audio, bank, bank_off and out must live on the same GPU")
    if not bool((r["kind"] != 0).any()):  # nothing to launch
        stats = torch.zeros((B, 3), dtype=torch.float64, device=audio.device)
        if out is audio:
            return audio, stats
        if out is None:
            out = torch.empty((B, n_max), dtype=F32, device=audio.device)
        out.copy_(audio)
        if n is not None:
            out.masked_fill_(torch.arange(n_max, device=audio.device)[None] >= n.clamp(0, n_max)[:, None], 0.0)
        return out, stats
    lib = L.load()
    nbytes = lib.wft_bg_mix_workspace_bytes(B, n_max)
    if out is None:
        out = torch.empty((B, n_max), dtype=F32, device=audio.device)
    rec_d = torch.from_numpy(r.view("u1").reshape(B, MF.RECORD_DTYPE.itemsize).copy()).to(audio.device)
    stats = torch.empty((B, 3), dtype=torch.float64, device=audio.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=audio.device)
    ld_in = audio.stride(0) if B > 1 else max(audio.stride(0), n_max)
    ld_out = out.stride(0) if B > 1 else max(out.stride(0), n_max)
    L.check(lib.wft_bg_mix_f32(_p(audio), ld_in, _p(n), n_max, _p(bank), _p(bank_off), K_, _p(rec_d), _p(out), ld_out, _p(stats), _p(ws),
                               nbytes, B, L.stream_ptr()), "wft_bg_mix_f32")
    return out, stats


def pcm_decode(raw, table_rows, n_max=None, out=None):
    """File bytes -> mono f32 rows, one launch for a ragged batch (wft_pcm_decode_f32, include/wft.h "PCM decode").

    raw: uint8 [nbytes] on the device, contiguous, at any alignment (a view into a larger buffer is fine).  table_rows: the rows on
    the HOST, (byte_off, frames, channels, format, channel) each — format a name of data/audio_io.py FORMATS or its WFT_PCM_*
    number, channel "mean" / -1 or 0..channels-1 — or an array of audio_io.ROW_DTYPE.  n_max: the output width (None: the largest
    frame count).  out: None (a new tensor) or f32 [B, n_max] on raw's device with unit column stride and rows that do not overlap.
    -> out f32 [B, n_max]: row b holds its decoded frames, zeros behind them.  Every row is checked on the host with the conditions
    the kernel clamps with (audio_io.pcm_rows): ValueError before the device is touched."""
    from whisper_finetune.data import audio_io as AIO

    if not torch.is_tensor(raw) or raw.dtype != torch.uint8 or raw.dim() != 1 or raw.numel() < 1 or raw.stride(0) != 1:
        raise ValueError("pcm_decode: raw must be a contiguous uint8 tensor [nbytes] with at least one byte")
    rec, n_max = AIO.pcm_rows(table_rows, int(raw.numel()), n_max)
    B = rec.shape[0]
    if out is not None and (not torch.is_tensor(out) or out.dtype != F32 or tuple(out.shape) != (B, n_max) or out.stride(1) != 1
                            or (B > 1 and out.stride(0) < n_max)):
        raise ValueError(f"pcm_decode: out must be f32 [{B}, {n_max}] with unit column stride and rows that do not overlap")
    _chk(raw, torch.uint8, "raw")  # (every ValueError above comes before the device is touched)
    if out is not None and out.device != raw.device:
        raise ValueError("pcm_decode: raw and out must live on the same GPU")
    if out is None:
        out = torch.empty((B, n_max), dtype=F32, device=raw.device)
    rows_d = torch.from_numpy(rec.view("u1").reshape(B, AIO.ROW_DTYPE.itemsize).copy()).to(raw.device)
    ld_out = out.stride(0) if B > 1 else max(out.stride(0), n_max)
    L.check(L.load().wft_pcm_decode_f32(_p(raw), int(raw.numel()), _p(rows_d), _p(out), ld_out, n_max, B, L.stream_ptr()), "wft_pcm_decode_f32")
    return out


EDIT_MAX_LEN = 4096   # wft_edit_max_len(): symbols per side of a pair
EDIT_MAX_PAIRS = 1 << 20


def _edit_row_dtype():
    import numpy as np

    return np.dtype([("ref_off", "<i8"), ("hyp_off", "<i8"), ("ref_len", "<i4"), ("hyp_len", "<i4"), ("reserved", "<i4", (2,))])


EDIT_ROW_DTYPE = _edit_row_dtype()  # numpy form of wft_edit_row (lib.EditRow), 32 bytes


def edit_rows(rows, n_sym: int, max_len=None):
    """A pair table -> (records of EDIT_ROW_DTYPE [P], max_len), checked with the conditions wft_edit_counts_i32 refuses a row with.

    rows: integers [P, 4], (ref_off, hyp_off, ref_len, hyp_len) each, or an EDIT_ROW_DTYPE array.  max_len: the longest side the
    launch is sized for (None: the longest side of the table, at least 1).  ValueError: no pair or more than 2^20, a length outside
    0..max_len, a negative offset, offset + length > n_sym, max_len outside 1..4096, n_sym < 1."""
    import numpy as np

    if isinstance(rows, np.ndarray) and rows.dtype == EDIT_ROW_DTYPE:
        rec = np.ascontiguousarray(rows).reshape(-1).copy()
    else:
        arr = np.asarray(rows)
        if arr.ndim != 2 or arr.shape[1] != 4 or arr.dtype.kind not in "iu":
            raise ValueError(f"edit_counts: rows must be integers [P, 4] of (ref_off, hyp_off, ref_len, hyp_len), got shape {arr.shape} of {arr.dtype}")
        arr = arr.astype(np.int64)
        if arr.shape[0] and (np.abs(arr[:, 2:]) >= (1 << 31)).any():
            raise ValueError("edit_counts: a length does not fit its 32-bit field")
        rec = np.zeros(arr.shape[0], dtype=EDIT_ROW_DTYPE)
        rec["ref_off"], rec["hyp_off"], rec["ref_len"], rec["hyp_len"] = arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3]
    P = rec.shape[0]
    if not 1 <= P <= EDIT_MAX_PAIRS:
        raise ValueError(f"edit_counts: 1 to 2^20 pairs per call, got {P}")
    if isinstance(n_sym, bool) or not isinstance(n_sym, (int, np.integer)) or n_sym < 1:
        raise ValueError(f"edit_counts: sym must hold at least one symbol, got {n_sym!r}")
    if max_len is None:
        max_len = max(1, int(rec["ref_len"].max()), int(rec["hyp_len"].max()))
    if isinstance(max_len, bool) or not isinstance(max_len, (int, np.integer)) or not 1 <= max_len <= EDIT_MAX_LEN:
        raise ValueError(f"edit_counts: max_len must be an integer inside [1, {EDIT_MAX_LEN}], got {max_len!r}")
    for off, ln in (("ref_off", "ref_len"), ("hyp_off", "hyp_len")):
        o, n = rec[off].astype(np.int64), rec[ln].astype(np.int64)
        bad = (n < 0) | (n > max_len) | (o < 0) | (o > n_sym - n)
        if bad.any():
            p = int(np.flatnonzero(bad)[0])
            raise ValueError(f"edit_counts: pair {p}: {off} {int(o[p])} with {ln} {int(n[p])} is outside sym [0, {n_sym}) or 0..max_len = {max_len}")
    return rec, int(max_len)


def edit_counts(sym, rows, max_len=None, rows_d=None):
    """(H, S, D, I) of every (reference, hypothesis) pair, one launch for a ragged batch (wft_edit_counts_i32, include/wft.h "Edit counts").

    sym: int32 [n_sym] on the device, contiguous: the symbols of every reference and hypothesis.  rows: the pairs on the HOST (see
    edit_rows).  max_len: the longest side the launch is sized for (None: the table's own).  rows_d: None (the table is copied to
    the device here) or a contiguous int32 [8 P] tensor on sym's device that already holds the records of `rows` — a caller that
    packs table and symbols into one host buffer pays one copy instead of two (eval/metrics.py edit_counts_batch).
    -> int32 [P, 4] on sym's device.
    Every row is checked on the host with the conditions the kernel refuses it with: ValueError before the device is touched."""
    if not torch.is_tensor(sym) or sym.dtype != torch.int32 or sym.dim() != 1 or sym.numel() < 1 or sym.stride(0) != 1:
        raise ValueError("edit_counts: sym must be a contiguous int32 tensor [n_sym] with at least one symbol")
    rec, max_len = edit_rows(rows, int(sym.numel()), max_len)
    _chk(sym, torch.int32, "sym")
    P = rec.shape[0]
    if rows_d is None:
        rows_d = torch.from_numpy(rec.view("u1").reshape(P, EDIT_ROW_DTYPE.itemsize).copy()).to(sym.device)
    elif (not torch.is_tensor(rows_d) or rows_d.dtype != torch.int32 or rows_d.dim() != 1 or rows_d.numel() != 8 * P or rows_d.stride(0) != 1
          or rows_d.device != sym.device or rows_d.data_ptr() % 8):
        raise ValueError(f"edit_counts: rows_d must be a contiguous, 8-byte aligned int32 tensor [{8 * P}] on sym's device")
    out = torch.empty((P, 4), dtype=torch.int32, device=sym.device)
    L.check(L.load().wft_edit_counts_i32(_p(sym), int(sym.numel()), _p(rows_d), _p(out), 4, P, max_len, L.stream_ptr()), "wft_edit_counts_i32")
    return out


def mel_to_tmajor(mel, c_pad: int):
    _chk(mel, F32, "mel")
    mel = mel.contiguous()
    B, n_mels, T = mel.shape
    out = torch.empty((B, T + 2, c_pad), dtype=BF16, device=mel.device)
    L.check(L.load().wft_mel_to_tmajor_bf16(_p(mel), _p(out), B, n_mels, T, c_pad, L.stream_ptr()), "wft_mel_to_tmajor_bf16")
    return out


# --------------------------------------------------------------------------- optimizer
def adamw_step(p, g, m, v, p_bf16, lr, beta1, beta2, eps, wd, bc1, bc2, gscale=None):
    L.check(
        L.load().wft_adamw_step(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), p.numel(), lr, beta1, beta2, eps, wd, bc1, bc2,
                                _p(gscale), L.stream_ptr()),
        "wft_adamw_step",
    )


def sumsq(g, out):
    L.check(L.load().wft_sumsq_f32(_p(g), g.numel(), _p(out), L.stream_ptr()), "wft_sumsq_f32")


# --------------------------------------------------------------------------- multi-tensor optimizer steps
MT_CHUNK = 65536  # include/wft.h WFT_MT_CHUNK


class _Stager:
    """Small integer tables (tensor addresses, element counts) to the device WITHOUT a host synchronisation.
    `torch.tensor(list, device=...)` goes through pageable memory: the copy waits for everything queued on the stream and the
    host waits for the copy — thirteen such stalls per optimizer step emptied the queue in front of every Muon bucket
    (profiles/r03_lora_gap_analysis.log: 16 of the 17.7 ms the GPU idled per LoRA + Muon step).  Here the values are written
    into a pinned staging buffer (recycled once its copy event has fired) and copied stream-ordered."""

    def __init__(self):
        self.pool = {}  # (dtype, capacity) -> [(pinned tensor, numpy view, event)]

    def upload(self, values, dtype, device) -> torch.Tensor:
        n = len(values)
        cap = max(256, 1 << max(n - 1, 0).bit_length())
        pool = self.pool.setdefault((dtype, cap), [])
        for i, ent in enumerate(pool):
            if ent[2].query():
                pool.pop(i)
                break
        else:
            host = torch.empty(cap, dtype=dtype, pin_memory=True)
            ent = (host, host.numpy(), torch.cuda.Event())
        host, view, ev = ent
        view[:n] = values
        dev = torch.empty(n, dtype=dtype, device=device)
        dev.copy_(host[:n], non_blocking=True)
        ev.record()
        pool.append(ent)
        return dev


_STAGER = _Stager()


def upload_table(values, dtype, device) -> torch.Tensor:
    """1-D integer table -> device tensor, stream-ordered, no host synchronisation (CPU tensors: plain construction)."""
    if torch.device(device).type != "cuda":
        return torch.tensor(values, dtype=dtype, device=device)
    return _STAGER.upload(values, dtype, device)


class TensorTable:
    """Device-side pointer table for the wft_mt_* / wft_muon_*_mt entry points: `rows` lists of equally long tensor
    lists (row r of tensor t at tab[r * n + t]).  numel / chunk_start depend only on the shapes and are cached by
    the caller; the pointer rows are rebuilt every step because gradient tensors are re-allocated."""

    def __init__(self, tensors):
        self.n = len(tensors)
        self.device = tensors[0].device
        numel = [t.numel() for t in tensors]
        starts, tot = [], 0
        for ne in numel:
            starts.append(tot)
            tot += (ne + MT_CHUNK - 1) // MT_CHUNK
        starts.append(tot)
        self.total_chunks = tot
        self.numel = upload_table(numel, torch.int64, self.device)
        self.chunk_start = upload_table(starts, torch.int32, self.device)

    def pointers(self, *rows, allow_none=False, static=(), dtypes=None):
        """`static`: indices of rows whose tensors live as long as the table (parameters, optimizer state): each is checked once
        (dtype / layout / device do not change under a live tensor object) — with 1 259 parameters the three checks on four rows
        were most of the 2.6 ms the GPU idled in front of the AdamW launch (profiles/r03_headline_gap_analysis.log)."""
        flat = []
        seen = self.__dict__.setdefault("_checked", set())
        for ri, r in enumerate(rows):
            assert len(r) == self.n
            trust = ri in static
            want = F32 if dtypes is None else dtypes[ri]  # (the 8-bit optimizer's code rows are uint8)
            for t in r:
                if t is None and allow_none:
                    flat.append(0)
                    continue
                ptr = t.data_ptr()
                # validated once per (object, storage address, dtype): an id recycled by another tensor after
                # optimizer.load_state_dict, or a parameter re-typed in place (.data = ..., model.half()), is checked again
                key = (id(t), ptr, t.dtype)
                if not (trust and key in seen):
                    if t.dtype != want or not t.is_contiguous() or not t.is_cuda:
                        raise L.WftError(f"multi-tensor optimizer kernels need contiguous {want} HIP tensors")
                    if trust:
                        seen.add(key)
                flat.append(ptr)
        return upload_table(flat, torch.int64, self.device)


def mt_sumsq(table: TensorTable, grads, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum over all tensors of g^2 -> f32 [1] on the device (fixed-order reduction); a None gradient adds nothing."""
    tab = table.pointers(grads, allow_none=True)
    partial = torch.empty(table.total_chunks, dtype=F32, device=table.device)
    out = torch.empty(1, dtype=F32, device=table.device) if out is None else out
    L.check(L.load().wft_mt_sumsq_f32(_p(tab), _p(table.numel), _p(table.chunk_start), table.n, table.total_chunks,
                                      _p(partial), _p(out), L.stream_ptr()), "wft_mt_sumsq_f32")
    return out


def mt_adamw(table: TensorTable, params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, wd, bc1, bc2, sumsq=None,
             max_norm=0.0):
    tab = table.pointers(params, grads, exp_avg, exp_avg_sq, static=(0, 2, 3))
    L.check(L.load().wft_mt_adamw(_p(tab), _p(table.numel), _p(table.chunk_start), table.n, table.total_chunks, lr, beta1,
                                  beta2, eps, wd, bc1, bc2, _p(sumsq), float(max_norm), L.stream_ptr()), "wft_mt_adamw")


def mt_adamw8(table: TensorTable, params, grads, state1, state2, absmax1, absmax2, qmap1, qmap2, lr, beta1, beta2, eps, wd, bc1, bc2,
              sumsq=None, max_norm=0.0):
    """Block-wise 8-bit AdamW for every tensor of the table in one launch (wft_mt_adamw8; include/wft.h)."""
    U8 = torch.uint8
    tab = table.pointers(params, grads, state1, state2, absmax1, absmax2, static=(0, 2, 3, 4, 5), dtypes=(F32, F32, U8, U8, F32, F32))
    L.check(L.load().wft_mt_adamw8(_p(tab), _p(table.numel), _p(table.chunk_start), table.n, table.total_chunks, _p(qmap1), _p(qmap2),
                                   lr, beta1, beta2, eps, wd, bc1, bc2, _p(sumsq), float(max_norm), L.stream_ptr()), "wft_mt_adamw8")


def transpose_bf16(src: torch.Tensor, dst: torch.Tensor):
    """src bf16 [batch, rows, cols] contiguous -> dst [batch, cols, rows]."""
    _chk(src, BF16, "src"); _chk(dst, BF16, "dst")
    b, r, c = src.shape
    assert src.is_contiguous() and dst.is_contiguous() and dst.shape == (b, c, r)
    L.check(L.load().wft_transpose_bf16(_p(src), r, c, _p(dst), b, L.stream_ptr()), "wft_transpose_bf16")
    return dst


NS_COEFFS = (3.4445, -4.7750, 2.0315)  # muon.py zeropower_via_newtonschulz5


def muon_group_step(params, grads, bufs, lr, wd, momentum, nesterov=True, ns_steps=5, sumsq=None, max_norm=0.0,
                    return_update=False, shard=None, validated=False):
    """One Muon step for a list of same-shape 2-D f32 parameters (muon.py muon_update + the p update of
    SingleDeviceMuonWithAuxAdam.step): momentum/nesterov -> bf16 -> Frobenius normalisation -> 5 Newton-Schulz
    iterations as batched MFMA GEMMs -> p = p(1 - lr wd) - lr sqrt(max(1, rows/cols)) X.

    shard = (rank, world, all_gather): the distributed variant (muon.MuonWithAuxAdam, reference model/optimizer.py:227-228,
    SURVEY.md §2.2 C6).  The matrices of the group are dealt to the ranks in contiguous chunks of ceil(n / world); a rank
    runs momentum + Newton-Schulz for ITS chunk only (`grads` / `bufs` then hold that chunk: bufs[i] belongs to
    params[lo + i]), the orthogonalised updates — a bf16 quantity — are all-gathered (half the bytes of gathering the fp32
    parameters, the package's form) and every rank applies all n updates in fp32, so parameters stay bit-identical across
    ranks.  `all_gather(out, inp)` fills out [world * chunk, ...] from every rank's inp [chunk, ...]."""
    lib = L.load()
    n_all = len(params)
    rows, cols = params[0].shape
    dev = params[0].device
    tall = rows > cols
    R, Cc = (cols, rows) if tall else (rows, cols)
    Rp, Cp = round_up(R, 128), round_up(Cc, 128)
    numel = rows * cols
    chunks = (numel + MT_CHUNK - 1) // MT_CHUNK
    if shard is None:
        lo, hi, per = 0, n_all, n_all
    else:
        rank, world, all_gather = shard
        per = (n_all + world - 1) // world
        lo, hi = min(rank * per, n_all), min((rank + 1) * per, n_all)
    n = hi - lo
    if len(grads) != n or len(bufs) != n:
        raise L.WftError(f"muon_group_step: {n} owned matrices but {len(grads)} gradients / {len(bufs)} momentum buffers")
    # (validated: the caller checked `params` and `bufs` when it built them — the optimizer's per-group plan; gradients are new
    # tensors every step and are always checked)
    for row in ((grads,) if validated else (params, grads, bufs)):
        for t in row:
            if t is None and row is grads:
                continue  # no gradient this step: an all-zero one to the momentum kernel (muon.py "force synchronization")
            if t.dtype != F32 or not t.is_contiguous() or t.shape != (rows, cols) or not t.is_cuda:
                raise L.WftError("muon_group_step needs contiguous f32 HIP tensors of one shape (there is no CPU path)")
    O = None
    ldo, so = (Rp, Cp * Rp) if tall else (Cp, Rp * Cp)
    if n > 0:
        flat = [t.data_ptr() for t in params[lo:hi]] + [0 if t is None else t.data_ptr() for t in grads] + [t.data_ptr() for t in bufs]
        tab = upload_table(flat, torch.int64, dev)
        U = torch.empty((n, rows, cols), dtype=BF16, device=dev)
        partial = torch.empty((n, chunks), dtype=F32, device=dev)
        L.check(lib.wft_muon_momentum_mt(_p(tab), n, numel, momentum, int(nesterov), _p(U), _p(partial), _p(sumsq),
                                         float(max_norm), L.stream_ptr()), "wft_muon_momentum_mt")
        X = torch.empty((n, Rp, Cp), dtype=BF16, device=dev)
        Xt = torch.empty((n, Cp, Rp), dtype=BF16, device=dev)
        L.check(lib.wft_muon_prepare(_p(U), rows, cols, _p(partial), chunks, _p(X), _p(Xt), Rp, Cp, n, L.stream_ptr()),
                "wft_muon_prepare")
        del U
        A = torch.empty((n, Rp, Rp), dtype=BF16, device=dev)
        Bm = torch.empty((n, Rp, Rp), dtype=BF16, device=dev)
        Xt2 = torch.empty((n, Cp, Rp), dtype=BF16, device=dev)
        a, b, c = NS_COEFFS
        for it in range(ns_steps):
            gemm_nt(X, X, M=Rp, N=Rp, K=Cp, lda=Cp, ldb=Cp, out=A, ldc=Rp, batch=n, strideA=Rp * Cp, strideB=Rp * Cp,
                    strideC=Rp * Rp)                                                        # A = X X^T
            gemm_nt(A, A, M=Rp, N=Rp, K=Rp, lda=Rp, ldb=Rp, out=Bm, ldc=Rp, batch=n, strideA=Rp * Rp, strideB=Rp * Rp,
                    strideC=Rp * Rp, alpha=c, residual=A, ldr=Rp, strideR=Rp * Rp, beta=b)  # B = b A + c A A   (A = A^T)
            gemm_nt(Xt, Bm, M=Cp, N=Rp, K=Rp, lda=Rp, ldb=Rp, out=Xt2, ldc=Rp, batch=n, strideA=Cp * Rp, strideB=Rp * Rp,
                    strideC=Cp * Rp, residual=Xt, ldr=Rp, strideR=Cp * Rp, beta=a)          # X'^T = a X^T + X^T B (B = B^T)
            Xt, Xt2 = Xt2, Xt
            if it + 1 < ns_steps or not tall:
                transpose_bf16(Xt, X)
        O = Xt if tall else X
    if shard is not None:
        mine = torch.zeros((per,) + ((Cp, Rp) if tall else (Rp, Cp)), dtype=BF16, device=dev)
        if n > 0:
            mine[:n].copy_(O)
        O = torch.empty((world * per,) + tuple(mine.shape[1:]), dtype=BF16, device=dev)
        all_gather(O, mine)
    scale = max(1.0, rows / cols) ** 0.5
    ptab = upload_table([t.data_ptr() for t in params], torch.int64, dev)
    L.check(lib.wft_muon_apply_mt(_p(ptab), n_all, rows, cols, _p(O), ldo, so, lr, wd, scale, L.stream_ptr()), "wft_muon_apply_mt")
    if return_update:
        return O[:n_all, :rows, :cols].float() * scale
    return None
