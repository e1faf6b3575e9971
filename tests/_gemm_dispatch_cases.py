"""The cases of the GEMM dispatch table (tests/golden/gemm_dispatch_256cu.json) and how one case is asked: shared by
tools/dev/record_gemm_dispatch.py, which records a library's answers, and tests/test_gemm_dispatch_host.py, which compares the
current library with the record.  Every entry point asked here is a pure host function; without a device the library assumes
256 CUs, the MI355X's count, so the answers are the same with and without a GPU."""
import ctypes

from whisper_finetune.engine import lib as L

PTR = 1 << 20  # placeholders with the alignment real operands have: nothing is dereferenced
DIMS = (384, 512, 768, 1024, 1280)
ROWS = (8, 100, 448, 1024, 1500, 3000, 4096, 8704, 12000, 48000, 144000)
VOCAB = 51968


def _pairs(d):
    return ((d, d), (3 * d, d), (4 * d, d), (d, 4 * d), (VOCAB, d), (d, VOCAB), (128, d))


NT_FLAGS = {
    "none": {},
    "bias": dict(bias=PTR),
    "bias+residual": dict(bias=PTR, residual=PTR, ldr="N"),
    "gelu_grad": dict(epilogue=L.EPI_GELU_GRAD, aux=PTR, ldaux="N"),
    "mul_aux": dict(epilogue=L.EPI_MUL_AUX, aux=PTR, ldaux="N"),
    "mul_aux+colsum": dict(epilogue=L.EPI_MUL_AUX, aux=PTR, ldaux="N", colsum=PTR),
    "gelu_grad8": dict(epilogue=L.EPI_GELU_GRAD8, aux=PTR),
    "mul_aux8": dict(epilogue=L.EPI_MUL_AUX8, aux=PTR),
    "mul_aux8+colsum": dict(epilogue=L.EPI_MUL_AUX8, aux=PTR, colsum=PTR),
    "f32": dict(c_is_f32=1),
    "variant1": dict(variant=1),
    "colsum": dict(colsum=PTR),
    "p_valid8": dict(p_valid=8),
}
TN_FLAGS = {
    "f32": dict(c_is_f32=1),
    "variant1": dict(c_is_f32=1, variant=1),
    "bf16": {},
    "p_valid8": dict(c_is_f32=1, p_valid=8),
    "p_valid8+col_scale": dict(c_is_f32=1, p_valid=8, tn_col_scale=PTR, tn_scale_rows=1),
    "batch2": dict(c_is_f32=1, batch=2),
    "seg1": dict(c_is_f32=1, segs=1),
    "seg3": dict(c_is_f32=1, segs=3),
}
# shapes at which the launcher changes kernel (M, N, K, flags)
NT_BOUNDARY = (
    (4224, 1024, 64, "none"),      # 128-tile kernel, two-buffer grid
    (256, 256, 256, "none"),       # 128-tile kernel, ring
    (128, 256, 4096, "none"),      # ring with split-K partials: 524 288 bytes
    (300, 128, 128, "p_valid8"),   # rank-r load-stream kernel
    (4096, 2048, 64, "none"),      # 256 x 256 ping-pong (K too short for the one-wave-per-SIMD kernel)
    (4096, 2048, 256, "none"),     # one-wave-per-SIMD kernel
)
TN_BOUNDARY = (
    (256, 256, 16384, "f32"),      # split: ping-pong kernel without a workspace, one-wave-per-SIMD kernel with it
    (768, 768, 4096, "f32"),       # 128-tile kernel
)


def nt_cases():
    """(M, N, K, flag name) in table order."""
    out = [(m, n, k, f) for d in DIMS for n, k in _pairs(d) for m in ROWS for f in NT_FLAGS]
    return out + list(NT_BOUNDARY)


def tn_cases():
    """(P, Q, R, flag name) in table order."""
    out = [(p, q, r, f) for d in DIMS for p, q in _pairs(d) for r in ROWS for f in TN_FLAGS]
    return out + list(TN_BOUNDARY)


def _args(M, N, K, lda, ldb, flags):
    a = L.GemmArgs()
    a.A = a.B = a.C = PTR
    a.M, a.N, a.K, a.batch, a.alpha, a.beta = M, N, K, 1, 1.0, 1.0
    a.lda, a.ldb, a.ldc = lda, ldb, N
    for k, v in flags.items():
        if k == "segs":
            a.tn_seg_count = v
            for i in range(v):
                a.tn_seg_end[i], a.tn_seg_ptr[i] = (M * (i + 1)) // v, PTR
        else:
            setattr(a, k, N if v == "N" else v)
    return a


def nt_args(M, N, K, flag):
    return _args(M, N, K, K, K, NT_FLAGS[flag])


def tn_args(P, Q, R, flag):
    return _args(P, Q, R, P, Q, TN_FLAGS[flag])


def nt_answers(h, case):
    """[variant, aux8 bytes, column-sum workspace bytes, split-K workspace bytes]"""
    a = ctypes.byref(nt_args(*case))
    return [int(h.wft_gemm_nt_variant(a)), int(h.wft_gemm_nt_aux8_bytes(a)), int(h.wft_gemm_nt_colsum_workspace_bytes(a)),
            int(h.wft_gemm_nt_splitk_workspace_bytes(a))]


def tn_answers(h, case):
    """[segments_ok, workspace bytes, variant without a workspace, variant with exactly the workspace asked for] — the order in
    which engine/kernels.py asks: a split product goes to the one-wave-per-SIMD kernel only once its workspace is granted."""
    args = tn_args(*case)
    a = ctypes.byref(args)
    seg_ok = int(h.wft_gemm_tn_segments_ok(a))
    need = int(h.wft_gemm_tn_workspace_bytes(a))
    bare = int(h.wft_gemm_tn_variant(a))
    args.workspace, args.workspace_bytes = 1 << 24, need
    return [seg_ok, need, bare, int(h.wft_gemm_tn_variant(a))]


def all_answers(h):
    return {"nt": [nt_answers(h, c) for c in nt_cases()], "tn": [tn_answers(h, c) for c in tn_cases()]}
