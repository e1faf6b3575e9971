"""Test helper of the W8A8 GEMM (csrc/gemm_i8.hip, wft_gemm_nt_i8): operand builders, the numpy restatement of include/wft.h's
definition, the case table and the mutants, shared by tests/test_gemm_i8_host.py (CPU) and tests/test_gemm_i8_gpu.py.

  make_case      operands of one product, built so that the conditions the tests rely on hold by construction (listed there).
  reference      int64 dot products, then the f32 epilogue in np.float32, one operation per line, one bf16 rounding
                 (_q8_cases.bf16_round), written into the caller's C buffer as the kernel writes it: ldc > N, guard rows behind M.
                 `mutant`: one wrong kernel (MUTANTS); the host test shows that each changes an output bit somewhere in the table.
  gelu_bound     what a GELU form may differ from the float64 evaluation of the EXACT f32 pre-activation by, per element.

The sum is integer arithmetic: for the plain / bias / residual forms the kernel is held to `reference` bit for bit.  The GELU forms
go through the kernel's own erf approximation, so they are held to a bound built from the constants of _q8_cases.gemm_bound with the
dot-product term set to zero (the pre-activation is exact):
    e_act = |pre| (0.75e-7 + 8u)          the kernel's gelu: erf to 1.5e-7 absolute inside 0.5 x (1 + erf), a handful of roundings
    e_out = e_act + u |out|               the residual add
    e     = e_out + ub (|out| + e_out)    one bf16 rounding
plus 1e-30 for results that underflow.  Nothing here is taken from what the kernel returns."""
import functools

import numpy as np

from tests._q8_cases import GELU_LIP, U32, UBF, _gelu64, bf16_round  # noqa: F401  (GELU_LIP: the bound's constants come from one place)

SENTINEL = np.float32(-1.5 * 2.0 ** -100)  # a bf16 value no case produces (the host test checks); fills C outside [M, N]
POISON = 0x7F                    # the pad columns of A and B
GUARD_ROWS = 2
PAD_A, PAD_B, PAD_C = 64, 128, 8  # lda = K + 64 (one whole k-step of poison for a kernel that takes K from lda), ldb >= lda, ldc = N + 8

FORMS = {
    "plain": dict(bias=False, gelu=False, res=False),
    "bias": dict(bias=True, gelu=False, res=False),
    "bias_res": dict(bias=True, gelu=False, res=True),
    "gelu": dict(bias=False, gelu=True, res=False),
    "gelu_bias_res": dict(bias=True, gelu=True, res=True),
}
EXACT_FORMS = ("plain", "bias", "bias_res")
SCALES = ("unit", "pow2", "general")
MS = (1, 33, 127, 128, 129, 255, 256, 257)  # both candidate row tiles (128, 256): one below, at, one above; M = 1; the first M served
NS = (128, 256, 384)
KS = (64, 128, 192, 320)                   # one k-step; even and odd step counts for a double buffer

MUTANTS = ("drop_last_kblock", "first_kblock_twice", "scales_swapped", "scale_one_by_one", "truncating_cvt", "skip_last_row",
           "write_row_M", "pad_column_read", "bias_before_scale", "residual_before_gelu", "unsigned_bytes")


def table():
    """[(id, kwargs of make_case, form)]: every (M, N, K) once, forms and scales cycling with coprime periods so that every M meets
    every form and every (form, scales) pair occurs; then the deep case and the one with -128 bytes."""
    out, i = [], 0
    forms = list(FORMS)
    for M in MS:
        for N in NS:
            for K in KS:
                form, sc = forms[i % 5], SCALES[i % 3]
                out.append((f"{M}x{N}x{K}-{form}-{sc}", dict(M=M, N=N, K=K, scales=sc), form))
                i += 1
    out.append(("deep-129x128x5120-bias-unit", dict(M=129, N=128, K=5120, scales="unit", kind="deep"), "bias"))
    out.append(("neg128-33x128x128-bias_res-general", dict(M=33, N=128, K=128, scales="general", kind="neg128"), "bias_res"))
    return out


@functools.lru_cache(maxsize=None)
def _make_case(M, N, K, scales, kind):
    rng = np.random.default_rng(1000003 + 7919 * M + 31 * N + K)
    lda, ldb, ldc = K + PAD_A, K + PAD_B, N + PAD_C
    A = np.full((M, lda), POISON, dtype=np.int8)
    B = np.full((N, ldb), POISON, dtype=np.int8)
    nk = K // 64
    if kind == "deep":
        # every byte +-127; row m of A is negative on its first 3m columns, row n of B on its last 5n + 1: the two ranges never
        # meet (3 * 128 + 5 * 127 + 1 < K), so acc = 127^2 (K - 2 (3m + 5n + 1)) >= 127^2 * 3080 > 2^25 everywhere
        k = np.arange(K)
        A[:, :K] = np.where(k[None, :] < 3 * np.arange(M)[:, None], -127, 127)
        B[:, :K] = np.where(k[None, :] >= K - (5 * np.arange(N)[:, None] + 1), -127, 127)
    else:
        A[:, :K] = rng.integers(-127, 128, size=(M, K))
        B[:, :K] = rng.integers(-127, 128, size=(N, K))
        # rows M-1 and M-2 differ from every other row: column 1 is small everywhere else
        A[:, 1] = np.clip(A[:, 1], -50, 50)
        A[M - 1, 1] = 101
        if M >= 2:
            A[M - 2, 1] = -99
        # k-block j contributes exactly 3 (j + 1) to element (0, 0): nonzero, different for every block
        B[0, :K] = 0
        A[0, 64 * np.arange(nk) + 5] = np.arange(nk) + 1
        B[0, 64 * np.arange(nk) + 5] = 3
        if kind == "neg128":
            A[M - 3, :K] = -128
            B[N - 2, :K] = -128
            A[2::7, 9:K:13] = -128
            B[3::5, 4:K:11] = -128
    if scales == "unit":
        a_scale, b_scale = np.ones(M, dtype=np.float32), np.ones(N, dtype=np.float32)
    elif scales == "pow2":
        a_scale = np.exp2(rng.integers(-9, 3, size=M)).astype(np.float32)
        b_scale = np.exp2(rng.integers(-12, -2, size=N)).astype(np.float32)
    else:  # what the quantiser writes: amax / 127 of bf16 rows
        a_scale = (bf16_round(np.abs(rng.standard_normal(M, dtype=np.float32)) * 3 + 0.25) / np.float32(127.0)).astype(np.float32)
        b_scale = (bf16_round(np.abs(rng.standard_normal(N, dtype=np.float32)) * 0.05 + 0.004) / np.float32(127.0)).astype(np.float32)
    bias = (rng.standard_normal(N, dtype=np.float32) * 0.5).astype(np.float32)
    res = bf16_round(rng.standard_normal((M, N), dtype=np.float32))
    case = dict(A=A, B=B, a_scale=a_scale, b_scale=b_scale, bias=bias, res=res, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, kind=kind)
    if kind == "deep":
        # the one case that sees the int -> float rounding.  A bf16 result hides one f32 ulp almost everywhere, so the bias of one
        # column puts one element ON a bf16 tie: acc = 6 (mod 8) in [2^25, 2^26) is an f32 tie that round-to-nearest-even takes UP to
        # acc + 2 (truncation gives acc - 2); with bias = P - (acc + 2), P = 2^25 + 1.5 * 2^18 the midpoint of two bf16 neighbours whose
        # even one is the upper, both sums are exact in f32: P rounds up to 2^25 + 2^19, P - 4 rounds down to 2^25 + 2^18.
        acc = blocks(case).sum(axis=0)
        hit = np.argwhere((acc >= 2 ** 25) & (acc < 2 ** 26) & (acc % 8 == 6))
        assert len(hit), "the deep case has no element on an f32 tie"
        m, n = (int(v) for v in hit[0])
        P = 2 ** 25 + 3 * 2 ** 17
        case["bias"][n] = np.float32(P - (int(acc[m, n]) + 2))
        assert int(case["bias"][n]) == P - (int(acc[m, n]) + 2)
        case["tie"] = (m, n)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def make_case(M, N, K, scales="general", kind="random"):
    """-> dict A int8 [M, lda], B int8 [N, ldb] (columns >= K: POISON), a_scale f32 [M], b_scale f32 [N], bias f32 [N], res bf16 values
    [M, N] (f32), M, N, K, lda, ldb, ldc.  Built once per process and read-only: the reference is shared by the tests."""
    return _make_case(int(M), int(N), int(K), scales, kind)


def blocks(case, unsigned=False):
    """int64 [K / 64, M, N]: the contribution of every 64-wide k-block to every element (cached per case)."""
    key = "_blocks_u8" if unsigned else "_blocks"
    if key not in case:
        K = case["K"]
        A, B = case["A"][:, :K], case["B"][:, :K]
        if unsigned:
            A, B = A.view(np.uint8), B.view(np.uint8)
        A, B = A.astype(np.int64), B.astype(np.int64)
        case[key] = np.stack([A[:, k:k + 64] @ B[:, k:k + 64].T for k in range(0, K, 64)])
    return case[key]


def new_c(case):
    """The C buffer a test hands to the kernel, as f32 values: [M + GUARD_ROWS, ldc] of SENTINEL."""
    return np.full((case["M"] + GUARD_ROWS, case["ldc"]), SENTINEL, dtype=np.float32)


def _to_f32(acc, truncate=False):
    f = acc.astype(np.float32)  # numpy converts int64 -> float32 to nearest, ties to even
    if truncate:
        over = np.abs(f.astype(np.float64)) > np.abs(acc)
        f = np.where(over, np.nextafter(f, np.float32(0.0)), f).astype(np.float32)
    return f


def pre_activation(case, bias=False, mutant=None):
    """The f32 value in front of the GELU / residual / bf16 rounding: exact integer sum, one conversion, three f32 operations."""
    M, N, K = case["M"], case["N"], case["K"]
    c = blocks(case, unsigned=mutant == "unsigned_bytes")
    if mutant == "drop_last_kblock":
        c = c[:-1]
    elif mutant == "first_kblock_twice" and len(c) > 1:
        c = np.concatenate([c[:1], c[:1], c[2:]])
    acc = c.sum(axis=0) if len(c) else np.zeros((M, N), dtype=np.int64)
    if mutant == "pad_column_read":  # K taken from lda
        lda = case["lda"]
        acc = acc + case["A"][:, K:lda].astype(np.int64) @ case["B"][:, K:lda].astype(np.int64).T
    f = _to_f32(acc, truncate=mutant == "truncating_cvt")
    sa, sb = case["a_scale"], case["b_scale"]
    b = case["bias"][None, :] if bias else None
    if mutant == "scales_swapped":  # a_scale indexed by n, b_scale by m
        s = (sa[np.arange(N) % M][None, :] * sb[np.arange(M) % N][:, None]).astype(np.float32)
        v = (f * s).astype(np.float32)
    elif mutant == "scale_one_by_one":
        v = (f * sa[:, None]).astype(np.float32)
        v = (v * sb[None, :]).astype(np.float32)
    elif mutant == "bias_before_scale" and b is not None:
        s = (sa[:, None] * sb[None, :]).astype(np.float32)
        v = (f + b).astype(np.float32)
        return (v * s).astype(np.float32)
    else:
        s = (sa[:, None] * sb[None, :]).astype(np.float32)
        v = (f * s).astype(np.float32)
    if b is not None:
        v = (v + b).astype(np.float32)
    return v


def reference(case, bias=False, gelu=False, res=False, mutant=None):
    """-> the C buffer [M + GUARD_ROWS, ldc] (bf16 values as f32) after the call: SENTINEL wherever the kernel must not write.
    GELU forms: the float64 gelu of the exact f32 pre-activation, rounded once to f32 (the kernel is held to `gelu_bound` there)."""
    M, N = case["M"], case["N"]
    v = pre_activation(case, bias, mutant)
    r = case["res"]
    if mutant == "residual_before_gelu" and res and gelu:
        v = (v + r).astype(np.float32)
        v = _gelu64(v.astype(np.float64)).astype(np.float32)
    else:
        if gelu:
            v = _gelu64(v.astype(np.float64)).astype(np.float32)
        if res:
            v = (v + r).astype(np.float32)
    out = new_c(case)
    rows = M - 1 if mutant == "skip_last_row" else M
    out[:rows, :N] = bf16_round(v)[:rows]
    if mutant == "write_row_M":  # the clamped read of row M - 1, stored one row too far
        out[M, :N] = out[M - 1, :N]
    return out


def ref64(case, bias=False, gelu=False, res=False):
    """float64 evaluation from the operands as given -> (out [M, N], pre [M, N])."""
    acc = blocks(case).sum(axis=0).astype(np.float64)
    pre = acc * (case["a_scale"].astype(np.float64)[:, None] * case["b_scale"].astype(np.float64)[None, :])
    if bias:
        pre = pre + case["bias"].astype(np.float64)[None, :]
    out = _gelu64(pre) if gelu else pre
    if res:
        out = out + case["res"].astype(np.float64)
    return out, pre


def gelu_bound(case, bias=False, res=False):
    """-> (target f64 [M, N]: gelu in float64 of the exact f32 pre-activation (+ residual), bound [M, N] on |kernel - target|)."""
    pre = pre_activation(case, bias).astype(np.float64)
    out = _gelu64(pre)
    if res:
        out = out + case["res"].astype(np.float64)
    e_act = np.abs(pre) * (0.75e-7 + 8 * U32)
    e_out = e_act + U32 * np.abs(out)
    return out, e_out + UBF * (np.abs(out) + e_out) + 1e-30
