"""Exact-arithmetic probes for the GEMM kernels behind nt_plan / tn_plan (csrc/gemm*.hip) and the weight-streaming kernel
(csrc/gemm_stream.hip): operand builders, the fp64 reference with the epilogue order of include/wft.h, the case table with the
kernel kind every case must reach, the plan rules restated for that table, and the ways a tiled GEMM goes wrong restated as wrong
references ("mutants").  CPU only, plain torch; shared by tests/test_gemm_exact_host.py (which proves on the CPU that the builders'
conditions hold and that the comparison fails every mutant) and tests/test_gemm_exact_gpu.py (which holds every kernel kind to it).

Why exact: with small-integer bf16 operands every product and every partial sum is an integer far below 2^24, so an fp32
accumulator holds the true value whatever the k order, split-K plan, ring depth or atomic order, and one bf16 rounding of a
representable value is the identity.  The output must then equal the fp64 reference bit for bit, element by element: a lost or
doubled k-slab, a stale fragment, a bias / residual / aux read one row, column or tile off, a leaked padding row, a split dropped
or added twice each move some element by at least 0.25 and fail torch.equal.

Operands (all seeded; every GPU case runs on two seeds into the same buffers):
  dense integer probe   entries of A and B from {-2 .. 2}, kept with probability min(1, 12 / sqrt(K)) (16 / sqrt(K) from K = 2048 on) where C is bf16 (max|acc|
                        then stays near 100, inside bf16's integers) and always where C is fp32 (TN: a 32-deep slab of a sparse
                        R = 16 421 reduction would be zero in most elements and its loss invisible — the density was raised, not
                        the condition lowered).  The proof of order independence is `sum_k |a| |b| < 2^24`, asserted per case.
  epilogue operands     bias[n] = (37 n mod 61) - 30, residual[m, n] = ((7 m + 13 n) mod 31) - 15, MUL_AUX aux[m, n] =
                        AUX_VALUES[(5 m + 3 n) mod 7]: signed powers of two from 1/8 to 1.  (One significant bit, not up to four:
                        acc x aux must stay a bf16, and |acc| reaches 133 = 8 bits.)  None equals its neighbour at offsets of 1,
                        16, 128, 256 rows or columns (asserted).  alpha in {1, 0.5, -2}, beta in {1, 0.5, -1.5}: -2 and 0.5 ride on
                        the fp32-C form (|-2 acc + bias + 0.5 res| passes 256), 0.5 and -1.5 on a bf16 C.
  gather probe          B (or A) has one-hot rows e_k(n), k(n) = (a n + b) mod K, a coprime to K; the other operand is arbitrary
                        bf16 (randn x 2^randint(-8, 8)): C[m, n] = A[m, k(n)] exactly, for bf16 and fp32 C.  Where the output has
                        fewer rows / columns than K the probe runs in rounds (n + round x N) until every k has been selected.  TN:
                        one-hot columns over R.
  poison                operands live inside larger allocations: rows >= M of A, residual and aux, columns K .. lda of A and B,
                        rows >= R of both TN operands hold 3 (finite: a leak is a wrong integer, never a NaN that a masking
                        multiply could launder); outputs have ldc > N and guard rows of a sentinel bit pattern.
GELU forms cannot be exact; they are held per element to |got - ref| <= 2^-8 |ref| + GELU_C (1 + |pre|) (DGELU: second term x |acc|)
against fp64 erf, the pre-activation taken as the kernels take it, fl32(alpha acc + bias).

GELU_C = 2^-20: measured by tests/test_gemm_exact_host.py on the GELU cases' own pre-activations as the worst
|fp32 restatement of gelu_f / dgelu_f / gelu_both_f - fp64| / (1 + |pre|) = 2.8e-7, doubled (hardware rcp / exp2, which the CPU
restatement does not model) and rounded up to a power of two; that test asserts this docstring's number.  Never from a kernel.

Shapes: the issue's, derived from the plan rules for 256 CUs; tests/test_gemm_exact_host.py pins every one to its kind through the
library's public queries.  Changed from the issue's list: none of the NT shapes; see TN_CASES for the TN ones.
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NCU = 256                  # the library's no-device assumption and the MI355X's count
POISON = 3.0
SEEDS = (0, 1)
GELU_C = 2.0 ** -20        # see the docstring; asserted by tests/test_gemm_exact_host.py
AUX_VALUES = (1.0, -0.5, 0.25, -0.25, 0.5, -0.125, -1.0)
NEIGHBOURS = (1, 16, 128, 256)
INV_SQRT2 = 0.70710678118654752440


# ------------------------------------------------------------------------------------------------ forms
@dataclass(frozen=True)
class Form:
    """one epilogue form of wft_gemm_nt_bf16"""
    name: str
    bias: str = ""             # "" / "int" (the probe's bias) / "randn" (GELU forms)
    residual: bool = False
    epilogue: str = "none"     # none / gelu / dgelu / gelu_grad / mul_aux
    alpha: float = 1.0
    beta: float = 1.0
    res_first: bool = False
    c_f32: bool = False
    accumulate: bool = False
    colsum: str = ""           # "" / "fused" (workspace granted) / "pass" (no workspace: wft_colsum_bf16 over C)
    valid: Optional[tuple] = None   # (period, valid_rows)
    aux_out: bool = False      # EPI_GELU: store the pre-activation

    @property
    def exact(self):
        return self.epilogue in ("none", "mul_aux")


FORMS = {f.name: f for f in (
    Form("plain"),
    Form("half", alpha=0.5),
    Form("bias", bias="int"),
    Form("bias_res", bias="int", residual=True),
    Form("alpha_beta_res", bias="int", residual=True, alpha=0.5, beta=-1.5),
    Form("mul_aux", epilogue="mul_aux"),
    Form("mul_aux_colsum_fused", epilogue="mul_aux", colsum="fused"),
    Form("mul_aux_colsum_pass", epilogue="mul_aux", colsum="pass"),
    Form("colsum", colsum="fused"),
    Form("colsum_res", residual=True, colsum="fused"),
    Form("res_first_mul_aux", residual=True, epilogue="mul_aux", alpha=0.5, res_first=True),
    Form("valid_rows", bias="int", residual=True, valid=(50, 47)),
    Form("f32", bias="int", residual=True, alpha=-2.0, beta=0.5, c_f32=True),
    Form("f32_acc", c_f32=True, accumulate=True),
    Form("gelu_grad", bias="randn", epilogue="gelu_grad", alpha=0.0625),
    Form("gelu_aux", bias="randn", epilogue="gelu", alpha=0.0625, aux_out=True),
    Form("dgelu", epilogue="dgelu"),
    # the streaming kernel takes alpha = 1 only
    Form("s_gelu", bias="randn", epilogue="gelu"),
    Form("s_gelu_aux", bias="randn", epilogue="gelu", aux_out=True),
)}
F4W = ("plain", "bias", "bias_res", "alpha_beta_res", "mul_aux", "mul_aux_colsum_fused", "mul_aux_colsum_pass", "gelu_grad")
F256_ONLY = ("colsum", "colsum_res", "res_first_mul_aux", "valid_rows", "f32", "f32_acc", "gelu_aux", "dgelu")
F128 = ("plain", "bias", "bias_res", "alpha_beta_res", "mul_aux", "mul_aux_colsum_pass", "res_first_mul_aux", "valid_rows", "f32", "f32_acc",
        "gelu_grad", "gelu_aux", "dgelu")


# ------------------------------------------------------------------------------------------------ the plan rules, restated
def nt_plan(M, N, K, batch=1, form=FORMS["plain"], variant=0, p_valid=0, lda=None, ncu=NCU, splitk_ws=True):
    """-> (kind, wft_gemm_nt_variant's answer, wft_gemm_nt_splitk_workspace_bytes' answer): nt_plan of csrc/gemm.hip over the rules
    beside each kernel, for operands with the alignment this module's buffers have."""
    lda = K if lda is None else lda
    if N % 256 == 0 and M >= 1024 and -(-M // 256) * (N // 256) * batch >= 128:
        epi_ok = form.epilogue == "none" or (form.epilogue in ("gelu_grad", "mul_aux") and not form.residual)
        cs_ok = not form.colsum or form.epilogue == "mul_aux"
        elig = (epi_ok and cs_ok and not form.c_f32 and not form.accumulate and K % 128 == 0 and K >= 256 and lda >= K and form.valid is None
                and not form.res_first)
        return ("NT_4W", 4, 0) if (elig and variant == 0) else ("NT_256", 256, 0)
    plain = (form.epilogue == "none" and not form.bias and not form.residual and not form.colsum and form.valid is None and not form.c_f32)
    if N == 128 and batch == 1 and 0 < p_valid <= 64 and plain:
        return "NT_RANK", 128, 0
    tiles = -(-M // 128) * (N // 128)
    kind = "NT_128_RING" if tiles * batch <= ncu else "NT_128_2BUF"
    nk, bytes_ = K // 64, 0
    if plain and batch == 1 and p_valid == 0 and N != 128 and tiles * 2 <= ncu and nk >= 64:
        nsplit = min(ncu // tiles, nk // 16)
        per = -(-nk // nsplit)
        nsplit = -(-nk // per)
        if nsplit > 1:
            bytes_ = nsplit * M * N * 4
            if splitk_ws:
                kind = "NT_128_SPLITK"
    return kind, 128, bytes_


def nt_splits(M, N, K, ncu=NCU):
    """the k ranges of the NT split-K plan: [(k0, k1)]"""
    nk = K // 64
    nsplit = min(ncu // (-(-M // 128) * (N // 128)), nk // 16)
    per = -(-nk // nsplit)
    return [(64 * s * per, min(K, 64 * (s + 1) * per)) for s in range(-(-nk // per))]


def _fill(tiles_x_sp_over, lo, cap, enough):
    best, nsplit = 0.0, 1
    for sp in range(1, cap + 1):
        if sp > 1 and not enough(sp):
            break
        waves = tiles_x_sp_over(sp)
        eff = waves / int(waves + 0.999999)
        if eff > best + lo:
            best, nsplit = eff, sp
    return nsplit


def tn_plan(R, P, Q, batch=1, c_f32=True, variant=0, p_valid=0, reduce_form=False, segs=0, workspace=True, ncu=NCU):
    """-> dict(kind, nsplit, ws_bytes, variant): tn_plan of csrc/gemm.hip.  `workspace`: the workspace asked for is granted."""
    nsteps = -(-R // 64) * batch
    t256 = (P // 256) * (Q // 256)
    if c_f32 and P % 256 == 0 and Q % 256 == 0 and nsteps >= 64 and (nsteps >= 256 or t256 >= 50 or (t256 >= 25 and nsteps >= 128)):
        nslabs = -(-R // 32) * batch
        ns256 = _fill(lambda sp: t256 * sp / ncu, 0.02, 16, lambda sp: nslabs // sp >= 48)
        per = -(-nslabs // ns256)
        ns256 = -(-nslabs // per)
        elig4 = batch == 1 and R >= 1024 and p_valid == 0 and not reduce_form
        ns4 = 0
        if elig4:
            nk = (-(-R // 64) + 1) // 2 * 2
            ns4 = _fill(lambda sp: t256 * sp / ncu, 0.02, 16, lambda sp: nk // sp >= 24)
            per = max(4, (-(-nk // ns4) + 1) & ~1)
            ns4 = -(-nk // per)
            while ns4 > 1 and nk - (ns4 - 1) * per < 4:
                per += 2
                ns4 = -(-nk // per)
        nsq = max(ns4, ns256)
        ws = nsq * P * Q * 4 if (nsq > 1 or segs or reduce_form) else 0
        if elig4 and variant == 0 and (ns4 == 1 or ((ns4 > 1 or segs) and workspace)):
            return dict(kind="TN_4W", nsplit=ns4, ws_bytes=ws, variant=4)
        return dict(kind="TN_256", nsplit=ns256, ws_bytes=ws, variant=256)
    tiles = (P // 128) * (Q // 128)
    ring = c_f32 and P != 128 and not reduce_form and tiles <= ncu and (tiles <= 32 or nsteps <= 32)
    if not c_f32:
        nsplit = 1
    elif ring:
        sp = max(1, min(ncu // tiles, nsteps // 4))
        per = -(-nsteps // sp)
        nsplit = -(-nsteps // per)
    else:
        nsplit = _fill(lambda sp: tiles * sp / 512.0, 0.03, 64, lambda sp: nsteps // sp >= (16 if sp <= 8 else 12))
        per = -(-nsteps // nsplit)
        nsplit = -(-nsteps // per)
    pb = (p_valid + 15) // 16 if (c_f32 and P == 128 and 0 < p_valid <= 64) else 0
    rows = 16 * pb if pb else P
    want = nsplit > 1 or reduce_form
    ws = nsplit * rows * Q * 4 if (want or segs) else 0
    use_ws = want and workspace
    if pb and (nsplit == 1 or use_ws):
        kind = "TN_RANK"
    elif not c_f32:
        kind = "TN_128_BF16C"
    elif pb:
        kind = "TN_128_PB"
    else:
        kind = "TN_128_RING" if ring else "TN_128_2BUF"
    return dict(kind=kind, nsplit=nsplit, ws_bytes=ws, variant=128)


# ------------------------------------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class NtCase:
    name: str
    kind: str                  # the kind the case's first form reaches with variant 0 and the split-K workspace granted
    M: int
    N: int
    K: int
    forms: tuple               # reach `kind` (under variant 1: NT_256 where kind is NT_4W)
    forms256: tuple = ()       # reach NT_256 whatever the variant (only where kind is NT_4W / NT_256)
    batch: int = 1
    windows: bool = False      # lda = K / 3: overlapping rows (conv windows)
    launches: tuple = (0,)
    p_valid: tuple = (0,)
    answers: tuple = (128, 0)  # recorded: wft_gemm_nt_variant, wft_gemm_nt_splitk_workspace_bytes of the first form

    @property
    def lda(self):
        return self.K // 3 if self.windows else self.K + 8


NT_CASES = (
    # 144 tiles, one per workgroup; a ragged 40-row last tile; K at the one-wave-per-SIMD kernel's minimum
    NtCase("4w-one-tile-each", "NT_4W", 2048 + 40, 4096, 256, F4W, answers=(4, 0)),
    # 297 tiles > 256 CUs: workgroups cross tile seams; 9 column tiles = a band of 5 and one of 4; three 128-deep steps
    NtCase("4w-persistent", "NT_4W", 8192 + 200, 2304, 384, F4W, F256_ONLY[:4], launches=(0, 1), answers=(4, 0)),
    NtCase("256-short-k", "NT_256", 1024 + 3, 8192, 64, F4W + F256_ONLY, answers=(256, 0)),
    NtCase("256-odd-k", "NT_256", 1100, 8192, 192, ("plain", "bias_res", "mul_aux_colsum_fused", "gelu_grad"), answers=(256, 0)),
    # batch 3, lda > K, ldc > N, strideB = 0: 5 x 11 x 3 = 165 tiles
    NtCase("4w-batched", "NT_4W", 1024 + 24, 2816, 256, ("plain", "bias_res", "alpha_beta_res", "mul_aux", "gelu_grad"), ("f32", "valid_rows"),
           batch=3, answers=(4, 0)),
    # M < 1024 keeps the 256 kernels out; 8 x 34 = 272 tiles
    NtCase("128-2buf", "NT_128_2BUF", 1000, 4352, 192, F128),
    NtCase("128-2buf-windows", "NT_128_2BUF", 1000, 4352, 192, ("plain", "valid_rows", "bias_res"), batch=2, windows=True),
    NtCase("128-ring", "NT_128_RING", 130, 384, 192, F128),
    NtCase("128-ring-smallest", "NT_128_RING", 1, 128, 64, F128),
    # 4 tiles, 4 splits of 16 k-steps
    NtCase("128-splitk", "NT_128_SPLITK", 133, 256, 4096, ("plain", "half"), answers=(128, 4 * 133 * 256 * 4)),
    NtCase("rank", "NT_RANK", 300, 128, 128, ("plain",), p_valid=(8, 16, 33, 64)),
)


@dataclass(frozen=True)
class TnCase:
    name: str
    kind: str
    R: int
    P: int
    Q: int
    forms: tuple = ("plain", "acc")
    batch: int = 1
    variant: int = 0
    workspace: bool = True     # False: the workspace is cleared from the arguments (the atomic path / TN_128_PB)
    p_valid: tuple = (0,)
    c_f32: bool = True
    answers: tuple = (0, 128, 128)   # recorded: workspace bytes, variant without / with the workspace granted

    def ragged(self):
        """the same case with R % 64 in {1, 31, 33, 63}, where the restated plan keeps the kind"""
        out = []
        for r in (1, 31, 33, 63):
            R = self.R // 64 * 64 + r
            if R != self.R and all(_tn_kind(self, R, pv) == _tn_kind(self, self.R, pv) for pv in self.p_valid):
                out.append(R)
        return out


def _tn_kind(c, R, pv, reduce_form=False):
    return tn_plan(R, c.P, c.Q, c.batch, c.c_f32, c.variant, pv, reduce_form, 0, c.workspace)["kind"]


TN_CASES = (
    TnCase("4w-square", "TN_4W", 16384 + 37, 256, 256, answers=(6 * 256 * 256 * 4, 256, 4)),
    TnCase("256-square", "TN_256", 16384 + 37, 256, 256, variant=1, answers=(6 * 256 * 256 * 4, 256, 256)),
    TnCase("256-atomic", "TN_256", 16384 + 37, 256, 256, workspace=False, answers=(6 * 256 * 256 * 4, 256, 4)),
    TnCase("4w-wide", "TN_4W", 4096 + 1, 1280, 2560, answers=(2 * 1280 * 2560 * 4, 256, 4)),
    TnCase("256-wide", "TN_256", 4096 + 1, 1280, 2560, variant=1, answers=(2 * 1280 * 2560 * 4, 256, 256)),
    TnCase("256-batched", "TN_256", 2100, 1280, 2560, ("plain",), batch=2, answers=(2 * 1280 * 2560 * 4, 256, 256)),
    TnCase("4w-segments", "TN_4W", 16384, 768, 256, ("seg3", "seg3_acc"), answers=(10 * 768 * 256 * 4, 256, 4)),
    TnCase("128-2buf", "TN_128_2BUF", 2100 + 33, 640, 1152, answers=(2 * 640 * 1152 * 4, 128, 128)),
    TnCase("128-ring", "TN_128_RING", 437, 256, 384),
    TnCase("128-ring-split", "TN_128_RING", 1024 + 1, 512, 512, answers=(4 * 512 * 512 * 4, 128, 128)),
    TnCase("128-ring-one-row", "TN_128_RING", 1, 256, 256),
    TnCase("128-bf16c", "TN_128_BF16C", 437, 256, 384, ("plain",), c_f32=False),
    TnCase("rank", "TN_RANK", 3001, 128, 384, ("plain", "acc", "col_scale", "block", "pair"), p_valid=(8, 33, 64)),
    # (3001 rows are ONE split on 3 tiles: the plan never leaves the rank kernel there.  6 144 + 57 rows make 6 splits.)
    TnCase("rank-split", "TN_RANK", 6144 + 57, 128, 384, ("plain", "acc", "col_scale", "block", "pair"), p_valid=(8, 33, 64), answers=(6 * 16 * 384 * 4, 128, 128)),
    TnCase("128-pb", "TN_128_PB", 6144 + 57, 128, 384, ("plain", "acc"), workspace=False, p_valid=(8, 33, 64), answers=(6 * 16 * 384 * 4, 128, 128)),
)

STREAM_CASES = tuple((M, N, K) for N, K in ((384, 1536), (1152, 384)) for M in (1, 5, 32))
STREAM_FORMS = ("plain", "bias", "bias_res", "s_gelu", "s_gelu_aux")
NT_KINDS = ("NT_4W", "NT_256", "NT_RANK", "NT_128_SPLITK", "NT_128_RING", "NT_128_2BUF")
TN_KINDS = ("TN_4W", "TN_256", "TN_RANK", "TN_128_PB", "TN_128_RING", "TN_128_2BUF", "TN_128_BF16C")


def nt_runs(c):
    """(form name, variant, launch mode, p_valid, kind that run must reach) of one NT case"""
    out = []
    for pv in c.p_valid:
        for launch in c.launches:
            for variant in ((0, 1) if c.kind == "NT_4W" else (0,)):
                for f in c.forms + c.forms256:
                    kind = nt_plan(c.M, c.N, c.K, c.batch, FORMS[f], variant, pv, c.lda)[0]
                    if variant == 1 and f in c.forms256:
                        continue       # NT_256 already under variant 0
                    out.append((f, variant, launch, pv, kind))
    return out


# ------------------------------------------------------------------------------------------------ operand builders
def density(K):
    """12 / sqrt(K); 16 / sqrt(K) from K = 2048 on, where 12 left a 32-deep slab of some 16 x 16 block zero in four fifths of its
    elements (the slab condition of tests/test_gemm_exact_host.py) — the forms that run that deep have no epilogue to overflow"""
    return min(1.0, (12.0 if K < 2048 else 16.0) / math.sqrt(K))


def _gen(seed, *dims):
    return torch.Generator().manual_seed(1000003 * seed + sum(int(d) * w for d, w in zip(dims, (1009, 31, 7, 3))) + 17)


def dense_int(shape, p, g):
    """fp32 integers from {-2 .. 2}, each kept with probability p"""
    v = torch.randint(-2, 3, shape, generator=g).float()
    return v if p >= 1.0 else v * (torch.rand(shape, generator=g) < p)


def arbitrary(shape, g):
    """bf16-exact fp32 values randn x 2^randint(-8, 8): every one normal and nonzero"""
    v = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-8, 9, shape, generator=g).float())
    v = v.to(BF).float()
    assert ((v != 0).float().mean() >= 0.5) and torch.isfinite(v).all() and (v[v != 0].abs() >= 2.0 ** -126).all()
    return v


def bias_vec(N):
    return ((37 * torch.arange(N)) % 61 - 30).float()


@functools.lru_cache(maxsize=8)
def residual_mat(b, M, N):
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    return ((7 * m + 13 * n + 5 * b) % 31 - 15).float()


@functools.lru_cache(maxsize=8)
def aux_mat(b, M, N):
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    return torch.tensor(AUX_VALUES)[(5 * m + 3 * n + 2 * b) % 7]


def assert_distinct_neighbours(x):
    """no entry equals its neighbour at offsets of 1, 16, 128 or 256 along any dimension"""
    for d in range(x.dim()):
        for off in NEIGHBOURS:
            if off < x.shape[d]:
                assert (x.narrow(d, off, x.shape[d] - off) != x.narrow(d, 0, x.shape[d] - off)).all(), (d, off)


def is_bf16(x):
    return torch.equal(x.to(BF).to(x.dtype), x)


def coprime_step(K, seed):
    a = (K // 3 + 7 * seed) | 1
    while math.gcd(a, K) != 1:
        a += 2
    return a % K if K > 1 else 1


def gather_sel(n_out, K, seed, round_, salt):
    """the k that output row / column n of round `round_` selects: (a (n + round n_out) + b) mod K, a coprime to K"""
    return (coprime_step(K, seed) * (torch.arange(n_out) + round_ * n_out) + 11 * seed + salt) % K


def pad_rows(M, tile=256):
    return (-M) % tile + 8


@dataclass
class NtOps:
    """operands of one NT case and seed; `*_buf` are the allocations (poisoned), A / B the logical fp32 values [batch, M, K] / [nb, N, K]"""
    A: torch.Tensor
    B: torch.Tensor
    A_buf: torch.Tensor
    B_buf: torch.Tensor
    lda: int
    ldb: int
    strideA: int
    strideB: int
    probe: str = "dense"
    sel: Optional[torch.Tensor] = None    # gather: the k each output column (B one-hot) or row (A one-hot) selects


def nt_operands(c, seed, probe="dense", round_=0):
    """probe: dense / gather_b (B one-hot) / gather_a (A one-hot)"""
    M, N, K, batch = c.M, c.N, c.K, c.batch
    g = _gen(seed, M, N, K, {"dense": 0, "gather_b": 1, "gather_a": 2}[probe])   # (the arbitrary operand is the same in every round)
    nb = 1   # strideB = 0: one weight for every batch entry
    p, sel = density(K), None
    if c.windows:   # A is a signal: row m = signal[m lda : m lda + K]
        lda = c.lda
        L = (M - 1) * lda + K
        sig = torch.full((batch, L + pad_rows(M) * lda), POISON)   # (the rows of a ragged last tile stay inside the allocation)
        sig[:, :L] = dense_int((batch, L), p, g) if probe == "dense" else arbitrary((batch, L), g)
        A = sig.unfold(1, K, lda)[:, :M].contiguous()
        A_buf, strideA = sig, sig.shape[1]
    else:
        A = None
    if probe == "dense":
        if A is None:
            A = dense_int((batch, M, K), p, g)
        B = dense_int((nb, N, K), p, g)
    elif probe == "gather_b":
        if A is None:
            A = arbitrary((batch, M, K), g)
        sel = gather_sel(N, K, seed, round_, 3)
        B = torch.zeros(nb, N, K)
        B[0, torch.arange(N), sel] = 1.0
    else:
        assert not c.windows
        sel = gather_sel(batch * M, K, seed, round_, 5)
        A = torch.zeros(batch * M, K)
        A[torch.arange(batch * M), sel] = 1.0
        A = A.view(batch, M, K)
        B = arbitrary((nb, N, K), g)
    if not c.windows:
        rows = M + pad_rows(M)
        A_buf = torch.full((batch, rows, c.lda), POISON)
        A_buf[:, :M, :K] = A
        strideA = rows * c.lda
    ldb = K + 8
    B_buf = torch.full((nb, N, ldb), POISON)
    B_buf[:, :, :K] = B
    assert is_bf16(A) and is_bf16(B)
    if probe == "dense":   # every partial sum in every order is an integer below 2^24
        assert float((A.abs().sum(-1).amax() * B.abs().amax())) < 2 ** 24
    return NtOps(A, B, A_buf.to(BF), B_buf.to(BF), c.lda, ldb, strideA, 0, probe, sel)


def stream_case(M, N, K):
    return NtCase(f"stream-{M}x{N}x{K}", "stream", M, N, K, STREAM_FORMS)


def stream_operands(M, N, K, seed):
    """dense operands of a streaming-kernel case and the epilogue operands its forms share (randn bias, integer residual)"""
    c = stream_case(M, N, K)
    e = nt_epilogue_operands(c, FORMS["s_gelu_aux"], seed)
    e.res = nt_epilogue_operands(c, FORMS["bias_res"], seed).res
    return nt_operands(c, seed), e


def gather_rounds(n_out, K):
    return -(-K // n_out)


@dataclass
class Epi:
    """epilogue operands of one (case, form, seed): logical fp32 values; res / aux carry one poison row behind row M"""
    bias: Optional[torch.Tensor] = None     # [N]
    res: Optional[torch.Tensor] = None      # [batch, M + 1, N]
    aux: Optional[torch.Tensor] = None      # [batch, M + 1, N]  (input of MUL_AUX / DGELU)
    base: Optional[torch.Tensor] = None     # [batch, M, N] integer base of an accumulating fp32 C


def nt_epilogue_operands(c, form, seed):
    M, N, batch = c.M, c.N, c.batch
    g = _gen(seed, M, N, 99)
    e = Epi()
    if form.bias == "int":
        e.bias = bias_vec(N)
        assert_distinct_neighbours(e.bias)
    elif form.bias == "randn":
        e.bias = torch.randn(N, generator=g)
    rows = lambda fn: torch.stack([torch.cat([fn(b, M, N), torch.full((1, N), POISON)]) for b in range(batch)])  # noqa: E731
    if form.residual:
        e.res = rows(residual_mat)
        assert_distinct_neighbours(e.res[:, :M])
    if form.epilogue == "mul_aux":
        e.aux = rows(aux_mat)
        assert_distinct_neighbours(e.aux[:, :M])
    elif form.epilogue == "dgelu":   # saved pre-activations: bf16 values over the whole GELU curve
        e.aux = torch.cat([(2.5 * torch.randn(batch, M, N, generator=g)).to(BF).float(), torch.full((batch, 1, N), POISON)], 1)
    if form.accumulate:
        e.base = torch.randint(-1000, 1001, (batch, M, N), generator=g).float()
    return e


# ------------------------------------------------------------------------------------------------ GELU, as fp64 and as the kernels' fp32
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * INV_SQRT2))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x * INV_SQRT2)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _fma(a, b, c):
    c = c if isinstance(c, torch.Tensor) else torch.tensor(c, dtype=F32)
    b = b if isinstance(b, torch.Tensor) else torch.tensor(b, dtype=F32)
    return (a.double() * b.double() + c.double()).float()


def _f(v):
    return torch.tensor(v, dtype=F32)


def _poly(t, c5, c4, c3, c2, c1):
    p = _fma(t, _f(c5), _f(c4))
    for c in (c3, c2, c1):
        p = _fma(p, t, _f(c))
    return p


def gelu_f32(x):
    """gelu_f of csrc/common.h (through erf_fast), restated in torch fp32"""
    ax = x.abs() * _f(INV_SQRT2)
    xs = x * _f(INV_SQRT2)
    t = torch.reciprocal(_fma(ax, _f(0.3275911), _f(1.0)))
    poly = _poly(t, 1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)
    y = 1.0 - poly * t * torch.exp(-ax * ax)
    return 0.5 * x * (1.0 + torch.copysign(y, xs))


def dgelu_f32(x):
    """dgelu_f of csrc/common.h"""
    ax = x.abs() * _f(INV_SQRT2)
    t = torch.reciprocal(_fma(ax, _f(0.3275911), _f(1.0)))
    e = torch.exp2(x * x * _f(-0.72134752044448170368))
    poly = _poly(t, 1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)
    half_erfc = 0.5 * poly * t * e
    cdf = torch.where(x >= 0, 1.0 - half_erfc, half_erfc)
    return _fma(x, _f(0.39894228040143267794) * e, cdf)


def gelu_both_f32(x):
    """gelu_both_f of csrc/common.h -> (gelu, gelu')"""
    t = torch.reciprocal(_fma(x.abs(), _f(0.23164189), _f(1.0)))
    xs = x * _f(0.84932180)
    e = torch.exp2(-(xs * xs))
    poly = _poly(t, 0.5307027145, -0.7265760135, 0.7107068705, -0.142248368, 0.127414796)
    half_erfc = poly * t * e
    cdf = torch.where(x >= 0, 1.0 - half_erfc, half_erfc)
    return x * cdf, _fma(x, _f(0.39894228040143267794) * e, cdf)


def gelu_bound(ref, pre, scale=None):
    """the per-element bound on |got - ref|"""
    b = GELU_C * (1.0 + pre.abs().double())
    if scale is not None:
        b = b * scale.abs().double()
    return 2.0 ** -8 * ref.abs() + b


# ------------------------------------------------------------------------------------------------ reference
def nt_acc(ops, device="cpu"):
    """fp64 [batch, M, N]"""
    return torch.matmul(ops.A.to(device).double(), ops.B.to(device).double().transpose(-1, -2))


def nt_expected(form, acc, e, mut=None, row0=0):
    """The documented epilogue order on the fp64 accumulator: alpha acc (+bias) (residual if residual_first) (epilogue)
    (+beta residual), valid_rows zeroing last, then the column sums of the C written.  `e` on acc's device.  `mut`: one fault.
    row0: acc and e hold rows row0 .. of the case (valid_rows counts from the case's first row).
    -> dict: C (fp64, before the output rounding), bound (None: exact), aux (stored pre-activation / gelu'), aux_bound, colsum"""
    mut = mut or {}
    batch, M, N = acc.shape
    dev = acc.device
    on = lambda t: None if t is None else t.to(dev)  # noqa: E731
    bias, res, aux, base = on(e.bias), on(e.res), on(e.aux), on(e.base)
    out = {"bound": None, "aux": None, "aux_bound": None, "colsum": None}
    row = slice(1, M + 1) if mut.get("row_shift") else slice(0, M)
    v = form.alpha * acc
    if bias is not None:
        sh = mut.get("bias_shift", 0)
        v = v + (torch.roll(bias, -sh) if sh else bias).double()
    if form.epilogue in ("gelu", "gelu_grad"):
        v = v.float()          # what the kernels hand to gelu: fl32(alpha acc + bias)
    beta = 1.0 if mut.get("beta_one") else form.beta
    res_first = form.res_first and not mut.get("ignore_res_first")
    if res is not None and res_first:
        v = v + beta * res[:, row].double()
    if form.epilogue == "gelu":
        if form.aux_out:
            out["aux"] = v.to(BF).double()
        out["bound"] = gelu_bound(gelu64(v.double()), v)
        v = gelu64(v.double())
    elif form.epilogue == "gelu_grad":
        out["aux"] = dgelu64(v.double())
        out["aux_bound"] = gelu_bound(out["aux"], v)
        out["bound"] = gelu_bound(gelu64(v.double()), v)
        v = gelu64(v.double())
    elif form.epilogue == "dgelu":
        x = aux[:, row].double()
        out["bound"] = gelu_bound(v * dgelu64(x), x, scale=v)
        v = v * dgelu64(x)
    elif form.epilogue == "mul_aux":
        v = v * aux[:, row].double()
    if res is not None and not res_first:
        v = v + beta * res[:, row].double()
    if form.valid is not None:
        period, valid = form.valid
        valid += mut.get("valid_shift", 0)
        v = torch.where((((torch.arange(M, device=dev) + row0) % period) >= valid)[None, :, None], torch.zeros_like(v), v)
    if form.colsum:
        out["colsum"] = v[0].sum(0)
    if base is not None:
        v = v + base.double()
    out["C"] = v
    return out


def assert_nt_representable(form, want):
    """what the exactness argument needs of the final value of an exact form"""
    v = want["C"]
    if form.c_f32:
        assert torch.equal(v.float().double(), v) and v.abs().max() < 2 ** 24
        return
    assert torch.equal(v.to(BF).double(), v), "a reference value is not its own bf16 rounding"
    # |value| <= 256 for integers, < 128 for the rest (half-integers; MUL_AUX's quarters and eighths are held by the line above)
    whole = v == v.round()
    assert v.abs().max() <= 256 and (whole.all() or v[~whole].abs().max() < 128)
    if want["colsum"] is not None:
        assert torch.equal(want["colsum"].float().double(), want["colsum"])


# ------------------------------------------------------------------------------------------------ TN
@dataclass
class TnOps:
    A: torch.Tensor            # [batch, R, P] logical fp32
    B: torch.Tensor            # [batch, R, Q]
    A_buf: torch.Tensor        # bf16 [batch, R + pad, lda]: rows >= R and columns >= P hold POISON
    B_buf: torch.Tensor
    lda: int
    ldb: int
    strideA: int
    strideB: int
    sel: Optional[torch.Tensor] = None


TN_PAD = 136    # rows behind R inside the allocation: two 64-row steps and a little


def tn_operands(c, R, seed, probe="dense", round_=0, p_valid=0):
    P, Q, batch = c.P, c.Q, c.batch
    g = _gen(seed, R, P, Q, {"dense": 0, "gather_a": 1, "gather_b": 2}[probe])
    p, sel = (1.0 if c.c_f32 else density(R * batch)), None
    if probe == "dense":
        A, B = dense_int((batch, R, P), p, g), dense_int((batch, R, Q), p, g)
    elif probe == "gather_a":   # one-hot columns over R: C[p, q] = B[r(p), q]
        assert batch == 1
        sel = gather_sel(P, R, seed, round_, 3)
        A = torch.zeros(1, R, P)
        A[0, sel, torch.arange(P)] = 1.0
        B = arbitrary((1, R, Q), g)
    else:
        assert batch == 1
        sel = gather_sel(Q, R, seed, round_, 5)
        B = torch.zeros(1, R, Q)
        B[0, sel, torch.arange(Q)] = 1.0
        A = arbitrary((1, R, P), g)
    if p_valid:    # a rank-r operand: columns >= p_valid of A are zero padding
        A[:, :, p_valid:] = 0.0
    lda, ldb, rows = P + 8, Q + 8, R + TN_PAD
    A_buf, B_buf = torch.full((batch, rows, lda), POISON), torch.full((batch, rows, ldb), POISON)
    A_buf[:, :R, :P], B_buf[:, :R, :Q] = A, B
    assert is_bf16(A) and is_bf16(B)
    if probe == "dense":
        assert 4.0 * R * batch < 2 ** 24
    return TnOps(A, B, A_buf.to(BF), B_buf.to(BF), lda, ldb, rows * lda, rows * ldb, sel)


def tn_acc(ops, device="cpu", extra_row=False):
    """fp64 [P, Q], the batch summed as extra reduction.  extra_row: the mutant that admits row R (poison) into the reduction."""
    A, B = ops.A.to(device).double(), ops.B.to(device).double()
    acc = torch.einsum("brp,brq->pq", A, B)
    return acc + POISON * POISON if extra_row else acc


def col_scale_mat(S, Q):
    """dyadic scales in {0, 0.5, 1, 1.25, 2}: f32 [S, Q]"""
    s, q = torch.arange(S)[:, None], torch.arange(Q)[None, :]
    return torch.tensor((1.25, 0.0, 2.0, 0.5, 1.0))[(3 * s + 2 * q) % 5]


def tn_expected(form, acc, p_valid=0, base=None, scale=None, scale_rows=0, block=None, alpha=1.0, mut=None):
    """acc fp64 [P, Q] -> what the output buffer holds (fp64).  plain / acc: [P, Q]; col_scale: [p_valid, Q]; block: flat
    Q / block_n blocks [block_n, block_r] (the transposed diagonal blocks)."""
    mut = mut or {}
    v = alpha * acc
    if form == "col_scale":
        rows = torch.arange(p_valid, device=acc.device) // scale_rows if scale_rows else torch.zeros(p_valid, dtype=torch.long, device=acc.device)
        return v[:p_valid] * scale.to(acc.device).double()[rows]
    if form == "block":
        bn, br = block
        blocks = [v[i * br:(i + 1) * br, i * bn:(i + 1) * bn] for i in range(acc.shape[1] // bn)]
        return torch.cat([(b if mut.get("no_transpose") else b.t()).reshape(-1) for b in blocks])
    if base is not None:
        v = v + base.to(acc.device).double()
        if p_valid:   # accumulation leaves the padding rows of a rank-r operand alone (their products are sums of zeros anyway)
            pass
    return v


def tn_splits(R, nsplit, step=64):
    """reduction row ranges of a split-K plan of `nsplit` non-empty splits"""
    nsteps = -(-R // step)
    per = -(-nsteps // nsplit)
    return [(step * s * per, min(R, step * (s + 1) * per)) for s in range(-(-nsteps // per))]


# ------------------------------------------------------------------------------------------------ mutants (on the accumulator)
def slab_delta_counts(X, Y, slab=32, block=16):
    """X [M, K], Y [N, K] fp32 integers -> for every 32-deep k-slab the fewest elements in which one 16 x 16 output block changes when
    the slab is dropped (or counted twice): min over blocks of count(delta != 0), min over slabs.  Ragged edge blocks count
    proportionally: returned is the minimum FRACTION of a block's elements that move."""
    M, K = X.shape
    N = Y.shape[0]
    worst = 1.0
    ones_m = torch.zeros(-(-M // block), M)
    ones_m[torch.arange(M) // block, torch.arange(M)] = 1.0
    ones_n = torch.zeros(N, -(-N // block))
    ones_n[torch.arange(N), torch.arange(N) // block] = 1.0
    size = ones_m.sum(1)[:, None] * ones_n.sum(0)[None, :]
    for k0 in range(0, K, slab):
        d = (X[:, k0:k0 + slab] @ Y[:, k0:k0 + slab].t()) != 0
        worst = min(worst, float(((ones_m @ d.float() @ ones_n) / size).min()))
    return worst


def drop_slab(acc2d, X, Y, bi, bj, k0, factor=-1.0, slab=32, block=16):
    """acc2d [M, N] with slab k0 of output block (bi, bj) dropped (factor -1) or counted twice (+1)"""
    out = acc2d.clone()
    r, c = slice(bi * block, (bi + 1) * block), slice(bj * block, (bj + 1) * block)
    out[r, c] += factor * (X[r, k0:k0 + slab].double() @ Y[c, k0:k0 + slab].double().t())
    return out


# ------------------------------------------------------------------------------------------------ comparison
def first_wrong(got, want, tile, what):
    """message for an exact comparison that failed: count, first wrong (m, n), its tile and 16 x 16 block, got / want"""
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    bad = (got != want) | torch.isnan(got)
    m, n = bad.nonzero()[0].tolist()
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong; first at (m, n) = ({m}, {n}), tile ({m // tile}, {n // tile}) of {tile}, "
            f"16x16 block ({m // 16}, {n // 16}), row {m % tile} column {n % tile} inside the tile: got {got[m, n].item()!r}, want {want[m, n].item()!r}")


def assert_exact(got, want, tile, what):
    """got (any float dtype) must equal the fp64 reference element by element"""
    got = got.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        raise AssertionError(first_wrong(got, want, tile, what))


def assert_bounded(got, want, bound, tile, what):
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    print(f"{what}: worst |err| / bound = {(err / bound).max().item():.3f}")
    if bad.any():
        m, n = bad.reshape(-1, bad.shape[-1]).nonzero()[0].tolist()
        e2, b2 = err.reshape(-1, bad.shape[-1]), bound.reshape(-1, bad.shape[-1])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at (m, n) = ({m}, {n}), tile "
                             f"({m // tile}, {n // tile}) of {tile}, 16x16 block ({m // 16}, {n // 16}): |err| {e2[m, n].item():.3e}, bound {b2[m, n].item():.3e}")
