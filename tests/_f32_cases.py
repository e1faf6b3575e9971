"""Per-element cases for the fp32 parity-mode kernels of csrc/f32.hip that had no direct test: wft_gemm_f32, wft_softmax_fwd_f32 /
_bwd_f32, wft_gelu_fwd_f32 / _bwd_f32, wft_axpby_f32, wft_colsum_f32, and the stride recipes of engine/ops32.py that reach
wft_gemm_f32.  Case tables, operand builders, float64 references, checkers, CPU restatements of each kernel's arithmetic and the
ways such kernels go wrong planted in those restatements ("mutants").  CPU only, plain torch; shared by tests/test_f32_host.py
(which proves on the CPU that the premises hold and that the checkers reject every mutant) and tests/test_f32_kernels_gpu.py (which
holds the kernels to the checkers).  u = 2^-24 throughout.

1. wft_gemm_f32 -- exact
   integer probe   A, B, bias and the base of C are fp32 integers from {-2 .. 2}; (alpha, beta) in {(1, 0), (-2, 0.5), (0.5, 1)}.
                   Every product, partial sum and epilogue term is a multiple of 1/2 and the builder asserts
                   |alpha| sum_k |a||b| + |bias| + |beta||c| < 2^24, so an fp32 accumulator holds the true value in any summation
                   order (test_f32_host.py sums in three orders and compares bits) and the output must be torch.equal to the
                   float64 reference cast to fp32.  A lost or doubled k, a bias read by row, a beta misapplied each move an element
                   by at least 1/2.
   gather probe    B (or, mirrored, A) is one-hot per column (row): B(k, n) = 1 iff k == k(n), k(n) = (7 (n + round N) + 3 + batch)
                   mod K; 7 is coprime to every K of the table and the rounds run until n + round N has covered 0 .. K - 1, so
                   every k is selected (asserted).  The other operand holds full-mantissa normal fp32 values
                   (randn x 2^randint(-8, 8)): C[m, n] = A[m, k(n)] bit for bit, since x * 1 + sum of (y * 0 = +-0) is x.
   layouts         every operand lives inside a larger flat allocation filled with poison (1e30, and NaN in a second pass)
                   wherever the strides never point; the set of touched addresses is computed from the strides, so the
                   overlapping-window rows of the conv stem are handled by the same code.  C has ldc = N + 5, a guard row behind
                   every batch and a sentinel (GUARD) in every element the strides never point to; with beta == 0 the M x N region
                   is NaN.  The check compares the WHOLE flat C buffer bit for bit with the expected image and, on a mismatch,
                   names the first differing (batch, m, n), the count, the 64 x 64 tiles and the wave quadrants hit.
   shapes          GEMM_SHAPES: M, N from {1, 31, 33, 64, 65, 129}, K from {1, 2, 15, 16, 17, 33, 50}; each runs under the four
                   staging combinations (A k-fast / m-fast x B k-fast / n-fast: NT, NN, TN and the fourth), batch = 3 with batch
                   strides that are no multiple of anything, bias present / absent and the three (alpha, beta) pairs.
   recipes         GEMM_RECIPES restates ops32's stride tuples as explicit layouts so that poison and guards can sit around them
                   (ops32 allocates its own buffers, which cannot be poisoned): conv1 / conv2 forward windows (a_rs = C / 2C <
                   K = 3C, b_bs = 0, bias), the three-tap scatter into the padded activation (ldc = 2d, an offset row, beta = 1),
                   the head-batched Q K^T and P V forms (batch stride dh inside a row, c_bs = dh with ldc = D) and the LoRA
                   product at K = rank = 8 and 3.  These are copies; the recipes THEMSELVES are tested through the functions:

2. ops32 functions, exact, on the GPU through the functions themselves (float64 autograd references, torch.equal)
   LinearFn        integer x, W, b, A, B, dy; scaling 0.5; mask in {0, 2}: A o m is even, so W_eff = W + s B (A o m), y, dx, dW,
                   db, dB = s dW (A o m)^T and dA = (s B^T dW) o m are integers < 2^24 (asserted).  Stands for ops32.linear: the
                   LoRA merge gemm (K = rank < 16, beta = 1 into a clone of W), _mm_nt with bias, _mm_nn, _mm_tn, colsum and the
                   two adapter-gradient gemms.
   ConvStemFn      signed integer mel, weights, positional table; each conv bias is 8 + the largest |conv| its channel can reach,
                   so every pre-activation is >= 8.  There fp32 exact-erf GELU is the identity (erff(v / sqrt 2) rounds to 1.0f
                   from v = 5.55 on, 0.5 v * 2 is exact) and its derivative rounds to 1.0f (v phi(v) < 2^-25 from v = 8 on): the
                   forward, dW1, db1, dW2, db2 are integer arithmetic and are compared bit for bit with a float64
                   conv1d(pad 1) -> conv1d(stride 2, pad 1) -> permute -> + pos reference WITHOUT GELU.  The host test proves
                   the premise in float64 and with CPU fp32 gelu; the GPU test asserts it on the device (GeluFn.apply(pre) has the
                   bits of pre) and says "premise" when that is what failed.  Stands for the window gemms, the per-clip beta = 1
                   weight-gradient accumulation, the three-tap scatter, wft_gelu_*, wft_axpby (1, 1) and wft_colsum.
   TiedLogitsFn    integers at V = 130, d = 40, 7 rows: _mm_nt, _mm_nn, _mm_tn.
   AttentionFn     its six stride recipes are inline in forward / backward with a softmax between them, so they cannot be called
                   as integer products without editing ops32.  They are covered by tests/test_fp32_mode_gpu.py::
                   test_f32_attention_on_probe_operands (packed [B, T, 3D] qkv, [B, Tk + guard, 2D] kv) and, as copies, by the
                   "heads_qk" / "heads_pv" recipes above.  ops32 was not restructured.

3. wft_softmax_fwd_f32 / _bwd_f32 -- bounds against float64
   forward   |got - p| <= SOFTMAX_CF u p (1 + 2 E), E = max over visible c of (|scale x_c| + |t_c|), t_c = scale x_c - max.
             Roundings on an element's path, in units of u relative to p: s = fl(scale x) and t = fl(s - m) perturb the exponent by
             at most (|s| + |t|) u <= E u; expf is taken at 2 ulp = 4 u (HIP documents 1 ulp); the same (4 + E) u holds for every
             positive term of the sum and so for the sum; each lane adds at most 3 terms (2 u) and the wave reduction adds 6 (6 u);
             the division is taken at 1 ulp = 2 u; the final product 1 u.  Total (4 + E) + (4 + E) + 8 + 2 + 1 = (19 + 2 E) u
             <= 19 u (1 + 2 E); rounded up for second-order terms: SOFTMAX_CF = 20.  The max itself is exact.
   backward  |got - ds| <= SOFTMAX_CB u |scale| p_c (|dp_c| + S), S = sum_c p_c |dp_c|, the reference taken on the same fp32 p.
             Products p dp 1 u each, lane sum 2 u, wave reduction 6 u: the dot is off by at most 9 u S; fl(dp - dot), fl(scale p)
             and the last product 3 u (|dp| + S).  Total <= 12 u (|dp| + S): SOFTMAX_CB = 12.  No transcendental.
   floor     4 x the worst ratio of the CPU torch-fp32 restatement (lane-strided sums, xor-butterfly reduction, as the kernel; expf
             and erff there are float64 values rounded once, so the figures are the same on every CPU)
             over all cases and seeds: forward 4 x SOFTMAX_CPU_F = 4 x 1.12, backward 4 x SOFTMAX_CPU_B = 4 x 2.55 (ratios
             of |err| to u p (1 + 2 E) and to u |scale| p (|dp| + S)); both below the counted constants, which stand.
   structure bit-level: masked columns are +0.0, elements cols .. ld keep their poison, causal row 0 is exactly 1.0, constant rows
             are within the bound of 1 / lim, no NaN or inf.  Causal cases carry a decoy of +300 / scale on every masked
             column: a max or a sum that reaches it turns the row into 0 or NaN.
   operands  randn, one column dominating by 30, two columns tied for the maximum, constant rows -- all held to the bound; and
             scores spanning +-80 after scaling, where p underflows fp32: structure only, plus both bounds with a floor of 2^-126
             (one smallest normal; this set's floor is this module's choice, the issue sets no bound for it).

4. element-wise kernels
   GELU      inputs in [-10, 10]: +-0, +-2^-126, +-1, +-5.5, +-8, +-10, 65 neighbours of each point where a correctly rounded erff saturates (5.5426) and where a 1-ulp-low one does (5.42), then
             a grid.  Forward |got - ref| <= GELU_CF u (|x| + |ref|): t = fl(v / sqrt 2) moves erf by < 1 u, erff taken at
             4 ulp = 8 u (HIP's documented figure), fl(1 + e) 2 u: 11 u absolute on (1 + e); 0.5 v is exact; the product 1 u |ref|:
             5.5 u |x| + u |ref|, GELU_CF = 6.  Backward |got - ref| <= GELU_CB u |dy| (1 + |x|): cdf 5.5 u; the density term
             v phi(v) (v^2 / 2 + 6.3) u <= 1.7 u (fl(v v) into the exponent, expf at 4 u, the constant and two products); the sum
             and the product with dy 1.2 u each: 9.6 u, GELU_CB = 10.  Floors: 4 x GELU_CPU_F = 4 x 0.68, 4 x GELU_CPU_B = 4 x 1.22.
             gelu(-0.0) must have the bits of the fp32 formula (-0.0).
   axpby     y == NULL and (a, b) = (1, 1): one rounding, torch.equal with the CPU's fp32 value.  General: the kernel may or may
             not contract to an fma, so |got - ref64| <= u (|a x| + |b y| + |ref|), a and b as the fp32 values the ABI carries.
   colsum    integers: torch.equal to the float64 sum; randn: rows are added in index order, so the CPU fp32 running sum in that
             order matches bit for bit.  ld = cols + 3 with NaN behind every row, a guard element behind the output.
   big n     BIG_N = 65535 x 256 + 300, the first size with a second grid-stride trip: the input is a 1021-periodic tiling of a
             pattern the small case has already judged, and the output must be that case's output tiled, bit for bit.

Mutants (test_f32_host.py asserts each is rejected wherever it changes a bit of the restated result, and changes some case):
GEMM_MUTANTS, CONV_MUTANTS, SOFTMAX_MUTANTS, "second_trip_skipped", "colsum_ld_is_cols".
"""
import math
import zlib
from dataclasses import dataclass, replace
from typing import Optional

import torch
import torch.nn.functional as Fn

F32, F64, I32 = torch.float32, torch.float64, torch.int32
U = 2.0 ** -24
SEEDS = (0, 1)
POISONS = (1.0e30, float("nan"))
GUARD = 12345.0
LIMIT = float(2 ** 24)
BATCH = 3

SOFTMAX_CF, SOFTMAX_CB = 20.0, 12.0
GELU_CF, GELU_CB = 6.0, 10.0
# worst ratios of the CPU fp32 restatements, measured by tests/test_f32_host.py (which asserts these numbers)
SOFTMAX_CPU_F, SOFTMAX_CPU_B = 1.12, 2.55
GELU_CPU_F, GELU_CPU_B = 0.68, 1.22
CPU_FIGURE_RTOL = 0.05     # another CPU's vector exp / erf may differ in a last bit

INV_SQRT2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794


def exp32(x):
    """fp32 exp / erf of the CPU restatements: float64, rounded once -- a correctly rounded fp32 function, the same on every CPU"""
    return torch.exp(x.double()).to(F32)


def erf32(x):
    return torch.erf(x.double()).to(F32)


def bits(t):
    return t.detach().cpu().contiguous().view(I32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(shape, g, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


def full_mantissa(shape, g):
    """normal fp32 values with all 24 bits in play: randn x 2^randint(-8, 8), zeros replaced"""
    v = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-8, 9, shape, generator=g).float())
    v = torch.where(v.abs() < 2.0 ** -100, torch.ones_like(v), v)
    return v.to(F32)


# ------------------------------------------------------------------------------------------------ layouts
@dataclass(frozen=True)
class Layout:
    """a logical [batch, rows, cols] operand inside a flat allocation: element (b, r, c) at off + b bs + r rs + c cs"""
    shape: tuple
    strides: tuple
    off: int
    tail: int = 4

    @property
    def total(self):
        return self.off + sum((n - 1) * s for n, s in zip(self.shape, self.strides)) + 1 + self.tail

    def addresses(self):
        b, r, c = (torch.arange(n) * s for n, s in zip(self.shape, self.strides))
        return self.off + b[:, None, None] + r[None, :, None] + c[None, None, :]

    def view(self, flat):
        return torch.as_strided(flat, self.shape, self.strides, self.off)


def poisoned(layout, poison, values=None, g=None):
    """flat buffer: poison everywhere the strides never point, integers (or `values`, for a layout without overlap) elsewhere"""
    flat = torch.full((layout.total,), poison, dtype=F32)
    addr = layout.addresses().reshape(-1)
    if values is None:
        uniq = torch.unique(addr)
        flat[uniq] = _ints((uniq.numel(),), g)
    else:
        assert torch.unique(addr).numel() == addr.numel(), "explicit values need a layout without overlap"
        layout.view(flat).copy_(values)
    return flat


def untouched_is_poison(flat, layout, poison):
    """the premise: poison sits at exactly the addresses the strides never reach"""
    hit = torch.zeros(flat.numel(), dtype=torch.bool)
    hit[layout.addresses().reshape(-1)] = True
    is_p = torch.isnan(flat) if math.isnan(poison) else flat == poison
    return bool((is_p == ~hit).all())


# ------------------------------------------------------------------------------------------------ wft_gemm_f32
GEMM_SHAPES = ((1, 1, 1), (31, 33, 2), (33, 31, 15), (64, 64, 16), (65, 64, 17), (64, 65, 33), (129, 31, 50), (31, 129, 16), (65, 129, 33),
               (129, 65, 17), (1, 64, 50))
ALPHA_BETA = ((1.0, 0.0), (-2.0, 0.5), (0.5, 1.0))
STAGINGS = ((True, True), (True, False), (False, False), (False, True))   # (a_kfast, b_kfast): NT, NN, TN, the fourth


@dataclass(frozen=True)
class GemmCase:
    name: str
    M: int
    N: int
    K: int
    la: Layout
    lb: Layout
    lc: Layout
    bias: bool
    alpha: float
    beta: float
    ragged: bool


def _std_layouts(M, N, K, a_kfast, b_kfast, batch=BATCH):
    lda = (K if a_kfast else M) + 3
    la = Layout((batch, M, K), ((M if a_kfast else K) * lda + 7, lda if a_kfast else 1, 1 if a_kfast else lda), 5)
    ldb = (K if b_kfast else N) + 3
    lb = Layout((batch, K, N), ((N if b_kfast else K) * ldb + 7, 1 if b_kfast else ldb, ldb if b_kfast else 1), 3)
    lc = Layout((batch, M, N), ((M + 1) * (N + 5) + 3, N + 5, 1), 2, tail=N + 9)
    return la, lb, lc


def gemm_cases(M, N, K):
    out = []
    for a_kfast, b_kfast in STAGINGS:
        for bias in (True, False):
            for alpha, beta in ALPHA_BETA:
                la, lb, lc = _std_layouts(M, N, K, a_kfast, b_kfast)
                name = f"{M}x{N}x{K}-A{'k' if a_kfast else 'm'}B{'k' if b_kfast else 'n'}-{'bias' if bias else 'nobias'}-a{alpha}b{beta}"
                out.append(GemmCase(name, M, N, K, la, lb, lc, bias, alpha, beta, bool(M % 64 or N % 64 or K % 16)))
    return out


def gather_cases(M, N, K):
    return [GemmCase(f"{M}x{N}x{K}-A{'k' if ak else 'm'}B{'k' if bk else 'n'}-gather", M, N, K, *_std_layouts(M, N, K, ak, bk), False, 1.0, 0.0,
                     bool(M % 64 or N % 64 or K % 16)) for ak, bk in STAGINGS]


def _recipes():
    """ops32's stride tuples, restated (see the docstring): name -> GemmCase"""
    out = []
    T, C, d, B = 6, 5, 24, 3
    T2 = T // 2
    # conv1 forward: gemm(x0, w1k, M=T, N=d, K=3C, a_strides=(C, 1, (T+2)C), b_strides=(1, 3C, 0), batch=B, bias, ldc=d, c_bs=T d)
    out.append(GemmCase("conv1_windows", T, d, 3 * C, Layout((B, T, 3 * C), ((T + 2) * C + 5, C, 1), 3), Layout((B, 3 * C, d), (0, 1, 3 * C), 2),
                        Layout((B, T, d), (T * d + 7, d, 1), 1, tail=d + 4), True, 1.0, 0.0, True))
    # conv2 forward: a_strides=(2d, 1, (T+2)d), M = T2, K = 3d
    out.append(GemmCase("conv2_windows", T2, d, 3 * d, Layout((B, T2, 3 * d), ((T + 2) * d + 5, 2 * d, 1), 3), Layout((B, 3 * d, d), (0, 1, 3 * d), 2),
                        Layout((B, T2, d), (T2 * d + 7, d, 1), 1, tail=d + 4), True, 1.0, 0.0, True))
    # three-tap scatter, tap kk = 1: gemm(dpre2, w2k[:, d:2d], M=T2, N=d, K=d, a=(d, 1, T2 d), b=(3d, 1, 0), out=dact1[:, 1:], ldc=2d, c_bs=(T+2)d, beta=1)
    out.append(GemmCase("tap_scatter", T2, d, d, Layout((B, T2, d), (T2 * d, d, 1), 0), Layout((B, d, d), (0, 3 * d, 1), d),
                        Layout((B, T2, d), ((T + 2) * d, 2 * d, 1), d, tail=3 * d), False, 1.0, 1.0, True))
    # per-clip weight-gradient accumulation: gemm(dpre2[b], act1[b], M=d, N=3d, K=T2, a=(1, d, 0), b=(2d, 1, 0), out=dw2k, ldc=3d, beta=1)
    out.append(GemmCase("dw2_windows", d, 3 * d, T2, Layout((1, d, T2), (0, 1, d), 1), Layout((1, T2, 3 * d), (0, 2 * d, 1), 4),
                        Layout((1, d, 3 * d), (0, 3 * d + 5, 1), 2, tail=3 * d + 9), False, 1.0, 1.0, True))
    H, dh, Tq, Tk = 2, 16, 7, 9
    D = H * dh
    # Q K^T from a packed [T, 3D] qkv and a [Tk + guard, 2D] kv: a=(3D, 1, dh), b=(1, 2D, dh), ldc=Tk, c_bs=Tq Tk
    out.append(GemmCase("heads_qk", Tq, Tk, dh, Layout((H, Tq, dh), (dh, 3 * D, 1), 0, tail=2 * D), Layout((H, dh, Tk), (dh, 1, 2 * D), 0, tail=D + 2 * D),
                        Layout((H, Tq, Tk), (Tq * Tk, Tk, 1), 0, tail=8), False, 1.0, 0.0, True))
    # P V: a=(Tk, 1, Tq Tk), b=(2D, 1, dh) from the V half, out=o[b] with ldc=D, c_bs=dh
    out.append(GemmCase("heads_pv", Tq, dh, Tk, Layout((H, Tq, Tk), (Tq * Tk, Tk, 1), 0), Layout((H, Tk, dh), (dh, 2 * D, 1), D, tail=2 * D),
                        Layout((H, Tq, dh), (dh, D, 1), 0, tail=D), False, 1.0, 0.0, True))
    # LoRA merge: gemm(lora_b, am, M=out, N=in, K=rank, a=(rank, 1, 0), b=(in, 1, 0), out=W.clone(), ldc=in, alpha=s, beta=1)
    for o, i, r in ((72, 40, 8), (40, 72, 3)):
        out.append(GemmCase(f"lora_rank{r}", o, i, r, Layout((1, o, r), (0, r, 1), 1), Layout((1, r, i), (0, i, 1), 1),
                            Layout((1, o, i), (0, i + 5, 1), 2, tail=i + 9), False, 0.5, 1.0, True))
    return out


GEMM_RECIPES = _recipes()


@dataclass
class GemmOp:
    case: GemmCase
    a_flat: torch.Tensor
    b_flat: torch.Tensor
    c_flat: torch.Tensor
    bias: Optional[torch.Tensor]
    poison: float
    selectors: Optional[torch.Tensor] = None   # gather probes: every k the one-hot operand selects


def _c_flat(case, g):
    flat = torch.full((case.lc.total,), GUARD, dtype=F32)
    addr = torch.unique(case.lc.addresses().reshape(-1))
    flat[addr] = _ints((addr.numel(),), g) if case.beta != 0 else float("nan")
    return flat


def gemm_operands(case, seed, poison):
    g = _gen("gemm", case.name, seed)
    op = GemmOp(case, poisoned(case.la, poison, g=g), poisoned(case.lb, poison, g=g), _c_flat(case, g),
                _ints((case.N,), g) if case.bias else None, poison)
    a, b, c = case.la.view(op.a_flat).double(), case.lb.view(op.b_flat).double(), case.lc.view(op.c_flat).double()
    mag = abs(case.alpha) * (a.abs() @ b.abs()) + (op.bias.abs().double() if case.bias else 0.0)
    if case.beta != 0:
        mag = mag + abs(case.beta) * c.abs()
    assert float(mag.max()) < LIMIT, case.name
    return op


def _selector(n_out, K, batch):
    """k(j) for j = n + round n_out, rounds until 0 .. K - 1 is covered: [rounds, batch, n_out]"""
    rounds = -(-K // n_out)
    j = torch.arange(n_out)[None, None, :] + n_out * torch.arange(rounds)[:, None, None]
    return (7 * j + 3 + torch.arange(batch)[None, :, None]) % K


def gather_operands(case, seed, poison, one_hot):
    """one GemmOp per round; one_hot = "B": C[m, n] = A[m, k(n)]; "A": C[m, n] = B[k(m), n]"""
    g = _gen("gather", case.name, seed, one_hot)
    batch, M, N, K = case.la.shape[0], case.M, case.N, case.K
    sel = _selector(N if one_hot == "B" else M, K, batch)
    dense = full_mantissa((batch, M, K) if one_hot == "B" else (batch, K, N), g)
    ops = []
    for r in range(sel.shape[0]):
        if one_hot == "B":
            hot = torch.zeros(batch, K, N).scatter_(1, sel[r][:, None, :], 1.0)
            a_flat, b_flat = poisoned(case.la, poison, dense), poisoned(case.lb, poison, hot)
        else:
            hot = torch.zeros(batch, M, K).scatter_(2, sel[r][:, :, None], 1.0)
            a_flat, b_flat = poisoned(case.la, poison, hot), poisoned(case.lb, poison, dense)
        ops.append(GemmOp(case, a_flat, b_flat, _c_flat(case, g), None, poison, sel))
    return ops


def gather_expected_logical(op, one_hot, rnd):
    """the gather stated without a product: fp32 [batch, M, N]"""
    case, sel = op.case, op.selectors[rnd]
    if one_hot == "B":
        return torch.gather(case.la.view(op.a_flat), 2, sel[:, None, :].expand(-1, case.M, -1))
    return torch.gather(case.lb.view(op.b_flat), 1, sel[:, :, None].expand(-1, -1, case.N))


def gemm_ref64(op):
    case = op.case
    v = case.alpha * (case.la.view(op.a_flat).double() @ case.lb.view(op.b_flat).double())
    if op.bias is not None:
        v = v + op.bias.double()
    if case.beta != 0:
        v = v + case.beta * case.lc.view(op.c_flat).double()
    return v


def gemm_expected(op, logical=None):
    """the whole flat C buffer after the call"""
    flat = op.c_flat.clone()
    op.case.lc.view(flat).copy_((gemm_ref64(op) if logical is None else logical).to(F32))
    return flat


def fp32_sum_orders(a, b):
    """sum_k a[.., m, k] b[.., k, n] in fp32 in three orders: ascending k, 16-deep slabs each summed then added, descending k"""
    K = a.shape[-1]
    term = lambda k: a[..., :, k:k + 1] * b[..., k:k + 1, :]   # noqa: E731
    up = sum((term(k) for k in range(1, K)), term(0))
    down = sum((term(k) for k in range(K - 2, -1, -1)), term(K - 1))
    slabs = torch.zeros_like(up)
    for k0 in range(0, K, 16):
        slabs = slabs + sum((term(k) for k in range(k0 + 1, min(k0 + 16, K))), term(k0))
    return up, slabs, down


GEMM_MUTANTS = ("drop_last_k_of_ragged_slab", "drop_slab", "double_slab", "swap_mfma_pair_in_A", "bias_by_m", "beta_applied_where_0",
                "beta_skipped_where_1", "write_row_M", "write_col_N", "batch_stride_0")


def gemm_restate(op, mutant=None):
    """the kernel's arithmetic on the flat buffers, on the CPU in fp32: 16-deep slabs, the epilogue order of gemm_f32_kernel"""
    case = op.case
    la = replace(case.la, strides=(0,) + case.la.strides[1:]) if mutant == "batch_stride_0" else case.la
    A, B = la.view(op.a_flat).clone(), case.lb.view(op.b_flat).clone()
    batch, M, K = A.shape
    N = B.shape[2]
    if mutant == "drop_last_k_of_ragged_slab" and K % 16:
        A[:, :, K - 1] = 0
    if mutant == "swap_mfma_pair_in_A" and K >= 2:
        A[:, :, [0, 1]] = A[:, :, [1, 0]]
    slabs = list(range(0, K, 16))
    if mutant == "drop_slab":
        slabs = slabs[:-1]
    if mutant == "double_slab":
        slabs = slabs + slabs[:1]
    acc = torch.zeros(batch, M, N, dtype=F32)
    for k0 in slabs:
        acc = acc + (A[:, :, k0:k0 + 16].double() @ B[:, k0:k0 + 16, :].double()).to(F32)
    v = torch.tensor(case.alpha, dtype=F32) * acc
    if op.bias is not None:
        v = v + (op.bias[torch.arange(M) % N][None, :, None] if mutant == "bias_by_m" else op.bias[None, None, :])
    c0 = case.lc.view(op.c_flat)
    beta = case.beta
    if mutant == "beta_applied_where_0" and beta == 0:
        beta = 1.0
    if mutant == "beta_skipped_where_1" and beta == 1:
        beta = 0.0
    if beta != 0:
        v = v + torch.tensor(beta, dtype=F32) * c0
    out = op.c_flat.clone()
    case.lc.view(out).copy_(v)
    bs, rs, cs = case.lc.strides
    if mutant == "write_row_M":
        out[case.lc.off + (batch - 1) * bs + M * rs + torch.arange(N) * cs] = v[batch - 1, M - 1]
    if mutant == "write_col_N":
        out[case.lc.off + (batch - 1) * bs + torch.arange(M) * rs + N * cs] = v[batch - 1, :, N - 1]
    return out


def gemm_mismatch(got_flat, want_flat, case):
    """None, or the report: first differing (batch, m, n), how many, which tiles and wave quadrants"""
    got, want = bits(got_flat), bits(want_flat)
    assert got.shape == want.shape
    if torch.equal(got, want):
        return None
    bad = (got != want).nonzero().view(-1)
    where = torch.full((want.numel(),), -1, dtype=torch.long)
    addr = case.lc.addresses().reshape(-1)
    where[addr] = torch.arange(addr.numel())
    _, M, N = case.lc.shape
    inside = where[bad][where[bad] >= 0]
    first = int(bad[0])
    gf, wf = got_flat.cpu().view(-1)[first].item(), want_flat.view(-1)[first].item()
    if int(where[first]) < 0:
        head = f"first at flat offset {first}, OUTSIDE C's {M} x {N} region (guard): got {gf!r}, want {wf!r}"
    else:
        j = int(where[first])
        head = f"first at (batch {j // (M * N)}, m {j // N % M}, n {j % N}): got {gf!r}, want {wf!r}"
    m, n = inside // N % M, inside % N
    tiles = [(t // 4096, t % 4096) for t in torch.unique(m // 64 * 4096 + n // 64).tolist()]
    quads = torch.unique((m % 64 // 32) * 2 + n % 64 // 32).tolist()
    return (f"{case.name}: {bad.numel()} elements differ ({inside.numel()} inside C, {bad.numel() - inside.numel()} in guards); {head}; "
            f"tiles (m / 64, n / 64) {tiles[:8]}; wave quadrants {quads}")


# ------------------------------------------------------------------------------------------------ ops32 functions
LINEAR_CASES = (  # (in, out, rank, masked, bias)
    (40, 72, 8, True, True), (72, 40, 3, True, True), (72, 72, 8, True, False), (40, 40, 0, False, True), (72, 40, 0, False, False))
LINEAR_ROWS = 37
LINEAR_SCALING = 0.5


def linear_case(case, seed):
    """-> (inputs, float64 results): x @ (W + s B (A o m))^T + b and the gradients under dy, by float64 autograd"""
    fin, fout, rank, masked, bias = case
    g = _gen("linear", case, seed)
    t = {"x": _ints((LINEAR_ROWS, fin), g), "w": _ints((fout, fin), g), "dy": _ints((LINEAR_ROWS, fout), g)}
    t["b"] = _ints((fout,), g) if bias else None
    t["A"], t["B"] = (_ints((rank, fin), g), _ints((fout, rank), g)) if rank else (None, None)
    t["mask"] = (2.0 * torch.randint(0, 2, (1, fin), generator=g)).to(F32) if masked else None
    leaf = {k: v.double().requires_grad_(True) for k, v in t.items() if v is not None and k not in ("dy", "mask")}
    w_eff = leaf["w"]
    if rank:
        am = leaf["A"] * t["mask"].double() if masked else leaf["A"]
        w_eff = w_eff + LINEAR_SCALING * (leaf["B"] @ am)
    y = leaf["x"] @ w_eff.T
    if bias:
        y = y + leaf["b"]
    y.backward(t["dy"].double())
    ref = {"y": y.detach(), "w_eff": w_eff.detach(), **{"d" + k: v.grad for k, v in leaf.items()}}
    return t, ref


def linear_magnitudes(t):
    """sum |.| |.| of every product LinearFn forms: all must stay below 2^24"""
    ab = lambda *xs: [None if x is None else x.double().abs() for x in xs]   # noqa: E731
    x, w, dy, A, B, m = ab(t["x"], t["w"], t["dy"], t["A"], t["B"], t["mask"])
    w_eff = w
    out = []
    if A is not None:
        am = A * m if m is not None else A
        w_eff = w + LINEAR_SCALING * (B @ am)
    dw = dy.T @ x
    out += [w_eff, x @ w_eff.T + (t["b"].double().abs() if t["b"] is not None else 0), dy @ w_eff, dw, dy.sum(0)]
    if A is not None:
        out += [LINEAR_SCALING * dw @ am.T, LINEAR_SCALING * (B.T @ dw) * (m if m is not None else 1)]
    return max(float(v.max()) for v in out)


CONV_CASES = ((5, 24, 6, 1), (8, 72, 22, 3), (5, 72, 130, 1), (8, 24, 130, 3))   # (n_mels, d, T, B)
CONV_MUTANTS = ("window_stride_1", "halo_not_zero", "taps_reversed")


def conv_inputs(case, seed):
    n_mels, d, T, B = case
    g = _gen("conv", case, seed)
    t = {"mel": _ints((B, n_mels, T), g), "w1": _ints((d, n_mels, 3), g, -1, 1), "w2": _ints((d, d, 3), g, -1, 1),
         "pos": _ints((T // 2, d), g), "dx": _ints((B, T // 2, d), g)}
    t["b1"] = 8.0 + 2.0 * t["w1"].abs().sum((1, 2))                       # |mel| <= 2
    act_max = float((t["b1"] + 2.0 * t["w1"].abs().sum((1, 2))).max())
    t["b2"] = 8.0 + act_max * t["w2"].abs().sum((1, 2))
    return t


def conv_ref64(t, mutant=None):
    """float64, no GELU: -> dict of pre1, pre2, out, dw1, db1, dw2, db2.  Mutants are the ways the window gemms go wrong."""
    p = {k: t[k].double().requires_grad_(k in ("w1", "b1", "w2", "b2")) for k in ("mel", "w1", "b1", "w2", "b2", "pos")}
    w1, w2 = (p["w1"].flip(2), p["w2"].flip(2)) if mutant == "taps_reversed" else (p["w1"], p["w2"])
    if mutant == "halo_not_zero":
        mel = Fn.pad(p["mel"], (1, 1), value=1.0)
        pre1 = Fn.conv1d(mel, w1, p["b1"])
        pre2 = Fn.conv1d(Fn.pad(pre1, (1, 1), value=1.0), w2, p["b2"], stride=2)
    else:
        pre1 = Fn.conv1d(p["mel"], w1, p["b1"], padding=1)
        if mutant == "window_stride_1":
            pre2 = Fn.conv1d(pre1, w2, p["b2"], stride=1, padding=1)[:, :, :t["pos"].shape[0]]
        else:
            pre2 = Fn.conv1d(pre1, w2, p["b2"], stride=2, padding=1)
    out = pre2.permute(0, 2, 1) + p["pos"]
    out.backward(t["dx"].double())
    return {"pre1": pre1.detach(), "pre2": pre2.detach(), "out": out.detach(), "dw1": p["w1"].grad, "db1": p["b1"].grad,
            "dw2": p["w2"].grad, "db2": p["b2"].grad}


CONV_CHECKED = ("out", "dw1", "db1", "dw2", "db2")


def conv_magnitudes(t):
    """the same chain on absolute values: the largest sum |.| |.| that any conv gemm, scatter or colsum forms (every entry of the
    backward-data buffer is a term of db1's sums, so db1 bounds it)"""
    a = {k: t[k].double().abs().requires_grad_(k in ("w1", "b1", "w2", "b2")) for k in ("mel", "w1", "b1", "w2", "b2", "pos", "dx")}
    pre1 = Fn.conv1d(a["mel"], a["w1"], a["b1"], padding=1)
    out = Fn.conv1d(pre1, a["w2"], a["b2"], stride=2, padding=1).permute(0, 2, 1) + a["pos"]
    out.backward(a["dx"])
    return max(float(v.max()) for v in (out.detach(), a["w1"].grad, a["b1"].grad, a["w2"].grad, a["b2"].grad))


def gelu_f32_cpu(x):
    """the kernel's formula in CPU fp32"""
    x = x.to(F32)
    return torch.tensor(0.5, dtype=F32) * x * (1.0 + erf32(x * torch.tensor(INV_SQRT2, dtype=F32)))


def dgelu_f32_cpu(dy, x):
    x = x.to(F32)
    cdf = 0.5 * (1.0 + erf32(x * torch.tensor(INV_SQRT2, dtype=F32)))
    return dy.to(F32) * (cdf + x * torch.tensor(INV_SQRT_2PI, dtype=F32) * exp32(-0.5 * x * x))


TIED = (130, 40, 7)   # V, d, rows


def tied_case(seed):
    V, d, rows = TIED
    g = _gen("tied", seed)
    t = {"x": _ints((rows, d), g), "emb": _ints((V, d), g), "dl": _ints((rows, V), g)}
    x, e, dl = (v.double() for v in (t["x"], t["emb"], t["dl"]))
    mag = max(float(v.max()) for v in (x.abs() @ e.abs().T, dl.abs() @ e.abs(), dl.abs().T @ x.abs()))
    return t, {"logits": x @ e.T, "dx": dl @ e, "demb": dl.T @ x}, mag


# ------------------------------------------------------------------------------------------------ softmax
@dataclass(frozen=True)
class SoftmaxCase:
    nrows: int
    cols: int
    causal: bool
    rpm: int
    scale: float
    kind: str    # randn / dominant / tie / flat / span80

    @property
    def name(self):
        return f"{self.nrows}x{self.cols}-{'causal' + str(self.rpm) if self.causal else 'full'}-s{self.scale}-{self.kind}"

    @property
    def ld(self):
        return self.cols + 3


SOFTMAX_COLS = (1, 63, 64, 65, 130)
SOFTMAX_KINDS = ("randn", "dominant", "tie", "flat", "span80")
DECOY = 300.0


def softmax_cases(cols):
    shapes = [(7, False, 7), (10, False, 10)]
    if cols >= 7:
        shapes += [(10, True, 5), (7, True, 7), (10, True, 7)]
    return [SoftmaxCase(nr, cols, causal, rpm, scale, kind) for nr, causal, rpm in shapes for scale in (0.125, 1.0) for kind in SOFTMAX_KINDS]


def softmax_lim(case, rpm=None, shift=0):
    rows = torch.arange(case.nrows)
    if not case.causal:
        return torch.full((case.nrows,), case.cols)
    return (rows % (case.rpm if rpm is None else rpm) + 1 + shift).clamp(1, case.cols)


def softmax_inputs(case, seed, poison=float("nan")):
    """-> (x [nrows, ld] with poison behind cols and decoys on masked columns, dp [nrows, ld])"""
    g = _gen("softmax", case.name, seed)
    R, Cc = case.nrows, case.cols
    s = torch.randn(R, Cc, generator=g)
    lim = softmax_lim(case)
    pick = (torch.rand(R, generator=g) * lim).long()            # a visible column per row
    if case.kind == "dominant":
        s[torch.arange(R), pick] += 30.0
    elif case.kind == "tie":
        other = (pick + 1 + (torch.rand(R, generator=g) * (lim - 1).clamp(min=1)).long()) % lim
        top = s.abs().max() + 0.5
        s[torch.arange(R), pick] = top
        s[torch.arange(R), other] = top
    elif case.kind == "flat":
        s = torch.full((R, Cc), 1.375)
    elif case.kind == "span80":
        s = (torch.rand(R, Cc, generator=g) * 160.0 - 80.0)
        s[:, 0] = 80.0
        if Cc > 1:
            s[:, 1] = -80.0
    x = (s / case.scale).to(F32)                                   # scale is a power of two: exact
    masked = torch.arange(Cc)[None, :] >= lim[:, None]
    x = torch.where(masked, torch.tensor(DECOY / case.scale, dtype=F32), x)
    full = torch.full((R, case.ld), poison, dtype=F32)
    full[:, :Cc] = x
    dp = torch.full((R, case.ld), poison, dtype=F32)
    dp[:, :Cc] = torch.randn(R, Cc, generator=g)
    return full, dp


def softmax_ref64(case, x):
    """-> (p, E): float64 probabilities (masked columns 0) and the bound's max_c(|scale x_c| + |t_c|) over visible columns"""
    Cc = case.cols
    t = x[:, :Cc].double() * case.scale
    vis = torch.arange(Cc)[None, :] < softmax_lim(case)[:, None]
    m = torch.where(vis, t, torch.tensor(-math.inf, dtype=F64)).max(1, keepdim=True).values
    e = torch.where(vis, torch.exp(t - m), torch.zeros_like(t))
    E = torch.where(vis, t.abs() + (t - m).abs(), torch.zeros_like(t)).max(1, keepdim=True).values
    return e / e.sum(1, keepdim=True), E


def softmax_bwd_ref64(case, p32, dp):
    Cc = case.cols
    p, d = p32[:, :Cc].double(), dp[:, :Cc].double()
    dot = (p * d).sum(1, keepdim=True)
    S = (p * d.abs()).sum(1, keepdim=True)
    return case.scale * p * (d - dot), abs(case.scale) * p * (d.abs() + S)


def _wave_reduce(v, op):
    """[rows, 64] -> [rows, 1]: the xor butterfly of wave_sum / wave_max (every lane ends with the same value; lane 0's is taken)"""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, lane ^ o])
    return v[:, :1]


def _lane_strided(vals, valid, op, init):
    """vals, valid [rows, n]: lane l folds columns l, l + 64, ... in order from `init`, then the wave butterfly"""
    R, n = vals.shape
    trips = -(-n // 64)
    pad = trips * 64 - n
    vals = Fn.pad(vals, (0, pad)).view(R, trips, 64)
    valid = Fn.pad(valid, (0, pad)).view(R, trips, 64)
    acc = torch.full((R, 64), init, dtype=F32)
    for i in range(trips):
        acc = torch.where(valid[:, i], op(acc, vals[:, i]), acc)
    return _wave_reduce(acc, op)


SOFTMAX_MUTANTS = ("lim_plus_1", "lim_minus_1", "rows_per_mat_is_nrows", "masked_left_at_input", "max_over_cols", "bwd_dot_over_ld",
                   "scale_twice")


def softmax_fwd_restate(case, x, mutant=None):
    """softmax_fwd_f32_kernel on the CPU in fp32, on the whole [nrows, ld] buffer"""
    Cc = case.cols
    out = x.clone()
    scale = torch.tensor(case.scale * (case.scale if mutant == "scale_twice" else 1.0), dtype=F32)
    lim = softmax_lim(case, rpm=case.nrows if mutant == "rows_per_mat_is_nrows" else None,
                      shift={"lim_plus_1": 1, "lim_minus_1": -1}.get(mutant, 0))
    cols = torch.arange(Cc)[None, :]
    vis = cols < lim[:, None]
    s = x[:, :Cc] * scale
    m = _lane_strided(s, torch.ones_like(vis) if mutant == "max_over_cols" else vis, torch.maximum, -3.0e38)
    e = exp32(s - m)
    inv = 1.0 / _lane_strided(e, vis, torch.add, 0.0)
    out[:, :Cc] = torch.where(vis, e * inv, x[:, :Cc] if mutant == "masked_left_at_input" else torch.zeros_like(e))
    return out


def softmax_bwd_restate(case, p, dp, mutant=None):
    Cc = case.cols
    out = dp.clone()
    n = case.ld if mutant == "bwd_dot_over_ld" else Cc
    scale = torch.tensor(case.scale * (case.scale if mutant == "scale_twice" else 1.0), dtype=F32)
    dot = _lane_strided(p[:, :n] * dp[:, :n], torch.ones(case.nrows, n, dtype=torch.bool), torch.add, 0.0)
    out[:, :Cc] = scale * p[:, :Cc] * (dp[:, :Cc] - dot)
    return out


def softmax_fwd_check(case, x, got, floor=0.0):
    """-> (problem or None, worst |err| / (u p (1 + 2 E))): structure first, then the per-element bound"""
    Cc = case.cols
    got = got.cpu()
    if not same_bits(got[:, Cc:], x[:, Cc:]):
        return "elements cols .. ld were written", math.nan
    lim = softmax_lim(case)
    masked = torch.arange(Cc)[None, :] >= lim[:, None]
    g = got[:, :Cc]
    if not bool((bits(g)[masked] == 0).all()):
        return "a masked column is not +0.0", math.nan
    if not bool(torch.isfinite(g).all()):
        return "NaN or inf", math.nan
    if case.causal and not bool((g[lim == 1, 0] == 1.0).all()):
        return "a causal row with one visible key is not exactly 1.0", math.nan
    p, E = softmax_ref64(case, x)
    unit = U * p * (1.0 + 2.0 * E) + floor
    ratio = ((g.double() - p).abs() / unit)[~masked].max().item()
    if case.kind == "flat":   # 1 / lim, to the same bound
        flat_ratio = ((g.double() - 1.0 / lim[:, None].double()).abs() / unit)[~masked].max().item()
        ratio = max(ratio, flat_ratio)
    return (None if ratio <= SOFTMAX_CF else f"{ratio:.2f} u p (1 + 2 E) off, bound {SOFTMAX_CF}"), ratio


def softmax_bwd_check(case, p32, dp, got, floor=0.0):
    Cc = case.cols
    got = got.cpu()
    if not same_bits(got[:, Cc:], dp[:, Cc:]):
        return "elements cols .. ld were written", math.nan
    g = got[:, :Cc]
    if not bool(torch.isfinite(g).all()):
        return "NaN or inf", math.nan
    ds, unit = softmax_bwd_ref64(case, p32, dp)
    err = (g.double() - ds).abs()
    zero = unit == 0
    if bool((err[zero] != 0).any()):
        return "a masked column has a gradient", math.nan
    ratio = (err[~zero] / (U * unit[~zero] + floor)).max().item() if bool((~zero).any()) else 0.0
    return (None if ratio <= SOFTMAX_CB else f"{ratio:.2f} u |scale| p (|dp| + S) off, bound {SOFTMAX_CB}"), ratio


# ------------------------------------------------------------------------------------------------ element-wise
EW_SIZES = (1, 255, 256, 257)
BIG_N = 65535 * 256 + 300
PERIOD = 1021
FILL = float("nan")


def erff_saturation_points():
    """the smallest positive fp32 v at which a correctly rounded erff(fl(v / sqrt 2)) is 1.0f, and its mirror"""
    lo, hi = torch.tensor(3.0, dtype=F32), torch.tensor(8.0, dtype=F32)
    c = torch.tensor(INV_SQRT2, dtype=F32)
    while bits(hi).item() - bits(lo).item() > 1:
        mid = ((bits(lo).long() + bits(hi).long()) // 2).to(I32).view(F32)
        lo, hi = (lo, mid) if erf32(mid * c).item() == 1.0 else (mid, hi)
    return hi.item(), -hi.item()


EARLY_SATURATION = 5.419983386993408   # where an erff that is 1 ulp low at the top (torch's CPU fp32 erf is one) reaches 1.0f first


def gelu_inputs():
    """PERIOD fp32 values in [-10, 10]: the edges first, the neighbours of the saturation points, then a grid"""
    edges = [0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 1.0, -1.0, 5.5, -5.5, 8.0, -8.0, 10.0, -10.0]
    v = [torch.tensor(edges, dtype=F32)]
    for s in erff_saturation_points() + (EARLY_SATURATION, -EARLY_SATURATION):
        b = bits(torch.tensor(s, dtype=F32)).item()
        v.append((b + torch.arange(-32, 33)).to(I32).view(F32))
    n = PERIOD - sum(t.numel() for t in v)
    g = _gen("gelu")
    v.append((torch.rand(n, generator=g, dtype=F64) * 20.0 - 10.0).to(F32))
    x = torch.cat(v)
    assert x.numel() == PERIOD and float(x.abs().max()) <= 10.0
    return x


def tiled(pattern, n):
    return pattern.repeat(-(-n // pattern.numel()))[:n].clone()


def gelu_ref64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def dgelu_ref64(dy, x):
    x = x.double()
    return dy.double() * (0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


def gelu_fwd_ratio(x, got):
    ref = gelu_ref64(x)
    err = (got.cpu().double() - ref).abs()
    unit = U * (x.double().abs() + ref.abs())
    assert bool((err[unit == 0] == 0).all()), "gelu(+-0) is not 0"
    return (err[unit > 0] / unit[unit > 0]).max().item() if bool((unit > 0).any()) else 0.0


def gelu_bwd_ratio(dy, x, got):
    ref = dgelu_ref64(dy, x)
    unit = U * dy.double().abs() * (1.0 + x.double().abs())
    return ((got.cpu().double() - ref).abs() / unit).max().item()


def gelu_dy(n):
    dy = torch.randn(n, generator=_gen("gelu_dy", n)).to(F32)
    return torch.where(dy == 0, torch.ones_like(dy), dy)


AXPBY_PAIRS = ((1.0, 1.0), (1.0 - 1.0 / 0.9, 1.0 / 0.9), (0.5, -1.5), (-0.3, 0.7))


def axpby_inputs(n):
    g = _gen("axpby", n)
    return torch.randn(n, generator=g).to(F32), torch.randn(n, generator=g).to(F32)


def f32_scalar(a):
    return torch.tensor(a, dtype=F32)


def axpby_ratio(a, x, b, y, got):
    """|got - ref64| / (u (|a x| + |b y| + |ref|)), a and b as the fp32 values the ABI carries"""
    ax, by = f32_scalar(a).double() * x.double(), f32_scalar(b).double() * y.double()
    ref = ax + by
    return ((got.cpu().double() - ref).abs() / (U * (ax.abs() + by.abs() + ref.abs()))).max().item()


def tiled_mismatch(got, small_out, n, fill=FILL):
    """a big element-wise output must be the small case's output tiled with period PERIOD, bit for bit; -> None or a report"""
    want = bits(tiled(small_out.cpu(), n))
    g = bits(got)
    if torch.equal(g, want):
        return None
    bad = (g != want).nonzero().view(-1)
    return f"{bad.numel()} of {n} elements differ, first at {int(bad[0])} (trip {int(bad[0]) // (65535 * 256)} of the grid-stride loop)"


def second_trip_skipped(small_out, n, fill=FILL):
    """the mutant: elements from 65535 x 256 on left at their fill value"""
    out = tiled(small_out, n)
    out[65535 * 256:] = fill
    return out


COLSUM_ROWS, COLSUM_COLS = (1, 5, 300), (1, 63, 64, 65, 130)


def colsum_input(rows, cols, kind, seed):
    g = _gen("colsum", rows, cols, kind, seed)
    x = torch.full((rows, cols + 3), float("nan"), dtype=F32)
    x[:, :cols] = _ints((rows, cols), g) if kind == "int" else torch.randn(rows, cols, generator=g)
    return x


def colsum_expected(x, cols, kind, mutant=None):
    """integers: the float64 sum; randn: the fp32 running sum in row order"""
    if mutant == "colsum_ld_is_cols":
        x = torch.as_strided(x, (x.shape[0], cols), (cols, 1))
    if kind == "int":
        return x[:, :cols].double().sum(0).to(F32)
    s = torch.zeros(cols, dtype=F32)
    for r in range(x.shape[0]):
        s = s + x[r, :cols]
    return s
