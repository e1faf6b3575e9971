"""Cases, operand builders, float64 references, premises and mutants for the exact tests of the bf16 autograd functions of
engine/ops.py (ConvStemFn, LinearFn through ops.linear, TiedLogitsFn).  CPU only: tests/test_ops_exact_host.py proves what is
claimed here and shows that the comparison rejects every mutant; tests/test_ops_exact_gpu.py holds the functions to torch.equal.

The premise.  Operands are small integers (or halves, where the LoRA scaling 0.5 or a forward scale 0.25 makes them), so that every
value the engine stores in bf16 IS a bf16 number and every fp32 accumulation is exact in any order.  The result of the engine must then
equal a float64 autograd reference of the plain formula bit for bit, element by element: no tolerance appears anywhere.

The conditions, asserted in float64 by every builder for every case, seed and pass (`_check`):
  (a) x, every effective weight W + s B (A o m) (and its forward-scaled image), y, dx, every partial sum of the grouped dx of a fork,
      du and u of the rank-r products, s (A o m) and s B, pre and act, dpre and the padded activations are unchanged by a round trip
      through bf16;
  (b) sum |a||b| (+ |bias| + |residual|) of every product and every column sum stays below 2^24, so fp32 sums are exact in any order;
  (c) in the GELU cases every pre-activation is an integer in [8, 256].

The GELU argument.  For fp32 v >= 8 the three device formulas of csrc/common.h are exact: exp(-v^2 / 2) <= 1.3e-14, so the erfc
term is below 2^-25 and cdf rounds to 1.0f; g = v * 1.0f = v; d = fma(v, 0.3989 e, 1.0f) = 1.0f.  The one-byte code of 1.0 is
round(200 * 1.0) + 26 = 226, and the decoder's fma(226, 0.005f, -0.13f) rounds to 1.0f.  With every pre-activation an integer in
[8, 256] GELU is the identity and its derivative 1 in all three forms (bf16 gelu', one-byte codes, recomputed from pre), and the
reference needs no GELU.  `gelu_premise_cpu` restates the formulas in CPU fp32 for the host test; the GPU test asserts the same on the
device and the GELU-dependent tests say "premise" when that fails.

Densities.  x, dy and W are integers from -2..2 kept with probability min(1, c / sqrt(K)), c = 12 unless the case says otherwise;
A and B are from {-1, 0, 1} kept with probability `c_ab` (1 unless the case says otherwise); bias from -30..30, residual from -15..15,
mask from {0, 2}, s = 0.5.  What had to move from c = 12, c_ab = 1, and why (every case of LINEAR_CASES not named here runs at the figures above):
  * lora_qkv_masked, lora_qkv_unmasked, lora_qkv_d384_r16, lora_ranks_8_16, lora_mask_on_one: c = 8, c_ab = 0.5.  The effective weight
    W + 0.5 B (A o m) is wider than W: with this module's generator dx (and once y) left bf16's numbers (odd integers above 256, e.g.
    299, 375, 434; without a mask odd halves above 128, e.g. 178.5);
  * lora_total_rank_80 (ranks 32, 16, 32): c_ab = 0.25, for the same reason at four times the rank;
  * fork: c = 6.  The running sum of three consumers is stored in bf16 after every consumer, in whatever order autograd runs them, so
    EVERY subset sum (with and without the fourth, plain-autograd gradient) must be a bf16 number;
  * homes_qkv_segmented: c = 6: dx sums 768 terms per element over 16384 rows;
  * MLP pair: dy has four nonzeros from +-1, +-2 per row, so that |dx| <= sum |dy| * 8 <= 64 whatever the signs.
The one-byte MLP pair runs at the smallest (M, d) -- fewest elements M * d, then the narrower -- for which both wft_gemm_nt_aux8_bytes
queries of LinearFn.forward answer nonzero: M = 1793, d = 1024 on an MI355X (8 x 16 = 128 tiles of 256 x 256, the least the 256-tile
kernels take); the GPU test finds it through the queries.

One case takes another route than its size suggests: a single adapted Linear with rank 3, every gradient wanted and
n == npad meets LinearFn's `fused` condition, so the paired rank-r launch DOES run for it (lora_single_r3 asserts that); the same
adapter on out = 192 (n != npad) takes the general route (lora_single_r3_out192)."""
import math
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as Fn

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SEEDS = (0, 1)
PASSES = (0, 1)          # pass 1: after an in-place change of every parameter
LIMIT = float(2 ** 24)
SCALING = 0.5


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(shape, g, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


def _sparse(shape, g, p, lo=-2, hi=2):
    v = _ints(shape, g, lo, hi)
    return v if p >= 1.0 else v * (torch.rand(shape, generator=g) < p).to(F32)


def _signs(shape, g):
    return 2.0 * torch.randint(0, 2, shape, generator=g).to(F32) - 1.0


def round_up(x, m):
    return (x + m - 1) // m * m


def bf16_exact(t) -> bool:
    t = t.detach().double()
    return bool((t.to(BF16).double() == t).all())


def mismatch(got, want64, what) -> Optional[str]:
    """None if `got` equals the float64 reference cast to got's dtype, element for element (torch.equal); else a report that names the
    tensor, the first differing index, got and want there, and the count of differing elements."""
    got = got.detach().cpu()
    want = want64.detach().to(got.dtype)
    if got.shape != want.shape:
        return f"{what}: shape {tuple(got.shape)}, want {tuple(want.shape)}"
    if torch.equal(got, want):
        return None
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    return f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: got {got[i].item()!r}, want {want[i].item()!r}"


def first_mismatch(got: dict, want: dict, what) -> Optional[str]:
    assert list(got) == list(want), (what, list(got), list(want))
    for k in want:
        r = mismatch(got[k], want[k], f"{what} {k}")
        if r is not None:
            return r
    return None


def _check(bf16_named: dict, sums_named: dict, pre_named: dict, what):
    for k, v in bf16_named.items():
        assert bf16_exact(v), f"{what}: condition (a) fails for {k}: max |v| {float(v.abs().max())}"
    for k, v in sums_named.items():
        assert float(v.max()) < LIMIT, f"{what}: condition (b) fails for {k}: {float(v.max())}"
    for k, v in pre_named.items():
        assert float(v.min()) >= 8.0 and float(v.max()) <= 256.0 and bool((v == v.round()).all()), f"{what}: condition (c) fails for {k}"


# ------------------------------------------------------------------------------------------------ GELU premise
def gelu_premise_cpu(v):
    """gelu_f, gelu_both_f, dgelu_f of csrc/common.h and the one-byte code / decode of gemm_nt4w.hip in CPU fp32 (numpy float32; an fma
    is the float64 product and sum rounded once; rcp and exp2 are float32 division and exp2) -> dict of float32 arrays."""
    f = np.float32
    v = np.asarray(v, dtype=f)

    def fma(a, b, c):
        return (np.float64(a) * np.float64(b) + np.float64(c)).astype(f)

    def rcp(x):
        return (f(1.0) / x).astype(f)
    # gelu_f: 0.5 x (1 + erf_fast(x / sqrt 2))
    ax = np.abs(v * f(0.70710678118654752440))
    t = rcp(fma(f(0.3275911), ax, f(1.0)))
    poly = fma(f(1.061405429), t, f(-1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        poly = fma(poly, t, f(c))
    erf = np.copysign(f(1.0) - poly * t * np.exp(-ax * ax).astype(f), v)
    gelu = f(0.5) * v * (f(1.0) + erf)
    # dgelu_f
    e = np.exp2(v * v * f(-0.72134752044448170368)).astype(f)
    half_erfc = f(0.5) * poly * t * e
    cdf = np.where(v >= 0, f(1.0) - half_erfc, half_erfc).astype(f)
    dgelu = fma(v, f(0.39894228040143267794) * e, cdf)
    # gelu_both_f
    t2 = rcp(fma(f(0.23164189), np.abs(v), f(1.0)))
    xs = v * f(0.84932180)
    e2 = np.exp2(-(xs * xs)).astype(f)
    p2 = fma(f(0.5307027145), t2, f(-0.7265760135))
    for c in (0.7107068705, -0.142248368, 0.127414796):
        p2 = fma(p2, t2, f(c))
    he2 = p2 * t2 * e2
    cdf2 = np.where(v >= 0, f(1.0) - he2, he2).astype(f)
    both_g = v * cdf2
    both_d = fma(v, f(0.39894228040143267794) * e2, cdf2)
    # one-byte code: low byte of the bits of fma(d, 200, 1.5 * 2^23 + 26); decode: fma(code, 0.005f, -0.13f)
    code = fma(both_d, f(200.0), f(12582912.0 + 26.0)).view(np.uint32) & 0xFF
    decoded = fma(code.astype(f), f(0.005), f(-0.13))
    return {"gelu": gelu, "dgelu": dgelu, "both_g": both_g, "both_d": both_d, "code": code, "decoded": decoded}


GELU_RANGE = (8, 256)


# ------------------------------------------------------------------------------------------------ ConvStemFn
CONV_CASES = ((80, 128, 2, 2), (80, 128, 6, 1), (80, 128, 130, 3), (128, 384, 22, 3), (128, 384, 258, 1))   # (n_mels, d, T, B)
CONV_MUTANTS = ("window_stride_1", "halo_not_zero", "taps_reversed", "odd_even_rows_swapped", "even_taps_swapped",
                "last_even_row_dropped", "dw2_window_one_row_late", "db1_counts_a_halo_row")
CONV_CHECKED = ("out", "dw1", "db1", "dw2", "db2")
# T = 2 has one output row: a window of stride 1 starts where the window of stride 2 does
CONV_NEVER = {"window_stride_1": {(80, 128, 2, 2)}}


def conv_tap_slots(d, cin):
    """flat slots ((4c + j) * 7) mod (3 cin), j = 0..3, of the [kk, ci] plane of channel c: int64 [d, 4]"""
    c = torch.arange(d).view(-1, 1)
    j = torch.arange(4).view(1, -1)
    return ((4 * c + j) * 7) % (3 * cin)


def _tap_weight(d, cin, g):
    slots = conv_tap_slots(d, cin)
    plane = torch.zeros(d, 3 * cin)
    plane.scatter_(1, slots, _signs((d, 4), g))
    return plane.view(d, 3, cin).permute(0, 2, 1).contiguous()   # [co, ci, kk]


def conv_inputs(case, seed, w2_sign=1.0):
    """w2_sign = -1: the operands after the in-place change w2 <- -w2 (b2 is symmetric in the sign of w2 and stays)"""
    n_mels, d, T, B = case
    g = _gen("conv", case, seed)
    t = {"mel": _ints((B, n_mels, T), g), "pos": _ints((T // 2, d), g), "dx": _ints((B, T // 2, d), g),
         "w1": _tap_weight(d, n_mels, g), "w2": _tap_weight(d, d, g)}
    t["b1"] = 8.0 + 2.0 * t["w1"].abs().sum((1, 2))                       # |mel| <= 2
    act1 = Fn.conv1d(t["mel"].double(), t["w1"].double(), t["b1"].double(), padding=1)
    t["b2"] = (8.0 + float(act1.max()) * t["w2"].abs().sum((1, 2)).double()).to(F32)
    t["w2"] = w2_sign * t["w2"]
    return t


def conv_ref64(t):
    """float64 autograd, no GELU: conv1d(pad 1) -> conv1d(stride 2, pad 1) -> permute -> + pos"""
    p = {k: t[k].double().requires_grad_(k in ("w1", "b1", "w2", "b2")) for k in ("mel", "w1", "b1", "w2", "b2", "pos")}
    pre1 = Fn.conv1d(p["mel"], p["w1"], p["b1"], padding=1)
    pre2 = Fn.conv1d(pre1, p["w2"], p["b2"], stride=2, padding=1)
    out = pre2.permute(0, 2, 1) + p["pos"]
    out.backward(t["dx"].double())
    return {"pre1": pre1.detach().permute(0, 2, 1), "pre2": pre2.detach().permute(0, 2, 1), "out": out.detach(), "dw1": p["w1"].grad,
            "db1": p["b1"].grad, "dw2": p["w2"].grad, "db2": p["b2"].grad}


def conv_restate(t, mutant=None):
    """ConvStemFn's forward and backward restated in float64 on its own layout (time-major, zero halo rows 0 and T + 1, overlapping
    windows, odd / even padded rows of the backward-data, column sums over the halo rows); GELU left out (the premise).  The mutants
    are the ways the stride recipes go wrong.  Also returns dpre1 (padded) for the premises."""
    mel, w1, b1, w2, b2, pos, dx = (t[k].double() for k in ("mel", "w1", "b1", "w2", "b2", "pos", "dx"))
    B, cin, T = mel.shape
    d, T2 = w1.shape[0], T // 2
    halo = 1.0 if mutant == "halo_not_zero" else 0.0
    melp = torch.full((B, T + 2, cin), halo, dtype=F64)
    melp[:, 1:T + 1] = mel.permute(0, 2, 1)
    w1k, w2k = w1.permute(0, 2, 1), w2.permute(0, 2, 1)          # [co, kk, ci]
    if mutant == "taps_reversed":
        w1k, w2k = w1k.flip(1), w2k.flip(1)
    win1 = torch.stack([melp[:, kk:kk + T] for kk in range(3)], 2)                                  # [B, T, 3, cin]
    pre1 = torch.einsum("btkc,okc->bto", win1, w1k) + b1
    act1p = torch.full((B, T + 2, d), halo, dtype=F64)
    act1p[:, 1:T + 1] = pre1
    step = 1 if mutant == "window_stride_1" else 2
    win2 = torch.stack([act1p[:, kk:kk + step * (T2 - 1) + 1:step] for kk in range(3)], 2)         # [B, T2, 3, d]
    pre2 = torch.einsum("btkc,okc->bto", win2, w2k) + b2
    out = pre2 + pos
    # backward
    dpre2 = dx
    db2 = dpre2.sum((0, 1))
    late = 1 if mutant == "dw2_window_one_row_late" else 0
    act_b = torch.cat([act1p, torch.zeros((B, 1, d), dtype=F64)], 1)
    winb = torch.stack([act_b[:, kk + late:kk + late + 2 * (T2 - 1) + 1:2] for kk in range(3)], 2)
    dw2 = torch.einsum("bto,btkc->okc", dpre2, winb).permute(0, 2, 1)
    nxt = torch.cat([dpre2[:, 1:], torch.zeros((B, 1, d), dtype=F64)], 1)                           # dpre2[j + 1], zero halo behind the last
    odd = torch.einsum("bjo,oc->bjc", dpre2, w2[:, :, 1])                                           # padded rows 2j + 1
    ta, tb = (0, 2) if mutant == "even_taps_swapped" else (2, 0)
    even = torch.einsum("bjo,oc->bjc", dpre2, w2[:, :, ta]) + torch.einsum("bjo,oc->bjc", nxt, w2[:, :, tb])   # padded rows 2j + 2
    if mutant == "last_even_row_dropped":
        even[:, T2 - 1] = 0.0
    dpre1p = torch.zeros((B, T + 2, d), dtype=F64)
    if mutant == "odd_even_rows_swapped":
        odd, even = even, odd
    dpre1p[:, 1:T:2] = odd
    dpre1p[:, 2:T + 1:2] = even
    db1 = dpre1p.sum((0, 1))
    if mutant == "db1_counts_a_halo_row":     # padded row 0 computed like an even row (j = 0) and summed
        db1 = db1 + torch.einsum("bo,oc->bc", dpre2[:, 0], w2[:, :, 0]).sum(0)
    dw1 = torch.einsum("bto,btkc->okc", dpre1p[:, 1:T + 1], win1).permute(0, 2, 1)
    return {"pre1": pre1, "pre2": pre2, "out": out, "dw1": dw1, "db1": db1, "dw2": dw2, "db2": db2, "dpre1p": dpre1p}


def conv_premises(t, what):
    r = conv_restate(t)
    a = {k: t[k].double().abs().requires_grad_(k in ("w1", "b1", "w2", "b2")) for k in ("mel", "w1", "b1", "w2", "b2", "pos", "dx")}
    pre1 = Fn.conv1d(a["mel"], a["w1"], a["b1"], padding=1)
    out = Fn.conv1d(pre1, a["w2"], a["b2"], stride=2, padding=1).permute(0, 2, 1) + a["pos"]
    out.backward(a["dx"])
    # (every entry of the backward-data buffer is a term of db1's sums on absolute values, so db1 bounds it)
    sums = {"out": out.detach(), "dw1": a["w1"].grad, "db1": a["b1"].grad, "dw2": a["w2"].grad, "db2": a["b2"].grad}
    _check({k: t[k] for k in ("mel", "w1", "w2", "pos", "dx")} | {k: r[k] for k in ("pre1", "pre2", "out", "dpre1p")}, sums,
           {"pre1": r["pre1"], "pre2": r["pre2"]}, what)
    return r


# ------------------------------------------------------------------------------------------------ LinearFn
@dataclass(frozen=True)
class Lora:
    rank: int
    masked: bool = True
    train_a: bool = True
    train_b: bool = True


@dataclass(frozen=True)
class LinCase:
    name: str
    K: int
    outs: Tuple[int, ...]
    M: int = 37
    bias: Optional[Tuple[bool, ...]] = None          # None: every weight has one
    residual: bool = False
    loras: Optional[Tuple[Optional[Lora], ...]] = None
    fwd_scales: Optional[Tuple[float, ...]] = None
    c: float = 12.0                                    # density of x, dy, W: min(1, c / sqrt(K))
    c_ab: float = 1.0                                  # density of A and B
    fused: Optional[bool] = None                       # LoRA: does the backward take the gemm_*_rank_pair route?

    def __str__(self):
        return self.name

    @property
    def has_bias(self):
        return self.bias if self.bias is not None else (True,) * len(self.outs)

    @property
    def n(self):
        return sum(self.outs)

    @property
    def npad(self):
        return round_up(self.n, 128)

    @property
    def lora_list(self):
        return self.loras if self.loras is not None else (None,) * len(self.outs)


_QKV = (True, False, True)   # whisper's key projection has no bias
_L8 = Lora(8)
LINEAR_CASES = (
    # plain
    LinCase("plain_bias_residual", 128, (128,), M=37, residual=True),
    LinCase("plain_bias_residual_m300", 128, (128,), M=300, residual=True),
    LinCase("plain_no_bias", 128, (128,), M=37, bias=(False,)),
    LinCase("plain_out192", 128, (192,), M=300),
    LinCase("plain_k1536", 1536, (384,), M=37, residual=True),
    # group of three
    LinCase("qkv", 128, (128,) * 3, M=300, bias=_QKV),
    LinCase("qkv_d384", 384, (384,) * 3, M=37, bias=_QKV),
    LinCase("qkv_fwd_scaled", 128, (128,) * 3, M=300, bias=_QKV, fwd_scales=(0.25, 1.0, 1.0)),
    # LoRA, fused route
    LinCase("lora_qkv_masked", 128, (128,) * 3, M=300, bias=_QKV, loras=(_L8,) * 3, c=8.0, c_ab=0.5, fused=True),
    LinCase("lora_qkv_unmasked", 128, (128,) * 3, M=37, bias=_QKV, loras=(Lora(8, masked=False),) * 3, c=8.0, c_ab=0.5, fused=True),
    LinCase("lora_qkv_d384_r16", 384, (384,) * 3, M=37, bias=_QKV, loras=(Lora(16),) * 3, c=8.0, c_ab=0.5, fused=True),
    LinCase("lora_qkv_scaled", 128, (128,) * 3, M=37, bias=_QKV, loras=(_L8,) * 3, fwd_scales=(0.25, 1.0, 1.0), fused=True),
    # (a single adapted Linear with every gradient wanted and n == npad meets LinearFn's `fused` condition: the pair launch runs)
    LinCase("lora_single_r3", 1536, (384,), M=37, loras=(Lora(3),), fused=True),
    # LoRA, general route
    LinCase("lora_only_v", 128, (128,) * 3, M=37, bias=_QKV, loras=(None, None, _L8), fused=False),
    LinCase("lora_a_frozen", 128, (128,) * 3, M=37, bias=_QKV, loras=(Lora(8, train_a=False),) * 3, fused=False),
    LinCase("lora_b_frozen", 128, (128,) * 3, M=37, bias=_QKV, loras=(Lora(8, train_b=False),) * 3, fused=False),
    LinCase("lora_ranks_8_16", 128, (128,) * 3, M=300, bias=_QKV, loras=(_L8, Lora(16), _L8), c=8.0, c_ab=0.5, fused=False),
    LinCase("lora_total_rank_80", 128, (128,) * 3, M=37, bias=_QKV, loras=(Lora(32), Lora(16), Lora(32)), c_ab=0.25, fused=False),
    LinCase("lora_mask_on_one", 128, (128,) * 3, M=37, bias=_QKV, loras=(Lora(8, masked=False), _L8, Lora(8, masked=False)), c=8.0, c_ab=0.5,
            fused=False),
    LinCase("lora_single_r3_out192", 128, (192,), M=37, loras=(Lora(3),), fused=False),
)
LINEAR_MUTANTS = ("bias_one_weight_late", "k_slice_given_bias", "mask_missing_from_dA", "mask_applied_twice", "scaling_twice_on_dB",
                  "dB_blocks_swapped", "dB_block_transposed", "residual_grad_dropped", "padded_columns_nonzero", "scale_reaches_WT")


def linear_mutant_applies(case: LinCase, mutant) -> bool:
    """does the mutant change an operand or a formula of this case at all"""
    ad = [s for s in case.lora_list if s is not None]
    return {
        "bias_one_weight_late": len(case.outs) > 1 and any(case.has_bias),
        "k_slice_given_bias": not all(case.has_bias) and any(case.has_bias),
        "mask_missing_from_dA": any(s.masked and s.train_a for s in ad),
        "mask_applied_twice": any(s.masked and s.train_a for s in ad),
        "scaling_twice_on_dB": any(s.train_b for s in ad),
        "dB_blocks_swapped": len(ad) > 1 and all(s.train_b for s in ad),
        "dB_block_transposed": any(s.train_b for s in ad),
        "residual_grad_dropped": case.residual,
        "padded_columns_nonzero": case.n != case.npad,
        "scale_reaches_WT": case.fwd_scales is not None,
    }[mutant]


def linear_operands(case: LinCase, seed, pas=0):
    """-> dict: x [M, K], dy [M, npad], res [M, npad] or None, W / b / A / B / mask: lists per weight (None where absent)"""
    g = _gen("linear", case.name, seed, pas)
    p = min(1.0, case.c / math.sqrt(case.K))
    M, K = case.M, case.K
    t = {"x": _sparse((M, K), g, p), "dy": _sparse((M, case.npad), g, p),
         "res": _ints((M, case.npad), g, -15, 15) if case.residual else None, "W": [], "b": [], "A": [], "B": [], "mask": []}
    for o, hb, sp in zip(case.outs, case.has_bias, case.lora_list):
        t["W"].append(_sparse((o, K), g, p))
        t["b"].append(_ints((o,), g, -30, 30) if hb else None)
        t["A"].append(None if sp is None else _sparse((sp.rank, K), g, case.c_ab, -1, 1))
        t["B"].append(None if sp is None else _sparse((o, sp.rank), g, case.c_ab, -1, 1))
        t["mask"].append(None if sp is None or not sp.masked else 2.0 * torch.randint(0, 2, (1, K), generator=g).to(F32))
    return t


def linear_ref64(case: LinCase, t, mutant=None):
    """float64 autograd of x @ (W + s B (A o m))^T + b (+ residual), once per weight of the group, the outputs side by side and padded
    with zero columns to npad.  With fwd_scales the forward output of weight i is f_i times that; the backward is that of the UNscaled
    projection.  -> (checked tensors in a fixed order, premise tensors).  The mutants are wrong references."""
    x = t["x"].double().requires_grad_(True)
    dy = t["dy"].double()
    M = case.M
    leaves, ys, weffs, blocks = {}, [], [], []
    nw = len(case.outs)
    for i, (o, sp) in enumerate(zip(case.outs, case.lora_list)):
        W = leaves[f"dW{i}"] = t["W"][i].double().requires_grad_(True)
        weff = W
        if sp is not None:
            A = t["A"][i].double().requires_grad_(True)
            Bm = t["B"][i].double().requires_grad_(True)
            if sp.train_a:
                leaves[f"dA{i}"] = A
            if sp.train_b:
                leaves[f"dB{i}"] = Bm
            am = A * t["mask"][i].double() if t["mask"][i] is not None else A
            weff = W + SCALING * (Bm @ am)
        weffs.append(weff.detach())
        ys.append(x @ weff.T)
    biases = [None if b is None else b.double().requires_grad_(True) for b in t["b"]]
    for i, b in enumerate(biases):
        if b is not None:
            leaves[f"db{i}"] = b
    added = list(biases)
    if mutant == "bias_one_weight_late":
        added = [biases[(i - 1) % nw] for i in range(nw)]
    elif mutant == "k_slice_given_bias":
        first = next(b for b in biases if b is not None)
        added = [first if b is None else b for b in biases]
    ys = [y if b is None else y + b for y, b in zip(ys, added)]
    y_un = torch.cat(ys + [torch.zeros((M, case.npad - case.n), dtype=F64)], 1)
    res = None
    if case.residual:
        res = t["res"].double().requires_grad_(True)
        y_un = y_un + res
    y_un.backward(dy)
    y = y_un.detach().clone()
    off = 0
    for i, o in enumerate(case.outs):
        if case.fwd_scales is not None:
            y[:, off:off + o] *= case.fwd_scales[i]
        off += o
    if mutant == "padded_columns_nonzero":
        y[:, case.n:] = 1.0
    dx = x.grad
    if mutant == "scale_reaches_WT":
        dx, off = torch.zeros_like(dx), 0
        for i, o in enumerate(case.outs):
            dx = dx + dy[:, off:off + o] @ (case.fwd_scales[i] * weffs[i])
            off += o
    out = {"y": y, "dx": dx}
    if case.residual:
        out["dres"] = torch.zeros_like(res.grad) if mutant == "residual_grad_dropped" else res.grad
    # the order LinearFn returns them in: weights, biases, A, B
    for kind in ("dW", "db", "dA", "dB"):
        for i in range(nw):
            if f"{kind}{i}" in leaves:
                out[f"{kind}{i}"] = leaves[f"{kind}{i}"].grad
    ad = [i for i, sp in enumerate(case.lora_list) if sp is not None]
    for i in ad:
        sp, m = case.lora_list[i], t["mask"][i]
        if sp.train_a and m is not None and mutant in ("mask_missing_from_dA", "mask_applied_twice"):
            off = sum(case.outs[:i])
            plain = SCALING * t["B"][i].double().T @ (dy[:, off:off + case.outs[i]].T @ t["x"].double())
            out[f"dA{i}"] = plain if mutant == "mask_missing_from_dA" else plain * m.double() * m.double()
        if sp.train_b and mutant == "scaling_twice_on_dB":
            out[f"dB{i}"] = out[f"dB{i}"] * SCALING
        if sp.train_b and mutant == "dB_block_transposed":
            out[f"dB{i}"] = out[f"dB{i}"].T.contiguous().view(out[f"dB{i}"].shape)
    if mutant == "dB_blocks_swapped":
        a, b = ad[0], ad[-1]
        out[f"dB{a}"], out[f"dB{b}"] = out[f"dB{b}"], out[f"dB{a}"]
    # premise tensors
    xa, dya = t["x"].double().abs(), dy.abs()
    prem_bf16 = {"x": t["x"], "y": y, "y_unscaled_dy": dy, "dx": x.grad}
    sums = {"dy colsum": dya.sum(0), "dW": dya.T @ xa}
    off = 0
    for i, (o, sp) in enumerate(zip(case.outs, case.lora_list)):
        f = 1.0 if case.fwd_scales is None else case.fwd_scales[i]
        prem_bf16[f"weff{i}"] = weffs[i]
        prem_bf16[f"fwd weff{i}"] = f * weffs[i]
        ba = 0.0 if t["b"][i] is None else t["b"][i].double().abs()
        ra = 0.0 if t["res"] is None else t["res"][:, off:off + o].double().abs()
        sums[f"y{i}"] = xa @ weffs[i].abs().T + ba + ra
        sums[f"dx{i}"] = dya[:, off:off + o] @ weffs[i].abs()
        if sp is not None:
            sam = SCALING * (t["A"][i].double() * (t["mask"][i].double() if t["mask"][i] is not None else 1.0))
            sb = SCALING * t["B"][i].double()
            du, u = dy[:, off:off + o] @ sb, t["x"].double() @ sam.T
            prem_bf16 |= {f"sAm{i}": sam, f"sB{i}": sb, f"du{i}": du, f"u{i}": u}
            sums |= {f"du{i}": dya[:, off:off + o] @ sb.abs(), f"u{i}": xa @ sam.abs().T, f"dA{i}": du.abs().T @ xa,
                     f"dB{i}": u.abs().T @ dya[:, off:off + o]}
        off += o
    sums["dx"] = sum(sums[f"dx{i}"] for i in range(nw))
    return out, (prem_bf16, sums)


def linear_case(case: LinCase, seed, pas=0):
    """-> (operands, checked float64 results); asserts the conditions"""
    t = linear_operands(case, seed, pas)
    ref, (prem, sums) = linear_ref64(case, t)
    _check(prem, sums, {}, f"{case.name} seed {seed} pass {pas}")
    return t, ref


# ------------------------------------------------------------------------------------------------ MLP pair
MLP_CASES = ((37, 128), (300, 128))     # (M, d), the bf16 form
MLP_CHECKED = ("y", "dx", "dres", "dW1", "db1", "dW2", "db2")
MLP_MUTANTS = ("gelu_derivative_half", "db1_from_dy", "residual_grad_dropped")


# the smallest (M, d) for which both wft_gemm_nt_aux8_bytes queries of LinearFn.forward answer nonzero, as the GPU test found it on an
# MI355X (it searches M <= 4096, d <= 1024 itself and runs whatever it finds; the host test builds the premises at this one)
AUX8_SHAPE_OBSERVED = (1793, 1024)


def mlp_operands(M, d, seed, pas=0):
    g = _gen("mlp", M, d, seed, pas)
    h = 4 * d
    x = torch.zeros(M, d)
    x.scatter_(1, torch.randint(0, d, (M, 4), generator=g), _signs((M, 4), g))          # at most four +-1 per row
    w1 = _ints((h, d), g, -1, 1)
    b1 = torch.full((h,), 8.0 + float((x.double() @ w1.double().T).abs().max()))
    i = torch.arange(d).view(-1, 1)
    j = torch.arange(8).view(1, -1)
    cols = ((8 * i + j) * 7) % h
    w2 = torch.zeros(d, h)
    w2.scatter_(1, cols, _signs((d, 8), g))
    dy = torch.zeros(M, d)
    dy.scatter_(1, torch.randint(0, d, (M, 4), generator=g), _signs((M, 4), g) * torch.randint(1, 3, (M, 4), generator=g))
    return {"x": x, "w1": w1, "b1": b1, "w2": w2, "b2": _ints((d,), g, -30, 30), "res": _ints((M, d), g, -15, 15), "dy": dy,
            "w2_cols": cols}


def mlp_ref64(t, mutant=None):
    """float64 autograd of (x W1^T + b1) W2^T + b2 + r: GELU is the identity on pre >= 8 (the premise)"""
    p = {k: t[k].double().requires_grad_(True) for k in ("x", "w1", "b1", "w2", "b2", "res")}
    pre = p["x"] @ p["w1"].T + p["b1"]
    y = pre @ p["w2"].T + p["b2"] + p["res"]
    y.backward(t["dy"].double())
    out = {"y": y.detach(), "dx": p["x"].grad, "dres": p["res"].grad, "dW1": p["w1"].grad, "db1": p["b1"].grad, "dW2": p["w2"].grad,
           "db2": p["b2"].grad}
    if mutant == "gelu_derivative_half":    # what flows back through the activation is halved: dx, dW1, db1
        for k in ("dx", "dW1", "db1"):
            out[k] = out[k] * 0.5
    if mutant == "db1_from_dy":
        out["db1"] = torch.cat([out["db2"]] * 4)
    if mutant == "residual_grad_dropped":
        out["dres"] = torch.zeros_like(out["dres"])
    dpre = t["dy"].double() @ t["w2"].double()
    return out, pre.detach(), dpre


def mlp_case(M, d, seed, pas=0):
    t = mlp_operands(M, d, seed, pas)
    ref, pre, dpre = mlp_ref64(t)
    a = {k: t[k].double().abs() for k in ("x", "w1", "b1", "w2", "b2", "res", "dy")}
    pre_a = a["x"] @ a["w1"].T + a["b1"]
    dpre_a = a["dy"] @ a["w2"]
    sums = {"pre": pre_a, "y": pre_a @ a["w2"].T + a["b2"] + a["res"], "dpre": dpre_a, "dx": dpre_a @ a["w1"], "dW1": dpre_a.T @ a["x"],
            "db1": dpre_a.sum(0), "dW2": a["dy"].T @ pre_a, "db2": a["dy"].sum(0)}
    _check({"x": t["x"], "w1": t["w1"], "w2": t["w2"], "pre": pre, "y": ref["y"], "res": t["res"], "dy": t["dy"], "dpre": dpre, "dx": ref["dx"]},
           sums, {"pre": pre}, f"mlp {M} x {d} seed {seed} pass {pas}")
    return t, ref


# ------------------------------------------------------------------------------------------------ fork
FORK_CASES = ((37, 128, (128, 128, 256)), (300, 128, (128, 256, 128)))   # (M, K, out-features of the three consumers)
FORK_C = 6.0
FORK_MUTANTS = ("fork_sum_misses_a_consumer",)


def fork_case(case, seed, left_out=None, mutant=None):
    """three Linear consumers of one forked x and a fourth use x * g4 through plain autograd.  left_out: index of a consumer that takes
    no part in the backward.  -> (operands, {"dx": float64 sum, "dW{i}", "db{i}"}); asserts that EVERY subset sum of the consumers' dx
    (with and without g4) is a bf16 number: the running sum is stored in bf16 in whatever order autograd runs the consumers."""
    M, K, outs = case
    g = _gen("fork", case, seed)
    p = min(1.0, FORK_C / math.sqrt(K))
    t = {"x": _sparse((M, K), g, p), "g4": _ints((M, K), g), "W": [_sparse((o, K), g, p) for o in outs],
         "b": [_ints((o,), g, -30, 30) for o in outs], "dy": [_sparse((M, o), g, p) for o in outs]}
    x64 = t["x"].double()
    parts = [dy.double() @ W.double() for dy, W in zip(t["dy"], t["W"])]
    for mask in range(1, 8):
        s = sum(parts[i] for i in range(3) if mask >> i & 1)
        assert bf16_exact(s) and bf16_exact(s + t["g4"].double()), f"fork {case} seed {seed}: condition (a) fails for subset {mask:03b}"
    sums = {}
    for i in range(3):
        assert bf16_exact(x64 @ t["W"][i].double().T + t["b"][i].double()), f"fork {case}: y{i}"
        sums[f"y{i}"] = x64.abs() @ t["W"][i].double().abs().T + t["b"][i].double().abs()
        sums[f"dW{i}"] = t["dy"][i].double().abs().T @ x64.abs()
    sums["dx"] = sum(dy.double().abs() @ W.double().abs() for dy, W in zip(t["dy"], t["W"])) + t["g4"].double().abs()
    _check({}, sums, {}, f"fork {case} seed {seed}")
    live = [i for i in range(3) if i != left_out]
    counted = live[:-1] if mutant == "fork_sum_misses_a_consumer" else live
    ref = {"dx": sum(parts[i] for i in counted) + t["g4"].double()}
    for i in live:
        ref[f"dW{i}"] = t["dy"][i].double().T @ x64
        ref[f"db{i}"] = t["dy"][i].double().sum(0)
    return t, ref


# ------------------------------------------------------------------------------------------------ gradient homes
# the small group's weight-gradient product is not one the library writes in segments (wft_gemm_tn_segments_ok: the 256 x 256 kernels
# only): LinearFn falls back to one tensor and slices, autograd accumulates.  The large one (256 reduction steps of 64 rows) is the
# smallest that takes the homes for real.
HOME_CASES = (LinCase("homes_qkv_small", 128, (128,) * 3, M=37, bias=_QKV),
              LinCase("homes_qkv_segmented", 256, (256,) * 3, M=16384, bias=_QKV, c=6.0))
HOME_PASSES = 3


def home_seeds(case):
    """the 16384-row case runs on one seed: its float64 reference is the slowest thing the CPU does here"""
    return SEEDS if case.M <= 300 else SEEDS[:1]


HOME_MUTANTS = ("home_overwritten",)


def homes_case(case: LinCase, seed, mutant=None):
    """three backward passes over the SAME parameters with fresh x / dy each: -> (list of per-pass (operands, results), float64 sums of
    the parameter gradients over the three passes)"""
    base = linear_operands(case, seed, 0)
    ts, total = [], {}
    for pas in range(HOME_PASSES):
        t = linear_operands(case, seed, pas)
        t["W"], t["b"] = base["W"], base["b"]
        ref, (prem, sums) = linear_ref64(case, t)
        _check(prem, {k: v * HOME_PASSES for k, v in sums.items()}, {}, f"{case.name} seed {seed} pass {pas}")
        for k, v in ref.items():
            if k[:2] in ("dW", "db"):
                total[k] = v if (k not in total or (mutant == "home_overwritten" and k[:2] == "dW")) else total[k] + v
        ts.append((t, ref))
    return ts, total


# ------------------------------------------------------------------------------------------------ TiedLogitsFn
TIED_V, TIED_D = 300, 128
TIED_ROWS = (7, 300)
TIED_MUTANTS = ("padding_columns_nonzero", "dE_from_padded_rows", "dx_reads_padding")


def tied_case(rows, seed, pas=0, mutant=None):
    V, d, Vpad = TIED_V, TIED_D, round_up(TIED_V, 128)
    g = _gen("tied", rows, seed, pas)
    t = {"x": _ints((rows, d), g), "emb": _ints((V, d), g), "dl": _ints((rows, Vpad), g)}
    x, e, dl = (v.double() for v in (t["x"], t["emb"], t["dl"]))
    logits = torch.cat([x @ e.T, torch.zeros((rows, Vpad - V), dtype=F64)], 1)
    ref = {"logits": logits, "dx": dl[:, :V] @ e, "dE": dl[:, :V].T @ x}
    _check({"x": x, "emb": e, "dl": dl, "logits": logits, "dx": ref["dx"]},
           {"logits": x.abs() @ e.abs().T, "dx": dl.abs()[:, :V] @ e.abs(), "dE": dl.abs().T @ x.abs()}, {}, f"tied rows {rows} seed {seed}")
    if mutant == "padding_columns_nonzero":
        ref["logits"] = logits.clone()
        ref["logits"][:, V:] = 1.0
    elif mutant == "dE_from_padded_rows":      # the slice taken one row late
        ref["dE"] = (dl.T @ x)[1:V + 1]
    elif mutant == "dx_reads_padding":         # the padding rows of the transposed shadow not zero
        ref["dx"] = ref["dx"] + dl[:, V:].sum(1, keepdim=True)
    return t, ref
