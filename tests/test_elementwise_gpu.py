"""The element-wise bf16 kernels of csrc/elementwise.hip and the casts of csrc/shadow.hip, per element, at the sizes where their
three paths can go wrong: the 16-byte vector loop (8 elements per lane, a grid-stride loop over at most 4096 workgroups of 256
lanes) and the scalar tail of the last n % 8 elements in workgroup 0.

    n = 1, 7                     tail only
    n = 8                        one vector, no tail
    n = 2053                     vectors plus a tail
    n = 4096 * 256 * 8 + 2403    the first size at which the capped grid's stride loop takes a second trip, with a tail left

cast_bf16, cast_f32, add_bf16 and the one-operand axpby_bf16 round an fp32 value that the CPU forms exactly as the kernel does:
torch.equal.  Two-operand axpby_bf16 keeps the bound of test_kernels_gpu.test_sd_rescale_kernel_and_transpose, 2^-7 max|want|
(the kernel may contract a*x + b*y into one fma; the CPU does not).  Kept sd_select blocks are the bits of axpby_bf16 on the same
operands (in the forward both run one shared 8-element body, so its arithmetic is checked by test_axpby alone); skipped ones pass
x / dy through and write zeros, with a NaN-filled block output.

dgelu_mul is compared with dy * gelu'(pre) in float64 with the exact erf, gelu'(x) = Phi(x) + x phi(x), on bf16 inputs with pre
in [-6, 6] (both ends, both zeros and the smallest steps round 0 and 6 among them).  Per element

    |got - ref| <= half a bf16 ulp at ref + C * |dy|

where the first term is the output rounding and C covers the kernel's fp32 evaluation of gelu' (erf_fast: Abramowitz & Stegun
7.1.26, |abs err| < 1.5e-7 on erf, so about 0.75e-7 on Phi; v_exp_f32, v_rcp_f32 and the fp32 products add a few 2^-24 relative).
C is 4 x the worst (|got - ref| - half ulp) / |dy| over all five sizes, measured on an MI355X with the library built from the
commit BEFORE the kernel was rewritten with bf8_unpack / bf8_pack (the convention of _loss_head_cases.py):

    measured worst ratio 1.3615e-07 (at n = 8 391 011; 6.15e-09 at 2053, 0 at 1, 7 and 8)      C = 4 x that = 5.446e-07
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from whisper_finetune.engine import kernels as K  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
SIZES = [1, 7, 8, 2053, 4096 * 256 * 8 + 2403]
KEEP = 0.9

DGELU_WORST = 1.3615237882307958e-07
DGELU_C = 4 * DGELU_WORST

PRE_EDGES = (-6.0, 6.0, 0.0, -0.0, 5.96875, -5.96875, 2.0 ** -126, -(2.0 ** -126), 1.0, -1.0)


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """CPU operands of size n: src f32; x, y, dy bf16 ~ N(0, 1); pre bf16 uniform in [-6, 6] behind the edge values."""
    g = torch.Generator().manual_seed(n)
    src = torch.randn(n, generator=g) * 3
    x, y, dy = (torch.randn(n, generator=g).to(BF16) for _ in range(3))
    pre = (torch.rand(n, generator=g) * 12 - 6).to(BF16)
    k = min(n, len(PRE_EDGES))
    pre[:k] = torch.tensor(PRE_EDGES[:k]).to(BF16)
    return src, x, y, dy, pre


@functools.lru_cache(maxsize=None)
def _dgelu_table():
    """gelu'(x) in float64 for every bf16 bit pattern x (the NaN patterns give NaN: no input holds one)"""
    p = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16).double()
    return 0.5 * (1 + torch.erf(p / math.sqrt(2))) + p * torch.exp(-0.5 * p * p) / math.sqrt(2 * math.pi)


@functools.lru_cache(maxsize=None)
def _dgelu_ref(n):
    """-> (ref float64, half a bf16 ulp at ref, |dy| float64)"""
    _, _, _, dy, pre = _inputs(n)
    d = dy.double()
    ref = d * _dgelu_table()[pre.view(torch.int16).long() & 0xffff]
    # bf16: 8 significant bits; |ref| = m * 2^e with m in [0.5, 1) -> ulp = 2^(e - 8); below the normal range the spacing is 2^-133
    e = torch.where(ref == 0, -125, torch.frexp(ref)[1]).clamp(min=-125)
    half_ulp = torch.ldexp(torch.ones_like(ref), e - 9)
    return ref, half_ulp, d.abs()


def dgelu_worst_ratio(n):
    """max over the elements of (|got - ref| - half ulp) / |dy|: the smallest C with which size n passes (inf: none does)."""
    _, _, _, dy, pre = _inputs(n)
    ref, half_ulp, ady = _dgelu_ref(n)
    got = K.dgelu_mul(dy.to(DEV), pre.to(DEV)).cpu().double()
    excess = (got - ref).abs() - half_ulp
    ratio = torch.where(excess > 0, excess / ady, torch.zeros_like(excess))  # dy = 0 with an error: x / 0 = inf
    ratio = torch.where(torch.isnan(got), torch.full_like(ratio, math.inf), ratio)
    return ratio.max().item()


@pytest.mark.parametrize("n", SIZES)
def test_casts_and_add_bit_exact(n):
    src, x, y, _, _ = _inputs(n)
    assert torch.equal(K.cast_bf16(src.to(DEV)).cpu(), src.to(BF16))
    assert torch.equal(K.cast_f32(x.to(DEV)).cpu(), x.float())
    assert torch.equal(K.add_bf16(x.to(DEV), y.to(DEV)).cpu(), (x.float() + y.float()).to(BF16))


@pytest.mark.parametrize("n", SIZES)
def test_axpby(n):
    _, x, y, _, _ = _inputs(n)
    s = 1.0 / KEEP
    got = K.axpby_bf16(1 - s, x.to(DEV), s, y.to(DEV)).cpu()
    want = ((1 - s) * x.float() + s * y.float()).to(BF16)
    err, bound = (got.float() - want.float()).abs().max().item(), 2 ** -7 * want.float().abs().max().item()
    print(f"axpby n={n}: max|got - want| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    for a in (2.0, 1 - s):
        assert torch.equal(K.axpby_bf16(a, x.to(DEV)).cpu(), (a * x.float()).to(BF16)), a


@pytest.mark.parametrize("n", SIZES)
def test_sd_select_kept_is_axpby_and_skipped_is_a_select(n):
    _, x, f, dy, _ = _inputs(n)
    x, f, dy = x.to(DEV), f.to(DEV), dy.to(DEV)
    s = 1.0 / KEEP
    kept = torch.tensor([0], dtype=torch.int32, device=DEV)
    skip = torch.tensor([1], dtype=torch.int32, device=DEV)
    assert torch.equal(K.sd_select_fwd(kept, KEEP, x, f), K.axpby_bf16(1.0 - s, x, s, f))
    dx, df = K.sd_select_bwd(kept, KEEP, dy)
    assert torch.equal(dx, K.axpby_bf16(1.0 - s, dy)) and torch.equal(df, K.axpby_bf16(s, dy))
    f_nan = torch.full_like(f, float("nan"))
    out = K.sd_select_fwd(skip, KEEP, x, f_nan)
    assert torch.equal(out.view(torch.int16), x.view(torch.int16))
    dx, df = K.sd_select_bwd(skip, KEEP, dy)
    assert torch.equal(dx.view(torch.int16), dy.view(torch.int16))
    assert torch.equal(df.view(torch.int16), torch.zeros_like(df.view(torch.int16)))


@pytest.mark.parametrize("n", SIZES)
def test_dgelu_mul(n):
    worst = dgelu_worst_ratio(n)
    print(f"dgelu_mul n={n}: worst (|got - ref| - half ulp) / |dy| = {worst:.3e}, C = {DGELU_C:.3e}")
    assert worst <= DGELU_C
