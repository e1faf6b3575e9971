"""Every kernel of the attention dispatch plan (csrc/attn.hip: attn_fwd_kernel, attn_fwd_pipe_kernel, the 8-wave attn_bwd_dq_kernel /
attn_bwd_dkdv_kernel, the one-wave-per-SIMD attn_bwd_dq4w_kernel / attn_bwd_dkdv4w_kernel) on probe operands (tests/_attn_probe.py):
every query row puts its softmax mass on two keys at tile edges and is aligned as strongly with a decoy key it must not see, so a
key lost or leaked at a seam moves that row by O(1) of its own size, and o, dq, dk, dv are held to a per-(row, head) bound against
the fp64 oracle, lse per row.  The bound's tolerance is derived on the CPU by tests/test_attn_probe_host.py, which also shows that
every such fault restated as a wrong mask fails it.

Each case asserts through wft_attn_variant which kernels serve it, runs the forward and then the backward on the forward's own
o / lse (as the model does), twice on two seeds into the same output buffers (the K loops are hand-synchronised: a fragment read
that runs ahead of its LDS-DMA piece would see the previous run's different operands), and writes o, lse, dq, dk, dv into views
inside larger buffers pre-filled with a sentinel bit pattern (wider row strides, sentinel rows before and after every batch
entry) of which every element must come back bit-unchanged.  K / V are followed by guard rows that the call's Tk excludes.

The shapes are the smallest on both sides of each kernel's rules (forward pipe: Tk >= 512; dQ 4w: Tq >= 512; dK/dV 4w: Tq >= 128;
non-causal only), with (B, H) = (1, 8) (the XCD-aware item walk) and (3, 2) (the plain walk); three of them run again forced onto
the 8-wave / non-pipelined twins, the one-wave-per-SIMD cases again with one launch per tile, and one causal, one 8-wave
non-causal and every one-wave-per-SIMD case again with q prescaled (both template instances)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _attn_dispatch_cases as dispatch  # noqa: E402
from tests import _attn_probe as P  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = "cuda:0"
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5   # NaN bit patterns: an element the kernel leaves unwritten inside the view fails the comparison
PAD_ROWS, PAD_COLS, PAD_LSE = 3, 32, 64

KERNELS = dict(P.TABLE)
# (shape, B, H, q_prescaled, forced onto the 8-wave twins, launch mode)
RUNS = [(s, B, H, False, False, K.LAUNCH_PERSISTENT) for s, _ in P.TABLE for B, H in P.GROUPS]
RUNS += [(s, *P.GROUPS[n % 2], False, True, K.LAUNCH_PERSISTENT) for n, s in enumerate(P.FORCED)]
RUNS += [(s, *P.GROUPS[n % 2], False, False, K.LAUNCH_PER_TILE) for n, (s, kern) in enumerate(P.TABLE) if 4 in kern]
RUNS += [(tuple(c[2:]), c[0], c[1], True, False, K.LAUNCH_PERSISTENT) for c in P.PRESCALED_CASES]
RUNS += [(tuple(c[2:]), c[0], c[1], True, False, K.LAUNCH_PER_TILE) for c in P.PRESCALED_CASES if KERNELS[tuple(c[2:])][1:] == (4, 4)]
IDS = ["{}x{}-c{}-B{}H{}{}{}{}".format(*s, B, H, "-pre" if pre else "", "-forced8" if forced else "", "-pertile" if launch else "")
       for s, B, H, pre, forced, launch in RUNS]


@pytest.fixture(autouse=True)
def _restore_variants():
    old = dict(K.VARIANT)
    yield
    K.VARIANT.update(old)


@functools.lru_cache(maxsize=None)
def _case(B, H, Tq, Tk, causal, pre, seed):
    """the operands and the forward oracle: computed once, shared by the runs on the same operands, left unchanged"""
    c = P.probe_case(B, H, Tq, Tk, causal, pre, seed=seed)
    return c, P.oracle_fwd(c)


class Guarded:
    """a bf16 [B, T, D] view inside a sentinel-filled [B, T + 2 PAD_ROWS, D + 2 PAD_COLS] buffer"""

    def __init__(self, B, T, D):
        self.buf = torch.full((B, T + 2 * PAD_ROWS, D + 2 * PAD_COLS), SENT16, dtype=torch.int16, device=DEV)
        self.inside = (slice(None), slice(PAD_ROWS, PAD_ROWS + T), slice(PAD_COLS, PAD_COLS + D))
        self.view = self.buf.view(torch.bfloat16)[self.inside]

    def assert_intact(self, what):
        outside = torch.ones_like(self.buf, dtype=torch.bool)
        outside[self.inside] = False
        bad = int((self.buf[outside] != SENT16).sum())
        assert bad == 0, f"{what}: {bad} sentinel elements around the output were overwritten"


class GuardedLse:
    def __init__(self, B, H, Tq):
        self.n = B * H * Tq
        self.buf = torch.full((self.n + 2 * PAD_LSE,), SENT32, dtype=torch.int32, device=DEV)
        self.view = self.buf.view(torch.float32)[PAD_LSE:PAD_LSE + self.n].view(B, H, Tq)

    def assert_intact(self, what):
        bad = int((self.buf[:PAD_LSE] != SENT32).sum() + (self.buf[PAD_LSE + self.n:] != SENT32).sum())
        assert bad == 0, f"{what}: {bad} sentinel elements around lse were overwritten"


def _served_by(Tq, Tk, causal, B, H, pre, launch, out_ld):
    """what wft_attn_variant answers for this call's shapes, strides, variant bits, launch mode and q_prescaled"""
    D = H * 64
    lds = {"ldq": 3 * D, "ldk": 2 * D, "ldv": 2 * D, "ldo": out_ld, "lddq": out_ld, "lddk": out_ld, "lddv": out_ld,
           "q_bs": Tq * 3 * D, "k_bs": (Tk + P.GUARD) * 2 * D, "v_bs": (Tk + P.GUARD) * 2 * D,
           "o_bs": (Tq + 2 * PAD_ROWS) * out_ld, "dq_bs": (Tq + 2 * PAD_ROWS) * out_ld,
           "dk_bs": (Tk + 2 * PAD_ROWS) * out_ld, "dv_bs": (Tk + 2 * PAD_ROWS) * out_ld}
    a = dispatch.attn_args(Tq, Tk, causal, B, H, K._attn_variant_bits(), launch, int(pre), lds)
    return tuple(int(L.load().wft_attn_variant(ctypes.byref(a), which)) for which in (0, 1, 2))


@pytest.mark.parametrize("shape,B,H,pre,forced,launch", RUNS, ids=IDS)
def test_probe_operands_through_every_kernel_of_the_plan(shape, B, H, pre, forced, launch):
    Tq, Tk, causal = shape
    D = H * 64
    out_ld = D + 2 * PAD_COLS
    assert _served_by(Tq, Tk, causal, B, H, pre, launch, out_ld) == KERNELS[shape]
    if forced:
        for which in ("fwd", "dq", "dkdv"):
            K.set_variant(which, 1)
        assert KERNELS[shape] != (1, 8, 8) and _served_by(Tq, Tk, causal, B, H, pre, launch, out_ld) == (1, 8, 8)
    o, dq, dk, dv, lse = Guarded(B, Tq, D), Guarded(B, Tq, D), Guarded(B, Tk, D), Guarded(B, Tk, D), GuardedLse(B, H, Tq)
    atol = 1e-6 if Tk == 1 else 0.0   # one key: dq = dk = 0 exactly, fp32 summation order leaves ~1e-8 (P.close_rows)
    for seed in (0, 1):
        c, (o64, lse64) = _case(B, H, Tq, Tk, causal, pre, seed)
        q, k, v, do = c.to(DEV)
        assert k.stride(0) == (Tk + P.GUARD) * 2 * D and q.stride(1) == 3 * D
        K.attn_fwd(q, k, v, H, bool(causal), P.SCALE, q_prescaled=pre, o=o.view, lse=lse.view)
        K.attn_bwd(q, k, v, o.view, lse.view, do, H, bool(causal), P.SCALE, dq=dq.view, dk=dk.view, dv=dv.view,
                   q_prescaled=pre, launch=launch)
        torch.cuda.synchronize()
        got_o, got_lse = o.view.cpu(), lse.view.cpu()
        failures = []
        for what, check in (("lse", lambda: P.close_lse(got_lse, lse64, f"seed {seed} lse")),
                            ("o", lambda: P.close_rows(got_o, o64, P.TOL, P.FLOOR, f"seed {seed} o"))):
            try:
                check()
            except AssertionError as e:   # go on to the backward: it is judged on the o / lse it was given
                failures.append(str(e))
        rdq, rdk, rdv = P.oracle_bwd(c, got_o, got_lse)
        for name, got, ref, at in (("dq", dq, rdq, atol), ("dk", dk, rdk, atol), ("dv", dv, rdv, 0.0)):
            try:
                P.close_rows(got.view.cpu(), ref, P.TOL, P.FLOOR, f"seed {seed} {name}", atol=at)
            except AssertionError as e:
                failures.append(str(e))
        assert not failures, "\n".join(failures)
        for name, g in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv), ("lse", lse)):
            g.assert_intact(f"seed {seed} {name}")
