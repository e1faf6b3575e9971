"""The cases of the attention dispatch table (tests/golden/attn_dispatch_256cu.json) and how one case is asked: shared by
tools/dev/record_attn_dispatch.py, which records a library's answers, and tests/test_attn_dispatch_host.py, which compares the
current library with the record.  wft_attn_variant and wft_attn_bwd_colsum_workspace_bytes are pure host functions that read
no pointer, so the answers are the same with and without a GPU."""
import ctypes

from whisper_finetune.engine import lib as L

PTR = 1 << 20  # placeholders with the alignment real operands have: nothing is dereferenced
LENS = (1, 31, 32, 33, 64, 127, 128, 129, 448, 511, 512, 513, 1500)
# (B, H): B * H a multiple of 8 (the XCD-aware placement) and not
GROUPS = ((2, 8), (3, 6))
# shapes on both sides of every threshold (forward pipe: Tk >= 512; dQ 4w: Tq >= 512; dK/dV 4w: Tq >= 128), asked with every
# variant / launch_mode / q_prescaled value
SWITCH_SHAPES = ((127, 1500, 0), (128, 511, 0), (511, 512, 0), (512, 511, 0), (512, 512, 0), (1500, 1500, 0),
                 (127, 127, 1), (512, 512, 1), (1500, 1500, 1))
# leading dimensions around the point where (T + 256) * ld * 2 leaves 31 bits at T = 1500 (attn_offsets_fit32): the last one
# that fits and the first one that does not, for each of the four operands the one-wave-per-SIMD kernels address through buffers
LD_FITS, LD_TOO_LARGE = 611464, 611472
LD_FIELDS = ("ldq", "lddo", "ldk", "ldv")


def cases():
    """(Tq, Tk, causal, B, H, variant, launch_mode, q_prescaled, {leading dimension overrides}) in table order."""
    out = []
    for tq in LENS:
        for tk in LENS:
            for causal in ((0, 1) if tq == tk else (0,)):
                for b, h in GROUPS:
                    out.append((tq, tk, causal, b, h, 0, 0, 0, {}))
    for tq, tk, causal in SWITCH_SHAPES:
        for variant in range(8):
            for launch_mode in (0, 1):
                for qpre in (0, 1):
                    b, h = GROUPS[(variant + launch_mode) % 2]
                    out.append((tq, tk, causal, b, h, variant, launch_mode, qpre, {}))
    for field in LD_FIELDS:
        for ld in (LD_FITS, LD_TOO_LARGE):
            out.append((1500, 1500, 0, 2, 8, 0, 0, 0, {field: ld}))
    return out


def attn_args(tq, tk, causal, b, h, variant=0, launch_mode=0, q_prescaled=0, lds=None):
    """A complete backward call on placeholder pointers: packed [B, T, H * 64] operands."""
    a = L.AttnArgs()
    d = h * 64
    for name in ("q", "k", "v", "o", "lse", "d_o", "delta", "dq", "dk", "dv"):
        setattr(a, name, PTR)
    for ld, bs, t in (("ldq", "q_bs", tq), ("ldk", "k_bs", tk), ("ldv", "v_bs", tk), ("ldo", "o_bs", tq), ("lddo", "do_bs", tq),
                      ("lddq", "dq_bs", tq), ("lddk", "dk_bs", tk), ("lddv", "dv_bs", tk)):
        setattr(a, ld, d)
        setattr(a, bs, t * d)
    a.B, a.H, a.Tq, a.Tk, a.causal, a.scale = b, h, tq, tk, causal, 0.125
    a.launch_mode, a.variant, a.q_prescaled = launch_mode, variant, q_prescaled
    for name, ld in (lds or {}).items():
        setattr(a, name, ld)
    return a


def answers(h, case):
    """[forward kernel, dQ kernel, dK/dV kernel, column-sum workspace bytes]"""
    a = ctypes.byref(attn_args(*case))
    return [int(h.wft_attn_variant(a, 0)), int(h.wft_attn_variant(a, 1)), int(h.wft_attn_variant(a, 2)),
            int(h.wft_attn_bwd_colsum_workspace_bytes(a))]


def all_answers(h):
    return [answers(h, c) for c in cases()]
