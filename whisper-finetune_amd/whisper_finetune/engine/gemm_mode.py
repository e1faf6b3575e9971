"""The thread-local GEMM modes of decoding: `stream_gemm` (the weight-streaming kernels of a cached step, bf16 or int8 weights) and
`int8_gemm` (the W8A8 kernel of the encoder and the prefill under weights="w8a8").  `ops.linear` and the tied logits product read the
three predicates; engine/decode enters the contexts.  Standard library only: nothing of the engine is imported here."""
from __future__ import annotations

import contextlib
import threading

# ----------------------------------------------------------------------------- the streaming-GEMM context
_TLS = threading.local()


WEIGHT_MODES = ("bf16", "int8")  # what the streaming GEMMs of a cached step read (stream_gemm(weights=...))
# the `weights=` keyword of every decode call: "w8a8" = the "int8" steps behind an encoder and a prefill on the W8A8 kernel (int8_gemm)
DECODE_WEIGHTS = ("bf16", "int8", "w8a8")


def step_weights(weights: str) -> str:
    """The weights mode of the CACHED steps: those of "w8a8" are the weight-only "int8" steps (wft_gemm_nt_stream_q8)."""
    return "int8" if weights == "w8a8" else weights


def stream_gemm_active() -> bool:
    return getattr(_TLS, "stream_gemm", False)


def stream_gemm_weights() -> str:
    """"int8" inside an active stream_gemm(weights="int8") context, else "bf16"."""
    return getattr(_TLS, "stream_weights", "bf16") if stream_gemm_active() else "bf16"


@contextlib.contextmanager
def stream_gemm(enabled: bool = True, weights: str = "bf16"):
    """Inside this context, under torch.no_grad(), `ops.linear` and the tied logits product send a GEMM to the weight-streaming
    kernel for M <= 32 (csrc/gemm_stream.hip, wft_gemm_nt_stream_bf16) when wft_gemm_nt_stream_ok serves it, and to
    wft_gemm_nt_bf16 otherwise.  Thread-local, in the style of runtime.exchange_launch_mode; outside it nothing changes.  A context
    and not a model attribute: whoever drives prefill / step / pick itself runs under it unchanged.
    weights="int8" (thread-local with the switch): the products that wft_gemm_nt_stream_q8_ok serves read the int8 image of the group's
    shadow (LinearGroup.shadows_q8, wft_gemm_nt_stream_q8) — weight-only: activations stay bf16; a call it does not serve goes on as
    under "bf16".  Everything that is not such a step (the prefill at M > 32, the encoder, training) never looks at the mode."""
    if weights not in WEIGHT_MODES:
        raise ValueError(f"weights must be one of {WEIGHT_MODES}, got {weights!r}")
    old = stream_gemm_active(), getattr(_TLS, "stream_weights", "bf16")
    _TLS.stream_gemm, _TLS.stream_weights = bool(enabled), weights
    try:
        yield
    finally:
        _TLS.stream_gemm, _TLS.stream_weights = old


def int8_gemm_active() -> bool:
    return getattr(_TLS, "int8_gemm", False)


@contextlib.contextmanager
def int8_gemm(enabled: bool = True):
    """Inside this context, under torch.no_grad(), `ops.linear` sends a product with M > 32 that wft_gemm_nt_i8_ok serves to the W8A8
    kernel (csrc/gemm_i8.hip): the input is quantised per row once per call (wft_quantize_rows_i8, the kernel that quantises the weight
    shadows), the weight operand is the int8 image of the group's shadow (LinearGroup.shadows_q8: merged LoRA delta and folded query
    scale included) and wft_gemm_nt_i8 multiplies them on the int8 matrix cores.  A fused q/k/v group is one call, so one quantiser
    pass.  Every other call — M <= 32, grad mode, the tied logits product, the fp32 compute mode — goes on exactly as outside.
    Thread-local beside `stream_gemm` and independent of it; decoding's weights="w8a8" runs the encoder and the prefill under it."""
    old = int8_gemm_active()
    _TLS.int8_gemm = bool(enabled)
    try:
        yield
    finally:
        _TLS.int8_gemm = old
