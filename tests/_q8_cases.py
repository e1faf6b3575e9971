"""Test helper of the weight-only int8 decoding path: cases, restated definitions and the per-element error bound shared by
tests/test_q8_host.py (CPU) and tests/test_q8_kernels_gpu.py / tests/test_q8_decode_gpu.py.

  quantize_rows     include/wft.h's definition of wft_quantize_rows_i8 in numpy float32, operation by operation (numpy's f32 divide,
                    multiply and rint are correctly rounded / half-even, as the kernel's __fdiv_rn / __fmul_rn / rintf): bit for bit.
  gemm_ref64        C = epi(scale[n] * sum_k A[m][k] Q[n][k] + bias[n]) + residual[m][n] in float64, from the operands as given.
  gemm_bound        what a bf16 C from the kernel of csrc/gemm_stream.hip may differ from gemm_ref64 by, per element (derived below).
  emulate           the kernel restated on the CPU: bf16 inputs, f32 sums in plan order — with the mutants the bound has to reject.

The bound.  u = 2^-24 (f32 round to nearest), ub = 2^-8 (bf16 round to nearest: 8 significant bits, half an ulp
of 2^-7 relative).  For one element, with
S = sum_k |A[m][k]| |Q[n][k]|, dot = sum_k A[m][k] Q[n][k], s = scale[n]:
  * every product of a bf16 (8 significant bits) and an integer of magnitude <= 128 (8 bits) has at most 16 significant bits: exact
    in f32.  What is left is summation error.
  * the K products of the element are summed in f32 inside `split` slices (MFMA accumulation, k ascending) and the slice sums are
    added in slice order: every product passes through at most K + split - 1 additions, whatever their order.  The MFMA's
    internal adder is not documented as round-to-nearest, so each addition is granted a full ulp, 2u, not half of one (the standard
    running-error bound with a truncating adder):                      |sum_hat - dot| <= (K + split) * 2u * S
  * one multiply by the scale:          t = fl(sum_hat * s),           |t - s dot|     <= s * (K + split) * 2u * S + u |s dot|  (+ second order)
  * the bias add:                       pre = fl(t + b),               e_pre = above + u |pre|
  * GELU where it applies: |gelu'| <= 1.13 everywhere (its maximum, 1.1289 at x = sqrt 2 ... rounded up), so the input error grows by
    at most 1.13; the kernel's own gelu (erf to 1.5e-7 absolute, A&S 7.1.26, inside 0.5 x (1 + erf)) adds 0.5 |x| 1.5e-7 and a handful
    of f32 roundings, granted 8u |x|:                                   e_act = 1.13 e_pre + |pre| (0.75e-7 + 8u)
  * the residual add (a bf16 value, exact in f32):                      e_out = e_act + u |out|
  * one bf16 rounding of a value within e_out of out:                   e = e_out + ub (|out| + e_out)
plus 1e-30 for results that underflow.  Second-order terms are covered by the factor 2 on the dominant first line.  Nothing here is
taken from what the kernel returns."""
import numpy as np
import torch

U32 = 2.0 ** -24
UBF = 2.0 ** -8
GELU_LIP = 1.13
CUS = 256  # the plan of the host tests: an MI355X

# (M, N, K) against stream_plan on 256 CUs
SHAPES = [
    (1, 128, 64),        # one k-step, one slice
    (16, 256, 384),      # six slices of one step each
    (17, 384, 1536),     # the second M tile with 15 dead rows
    (5, 32768, 320),     # slices of 2, 2 and 1 steps
    (32, 51968, 384),    # the tied-logits grid: two slices of three steps, pair loop plus tail
]
FORMS = {
    "none": dict(bias=False, gelu=False, res=False),
    "bias": dict(bias=True, gelu=False, res=False),
    "gelu": dict(bias=True, gelu=True, res=False),
    "residual": dict(bias=True, gelu=False, res=True),
}


def bf16_round(x: np.ndarray) -> np.ndarray:
    """f32 -> nearest bf16 (ties to even), returned as f32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def stream_plan(N: int, K: int, cus: int = CUS):
    """csrc/gemm_stream.hip stream_plan -> (split, per)."""
    nblk, nk = N // 128, K // 64
    split = max(1, min((4 * cus) // nblk, nk))
    per = (nk + split - 1) // split
    return (nk + per - 1) // per, per


# ----------------------------------------------------------------------------- the quantiser
def quantize_rows(w: np.ndarray, mutant: str = None):
    """w f32 [rows, cols] holding bf16 values -> (q int8 [rows, cols], scale f32 [rows]).  mutant: one wrong quantiser
    ("half_away", "amax_short", "clamp128")."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    src = w[:, :-1] if mutant == "amax_short" else w
    amax = np.abs(src).max(axis=1).astype(np.float32)
    top = np.float32(128.0 if mutant == "clamp128" else 127.0)
    scale = (amax / top).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(amax > 0, top / amax, np.float32(0.0)).astype(np.float32)
    t = (w * inv[:, None]).astype(np.float32)
    if mutant == "half_away":
        r = np.sign(t) * np.floor(np.abs(t) + np.float32(0.5))
    else:
        r = np.rint(t)
    if mutant == "clamp128":
        q = np.clip(r, -128, 128).astype(np.int32).astype(np.uint8).astype(np.int8)  # 128 wraps to -128
    else:
        q = np.clip(r, -127, 127).astype(np.int8)
    return q, scale


def fake_quantize(w: np.ndarray) -> np.ndarray:
    """f32 weights -> what the int8 path reads of them: bf16-rounded, quantised per row, q * scale (f32)."""
    q, s = quantize_rows(bf16_round(w))
    return (q.astype(np.float32) * s[:, None]).astype(np.float32)


def quantizer_rows(cols: int = 128) -> np.ndarray:
    """Structured bf16 rows [9, cols] (cols % 64 == 0) for the bit-equality test of the quantiser:
      0 all zero (a padding row)           1 lossless: w = q 2^-6, q cycling over -127..127, max |q| = 127
      2 the maximum alone in the LAST column, everything else far smaller
      3 ties: amax = 127 * 2^-3 so inv = 8 exactly, the rest (m + 0.5) / 8 with even and odd m, both signs
      4 the maximum negative               5 one nonzero element        6 tiny values, amax = 2^-100
      7, 8 random."""
    rng = np.random.default_rng(7)
    r = np.zeros((9, cols), dtype=np.float32)
    q = (np.arange(cols) * 37) % 255 - 127
    q[5] = 127
    r[1] = q * 2.0 ** -6
    r[2] = bf16_round(rng.standard_normal(cols) * 0.01)
    r[2, -1] = 1.5
    m = np.arange(cols) % 100
    r[3] = (m + 0.5) / 8.0 * np.where(np.arange(cols) % 3 == 0, -1.0, 1.0)
    r[3, 7] = 127.0 / 8.0
    r[4] = bf16_round(rng.standard_normal(cols) * 0.05)
    r[4, 11] = -0.75
    r[5, 64 % cols] = -3.0
    r[6] = bf16_round(rng.standard_normal(cols)) * np.float32(2.0 ** -103)
    r[6, 3] = 2.0 ** -100
    r[7] = bf16_round(rng.standard_normal(cols) * 0.05)
    r[8] = bf16_round(rng.standard_normal(cols) * 3.0)
    assert np.array_equal(r, bf16_round(r))
    return r


# ----------------------------------------------------------------------------- the GEMM
def make_case(M: int, N: int, K: int, seed: int = 0, scales: str = "general"):
    """Operands of one product: A bf16 values [M, K] (as f32), Q int8 [N, K], scale f32 [N], bias f32 [N], res bf16 values [M, N].
    scales: "general" — Q and scale are the quantiser's image of random bf16 weights with a per-row spread of magnitudes;
    "unit" — ones; "pow2" — 2^e(n), e in -9..2."""
    rng = np.random.default_rng(1000003 * seed + 7919 * M + 31 * N + K)
    A = bf16_round(rng.standard_normal((M, K), dtype=np.float32))
    row_mag = (0.02 * np.exp2(rng.integers(-2, 3, size=N))).astype(np.float32)
    W = bf16_round(rng.standard_normal((N, K), dtype=np.float32) * row_mag[:, None])
    Q, scale = quantize_rows(W)
    if scales == "unit":
        scale = np.ones(N, dtype=np.float32)
    elif scales == "pow2":
        scale = np.exp2(rng.integers(-9, 3, size=N)).astype(np.float32)
    bias = (rng.standard_normal(N, dtype=np.float32) * 0.5).astype(np.float32)
    res = bf16_round(rng.standard_normal((M, N), dtype=np.float32))
    return dict(A=A, Q=Q, scale=scale, bias=bias, res=res, M=M, N=N, K=K)


def _gelu64(x):
    from math import sqrt

    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(x) / sqrt(2.0)).numpy())


def _dots(case):
    """(sum_k A Q, sum_k |A| |Q|) in float64, computed once per case (the vocabulary-sized one takes a second)."""
    if "_dot" not in case:
        A, Q = case["A"].astype(np.float64), case["Q"].astype(np.float64)
        case["_dot"], case["_S"] = A @ Q.T, np.abs(A) @ np.abs(Q).T
    return case["_dot"], case["_S"]


def gemm_ref64(case, bias=False, gelu=False, res=False):
    """-> (out f64 [M, N], pre f64 [M, N]: the value the GELU epilogue stores as aux)."""
    dot = _dots(case)[0]
    pre = dot * case["scale"].astype(np.float64)[None, :]
    if bias:
        pre = pre + case["bias"].astype(np.float64)[None, :]
    out = _gelu64(pre) if gelu else pre
    if res:
        out = out + case["res"].astype(np.float64)
    return out, pre


def gemm_bound(case, split: int, bias=False, gelu=False, res=False):
    """Per-element bound [M, N] on |kernel - gemm_ref64| (the derivation is the head of this file) -> (for out, for the stored
    pre-activation)."""
    K = case["K"]
    s = np.abs(case["scale"].astype(np.float64))[None, :]
    S = _dots(case)[1]
    out, pre = gemm_ref64(case, bias, gelu, res)
    sdot = np.abs(pre - (case["bias"].astype(np.float64)[None, :] if bias else 0.0))
    e_pre = s * (K + split) * 2 * U32 * S + U32 * sdot + U32 * np.abs(pre)
    e_act = GELU_LIP * e_pre + np.abs(pre) * (0.75e-7 + 8 * U32) if gelu else e_pre
    e_out = e_act + U32 * np.abs(out)
    return e_out + UBF * (np.abs(out) + e_out) + 1e-30, e_pre + UBF * (np.abs(pre) + e_pre) + 1e-30


def emulate(case, split: int, per: int, bias=False, gelu=False, res=False, mutant: str = None):
    """The kernel pair on the CPU -> bf16 values [M, N] as f32: per slice (k-steps ascending, the two 32-wide MFMAs of a step
    ascending) f32 partial sums, slices added in order, one f32 multiply by the scale, bias, GELU, residual, one bf16 rounding.
    mutant: "no_scale", "scale_next_row", "scale_after_bias", "unsigned", "drop_last_slice", "drop_odd_step"."""
    A, Q = case["A"], case["Q"]
    M, N, K = case["M"], case["N"], case["K"]
    nk = K // 64
    Qf = (Q.astype(np.uint8) if mutant == "unsigned" else Q).astype(np.float32)
    total = None
    for sl in range(split):
        if mutant == "drop_last_slice" and sl == split - 1 and split > 1:
            continue
        acc = np.zeros((M, N), dtype=np.float32)
        for ks in range(sl * per, min(sl * per + per, nk)):
            if mutant == "drop_odd_step" and (ks - sl * per) % 2 == 1:
                continue
            for h in range(2):
                # MFMA h of the step reads k = 64 ks + 16 g + 8 h + e (g < 4, e < 8)
                cols = (64 * ks + 16 * np.arange(4)[:, None] + 8 * h + np.arange(8)[None, :]).reshape(-1)
                acc = (acc + A[:, cols] @ Qf[:, cols].T).astype(np.float32)
        total = acc if total is None else (total + acc).astype(np.float32)
    scale = case["scale"].astype(np.float32)
    if mutant == "scale_next_row":
        scale = np.roll(scale, -1)
    b = case["bias"].astype(np.float32)[None, :] if bias else None
    if mutant == "no_scale":
        t = total if b is None else (total + b).astype(np.float32)
    elif mutant == "scale_after_bias":
        t = ((total if b is None else (total + b).astype(np.float32)) * scale[None, :]).astype(np.float32)
    else:
        t = (total * scale[None, :]).astype(np.float32)
        if b is not None:
            t = (t + b).astype(np.float32)
    if gelu:
        t = _gelu64(t.astype(np.float64)).astype(np.float32)
    if res:
        t = (t + case["res"]).astype(np.float32)
    return bf16_round(t)


# ----------------------------------------------------------------------------- the decoder under fake-quantised weights
DECODE_DIMS = (80, 1500, 384, 6, 2, 51865, 448, 384, 6, 2)  # whisper-tiny's widths, 2 + 2 layers
DECODE_SEED = 0
DECODE_B, DECODE_STEPS = 3, 12
DECODE_PROMPT_LEN = (4, 6, 9)  # ragged; B * widest = 27 <= 32: every projection of the prefill is a streaming call too


def int8_read(name: str, t) -> bool:
    """True for the decoder weights a cached step reads as int8: every Linear weight but the cross-attention key / value
    projections (computed once per audio by the prefill's bf16 kernels).  The token embedding is handled apart: the tied logits
    product reads its int8 image, the embedding lookup its fp32 rows."""
    return (name.startswith("decoder.blocks.") and name.endswith(".weight") and t.dim() == 2
            and ".cross_attn.key." not in name and ".cross_attn.value." not in name)


def fake_quantized_params(params: dict):
    """-> (params with every int8-read decoder weight replaced by q * scale of its bf16 rounding, the fake-quantised embedding)."""
    out = dict(params)
    for name, t in params.items():
        if int8_read(name, t):
            out[name] = torch.from_numpy(fake_quantize(t.detach().float().numpy()))
    return out, torch.from_numpy(fake_quantize(params["decoder.token_embedding.weight"].detach().float().numpy()))


def oracle_last_logits(oracle, xa_ref, tokens, lens, emb_out=None):
    """tests/_decode_oracle.oracle_last_logits with the output side of the tied embedding given apart (emb_out; None: the
    parameter itself): logits [B, V] of every row's position lens[b] - 1 from one re-forward over the right-padded prefixes."""
    import torch.nn.functional as F

    from oracle import whisper_oracle as O

    L = int(lens.max())
    p, dims = oracle.p, oracle.dims
    emb_out = p["decoder.token_embedding.weight"] if emb_out is None else emb_out
    with torch.no_grad():
        x = F.embedding(tokens[:, :L], p["decoder.token_embedding.weight"]) + p["decoder.positional_embedding"][:L]
        x = oracle.ra(x.to(xa_ref.dtype))
        for i in range(dims.n_text_layer):
            x = oracle.block(x, f"decoder.blocks.{i}", dims.n_text_head, xa=xa_ref, causal=True)
        x = x[torch.arange(tokens.shape[0]), lens.long() - 1]
        x = oracle.ra(O.layer_norm(x, p["decoder.ln.weight"], p["decoder.ln.bias"]))
        return oracle.ra(x @ oracle.rw(emb_out).to(x.dtype).T).float()


def decode_case(seed: int = DECODE_SEED):
    """(dims, params, audio, prompt i64 [B, T] right-padded with eot, prompt_len) of the small decoding model."""
    from oracle import whisper_oracle as O

    dims = O.ModelDimensions(*DECODE_DIMS)
    params = O.init_params(dims, seed=seed)
    g = torch.Generator().manual_seed(seed + 5)
    for k, v in params.items():
        if k.endswith("bias"):
            params[k] = torch.randn(v.shape, generator=g) * 0.02
        elif "ln" in k and k.endswith("weight"):
            params[k] = 1 + torch.randn(v.shape, generator=g) * 0.05
    audio, y_in, y_out = O.synthetic_batch(dims, DECODE_B, 16)
    plen = torch.tensor(DECODE_PROMPT_LEN)
    prompt = torch.full((DECODE_B, int(plen.max())), 50257, dtype=torch.int64)
    for b in range(DECODE_B):
        prompt[b, :plen[b]] = y_in[b, :plen[b]]
    return dims, params, audio, prompt, plen, y_in, y_out
