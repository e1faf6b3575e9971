"""Correctness at the sizes bench.py TIMES (VERDICT r5 "weak" 1a): the headline is 96 clips of whisper-large-v3 — 144 000 activation rows,
1.47 GB GEMM operands, byte offsets close to the 32-bit eligibility limits of the one-wave-per-SIMD kernels (gemm_nt4w.hip, gemm_tn4w.hip,
attn_dq4w.hip, attn_dkdv4w.hip: the dispatch predicates) — and the turbo YAML's B = 64, S = 448 logits (28 672 x 51 866).  The row-count tests run at 96 clips
(bench.py's --batch default, read from its source: test_headline_sizes_cover_the_benchmark_default_batch) AND at the 87 clips = 130 500
rows of the earlier headline; each has edges the other lacks: 130 500 = 509 x 256 + 196 (ragged last row tile) = 2039 x 64 + 4 (ragged
reduction tail), 144 000 = 562 x 256 + 128 (half a last row tile) = 2250 x 64 (no tail).  The CPU oracle cannot run these sizes:
the checks are size-independent properties (identity, linearity, rows of a softmax sum to one, rows of a CE gradient sum to zero),
chunked fp32 / fp64 math on the GPU on sampled row blocks and chunked fp64 reductions over all rows, each also asserting WHICH kernel
the dispatcher chose.
Reference call sites: whisper.model.Linear / LayerNorm / MultiHeadAttention.qkv_attention reached from model/model_utils.py:283-285,320-325;
F.gelu between mlp.0 and mlp.2 of whisper.model.ResidualAttentionBlock; F.cross_entropy at model/model_utils.py:66-68."""
import ctypes as C
import re
import time
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

from tests._gelu_codes import _code_index, _decode, _dgelu  # noqa: E402

DEV = "cuda:0"
T_ENC = 1500       # encoder rows per clip
CLIPS = (87, 96)   # 96: bench.py's headline batch; 87: the earlier one (module docstring)
WIN = 200          # rows of a probed window


def _with_clips(names, cases):
    """clips x cases; the 87-clip cases keep the ids they had before the row count became a parameter"""
    return pytest.mark.parametrize("clips," + names, [pytest.param(c, *case, id=("" if c == 87 else f"{c}clips-") + "-".join(map(str, case)))
                                                      for c in CLIPS for case in cases])


def bf(x):
    return x.to(torch.bfloat16)


def _randn_bf16(rows, cols, gen, scale=1.0, shift=0.0):
    """bf16 N(shift, scale^2) [rows, cols] without an fp32 copy of the whole tensor alive."""
    out = torch.empty(rows, cols, dtype=torch.bfloat16, device=DEV)
    step = 16384
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        out[r0:r0 + n] = bf(torch.randn(n, cols, device=DEV, generator=gen) * scale + shift)
    return out


def _last_tile_start(rows):
    """first row of the last (possibly ragged) 256-row tile"""
    return (rows - 1) // 256 * 256


def test_headline_sizes_cover_the_benchmark_default_batch():
    """bench.py's --batch default is one of the clip counts of this file (the file went stale for a round when the default moved from
    87 to 96): read from the benchmark's source, which this test does not import or change."""
    src = (Path(__file__).resolve().parents[1] / "bench.py").read_text()
    m = re.search(r'add_argument\(\s*"--batch"[^\n]*?default=(\d+)', src)
    assert m, "bench.py no longer declares --batch with an integer default"
    assert int(m.group(1)) in CLIPS, (int(m.group(1)), CLIPS)


@_with_clips("N,Kd", [(1280, 1280), (3840, 1280), (5120, 1280), (1280, 5120)])
def test_headline_nt_gemm_identity_and_linearity(clips, N, Kd):
    """The four encoder GEMM shapes of the headline step (out-proj, fused QKV, fc1, fc2) at M = 130 500 / 144 000."""
    rows = clips * T_ENC
    g = torch.Generator(device=DEV).manual_seed(N + Kd)
    a1 = _randn_bf16(rows, Kd, g)
    args, _ = K.gemm_nt(a1, bf(torch.zeros(N, Kd, device=DEV)), _args_only=True)
    assert L.load().wft_gemm_nt_variant(C.byref(args)) == 4, "the headline shapes run on gemm_nt4w_kernel"
    eye = bf(torch.eye(N, Kd, device=DEV))
    y = K.gemm_nt(a1, eye)
    n0 = min(N, Kd)
    assert torch.equal(y[:, :n0], a1[:, :n0])  # A @ I^T == A exactly, every row of every tile
    if N > Kd:
        assert not y[:, Kd:].any()
    del y
    # rows in the LAST row tile (130 500 = 509 * 256 + 196, 144 000 = 562 * 256 + 128) and bias: C = A W^T + b against an fp32 product
    # of those rows — windows at the start, across row 65 536, across the last tile's first row, and the last rows
    w = bf(torch.randn(N, Kd, device=DEV, generator=g) * 0.05)
    bias = torch.randn(N, device=DEV, generator=g)
    y = K.gemm_nt(a1, w, bias=bias)
    last0 = _last_tile_start(rows)
    assert rows - last0 == {87: 196, 96: 128}[clips]
    for r0 in (0, 65536 - 128, last0 - 64, rows - WIN):
        ref = a1[r0:r0 + WIN].float() @ w.float().t() + bias
        err = (y[r0:r0 + WIN].float() - ref).abs().max().item()
        assert err <= 1e-2 * ref.abs().max().item(), (r0, err)
    # linearity in A (fp32 outputs): (a1 + a2) W^T == a1 W^T + a2 W^T up to the rounding of the summed operand, which is corrected
    # to first order by the GEMM of the rounding residual
    a2 = _randn_bf16(rows, Kd, g)
    s = torch.empty_like(a1)
    resid = torch.empty_like(a1)
    for r0 in range(0, rows, 16384):
        sl = slice(r0, min(r0 + 16384, rows))
        exact = a1[sl].float() + a2[sl].float()
        s[sl] = bf(exact)
        resid[sl] = bf(s[sl].float() - exact)
    y1 = K.gemm_nt(a1, w, out_f32=True)
    y1 += K.gemm_nt(a2, w, out_f32=True)
    y1 += K.gemm_nt(resid, w, out_f32=True)
    r = K.gemm_nt(s, w, out_f32=True)
    assert ((r - y1).abs().max() / y1.abs().max()).item() < 2e-3


@_with_clips("P", [(1280,), (3840,), (5120,)])
def test_headline_weight_gradient_matches_chunked_fp32(clips, P):
    """dW = dy^T x with 130 500 / 144 000 reduction rows (out-proj / QKV / fc1 weight gradients of the headline step) against an fp32
    product accumulated in 15 chunks on the GPU; bitwise reproducible across two launches."""
    rows = clips * T_ENC
    g = torch.Generator(device=DEV).manual_seed(P)
    dy = _randn_bf16(rows, P, g)
    x = _randn_bf16(rows, 1280, g)
    args, _ = K.gemm_tn(dy, x, _args_only=True)
    assert L.load().wft_gemm_tn_variant(C.byref(args)) == 4, "the headline weight gradients run on gemm_tn4w_kernel"
    got = K.gemm_tn(dy, x)
    assert torch.equal(got, K.gemm_tn(dy, x))
    chunk = rows // 15
    assert chunk * 15 == rows
    ref = torch.zeros(P, 1280, device=DEV, dtype=torch.float64)
    for r0 in range(0, rows, chunk):
        ref += (dy[r0:r0 + chunk].float().t() @ x[r0:r0 + chunk].float()).double()
    err = (got.double() - ref).abs().max().item()
    assert err <= 3e-5 * ref.abs().max().item() + 1e-3, err  # fp32 accumulation over 130 500+ terms of size ~1, two different orders
    # the last 64-row reduction step: ragged at 130 500 = 2039 * 64 + 4 rows (the last 4 rows count), full at 144 000 = 2250 * 64
    tail = rows % 64 or 64
    assert tail == {87: 4, 96: 64}[clips]
    x2 = x.clone()
    x2[-tail:] = 0
    d = (got - K.gemm_tn(dy, x2)).double()
    ref_tail = (dy[-tail:].float().t() @ x[-tail:].float()).double()
    assert (d - ref_tail).abs().max().item() <= 1e-3 + 1e-4 * ref_tail.abs().max().item()


def _encoder_attention_properties(B):
    H, T = 20, T_ENC
    d = H * 64
    g = torch.Generator(device=DEV).manual_seed(7)
    qkv = _randn_bf16(B * T, 3 * d, g).view(B, T, 3 * d)
    qkv[..., 2 * d:] = 1.0
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    a = L.AttnArgs()
    a.q, a.ldq, a.q_bs = K._attn_view(q)
    a.k, a.ldk, a.k_bs = K._attn_view(k)
    a.v, a.ldv, a.v_bs = K._attn_view(v)
    a.B, a.H, a.Tq, a.Tk, a.causal, a.scale = B, H, T, T, 0, 0.125
    a.lddo, a.do_bs = d, T * d
    lib = L.load()
    assert lib.wft_attn_variant(C.byref(a), 0) == 2 and lib.wft_attn_variant(C.byref(a), 1) == 4 and lib.wft_attn_variant(C.byref(a), 2) == 4, \
        "the encoder call runs on attn_fwd_pipe_kernel / attn_bwd_dq4w_kernel / attn_bwd_dkdv4w_kernel"
    o, lse = K.attn_fwd(q, k, v, H, False, 0.125)
    assert (o.float() - 1).abs().max().item() < 1e-2
    # lse of the first and the last (batch, head) against fp32 math
    for b, h in ((0, 0), (B - 1, H - 1), (43, 7)):
        s = (q[b, :, 64 * h:64 * h + 64].float() @ k[b, :, 64 * h:64 * h + 64].float().t()) * 0.125
        assert (lse[b, h] - torch.logsumexp(s, -1)).abs().max().item() < 2e-3
    do = torch.ones_like(o)
    dq, dk, dv = K.attn_bwd(q, k, v, o, lse, do, H, False, 0.125)
    assert dq.float().abs().max().item() < 2e-2 and dk.float().abs().max().item() < 2e-2
    assert (dv.float().view(B, T, H, 64).sum(1) - T).abs().max().item() < 0.02 * T
    del do, dq, dk, dv, o
    # a real backward on one slice of the batch, last batch element included: the B-clip launch against the same kernels run on
    # that element alone (same arithmetic per (batch, head): bit-identical) and against fp32 math
    qkv[..., 2 * d:] = _randn_bf16(B * T, d, g).view(B, T, d)
    do = _randn_bf16(B * T, d, g).view(B, T, d)
    o, lse = K.attn_fwd(q, k, v, H, False, 0.125)
    dq, dk, dv = K.attn_bwd(q, k, v, o, lse, do, H, False, 0.125)
    b = B - 1
    o1, lse1 = K.attn_fwd(q[b:], k[b:], v[b:], H, False, 0.125)
    dq1, dk1, dv1 = K.attn_bwd(q[b:], k[b:], v[b:], o1, lse1, do[b:], H, False, 0.125)
    assert torch.equal(o[b:], o1) and torch.equal(dq[b:], dq1) and torch.equal(dk[b:], dk1) and torch.equal(dv[b:], dv1)
    h = H - 1
    qf, kf, vf = (t[b, :, 64 * h:64 * h + 64].float().requires_grad_(True) for t in (q, k, v))
    ref = torch.softmax((qf @ kf.t()) * 0.125, -1) @ vf
    ref.backward(do[b, :, 64 * h:64 * h + 64].float())
    for got, want, nm in ((o, ref, "o"), (dq, qf.grad, "dq"), (dk, kf.grad, "dk"), (dv, vf.grad, "dv")):
        e = (got[b, :, 64 * h:64 * h + 64].float() - want).norm() / want.norm()
        assert e.item() < 2e-2, (nm, e.item())


def test_headline_encoder_attention_properties():
    """B = 87, 20 heads, 1500 x 1500 on the fused [B*T, 3d] QKV buffer layout the model uses (row stride 3840).  v = 1 makes every
    output row the sum of its softmax weights (= 1); dO = 1 then gives dS = P (dP - delta) = 0, so dq = dk = 0, and dv's column sums over
    keys are the number of queries."""
    _encoder_attention_properties(87)


def test_headline_encoder_attention_properties_at_the_benchmark_batch():
    """The same at B = 96, bench.py's batch: a 1.1 GB fused QKV buffer."""
    _encoder_attention_properties(96)


@pytest.mark.parametrize("clips", CLIPS)
def test_headline_one_byte_gelu_pair_aux8(clips):
    """The large-v3 MLP's two fused products at the timed row counts, 5 120 x 1 280: fc1 forward with WFT_EPI_GELU_GRAD8 (gelu' as one
    byte per element in gemm_nt4w_kernel's fragment order), then fc2's backward-data product with WFT_EPI_MUL_AUX8 and the fused column
    sums (fc1's bias gradient) — the pair had not been run above 33 000 rows (tests/test_gelu_aux8_gpu.py, whose bounds these are).
    The activation (all rows) is bit-equal to the WFT_EPI_GELU_GRAD form's; on sampled 256-row blocks (the first, one straddling row
    65 536, the last full tile, the ragged last tile) the decoded codes are within half a grid step + 2e-3 of the fp64 derivative of
    the fp32 pre-activation; the backward output (all rows) is bit-equal to bf16(acc * decode(code)); the column sums against a
    chunked fp64 sum over all rows; the bytes of the code buffer that belong to rows past the end of the ragged last tile have no
    influence on either."""
    t_start = time.time()
    M, N, Kd = clips * T_ENC, 5120, 1280
    g = torch.Generator(device=DEV).manual_seed(clips)
    x = _randn_bf16(M, Kd, g)
    w = bf(torch.randn(N, Kd, device=DEV, generator=g) * (2.0 / Kd ** 0.5))
    bias = torch.randn(N, device=DEV, generator=g) * 0.5
    nb = K.gemm_nt_aux8_bytes(M, N, Kd, DEV)
    assert nb == -(-M // 256) * 20 * 65536, "the shape runs on gemm_nt4w_kernel"
    codes = torch.full((nb,), 255, dtype=torch.uint8, device=DEV)
    act8 = K.gemm_nt(x, w, bias=bias, epilogue=L.EPI_GELU_GRAD8, aux=codes)
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    act = K.gemm_nt(x, w, bias=bias, epilogue=L.EPI_GELU_GRAD, aux=aux)
    assert torch.equal(act8, act)
    del act8, act
    pre = K.gemm_nt(x, w, bias=bias, out_f32=True)  # (same k order as the bf16-output call: bit-identical accumulators)
    last0 = _last_tile_start(M)
    blocks = ((0, 256), (65536 - 128, 65536 + 128), (last0 - 256, last0), (last0, M))
    for r0, r1 in blocks:
        dec = _decode(codes, M, N, rows=(r0, r1))
        true = _dgelu(pre[r0:r1]).float()
        assert (dec - true).abs().max().item() <= 0.0025 + 2e-3, (r0, r1)
        assert (dec - aux[r0:r1].float()).abs().max().item() <= 0.0025 + 2 ** -8, (r0, r1)  # half a grid step + the bf16 rounding of the other form
        assert dec.min().item() >= -0.13 and dec.max().item() <= 1.145
    del pre, aux

    # backward-data epilogue: C = bf16(acc * decode(code)), bit for bit; column sums of the fp32 values before their rounding
    dy = _randn_bf16(M, Kd, g)
    wt = bf(torch.randn(N, Kd, device=DEV, generator=g) * 0.1)
    cs = torch.full((N,), float("nan"), device=DEV)
    assert K.gemm_nt_aux8_bytes(M, N, Kd, DEV, epilogue=L.EPI_MUL_AUX8, colsum=True) == nb
    got = K.gemm_nt(dy, wt, epilogue=L.EPI_MUL_AUX8, aux=codes, colsum=cs)
    acc = K.gemm_nt(dy, wt, out_f32=True)
    scale, off = float(torch.tensor(0.005, dtype=torch.float32)), float(torch.tensor(-0.13, dtype=torch.float32))
    ref_cs = torch.zeros(N, dtype=torch.float64, device=DEV)
    chunk = 4096  # (16 row tiles: the code index of a chunk is 168 MB of int64)
    for r0 in range(0, M, chunk):
        r1 = min(r0 + chunk, M)
        gq = (codes[_code_index(M, N, (r0, r1))].double() * scale + off).float()
        prod = acc[r0:r1].double() * gq.double()
        assert torch.equal(got[r0:r1], bf(prod.float())), (r0, r1)
        ref_cs += prod.sum(0)
    err = (cs.double() - ref_cs).abs().max().item()
    print(f"[headline aux8, {M} rows] fused column sums: max|err| {err:.3e} of max {ref_cs.abs().max().item():.3e}")
    assert err <= 1e-4 * ref_cs.abs().max().item() + 1e-3
    del acc
    # the last row tile is ragged (196 / 128 of 256 rows): the code bytes of its rows past the end must not reach C or the column sums
    pad = _code_index(last0 + 256, N, (M, last0 + 256))
    assert pad.numel() == (last0 + 256 - M) * N and int(pad.max()) < nb
    codes2 = codes.clone()
    codes2[pad] = 255 - codes[pad]
    cs2 = torch.full((N,), float("nan"), device=DEV)
    got2 = K.gemm_nt(dy, wt, epilogue=L.EPI_MUL_AUX8, aux=codes2, colsum=cs2)
    assert torch.equal(got2, got) and torch.equal(cs2, cs)
    torch.cuda.synchronize()
    print(f"[headline aux8, {M} rows] wall {time.time() - t_start:.1f} s")


def _ln_reference(x, dy, dres, gamma, beta, r0, r1, mask):
    """fp64 LayerNorm forward / backward of rows [r0, r1) (eps = 1e-5, as whisper.model.LayerNorm): y, mean, rstd, dx and the
    per-element products whose column sums are dgamma / dbeta.  mask = (rows_per_batch, t0, t1, c0, c1): the deep-SpecAugment span
    — y is zeroed there (masked_fill), so no gradient flows back through those elements; the residual gradient dres is not masked."""
    xs = x[r0:r1].double()
    mean = xs.mean(-1, keepdim=True)
    rstd = (xs.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    xh = (xs - mean) * rstd
    y = xh * gamma.double() + beta.double()
    d = dy[r0:r1].double()
    if mask is not None:
        rpb, t0, t1, c0, c1 = mask
        t = torch.arange(r0, r1, device=x.device) % rpb
        hit = ((t >= t0) & (t < t1)).view(-1, 1) | ((torch.arange(x.shape[1], device=x.device) >= c0) & (torch.arange(x.shape[1], device=x.device) < c1)).view(1, -1)
        y = y.masked_fill(hit, 0.0)
        d = d.masked_fill(hit, 0.0)
    gg = d * gamma.double()
    dx = rstd * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True)) + dres[r0:r1].double()
    return y, mean.view(-1), rstd.view(-1), dx, d * xh, d


def _rel_max(got, ref):
    return ((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-300)).item()


@pytest.mark.parametrize("clips", CLIPS)
def test_headline_layernorm_fwd_bwd(clips):
    """K.layernorm_fwd / K.layernorm_bwd at 144 000 x 1 280 and 130 500 x 1 280 (48 x the rows of test_kernels_gpu.test_layernorm_fwd_bwd),
    bf16 inputs, the residual gradient present, the dx column sums wanted: the instantiations the timed step runs (non-temporal loads and
    stores from 64 MB on; 512 partial rows of dgamma / dbeta folded in two levels).  y, mean, rstd, dx against fp64 math on three
    256-row blocks (first, one in the middle that crosses the masked time span, last) with that test's tolerances (1e-2 of max for the
    bf16 outputs, 1e-5 for mean; rstd, also fp32 statistics, gets the same 1e-5); dgamma, dbeta and the dx column sums against chunked
    fp64 reductions over ALL rows; two launches bit-equal (fixed fold order); the same with a deep-SpecAugment span, through the
    host-span entry points and through wft_layernorm_fwd_dspan / wft_layernorm_bwd_dspan (span in device memory), bit-equal to each other.

    Tolerance of the reductions: 1e-4 of max was set at 3 000 rows.  Here it is max(1e-4, 4 x e32), e32 = the error, relative to max, of
    a plain fp32 torch column sum (tensor.sum(0)) of the same fp32 products against their fp64 sum, measured in the test.  Measured on
    an MI355X (relative to max; kernel | plain fp32 torch sum, without the span):
      130 500 rows: dgamma 1.8e-07 | 2.7e-07, dbeta 6.4e-08 | 2.1e-07, dx sums 9.6e-08 | 2.2e-07
      144 000 rows: dgamma 2.2e-07 | 3.3e-07, dbeta 9.3e-08 | 3.4e-07, dx sums 1.1e-07 | 2.3e-07
    (with the span: dgamma 1.7e-07 / 1.8e-07, dbeta 8.8e-08 / 9.3e-08), so the bound in force is 1e-4 at both sizes: the kernel's fold
    (70 rows per wave, 4 waves, 512 partial rows in two levels) is more accurate than torch's fp32 column sum."""
    t_start = time.time()
    rows, cols = clips * T_ENC, 1280
    g = torch.Generator(device=DEV).manual_seed(clips)
    x = _randn_bf16(rows, cols, g, 2.0, 0.5)
    dy = _randn_bf16(rows, cols, g)
    dres = _randn_bf16(rows, cols, g)
    gamma = torch.randn(cols, device=DEV, generator=g)
    beta = torch.randn(cols, device=DEV, generator=g)
    span = (T_ENC, 700, 790, 400, 443)  # (rows_per_batch, t0, t1, c0, c1): deep SpecAugment's time 100 / freq 43 parameters
    mid = (clips // 2) * T_ENC + 600     # rows t = 600 .. 855 of a clip in the middle: crosses the masked time span
    blocks = ((0, 256), (mid, mid + 256), (rows - 256, rows))
    dev_span = torch.tensor(span[1:], dtype=torch.int32, device=DEV)

    def run(mask):
        y, mean, rstd = K.layernorm_fwd(x, gamma, beta, mask=mask)
        dx, dg, db, dxs = K.layernorm_bwd(dy, x, gamma, mean, rstd, dres, mask=mask, want_colsum=True)
        return y, mean, rstd, dx, dg, db, dxs

    for mask in (None, span):
        tag = f"[headline layernorm, {rows} rows, mask={mask is not None}]"
        y, mean, rstd, dx, dg, db, dxs = out = run(mask)
        again = run(mask)
        assert all(torch.equal(a, b) for a, b in zip(out, again)), "two launches: bit-equal (dgamma / dbeta fold in a fixed order)"
        for r0, r1 in blocks:
            ry, rmean, rrstd, rdx, _, _ = _ln_reference(x, dy, dres, gamma, beta, r0, r1, mask)
            assert _rel_max(y[r0:r1], ry) <= 1e-2, ("y", r0)
            assert _rel_max(mean[r0:r1], rmean) <= 1e-5, ("mean", r0)
            assert _rel_max(rstd[r0:r1], rrstd) <= 1e-5, ("rstd", r0)
            assert _rel_max(dx[r0:r1], rdx) <= 1e-2, ("dx", r0)
        if mask is not None:
            yv = y.view(clips, T_ENC, cols)
            assert not yv[:, span[1]:span[2]].any() and not yv[:, :, span[3]:span[4]].any()  # exact zeros, as masked_fill gives
        # dgamma / dbeta / dx column sums over all rows: chunked fp64, and the plain fp32 torch sums of the same fp32 products
        ref = {n: torch.zeros(cols, dtype=torch.float64, device=DEV) for n in ("dgamma", "dbeta", "dxsum")}
        p32 = {n: torch.empty(rows, cols, dtype=torch.float32, device=DEV) for n in ("dgamma", "dbeta")}
        for r0 in range(0, rows, 12000):
            r1 = min(r0 + 12000, rows)
            _, _, _, _, pg, pb = _ln_reference(x, dy, dres, gamma, beta, r0, r1, mask)
            ref["dgamma"] += pg.sum(0)
            ref["dbeta"] += pb.sum(0)
            ref["dxsum"] += dx[r0:r1].double().sum(0)  # (the sums of the bf16 values written: what wft_colsum_bf16 would read back)
            p32["dgamma"][r0:r1], p32["dbeta"][r0:r1] = pg.float(), pb.float()
        e32 = {n: _rel_max(p32[n].sum(0), p32[n].double().sum(0)) for n in p32}
        e32["dxsum"] = _rel_max(dx.float().sum(0), ref["dxsum"])
        del p32
        for n, got in (("dgamma", dg), ("dbeta", db), ("dxsum", dxs)):
            e = _rel_max(got, ref[n])
            tol = max(1e-4, 4 * e32[n])
            print(f"{tag} {n}: kernel {e:.2e}, plain fp32 torch column sum {e32[n]:.2e}, bound {tol:.2e}")
            assert e <= tol, (n, e, tol)
        if mask is not None:
            assert not dg[span[3]:span[4]].any() and not db[span[3]:span[4]].any()  # masked columns: no gradient at all
            # the span read from device memory (a captured graph replays the kernels with the values its host wrote there)
            dspan = run((T_ENC, dev_span))
            assert all(torch.equal(a, b) for a, b in zip(out, dspan)), "device-span entry points: bit-equal to the host-span call"
    torch.cuda.synchronize()
    print(f"[headline layernorm, {rows} rows] wall {time.time() - t_start:.1f} s")


def test_turbo_yaml_size_ce_gradient_rows_sum_to_zero():
    """config_turbo_best.yaml's B = 64 at S = 448: 28 672 rows x 51 866 classes, 2.98 GB of bf16 logits (row stride 51 968)."""
    rows, V = 64 * 448, 51866
    ld = K.round_up(V, 128)
    g = torch.Generator(device=DEV).manual_seed(2)
    logits = _randn_bf16(rows, ld, g)
    tgt = torch.randint(0, V, (rows,), device=DEV, generator=g)
    tgt[::7] = -100
    _, lse, stats, am = K.ce_fwd(logits, tgt, V, 0.1, want_argmax=True)
    for r0 in (0, rows - 512):
        assert torch.equal(am[r0:r0 + 512], logits[r0:r0 + 512, :V].float().argmax(-1))
        assert (lse[r0:r0 + 512] - torch.logsumexp(logits[r0:r0 + 512, :V].float(), -1)).abs().max().item() < 1e-3
    dl = K.ce_bwd(logits, tgt, V, 0.1, lse, stats, torch.ones(1, device=DEV), inplace=True)
    worst = 0.0
    for r0 in range(0, rows, 2048):
        worst = max(worst, dl[r0:r0 + 2048, :V].float().sum(-1).abs().max().item())
    assert worst < 1e-4
    assert not dl[::7, :V].any()  # ignored rows carry no gradient
