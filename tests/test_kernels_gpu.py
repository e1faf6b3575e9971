"""GPU parity tests of every libwft kernel, called through the C ABI (ctypes), against fp32 CPU
math (torch CPU / the oracle).  Tolerances: bit-exact for integer / index / pure-copy results;
fp32-accumulated results from bf16 inputs compare at 1e-5 (relative to max) when the output is
fp32 and at bf16 resolution (<= 1e-2 of max) when the output itself is rounded to bf16."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = "cuda:0"


def bf(x):
    return x.to(torch.bfloat16)


def close(got, ref, tol, what="", atol=1e-30):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-12
    assert math.isfinite(err) and err <= tol * scale + atol, f"{what}: max|err|={err:.3e} rel-to-max={err / scale:.3e} tol={tol}"


def test_casts_bit_exact():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1000, 77, generator=g)
    assert torch.equal(K.cast_bf16(x.to(DEV)).cpu(), bf(x))
    w = torch.randn(300, 256, generator=g)
    d, dt = K.weight_shadow(w.to(DEV), 384, 256, True)
    ref = torch.zeros(384, 256); ref[:300] = w
    assert torch.equal(d.cpu(), bf(ref)) and torch.equal(dt.cpu(), bf(ref).t())
    a, b = bf(torch.randn(4097, generator=g)), bf(torch.randn(4097, generator=g))
    assert torch.equal(K.add_bf16(a.to(DEV), b.to(DEV)).cpu(), bf(a.float() + b.float()))


@pytest.mark.parametrize("rows,cols", [(3000, 384), (777, 1280), (1, 512), (130, 2048)])
def test_layernorm_fwd_bwd(rows, cols):
    g = torch.Generator().manual_seed(rows)
    x = bf(torch.randn(rows, cols, generator=g) * 2 + 0.5)
    gamma = torch.randn(cols, generator=g); beta = torch.randn(cols, generator=g)
    y, mean, rstd = K.layernorm_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV))
    xr = x.float().requires_grad_(True); gr = gamma.clone().requires_grad_(True); br = beta.clone().requires_grad_(True)
    ref = O.layer_norm(xr, gr, br)
    close(y, ref, 1e-2, "ln fwd")
    close(mean, x.float().mean(-1), 1e-5, "mean")
    dy = bf(torch.randn(rows, cols, generator=g)); dres = bf(torch.randn(rows, cols, generator=g))
    ref.backward(dy.float())
    dx, dg, db = K.layernorm_bwd(dy.to(DEV), x.to(DEV), gamma.to(DEV), mean, rstd, dres.to(DEV))
    close(dx, xr.grad + dres.float(), 1e-2, "dx")
    close(dg, gr.grad, 1e-4, "dgamma")
    close(db, br.grad, 1e-4, "dbeta")


def test_layernorm_deep_specaug_mask():
    B, T, cols = 2, 150, 384
    g = torch.Generator().manual_seed(1)
    x = bf(torch.randn(B * T, cols, generator=g)); gamma = torch.randn(cols, generator=g); beta = torch.randn(cols, generator=g)
    y, mean, rstd = K.layernorm_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV), mask=(T, 10, 35, 100, 120))
    ref = O.layer_norm(x.float(), gamma, beta).view(B, T, cols).clone()
    ref[:, 10:35] = 0; ref[:, :, 100:120] = 0
    close(y, ref.view(B * T, cols), 1e-2)
    yc = y.view(B, T, cols)
    assert (yc[:, 10:35] == 0).all() and (yc[:, :, 100:120] == 0).all()  # exact zeros, as masked_fill gives


@pytest.mark.parametrize("M,N,Kd", [(256, 128, 64), (300, 256, 128), (1500, 384, 384), (4096, 1280, 1280), (1, 128, 64), (777, 1536, 5120)])
def test_gemm_nt_and_epilogues(M, N, Kd):
    g = torch.Generator().manual_seed(M + N)
    a = bf(torch.randn(M, Kd, generator=g)); b = bf(torch.randn(N, Kd, generator=g))
    bias = torch.randn(N, generator=g); res = bf(torch.randn(M, N, generator=g))
    ref = a.float() @ b.float().t()
    ad, bd = a.to(DEV), b.to(DEV)
    close(K.gemm_nt(ad, bd, out_f32=True), ref, 1e-5, "f32 out")
    close(K.gemm_nt(ad, bd, bias=bias.to(DEV), residual=res.to(DEV)), ref + bias + res.float(), 1e-2, "bias+res")
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    out = K.gemm_nt(ad, bd, bias=bias.to(DEV), epilogue=L.EPI_GELU, aux=aux)
    close(out, torch.nn.functional.gelu(ref + bias), 1e-2, "gelu")
    close(aux, ref + bias, 1e-2, "gelu pre")
    pre = aux.float().cpu().requires_grad_(True)
    torch.nn.functional.gelu(pre).backward(torch.ones_like(pre))
    close(K.gemm_nt(ad, bd, epilogue=L.EPI_DGELU, aux=aux), ref * pre.grad, 1e-2, "dgelu")
    close(K.gemm_nt(ad, bd, residual=res.to(DEV), residual_first=True, epilogue=L.EPI_GELU, aux=aux),
          torch.nn.functional.gelu(ref + res.float()), 1e-2, "residual-first gelu")
    # training pair: the forward stores gelu'(pre) (GELU_GRAD), the backward-data GEMM multiplies by it (MUL_AUX)
    dact = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    out2 = K.gemm_nt(ad, bd, bias=bias.to(DEV), epilogue=L.EPI_GELU_GRAD, aux=dact)
    close(out2, torch.nn.functional.gelu(ref + bias), 1e-2, "gelu (GELU_GRAD)")
    pre32 = (ref + bias).clone().requires_grad_(True)
    torch.nn.functional.gelu(pre32).backward(torch.ones_like(pre32))
    close(dact, pre32.grad, 1e-2, "gelu' (GELU_GRAD aux)")
    close(K.gemm_nt(ad, bd, epilogue=L.EPI_MUL_AUX, aux=dact), ref * dact.float().cpu(), 1e-2, "mul aux")


@pytest.mark.parametrize("M,N,Kd", [(70001, 1280, 128), (20000, 2560, 256), (33000, 1280, 1280)])
def test_gemm_nt_persistent_epilogues_counted_waits(M, N, Kd):
    """More tiles than CUs (persistent workgroups, continuous staging across tile seams), with the residual / aux operands
    whose rows the epilogue fetches ahead by inline-asm loads behind hand-counted s_waitcnt (gemm_pp256.hip, COUNTED body), and
    a ragged last row tile (general body): results against fp32 torch, and bit-identical over repeats (a miscounted wait
    or a seam race shows up as run-to-run differences)."""
    g = torch.Generator().manual_seed(M)
    a = bf(torch.randn(M, Kd, generator=g)).to(DEV); b = bf(torch.randn(N, Kd, generator=g) * 0.05).to(DEV)
    res = bf(torch.randn(M, N, generator=g)).to(DEV); aux = bf(torch.randn(M, N, generator=g)).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    ref = a.float() @ b.float().t()
    cases = {
        "bias+res": (lambda: K.gemm_nt(a, b, bias=bias, residual=res), ref + bias + res.float()),
        "res beta": (lambda: K.gemm_nt(a, b, residual=res, beta=0.5), ref + 0.5 * res.float()),
        "mul aux + colsum": (lambda: K.gemm_nt(a, b, epilogue=L.EPI_MUL_AUX, aux=aux, colsum=torch.empty(N, device=DEV)), ref * aux.float()),
        "gelu_grad": (lambda: K.gemm_nt(a, b, bias=bias, epilogue=L.EPI_GELU_GRAD, aux=torch.empty_like(res)),
                      torch.nn.functional.gelu(ref + bias)),
    }
    for name, (fn, want) in cases.items():
        first = fn()
        close(first, want, 1e-2, name)
        for _ in range(3):
            assert torch.equal(fn(), first), f"{name}: not reproducible"
    # fused column sums across full row tiles (register body) AND the ragged last one (direct body): every row counted once
    for epi, kw in ((L.EPI_MUL_AUX, dict(aux=aux)), (L.EPI_NONE, dict(residual=res)), (L.EPI_NONE, dict())):
        cs = torch.full((N,), 7.0, device=DEV)
        c = K.gemm_nt(a, b, epilogue=epi, colsum=cs, **kw)
        want_cs = c.double().sum(0)
        scale = c.double().abs().sum(0).max()
        assert (cs.double() - want_cs).abs().max() < 2e-3 * scale, "fused column sums"  # (sums of the un-rounded fp32 values)
        cs2 = torch.empty(N, device=DEV)
        K.gemm_nt(a, b, epilogue=epi, colsum=cs2, **kw)
        assert torch.equal(cs, cs2), "column sums not reproducible"


def test_gemm_nt_rejects_bad_shapes():
    a = torch.zeros(10, 70, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.WftError, match="K must be a multiple of 64"):
        K.gemm_nt(a, torch.zeros(128, 70, dtype=torch.bfloat16, device=DEV), K=70, lda=72, ldb=72)
    with pytest.raises(L.WftError, match="N must be a multiple of 128"):
        K.gemm_nt(torch.zeros(10, 64, dtype=torch.bfloat16, device=DEV), torch.zeros(200, 64, dtype=torch.bfloat16, device=DEV), N=200)


def test_conv1d_as_gemm_matches_conv():
    B, T, Cin, Cout = 2, 100, 128, 256
    g = torch.Generator().manual_seed(3)
    x = bf(torch.randn(B, Cin, T, generator=g)); w = bf(torch.randn(Cout, Cin, 3, generator=g)); bias = torch.randn(Cout, generator=g)
    xt = torch.zeros(B, T + 2, Cin); xt[:, 1:T + 1] = x.float().transpose(1, 2)
    xt = bf(xt).to(DEV)
    wk = w.permute(0, 2, 1).reshape(Cout, 3 * Cin).contiguous().to(DEV)
    ref1 = torch.nn.functional.conv1d(x.float(), w.float(), bias, padding=1).transpose(1, 2)
    out = torch.zeros((B, T + 2, Cout), dtype=torch.bfloat16, device=DEV)
    K.gemm_nt(xt, wk, M=T, N=Cout, K=3 * Cin, lda=Cin, ldb=3 * Cin, out=out[:, 1:], ldc=Cout, bias=bias.to(DEV), batch=B,
              strideA=(T + 2) * Cin, strideC=(T + 2) * Cout)
    close(out[:, 1:T + 1], ref1, 1e-2, "stride 1")
    assert (out[:, 0] == 0).all() and (out[:, T + 1] == 0).all()
    ref2 = torch.nn.functional.conv1d(x.float(), w.float(), bias, padding=1, stride=2).transpose(1, 2)
    out2 = K.gemm_nt(xt, wk, M=T // 2, N=Cout, K=3 * Cin, lda=2 * Cin, ldb=3 * Cin, bias=bias.to(DEV), batch=B,
                     strideA=(T + 2) * Cin, strideC=(T // 2) * Cout)
    close(out2.view(B, T // 2, Cout), ref2, 1e-2, "stride 2")


@pytest.mark.parametrize("R,P,Q", [(64, 128, 128), (100, 128, 256), (1, 128, 128), (1500, 384, 384), (4097, 1280, 256), (48000, 256, 128)])
def test_gemm_tn(R, P, Q):
    g = torch.Generator().manual_seed(R)
    a = bf(torch.randn(R, P, generator=g)); b = bf(torch.randn(R, Q, generator=g))
    ref = a.float().t() @ b.float()
    close(K.gemm_tn(a.to(DEV), b.to(DEV)), ref, 2e-5, "tn")
    c = torch.ones(P, Q, device=DEV)
    K.gemm_tn(a.to(DEV), b.to(DEV), out=c, accumulate=True)
    close(c, ref + 1, 2e-5, "tn accumulate")


def _ref_attn(q, k, v, H, causal, scale):
    B, Tq, D = q.shape
    Tk = k.shape[1]
    qh = q.view(B, Tq, H, 64).transpose(1, 2); kh = k.view(B, Tk, H, 64).transpose(1, 2); vh = v.view(B, Tk, H, 64).transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2)) * scale
    if causal:
        s = s + torch.full((Tq, Tk), float("-inf")).triu_(1)
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Tq, D), torch.logsumexp(s, -1)


@pytest.mark.parametrize("B,H,Tq,Tk,causal", [(2, 6, 1500, 1500, False), (2, 4, 128, 128, True), (3, 2, 37, 37, True),
                                              (2, 6, 50, 1500, False), (1, 20, 448, 448, True), (2, 2, 200, 77, False), (1, 1, 1, 1, True)])
def test_attention_fwd_bwd(B, H, Tq, Tk, causal):
    D = H * 64
    g = torch.Generator().manual_seed(Tq * 7 + Tk)
    q = bf(torch.randn(B, Tq, D, generator=g)); kv = bf(torch.randn(B, Tk, 2 * D, generator=g))
    k, v = kv[..., :D], kv[..., D:]
    qd, kvd = q.to(DEV), kv.to(DEV)
    o, lse = K.attn_fwd(qd, kvd[..., :D], kvd[..., D:], H, causal, 0.125)
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    oref, lref = _ref_attn(qr, kr, vr, H, causal, 0.125)
    close(o, oref, 2e-2, "o"); close(lse, lref, 1e-4, "lse")
    do = bf(torch.randn(B, Tq, D, generator=g))
    oref.backward(do.float())
    dq, dk, dv = K.attn_bwd(qd, kvd[..., :D], kvd[..., D:], o, lse, do.to(DEV), H, causal, 0.125)
    # atol: with one key the exact dq / dk are 0 (dP == delta); fp32 summation order leaves ~1e-8 on O(1) operands
    close(dq, qr.grad, 2e-2, "dq", atol=1e-6); close(dk, kr.grad, 2e-2, "dk", atol=1e-6); close(dv, vr.grad, 2e-2, "dv")


def test_attention_forced_rescale_branch():
    """online-softmax rescale: one key far above the rest in a late tile (cdna guide rule 26)."""
    B, H, T = 1, 1, 256
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, T, 64, generator=g); k = torch.randn(B, T, 64, generator=g); v = torch.randn(B, T, 64, generator=g)
    k[0, 200] = q[0, 17] * 40.0
    qd, kd, vd = (bf(t).to(DEV) for t in (q, k, v))
    o, lse = K.attn_fwd(qd, kd, vd, H, False, 0.125)
    oref, lref = _ref_attn(bf(q).float(), bf(k).float(), bf(v).float(), H, False, 0.125)
    close(o, oref, 2e-2); close(lse, lref, 1e-4)


def test_embedding_and_cross_entropy():
    B, S, d, V = 3, 17, 384, 1000
    g = torch.Generator().manual_seed(2)
    tok = torch.randint(0, V, (B, S), generator=g); emb = torch.randn(V, d, generator=g); pos = torch.randn(448, d, generator=g)
    out = K.embed_fwd(tok.to(DEV), emb.to(DEV), pos.to(DEV))
    close(out, emb[tok] + pos[:S], 1e-2)
    dout = bf(torch.randn(B, S, d, generator=g))
    demb = torch.zeros(V, d, device=DEV); dpos = torch.zeros(448, d, device=DEV)
    K.embed_bwd(tok.to(DEV), dout.to(DEV), demb, dpos)
    close(demb, torch.zeros(V, d).index_add_(0, tok.view(-1), dout.float().view(-1, d)), 1e-6)
    close(dpos[:S], dout.float().sum(0), 1e-6)
    for V, eps in ((51865, 0.0), (51866, 0.1), (1000, 0.05)):
        rows, ld = 50, K.round_up(V, 128)
        logits = bf(torch.randn(rows, ld, generator=g) * 3)
        tgt = torch.randint(0, V, (rows,), generator=g); tgt[::7] = -100
        lr = logits[:, :V].float().requires_grad_(True)
        ref = O.cross_entropy(lr.unsqueeze(0), tgt.unsqueeze(0), eps)
        (ref * 0.25).backward()
        ld_dev = logits.to(DEV)
        row_loss, row_lse, stats, am = K.ce_fwd(ld_dev, tgt.to(DEV), V, eps, want_argmax=True)
        close((stats[0] / stats[1]).reshape(1), ref.reshape(1), 2e-5, "loss")  # fp32 sum of 5e4 exps, different order
        assert torch.equal(am.cpu(), lr.argmax(-1))  # teacher-forced argmax: bit-exact token ids
        dl = K.ce_bwd(ld_dev, tgt.to(DEV), V, eps, row_lse, stats, torch.tensor([0.25], device=DEV))
        close(dl[:, :V], lr.grad, 1e-2, "dlogits")
        assert (dl[:, V:] == 0).all()
    # all-ignored batch edge case: loss 0/0 is NaN in torch as well; here stats[1] == 0
    _, _, stats, _ = K.ce_fwd(bf(torch.randn(4, 128)).to(DEV), torch.full((4,), -100).to(DEV), 100, 0.0)
    assert stats[1].item() == 0 and stats[0].item() == 0


@pytest.mark.parametrize("n_mels", [80, 128])
def test_logmel_matches_oracle_and_golden(n_mels, golden_logmel):
    clips = []
    for i in range(2):
        a = torch.randn(O.N_SAMPLES, generator=torch.Generator().manual_seed(1234 + i)) * 0.1
        if i == 1:
            a[200000:] = 0.0
            a[:200000] *= torch.linspace(0.0, 1.0, 200000)
        clips.append(a)
    t = np.arange(O.N_SAMPLES) / 16000.0
    clips.append(torch.from_numpy((0.3 * np.sin(2 * np.pi * (200.0 + 120.0 * t) * t)).astype(np.float32)))
    audio = torch.stack(clips)
    got = K.logmel(audio.to(DEV), O.mel_filters(n_mels).to(DEV)).cpu()
    ref = O.log_mel_spectrogram(audio, n_mels)
    d = (got - ref).abs()
    assert d.max() < 2e-3 and d.mean() < 1e-5, (d.max(), d.mean())
    dg = np.abs(got[:, :, ::7].numpy() - golden_logmel[f"mel{n_mels}_sub"])
    assert np.quantile(dg, 0.999) < 2e-4 and dg.max() < 5e-3


def test_specaug_matches_reference_golden(golden_host):
    """time-warp + masks kernel vs the reference's own TimeWarpAugmenter output.  Tolerance 1e-3 absolute: the
    warped sample position (~1e3 frames) carries fp32 rounding of ~1e-4 frames in both implementations."""
    spec = torch.from_numpy(golden_host["tw_spec"])
    for i in range(3):
        wp, wd = (int(v) for v in golden_host[f"tw_params{i}"])
        params = torch.tensor([[1, wp, wd, 0, 0, 0, 0, 0]], dtype=torch.int32, device=DEV)
        got = K.specaug(spec[None].to(DEV), params).cpu()[0]
        assert (got - torch.from_numpy(golden_host[f"tw_out{i}"])).abs().max() < 1e-3
    # masks + extremes are exact
    mel = torch.randn(2, 16, 300)
    params = torch.tensor([[0, 0, 0, 100, 180, 3, 9, 0], [0, 0, 0, 290, 300, 0, 0, 0]], dtype=torch.int32, device=DEV)
    ext = torch.tensor([[2, 3], [0, 0]], dtype=torch.int32, device=DEV)
    got = K.specaug(mel.to(DEV), params, ext).cpu()
    ref0 = O.spec_augment(mel[0], None, (100, 180), (3, 9), (2, 3)); ref1 = O.spec_augment(mel[1], None, (290, 300), (0, 0))
    assert torch.equal(got[0], ref0) and torch.equal(got[1], ref1)
    tm = K.mel_to_tmajor(mel.to(DEV), 128).cpu()
    ref_t = torch.zeros(2, 302, 128); ref_t[:, 1:301, :16] = mel.transpose(1, 2)
    assert torch.equal(tm, bf(ref_t))


def test_adamw_matches_torch():
    n = 100003
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=g); grad = torch.randn(n, generator=g)
    pr = torch.nn.Parameter(p0.clone()); pr.grad = grad * 0.5
    opt = torch.optim.AdamW([pr], lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.1)
    p = p0.to(DEV); gd = grad.to(DEV); m = torch.zeros(n, device=DEV); v = torch.zeros(n, device=DEV)
    gs = torch.tensor([0.5], device=DEV)
    for step in (1, 2, 3):
        opt.step()
        K.adamw_step(p, gd, m, v, None, 1e-3, 0.9, 0.98, 1e-6, 0.1, 1 - 0.9 ** step, 1 - 0.98 ** step, gs)
    close(p, pr.data, 1e-6)
    out = torch.zeros(1, device=DEV)
    K.sumsq(gd, out)
    close(out, (grad.double() ** 2).sum().float().reshape(1), 1e-5)


# ---- BASELINE-size (large-v3, 32 clips) size-independent properties -------------------------------------------
def test_full_size_gemm_linearity_and_identity():
    M, N, Kd = 48000, 1280, 1280
    g = torch.Generator(device=DEV).manual_seed(0)
    a1 = bf(torch.randn(M, Kd, device=DEV, generator=g)); a2 = bf(torch.randn(M, Kd, device=DEV, generator=g))
    eye = bf(torch.eye(N, Kd, device=DEV))
    assert torch.equal(K.gemm_nt(a1, eye), a1)  # A @ I^T == A exactly
    w = bf(torch.randn(N, Kd, device=DEV, generator=g) * 0.05)
    y1 = K.gemm_nt(a1, w, out_f32=True); y2 = K.gemm_nt(a2, w, out_f32=True)
    s = bf(a1.float() + a2.float())  # rounded sum: compare against the GEMM of exactly that operand
    r = K.gemm_nt(s, w, out_f32=True)
    lin = y1 + y2
    resid = (s.float() - (a1.float() + a2.float()))
    corr = K.gemm_nt(bf(resid), w, out_f32=True)  # first-order correction for the operand rounding
    assert ((r - lin - corr).abs().max() / lin.abs().max()).item() < 2e-3


def test_full_size_attention_rows_are_convex_combinations():
    B, H, T = 4, 20, 1500
    g = torch.Generator(device=DEV).manual_seed(1)
    q = bf(torch.randn(B, T, H * 64, device=DEV, generator=g)); k = bf(torch.randn(B, T, H * 64, device=DEV, generator=g))
    v = torch.ones(B, T, H * 64, device=DEV, dtype=torch.bfloat16)
    o, lse = K.attn_fwd(q, k, v, H, False, 0.125)
    assert (o.float() - 1).abs().max().item() < 1e-2  # softmax weights sum to 1
    dq, dk, dv = K.attn_bwd(q, k, v, o, lse, torch.ones_like(o), H, False, 0.125)
    assert dq.float().abs().max().item() < 2e-2 and dk.float().abs().max().item() < 2e-2  # d(softmax)·1 = 0
    assert (dv.float().view(B, T, H, 64).sum(1) - T).abs().max().item() < 0.02 * T  # each head's weights sum to T over queries


def test_full_size_ce_gradient_rows_sum_to_zero():
    rows, V = 4096, 51866
    ld = K.round_up(V, 128)
    g = torch.Generator(device=DEV).manual_seed(2)
    logits = bf(torch.randn(rows, ld, device=DEV, generator=g))
    tgt = torch.randint(0, V, (rows,), device=DEV, generator=g)
    _, lse, stats, am = K.ce_fwd(logits, tgt, V, 0.1, want_argmax=True)
    assert torch.equal(am, logits[:, :V].float().argmax(-1))
    dl = K.ce_bwd(logits, tgt, V, 0.1, lse, stats, torch.ones(1, device=DEV), inplace=False)
    assert dl[:, :V].float().sum(-1).abs().max().item() < 1e-4


def test_gemm_tn_split_k_is_bitwise_reproducible():
    """Weight-gradient GEMM at the BASELINE size: the split-K partials go through the workspace and are summed in a
    fixed order, so two launches agree bit for bit (the fp32-atomic fallback does not)."""
    g = torch.Generator(device=DEV).manual_seed(5)
    a = bf(torch.randn(48000, 1280, device=DEV, generator=g)); b = bf(torch.randn(48000, 1280, device=DEV, generator=g))
    c1 = K.gemm_tn(a, b); c2 = K.gemm_tn(a, b)
    assert torch.equal(c1, c2)
    ref = a[:6000].float().t() @ b[:6000].float()
    close(K.gemm_tn(a[:6000], b[:6000]), ref, 2e-5)
    acc = torch.ones(1280, 1280, device=DEV)
    K.gemm_tn(a, b, out=acc, accumulate=True)
    close(acc, c1 + 1, 1e-6)


@pytest.mark.parametrize("R,P,Q", [(48000, 128, 1280), (3000, 384, 1536), (24000, 1280, 128)])
def test_gemm_tn_128_tile_split_k_is_bitwise_reproducible(R, P, Q):
    """The 128x128 weight-gradient kernel (rank-r LoRA gradients, small models) splits the reduction up to 64 ways; its
    partial tiles go through the workspace + fixed-order reduce as well, so repeated launches agree bit for bit, with and
    without accumulation into C."""
    g = torch.Generator(device=DEV).manual_seed(R + P)
    a = bf(torch.randn(R, P, device=DEV, generator=g)); b = bf(torch.randn(R, Q, device=DEV, generator=g))
    outs = [K.gemm_tn(a, b) for _ in range(4)]
    assert all(torch.isfinite(o).all() for o in outs), [int((~torch.isfinite(o)).sum()) for o in outs]
    assert all(torch.equal(outs[0], o) for o in outs[1:]), [
        (int((outs[0] != o).sum()), float((outs[0] - o).abs().max())) for o in outs[1:]]
    close(outs[0], a.float().t() @ b.float(), 2e-5)
    accs = []
    for _ in range(2):
        acc = torch.full((P, Q), 0.5, device=DEV)
        K.gemm_tn(a, b, out=acc, accumulate=True)
        accs.append(acc)
    assert torch.equal(accs[0], accs[1])
    close(accs[0], outs[0] + 0.5, 1e-6)


@pytest.mark.parametrize("rows,cols,r,masked", [(384, 384, 16, True), (1536, 384, 4, False), (100, 200, 64, True)])
def test_lora_merge_matches_minlora_parametrization(rows, cols, r, masked):
    """wft_lora_merge: W + s*B@(A*mask) as f32 (merge_lora) and as padded bf16 shadows (+T) for the GEMMs."""
    g = torch.Generator().manual_seed(rows + r)
    W = torch.randn(rows, cols, generator=g) * 0.05
    A = torch.randn(r, cols, generator=g) * 0.1
    B = torch.randn(rows, r, generator=g) * 0.1
    mask = (torch.rand(1, cols, generator=g) > 0.2).float() / 0.8 if masked else None
    want = W + (B @ (A if mask is None else A * mask)) * 2.0
    rp, cp = K.round_up(rows, 128), K.round_up(cols, 128)
    out = torch.full((rp, cp), 7.0, dtype=torch.bfloat16, device=DEV)
    out_t = torch.full((cp, rp), 7.0, dtype=torch.bfloat16, device=DEV)
    out32 = torch.empty(rows, cols, device=DEV)
    K.lora_merge(W.to(DEV), B.to(DEV), A.to(DEV), None if mask is None else mask.to(DEV), 2.0, out=out, out_t=out_t, out_f32=out32)
    assert (out32.cpu() - want).abs().max() < 1e-5
    assert torch.equal(out[:rows, :cols].cpu(), out32.cpu().to(torch.bfloat16))      # shadow = bf16(f32 result)
    assert torch.equal(out_t.cpu(), out.cpu().t())
    assert out[rows:].abs().sum() == 0 and out[:, cols:].abs().sum() == 0          # pad written as zeros
    with pytest.raises(L.WftError):
        K.lora_merge(W.to(DEV), torch.zeros(rows, 65, device=DEV), torch.zeros(65, cols, device=DEV), None, 1.0, out_f32=out32)


def test_sd_rescale_kernel_and_transpose():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 77, 40, generator=g).to(torch.bfloat16).to(DEV)
    y = torch.randn(3, 77, 40, generator=g).to(torch.bfloat16).to(DEV)
    s = 1 / 0.9
    got = K.axpby_bf16(1 - s, x, s, y)
    want = ((1 - s) * x.float() + s * y.float()).to(torch.bfloat16)
    assert (got.float() - want.float()).abs().max() <= 2 ** -7 * want.float().abs().max()
    assert torch.equal(K.axpby_bf16(2.0, x), (2.0 * x.float()).to(torch.bfloat16))
    t = torch.empty(3, 40, 77, dtype=torch.bfloat16, device=DEV)
    assert torch.equal(K.transpose_bf16(x, t), x.transpose(1, 2).contiguous())


def test_fused_bias_gradient_column_sums():
    """colsum(dx) out of the LayerNorm backward and colsum(C) out of the 256x256 GEMM epilogue (and its fallback)."""
    g = torch.Generator().manual_seed(9)
    rows, cols = 3000, 384
    x = torch.randn(rows, cols, generator=g).to(torch.bfloat16).to(DEV)
    dy = torch.randn(rows, cols, generator=g).to(torch.bfloat16).to(DEV)
    dres = torch.randn(rows, cols, generator=g).to(torch.bfloat16).to(DEV)
    gamma = (1 + 0.1 * torch.randn(cols, generator=g)).to(DEV)
    _, mean, rstd = K.layernorm_fwd(x, gamma, torch.zeros(cols, device=DEV))
    dx, dg, db, cs = K.layernorm_bwd(dy, x, gamma, mean, rstd, dres, want_colsum=True)
    dx2, dg2, db2 = K.layernorm_bwd(dy, x, gamma, mean, rstd, dres)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    want = dx.float().sum(0)
    assert (cs - want).abs().max() < 1e-3 * want.abs().max() + 1e-3
    # GEMM epilogue (M >= 1024, N % 256 == 0 -> 256 kernel, fused) and the 128-kernel fallback
    for M, N, Kd in ((2304, 512, 256), (300, 384, 128)):
        a = (torch.randn(M, Kd, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
        b = (torch.randn(N, Kd, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
        pre = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
        cs = torch.full((N,), 123.0, device=DEV)
        c = K.gemm_nt(a, b, epilogue=L.EPI_DGELU, aux=pre, colsum=cs)
        c0 = K.gemm_nt(a, b, epilogue=L.EPI_DGELU, aux=pre)
        assert torch.equal(c, c0)
        want = c.float().sum(0)
        assert (cs - want).abs().max() < 4e-3 * want.abs().max() + 1e-2  # fused sums are of the un-rounded fp32 values


@pytest.mark.parametrize("rows,cols,ld", [(70001, 384, 384), (204000, 1280, 1280), (65536, 64, 128), (3000, 384, 384), (24000, 512, 512), (8192, 2048, 2048)])
def test_colsum_chunked_over_the_chip(rows, cols, ld):
    """wft_colsum_bf16_ws (large inputs: 64 row chunks, folded in chunk order) and the one-pass kernel (small inputs): column
    sums of a bf16 matrix with a row stride, accumulate form, bitwise reproducible."""
    g = torch.Generator().manual_seed(rows + cols)
    buf = bf(torch.randn(rows, ld, generator=g)).to(DEV)
    x = buf[:, :cols]
    want = x.double().sum(0)
    got = K.colsum(x)
    tol = 1e-5 * x.double().abs().sum(0).max().item() + 1e-4
    assert (got.double() - want).abs().max().item() < tol
    assert torch.equal(K.colsum(x), got)
    base = torch.randn(cols, generator=g).to(DEV)
    acc = K.colsum(x, out=base.clone(), accumulate=True)
    assert (acc.double() - (want + base.double())).abs().max().item() < tol
    assert (L.load().wft_colsum_workspace_bytes(rows, cols) > 0) == (rows >= 8192)


@pytest.mark.parametrize("B,H,Tq,Tk,causal", [(2, 3, 1500, 1500, False), (2, 2, 130, 130, True), (1, 2, 50, 333, False)])
def test_attention_backward_fused_projection_bias_sums(B, H, Tq, Tk, causal):
    """dq_colsum / dv_colsum of wft_attn_bwd_bf16 = column sums of the bf16 dq / dv it wrote (ragged last 32-row groups,
    waves beyond T, causal early exit)."""
    D = H * 64
    g = torch.Generator().manual_seed(B + Tq)
    q = bf(torch.randn(B, Tq, D, generator=g)).to(DEV); k = bf(torch.randn(B, Tk, D, generator=g)).to(DEV)
    v = bf(torch.randn(B, Tk, D, generator=g)).to(DEV); do = bf(torch.randn(B, Tq, D, generator=g)).to(DEV)
    o, lse = K.attn_fwd(q, k, v, H, causal, 0.125)
    cs_q = torch.full((D,), 7.0, device=DEV); cs_v = torch.full((D,), 7.0, device=DEV)
    dq, dk, dv = K.attn_bwd(q, k, v, o, lse, do, H, causal, 0.125, colsums=(cs_q, cs_v))
    dq0, dk0, dv0 = K.attn_bwd(q, k, v, o, lse, do, H, causal, 0.125)
    assert torch.equal(dq, dq0) and torch.equal(dk, dk0) and torch.equal(dv, dv0)
    for got, full in ((cs_q, dq), (cs_v, dv)):
        want = full.float().sum((0, 1))
        assert (got - want).abs().max() < 2e-4 * want.abs().max() + 1e-3


@pytest.mark.parametrize("R,Q,rc", [(48000, 1280, 16), (5000, 5120, 48), (3001, 384, 64), (48000, 5120, 32), (100, 256, 16),
                                    (449, 128, 32), (64, 128, 16), (1, 128, 16)])
def test_gemm_tn_p_valid_skips_only_zero_columns(R, Q, rc):
    """Weight-gradient GEMM with a rank-r operand in its 128-wide zero-padded buffer (dA = du^T x, dB^T = u^T dy): p_valid selects
    the load-stream kernel for rank-r operands (gemm_tn_rank_kernel: compact A staging, only the valid rows of the split-K
    partials in the workspace) and gives exactly the result of the 128-tile kernel (same products, same order), padding rows of
    C zero; ragged reduction lengths, one-step and one-row reductions, a single split (direct store) and accumulation."""
    g = torch.Generator().manual_seed(R + rc)
    a = torch.zeros(R, 128)
    a[:, :rc - 5] = torch.randn(R, rc - 5, generator=g)
    a = bf(a).to(DEV)
    b = bf(torch.randn(R, Q, generator=g)).to(DEV)
    full = K.gemm_tn(a, b)
    fast = K.gemm_tn(a, b, p_valid=rc)
    assert torch.equal(full, fast)
    assert torch.count_nonzero(fast[rc:]) == 0
    close(fast, a.float().t() @ b.float(), 2e-5)
    again = K.gemm_tn(a, b, p_valid=rc)
    assert torch.equal(fast, again)  # split-K through the workspace: reproducible
    base = torch.randn(128, Q, generator=g).to(DEV)
    acc = K.gemm_tn(a, b, out=base.clone(), accumulate=True, p_valid=rc, alpha=0.5)
    want = K.gemm_tn(a, b, out=base.clone(), accumulate=True, alpha=0.5)
    assert torch.equal(acc, want)
    assert torch.equal(acc[rc + 15:], base[rc + 15:])  # accumulation leaves the padding rows alone


@pytest.mark.parametrize("R,Q,nb,r", [(48000, 1280, 1, 16), (5000, 3840, 3, 16), (449, 256, 2, 8), (100, 128, 1, 16), (3001, 2560, 2, 32),
                                      (2000, 384, 3, 8), (1000, 384, 3, 5), (777, 256, 2, 24), (64, 128, 1, 1)])
def test_gemm_tn_adapter_gradient_outputs(R, Q, nb, r):
    """The two output forms of the rank-r weight-gradient GEMM that finish the LoRA adapter gradients inside the split-K reduce
    (wft.h tn_col_scale / tn_block_n): dA = (du^T x) * mask with one mask row per adapter of the group, and dB as per-adapter
    [out, r] row-major blocks (the transposed diagonal blocks of u^T dy) — both exactly the plain product followed by the
    torch ops they replace, also with a single split (short reductions) and when accumulating."""
    g = torch.Generator().manual_seed(R + Q + r)
    rtot, n = nb * r, Q // nb
    a = torch.zeros(R, 128)
    a[:, :rtot] = torch.randn(R, rtot, generator=g)
    a = bf(a).to(DEV)
    b = bf(torch.randn(R, Q, generator=g)).to(DEV)
    ref = K.gemm_tn(a, b, p_valid=rtot)
    scale = (torch.rand(nb, Q, generator=g) < 0.8).float().mul(1.25).to(DEV)
    got = K.gemm_tn(a, b, p_valid=rtot, col_scale=scale, scale_rows=r if nb > 1 else 0)
    want = ref.clone()
    for i in range(nb):
        want[i * r:(i + 1) * r] *= scale[i]
    assert got.shape == (rtot, Q) and torch.equal(got, want[:rtot])  # compact: p_valid rows, nothing written below them
    guard = torch.full((rtot + 4, Q), 3.0, device=DEV)
    K.gemm_tn(a, b, p_valid=rtot, col_scale=scale, scale_rows=r if nb > 1 else 0, out=guard, accumulate=False)
    assert torch.equal(guard[:rtot], want[:rtot]) and bool((guard[rtot:] == 3.0).all())
    blocks = K.gemm_tn(a, b, p_valid=rtot, block_n=n, block_r=r)
    assert blocks.shape == (Q * r,)
    for i in range(nb):
        assert torch.equal(blocks[i * n * r:(i + 1) * n * r].view(n, r), ref[i * r:(i + 1) * r, i * n:(i + 1) * n].t())
    base = torch.randn(Q * r, generator=g).to(DEV)
    acc = K.gemm_tn(a, b, p_valid=rtot, block_n=n, block_r=r, out=base.clone(), accumulate=True)
    assert torch.equal(acc, base + blocks)
    with pytest.raises(Exception):
        K.gemm_tn(a, b, col_scale=scale)  # only for rank-r operands


@pytest.mark.parametrize("M,Kx,Ny,nb,r", [(48000, 1280, 1280, 1, 16), (4096, 1280, 3840, 3, 16), (3001, 384, 1280, 2, 8), (130, 5120, 1280, 1, 64)])
def test_rank_pair_launches_are_bit_identical_to_the_single_ones(M, Kx, Ny, nb, r):
    """wft_gemm_nt_rank_pair_bf16 / wft_gemm_tn_rank_pair_bf16: the four rank-r products of an adapted group's backward as two
    paired launches (+ one reduce launch) give exactly what the four single calls give — ragged M, one to three adapters,
    column scale and block layout included; unequal rank blocks fall back to the single entry points."""
    g = torch.Generator().manual_seed(M + Kx + Ny)
    rtot = nb * r
    x = bf(torch.randn(M, Kx, generator=g)).to(DEV); dy = bf(torch.randn(M, Ny, generator=g)).to(DEV)
    Am = torch.zeros(128, Kx); Am[:rtot] = torch.randn(rtot, Kx, generator=g) * 0.1
    BbT = torch.zeros(128, Ny); BbT[:rtot] = torch.randn(rtot, Ny, generator=g) * 0.1
    Am, BbT = bf(Am).to(DEV), bf(BbT).to(DEV)
    pvb = 16 * ((rtot + 15) // 16)
    du1, u1 = K.gemm_nt(dy, BbT, p_valid=rtot), K.gemm_nt(x, Am, p_valid=rtot)
    du2, u2 = K.gemm_nt_rank_pair(dy, BbT, x, Am, rtot)
    assert torch.equal(du1[:, :pvb], du2[:, :pvb]) and torch.equal(u1[:, :pvb], u2[:, :pvb])
    mask = (torch.rand(nb, Kx, generator=g) < 0.9).float().mul(1 / 0.9).to(DEV)
    n0 = Ny // nb
    kw_a = dict(a=du1, b=x, p_valid=rtot, col_scale=mask, scale_rows=r if nb > 1 else 0)
    kw_b = dict(a=u1, b=dy, p_valid=rtot, block_n=n0, block_r=r)
    dA1, dB1 = K.gemm_tn(**kw_a), K.gemm_tn(**kw_b)
    dA2, dB2 = K.gemm_tn_rank_pair(kw_a, kw_b)
    assert torch.equal(dA1, dA2) and torch.equal(dB1, dB2)
    for _ in range(2):
        dA3, dB3 = K.gemm_tn_rank_pair(kw_a, kw_b)
        assert torch.equal(dA3, dA2) and torch.equal(dB3, dB2)
    # different rank blocks in the two products: the library falls back to two single launches
    du4, u4 = K.gemm_nt_rank_pair(dy, BbT, x, Am, rtot) if rtot > 16 else (du2, u2)
    assert torch.equal(du4[:, :pvb], du2[:, :pvb])


@pytest.mark.parametrize("M,Kd,rc", [(48000, 1280, 16), (4096, 5120, 48), (3001, 384, 64), (100, 128, 32), (1, 64, 16)])
def test_gemm_nt_p_valid_writes_only_the_rank_columns(M, Kd, rc):
    """u = x (sA*mask)^T / du = dy (sB): the rank-r operand sits in the first rows of a 128-row zero-padded buffer; p_valid selects the
    load-stream kernel (gemm_nt_rank_kernel), which gives exactly the 128-tile kernel's values in the 16*ceil(p_valid/16) data
    columns and leaves the other columns of the output buffer untouched; ragged M, one k-step, one row."""
    g = torch.Generator().manual_seed(M + rc)
    b = torch.zeros(128, Kd)
    b[:rc - 3] = torch.randn(rc - 3, Kd, generator=g)
    b = bf(b).to(DEV)
    a = bf(torch.randn(M, Kd, generator=g)).to(DEV)
    full = K.gemm_nt(a, b)
    out = torch.full((M, 128), 7.0, dtype=torch.bfloat16, device=DEV)
    K.gemm_nt(a, b, out=out, p_valid=rc)
    nc = 16 * ((rc + 15) // 16)
    assert torch.equal(out[:, :nc], full[:, :nc])
    assert (out[:, nc:] == 7.0).all()
    close(out[:, :nc].float(), (a.float() @ b.float().t())[:, :nc], 1e-2)


def test_rank_kernels_random_shapes():
    """The two load-stream kernels for rank-r LoRA operands against the 128-tile kernels on 40 seeded random shapes each: every
    rank 1..64, reduction / row counts that are not multiples of the tile, k extents of one to 40 steps — bit-identical."""
    rng = np.random.RandomState(1234)
    for _ in range(40):
        M, Kd, rc = int(rng.randint(1, 4000)), 64 * int(rng.randint(1, 41)), int(rng.randint(1, 65))
        g = torch.Generator().manual_seed(M * 7 + rc)
        b = torch.zeros(128, Kd)
        b[:rc] = torch.randn(rc, Kd, generator=g)
        a, b = bf(torch.randn(M, Kd, generator=g)).to(DEV), bf(b).to(DEV)
        nc = 16 * ((rc + 15) // 16)
        out = torch.full((M, 128), -3.0, dtype=torch.bfloat16, device=DEV)
        K.gemm_nt(a, b, out=out, p_valid=rc)
        assert torch.equal(out[:, :nc], K.gemm_nt(a, b)[:, :nc]) and (out[:, nc:] == -3.0).all(), (M, Kd, rc)
    for _ in range(40):
        R, Q, rc = int(rng.randint(1, 6000)), 128 * int(rng.randint(1, 9)), int(rng.randint(1, 65))
        g = torch.Generator().manual_seed(R * 5 + rc)
        a = torch.zeros(R, 128)
        a[:, :rc] = torch.randn(R, rc, generator=g)
        a, b = bf(a).to(DEV), bf(torch.randn(R, Q, generator=g)).to(DEV)
        assert torch.equal(K.gemm_tn(a, b, p_valid=rc), K.gemm_tn(a, b)), (R, Q, rc)
