"""Model-versus-oracle parity in the kernel dispatch regime of the timed step (VERDICT r6 "What's weak" 1 / "Next round" 1).

bench.py times whisper-large-v3 at 96 clips: every encoder Linear runs on gemm_nt4w_kernel, every encoder weight gradient on
gemm_tn4w_kernel, the MLP carries gelu' as ONE BYTE per element (WFT_EPI_GELU_GRAD8 / WFT_EPI_MUL_AUX8 with the fused column sums),
the tied logits run on a 256-tile kernel.  All of these need >= 128 output tiles and M >= 1024 (gemm.hip nt_uses_256, tn_uses_256;
ops.py LinearFn.forward), which the 1- and 2-clip oracle tests of test_large_v3_gpu.py / test_model_gpu.py do not reach: there the
engine takes the 128-tile kernels and the bf16 gelu' pair (at 2 clips of large-v3 only the fused QKV and fc1 pass 128 tiles; every
other Linear, every weight gradient and the logits stay on the 128-tile kernels).  Here: large-v3 width and heads, 2 + 2 layers,
8 clips, S = 128 —

    8 x 1500 = 12 000 encoder rows = 47 row tiles x 5 / 15 / 20 column tiles (every encoder Linear >= 128 tiles, ragged last row
    tile: 12 000 = 46 x 256 + 224), 188 reduction steps of 64 rows for every encoder dW (the 1280 x 1280 products just pass
    tn_uses_256: 25 output tiles, >= 128 steps), 8 x 128 = 1 024 decoder rows (tied logits: 4 x 203 tiles of 256), Tq = 128 in the
    cross-attention (dK/dV eligible for attn_bwd_dkdv4w_kernel<false>)

— a size the CPU oracle still evaluates in ~15 s per pass.  Loss and every gradient tensor (88: the 89 state-dict entries less the
sinusoid buffer) against both oracle evaluations with the conditioning-aware bounds of test_large_v3_gpu.py (its harness, imported,
bounds unchanged), and the dispatch is ASSERTED from spies on K.gemm_nt / K.gemm_tn / K.attn_fwd / K.attn_bwd (variants from
wft_gemm_nt_variant / wft_gemm_tn_variant / wft_attn_variant on the very argument structs), so that the test goes red instead of
silently measuring another path when a threshold moves.
Reference arithmetic: whisper.model.Whisper.forward + F.cross_entropy(label_smoothing) as restated in oracle/whisper_oracle.py
(model/model_utils.py:54-73 of the reference)."""
import ctypes as C
import time
from collections import Counter

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402
from whisper_finetune.engine import ops  # noqa: E402
from whisper_finetune.engine.whisper_model import ModelDimensions, Whisper  # noqa: E402
from whisper_finetune.model import lora as lora_mod  # noqa: E402

from tests.test_large_v3_gpu import DEV, _both_oracles, _check, _oracle_grads, _report, rel  # noqa: E402

CLIPS, SEQ = 8, 128
DIMS = O.ModelDimensions(128, 1500, 1280, 20, 2, 51866, 448, 1280, 20, 2)
ROWS = CLIPS * DIMS.n_audio_ctx   # 12 000 encoder rows
DROWS = CLIPS * SEQ               # 1 024 decoder rows
D, H4 = DIMS.n_audio_state, 4 * DIMS.n_audio_state
VPAD = K.round_up(DIMS.n_vocab, 128)
BF16_GELU_EPIS = (L.EPI_GELU, L.EPI_DGELU, L.EPI_GELU_GRAD, L.EPI_MUL_AUX)


def _params(seed=7):
    params = O.init_params(DIMS, seed=seed)  # the CPU generator
    g = torch.Generator().manual_seed(seed + 1)
    for k, v in params.items():  # non-trivial biases / LayerNorm gains (test_large_v3_gpu._large_v3_params): every gradient term counts
        if k.endswith("bias"):
            params[k] = torch.randn(v.shape, generator=g) * 0.02
        elif "ln" in k and k.endswith("weight"):
            params[k] = 1 + torch.randn(v.shape, generator=g) * 0.05
    return params


def _inputs():
    audio, y_in, y_out = O.synthetic_batch(DIMS, CLIPS, SEQ)
    y_out[CLIPS - 1, :7] = -100  # a ragged ignored prefix on one clip
    return audio, y_in, y_out


class _Spies:
    """Records every K.gemm_nt / K.gemm_tn / K.attn_fwd / K.attn_bwd call of a step with the kernel the library answers for its
    argument struct (the pattern of test_gelu_aux8_gpu._mlp_grads, plus the variant queries).  `phase` is set by the caller."""

    def __init__(self):
        self.nt, self.tn, self.afwd, self.abwd, self.phase = [], [], [], [], "fwd"

    def __enter__(self):
        lib = L.load()
        self.real = (K.gemm_nt, K.gemm_tn, K.attn_fwd, K.attn_bwd)
        real_nt, real_tn, real_fwd, real_bwd = self.real

        def nt(a, b, **kw):
            paired = bool(kw.get("_args_only"))  # (K.gemm_nt_rank_pair builds its two structs through this wrapper)
            args, _ = real_nt(a, b, **{**kw, "_args_only": True})
            self.nt.append(dict(phase=self.phase, epi=args.epilogue, M=args.M, N=args.N, K=args.K, batch=args.batch, p_valid=args.p_valid,
                                colsum=bool(args.colsum), residual=bool(args.residual), paired=paired,
                                variant=lib.wft_gemm_nt_variant(C.byref(args))))
            return real_nt(a, b, **kw)

        def tn(a, b, **kw):
            paired = bool(kw.get("_args_only"))
            res = real_tn(a, b, **{**kw, "_args_only": True})
            if res is not None:  # (None: a segmented call the library does not take; the caller re-issues it unsegmented)
                args = res[0]
                self.tn.append(dict(phase=self.phase, P=args.M, Q=args.N, R=args.K, batch=args.batch, p_valid=args.p_valid, paired=paired,
                                    seg=args.tn_seg_count, variant=lib.wft_gemm_tn_variant(C.byref(args))))
            return real_tn(a, b, **kw)

        def attn_args(q, k, v, n_head, causal, scale, do=None):
            a = L.AttnArgs()
            a.q, a.ldq, a.q_bs = K._attn_view(q)
            a.k, a.ldk, a.k_bs = K._attn_view(k)
            a.v, a.ldv, a.v_bs = K._attn_view(v)
            a.B, a.H, a.Tq, a.Tk, a.causal, a.scale = q.shape[0], n_head, q.shape[1], k.shape[1], int(causal), scale
            a.variant = K._attn_variant_bits()
            if do is not None:
                do = do if do.stride(2) == 1 else do.contiguous()  # (as K.attn_bwd does)
                _, a.lddo, a.do_bs = K._attn_view(do)
            return a

        def fwd(q, k, v, n_head, causal, scale, *rest, **kw):
            a = attn_args(q, k, v, n_head, causal, scale)
            self.afwd.append(dict(B=a.B, Tq=a.Tq, Tk=a.Tk, causal=bool(causal), fwd=lib.wft_attn_variant(C.byref(a), 0)))
            return real_fwd(q, k, v, n_head, causal, scale, *rest, **kw)

        def bwd(q, k, v, o, lse, do, n_head, causal, scale, *rest, **kw):
            a = attn_args(q, k, v, n_head, causal, scale, do)
            self.abwd.append(dict(B=a.B, Tq=a.Tq, Tk=a.Tk, causal=bool(causal), dq=lib.wft_attn_variant(C.byref(a), 1),
                                  dkdv=lib.wft_attn_variant(C.byref(a), 2)))
            return real_bwd(q, k, v, o, lse, do, n_head, causal, scale, *rest, **kw)

        K.gemm_nt, K.gemm_tn, K.attn_fwd, K.attn_bwd = nt, tn, fwd, bwd
        return self

    def __exit__(self, *exc):
        K.gemm_nt, K.gemm_tn, K.attn_fwd, K.attn_bwd = self.real
        return False


def _engine_step(model, mel, y_in, y_out):
    """forward + label-smoothed CE + backward under the spies -> (loss tensor, spies)"""
    with _Spies() as spy:
        loss = model(mel, y_in.to(DEV), targets=y_out.to(DEV), label_smoothing=0.1)
        spy.phase = "bwd"
        loss.backward()
    torch.cuda.synchronize()
    return loss, spy


def _full_model(params):
    m = Whisper(ModelDimensions(**vars(DIMS)))
    m.load_state_dict(params)
    return m.to(DEV).train()


def _shapes(recs, *keys):
    return Counter(tuple(r[k] for k in keys) for r in recs)


def _assert_full_finetune_dispatch(spy, aux8=True):
    """Every dispatch expectation is evaluated; the failure lists all that do not hold."""
    nl, bad = DIMS.n_audio_layer, []

    def expect(ok, what, detail=None):
        if not ok:
            bad.append((what, detail))

    # ---- the encoder-row Linears: self-attention QKV / out, fc1 / fc2 of each encoder block and the decoder's cross-attention K / V
    # projections of the encoder output (x: 12 000 rows) — forward and backward-data
    enc = [r for r in spy.nt if r["M"] == ROWS and r["batch"] == 1]
    f, b = [r for r in enc if r["phase"] == "fwd"], [r for r in enc if r["phase"] == "bwd"]
    print("[regime] encoder-row NT products (N, K, epilogue, variant): forward", sorted(_shapes(f, "N", "K", "epi", "variant").items()),
          "| backward", sorted(_shapes(b, "N", "K", "epi", "variant").items()))
    epi_f, epi_b = (L.EPI_GELU_GRAD8, L.EPI_MUL_AUX8) if aux8 else (L.EPI_GELU_GRAD, L.EPI_MUL_AUX)
    expect(_shapes(f, "N", "K", "epi") == Counter({(3 * D, D, L.EPI_NONE): nl, (D, D, L.EPI_NONE): nl, (H4, D, epi_f): nl, (D, H4, L.EPI_NONE): nl,
                                                  (2 * D, D, L.EPI_NONE): DIMS.n_text_layer}),
           "the forward's encoder-row Linears (N, K, epilogue)", _shapes(f, "N", "K", "epi"))
    # backward-data: fc2 (the gelu' multiply with the fused column sums = fc1's bias gradient), fc1, out, QKV per block, K / V
    # projections of each decoder block (summed into one running gradient of the encoder output: ops.GradAccum)
    expect(_shapes(b, "N", "K", "epi") == Counter({(H4, D, epi_b): nl, (D, H4, L.EPI_NONE): nl, (D, D, L.EPI_NONE): nl, (D, 3 * D, L.EPI_NONE): nl,
                                                  (D, 2 * D, L.EPI_NONE): DIMS.n_text_layer}),
           "the backward's encoder-row data products (N, K, epilogue)", _shapes(b, "N", "K", "epi"))
    if aux8:
        expect(sum(r["epi"] == L.EPI_GELU_GRAD8 for r in f) == nl, "WFT_EPI_GELU_GRAD8 once per encoder block in the forward")
        mul = [r for r in b if r["epi"] == L.EPI_MUL_AUX8]
        expect(len(mul) == nl, "WFT_EPI_MUL_AUX8 once per encoder block in the backward")
        expect(all(r["colsum"] == bool(ops.BIAS_GRADS[0]) for r in mul), "fc1's bias gradient comes out of the gelu' multiply's epilogue", mul)
        expect(not [r for r in enc if r["epi"] in BF16_GELU_EPIS], "no encoder MLP on the bf16 gelu' pair")
        expect(not [r for r in spy.nt if r["epi"] in (L.EPI_GELU_GRAD8, L.EPI_MUL_AUX8) and r["M"] != ROWS], "the one-byte form on encoder rows only")
    else:
        expect(not [r for r in spy.nt if r["epi"] in (L.EPI_GELU_GRAD8, L.EPI_MUL_AUX8)], "no one-byte form with ops._GELU_AUX8 off")
    expect(enc and all(r["variant"] == 4 for r in enc), "every encoder-row Linear on gemm_nt4w_kernel (variant 4)", [r for r in enc if r["variant"] != 4])
    # (the decoder's MLPs, 1 024 rows = 4 x 20 tiles < 128, stay on the 128-tile kernel and the bf16 pair: the regime boundary)
    dec_mlp = [r for r in spy.nt if r["M"] == DROWS and r["N"] == H4 and r["K"] == D and r["phase"] == "fwd"]
    expect(len(dec_mlp) == DIMS.n_text_layer and all(r["epi"] == L.EPI_GELU_GRAD and r["variant"] == 128 for r in dec_mlp),
           "the decoder's fc1 on the 128-tile kernel with the bf16 pair", dec_mlp)
    # ---- encoder weight gradients: 12 000 reduction rows
    dw = [r for r in spy.tn if r["R"] == ROWS and r["batch"] == 1]
    print("[regime] encoder-row TN products (P, Q, variant):", sorted(_shapes(dw, "P", "Q", "variant").items()))
    expect(_shapes(dw, "P", "Q") == Counter({(3 * D, D): nl, (D, D): nl, (H4, D): nl, (D, H4): nl, (2 * D, D): DIMS.n_text_layer}),
           "the encoder-row weight-gradient products (P, Q)", _shapes(dw, "P", "Q"))
    expect(dw and all(r["variant"] == 4 for r in dw), "every encoder weight gradient on gemm_tn4w_kernel (variant 4)", [r for r in dw if r["variant"] != 4])
    # ---- tied logits: [1 024, 1280] x [51 968, 1280]^T
    logits = [r for r in spy.nt if r["phase"] == "fwd" and r["M"] == DROWS and r["N"] == VPAD and r["K"] == D]
    print("[regime] tied-logits GEMM variant:", [r["variant"] for r in logits])
    expect(len(logits) == 1 and logits[0]["variant"] != 128, "the tied-logits GEMM on a 256-tile kernel", logits)
    bad += _attention_dispatch_violations(spy)
    assert not bad, bad


def _attention_dispatch_violations(spy):
    T, bad = DIMS.n_audio_ctx, []
    enc_f = [r for r in spy.afwd if (r["Tq"], r["Tk"], r["causal"]) == (T, T, False)]
    enc_b = [r for r in spy.abwd if (r["Tq"], r["Tk"], r["causal"]) == (T, T, False)]
    if not (len(enc_f) == len(enc_b) == DIMS.n_audio_layer and all(r["fwd"] == 2 for r in enc_f) and all((r["dq"], r["dkdv"]) == (4, 4) for r in enc_b)):
        bad.append(("encoder attention on attn_fwd_pipe_kernel / attn_bwd_dq4w_kernel / attn_bwd_dkdv4w_kernel (2 / 4 / 4)", (enc_f, enc_b)))
    cross_b = [r for r in spy.abwd if (r["Tq"], r["Tk"], r["causal"]) == (SEQ, T, False)]
    if not (len(cross_b) == DIMS.n_text_layer and all(r["dkdv"] == 4 for r in cross_b)):
        bad.append(("cross-attention dK / dV on attn_bwd_dkdv4w_kernel<false> (4)", cross_b))
    if not all(r["B"] == CLIPS for r in spy.afwd + spy.abwd):
        bad.append(("every attention call covers the whole batch", None))
    return bad


def test_dispatch_regime_full_finetune_step_matches_oracle():
    """Loss (1e-3 against the emulated oracle, 2e-3 against the fp32 one) and all 88 gradients (test_large_v3_gpu._check, bounds
    unchanged) of one engine step at 8 clips, with the dispatch asserted; then the same step with the bf16 gelu' pair
    (ops._GELU_AUX8 = False, fresh model, same parameters): bit-equal loss (the forward values do not depend on the form), and on
    every tensor the one-byte form is no further from the fp32 oracle than the bf16 pair + 2e-3 (the margin of
    test_gelu_aux8_gpu.test_mlp_gradients_with_one_byte_derivative_against_fp32_math).

    Measured on an MI355X (relative L2 per tensor; max / median over the 88): emulated against fp32 oracle (cond) 0.030 / 0.0074, GPU
    against emulated 0.030 / 0.0055, GPU against fp32 0.039 / 0.0076, the maxima on the decoder's self-attention q / k of block 1;
    everywhere else at most 0.0088 / 0.0128.  One-byte form against bf16 pair: the largest rel(one-byte) - rel(pair) is 1.9e-5.

    What this catches: STRUCTURAL faults of the wiring in ops.py and of the kernels at this size — a wrong tile-to-buffer mapping of
    the code buffer, the ragged last row tile (224 of 256 rows), a code buffer reused or under-sized between two blocks, a missing or
    doubled bias-gradient term of the fused column sums, a product that silently changed kernel.  Each moves the mlp.0.* (or the
    affected Linear's) gradients by tens of per cent against bounds of 2-6 %.
    What it does NOT catch: a one-code offset of the gelu' grid.  0.005 in gelu' moves a gradient by less than 1 %, inside the bf16
    noise of any two evaluations; tests/test_gelu_aux8_gpu.py pins the codes and the multiply bit for bit instead."""
    t_start = time.time()
    params = _params()
    audio, y_in, y_out = _inputs()
    mel_ref = O.log_mel_spectrogram(audio, DIMS.n_mels)
    mel = K.logmel(audio.to(DEV), O.mel_filters(DIMS.n_mels).to(DEV))
    assert (mel.cpu() - mel_ref).abs().max() < 2e-3

    m = _full_model(params)
    loss, spy = _engine_step(m, mel, y_in, y_out)
    got = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
    del m
    _assert_full_finetune_dispatch(spy, aux8=True)

    old = ops._GELU_AUX8
    ops._GELU_AUX8 = False
    try:
        m = _full_model(params)
        loss_b, spy_b = _engine_step(m, mel, y_in, y_out)
        got_b = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
        del m
    finally:
        ops._GELU_AUX8 = old
    _assert_full_finetune_dispatch(spy_b, aux8=False)
    torch.cuda.empty_cache()
    t_engine = time.time() - t_start

    mel_cpu = mel.cpu()

    def run(emulate):
        p_req = {k: v.clone().requires_grad_(k != "encoder.positional_embedding") for k, v in params.items()}
        loss_ref = _oracle_grads(DIMS, p_req, mel_cpu if emulate else mel_ref, y_in, y_out, emulate)
        return loss_ref, {n: p_req[n].grad for n in got}

    t0 = time.time()
    res = _both_oracles(run)
    t_oracle = time.time() - t0
    for emulate, ltol in ((True, 1e-3), (False, 2e-3)):
        print(f"[regime] loss {loss.item():.6f} vs oracle (emulate_bf16={emulate}) {res[emulate][0]:.6f}")
        assert abs(loss.item() - res[emulate][0]) < ltol * res[emulate][0], (emulate, loss.item(), res[emulate][0])
    # (89 state-dict entries; the encoder's sinusoid positions are a buffer, not a parameter)
    assert len(params) == 89 and len(got) == len([k for k in params if k != "encoder.positional_embedding"]) == 88
    _check(got, res[True][1], res[False][1], "regime full-FT")

    # ---- A/B: the one-byte form against the bf16 pair, both against the fp32 oracle
    assert loss_b.item() == loss.item(), (loss_b.item(), loss.item())
    f32 = res[False][1]
    e8 = {n: rel(got[n], f32[n]) for n in got}
    e16 = {n: rel(got_b[n], f32[n]) for n in got}
    _report(e8, "regime one-byte gelu' vs fp32 oracle")
    _report(e16, "regime bf16 gelu' pair vs fp32 oracle")
    mlp0 = sorted(n for n in got if ".mlp.0." in n and n.startswith("encoder"))
    print("[regime] encoder mlp.0.* (one-byte, bf16 pair):", {n: (round(e8[n], 5), round(e16[n], 5)) for n in mlp0})
    diff = {n: e8[n] - e16[n] for n in got}
    print(f"[regime] largest rel(one-byte) - rel(bf16 pair): {max(diff.items(), key=lambda kv: kv[1])}")
    worse = {n: (e8[n], e16[n]) for n in got if e8[n] > e16[n] + 2e-3}
    assert not worse, worse
    print(f"[regime] wall: two engine steps + dispatch checks {t_engine:.1f} s, two oracle passes side by side {t_oracle:.1f} s, "
          f"total {time.time() - t_start:.1f} s")


def test_dispatch_regime_lora_step_matches_oracle():
    """The same dimensions and inputs with rank-16 adapters (alpha 32, a FIXED non-trivial dropout mask per Linear, p = 0.1) built as
    test_large_v3_lora_muon_config_step_matches_oracle builds them: lora.apply_lora attaches them to every Linear — the attention
    projections, whose fused groups are the rank-r kernels' multi-adapter forms, and the MLPs.  At 12 000 rows the merged-shadow
    forward runs on gemm_nt4w_kernel and the rank-r products (x A^T, dy B, the two adapter gradients) take 12 000 rows / reduction
    rows; no model-level test reached either.  All 64 adapter gradients against both oracles: _check with the adapter medians
    3e-2 / 3e-2, loss 1e-3 / 2e-3.  Measured on an MI355X (max / median): cond 0.040 / 0.0079, GPU against emulated 0.041 / 0.0061,
    GPU against fp32 0.040 / 0.0085; outside the decoder's self-attention q / k at most 0.0096 / 0.0128."""
    t_start = time.time()
    params = _params()
    audio, y_in, y_out = _inputs()
    mel_ref = O.log_mel_spectrogram(audio, DIMS.n_mels)
    mel = K.logmel(audio.to(DEV), O.mel_filters(DIMS.n_mels).to(DEV))
    r, alpha, p_drop = 16, 32, 0.1
    m = Whisper(ModelDimensions(**vars(DIMS)))
    m.load_state_dict(params)
    torch.manual_seed(17)  # lora_A's kaiming init draws from the global generator: the same adapters in every run
    lora_mod.apply_lora(m, {"rank": r, "lora_alpha": alpha, "lora_dropout": p_drop})
    g = torch.Generator().manual_seed(23)
    adapters = {}
    for name, mod in m.named_modules():
        if "parametrizations" in mod._modules:
            ad = mod.parametrizations.weight[0]
            with torch.no_grad():
                ad.lora_B.copy_(torch.randn(ad.lora_B.shape, generator=g) * 0.02)
            mask = (torch.rand(1, ad.lora_A.shape[1], generator=g) >= p_drop).float() / (1.0 - p_drop)
            adapters[name] = (ad, mask)
    assert len(adapters) == 6 * DIMS.n_audio_layer + 10 * DIMS.n_text_layer
    assert all(any(f"{side}.blocks.{i}.{a}.{p}" in adapters for p in ("query", "key", "value", "out"))
               for side, a, i in (("encoder", "attn", 0), ("decoder", "attn", 1), ("decoder", "cross_attn", 0)))
    m.to(DEV).train()
    for ad, mask in adapters.values():
        dev_mask = mask.to(DEV)
        ad.draw_mask = (lambda mk: (lambda training: mk))(dev_mask)
    loss, spy = _engine_step(m, mel, y_in, y_out)
    named = dict(m.named_parameters())
    assert all(p.grad is None for n, p in named.items() if "lora" not in n)  # base stays frozen
    got = {}
    for n, (ad, _) in adapters.items():
        got[n + ".lora_A"], got[n + ".lora_B"] = ad.lora_A.grad.detach().cpu(), ad.lora_B.grad.detach().cpu()

    # dispatch: merged-shadow forward and backward-data products of the encoder-row Linears on gemm_nt4w_kernel; the rank-r products
    # (p_valid = 16) at 12 000 rows / reduction rows; no full weight-gradient product (the base is frozen); attention as without adapters
    enc = [x for x in spy.nt if x["M"] == ROWS and x["batch"] == 1 and x["p_valid"] == 0]
    print("[regime LoRA] encoder-row NT products (phase, N, K, epilogue, variant):", sorted(_shapes(enc, "phase", "N", "K", "epi", "variant").items()))
    assert _shapes([x for x in enc if x["phase"] == "fwd"], "N", "K") == Counter(
        {(3 * D, D): DIMS.n_audio_layer, (D, D): DIMS.n_audio_layer, (H4, D): DIMS.n_audio_layer, (D, H4): DIMS.n_audio_layer,
         (2 * D, D): DIMS.n_text_layer})
    assert all(x["variant"] == 4 for x in enc), [x for x in enc if x["variant"] != 4]
    rank_nt = [x for x in spy.nt if x["M"] == ROWS and x["p_valid"] > 0]
    rank_tn = [x for x in spy.tn if x["R"] == ROWS and x["p_valid"] > 0]
    print("[regime LoRA] rank-r products at 12 000 rows: NT", sorted(_shapes(rank_nt, "N", "K", "p_valid", "paired").items()),
          "| TN", sorted(_shapes(rank_tn, "P", "Q", "p_valid", "paired").items()))
    # two NT products (x A^T, dy B) and two TN products (the adapter gradients) per Linear group whose input has 12 000 rows; a fused
    # group stacks its adapters in one rank-r operand: QKV 3 x 16 and the decoder's K / V 2 x 16 valid rows, out / fc1 / fc2 16
    per_group = Counter({3 * r: 2 * DIMS.n_audio_layer, 2 * r: 2 * DIMS.n_text_layer, r: 2 * 3 * DIMS.n_audio_layer})
    assert _shapes(rank_nt, "p_valid") == Counter({(k,): v for k, v in per_group.items()}) == _shapes(rank_tn, "p_valid")
    assert all(x["phase"] == "bwd" for x in rank_nt + rank_tn)
    assert not [x for x in spy.tn if x["p_valid"] == 0], "frozen base weights: no full weight-gradient product"
    assert not _attention_dispatch_violations(spy)
    t_engine = time.time() - t_start

    mel_cpu = mel.cpu()
    cfgs = {e: {n: (ad.lora_A.detach().cpu().clone().requires_grad_(True), ad.lora_B.detach().cpu().clone().requires_grad_(True),
                    ad.scaling, mask) for n, (ad, mask) in adapters.items()} for e in (True, False)}
    del m
    torch.cuda.empty_cache()
    t0 = time.time()
    res = _both_oracles(lambda e: _oracle_grads(DIMS, params, mel_cpu if e else mel_ref, y_in, y_out, e, lora=cfgs[e]))
    t_oracle = time.time() - t0
    refs = {}
    for emulate, ltol in ((True, 1e-3), (False, 2e-3)):
        print(f"[regime LoRA] loss {loss.item():.6f} vs oracle (emulate_bf16={emulate}) {res[emulate]:.6f}")
        assert abs(loss.item() - res[emulate]) < ltol * res[emulate], (emulate, loss.item(), res[emulate])
        refs[emulate] = {}
        for n, (A, Bm, _, _) in cfgs[emulate].items():
            refs[emulate][n + ".lora_A"], refs[emulate][n + ".lora_B"] = A.grad, Bm.grad
    assert len(got) == 2 * len(adapters) == 64
    _check(got, refs[True], refs[False], "regime LoRA", emu_med=3e-2, f32_med=3e-2)
    print(f"[regime LoRA] wall: engine step + dispatch checks {t_engine:.1f} s, two oracle passes side by side {t_oracle:.1f} s, "
          f"total {time.time() - t_start:.1f} s")
