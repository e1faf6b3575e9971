"""Decoding with weights="w8a8" end to end on the GPU: whisper-tiny's widths with 2 + 2 layers (tests/_q8_cases.decode_case), B = 3,
ragged prompts of 12 / 9 / 14 tokens (B x widest = 42 > 32: every projection of the prefill takes the W8A8 kernel), 12 steps.

The W8A8 oracle is oracle.whisper_oracle.Oracle with its one seam, `linear(x, prefix)`, overridden: x rounded to bf16, x and the
bf16-rounded weight fake-quantised per row with the restated quantiser (_q8_cases.quantize_rows), the product in fp32.  Per-row
quantisation makes every row of a Linear independent of the others, so `act_rows` can say, per (audio, position), whether the
engine computed that decoder row in the prefill (activations quantised) or in a cached step (weight-only) — the oracle then mixes
the two exactly as the KV cache does.

 (a) dispatch: under "w8a8" every LinearGroup product of the encoder and of the prefill goes through K.gemm_nt_i8 — the count in
     closed form from the dims, the cross key / value projections included; under "bf16" and "int8" none does;
 (b) numerics: per audio, the engine's encoder output and the prefill's last-position logits under "w8a8" are closer (relative L2) to
     the W8A8 oracle than to the plain one; the prefill logits stay under the 2e-2 of tests/test_decode_graph_gpu.py; the encoder
     error against the W8A8 oracle is at most twice e0, the bf16 engine's error against the plain oracle measured in the same test
     (engine and oracle quantise activations that differ by bf16 roundings upstream, so a share of the int8 codes differs by one
     step: an error of the order of the quantisation step on those elements — hence two, not one);
 (c) prefix-following over 12 steps with tests/_decode_oracle.py's TAU / FLIP_SHARE as they stand;
 (d) an optimizer step between two calls: the second call's encoder output follows the new weights;
 (e) two w8a8 decodes are bit-identical, and "bf16" / "int8" results equal those of runs made before the first w8a8 call;
 (f) the evaluator's wft_eval_decode_weights: w8a8.

Measured on an MI355X: encoder output, worst audio, e0 = 0.00457 (bf16 engine vs plain oracle), w8a8 engine vs W8A8 oracle 0.00679
(ratio 1.49 of the cap 2; 0.00784 vs the plain oracle); 16.2 % of the first quantised activation's int8 codes differ from the oracle's, by at
most 2 steps.  Prefill logits per audio 0.0170 / 0.0199 / 0.0168 vs the W8A8 oracle, 0.0208 / 0.0216 / 0.0202 vs the plain one.  12 steps:
0 of 36 picks off the oracle's argmax, 0.0056-0.0066 per cached step.  After an optimizer step: 0.0059 vs the oracle on the new weights, 0.63 vs the old."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests import _decode_oracle as DO  # noqa: E402
from tests import _q8_cases as Q8  # noqa: E402
from tests.test_decode_graph_gpu import _text_batch  # noqa: E402
from tests.test_model_gpu import _engine  # noqa: E402
from whisper_finetune.engine import decode as D  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.eval import evaluator  # noqa: E402

DEV = torch.device("cuda:0")
EOT = 50257
STEPS = Q8.DECODE_STEPS
PROMPT_LEN = (12, 9, 14)


def _fq_rows(t: torch.Tensor, codes: list = None) -> torch.Tensor:
    """[..., K] -> every row bf16-rounded, quantised per row, q * scale (f32).  codes: a list that receives the int8 codes."""
    a = Q8.bf16_round(t.detach().float().reshape(-1, t.shape[-1]).numpy())
    q, s = Q8.quantize_rows(a)
    if codes is not None:
        codes.append(q)
    return torch.from_numpy((q.astype(np.float32) * s[:, None]).astype(np.float32)).reshape(t.shape)


class W8A8Oracle(O.Oracle):
    """act_rows: None — every Linear quantises its input rows; bool [B, L] — a decoder Linear whose input is [B, L, *] quantises
    only the rows marked True (the prompt positions, computed by the prefill) and reads the others as they are (cached steps:
    weight-only).  The cross key / value projections see the encoder output ([B, n_audio_ctx, d]) and always quantise it."""

    def __init__(self, dims, params):
        super().__init__(dims, params)
        self.act_rows = None
        self._fqw = {}
        self.first_codes = []  # the int8 codes of the first quantised activation: the input of encoder block 0's query projection

    def linear(self, x, prefix):
        if prefix not in self._fqw:
            self._fqw[prefix] = _fq_rows(self.weight(prefix))
        w, b = self._fqw[prefix], self.p.get(prefix + ".bias")
        y = F.linear(_fq_rows(x, self.first_codes if prefix == "encoder.blocks.0.attn.query" and not self.first_codes else None), w, b)
        rows = self.act_rows
        if rows is not None and prefix.startswith("decoder.") and x.dim() == 3 and tuple(x.shape[:2]) == tuple(rows.shape):
            y = torch.where(rows[..., None], y, F.linear(x, w, b))
        return y


@pytest.fixture(scope="module")
def case():
    dims, params, audio, _, _, y_in, y_out = Q8.decode_case()
    plen = torch.tensor(PROMPT_LEN)
    prompt = torch.full((Q8.DECODE_B, int(plen.max())), EOT, dtype=torch.int64)
    for b in range(Q8.DECODE_B):
        prompt[b, :plen[b]] = y_in[b, :plen[b]]
    assert prompt.shape[0] * prompt.shape[1] > 32
    m = _engine(dims, params).eval()
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    T = prompt.shape[1]
    kw = dict(eot=EOT, max_len=T + STEPS)
    args = (mel, prompt.to(DEV), plen)
    # runs made before the first w8a8 call in this process (e)
    first = {w: m.greedy_decode(*args, step="graph", weights=w, **kw) for w in ("bf16", "int8")}
    D.release_graphs(m)
    plain, w8 = O.Oracle(dims, params), W8A8Oracle(dims, params)
    with torch.no_grad():
        xa_plain, xa_w8 = plain.encoder(mel.float().cpu()), w8.encoder(mel.float().cpu())
    return dict(dims=dims, params=params, model=m, mel=mel, prompt=prompt.to(DEV), plen=plen, kw=kw, args=args, y_in=y_in, y_out=y_out,
                first=first, plain=plain, w8=w8, xa_plain=xa_plain, xa_w8=xa_w8)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.real = K.gemm_nt_i8

        def rec(a_q, a_scale, b_q, b_scale, **kw):
            self.calls.append((a_q.shape[0], b_q.shape[0], a_q.shape[1]))
            return self.real(a_q, a_scale, b_q, b_scale, **kw)

        K.gemm_nt_i8 = rec
        return self

    def __exit__(self, *exc):
        K.gemm_nt_i8 = self.real


def _same(a, b, what):
    for x, y, name in zip(a, b, ("tokens", "lengths", "sum_logprob")):
        assert torch.equal(x, y), f"{what}: {name} differ"


def test_dispatch_every_product_of_encoder_and_prefill_takes_the_i8_kernel(case):
    m, dims, args, kw = case["model"], case["dims"], case["args"], case["kw"]
    B, T, d, Ta = 3, max(PROMPT_LEN), dims.n_audio_state, dims.n_audio_ctx
    D.release_graphs(m)
    with _Recorder() as r:
        m.greedy_decode(*args, step="graph", weights="w8a8", **kw)
    enc = [(B * Ta, 3 * d, d), (B * Ta, d, d), (B * Ta, 4 * d, d), (B * Ta, d, 4 * d)] * dims.n_audio_layer
    # per decoder layer: fused q/k/v, self out, cross q, the cross key / value projection of the encoder output, cross out, mlp.0, mlp.2
    dec = [(B * T, 3 * d, d), (B * T, d, d), (B * T, d, d), (B * Ta, 2 * d, d), (B * T, d, d), (B * T, 4 * d, d), (B * T, d, 4 * d)] * dims.n_text_layer
    assert len(r.calls) == 4 * dims.n_audio_layer + 7 * dims.n_text_layer
    assert sorted(r.calls) == sorted(enc + dec), r.calls
    assert r.calls[:len(enc)] == enc  # the encoder first, block by block
    for blk in m.decoder.blocks:
        assert blk.cross_attn._kv_group.Q is not None
    used = [g for _, g in D._groups(m.encoder) if g.W is not None]
    assert len(used) == 4 * dims.n_audio_layer and all(g.Q is not None and g.qkey == g.key for g in used)
    # the cached steps of w8a8 are the int8 steps: they share that mode's session
    assert list(D.sessions(m)) == [(3, str(DEV), "int8")]
    for w in ("bf16", "int8"):
        with _Recorder() as r:
            m.greedy_decode(*args, step="graph", weights=w, **kw)
            m.beam_decode(*args, beam_size=2, step="graph", weights=w, **kw)
        assert r.calls == [], w
    with _Recorder() as r:  # the ladder runs the encoder itself and hands it on as _xa
        m.decode_with_fallback(*args, temperatures=(0.0,), step="graph", weights="w8a8", logprob_threshold=None, no_speech_threshold=None, **kw)
    assert sorted(r.calls) == sorted(enc + dec)
    with _Recorder() as r:  # a short prefill stays on the bf16 kernels: B x T = 27 <= 32; the encoder and the cross k / v do not
        short = torch.tensor(Q8.DECODE_PROMPT_LEN)
        m.greedy_decode(case["mel"], case["prompt"][:, :int(short.max())].contiguous(), short, step="graph", weights="w8a8", eot=EOT,
                        max_len=int(short.max()) + 2)
    assert r.calls == enc + [(B * Ta, 2 * d, d)] * dims.n_text_layer
    D.release_graphs(m)
    with pytest.raises(ValueError, match="w8a8.*graph"):
        m.greedy_decode(*args, weights="w8a8", **kw)


def test_encoder_and_prefill_follow_the_w8a8_oracle(case):
    m, dims, mel, prompt, plen, kw = case["model"], case["dims"], case["mel"], case["prompt"], case["plen"], case["kw"]
    plain, w8, xa_plain, xa_w8 = case["plain"], case["w8"], case["xa_plain"], case["xa_w8"]
    V, B = dims.n_vocab, prompt.shape[0]
    with torch.no_grad():
        xa_bf16 = m.encoder(mel)
        seen, real_q = [], K.quantize_rows_i8
        K.quantize_rows_i8 = lambda x, *a, **k: (seen.append(real_q(x, *a, **k)) or seen[-1])
        try:
            xa = D.encode(m, mel, "w8a8")
        finally:
            K.quantize_rows_i8 = real_q
        e0 = max(DO.rel(xa_bf16[b], xa_plain[b]) for b in range(B))
        per_row = [(DO.rel(xa[b], xa_w8[b]), DO.rel(xa[b], xa_plain[b])) for b in range(B)]
        e8 = max(a for a, _ in per_row)
        print(f"encoder output, worst audio: bf16 engine vs plain oracle e0 = {e0:.5f}; w8a8 engine vs W8A8 oracle = {e8:.5f} "
              f"(vs plain oracle {max(b for _, b in per_row):.5f}); ratio {e8 / e0:.3f} (cap 2)")
        # the share of int8 codes of the first quantised activation (the input of encoder block 0's fused q/k/v) that differ
        codes_eng, codes_ref = seen[0][0].cpu().numpy(), w8.first_codes[0]
        diff = codes_eng.astype(np.int32) - codes_ref.astype(np.int32)
        print(f"first quantised activation: {np.mean(diff != 0):.4f} of the int8 codes differ from the oracle's, largest difference {np.abs(diff).max()} step(s)")
        assert all(a < b for a, b in per_row), per_row
        cache = D.KVCache(m.decoder, B, device=DEV)
        cache.start(prompt, plen, n_vocab=V, **kw)
        with D.int8_gemm():
            logits = D.prefill(m.decoder, cache, xa)
        lens, toks = cache.len.cpu(), cache.tokens.cpu()
        got = logits[:, :V].float().cpu()
        w8.act_rows = None
        ref = DO.oracle_last_logits(w8, xa_w8, toks, lens)
        ref_plain = DO.oracle_last_logits(plain, xa_plain, toks, lens)
        rows = [(DO.rel(got[b], ref[b]), DO.rel(got[b], ref_plain[b])) for b in range(B)]
        print("prefill last-position logits per audio, (vs W8A8 oracle, vs plain oracle):", " ".join(f"({a:.4f}, {b:.4f})" for a, b in rows))
        assert all(a < b for a, b in rows), rows
        assert max(a for a, _ in rows) < 2e-2, rows
        assert e8 <= 2 * e0, (e8, e0)


def test_w8a8_decode_follows_the_oracle_prefix_by_prefix(case):
    m, dims, params = case["model"], case["dims"], case["params"]
    mel, prompt, plen, kw = case["mel"], case["prompt"], case["plen"], case["kw"]
    w8, xa_w8 = case["w8"], case["xa_w8"]
    V = dims.n_vocab
    fq_emb = torch.from_numpy(Q8.fake_quantize(params["decoder.token_embedding.weight"].detach().float().numpy()))
    tr = DO.Trace()
    rels = []
    try:
        with torch.no_grad():
            xa = D.encode(m, mel, "w8a8")
            cache = D.KVCache(m.decoder, prompt.shape[0], device=DEV)
            cache.start(prompt, plen, n_vocab=V, **kw)
            for i in range(STEPS):
                if i == 0:
                    with D.int8_gemm():
                        logits = D.prefill(m.decoder, cache, xa)
                else:
                    with D.stream_gemm(True, weights="int8"):
                        logits = D.step(m.decoder, cache)
                lens, toks = cache.len.cpu(), cache.tokens.cpu()
                got = logits[:, :V].float().cpu()
                L = int(lens.max())
                # prompt positions were computed by the prefill (activations quantised), later ones by weight-only steps; the tied
                # logits product of the prefill is bf16, that of a step reads the int8 image of the embedding
                w8.act_rows = torch.arange(L)[None, :] < plen[:, None]
                ref = Q8.oracle_last_logits(w8, xa_w8, toks, lens, None if i == 0 else fq_emb)
                rels.append(max(DO.rel(got[b], ref[b]) for b in range(got.shape[0])))
                tr.ref_logits.append(ref)
                tr.active.append(cache.finished.cpu() == 0)
                p, lp = D.pick(m.decoder, cache, logits, want_pick=True)
                tr.picks.append(p.cpu()); tr.logprobs.append(lp.cpu())
    finally:
        w8.act_rows = None
    print("w8a8 decode vs the W8A8 oracle (weight-only rows behind the prompt), worst row per step:", " ".join(f"{v:.4f}" for v in rels))
    assert max(rels) < 2e-2, rels
    DO.check_prefix_following(tr, "2 + 2 layers, B = 3, w8a8 encoder + prefill, int8 steps vs the W8A8 oracle")


def test_an_optimizer_step_reaches_the_images_in_front_of_the_encoder(case):
    dims, mel = case["dims"], case["mel"]
    m = _engine(dims, case["params"])
    m.eval()
    with torch.no_grad():
        xa1 = D.encode(m, mel, "w8a8")
    old = {id(g): g.Q.clone() for _, g in D._groups(m.encoder) if g.Q is not None}
    assert len(old) == 4 * dims.n_audio_layer
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    m(mel, case["y_in"].to(DEV), targets=case["y_out"].to(DEV), label_smoothing=0.1).backward()
    opt.step()
    m.eval()
    with torch.no_grad():
        xa2 = D.encode(m, mel, "w8a8")
    assert all(not torch.equal(g.Q, old[id(g)]) and g.qkey == g.key for _, g in D._groups(m.encoder) if g.Q is not None), "an encoder image was not refreshed"
    new_params = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref_new = W8A8Oracle(dims, new_params).encoder(mel.float().cpu())
    rows = [(DO.rel(xa2[b], ref_new[b]), DO.rel(xa2[b], case["xa_w8"][b]), DO.rel(xa1[b], case["xa_w8"][b])) for b in range(xa2.shape[0])]
    print("after an optimizer step, per audio (second call vs W8A8 oracle on the NEW weights, vs the one on the old weights; first call vs old):",
          " ".join(f"({a:.4f}, {b:.4f}; {c:.4f})" for a, b, c in rows))
    assert all(a < b for a, b, _ in rows), rows
    assert all(c < DO.rel(xa1[b], ref_new[b]) for b, (_, _, c) in enumerate(rows))


def test_w8a8_is_reproducible_and_leaves_nothing_behind(case):
    m, args, kw = case["model"], case["args"], case["kw"]
    D.release_graphs(m)
    a = m.greedy_decode(*args, step="graph", weights="w8a8", **kw)
    b = m.greedy_decode(*args, step="graph", weights="w8a8", **kw)
    _same(a, b, "two w8a8 decodes")
    assert not D.int8_gemm_active() and not D.stream_gemm_active()
    for w in ("bf16", "int8"):
        _same(m.greedy_decode(*args, step="graph", weights=w, **kw), case["first"][w], f"{w} after w8a8 vs before the first w8a8 call")
    _same(m.greedy_decode(*args, step="graph", weights="w8a8", **kw), a, "w8a8 again")
    # beam search and sampling take the keyword too
    bk = dict(beam_size=3, **kw)
    _same(m.beam_decode(*args, step="graph", weights="w8a8", **bk), m.beam_decode(*args, step="graph", weights="w8a8", **bk), "beam")
    sk = dict(temperature=0.7, best_of=2, seed=11, **kw)
    _same(m.sample_decode(*args, step="graph", weights="w8a8", **sk), m.sample_decode(*args, step="graph", weights="w8a8", **sk), "sampling")
    D.release_graphs(m)


def test_evaluator_w8a8_returns_finite_metrics(case):
    from whisper_finetune.data.data_loader import SimpleTokenizer

    m = case["model"]
    D.release_graphs(m)
    y_in, y_out = _text_batch(["the quick brown fox", "jumps over", "the lazy dog"])
    cfg = {"mixed_precision_training": True, "mp_dtype": "bf16", "wft_eval_decode": "greedy", "wft_eval_decode_step": "graph",
           "wft_eval_decode_weights": "w8a8"}
    with _Recorder() as r:
        got = evaluator.evaluate_single_dataset(m, [(case["mel"], y_in, y_out)], "syn", cfg, tokenizer=SimpleTokenizer())
    assert len(r.calls) >= 4 * case["dims"].n_audio_layer + case["dims"].n_text_layer  # the encoder and the cross key / value projections at least
    assert got.num_samples == 3 and np.isfinite(got.wer) and np.isfinite(got.cer) and np.isfinite(got.mean_token_nll)
    assert D.sessions(m) == {}
    with pytest.raises(ValueError, match="wft_eval_decode_weights"):
        evaluator.evaluate_single_dataset(m, [(case["mel"], y_in, y_out)], "syn", dict(cfg, wft_eval_decode_step="eager"), tokenizer=SimpleTokenizer())
