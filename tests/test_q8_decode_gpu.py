"""Decoding with weights="int8" end to end on the GPU: whisper-tiny's widths with 2 + 2 layers (tests/_q8_cases.decode_case),
B = 3, ragged prompts of 4 / 6 / 9 tokens, 12 steps.

 (a) a captured int8 step changes nothing against the same steps issued launch by launch (greedy, beam W = 3, sampled best_of = 2):
     bit equality; one capture, then replays; bf16 sessions live apart;
 (b) every group's (Q, scale) is the restated quantiser's image of its own bf16 shadow W, also after an optimizer step;
 (c) prefix-following against the fp32 oracle over FAKE-QUANTISED decoder weights (bf16-rounded, restated quantiser, q * scale) with
     tests/_decode_oracle.py's TAU and FLIP_SHARE as they stand — and at every step the cached logits are closer to that oracle than
     to the one over the unquantised weights: int8 weights were really read.  What the engine leaves in bf16 / fp32 — the cross key /
     value projections, the embedding lookup — is left unquantised in the oracle too.  On the CPU the fake-quantised oracle against
     its own bf16-emulation mode on these inputs (seed 0) needs no TAU excuse at all: 0 of 36 picks differ, relative L2 <= 0.0068.
     Measured on an MI355X: worst row per step 0.0051-0.0056 against the fake-quantised oracle, 0.0161-0.0170 against the
     unquantised one, 0 of 36 picks off the oracle's argmax.
 (d) the evaluator's wft_eval_decode_weights: int8."""
import numpy as np
import pytest
import torch

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


@pytest.fixture(scope="module")
def case():
    dims, params, audio, prompt, plen, y_in, y_out = Q8.decode_case()
    m = _engine(dims, params).eval()
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    T = prompt.shape[1]
    return dict(dims=dims, params=params, model=m, mel=mel, prompt=prompt.to(DEV), plen=plen, kw=dict(eot=EOT, max_len=T + STEPS),
                y_in=y_in, y_out=y_out)


def _same(a, b, what):
    for x, y, name in zip(a, b, ("tokens", "lengths", "sum_logprob")):
        assert torch.equal(x, y), f"{what}: {name} differ"


def _check_images(m, what):
    """Every group that has an int8 image: (Q, scale) bit-equal to the restatement applied to its W.  -> how many there are."""
    n = 0
    for mod, g in D._groups(m.decoder):
        if g.Q is None:
            continue
        n += 1
        assert g.qkey == g.key and g.Q.shape == g.W.shape and g.qscale.shape == (g.W.shape[0],)
        want_q, want_s = Q8.quantize_rows(g.W.float().cpu().numpy())
        assert np.array_equal(g.Q.cpu().numpy(), want_q), (what, type(mod).__name__)
        assert np.array_equal(g.qscale.cpu().numpy().view(np.uint32), want_s.view(np.uint32)), (what, type(mod).__name__)
    return n


def test_int8_capture_changes_nothing_and_sessions_live_apart(case):
    m, args, kw = case["model"], (case["mel"], case["prompt"], case["plen"]), case["kw"]
    D.release_graphs(m)
    g8 = m.greedy_decode(*args, step="graph", weights="int8", **kw)
    key8 = (3, str(DEV), "int8")
    assert list(D.sessions(m)) == [key8]
    s8 = D.sessions(m)[key8]
    assert s8.captures == 1 and s8.replays >= STEPS - 3, (s8.captures, s8.replays)
    _same(g8, m.greedy_decode(*args, step="graph", weights="int8", _capture=False, **kw), "greedy: captured vs launch by launch")
    counts = (s8.captures, s8.replays)
    # a bf16 call in between: its own session, the int8 one neither used nor invalidated
    gb = m.greedy_decode(*args, step="graph", **kw)
    assert set(D.sessions(m)) == {key8, (3, str(DEV))} and (s8.captures, s8.replays) == counts
    sb = D.sessions(m)[(3, str(DEV))]
    assert sb.captures == 1 and sb is not s8
    _same(gb, m.greedy_decode(*args, step="graph", weights="bf16", _capture=False, **kw), "bf16 after int8")
    _same(m.greedy_decode(*args, step="graph", weights="int8", **kw), g8, "int8 again")
    assert s8.captures == 1 and s8.replays > counts[1] and sb.captures == 1, "the second int8 call must replay its own graph"
    assert not all(torch.equal(a, b) for a, b in zip(g8, gb)), "int8 and bf16 decoding agree to the bit: was int8 read at all?"
    # beam search and sampling
    bk = dict(beam_size=3, **kw)
    b8 = m.beam_decode(*args, step="graph", weights="int8", **bk)
    _same(b8, m.beam_decode(*args, step="graph", weights="int8", _capture=False, **bk), "beam: captured vs launch by launch")
    (bs,) = D.beam_sessions(m).values()
    assert list(D.beam_sessions(m))[0][-1] == "int8" and bs.captures == 1 and bs.replays >= 1
    sk = dict(temperature=0.7, best_of=2, seed=11, **kw)
    s1 = m.sample_decode(*args, step="graph", weights="int8", **sk)
    _same(s1, m.sample_decode(*args, step="graph", weights="int8", _capture=False, **sk), "sampling: captured vs launch by launch")
    (ss,) = D.sample_sessions(m).values()
    assert list(D.sample_sessions(m)) == [(3, 2, str(DEV), "int8")] and ss.captures == 1 and ss.replays >= 1
    # the ladder passes the keyword on
    f8 = m.decode_with_fallback(*args, temperatures=(0.0,), step="graph", weights="int8", logprob_threshold=None, no_speech_threshold=None, **kw)
    _same(f8[:3], g8, "decode_with_fallback(weights='int8') at temperature 0")
    D.release_graphs(m)
    assert D.sessions(m) == {} and D.beam_sessions(m) == {} and D.sample_sessions(m) == {}
    with pytest.raises(ValueError, match="int8.*graph"):
        m.greedy_decode(*args, weights="int8", **kw)


def test_images_are_the_quantiser_of_the_shadows_and_follow_an_optimizer_step(case):
    dims = case["dims"]
    m = _engine(dims, case["params"])
    args, kw = (case["mel"], case["prompt"], case["plen"]), case["kw"]
    for mod, g in D._groups(m.decoder):
        assert g.Q is None and g.qscale is None, "an int8 image exists before anyone asked for it"
    m.eval()
    before = m.greedy_decode(*args, step="graph", weights="int8", **kw)
    n = _check_images(m, "fresh model")
    assert n == 6 * dims.n_text_layer + 1, n  # fused q/k/v, self out, cross q, cross out, mlp.0, mlp.2 per layer + the tied embedding
    for blk in m.decoder.blocks:  # the cross key / value projection belongs to the prefill: bf16, never quantised
        assert blk.cross_attn._kv_group.W is not None and blk.cross_attn._kv_group.Q is None
    for mod, g in D._groups(m.encoder):
        assert g.Q is None
    old = {id(g): (g.Q.clone(), g.Q.data_ptr()) for _, g in D._groups(m.decoder) if g.Q is not None}
    # one training step: nothing of it touches the images; the next int8 decode refreshes every one of them, in place
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    loss = m(case["mel"], case["y_in"].to(DEV), targets=case["y_out"].to(DEV), label_smoothing=0.1)
    loss.backward()
    for _, g in D._groups(m.decoder):
        if g.Q is not None:
            assert torch.equal(g.Q, old[id(g)][0])
    opt.step()
    m.eval()
    after = m.greedy_decode(*args, step="graph", weights="int8", **kw)
    assert _check_images(m, "after an optimizer step") == n
    changed = sum(not torch.equal(g.Q, old[id(g)][0]) for _, g in D._groups(m.decoder) if g.Q is not None)
    assert changed == n, f"only {changed} of {n} images were refreshed"
    assert all(g.Q.data_ptr() == old[id(g)][1] for _, g in D._groups(m.decoder) if g.Q is not None), "an image moved: a captured step would go stale"
    _same(after, m.greedy_decode(*args, step="graph", weights="int8", _capture=False, **kw), "after the step: captured vs launch by launch")
    assert before[0].shape[0] == after[0].shape[0] == 3
    D.release_graphs(m)


def test_int8_steps_follow_the_fake_quantised_oracle(case):
    m, dims, params = case["model"], case["dims"], case["params"]
    mel, prompt, plen, kw = case["mel"], case["prompt"], case["plen"], case["kw"]
    V = dims.n_vocab
    fq_params, fq_emb = Q8.fake_quantized_params(params)
    fq, plain = O.Oracle(dims, fq_params), O.Oracle(dims, params)
    tr = DO.Trace()
    rel_fq, rel_plain = [], []
    with torch.no_grad():
        xa = m.encoder(mel)
        xa_ref = plain.encoder(mel.float().cpu())  # (the encoder has no int8 weights: one reference output for both oracles)
        cache = D.KVCache(m.decoder, prompt.shape[0], device=DEV)
        cache.start(prompt, plen, n_vocab=V, **kw)
        for i in range(STEPS):
            with D.stream_gemm(True, weights="int8"):
                logits = D.prefill(m.decoder, cache, xa) if i == 0 else D.step(m.decoder, cache)
            lens, toks = cache.len.cpu(), cache.tokens.cpu()
            got = logits[:, :V].float().cpu()
            ref = Q8.oracle_last_logits(fq, xa_ref, toks, lens, fq_emb)
            ref_plain = Q8.oracle_last_logits(plain, xa_ref, toks, lens)
            per_row = [(DO.rel(got[b], ref[b]), DO.rel(got[b], ref_plain[b])) for b in range(got.shape[0])]
            rel_fq.append(max(a for a, _ in per_row)); rel_plain.append(max(b for _, b in per_row))
            assert all(a < b for a, b in per_row), (i, per_row)
            tr.ref_logits.append(ref)
            tr.active.append(cache.finished.cpu() == 0)
            p, lp = D.pick(m.decoder, cache, logits, want_pick=True)
            tr.picks.append(p.cpu()); tr.logprobs.append(lp.cpu())
    print("int8 steps vs the fp32 oracle over fake-quantised weights, worst row per step:", " ".join(f"{v:.4f}" for v in rel_fq))
    print("int8 steps vs the fp32 oracle over the unquantised weights,  worst row per step:", " ".join(f"{v:.4f}" for v in rel_plain))
    print(f"largest relative L2 error against the fake-quantised oracle: {max(rel_fq):.4f}")
    assert max(rel_fq) < 2e-2, max(rel_fq)  # the bound tests/test_decode_graph_gpu.py holds the bf16 streaming steps to
    DO.check_prefix_following(tr, "2 + 2 layers, B = 3, int8 weights vs the fake-quantised fp32 oracle")
    assert _check_images(m, "after the trace") == 6 * dims.n_text_layer + 1


def test_evaluator_int8_returns_finite_metrics(case):
    from whisper_finetune.data.data_loader import SimpleTokenizer

    m = case["model"]
    D.release_graphs(m)
    y_in, y_out = _text_batch(["the quick brown fox", "jumps over", "the lazy dog"])
    cfg = {"mixed_precision_training": True, "mp_dtype": "bf16", "wft_eval_decode": "greedy", "wft_eval_decode_step": "graph",
           "wft_eval_decode_weights": "int8"}
    calls = []
    real = m.greedy_decode

    def recording(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    m.greedy_decode = recording
    try:
        got = evaluator.evaluate_single_dataset(m, [(case["mel"], y_in, y_out)], "syn", cfg, tokenizer=SimpleTokenizer())
    finally:
        del m.greedy_decode
    assert len(calls) == 1 and calls[0].get("weights") == "int8" and calls[0].get("step") == "graph"
    assert got.num_samples == 3 and np.isfinite(got.wer) and np.isfinite(got.cer) and np.isfinite(got.mean_token_nll)
    assert D.sessions(m) == {}
    with pytest.raises(ValueError, match="wft_eval_decode_weights"):
        evaluator.evaluate_single_dataset(m, [(case["mel"], y_in, y_out)], "syn", dict(cfg, wft_eval_decode_step="eager"), tokenizer=SimpleTokenizer())
