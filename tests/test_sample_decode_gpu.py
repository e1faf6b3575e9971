"""Sampled decoding end to end on the GPU (engine/decode/ sample_decode, SampleCache, no_speech_prob, decode_with_fallback and the
evaluator's `fallback` mode): whisper-tiny, the case of tests/test_beam_decode_gpu.py (B = 4 audios, ragged prompts of 4 + 2b
tokens), N = 5 samples per audio (20 rows per cached step), 10 steps.

 (a) logits — at every step every live row's cached logits on that row's OWN token prefix against the engine's teacher-forced
     logits, relative L2 < 2e-2 (the bound of tests/test_beam_decode_gpu.py): the check of the static ancestry table, the per-audio
     prefill and the grouped cross form.
 (b) replay — every step's engine logits through tests/_sample_oracle.py with the documented seeds: picks, lengths and finished
     flags exact apart from rows whose fp64 top-two key gap is under 1e-3 (at most 2 % of the draws; a row that left the oracle's
     path is followed on its own tokens from there on), sum_logprob within 1e-3 relative.
 (c)-(i): N = 1 at temperature 0 against greedy_decode, graph against eager steps, seeds, ranking, the no-speech probability, the
     ladder, the evaluator."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests import _decode_oracle as DO  # noqa: E402
from tests import _sample_oracle as SO  # noqa: E402
from tests.test_decode_gpu import B, EOT, PROMPT_LEN, S, T, _prompts  # noqa: E402
from tests.test_model_gpu import _engine, _tiny_case  # noqa: E402
from whisper_finetune.engine import decode as D  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402

DEV = torch.device("cuda:0")
N = 5
STEPS = 10
MAX_LEN = T + STEPS
TEMP = 0.8
SEED = 31
GAP = 1e-3


def drive(m, mel, prompt, plen, steps, *, temperature, seeds, eot, max_len, best_of=N):
    """`steps` sampling steps from the pieces sample_decode is made of.  Per step: (a) the logits of every live row against the
    teacher-forced engine on that row's own prefix, worst row; (b) the oracle's pick from the same logits for every live row."""
    V, nB = m.dims.n_vocab, prompt.shape[0]
    R = nB * best_of
    rec = dict(rel_teacher=[], rows=0, draws=0, under=0, lp_err=0.0)
    m.eval()
    with torch.no_grad():
        xa = m.encoder(mel)
        cache = D.SampleCache(m.decoder, nB, best_of, device=mel.device)
        cache.start(prompt, plen, temperature=temperature, seeds=seeds, eot=eot, max_len=max_len, n_vocab=V)
        # the static ancestry table: the prompt positions of a row live in its audio's slot a*N, everything behind in its own
        anc = cache.anc.cpu()
        for r in range(R):
            p = int(plen[r // best_of])
            assert (anc[r, :p] == (r // best_of) * best_of).all() and (anc[r, p:] == r).all()
        assert cache.len.cpu().tolist() == [int(plen[r // best_of]) for r in range(R)] and int(cache.unfinished) == R
        slp = np.zeros(R)
        for i in range(steps):
            first = i == 0
            logits = D.beam_prefill(m.decoder, cache, xa) if first else D.step(m.decoder, cache)
            assert logits.shape[0] == (nB if first else R)
            toks, lens, fin = cache.tokens.cpu(), cache.len.cpu(), cache.finished.cpu()
            live = [r for r in range(R) if not int(fin[r])]
            got = logits[:, :V].float().cpu()
            if live:
                sel = torch.tensor(live)
                Lm = int(lens[sel].max())
                tf = m.decoder(toks[sel, :Lm].to(mel.device), xa[(sel // best_of).to(mel.device)])[torch.arange(len(live)), lens[sel].long() - 1].cpu()
                rec["rel_teacher"].append(max(DO.rel(got[r // best_of if first else r], tf[k]) for k, r in enumerate(live)))
                rec["rows"] += len(live)
            pick, lp = D.sample_pick(m.decoder, cache, logits, want_pick=True)
            pick, lp = pick.cpu(), lp.cpu()
            new_len, new_fin, new_tok = cache.len.cpu(), cache.finished.cpu(), cache.tokens.cpu()
            for r in live:
                w = SO.pick(got[r // best_of if first else r].double().numpy(), temperature, seeds[r], int(lens[r]), eot)
                rec["draws"] += 1
                if w.gap < GAP:
                    rec["under"] += 1  # (left out of the exact comparison; the row goes on from the engine's own token)
                    slp[r] += lp[r].item()
                else:
                    assert int(pick[r]) == w.col, (i, r, int(pick[r]), w)
                    rec["lp_err"] = max(rec["lp_err"], abs(lp[r].item() - w.logp))
                    slp[r] += w.logp
                # the state follows the pick
                assert int(new_len[r]) == int(lens[r]) + 1 and int(new_tok[r, int(lens[r])]) == int(pick[r])
                assert int(new_fin[r]) == int(int(pick[r]) == eot or int(lens[r]) + 1 >= max_len)
            for r in range(R):
                if r not in live:
                    assert int(new_len[r]) == int(lens[r]) and int(new_fin[r]) == 1
            assert int(cache.unfinished) == R - int(new_fin.sum())
    rec["slp"] = slp
    return cache, rec


@pytest.fixture(scope="module")
def case():
    dims, params, audio, y_in, y_out = _tiny_case(B=B, S=S)
    m = _engine(dims, params).eval()
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    prompt = _prompts(y_in)
    seeds = D.sample_seeds(SEED, B, N)
    cache, rec = drive(m, mel, prompt.to(DEV), PROMPT_LEN, STEPS, temperature=TEMP, seeds=seeds, eot=EOT, max_len=MAX_LEN)
    return dict(dims=dims, model=m, mel=mel, prompt=prompt, cache=cache, rec=rec, seeds=seeds)


def _args(case):
    return case["mel"], case["prompt"].to(DEV), PROMPT_LEN


def _same(a, b, what=""):
    for x, y, name in zip(a[:3], b[:3], ("tokens", "lengths", "sum_logprob")):
        assert torch.equal(x, y), f"{what}: {name} differ"
    if len(a) > 3 and len(b) > 3:
        assert a[3] == b[3], f"{what}: the ranked lists differ"


def test_a_cached_logits_of_every_sample_on_its_own_prefix(case):
    rec = case["rec"]
    print(f"{rec['rows']} rows compared.  cached vs teacher-forced, worst row per step:", " ".join(f"{v:.4f}" for v in rec["rel_teacher"]))
    assert len(rec["rel_teacher"]) == STEPS and rec["rows"] >= B * N + (STEPS - 4) * B * N // 2
    assert max(rec["rel_teacher"]) < 2e-2, max(rec["rel_teacher"])
    # the samples of an audio did part ways: the rows of some audio hold different tokens (their own keys were exercised)
    tok, first = case["cache"].tokens.cpu(), case["cache"].first_len.cpu()
    assert any(len({tuple(tok[a * N + j, int(first[a * N]):int(first[a * N]) + 3].tolist()) for j in range(N)}) > 1 for a in range(B))


def test_b_replay_through_the_oracle_and_sample_decode_equals_its_pieces(case):
    m, rec, cache = case["model"], case["rec"], case["cache"]
    print(f"{rec['draws']} draws replayed, {rec['under']} under the key gap {GAP} (cap {int(0.02 * rec['draws'])}); "
          f"log-probability max |err| vs fp64 {rec['lp_err']:.3e}")
    assert rec["draws"] >= B * N * (STEPS - 4) and rec["under"] <= 0.02 * rec["draws"]
    assert rec["lp_err"] < 1e-4
    got = cache.sum_logprob.cpu().double().numpy()
    assert (np.abs(got - rec["slp"]) <= 1e-3 * np.maximum(np.abs(rec["slp"]), 1.0)).all(), np.abs(got - rec["slp"]).max()
    # sample_decode as a whole: the audio with the longest prompt has run exactly the STEPS steps of drive()
    tokens, lengths, slp, ranked = m.sample_decode(*_args(case), temperature=TEMP, best_of=N, seed=SEED, eot=EOT, max_len=MAX_LEN, return_all=True)
    assert tokens.dtype == torch.int64 and tokens.shape == (B, int(lengths.max())) and slp.dtype == torch.float32 and m.training is False
    a = B - 1
    ctok, clen, cslp = cache.tokens.cpu(), cache.len.cpu().tolist(), cache.sum_logprob.cpu().tolist()
    rows = {tuple(ctok[r, :clen[r]].tolist()): cslp[r] for r in range(a * N, (a + 1) * N)}
    assert {tuple(t) for t, _, _ in ranked[a]} == set(rows) and all(rows[tuple(t)] == s for t, s, _ in ranked[a])
    for b in range(B):
        assert torch.equal(tokens[b, :PROMPT_LEN[b]].cpu(), case["prompt"][b, :PROMPT_LEN[b]]) and (tokens[b, int(lengths[b]):] == EOT).all()
        assert len(ranked[b]) == N and ranked[b][0][0] == tokens[b, :int(lengths[b])].tolist()
    with pytest.raises(ValueError):
        m.sample_decode(*_args(case), temperature=TEMP, eot=EOT, max_len=T - 1)  # _Cache._start's checks hold


def test_c_one_sample_at_temperature_zero_is_greedy_decoding(case):
    """The SampleCache path itself (not sample_decode's shortcut to greedy_decode) with N = 1 and a zero temperature tensor."""
    m = case["model"]
    V = m.dims.n_vocab
    g = m.greedy_decode(*_args(case), eot=EOT, max_len=MAX_LEN)
    with torch.no_grad():
        cache = D.SampleCache(m.decoder, B, 1, device=DEV)
        cache.start(case["prompt"].to(DEV), PROMPT_LEN, temperature=0.0, seeds=[5] * B, eot=EOT, max_len=MAX_LEN, n_vocab=V)
        D.sample_pick(m.decoder, cache, D.beam_prefill(m.decoder, cache, m.encoder(case["mel"])))
        for _ in range(MAX_LEN - int(PROMPT_LEN.min()) - 1):
            D._sample_body(m.decoder, cache)
    lens = cache.len.long()
    assert torch.equal(lens, g[1])
    for b in range(B):
        assert torch.equal(cache.tokens[b, :int(lens[b])], g[0][b, :int(lens[b])]), b
    err = (g[2] - cache.sum_logprob).abs().cpu()
    assert (err <= 1e-3 * g[2].abs().cpu().clamp(min=1.0)).all(), err
    # and the public shortcut: temperature 0 returns greedy_decode's result, whatever best_of says
    _same(m.sample_decode(*_args(case), temperature=0, best_of=3, eot=EOT, max_len=MAX_LEN), g, "temperature 0")
    full = m.sample_decode(*_args(case), temperature=0.0, eot=EOT, max_len=MAX_LEN, return_all=True)
    assert [len(e) for e in full[3]] == [1] * B and full[3][0][0][0] == g[0][0, :int(g[1][0])].tolist()


def test_d_graph_steps_change_nothing_and_replay_other_temperatures_and_seeds(case):
    m = case["model"]
    D.release_graphs(m)
    kw = dict(best_of=N, eot=EOT, max_len=MAX_LEN, return_all=True)
    eager = m.sample_decode(*_args(case), temperature=TEMP, seed=SEED, **kw)
    graph = m.sample_decode(*_args(case), temperature=TEMP, seed=SEED, step="graph", **kw)
    _same(graph, m.sample_decode(*_args(case), temperature=TEMP, seed=SEED, step="graph", _capture=False, **kw), "graph vs eager steps on the streaming GEMMs")
    _same(m.sample_decode(*_args(case), temperature=TEMP, seed=SEED, step="graph", _stream_gemm=False, **kw), eager, "graph on the eager step's GEMMs")
    D.release_graphs(m)
    first = m.sample_decode(*_args(case), temperature=TEMP, seed=SEED, step="graph", **kw)
    _same(first, graph, "after release_graphs")
    (sess,) = D.sample_sessions(m).values()
    assert list(D.sample_sessions(m)) == [(B, N, str(DEV))] and sess.captures == 1 and sess.replays >= STEPS - 3
    # another temperature and other seeds are memory: the same session replays, nothing is captured again
    r0 = sess.replays
    other = m.sample_decode(*_args(case), temperature=0.3, seed=[7, 8, 9, 10], step="graph", **kw)
    assert sess.captures == 1 and sess.replays >= r0 + STEPS - 1, (sess.captures, sess.replays)
    _same(other, m.sample_decode(*_args(case), temperature=0.3, seed=[7, 8, 9, 10], step="graph", _capture=False, **kw), "second call vs its eager twin")
    assert not torch.equal(other[0], first[0])
    # greedy and beam sessions live in their own tables; release_graphs empties all three
    m.greedy_decode(*_args(case), eot=EOT, max_len=MAX_LEN, step="graph")
    m.beam_decode(*_args(case), beam_size=2, eot=EOT, max_len=MAX_LEN, step="graph")
    assert len(D.sessions(m)) == 1 and len(D.beam_sessions(m)) == 1 and len(D.sample_sessions(m)) == 1
    D.release_graphs(m)
    assert D.sessions(m) == {} and D.beam_sessions(m) == {} and D.sample_sessions(m) == {}


def test_e_seeds(case):
    m = case["model"]
    kw = dict(temperature=TEMP, best_of=N, eot=EOT, max_len=MAX_LEN, return_all=True)
    one = m.sample_decode(*_args(case), seed=SEED, **kw)
    _same(one, m.sample_decode(*_args(case), seed=SEED, **kw), "the same seed")
    _same(one, m.sample_decode(*_args(case), seed=[SEED + a for a in range(B)], **kw), "an int seed is seed + a per audio")
    other = m.sample_decode(*_args(case), seed=SEED + 1000, **kw)
    assert any(one[3][a] != other[3][a] for a in range(B)), "another seed changed nothing"


def test_f_ranking(case):
    m = case["model"]
    for lp in (None, 0.6, 1.0):
        tokens, lengths, slp, ranked = m.sample_decode(*_args(case), temperature=TEMP, best_of=N, seed=SEED, length_penalty=lp, eot=EOT,
                                                       max_len=MAX_LEN, return_all=True)
        cache = case["cache"]
        ctok, clen, cfirst, cslp = cache.tokens.cpu(), cache.len.cpu().tolist(), cache.first_len.cpu().tolist(), cache.sum_logprob.cpu().tolist()
        for a in range(B):
            assert all(ranked[a][i][2] >= ranked[a][i + 1][2] for i in range(N - 1))
            assert tokens[a, :int(lengths[a])].tolist() == ranked[a][0][0] and slp[a].item() == np.float32(ranked[a][0][1])
            for t, s, score in ranked[a]:
                n = len(t) - int(PROMPT_LEN[a]) - (1 if t[-1] == EOT and len(t) > int(PROMPT_LEN[a]) else 0)
                assert score == D.beam_score(n, s, lp)
        # the audio with the longest prompt ran drive()'s steps: the winner is beam_rank of its rows in sample order
        a = B - 1
        rows = range(a * N, (a + 1) * N)
        entries = [(clen[r] - cfirst[r] - (1 if int(ctok[r, clen[r] - 1]) == EOT else 0), cslp[r]) for r in rows]
        win = a * N + D.beam_rank(entries, lp)
        assert tokens[a, :int(lengths[a])].tolist() == ctok[win, :clen[win]].tolist()


def test_g_no_speech_prob(case):
    m = case["model"]
    V = m.dims.n_vocab
    no_speech = 50362
    with torch.no_grad():
        xa = m.encoder(case["mel"])
        prompt = case["prompt"].to(DEV)
        for sot_index in (0, [0, 1, 2, 3]):
            got = D.no_speech_prob(m, xa, prompt, sot_index, no_speech).cpu()
            idx = [sot_index] * B if isinstance(sot_index, int) else sot_index
            logits = m.decoder(prompt, xa)[torch.arange(B), torch.tensor(idx)].float().cpu()  # the engine's own logits rows (bf16 values)
            want = torch.softmax(logits, -1)[:, no_speech]
            print(f"sot_index={sot_index}: no_speech_prob {got.tolist()} vs fp32 softmax, max |err| {(got - want).abs().max().item():.3e}")
            assert got.dtype == torch.float32 and (got - want).abs().max().item() < 1e-4
    with pytest.raises(ValueError):
        D.no_speech_prob(m, xa, prompt, T, no_speech)
    with pytest.raises(ValueError):
        D.no_speech_prob(m, xa, prompt, 0, V)


def test_h_decode_with_fallback(case):
    m = case["model"]
    kw = dict(eot=EOT, max_len=MAX_LEN)
    inf = float("inf")
    g = m.greedy_decode(*_args(case), **kw)
    out = m.decode_with_fallback(*_args(case), logprob_threshold=-inf, no_speech=50362, sot_index=0, **kw)
    _same(out, g, "threshold -inf: the rung at 0")
    info = out[3]
    assert info["rungs"] == [[0, 1, 2, 3]] and info["temperature"] == [0.0] * B and all(0 <= p <= 1 for p in info["no_speech_prob"])
    gl, gs = g[1].cpu().tolist(), g[2].cpu().tolist()
    n = [gl[a] - int(PROMPT_LEN[a]) - (1 if int(g[0][a, gl[a] - 1]) == EOT else 0) for a in range(B)]
    assert info["avg_logprob"] == pytest.approx([gs[a] / (n[a] + 1) for a in range(B)])
    bm = m.beam_decode(*_args(case), beam_size=3, **kw)
    _same(m.decode_with_fallback(*_args(case), beam_size=3, logprob_threshold=-inf, **kw), bm, "threshold -inf with beam_size")
    # +inf walks every rung; the last one's sample_decode result stands, drawn with that rung's seeds
    temps = (0.0, 0.4, 0.9)
    out = m.decode_with_fallback(*_args(case), temperatures=temps, best_of=3, seed=11, logprob_threshold=inf, **kw)
    want = m.sample_decode(*_args(case), temperature=0.9, best_of=3, seed=[11 + 2 * B + a for a in range(B)], **kw)
    _same(out, want, "threshold +inf: the last rung")
    assert out[3]["rungs"] == [[0, 1, 2, 3]] * 3 and out[3]["temperature"] == [0.9] * B
    # a threshold at the median of the rung-0 averages: a strict subset is decoded again
    avg = info["avg_logprob"]
    thr = float(np.median(avg))
    retried = [a for a in range(B) if avg[a] < thr]
    assert 0 < len(retried) < B
    out = m.decode_with_fallback(*_args(case), temperatures=(0.0, 0.5), best_of=N, seed=3, logprob_threshold=thr, **kw)
    assert out[3]["rungs"] == [[0, 1, 2, 3], retried]
    sel = torch.tensor(retried)
    with torch.no_grad():  # (the ladder's encoder ran once, on the whole batch: the twin gets those rows, not an encoder pass at another batch size)
        xa = m.encoder(case["mel"])[sel.to(DEV)]
    sub = D.sample_decode(m, case["mel"][sel.to(DEV)], case["prompt"][sel].to(DEV), PROMPT_LEN[sel], temperature=0.5, best_of=N,
                          seed=[3 + B + a for a in retried], _xa=xa, **kw)
    for a in range(B):
        if a in retried:
            j = retried.index(a)
            L = int(sub[1][j])
            assert int(out[1][a]) == L and torch.equal(out[0][a, :L], sub[0][j, :L]) and out[2][a].item() == sub[2][j].item()
            assert out[3]["temperature"][a] == 0.5
        else:
            L = gl[a]
            assert int(out[1][a]) == L and torch.equal(out[0][a, :L], g[0][a, :L]) and out[2][a].item() == gs[a] and out[3]["temperature"][a] == 0.0
        assert (out[0][a, int(out[1][a]):] == EOT).all()


def test_i_evaluator_fallback_mode(case):
    from tests.test_decode_graph_gpu import _text_batch
    from whisper_finetune.data.data_loader import SimpleTokenizer
    from whisper_finetune.eval import evaluator

    m = case["model"]
    y_in, y_out = _text_batch(["the quick brown fox", "jumps over", "the lazy dog and runs", "far away"])
    calls = []
    real = m.decode_with_fallback

    def recording(*a, **kw):
        out = real(*a, **kw)
        calls.append((kw, out))
        return out

    m.decode_with_fallback = recording
    try:
        cfg = {"mixed_precision_training": True, "mp_dtype": "bf16", "wft_eval_decode": "fallback", "wft_eval_decode_temperatures": [0.0, 0.5],
               "wft_eval_decode_best_of": 2}
        got = evaluator.evaluate_single_dataset(m, [(case["mel"], y_in, y_out)], "syn", cfg, tokenizer=SimpleTokenizer())
    finally:
        del m.decode_with_fallback
    ((kw, out),) = calls
    assert kw["temperatures"] == (0.0, 0.5) and kw["best_of"] == 2 and kw["compression_ratio_threshold"] == 2.4 and kw["no_speech"] == 50362
    assert kw["sot_index"] == [0, 0, 0, 0] and len(out[3]["rungs"]) == 2  # a random-init model is far below -1.0 per token: the ladder was walked
    assert got.num_samples == 4 and np.isfinite(got.wer) and np.isfinite(got.cer)
