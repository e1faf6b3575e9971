"""Decoding under the timestamp rules end to end on the GPU (greedy_decode / beam_decode with timestamp_begin=, eager and graph
steps, the evaluator's wft_eval_decode_timestamps): whisper-tiny, B = 4, the ragged prompts of tests/test_decode_gpu.py.

A random-init model is near-uniform: 1 500 timestamp columns together always outweigh the best text column, so on its own every
step would sit on one side of the probability rule.  The timestamp rows of the tied embedding therefore carry a fixed bias along
the mean final hidden state of the CPU oracle (BIAS, chosen on the CPU oracle: the logits of the timestamp columns move by about
BIAS, which puts logsumexp(timestamps) on both sides of the best text logit as the live timestamp range shrinks); the test asserts
that both sides occurred.

Greedy: prefix-following as tests/_decode_oracle.py defines it (TAU, FLIP_SHARE, imported), against the fp32 oracle's re-forward
over the engine's own prefix with the rule oracle (tests/_ts_oracle.py) applied to the oracle logits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests import _beam_oracle as BO  # noqa: E402
from tests import _decode_oracle as DO  # noqa: E402
from tests import _ts_oracle as TO  # noqa: E402
from tests._decode_oracle import FLIP_SHARE, TAU  # noqa: E402
from tests.test_beam_decode_gpu import _check_final, _view  # noqa: E402
from tests.test_beam_kernels_gpu import _as_lists  # noqa: E402
from tests.test_decode_gpu import B, EOT, PROMPT_LEN, S, T, _prompts  # noqa: E402
from tests.test_model_gpu import _engine, _tiny_case  # noqa: E402
from whisper_finetune.engine import decode as D  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.eval import evaluator  # noqa: E402

DEV = torch.device("cuda:0")
TSB, NO_TS, MAX_INITIAL = 50364, 50363, 50
SUPPRESS = list(range(EOT + 1, TSB))  # the specials, as the evaluator suppresses them
STEPS = 28
MAX_LEN = T + STEPS
BIAS = -4.5
RULES = dict(timestamp_begin=TSB, no_timestamps=NO_TS, max_initial_timestamp_index=MAX_INITIAL)
ORACLE_KW = dict(ts_begin=TSB, eot=EOT, no_timestamps=NO_TS, max_initial=MAX_INITIAL)
W = 3


def _biased_params(dims, params, audio, y_in):
    """params with BIAS * hbar / |hbar|^2 added to the timestamp rows of the tied embedding, hbar = the oracle's mean final hidden
    state over the teacher-forced rows: a hidden state h then moves every timestamp logit by BIAS * (h . hbar) / |hbar|^2."""
    oracle = O.Oracle(dims, params)
    p = oracle.p
    with torch.no_grad():
        xa = oracle.encoder(O.log_mel_spectrogram(audio, dims.n_mels))
        x = F.embedding(y_in, p["decoder.token_embedding.weight"]) + p["decoder.positional_embedding"][:y_in.shape[1]]
        x = oracle.ra(x.to(xa.dtype))
        for i in range(dims.n_text_layer):
            x = oracle.block(x, f"decoder.blocks.{i}", dims.n_text_head, xa=xa, causal=True)
        hbar = O.layer_norm(x, p["decoder.ln.weight"], p["decoder.ln.bias"]).reshape(-1, x.shape[-1]).float().mean(0)
    out = dict(params)
    emb = params["decoder.token_embedding.weight"].clone()
    emb[TSB:] += BIAS * hbar / hbar.norm() ** 2
    out["decoder.token_embedding.weight"] = emb
    return out


def _follow(m, oracle, mel, prompt, plen, steps, max_len):
    """DO.follow with the timestamp rules switched on -> per step (picks, active, oracle logits on the engine's prefix, the sampled
    tokens of every row before the pick)."""
    V = m.dims.n_vocab
    tr = dict(picks=[], active=[], ref=[], sampled=[], rel=[])
    m.eval()
    with torch.no_grad():
        xa, xa_ref = m.encoder(mel), oracle.encoder(mel.float().cpu())
        cache = D.KVCache(m.decoder, prompt.shape[0], device=mel.device)
        cache.start(prompt, plen, eot=EOT, max_len=max_len, suppress=SUPPRESS, suppress_first=[EOT], n_vocab=V, **RULES)
        for i in range(steps):
            logits = D.prefill(m.decoder, cache, xa) if i == 0 else D.step(m.decoder, cache)
            lens, toks = cache.len.cpu(), cache.tokens.cpu()
            ref = DO.oracle_last_logits(oracle, xa_ref, toks, lens)
            got = logits[:, :V].float().cpu()
            tr["rel"].append(max(DO.rel(got[b], ref[b]) for b in range(got.shape[0])))
            tr["ref"].append(ref)
            tr["active"].append(cache.finished.cpu() == 0)
            tr["sampled"].append([toks[b, int(plen[b]):int(lens[b])].tolist() for b in range(got.shape[0])])
            p, _ = D.pick(m.decoder, cache, logits, want_pick=True)
            tr["picks"].append(p.cpu())
        tr["tokens"], tr["lens"] = cache.tokens.cpu(), cache.len.cpu()
    return tr


@pytest.fixture(scope="module")
def case():
    dims, params, audio, y_in, _ = _tiny_case(B=B, S=S)
    params = _biased_params(dims, params, audio, y_in)
    m = _engine(dims, params).eval()
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    oracle = O.Oracle(dims, params)
    prompt = _prompts(y_in)
    tr = _follow(m, oracle, mel, prompt.to(DEV), PROMPT_LEN, STEPS, MAX_LEN)
    return dict(dims=dims, params=params, model=m, mel=mel, oracle=oracle, prompt=prompt, trace=tr)


def _args(case):
    return case["mel"], case["prompt"].to(DEV), PROMPT_LEN


def _kw(**over):
    kw = dict(eot=EOT, max_len=MAX_LEN, suppress=SUPPRESS, suppress_first=[EOT], **RULES)
    kw.update(over)
    return kw


def _sampled(tokens, lengths, b):
    return tokens[b, int(PROMPT_LEN[b]):int(lengths[b])].tolist()


def _same(a, b, what=""):
    for x, y, name in zip(a[:3], b[:3], ("tokens", "lengths", "sum_logprob")):
        assert torch.equal(x, y), f"{what}: {name} differ"
    if len(a) > 3:
        assert a[3] == b[3], f"{what}: the ranked lists differ"


def test_greedy_follows_the_rule_oracle_on_the_engines_prefix(case):
    tr = case["trace"]
    print("cached logits vs the fp32 oracle, worst row per step:", " ".join(f"{v:.4f}" for v in tr["rel"]))
    assert max(tr["rel"]) < 2e-2
    n = flips = near = wins = losses = 0
    worst = 0.0
    for p, ref, act, samp in zip(tr["picks"], tr["ref"], tr["active"], tr["sampled"]):
        for b in range(p.shape[0]):
            if not bool(act[b]):
                continue
            n += 1
            r = TO.rules(ref[b], samp[b], dead=SUPPRESS + ([EOT] if not samp[b] else []), **ORACLE_KW)
            contested = r.margin == r.margin and abs(r.margin) != float("inf")
            wins += contested and r.ts_wins
            losses += contested and not r.ts_wins
            got = int(p[b])
            if got == int(r.x.argmax()):
                continue
            flips += 1
            if contested and abs(r.margin) < 1e-2:  # the oracle's own rule 5 sits on its threshold: either side is a correct step
                near += 1
                continue
            assert torch.isfinite(r.x[got]), (b, got, "the engine picked a column the rules remove")
            worst = max(worst, float(r.x.max() - r.x[got]))
    share = flips / max(n, 1)
    print(f"{flips} of {n} picks are not the rule oracle's (share {share:.4f}, cap {FLIP_SHARE}; {near} of them within 1e-2 of rule 5's "
          f"threshold); largest shortfall {worst:.3e} (tau {TAU}); rule 5 contested {wins + losses} times, the timestamps won {wins}")
    assert n > 0 and worst <= TAU and share <= FLIP_SHARE
    assert wins >= 3 and losses >= 3, "both sides of the probability rule must occur within the decoded length"


def test_greedy_decode_equals_its_pieces_and_keeps_the_structure(case):
    tr, m = case["trace"], case["model"]
    tokens, lengths, slp = m.greedy_decode(*_args(case), **_kw())
    tokens, lengths = tokens.cpu(), lengths.cpu()
    n_ts = 0
    for b in range(B):
        n = min(int(PROMPT_LEN[b]) + STEPS, int(lengths[b]))
        assert torch.equal(tokens[b, :n], tr["tokens"][b, :n]), b
        s = _sampled(tokens, lengths, b)
        assert TO.check_structure(s, ts_begin=TSB, eot=EOT, max_initial=MAX_INITIAL) is None, (b, s)
        assert not set(s) & (set(SUPPRESS) | {NO_TS})
        n_ts += sum(t >= TSB for t in s)
    assert n_ts >= 3 * B  # every row closed at least one segment and opened the next
    segs = D.timestamp_segments(tokens, PROMPT_LEN, lengths, TSB, EOT)
    for b in range(B):
        assert segs[b] and segs[b][0][0] is not None and segs[b][0][0] <= MAX_INITIAL * 0.02 + 1e-9
        assert all(e is None or e >= st for st, e, _ in segs[b]) and all(e is not None for _, e, _ in segs[b][:-1])
        text = [t for t in _sampled(tokens, lengths, b) if t < TSB and t != EOT]
        assert [t for _, _, ids in segs[b] for t in ids] == text  # every text token lands in exactly one segment, in order


def test_beam_search_follows_the_oracle_on_the_engines_candidates(case):
    """The replay of tests/test_beam_decode_gpu.py's drive() with the rules on: after every step the device state equals the plain
    Python beam search fed the engine's candidate lists; the candidate lists themselves equal the rule oracle on the bf16 logits
    the kernel read, every hypothesis under ITS OWN history (the rows of `tokens` move with the beams)."""
    m, V = case["model"], case["dims"].n_vocab
    steps, max_len = 10, T + 10
    prompt = case["prompt"].to(DEV).clone()
    with torch.no_grad():
        xa = m.encoder(case["mel"])
        cache = D.BeamCache(m.decoder, B, W, W, device=DEV)
        cache.start(prompt, PROMPT_LEN, eot=EOT, max_len=max_len, suppress=SUPPRESS, suppress_first=[EOT], n_vocab=V, **RULES)
        st = BO.State([prompt[a, :int(PROMPT_LEN[a])].tolist() for a in range(B)], W, W, EOT, max_len)
        checked = skipped = 0
        for i in range(steps):
            first = i == 0
            logits = D.beam_prefill(m.decoder, cache, xa) if first else D.beam_step(m.decoder, cache)
            toks, lens, fl = cache.tokens.cpu(), cache.len.cpu(), cache.first_len.cpu()
            D.beam_topk(m.decoder, cache, logits, first=first)
            ct, cl = cache.cand_tok.cpu(), cache.cand_logp.cpu()
            lg = logits[:, :V].float().cpu()
            for k in range(lg.shape[0]):
                r = k * W if first else k
                if st.audios[r // W].done:
                    continue
                samp = toks[r, int(fl[r]):int(lens[r])].tolist()
                ru = TO.rules(lg[k], samp, dead=SUPPRESS + ([EOT] if not samp else []), **ORACLE_KW)
                if ru.margin == ru.margin and abs(ru.margin) < 1e-2:
                    skipped += 1
                    continue
                want = TO.topk_of(ru, W + 1)
                assert ct[r].tolist() == [c for c, _ in want], (i, r, ct[r].tolist(), want)
                assert max(abs(float(cl[r, j]) - w) for j, (c, w) in enumerate(want) if c >= 0) < 1e-4
                checked += 1
            D.beam_update(cache, first=first)
            BO.step_candidates(st, _as_lists(ct.numpy(), cl.numpy(), B, W))
            _view(cache).check(st, f"step {i}")
    print(f"{checked} candidate rows equal the rule oracle, {skipped} within 1e-2 of rule 5's threshold left out")
    assert checked >= B + (steps - 2) * B * W and skipped <= 0.1 * (checked + skipped)
    _check_final(cache, st)
    out = m.beam_decode(*_args(case), beam_size=W, return_all=True, **_kw(max_len=max_len))
    entries, win = BO.finalize(st)[B - 1]  # the longest prompt ran exactly these steps
    assert out[0][B - 1, :int(out[1][B - 1])].tolist() == entries[win][0]
    for b in range(B):
        for hyp, _, _ in out[3][b]:
            s = hyp[int(PROMPT_LEN[b]):]
            assert TO.check_structure(s, ts_begin=TSB, eot=EOT, max_initial=MAX_INITIAL) is None, (b, s)
    assert len({tuple(h) for h, _, _ in out[3][0]}) == W


def test_graph_steps_change_nothing_and_other_rules_recapture(case):
    m = case["model"]
    D.release_graphs(m)
    kw = _kw()
    eager = m.greedy_decode(*_args(case), **kw)
    _same(m.greedy_decode(*_args(case), step="graph", _stream_gemm=False, **kw), eager, "graph on the eager step's GEMMs")
    g = m.greedy_decode(*_args(case), step="graph", **kw)
    _same(g, m.greedy_decode(*_args(case), step="graph", _capture=False, **kw), "graph vs eager steps on the streaming GEMMs")
    (sess,) = D.sessions(m).values()
    caps = sess.captures
    _same(m.greedy_decode(*_args(case), step="graph", **kw), g, "second call")
    assert sess.captures == caps, "the same rules must replay"
    # other rule constants: the captured pick holds them by value, so the step is captured again — and computes what eager computes
    for other in (dict(max_initial_timestamp_index=3), dict(timestamp_begin=None)):
        kw2 = _kw(**other)
        g2 = m.greedy_decode(*_args(case), step="graph", **kw2)
        caps += 1
        assert sess.captures == caps, (other, sess.captures)
        _same(g2, m.greedy_decode(*_args(case), step="graph", _capture=False, **kw2), f"recaptured under {other}")
        assert not torch.equal(g2[0], g[0])
    first = int(m.greedy_decode(*_args(case), step="graph", **_kw(max_initial_timestamp_index=3))[0][0, int(PROMPT_LEN[0])])
    assert TSB <= first <= TSB + 3
    bk = dict(beam_size=W, return_all=True)
    be = m.beam_decode(*_args(case), **bk, **kw)
    _same(m.beam_decode(*_args(case), step="graph", _stream_gemm=False, **bk, **kw), be, "beam: graph on the eager step's GEMMs")
    bg = m.beam_decode(*_args(case), step="graph", **bk, **kw)
    _same(bg, m.beam_decode(*_args(case), step="graph", _capture=False, **bk, **kw), "beam: graph vs eager steps on the streaming GEMMs")
    (bsess,) = D.beam_sessions(m).values()
    bc = bsess.captures
    m.beam_decode(*_args(case), step="graph", **bk, **_kw(no_timestamps=None))
    assert bsess.captures == bc + 1
    D.release_graphs(m)


def test_full_context_run_keeps_the_structure(case):
    """448 tokens: the in-kernel scan of the sampled tokens at full length, eager against the captured step."""
    m = case["model"]
    n_ctx = case["dims"].n_text_ctx
    args = (case["mel"][:2], case["prompt"][:2].to(DEV), PROMPT_LEN[:2])
    kw = _kw(max_len=n_ctx, suppress=SUPPRESS + [EOT])  # (eot suppressed: no row ends before the cache does)
    tokens, lengths, slp = m.greedy_decode(*args, step="graph", **kw)
    _same(m.greedy_decode(*args, step="graph", _capture=False, **kw), (tokens, lengths, slp), "448 tokens, graph vs eager steps")
    D.release_graphs(m)
    tokens, lengths = tokens.cpu(), lengths.cpu()
    print("lengths", lengths.tolist(), "timestamps per row", [(tokens[b, :int(lengths[b])] >= TSB).sum().item() for b in range(2)])
    assert lengths.tolist() == [n_ctx, n_ctx]
    for b in range(2):
        s = _sampled(tokens, lengths, b)
        assert TO.check_structure(s, ts_begin=TSB, eot=EOT, max_initial=MAX_INITIAL) is None, b
        print(f"row {b}: timestamps at sampled positions", [i for i, t in enumerate(s) if t >= TSB])


def test_evaluator_with_timestamps_returns_text_free_of_timestamp_ids(case):
    from tests.test_decode_graph_gpu import _text_batch
    from whisper_finetune.data.data_loader import SimpleTokenizer

    m = case["model"]
    seen, calls = [], []

    class Tok(SimpleTokenizer):
        def decode(self, ids):
            seen.append(list(ids))
            return super().decode(ids)

    tok = Tok()
    y_in, y_out = _text_batch(["the quick brown fox", "jumps over", "the lazy dog and runs", "far away"])
    real = m.greedy_decode

    def recording(*a, **kw):
        out = real(*a, **kw)
        calls.append((a, kw, out))
        return out

    m.greedy_decode = recording
    try:
        cfg = {"mixed_precision_training": True, "mp_dtype": "bf16", "wft_eval_decode": "greedy", "wft_eval_decode_timestamps": True}
        got = evaluator.evaluate_single_dataset(m, [(case["mel"], y_in, y_out)], "syn", cfg, tokenizer=tok)
    finally:
        del m.greedy_decode
    ((a, kw, out),) = calls
    assert kw["timestamp_begin"] == tok.timestamp_begin == TSB and kw["no_timestamps"] == NO_TS and max(kw["suppress"]) < TSB
    assert a[2].tolist() == [3, 3, 3, 3] and not (a[1] == NO_TS).any()  # the prefix stops behind the task token
    assert int((out[0] >= TSB).sum()) >= 4, "the decode produced no timestamps: the test shows nothing"
    assert got.num_samples == 4 and seen and all(t < EOT for ids in seen for t in ids)
