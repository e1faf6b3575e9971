"""Beam-search decoding end to end on the GPU (engine/decode/beam.py beam_decode, BeamCache): whisper-tiny, B = 4 audios with ragged
prompts of 4 + 2b tokens, W = 5 beams (20 rows per cached step).

What is checked and against what:
 (a) logits — at every step every live row's cached logits on that row's OWN token prefix, against the engine's teacher-forced
     logits and against the fp32 CPU oracle, relative L2 < 2e-2 each (the bound of tests/test_decode_gpu.py).  This is the
     end-to-end check of the ancestry table, the per-audio prefill and the grouped cross form.  (A free-running token comparison
     against an fp32 model means nothing on a random-init model: tests/_decode_oracle.py.)
 (b) replay — the same run replayed through tests/_beam_oracle.py fed the engine's own candidate lists of each step: beams, sources,
     scores, finished lists, done flags and the final ranked result, exact.
 (c)-(f): a small live vocabulary, W = 1 against greedy_decode, step="graph" against step="eager", reruns and LoRA."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests import _beam_oracle as BO  # noqa: E402
from tests import _decode_oracle as DO  # noqa: E402
from tests.test_beam_kernels_gpu import _DevState, _as_lists  # noqa: E402
from tests.test_decode_gpu import B, EOT, PROMPT_LEN, S, T, _prompts  # noqa: E402
from tests.test_model_gpu import _engine, _tiny_case  # noqa: E402
from whisper_finetune.engine import decode as D  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine.whisper_model import MODEL_DIMS, Whisper  # noqa: E402
from whisper_finetune.model import lora as lora_mod  # noqa: E402

DEV = torch.device("cuda:0")
W = 5
STEPS = 10
MAX_LEN = T + STEPS


def _view(cache):
    """The cache's state under the names tests/test_beam_kernels_gpu.py's checker reads."""
    dv = object.__new__(_DevState)
    dv.B, dv.W, dv.C, dv.eot, dv.max_len, dv.n_ctx = cache.audios, cache.beam, cache.cands, cache.eot, cache.max_len, cache.n_ctx
    dv.tokens, dv.len, dv.anc, dv.slp, dv.done, dv.unfinished = cache.tokens, cache.len, cache.anc, cache.sum_logprob, cache.done, cache.unfinished
    dv.fin_tokens, dv.fin_len, dv.fin_score, dv.fin_n, dv.src = cache.fin_tokens, cache.fin_len, cache.fin_score, cache.fin_n, cache.src
    return dv


def drive(m, oracle, mel, prompt, plen, steps, *, beam, cands, eot, max_len, suppress=(), suppress_first=(), compare_teacher=True,
          check_steps=None):
    """`steps` beam-search steps from the pieces beam_decode is made of.  Per step: (a) the logits of every live row against the
    teacher-forced engine and the fp32 oracle on that row's own prefix, worst row; (b) the oracle replay on the engine's candidates.
    check_steps(i, lens of the live rows) -> bool restricts (a) to chosen steps (None: every step; rec["checked"] lists them); (b)
    runs after every step regardless."""
    V, nB = m.dims.n_vocab, prompt.shape[0]
    rec = dict(rel_teacher=[], rel_oracle=[], done_at={}, first_cands=None, rows=0, checked=[])
    m.eval()
    with torch.no_grad():
        xa = m.encoder(mel)
        xa_ref = oracle.encoder(mel.float().cpu()) if oracle is not None else None
        cache = D.BeamCache(m.decoder, nB, beam, cands, device=mel.device)
        prompt = prompt.clone()  # (the checker expects `eot` behind every row's end, the prompt block's padding included)
        prompt[torch.arange(prompt.shape[1], device=prompt.device)[None, :] >= torch.as_tensor(plen, device=prompt.device)[:, None]] = eot
        cache.start(prompt, plen, eot=eot, max_len=max_len, suppress=suppress, suppress_first=suppress_first, n_vocab=V)
        st = BO.State([prompt[a, :int(plen[a])].tolist() for a in range(nB)], beam, cands, eot, max_len)
        _view(cache).check(st, "after start")
        for i in range(steps):
            first = i == 0
            logits = D.beam_prefill(m.decoder, cache, xa) if first else D.beam_step(m.decoder, cache)
            state_rows = [a * beam for a in range(nB)] if first else list(range(nB * beam))
            live = [k for k, r in enumerate(state_rows) if not st.audios[r // beam].done]
            if live:
                sel = torch.tensor([state_rows[k] for k in live])
                toks, lens = cache.tokens.cpu()[sel], cache.len.cpu()[sel]
            if live and (check_steps is None or check_steps(i, lens.tolist())):
                rec["checked"].append(i)
                got = logits[:, :V].float().cpu()[live]
                rec["rows"] += len(live)
                if oracle is not None:
                    ref = DO.oracle_last_logits(oracle, xa_ref[sel // beam], toks, lens)
                    rec["rel_oracle"].append(max(DO.rel(got[k], ref[k]) for k in range(len(live))))
                if compare_teacher:
                    Lm = int(lens.max())
                    tf = m.decoder(toks[:, :Lm].to(mel.device), xa[(sel // beam).to(mel.device)])[torch.arange(len(live)), lens.long() - 1].cpu()
                    rec["rel_teacher"].append(max(DO.rel(got[k], tf[k]) for k in range(len(live))))
            D.beam_topk(m.decoder, cache, logits, first=first)
            ct, cl = cache.cand_tok.cpu().numpy(), cache.cand_logp.cpu().numpy()
            if first:
                rec["first_cands"] = ct.copy()
            D.beam_update(cache, first=first)
            BO.step_candidates(st, _as_lists(ct, cl, nB, beam))
            _view(cache).check(st, f"step {i}")
            for au in st.audios:
                if au.done and au.a not in rec["done_at"]:
                    rec["done_at"][au.a] = i
    return cache, st, rec


def _check_final(cache, st, length_penalty=None):
    got, want = D.beam_finalize(cache, length_penalty), BO.finalize(st, length_penalty)
    for a, ((ge, gw), (we, ww)) in enumerate(zip(got, want)):
        assert gw == ww and len(ge) == len(we), a
        for (gt, gs, gsc), (wt, ws, wn) in zip(ge, we):
            assert gt == wt and np.float32(gs).tobytes() == np.float32(ws).tobytes() and gsc == BO.score(wn, ws, length_penalty), a


@pytest.fixture(scope="module")
def case():
    dims, params, audio, y_in, y_out = _tiny_case(B=B, S=S)
    m = _engine(dims, params).eval()
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    oracle = O.Oracle(dims, params)
    prompt = _prompts(y_in)
    cache, st, rec = drive(m, oracle, mel, prompt.to(DEV), PROMPT_LEN, STEPS, beam=W, cands=W, eot=EOT, max_len=MAX_LEN)
    return dict(dims=dims, params=params, model=m, mel=mel, oracle=oracle, prompt=prompt, cache=cache, st=st, rec=rec, y_in=y_in, y_out=y_out)


def _args(case):
    return case["mel"], case["prompt"].to(DEV), PROMPT_LEN


def _same(a, b, what=""):
    for x, y, name in zip(a[:3], b[:3], ("tokens", "lengths", "sum_logprob")):
        assert torch.equal(x, y), f"{what}: {name} differ"
    if len(a) > 3:
        assert a[3] == b[3], f"{what}: the ranked lists differ"


def test_a_cached_logits_of_every_beam_on_its_own_prefix(case):
    rec = case["rec"]
    print(f"{rec['rows']} rows compared.  cached vs teacher-forced, worst row per step:", " ".join(f"{v:.4f}" for v in rec["rel_teacher"]))
    print("cached vs the fp32 oracle, worst row per step:", " ".join(f"{v:.4f}" for v in rec["rel_oracle"]))
    assert len(rec["rel_oracle"]) == STEPS and rec["rows"] >= B + (STEPS - 4) * B * W
    assert max(rec["rel_teacher"]) < 2e-2, max(rec["rel_teacher"])
    assert max(rec["rel_oracle"]) < 2e-2, max(rec["rel_oracle"])
    # the run did reorder beams: some slot was filled from another source, and some audio holds two beams with a common ancestor slot
    anc, lens, first = case["cache"].anc.cpu(), case["cache"].len.cpu(), case["cache"].first_len.cpu()
    moved = sum(int((anc[r, int(first[r]):int(lens[r]) - 1] != r).sum()) for r in range(B * W))
    print(f"{moved} generated positions are read from another slot than the row's own")
    assert moved > 0, "no beam was ever reordered: the ancestry table was not exercised"


def test_b_replay_through_the_oracle_and_beam_decode_equals_its_pieces(case):
    """drive() has compared the state with the oracle after every step; here the end of decoding, and beam_decode as a whole."""
    m = case["model"]
    _check_final(case["cache"], case["st"])
    _check_final(case["cache"], case["st"], length_penalty=0.6)
    tokens, lengths, slp, ranked = m.beam_decode(*_args(case), beam_size=W, eot=EOT, max_len=MAX_LEN, return_all=True)
    assert tokens.dtype == torch.int64 and tokens.shape == (B, int(lengths.max())) and slp.dtype == torch.float32 and m.training is False
    # the audio with the longest prompt has run exactly the STEPS steps of drive(): same winner; every audio: prompt kept, padded with eot
    want = BO.finalize(case["st"])
    a = B - 1
    entries, win = want[a]
    assert tokens[a, :int(lengths[a])].tolist() == entries[win][0] and np.float32(slp[a].item()).tobytes() == np.float32(entries[win][1]).tobytes()
    for b in range(B):
        assert torch.equal(tokens[b, :PROMPT_LEN[b]].cpu(), case["prompt"][b, :PROMPT_LEN[b]]) and (tokens[b, int(lengths[b]):] == EOT).all()
        assert len(ranked[b]) == W and ranked[b][0][0] == tokens[b, :int(lengths[b])].tolist()
        assert all(ranked[b][i][2] >= ranked[b][i + 1][2] for i in range(W - 1))
    with pytest.raises(ValueError):
        m.beam_decode(*_args(case), beam_size=W, eot=EOT, max_len=T - 1)  # KVCache.start's checks hold
    with pytest.raises(NotImplementedError):
        m.decoder(case["prompt"].to(DEV), m.encoder(case["mel"]), kv_cache={"k": 1})


def test_c_small_live_vocabulary_fills_the_lists_and_stops_early(case, monkeypatch):
    """Six live columns, `eot` among them: every beam offers eot at every step, so finished lists fill.  Audios complete at different
    steps by construction — the longest prompt is at max_len after ONE step, and a list of C = 5 cannot fill in the first step,
    which finishes at most one sequence.  The host stops once `unfinished` is 0, and sync_every changes nothing.
    Which of the six tokens plays eot is taken from the run itself (the first, in the order of audio 0's first candidates, with
    which a list fills and everybody is done before the shortest prompt reaches max_len): a random-init model has no real eot."""
    m, V = case["model"], case["dims"].n_vocab
    live = [int(t) for t in case["rec"]["first_cands"][0]]
    suppress = sorted(set(range(V)) - set(live))
    max_len = T + 1
    most = max_len - int(PROMPT_LEN.min())
    found = None
    for eot2 in live:
        cache, st, rec = drive(m, None, case["mel"], case["prompt"].to(DEV), PROMPT_LEN, most, compare_teacher=False, beam=W, cands=W, eot=eot2,
                               max_len=max_len, suppress=suppress)
        print(f"eot = {eot2}: audios done at steps {rec['done_at']}, finished per audio {[len(au.fin) for au in st.audios]}")
        assert st.unfinished == 0 and rec["done_at"][B - 1] == 0 < rec["done_at"][0]
        if any(len(au.fin) == W for au in st.audios) and max(rec["done_at"].values()) + 1 < most:
            found = eot2
            break
    assert found is not None, "with none of the six tokens as eot did a list fill and the decode end early: the case tests nothing"
    eot2 = found
    assert len(set(rec["done_at"].values())) > 1
    _check_final(cache, st)
    calls = []
    real = D.beam_update
    monkeypatch.setattr(D.beam, "beam_update", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    res = {}
    for se in (1, 8):
        calls.clear()
        res[se] = m.beam_decode(*_args(case), beam_size=W, eot=eot2, max_len=max_len, suppress=suppress, sync_every=se, return_all=True)
        res[se, "updates"] = len(calls)
    _same(res[1], res[8], "sync_every")
    last = max(rec["done_at"].values())
    assert res[1, "updates"] == last + 1 < most, (res[1, "updates"], last)  # stopped after the step that left nobody
    assert res[8, "updates"] == most  # (fewer than 8 steps: the counter is never read, every step is issued, the result is the same)
    want = BO.finalize(st)
    for a in range(B):
        entries, win = want[a]
        assert res[1][0][a, :int(res[1][1][a])].tolist() == entries[win][0], a
        assert entries[win][0][-1] == eot2 or len(entries[win][0]) == max_len


def test_d_beam_of_one_is_greedy_decoding(case):
    m = case["model"]
    gen = [int(t) for t in case["rec"]["first_cands"][0][:3]]
    for kw in (dict(eot=EOT), dict(eot=EOT, suppress=[gen[0]]), dict(eot=EOT, suppress_first=[gen[0], gen[1]])):
        g = m.greedy_decode(*_args(case), max_len=MAX_LEN, **kw)
        b = m.beam_decode(*_args(case), beam_size=1, max_len=MAX_LEN, **kw)
        assert torch.equal(g[0], b[0]) and torch.equal(g[1], b[1]), kw
        err = (g[2] - b[2]).abs().cpu()
        assert (err <= 1e-3 * g[2].abs().cpu().clamp(min=1.0)).all(), (kw, err)
    # an eot that some rows emit: greedy rows end there, so does a beam of one
    full = m.greedy_decode(*_args(case), eot=EOT, max_len=MAX_LEN)[0]
    rows = [full[b, int(PROMPT_LEN[b]):int(PROMPT_LEN[b]) + STEPS].tolist() for b in range(B)]
    eot2 = next((t for t in sorted({t for r in rows for t in r[1:]}) if 0 < sum(t in r for r in rows) < B), None)
    assert eot2 is not None
    g = m.greedy_decode(*_args(case), eot=eot2, max_len=MAX_LEN)
    b = m.beam_decode(*_args(case), beam_size=1, eot=eot2, max_len=MAX_LEN)
    assert torch.equal(g[0], b[0]) and torch.equal(g[1], b[1]) and 0 < int((g[1] < MAX_LEN).sum()) < B
    assert ((g[2] - b[2]).abs().cpu() <= 1e-3 * g[2].abs().cpu().clamp(min=1.0)).all()


def test_e_graph_steps_change_nothing_and_keep_greedy_sessions_apart(case):
    m = case["model"]
    D.release_graphs(m)
    gk = dict(eot=EOT, max_len=MAX_LEN)
    greedy = m.greedy_decode(*_args(case), step="graph", **gk)
    before = dict(D.sessions(m))
    (gsess,) = before.values()
    gcounts = (gsess.captures, gsess.replays)
    live = [int(t) for t in case["rec"]["first_cands"][0]]
    variants = [dict(eot=EOT, max_len=MAX_LEN), dict(eot=live[2], max_len=MAX_LEN, suppress_first=[live[0]]),
                dict(eot=EOT, max_len=MAX_LEN, patience=2.0, length_penalty=1.0)]
    for kw in variants:
        for se in (1, 8):
            kw2 = dict(kw, beam_size=W, sync_every=se, return_all=True)
            eager = m.beam_decode(*_args(case), **kw2)
            _same(m.beam_decode(*_args(case), step="graph", _stream_gemm=False, **kw2), eager, f"graph on the eager step's GEMMs {kw2}")
            _same(m.beam_decode(*_args(case), step="graph", **kw2), m.beam_decode(*_args(case), step="graph", _capture=False, **kw2),
                  f"graph vs eager steps on the streaming GEMMs {kw2}")
    # greedy sessions: same keys, same objects, untouched counters; beam sessions live in their own table, capped like the others
    assert D.sessions(m) == before and (gsess.captures, gsess.replays) == gcounts
    assert len(D.beam_sessions(m)) == D.MAX_SESSIONS and all(k[1] == W for k in D.beam_sessions(m))
    _same(m.greedy_decode(*_args(case), step="graph", **gk), greedy, "greedy graph after beam decodes")
    D.release_graphs(m)
    assert D.sessions(m) == {} and D.beam_sessions(m) == {}
    # one capture, then replays
    first = m.beam_decode(*_args(case), beam_size=W, step="graph", **gk)
    (sess,) = D.beam_sessions(m).values()
    assert sess.captures == 1 and sess.replays >= STEPS - 3, (sess.captures, sess.replays)
    r0 = sess.replays
    _same(m.beam_decode(*_args(case), beam_size=W, step="graph", **gk), first, "second call")
    assert sess.captures == 1 and sess.replays >= r0 + STEPS - 1, "the second call must replay every cached step"
    D.release_graphs(m)
    assert D.beam_sessions(m) == {}


def test_e_a_stale_beam_graph_is_never_replayed_after_a_weight_update():
    dims, params, audio, y_in, y_out = _tiny_case(B=B, S=S)
    m = _engine(dims, params)
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    args = (mel, _prompts(y_in).to(DEV), PROMPT_LEN)
    kw = dict(beam_size=W, eot=EOT, max_len=T + 8)
    before = m.beam_decode(*args, step="graph", **kw)
    (sess,) = D.beam_sessions(m).values()
    assert sess.captures == 1
    fp = sess.fingerprint
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=3e-3)
    m(mel, y_in.to(DEV), targets=y_out.to(DEV), label_smoothing=0.1).backward()
    opt.step()
    after = m.beam_decode(*args, step="graph", **kw)
    assert m.training
    _same(after, m.beam_decode(*args, step="graph", _capture=False, **kw), "after an optimizer step")
    assert not torch.equal(after[2], before[2]), "the optimizer step did not reach the decode"
    # recaptured exactly if an address the graph holds changed (weight shadows, scratch slots); otherwise the replay read the new values
    print("fingerprint changed:", sess.fingerprint != fp, "captures:", sess.captures)
    assert sess.captures == (2 if sess.fingerprint != fp else 1), sess.captures
    # adapters change what the graph would have to launch: the fingerprint differs, the step is captured again, nothing is merged
    caps = sess.captures
    torch.manual_seed(9)
    lora_mod.apply_lora(m, {"rank": 8, "lora_alpha": 16, "lora_dropout": 0.1})
    gl = torch.Generator().manual_seed(9)
    for n, mod in m.named_modules():
        if "parametrizations" in mod._modules:
            ad = mod.parametrizations.weight[0]
            with torch.no_grad():
                ad.lora_B.copy_((torch.randn(ad.lora_B.shape, generator=gl) * 0.05).to(ad.lora_B.device))
    m.to(DEV)
    adapted = m.beam_decode(*args, step="graph", **kw)
    _same(adapted, m.beam_decode(*args, step="graph", _capture=False, **kw), "after apply_lora")
    assert sess.captures == caps + 1 and not torch.equal(adapted[2], after[2])
    assert any("parametrizations" in mod._modules for mod in m.modules())
    D.release_graphs(m)


def test_f_reruns_are_bit_identical_and_lora_decodes_without_merge(case):
    m = case["model"]
    kw = dict(beam_size=W, eot=EOT, max_len=MAX_LEN, return_all=True)
    _same(m.beam_decode(*_args(case), **kw), m.beam_decode(*_args(case), **kw), "second run")
    dims, params, audio, y_in, _ = _tiny_case(B=B, S=S)
    ml = Whisper(MODEL_DIMS["tiny"]); ml.load_state_dict(params)
    torch.manual_seed(9)
    lora_mod.apply_lora(ml, {"rank": 8, "lora_alpha": 16, "lora_dropout": 0.1})
    gl = torch.Generator().manual_seed(9)
    cfg = {}
    for n, mod in ml.named_modules():
        if "parametrizations" in mod._modules:
            ad = mod.parametrizations.weight[0]
            with torch.no_grad():
                ad.lora_B.copy_(torch.randn(ad.lora_B.shape, generator=gl) * 0.05)
            cfg[n] = (ad.lora_A.detach().clone(), ad.lora_B.detach().clone(), ad.scaling, None)
    ml.to(DEV).train()
    steps = 5
    cache, st, rec = drive(ml, O.Oracle(dims, params, lora=cfg), case["mel"], case["prompt"].to(DEV), PROMPT_LEN, steps, beam=W, cands=W,
                           eot=EOT, max_len=T + steps, compare_teacher=False)
    print("adapted model, cached beam logits vs the fp32 oracle with the same adapters:", " ".join(f"{v:.4f}" for v in rec["rel_oracle"]))
    assert max(rec["rel_oracle"]) < 2e-2
    ml.train()
    out = ml.beam_decode(*_args(case), beam_size=W, eot=EOT, max_len=T + steps)
    assert ml.training
    entries, win = BO.finalize(st)[B - 1]
    assert out[0][B - 1, :int(out[1][B - 1])].tolist() == entries[win][0]
    assert all("parametrizations" in mod._modules for n, mod in ml.named_modules() if n in cfg)  # nothing was merged
