"""Host side of beam-search decoding that needs no GPU: the plain-Python oracle (tests/_beam_oracle.py) against brute force and a
greedy walk, its order rules, the evaluator's `beam_search` mode with a stub model, and beam_decode's argument checks, which are
raised before a device is touched."""
import itertools

import numpy as np
import pytest
import torch

from tests import _beam_oracle as BO
from tests.test_decode_host import _Stub, _Tok, _batch
from whisper_finetune.eval import evaluator

F = np.float32
EOT = 2


def _toy_logits(prefix, V, seed, depth_eot=None):
    """Deterministic fp32 logits of a prefix: tokens 0 / 1 carry the mass, eot some, everything else lies 30 below (so a beam of 8
    holds every prefix that matters: the search is exhaustive over them).  At generated depth `depth_eot`, eot dominates."""
    rng = np.random.default_rng(abs(hash((seed,) + tuple(prefix))) % (2 ** 32))
    x = (rng.standard_normal(V) * 0.5 - 30.0).astype(F)
    x[:3] = (rng.standard_normal(3) * 1.5).astype(F)
    if depth_eot is not None and len(prefix) >= depth_eot:
        x[EOT] = F(25.0)
    return x


def _logp(x):
    x = x.astype(F)
    m = x.max()
    return (x - F(m + F(np.log(np.exp((x - m).astype(F)).sum(dtype=F))))).astype(F)


def _run(prompts, W, C, max_len, V, seed, depth_eot=None, steps=None, **kw):
    st = BO.State(prompts, W, C, EOT, max_len)
    n = 0
    while st.unfinished and (steps is None or n < steps):
        logits = np.stack([_toy_logits(b.tokens[au.first_len:], V, seed + au.a, None if depth_eot is None else depth_eot)
                           for au in st.audios for b in au.beams])
        BO.step_logits(st, logits, **kw)
        n += 1
    return st


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_exhaustive_beam_equals_brute_force(seed):
    """V = 12, three generated tokens at most, W = 8, a list that never fills: the winner is the maximum of sum_logprob / n over
    EVERY sequence (eot-terminated, or cut at max_len), summed in the same fp32 order."""
    V, G, W = 12, 3, 8
    prompt = [7, 7]
    st = _run([prompt], W, BO.candidates(W, 50.0), len(prompt) + G, V, seed, depth_eot=G - 1)
    entries, win = BO.finalize(st)[0]
    best, best_seq = None, None
    for k in range(1, G + 1):
        for seq in itertools.product(range(V), repeat=k):
            if EOT in seq[:-1] or (k < G and seq[-1] != EOT):
                continue  # eot ends a sequence; a shorter one must end with it
            slp = F(0.0)
            for i, t in enumerate(seq):
                slp = F(slp + _logp(_toy_logits(seq[:i], V, seed, G - 1))[t])
            n = k - 1 if seq[-1] == EOT else k
            sc = BO.score(n, slp)
            if best is None or sc > best:
                best, best_seq = sc, list(seq)
    assert entries[win][0] == prompt + best_seq, (entries[win], best_seq, best)
    assert BO.score(entries[win][2], entries[win][1]) == best


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_beam_of_one_is_a_greedy_walk(seed):
    V, max_len = 12, 9
    prompts = [[5], [5, 6, 7]]
    st = _run(prompts, 1, 1, max_len, V, seed)
    res = BO.finalize(st)
    for a, p in enumerate(prompts):
        toks, slp = list(p), F(0.0)
        while len(toks) < max_len:
            lp = _logp(_toy_logits(toks[len(p):], V, seed + a))
            t = int(np.argmax(lp))  # (numpy's argmax: the lowest index on ties)
            toks.append(t); slp = F(slp + lp[t])
            if t == EOT:
                break
        entries, win = res[a]
        assert win == 0 and entries[0][0] == toks and entries[0][1] == slp


def _cands(*rows):
    return [[(t, F(lp)) for t, lp in row] for row in rows]


def test_first_step_collapses_the_copies_of_the_prompt():
    """W identical prompts are ONE hypothesis: only beam 0's candidates are read, and the W new beams all descend from it."""
    W = 3
    st = BO.State([[9, 9]], W, 3, EOT, 10)
    row0 = [(4, -0.1), (5, -0.7), (6, -1.5), (7, -2.0)]
    junk = [(8, 0.0), (3, 0.0), (1, 0.0), (0, 0.0)]  # would win every slot if it were read
    BO.step_candidates(st, [_cands(row0, junk, junk)])
    au = st.audios[0]
    assert [b.tokens for b in au.beams] == [[9, 9, 4], [9, 9, 5], [9, 9, 6]] and au.src == [0, 0, 0]
    assert [b.slp for b in au.beams] == [F(-0.1), F(-0.7), F(-1.5)]
    # the second step reads all W rows
    BO.step_candidates(st, [_cands([(1, -0.1)] + row0[:3], [(3, -0.05)] + row0[:3], row0)])
    assert au.src[0] == 0 and au.beams[0].tokens == [9, 9, 4, 1]  # -0.1 - 0.1 beats -0.7 - 0.05 and 2 * -0.1


@pytest.mark.parametrize("patience,C", [(1.0, 4), (2.0, 8), (0.5, 2), (0.3, 1), (0.625, 2)])
def test_patience_sets_how_many_finished_sequences_end_an_audio(patience, C):
    W = 4
    assert BO.candidates(W, patience) == C  # (0.625 * 4 = 2.5 rounds to the even 2: Python's round)
    st = BO.State([[9]], W, C, EOT, 40)
    steps = 0
    while st.unfinished:
        # every beam offers eot at -0.5 and four others below: after the first step each step finishes W sequences
        row = [(EOT, -0.5), (10 + steps, -1.0), (11 + steps, -1.1), (12 + steps, -1.2), (13 + steps, -1.3)]
        BO.step_candidates(st, [_cands(*([row] * W))])
        steps += 1
        assert len(st.audios[0].fin) == min(C, 1 + (steps - 1) * W)
    assert steps == 1 + -(-(C - 1) // W) and len(st.audios[0].fin) == C


def test_ties_go_to_the_lower_beam_then_the_lower_position():
    W = 2
    st = BO.State([[9]], W, 2, EOT, 10)
    BO.step_candidates(st, [_cands([(4, -1.0), (5, -1.0), (6, -1.0)], [])])
    au = st.audios[0]
    assert [b.tokens[-1] for b in au.beams] == [4, 5]  # equal scores: the lower list position first
    # both beams at -1.0; all four continuations tie at -2.0: beam 0's two candidates win, in list order
    BO.step_candidates(st, [_cands([(7, -1.0), (8, -1.0), (3, -1.0)], [(1, -1.0), (0, -1.0), (3, -1.0)])])
    assert au.src == [0, 0] and [b.tokens[-1] for b in au.beams] == [7, 8]
    # everything ties again: the walk takes beam 0's list in order — 7 (a beam), eot (finished), 3 (the second beam) — and stops there:
    # beam 1's eot, ranked below the point where W beams are saved, is dropped
    BO.step_candidates(st, [_cands([(7, -1.0), (EOT, -1.0), (3, -1.0)], [(EOT, -1.0), (0, -1.0), (3, -1.0)])])
    assert au.src == [0, 0] and [b.tokens[-1] for b in au.beams] == [7, 3]
    assert [t for t, _ in au.fin] == [[9, 4, 7, EOT]] and not au.done


def test_done_audios_are_frozen_and_max_len_ends_an_audio():
    W = 2
    st = BO.State([[9, 9, 9], [9]], W, 2, EOT, 4)  # audio 0 reaches max_len after one step
    row = [(4, -0.5), (5, -0.6), (6, -0.9)]
    BO.step_candidates(st, [_cands(row, row), _cands(row, row)])
    assert st.audios[0].done and not st.audios[1].done and st.unfinished == 1
    snap = [(b.tokens[:], b.slp) for b in st.audios[0].beams]
    BO.step_candidates(st, [_cands(row, row), _cands(row, row)])
    assert [(b.tokens, b.slp) for b in st.audios[0].beams] == snap and st.audios[0].fin == []
    res = BO.finalize(st)
    assert res[0][0][res[0][1]][0] == [9, 9, 9, 4] and len(res[0][0]) == W  # no eot: cut at max_len, beams fill the list
    # length penalty changes the divisor only
    assert BO.score(3, F(-3.0)) == -1.0 and BO.score(1, F(-3.0), 1.0) == -3.0 and BO.score(0, F(-1.0)) == float("-inf")


# ----------------------------------------------------------------------------- the evaluator's beam_search mode
class _BeamStub(_Stub):
    def __init__(self, decoded):
        super().__init__(decoded)
        self.beam_calls = []

    def beam_decode(self, mel, prompt, prompt_len, *, beam_size, patience=1.0, eot, max_len=None, suppress=(), suppress_first=(), step="eager"):
        self.beam_calls.append(dict(beam_size=beam_size, patience=patience, step=step, max_len=max_len, suppress=list(suppress),
                                    suppress_first=list(suppress_first), prompt_len=torch.as_tensor(prompt_len).tolist()))
        return self.greedy_decode(mel, prompt, prompt_len, eot=eot)


def test_evaluator_beam_search_mode_calls_beam_decode(monkeypatch):
    from whisper_finetune.engine import decode as D

    released = []
    monkeypatch.setattr(D, "release_graphs", lambda m: released.append(m))
    cfg = {"mixed_precision_training": False}
    stub = _BeamStub([[0, 1, 26, 2, 3], [0, 1, 26, 4, 5, 26, 6]])
    base = evaluator.evaluate_single_dataset(stub, [_batch()], "syn", cfg, tokenizer=_Tok())
    got = evaluator.evaluate_single_dataset(stub, [_batch(), _batch()], "syn", dict(cfg, wft_eval_decode="beam_search"), tokenizer=_Tok())
    assert len(stub.beam_calls) == 2 and len(stub.calls) == 2  # (the stub's beam_decode goes through its greedy_decode)
    call = stub.beam_calls[0]
    assert call["beam_size"] == 5 and call["patience"] == 1.0 and call["step"] == "eager"  # the defaults
    assert call["prompt_len"] == [4, 7] and call["suppress"] == [90, 92, 93, 94] and call["suppress_first"] == [91, 26]
    assert call["max_len"] == 7 + 448 // 2
    assert got.wer == pytest.approx(0.5) and not released
    for key in ("mean_token_nll", "avg_log_prob", "mean_token_entropy", "ece"):  # token metrics stay teacher-forced
        assert getattr(got, key) == getattr(base, key), key
    stub.beam_calls.clear()
    evaluator.evaluate_single_dataset(stub, [_batch(), _batch()], "syn",
                                      dict(cfg, wft_eval_decode="beam_search", wft_eval_decode_beam_size=3, wft_eval_decode_patience=2.0,
                                           wft_eval_decode_step="graph"), tokenizer=_Tok())
    assert [(c["beam_size"], c["patience"], c["step"]) for c in stub.beam_calls] == [(3, 2.0, "graph")] * 2
    assert released == [stub]  # once per dataset, not per batch


@pytest.mark.parametrize("extra", [{"wft_eval_decode_beam_size": 0}, {"wft_eval_decode_beam_size": 9}, {"wft_eval_decode_beam_size": 2.5},
                                   {"wft_eval_decode_patience": 0}, {"wft_eval_decode_patience": -1.0},
                                   {"wft_eval_decode_beam_size": 1, "wft_eval_decode_patience": 0.2}, {"wft_eval_decode_step": "fast"}])
def test_evaluator_beam_search_refuses_bad_values(extra):
    stub = _BeamStub([[0], [0]])
    with pytest.raises(ValueError):
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict({"mixed_precision_training": False, "wft_eval_decode": "beam_search"}, **extra),
                                          tokenizer=_Tok())
    assert not stub.beam_calls


def test_evaluator_still_refuses_beam_and_names_beam_search():
    stub = _BeamStub([[0], [0]])
    with pytest.raises(ValueError, match="beam_search"):
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", {"mixed_precision_training": False, "wft_eval_decode": "beam"}, tokenizer=_Tok())
    with pytest.raises(RuntimeError, match="beam_decode"):
        evaluator.evaluate_single_dataset(_Stub([[0], [0]]), [_batch()], "syn", {"mixed_precision_training": False, "wft_eval_decode": "beam_search"},
                                          tokenizer=_Tok())


# ----------------------------------------------------------------------------- beam_decode's argument checks
class _NoDevice:
    """Anything beam_decode could touch after its argument checks raises."""

    class dims:
        n_vocab = 20

    compute_dtype = "bf16"

    def __getattr__(self, name):
        raise AssertionError(f"beam_decode touched model.{name} before refusing its arguments")


@pytest.mark.parametrize("kw", [dict(beam_size=0), dict(beam_size=9), dict(beam_size=2.0), dict(beam_size=True),
                                dict(beam_size=5, patience=0.0), dict(beam_size=5, patience=-1.0), dict(beam_size=1, patience=0.3),
                                dict(beam_size=5, patience=float("nan")),
                                dict(beam_size=5, step="fast"),
                                dict(beam_size=5, suppress=list(range(10)), suppress_first=list(range(8, 15))),  # 5 live columns < 6
                                dict(beam_size=5, suppress=[20]),
                                dict(beam_size=5, length_penalty="1")])
def test_beam_decode_refuses_bad_arguments_before_any_device_work(kw):
    from whisper_finetune.engine import decode as D

    with pytest.raises(ValueError):
        D.beam_decode(_NoDevice(), None, None, None, eot=3, **kw)


def test_candidate_count_and_live_column_rule():
    from whisper_finetune.engine import decode as D

    assert D.beam_candidates(5) == 5 and D.beam_candidates(5, 0.5) == 2 and D.beam_candidates(5, 2.0) == 10 and D.beam_candidates(8, 1.3) == 10
    with pytest.raises(ValueError):
        D.beam_candidates(5, 0.09)  # round(0.45) = 0
    D._check_live_columns(5, 20, list(range(10)), list(range(8, 14)))  # 6 live: just enough
    assert D.beam_rank([(0, -0.1), (2, -4.0), (4, -8.0), (1, -2.5)]) == 1  # n = 0 is -inf; -2.0 twice: the first wins
    # -1.0 / 1 against -6.5 / 7 = -0.93 without a penalty; with it (5 + n) / 6 = 1 and 2: -1.0 against -3.25
    assert D.beam_rank([(1, -1.0), (7, -6.5)]) == 1 and D.beam_rank([(1, -1.0), (7, -6.5)], length_penalty=1.0) == 0
    assert D.beam_rank([(0, 0.0)]) == 0
