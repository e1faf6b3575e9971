"""Host side of sampled decoding that needs no GPU: the numpy Philox oracle (tests/_sample_oracle.py) against the generator's known
answers, the exactness of the uniforms, `needs_fallback`'s truth table, the temperature ladder against stub decoders that record
their calls, avg_logprob / compression ratio, the argument checks (raised before a device is touched) and the evaluator's
`fallback` mode with a stub model."""
import math
import zlib

import numpy as np
import pytest
import torch

from tests import _sample_oracle as SO
from tests.test_decode_host import _Stub, _Tok, _batch
from whisper_finetune.engine import decode as D
from whisper_finetune.eval import evaluator

EOT = 9


# ----------------------------------------------------------------------------- the generator
def test_philox_known_answers():
    assert [f"{w:08x}" for w in SO.philox4x32_10([0, 0, 0, 0], [0, 0])] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = 0xFFFFFFFF
    assert [f"{w:08x}" for w in SO.philox4x32_10([ones] * 4, [ones] * 2)] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    # vectorised over leading axes, and the column -> (block, word) mapping of the kernel
    both = SO.philox4x32_10([[0, 0, 0, 0], [ones] * 4], [[0, 0], [ones] * 2])
    assert both.shape == (2, 4) and int(both[1, 3]) == 0x6d5451fd
    w = SO.words(0, 0, [0, 1, 2, 3])
    assert [f"{x:08x}" for x in w] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert int(SO.words(5, 7, [13])[0]) == int(SO.philox4x32_10([3, 7, 0, 0], [5, 0])[1])
    assert int(SO.words((9 << 32) | 5, 7, [13])[0]) == int(SO.philox4x32_10([3, 7, 0, 0], [5, 9])[1])


def test_every_uniform_is_exact_in_fp32_and_inside_the_open_interval():
    cols = np.arange(51866)
    for seed, pos in ((0, 0), (1234, 3), ((1 << 64) - 1, 447)):
        v = SO.uniforms(seed, pos, cols)
        assert (v.astype(np.float32).astype(np.float64) == v).all()
        assert v.min() >= 2.0 ** -24 and v.max() <= 1.0 - 2.0 ** -24
        assert np.isfinite(SO.gumbel(seed, pos, cols)).all()
    # the extremes of the word: k = 0 and k = 2^23 - 1
    assert (2.0 * 0 + 1) * 2.0 ** -24 > 0 and np.float32((2.0 * (2 ** 23 - 1) + 1) * 2.0 ** -24) < np.float32(1.0)
    # the 24-bit (k + 0.5) * 2^-24 form the header rejects is NOT exact in fp32
    k = (SO.words(1234, 3, cols) >> np.uint32(8)).astype(np.float64)
    bad = (k + 0.5) * 2.0 ** -24
    assert (bad.astype(np.float32).astype(np.float64) != bad).any()


def test_noise_depends_on_seed_position_and_column_only():
    a = SO.gumbel(7, 3, np.arange(64))
    assert np.array_equal(a[[5, 9, 60]], SO.gumbel(7, 3, [5, 9, 60]))  # (not on which other columns are live)
    assert not np.array_equal(a, SO.gumbel(8, 3, np.arange(64))) and not np.array_equal(a, SO.gumbel(7, 4, np.arange(64)))


def test_oracle_pick_rules():
    x = np.array([0.0, 3.0, -np.inf, 3.0, 1.0])
    p = SO.pick(x, 0.0, 1, 3, EOT)
    assert (p.col, p.gap) == (1, 0.0) and p.logp == pytest.approx(3.0 - math.log(1 + 2 * math.exp(3) + math.exp(1)))
    assert SO.pick(np.full(4, -np.inf), 1.0, 1, 3, EOT) == SO.Pick(EOT, 0.0, float("inf"))
    picks = [SO.pick(x, 1.0, s, 3, EOT) for s in range(200)]
    assert all(p.col != 2 for p in picks) and {p.col for p in picks} >= {1, 3}
    lse = math.log(1 + 2 * math.exp(3) + math.exp(1))
    assert all(p.logp == pytest.approx(x[p.col] - lse) for p in picks)  # the log-probability is the one at temperature 1
    cold = [SO.pick(x, 1e-3, s, 3, EOT).col for s in range(50)]
    assert set(cold) <= {1, 3}


def test_sample_seeds():
    assert D.sample_seeds(3, 2, 3) == [24, 25, 26, 32, 33, 34]
    assert D.sample_seeds([10, 2], 2, 2) == [80, 81, 16, 17]
    assert D.sample_seeds(torch.tensor([10, 2]), 2, 1) == [80, 16]
    assert D.sample_seeds((1 << 64) - 1, 1, 2) == [(1 << 64) - 8, (1 << 64) - 7]  # mod 2^64
    with pytest.raises(ValueError):
        D.sample_seeds([1, 2, 3], 2, 2)
    with pytest.raises(ValueError):
        D.sample_seeds(True, 2, 2)


# ----------------------------------------------------------------------------- needs_fallback
TH = {"compression_ratio": 2.4, "logprob": -1.0, "no_speech": 0.6}


@pytest.mark.parametrize("alp,nsp,ratio,th,want", [
    (-0.5, 0.1, 1.0, TH, False),                    # all three pass
    (-0.5, 0.1, 2.5, TH, True),                     # 1: the ratio alone
    (-0.5, 0.1, 2.4, TH, False),                    # (strictly above)
    (-1.5, 0.1, 1.0, TH, True),                     # 2: the average log-probability alone
    (-1.0, 0.1, 1.0, TH, False),                    # (strictly below)
    (-1.5, 0.1, 3.0, TH, True),                     # both
    (-1.5, 0.7, 1.0, TH, False),                    # 3: silence overrides test 2
    (-1.5, 0.7, 3.0, TH, False),                    # ... and test 1, as upstream's order has it
    (-1.5, 0.6, 1.0, TH, True),                     # (strictly above)
    (-0.5, 0.9, 3.0, TH, True),                     # silence needs the low log-probability too
    (-1.5, 0.1, 3.0, dict(TH, compression_ratio=None), True),
    (-0.5, 0.1, 3.0, dict(TH, compression_ratio=None), False),   # None switches test 1 off
    (-1.5, 0.1, 1.0, dict(TH, logprob=None), False),             # None switches test 2 off
    (-1.5, 0.9, 3.0, dict(TH, logprob=None), True),              # ... and with it the silence override
    (-1.5, 0.9, 1.0, dict(TH, no_speech=None), True),            # None switches test 3 off
    (-1.5, None, 1.0, TH, True),                                 # no no-speech probability: no override
    (-1.5, 0.9, None, TH, False),                                # no ratio: test 1 off
    (-5.0, 0.0, 99.0, {}, False),                                # no thresholds at all
])
def test_needs_fallback_truth_table(alp, nsp, ratio, th, want):
    assert D.needs_fallback(alp, nsp, ratio, thresholds=th) is want


# ----------------------------------------------------------------------------- avg_logprob, compression ratio
def test_avg_logprob_with_and_without_a_final_eot():
    row = [1, 2, 3, 4, 5, EOT, EOT, EOT]
    ids, text = D.generated_ids(row, 2, 6, EOT)            # ended by eot: 3 generated tokens before it
    assert ids == [3, 4, 5] == text and D.avg_logprob(-8.0, len(ids)) == -2.0
    ids, _ = D.generated_ids(row, 2, 5, EOT)               # cut at max_len: all 3 generated tokens count, no eot to drop
    assert ids == [3, 4, 5] and D.avg_logprob(-8.0, len(ids)) == -2.0
    ids, _ = D.generated_ids([1, 2, EOT], 2, 3, EOT)       # eot at once: n = 0, the divisor is 1
    assert ids == [] and D.avg_logprob(-0.25, 0) == -0.25
    ids, text = D.generated_ids([1, 2, 50, 3, 51, EOT], 2, 6, EOT, timestamp_begin=50)
    assert ids == [50, 3, 51] and text == [3]              # timestamps count for the average, not for the text


def test_compression_ratio_with_the_byte_tokenizer():
    from whisper_finetune.data.data_loader import SimpleTokenizer

    tok = SimpleTokenizer()
    loop = tok.encode("und dann " * 40)
    plain = tok.encode("der schnelle braune fuchs springt ueber den faulen hund")
    for ids in (loop, plain):
        b = tok.decode(ids).encode("utf-8")
        assert D.compression_ratio(tok.decode(ids)) == len(b) / len(zlib.compress(b))
    assert D.compression_ratio(tok.decode(loop)) > 2.4 > D.compression_ratio(tok.decode(plain))
    assert D.compression_ratio("") == 0.0
    assert D.compression_ratio(tok.decode(loop + [tok.eot, tok.timestamp_begin + 3])) == D.compression_ratio(tok.decode(loop))


# ----------------------------------------------------------------------------- the ladder against stub decoders
class _Model:
    """What decode_with_fallback touches of a model: the mode flag, eval / train, the encoder (counted)."""
    compute_dtype = "bf16"

    class dims:
        n_vocab = 100

    def __init__(self):
        self.training = True
        self.encoder_calls = 0

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode

    def encoder(self, mel):
        assert not self.training
        self.encoder_calls += 1
        return mel * 2.0  # (the audio's identity stays readable: xa[a, 0, 0] = 2 * a)


def _ladder(monkeypatch, gen, slp):
    """Stub decoders: audio a at temperature t returns prompt + gen[a](t) (+ eot unless the list ends with None) with sum_logprob
    slp(a, t); every call is recorded."""
    calls = []

    def decode(kind):
        def fn(model, mel, prompt, prompt_len=None, **kw):
            ids = [int(round(float(v))) for v in mel[:, 0, 0]]
            assert [int(round(float(v) / 2)) for v in kw["_xa"][:, 0, 0]] == ids  # the encoder output rides along, row for row
            t = float(kw.get("temperature", 0.0))
            calls.append(dict(kind=kind, audios=ids, **{k: v for k, v in kw.items() if k != "_xa"}, prompt_len=torch.as_tensor(prompt_len).tolist()))
            rows = []
            for j, a in enumerate(ids):
                g = list(gen(a, t))
                tail = [] if g and g[-1] is None else [kw["eot"]]
                rows.append(prompt[j, :int(prompt_len[j])].tolist() + [x for x in g if x is not None] + tail)
            L = max(len(r) for r in rows)
            tokens = torch.tensor([r + [kw["eot"]] * (L - len(r)) for r in rows])
            return tokens, torch.tensor([len(r) for r in rows]), torch.tensor([slp(a, t) for a in ids], dtype=torch.float32)
        return fn

    for kind in ("greedy_decode", "beam_decode", "sample_decode"):
        monkeypatch.setattr(D.fallback, kind, decode(kind))
    return calls


def _inputs(B=4):
    mel = torch.arange(B, dtype=torch.float32)[:, None, None].expand(B, 2, 3).clone()
    prompt = torch.full((B, 3), EOT, dtype=torch.int64)
    plen = [1, 2, 3, 2][:B]
    for a in range(B):
        prompt[a, :plen[a]] = 40 + a
    return mel, prompt, torch.tensor(plen)


def test_ladder_rungs_seeds_padding_and_info(monkeypatch):
    # audio 0 passes at once; 1 passes at 0.2; 2 at 0.4 with a long row; 3 never passes (the last rung stands)
    need = {0: 0.0, 1: 0.2, 2: 0.4, 3: 9.0}
    gen = lambda a, t: [10 + a] * (6 if (a == 2 and t >= 0.4) else 2)
    slp = lambda a, t: -0.3 if t >= need[a] - 1e-9 else -30.0
    calls = _ladder(monkeypatch, gen, slp)
    model = _Model()
    mel, prompt, plen = _inputs()
    tokens, lengths, s, info = D.decode_with_fallback(model, mel, prompt, plen, temperatures=(0.0, 0.2, 0.4), best_of=3, seed=100, eot=EOT, max_len=20,
                                                      suppress=[1], step="eager")
    assert model.encoder_calls == 1 and model.training  # the encoder ran once; the mode is restored
    assert [(c["kind"], c["audios"]) for c in calls] == [("greedy_decode", [0, 1, 2, 3]), ("sample_decode", [1, 2, 3]), ("sample_decode", [2, 3])]
    assert info["rungs"] == [[0, 1, 2, 3], [1, 2, 3], [2, 3]]
    # greedy at 0 gets neither best_of nor a seed; above 0: best_of, and seed + i*B + a for the ORIGINAL index a
    assert "best_of" not in calls[0] and "seed" not in calls[0] and "temperature" not in calls[0]
    assert calls[1]["best_of"] == 3 and calls[1]["temperature"] == 0.2 and calls[1]["seed"] == [100 + 4 + 1, 100 + 4 + 2, 100 + 4 + 3]
    assert calls[2]["seed"] == [100 + 8 + 2, 100 + 8 + 3] and calls[2]["prompt_len"] == [3, 2]
    assert all(c["eot"] == EOT and c["max_len"] == 20 and c["suppress"] == [1] and c["step"] == "eager" for c in calls)
    assert info["temperature"] == [0.0, 0.2, 0.4, 0.4]
    # rows from different rungs, padded with eot to one width
    assert lengths.tolist() == [1 + 2 + 1, 2 + 2 + 1, 3 + 6 + 1, 2 + 2 + 1] and tokens.shape == (4, 10)
    assert tokens[0].tolist() == [40, 10, 10, EOT] + [EOT] * 6 and tokens[2].tolist() == [42] * 3 + [12] * 6 + [EOT]
    assert tokens[3].tolist() == [43, 43, 13, 13, EOT] + [EOT] * 5
    assert s.tolist() == pytest.approx([-0.3, -0.3, -0.3, -30.0])
    assert info["avg_logprob"] == pytest.approx([-0.3 / 3, -0.3 / 3, -0.3 / 7, -30.0 / 3])
    assert info["no_speech_prob"] == [None] * 4 and info["compression_ratio"] == [None] * 4


def test_ladder_beam_at_zero_stops_early_and_counts_rows_cut_at_max_len(monkeypatch):
    calls = _ladder(monkeypatch, lambda a, t: [5, 6, 7, None], lambda a, t: -2.0)  # no final eot: cut at max_len, n = 3
    model = _Model()
    model.training = False
    mel, prompt, plen = _inputs(2)
    out = D.decode_with_fallback(model, mel, prompt, plen, beam_size=4, patience=2.0, length_penalty=0.5, logprob_threshold=-0.6, eot=EOT)
    assert [(c["kind"], c["beam_size"], c["patience"], c["length_penalty"]) for c in calls] == [("beam_decode", 4, 2.0, 0.5)]  # -2/4 passes: one rung
    assert out[3]["avg_logprob"] == pytest.approx([-0.5, -0.5]) and out[3]["rungs"] == [[0, 1]] and not model.training
    assert out[1].tolist() == [4, 5] and out[0][0].tolist() == [40, 5, 6, 7, EOT]
    # with the text function: the ratio is taken over the ids without eot and timestamps, and a looping text is retried
    calls.clear()
    loop = lambda a, t: ([1, 2] * 60 + [70]) if t == 0 else [1, 2, 3, 70]
    calls = _ladder(monkeypatch, loop, lambda a, t: -0.1)
    text_of = lambda ids: "".join(chr(97 + i) for i in ids)
    out = D.decode_with_fallback(model, mel, prompt, plen, temperatures=(0.0, 0.5), best_of=2, compression_ratio_threshold=2.4, text_of=text_of,
                                 timestamp_begin=70, eot=EOT)
    assert [c["kind"] for c in calls] == ["greedy_decode", "sample_decode"] and calls[1]["timestamp_begin"] == 70
    assert out[3]["compression_ratio"] == pytest.approx([D.compression_ratio("bcd")] * 2) and out[3]["temperature"] == [0.5, 0.5]


def test_ladder_argument_errors(monkeypatch):
    calls = _ladder(monkeypatch, lambda a, t: [1], lambda a, t: 0.0)
    model = _Model()
    mel, prompt, plen = _inputs(2)
    for kw in (dict(temperatures=()), dict(temperatures=(0.0, -0.2)), dict(temperatures=(float("inf"),)), dict(best_of=0), dict(best_of=9),
               dict(best_of=2.0), dict(beam_size=9), dict(compression_ratio_threshold=2.4), dict(seed=1.5), dict(step="fast"),
               dict(length_penalty="1")):
        with pytest.raises(ValueError):
            D.decode_with_fallback(model, mel, prompt, plen, eot=EOT, **kw)
    with pytest.raises(TypeError):
        D.decode_with_fallback(model, mel, prompt, plen)
    model.compute_dtype = "fp32"
    with pytest.raises(NotImplementedError, match="bf16"):
        D.decode_with_fallback(model, mel, prompt, plen, eot=EOT)
    assert not calls and model.encoder_calls == 0


class _NoDevice:
    """Anything sample_decode could touch after its argument checks raises."""

    class dims:
        n_vocab = 20

    compute_dtype = "bf16"

    def __getattr__(self, name):
        raise AssertionError(f"sample_decode touched model.{name} before refusing its arguments")


@pytest.mark.parametrize("kw", [dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature=True),
                                dict(temperature="1"), dict(temperature=1.0, best_of=0), dict(temperature=1.0, best_of=9),
                                dict(temperature=1.0, best_of=2.0), dict(temperature=0.0, best_of=9), dict(temperature=1.0, seed=[1, 2, 3]),
                                dict(temperature=1.0, step="fast"), dict(temperature=1.0, length_penalty="1"),
                                dict(temperature=1.0, timestamp_begin=2)])
def test_sample_decode_refuses_bad_arguments_before_any_device_work(kw):
    with pytest.raises(ValueError):
        D.sample_decode(_NoDevice(), None, torch.zeros(2, 3, dtype=torch.int64), None, eot=3, **kw)


def test_sample_decode_refuses_the_fp32_mode():
    m = _NoDevice()
    m.compute_dtype = "fp32"
    with pytest.raises(NotImplementedError, match="bf16"):
        D.sample_decode(m, None, torch.zeros(2, 3, dtype=torch.int64), None, eot=3, temperature=0.5)


def test_public_methods_exist_and_sessions_are_a_third_table():
    from whisper_finetune.engine.whisper_model import Whisper

    assert callable(Whisper.sample_decode) and callable(Whisper.decode_with_fallback)
    assert D._SAMPLE_SESSIONS is not D._SESSIONS and D._SAMPLE_SESSIONS is not D._BEAM_SESSIONS
    m = _Model()
    D._SAMPLE_SESSIONS[m] = {"k": object()}
    assert list(D.sample_sessions(m)) == ["k"]
    D.release_graphs(m)
    assert D.sample_sessions(m) == {}


# ----------------------------------------------------------------------------- the evaluator's fallback mode
class _FallbackStub(_Stub):
    def __init__(self, decoded):
        super().__init__(decoded)
        self.fb_calls = []

    def decode_with_fallback(self, mel, prompt, prompt_len, **kw):
        self.fb_calls.append(dict(kw, prompt_len=torch.as_tensor(prompt_len).tolist()))
        t, n, s = self.greedy_decode(mel, prompt, prompt_len, eot=kw["eot"])
        return t, n, s, {}


class _TokNS(_Tok):
    no_speech = 95
    special_tokens = dict(_Tok.special_tokens, **{"<|nospeech|>": 95})


CFG = {"mixed_precision_training": False}


def test_evaluator_fallback_mode_calls_the_ladder(monkeypatch):
    released = []
    monkeypatch.setattr(D, "release_graphs", lambda m: released.append(m))
    stub = _FallbackStub([[0, 1, 26, 2, 3], [0, 1, 26, 4, 5, 26, 6]])
    base = evaluator.evaluate_single_dataset(stub, [_batch()], "syn", CFG, tokenizer=_Tok())
    assert not stub.fb_calls and not stub.calls  # a minimal config still takes today's path
    tok = _Tok()
    got = evaluator.evaluate_single_dataset(stub, [_batch(), _batch()], "syn", dict(CFG, wft_eval_decode="fallback"), tokenizer=tok)
    assert len(stub.fb_calls) == 2
    c = stub.fb_calls[0]
    assert c["temperatures"] == (0.0, 0.2, 0.4, 0.6, 0.8, 1.0) and c["best_of"] == 5 and c["seed"] == 0   # upstream's defaults
    assert (c["logprob_threshold"], c["no_speech_threshold"], c["compression_ratio_threshold"]) == (-1.0, 0.6, 2.4)
    assert c["text_of"] == tok.decode and "beam_size" not in c and "no_speech" not in c and "step" not in c
    # the prefix / suppression / length rules of the greedy mode
    assert c["prompt_len"] == [4, 7] and c["suppress"] == [90, 92, 93, 94] and c["suppress_first"] == [91, 26] and c["max_len"] == 7 + 448 // 2
    assert got.wer == pytest.approx(0.5) and not released
    for key in ("mean_token_nll", "avg_log_prob", "mean_token_entropy", "ece"):  # token metrics stay teacher-forced
        assert getattr(got, key) == getattr(base, key), key
    stub.fb_calls.clear()
    cfg = dict(CFG, wft_eval_decode="fallback", wft_eval_decode_temperatures=[0, 0.5], wft_eval_decode_best_of=3, wft_eval_decode_seed=7,
               wft_eval_decode_logprob_threshold=None, wft_eval_decode_no_speech_threshold=0.5, wft_eval_decode_compression_ratio_threshold=3,
               wft_eval_decode_beam_size=4, wft_eval_decode_patience=2.0, wft_eval_decode_step="graph", wft_eval_decode_timestamps=False)
    evaluator.evaluate_single_dataset(stub, [_batch()], "syn", cfg, tokenizer=_TokNS())
    c = stub.fb_calls[0]
    assert c["temperatures"] == (0.0, 0.5) and c["best_of"] == 3 and c["seed"] == 7 and c["logprob_threshold"] is None
    assert (c["no_speech_threshold"], c["compression_ratio_threshold"], c["beam_size"], c["patience"], c["step"]) == (0.5, 3, 4, 2.0, "graph")
    assert c["no_speech"] == 95 and c["sot_index"] == [0, 3]  # the tokenizer has no_speech: read at each row's sot
    assert released == [stub]


@pytest.mark.parametrize("extra", [{"wft_eval_decode_temperatures": []}, {"wft_eval_decode_temperatures": 0.5}, {"wft_eval_decode_temperatures": [0, -1]},
                                   {"wft_eval_decode_temperatures": [0, "1"]}, {"wft_eval_decode_best_of": 0}, {"wft_eval_decode_best_of": 9},
                                   {"wft_eval_decode_best_of": 2.5}, {"wft_eval_decode_logprob_threshold": "low"},
                                   {"wft_eval_decode_no_speech_threshold": True}, {"wft_eval_decode_compression_ratio_threshold": [2.4]},
                                   {"wft_eval_decode_seed": 1.5}, {"wft_eval_decode_beam_size": 9}, {"wft_eval_decode_patience": 0},
                                   {"wft_eval_decode_step": "fast"}])
def test_evaluator_fallback_refuses_bad_values_before_the_loop(extra):
    stub = _FallbackStub([[0], [0]])
    with pytest.raises(ValueError):
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(CFG, wft_eval_decode="fallback", **extra), tokenizer=_Tok())
    assert not stub.fb_calls


def test_evaluator_unknown_mode_still_names_the_others_and_fallback_needs_the_method():
    with pytest.raises(ValueError, match='"greedy".*"beam_search".*"fallback"'):
        evaluator.evaluate_single_dataset(_FallbackStub([[0], [0]]), [_batch()], "syn", dict(CFG, wft_eval_decode="ladder"), tokenizer=_Tok())
    with pytest.raises(RuntimeError, match="decode_with_fallback"):
        evaluator.evaluate_single_dataset(_Stub([[0], [0]]), [_batch()], "syn", dict(CFG, wft_eval_decode="fallback"), tokenizer=_Tok())
