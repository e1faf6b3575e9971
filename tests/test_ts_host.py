"""Host side of decoding under the timestamp rules, no GPU: the rule oracle (tests/_ts_oracle.py) on hand-written rows, one per
branch of include/wft.h "Timestamp rules"; `timestamp_segments`; every argument error of greedy_decode / beam_decode, raised before
any device work; the evaluator's `wft_eval_decode_timestamps`; the graph fingerprint; the binding of the two new entry points."""
import ctypes
import math
from types import SimpleNamespace

import pytest
import torch

from tests import _ts_oracle as TO
from whisper_finetune.engine import decode as D
from whisper_finetune.engine import lib as L
from whisper_finetune.eval import evaluator
from whisper_finetune.eval.utils import decode_prefix_len

V, EOT, NO_TS, TSB = 40, 20, 25, 30
KW = dict(ts_begin=TSB, eot=EOT, no_timestamps=NO_TS)
NEG = float("-inf")


def _live(r):
    return torch.isfinite(r.x).nonzero().flatten().tolist()


def _flat():
    return torch.zeros(V)


# ----------------------------------------------------------------------------- the oracle, one row per branch
def test_oracle_first_token_only_timestamps_up_to_max_initial():
    r = TO.rules(_flat(), [], max_initial=3, **KW)
    assert _live(r) == [30, 31, 32, 33] and r.ts_wins and r.margin == float("inf")
    assert r.logp[30].item() == pytest.approx(-math.log(4))
    r = TO.rules(_flat(), [], max_initial=0, **KW)
    assert _live(r) == [30] and r.logp[30].item() == 0.0
    r = TO.rules(_flat(), [], max_initial=None, **KW)
    assert _live(r) == list(range(30, 40))
    r = TO.rules(_flat(), [], max_initial=500, **KW)  # beyond the vocabulary: every timestamp
    assert _live(r) == list(range(30, 40))


def test_oracle_single_timestamp_then_text_only():
    # one sampled token, a timestamp: pen_ts counts as true, no timestamp may follow; rule 5 has an empty timestamp side
    r = TO.rules(_flat(), [32], **KW)
    assert _live(r) == [c for c in range(30) if c != NO_TS] and not r.ts_wins and r.margin == NEG


def test_oracle_text_then_timestamp():
    # last_ts && !pen_ts: text below eot is removed, the timestamp t itself stays; flat logits: 7 timestamps outweigh any one text column
    r = TO.rules(_flat(), [31, 5, 33], **KW)
    assert r.ts_wins and _live(r) == list(range(33, 40))
    # with the timestamps pushed down the specials between eot and ts_begin survive too
    x = _flat(); x[TSB:] = -20.0
    r = TO.rules(x, [31, 5, 33], **KW)
    assert not r.ts_wins and _live(r) == [c for c in range(EOT, 30) if c != NO_TS] + list(range(33, 40))


def test_oracle_timestamp_then_timestamp():
    x = _flat()
    r = TO.rules(x, [31, 5, 33, 33], **KW)
    assert _live(r) == [c for c in range(30) if c != NO_TS] and not r.ts_wins


def test_oracle_text_then_text_with_an_earlier_timestamp():
    x = _flat(); x[TSB:] = -20.0
    r = TO.rules(x, [31, 5, 6], **KW)
    assert not r.ts_wins and _live(r) == [c for c in range(30) if c != NO_TS] + list(range(32, 40))
    r = TO.rules(_flat(), [31, 5, 6], **KW)  # flat: the 8 timestamps left win
    assert r.ts_wins and _live(r) == list(range(32, 40))


def test_oracle_last_timestamp_is_the_last_column():
    r = TO.rules(_flat(), [31, 5, V - 1], **KW)   # closing with V - 1: only V - 1 itself may open the next segment
    assert _live(r)[-1] == V - 1 and [c for c in _live(r) if c >= TSB] == [V - 1]
    r = TO.rules(_flat(), [31, 5, V - 1, 6], **KW)  # text behind it: no timestamp is left at all
    assert [c for c in _live(r) if c >= TSB] == [] and not r.ts_wins


def test_oracle_probability_rule_is_strict_and_picks_lowest_on_ties():
    # one live timestamp (V - 1) that equals the text maximum: logsumexp == max, not strictly greater -> text stays, lower column wins
    x = torch.full((V,), -30.0); x[7] = 2.0; x[V - 1] = 2.0
    col, lp, r = TO.pick(x, [31, 5, V - 2, 6], **KW)
    assert not r.ts_wins and r.margin == 0.0 and col == 7
    x[V - 1] = 2.5
    col, lp, r = TO.pick(x, [31, 5, V - 2, 6], **KW)
    assert r.ts_wins and col == V - 1 and lp == 0.0
    # static masks join in; everything removed -> (eot, 0)
    col, lp, r = TO.pick(_flat(), [32], dead=[c for c in range(30) if c != NO_TS], **KW)
    assert (col, lp) == (EOT, 0.0)
    cands, _ = TO.topk(_flat(), 3, [], max_initial=1, **KW)
    assert [c for c, _ in cands] == [30, 31, -1] and cands[2][1] == NEG


def test_structure_checker_knows_the_invariants():
    ok = dict(ts_begin=TSB, eot=EOT, max_initial=5)
    assert TO.check_structure([31, 5, 6, 33, 33, 7, 35, EOT, 3], **ok) is None
    assert "starts with text" in TO.check_structure([5, 31], **ok)
    assert "max_initial" in TO.check_structure([37, 5], **ok)
    assert "decrease" in TO.check_structure([33, 5, 32], **ok)
    assert "lone closing" in TO.check_structure([31, 5, 33, 6], **ok)
    assert "three" in TO.check_structure([31, 5, 33, 33, 34], **ok)


# ----------------------------------------------------------------------------- timestamp_segments
def test_timestamp_segments():
    P = [90, 92, 93]
    rows = [P + [30, 5, 6, 32, 32, 7, 35, EOT],          # two pairs
            P + [31, 5, 33, 33, 8, 9, EOT, EOT],         # a pair, then text behind an unpaired opening timestamp
            P + [30, 31, 31, 5, 6, 7, 8, 9],             # an empty segment; then a row cut at max_len inside a segment
            P + [30, 5, 34, 34, EOT, EOT, EOT, EOT]]     # a lone opening timestamp at the end: no segment for it
    lens = [11, 10, 11, 8]
    segs = D.timestamp_segments(torch.tensor(rows), torch.tensor([3, 3, 3, 3]), torch.tensor(lens), TSB, EOT)
    assert segs[0] == [(0.0, pytest.approx(0.04), [5, 6]), (pytest.approx(0.04), pytest.approx(0.10), [7])]
    assert segs[1] == [(pytest.approx(0.02), pytest.approx(0.06), [5]), (pytest.approx(0.06), None, [8, 9])]
    assert segs[2] == [(0.0, pytest.approx(0.02), []), (pytest.approx(0.02), None, [5, 6, 7, 8, 9])]
    assert segs[3] == [(0.0, pytest.approx(0.08), [5])]
    # nested lists, another precision, the length (not an eot) ends the row
    assert D.timestamp_segments([[30, 1, 2, 40]], [0], [3], 30, EOT, time_precision=0.5) == [[(0.0, None, [1, 2])]]
    assert D.timestamp_segments([[30, 1, 2, 40]], [0], [4], 30, EOT, time_precision=0.5) == [[(0.0, 5.0, [1, 2])]]


# ----------------------------------------------------------------------------- argument errors, before any device work
def _model(n_vocab=100):
    class M:  # (touching anything but these two attributes is device work: it raises AttributeError, not ValueError)
        dims = SimpleNamespace(n_vocab=n_vocab)
        compute_dtype = "bf16"
    return M()


BAD = [
    (dict(timestamp_begin=50), "timestamp_begin"),           # == eot
    (dict(timestamp_begin=100), "timestamp_begin"),          # == n_vocab
    (dict(timestamp_begin=10), "timestamp_begin"),           # below eot
    (dict(timestamp_begin=80, no_timestamps=100), "no_timestamps"),
    (dict(timestamp_begin=80, no_timestamps=-2), "no_timestamps"),
    (dict(timestamp_begin=80, suppress=[3, 80]), "timestamp id"),
    (dict(timestamp_begin=80, suppress_first=[99]), "timestamp id"),
    (dict(timestamp_begin=80, max_initial_timestamp_index=-1), "max_initial_timestamp_index"),
]


@pytest.mark.parametrize("kw,match", BAD)
def test_greedy_decode_argument_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        D.greedy_decode(_model(), None, torch.zeros(1, 3, dtype=torch.int64), eot=50, **kw)


@pytest.mark.parametrize("kw,match", BAD + [
    (dict(timestamp_begin=80, max_initial_timestamp_index=1), "max_initial_timestamp_index"),   # < beam_size - 1
    (dict(timestamp_begin=98, max_initial_timestamp_index=None), "live timestamps"),           # 2 timestamps for 3 beams
    (dict(timestamp_begin=80, suppress=list(range(78)), max_initial_timestamp_index=None), "text columns"),
])
def test_beam_decode_argument_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        D.beam_decode(_model(), None, torch.zeros(1, 3, dtype=torch.int64), eot=50, beam_size=3, **kw)


def test_rule_constants_and_defaults():
    assert D.check_ts_rules(100, 50, [], [], None) is None
    assert D.check_ts_rules(100, 50, [], [], None, no_timestamps=1000, max_initial_timestamp_index=-5) is None  # off: not looked at
    assert D.check_ts_rules(100, 50, [3], [50], 80) == (80, None, 50)
    assert D.check_ts_rules(100, 50, [], [], 80, 60, None) == (80, 60, None)
    assert D.check_ts_rules(100, 50, [], [], 80, 60, 2, beam_size=3) == (80, 60, 2)  # max_initial == beam_size - 1 is enough
    import inspect
    for fn in (D.greedy_decode, D.beam_decode):
        sig = inspect.signature(fn).parameters
        assert sig["timestamp_begin"].default is None and sig["no_timestamps"].default is None
        assert sig["max_initial_timestamp_index"].default == 50


def test_graph_fingerprint_carries_the_rule_constants():
    extras = [D.ts_extra(r) for r in (None, (80, None, 50), (80, 60, 50), (80, 60, None), (81, 60, 50), (80, 60, 49))]
    assert extras[0] == () and len(set(extras)) == len(extras)

    class FakeCache:  # what _GraphSession.__init__ reads
        tokens = torch.zeros(1, 4, dtype=torch.int64)

    dec = SimpleNamespace(token_embedding=SimpleNamespace(weight=torch.zeros(10, 2)))
    s = D._GraphSession(dec, FakeCache(), None, extras[2], "t")
    assert s._extra == extras[2]


# ----------------------------------------------------------------------------- the binding
def test_binding_of_the_two_entry_points():
    assert ctypes.sizeof(L.TsRules) == 12 and [f[0] for f in L.TsRules._fields_] == ["ts_begin", "no_timestamps", "max_initial"]
    assert L.SIGNATURES["wft_decode_pick_ts"][0]._type_ is L.DecodePickArgs and L.SIGNATURES["wft_decode_topk_ts"][0]._type_ is L.DecodeTopkArgs
    h = L.load()
    assert hasattr(h, "wft_decode_pick_ts") and hasattr(h, "wft_decode_topk_ts")
    # the existing structs keep their layout
    assert ctypes.sizeof(L.DecodePickArgs) == 128 and ctypes.sizeof(L.DecodeTopkArgs) == 88


# ----------------------------------------------------------------------------- the evaluator
class _Tok:
    """Duck-typed tokenizer: ids 0..25 -> letters, 26 -> blank; specials 90..94, timestamps 95.."""
    special_tokens = {"<|sot|>": 90, "<|eot|>": 91, "<|de|>": 92, "<|transcribe|>": 93, "<|notimestamps|>": 94, "<|0.00|>": 95, "<|0.02|>": 96}
    sot, eot, no_timestamps, timestamp_begin = 90, 91, 94, 95

    def decode(self, ids):
        assert all(0 <= i <= 26 for i in ids), ids
        return "".join(" " if i == 26 else chr(97 + i) for i in ids)

    def encode(self, text):
        return [26 if c == " " else ord(c) - 97 for c in text]


class _Stub(torch.nn.Module):
    V = 100

    def __init__(self, decoded):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.decoded, self.calls = decoded, []

    def forward(self, x, y_in):
        lg = torch.zeros(y_in.shape[0], y_in.shape[1], self.V)
        nxt = torch.cat([y_in[:, 1:], torch.full((y_in.shape[0], 1), 91)], 1)
        return lg.scatter(2, nxt[..., None], 8.0)

    def _run(self, prompt, prompt_len, eot, kw):
        self.calls.append(dict(kw, prompt=prompt.clone(), prompt_len=torch.as_tensor(prompt_len).tolist()))
        rows = [prompt[b, :int(prompt_len[b])].tolist() + self.decoded[b] + [eot] for b in range(prompt.shape[0])]
        n = max(len(r) for r in rows)
        return torch.tensor([r + [eot] * (n - len(r)) for r in rows]), torch.tensor([len(r) for r in rows]), torch.zeros(len(rows))

    def greedy_decode(self, mel, prompt, prompt_len, *, eot, **kw):
        return self._run(prompt, prompt_len, eot, dict(kw, kind="greedy"))

    def beam_decode(self, mel, prompt, prompt_len, *, eot, **kw):
        return self._run(prompt, prompt_len, eot, dict(kw, kind="beam"))


def _batch():
    text = [0, 1, 26, 2, 3]
    y_in = torch.tensor([[90, 92, 93, 94] + text + [91, 91, 91],        # <|notimestamps|> behind the task token
                         [7, 8, 9, 90, 92, 93, 95] + text[:4] + [96]])  # prompted, trained with timestamps
    y_out = torch.tensor([[92, 93, 94] + text + [91, -100, -100, -100],
                          [-100, -100, 90, 92, 93, 95] + text[:4] + [96, 91]])
    return torch.zeros(2, 80, 20), y_in, y_out


def test_prefix_stops_behind_the_task_token():
    assert decode_prefix_len([90, 92, 93, 94, 1, 2], 90, 94) == 4
    assert decode_prefix_len([90, 92, 93, 94, 1, 2], 90, 94, with_timestamps=True) == 3
    assert decode_prefix_len([7, 90, 92, 93, 95, 1], 90, 94, with_timestamps=True) == 4


@pytest.mark.parametrize("mode", ["greedy", "beam_search"])
def test_evaluator_decodes_with_timestamps(mode):
    cfg = {"mixed_precision_training": False, "wft_eval_decode": mode}
    decoded = [[95, 0, 1, 26, 2, 3, 96], [95, 0, 1, 26, 2, 96, 96, 4]]
    stub = _Stub(decoded)
    got = evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode_timestamps=True), tokenizer=_Tok())
    (call,) = stub.calls
    assert call["kind"] == ("greedy" if mode == "greedy" else "beam")
    assert call["prompt_len"] == [3, 6]                                  # <|notimestamps|> is not copied
    assert call["prompt"][0, :3].tolist() == [90, 92, 93] and call["prompt"][1].tolist() == [7, 8, 9, 90, 92, 93]
    assert call["suppress"] == [90, 92, 93, 94]                          # no timestamp id
    assert call["timestamp_begin"] == 95 and call["no_timestamps"] == 94 and "max_initial_timestamp_index" not in call
    # the timestamps never reach the text (the tokenizer stub asserts it): row 0 "ab cd" right, row 1 "ab ce" vs "ab c"
    assert got.num_samples == 2 and got.wer == pytest.approx(0.25)
    # absent or false: the call of today
    for off in ({}, {"wft_eval_decode_timestamps": False}):
        stub = _Stub([[0, 1], [2]])
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, **off), tokenizer=_Tok())
        (call,) = stub.calls
        assert call["prompt_len"] == [4, 6] and "timestamp_begin" not in call and "no_timestamps" not in call
        assert call["suppress"] == [90, 92, 93, 94, 95, 96]


def test_evaluator_key_validation():
    stub = _Stub([[0], [0]])
    with pytest.raises(ValueError, match="wft_eval_decode_timestamps"):
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", {"mixed_precision_training": False, "wft_eval_decode_timestamps": True},
                                          tokenizer=_Tok())
    with pytest.raises(ValueError, match="wft_eval_decode_timestamps"):
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", {"mixed_precision_training": False, "wft_eval_decode": "greedy",
                                                                    "wft_eval_decode_timestamps": "yes"}, tokenizer=_Tok())
    assert not stub.calls
    # false without a decoding mode is today's teacher-forced evaluation
    evaluator.evaluate_single_dataset(stub, [_batch()], "syn", {"mixed_precision_training": False, "wft_eval_decode_timestamps": False}, tokenizer=_Tok())
    assert not stub.calls
