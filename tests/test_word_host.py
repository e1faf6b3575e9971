"""Word timestamps on the host: the float64 reference of wft_word_spans (tests/_word_cases.py) against `D.alignment_words`, the
CPU proof that the checks of tests/test_word_spans_gpu.py bite (the kernel restated in numpy passes, every listed mutant of the
restatement is rejected), upstream's string rules (`merge_punctuations`, `add_word_timestamps`, the anomaly scores) on hand-worked
cases — one per branch — and the word-timestamp rules of the `transcribe` loop under scripted stand-ins for decode_with_fallback
and find_alignment (no device)."""
import numpy as np
import pytest

from tests import _word_cases as WC
from tests import test_transcribe_host as H
from whisper_finetune.engine import decode as D
from whisper_finetune.engine import transcribe as T

CASES = WC.cases()
EOT, TSB, NO_TS = H.EOT, H.TSB, H.NO_TS
ts = H.ts


# ============================================================================= the reference and its mutants
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_is_alignment_words(case):
    live = 0
    for b in range(case["B"]):
        ref = WC.spans_ref(case, b)
        L = int(case["path_len"][b])
        if ref is None:
            assert L == 0
            continue
        live += 1
        n_text = sum(case["counts"][b]) - 1
        at = int(case["tok_off"][b])
        tp = case["token_probs"][at:at + n_text]
        words = D.alignment_words(case["path_text"][b, :L], case["path_time"][b, :L], case["counts"][b], tp, list(range(n_text)))
        s, e, p, n = ref
        assert len(words) == len(s) == int(case["n_words"][b])
        for w, (ws, we, wp, ids) in enumerate(words):
            assert ws == int(s[w]) / D.TOKENS_PER_SECOND and we == int(e[w]) / D.TOKENS_PER_SECOND and len(ids) == int(n[w])
            assert abs(wp - p[w]) <= WC.prob_bound(p[w], n[w])
        assert e[-1] == case["path_time"][b, L - 1] or case["path_text"][b, L - 2] == case["path_text"][b, L - 1]
    assert live >= 1


def test_cases_hold_what_they_are_meant_to():
    by = {c["name"]: c for c in CASES}
    c = by["one_word_8_token_word_empty_path"]
    assert c["n_words"].tolist() == [1, 4, 2] and c["path_len"][2] == 0 and sorted(c["counts"][1][:-1]) == [1, 1, 1, 8]
    c = by["vertical_horizontal_runs_last_entry"]
    s, e, _, _ = WC.spans_ref(c, 0)
    assert (s == e).any() and (e - s > 3).any()                      # a word inside a vertical run, one over a horizontal run
    L = int(c["path_len"][0])
    assert c["path_text"][0, L - 1] != c["path_text"][0, L - 2] and e[-1] == c["path_time"][0, L - 1]   # first seen at the last entry
    c = by["probabilities_1e-30_to_1"]
    assert c["token_probs"].min() < 2e-30 and c["token_probs"].max() == 1.0
    c = by["path_beyond_one_chunk"]
    s, _, _, _ = WC.spans_ref(c, 0)
    assert c["path_len"][0] > 2048 and list(c["path_text"][0]).index(1) >= 2048
    for c in CASES:
        assert c["B"] == 3 and c["ld_words"] > c["n_words"].max()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restated_kernel_passes(case):
    worst = WC.check(case, *WC.restate(case))
    print(f"{case['name']}: worst |err| / bound {worst:.3f}")
    WC.check(case, *WC.restate(case, dtype=np.float64))


@pytest.mark.parametrize("mutant", WC.MUTANTS)
def test_mutants_are_rejected(mutant):
    caught = []
    for case in CASES:
        try:
            WC.check(case, *WC.restate(case, mutant))
        except AssertionError:
            caught.append(case["name"])
    print(f"{mutant}: rejected on {caught}")
    assert caught, f"no case rejects the mutant {mutant}"


def test_untouched_buffers_and_a_stray_write_are_told_apart():
    case = CASES[0]
    start, end, prob = WC.restate(case)
    prob[2, 0] = 0.5                                   # the audio with the empty path
    with pytest.raises(AssertionError):
        WC.check(case, start, end, prob)
    start, end, prob = WC.restate(case)
    end[0, int(case["n_words"][0])] = 3                # one element beyond n_words
    with pytest.raises(AssertionError):
        WC.check(case, start, end, prob)


# ============================================================================= merge_punctuations
def _w(word, start=0.0, end=0.0, p=0.9, tokens=None):
    return {"word": word, "tokens": [abs(hash(word)) % 1000] if tokens is None else tokens, "start": start, "end": end, "probability": p}


def test_defaults_are_upstreams():
    assert D.PREPEND_PUNCTUATIONS == "\"'“¿([{-" and D.APPEND_PUNCTUATIONS == "\"'.。,，!！?？:：”)]}、"


def test_a_chain_of_prepended_marks_and_an_appended_one():
    words = [_w(" (", 0.0, 0.1, tokens=[1]), _w(" \"", 0.1, 0.2, tokens=[2]), _w("hello", 0.2, 0.6, tokens=[3, 4]), _w(",", 0.6, 0.7, tokens=[5]),
             _w(" world", 0.7, 1.0, tokens=[6])]
    times = [(w["start"], w["end"], w["probability"]) for w in words]
    D.merge_punctuations(words)
    assert [w["word"] for w in words] == ["", "", " ( \"hello,", "", " world"]
    assert [w["tokens"] for w in words] == [[], [], [1, 2, 3, 4, 5], [], [6]]
    assert [(w["start"], w["end"], w["probability"]) for w in words] == times      # times and probabilities are not touched


def test_no_append_behind_a_word_that_ends_in_a_space_and_no_prepend_without_the_leading_space():
    words = [_w("hello ", tokens=[1]), _w(".", tokens=[2]), _w("(", tokens=[3]), _w(" x", tokens=[4])]
    D.merge_punctuations(words)
    assert [w["word"] for w in words] == ["hello ", ".", "(", " x"] and [w["tokens"] for w in words] == [[1], [2], [3], [4]]
    words = [_w(" a", tokens=[1]), _w("!", tokens=[2]), _w("?", tokens=[3])]
    D.merge_punctuations(words, "", "!")            # caller's sets: "?" is no mark here
    assert [w["word"] for w in words] == [" a!", "", "?"]


# ============================================================================= add_word_timestamps
def _seg(start, end, ids, seek=0):
    return {"seek": seek, "start": start, "end": end, "tokens": [TSB] + list(ids) + [TSB + 1]}


def _awt(segments, alignment, **kw):
    args = dict(time_offset=0.0, last_speech_timestamp=0.0, eot=EOT)
    args.update(kw)
    return D.add_word_timestamps(segments, alignment, **args)


def _times(seg):
    return [(w["word"], w["start"], w["end"]) for w in seg["words"]]


def test_sentence_mark_clamps():
    # durations .2 .2 1.6 1.5 .2 1.3 .2 .2: median 0.2, max_duration 0.4
    al = [_w(" a", 0.0, 0.2, tokens=[1]), _w(" b", 0.2, 0.4, tokens=[2]), _w(".", 0.4, 2.0, tokens=[3]), _w(" c", 2.0, 3.5, tokens=[4]),
          _w(" d", 3.5, 3.7, tokens=[5]), _w(" e", 3.7, 5.0, tokens=[6]), _w(" f", 5.0, 5.2, tokens=[7]), _w(" g", 5.2, 5.4, tokens=[8])]
    seg = _seg(0.0, 5.4, range(1, 9))
    last = _awt([seg], al)
    # "." is long and a mark: end = start + 0.4 (its times stay with the emptied word; " b." keeps " b"'s times);
    # " c" is long behind a mark: start = end - 0.4; " e" is long but next to no mark: untouched
    assert (al[2]["start"], round(al[2]["end"], 9)) == (0.4, 0.8) and al[2]["word"] == ""
    assert _times(seg) == [(" a", 0.0, 0.2), (" b.", 0.2, 0.4), (" c", 3.1, 3.5), (" d", 3.5, 3.7), (" e", 3.7, 5.0), (" f", 5.0, 5.2), (" g", 5.2, 5.4)]
    assert seg["words"][1]["tokens"] == [2, 3] and (seg["start"], seg["end"], last) == (0.0, 5.4, 5.4)


def test_word_0_is_not_clamped_and_no_durations_means_no_clamp():
    al = [_w(".", 0.0, 3.0, tokens=[1]), _w(" b", 3.0, 3.2, tokens=[2]), _w(" c", 3.2, 3.4, tokens=[3])]
    seg = _seg(0.0, 3.4, [1, 2, 3])
    _awt([seg], al, last_speech_timestamp=3.0)
    assert _times(seg)[0] == (".", 0.0, 3.0)
    al = [_w(" a", 1.0, 1.0, tokens=[1]), _w(".", 1.0, 1.0, tokens=[2])]     # every duration is zero: median 0.0
    seg = _seg(0.0, 2.0, [1, 2])
    assert _awt([seg], al) == 1.0 and _times(seg) == [(" a.", 1.0, 1.0)] and (seg["start"], seg["end"]) == (1.0, 1.0)


def _pause_words(first, second):
    return [_w(" x", *first, tokens=[1]), _w(" y", *second, tokens=[2]), _w(" z", 5.2, 5.4, tokens=[3]), _w(" q", 5.4, 5.6, tokens=[4]),
            _w(" r", 5.6, 5.8, tokens=[5])]


def test_pause_rule_first_word_long():
    seg = _seg(12.0, 15.8, [1, 2, 3, 4, 5])
    last = _awt([seg], _pause_words((2.0, 5.0), (5.0, 5.2)), time_offset=10.0)          # median 0.2, max_duration 0.4; pause 15.0 > 0.8
    assert _times(seg)[:2] == [(" x", 14.6, 15.0), (" y", 15.0, 15.2)]                    # w0.start = w0.end - 0.4; w1 is short: no boundary
    assert (seg["start"], seg["end"], last) == (14.6, 15.8, 15.8)                        # (b) else, (c) else


def test_pause_rule_second_word_long_moves_the_boundary():
    seg = _seg(12.0, 15.8, [1, 2, 3, 4, 5])
    _awt([seg], _pause_words((2.0, 2.2), (2.2, 5.2)), time_offset=10.0)
    # w0 is short, but w1.end - w0.start = 3.2 > 0.8; w1 is long: boundary = max(15.2 / 2, 15.2 - 0.4) = 14.8
    # (max_duration is twice a median of float differences, 0.4 to an ulp: the moved times are compared to 1e-9)
    ap = lambda v: pytest.approx(v, abs=1e-9)
    assert _times(seg)[:2] == [(" x", ap(14.4), ap(14.8)), (" y", ap(14.8), 15.2)] and seg["start"] == ap(14.4)
    assert seg["words"][0]["end"] == seg["words"][1]["start"]


def test_pause_rule_needs_the_pause_and_a_long_word():
    seg = _seg(12.0, 15.8, [1, 2, 3, 4, 5])
    _awt([seg], _pause_words((2.0, 5.0), (5.0, 5.2)), time_offset=10.0, last_speech_timestamp=14.5)   # 15.0 - 14.5 <= 0.8: no pause
    assert _times(seg)[0] == (" x", 12.0, 15.0) and seg["start"] == 12.0
    seg = _seg(12.0, 15.8, [1, 2, 3, 4, 5])
    _awt([seg], _pause_words((4.8, 5.0), (5.0, 5.2)), time_offset=10.0)                                # a pause, but no long word
    assert _times(seg)[:2] == [(" x", 14.8, 15.0), (" y", 15.0, 15.2)]


def test_segment_start_rule_both_ways():
    def run(seg_start):
        seg = _seg(seg_start, 15.8, [1, 2, 3, 4, 5])
        _awt([seg], _pause_words((2.0, 5.0), (5.0, 5.2)), time_offset=10.0, last_speech_timestamp=14.9)   # no pause: (a) is off
        return seg

    seg = run(14.0)        # 14.0 < w0.end = 15.0 and 13.5 > w0.start = 12.0: w0.start = min(15.0 - 0.2, 14.0); the segment keeps its start
    assert _times(seg)[0] == (" x", 14.0, 15.0) and seg["start"] == 14.0
    seg = run(14.95)       # ... = min(14.8, 14.95): the median keeps the word from collapsing
    assert _times(seg)[0] == (" x", pytest.approx(14.8), 15.0) and seg["start"] == 14.95
    seg = run(12.4)        # 11.9 > 12.0 fails: the segment takes the word's start
    assert _times(seg)[0] == (" x", 12.0, 15.0) and seg["start"] == 12.0
    seg = run(15.5)        # seg.start < w0.end fails
    assert _times(seg)[0] == (" x", 12.0, 15.0) and seg["start"] == 12.0


def test_segment_end_rule_both_ways():
    def run(seg_end):
        al = [_w(" x", 2.0, 2.2, tokens=[1]), _w(" y", 2.2, 2.4, tokens=[2]), _w(" z", 2.4, 2.6, tokens=[3]), _w(" q", 2.6, 5.6, tokens=[4])]
        seg = _seg(12.0, seg_end, [1, 2, 3, 4])
        return seg, _awt([seg], al, time_offset=10.0, last_speech_timestamp=12.0)

    seg, last = run(13.0)   # 13.0 > wl.start = 12.6 and 13.5 < wl.end = 15.6: wl.end = max(12.6 + 0.2, 13.0)
    assert _times(seg)[-1] == (" q", 12.6, 13.0) and (seg["end"], last) == (13.0, 13.0)
    seg, last = run(12.7)   # ... = max(12.8, 12.7)
    assert _times(seg)[-1] == (" q", 12.6, pytest.approx(12.8)) and (seg["end"], last) == (12.7, 12.7)
    seg, last = run(15.4)   # 15.9 < 15.6 fails: the segment takes the word's end
    assert _times(seg)[-1] == (" q", 12.6, 15.6) and (seg["end"], last) == (15.6, 15.6)
    seg, last = run(12.5)   # seg.end > wl.start fails
    assert _times(seg)[-1] == (" q", 12.6, 15.6) and seg["end"] == 15.6


def test_words_are_dealt_to_the_segments_by_token_count():
    al = [_w(" (", 0.0, 0.2, tokens=[1]), _w(" ab", 0.2, 0.6, tokens=[2, 3]), _w(" c", 0.6, 1.0, tokens=[4]), _w(",", 1.0, 1.2, tokens=[5]),
          _w(" d", 1.2, 1.6, tokens=[6])]
    segs = [_seg(0.0, 0.6, [1, 2, 3]), {"seek": 0, "start": 0.6, "end": 0.6, "tokens": [TSB, TSB]}, _seg(0.6, 1.6, [4, 5, 6])]
    last = _awt(segs, al, time_offset=100.0)
    assert _times(segs[0]) == [(" ( ab", 100.2, 100.6)] and segs[0]["words"][0]["tokens"] == [1, 2, 3]   # the emptied " (" is taken, not kept
    assert segs[1]["words"] == [] and (segs[1]["start"], segs[1]["end"]) == (0.6, 0.6)                    # no text token: no words, times stay
    assert _times(segs[2]) == [(" c,", 100.6, 101.0), (" d", 101.2, 101.6)] and last == 101.6
    assert D.add_word_timestamps([], [], time_offset=0.0, last_speech_timestamp=7.0) == 7.0


# ============================================================================= the anomaly scores
def test_word_anomaly_score_thresholds():
    assert D.word_anomaly_score(_w("a", 0.0, 1.0, p=0.15)) == 0.0 and D.word_anomaly_score(_w("a", 0.0, 1.0, p=0.1499)) == 1.0
    assert D.word_anomaly_score(_w("a", 1.0, 1.133, p=0.9)) == pytest.approx(0.0, abs=1e-12)
    assert D.word_anomaly_score(_w("a", 1.0, 1.033, p=0.9)) == pytest.approx(1.5)
    assert D.word_anomaly_score(_w("a", 0.0, 2.0, p=0.9)) == 0.0 and D.word_anomaly_score(_w("a", 0.0, 3.0, p=0.9)) == 1.0
    assert D.word_anomaly_score(_w("a", 0.0, 3.5, p=0.0)) == 2.5


def test_is_segment_anomaly_thresholds():
    bad, good = _w(" bad", 0.0, 1.0, p=0.1), _w(" good", 0.0, 1.0, p=0.9)      # scores 1.0 and 0.0
    assert not D.is_segment_anomaly(None) and not D.is_segment_anomaly({"words": []}) and not D.is_segment_anomaly({})
    assert D.is_segment_anomaly({"words": [bad, bad, bad, good, good]})                    # score 3 >= 3
    assert not D.is_segment_anomaly({"words": [bad, bad, good, good]})                    # 2 < 3 and 2.01 < 4
    assert D.is_segment_anomaly({"words": [bad, bad]}) and D.is_segment_anomaly({"words": [bad]})    # score + 0.01 >= the word count
    assert not D.is_segment_anomaly({"words": [bad, good]})
    almost = _w(" x", 0.0, 2.995, p=0.9)                                                 # score 0.995: 0.995 + 0.01 >= 1
    assert D.is_segment_anomaly({"words": [almost]}) and not D.is_segment_anomaly({"words": [_w(" x", 0.0, 2.98, p=0.9)]})
    marks = [_w(",", 0.0, 0.0, p=0.0), _w(" (", 0.0, 0.0, p=0.0)]
    assert D.is_segment_anomaly({"words": marks + [bad, good]})                          # " (" is no mark (the space), "," is: 3.995 >= 3
    assert not D.is_segment_anomaly({"words": [_w(",", 0.0, 0.0, p=0.0), good, good]})    # the mark's own score does not count
    assert not D.is_segment_anomaly({"words": [good] * 8 + [bad] * 5})                    # only the first 8 words count


# ============================================================================= the transcribe loop, scripted
TIMES = {}   # text id -> (start, end, probability) inside its window


def _split(ids):
    return [f" w{t}" for t in ids[:-1]] + ["<eot>"], [[t] for t in ids]


class _Align:
    """find_alignment's stand-in: one word per id with the times of TIMES, every call recorded."""

    def __init__(self):
        self.calls = []

    def __call__(self, model, mel, text_tokens, **kw):
        self.calls.append(dict(texts=[list(t) for t in text_tokens], **kw))
        assert mel is None and kw["_xa"] is None and kw["word_spans"] == "device" and kw["eot"] == EOT and kw["no_timestamps"] == NO_TS
        assert [[1] * (len(t) + 1) for t in text_tokens] == kw["word_token_counts"]
        return [[TIMES[t][:2] + (TIMES[t][2], [t]) for t in text] for text in text_tokens]


def _run(script, frames, **kw):
    stand, align = H._Stand(script), _Align()
    args = dict(sot_sequence=H.SOTS[0], eot=EOT, timestamp_begin=TSB, no_timestamps=NO_TS, sample_len=12, word_timestamps=True,
                split_words=_split, _decode=stand, _align=align, _frames=[frames])
    args.update(kw)
    return T.transcribe(H._Model(), [None], **args)[0], stand, align


TIMES.update({11: (0.4, 0.8, 0.9), 12: (0.8, 1.2, 0.9), 13: (10.2, 10.6, 0.9), 14: (1.0, 1.4, 0.9), 15: (0.2, 0.6, 0.9), 16: (0.6, 1.0, 0.9),
              17: (3.0, 3.4, 0.9)})
SEEK_SCRIPT = [
    [(0, [ts(0), 11, 12, ts(10), ts(10), 13, ts(20), ts(20)], 0.0, 0.01, -0.3)],   # ends on a pair: seek -> the last word end, 10.6 s
    [(0, [ts(0), 14, ts(5)], 0.0, 0.01, -0.3)],                                    # a single ending timestamp: seek += 3000
    [(0, [ts(0), 15, 16], 0.0, 0.01, -0.3)],                                       # no timestamp at the end: seek -> 40.6 + 1.0 s
    [(0, [ts(0), 17, ts(18.4)], 0.0, 0.01, -0.3)],                                 # single ending: done
]


def test_seek_goes_to_the_last_word_end_unless_the_window_ends_on_a_single_timestamp():
    res, stand, align = _run(SEEK_SCRIPT, 6000)
    assert res["windows"] == 4 and not res["truncated"] and len(align.calls) == 4
    segs = res["segments"]
    assert [s["seek"] for s in segs] == [0, 0, 1060, 4060, 4160]
    assert [c["num_frames"] for c in align.calls] == [[3000], [3000], [1940], [1840]]
    assert [c["texts"] for c in align.calls] == [[[11, 12, 13]], [[14]], [[15, 16]], [[17]]] and align.calls[0]["sot_sequence"] == H.SOTS[0]
    # window 0: both segments shrink to their words (rules (b) and (c), else branches)
    assert [(s["start"], s["end"]) for s in segs[:2]] == [(0.4, 1.2), (10.2, 10.6)]
    assert [[(w["word"], w["tokens"], w["start"], w["end"], w["probability"]) for w in s["words"]] for s in segs[:2]] == \
        [[(" w11", [11], 0.4, 0.8, 0.9), (" w12", [12], 0.8, 1.2, 0.9)], [(" w13", [13], 10.2, 10.6, 0.9)]]
    # window 1 at 10.6 s: the word times carry the offset
    assert [(w["start"], w["end"]) for w in segs[2]["words"]] == [(11.6, 12.0)]
    assert [(w["start"], w["end"]) for w in segs[3]["words"]] == [(40.8, 41.2), (41.2, 41.6)]
    assert res["tokens"] == [t for s in segs for t in s["tokens"]]
    # the same script without word timestamps goes 0 -> 2000: the seek differs, and no alignment runs
    align = _Align()
    res = T.transcribe(H._Model(), [None], sot_sequence=H.SOTS[0], eot=EOT, timestamp_begin=TSB, no_timestamps=NO_TS, sample_len=12,
                       split_words=_split, max_windows=1, _decode=H._Stand(SEEK_SCRIPT), _align=align, _frames=[6000])[0]
    assert align.calls == [] and all("words" not in s for s in res["segments"]) and [(s["start"], s["end"]) for s in res["segments"]] == [(0.0, 10.0), (10.0, 20.0)]


def test_hallucination_rule_on_the_remaining_window():
    # window 0 of SEEK_SCRIPT: 30.0 - 10.6 s are left behind the last word
    res, _, _ = _run(SEEK_SCRIPT[:1], 6000, max_windows=1, hallucination_silence_threshold=2.0)
    assert len(res["segments"]) == 2 and res["truncated"]
    res2, stand, _ = _run(SEEK_SCRIPT[:1] + [[(0, [ts(0), 14, ts(5)], 0.0, 0.01, -0.3)]], 6000, max_windows=2, hallucination_silence_threshold=2.0)
    assert [s["seek"] for s in res2["segments"]] == [0, 0, 1060]                       # 19.4 s > 2 s: the seek stays at the last word end
    res3, _, _ = _run(SEEK_SCRIPT[:1] + [[(0, [ts(0), 14, ts(5)], 0.0, 0.01, -0.3)]], 6000, max_windows=2, hallucination_silence_threshold=25.0)
    assert [s["seek"] for s in res3["segments"]] == [0, 0, 3000]                       # 19.4 s <= 25 s: previous seek + segment_size


TIMES.update({21: (5.0, 5.05, 0.05), 22: (5.05, 5.1, 0.05), 23: (0.4, 0.8, 0.9)})


def test_an_anomalous_first_segment_behind_a_silence_emits_nothing():
    script = [[(0, [ts(5), 21, 22, ts(6)], 0.0, 0.01, -0.3)], [(0, [ts(0), 23, ts(29)], 0.0, 0.01, -0.3)]]
    res, stand, align = _run(script, 3400, hallucination_silence_threshold=2.0)
    assert res["windows"] == 2 and len(align.calls) == 2
    assert [s["seek"] for s in res["segments"]] == [500] and res["tokens"] == [ts(0), 23, ts(29)]     # gap 5.0 s > 2 s: seek 0 -> 500
    assert stand.calls[1]["prompts"] == [H.SOTS[0]]                                                  # nothing of window 0 joined the history
    # without the threshold the same window is kept (a single ending timestamp: seek 0 -> 3000)
    res, _, _ = _run(script[:1] + [[(0, [ts(0), 23, ts(3)], 0.0, 0.01, -0.3)]], 3400, sot_prev=H.SOT_PREV)
    assert [s["seek"] for s in res["segments"]] == [0, 3000] and [w["word"] for w in res["segments"][0]["words"]] == [" w21", " w22"]
    assert (res["segments"][0]["start"], res["segments"][0]["end"]) == (5.0, 5.1)


TIMES.update({31: (0.2, 0.6, 0.9), 32: (0.6, 1.0, 0.9), 33: (1.0, 1.4, 0.9), 34: (10.0, 10.05, 0.05), 35: (10.05, 10.1, 0.05), 36: (20.0, 20.4, 0.9)})
HAL_WINDOW = [(0, [ts(0), 31, 32, 33, ts(2), ts(10), 34, 35, ts(10.2), ts(20), 36, ts(21), ts(21)], 0.0, 0.01, -0.3)]


def test_an_anomalous_segment_between_silences_is_dropped_with_what_follows():
    res, _, _ = _run([HAL_WINDOW, [(0, [ts(0), 23, ts(29)], 0.0, 0.01, -0.3)]], 6000, max_windows=2, hallucination_silence_threshold=2.0)
    segs = res["segments"]
    assert [s["seek"] for s in segs] == [0, 1000]                    # seek = max(0 + 1, 10.0) s; the segments at 10 s and 20 s are gone
    assert [w["word"] for w in segs[0]["words"]] == [" w31", " w32", " w33"] and (segs[0]["start"], segs[0]["end"]) == (0.2, 1.4)
    # less than the threshold of content behind the dropped segment: the recording is finished
    res, _, _ = _run([HAL_WINDOW], 1100, hallucination_silence_threshold=2.0)
    assert res["windows"] == 1 and not res["truncated"] and len(res["segments"]) == 1
    # without the threshold all three segments stay and the seek goes to the last word end, 20.4 s
    res, _, _ = _run([HAL_WINDOW, [(0, [ts(0), 23, ts(29)], 0.0, 0.01, -0.3)]], 6000, max_windows=2)
    assert [s["seek"] for s in res["segments"]] == [0, 0, 0, 2040]
    # a neighbour that speaks right behind it: no silence after, the segment stays
    TIMES[36] = (10.5, 10.9, 0.9)
    try:
        res, _, _ = _run([HAL_WINDOW], 6000, max_windows=1, hallucination_silence_threshold=2.0)
    finally:
        TIMES[36] = (20.0, 20.4, 0.9)
    assert len(res["segments"]) == 3


def test_rows_without_text_and_two_sot_sequences():
    script = [[(0, [ts(0), 11, ts(1)], 0.0, 0.01, -0.3), (1, [ts(0), ts(1)], 0.0, 0.01, -0.3), (2, [ts(0), 12, ts(1)], 0.0, 0.01, -0.3)]]
    stand, align = H._Stand(script), _Align()
    res = T.transcribe(H._Model(), [None] * 3, sot_sequence=H.SOTS, eot=EOT, timestamp_begin=TSB, no_timestamps=NO_TS, sample_len=12,
                       word_timestamps=True, split_words=_split, _decode=stand, _align=align, _frames=[900, 900, 900])
    assert [c["sot_sequence"] for c in align.calls] == [H.SOTS[0], H.SOTS[2]]      # one call per distinct sequence, none for the empty row
    assert res[1]["segments"][0]["words"] == [] and res[0]["segments"][0]["words"][0]["word"] == " w11"
    same = [H.SOTS[0][:3] + [H.MARK + a] for a in range(3)]
    assert same == H.SOTS   # (the stand-in reads the row from the last id, so the sequences differ; one shared sequence: one call)
    script = [[(0, [ts(0), 11, ts(1)], 0.0, 0.01, -0.3)]]
    res, _, align = _run(script, 900)
    assert len(align.calls) == 1


def test_argument_errors():
    kw = dict(sot_sequence=H.SOTS[0], eot=EOT, _frames=[900], _decode=H._Stand(), _align=_Align())
    with pytest.raises(ValueError):
        T.transcribe(H._Model(), [None], word_timestamps=True, timestamp_begin=TSB, no_timestamps=NO_TS, **kw)          # no split_words
    with pytest.raises(ValueError):
        T.transcribe(H._Model(), [None], word_timestamps=True, split_words=_split, no_timestamps=NO_TS, **kw)           # no timestamp_begin
    with pytest.raises(ValueError):
        T.transcribe(H._Model(), [None], word_timestamps=True, split_words=_split, timestamp_begin=TSB, **kw)           # no no_timestamps
    with pytest.raises(ValueError):
        T.transcribe(H._Model(), [None], hallucination_silence_threshold=2.0, timestamp_begin=TSB, no_timestamps=NO_TS, **kw)
    assert kw["_decode"].calls == [] and kw["_align"].calls == []


def test_advance_window_reports_the_single_ending():
    toks = [ts(0), 1, ts(2), ts(2), 2, ts(3)]
    assert T.advance_window(toks, seek=1000, segment_size=3000, timestamp_begin=TSB, return_single_ending=True)[1:] == (4000, True)
    assert T.advance_window(toks + [ts(3)], seek=0, segment_size=3000, timestamp_begin=TSB, return_single_ending=True)[1:] == (300, False)
    assert T.advance_window([ts(0), 1, 2], seek=0, segment_size=3000, timestamp_begin=TSB, return_single_ending=True)[1:] == (3000, False)
    assert len(T.advance_window(toks, seek=0, segment_size=3000, timestamp_begin=TSB)) == 2
