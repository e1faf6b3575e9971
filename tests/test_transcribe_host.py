"""Long-form transcription on the host (engine/transcribe.py): the pure functions `advance_window` and `window_prompt` on hand-worked
cases, the loop of `transcribe` driven by scripted stand-ins for decode_with_fallback and detect_language (no device, no mel), and
the CPU proof that the checks of tests/test_transcribe_kernels_gpu.py bite: the kernels of csrc/transcribe.hip restated in numpy
meet the bounds of tests/_transcribe_cases.py, and every listed mutant of the restatements is rejected."""
import numpy as np
import pytest
import torch

from tests import _transcribe_cases as TC
from whisper_finetune.engine import transcribe as T

TSB = 50364
EOT = 50257
SOT, LANG, TRANSCRIBE, SOT_PREV, NO_SPEECH, NO_TS = 50258, 50259, 50359, 50361, 50362, 50363
MARK = 100  # the last id of recording a's sot_sequence is MARK + a: the stand-in reads the batch composition from the prompts


def ts(seconds: float) -> int:
    return TSB + round(seconds / 0.02)


def _units(x: float) -> int:
    """seconds -> units of 0.02 s; asserts that x is such a multiple to 1e-9"""
    u = round(x / 0.02)
    assert abs(x - u * 0.02) < 1e-9, x
    return u


def _spans(segments):
    return [(_units(s["start"]), _units(s["end"]), s["tokens"]) for s in segments]


# ============================================================================= advance_window
def test_two_pairs_and_the_row_ends_on_a_pair():
    toks = [ts(0), 11, 12, ts(10), ts(10), 13, ts(20), ts(20)]
    segs, seek = T.advance_window(toks, seek=0, segment_size=3000, timestamp_begin=TSB)
    assert _spans(segs) == [(0, 500, toks[0:4]), (500, 1000, toks[4:7])]
    assert seek == 2000 and all(s["seek"] == 0 for s in segs)      # 20.00 s = 1000 timestamp steps = 2000 frames; the last id is dropped


def test_a_pair_and_a_single_ending_timestamp():
    toks = [ts(0), 1, ts(2), ts(2), 2, ts(3)]
    segs, seek = T.advance_window(toks, seek=1000, segment_size=3000, timestamp_begin=TSB)
    assert _spans(segs) == [(500, 600, toks[0:3]), (600, 650, toks[3:6])]   # offset 10.00 s
    assert seek == 4000


def test_no_pair_and_a_final_timestamp_other_than_zero():
    toks = [ts(0), 1, 2, ts(7.5)]
    segs, seek = T.advance_window(toks, seek=200, segment_size=3000, timestamp_begin=TSB)
    assert _spans(segs) == [(100, 100 + 375, toks)] and seek == 3200


def test_no_pair_and_only_the_zero_timestamp_in_a_row_cut_without_eot():
    toks = [ts(0), 1, 2, 3]
    segs, seek = T.advance_window(toks, seek=0, segment_size=3000, timestamp_begin=TSB)
    assert _spans(segs) == [(0, 1500, toks)] and seek == 3000      # the whole window: 30.00 s


def test_empty_tokens_give_one_empty_segment_over_the_window():
    segs, seek = T.advance_window([], seek=600, segment_size=3000, timestamp_begin=TSB)
    assert _spans(segs) == [(300, 1800, [])] and seek == 3600


def test_without_timestamps_no_id_is_a_timestamp():
    toks = [TSB + 5, TSB + 5, 1]
    segs, seek = T.advance_window(toks, seek=3000, segment_size=3000, timestamp_begin=None)
    assert _spans(segs) == [(1500, 3000, toks)] and seek == 6000


def test_the_zero_advance_guard_steps_over_the_window():
    toks = [ts(0), ts(0)]
    segs, seek = T.advance_window(toks, seek=1200, segment_size=3000, timestamp_begin=TSB)
    assert _spans(segs) == [(600, 600, [ts(0)])]                  # upstream: new_seek = 1200 + 0, the same window for ever
    assert seek == 4200


def test_the_last_window_of_a_recording_is_shorter():
    toks = [ts(0), 1, 2]
    segs, seek = T.advance_window(toks, seek=3000, segment_size=100, timestamp_begin=TSB)
    assert _spans(segs) == [(1500, 1550, toks)] and seek == 3100  # 1.00 s of content
    toks = [ts(0), 1, ts(4), ts(4)]
    segs, seek = T.advance_window(toks, seek=3000, segment_size=1700, timestamp_begin=TSB)
    assert _spans(segs) == [(1500, 1700, toks[:3])] and seek == 3400   # a pair moves the seek by its time, not by the window


def test_advance_window_rejects_an_empty_window():
    with pytest.raises(ValueError):
        T.advance_window([1], seek=0, segment_size=0, timestamp_begin=TSB)


# ============================================================================= window_prompt
SOT_SEQ = [SOT, LANG, TRANSCRIBE]


def test_prompt_without_history():
    assert T.window_prompt([], 0, SOT_SEQ, SOT_PREV, 448) == (SOT_SEQ, 0)


def test_prompt_with_a_short_history():
    hist = list(range(1, 11))
    assert T.window_prompt(hist, 0, SOT_SEQ, SOT_PREV, 448) == ([SOT_PREV] + hist + SOT_SEQ, 11)


def test_prompt_keeps_only_the_tail_of_a_long_history():
    hist = list(range(1000, 1300))
    prompt, idx = T.window_prompt(hist, 0, SOT_SEQ, SOT_PREV, 448)
    assert prompt == [SOT_PREV] + hist[-223:] + SOT_SEQ and idx == 224 and prompt[idx] == SOT   # n_text_ctx // 2 - 1 = 223


def test_prompt_reset_in_the_middle():
    hist = list(range(1, 11))
    assert T.window_prompt(hist, 6, SOT_SEQ, SOT_PREV, 448) == ([SOT_PREV] + hist[6:] + SOT_SEQ, 5)
    assert T.window_prompt(hist, 10, SOT_SEQ, SOT_PREV, 448) == (SOT_SEQ, 0)


def test_prompt_without_sot_prev():
    assert T.window_prompt(list(range(1, 11)), 0, SOT_SEQ, None, 448) == (SOT_SEQ, 0)


# ============================================================================= the loop, scripted
class _Dims:
    n_text_ctx, n_vocab, n_mels = 448, 51865, 80


class _Model:
    """What transcribe() touches of a model when the stand-ins decode."""
    dims, compute_dtype, training = _Dims(), "bf16", False

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode


FRAMES = [4700, 3100, 900]
SOTS = [[SOT, LANG, TRANSCRIBE, MARK + a] for a in range(3)]
# SCRIPT[i] = the rows of iteration i in batch order: (recording, generated ids, temperature, no_speech_prob, avg_logprob)
SCRIPT = [
    [(0, [ts(0), 11, 12, ts(10), ts(10), 13, ts(20), ts(20)], 0.0, 0.01, -0.3),   # two pairs: seek 0 -> 2000
     (1, [ts(0), 31, ts(1)], 0.0, 0.9, -2.0),                                     # silence: skipped, seek 0 -> 3000
     (2, [ts(0), 21, ts(5)], 0.0, 0.9, -0.5)],                                    # silence, but avg_logprob > -1: kept, done
    [(0, [ts(0), 14, ts(4), ts(4)], 0.8, 0.01, -0.9),                             # a pair: seek 2000 -> 2400; temperature > 0.5: reset
     (1, [ts(0), 31, 32], 0.0, 0.02, -0.2)],                                      # the last 100 frames: done
    [(0, [ts(0), 15, ts(23)], 0.0, 0.01, -0.1)],                                  # seek 2400 -> 4700: done
]


class _Stand:
    """decode_with_fallback's stand-in: plays SCRIPT, records every call."""

    def __init__(self, script=SCRIPT):
        self.script, self.calls = script, []

    def __call__(self, model, mel, prompt, prompt_len, **kw):
        i = len(self.calls)
        plen = [int(v) for v in prompt_len.tolist()]
        prompts = [prompt[j, :plen[j]].tolist() for j in range(prompt.shape[0])]
        assert mel is None and (prompt[:, :] == EOT).sum() == sum(prompt.shape[1] - p for p in plen)   # right-padded with eot
        self.calls.append(dict(rows=[p[-1] - MARK for p in prompts], prompts=prompts, sot_index=list(kw["sot_index"]), seed=kw["seed"],
                               max_len=kw["max_len"], kw=kw))
        rows = self.script[i]
        assert [r[0] for r in rows] == self.calls[-1]["rows"], f"iteration {i}: batch {self.calls[-1]['rows']}"
        full = [prompts[j] + list(rows[j][1]) + [EOT] for j in range(len(rows))]
        width = max(len(f) for f in full)
        toks = torch.tensor([f + [EOT] * (width - len(f)) for f in full], dtype=torch.int64)
        info = {"temperature": [r[2] for r in rows], "no_speech_prob": [r[3] for r in rows], "avg_logprob": [r[4] for r in rows],
                "compression_ratio": [None] * len(rows)}
        return toks, torch.tensor([len(f) for f in full]), torch.zeros(len(rows)), info


def _run(stand=None, **kw):
    stand = _Stand() if stand is None else stand
    args = dict(sot_sequence=SOTS, eot=EOT, timestamp_begin=TSB, no_timestamps=NO_TS, sot_prev=SOT_PREV, no_speech=NO_SPEECH, seed=40,
                sample_len=12, _decode=stand, _frames=FRAMES)
    args.update(kw)
    return T.transcribe(_Model(), [None, None, None], **args), stand


def test_loop_batches_rows_drop_out_and_seeds():
    res, stand = _run()
    assert [c["rows"] for c in stand.calls] == [[0, 1, 2], [0, 1], [0]]
    assert [c["seed"] for c in stand.calls] == [40, 41, 42]
    assert [r["windows"] for r in res] == [3, 2, 1] and not any(r["truncated"] for r in res)
    assert all(r["language"] is None and r["language_probs"] is None for r in res)
    # iteration 0: no history, the prompts are the sot sequences; max_len = widest prompt + sample_len
    assert stand.calls[0]["prompts"] == SOTS and stand.calls[0]["sot_index"] == [0, 0, 0] and stand.calls[0]["max_len"] == 4 + 12
    for c in stand.calls:
        assert c["kw"]["timestamp_begin"] == TSB and c["kw"]["no_timestamps"] == NO_TS and c["kw"]["no_speech"] == NO_SPEECH and c["kw"]["eot"] == EOT


def test_loop_segments_and_seeks():
    res, _ = _run()
    g0 = SCRIPT[0][0][1]
    assert [(s["seek"],) + t for s, t in zip(res[0]["segments"], _spans(res[0]["segments"]))] == [
        (0, 0, 500, g0[0:4]), (0, 500, 1000, g0[4:7]), (2000, 1000, 1200, SCRIPT[1][0][1][:3]), (2400, 1200, 2350, SCRIPT[2][0][1])]
    assert res[0]["tokens"] == g0[0:4] + g0[4:7] + SCRIPT[1][0][1][:3] + SCRIPT[2][0][1]
    assert [s["temperature"] for s in res[0]["segments"]] == [0.0, 0.0, 0.8, 0.0]
    assert [s["avg_logprob"] for s in res[0]["segments"]] == [-0.3, -0.3, -0.9, -0.1]
    assert all(s["no_speech_prob"] == 0.01 and s["compression_ratio"] is None for s in res[0]["segments"])
    # recording 1: its first window was silence; the second is the last 100 frames, a row cut without a closing timestamp
    assert [(s["seek"],) + t for s, t in zip(res[1]["segments"], _spans(res[1]["segments"]))] == [(3000, 1500, 1550, SCRIPT[1][1][1])]
    # recording 2: no-speech probability above the threshold, but the average log-probability overrides the skip
    assert [(s["seek"],) + t for s, t in zip(res[2]["segments"], _spans(res[2]["segments"]))] == [(0, 0, 250, SCRIPT[0][2][1])]


def test_loop_silence_skip_and_its_override():
    res, _ = _run()
    assert res[1]["windows"] == 2 and len(res[1]["segments"]) == 1 and res[1]["segments"][0]["seek"] == 3000   # window 0 skipped whole
    assert len(res[2]["segments"]) == 1
    # without a log-probability threshold nothing overrides: recording 2's only window is skipped too
    res, _ = _run(logprob_threshold=None)
    assert res[2]["segments"] == [] and res[2]["windows"] == 1 and res[2]["tokens"] == []
    # without a no-speech threshold nothing is skipped: recording 1's first window [0.00, 31, 1.00] is a segment and moves the seek whole
    script = [SCRIPT[0], SCRIPT[1], SCRIPT[2]]
    res, _ = _run(_Stand(script), no_speech_threshold=None)
    assert [s["seek"] for s in res[1]["segments"]] == [0, 3000] and _spans(res[1]["segments"])[0][:2] == (0, 50)


def test_loop_previous_text_prompt_and_its_reset():
    res, stand = _run()
    hist = res[0]["tokens"]
    # iteration 1: recording 0 is conditioned on its 7 tokens, recording 1 has none (its window was skipped)
    assert stand.calls[1]["prompts"] == [[SOT_PREV] + hist[:7] + SOTS[0], SOTS[1]] and stand.calls[1]["sot_index"] == [8, 0]
    assert stand.calls[1]["max_len"] == 12 + 12
    # iteration 2: the window before was decoded at temperature 0.8 > 0.5 — the history is cut there, the prompt is bare
    assert stand.calls[2]["prompts"] == [SOTS[0]] and stand.calls[2]["sot_index"] == [0]


def test_loop_without_conditioning_on_previous_text():
    res, stand = _run(condition_on_previous_text=False)
    assert all(c["prompts"] == [SOTS[a] for a in c["rows"]] and set(c["sot_index"]) == {0} for c in stand.calls)
    assert [r["windows"] for r in res] == [3, 2, 1]


def test_loop_initial_prompt():
    res, stand = _run(initial_prompt=[7, 8])
    assert stand.calls[0]["prompts"] == [[SOT_PREV, 7, 8] + s for s in SOTS] and stand.calls[0]["sot_index"] == [3, 3, 3]
    assert stand.calls[1]["prompts"][0] == [SOT_PREV, 7, 8] + res[0]["tokens"][:7] + SOTS[0]
    assert stand.calls[1]["prompts"][1] == [SOT_PREV, 7, 8] + SOTS[1]
    assert res[0]["tokens"][:2] != [7, 8]     # the initial prompt conditions, it is not part of the result


def test_loop_max_windows_and_truncated():
    res, stand = _run(max_windows=2)
    assert [c["rows"] for c in stand.calls] == [[0, 1, 2], [0, 1]]
    assert [r["windows"] for r in res] == [2, 2, 1] and [r["truncated"] for r in res] == [True, False, False]
    res, stand = _run(max_windows=1)
    assert [c["rows"] for c in stand.calls] == [[0, 1, 2]] and [r["truncated"] for r in res] == [True, True, False]


def test_loop_language_detection_replaces_the_language_token():
    seen = {}

    def detect(model, mel, *, sot, language_tokens, _xa=None):
        seen.update(sot=sot, language_tokens=list(language_tokens), mel=mel, xa=_xa)
        return torch.tensor([LANG + 5, LANG + 6, LANG + 7]), torch.tensor([[0.25, 0.75]] * 3)

    res, stand = _run(language_tokens=[LANG + 5, LANG + 7], _detect=detect)
    assert seen["sot"] == SOT and seen["language_tokens"] == [LANG + 5, LANG + 7] and seen["mel"] is None and seen["xa"] is None
    assert [r["language"] for r in res] == [LANG + 5, LANG + 6, LANG + 7] and all(r["language_probs"].tolist() == [0.25, 0.75] for r in res)
    for c in stand.calls:
        for a, p, i in zip(c["rows"], c["prompts"], c["sot_index"]):
            assert p[i] == SOT and p[i + 1] == LANG + 5 + a


def test_loop_clears_instantaneous_and_blank_segments_but_keeps_them():
    script = [[(0, [ts(1), ts(1), 5, ts(2)], 0.0, 0.0, -0.1)]]
    kw = dict(sot_sequence=SOTS[0], _frames=[900])
    res = T.transcribe(_Model(), [None], eot=EOT, timestamp_begin=TSB, sample_len=12, _decode=_Stand(script), **kw)[0]
    assert _spans(res["segments"]) == [(50, 50, []), (50, 100, [ts(1), 5, ts(2)])] and res["tokens"] == [ts(1), 5, ts(2)]
    res = T.transcribe(_Model(), [None], eot=EOT, timestamp_begin=TSB, sample_len=12, _decode=_Stand(script), text_of=lambda ids: " " * len(ids), **kw)[0]
    assert _spans(res["segments"]) == [(50, 50, []), (50, 100, [])] and res["tokens"] == []


def test_loop_argument_errors_and_the_fp32_mode():
    m = _Model()
    with pytest.raises(ValueError):
        T.transcribe(m, [None], sot_sequence=SOTS, eot=EOT, _frames=[900], _decode=_Stand())          # 3 sequences for 1 recording
    with pytest.raises(ValueError):
        T.transcribe(m, [None], sot_sequence=SOTS[0], eot=EOT, _frames=[900], _decode=_Stand(), sample_len=0)
    with pytest.raises(ValueError):
        T.transcribe(m, [None], sot_sequence=SOTS[0], eot=EOT, _frames=[900], _decode=_Stand(), compression_ratio_threshold=2.4)
    with pytest.raises(ValueError):
        T.transcribe(m, [None], sot_sequence=[SOT], eot=EOT, _frames=[900], _decode=_Stand(), language_tokens=[LANG])
    m.compute_dtype = "fp32"
    with pytest.raises(NotImplementedError):
        T.transcribe(m, [None], sot_sequence=SOTS[0], eot=EOT, _frames=[900], _decode=_Stand())
    with pytest.raises(NotImplementedError):
        T.detect_language(m, None, sot=SOT, language_tokens=[LANG])


# ============================================================================= the kernel checks bite: wft_lang_probs
LANG_CASES = TC.lang_cases()


def _lang_inputs(poison):
    for name, V, ld, ids in LANG_CASES:
        for B in TC.LANG_ROWS:
            for kind in TC.LANG_KINDS:
                yield f"{name} B={B} {kind}", TC.lang_logits(B, V, ld, ids, kind, poison=poison), V, ids


def test_the_lang_probs_restatement_meets_the_derived_bound():
    worst = 0.0
    for poison in (True, False):
        for what, x, V, ids in _lang_inputs(poison):
            probs, best = TC.lang_restate(x, V, ids)
            worst = max(worst, TC.lang_check(probs, best, x, V, ids, what))
            assert abs(float(probs.astype(np.float64).sum(axis=1).max()) - 1.0) < 1e-5
    print(f"worst |p - ref| / bound of the honest restatement: {worst:.3f}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("mutant", TC.LANG_MUTANTS)
def test_every_lang_probs_mutant_is_rejected(mutant):
    hit, total = [], 0
    for what, x, V, ids in _lang_inputs(poison=False):
        total += 1
        try:
            TC.lang_check(*TC.lang_restate(x, V, ids, mutant), x, V, ids, what)
        except AssertionError as e:
            hit.append(str(e)[:160])
    print(f"{mutant}: rejected by {len(hit)} of {total} inputs")
    for h in hit[:6]:
        print("  " + h)
    assert hit, f"the mutant '{mutant}' passes every input"
    if mutant == "no maximum subtraction":   # it is the values near +-80 that catch it
        assert any("extreme" in h for h in hit)


def test_the_lang_cases_are_the_ones_the_issue_names():
    assert [(V, ld, len(ids)) for _, V, ld, ids in LANG_CASES] == [(51865, 51968, 99), (51866, 51968, 100)] + [(300, 384, n) for n in (1, 2, 63, 64, 65)]
    assert LANG_CASES[0][3] == list(range(50259, 50358)) and LANG_CASES[1][3] == list(range(50259, 50359))
    for _, V, ld, ids in LANG_CASES:
        assert ids == sorted(set(ids)) and 0 <= ids[0] and ids[-1] < V
        if V == 300 and len(ids) > 1:
            assert ids[0] == 0 and ids[-1] == V - 1 and (len(ids) == 2 or max(np.diff(ids)) > 1)
        x = TC.lang_logits(3, V, ld, ids, "tie")
        other = np.setdiff1d(np.arange(ld), ids)
        assert not np.isfinite(x[:, other]).any() and np.isnan(x[:, other]).any() and np.isinf(x[:, other]).any() and np.isfinite(x[:, ids]).all()
        assert (x[:, ids[0]] == x[:, ids[-1]]).all() and (x[:, ids].max(axis=1) == x[:, ids[0]]).all()
        assert np.abs(TC.lang_logits(3, V, ld, ids, "extreme")[:, ids]).min() > 75


# ============================================================================= the kernel checks bite: wft_mel_windows
@pytest.fixture(scope="module", params=[80, 128])
def mel_case(request):
    case = TC.mel_case(request.param)
    return case, TC.mel_expected(case)


def test_the_mel_windows_restatement_equals_slicing_bit_for_bit(mel_case):
    case, want = mel_case
    assert np.isfinite(want).all() and TC.same_bits(TC.mel_restate(case), want)
    for a, (off, ld, cf) in enumerate(zip(case["off"], case["ld"], case["cf"])):   # the source's padding region is NaN throughout
        rec = case["mel"][off:off + case["n_mels"] * ld].reshape(case["n_mels"], ld)
        assert np.isnan(rec[:, cf:]).all() and np.isfinite(rec[:, :cf]).all() and ld == cf + TC.N_WIN and off % 2 == 1
    seeks = {(a, s) for a, s in zip(case["rows"], case["seeks"])}
    assert {(0, 0), (0, 1233), (0, 4700 - 3000), (0, 4700 - 2999), (0, 4699), (1, 3001 - 3000), (1, 3001 - 2999), (1, 3000), (2, 0), (2, 6)} <= seeks
    assert case["rows"] != sorted(case["rows"]) and len(case["rows"]) > len(seeks)


@pytest.mark.parametrize("mutant", TC.MEL_MUTANTS)
def test_every_mel_windows_mutant_is_rejected(mel_case, mutant):
    case, want = mel_case
    assert not TC.same_bits(TC.mel_restate(case, mutant), want), f"the mutant '{mutant}' equals the reference"
