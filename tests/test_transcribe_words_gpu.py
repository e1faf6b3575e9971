"""Word timestamps inside transcribe() end to end on the GPU: whisper-tiny and the three ragged recordings of
tests/test_transcribe_gpu.py (its helpers are imported), with a synthetic `split_words`: two ids per word, the string derived from
the word's first id — " w<id>", but "," for ids that are 0 mod 5 and " (" for ids that are 1 mod 5, so both merges of
`merge_punctuations` fire.

The bar for the loop is bit equality with a replay from the public pieces — LongMel.windows, window_prompt, model.encoder,
model.decode_with_fallback(_xa=), advance_window(return_single_ending=True), model.find_alignment(word_spans="device", _xa=),
D.add_word_timestamps — with the batch composition transcribe's docstring states, and the seek rule written out here.

Constants: LOGPROB_TS = -5.525 is that file's (picked there between the first windows' average log-probabilities, so both rungs
of the ladder occur); sample_len = 12 and max_windows = 3 are that file's too, and nothing else was tuned.  A first look on an
MI355X with these constants: windows per recording 2, 2, 1; the first window of recording 1 does not end on a single timestamp,
`advance_window` alone moves its seek to 2986, the end of its last word to 2524 (every other window ends on a single timestamp
and moves by its segment_size).  The test asserts that at least one such window exists and that its recording's seeks differ from
the run without word timestamps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _word_cases as WC  # noqa: E402
from tests import test_transcribe_gpu as TG  # noqa: E402
from tests.test_transcribe_gpu import case  # noqa: E402,F401  (the module fixture: model, recordings, packed log-mels)
from whisper_finetune.engine import decode as D  # noqa: E402
from whisper_finetune.engine import transcribe as T  # noqa: E402

DEV = TG.DEV
EOT, SOT, LANG_EN, TRANSCRIBE, NO_TS, TSB = TG.EOT, TG.SOT, TG.LANG_EN, TG.TRANSCRIBE, TG.NO_TS, TG.TSB
SOT_SEQ = (SOT, LANG_EN, TRANSCRIBE)
KW = dict(timestamp_begin=TSB, no_timestamps=NO_TS)
MAX_WINDOWS = 3


def split_words(ids):
    """ids + [eot] -> (words, word_tokens): two ids per word (the last text word may hold one), the eot a word of its own"""
    text = list(ids[:-1])
    groups = [text[i:i + 2] for i in range(0, len(text), 2)]
    names = ["," if g[0] % 5 == 0 else " (" if g[0] % 5 == 1 else f" w{g[0]}" for g in groups]
    return names + ["<eot>"], groups + [[ids[-1]]]


def _counts(text):
    return [len(g) for g in split_words(list(text) + [EOT])[1]]


# ----------------------------------------------------------------------------- 1. find_alignment: device spans, _xa
TEXTS = [[464, 2068, 7586, 21831, 18045, 625, 262, 16931, 3290], [15496, 995], [40, 716, 257, 1332, 13]]
NUM_FRAMES = [3000, 3000, 900]


def test_device_spans_and_xa_against_the_host_path(case):
    m, packed = case["model"], case["packed"]
    mel = packed.windows([0, 1, 2], [0, 0, 0])
    counts = [_counts(t) for t in TEXTS]
    args = dict(sot_sequence=SOT_SEQ, no_timestamps=NO_TS, eot=EOT, num_frames=NUM_FRAMES, word_token_counts=counts)
    host, dbg = m.find_alignment(mel, TEXTS, return_debug=True, **args)
    # the default call is what it was: alignment_words over the paths of the debug dict
    pt, pj, pl = dbg["paths"]
    at = 0
    for b, text in enumerate(TEXTS):
        n = int(pl[b])
        want = D.alignment_words(pt[b, :n].numpy(), pj[b, :n].numpy(), counts[b], dbg["token_probs"][at:at + len(text)], text)
        at += len(text)
        assert host[b] == want and len(want) == len(counts[b]) - 1
    assert m.find_alignment(mel, TEXTS, **args) == host
    with torch.no_grad():
        xa = m.encoder(mel)
    calls = []
    hook = m.encoder.register_forward_hook(lambda *a: calls.append(1))
    try:
        dev = m.find_alignment(mel, TEXTS, word_spans="device", _xa=xa, **args)
        assert m.find_alignment(None, TEXTS, word_spans="device", _xa=xa, **args) == dev      # the mel is not read
        assert m.find_alignment(mel, TEXTS, _xa=xa, **args) == host                           # _xa alone changes nothing
    finally:
        hook.remove()
    assert calls == [], "with _xa the encoder must not run"
    worst = 0.0
    for b in range(3):
        assert len(dev[b]) == len(host[b])
        for (s0, e0, p0, ids0), (s1, e1, p1, ids1) in zip(dev[b], host[b]):
            assert (s0, e0, ids0) == (s1, e1, ids1) and isinstance(s0, float) and isinstance(p0, float)
            bound = WC.prob_bound(p1, len(ids1))
            worst = max(worst, abs(p0 - p1) / bound)
    print(f"device word probabilities vs the host path: worst |diff| / bound {worst:.3f}")
    assert worst <= 1.0
    # a subset of the rows: row 1 has no text
    texts = [TEXTS[0], [], TEXTS[2]]
    sub = m.find_alignment(mel, texts, word_spans="device", _xa=xa, **dict(args, word_token_counts=[counts[0], None, counts[2]]))
    ref = m.find_alignment(mel, texts, **dict(args, word_token_counts=[counts[0], None, counts[2]]))
    assert sub[1] == [] and [[w[:2] + w[3:] for w in r] for r in sub] == [[w[:2] + w[3:] for w in r] for r in ref]
    with pytest.raises(ValueError):
        m.find_alignment(mel, TEXTS, word_spans="gpu", **args)
    with pytest.raises(ValueError):
        m.find_alignment(mel, TEXTS, word_spans="device", **dict(args, word_token_counts=[[1, 1], counts[1], counts[2]]))


# ----------------------------------------------------------------------------- 2. the loop against a replay
def replay_words(case, *, logprob_threshold, max_windows):
    """transcribe(word_timestamps=True)'s loop from the public pieces -> (per recording: segments, windows, seeks, final seek;
    per iteration: rows)."""
    m, packed = case["model"], case["packed"]
    n_ctx, n = m.dims.n_text_ctx, len(TG.FRAMES)
    history, reset, seek, last_speech = [[] for _ in range(n)], [0] * n, [0] * n, [0.0] * n
    out = [dict(segments=[], windows=0, seeks=[], single=[]) for _ in range(n)]
    batches, i = [], 0
    while True:
        rows = [a for a in range(n) if seek[a] < TG.FRAMES[a] and out[a]["windows"] < max_windows]
        if not rows:
            break
        batches.append(rows)
        mel = packed.windows(rows, [seek[a] for a in rows])
        with torch.no_grad():
            xa = m.encoder(mel)
        prompts = [T.window_prompt(history[a], reset[a], list(SOT_SEQ), TG.SOT_PREV, n_ctx) for a in rows]
        width = max(len(p) for p, _ in prompts)
        prompt = torch.full((len(rows), width), EOT, dtype=torch.int64)
        for j, (p, _) in enumerate(prompts):
            prompt[j, :len(p)] = torch.tensor(p)
        plen = [len(p) for p, _ in prompts]
        toks, lens, _, info = m.decode_with_fallback(
            mel, prompt.to(DEV), torch.tensor(plen), temperatures=TG.LADDER["temperatures"], best_of=TG.LADDER["best_of"],
            logprob_threshold=logprob_threshold, no_speech_threshold=0.6, no_speech=TG.NO_SPEECH, sot_index=[s for _, s in prompts],
            seed=TG.SEED + i, eot=EOT, max_len=min(n_ctx, width + TG.LADDER["sample_len"]), suppress=TG.SUPPRESS, _xa=xa, **KW)
        toks, lens = toks.cpu().tolist(), lens.cpu().tolist()
        windows = {}
        for j, a in enumerate(rows):
            ids, _ = D.generated_ids(toks[j], plen[j], lens[j], EOT)
            size = min(3000, TG.FRAMES[a] - seek[a])
            out[a]["windows"] += 1
            out[a]["seeks"].append(seek[a])
            nsp, alp = info["no_speech_prob"][j], info["avg_logprob"][j]
            if nsp > 0.6 and not alp > logprob_threshold:
                seek[a] += size
                out[a]["single"].append(None)
                continue
            segs, new_seek, single = T.advance_window(ids, seek=seek[a], segment_size=size, timestamp_begin=TSB, return_single_ending=True)
            out[a]["single"].append(single)
            windows[j] = (segs, seek[a], size, single, new_seek)
        texts = {j: [t for s in w[0] for t in s["tokens"] if t < EOT] for j, w in windows.items()}
        js = [j for j in windows if texts[j]]
        words = {j: [] for j in windows}
        if js:
            whole = len(js) == len(rows)
            sel = None if whole else torch.tensor(js, device=DEV)
            split = [split_words(texts[j] + [EOT]) for j in js]
            found = m.find_alignment(mel if whole else mel[sel], [texts[j] for j in js], sot_sequence=SOT_SEQ, no_timestamps=NO_TS, eot=EOT,
                                     num_frames=[windows[j][2] for j in js], word_token_counts=[[len(g) for g in s[1]] for s in split],
                                     word_spans="device", _xa=xa if whole else xa[sel])
            for j, s, f in zip(js, split, found):
                words[j] = [dict(word=name, tokens=ids, start=st, end=en, probability=p) for name, (st, en, p, ids) in zip(s[0][:-1], f)]
        for j, a in enumerate(rows):
            if j not in windows:
                continue
            segs, before, size, single, new_seek = windows[j]
            offset = before * 0.01
            D.add_word_timestamps(segs, words[j], time_offset=offset, last_speech_timestamp=last_speech[a], eot=EOT)
            ends = [w["end"] for s in segs for w in s["words"]]
            end = ends[-1] if ends else segs[-1]["end"]
            if not single and end > offset:
                new_seek = round(end * 100)
            seek[a] = new_seek if new_seek > before else before + size
            last_speech[a] = end
            temp = info["temperature"][j]
            for s in segs:
                if s["start"] == s["end"]:
                    s["tokens"], s["words"] = [], []
                s.update(temperature=temp, avg_logprob=info["avg_logprob"][j], no_speech_prob=info["no_speech_prob"][j])
                out[a]["segments"].append(s)
                history[a].extend(s["tokens"])
            if temp > 0.5:
                reset[a] = len(history[a])
        i += 1
    for a in range(n):
        out[a]["seek"] = seek[a]
    return out, batches


class AlignSpy:
    def __init__(self):
        self.calls = []

    def __call__(self, model, mel, text_tokens, **kw):
        self.calls.append(dict(batch=len(text_tokens), sot=tuple(kw["sot_sequence"]), word_spans=kw["word_spans"], xa=kw["_xa"] is not None))
        return D.find_alignment(model, mel, text_tokens, **kw)


def _window_seeks(segments):
    seeks = []
    for s in segments:
        if not seeks or s["seek"] != seeks[-1]:
            seeks.append(s["seek"])
    return seeks


def test_transcribe_with_word_timestamps_is_the_replay(case):
    m = case["model"]
    spy, aspy, enc = TG.Spy(), AlignSpy(), []
    hook = m.encoder.register_forward_hook(lambda *a: enc.append(1))
    try:
        res = m.transcribe(case["audios"], sot_sequence=SOT_SEQ, eot=EOT, filters=case["filters"], logprob_threshold=TG.LOGPROB_TS,
                           max_windows=MAX_WINDOWS, word_timestamps=True, split_words=split_words, _decode=spy, _align=aspy, **KW, **TG.LADDER)
    finally:
        hook.remove()
    iterations = len(spy.calls)
    assert len(enc) == iterations, f"{len(enc)} encoder calls in {iterations} iterations"
    assert len(aspy.calls) <= iterations and all(c["word_spans"] == "device" and c["xa"] and c["sot"] == SOT_SEQ for c in aspy.calls)
    want, batches = replay_words(case, logprob_threshold=TG.LOGPROB_TS, max_windows=MAX_WINDOWS)
    assert [c["batch"] for c in spy.calls] == [len(b) for b in batches]
    print("windows:", [r["windows"] for r in res], "seeks:", [w["seeks"] for w in want], "single endings:", [w["single"] for w in want])
    merged = 0
    for a in range(3):
        TG._same_segments(res[a]["segments"], want[a]["segments"], f"recording {a}")
        assert res[a]["windows"] == want[a]["windows"] and res[a]["truncated"] == (want[a]["seek"] < TG.FRAMES[a])
        for g, w in zip(res[a]["segments"], want[a]["segments"]):
            assert g["words"] == w["words"]
            assert all(x["start"] <= x["end"] and 0.0 <= x["probability"] <= 1.0 for x in g["words"])
            merged += sum(1 for x in g["words"] if x["word"].startswith(" (") and len(x["word"]) > 2 or x["word"].endswith(",") and len(x["word"]) > 1)
        assert _window_seeks(res[a]["segments"]) == [s for s, single in zip(want[a]["seeks"], want[a]["single"]) if single is not None]
        # the words of a window carry the window's text tokens, in order (a two-id word may straddle two segments: it stays with
        # the first); a window with a blanked segment is left out
        for seek in _window_seeks(res[a]["segments"]):
            segs = [s for s in res[a]["segments"] if s["seek"] == seek]
            if all(s["tokens"] for s in segs):
                assert [t for s in segs for x in s["words"] for t in x["tokens"]] == [t for s in segs for t in s["tokens"] if t < EOT]
        assert res[a]["tokens"] == [t for s in res[a]["segments"] for t in s["tokens"]]
    assert merged > 0, "no punctuation word was merged: the synthetic split_words must make both merges fire"
    # at least one window did not end on a single timestamp, and the recording's next seek differs from the run without words
    plain, _ = TG.replay(case, logprob_threshold=TG.LOGPROB_TS, max_windows=MAX_WINDOWS, **KW)
    with_words = [_window_seeks(res[a]["segments"]) + [want[a]["seek"]] for a in range(3)]
    without = [_window_seeks(plain[a]["segments"]) + [plain[a]["seek"]] for a in range(3)]
    moved = [a for a in range(3) if False in want[a]["single"] and with_words[a] != without[a]]
    print("window seeks and final seek with words:", with_words, "without:", without, "moved:", moved)
    assert moved, "no window without a single ending timestamp moved the seek"
    assert not m.training


# ----------------------------------------------------------------------------- 3. without word timestamps nothing changes
def test_without_word_timestamps_nothing_changes(case):
    m = case["model"]
    aspy = AlignSpy()
    res = m.transcribe(case["audios"], sot_sequence=SOT_SEQ, eot=EOT, filters=case["filters"], logprob_threshold=TG.LOGPROB_TS,
                       max_windows=MAX_WINDOWS, split_words=split_words, _align=aspy, **KW, **TG.LADDER)
    want, _ = TG.replay(case, logprob_threshold=TG.LOGPROB_TS, max_windows=MAX_WINDOWS, **KW)
    assert aspy.calls == []
    for a in range(3):
        TG._same_segments(res[a]["segments"], want[a]["segments"], f"recording {a}")
        assert all("words" not in s for s in res[a]["segments"]) and res[a]["windows"] == want[a]["windows"]
        assert res[a]["truncated"] == (want[a]["seek"] < TG.FRAMES[a])


# ----------------------------------------------------------------------------- 4. the fp32 compute mode
def test_fp32_mode_still_raises(case):
    m = case["model"]
    m.set_compute_dtype("fp32")
    try:
        with pytest.raises(NotImplementedError):
            m.transcribe(case["audios"], sot_sequence=SOT_SEQ, eot=EOT, filters=case["filters"], word_timestamps=True, split_words=split_words, **KW)
        with pytest.raises(NotImplementedError):
            m.find_alignment(case["packed"].windows([0], [0]), [[1, 2]], sot_sequence=SOT_SEQ, no_timestamps=NO_TS, eot=EOT, num_frames=3000,
                             word_spans="device")
    finally:
        m.set_compute_dtype("bf16")
