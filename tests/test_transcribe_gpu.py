"""Language detection and long-form transcription end to end on the GPU (engine/transcribe.py; Whisper.detect_language /
Whisper.transcribe): whisper-tiny with the weights of tests/test_model_gpu.py, three recordings of seeded noise N(0, 0.1^2) of
47 s, 31 s and 9 s plus a few samples (no length is a multiple of 160), sample_len = 12, temperatures (0.0, 0.6), best_of = 2.

The bar for the loop is bit equality with a replay from the public pieces — LongMel.windows (K.mel_windows), window_prompt,
model.decode_with_fallback, advance_window — with the batch composition and the seed of every iteration that transcribe's docstring
states: the batches are the same, so the kernels see the same shapes.

The log-probability thresholds were picked from a first look at this model's values on an MI355X, between the average
log-probabilities that the three first windows reach at temperature 0, so that the ladder is exercised on both rungs:
  without timestamps: LOGPROB_TEXT = -8.38 (first windows at temperature 0: -8.3954, -8.3960, -8.3673); windows per rung observed: 3 at 0.0, 2 at 0.6
  with timestamps:    LOGPROB_TS = -5.525 (first windows at temperature 0: -5.5329, -5.5335, -5.5175); windows per rung observed: 3 at 0.0, 2 at 0.6
Both tests assert that both rungs occurred."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests import _transcribe_cases as TC  # noqa: E402
from tests.test_model_gpu import _engine, _tiny_case  # noqa: E402
from whisper_finetune.engine import decode as D  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import transcribe as T  # noqa: E402

DEV = torch.device("cuda:0")
EOT, SOT, LANG_EN, TRANSCRIBE, SOT_PREV, NO_SPEECH, NO_TS, TSB = 50257, 50258, 50259, 50359, 50361, 50362, 50363, 50364
LANGS = list(range(50259, 50358))
SUPPRESS = list(range(EOT + 1, TSB))  # the specials, as the evaluator suppresses them
SECONDS = (47, 31, 9)
EXTRA = (37, 101, 159)                # samples on top: no length is a multiple of 160
FRAMES = [4700, 3100, 900]
SEED = 23
LOGPROB_TEXT = -8.38   # picked from the first look (module docstring)
LOGPROB_TS = -5.525
LADDER = dict(temperatures=(0.0, 0.6), best_of=2, sample_len=12, seed=SEED, no_speech=NO_SPEECH, sot_prev=SOT_PREV, suppress=SUPPRESS)


@pytest.fixture(scope="module")
def case():
    dims, params, _, _, _ = _tiny_case()
    m = _engine(dims, params).eval()
    g = torch.Generator().manual_seed(77)
    audios = [torch.randn(s * T.SAMPLE_RATE + e, generator=g) * 0.1 for s, e in zip(SECONDS, EXTRA)]
    filters = O.mel_filters(dims.n_mels).to(DEV)
    packed = T.pack_logmels(audios, filters)
    assert list(packed.host[2]) == FRAMES
    return dict(model=m, audios=audios, filters=filters, packed=packed)


# ----------------------------------------------------------------------------- 1. the long log-mel
def test_long_logmel(case):
    audio, filters = case["audios"][0], case["filters"]
    long = T.long_logmel(audio, filters)
    assert tuple(long.shape) == (80, 4700 + 3000)
    # the helper is wft_logmel on the hand-padded array: bit for bit
    padded = torch.cat([audio[:4700 * 160], torch.zeros(480000)]).to(DEV)
    assert torch.equal(long, K.logmel(padded.view(1, -1), filters, n_frames=7700)[0])
    # and the packed copy is that array
    off, ld = case["packed"].host[0][0], case["packed"].host[1][0]
    assert torch.equal(case["packed"].mel[off:off + 80 * ld].view(80, ld), long)
    # window 0 against the log-mel of the first 30 s with the samples that follow them appended (one more second: the frames at
    # the 30 s edge see the same samples as in the long recording).  Frame arithmetic is the same; only the floor max - 8 could
    # differ, through the maximum over 31 s instead of 77 s — it is inactive for this noise, so the frames are equal bit for bit.
    win = case["packed"].windows([0], [0])[0]
    assert torch.equal(win, long[:, :3000])
    short = K.logmel(audio[:3100 * 160].to(DEV).view(1, -1), filters, n_frames=3100)[0]
    diff = (win - short[:, :3000]).abs().max().item()
    print(f"window 0 vs the 31 s log-mel: max |diff| {diff:.3e}; floor of the long mel {long.max().item() - 2.0:.4f}, min {long[:, :4700].min().item():.4f}")
    assert long[:, :4700].min().item() > long.max().item() - 2.0     # (x + 4) / 4: the floor max - 8 is max - 2 here — inactive
    assert torch.equal(win, short[:, :3000])


# ----------------------------------------------------------------------------- 2. detect_language
def test_detect_language(case):
    m, packed = case["model"], case["packed"]
    mel = packed.windows([0, 1, 2], [0, 0, 0])
    best, probs = m.detect_language(mel, sot=SOT, language_tokens=LANGS)
    assert best.dtype == torch.int64 and tuple(best.shape) == (3,) and probs.dtype == torch.float32 and tuple(probs.shape) == (3, len(LANGS))
    with torch.no_grad():
        xa = m.encoder(mel)
        logits = m.decoder(torch.full((3, 1), SOT, dtype=torch.int64, device=DEV), xa)[:, 0]   # the engine's teacher-forced logits for [sot]
    x = logits.cpu().numpy()
    worst = TC.lang_check(probs.cpu().numpy(), best.cpu().numpy(), x, m.dims.n_vocab, LANGS, "detect_language")
    print(f"detect_language: best {best.tolist()}, worst |p - ref| / bound {worst:.3f}, top probability {probs.max(dim=1).values.tolist()}")
    again = m.detect_language(mel, sot=SOT, language_tokens=LANGS, _xa=xa)
    assert torch.equal(again[0], best) and torch.equal(again[1], probs)
    assert not m.training


# ----------------------------------------------------------------------------- the replay
def replay(case, *, logprob_threshold, no_speech_threshold=0.6, timestamp_begin=None, no_timestamps=None, language=None, max_windows=None,
           sot_sequence=(SOT, LANG_EN, TRANSCRIBE)):
    """The loop of transcribe's docstring from the public pieces -> (per recording: segments, windows, final seek; per iteration: rows)."""
    m, packed = case["model"], case["packed"]
    n_ctx = m.dims.n_text_ctx
    n = len(FRAMES)
    sots = [list(sot_sequence) for _ in range(n)]
    if language is not None:
        for a in range(n):
            sots[a][1] = language[a]
    history, reset, seek = [[] for _ in range(n)], [0] * n, [0] * n
    out = [dict(segments=[], windows=0, prompts=[]) for _ in range(n)]
    batches, i = [], 0
    while True:
        rows = [a for a in range(n) if seek[a] < FRAMES[a] and (max_windows is None or out[a]["windows"] < max_windows)]
        if not rows:
            break
        batches.append(rows)
        mel = packed.windows(rows, [seek[a] for a in rows])
        prompts = [T.window_prompt(history[a], reset[a], sots[a], SOT_PREV, n_ctx) for a in rows]
        width = max(len(p) for p, _ in prompts)
        prompt = torch.full((len(rows), width), EOT, dtype=torch.int64)
        for j, (p, _) in enumerate(prompts):
            prompt[j, :len(p)] = torch.tensor(p)
        plen = [len(p) for p, _ in prompts]
        toks, lens, _, info = m.decode_with_fallback(
            mel, prompt.to(DEV), torch.tensor(plen), temperatures=LADDER["temperatures"], best_of=LADDER["best_of"], logprob_threshold=logprob_threshold,
            no_speech_threshold=no_speech_threshold, no_speech=NO_SPEECH, sot_index=[s for _, s in prompts], seed=SEED + i, eot=EOT,
            max_len=min(n_ctx, width + LADDER["sample_len"]), suppress=SUPPRESS, timestamp_begin=timestamp_begin, no_timestamps=no_timestamps)
        toks, lens = toks.cpu().tolist(), lens.cpu().tolist()
        for j, a in enumerate(rows):
            ids, _ = D.generated_ids(toks[j], plen[j], lens[j], EOT)
            size = min(3000, FRAMES[a] - seek[a])
            out[a]["windows"] += 1
            out[a]["prompts"].append(prompts[j])
            nsp, alp, temp = info["no_speech_prob"][j], info["avg_logprob"][j], info["temperature"][j]
            skip = no_speech_threshold is not None and nsp > no_speech_threshold
            if skip and logprob_threshold is not None and alp > logprob_threshold:
                skip = False
            if skip:
                seek[a] += size
                continue
            segs, seek[a] = T.advance_window(ids, seek=seek[a], segment_size=size, timestamp_begin=timestamp_begin)
            for s in segs:
                if s["start"] == s["end"]:
                    s["tokens"] = []
                s.update(temperature=temp, avg_logprob=alp, no_speech_prob=nsp)
                out[a]["segments"].append(s)
                history[a].extend(s["tokens"])
            if temp > 0.5:
                reset[a] = len(history[a])
        i += 1
    for a in range(n):
        out[a]["seek"] = seek[a]
    return out, batches


class Spy:
    """decode_with_fallback, with every call's batch size, seed and prompts recorded."""

    def __init__(self):
        self.calls = []

    def __call__(self, model, mel, prompt, prompt_len, **kw):
        res = D.decode_with_fallback(model, mel, prompt, prompt_len, **kw)
        self.calls.append(dict(batch=int(mel.shape[0]), seed=kw["seed"], max_len=kw["max_len"], sot_index=list(kw["sot_index"]),
                               prompts=[prompt[j, :int(prompt_len[j])].tolist() for j in range(prompt.shape[0])], info=res[3]))
        return res


def _same_segments(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} segments, the replay has {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        for key in ("seek", "start", "end", "tokens", "temperature", "avg_logprob", "no_speech_prob"):
            assert g[key] == w[key], f"{what}, segment {k}: {key} {g[key]!r} != {w[key]!r}"


def _rungs(spy):
    temps = [t for c in spy.calls for t in c["info"]["temperature"]]
    return {t: temps.count(t) for t in sorted(set(temps))}


# ----------------------------------------------------------------------------- 3. without timestamps
def test_transcribe_without_timestamps(case):
    m = case["model"]
    spy = Spy()
    res = m.transcribe(case["audios"], sot_sequence=(SOT, LANG_EN, TRANSCRIBE), eot=EOT, filters=case["filters"], logprob_threshold=LOGPROB_TEXT,
                       _decode=spy, **LADDER)
    print("avg_logprob of the first windows per call:", [c["info"]["avg_logprob"] for c in spy.calls], "rungs:", _rungs(spy))
    assert [r["windows"] for r in res] == [2, 2, 1] and not any(r["truncated"] for r in res)
    assert [c["batch"] for c in spy.calls] == [3, 2] and [c["seed"] for c in spy.calls] == [SEED, SEED + 1]
    assert all(r["language"] is None for r in res)
    want, batches = replay(case, logprob_threshold=LOGPROB_TEXT)
    assert batches == [[0, 1, 2], [0, 1]]
    for a in range(3):
        _same_segments(res[a]["segments"], want[a]["segments"], f"recording {a}")
        # every segment spans its window
        seeks = [0, 3000][:res[a]["windows"]]
        assert [s["seek"] for s in res[a]["segments"]] == seeks
        for s in res[a]["segments"]:
            size = min(3000, FRAMES[a] - s["seek"])
            assert s["start"] == s["seek"] * 0.01 and s["end"] == s["seek"] * 0.01 + size * 0.01 and len(s["tokens"]) > 0
        assert res[a]["tokens"] == [t for s in res[a]["segments"] for t in s["tokens"]]
    # the second windows are conditioned on the first (ragged prompts), unless the first was decoded at 0.6 > 0.5
    for j, a in enumerate([0, 1]):
        first = res[a]["segments"][0]
        p, idx = spy.calls[1]["prompts"][j], spy.calls[1]["sot_index"][j]
        assert p == ([SOT, LANG_EN, TRANSCRIBE] if first["temperature"] > 0.5 else [SOT_PREV] + first["tokens"] + [SOT, LANG_EN, TRANSCRIBE]) and p[idx] == SOT
    rungs = _rungs(spy)
    assert set(rungs) == {0.0, 0.6}, f"both rungs of the ladder must occur, got {rungs}"
    assert not m.training


# ----------------------------------------------------------------------------- 4. with timestamps
def test_transcribe_with_timestamps(case):
    m = case["model"]
    spy = Spy()
    kw = dict(timestamp_begin=TSB, no_timestamps=NO_TS)
    res = m.transcribe(case["audios"], sot_sequence=(SOT, LANG_EN, TRANSCRIBE), eot=EOT, filters=case["filters"], logprob_threshold=LOGPROB_TS,
                       language_tokens=LANGS, max_windows=3, _decode=spy, **kw, **LADDER)
    print("avg_logprob per call:", [c["info"]["avg_logprob"] for c in spy.calls], "rungs:", _rungs(spy))
    print("seeks:", [[s["seek"] for s in r["segments"]] for r in res], "windows:", [r["windows"] for r in res])
    # the language: what detect_language says about the first windows
    best, probs = m.detect_language(case["packed"].windows([0, 1, 2], [0, 0, 0]), sot=SOT, language_tokens=LANGS)
    assert [r["language"] for r in res] == best.tolist()
    for a in range(3):
        assert torch.equal(res[a]["language_probs"], probs[a].cpu())
    want, batches = replay(case, logprob_threshold=LOGPROB_TS, language=best.tolist(), max_windows=3, **kw)
    assert [c["batch"] for c in spy.calls] == [len(b) for b in batches] and [c["seed"] for c in spy.calls] == [SEED + i for i in range(len(batches))]
    at = [0, 0, 0]
    for i, rows in enumerate(batches):
        for j, a in enumerate(rows):
            p, idx = spy.calls[i]["prompts"][j], spy.calls[i]["sot_index"][j]
            assert (p, idx) == want[a]["prompts"][at[a]]
            assert p[idx] == SOT and p[idx + 1] == res[a]["language"]       # the detected language sits behind sot in every prompt
            at[a] += 1
    for a in range(3):
        _same_segments(res[a]["segments"], want[a]["segments"], f"recording {a}")
        assert res[a]["windows"] == want[a]["windows"] <= 3
        seeks = []
        for s in res[a]["segments"]:
            if not seeks or s["seek"] != seeks[-1]:
                seeks.append(s["seek"])
        assert seeks == sorted(set(seeks)), f"recording {a}: seek is not strictly increasing: {seeks}"
        assert res[a]["truncated"] == (want[a]["seek"] < FRAMES[a]) and (not res[a]["truncated"] or res[a]["windows"] == 3)
    rungs = _rungs(spy)
    assert set(rungs) == {0.0, 0.6}, f"both rungs of the ladder must occur, got {rungs}"


# ----------------------------------------------------------------------------- 5. the silence skip
def test_transcribe_skips_everything_at_threshold_zero(case):
    res = case["model"].transcribe(case["audios"], sot_sequence=(SOT, LANG_EN, TRANSCRIBE), eot=EOT, filters=case["filters"],
                                   no_speech_threshold=0.0, logprob_threshold=None, **LADDER)
    for a in range(3):
        assert res[a]["segments"] == [] and res[a]["tokens"] == [] and res[a]["windows"] == math.ceil(FRAMES[a] / 3000) and not res[a]["truncated"]


# ----------------------------------------------------------------------------- 6. the fp32 compute mode
def test_fp32_mode_raises(case):
    m = case["model"]
    m.set_compute_dtype("fp32")
    try:
        with pytest.raises(NotImplementedError):
            m.transcribe(case["audios"], sot_sequence=(SOT, LANG_EN, TRANSCRIBE), eot=EOT, filters=case["filters"])
        with pytest.raises(NotImplementedError):
            m.detect_language(torch.zeros((1, 80, 3000), device=DEV), sot=SOT, language_tokens=LANGS)
    finally:
        m.set_compute_dtype("bf16")
