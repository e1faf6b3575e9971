"""Language detection and long-form transcription: a recording in, timed segments of token ids out.

Upstream's `whisper.decoding.detect_language` and the window loop of `whisper.transcribe.transcribe`, restated on the window decoders
of engine/decode/ (openai-whisper is not a dependency: parity with its binary is unpinned).  Ids go in and ids come out — no
tokenizer: `audio` is mono f32, at 16 kHz or at the `sample_rate` it is declared with (then it is resampled on the device first:
data/gpu_frontend.py `resample`, csrc/audio.hip `wft_resample_f32`), or a WAV file as a path or `bytes`, decoded and downmixed on
the device at the rate of its header (data/audio_io.py `parse_wav`, csrc/pcm.hip `wft_pcm_decode_f32`).

Device stages (csrc/transcribe.hip, include/wft.h "Language detection and long-form windows"): `wft_lang_probs` is the tail of
detect_language, `wft_mel_windows` cuts one zero-padded 30 s window per batch row out of the packed long log-mels; the long log-mel
itself is `wft_logmel` over the whole recording (`long_logmel`).  Everything else of a window is `decode_with_fallback`.

Several recordings advance side by side in ONE batch (upstream handles one at a time); `transcribe` states the batching rule.
The seek arithmetic (`advance_window`, and `word_seek` on top of it) and the previous-text prompt (`window_prompt`) are pure host
functions.

`word_timestamps=True`: every iteration aligns the windows it has just decoded — ONE `find_alignment` call per distinct sot sequence
over the rows that have segments, on the encoder output the decoders used, with the word spans formed on the device
(csrc/align.hip `wft_word_spans`) — then upstream's string rules (engine/decode/words.py `add_word_timestamps`), its seek-to-the-last-word
rule and, with `hallucination_silence_threshold`, its hallucination filter (`word_seek`).  Strings come from the caller's
`split_words`; ids go in and ids come out as before.

Not built: `clip_timestamps`, `carry_initial_prompt`, a tokenizer, the fp32 compute mode.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import decode as D
from . import kernels as K

SAMPLE_RATE = 16000
HOP_LENGTH = 160
N_FRAMES = 3000                      # frames of one 30 s window
N_SAMPLES = N_FRAMES * HOP_LENGTH    # 480 000: upstream pads every recording with 30 s of zeros


# ============================================================================= pure host functions
def window_prompt(all_tokens: Sequence[int], prompt_reset_since: int, sot_sequence: Sequence[int], sot_prev: Optional[int], n_text_ctx: int):
    """Upstream's `DecodingTask._get_initial_tokens` for one window -> (prompt ids, sot_index).

    [sot_prev] + all_tokens[prompt_reset_since:][-(n_text_ctx // 2 - 1):] + sot_sequence; without previous tokens, or with sot_prev
    None, the prompt is sot_sequence alone.  sot_index is the position of sot_sequence[0]."""
    sot = [int(t) for t in sot_sequence]
    if not sot:
        raise ValueError("sot_sequence must not be empty")
    prev = [int(t) for t in all_tokens[int(prompt_reset_since):]]
    keep = int(n_text_ctx) // 2 - 1
    if not prev or sot_prev is None or keep < 1:
        return sot, 0
    prev = prev[-keep:]
    return [int(sot_prev)] + prev + sot, 1 + len(prev)


def advance_window(tokens: Sequence[int], *, seek: int, segment_size: int, timestamp_begin: Optional[int], input_stride: int = 2,
                   time_precision: float = 0.02, frame_s: float = 0.01, return_single_ending: bool = False):
    """Upstream's segment split and seek rule for the decoded tokens of ONE window -> (segments, new_seek).

    tokens: the generated ids before the eot, timestamps included.  A segment is {"seek", "start", "end", "tokens"}, times in
    seconds from the start of the recording: seek * frame_s + (id - timestamp_begin) * time_precision.
    With ts[i] = tokens[i] >= timestamp_begin, single_ending = (ts[-2:] == [False, True]) and cuts = every i + 1 with ts[i] and
    ts[i + 1]:
      cuts non-empty: len(tokens) joins the cuts when single_ending; one segment per slice tokens[last:cut], from its first id's
        time to its last id's; new_seek = seek + segment_size when single_ending, else seek + (tokens[last_cut - 1] -
        timestamp_begin) * input_stride — the tokens behind the last cut are dropped and decoded again with the next window;
      cuts empty: one segment with all the tokens, from seek * frame_s for segment_size * frame_s — or, if the last timestamp of the
        row exists and is not timestamp_begin itself, for that timestamp's time; new_seek = seek + segment_size.
    timestamp_begin None (upstream's without_timestamps): no id is a timestamp, the second branch always applies.
    Deviation from upstream, stated: if new_seek == seek (a window that closes at <|0.00|>) the window is stepped over whole,
    new_seek = seek + segment_size — upstream would decode the same window forever.
    return_single_ending: -> (segments, new_seek, single_ending), for the word-timestamp seek rule of `transcribe`."""
    toks = [int(t) for t in tokens]
    seek, size = int(seek), int(segment_size)
    if size < 1:
        raise ValueError(f"segment_size must be >= 1, got {segment_size}")
    offset = seek * frame_s
    tsb = None if timestamp_begin is None else int(timestamp_begin)
    ts = [tsb is not None and t >= tsb for t in toks]
    single_ending = ts[-2:] == [False, True]
    cuts = [i + 1 for i in range(len(toks) - 1) if ts[i] and ts[i + 1]]
    segments = []
    if cuts:
        if single_ending:
            cuts.append(len(toks))
        last = 0
        for cut in cuts:
            piece = toks[last:cut]
            segments.append({"seek": seek, "start": offset + (piece[0] - tsb) * time_precision,
                             "end": offset + (piece[-1] - tsb) * time_precision, "tokens": piece})
            last = cut
        new_seek = seek + size if single_ending else seek + (toks[last - 1] - tsb) * int(input_stride)
    else:
        duration = size * frame_s
        stamps = [t for t, is_ts in zip(toks, ts) if is_ts]
        if stamps and stamps[-1] != tsb:
            duration = (stamps[-1] - tsb) * time_precision
        segments.append({"seek": seek, "start": offset, "end": offset + duration, "tokens": toks})
        new_seek = seek + size
    if new_seek == seek:
        new_seek = seek + size
    return (segments, new_seek, single_ending) if return_single_ending else (segments, new_seek)


# ============================================================================= the long log-mel
def long_logmel(audio, filters: torch.Tensor) -> torch.Tensor:
    """Upstream's `log_mel_spectrogram(audio, padding=N_SAMPLES)` for ONE recording (1-D f32, 16 kHz; a tensor or an array)
    -> f32 [n_mels, content_frames + 3000] on the device of `filters`, content_frames = len(audio) // 160.

    The recording is cut to a multiple of 160 samples, 480 000 zeros are appended and wft_logmel runs once with B = 1, so the
    maximum behind the `max - 8` floor is taken over the whole recording, as upstream takes it.  The cut is exact: a frame it could
    touch reads only the zero padding (upstream drops the last STFT frame for the same reason), and the kernel's reflection at the
    far end sees zeros too."""
    a = torch.as_tensor(audio)
    if a.dim() != 1 or a.dtype != torch.float32:
        raise ValueError(f"a recording must be a 1-D float32 tensor or array, got {a.dtype} {tuple(a.shape)}")
    frames = a.numel() // HOP_LENGTH
    dev = filters.device
    padded = torch.zeros(frames * HOP_LENGTH + N_SAMPLES, dtype=torch.float32, device=dev)
    padded[:frames * HOP_LENGTH].copy_(a[:frames * HOP_LENGTH])
    return K.logmel(padded.view(1, -1), filters, n_frames=frames + N_FRAMES)[0]


class LongMel:
    """The packed long log-mels of A recordings, as wft_mel_windows reads them: `mel` f32 1-D, recording a = [n_mels, ld_frames[a]]
    from element mel_off[a]; content_frames[a] = ld_frames[a] - 3000.  The three tables live on the device and, as `host`, here."""

    def __init__(self, mels: Sequence[torch.Tensor]):
        if not mels:
            raise ValueError("at least one recording is needed")
        n_mels = int(mels[0].shape[0])
        if any(m.dim() != 2 or m.shape[0] != n_mels or m.shape[1] < N_FRAMES or m.dtype != torch.float32 for m in mels):
            raise ValueError(f"every long log-mel must be f32 [{n_mels}, >= {N_FRAMES}]")
        dev = mels[0].device
        self.n_mels = n_mels
        lds = [int(m.shape[1]) for m in mels]
        offs = [0]
        for ld in lds[:-1]:
            offs.append(offs[-1] + n_mels * ld)
        self.host = (offs, lds, [ld - N_FRAMES for ld in lds])
        self.mel = torch.cat([m.reshape(-1) for m in mels])
        self.mel_off = torch.tensor(offs, dtype=torch.int64, device=dev)
        self.ld_frames = torch.tensor(lds, dtype=torch.int32, device=dev)
        self.content_frames = torch.tensor(self.host[2], dtype=torch.int32, device=dev)

    def windows(self, audio: Sequence[int], seek: Sequence[int]) -> torch.Tensor:
        """f32 [R, n_mels, 3000]: row r = recording audio[r] from frame seek[r], zero behind its content (K.mel_windows)."""
        return K.mel_windows(self.mel, self.mel_off, self.ld_frames, self.content_frames, audio, seek, self.n_mels, N_FRAMES, host=self.host)


def pack_logmels(audios, filters: torch.Tensor) -> LongMel:
    """`long_logmel` of every recording (ragged lengths), packed for wft_mel_windows."""
    return LongMel([long_logmel(a, filters) for a in audios])


# ============================================================================= language detection
def _check_mode(model, who: str) -> None:
    if getattr(model, "compute_dtype", "bf16") != "bf16":
        raise NotImplementedError(f"{who} runs in the bf16 compute mode only: wft_lang_probs reads bf16 logits and the window decoders "
                                  "(csrc/decode_*.hip) are bf16; call model.set_compute_dtype('bf16')")


@torch.no_grad()
def detect_language(model, mel: torch.Tensor, *, sot: int, language_tokens: Sequence[int], _xa: Optional[torch.Tensor] = None):
    """Upstream's `detect_language` -> (lang_token i64 [B], probs f32 [B, n_lang]).

    mel f32 [B, n_mels, 3000].  The encoder runs once (`_xa`: its output, when the caller has it already), the decoder makes one
    teacher-forced pass over the single token `sot`, that row goes through the tied logits product, and wft_lang_probs takes the
    softmax and the argmax over the `language_tokens` columns (strictly increasing ids; ties go to the lowest).  probs[b, j]
    belongs to language_tokens[j].  eval() semantics; the fp32 compute mode raises NotImplementedError."""
    _check_mode(model, "detect_language")
    V = model.dims.n_vocab
    if not 0 <= int(sot) < V:
        raise ValueError(f"sot={sot} is outside the vocabulary")
    was_training = model.training
    model.eval()
    try:
        xa = model.encoder(mel) if _xa is None else _xa
        tokens = torch.full((xa.shape[0], 1), int(sot), dtype=torch.int64, device=xa.device)
        logits = model.decoder.padded_logits(model.decoder.hidden(tokens, xa))
        probs, best = K.lang_probs(logits, V, language_tokens)
    finally:
        model.train(was_training)
    return best, probs


# ============================================================================= transcribe
def _per_recording(sot_sequence, n: int) -> list:
    seq = list(sot_sequence)
    if seq and isinstance(seq[0], (list, tuple)):
        rows = [[int(t) for t in row] for row in seq]
        if len(rows) != n:
            raise ValueError(f"sot_sequence: one sequence, or one per recording ({n}), got {len(rows)}")
    else:
        rows = [[int(t) for t in seq] for _ in range(n)]
    if any(not row for row in rows):
        raise ValueError("sot_sequence must not be empty")
    return rows


def _is_file(a) -> bool:
    """An entry of `audio` that names or holds a WAV file: a path (str / PathLike) or the bytes of the file."""
    return isinstance(a, (str, bytes)) or hasattr(a, "__fspath__")


def _to_list(v):
    return v.tolist() if hasattr(v, "tolist") else list(v)


def get_end(segments: Sequence[dict]) -> Optional[float]:
    """Upstream's `get_end`: the end of the last word of the segments, else the last segment's end; None without segments."""
    for seg in reversed(segments):
        if seg.get("words"):
            return seg["words"][-1]["end"]
    return segments[-1]["end"] if segments else None


def _next_words_segment(segments: Sequence[dict]) -> Optional[dict]:
    return next((s for s in segments if s.get("words")), None)


def word_seek(segments: list, *, seek: int, new_seek: int, segment_size: int, single_ending: bool, content_frames: int,
              last_speech_timestamp: float, threshold: Optional[float], frame_s: float = 0.01):
    """Upstream's seek rules of a window whose segments carry `words` (after `add_word_timestamps`) -> (new_seek, segments).

    seek: the frame the window started at; new_seek: what `advance_window` gave.  With time_offset = seek * frame_s:
      * not single_ending and get_end(segments) > time_offset: new_seek = round(get_end / frame_s) — the window did not close on a
        timestamp of its own, so the next one starts where the last word ends;
      * threshold (hallucination_silence_threshold) set: in that same case new_seek stays at the last word end only if the window
        goes on for more than `threshold` seconds behind it, otherwise it is seek + segment_size; if the first segment with words
        is anomalous (`is_segment_anomaly`) and starts more than `threshold` behind time_offset, new_seek = seek + round(gap /
        frame_s) and the window emits nothing: (new_seek, None); otherwise the first anomalous segment with silence before and
        after it (transcribe's docstring has the two tests) is dropped together with everything behind it, new_seek =
        round(max(time_offset + 1, its start) / frame_s), or content_frames if less than `threshold` of content is left behind it."""
    time_offset = seek * frame_s
    per_second = round(1.0 / frame_s)
    if not single_ending:
        end = get_end(segments)
        if end is not None and end > time_offset:
            new_seek = round(end * per_second)
    if threshold is None:
        return new_seek, segments
    window_end = (seek + N_FRAMES) * frame_s
    if not single_ending:
        end = get_end(segments)
        if end is not None and end > time_offset:
            new_seek = round(end * per_second) if window_end - end > threshold else seek + segment_size
    first = _next_words_segment(segments)
    if first is not None and D.is_segment_anomaly(first):
        gap = first["start"] - time_offset
        if gap > threshold:
            return seek + round(gap * per_second), None
    hal_last_end = last_speech_timestamp
    for si, seg in enumerate(segments):
        if not seg["words"]:
            continue
        if D.is_segment_anomaly(seg):
            nxt = _next_words_segment(segments[si + 1:])
            next_start = nxt["words"][0]["start"] if nxt is not None else time_offset + segment_size * frame_s
            silence_before = seg["start"] - hal_last_end > threshold or seg["start"] < threshold or seg["start"] - time_offset < 2.0
            silence_after = next_start - seg["end"] > threshold or D.is_segment_anomaly(nxt) or window_end - seg["end"] < 2.0
            if silence_before and silence_after:
                new_seek = round(max(time_offset + 1, seg["start"]) * per_second)
                if content_frames * frame_s - seg["end"] < threshold:
                    new_seek = content_frames
                return new_seek, segments[:si]
        hal_last_end = seg["end"]
    return new_seek, segments


def _align_windows(model, align, mel, xa, windows: dict, sots: list, split_words, eot: int, no_timestamps: int) -> dict:
    """The alignment pass of one iteration -> {batch row: the window's words, dicts for `add_word_timestamps`}.  One `align` call
    per distinct sot sequence over the rows of `windows` that have a text token; a row without one gets []."""
    texts = {j: [t for seg in w[0] for t in seg["tokens"] if t < eot] for j, w in windows.items()}
    out = {j: [] for j in windows}
    groups = {}
    for j in windows:
        if texts[j]:
            groups.setdefault(tuple(sots[j]), []).append(j)
    for sot, js in groups.items():
        split = [split_words(texts[j] + [eot]) for j in js]
        whole = mel is None or len(js) == mel.shape[0]
        sel = None if whole else torch.tensor(js, device=mel.device)
        found = align(model, mel if whole else mel[sel], [texts[j] for j in js], sot_sequence=list(sot), no_timestamps=no_timestamps, eot=eot,
                      num_frames=[max(2, windows[j][2]) for j in js],  # (a last window of one frame still has one key)
                      word_token_counts=[[len(t) for t in s[1]] for s in split], word_spans="device",
                      _xa=xa if whole else xa[sel])
        for j, (strings, _), words in zip(js, split, found):
            out[j] = [{"word": s, "tokens": list(ids), "start": start, "end": end, "probability": p}
                      for s, (start, end, p, ids) in zip(strings[:-1], words)]
    return out


@torch.no_grad()
def transcribe(model, audio, *, sot_sequence, eot: int, timestamp_begin: Optional[int] = None, no_timestamps: Optional[int] = None,
               language_tokens: Optional[Sequence[int]] = None, sot_prev: Optional[int] = None, initial_prompt: Optional[Sequence[int]] = None,
               condition_on_previous_text: bool = True, sample_len: Optional[int] = None, max_windows: Optional[int] = None, text_of=None,
               temperatures=D.UPSTREAM_TEMPERATURES, best_of: int = 5, beam_size: Optional[int] = None, patience: float = 1.0,
               length_penalty: Optional[float] = None, logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6,
               compression_ratio_threshold: Optional[float] = None, no_speech: Optional[int] = None, seed: int = 0, suppress: Sequence[int] = (),
               suppress_first: Sequence[int] = (), max_initial_timestamp_index: Optional[int] = 50, sync_every: int = 8, step: str = "eager",
               weights: str = "bf16", filters: Optional[torch.Tensor] = None, sample_rate=SAMPLE_RATE, word_timestamps: bool = False, split_words=None,
               prepend_punctuations: str = D.PREPEND_PUNCTUATIONS, append_punctuations: str = D.APPEND_PUNCTUATIONS,
               hallucination_silence_threshold: Optional[float] = None, audio_channel="mean", _decode=None, _detect=None, _align=None,
               _frames: Optional[Sequence[int]] = None) -> list:
    """Upstream's `transcribe()` over one recording or a list of them -> one dict per recording, in input order:
      "language": the detected language token id (None without `language_tokens`), "language_probs": f32 [n_lang] or None,
      "segments": [{"seek", "start", "end", "tokens", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob"}],
      "tokens": all segment tokens concatenated, "windows": how many windows were decoded, "truncated": True if `max_windows`
      stopped the recording before its end.

    audio: one 1-D f32 tensor / array, or a list of them with ragged lengths, at `sample_rate` Hz: one integer for all recordings
    or one per recording, each inside [1000, 384000] (default 16000).  A recording at another rate than 16 kHz is resampled on the
    device (data.gpu_frontend.resample: one wft_resample_f32 launch) before its long log-mel, so its content_frames =
    ceil(len * 16000 / rate) // 160; at 16 kHz nothing runs differently.  An entry may also be a WAV file: a `str` / `PathLike`
    path or the `bytes` of the file (data/audio_io.py parse_wav says what is read).  The file entries of a call are decoded and
    downmixed on the device in one launch (data.gpu_frontend: wft_pcm_decode_f32; `audio_channel`: "mean" or the index of one
    channel), each at the rate of its header, and then go the way of an array declared at that rate — so the result is bit-equal
    to a call with the decoded arrays and `sample_rate=[...]`.  With a file entry `sample_rate` must be left at its default
    (ValueError otherwise); array entries of the same list are at 16 kHz.  sot_sequence: one sequence for all
    recordings or one per recording, e.g. (sot, language, task); with `language_tokens` the language is detected on each recording's
    first window (`detect_language`, sot = sot_sequence[0]) and replaces sot_sequence[1] of that recording.  Ids in, ids out:
    `text_of` (ids -> str) is needed only for `compression_ratio_threshold` and for the blank-text rule below.  `no_speech`: the id
    whose probability at the sot position is the window's no-speech probability (None: the silence skip never fires).  The ladder
    keywords (temperatures, best_of, beam_size, patience, length_penalty, the three thresholds, seed), `suppress`,
    `suppress_first`, `max_initial_timestamp_index`, `sync_every`, `step` and `weights` ("int8": the cached steps of every window read int8 weights, needs step="graph"; "w8a8": in addition the encoder
    of every window — language detection's and word_timestamps' included — and the prefill run int8 x int8, decode.encode / decode.int8_gemm; the alignment
    pass of word_timestamps stays bf16) are those of `decode_with_fallback`.  `filters`:
    the mel filterbank f32 [n_mels, 201] (default: data.gpu_frontend.mel_filters(n_mels)).

    The loop.  Recordings are numbered in input order; the long log-mel of each is computed once (`long_logmel`) and packed;
    content_frames = len(audio) // 160.  Every recording keeps its own seek (frames), token history and prompt-reset mark.
    Iteration i = 0, 1, ...:
      * takes every recording with seek < content_frames that has not decoded `max_windows` windows, in index order, as ONE batch
        (no such recording: the loop ends); a recording that finishes drops out of the later batches;
      * ONE wft_mel_windows call cuts the batch's windows (zero behind a recording's content, as upstream's pad_or_trim);
      * ONE decode_with_fallback call decodes them, with ragged per-row prompts (`window_prompt`, right-padded with eot, their
        lengths as prompt_len), the per-row sot_index for the no-speech probability, seed + i as the seed, and
        max_len = min(n_text_ctx, widest prompt of the batch + sample_len);
      * per row, in upstream's order: the silence skip — no_speech_prob > no_speech_threshold, unless logprob_threshold is set
        and avg_logprob > logprob_threshold, emits no segments and moves seek by the window's segment_size = min(3000,
        content_frames - seek); otherwise `advance_window` gives the segments and the new seek; a segment with start == end, and
        with `text_of` one whose text (of its ids below eot) is blank, loses its tokens but stays in the result; the segment
        tokens join the history; the prompt-reset mark moves to the end of the history if not condition_on_previous_text or the
        window's temperature is > 0.5.  `initial_prompt` ids are put into every history first.
    The encoder runs once per iteration (language detection shares the first iteration's encoder output).

    Deviations from upstream, stated: (1) `sample_len` (default n_text_ctx // 2, as upstream) bounds the row with the WIDEST
    prompt of a batch exactly; max_len is one absolute length per decode call, so a row with a shorter prompt may generate more
    than sample_len tokens.  (2) The zero-advance guard of `advance_window`.  (3) Recordings share batches, so a window's bits can
    depend on its batch partners through the GEMM shapes; replaying the same batches gives the same bits.  (4) Without
    `text_of` no compression ratio exists and the blank-text rule is off.  A recording shorter than one frame decodes nothing.
    The fp32 compute mode raises NotImplementedError.  (`_decode`, `_detect`, `_align`, `_frames`: stand-ins for
    decode_with_fallback, detect_language, find_alignment and the content frames — the host tests drive the loop through them
    without a device.)

    word_timestamps=True (upstream's rules restated; parity with its binary is unpinned) needs `split_words`: ids + [eot] ->
    (words, word_tokens), the tokenizer's `split_to_word_tokens` — one string and one id list per word, the eot last — plus
    `timestamp_begin` and `no_timestamps`; `hallucination_silence_threshold` needs word_timestamps; each raises ValueError
    otherwise.  With word_timestamps=False nothing runs differently.  With it, per iteration:
      * the encoder runs once, xa = model.encoder(mel); the decode call and the alignment call both get `_xa=xa`;
      * behind the silence skip and `advance_window` of every row, ONE `find_alignment(word_spans="device")` call per distinct
        sot sequence (after language detection usually one) covers the rows that have a text token: num_frames = the row's
        segment_size, text_tokens = the ids below eot of the row's segments concatenated, word_token_counts from `split_words`;
        a row without a text token gets words = [] on all its segments;
      * then per row, in upstream's order: (1) `add_word_timestamps` with time_offset = seek * 0.01 and the recording's running
        last_speech_timestamp (0.0 at first), which gives every segment its "words": [{"word", "tokens", "start", "end",
        "probability"}] and may move the segment's start and end; (2) if the window did not end on a single timestamp and the
        end of its last word (`get_end`: else of its last segment) is > time_offset, seek = round(that end * 100); (3) with a
        threshold, the hallucination rules of `word_seek`: that seek stays only if the window goes on for more than the
        threshold behind the last word, else seek = previous seek + segment_size; an anomalous first segment
        (`is_segment_anomaly`) more than the threshold behind the window start moves seek to previous seek + round(gap * 100)
        and the window emits nothing; otherwise the first anomalous segment with silence_before = seg.start - hal_last_end >
        threshold or seg.start < threshold or seg.start - time_offset < 2.0 and silence_after = next_start - seg.end > threshold
        or the next segment with words is anomalous or window_end - seg.end < 2.0 is dropped with all later segments, seek =
        round(max(time_offset + 1, seg.start) * 100), or content_frames if content_duration - seg.end < threshold (hal_last_end:
        the end of the segment with words before it, first last_speech_timestamp; next_start: the first word start of the next
        segment with words, else the end of the window's content; window_end = (previous seek + 3000) * 0.01);
        (4) last_speech_timestamp = `get_end` of what is left; (5) the blank-segment cleanup also empties "words".
      The zero-advance guard holds behind all of it: a seek that did not move goes to previous seek + segment_size.
    Deviation (5): one alignment call covers the rows of a batch, so a window's word times and probabilities can depend on its
    batch partners through the GEMM shapes, as for decoding; replaying the same batches gives the same bits.  As upstream,
    `add_word_timestamps` does not hand its own last_speech_timestamp back to the loop: only step (4) moves the running value."""
    _check_mode(model, "transcribe")
    D._check_mode(model, "transcribe", step, sync_every, weights)
    single = isinstance(audio, torch.Tensor) and audio.dim() == 1 or (not isinstance(audio, (list, tuple)) and getattr(audio, "ndim", 0) == 1)
    single = single or _is_file(audio)
    audios = [audio] if single else list(audio)
    files = [k for k, a in enumerate(audios) if _is_file(a)]
    n = len(audios)
    if n < 1:
        raise ValueError("transcribe needs at least one recording")
    n_ctx = int(model.dims.n_text_ctx)
    sots = _per_recording(sot_sequence, n)
    if sample_len is None:
        sample_len = n_ctx // 2
    if isinstance(sample_len, bool) or not isinstance(sample_len, int) or sample_len < 1:
        raise ValueError(f"sample_len must be a positive integer, got {sample_len!r}")
    if max_windows is not None and (isinstance(max_windows, bool) or not isinstance(max_windows, int) or max_windows < 1):
        raise ValueError(f"max_windows must be None or a positive integer, got {max_windows!r}")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"seed must be an integer, got {seed!r}")
    if compression_ratio_threshold is not None and text_of is None:
        raise ValueError("compression_ratio_threshold needs text_of (ids -> str): the ratio is taken over the decoded text")
    if language_tokens is not None:
        language_tokens = [int(t) for t in language_tokens]
        if any(len(s) < 2 for s in sots) or len({s[0] for s in sots}) != 1:
            raise ValueError("language detection replaces sot_sequence[1]: every sot_sequence needs two ids and the same first id")
    longest = 1 + (n_ctx // 2 - 1) + max(len(s) for s in sots) if sot_prev is not None else max(len(s) for s in sots)
    if longest >= n_ctx:
        raise ValueError(f"sot_sequence of {max(len(s) for s in sots)} ids leaves no room to generate inside n_text_ctx = {n_ctx}")
    from ..data.gpu_frontend import check_rate

    if files and (isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate != SAMPLE_RATE):
        raise ValueError("sample_rate must be left at its default when an entry of audio is a file: a file's rate comes from its header "
                         "(array entries of the same list are at 16 kHz)")
    if isinstance(sample_rate, (list, tuple)) or getattr(sample_rate, "ndim", 0) == 1:
        rates = [check_rate(r) for r in sample_rate]
        if len(rates) != n:
            raise ValueError(f"sample_rate: one rate, or one per recording ({n}), got {len(rates)}")
    else:
        rates = [check_rate(sample_rate)] * n
    if word_timestamps:
        if split_words is None:
            raise ValueError("word_timestamps needs split_words (ids + [eot] -> (words, word_tokens)): the tokenizer's split_to_word_tokens")
        if timestamp_begin is None or no_timestamps is None:
            raise ValueError("word_timestamps needs timestamp_begin and no_timestamps: the alignment pass runs behind the no-timestamps token")
    elif hallucination_silence_threshold is not None:
        raise ValueError("hallucination_silence_threshold needs word_timestamps=True: the rule reads the word times")
    decode = D.decode_with_fallback if _decode is None else _decode
    detect = detect_language if _detect is None else _detect
    align = D.find_alignment if _align is None else _align
    last_speech = [0.0] * n

    packed = None
    if _frames is None:
        if filters is None:
            from ..data.gpu_frontend import mel_filters

            filters = mel_filters(model.dims.n_mels).to(model.device)
        if files:  # one copy of the file bytes, one decode launch; every file then goes on at the rate of its header
            from ..data.gpu_frontend import _decode_files

            decoded, infos = _decode_files([audios[k] for k in files], audio_channel, filters.device, "transcribe")
            for k, a, info in zip(files, decoded, infos):
                audios[k], rates[k] = a, check_rate(info.sample_rate)
        if any(r != SAMPLE_RATE for r in rates):
            from ..data.gpu_frontend import resample

            audios = [a if r == SAMPLE_RATE else resample(a, r, device=filters.device) for a, r in zip(audios, rates)]
        packed = pack_logmels(audios, filters)
        frames = list(packed.host[2])
    else:
        frames = [int(f) for f in _frames]
        if len(frames) != n:
            raise ValueError(f"_frames: one frame count per recording ({n}), got {len(frames)}")

    history = [[int(t) for t in (initial_prompt or ())] for _ in range(n)]
    reset = [0] * n
    seek = [0] * n
    results = [{"language": None, "language_probs": None, "segments": [], "tokens": [], "windows": 0, "truncated": False} for _ in range(n)]
    shared = dict(temperatures=temperatures, best_of=best_of, beam_size=beam_size, patience=patience, length_penalty=length_penalty,
                  logprob_threshold=logprob_threshold, no_speech_threshold=no_speech_threshold,
                  compression_ratio_threshold=compression_ratio_threshold, text_of=text_of, no_speech=no_speech, eot=int(eot),
                  suppress=suppress, suppress_first=suppress_first, sync_every=sync_every, step=step, timestamp_begin=timestamp_begin,
                  no_timestamps=no_timestamps, max_initial_timestamp_index=max_initial_timestamp_index)
    if weights != "bf16":
        shared["weights"] = weights
    was_training = model.training
    model.eval()
    try:
        i = 0
        while True:
            rows = [a for a in range(n) if seek[a] < frames[a] and (max_windows is None or results[a]["windows"] < max_windows)]
            if not rows:
                break
            mel = None if packed is None else packed.windows(rows, [seek[a] for a in rows])
            xa = None
            if i == 0 and language_tokens is not None:
                xa = None if packed is None else D.encode(model, mel, weights)
                best, probs = detect(model, mel, sot=sots[rows[0]][0], language_tokens=language_tokens, _xa=xa)
                best, probs = _to_list(best), (probs.cpu() if hasattr(probs, "cpu") else probs)
                for j, a in enumerate(rows):
                    results[a]["language"], results[a]["language_probs"] = int(best[j]), probs[j]
                    sots[a][1] = int(best[j])
            prompts = [window_prompt(history[a], reset[a], sots[a], sot_prev, n_ctx) for a in rows]
            width = max(len(p) for p, _ in prompts)
            prompt = torch.full((len(rows), width), int(eot), dtype=torch.int64)
            for j, (p, _) in enumerate(prompts):
                prompt[j, :len(p)] = torch.tensor(p, dtype=torch.int64)
            plen = [len(p) for p, _ in prompts]
            kw = dict(shared, sot_index=[s for _, s in prompts], seed=seed + i, max_len=min(n_ctx, width + sample_len))
            if word_timestamps and xa is None and packed is not None:
                xa = D.encode(model, mel, weights)
            if xa is not None:
                kw["_xa"] = xa
            toks, lens, _, info = decode(model, mel, prompt if mel is None else prompt.to(mel.device), torch.tensor(plen), **kw)
            toks, lens = _to_list(toks), _to_list(lens)
            windows = {}  # batch row j -> (segments, seek before, segment_size, single_ending) of a row that was not skipped
            for j, a in enumerate(rows):
                ids, _ = D.generated_ids(toks[j], plen[j], lens[j], eot)
                size = min(N_FRAMES, frames[a] - seek[a])
                results[a]["windows"] += 1
                nsp, alp = info["no_speech_prob"][j], info["avg_logprob"][j]
                skip = no_speech_threshold is not None and nsp is not None and nsp > no_speech_threshold
                if skip and logprob_threshold is not None and alp > logprob_threshold:
                    skip = False
                if skip:
                    seek[a] += size
                    continue
                before = seek[a]
                segments, seek[a], single = advance_window(ids, seek=before, segment_size=size, timestamp_begin=timestamp_begin,
                                                           return_single_ending=True)
                windows[j] = (segments, before, size, single)
            aligned = _align_windows(model, align, mel, xa, windows, [sots[a] for a in rows], split_words, int(eot), no_timestamps) \
                if word_timestamps else {}
            for j, a in enumerate(rows):
                if j not in windows:
                    continue
                segments, before, size, single = windows[j]
                res = results[a]
                nsp, alp, temp = info["no_speech_prob"][j], info["avg_logprob"][j], info["temperature"][j]
                if word_timestamps:
                    D.add_word_timestamps(segments, aligned[j], time_offset=before * 0.01, last_speech_timestamp=last_speech[a], eot=int(eot),
                                          prepend_punctuations=prepend_punctuations, append_punctuations=append_punctuations)
                    seek[a], segments = word_seek(segments, seek=before, new_seek=seek[a], segment_size=size, single_ending=single,
                                                  content_frames=frames[a], last_speech_timestamp=last_speech[a],
                                                  threshold=hallucination_silence_threshold)
                    if seek[a] <= before:  # the zero-advance guard, after every seek rule
                        seek[a] = before + size
                    if segments is None:  # an anomalous first segment behind a silence: the window emits nothing
                        continue
                    end = get_end(segments)
                    if end is not None:
                        last_speech[a] = end
                for seg in segments:
                    blank = text_of is not None and text_of([t for t in seg["tokens"] if t < int(eot)]).strip() == ""
                    if seg["start"] == seg["end"] or blank:
                        seg["tokens"] = []
                        if word_timestamps:
                            seg["words"] = []
                    seg.update(temperature=temp, avg_logprob=alp, compression_ratio=info["compression_ratio"][j], no_speech_prob=nsp)
                    res["segments"].append(seg)
                    res["tokens"].extend(seg["tokens"])
                    history[a].extend(seg["tokens"])
                if not condition_on_previous_text or temp > 0.5:
                    reset[a] = len(history[a])
            i += 1
    finally:
        model.train(was_training)
    for a in range(n):
        results[a]["truncated"] = seek[a] < frames[a]
    return results
