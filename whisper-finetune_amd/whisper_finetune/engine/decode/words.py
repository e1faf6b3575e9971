"""Word-level timestamps: the alignment-head capture, `find_alignment`, and upstream's string-level rules on top of its words."""
from __future__ import annotations

import contextlib
import threading
from typing import Optional, Sequence

import torch

from .. import kernels as K

_TLS = threading.local()  # the capture of the running find_alignment pass (capture_alignment)

# ============================================================================= word-level timestamps
# Upstream's `whisper/timing.py: find_alignment`, restated (openai-whisper is not a dependency: parity with its binary is unpinned).
# Device stages: csrc/align.hip (include/wft.h "Word-level alignment"); the rest is upstream's numpy on the host, or — with
# word_spans="device" — wft_word_spans.  Upstream's string-level post-processing is restated as pure host functions below
# `alignment_words`: `merge_punctuations`, `add_word_timestamps` (the long-word clamps, the segment-edge preference) and the
# anomaly scores of its hallucination filter; engine/transcribe.py calls them per window.
TOKENS_PER_SECOND = 50  # one cross-attention frame = 20 ms
PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
SENTENCE_END_MARKS = ".。!！?？"


def dump_alignment_heads(mask) -> bytes:
    """A bool [n_text_layer, n_text_head] mask -> upstream's dump format: base85 of the gzipped bool bytes."""
    import base64
    import gzip

    import numpy as np

    return base64.b85encode(gzip.compress(np.ascontiguousarray(np.asarray(mask, dtype=bool)).tobytes()))


def parse_alignment_heads(heads, n_layer: int, n_head: int) -> torch.Tensor:
    """A bool [n_layer, n_head] mask (tensor, array, nested list) or upstream's base85-gzip dump of one -> bool tensor [n_layer, n_head]."""
    if isinstance(heads, (bytes, str)):
        import base64
        import gzip

        import numpy as np

        arr = np.frombuffer(gzip.decompress(base64.b85decode(heads)), dtype=bool).copy()
        if arr.size != n_layer * n_head:
            raise ValueError(f"alignment-head dump holds {arr.size} entries, the model has {n_layer} x {n_head} heads")
        return torch.from_numpy(arr).reshape(n_layer, n_head)
    if isinstance(heads, torch.Tensor) and heads.is_sparse:
        heads = heads.to_dense()
    mask = torch.as_tensor(heads).cpu()
    if mask.dtype != torch.bool or tuple(mask.shape) != (n_layer, n_head):
        raise ValueError(f"alignment heads must be a bool [{n_layer}, {n_head}] mask or a base85 dump, got {mask.dtype} {tuple(mask.shape)}")
    return mask.clone()


class AlignCapture:
    """What one `find_alignment` pass collects: for every cross-attention module named in `slots` the probabilities of its
    alignment heads go into that module's slice of `probs` [B, n_sel, Tq, Tk] (K.attn_probs on the q / kv the module has at hand)."""

    def __init__(self, slots: dict, probs: torch.Tensor, n_tok, n_key, host_lens, scale: float, keep_views: bool):
        self.slots, self.probs, self.n_tok, self.n_key, self.host_lens, self.scale = slots, probs, n_tok, n_key, host_lens, scale
        self.views = {} if keep_views else None

    def record(self, module, q: torch.Tensor, k: torch.Tensor, n_head: int) -> None:
        slot = self.slots.get(module)
        if slot is None:
            return
        heads, at = slot
        K.attn_probs(q, k, heads, self.n_tok, self.n_key, n_head, self.scale, self.probs[:, at:at + heads.numel()], host_lens=self.host_lens)
        if self.views is not None:
            self.views[module] = (q, k)


def alignment_capture() -> Optional[AlignCapture]:
    return getattr(_TLS, "align_capture", None)


@contextlib.contextmanager
def capture_alignment(cap: AlignCapture):
    """Inside this context, under torch.no_grad(), the uncached cross-attention forward of every module `cap` names also writes its
    alignment-head probabilities.  Thread-local, in the style of runtime.exchange_launch_mode: nothing is stored in the library or
    on a module, and outside it nothing runs differently."""
    old = alignment_capture()
    _TLS.align_capture = cap
    try:
        yield cap
    finally:
        _TLS.align_capture = old


def alignment_words(path_text, path_time, word_token_counts, token_probs, text) -> list:
    """Upstream's host arithmetic behind the DTW path of ONE audio -> [(start_s, end_s, probability, [token ids])].
    path_text / path_time: the path in forward order (row 0 = the no-timestamps token, then the text tokens); word_token_counts: the
    tokens per word over text + [eot] (the last word, the eot, is dropped as upstream drops it); token_probs: one per text token."""
    import numpy as np

    counts = [int(c) for c in word_token_counts]
    if len(counts) <= 1:
        return []
    if sum(counts) != len(text) + 1 or min(counts) < 1:
        raise ValueError(f"word_token_counts {counts} must be positive and sum to len(text) + 1 = {len(text) + 1}")
    ti, tj = np.asarray(path_text, dtype=np.int64), np.asarray(path_time, dtype=np.int64)
    bounds = np.pad(np.cumsum(counts[:-1]), (1, 0))
    jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
    jump_times = tj[jumps] / TOKENS_PER_SECOND
    starts, ends = jump_times[bounds[:-1]], jump_times[bounds[1:]]
    probs = np.asarray(token_probs, dtype=np.float64)
    return [(float(s), float(e), float(np.mean(probs[i:j])), [int(t) for t in text[i:j]])
            for s, e, i, j in zip(starts, ends, bounds[:-1], bounds[1:])]


def merge_punctuations(words: list, prepended: str = PREPEND_PUNCTUATIONS, appended: str = APPEND_PUNCTUATIONS) -> None:
    """Upstream's `merge_punctuations`, in place, over word dicts {"word", "tokens", ...}: times and probabilities are not touched.
    Backward pass: a word that starts with " " and whose strip() is in `prepended` gives its string and tokens to the front of the
    word that follows it and is emptied (word "", tokens []).  Forward pass: a word that is in `appended` is added to the end of
    the word before it — unless that one ends with " " — and is emptied.  Emptied words stay in the list."""
    i, j = len(words) - 2, len(words) - 1
    while i >= 0:
        prev, nxt = words[i], words[j]
        if prev["word"].startswith(" ") and prev["word"].strip() in prepended:
            nxt["word"] = prev["word"] + nxt["word"]
            nxt["tokens"] = prev["tokens"] + nxt["tokens"]
            prev["word"], prev["tokens"] = "", []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(words):
        prev, nxt = words[i], words[j]
        if not prev["word"].endswith(" ") and nxt["word"] in appended:
            prev["word"] = prev["word"] + nxt["word"]
            prev["tokens"] = prev["tokens"] + nxt["tokens"]
            nxt["word"], nxt["tokens"] = "", []
        else:
            i = j
        j += 1


def add_word_timestamps(segments: list, alignment: list, *, time_offset: float, last_speech_timestamp: float, eot: Optional[int] = None,
                        prepend_punctuations: str = PREPEND_PUNCTUATIONS, append_punctuations: str = APPEND_PUNCTUATIONS) -> float:
    """Upstream's `add_word_timestamps` behind its `find_alignment` call, for the segments of ONE window -> last_speech_timestamp.

    alignment: the words of the window in order, dicts {"word": str, "tokens": [ids], "start", "end", "probability"} with times in
    seconds from the start of the window — `find_alignment` over the concatenated text tokens (ids < eot) of the segments, joined
    with the strings of `split_words`.  It is edited in place.  A segment's text tokens are its ids below `eot` (None: all of them).
      1. durations = end - start of the words where that is not zero; median = min(0.7, median(durations)), 0.0 without any;
         max_duration = 2 * median.
      2. With durations, for i >= 1 and end - start > max_duration: a word that is a sentence mark (".。!！?？") keeps its start,
         end = start + max_duration; else, if word i - 1 is one, start = end - max_duration.
      3. `merge_punctuations`.
      4. Per segment, words are taken until the taken tokens reach the segment's text-token count; a taken word with a non-empty
         string is kept as {"word", "tokens", "start": round(time_offset + start, 2), "end": round(time_offset + end, 2),
         "probability"}.  For a segment with words w0 .. wl, in this order:
         (a) after a pause — w0.end - last_speech_timestamp > 4 * median — with w0 longer than max_duration, or w0 and w1 together
             longer than 2 * max_duration: if w1 is longer than max_duration, w0.end = w1.start = max(w1.end / 2, w1.end -
             max_duration); then w0.start = max(0, w0.end - max_duration);
         (b) seg.start < w0.end and seg.start - 0.5 > w0.start: w0.start = max(0, min(w0.end - median, seg.start)); otherwise
             seg.start = w0.start;
         (c) seg.end > wl.start and seg.end + 0.5 < wl.end: wl.end = max(wl.start + median, seg.end); otherwise seg.end = wl.end;
         (d) last_speech_timestamp = seg.end.
      Every segment gets seg["words"]."""
    import numpy as np

    if not segments:
        return last_speech_timestamp
    durations = np.array([w["end"] - w["start"] for w in alignment], dtype=np.float64)
    durations = durations[durations.nonzero()]
    median = min(0.7, float(np.median(durations))) if len(durations) else 0.0
    max_duration = median * 2
    if len(durations):
        for i in range(1, len(alignment)):
            w = alignment[i]
            if w["end"] - w["start"] > max_duration:
                if w["word"] in SENTENCE_END_MARKS:
                    w["end"] = w["start"] + max_duration
                elif alignment[i - 1]["word"] in SENTENCE_END_MARKS:
                    w["start"] = w["end"] - max_duration
    merge_punctuations(alignment, prepend_punctuations, append_punctuations)
    at = 0
    for seg in segments:
        n_text = sum(1 for t in seg["tokens"] if eot is None or t < eot)
        saved, words = 0, []
        while at < len(alignment) and saved < n_text:
            w = alignment[at]
            if w["word"]:
                words.append({"word": w["word"], "tokens": list(w["tokens"]), "start": round(time_offset + w["start"], 2),
                              "end": round(time_offset + w["end"], 2), "probability": w["probability"]})
            saved += len(w["tokens"])
            at += 1
        if words:
            if words[0]["end"] - last_speech_timestamp > median * 4 and (
                    words[0]["end"] - words[0]["start"] > max_duration
                    or (len(words) > 1 and words[1]["end"] - words[0]["start"] > max_duration * 2)):
                if len(words) > 1 and words[1]["end"] - words[1]["start"] > max_duration:
                    boundary = max(words[1]["end"] / 2, words[1]["end"] - max_duration)
                    words[0]["end"] = words[1]["start"] = boundary
                words[0]["start"] = max(0, words[0]["end"] - max_duration)
            if seg["start"] < words[0]["end"] and seg["start"] - 0.5 > words[0]["start"]:
                words[0]["start"] = max(0, min(words[0]["end"] - median, seg["start"]))
            else:
                seg["start"] = words[0]["start"]
            if seg["end"] > words[-1]["start"] and seg["end"] + 0.5 < words[-1]["end"]:
                words[-1]["end"] = max(words[-1]["start"] + median, seg["end"])
            else:
                seg["end"] = words[-1]["end"]
            last_speech_timestamp = seg["end"]
        seg["words"] = words
    return last_speech_timestamp


def word_anomaly_score(word: dict) -> float:
    """Upstream's `word_anomaly_score`: 1.0 for a probability below 0.15, (0.133 - d) * 15 for a duration d = end - start below
    0.133 s, d - 2.0 for one above 2.0 s."""
    d = word["end"] - word["start"]
    score = 0.0
    if word.get("probability", 0.0) < 0.15:
        score += 1.0
    if d < 0.133:
        score += (0.133 - d) * 15
    if d > 2.0:
        score += d - 2.0
    return score


def is_segment_anomaly(segment: Optional[dict]) -> bool:
    """Upstream's `is_segment_anomaly`: over the first 8 words of the segment that are not punctuation marks, the summed
    `word_anomaly_score` is >= 3, or (to 0.01) at least the number of those words.  None, or a segment without words: False."""
    if segment is None or not segment.get("words"):
        return False
    words = [w for w in segment["words"] if w["word"] not in PREPEND_PUNCTUATIONS + APPEND_PUNCTUATIONS][:8]
    score = sum(word_anomaly_score(w) for w in words)
    return score >= 3 or score + 0.01 >= len(words)


def alignment_slots(model, device) -> tuple:
    """model.alignment_heads -> ({cross_attn module: (heads i32 on the device, first slice)}, n_sel): the heads of a layer in the
    buffer's order, the layers in ascending order — the order of upstream's `alignment_heads.indices().T`."""
    mask = model.alignment_heads
    mask = (mask.to_dense() if mask.is_sparse else mask).cpu()
    blocks = model.decoder.blocks
    if tuple(mask.shape) != (len(blocks), model.dims.n_text_head):
        raise ValueError(f"alignment_heads {tuple(mask.shape)} does not fit {len(blocks)} decoder layers of {model.dims.n_text_head} heads")
    slots, at = {}, 0
    for layer, block in enumerate(blocks):
        hs = torch.nonzero(mask[layer]).flatten().tolist()
        if hs:
            slots[block.cross_attn] = (torch.tensor(hs, dtype=torch.int32, device=device), at)
            at += len(hs)
    if at == 0:
        raise ValueError("alignment_heads selects no head")
    return slots, at


@torch.no_grad()
def find_alignment(model, mel: torch.Tensor, text_tokens, *, sot_sequence: Sequence[int], no_timestamps: int, eot: int, num_frames,
                   word_token_counts=None, medfilt_width: int = 7, qk_scale: float = 1.0, return_debug: bool = False, word_spans: str = "host",
                   _xa=None):
    """Word-level timestamps for already-decoded text -> per audio [(start_s, end_s, probability, [token ids])].

    mel f32 [B, n_mels, 2 * n_audio_ctx]; text_tokens: one list of text token ids (< eot) per audio, ragged; num_frames: the mel
    frames that hold audio, an int or one per audio (keys at or beyond num_frames // 2 take no part in the softmax);
    word_token_counts: per audio the tokens per word over text + [eot] (what upstream's `tokenizer.split_to_word_tokens` gives;
    None: every token is its own word).  One teacher-forced pass over [*sot_sequence, no_timestamps, *text, eot] (right padding lies
    behind the eot: causal attention never sees it) with the alignment-head probabilities captured (wft_attn_probs_bf16), then
    wft_align_matrix, wft_dtw_f32 on rows len(sot_sequence) .. of the matrix, the paths to the host, `alignment_words` there.  A
    word's probability is the mean over its tokens of softmax(logits[:eot]) at the token's position (wft_token_stats with V = eot).
    An audio with no text gives [].  return_debug adds a dict: "q" / "k" (per captured module, the views the kernel read), "probs",
    "matrix", "paths", "n_tok", "n_key", "rows" (the audios that ran), "token_probs".  Call it in eval mode; the fp32 compute mode raises.

    word_spans="device": the paths and the token probabilities stay on the device, wft_word_spans forms the boundary frames and the
    mean probabilities of all audios in one launch, and only those three word arrays come to the host; times are frame /
    TOKENS_PER_SECOND in Python floats, exactly as `alignment_words` forms them, and the probability is the kernel's fp32 mean (the
    host path takes it in float64: the two differ by rounding only).  `_xa`: the encoder output of `mel`, [B, n_audio_ctx, d],
    when the caller has it already — `embed_audio` is not called and `mel` is not read then, it may be None (engine/transcribe.py
    aligns the window it has just decoded).
    The string-level rules on top of the words are `merge_punctuations` and `add_word_timestamps` above."""
    if getattr(model, "compute_dtype", "bf16") != "bf16":
        raise NotImplementedError("find_alignment runs in the bf16 compute mode only: the alignment kernels (csrc/align.hip) read bf16 q / k; "
                                  "call model.set_compute_dtype('bf16')")
    if word_spans not in ("host", "device"):
        raise ValueError(f"word_spans must be 'host' or 'device', got {word_spans!r}")
    B = mel.shape[0] if _xa is None else _xa.shape[0]
    texts = [[int(t) for t in row] for row in text_tokens]
    if len(texts) != B:
        raise ValueError(f"text_tokens holds {len(texts)} rows for {B} audios")
    sot = [int(t) for t in sot_sequence]
    eot = int(eot)
    frames = [int(num_frames)] * B if isinstance(num_frames, int) else [int(f) for f in num_frames]
    n_ctx, Ta = model.dims.n_text_ctx, model.dims.n_audio_ctx
    if len(frames) != B or any(f < 2 or f // 2 > Ta for f in frames):
        raise ValueError(f"num_frames must be an int or one per audio with 1 <= num_frames // 2 <= {Ta}")
    if any(t < 0 or t >= eot for row in texts for t in row):
        raise ValueError("text tokens must lie in [0, eot)")
    if any(len(sot) + len(row) + 2 > n_ctx for row in texts):
        raise ValueError(f"sot_sequence + no_timestamps + text + eot must fit the text context of {n_ctx}")
    counts = [None] * B if word_token_counts is None else list(word_token_counts)
    if len(counts) != B:
        raise ValueError(f"word_token_counts holds {len(counts)} rows for {B} audios")
    rows = [b for b in range(B) if texts[b]]
    result = [[] for _ in range(B)]
    if not rows:
        return (result, {}) if return_debug else result
    dev = model.device
    n = len(rows)
    head = sot + [int(no_timestamps)]
    lens = [len(head) + len(texts[b]) + 1 for b in rows]
    T = max(lens)
    tokens = torch.full((n, T), eot, dtype=torch.int64)
    for i, b in enumerate(rows):
        tokens[i, :lens[i] - 1] = torch.tensor(head + texts[b], dtype=torch.int64)
    tokens = tokens.to(dev)
    keys = [frames[b] // 2 for b in rows]
    n_tok, n_key = torch.tensor(lens, dtype=torch.int32, device=dev), torch.tensor(keys, dtype=torch.int32, device=dev)
    slots, n_sel = alignment_slots(model, dev)
    probs = torch.zeros((n, n_sel, T, Ta), dtype=torch.float32, device=dev)
    cap = AlignCapture(slots, probs, n_tok, n_key, (lens, keys), 64 ** -0.5 * float(qk_scale), return_debug)
    if _xa is None:
        mel = mel.to(dev)
        xa = model.embed_audio(mel if n == B else mel[torch.tensor(rows, device=dev)])
    else:
        if mel is not None and mel.shape[0] != B:
            raise ValueError(f"_xa holds {B} rows, mel {mel.shape[0]}")
        xa = _xa if n == B else _xa[torch.tensor(rows, device=_xa.device)]
    with capture_alignment(cap):
        h = model.decoder.hidden(tokens, xa)  # [n, T, d]
    matrix = K.align_matrix(probs, n_tok, n_key, medfilt_width, host_lens=(lens, keys))
    n_rows = [len(texts[b]) + 1 for b in rows]
    paths = K.dtw(matrix, len(sot), torch.tensor(n_rows, dtype=torch.int32, device=dev), n_key, host_lens=(n_rows, keys))
    # softmax(logits[:eot]) at the positions that predict the text tokens: position len(sot) + i predicts text[i]
    pos = torch.tensor([i * T + len(sot) + j for i, b in enumerate(rows) for j in range(len(texts[b]))], dtype=torch.int64, device=dev)
    tgt = torch.tensor([t for b in rows for t in texts[b]], dtype=torch.int64, device=dev)
    logits = model.decoder.padded_logits(h.reshape(n * T, -1).index_select(0, pos).view(pos.numel(), 1, -1))
    stats, _ = K.token_stats(logits, tgt, eot)
    if word_spans == "device":
        probs_dev = torch.exp(stats[:, 3] - stats[:, 0]).contiguous()
        wcs = [[int(c) for c in counts[b]] if counts[b] is not None else [1] * (len(texts[b]) + 1) for b in rows]
        for wc, b in zip(wcs, rows):
            if len(wc) > 1 and (sum(wc) != len(texts[b]) + 1 or min(wc) < 1):
                raise ValueError(f"word_token_counts {wc} must be positive and sum to len(text) + 1 = {len(texts[b]) + 1}")
        nw = [max(len(wc) - 1, 0) for wc in wcs]
        bounds = torch.zeros((n, max(nw) + 1 if max(nw) else 2), dtype=torch.int32)
        offs, at = [], 0
        for i, (wc, b) in enumerate(zip(wcs, rows)):
            if nw[i]:
                bounds[i, 1:nw[i] + 1] = torch.cumsum(torch.tensor(wc[:-1], dtype=torch.int32), 0)
            offs.append(at)
            at += len(texts[b])
        sf, ef, pr = K.word_spans(paths, bounds.to(dev), torch.tensor(nw, dtype=torch.int32, device=dev), probs_dev,
                                  torch.tensor(offs, dtype=torch.int32, device=dev), max(n_rows), host_lens=(nw,))
        sf, ef, pr = sf.cpu().tolist(), ef.cpu().tolist(), pr.cpu().tolist()
        for i, b in enumerate(rows):
            bd = bounds[i].tolist()
            result[b] = [(sf[i][w] / TOKENS_PER_SECOND, ef[i][w] / TOKENS_PER_SECOND, pr[i][w], texts[b][bd[w]:bd[w + 1]]) for w in range(nw[i])]
        if not return_debug:
            return result
        token_probs = probs_dev.cpu().tolist()
        pt, pj, pl = (t.cpu() for t in paths)
    else:
        token_probs = torch.exp(stats[:, 3] - stats[:, 0]).cpu().tolist()
        pt, pj, pl = (t.cpu() for t in paths)
        at = 0
        for i, b in enumerate(rows):
            L_ = int(pl[i])
            tp = token_probs[at:at + len(texts[b])]
            at += len(texts[b])
            wc = counts[b] if counts[b] is not None else [1] * (len(texts[b]) + 1)
            result[b] = alignment_words(pt[i, :L_].numpy(), pj[i, :L_].numpy(), wc, tp, texts[b])
    if not return_debug:
        return result
    debug = {"q": {m: v[0] for m, v in cap.views.items()}, "k": {m: v[1] for m, v in cap.views.items()}, "probs": probs, "matrix": matrix,
             "paths": (pt, pj, pl), "n_tok": lens, "n_key": keys, "rows": rows, "token_probs": token_probs, "slots": slots,
             "logits": logits, "token_stats": stats}
    return result, debug
