"""The temperature ladder `decode_with_fallback` with its host-side result helpers (`needs_fallback`: average log-probability,
compression ratio, no-speech probability), and `timestamp_segments`."""
from __future__ import annotations

from typing import Optional

import torch

from .. import kernels as K
from .beam import beam_candidates, beam_decode
from .greedy import greedy_decode
from .runner import _check_mode, encode
from .sample import _check_sampling, sample_decode


@torch.no_grad()
def no_speech_prob(model, xa: torch.Tensor, prompt: torch.Tensor, sot_index, no_speech: int) -> torch.Tensor:
    """Upstream's `probs_at_sot[:, no_speech]` -> f32 [B]: the probability of the `no_speech` id under the softmax of the logits at
    the start-of-transcript position `sot_index` (an int, or one per row) of the prompt block.  One teacher-forced pass over the
    prompts (right padding lies behind sot: causal attention never sees it), the row at sot_index through the tied logits product,
    exp(x_target - logsumexp) from wft_token_stats.  Call it in eval mode."""
    B, T = prompt.shape
    V = model.dims.n_vocab
    idx = torch.as_tensor(sot_index, dtype=torch.int64).reshape(-1).cpu()
    if idx.numel() == 1:
        idx = idx.expand(B)
    if idx.numel() != B or int(idx.min()) < 0 or int(idx.max()) >= T:
        raise ValueError(f"sot_index must be an int or one per row, inside the prompt width {T}")
    if not 0 <= int(no_speech) < V:
        raise ValueError(f"no_speech={no_speech} is outside the vocabulary")
    dec = model.decoder
    h = dec.hidden(prompt.to(xa.device), xa)  # [B, T, d], final LayerNorm applied
    rows = torch.arange(B, device=h.device) * T + idx.to(h.device)
    logits = dec.padded_logits(h.reshape(B * T, -1).index_select(0, rows).view(B, 1, -1))
    stats, _ = K.token_stats(logits, torch.full((B,), int(no_speech), dtype=torch.int64, device=h.device), V)
    return torch.exp(stats[:, 3] - stats[:, 0])


UPSTREAM_TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)


def needs_fallback(avg_logprob: float, no_speech_prob: Optional[float], compression_ratio: Optional[float], *, thresholds: dict) -> bool:
    """Upstream's three tests of a decoded window, in its order -> True: decode again at the next temperature.  thresholds: a dict
    with "compression_ratio", "logprob" and "no_speech" (a missing key or None switches that test off).
      1. the compression ratio above its threshold -> retry (the text repeats itself);
      2. the average log-probability below its threshold -> retry;
      3. but a no-speech probability above its threshold together with an average log-probability below the log-probability
         threshold -> accept: the window is silence, another temperature will not help."""
    cr, lp, ns = thresholds.get("compression_ratio"), thresholds.get("logprob"), thresholds.get("no_speech")
    retry = False
    if cr is not None and compression_ratio is not None and compression_ratio > cr:
        retry = True
    if lp is not None and avg_logprob < lp:
        retry = True
    if ns is not None and no_speech_prob is not None and no_speech_prob > ns and lp is not None and avg_logprob < lp:
        retry = False
    return retry


def avg_logprob(sum_logprob: float, n: int) -> float:
    """Upstream's `sum_logprob / (len(tokens) + 1)`, n = the generated tokens before the eot."""
    return float(sum_logprob) / (int(n) + 1)


def compression_ratio(text: str) -> float:
    """len(utf-8 bytes) / len(zlib.compress(them)): upstream's measure of a text that repeats itself."""
    import zlib

    b = text.encode("utf-8")
    return len(b) / len(zlib.compress(b))


def generated_ids(row, first: int, length: int, eot: int, timestamp_begin: Optional[int] = None) -> tuple:
    """(ids of row[first:length] up to the first eot, the same without timestamp ids)."""
    ids = [int(t) for t in row[int(first):int(length)]]
    if int(eot) in ids:
        ids = ids[:ids.index(int(eot))]
    return ids, (ids if timestamp_begin is None else [t for t in ids if t < int(timestamp_begin)])


@torch.no_grad()
def decode_with_fallback(model, mel: torch.Tensor, prompt: torch.Tensor, prompt_len=None, *, temperatures=UPSTREAM_TEMPERATURES,
                         best_of: int = 5, beam_size: Optional[int] = None, patience: float = 1.0, length_penalty: Optional[float] = None,
                         logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6,
                         compression_ratio_threshold: Optional[float] = None, text_of=None, no_speech: Optional[int] = None, sot_index=None,
                         seed: int = 0, _xa=None, **decode_kw):
    """Upstream's temperature ladder (`transcribe()`'s decode_with_fallback) -> (tokens i64 [B, L], lengths i64 [B], sum_logprob f32
    [B], info) in greedy_decode's layout, rows from different rungs padded with `eot` to one width.

    The encoder runs once.  Rung i decodes the audios still pending at temperatures[i]: at 0 with beam_decode (beam_size, patience)
    if beam_size is given, else greedy_decode; above 0 with sample_decode(best_of), the audio with original index a drawing with
    seed + i*B + a.  An audio leaves the ladder when `needs_fallback` accepts its result; the last rung's result stands for audios
    that never pass.  Per result: avg_logprob = sum_logprob / (n + 1) over the n generated tokens before the eot (a row cut at
    max_len counts all of them); compression ratio = `compression_ratio(text_of(ids))` over the generated ids without eot and
    timestamp ids (a ratio threshold needs `text_of`, e.g. a tokenizer's decode: ValueError otherwise); the no-speech probability
    comes from `no_speech_prob` at `sot_index` (default 0: the prompt starts with sot) when the `no_speech` id is given.  A None
    threshold switches its test off.
    info: {"temperature": [B] the rung that produced each result, "avg_logprob": [B], "no_speech_prob": [B] (None without
    `no_speech`), "compression_ratio": [B] (None without `text_of`), "rungs": per rung the original indices decoded there}.
    decode_kw: what all three decoders share (eot — required —, max_len, suppress, suppress_first, sync_every, step, weights and the
    timestamp keywords).  Under step="graph" a rung with a new number of pending audios is a new graph session (sessions are keyed
    by batch size): accepted, not optimised — at most MAX_SESSIONS of a kind are kept, so a long ladder recaptures.
    `_xa`: the encoder output of `mel`, when the caller has it already (engine/transcribe.py detects the language on it first)."""
    temps = list(temperatures)
    if not temps:
        raise ValueError("temperatures must not be empty")
    for t in temps:
        _check_sampling(t, best_of, length_penalty)
    if beam_size is not None:
        beam_candidates(beam_size, patience)
    if compression_ratio_threshold is not None and text_of is None:
        raise ValueError("compression_ratio_threshold needs text_of (ids -> str): the ratio is taken over the decoded text")
    if "eot" not in decode_kw:
        raise TypeError("decode_with_fallback needs eot=")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"seed must be an integer, got {seed!r}")
    _check_mode(model, "decode_with_fallback", decode_kw.get("step", "eager"), decode_kw.get("sync_every", 8), decode_kw.get("weights", "bf16"))
    eot, ts_begin = int(decode_kw["eot"]), decode_kw.get("timestamp_begin")
    thresholds = {"compression_ratio": compression_ratio_threshold, "logprob": logprob_threshold, "no_speech": no_speech_threshold}
    B = int(prompt.shape[0])
    first = [int(prompt.shape[1])] * B if prompt_len is None else [int(n) for n in torch.as_tensor(prompt_len).reshape(B).tolist()]

    was_training = model.training
    model.eval()
    try:
        xa = encode(model, mel, decode_kw.get("weights", "bf16")) if _xa is None else _xa
        nsp = [None] * B
        if no_speech is not None:
            nsp = no_speech_prob(model, xa, prompt, 0 if sot_index is None else sot_index, no_speech).cpu().tolist()
        result = [None] * B  # per audio (tokens, sum_logprob)
        info = {"temperature": [None] * B, "avg_logprob": [None] * B, "no_speech_prob": nsp, "compression_ratio": [None] * B, "rungs": []}
        pending = list(range(B))
        for i, t in enumerate(temps):
            if not pending:
                break
            info["rungs"].append(list(pending))
            sel = torch.tensor(pending, dtype=torch.int64)
            sub = dict(prompt_len=torch.tensor([first[a] for a in pending]), _xa=xa[sel.to(xa.device)], **decode_kw)
            sub_mel, sub_prompt = mel[sel.to(mel.device)], prompt[sel.to(prompt.device)]
            if t > 0:
                out = sample_decode(model, sub_mel, sub_prompt, temperature=t, best_of=best_of, seed=[seed + i * B + a for a in pending],
                                    length_penalty=length_penalty, **sub)
            elif beam_size is not None:
                out = beam_decode(model, sub_mel, sub_prompt, beam_size=beam_size, patience=patience, length_penalty=length_penalty, **sub)
            else:
                out = greedy_decode(model, sub_mel, sub_prompt, **sub)
            toks, lens, slp = out[0].cpu().tolist(), out[1].cpu().tolist(), out[2].cpu().tolist()
            still = []
            for j, a in enumerate(pending):
                ids, text_ids = generated_ids(toks[j], first[a], lens[j], eot, ts_begin)
                alp = avg_logprob(slp[j], len(ids))
                ratio = compression_ratio(text_of(text_ids)) if text_of is not None else None
                result[a] = (toks[j][:lens[j]], slp[j])
                info["temperature"][a], info["avg_logprob"][a], info["compression_ratio"][a] = float(t), alp, ratio
                if needs_fallback(alp, nsp[a], ratio, thresholds=thresholds):
                    still.append(a)
            pending = still
    finally:
        model.train(was_training)
    width = max(len(t) for t, _ in result)
    tokens = torch.full((B, width), eot, dtype=torch.int64)
    for a, (t, _) in enumerate(result):
        tokens[a, :len(t)] = torch.tensor(t, dtype=torch.int64)
    dev = mel.device
    return (tokens.to(dev), torch.tensor([len(t) for t, _ in result], dtype=torch.int64, device=dev),
            torch.tensor([s for _, s in result], dtype=torch.float32, device=dev), info)


# ============================================================================= timed segments
def timestamp_segments(tokens, prompt_len, lengths, timestamp_begin: int, eot: int, time_precision: float = 0.02):
    """The decoded rows of greedy_decode / beam_decode under timestamp rules -> per row [(start_s, end_s, [text token ids])].

    The sampled tokens of a row are tokens[r][prompt_len[r]:lengths[r]], read up to the first `eot`.  A timestamp opens a segment,
    the next one closes it; the timestamp right behind a closing one opens the next segment — the split at consecutive timestamp
    pairs that upstream's `transcribe` makes.  Seconds = (id - timestamp_begin) * time_precision.  Text that is still open at the
    end of the row (a row cut at max_len, or an eot inside a segment) ends at None, text before any opening timestamp starts at
    None; a lone opening timestamp at the very end gives no segment; a pair with nothing in between gives one with no tokens.
    Pure Python on the host, no tokenizer: tokens / prompt_len / lengths may be tensors or nested lists."""
    as_list = lambda v: v.tolist() if hasattr(v, "tolist") else list(v)
    rows, plen, lens = as_list(tokens), as_list(prompt_len), as_list(lengths)
    tsb = int(timestamp_begin)
    out = []
    for row, p, n in zip(rows, plen, lens):
        segs, start, is_open, text = [], None, False, []
        for t in row[int(p):int(n)]:
            t = int(t)
            if t == int(eot):
                break
            if t < tsb:
                text.append(t)
            elif is_open or text:  # closes the open segment (or text that no timestamp opened)
                segs.append((start, (t - tsb) * time_precision, text))
                start, is_open, text = None, False, []
            else:
                start, is_open = (t - tsb) * time_precision, True
        if text:
            segs.append((start, None, text))
        out.append(segs)
    return out
