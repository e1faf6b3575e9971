"""Greedy decoding: the prefill, one cached step, the pick and `greedy_decode`.

Everything that changes from token to token lives in device memory (`KVCache`: len / tokens / finished / sum_logprob), so a
step is a fixed sequence of launches whose arguments never change: LayerNorm and every projection through the existing
kernels at M = B, attention / embedding / the pick through csrc/decode_attn.hip and csrc/decode_pick.hip.  The host reads one counter every `sync_every`
steps.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .. import kernels as K
from ..gemm_mode import step_weights
from .cache import KVCache, check_ts_rules, ts_extra
from .runner import _SESSIONS, _check_mode, _decode


def prefill(decoder, cache: KVCache, xa: torch.Tensor) -> torch.Tensor:
    """The prompts through the teacher-forced kernels (causal; k / v stored, cross k / v computed) -> padded bf16 logits [B, Vpad]
    of every row's LAST prompt position (len[b] - 1), from which its first token is picked."""
    T = cache.prompt_T
    h = decoder.hidden(cache.tokens[:, :T], xa, kv_cache=cache)  # [B, T, d], final LayerNorm applied
    rows = torch.arange(cache.batch, device=h.device) * T + (cache.len.long() - 1)
    last = h.reshape(cache.batch * T, -1).index_select(0, rows)
    cache.prefilled = True
    return decoder.padded_logits(last.view(cache.batch, 1, -1))


def step(decoder, cache) -> torch.Tensor:
    """One cached step: the token at len[r] - 1 of every row (KVCache) or hypothesis (BeamCache) through the decoder -> padded bf16
    logits [rows, Vpad]."""
    h = decoder.hidden(None, None, kv_cache=cache)  # [rows, 1, d]
    return decoder.padded_logits(h)


def pick(decoder, cache: KVCache, logits: torch.Tensor, want_pick: bool = False):
    """Greedy pick from the padded logits and the state update of every unfinished row (wft_decode_pick; wft_decode_pick_ts when
    the cache was started with timestamp rules)."""
    V = decoder.token_embedding.weight.shape[0]
    return K.decode_pick(logits, V, cache.tokens, cache.len, cache.finished, cache.sum_logprob, cache.unfinished, eot=cache.eot,
                         max_len=cache.max_len, suppress=cache.suppress, suppress_first=cache.suppress_first,
                         first_len=cache.prompt_len, want_pick=want_pick, ts_rules=cache.ts_rules)


def _greedy_body(decoder, cache: KVCache) -> torch.Tensor:
    logits = step(decoder, cache)
    pick(decoder, cache, logits)
    return logits


@torch.no_grad()
def greedy_decode(model, mel: torch.Tensor, prompt: torch.Tensor, prompt_len=None, *, eot: int, max_len: Optional[int] = None,
                  suppress: Sequence[int] = (), suppress_first: Sequence[int] = (), sync_every: int = 8, step: str = "eager",
                  timestamp_begin: Optional[int] = None, no_timestamps: Optional[int] = None,
                  max_initial_timestamp_index: Optional[int] = 50, weights: str = "bf16", _capture: bool = True, _stream_gemm: bool = True, _xa=None):
    """-> (tokens i64 [B, L] — prompt included, padded with `eot` behind each row's end —, lengths i64 [B], sum_logprob f32 [B]).

    timestamp_begin (default None: no rules, today's path exactly): the first timestamp id; every pick then runs under upstream's
    timestamp rules (include/wft.h "Timestamp rules") with `no_timestamps` removed and the first timestamp at most
    `max_initial_timestamp_index` (None: unbounded); the log-probabilities are those of the rule-filtered rows.  Argument errors
    (check_ts_rules) are raised before any device work.  `timestamp_segments` splits the result into timed segments.

    A row ends with the `eot` it picked (counted in its length) or at `max_len` tokens (default n_text_ctx).  `sum_logprob` sums
    the log-probabilities of the generated tokens, the `eot` included, under the softmax of the suppressed logits.

    step="eager": every cached step is issued launch by launch.  step="graph": the cached steps run on the weight-streaming GEMMs
    (`stream_gemm`) and are replayed from ONE captured HIP graph per (batch, device) session — the first step of a decode that
    has no valid graph runs eagerly, the second is captured; at most MAX_SESSIONS sessions per model, `release_graphs(model)` frees
    them.  The prefill and the encoder keep their kernels in both modes.  weights="int8" (needs step="graph"; ValueError otherwise,
    before any device work): the cached steps read per-row int8 images of the weight shadows (wft_gemm_nt_stream_q8) — weight-only,
    activations stay bf16; the encoder, the prefill and the cross key / value projections stay bf16; "bf16" is today's path, bit
    for bit; the captured int8 steps live in sessions of their own (key + ("int8",)).  weights="w8a8" (needs step="graph" likewise):
    in addition the encoder, the prefill and the cross key / value projections it stores run every Linear product with M > 32 on
    per-row quantised activations and the int8 images of the shadows (`int8_gemm`, wft_gemm_nt_i8); its cached steps are the "int8"
    steps and share their session.  Still bf16 under "w8a8": the cached steps' activations, products with M <= 32 in a short
    prefill, the conv stem, the embedding lookup, the prefill's tied-logits product, find_alignment's teacher-forced pass; attention
    is unchanged.  `_capture=False` / `_stream_gemm=False` switch off one
    half each (tests and the A/B bench only); `_xa`: the encoder output of `mel`, when decode_with_fallback has it already."""
    _check_mode(model, "greedy_decode", step, sync_every, weights)
    rules = check_ts_rules(model.dims.n_vocab, eot, suppress, suppress_first, timestamp_begin, no_timestamps, max_initial_timestamp_index)
    ts_kw = dict(timestamp_begin=timestamp_begin, no_timestamps=no_timestamps, max_initial_timestamp_index=max_initial_timestamp_index)
    B = prompt.shape[0]

    def readout(cache):
        lengths = cache.len.long()
        L = int(lengths.max())
        tokens = cache.tokens[:, :L].clone()
        tokens.masked_fill_(torch.arange(L, device=tokens.device)[None, :] >= lengths[:, None], cache.eot)
        return tokens, lengths, cache.sum_logprob.clone()

    return _decode(model, mel, dict(prompt=prompt, prompt_len=prompt_len, eot=eot, max_len=max_len, suppress=suppress, suppress_first=suppress_first, **ts_kw),
                   who="greedy_decode", table=_SESSIONS, key=(int(B),), make_cache=lambda dec: KVCache(dec, B, device=mel.device),
                   prefill=prefill, first=pick, body=_greedy_body, readout=readout, extra=ts_extra(rules), graph=step == "graph" and _capture,
                   stream=step == "graph" and _stream_gemm and step_weights(weights), sync_every=sync_every, xa=_xa, weights=weights)
