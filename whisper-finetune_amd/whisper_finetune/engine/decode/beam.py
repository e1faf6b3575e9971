"""Beam search on a KV cache that the beams of an audio share: `BeamCache`, the `beam_*` steps, `beam_decode`."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .. import kernels as K
from ..gemm_mode import step_weights
from .cache import _Cache, check_ts_rules, ts_extra
from .greedy import step
from .runner import _BEAM_SESSIONS, _check_mode, _decode

# ============================================================================= beam search
# Upstream's `BeamSearchDecoder` + `MaximumLikelihoodRanker` under `without_timestamps=True`, restated (neither is in the reference
# tree and openai-whisper is not a dependency: parity with the upstream binary is unpinned).  W = beam_size; audio a owns the rows
# r = a*W + j; all rows of an audio hold the same `len`; C = round(W * patience) finished sequences end an audio.  One step, per
# audio that is not done (csrc/decode_beam.hip: wft_decode_topk, wft_beam_update; include/wft.h states the order rules):
#   the W + 1 most probable continuations of every beam -> candidates scored sum_logprob + logp -> walked in descending order: an
#   `eot` candidate joins the audio's finished list (while that holds fewer than C), any other becomes the next beam, until W beams.
# What makes it cheap (DESIGN.md §3 "Beam-search layouts"): the cross keys / values exist once per AUDIO and are read once per step
# for all of its beams; self-attention keys are never moved — a beam reorder permutes rows of the i32 ancestry table `anc`.
MAX_BEAM = 8


def beam_candidates(beam_size: int, patience: float = 1.0) -> int:
    """C = round(beam_size * patience) with Python's round — how many finished sequences end an audio.  Raises ValueError on a bad
    beam size or patience."""
    if isinstance(beam_size, bool) or not isinstance(beam_size, int) or not 1 <= beam_size <= MAX_BEAM:
        raise ValueError(f"beam_size must be an integer in [1, {MAX_BEAM}], got {beam_size!r}")
    if isinstance(patience, bool) or not isinstance(patience, (int, float)) or not patience > 0 or patience != patience or patience == float("inf"):
        raise ValueError(f"patience must be a positive finite number, got {patience!r}")
    C = round(beam_size * patience)
    if C < 1:
        raise ValueError(f"round(beam_size * patience) = {C}: patience={patience!r} leaves no room for a finished sequence")
    return C


def _check_live_columns(beam_size: int, n_vocab: int, suppress: Sequence[int], suppress_first: Sequence[int]) -> None:
    """At least W + 1 columns stay live under suppress | suppress_first: then every step has >= W candidates that are not `eot`."""
    dead = {int(t) for t in suppress} | {int(t) for t in suppress_first}
    if dead and (min(dead) < 0 or max(dead) >= n_vocab):
        raise ValueError("suppressed token ids must lie inside the vocabulary")
    if n_vocab - len(dead) < beam_size + 1:
        raise ValueError(f"beam_size={beam_size} needs at least {beam_size + 1} un-suppressed columns, {n_vocab - len(dead)} of {n_vocab} are left")


class BeamCache(_Cache):
    """Keys / values plus the beam-search state of `audios` audios x `beam_size` hypotheses (R = audios * beam_size slot rows).

    Handed to the decoder as `kv_cache=` like a KVCache: a call with T > 1 tokens is the prefill — ONE row per audio through the
    teacher-forced kernels, its k / v stored into slot row a*W —, a call with T = 1 a cached step of all R rows.
      self_kv[attn]  bf16 [R, n_text_ctx, 2d]   slot rows; hypothesis r reads position t at slot anc[r, t]
      anc            i32 [R, n_text_ctx]         the ancestry table: keys never move, a beam reorder permutes these rows
      cross_kv[attn] bf16 [audios, n_audio_ctx, 2d]   one copy per audio, shared by its beams
      tokens i64 [R, n_ctx], len / first_len i32 [R], sum_logprob f32 [R], done i32 [audios], unfinished i32 [1]
      cand_tok i32 / cand_logp f32 [R, W + 1]    the step's candidates;  src i32 [R]: the source beam of every slot's last update
      fin_tokens i64 [audios, C, n_ctx], fin_len i32 / fin_score f32 [audios, C], fin_n i32 [audios]   the finished lists"""

    def __init__(self, decoder, audios: int, beam_size: int, candidates: Optional[int] = None, device=None):
        W = int(beam_size)
        C = beam_candidates(W) if candidates is None else int(candidates)
        if not 1 <= W <= MAX_BEAM or C < 1:
            raise ValueError(f"beam_size must lie in [1, {MAX_BEAM}] and candidates be >= 1")
        self.audios, self.beam, self.cands = int(audios), W, C
        R = self.audios * W
        super().__init__(decoder, R, self.audios, device)
        device = self.tokens.device
        i32 = dict(dtype=torch.int32, device=device)
        f32 = dict(dtype=torch.float32, device=device)
        self.anc = torch.zeros((R, self.n_ctx), **i32)
        self.first_len = torch.ones(R, **i32)
        self.done = torch.zeros(self.audios, **i32)
        self.cand_tok = torch.full((R, W + 1), -1, **i32)
        self.cand_logp = torch.zeros((R, W + 1), **f32)
        self.src = torch.zeros(R, **i32)
        self.fin_tokens = torch.zeros((self.audios, C, self.n_ctx), dtype=torch.int64, device=device)
        self.fin_len = torch.zeros((self.audios, C), **i32)
        self.fin_score = torch.zeros((self.audios, C), **f32)
        self.fin_n = torch.zeros(self.audios, **i32)

    def start(self, prompt: torch.Tensor, prompt_len: Optional[torch.Tensor], *, eot: int, max_len: Optional[int] = None,
              suppress: Sequence[int] = (), suppress_first: Sequence[int] = (), n_vocab: int, timestamp_begin: Optional[int] = None,
              no_timestamps: Optional[int] = None, max_initial_timestamp_index: Optional[int] = 50) -> None:
        """Load the prompts (i64 [audios, T], right-padded; prompt_len [audios] or None) into all W rows of every audio and reset
        the state.  The checks of KVCache.start plus the live-column count (under timestamp rules: check_ts_rules' beam clauses)."""
        B, W = self.audios, self.beam
        _check_live_columns(W, n_vocab, suppress, suppress_first)
        rules = check_ts_rules(n_vocab, eot, suppress, suppress_first, timestamp_begin, no_timestamps, max_initial_timestamp_index, beam_size=W)
        T, pl = self._start(B, prompt, prompt_len, eot, max_len, suppress, suppress_first, n_vocab, rules)
        dev = self.tokens.device
        self.tokens.view(B, W, self.n_ctx)[:, :, :T].copy_(prompt.to(dev)[:, None, :])
        self.len.copy_(pl.to(dev).repeat_interleave(W))
        self.first_len.copy_(self.len)
        self.anc.copy_((torch.arange(B, dtype=torch.int32, device=dev) * W).repeat_interleave(W)[:, None].expand(-1, self.n_ctx))
        self.done.copy_((pl >= self.max_len).to(torch.int32))
        self.unfinished.copy_((self.done == 0).sum().to(torch.int32).reshape(1))
        self.cand_tok.fill_(-1); self.cand_logp.zero_(); self.src.zero_()
        self.fin_tokens.fill_(int(eot)); self.fin_len.zero_(); self.fin_score.zero_(); self.fin_n.zero_()

    def store_prefill(self, attn, kv: torch.Tensor) -> None:
        """kv bf16 [audios, T, 2d]: the {k | v} rows of the prompt block, into slot row a*W of every audio."""
        B, T = kv.shape[:2]
        self.self_kv[attn].view(B, self.beam, -1, kv.shape[2])[:, 0, :T].copy_(kv)

    def self_step(self, attn, q, k, v, n_head: int, scale: float, q_prescaled: bool) -> torch.Tensor:
        return K.attn_decode_beam(q, self.self_kv[attn], n_head, scale, new_kv=(k, v), lens=self.len, anc=self.anc, q_prescaled=q_prescaled)

    def cross_step(self, attn, q, n_head: int, scale: float) -> torch.Tensor:
        return K.attn_decode_beam(q, self.cross_kv[attn], n_head, scale, group=self.beam)


def beam_prefill(decoder, cache: BeamCache, xa: torch.Tensor) -> torch.Tensor:
    """The prompts, ONE row per audio, through the teacher-forced kernels (k / v stored into slot row a*W, cross k / v computed once
    per audio) -> padded bf16 logits [audios, Vpad] of every audio's last prompt position."""
    B, W = cache.audios, cache.beam
    T = min(max(cache.prompt_T, 2), cache.n_ctx)  # (a one-token prompt block is widened by a pad column: T = 1 means "cached step")
    h = decoder.hidden(cache.tokens[::W, :T], xa, kv_cache=cache)  # [B, T, d]
    rows = torch.arange(B, device=h.device) * T + (cache.len[::W].long() - 1)
    last = h.reshape(B * T, -1).index_select(0, rows)
    cache.prefilled = True
    return decoder.padded_logits(last.view(B, 1, -1))


beam_step = step


def beam_topk(decoder, cache: BeamCache, logits: torch.Tensor, first: bool = False) -> None:
    """cand_tok / cand_logp <- the W + 1 best continuations per logits row (wft_decode_topk; wft_decode_topk_ts when the cache was
    started with timestamp rules — the kernel reads each hypothesis' sampled tokens from `tokens`, whose rows wft_beam_update
    permutes with the beams).  first: `logits` are the prefill's, one row per audio, and fill the candidate row of beam 0."""
    V = decoder.token_embedding.weight.shape[0]
    K.decode_topk(logits, V, cache.cand_tok, cache.cand_logp, lens=cache.len, first_len=cache.first_len, suppress=cache.suppress,
                  suppress_first=cache.suppress_first, row_step=cache.beam if first else 1, ts_rules=cache.ts_rules, tokens=cache.tokens,
                  eot=cache.eot)


def beam_update(cache: BeamCache, first: bool = False) -> None:
    """One beam-search step of every audio that is not done, from cand_tok / cand_logp (wft_beam_update)."""
    K.beam_update(cache.cand_tok, cache.cand_logp, cache.tokens, cache.anc, cache.len, cache.sum_logprob, cache.done, cache.unfinished,
                  cache.fin_tokens, cache.fin_len, cache.fin_score, cache.fin_n, eot=cache.eot, max_len=cache.max_len, first=first,
                  src_out=cache.src)


def _beam_first(decoder, cache: BeamCache, logits: torch.Tensor) -> None:
    beam_topk(decoder, cache, logits, first=True)
    beam_update(cache, first=True)


def _beam_body(decoder, cache: BeamCache) -> torch.Tensor:
    logits = beam_step(decoder, cache)
    beam_topk(decoder, cache, logits)
    beam_update(cache)
    return logits


def beam_rank(entries, length_penalty: Optional[float] = None) -> int:
    """entries: [(n generated tokens without the final eot, sum_logprob)] in list order -> index of the first maximum of
    sum_logprob / n, or / ((5 + n) / 6) ** length_penalty; n = 0 ranks as -inf."""
    best, best_i = None, 0
    for i, (n, slp) in enumerate(entries):
        score = beam_score(n, slp, length_penalty)
        if best is None or score > best:
            best, best_i = score, i
    return best_i


def beam_score(n: int, sum_logprob: float, length_penalty: Optional[float] = None) -> float:
    if n <= 0:
        return float("-inf")
    return float(sum_logprob) / (float(n) if length_penalty is None else ((5.0 + n) / 6.0) ** float(length_penalty))


def beam_finalize(cache: BeamCache, length_penalty: Optional[float] = None):
    """End of decoding, on the host (one small read-back): an audio with fewer than W finished entries receives its current beams in
    descending sum_logprob (ties to the lower j) until it holds W; the entries are ranked by beam_score; the first maximum in list
    order wins.  -> per audio the list of (tokens incl. prompt and a final eot if the hypothesis ended with one, sum_logprob, score),
    in LIST order, and the winner's index."""
    B, W = cache.audios, cache.beam
    fin_tokens, fin_len, fin_score, fin_n = cache.fin_tokens.cpu(), cache.fin_len.cpu().tolist(), cache.fin_score.cpu(), cache.fin_n.cpu().tolist()
    tokens, lens, first, slp = cache.tokens.cpu(), cache.len.cpu().tolist(), cache.first_len.cpu().tolist(), cache.sum_logprob.cpu()
    out = []
    for a in range(B):
        r0 = a * W
        entries = [(fin_tokens[a, p, :fin_len[a][p]].tolist(), float(fin_score[a, p]), fin_len[a][p] - first[r0] - 1) for p in range(fin_n[a])]
        order = sorted(range(W), key=lambda j: -float(slp[r0 + j]))  # (stable: ties to the lower j)
        for j in order:
            if len(entries) >= W:
                break
            entries.append((tokens[r0 + j, :lens[r0 + j]].tolist(), float(slp[r0 + j]), lens[r0 + j] - first[r0 + j]))
        win = beam_rank([(n, s) for _, s, n in entries], length_penalty)
        out.append(([(t, s, beam_score(n, s, length_penalty)) for t, s, n in entries], win))
    return out


@torch.no_grad()
def beam_decode(model, mel: torch.Tensor, prompt: torch.Tensor, prompt_len=None, *, beam_size: int, patience: float = 1.0,
                length_penalty: Optional[float] = None, eot: int, max_len: Optional[int] = None, suppress: Sequence[int] = (),
                suppress_first: Sequence[int] = (), sync_every: int = 8, step: str = "eager", return_all: bool = False,
                timestamp_begin: Optional[int] = None, no_timestamps: Optional[int] = None,
                max_initial_timestamp_index: Optional[int] = 50, weights: str = "bf16", _capture: bool = True, _stream_gemm: bool = True, _xa=None):
    """Beam search -> (tokens i64 [B, L], lengths i64 [B], sum_logprob f32 [B]) of the winning hypothesis per audio, in greedy_decode's
    layout: prompt included, the `eot` that ended the hypothesis included (one that ran into `max_len` has none), padded with `eot`.
    return_all: a fourth value, per audio the list of (tokens, sum_logprob, score) of all its entries, best score first (stable).

    beam_size 1..8; an audio ends once round(beam_size * patience) sequences have finished or at `max_len`; the winner maximises
    sum_logprob / n over the generated tokens (n without the final eot), or sum_logprob / ((5 + n) / 6) ** length_penalty.
    timestamp_begin / no_timestamps / max_initial_timestamp_index: as greedy_decode (default: no rules), every hypothesis under
    its own history; beam search needs max_initial_timestamp_index >= beam_size - 1 or None (check_ts_rules says why).
    Argument errors are raised before any device work.  `step`, `weights`, `sync_every`, `_capture`, `_stream_gemm`, `_xa`: as greedy_decode; the
    captured beam steps live in their own sessions (`beam_sessions`), freed by `release_graphs` too."""
    C = beam_candidates(beam_size, patience)
    if length_penalty is not None and (isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float))):
        raise ValueError(f"length_penalty must be None or a number, got {length_penalty!r}")
    _check_live_columns(beam_size, model.dims.n_vocab, suppress, suppress_first)
    _check_mode(model, "beam_decode", step, sync_every, weights)
    rules = check_ts_rules(model.dims.n_vocab, eot, suppress, suppress_first, timestamp_begin, no_timestamps, max_initial_timestamp_index,
                           beam_size=beam_size)
    ts_kw = dict(timestamp_begin=timestamp_begin, no_timestamps=no_timestamps, max_initial_timestamp_index=max_initial_timestamp_index)
    B = prompt.shape[0]

    def readout(cache):
        ranked = beam_finalize(cache, length_penalty)
        wins = [entries[win] for entries, win in ranked]
        L = max(len(t) for t, _, _ in wins)
        tokens = torch.full((B, L), cache.eot, dtype=torch.int64)
        for a, (t, _, _) in enumerate(wins):
            tokens[a, :len(t)] = torch.tensor(t, dtype=torch.int64)
        dev = cache.tokens.device
        res = (tokens.to(dev), torch.tensor([len(t) for t, _, _ in wins], dtype=torch.int64, device=dev),
               torch.tensor([s for _, s, _ in wins], dtype=torch.float32, device=dev))
        if return_all:
            res += ([sorted(entries, key=lambda e: -e[2]) for entries, _ in ranked],)
        return res

    return _decode(model, mel, dict(prompt=prompt, prompt_len=prompt_len, eot=eot, max_len=max_len, suppress=suppress, suppress_first=suppress_first, **ts_kw),
                   who="beam_decode", table=_BEAM_SESSIONS, key=(int(B), int(beam_size), int(C)),
                   make_cache=lambda dec: BeamCache(dec, B, beam_size, C, device=mel.device), prefill=beam_prefill, first=_beam_first,
                   body=_beam_body, readout=readout, extra=(("beam", beam_size, C),) + ts_extra(rules), graph=step == "graph" and _capture,
                   stream=step == "graph" and _stream_gemm and step_weights(weights), sync_every=sync_every, xa=_xa, weights=weights)
