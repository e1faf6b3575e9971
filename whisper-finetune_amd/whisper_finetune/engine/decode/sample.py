"""Sampled decoding: `best_of` samples per audio at a temperature on a cache whose samples share the prompt keys and the cross keys /
values (`SampleCache`), `sample_decode`."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .. import kernels as K
from ..gemm_mode import step_weights
from .beam import MAX_BEAM, BeamCache, beam_prefill, beam_rank, beam_score
from .cache import _Cache, check_ts_rules, ts_extra
from .greedy import greedy_decode, step
from .runner import _SAMPLE_SESSIONS, _check_mode, _decode

# ============================================================================= sampling and the temperature ladder
# Upstream's `GreedyDecoder` at temperature > 0 with `best_of` samples, its `MaximumLikelihoodRanker`, and the fallback loop of
# `transcribe()` (`decode_with_fallback`), restated (none of it is in the reference tree and openai-whisper is not a dependency:
# parity with the upstream binary and with torch's random stream is unpinned).  N = best_of; audio a owns the state rows
# r = a*N + j.  The N samples of an audio are what the beam kernels were built for (DESIGN.md §3 "Sampling layouts"): one copy of the
# cross keys / values per audio read once per step for all N rows (the group = N form), and the prompt keys shared through the
# ancestry table — which for samples is STATIC: position t of row r lives in slot a*N while t is a prompt position and in slot r
# from there on.  The pick is wft_decode_sample: temperature and seed per row are device memory, so one captured step serves every
# rung of the ladder and every seed.
class SampleCache(_Cache):
    """Keys / values plus the state of `audios` audios x `best_of` samples (R = audios * best_of slot rows), handed to the decoder
    as `kv_cache=` like a BeamCache: the prefill carries ONE row per audio (k / v into slot row a*N), a step all R rows.
      self_kv[attn]  bf16 [R, n_text_ctx, 2d];  anc i32 [R, n_text_ctx]: a*N below the prompt length of audio a, r from there on
      cross_kv[attn] bf16 [audios, n_audio_ctx, 2d]   one copy per audio, shared by its samples
      tokens i64 [R, n_ctx], len / first_len / finished i32 [R], sum_logprob f32 [R], unfinished i32 [1] (counts ROWS)
      temperature f32 [R], seed i64 [R] (the bits of the u64 the kernel reads)"""

    def __init__(self, decoder, audios: int, best_of: int, device=None):
        N = int(best_of)
        if not 1 <= N <= MAX_BEAM:
            raise ValueError(f"best_of must lie in [1, {MAX_BEAM}] (the group limit of the cross-attention form)")
        self.audios, self.beam = int(audios), N  # (`beam`: the rows per audio, under the name beam_prefill and the step methods read)
        R = self.audios * N
        super().__init__(decoder, R, R, device)
        device = self.tokens.device
        self.anc = torch.zeros((R, self.n_ctx), dtype=torch.int32, device=device)
        self.first_len = torch.ones(R, dtype=torch.int32, device=device)
        self.finished = torch.zeros(R, dtype=torch.int32, device=device)
        self.temperature = torch.zeros(R, dtype=torch.float32, device=device)
        self.seed = torch.zeros(R, dtype=torch.int64, device=device)

    def start(self, prompt: torch.Tensor, prompt_len: Optional[torch.Tensor], *, temperature, seeds: Sequence[int], eot: int,
              max_len: Optional[int] = None, suppress: Sequence[int] = (), suppress_first: Sequence[int] = (), n_vocab: int,
              timestamp_begin: Optional[int] = None, no_timestamps: Optional[int] = None, max_initial_timestamp_index: Optional[int] = 50) -> None:
        """Load the prompts (i64 [audios, T], right-padded; prompt_len [audios] or None) into all N rows of every audio, write the
        static ancestry table and reset the state.  temperature: one number or R of them; seeds: R integers (taken mod 2^64)."""
        B, N, R = self.audios, self.beam, self.batch
        rules = check_ts_rules(n_vocab, eot, suppress, suppress_first, timestamp_begin, no_timestamps, max_initial_timestamp_index)
        seeds = [int(s) % (1 << 64) for s in seeds]
        if len(seeds) != R:
            raise ValueError(f"seeds: {R} integers expected, got {len(seeds)}")
        T, pl = self._start(B, prompt, prompt_len, eot, max_len, suppress, suppress_first, n_vocab, rules)
        dev = self.tokens.device
        self.tokens.view(B, N, self.n_ctx)[:, :, :T].copy_(prompt.to(dev)[:, None, :])
        plr = pl.repeat_interleave(N)
        self.len.copy_(plr)
        self.first_len.copy_(self.len)
        own = torch.arange(R, dtype=torch.int32)
        shared = (torch.arange(B, dtype=torch.int32) * N).repeat_interleave(N)
        self.anc.copy_(torch.where(torch.arange(self.n_ctx)[None, :] < plr[:, None], shared[:, None], own[:, None]))
        self.finished.copy_((plr >= self.max_len).to(torch.int32))
        self.unfinished.copy_((self.finished == 0).sum().to(torch.int32).reshape(1))
        t = torch.as_tensor(temperature, dtype=torch.float32).reshape(-1)
        self.temperature.copy_(t.expand(R) if t.numel() == 1 else t.reshape(R))
        self.seed.copy_(torch.tensor([s - (1 << 64) if s >= (1 << 63) else s for s in seeds], dtype=torch.int64))

    # the layout is BeamCache's (slot rows behind an ancestry table, one cross copy per audio), and so is the code that reads it
    store_prefill = BeamCache.store_prefill
    self_step = BeamCache.self_step
    cross_step = BeamCache.cross_step


def sample_pick(decoder, cache: SampleCache, logits: torch.Tensor, want_pick: bool = False):
    """Sampled pick and state update of every unfinished row (wft_decode_sample; _ts under timestamp rules).  logits: one row per
    state row, or — the prefill's — one per audio, which then feeds all of its N samples (group = N)."""
    V = decoder.token_embedding.weight.shape[0]
    return K.decode_sample(logits, V, cache.tokens, cache.len, cache.finished, cache.sum_logprob, cache.unfinished, cache.temperature, cache.seed,
                           group=cache.batch // logits.shape[0], eot=cache.eot, max_len=cache.max_len, suppress=cache.suppress,
                           suppress_first=cache.suppress_first, first_len=cache.first_len, want_pick=want_pick, ts_rules=cache.ts_rules)


def _sample_body(decoder, cache: SampleCache) -> torch.Tensor:
    logits = step(decoder, cache)
    sample_pick(decoder, cache, logits)
    return logits


def sample_seeds(seed, audios: int, best_of: int) -> list:
    """The per-row seeds of sample_decode: `seed` an int (audio a draws with seed + a) or one int per audio; sample j of an audio
    with seed s draws with (8*s + j) mod 2^64."""
    if isinstance(seed, bool):
        raise ValueError(f"seed must be an integer or one per audio, got {seed!r}")
    if isinstance(seed, int):
        per_audio = [seed + a for a in range(audios)]
    else:
        per_audio = [int(s) for s in (seed.tolist() if hasattr(seed, "tolist") else seed)]
        if len(per_audio) != audios:
            raise ValueError(f"seed: one integer or {audios} of them (one per audio), got {len(per_audio)}")
    return [(8 * s + j) % (1 << 64) for s in per_audio for j in range(best_of)]


def _check_sampling(temperature, best_of, length_penalty=None) -> None:
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not 0 <= temperature < float("inf"):
        raise ValueError(f"temperature must be a finite number >= 0, got {temperature!r}")
    if isinstance(best_of, bool) or not isinstance(best_of, int) or not 1 <= best_of <= MAX_BEAM:
        raise ValueError(f"best_of must be an integer in [1, {MAX_BEAM}], got {best_of!r}")
    if length_penalty is not None and (isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float))):
        raise ValueError(f"length_penalty must be None or a number, got {length_penalty!r}")


@torch.no_grad()
def sample_decode(model, mel: torch.Tensor, prompt: torch.Tensor, prompt_len=None, *, temperature: float, best_of: int = 1, seed=0,
                  length_penalty: Optional[float] = None, return_all: bool = False, eot: int, max_len: Optional[int] = None,
                  suppress: Sequence[int] = (), suppress_first: Sequence[int] = (), sync_every: int = 8, step: str = "eager",
                  timestamp_begin: Optional[int] = None, no_timestamps: Optional[int] = None,
                  max_initial_timestamp_index: Optional[int] = 50, weights: str = "bf16", _capture: bool = True, _stream_gemm: bool = True, _xa=None):
    """`best_of` samples per audio at `temperature`, the best of them -> (tokens i64 [B, L], lengths i64 [B], sum_logprob f32 [B]) in
    greedy_decode's layout.  return_all: a fourth value, per audio the list of (tokens, sum_logprob, score) of its samples, best
    score first (stable).

    Every token is a draw from softmax(logits / temperature) over the live columns — the suppress masks and, with timestamp_begin,
    the timestamp rules, as in greedy_decode — made on the device (wft_decode_sample); `sum_logprob` sums the tokens'
    log-probabilities at temperature 1, as upstream does.  The winner maximises sum_logprob / n (n generated tokens without the
    final eot), or sum_logprob / ((5 + n) / 6) ** length_penalty (`beam_rank`: upstream's MaximumLikelihoodRanker); ties go to the
    lower sample.  temperature = 0 returns greedy_decode's result (upstream drops best_of at 0).
    seed: an int — audio a then draws with seed + a — or one int per audio; sample j of an audio with seed s draws with
    (8*s + j) mod 2^64.  The noise depends on (that seed, position, column) only, so a result does not depend on the batch an audio
    is decoded in.  Errors (temperature < 0, best_of outside 1..8, ...) are raised before any device work.
    `step`, `weights`, `sync_every`, `_capture`, `_stream_gemm`, `_xa`: as greedy_decode.  The captured steps live in a third table
    (`sample_sessions`, keyed (audios, best_of, device)); temperature and seeds are device memory, so a second call with other
    values replays the same graph."""
    _check_sampling(temperature, best_of, length_penalty)
    B, N = int(prompt.shape[0]), int(best_of)
    seeds = sample_seeds(seed, B, N)
    _check_mode(model, "sample_decode", step, sync_every, weights)
    rules = check_ts_rules(model.dims.n_vocab, eot, suppress, suppress_first, timestamp_begin, no_timestamps, max_initial_timestamp_index)
    ts_kw = dict(timestamp_begin=timestamp_begin, no_timestamps=no_timestamps, max_initial_timestamp_index=max_initial_timestamp_index)
    if temperature == 0:
        res = greedy_decode(model, mel, prompt, prompt_len, eot=eot, max_len=max_len, suppress=suppress, suppress_first=suppress_first,
                            sync_every=sync_every, step=step, weights=weights, _capture=_capture, _stream_gemm=_stream_gemm, _xa=_xa, **ts_kw)
        if return_all:
            toks, lens, slp = res[0].cpu().tolist(), res[1].cpu().tolist(), res[2].cpu().tolist()
            first = [int(prompt.shape[1])] * B if prompt_len is None else torch.as_tensor(prompt_len).reshape(B).tolist()
            res += ([[(toks[a][:lens[a]], slp[a], beam_score(_generated_n(toks[a], first[a], lens[a], eot), slp[a], length_penalty))] for a in range(B)],)
        return res

    def readout(cache):
        tokens, lens, first, slp = cache.tokens.cpu().tolist(), cache.len.cpu().tolist(), cache.first_len.cpu().tolist(), cache.sum_logprob.cpu().tolist()
        ranked, wins = [], []
        for a in range(B):
            rows = range(a * N, (a + 1) * N)
            ns = [_generated_n(tokens[r], first[r], lens[r], cache.eot) for r in rows]
            entries = [(tokens[r][:lens[r]], slp[r], beam_score(n, slp[r], length_penalty)) for r, n in zip(rows, ns)]
            wins.append(entries[beam_rank([(n, slp[r]) for r, n in zip(rows, ns)], length_penalty)])
            ranked.append(sorted(entries, key=lambda e: -e[2]))
        L = max(len(t) for t, _, _ in wins)
        out = torch.full((B, L), cache.eot, dtype=torch.int64)
        for a, (t, _, _) in enumerate(wins):
            out[a, :len(t)] = torch.tensor(t, dtype=torch.int64)
        dev = cache.tokens.device
        res = (out.to(dev), torch.tensor([len(t) for t, _, _ in wins], dtype=torch.int64, device=dev),
               torch.tensor([s for _, s, _ in wins], dtype=torch.float32, device=dev))
        return res + ((ranked,) if return_all else ())

    return _decode(model, mel, dict(prompt=prompt, prompt_len=prompt_len, temperature=float(temperature), seeds=seeds, eot=eot, max_len=max_len,
                                    suppress=suppress, suppress_first=suppress_first, **ts_kw),
                   who="sample_decode", table=_SAMPLE_SESSIONS, key=(B, N), make_cache=lambda dec: SampleCache(dec, B, N, device=mel.device),
                   prefill=beam_prefill, first=sample_pick, body=_sample_body, readout=readout, extra=ts_extra(rules),
                   graph=step == "graph" and _capture, stream=step == "graph" and _stream_gemm and step_weights(weights), sync_every=sync_every, xa=_xa, weights=weights)


def _generated_n(row, first: int, length: int, eot: int) -> int:
    """Generated tokens of a decoded row without the eot that ended it (a row cut at max_len has none and counts them all)."""
    n = int(length) - int(first)
    return n - 1 if n > 0 and int(row[int(length) - 1]) == int(eot) else n
