"""The key / value cache of greedy decoding and what every cache shares: `_Cache`, `KVCache`, the timestamp-rule checks.

Cache layout (DESIGN.md §3 "Greedy-decoding layouts"): per decoder layer one self-attention buffer bf16 [B, n_text_ctx, 2d] whose row (b, t) is
{k | v} of token t — the k and v thirds of the fused q/k/v projection row, appended by the attention kernel itself — and one
cross-attention buffer bf16 [B, n_audio_ctx, 2d], the output of the fused key/value GEMM, computed once per audio batch.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .. import kernels as K

BF16 = torch.bfloat16


class _Cache:
    """What KVCache and BeamCache share: the key / value buffers of every decoder layer for `rows` cached rows, the state every
    decode keeps, and the argument checks of start().  The attention modules ask the cache to store the prefill's rows and to run a
    step (store_prefill / self_step / cross_step), so only the cache knows its layout."""

    def __init__(self, decoder, rows: int, audios: int, device=None):
        pos = decoder.positional_embedding
        device = pos.device if device is None else device
        self.n_ctx, d = pos.shape
        self.batch = int(rows)  # rows of a cached step (the name the decoder reads)
        self.self_kv = {blk.attn: torch.empty((rows, self.n_ctx, 2 * d), dtype=BF16, device=device) for blk in decoder.blocks}
        self.cross_kv = {blk.cross_attn: None for blk in decoder.blocks}
        self.tokens = torch.zeros((rows, self.n_ctx), dtype=torch.int64, device=device)
        self.len = torch.ones(rows, dtype=torch.int32, device=device)
        self.sum_logprob = torch.zeros(rows, dtype=torch.float32, device=device)
        self.unfinished = torch.full((1,), audios, dtype=torch.int32, device=device)
        self.prompt_T = 0       # width of the right-padded prompt block (host constant of this decode)
        self.prefilled = False
        self.eot, self.max_len = 0, self.n_ctx
        self.suppress = self.suppress_first = None
        self.ts_rules = None    # (timestamp_begin, no_timestamps or None, max_initial_timestamp_index or None), or None: no rules

    def is_cross(self, attn) -> bool:
        return attn in self.cross_kv

    def _start(self, audios: int, prompt: torch.Tensor, prompt_len, eot: int, max_len: Optional[int], suppress, suppress_first, n_vocab: int,
               ts_rules=None):
        """The checks and resets of both start()s -> (prompt width T, the prompt lengths as i32 [audios] on the host).  ts_rules: what
        check_ts_rules returned."""
        B, T = prompt.shape
        max_len = self.n_ctx if max_len is None else int(max_len)
        if B != audios or not 1 <= T <= self.n_ctx:
            raise ValueError(f"prompt {tuple(prompt.shape)} does not fit a cache of {audios} x {self.n_ctx}")
        if not T <= max_len <= self.n_ctx:
            raise ValueError(f"max_len={max_len} must lie in [prompt width {T}, n_text_ctx {self.n_ctx}]")
        if not 0 <= int(eot) < n_vocab:
            raise ValueError(f"eot={eot} is outside the vocabulary")
        if prompt_len is None:
            pl = torch.full((B,), T, dtype=torch.int32)
        else:
            pl = torch.as_tensor(prompt_len).to(device="cpu", dtype=torch.int32).reshape(B)
            if int(pl.min()) < 1 or int(pl.max()) > T:
                raise ValueError("prompt_len must lie in [1, prompt width]")
        dev = self.tokens.device
        self.suppress = _mask(suppress, n_vocab, dev)
        self.suppress_first = _mask(suppress_first, n_vocab, dev)
        self.prompt_T, self.prefilled = T, False
        self.eot, self.max_len = int(eot), max_len
        self.ts_rules = ts_rules
        self.tokens.fill_(int(eot))
        self.sum_logprob.zero_()
        for key in self.cross_kv:
            self.cross_kv[key] = None
        return T, pl


class KVCache(_Cache):
    """Keys / values of every decoder layer plus the per-row decoding state, for `batch` sequences.

    Handed to the decoder as `kv_cache=`: a call with T > 1 tokens is the prefill (the teacher-forced kernels over the
    right-padded prompts; k / v rows stored), a call with T = 1 is a cached step on the single-token kernels."""

    def __init__(self, decoder, batch: int, device=None):
        super().__init__(decoder, batch, batch, device)
        self.prompt_len = torch.ones_like(self.len)
        self.finished = torch.zeros_like(self.len)

    def start(self, prompt: torch.Tensor, prompt_len: Optional[torch.Tensor], *, eot: int, max_len: Optional[int] = None,
              suppress: Sequence[int] = (), suppress_first: Sequence[int] = (), n_vocab: int, timestamp_begin: Optional[int] = None,
              no_timestamps: Optional[int] = None, max_initial_timestamp_index: Optional[int] = 50) -> None:
        """Load the prompts (i64 [B, T], right-padded; prompt_len [B] or None = all T long) and reset the state.  timestamp_begin:
        every pick of this decode runs under the timestamp rules (check_ts_rules)."""
        rules = check_ts_rules(n_vocab, eot, suppress, suppress_first, timestamp_begin, no_timestamps, max_initial_timestamp_index)
        T, pl = self._start(self.batch, prompt, prompt_len, eot, max_len, suppress, suppress_first, n_vocab, rules)
        self.tokens[:, :T].copy_(prompt.to(self.tokens.device))
        self.len.copy_(pl)
        self.prompt_len.copy_(self.len)
        self.finished.copy_((self.len >= self.max_len).to(torch.int32))
        self.unfinished.copy_((self.finished == 0).sum().to(torch.int32).reshape(1))

    def store_prefill(self, attn, kv: torch.Tensor) -> None:
        """kv bf16 [B, T, 2d]: the {k | v} rows of the prompt block."""
        self.self_kv[attn][:, :kv.shape[1]].copy_(kv)

    def self_step(self, attn, q, k, v, n_head: int, scale: float, q_prescaled: bool) -> torch.Tensor:
        return K.attn_decode(q, self.self_kv[attn], n_head, scale, new_kv=(k, v), lens=self.len, q_prescaled=q_prescaled)

    def cross_step(self, attn, q, n_head: int, scale: float) -> torch.Tensor:
        return K.attn_decode(q, self.cross_kv[attn], n_head, scale)


def check_ts_rules(n_vocab: int, eot: int, suppress: Sequence[int], suppress_first: Sequence[int], timestamp_begin: Optional[int],
                   no_timestamps: Optional[int] = None, max_initial_timestamp_index: Optional[int] = 50, beam_size: Optional[int] = None):
    """The constants of the timestamp rules (include/wft.h "Timestamp rules") -> (timestamp_begin, no_timestamps or None,
    max_initial_timestamp_index or None), or None when timestamp_begin is None (no rules: the other two are not looked at).
    ValueError: timestamp_begin outside (eot, n_vocab); no_timestamps outside the vocabulary; a negative max_initial_timestamp_index;
    a suppressed id that is a timestamp (the rules own those columns); and for beam search (beam_size = W) what guarantees W
    candidates that are not `eot` at every step, so that wft_beam_update never runs out of them:
      first step: only beam 0 counts and rule 4 leaves it the timestamps 0..max_initial — W of them must exist;
      later steps: all W beams count and each keeps a live column that is not eot.  Last token a timestamp after a timestamp
      (or the only sampled token): every text column is live and rule 5 cannot fire (no live timestamp) — so at least W + 1 text
      columns must survive suppress | suppress_first | {no_timestamps}, which also covers a text token behind which no timestamp
      is left (t = V - 1).  Last token a timestamp after text: that timestamp t itself stays live (rule 3 keeps it, rule 5 only
      ever removes text).  Otherwise text is live unless rule 5 removes it, which needs a live timestamp to win."""
    if timestamp_begin is None:
        return None
    V, tsb = int(n_vocab), int(timestamp_begin)
    if not int(eot) < tsb < V:
        raise ValueError(f"timestamp_begin={timestamp_begin} must lie in (eot={eot}, n_vocab={V})")
    if no_timestamps is not None and not 0 <= int(no_timestamps) < V:
        raise ValueError(f"no_timestamps={no_timestamps} is outside the vocabulary")
    if max_initial_timestamp_index is not None and (isinstance(max_initial_timestamp_index, bool) or int(max_initial_timestamp_index) < 0):
        raise ValueError(f"max_initial_timestamp_index must be None or >= 0, got {max_initial_timestamp_index!r}")
    dead = {int(t) for t in suppress} | {int(t) for t in suppress_first}
    if dead and max(dead) >= tsb:
        raise ValueError(f"suppress / suppress_first hold a timestamp id (>= timestamp_begin={tsb}): the timestamp rules own those columns")
    no_ts = None if no_timestamps is None else int(no_timestamps)
    max_initial = None if max_initial_timestamp_index is None else int(max_initial_timestamp_index)
    if beam_size is not None:
        W = int(beam_size)
        if max_initial is not None and max_initial < W - 1:
            raise ValueError(f"beam_size={W} needs max_initial_timestamp_index >= {W - 1}: only the timestamps 0..max_initial are live at the first step")
        last = V - 1 if max_initial is None else min(V - 1, tsb + max_initial)
        first_live = last - tsb + 1 - (1 if no_ts is not None and tsb <= no_ts <= last else 0)
        if first_live < W:
            raise ValueError(f"beam_size={W} needs {W} live timestamps at the first step, {first_live} are left")
        text_live = tsb - len({t for t in dead | ({no_ts} if no_ts is not None else set()) if 0 <= t < tsb})
        if text_live < W + 1:
            raise ValueError(f"beam_size={W} needs at least {W + 1} un-suppressed text columns under the timestamp rules, {text_live} are left")
    return (tsb, no_ts, max_initial)


def ts_extra(ts_rules) -> tuple:
    """What the rule constants add to a graph session's fingerprint: the captured pick / top-k launch holds them BY VALUE, so a step
    captured under other rules (or none) must never be replayed."""
    return (("ts_rules",) + tuple(ts_rules),) if ts_rules is not None else ()


def _mask(ids: Sequence[int], n_vocab: int, device) -> Optional[torch.Tensor]:
    ids = [int(i) for i in ids]
    if not ids:
        return None
    if min(ids) < 0 or max(ids) >= n_vocab:
        raise ValueError("suppressed token ids must lie inside the vocabulary")
    m = torch.zeros(n_vocab, dtype=torch.uint8)
    m[ids] = 1
    return m.to(device)
