"""KV-cached greedy decoding on the engine's decoder: token ids in, token ids out.

The greedy path of upstream's `whisper.decoding` (`DecodingTask._main_loop` with `GreedyDecoder`, `SuppressTokens`,
`SuppressBlank`, `DecodingOptions(without_timestamps=True)`); no tokenizer, beam search, temperature fallback, timestamp rules
or language detection.

Everything that changes from token to token lives in device memory (`KVCache`: len / tokens / finished / sum_logprob), so a
step is a fixed sequence of launches whose arguments never change: LayerNorm and every projection through the existing
kernels at M = B, attention / embedding / the pick through csrc/decode.hip.  The host reads one counter every `sync_every`
steps.

Cache layout (DESIGN.md §3 "Greedy-decoding layouts"): per decoder layer one self-attention buffer bf16 [B, n_text_ctx, 2d] whose row (b, t) is
{k | v} of token t — the k and v thirds of the fused q/k/v projection row, appended by the attention kernel itself — and one
cross-attention buffer bf16 [B, n_audio_ctx, 2d], the output of the fused key/value GEMM, computed once per audio batch.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import kernels as K

BF16 = torch.bfloat16


class KVCache:
    """Keys / values of every decoder layer plus the per-row decoding state, for `batch` sequences.

    Handed to the decoder as `kv_cache=`: a call with T > 1 tokens is the prefill (the teacher-forced kernels over the
    right-padded prompts; k / v rows stored), a call with T = 1 is a cached step on the single-token kernels."""

    def __init__(self, decoder, batch: int, device=None):
        pos = decoder.positional_embedding
        device = pos.device if device is None else device
        self.n_ctx, d = pos.shape
        self.batch = int(batch)
        self.self_kv = {blk.attn: torch.empty((batch, self.n_ctx, 2 * d), dtype=BF16, device=device) for blk in decoder.blocks}
        self.cross_kv = {blk.cross_attn: None for blk in decoder.blocks}
        i32 = dict(dtype=torch.int32, device=device)
        self.tokens = torch.zeros((batch, self.n_ctx), dtype=torch.int64, device=device)
        self.len = torch.ones(batch, **i32)
        self.prompt_len = torch.ones(batch, **i32)
        self.finished = torch.zeros(batch, **i32)
        self.unfinished = torch.full((1,), batch, **i32)
        self.sum_logprob = torch.zeros(batch, dtype=torch.float32, device=device)
        self.prompt_T = 0       # width of the right-padded prompt block (host constant of this decode)
        self.prefilled = False
        self.eot, self.max_len = 0, self.n_ctx
        self.suppress = self.suppress_first = None

    def is_cross(self, attn) -> bool:
        return attn in self.cross_kv

    def start(self, prompt: torch.Tensor, prompt_len: Optional[torch.Tensor], *, eot: int, max_len: Optional[int] = None,
              suppress: Sequence[int] = (), suppress_first: Sequence[int] = (), n_vocab: int) -> None:
        """Load the prompts (i64 [B, T], right-padded; prompt_len [B] or None = all T long) and reset the state."""
        B, T = prompt.shape
        max_len = self.n_ctx if max_len is None else int(max_len)
        if B != self.batch or not 1 <= T <= self.n_ctx:
            raise ValueError(f"prompt {tuple(prompt.shape)} does not fit a cache of {self.batch} x {self.n_ctx}")
        if not T <= max_len <= self.n_ctx:
            raise ValueError(f"max_len={max_len} must lie in [prompt width {T}, n_text_ctx {self.n_ctx}]")
        if not 0 <= int(eot) < n_vocab:
            raise ValueError(f"eot={eot} is outside the vocabulary")
        dev = self.tokens.device
        self.tokens.fill_(int(eot))
        self.tokens[:, :T].copy_(prompt.to(dev))
        if prompt_len is None:
            self.len.fill_(T)
        else:
            pl = torch.as_tensor(prompt_len).to(device=dev, dtype=torch.int32).reshape(B)
            if int(pl.min()) < 1 or int(pl.max()) > T:
                raise ValueError("prompt_len must lie in [1, prompt width]")
            self.len.copy_(pl)
        self.prompt_len.copy_(self.len)
        self.finished.copy_((self.len >= max_len).to(torch.int32))
        self.unfinished.copy_((self.finished == 0).sum().to(torch.int32).reshape(1))
        self.sum_logprob.zero_()
        self.prompt_T, self.prefilled = T, False
        self.eot, self.max_len = int(eot), max_len
        self.suppress = _mask(suppress, n_vocab, dev)
        self.suppress_first = _mask(suppress_first, n_vocab, dev)
        for key in self.cross_kv:
            self.cross_kv[key] = None


def _mask(ids: Sequence[int], n_vocab: int, device) -> Optional[torch.Tensor]:
    ids = [int(i) for i in ids]
    if not ids:
        return None
    if min(ids) < 0 or max(ids) >= n_vocab:
        raise ValueError("suppressed token ids must lie inside the vocabulary")
    m = torch.zeros(n_vocab, dtype=torch.uint8)
    m[ids] = 1
    return m.to(device)


def prefill(decoder, cache: KVCache, xa: torch.Tensor) -> torch.Tensor:
    """The prompts through the teacher-forced kernels (causal; k / v stored, cross k / v computed) -> padded bf16 logits [B, Vpad]
    of every row's LAST prompt position (len[b] - 1), from which its first token is picked."""
    T = cache.prompt_T
    h = decoder.hidden(cache.tokens[:, :T], xa, kv_cache=cache)  # [B, T, d], final LayerNorm applied
    rows = torch.arange(cache.batch, device=h.device) * T + (cache.len.long() - 1)
    last = h.reshape(cache.batch * T, -1).index_select(0, rows)
    cache.prefilled = True
    return decoder.padded_logits(last.view(cache.batch, 1, -1))


def step(decoder, cache: KVCache) -> torch.Tensor:
    """One cached step: the token at len[b] - 1 of every row through the decoder -> padded bf16 logits [B, Vpad]."""
    h = decoder.hidden(None, None, kv_cache=cache)  # [B, 1, d]
    return decoder.padded_logits(h)


def pick(decoder, cache: KVCache, logits: torch.Tensor, want_pick: bool = False):
    """Greedy pick from the padded logits and the state update of every unfinished row (wft_decode_pick)."""
    V = decoder.token_embedding.weight.shape[0]
    return K.decode_pick(logits, V, cache.tokens, cache.len, cache.finished, cache.sum_logprob, cache.unfinished, eot=cache.eot,
                         max_len=cache.max_len, suppress=cache.suppress, suppress_first=cache.suppress_first,
                         first_len=cache.prompt_len, want_pick=want_pick)


@torch.no_grad()
def greedy_decode(model, mel: torch.Tensor, prompt: torch.Tensor, prompt_len=None, *, eot: int, max_len: Optional[int] = None,
                  suppress: Sequence[int] = (), suppress_first: Sequence[int] = (), sync_every: int = 8):
    """-> (tokens i64 [B, L] — prompt included, padded with `eot` behind each row's end —, lengths i64 [B], sum_logprob f32 [B]).

    A row ends with the `eot` it picked (counted in its length) or at `max_len` tokens (default n_text_ctx).  `sum_logprob` sums
    the log-probabilities of the generated tokens, the `eot` included, under the softmax of the suppressed logits."""
    if getattr(model, "compute_dtype", "bf16") != "bf16":
        raise NotImplementedError("greedy_decode runs in the bf16 compute mode only: the single-token kernels (csrc/decode.hip) are bf16; "
                                  "call model.set_compute_dtype('bf16') to decode")
    if sync_every < 1:
        raise ValueError("sync_every must be >= 1")
    was_training = model.training
    model.eval()
    try:
        dec = model.decoder
        B = prompt.shape[0]
        cache = KVCache(dec, B, device=mel.device)
        cache.start(prompt, prompt_len, eot=eot, max_len=max_len, suppress=suppress, suppress_first=suppress_first, n_vocab=model.dims.n_vocab)
        most = cache.max_len - int(cache.prompt_len.min())  # picks until the shortest prompt reaches max_len
        if most > 0:
            logits = prefill(dec, cache, model.encoder(mel))
            for i in range(most):
                if i > 0:
                    if i % sync_every == 0 and int(cache.unfinished.item()) == 0:
                        break
                    logits = step(dec, cache)
                pick(dec, cache, logits)
        lengths = cache.len.long()
        L = int(lengths.max())
        tokens = cache.tokens[:, :L].clone()
        tokens.masked_fill_(torch.arange(L, device=tokens.device)[None, :] >= lengths[:, None], cache.eot)
        return tokens, lengths, cache.sum_logprob.clone()
    finally:
        model.train(was_training)
