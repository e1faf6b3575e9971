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

import contextlib
import threading
import weakref
from collections import OrderedDict
from typing import Optional, Sequence

import torch

from . import kernels as K

BF16 = torch.bfloat16

# ----------------------------------------------------------------------------- the streaming-GEMM context
_TLS = threading.local()


def stream_gemm_active() -> bool:
    return getattr(_TLS, "stream_gemm", False)


@contextlib.contextmanager
def stream_gemm(enabled: bool = True):
    """Inside this context, under torch.no_grad(), `ops.linear` and the tied logits product send a GEMM to the weight-streaming
    kernel for M <= 32 (csrc/gemm_stream.hip, wft_gemm_nt_stream_bf16) when wft_gemm_nt_stream_ok serves it, and to
    wft_gemm_nt_bf16 otherwise.  Thread-local, in the style of runtime.exchange_launch_mode; outside it nothing changes.  A context
    and not a model attribute: whoever drives prefill / step / pick itself runs under it unchanged."""
    old = stream_gemm_active()
    _TLS.stream_gemm = bool(enabled)
    try:
        yield
    finally:
        _TLS.stream_gemm = old


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


_cached_step = step  # (greedy_decode has a keyword of that name)


def pick(decoder, cache: KVCache, logits: torch.Tensor, want_pick: bool = False):
    """Greedy pick from the padded logits and the state update of every unfinished row (wft_decode_pick)."""
    V = decoder.token_embedding.weight.shape[0]
    return K.decode_pick(logits, V, cache.tokens, cache.len, cache.finished, cache.sum_logprob, cache.unfinished, eot=cache.eot,
                         max_len=cache.max_len, suppress=cache.suppress, suppress_first=cache.suppress_first,
                         first_len=cache.prompt_len, want_pick=want_pick)


# ----------------------------------------------------------------------------- the captured step
MAX_SESSIONS = 2  # graph sessions kept per model (one per (batch, device)); the oldest is evicted
# model -> OrderedDict[(batch, device) -> _GraphSession].  Kept OFF the module, like engine/graph.py's registry: CUDAGraph objects
# neither pickle nor deep-copy, and a dropped model drops its sessions.
_SESSIONS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _groups(decoder):
    from . import ops

    for mod in decoder.modules():
        for v in vars(mod).values():
            if isinstance(v, ops.LinearGroup):
                yield mod, v


class _GraphSession:
    """One HIP graph = step(dec, cache) + pick(dec, cache, logits) on the static buffers of ONE KVCache, replayed once per token.

    Everything a step reads that changes between tokens or between decodes lives in buffers this session owns (the KVCache, the
    cross keys / values, the two suppression masks); everything else whose ADDRESS the graph holds — decoder parameters, the bf16
    weight shadows and stacked biases of every Linear group, the scratch slots — is referenced by `keep` and named in the
    fingerprint that is compared after every prefill: any difference recaptures, a mismatch never replays."""

    def __init__(self, decoder, batch: int, device):
        self.cache = KVCache(decoder, batch, device=device)
        self.cross = {}      # attn module -> static bf16 [B, n_audio_ctx, 2d]
        V = decoder.token_embedding.weight.shape[0]
        self.suppress = torch.zeros(V, dtype=torch.uint8, device=device)
        self.suppress_first = torch.zeros(V, dtype=torch.uint8, device=device)
        self.graph = None
        self.fingerprint = None
        self.keep = self.slots = None
        self.captures = self.replays = 0

    def adopt_prefill(self) -> None:
        """After start() + prefill(): move what they allocated afresh into the static buffers."""
        c = self.cache
        for attn, kv in c.cross_kv.items():
            buf = self.cross.get(attn)
            if buf is None or buf.shape != kv.shape:
                buf = self.cross[attn] = torch.empty_like(kv)
                self.graph = None
            if kv is not buf:
                buf.copy_(kv)
            c.cross_kv[attn] = buf
        for name in ("suppress", "suppress_first"):
            buf, m = getattr(self, name), getattr(c, name)
            if m is None:
                buf.zero_()  # (an all-zero mask suppresses nothing: the pick is the one of a NULL mask)
            elif m is not buf:
                buf.copy_(m)
            setattr(c, name, buf)

    def _fingerprint(self, decoder, stream: bool, slots=None):
        c = self.cache
        dev = c.tokens.device
        fp = [bool(stream), c.eot, c.max_len, decoder.token_embedding.weight.shape[0]]
        keep = []
        for p in decoder.parameters():
            fp.append(p.data_ptr()); keep.append(p.data)
        for mod, g in _groups(decoder):
            fp.append((None if g.W is None else g.W.data_ptr(), None if g.bias is None else g.bias.data_ptr(), g.lkey is not None,
                       "parametrizations" in mod._modules))
            keep += [g.W, g.bias]
        fp.append(("adapted", sum("parametrizations" in mod._modules for mod in decoder.modules())))
        # scratch slots of this device: all of them when capturing, afterwards the captured ones (a slot that appears later — a
        # training step in between — is not in the graph; one that was replaced or dropped is a mismatch)
        if slots is None:
            slots = sorted(key[2] for key in K._TN_WS if key[0] == dev.type and key[1] == dev.index)
        for name in slots:
            ws = K._TN_WS.get((dev.type, dev.index, name))
            fp.append((name, None if ws is None else ws.data_ptr())); keep.append(ws)
        return tuple(fp), keep, tuple(slots)

    def valid(self, decoder, stream: bool) -> bool:
        return self.graph is not None and self.fingerprint == self._fingerprint(decoder, stream, self.slots)[0]

    def capture(self, decoder, stream: bool) -> None:
        """Called behind one EAGER step of the same kind in the same decode (the warm-up: scratch slots, dynamic-LDS attributes and
        code objects exist, so nothing lazy falls into the capture).  A linear graph: one side stream, no forks."""
        self.graph = self.keep = self.fingerprint = None
        c = self.cache
        dev = c.tokens.device
        fp, keep, slots = self._fingerprint(decoder, stream)
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(cur)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    with stream_gemm(stream):
                        logits = step(decoder, c)
                        pick(decoder, c, logits)
        except Exception as exc:
            # (tensors first allocated inside a failed capture must not be used: nothing of this session survives)
            self.graph = None
            raise RuntimeError(f"greedy_decode(step='graph'): capturing the decoding step failed ({type(exc).__name__}: {exc}); "
                               "use step='eager'") from exc
        cur.wait_stream(side)
        if self._fingerprint(decoder, stream)[0] != fp:
            raise RuntimeError("greedy_decode(step='graph'): a buffer of the decoding step was replaced DURING its capture (a scratch slot "
                               "or a weight shadow that the warm-up step should have created); use step='eager'")
        self.graph, self.fingerprint, self.keep, self.slots = g, fp, keep + [logits], slots
        self.captures += 1

    def replay(self) -> None:
        self.graph.replay()
        self.replays += 1


def _session(model, batch: int, device) -> _GraphSession:
    reg = _SESSIONS.get(model)
    if reg is None:
        reg = _SESSIONS[model] = OrderedDict()
    key = (int(batch), str(device))
    sess = reg.get(key)
    if sess is None:
        while len(reg) >= MAX_SESSIONS:
            reg.popitem(last=False)
        sess = reg[key] = _GraphSession(model.decoder, batch, device)
    else:
        reg.move_to_end(key)
    return sess


def sessions(model) -> dict:
    """{(batch, device): session} of `model` (tests and tools read the capture / replay counters)."""
    return dict(_SESSIONS.get(model) or {})


def release_graphs(model) -> None:
    """Drop every captured decoding step of `model` with the static buffers it pins (self-attention cache, cross keys / values,
    the graph's private pool).  The evaluator calls it when a dataset is done, so nothing stays pinned during training."""
    reg = _SESSIONS.pop(model, None)
    if reg:
        reg.clear()


STEP_MODES = ("eager", "graph")


@torch.no_grad()
def greedy_decode(model, mel: torch.Tensor, prompt: torch.Tensor, prompt_len=None, *, eot: int, max_len: Optional[int] = None,
                  suppress: Sequence[int] = (), suppress_first: Sequence[int] = (), sync_every: int = 8, step: str = "eager",
                  _capture: bool = True, _stream_gemm: bool = True):
    """-> (tokens i64 [B, L] — prompt included, padded with `eot` behind each row's end —, lengths i64 [B], sum_logprob f32 [B]).

    A row ends with the `eot` it picked (counted in its length) or at `max_len` tokens (default n_text_ctx).  `sum_logprob` sums
    the log-probabilities of the generated tokens, the `eot` included, under the softmax of the suppressed logits.

    step="eager": every cached step is issued launch by launch.  step="graph": the cached steps run on the weight-streaming GEMMs
    (`stream_gemm`) and are replayed from ONE captured HIP graph per (batch, device) session — the first step of a decode that
    has no valid graph runs eagerly, the second is captured; at most MAX_SESSIONS sessions per model, `release_graphs(model)` frees
    them.  The prefill and the encoder keep their kernels in both modes.  `_capture=False` / `_stream_gemm=False` switch off one
    half each (tests and the A/B bench only)."""
    if step not in STEP_MODES:
        raise ValueError(f"step must be one of {STEP_MODES}, got {step!r}")
    if getattr(model, "compute_dtype", "bf16") != "bf16":
        raise NotImplementedError("greedy_decode runs in the bf16 compute mode only: the single-token kernels (csrc/decode.hip) are bf16; "
                                  "call model.set_compute_dtype('bf16') to decode")
    if sync_every < 1:
        raise ValueError("sync_every must be >= 1")
    graph = step == "graph" and _capture
    stream = step == "graph" and _stream_gemm
    was_training = model.training
    model.eval()
    try:
        dec = model.decoder
        B = prompt.shape[0]
        sess = _session(model, B, mel.device) if graph else None
        cache = sess.cache if graph else KVCache(dec, B, device=mel.device)
        cache.start(prompt, prompt_len, eot=eot, max_len=max_len, suppress=suppress, suppress_first=suppress_first, n_vocab=model.dims.n_vocab)
        most = cache.max_len - int(cache.prompt_len.min())  # picks until the shortest prompt reaches max_len
        if most > 0:
            logits = prefill(dec, cache, model.encoder(mel))
            if graph:
                sess.adopt_prefill()
            pick(dec, cache, logits)
            ready = graph and sess.valid(dec, stream)  # (the fingerprint check a replay cannot make: once per decode, after the prefill)
            warmed = False
            for i in range(1, most):
                if i % sync_every == 0 and int(cache.unfinished.item()) == 0:
                    break
                if graph and not ready and warmed:
                    sess.capture(dec, stream)
                    ready = True
                if ready:
                    sess.replay()
                    continue
                with stream_gemm(stream):
                    logits = _cached_step(dec, cache)
                    pick(dec, cache, logits)
                warmed = True
        lengths = cache.len.long()
        L = int(lengths.max())
        tokens = cache.tokens[:, :L].clone()
        tokens.masked_fill_(torch.arange(L, device=tokens.device)[None, :] >= lengths[:, None], cache.eot)
        return tokens, lengths, cache.sum_logprob.clone()
    finally:
        model.train(was_training)
