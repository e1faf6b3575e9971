"""KV-cached greedy and beam-search decoding on the engine's decoder: token ids in, token ids out.

The greedy path of upstream's `whisper.decoding` (`DecodingTask._main_loop` with `GreedyDecoder`, `SuppressTokens`,
`SuppressBlank`, `DecodingOptions(without_timestamps=True)`) and, in the second half of this file, its `BeamSearchDecoder` +
`MaximumLikelihoodRanker` on a KV cache that the beams of an audio share (`BeamCache`, `beam_decode`); with `timestamp_begin=` both
decode under upstream's `ApplyTimestampRules` (restated in include/wft.h "Timestamp rules"; the pick / top-k kernels apply them,
`timestamp_segments` reads the result).  The third part is sampling: `sample_decode` draws `best_of` samples per audio at a
temperature on the device (wft_decode_sample: Gumbel-max over Philox noise, include/wft.h "Sampled decoding") on a cache whose samples
share the prompt keys and the cross keys / values (`SampleCache`), and `decode_with_fallback` is upstream's temperature ladder of
`transcribe()` (`decode_with_fallback`, `needs_fallback`: average log-probability, compression ratio, no-speech probability).
Upstream's behaviour is restated; parity with its binary and with torch's random stream is unpinned.  No tokenizer; language
detection and the long-audio `transcribe()` loop live in engine/transcribe.py.

Everything that changes from token to token lives in device memory (`KVCache`: len / tokens / finished / sum_logprob), so a
step is a fixed sequence of launches whose arguments never change: LayerNorm and every projection through the existing
kernels at M = B, attention / embedding / the pick through csrc/decode_attn.hip and csrc/decode_pick.hip.  The host reads one counter every `sync_every`
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


WEIGHT_MODES = ("bf16", "int8")  # what the streaming GEMMs of a cached step read (stream_gemm(weights=...))
# the `weights=` keyword of every decode call: "w8a8" = the "int8" steps behind an encoder and a prefill on the W8A8 kernel (int8_gemm)
DECODE_WEIGHTS = ("bf16", "int8", "w8a8")


def step_weights(weights: str) -> str:
    """The weights mode of the CACHED steps: those of "w8a8" are the weight-only "int8" steps (wft_gemm_nt_stream_q8)."""
    return "int8" if weights == "w8a8" else weights


def stream_gemm_active() -> bool:
    return getattr(_TLS, "stream_gemm", False)


def stream_gemm_weights() -> str:
    """"int8" inside an active stream_gemm(weights="int8") context, else "bf16"."""
    return getattr(_TLS, "stream_weights", "bf16") if stream_gemm_active() else "bf16"


@contextlib.contextmanager
def stream_gemm(enabled: bool = True, weights: str = "bf16"):
    """Inside this context, under torch.no_grad(), `ops.linear` and the tied logits product send a GEMM to the weight-streaming
    kernel for M <= 32 (csrc/gemm_stream.hip, wft_gemm_nt_stream_bf16) when wft_gemm_nt_stream_ok serves it, and to
    wft_gemm_nt_bf16 otherwise.  Thread-local, in the style of runtime.exchange_launch_mode; outside it nothing changes.  A context
    and not a model attribute: whoever drives prefill / step / pick itself runs under it unchanged.
    weights="int8" (thread-local with the switch): the products that wft_gemm_nt_stream_q8_ok serves read the int8 image of the group's
    shadow (LinearGroup.shadows_q8, wft_gemm_nt_stream_q8) — weight-only: activations stay bf16; a call it does not serve goes on as
    under "bf16".  Everything that is not such a step (the prefill at M > 32, the encoder, training) never looks at the mode."""
    if weights not in WEIGHT_MODES:
        raise ValueError(f"weights must be one of {WEIGHT_MODES}, got {weights!r}")
    old = stream_gemm_active(), getattr(_TLS, "stream_weights", "bf16")
    _TLS.stream_gemm, _TLS.stream_weights = bool(enabled), weights
    try:
        yield
    finally:
        _TLS.stream_gemm, _TLS.stream_weights = old


def int8_gemm_active() -> bool:
    return getattr(_TLS, "int8_gemm", False)


@contextlib.contextmanager
def int8_gemm(enabled: bool = True):
    """Inside this context, under torch.no_grad(), `ops.linear` sends a product with M > 32 that wft_gemm_nt_i8_ok serves to the W8A8
    kernel (csrc/gemm_i8.hip): the input is quantised per row once per call (wft_quantize_rows_i8, the kernel that quantises the weight
    shadows), the weight operand is the int8 image of the group's shadow (LinearGroup.shadows_q8: merged LoRA delta and folded query
    scale included) and wft_gemm_nt_i8 multiplies them on the int8 matrix cores.  A fused q/k/v group is one call, so one quantiser
    pass.  Every other call — M <= 32, grad mode, the tied logits product, the fp32 compute mode — goes on exactly as outside.
    Thread-local beside `stream_gemm` and independent of it; decoding's weights="w8a8" runs the encoder and the prefill under it."""
    old = int8_gemm_active()
    _TLS.int8_gemm = bool(enabled)
    try:
        yield
    finally:
        _TLS.int8_gemm = old


def encode(model, mel: torch.Tensor, weights: str = "bf16") -> torch.Tensor:
    """model.encoder(mel) as a decode under `weights` runs it: under int8_gemm() when weights == "w8a8", else today's call.  Every
    group asks for its image through LinearGroup.shadows_q8 at its product, which first brings the bf16 shadow up to date and then
    the image (an optimizer step between two calls is seen here, in front of the first int8 product — not only behind the prefill)."""
    with int8_gemm(weights == "w8a8"):
        return model.encoder(mel)


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


# ----------------------------------------------------------------------------- the captured step
MAX_SESSIONS = 2  # graph sessions kept per model and kind of decoding; the oldest is evicted
# model -> OrderedDict[key -> _GraphSession], one table per kind, so greedy and beam sessions are counted and evicted apart:
# key = (batch, device), (audios, beam, candidates, device) for beam search, (audios, best_of, device) for sampling.  Kept OFF the module, like engine/graph.py's
# registry: CUDAGraph objects neither pickle nor deep-copy, and a dropped model drops its sessions.
_SESSIONS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_BEAM_SESSIONS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_SAMPLE_SESSIONS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _groups(decoder):
    from . import ops

    for mod in decoder.modules():
        for v in vars(mod).values():
            if isinstance(v, ops.LinearGroup):
                yield mod, v


class _GraphSession:
    """One HIP graph = body(decoder, cache) — a cached step and its state update — on the static buffers of ONE cache, replayed once
    per token (the first update of a decode, fed by the prefill, stays outside).

    Everything a step reads that changes between tokens or between decodes lives in buffers this session owns (the cache, the
    cross keys / values, the two suppression masks); everything else whose ADDRESS the graph holds — decoder parameters, the bf16
    weight shadows and stacked biases of every Linear group, the scratch slots — is referenced by `keep` and named in the
    fingerprint that is compared after every prefill: any difference recaptures, a mismatch never replays.  `extra`: what the
    caller adds to the fingerprint; `who` names the caller in error messages."""

    def __init__(self, decoder, cache, body, extra: tuple, who: str):
        self.cache, self._body, self._extra, self.who = cache, body, tuple(extra), who
        device = cache.tokens.device
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

    def _fingerprint(self, decoder, stream, slots=None):
        """stream: False, or the weights mode of the streaming GEMMs ("bf16" / "int8"; True is read as "bf16")."""
        c = self.cache
        dev = c.tokens.device
        stream = "bf16" if stream is True else stream
        fp = [stream, c.eot, c.max_len, decoder.token_embedding.weight.shape[0]]
        keep = []
        for p in decoder.parameters():
            fp.append(p.data_ptr()); keep.append(p.data)
        for mod, g in _groups(decoder):
            fp.append((None if g.W is None else g.W.data_ptr(), None if g.bias is None else g.bias.data_ptr(), g.lkey is not None,
                       "parametrizations" in mod._modules))
            keep += [g.W, g.bias]
            if stream == "int8":  # the int8 images a captured step reads: replaced, dropped or first made later -> never replayed
                fp.append((None if g.Q is None else g.Q.data_ptr(), None if g.qscale is None else g.qscale.data_ptr()))
                keep += [g.Q, g.qscale]
        fp.append(("adapted", sum("parametrizations" in mod._modules for mod in decoder.modules())))
        # scratch slots of this device: all of them when capturing, afterwards the captured ones (a slot that appears later — a
        # training step in between — is not in the graph; one that was replaced or dropped is a mismatch)
        if slots is None:
            slots = sorted(key[2] for key in K._TN_WS if key[0] == dev.type and key[1] == dev.index)
        for name in slots:
            ws = K._TN_WS.get((dev.type, dev.index, name))
            fp.append((name, None if ws is None else ws.data_ptr())); keep.append(ws)
        return tuple(fp) + self._extra, keep, tuple(slots)

    def valid(self, decoder, stream) -> bool:
        return self.graph is not None and self.fingerprint == self._fingerprint(decoder, stream, self.slots)[0]

    def capture(self, decoder, stream) -> None:
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
                    with stream_gemm(bool(stream), "int8" if stream == "int8" else "bf16"):
                        logits = self._body(decoder, c)
        except Exception as exc:
            # (tensors first allocated inside a failed capture must not be used: nothing of this session survives)
            self.graph = None
            raise RuntimeError(f"{self.who}(step='graph'): capturing the decoding step failed ({type(exc).__name__}: {exc}); "
                               "use step='eager'") from exc
        cur.wait_stream(side)
        if self._fingerprint(decoder, stream)[0] != fp:
            raise RuntimeError(f"{self.who}(step='graph'): a buffer of the decoding step was replaced DURING its capture (a scratch slot "
                               "or a weight shadow that the warm-up step should have created); use step='eager'")
        self.graph, self.fingerprint, self.keep, self.slots = g, fp, keep + [logits], slots
        self.captures += 1

    def replay(self) -> None:
        self.graph.replay()
        self.replays += 1


def _session(table, model, key: tuple, make) -> _GraphSession:
    """The session of `model` under `key` in `table`, most recently used last; make() builds a missing one once the oldest is gone."""
    reg = table.get(model)
    if reg is None:
        reg = table[model] = OrderedDict()
    sess = reg.get(key)
    if sess is None:
        while len(reg) >= MAX_SESSIONS:
            reg.popitem(last=False)
        sess = reg[key] = make()
    else:
        reg.move_to_end(key)
    return sess


def sessions(model) -> dict:
    """{(batch, device): session} of `model` (tests and tools read the capture / replay counters)."""
    return dict(_SESSIONS.get(model) or {})


def beam_sessions(model) -> dict:
    """{(audios, beam_size, candidates, device): session} of `model`: the captured beam steps (kept apart from `sessions(model)`)."""
    return dict(_BEAM_SESSIONS.get(model) or {})


def sample_sessions(model) -> dict:
    """{(audios, best_of, device): session} of `model`: the captured sampling steps (a third table, counted and evicted apart)."""
    return dict(_SAMPLE_SESSIONS.get(model) or {})


def release_graphs(model) -> None:
    """Drop every captured decoding step of `model` with the static buffers it pins (self-attention cache, cross keys / values,
    the graph's private pool).  The evaluator calls it when a dataset is done, so nothing stays pinned during training."""
    for table in (_SESSIONS, _BEAM_SESSIONS, _SAMPLE_SESSIONS):
        reg = table.pop(model, None)
        if reg:
            reg.clear()


STEP_MODES = ("eager", "graph")


def _check_mode(model, who: str, step: str, sync_every: int, weights: str = "bf16") -> None:
    if step not in STEP_MODES:
        raise ValueError(f"step must be one of {STEP_MODES}, got {step!r}")
    if weights not in DECODE_WEIGHTS:
        raise ValueError(f"weights must be one of {DECODE_WEIGHTS}, got {weights!r}")
    if weights != "bf16" and step != "graph":
        raise ValueError(f"{who}(weights={weights!r}) needs step='graph': only the captured steps run on the weight-streaming kernels that read int8")
    if getattr(model, "compute_dtype", "bf16") != "bf16":
        raise NotImplementedError(f"{who} runs in the bf16 compute mode only: the single-token kernels (csrc/decode_*.hip) are bf16; "
                                  "call model.set_compute_dtype('bf16') to decode")
    if sync_every < 1:
        raise ValueError("sync_every must be >= 1")


def _decode(model, mel: torch.Tensor, start: dict, *, who: str, table, key: tuple, make_cache, prefill, first, body, readout, extra=(),
            graph: bool, stream, sync_every: int, xa: Optional[torch.Tensor] = None, weights: str = "bf16"):
    """The loop of greedy_decode and beam_decode -> readout(cache) after the last step (read while the model is still in eval mode).  make_cache(decoder) builds the cache (kept in a
    graph session of `table` under key + (device,) when `graph`), start: the arguments of its start(); prefill(decoder, cache, xa)
    -> logits, first(decoder, cache, logits): the update they feed, body(decoder, cache): one cached step with its update.
    stream: False, or the weights mode of the cached steps' streaming GEMMs ("bf16" / "int8"); an int8 session is kept under its own key.
    Host reads: the fingerprint check once after the prefill, the `unfinished` counter every `sync_every` steps.
    xa: the encoder output of `mel` when the caller already has it (decode_with_fallback runs the encoder once for all rungs).
    weights: the caller's mode; "w8a8" runs the encoder and the prefill (with the cross key / value projections it stores) under
    int8_gemm(), and its cached steps are the "int8" ones (`stream` is then "int8": they share that mode's session)."""
    was_training = model.training
    model.eval()
    try:
        dec = model.decoder
        sess = None
        if graph:
            sess = _session(table, model, key + (str(mel.device),) + (("int8",) if stream == "int8" else ()), lambda: _GraphSession(dec, make_cache(dec), body, extra, who))
            sess._extra = tuple(extra)  # (a kept session may have been captured under other timestamp rules: then it recaptures)
        cache = sess.cache if graph else make_cache(dec)
        cache.start(**start, n_vocab=model.dims.n_vocab)
        # updates until the shortest prompt reaches max_len (start() has just set len to the prompt lengths; nothing ran since)
        most = cache.max_len - int(cache.len.min())
        if most > 0:
            with int8_gemm(weights == "w8a8"):
                logits = prefill(dec, cache, encode(model, mel, weights) if xa is None else xa)
            if graph:
                sess.adopt_prefill()
            if stream == "int8":
                # the prefill (bf16) has brought every weight shadow up to date; their int8 images follow here, in place — a replayed
                # step runs no Python that could notice a stale one
                for _, g in _groups(dec):
                    g.refresh_q8()
            first(dec, cache, logits)
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
                with stream_gemm(bool(stream), "int8" if stream == "int8" else "bf16"):
                    body(dec, cache)
                warmed = True
        return readout(cache)
    finally:
        model.train(was_training)


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
