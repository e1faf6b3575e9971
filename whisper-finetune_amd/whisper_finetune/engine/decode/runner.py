"""The captured step and the loop every decoder shares: `_GraphSession`, the three session tables (greedy, beam search, sampling),
`release_graphs`, the mode checks, `encode` and `_decode`."""
from __future__ import annotations

import weakref
from collections import OrderedDict
from typing import Optional

import torch

from .. import kernels as K
from .. import ops
from ..gemm_mode import DECODE_WEIGHTS, int8_gemm, stream_gemm

# ----------------------------------------------------------------------------- the captured step
MAX_SESSIONS = 2  # graph sessions kept per model and kind of decoding; the oldest is evicted
# model -> OrderedDict[key -> _GraphSession], one table per kind, so greedy and beam sessions are counted and evicted apart:
# key = (batch, device), (audios, beam, candidates, device) for beam search, (audios, best_of, device) for sampling.  Kept OFF the module, like engine/graph.py's
# registry: CUDAGraph objects neither pickle nor deep-copy, and a dropped model drops its sessions.
_SESSIONS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_BEAM_SESSIONS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_SAMPLE_SESSIONS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _groups(decoder):
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


def encode(model, mel: torch.Tensor, weights: str = "bf16") -> torch.Tensor:
    """model.encoder(mel) as a decode under `weights` runs it: under int8_gemm() when weights == "w8a8", else today's call.  Every
    group asks for its image through LinearGroup.shadows_q8 at its product, which first brings the bf16 shadow up to date and then
    the image (an optimizer step between two calls is seen here, in front of the first int8 product — not only behind the prefill)."""
    with int8_gemm(weights == "w8a8"):
        return model.encoder(mel)


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
