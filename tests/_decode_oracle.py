"""Test helper: greedy decoding as its definition — a full decoder re-forward of the CPU oracle (oracle/whisper_oracle.py) over the
growing prefix — and the prefix-following comparison of the engine's cached decoder against it.

A free-running comparison of two token streams means nothing on a random-init model (one near-tie flips a token and everything
after it differs), so the oracle is evaluated ON THE ENGINE'S OWN PREFIX at every step."""
from dataclasses import dataclass, field
from typing import List

import torch
import torch.nn.functional as F

from oracle import whisper_oracle as O
from whisper_finetune.engine import decode as D

TAU = 0.05         # an engine pick that is not the oracle's argmax must have an oracle logit within TAU of the oracle's maximum
FLIP_SHARE = 0.10  # and at most this share of the steps may need that excuse


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def oracle_last_logits(oracle, xa_ref, tokens, lens):
    """fp32 oracle logits [B, V] of every row's position lens[b] - 1, from ONE re-forward over the right-padded prefixes (causal:
    what lies behind a row's end cannot reach it).  Oracle.decoder restated up to its last two lines, which act on every position
    by itself (LayerNorm, the tied product): they are applied to the gathered row only — the logits of all positions of 20 rows x
    448 tokens would be 1.9 GB."""
    L = int(lens.max())
    p, dims = oracle.p, oracle.dims
    with torch.no_grad():
        x = F.embedding(tokens[:, :L], p["decoder.token_embedding.weight"]) + p["decoder.positional_embedding"][:L]
        x = oracle.ra(x.to(xa_ref.dtype))
        for i in range(dims.n_text_layer):
            x = oracle.block(x, f"decoder.blocks.{i}", dims.n_text_head, xa=xa_ref, causal=True)
        x = x[torch.arange(tokens.shape[0]), lens.long() - 1]
        x = oracle.ra(O.layer_norm(x, p["decoder.ln.weight"], p["decoder.ln.bias"]))
        return oracle.ra(x @ oracle.rw(p["decoder.token_embedding.weight"]).to(x.dtype).T).float()


@dataclass
class Trace:
    picks: List[torch.Tensor] = field(default_factory=list)      # per step: i64 [B], what the engine picked
    logprobs: List[torch.Tensor] = field(default_factory=list)   # per step: f32 [B]
    active: List[torch.Tensor] = field(default_factory=list)     # per step: bool [B], row unfinished before the pick
    ref_logits: List[torch.Tensor] = field(default_factory=list)  # per step: oracle logits [B, V] on the engine's prefix
    rel_teacher: List[float] = field(default_factory=list)       # cached logits vs the engine's own teacher-forced last row
    rel_oracle: List[float] = field(default_factory=list)        # cached logits vs the fp32 oracle
    tokens: torch.Tensor = None
    lens: torch.Tensor = None
    sum_logprob: torch.Tensor = None


def follow(model, oracle, mel, prompt, prompt_len, steps: int, *, eot: int, max_len: int, compare_teacher: bool = True) -> Trace:
    """Run `steps` cached steps of the engine (prefill + steps - 1 single-token steps) from the pieces greedy_decode is made of,
    recording at every step the cached logits row of each sequence against (a) the engine's teacher-forced logits and (b) the
    fp32 oracle's, both on the same prefix, worst row per step."""
    V = model.dims.n_vocab
    tr = Trace()
    model.eval()
    with torch.no_grad():
        xa = model.encoder(mel)
        xa_ref = oracle.encoder(mel.float().cpu())
        cache = D.KVCache(model.decoder, prompt.shape[0], device=mel.device)
        cache.start(prompt, prompt_len, eot=eot, max_len=max_len, n_vocab=V)
        for i in range(steps):
            logits = D.prefill(model.decoder, cache, xa) if i == 0 else D.step(model.decoder, cache)
            lens, toks = cache.len.cpu(), cache.tokens.cpu()
            got = logits[:, :V].float().cpu()
            ref = oracle_last_logits(oracle, xa_ref, toks, lens)
            tr.rel_oracle.append(max(rel(got[b], ref[b]) for b in range(got.shape[0])))
            if compare_teacher:
                L = int(lens.max())
                tf = model.decoder(toks[:, :L].to(mel.device), xa)[torch.arange(got.shape[0]), lens.long() - 1].cpu()
                tr.rel_teacher.append(max(rel(got[b], tf[b]) for b in range(got.shape[0])))
            tr.ref_logits.append(ref)
            tr.active.append(cache.finished.cpu() == 0)
            p, lp = D.pick(model.decoder, cache, logits, want_pick=True)
            tr.picks.append(p.cpu()); tr.logprobs.append(lp.cpu())
        tr.tokens, tr.lens, tr.sum_logprob = cache.tokens.cpu(), cache.len.cpu(), cache.sum_logprob.cpu()
    return tr


def check_prefix_following(tr: Trace, what: str):
    """Every engine pick equals the oracle's argmax on the same prefix or has an oracle logit within TAU of the oracle's maximum;
    the share of steps that need the TAU clause is at most FLIP_SHARE.  Prints both figures."""
    n = flips = 0
    worst = 0.0
    for p, ref, act in zip(tr.picks, tr.ref_logits, tr.active):
        for b in range(p.shape[0]):
            if not bool(act[b]):
                continue
            n += 1
            if int(p[b]) != int(ref[b].argmax()):
                flips += 1
                worst = max(worst, float(ref[b].max() - ref[b, int(p[b])]))
    share = flips / max(n, 1)
    print(f"{what}: {flips} of {n} picks are not the fp32 oracle's argmax (share {share:.4f}, cap {FLIP_SHARE}); largest shortfall {worst:.3e} (tau {TAU})")
    assert n > 0
    assert worst <= TAU, (what, worst)
    assert share <= FLIP_SHARE, (what, share)
