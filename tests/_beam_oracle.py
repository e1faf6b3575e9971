"""Test helper: beam search as its definition, in plain Python (lists and dictionaries, fp32 adds through numpy).  Imports nothing
from the engine.  Written from the algorithm the package documents (engine/decode/beam.py, include/wft.h), which restates
upstream whisper's BeamSearchDecoder + MaximumLikelihoodRanker under without_timestamps=True:

  W = beam size, audio a owns rows r = a*W + j; C = round(W * patience) (Python's round).  One step per audio that is not done:
   1. logp[r, :] = log-softmax of row r over its live columns (`suppress` always, `suppress_first` while len == first_len);
   2. cand[r] = the W + 1 largest, descending, ties to the lower token id;
   3. candidates (j, i) score sum_logprob[j] + cand_logp[j][i] (one fp32 add); at the audio's FIRST step only j = 0 contributes;
   4. order: score descending, ties to the lower j, then the lower i;
   5. walk: an eot candidate is newly finished (beam j's tokens + eot, that score); any other becomes the next beam; stop at W beams;
   6. newly finished sequences join the audio's list, in walk order, while it holds fewer than C;
   7. done when the list holds C entries or the new length is max_len; a done audio is frozen.
  End: an audio with fewer than W entries receives its beams in descending sum_logprob (ties to the lower j) until it holds W; rank by
  sum_logprob / n (n = generated tokens without the final eot; with length_penalty a: / ((5 + n) / 6) ** a; n = 0 -> -inf); the first
  maximum in list order wins.

Two entry points: `step_logits` (fp32 logits per row) and `step_candidates` (per-row candidate lists, e.g. the engine's own)."""
import numpy as np

F = np.float32


class Beam:
    def __init__(self, tokens, slp, anc):
        self.tokens, self.slp, self.anc = list(tokens), F(slp), list(anc)


class Audio:
    def __init__(self, a, prompt, W, max_len):
        self.a, self.first_len = a, len(prompt)
        self.beams = [Beam(prompt, 0.0, [a * W] * len(prompt)) for _ in range(W)]
        self.fin = []            # [(tokens incl. eot, fp32 score)]
        self.first = True        # no step taken yet
        self.done = len(prompt) >= max_len
        self.src = None          # source beam of every slot at the last update


class State:
    def __init__(self, prompts, W, C, eot, max_len):
        assert W >= 1 and C >= 1
        self.W, self.C, self.eot, self.max_len = W, C, int(eot), int(max_len)
        self.audios = [Audio(a, p, W, max_len) for a, p in enumerate(prompts)]

    @property
    def unfinished(self):
        return sum(not au.done for au in self.audios)


def candidates(W, patience=1.0):
    """C = round(W * patience) with Python's round."""
    return round(W * patience)


def topk_logits(row, k, dead=()):
    """row: fp32 logits [V] -> [(token, fp32 log-softmax over the live columns)] of the k largest, descending, ties to the lower id."""
    x = np.asarray(row, dtype=F).copy()
    live = np.ones(x.shape[0], dtype=bool)
    live[list(dead)] = False
    xl = x[live]
    m = xl.max()
    lse = F(m + F(np.log(np.exp((xl - m).astype(F)).astype(F).sum(dtype=F))))
    key = np.where(live, x, -np.inf)
    order = np.argsort(-key, kind="stable")[:k]  # stable: ties to the lower id
    return [(int(t), F(x[t] - lse)) for t in order if live[t]]


def step_candidates(st, cands):
    """cands[a][j] = [(token, logp)] of beam j of audio a, descending (rows of done audios are ignored; at an audio's first step only
    j = 0 is read).  Mutates the state."""
    W = st.W
    for au, per_beam in zip(st.audios, cands):
        if au.done:
            continue
        L = len(au.beams[0].tokens)
        flat = []
        for j in range(1 if au.first else W):
            for i, (tok, lp) in enumerate(per_beam[j]):
                flat.append((F(au.beams[j].slp + F(lp)), j, i, int(tok)))
        flat.sort(key=lambda c: (-float(c[0]), c[1], c[2]))
        new, newly = [], []
        for score, j, i, tok in flat:
            if tok == st.eot:
                newly.append((au.beams[j].tokens + [tok], score))
            else:
                new.append(Beam(au.beams[j].tokens + [tok], score, au.beams[j].anc[:L - 1] + [au.a * W + j]))
                new[-1].src = j
                if len(new) == W:
                    break
        assert len(new) == W, "fewer than W candidates that are not eot: the host check should have refused this"
        for seq in newly:
            if len(au.fin) < st.C:
                au.fin.append(seq)
        au.beams, au.src, au.first = new, [b.src for b in new], False
        au.done = len(au.fin) >= st.C or L + 1 >= st.max_len


def step_logits(st, logits, suppress=(), suppress_first=()):
    """logits: fp32 [R, V], row a*W + j for beam j of audio a (at an audio's first step only row a*W is read)."""
    W = st.W
    cands = []
    for au in st.audios:
        per = []
        for j in range(W):
            b = au.beams[j]
            dead = set(suppress) | (set(suppress_first) if len(b.tokens) == au.first_len else set())
            per.append(topk_logits(logits[au.a * W + j], W + 1, dead))
        cands.append(per)
    step_candidates(st, cands)
    return cands


def score(n, slp, length_penalty=None):
    if n <= 0:
        return float("-inf")
    return float(slp) / (float(n) if length_penalty is None else ((5.0 + n) / 6.0) ** float(length_penalty))


def finalize(st, length_penalty=None):
    """-> per audio ([(tokens, fp32 sum_logprob, n)] in list order, index of the winner)."""
    out = []
    for au in st.audios:
        entries = [(t, s, len(t) - au.first_len - 1) for t, s in au.fin]
        for j in sorted(range(st.W), key=lambda j: -float(au.beams[j].slp)):
            if len(entries) >= st.W:
                break
            entries.append((au.beams[j].tokens, au.beams[j].slp, len(au.beams[j].tokens) - au.first_len))
        best, win = None, 0
        for i, (t, s, n) in enumerate(entries):
            sc = score(n, s, length_penalty)
            if best is None or sc > best:
                best, win = sc, i
        out.append((entries, win))
    return out
