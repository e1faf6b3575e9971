"""Evaluation metrics with the reference's names (eval/metrics.py): PerUtteranceMetrics / DatasetMetrics,
compute_wer, compute_cer_batch, compute_token_metrics, compute_ece, aggregate_dataset_metrics,
compute_macro_average.  WER / CER are plain Levenshtein rates (jiwer's definition: edits / reference length);
the per-token statistics come from ONE pass of the `wft_token_stats` kernel when logits live on the GPU.
Beside the reference's names: edit_counts_host / edit_counts_batch / word_error_counts / char_error_counts — hits, substitutions,
deletions and insertions per utterance (one `wft_edit_counts_i32` launch for a whole dataset on the GPU) and the corpus-level
rates DatasetMetrics carries behind the reference's fields."""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field
from typing import Dict, Hashable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F


@dataclass
class PerUtteranceMetrics:
    prediction: str
    reference: str
    wer: float
    cer: float
    token_nll: float
    avg_log_prob: float
    token_entropy: float
    token_confidences: List[float] = field(default_factory=list)
    token_correct: List[bool] = field(default_factory=list)
    # (hits, substitutions, deletions, insertions) of the word / character alignment (edit_counts_host's rule); None: not counted
    word_counts: Optional[Tuple[int, int, int, int]] = None
    char_counts: Optional[Tuple[int, int, int, int]] = None


@dataclass
class DatasetMetrics:
    dataset_name: str
    num_samples: int
    wer: float
    cer: float
    mean_token_nll: float
    avg_log_prob: float
    mean_token_entropy: float
    ece: float
    per_utterance: List[PerUtteranceMetrics] = field(default_factory=list)
    # corpus-level rates: dataset totals over the total reference length (words; characters for corpus_cer).  None when an
    # utterance of the dataset carries no counts
    corpus_wer: Optional[float] = None
    corpus_cer: Optional[float] = None
    word_sub_rate: Optional[float] = None
    word_del_rate: Optional[float] = None
    word_ins_rate: Optional[float] = None


def _edit_distance(ref: Sequence, hyp: Sequence) -> int:
    prev = list(range(len(hyp) + 1))
    for i, r in enumerate(ref, 1):
        cur = [i] + [0] * len(hyp)
        for j, h in enumerate(hyp, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (r != h))
        prev = cur
    return prev[-1]


def wer(reference: str, hypothesis: str) -> float:
    """word error rate = (S + D + I) / #reference words."""
    ref = reference.split()
    if not ref:
        raise ValueError("one or more references are empty strings")
    return _edit_distance(ref, hypothesis.split()) / len(ref)


def cer(reference: str, hypothesis: str) -> float:
    """character error rate over the characters of the (stripped) strings, blanks included."""
    ref = list(reference.strip())
    if not ref:
        raise ValueError("one or more references are empty strings")
    return _edit_distance(ref, list(hypothesis.strip())) / len(ref)


def compute_wer(predictions: List[str], references: List[str]) -> List[float]:
    """Per-utterance WER; an empty reference scores 0 for an empty prediction, else 1 (eval/metrics.py:46-62)."""
    out = []
    for pred, ref in zip(predictions, references):
        out.append((0.0 if pred.strip() == "" else 1.0) if ref.strip() == "" else wer(ref, pred))
    return out


def compute_cer_batch(predictions: List[str], references: List[str]) -> List[float]:
    out = []
    for pred, ref in zip(predictions, references):
        out.append((0.0 if pred.strip() == "" else 1.0) if ref.strip() == "" else cer(ref, pred))
    return out


def edit_counts_host(ref: Sequence, hyp: Sequence) -> Tuple[int, int, int, int]:
    """(H, S, D, I) of the Levenshtein alignment of hyp against ref, the rule of include/wft.h "Edit counts" in plain Python:
    cell (i, j) takes the cheapest of diagonal (S + 1 on a mismatch), deletion (D + 1), insertion (I + 1), in that priority on equal
    cost — a later candidate wins only when strictly cheaper.  S + D + I == _edit_distance(ref, hyp); H = len(ref) - S - D.
    The device kernel computes the same integers (wft_edit_counts_i32); this is what runs for a model on the CPU and for a pair
    longer than the kernel's cap per side.  The split into S, D and I may differ from jiwer's (another optimal alignment)."""
    ref, hyp = list(ref), list(hyp)
    m = len(hyp)
    cost = list(range(m + 1))
    trip = [(0, 0, j) for j in range(m + 1)]
    for i, r in enumerate(ref, 1):
        ncost, ntrip = [i] + [0] * m, [(0, i, 0)] + [None] * m
        for j, h in enumerate(hyp, 1):
            sub = r != h
            c, t = cost[j - 1] + sub, trip[j - 1]
            best = (t[0] + 1, t[1], t[2]) if sub else t
            if cost[j] + 1 < c:
                c, t = cost[j] + 1, trip[j]
                best = (t[0], t[1] + 1, t[2])
            if ncost[j - 1] + 1 < c:
                c, t = ncost[j - 1] + 1, ntrip[j - 1]
                best = (t[0], t[1], t[2] + 1)
            ncost[j], ntrip[j] = c, best
        cost, trip = ncost, ntrip
    S, D, I = trip[m]
    return len(ref) - S - D, S, D, I


def edit_counts_batch(refs: Sequence[Sequence[Hashable]], hyps: Sequence[Sequence[Hashable]], device=None) -> np.ndarray:
    """(H, S, D, I) of every pair -> int64 [P, 4].  refs / hyps: P sequences of hashable items each (words, characters, token ids).
    `device` None or a CPU device: edit_counts_host per pair.  A GPU: one dict per call maps the items to int32 ids, the pair table
    and the ids go to the device in ONE packed copy, one wft_edit_counts_i32 launch scores every pair and one copy brings the counts
    back.  A pair with a side longer than the kernel's cap (4096) is an input size the kernel does not serve: it is scored on the host."""
    refs, hyps = [list(r) for r in refs], [list(h) for h in hyps]
    if len(refs) != len(hyps):
        raise ValueError(f"edit_counts_batch: {len(refs)} references for {len(hyps)} hypotheses")
    out = np.zeros((len(refs), 4), dtype=np.int64)
    dev = None if device is None else torch.device(device)
    if dev is None or dev.type == "cpu":
        for p, (r, h) in enumerate(zip(refs, hyps)):
            out[p] = edit_counts_host(r, h)
        return out
    from whisper_finetune.engine import kernels as K

    served = []
    for p, (r, h) in enumerate(zip(refs, hyps)):
        if len(r) <= K.EDIT_MAX_LEN and len(h) <= K.EDIT_MAX_LEN:
            served.append(p)
        else:
            out[p] = edit_counts_host(r, h)
    # one dict per call: item -> id in order of first appearance (dict.fromkeys and map keep the per-item work out of the interpreter)
    ids: Dict[Hashable, int] = {x: k for k, x in enumerate(dict.fromkeys(itertools.chain.from_iterable(refs[p] + hyps[p] for p in served)))}
    for c0 in range(0, len(served), K.EDIT_MAX_PAIRS):
        chunk = served[c0:c0 + K.EDIT_MAX_PAIRS]
        lens = np.array([(len(refs[p]), len(hyps[p])) for p in chunk], dtype=np.int64).reshape(-1, 2)
        total = int(lens.sum())
        flat = np.zeros(total + 1, dtype=np.int32)  # one symbol more: the kernel wants at least one, also when every pair is empty
        flat[:total] = np.fromiter(map(ids.__getitem__, itertools.chain.from_iterable(refs[p] + hyps[p] for p in chunk)), dtype=np.int32, count=total)
        rows = np.zeros((len(chunk), 4), dtype=np.int64)
        rows[:, 2:] = lens
        rows[:, 0] = np.cumsum(lens.sum(axis=1)) - lens.sum(axis=1)  # every reference, then its hypothesis, back to back
        rows[:, 1] = rows[:, 0] + lens[:, 0]
        rec, max_len = K.edit_rows(rows, total + 1)
        table = rec.view("<i4").reshape(-1)
        packed = torch.from_numpy(np.concatenate([table, flat])).to(dev)
        got = K.edit_counts(packed[table.shape[0]:], rec, max_len, rows_d=packed[:table.shape[0]]).cpu().numpy()
        if (got < 0).any():
            raise RuntimeError(f"edit_counts_batch: the kernel refused pair {chunk[int(np.flatnonzero((got < 0).any(1))[0])]}")
        out[chunk] = got
    return out


def word_error_counts(predictions: Sequence[str], references: Sequence[str], device=None) -> np.ndarray:
    """(H, S, D, I) over words per utterance -> int64 [P, 4]; wer's tokenisation (`split()`): wer == (S + D + I) / (H + S + D)."""
    return edit_counts_batch([r.split() for r in references], [p.split() for p in predictions], device)


def char_error_counts(predictions: Sequence[str], references: Sequence[str], device=None) -> np.ndarray:
    """(H, S, D, I) over characters per utterance -> int64 [P, 4]; cer's tokenisation (`list(s.strip())`, blanks included)."""
    return edit_counts_batch([list(r.strip()) for r in references], [list(p.strip()) for p in predictions], device)


def compute_token_metrics(logits: torch.Tensor, target_ids: torch.Tensor, predicted_ids: torch.Tensor
                          ) -> Tuple[float, float, float, List[float], List[bool]]:
    """(mean NLL, mean log p(predicted token), mean entropy, per-token max-prob, per-token correctness) over the
    rows whose target is not -100; logits [S, V] (eval/metrics.py:85-137)."""
    valid = target_ids != -100
    if valid.sum() == 0:
        return 0.0, 0.0, 0.0, [], []
    lg, tg, pr = logits[valid].float(), target_ids[valid], predicted_ids[valid]
    logp = F.log_softmax(lg, dim=-1)
    p = logp.exp()
    nll = F.cross_entropy(lg, tg, reduction="none").mean().item()
    avg_lp = logp.gather(1, pr.unsqueeze(1)).squeeze(1).mean().item()
    ent = -(p * logp).sum(-1).mean().item()
    return nll, avg_lp, ent, p.max(-1).values.cpu().tolist(), (pr == tg).cpu().tolist()


def token_metrics_from_stats(stats: np.ndarray, argmax: np.ndarray, targets: np.ndarray):
    """Same five quantities from the fused kernel's per-token {lse, max, E_p[x], x_target} (host numpy, one sample).
    The predicted token is the argmax, so log p(pred) = max - lse."""
    valid = targets != -100
    if not valid.any():
        return 0.0, 0.0, 0.0, [], []
    lse, mx, ex, xt = (stats[valid, k].astype(np.float64) for k in range(4))
    return (float(np.mean(lse - xt)), float(np.mean(mx - lse)), float(np.mean(lse - ex)),
            np.exp(mx - lse).tolist(), (argmax[valid] == targets[valid]).tolist())


def compute_ece(all_confidences: List[float], all_correct: List[bool], n_bins: int = 20) -> float:
    """Expected calibration error over equal-width confidence bins (lower, upper]."""
    if len(all_confidences) == 0:
        return 0.0
    conf = np.asarray(all_confidences)
    ok = np.asarray(all_correct, dtype=float)
    edges = np.linspace(0, 1, n_bins + 1)
    ece = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (conf > lo) & (conf <= hi)
        frac = sel.mean()
        if frac > 0:
            ece += frac * abs(conf[sel].mean() - ok[sel].mean())
    return ece


def aggregate_dataset_metrics(per_utterance_metrics: List[PerUtteranceMetrics], dataset_name: str) -> DatasetMetrics:
    """mean over utterances of each scalar; ECE over all tokens of the dataset; the corpus-level rates from the utterances'
    word_counts / char_counts (corpus_rates)."""
    ms = per_utterance_metrics
    if not ms:
        return DatasetMetrics(dataset_name, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, [])
    conf = [c for m in ms for c in m.token_confidences]
    ok = [c for m in ms for c in m.token_correct]
    return DatasetMetrics(
        dataset_name=dataset_name, num_samples=len(ms),
        wer=np.mean([m.wer for m in ms]), cer=np.mean([m.cer for m in ms]),
        mean_token_nll=np.mean([m.token_nll for m in ms]), avg_log_prob=np.mean([m.avg_log_prob for m in ms]),
        mean_token_entropy=np.mean([m.token_entropy for m in ms]), ece=compute_ece(conf, ok), per_utterance=ms,
        **corpus_rates(ms),
    )


def corpus_rates(per_utterance_metrics: List[PerUtteranceMetrics]) -> Dict[str, Optional[float]]:
    """The five corpus-level fields of DatasetMetrics: total edits over total reference length, the number papers report
    (DatasetMetrics.wer is the mean of the per-utterance rates).  corpus_wer = sum(S + D + I) / sum(H + S + D) over the word counts,
    word_sub_rate / word_del_rate / word_ins_rate = sum(S) / sum(D) / sum(I) over the same denominator, corpus_cer likewise over the
    character counts.  An utterance without counts whose reference is empty has nothing to count and stays out of the totals (the
    evaluator's empty normalised references); any other utterance without counts makes the rates None, and so does an empty total."""
    def totals(attr):
        tot = np.zeros(4, dtype=np.int64)
        for m in per_utterance_metrics:
            c = getattr(m, attr)
            if c is None:
                if m.reference.strip() == "":
                    continue
                return None
            tot += np.asarray(c, dtype=np.int64)
        return tot if tot[0] + tot[1] + tot[2] > 0 else None

    w, c = totals("word_counts"), totals("char_counts")
    out: Dict[str, Optional[float]] = dict(corpus_wer=None, corpus_cer=None, word_sub_rate=None, word_del_rate=None, word_ins_rate=None)
    if w is not None:
        n = int(w[0] + w[1] + w[2])
        out.update(corpus_wer=int(w[1] + w[2] + w[3]) / n, word_sub_rate=int(w[1]) / n, word_del_rate=int(w[2]) / n, word_ins_rate=int(w[3]) / n)
    if c is not None:
        out["corpus_cer"] = int(c[1] + c[2] + c[3]) / int(c[0] + c[1] + c[2])
    return out


def compute_macro_average(dataset_metrics: List[DatasetMetrics]) -> Dict[str, float]:
    """Unweighted mean over datasets (every dataset counts equally)."""
    keys = {"macro_wer": "wer", "macro_cer": "cer", "macro_mean_token_nll": "mean_token_nll",
            "macro_avg_log_prob": "avg_log_prob", "macro_mean_token_entropy": "mean_token_entropy", "macro_ece": "ece"}
    if not dataset_metrics:
        return {k: 0.0 for k in keys}
    return {k: np.mean([getattr(m, a) for m in dataset_metrics]) for k, a in keys.items()}
