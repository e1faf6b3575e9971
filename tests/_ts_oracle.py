"""Test helper: the timestamp rules of include/wft.h "Timestamp rules" (upstream whisper's ApplyTimestampRules, restated) as plain
slice assignments on one fp64 row, in the order the header lists them.  Imports nothing from the engine.

  rules(row, ...)  -> Ruled: the fp64 row with every removed column at -inf, its log-softmax, whether rule 5 fired and its margin
  pick(row, ...)   -> (column, log-probability): the arg-max of what is left, the lowest column on ties; nothing left: (eot, 0.0)
  topk(row, k, ..) -> k x (column, log-probability), descending, ties to the lower column, padded with (-1, -inf)

`row`: the logits the kernel reads (bf16 values), any float dtype; `sampled`: the row's sampled tokens tokens[first_len:len];
`dead`: the statically suppressed columns of this step (suppress, and suppress_first while nothing is sampled)."""
from dataclasses import dataclass

import numpy as np
import torch

NEG = float("-inf")


@dataclass
class Ruled:
    x: torch.Tensor        # fp64 [V], removed columns -inf
    logp: torch.Tensor     # fp64 [V], log-softmax of x (all -inf when nothing is live)
    ts_wins: bool          # rule 5 removed the text columns
    margin: float          # logsumexp(live timestamps) - max(live text), before rule 5 (+-inf when a side is empty, nan when both)


def rules(row, sampled, *, ts_begin, eot, no_timestamps=None, max_initial=None, dead=()):
    x = torch.as_tensor(row).detach().to(torch.float64).clone()
    V = x.shape[0]
    sampled = [int(t) for t in sampled]
    assert eot < ts_begin < V
    dead = [int(t) for t in dead]
    if dead:
        x[dead] = NEG
    # 1
    if no_timestamps is not None and no_timestamps >= 0:
        x[no_timestamps] = NEG
    # 2
    last_ts = len(sampled) >= 1 and sampled[-1] >= ts_begin
    pen_ts = len(sampled) < 2 or sampled[-2] >= ts_begin
    if last_ts:
        if pen_ts:
            x[ts_begin:] = NEG
        else:
            x[:eot] = NEG
    # 3
    stamps = [t for t in sampled if t >= ts_begin]
    if stamps:
        t = stamps[-1]
        x[ts_begin:(t if last_ts and not pen_ts else t + 1)] = NEG
    # 4
    if not sampled:
        x[:ts_begin] = NEG
        if max_initial is not None and max_initial >= 0:
            x[ts_begin + max_initial + 1:] = NEG
    # 5 (both sides under the same softmax: the normaliser cancels)
    lse_ts = torch.logsumexp(x[ts_begin:], 0).item() if torch.isfinite(x[ts_begin:]).any() else NEG
    max_text = x[:ts_begin].max().item()
    margin = lse_ts - max_text if not (lse_ts == NEG and max_text == NEG) else float("nan")
    ts_wins = lse_ts > max_text
    if ts_wins:
        x[:ts_begin] = NEG
    logp = torch.log_softmax(x, 0) if torch.isfinite(x).any() else torch.full_like(x, NEG)
    return Ruled(x, logp, bool(ts_wins), margin)


def pick(row, sampled, *, eot, **kw):
    r = rules(row, sampled, eot=eot, **kw)
    if not torch.isfinite(r.x).any():
        return eot, 0.0, r
    col = int(r.x.argmax())  # (torch.argmax on the CPU returns the first maximum; asserted below all the same)
    assert col == int((r.x == r.x.max()).nonzero()[0])
    return col, r.logp[col].item(), r


def topk_of(r: Ruled, k):
    """The k best of an already ruled row.  Every column at or above the k-th largest value is a candidate (all its ties included),
    sorted by value descending, then the lower column."""
    n_live = int(torch.isfinite(r.x).sum())
    out = []
    if n_live:
        kth = torch.topk(r.x, min(k, n_live)).values[-1]
        cols = (r.x >= kth).nonzero().flatten().numpy()
        vals = r.x[cols].numpy()
        order = cols[np.lexsort((cols, -vals))][:k]
        out = [(int(c), r.logp[int(c)].item()) for c in order]
    return out + [(-1, NEG)] * (k - len(out))


def topk(row, k, sampled, **kw):
    r = rules(row, sampled, **kw)
    return topk_of(r, k), r


def check_structure(sampled, *, ts_begin, eot, max_initial=None):
    """What every sequence decoded under the rules satisfies (eot and what follows it cut off): it starts with a timestamp <=
    max_initial; timestamps never decrease; text never follows directly a lone closing timestamp (text, ts, text: the closing
    timestamp must be followed by the opening one of the next segment, or by eot; "text" here: a column below eot, the range
    rule 2 removes).  -> None, or a message."""
    s = [int(t) for t in sampled]
    if eot in s:
        s = s[:s.index(eot)]
    if not s:
        return None
    if s[0] < ts_begin:
        return f"starts with text {s[0]}"
    if max_initial is not None and s[0] - ts_begin > max_initial:
        return f"first timestamp {s[0] - ts_begin} > max_initial {max_initial}"
    stamps = [t for t in s if t >= ts_begin]
    if any(b < a for a, b in zip(stamps, stamps[1:])):
        return "timestamps decrease"
    for i in range(2, len(s)):
        if s[i] < eot and s[i - 1] >= ts_begin and s[i - 2] < ts_begin:
            return f"text at {i} directly after a lone closing timestamp"
    for i in range(2, len(s)):
        if s[i] >= ts_begin and s[i - 1] >= ts_begin and s[i - 2] >= ts_begin:
            return f"three timestamps in a row at {i}"
    return None
