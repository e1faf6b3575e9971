"""Test helper: the sampled pick of include/wft.h "Sampled decoding" in numpy / fp64.  Imports nothing from the engine.

  philox4x32_10(counter, key)  -> the 4 output words of Philox4x32-10 (Salmon et al. 2011), vectorised over leading axes
  uniforms(seed, pos, cols)    -> v = (2k + 1) * 2^-24 per column, k = the top 23 bits of word col & 3 of the block at counter
                                  (col >> 2, pos, 0, 0) under key (seed low, seed high); fp64 values that are exact in fp32
  gumbel(seed, pos, cols)      -> g = -log(-log(v)) in fp64
  live_row(row, ...)           -> the fp64 row with every removed column at -inf: the static masks, then tests/_ts_oracle.py's rules
  pick(x_live, t, seed, pos, eot) -> Pick(col, logp, gap): arg-max of x / t + g over the live columns (lowest column on ties; a -inf
                                  logit never wins), its log-softmax at temperature 1, and the gap between the two largest keys;
                                  t <= 0: the arg-max of x itself (gap: between the two largest logits); nothing live: (eot, 0, inf)
  gumbel_rows / pick_rows      -> the same for many rows that share one logits row (the distribution test)
  counts / chi_square          -> the distribution test's helpers"""
from dataclasses import dataclass

import numpy as np
import torch

from tests import _ts_oracle as TO

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
NEG = float("-inf")


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (anything that casts to uint32 words) -> uint32 [..., 4]."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & MASK for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed: int, pos: int, cols) -> np.ndarray:
    """The 32-bit word of every column: block (col >> 2, pos, 0, 0), word col & 3, key = the seed's halves."""
    cols = np.asarray(cols, dtype=np.int64)
    seed = int(seed) % (1 << 64)
    blocks = np.unique(cols >> 2)
    ctr = np.zeros((len(blocks), 4), dtype=np.uint64)
    ctr[:, 0] = blocks
    ctr[:, 1] = int(pos) & 0xFFFFFFFF
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (len(blocks), 2))
    out = philox4x32_10(ctr, key)
    return out[np.searchsorted(blocks, cols >> 2), cols & 3]


def uniforms(seed: int, pos: int, cols) -> np.ndarray:
    k = (words(seed, pos, cols) >> np.uint32(9)).astype(np.float64)
    return (2.0 * k + 1.0) * 2.0 ** -24


def gumbel(seed: int, pos: int, cols) -> np.ndarray:
    return -np.log(-np.log(uniforms(seed, pos, cols)))


def live_row(row, sampled=(), *, eot, dead=(), ts_begin=None, no_timestamps=None, max_initial=None) -> np.ndarray:
    """fp64 [V]: removed columns at -inf.  ts_begin None: the static masks alone; otherwise the timestamp rules on top (rule 5 is
    decided on this untempered row)."""
    if ts_begin is None:
        x = torch.as_tensor(row).detach().to(torch.float64).clone()
        dead = [int(t) for t in dead]
        if dead:
            x[dead] = NEG
        return x.numpy()
    return TO.rules(row, sampled, ts_begin=ts_begin, eot=eot, no_timestamps=no_timestamps, max_initial=max_initial, dead=dead).x.numpy()


@dataclass
class Pick:
    col: int
    logp: float
    gap: float   # the largest key minus the second largest (inf with fewer than two finite keys)


def _top_two(v: np.ndarray):
    """(lowest index of the maximum, max - second largest) of the finite entries."""
    col = int(np.argmax(v))  # (numpy: the first maximum)
    rest = np.delete(v, col)
    rest = rest[np.isfinite(rest)]
    return col, (float(v[col] - rest.max()) if rest.size else float("inf"))


def pick(x_live, t: float, seed: int, pos: int, eot: int) -> Pick:
    x = np.asarray(x_live, dtype=np.float64)
    live = np.isfinite(x) | (x == np.inf)
    if not live.any():
        return Pick(int(eot), 0.0, float("inf"))
    m = x[live].max()
    lse = m + np.log(np.exp(x[live] - m).sum())
    if t <= 0:
        col, gap = _top_two(np.where(live, x, NEG))
        return Pick(col, float(x[col] - lse), gap)
    cols = np.nonzero(live)[0]
    # the kernel's key: the fp32 reciprocal of the fp32 temperature times the logit, plus the noise (in fp64 here)
    inv_t = float(np.float32(1.0) / np.float32(t))
    key = np.full(x.shape, NEG)
    key[cols] = x[cols] * inv_t + gumbel(seed, pos, cols)
    col, gap = _top_two(key)
    return Pick(col, float(x[col] - lse), gap)


def gumbel_rows(seeds, pos, V: int) -> np.ndarray:
    """fp64 [R, V]: the noise of R rows at once (seeds [R]; pos an int or [R]) — the vectorised form of gumbel()."""
    seeds = [int(s) % (1 << 64) for s in seeds]
    R, nb = len(seeds), (V + 3) // 4
    ctr = np.zeros((R, nb, 4), dtype=np.uint64)
    ctr[:, :, 0] = np.arange(nb)
    ctr[:, :, 1] = (np.broadcast_to(np.asarray(pos, dtype=np.int64), (R,)) & 0xFFFFFFFF)[:, None]
    key = np.zeros((R, nb, 2), dtype=np.uint64)
    key[:, :, 0] = np.array([s & 0xFFFFFFFF for s in seeds], dtype=np.uint64)[:, None]
    key[:, :, 1] = np.array([s >> 32 for s in seeds], dtype=np.uint64)[:, None]
    k = (philox4x32_10(ctr, key).reshape(R, nb * 4)[:, :V] >> np.uint32(9)).astype(np.float64)
    return -np.log(-np.log((2.0 * k + 1.0) * 2.0 ** -24))


def pick_rows(x_live, t: float, seeds, pos):
    """R draws from ONE live row (fp64 [V], at least two finite columns) at temperature t > 0 -> (columns [R], key gaps [R])."""
    x = np.asarray(x_live, dtype=np.float64)
    key = x[None, :] * float(np.float32(1.0) / np.float32(t)) + gumbel_rows(seeds, pos, x.shape[0])
    key[:, ~np.isfinite(x)] = NEG
    top = np.sort(key, axis=1)[:, -2:]
    return np.argmax(key, axis=1), top[:, 1] - top[:, 0]


def counts(picks, V: int) -> np.ndarray:
    return np.bincount(np.asarray(picks, dtype=np.int64), minlength=V)[:V]


def chi_square(observed, probs, min_expected: float = 5.0):
    """Pearson's statistic of the counts against n * probs, cells with an expectation below `min_expected` pooled into one
    -> (statistic, degrees of freedom)."""
    observed = np.asarray(observed, dtype=np.float64)
    expected = np.asarray(probs, dtype=np.float64) * observed.sum()
    small = expected < min_expected
    o, e = list(observed[~small]), list(expected[~small])
    if small.any():
        o.append(observed[small].sum()); e.append(expected[small].sum())
    o, e = np.array(o), np.array(e)
    return float(((o - e) ** 2 / e).sum()), len(o) - 1
