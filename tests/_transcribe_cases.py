"""Cases, float64 references and bounds for the two kernels of csrc/transcribe.hip (wft_lang_probs, wft_mel_windows), shared by
tests/test_transcribe_host.py (which proves on the CPU that the bounds bite) and tests/test_transcribe_kernels_gpu.py.  numpy only.

The language-probability bound, derived (u = 2^-24, the unit roundoff of fp32; expf and logf of the device library are accurate
to 1 ulp, i.e. to a relative 2u).  Kernel and reference read the SAME bf16 logits x_k, k over the n language columns; with m the
maximum the kernel computes
    d_k = fl(x_k - m)       e_k = expf(d_k)       s = fl(sum e_k)       l = logf(s)       p_j = expf(fl(d_j - l)).
  1. d_k: one fp32 subtraction, |delta d_k| <= |d_k| u (exact whenever the two exponents are within 16 of each other).
  2. e_k: the error of d_k moves it by a relative |d_k| u, expf adds 2u.
  3. s: every e_k passes through at most DEPTH = 3 + 6 + 3 additions (a thread's four values, the six butterfly levels of its
     wave, the four waves), each a relative u: with (2) the relative error of s is at most (W + 2 + DEPTH) u, where
     W = sum_k q_k |d_k| is the mean of |d_k| under the exact softmax q.  (W = H(q) - log s <= log n: at most 6.94.)
  4. l: the error of s moves log(s) by that much absolutely, logf adds 2 |l| u.
  5. t = fl(d_j - l): the errors of d_j and l, plus |d_j - l| u for the subtraction; all absolute.
  6. p_j = expf(t): an absolute error of t is a relative error of p_j, expf adds 2u.
 To first order |p_j - q_j| / q_j <= (|d_j| + W + 2 + DEPTH + 2 |l| + |d_j - l| + 2) u          (2 + DEPTH + 2 = 16)
                                  =  c_j 2^-23,   c_j = (|d_j| + W + |d_j - l| + 2 |l| + 16) / 2,
 evaluated per element on the float64 reference (d, l, W are known there) and multiplied by SLACK = 1.25 for the second-order terms
 and for the reference's own float64 rounding.  For the most probable language of a peaked row c_j is about 8; it cannot exceed
 (87.4 + 6.94 + 87.4 + 13.9 + 16) / 2 = 106 for a result that is a normal fp32 number (|d_j| + l <= 126 ln 2).  Results below the
 smallest normal number 2^-126 have no relative precision in fp32 (and may be flushed to zero): the bound carries that one
 absolute term.  Nothing here was tuned on what a kernel returned.
"""
from __future__ import annotations

import numpy as np

SUM_DEPTH = 3 + 6 + 3
SLACK = 1.25
TINY = 2.0 ** -126
LP_THREADS = 256


# ----------------------------------------------------------------------------- bf16 on the host
def bf16_bits(x) -> np.ndarray:
    """float32 array -> uint16 bf16 bit patterns, round to nearest even (inf and NaN keep their class)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    r[nan] = 0x7FC0
    return r


def bf16_round(x) -> np.ndarray:
    """float32 array -> the float32 values of its bf16 rounding."""
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32)


# ----------------------------------------------------------------------------- wft_lang_probs
def lang_cases():
    """(name, V, ld, ids): the two multilingual vocabularies with their contiguous language blocks, and a small vocabulary with
    n_lang on both sides of a wave (63, 64, 65), 1 and 2, non-contiguous ids that include column 0 and column V - 1."""
    out = [("v51865-99", 51865, 51968, list(range(50259, 50358))), ("v51866-100", 51866, 51968, list(range(50259, 50359)))]
    V = 300
    for n in (1, 2, 63, 64, 65):
        if n == 1:
            ids = [V - 1]
        elif n == 2:
            ids = [0, V - 1]
        else:
            rng = np.random.default_rng(n)
            ids = sorted({0, V - 1} | set(rng.choice(np.arange(1, V - 1), size=n - 2, replace=False).tolist()))
        assert len(ids) == n
        out.append((f"v300-{n}", V, 384, ids))
    return out


LANG_KINDS = ("dominant", "equal", "tie", "extreme", "spread")
LANG_ROWS = (1, 3, 5)


def lang_logits(B: int, V: int, ld: int, ids, kind: str, seed: int = 0, poison: bool = True) -> np.ndarray:
    """f32 [B, ld] of bf16-representable values.  The language columns by `kind`:
      dominant  N(0, 1) with one column (another in every row) 12 above
      equal     one value everywhere: every language ties, the first id wins
      tie       N(0, 1) with the first and the last id planted 6 above, equal: the first wins
      extreme   values near +80 and -80 (alternating, jittered), so that exp(x) without the maximum subtracted loses its precision
      spread    N(0, 8): probabilities over many orders of magnitude
    poison: every other column < V holds +inf or NaN (alternating), every column >= V likewise — they must not be read or must
    not matter.  Without poison those columns hold N(2, 3) noise, so a softmax over all V columns is visibly another one."""
    rng = np.random.default_rng(1000 * seed + 17 * B + len(ids) + LANG_KINDS.index(kind))
    n = len(ids)
    x = rng.normal(2.0, 3.0, size=(B, ld)).astype(np.float32)
    if poison:
        x[:, 0::2] = np.inf
        x[:, 1::2] = np.nan
    lang = rng.normal(0.0, 1.0, size=(B, n)).astype(np.float32)
    if kind == "dominant":
        for b in range(B):
            lang[b, (7 * b + n // 2) % n] += 12.0
    elif kind == "equal":
        lang[:] = 1.375
    elif kind == "tie":
        lang[:, 0] = lang[:, -1] = 6.0
    elif kind == "extreme":
        sign = np.where(np.arange(n)[None, :] % 2 == 0, 1.0, -1.0)
        lang = (sign * 80.0 + rng.normal(0.0, 0.5, size=(B, n))).astype(np.float32)
    elif kind == "spread":
        lang = rng.normal(0.0, 8.0, size=(B, n)).astype(np.float32)
    else:
        raise ValueError(kind)
    x[:, ids] = lang
    return bf16_round(x)


def lang_reference(x: np.ndarray, V: int, ids):
    """float64 softmax over the language columns -> (probs f64 [B, n], best i64 [B] — the lowest id at the maximum —,
    tol f64 [B, n]: the derived bound, per element)."""
    g = x[:, ids].astype(np.float64)
    m = g.max(axis=1, keepdims=True)
    d = g - m
    e = np.exp(d)
    s = e.sum(axis=1, keepdims=True)
    l = np.log(s)
    q = e / s
    W = (q * np.abs(d)).sum(axis=1, keepdims=True)
    c = (np.abs(d) + W + np.abs(d - l) + 2 * np.abs(l) + 2 + SUM_DEPTH + 2) / 2
    best = np.asarray(ids, dtype=np.int64)[np.argmax(g == m, axis=1)]
    return q, best, SLACK * c * 2.0 ** -23 * q + TINY


def lang_check(probs, best, x: np.ndarray, V: int, ids, what: str = "") -> float:
    """Assert probs within the derived bound of float64 and best exact -> the worst |err| / tol."""
    q, b, tol = lang_reference(x, V, ids)
    probs = np.asarray(probs, dtype=np.float64)
    assert probs.shape == q.shape, f"{what}: probs {probs.shape}, expected {q.shape}"
    assert np.array_equal(np.asarray(best, dtype=np.int64), b), f"{what}: best {np.asarray(best).tolist()} != {b.tolist()}"
    assert np.isfinite(probs).all(), f"{what}: non-finite probabilities"
    ratio = np.abs(probs - q) / tol
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: |p - ref| is {worst:.2f} x the bound at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst


LANG_MUTANTS = ("softmax over all V columns", "highest index on ties", "no maximum subtraction", "row stride V instead of ld",
                "last language id left out")


def lang_restate(x: np.ndarray, V: int, ids, mutant: str | None = None):
    """wft_lang_probs in numpy float32, in the kernel's order of operations, reading the flat buffer with the row stride ld
    -> (probs f32 [B, n], best i64 [B])."""
    assert mutant is None or mutant in LANG_MUTANTS, mutant
    B, ld = x.shape
    flat = x.reshape(-1)
    stride = V if mutant == "row stride V instead of ld" else ld
    ids = list(ids)
    n = len(ids)
    cols = list(range(V)) if mutant == "softmax over all V columns" else (ids[:-1] if mutant == "last language id left out" and n > 1 else ids)
    probs = np.zeros((B, n), dtype=np.float32)
    best = np.zeros(B, dtype=np.int64)
    f32 = np.float32
    with np.errstate(all="ignore"):
        for b in range(B):
            g = flat[b * stride + np.asarray(cols)].astype(f32)
            mx = g.max()
            at = np.nonzero(g == mx)[0]
            j = int(at[-1] if mutant == "highest index on ties" else at[0]) if at.size else 0
            best[b] = cols[j]
            m = f32(0.0) if mutant == "no maximum subtraction" else mx
            d = (g - m).astype(f32)
            e = np.exp(d).astype(f32)
            # the kernel's sum: thread t holds columns t, t + 256, ...; its values in order, the xor butterfly of its wave, the waves in order
            pad = np.zeros(LP_THREADS * ((len(cols) + LP_THREADS - 1) // LP_THREADS), dtype=f32)
            pad[:len(cols)] = e
            part = np.zeros(LP_THREADS, dtype=f32)
            for row in pad.reshape(-1, LP_THREADS):
                part = (part + row).astype(f32)
            v = part.reshape(LP_THREADS // 64, 64)
            lane = np.arange(64)
            for o in (32, 16, 8, 4, 2, 1):
                v = (v + v[:, lane ^ o]).astype(f32)
            total = f32(0.0)
            for w in range(v.shape[0]):
                total = f32(total + v[w, 0])
            lg = np.log(total).astype(f32)
            mine = flat[b * stride + np.asarray(ids)].astype(f32)
            p = np.exp(((mine - m).astype(f32) - lg).astype(f32)).astype(f32)
            if mutant == "last language id left out" and n > 1:
                p[-1] = 0.0
            probs[b] = p
    return probs, best


# ----------------------------------------------------------------------------- wft_mel_windows
N_WIN = 3000
MEL_CONTENT = (4700, 3001, 7)
MEL_ROWS = (  # (recording, seek): not in index order, several rows per recording
    (2, 0), (0, 1233), (1, 1), (0, 0), (0, 1700), (1, 2), (0, 1701), (2, 6), (0, 4699), (1, 3000), (1, 0), (2, 3), (0, 1233),
)


def mel_case(n_mels: int, seed: int = 0):
    """Three recordings of content_frames 4 700, 3 001 and 7 (ld_frames = 3 000 more), packed with ODD mel_off and gaps between
    them.  Every source element at or behind a recording's content_frames — the trailing 30 s, what upstream's zero pad must NOT
    copy — and every gap element is NaN; the content is finite noise.
    -> dict(mel f32 1-D, off, ld, cf (lists), rows, seeks, n_mels).  The rows cover seek 0, an odd seek (1 233), content - 3000
    (exactly full), content - 2999, content - 1 (one valid frame), the 7-frame recording at 0 / 3 / 6, and a repeated row."""
    rng = np.random.default_rng(seed + n_mels)
    lds = [c + N_WIN for c in MEL_CONTENT]
    offs, at = [], 1
    for ld in lds:
        offs.append(at)
        at += n_mels * ld + 2
        at += 1 - at % 2  # the next offset is odd again
    mel = np.full(at + 5, np.nan, dtype=np.float32)
    for off, ld, cf in zip(offs, lds, MEL_CONTENT):
        rec = np.full((n_mels, ld), np.nan, dtype=np.float32)
        rec[:, :cf] = rng.normal(0.0, 1.0, size=(n_mels, cf)).astype(np.float32)
        mel[off:off + n_mels * ld] = rec.reshape(-1)
    # every source alignment (element address mod 4) occurs among the rows
    assert all(o % 2 == 1 for o in offs) and {(offs[a] + m * lds[a] + s) % 4 for a, s in MEL_ROWS for m in (0, 1)} == {0, 1, 2, 3}
    return dict(mel=mel, off=offs, ld=lds, cf=list(MEL_CONTENT), rows=[a for a, _ in MEL_ROWS], seeks=[s for _, s in MEL_ROWS], n_mels=n_mels)


def mel_expected(case) -> np.ndarray:
    """The reference: slice every recording's [n_mels, ld] view, zero-fill behind the content -> f32 [R, n_mels, N_WIN]."""
    n_mels = case["n_mels"]
    out = np.zeros((len(case["rows"]), n_mels, N_WIN), dtype=np.float32)
    for r, (a, sk) in enumerate(zip(case["rows"], case["seeks"])):
        rec = case["mel"][case["off"][a]:case["off"][a] + n_mels * case["ld"][a]].reshape(n_mels, case["ld"][a])
        piece = rec[:, sk:min(sk + N_WIN, case["cf"][a])]
        out[r, :, :piece.shape[1]] = piece
    return out


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


MEL_MUTANTS = ("pad with the source's own values", "valid length off by one", "seek of row 0 for every row", "mel_off ignored")


def mel_restate(case, mutant: str | None = None) -> np.ndarray:
    """wft_mel_windows in numpy, by the kernel's index arithmetic (element address = mel_off + m * ld + seek + t, a select against
    the valid length, clamped so that nothing outside the recording is addressed)."""
    assert mutant is None or mutant in MEL_MUTANTS, mutant
    n_mels, mel = case["n_mels"], case["mel"]
    R = len(case["rows"])
    out = np.empty((R, n_mels, N_WIN), dtype=np.float32)
    t = np.arange(N_WIN)
    for r in range(R):
        a = min(max(case["rows"][r], 0), len(case["off"]) - 1)
        ld = case["ld"][a]
        cf = min(max(case["cf"][a], 0), ld)
        sk = min(max(case["seeks"][0 if mutant == "seek of row 0 for every row" else r], 0), cf)
        limit = min(N_WIN, cf - sk) + (1 if mutant == "valid length off by one" else 0)
        off = 0 if mutant == "mel_off ignored" else case["off"][a]
        for m in range(n_mels):
            idx = np.clip(m * ld + sk + t, 0, n_mels * ld - 1)
            src = mel[off + idx]
            out[r, m] = src if mutant == "pad with the source's own values" else np.where(t < limit, src, np.float32(0.0))
    return out
