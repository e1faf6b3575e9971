"""Oracle for the word-level alignment kernels (csrc/align.hip, include/wft.h "Word-level alignment"): an fp64 restatement of the
softmax over n_key, the standardisation, the reflect-padded median and the head mean; the serial fp32 dynamic time warping with
upstream's comparison order and backtrace (swept by anti-diagonals: every cell is one fp32 add of the same two operands as in the
double loop, so the bits cannot differ — tests/test_align_host.py checks it against the literal loop); the jumps / words
arithmetic; fp32 restatements with switchable defects ("mutants"); and the per-element bounds.  CPU only, torch + numpy; shared by
tests/test_align_host.py (the bounds pass the correct fp32 restatement and fail every mutant) and the two GPU test files.

Bounds (u = 2^-24, the unit roundoff of fp32; nothing here comes from a kernel's output).

Probabilities.  x_j = fl(acc_j * alpha) in log2 units, alpha = fl(scale * log2 e), acc_j the MFMA sum of 64 bf16 products with fp32
accumulation.  A product of two bf16 values is exact in fp32 (8 + 8 significand bits); 64 of them summed in fp32 in any order and
with any rounding direction are off by at most 64 * 2u * A_j, A_j = sum_d |q_d k_d|.  The multiply by alpha and alpha's own
rounding add 2u |x_j| (taken as 4u), the subtraction of the row maximum u |x_j - m|, and the running-sum rescales exp2(m_old - m_new)
telescope to at most 2u R, R = the row's score range.  In natural-log units a row's score error is therefore at most
  delta(b, h, t) = ln 2 * max_j [alpha * 128 u * A_j + 4u |x_j| + 3u R],
every exp2 carries the hardware's relative error (v_exp_f32: 1 ulp, taken as 2u each for numerator and denominator), and the
sum of at most 1500 terms runs as chains of at most 12 adds per lane, 5 shuffle steps and 4 waves, each add and each rescale
product one rounding: 48 roundings of 2u cover them with the final reciprocal and product.  Numerator and denominator each move
by a factor inside e^{+-delta}, so
  |p - p_ref| <= p_ref * (e^{2 delta} - 1 + 100 u) + 2^-120,
the last term for results the hardware exp2 flushes to zero.

Matrix.  Median and mean are 1-Lipschitz in the sup norm, so the error of an output element is at most the largest
standardisation error inside its window, over the heads, plus the head mean's own rounding.  For a column with n rows, exact fp32
inputs p >= 0, mean mu and biased deviation sigma: the fp32 mean is off by at most d_mu = (n + 1) u mu (n - 1 adds in any order
and a division); a shifted mean changes the deviation by at most d_mu, and the n squares, n - 1 adds, the division and the square
root by a relative (n + 4) u; the difference p - mu-hat by d_mu + u |p - mu|; the final division by u.  With z = (p - mu) / sigma:
  eps_z = d_mu / sigma + |z| * (d_mu / sigma + (n + 8) u),
and the head mean adds (n_sel + 1) u * max |z| of the window.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
LOG2E = 1.4426950408889634
HD = 64
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ probabilities
def head_view(t, H):
    """[B, T, H * 64] (any strides) -> fp64 [B, H, T, 64]"""
    B, T, _ = t.shape
    return t.to(F64).reshape(B, T, H, HD).permute(0, 2, 1, 3)


def scores_ref(q, k, heads, scale):
    """bf16 q [B, Tq, H * 64], k [B, Tk, H * 64] -> fp64 natural-log scores [B, n, Tq, Tk] of the listed heads, and
    A = sum_d |q_d k_d| of the same shape."""
    H = q.shape[2] // HD
    qh, kh = head_view(q, H)[:, list(heads)], head_view(k, H)[:, list(heads)]
    return scale * qh @ kh.transpose(-1, -2), qh.abs() @ kh.abs().transpose(-1, -2)


def probs_ref(q, k, heads, n_tok, n_key, scale):
    """fp64 softmax over the first n_key[b] keys for the first n_tok[b] rows; 0 elsewhere -> [B, n, Tq, Tk]"""
    s, _ = scores_ref(q, k, heads, scale)
    out = torch.zeros_like(s)
    for b in range(s.shape[0]):
        nt, nk = n_tok[b], n_key[b]
        if nt and nk:
            out[b, :, :nt, :nk] = torch.softmax(s[b, :, :nt, :nk], dim=-1)
    return out


def probs_bound(q, k, heads, n_tok, n_key, scale, p_ref):
    """The per-element bound of the module docstring, fp64 [B, n, Tq, Tk] (0 where nothing is written)."""
    s, A = scores_ref(q, k, heads, scale)
    alpha = scale * LOG2E
    out = torch.zeros_like(s)
    for b in range(s.shape[0]):
        nt, nk = n_tok[b], n_key[b]
        if not (nt and nk):
            continue
        x = s[b, :, :nt, :nk] * LOG2E
        R = x.amax(-1, keepdim=True) - x.amin(-1, keepdim=True)
        delta = math.log(2.0) * (alpha * 128 * U * A[b, :, :nt, :nk] + 4 * U * x.abs() + 3 * U * R).amax(-1, keepdim=True)
        out[b, :, :nt, :nk] = p_ref[b, :, :nt, :nk] * (torch.expm1(2 * delta) + 100 * U) + 2.0 ** -120
    return out


def probs_f32(q, k, heads, n_tok, n_key, scale, mutant=None):
    """An fp32 torch restatement of stage a (bf16 operands widened to fp32, fp32 matmul and softmax) -> f32 [B, n, Tq, Tk].
    mutant: "drop_last_key" (the softmax runs over n_key - 1 keys), "leak_key" (over n_key + 1, where the buffer has one),
    "sorted_heads" (the head list is read in ascending order)."""
    H = q.shape[2] // HD
    hs = sorted(heads) if mutant == "sorted_heads" else list(heads)
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    qh = q.float().reshape(B, Tq, H, HD).permute(0, 2, 1, 3)[:, hs]
    kh = k.float().reshape(B, Tk, H, HD).permute(0, 2, 1, 3)[:, hs]
    s = (qh @ kh.transpose(-1, -2)) * np.float32(scale)
    out = torch.zeros_like(s)
    for b in range(B):
        nt, nk = n_tok[b], n_key[b]
        if not (nt and nk):
            continue
        m = nk - 1 if (mutant == "drop_last_key" and nk > 1) else min(nk + 1, Tk) if mutant == "leak_key" else nk
        p = torch.softmax(s[b, :, :nt, :m], dim=-1)
        w = min(m, nk)
        out[b, :, :nt, :w] = p[..., :w]
    return out


def probs_case(Tq, n_tok, n_key, seed=0, B=3, H=6, Tk=1500):
    """The GPU test's operands: q a [B, Tq, H * 64] buffer, k the first half of a [B, Tk, 2 * H * 64] kv buffer, bf16, drawn so that
    the natural-log scores have a standard deviation of about 2 (rows neither flat nor one-hot) -> dict."""
    g = torch.Generator().manual_seed(1000 + seed)
    D = H * HD
    qbuf = (torch.randn(B, Tq, D, generator=g) * math.sqrt(2.0)).to(torch.bfloat16)
    kv = (torch.randn(B, Tk, 2 * D, generator=g) * math.sqrt(2.0)).to(torch.bfloat16)
    return dict(qbuf=qbuf, kv=kv, q=qbuf, k=kv[..., :D], H=H, heads=[5, 0, 3], n_tok=list(n_tok), n_key=list(n_key),
                scale=0.125)


PROBS_CASES = [  # (Tq, n_tok, n_key): every Tq with the tile edges of the key axis (1500 = 46 * 32 + 28, 1499, 750, 65 = 2 * 32 + 1, 1)
    (1, (1, 1, 1), (1500, 65, 1)),
    (5, (5, 3, 1), (1499, 750, 1)),
    (33, (33, 17, 32), (1500, 1499, 750)),
    (33, (1, 33, 31), (65, 1, 1500)),
]


# ------------------------------------------------------------------------------------------------ matrix
def _reflect_windows(z, width):
    """z [..., n] -> [..., n, width]: the windows of the reflect-padded last axis (n > width // 2)"""
    hw = width // 2
    n = z.shape[-1]
    idx = torch.arange(-hw, n + hw).abs()
    idx = torch.where(idx >= n, 2 * (n - 1) - idx, idx)
    return z[..., idx].unfold(-1, width, 1)


def matrix_ref(probs, n_tok, n_key, width=7):
    """fp64: standardise over the n_tok[b] rows (biased deviation), median over reflect-padded windows of `width` frames (skipped
    where n_key[b] <= width // 2), mean over the heads -> (matrix [B, Tq, Tk], bound [B, Tq, Tk]); 0 where nothing is written."""
    B, S, Tq, Tk = probs.shape
    out = torch.zeros(B, Tq, Tk, dtype=F64)
    bound = torch.zeros(B, Tq, Tk, dtype=F64)
    for b in range(B):
        nt, nk = n_tok[b], n_key[b]
        if not (nt and nk):
            continue
        p = probs[b, :, :nt, :nk].to(F64)
        mu = p.mean(-2, keepdim=True)
        sd = (p - mu).pow(2).mean(-2, keepdim=True).sqrt()
        z = (p - mu) / sd
        d_mu = (nt + 1) * U * mu
        eps = d_mu / sd + z.abs() * (d_mu / sd + (nt + 8) * U)
        if nk > width // 2:
            zw, ew = _reflect_windows(z, width), _reflect_windows(eps, width)
            med = zw.sort(-1)[0][..., width // 2]
            e, za = ew.amax(-1), zw.abs().amax(-1)
        else:
            med, e, za = z, eps, z.abs()
        out[b, :nt, :nk] = med.mean(0)
        bound[b, :nt, :nk] = e.amax(0) + (S + 1) * U * za.amax(0)
    return out, bound


def matrix_f32(probs, n_tok, n_key, width=7, mutant=None):
    """An fp32 torch restatement of stage b -> f32 [B, Tq, Tk].  mutant: "unbiased" (the deviation divides by n - 1), "zero_pad"
    (padding by zeros instead of reflection), "width5", "padded_rows" (the statistics run over all Tq rows), "drop_last_head"."""
    B, S, Tq, Tk = probs.shape
    out = torch.zeros(B, Tq, Tk, dtype=torch.float32)
    if mutant == "width5":
        width = 5
    hw = width // 2
    for b in range(B):
        nt, nk = n_tok[b], n_key[b]
        if not (nt and nk):
            continue
        rows = Tq if mutant == "padded_rows" else nt
        p = probs[b, :, :rows, :nk].float()
        sd, mu = torch.std_mean(p, dim=-2, keepdim=True, unbiased=(mutant == "unbiased" and rows > 1))
        z = ((p - mu) / sd)[:, :nt]
        if nk > hw:
            if mutant == "zero_pad":
                zw = torch.nn.functional.pad(z, (hw, hw)).unfold(-1, width, 1)
            else:
                zw = _reflect_windows(z, width)
            z = zw.sort(-1)[0][..., hw]
        if mutant == "drop_last_head" and S > 1:
            z = z[:-1]
        out[b, :nt, :nk] = z.mean(0)
    return out


def crafted_probs(B, S, Tq, Tk, n_key, seed=0):
    """f32 [B, S, Tq, Tk]: every row a softmax of N(0, 2^2) scores over the audio's n_key[b] keys, 0 behind them — ALL Tq rows are
    filled (rows at or beyond n_tok are what a kernel that ignores n_tok would read)."""
    g = torch.Generator().manual_seed(2000 + seed)
    out = torch.zeros(B, S, Tq, Tk, dtype=torch.float32)
    for b in range(B):
        out[b, ..., :n_key[b]] = torch.softmax(torch.randn(S, Tq, n_key[b], generator=g) * 2.0, dim=-1)
    return out


MATRIX_TOK = (2, 7, 448)                                 # n_tok of the three audios of every matrix case
MATRIX_KEYS = [(3, 4, 7), (65, 1500, 4), (1500, 3, 65)]  # n_key: 3 skips the filter, 4 is the smallest size that reflects
MATRIX_SEL = (1, 3)


# ------------------------------------------------------------------------------------------------ dynamic time warping
def dtw_ref(x):
    """x: float32 [N, M] cost -> (text_indices, time_indices) int64, forward order: upstream's `dtw_cpu` recurrence in fp32 (diagonal
    if strictly below both others, else vertical if strictly below both others, else horizontal) and its `backtrace`, the cost
    table filled by anti-diagonals."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.full((N + 1, M + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    for s in range(2, N + M + 1):
        i = np.arange(max(1, s - M), min(N, s - 1) + 1)
        j = s - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2)).astype(np.int8)
        c = np.where(t == 0, c0, np.where(t == 1, c1, c2))
        cost[i, j] = x[i - 1, j - 1] + c
        trace[i, j] = t
    return backtrace(trace)


def backtrace(trace):
    """upstream's `backtrace`: from the last cell to (0, 0), the borders forced to "left" (row 0) and "up" (column 0)"""
    i, j = trace.shape[0] - 1, trace.shape[1] - 1
    trace = trace.copy()
    trace[0, :] = 2
    trace[:, 0] = 1
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        elif t == 2:
            j -= 1
        else:
            raise ValueError("unexpected trace value")
    return np.array(text[::-1], dtype=np.int64), np.array(time[::-1], dtype=np.int64)


def dtw_matrix(N, M, kind="randn", seed=0):
    """float32 [N, M]: "randn"; "ints" (values in {-1, 0, 1}: exact ties everywhere); "equal" (all 0: every comparison of
    the recurrence is a tie)"""
    g = np.random.default_rng(3000 + seed)
    if kind == "randn":
        return g.standard_normal((N, M)).astype(np.float32)
    if kind == "ints":
        return g.integers(-1, 2, size=(N, M)).astype(np.float32)
    return np.zeros((N, M), dtype=np.float32)


DTW_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 3), (63, 65), (64, 64), (65, 1500), (445, 1500)]
DTW_TIE_CASES = [(5, 7, "equal"), (7, 5, "equal"), (6, 9, "ints"), (9, 6, "ints"), (1, 4, "ints"), (4, 1, "equal")]


# ------------------------------------------------------------------------------------------------ jumps and words
def words_ref(path_text, path_time, counts, token_probs, text):
    """Upstream's arithmetic behind the path, in plain loops.  A "jump" is a path entry whose text index differs from the one before
    it (the first entry is one); jump k's time is its frame / 50.  Word w covers tokens bounds[w] .. bounds[w + 1] - 1 of
    [text..., eot] with bounds the running sum of `counts` without the last word (the eot): it starts at jump bounds[w] and ends at
    jump bounds[w + 1]; its probability is the mean of its tokens' probabilities."""
    if len(counts) <= 1:
        return []
    jump_times, last = [], None
    for ti, tj in zip(path_text, path_time):
        if last is None or ti != last:
            jump_times.append(int(tj) / 50.0)
        last = ti
    words, at = [], 0
    for c in counts[:-1]:
        probs = [float(v) for v in token_probs[at:at + c]]
        words.append((jump_times[at], jump_times[at + c], sum(probs) / len(probs), [int(t) for t in text[at:at + c]]))
        at += c
    return words
