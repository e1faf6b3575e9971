"""Reference, error bound, cases and mutants for the resampler (csrc/audio.hip wft_resample_f32; data/gpu_frontend.py resample_taps).

The reference is written from the definition (include/wft.h "wft_resample_f32"), in float64, with its own g and its own index
arithmetic; it imports nothing from the product.  With o = orig / gcd, n = new / gcd, base = 0.99 * min(o, n), width = ceil(6 o / base):
  g(t) = (base / o) * sinc(pi t) * cos^2(pi t / 12) for |t| < 6, exactly 0 otherwise
  out[m] = sum_j x[j] * g((j / o - m / n) * base),  0 <= m < n_out = ceil(n_in * n / o),  x[j] = 0 outside [0, n_in).
`definition` is that direct sum (over every j that can lie inside |t| < 6, two more on each side than the polyphase window);
`weights` are the polyphase weights taps[r][k + width - 1] = g((k - r / n) * base / o), m * o = j0 * n + r, j = j0 + k.

The bound.  A device output is one f32 sum of 2 * width products of f32 numbers.  For ANY order of the additions, fused or not,
  |fl(sum) - sum| <= gamma_N * sum_k |taps32 * x|,   gamma_N = N u / (1 - N u),  u = 2^-24,  N = 2 * width terms
(Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5; a fused multiply-add only removes roundings).  The tests use
(2 * width + 1) * 2^-24 >= gamma_{2 width} for every width here (N u < 1e-5), against `ref` = the float64 sum over the SAME f32 table,
so an element whose bound is 0 (every product 0) must be exactly 0.  On the CPU an f32 emulation of the kernel's chain stays below
a third of the bound (0.30 at worst) for every rate below, on inputs spread over three decades and on a constant
(tests/test_resample_host.py prints the figure).
"""
import math

import numpy as np

U = 2.0 ** -24
RATES_TO_16K = (48000, 44100, 32000, 22050, 11025, 8000)
PAIRS = tuple((r, 16000) for r in RATES_TO_16K) + ((16000, 44100),)
TAPS = {48000: 38, 44100: 34, 22050: 18, 11025: 14, 8000: 14}  # 2 * width to 16 kHz, as the issue lists them


def reduced(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def geometry(orig, new):
    """-> (o, n, base, width)."""
    o, n = reduced(orig, new)
    base = 0.99 * min(o, n)
    return o, n, base, math.ceil(6 * o / base)


def n_out_of(n_in, o, n):
    return -(-n_in * n // o)


def g(t, base, o):
    """The filter of the definition at float64 t (any shape)."""
    t = np.asarray(t, dtype=np.float64)
    safe = np.where(t == 0.0, 1.0, t)
    s = np.where(t == 0.0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))
    w = (base / o) * s * np.cos(np.pi * t / 12.0) ** 2
    return np.where(np.abs(t) < 6.0, w, 0.0)


def weights(orig, new, *, r_over="n", scale=True):
    """float64 [n, 2 * width]: taps[r][k + width - 1] = g((k - r / n) * base / o).  (r_over = "o" and scale = False are mutants.)"""
    o, n, base, width = geometry(orig, new)
    k = np.arange(-width + 1, width + 1, dtype=np.float64)[None, :]
    r = np.arange(n, dtype=np.float64)[:, None]
    t = (k - r / (n if r_over == "n" else o)) * base / o
    w = g(t, base, o)
    return w if scale else w / (base / o)


def lengths(orig, new):
    o, _ = reduced(orig, new)
    return sorted({1, 2, o, o + 1, 3 * o + 2, 257})


def signal(n, seed, kind="decades"):
    """f32 [n]: normal samples, each scaled by its own 10^U(-3, 0) (three decades), or the constant 0.75."""
    if kind == "constant":
        return np.full(n, 0.75, dtype=np.float32)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 0.0, n)).astype(np.float32)


def _take(x, j):
    """x[j] with zeros outside [0, len(x)) — j an int64 array of any shape."""
    inside = (j >= 0) & (j < x.shape[0])
    return np.where(inside, x[np.clip(j, 0, x.shape[0] - 1)], 0)


def definition(x, orig, new, ms=None):
    """The direct sum of the definition in float64 at the outputs `ms` (default: all n_out)."""
    o, n, base, width = geometry(orig, new)
    x = np.asarray(x, dtype=np.float64)
    ms = np.arange(n_out_of(x.shape[0], o, n), dtype=np.int64) if ms is None else np.asarray(ms, dtype=np.int64)
    centre = (ms * o) // n
    j = centre[:, None] + np.arange(-width - 1, width + 3, dtype=np.int64)[None, :]
    t = (j * n - ms[:, None] * o).astype(np.float64) * (base / (o * n))   # (j / o - m / n) * base, the numerator exact
    return (_take(x, j) * g(t, base, o)).sum(axis=1)


def ref_on_table(x, taps32, orig, new, ms=None):
    """-> (ref, bound) in float64 at the outputs `ms`: the exact-in-float64 polyphase sum over the f32 table, and
    (2 * width + 1) * 2^-24 * sum_k |taps32 * x|."""
    o, n, _, width = geometry(orig, new)
    taps = np.asarray(taps32)
    assert taps.dtype == np.float32 and taps.shape == (n, 2 * width)
    x = np.asarray(x)
    assert x.dtype == np.float32
    ms = np.arange(n_out_of(x.shape[0], o, n), dtype=np.int64) if ms is None else np.asarray(ms, dtype=np.int64)
    p = ms * o
    j0, r = p // n, p % n
    j = j0[:, None] + np.arange(-width + 1, width + 1, dtype=np.int64)[None, :]
    prod = taps[r].astype(np.float64) * _take(x, j).astype(np.float64)
    return prod.sum(axis=1), (2 * width + 1) * U * np.abs(prod).sum(axis=1)


def violations(got, ref, bound):
    """How many elements miss |got - ref| <= bound (a bound of 0 asks for exactly 0; a non-finite value always misses)."""
    got = np.asarray(got, dtype=np.float64)
    return int((~(np.abs(got - ref) <= bound)).sum())


def worst_ratio(got, ref, bound):
    got = np.asarray(got, dtype=np.float64)
    live = bound > 0
    return float((np.abs(got - ref)[live] / bound[live]).max()) if live.any() else 0.0


# ------------------------------------------------------------------------------------------------- the kernel, emulated
MUTANTS = ("phase_from_m_times_n", "r_over_o", "taps_reversed", "first_tap_dropped", "last_tap_dropped", "edge_clamped", "scale_missing",
           "phase_32bit", "j0_off_by_one", "n_out_floor")


def emulate(x, taps32, orig, new, ms=None, mutant=None):
    """numpy emulation of the kernel: per output one f32 fma chain from 0.0f in ascending k over taps32[r] (the fma as a float64
    product and sum rounded to f32: the product is exact, the double rounding is far below the bound).  -> f32 at `ms`
    (default all; the length is the mutant's n_out).  Table mutants (r_over_o, scale_missing) come in through `taps32`."""
    assert mutant is None or mutant in MUTANTS
    o, n, _, width = geometry(orig, new)
    x = np.asarray(x)
    taps = np.asarray(taps32)
    assert x.dtype == np.float32 and taps.dtype == np.float32
    n_in = x.shape[0]
    n_out = n_in * n // o if mutant == "n_out_floor" else n_out_of(n_in, o, n)
    ms = np.arange(n_out, dtype=np.int64) if ms is None else np.asarray(ms, dtype=np.int64)
    p = ms * (n if mutant == "phase_from_m_times_n" else o)
    if mutant == "phase_32bit":
        p = p.astype(np.int32).astype(np.int64)  # wraps behind 2^31
    j0, r = p // n, p % n
    if mutant == "j0_off_by_one":
        j0 = j0 + 1
    rows = taps[r]
    if mutant == "taps_reversed":
        rows = rows[:, ::-1]
    acc = np.zeros(ms.shape[0], dtype=np.float32)
    for c in range(2 * width):
        if (mutant == "first_tap_dropped" and c == 0) or (mutant == "last_tap_dropped" and c == 2 * width - 1):
            continue
        j = j0 + (c - width + 1)
        xv = x[np.clip(j, 0, n_in - 1)] if mutant == "edge_clamped" else _take(x, j).astype(np.float32)
        acc = (acc.astype(np.float64) + rows[:, c].astype(np.float64) * xv.astype(np.float64)).astype(np.float32)
    return acc


def impulse_expected(taps32, orig, new, n_in, j_imp):
    """The exact response to x = delta(j - j_imp): out[m] = taps32[r][j_imp - j0 + width - 1] where that column exists, else 0."""
    o, n, _, width = geometry(orig, new)
    ms = np.arange(n_out_of(n_in, o, n), dtype=np.int64)
    j0, r = (ms * o) // n, (ms * o) % n
    c = j_imp - j0 + width - 1
    ok = (c >= 0) & (c < 2 * width)
    return np.where(ok, np.asarray(taps32)[r, np.clip(c, 0, 2 * width - 1)], np.float32(0)).astype(np.float32)


def lengths_around(orig, new, target):
    """Input lengths whose n_out is the largest below `target`, the smallest >= target and the smallest > target."""
    o, n = reduced(orig, new)
    at = -(-((target - 1) * o + 1) // n)          # smallest n_in with n_out >= target
    while n_out_of(at, o, n) < target:
        at += 1
    while at > 1 and n_out_of(at - 1, o, n) >= target:
        at -= 1
    above = at
    while n_out_of(above, o, n) <= target:
        above += 1
    return sorted({max(at - 1, 1), at, above})
