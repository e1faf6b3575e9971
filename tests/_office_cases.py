"""Shared by test_office_host.py (CPU) and test_office_gpu.py: the float64 reference of wft_fir_conv_f32, a numpy f32 EMULATION of
its scheme (the same radix-2 order, partitions, one-sided product and scale; optionally with one planted defect), the per-element
bound, numpy's bit crush, and the case table.

The bound of an element of output block k of row b (include/wft.h "Office effects"):

    |out - ref| <= C * 11 * 2^-24 * sum_p ||x_seg(k - p)||_2 * ||h_p||_2 + ABS_TERM

over the block's live partitions p (p < ceil(T / 1024), p <= k), x_seg(m) = x[(m - 1) * 1024 .. (m + 1) * 1024) inside [0, N) and
h_p = ir[p * 1024 .. (p + 1) * 1024) inside [0, T).  11 = log2(2048) butterfly stages, 2^-24 = the unit roundoff of f32.

C: the largest ratio |emulation - ref| / (11 * 2^-24 * sum) that the emulation reaches over the whole case table on the CPU is
MEASURED_RATIO (test_office_host.py asserts that it still is); C is four times that.  The margin covers what the emulation does not
model: FMA contraction of the butterflies and products, and sincospif twiddles that may differ from the correctly rounded ones by an
ulp.  Zeros behind n[b], a T == 0 row (a bit copy) and everything behind n_max (untouched) are compared exactly.
"""
import random

import numpy as np

from whisper_finetune.data import office_fx as OF

L = 1024
NFFT = 2048
LOGN = 11
SENTINEL = np.float32(-7.25)
MEASURED_RATIO = 0.17  # 0.16998 on the CPU, at case n1025_t2_x_impulses_p1 (impulses at the block seams against a 2-tap response)
C = 4 * MEASURED_RATIO  # 0.68
ABS_TERM = 2.0 ** -120  # subnormal products and sums
EPS_TERM = 11 * 2.0 ** -24

N_MAXES = (1, 1023, 1024, 1025, 2049, 3 * 1024 + 5)
TAPS_MAXES = (1, 2, 1023, 1024, 1025, 2048, 2049)
PAD_X, PAD_IR = 3, 2  # columns behind n_max / taps_max of a row's buffer (poisoned on input, sentinel on output)

MUTANTS = ("block_start_off_by_one", "last_partition_dropped", "partition_segment_mismatch", "first_half_kept", "tap_behind_n_taps_read",
           "sample_at_n_read", "neighbour_ir", "no_zero_fill", "no_conjugate", "scale_lost", "negative_wrapped", "t0_not_copied")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the f32 emulation
_M = np.arange(NFFT // 2, dtype=np.float64)
TW_RE = np.cos(np.pi * _M / (NFFT // 2)).astype(np.float32)
TW_IM = (-np.sin(np.pi * _M / (NFFT // 2))).astype(np.float32)
BREV = np.array([int(format(i, "011b")[::-1], 2) for i in range(NFFT)], dtype=np.int64)


def fft_f32(re, im, inverse=False):
    """The kernel's FFT on f32 arrays [2048] that hold the input in bit-reversed order: 11 decimation-in-time stages, each product and
    sum rounded to f32 on its own.  Returns (re, im) in natural order; the inverse is unscaled."""
    re, im = re.astype(np.float32).copy(), im.astype(np.float32).copy()
    j = np.arange(NFFT // 2)
    for s in range(LOGN):
        half = 1 << s
        pos = j & (half - 1)
        i0 = ((j >> s) << (s + 1)) + pos
        i1 = i0 + half
        wr, wi = TW_RE[pos << (LOGN - 1 - s)], TW_IM[pos << (LOGN - 1 - s)]
        if inverse:
            wi = -wi
        ar, ai, br, bi = re[i0], im[i0], re[i1], im[i1]
        tr = wr * br - wi * bi
        ti = wr * bi + wi * br
        re[i0], im[i0], re[i1], im[i1] = ar + tr, ai + ti, ar - tr, ai - ti
    return re, im


def _spectrum(seg):
    """seg f32 [2048] in natural order -> its one-sided spectrum (re, im) f32 [1025]."""
    re, im = fft_f32(seg[BREV], np.zeros(NFFT, dtype=np.float32))
    return re[:L + 1], im[:L + 1]


def emulate(X, ns, IR, Ts, n_max, taps_max, mutant=None):
    """The scheme of csrc/office.hip in numpy f32.  X f32 [B, ld >= n_max], IR f32 [B, ld_ir >= taps_max] (whatever lies behind n[b] /
    n_taps[b] must not matter), ns / Ts integers (clamped as the kernel clamps them) -> f32 [B, ld], SENTINEL where nothing is
    written.  mutant: None, or one of MUTANTS = a planted defect."""
    assert mutant is None or mutant in MUTANTS, mutant
    B, ld = X.shape
    out = np.full((B, ld), SENTINEL, dtype=np.float32)
    blocks = -(-n_max // L)
    for b in range(B):
        N, T = min(max(int(ns[b]), 0), n_max), min(max(int(Ts[b]), 0), taps_max)
        row = X[b]
        ir = IR[(b + 1) % B] if mutant == "neighbour_ir" else IR[b]
        t_read = taps_max if mutant == "tap_behind_n_taps_read" else T
        H = []
        for p in range(-(-T // L)):
            h = np.zeros(NFFT, dtype=np.float32)
            cnt = min(L, t_read - p * L)
            h[:cnt] = ir[p * L:p * L + cnt]
            H.append(_spectrum(h))
        for k in range(blocks):
            i0 = k * L
            cnt = min(L, n_max - i0)
            idx = i0 + np.arange(cnt)
            if i0 >= N or (T == 0 and mutant != "t0_not_copied"):
                vals = np.where(idx < N, row[np.minimum(idx, ld - 1)], np.float32(0)) if T == 0 else np.zeros(cnt, dtype=np.float32)
            else:
                live = min(len(H), k + 1)
                if mutant == "last_partition_dropped":
                    live -= 1
                acc_r, acc_i = np.zeros(L + 1, dtype=np.float32), np.zeros(L + 1, dtype=np.float32)
                for p in range(live):
                    m = k - p + 1 if mutant == "partition_segment_mismatch" else k - p
                    j = (m - 1) * L + np.arange(NFFT) + (1 if mutant == "block_start_off_by_one" else 0)
                    inside = (j >= 0) & ((j <= N) if mutant == "sample_at_n_read" else (j < N))
                    jj = np.clip(j, 0, ld - 1)
                    if mutant == "negative_wrapped" and N > 0:
                        inside, jj = inside | (j < 0), np.where(j < 0, j % N, jj)
                    seg = np.where(inside, row[jj], np.float32(0)).astype(np.float32)
                    xr, xi = _spectrum(seg)
                    hr, hi = H[p]
                    acc_r = acc_r + (xr * hr - xi * hi)
                    acc_i = acc_i + (xr * hi + xi * hr)
                full_r, full_i = np.zeros(NFFT, dtype=np.float32), np.zeros(NFFT, dtype=np.float32)
                full_r[:L + 1], full_i[:L + 1] = acc_r, acc_i
                full_r[NFFT - 1:L:-1] = acc_r[1:L]
                full_i[NFFT - 1:L:-1] = acc_i[1:L] if mutant == "no_conjugate" else -acc_i[1:L]
                yr, _ = fft_f32(full_r[BREV], full_i[BREV], inverse=True)
                y = (yr[:L] if mutant == "first_half_kept" else yr[L:])[:cnt]
                if mutant != "scale_lost":
                    y = y * np.float32(1.0 / NFFT)
                vals = np.where(idx < N, y, np.float32(0)).astype(np.float32)
            if mutant == "no_zero_fill":
                keep = idx < N
                out[b, idx[keep]] = vals[keep]
            else:
                out[b, idx] = vals
    return out


# ------------------------------------------------------------------------------------------------------------ reference and bound
def reference(x, n, h, T, n_max):
    """out[i] = sum_{j < T} h[j] x[i - j] for i < N in float64, zeros up to n_max."""
    N, T = min(max(int(n), 0), n_max), max(int(T), 0)
    out = np.zeros(n_max, dtype=np.float64)
    if N > 0:
        xs = np.asarray(x[:N], dtype=np.float64)
        out[:N] = np.convolve(xs, np.asarray(h[:T], dtype=np.float64))[:N] if T > 0 else xs
    return out


def norm_sum(x, n, h, T, n_max):
    """sum_p ||x_seg(k - p)||_2 * ||h_p||_2 of every element's block, float64 [n_max]."""
    N, T = min(max(int(n), 0), n_max), max(int(T), 0)
    xs, hs = np.asarray(x[:N], dtype=np.float64), np.asarray(h[:T], dtype=np.float64)
    out = np.zeros(n_max, dtype=np.float64)
    for k in range(-(-n_max // L)):
        s = 0.0
        for p in range(min(-(-T // L), k + 1)):
            lo, hi = max((k - p - 1) * L, 0), min((k - p + 1) * L, N)
            if hi > lo:
                s += float(np.sqrt((xs[lo:hi] ** 2).sum())) * float(np.sqrt((hs[p * L:(p + 1) * L] ** 2).sum()))
        out[k * L:(k + 1) * L] = s
    return out


def bound(x, n, h, T, n_max, c=None):
    return (C if c is None else c) * EPS_TERM * norm_sum(x, n, h, T, n_max) + ABS_TERM


def check(out, case, c=None):
    """out f32 [B, ld] (a kernel's or the emulation's whole output buffer, SENTINEL-filled before the call) against the case:
    -> (ok, worst ratio |out - ref| / (11 * 2^-24 * sum) over the bounded elements, the first complaint or None)."""
    X, IR, n_max = case["X"], case["IR"], case["n_max"]
    worst, complaint = 0.0, None
    for b in range(X.shape[0]):
        N, T = min(max(int(case["ns"][b]), 0), n_max), min(max(int(case["Ts"][b]), 0), case["taps_max"])
        got = out[b]
        if not bool((bits(got[n_max:]) == bits(SENTINEL)).all()):
            complaint = complaint or (b, "written behind n_max")
        if bits(got[N:n_max]).any():
            complaint = complaint or (b, "not +0.0 behind n[b]")
        if T == 0:
            if not bool((bits(got[:N]) == bits(X[b, :N])).all()):
                complaint = complaint or (b, "a T == 0 row is not a bit copy")
            continue
        ref = reference(X[b], N, IR[b], T, n_max)[:N]
        err = np.abs(got[:N].astype(np.float64) - ref)
        lim = bound(X[b], N, IR[b], T, n_max, c)[:N]
        bad = np.flatnonzero(~(err <= lim))  # (a NaN is bad)
        if bad.size:
            complaint = complaint or (b, "outside the bound", int(bad[0]), float(got[bad[0]]), float(ref[bad[0]]), float(lim[bad[0]]))
        s = norm_sum(X[b], N, IR[b], T, n_max)[:N]
        ok = s > 0
        if ok.any():
            with np.errstate(invalid="ignore"):
                r = err[ok] / (EPS_TERM * s[ok])
            worst = max(worst, float(np.nanmax(r))) if np.isfinite(r).any() else worst
    return complaint is None, worst, complaint


# ------------------------------------------------------------------------------------------------------------ bit crush
def bitcrush_numpy(x, depth):
    """audiomentations' BitCrush.apply on an f32 array: np.round(x * q) / q with q = 2^(depth - 1) + 1; a depth outside [1, 24]
    (0 included) copies."""
    x = np.asarray(x, dtype=np.float32)
    if not 1 <= int(depth) <= 24:
        return x.copy()
    q = np.float32(2 ** (int(depth) - 1) + 1)
    return (np.round(x * q) / q).astype(np.float32)


def crush_values():
    """Ties, +-0, values above 1, subnormals and dense values: f32 [N]."""
    rng = np.random.default_rng(3)
    ties = np.concatenate([(np.arange(-9, 10) + 0.5) / q for q in (2.0, 33.0, 8193.0, 8388609.0)])
    special = np.array([0.0, -0.0, 1.0, -1.0, 1.5, -2.75, 3.0e5, 1e-40, -1e-40, 0.99999994, 1e-8, -1e-8])
    return np.concatenate([ties, special, rng.uniform(-1.2, 1.2, 1500)]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the case table
def _room_row():
    state = random.getstate()
    random.seed(17)
    names, row = OF.OfficeAug(16000, room={"p": 1.0}).draw()
    random.setstate(state)
    assert names["room"]
    return row[2:2 + int(row[1])].astype(np.float32)


def _buffers(rows, ns, irs, Ts, n_max, taps_max):
    """-> X f32 [B, n_max + PAD_X] with NaN behind n[b], IR f32 [B, taps_max + PAD_IR] with NaN behind n_taps[b]."""
    B = len(rows)
    X = np.full((B, n_max + PAD_X), np.nan, dtype=np.float32)
    IR = np.full((B, taps_max + PAD_IR), np.nan, dtype=np.float32)
    for b in range(B):
        X[b, :ns[b]] = rows[b][:ns[b]]
        IR[b, :Ts[b]] = irs[b][:Ts[b]]
    return X, IR


def _case(name, rows, ns, irs, Ts, n_max, taps_max):
    X, IR = _buffers(rows, ns, irs, Ts, n_max, taps_max)
    return dict(name=name, X=X, IR=IR, ns=list(ns), Ts=list(Ts), n_max=n_max, taps_max=taps_max)


def _build_cases():
    rng = np.random.default_rng(20261021)
    cases = []
    i = 0
    for n_max in N_MAXES:
        for taps_max in TAPS_MAXES:
            pattern, kind = (i // 3) % 3, i % 3
            i += 1
            tm = taps_max
            ns, Ts = (([n_max, 2 * n_max // 3, 0], [tm, tm // 2, tm]), ([2 * n_max // 3, n_max, n_max - 1], [0, tm, (tm + 1) // 2]),
                      ([n_max - 1, 0, n_max], [tm - 1, tm, 0]))[pattern]
            rows = [(rng.standard_normal(n_max) * 0.25).astype(np.float32) for _ in range(3)]
            irs = [(rng.standard_normal(tm) * (0.5 / np.sqrt(tm))).astype(np.float32) for _ in range(3)]
            if kind == 1:  # impulses in the input at the block seams and at the row's end
                for b in range(3):
                    rows[b][:] = 0
                    for q, at in enumerate((0, 1023, 1024, 1025, ns[b] - 1)):
                        if 0 <= at < ns[b]:
                            rows[b][at] = np.float32((1.0, -0.75, 0.5, -1.25, 0.625)[q])
            if kind == 2:  # one impulse in the IR: the output is a shifted, scaled copy
                for b in range(3):
                    irs[b][:] = 0
                    spots = [at for at in (0, 1023, 1024, Ts[b] - 1) if 0 <= at < Ts[b]]
                    if spots:
                        irs[b][spots[(b + i) % len(spots)]] = np.float32(0.75)
            cases.append(_case(f"n{n_max}_t{tm}_{('dense', 'x_impulses', 'ir_impulse')[kind]}_p{pattern}", rows, ns, irs, Ts, n_max, tm))
    room = _room_row()
    n_max = 3 * 1024 + 5
    rows = [(rng.standard_normal(n_max) * 0.25).astype(np.float32) for _ in range(3)]
    cases.append(_case("room_ir", rows, [n_max, 1500, n_max - 1], [room, room, room[:700]], [room.shape[0], room.shape[0], 700], n_max, 2048))
    return cases


CASES = _build_cases()
CASE_IDS = [c["name"] for c in CASES]