"""Reference, per-element bound, cases and mutants for the time stretch (csrc/stretch.hip, include/wft.h "Time stretch").  numpy
float64 throughout; nothing is imported from the product.

THE REFERENCE restates the three stages of the header's definition, N = 2048, H = 512:
  stft     zero centre padding, F = 1 + n // H frames, periodic Hann, one-sided DFT (numpy's rfft)
  vocoder  steps = t * rate in float64 for t < T = ceil(F / rate) = len(np.arange(0, F, rate)); i = floor(step), alpha = step - i,
           mag = (1 - alpha) |D[i]| + alpha |D[i + 1]| on D extended by two zero frames, S[t] = mag * P[t], in two forms:
             "product"   P[0] = u(D[0]), P[t + 1] = P[t] u(D[i + 1]) conj(u(D[i])), u(c) = c / |c| and 1 where |c| == 0
             "additive"  librosa's accumulator: acc = angle(D[0]); acc += phi + wrap(angle(D[i + 1]) - angle(D[i]) - phi),
                         phi_k = 2 pi H k / N, wrap(x) = x - 2 pi round(x / 2 pi), P[t] = exp(i acc); the angle of an exact zero
                         counts as 0, whatever the signs of its zeros
  istft    irfft of every S[t] times the window, overlap-add at hop H, division by the window's sum of squares where that exceeds
           the smallest normal float32, the first N/2 samples dropped, trimmed or zero-padded to n_out = int(round(n / rate)).
`emulate_f32` is an honest float32 restatement: scipy.fft on float32 input (pocketfft keeps float32), the product recurrence in
complex64 renormalised every step, float32 window, overlap-add and division; only t * rate, its floor and alpha stay float64.

THE BOUND is built from the float64 reference's own intermediates, with u = 2^-24 and a constant c:
  * delta_t = c u log2(N) ||windowed frame t||_2 is the allowance of every bin of D[t].
      An FFT of N points in floating point has a normwise error of at most about log2(N) u ||X||_2 (Higham, Accuracy and Stability
      of Numerical Algorithms, th. 24.2); spread evenly over the N bins that is log2(N) u ||x||_2 per bin (Parseval: ||X||_2 =
      sqrt(N) ||x||_2).  c scales it: it also pays for the rounding of the fp32 window and of the windowed sample, and it is below 1
      when the errors of the butterflies add like a random walk, as they do.
  * a unit vector u(D[j, k]) computed from a bin that is off by at most delta_j is off by an angle of at most
      pe(j, k) = min(pi, delta_j / |D[j, k]|)      (and exactly 0 where delta_j = 0: an all-zero frame transforms to exact zeros)
    so the phase of bin k at step t is off by at most the running sum, over the EARLIER steps s < t, of
      pe(i_s, k) + pe(i_s + 1, k) + 4 u            (4 u: the two complex products, the division and the renormalisation)
    called theta[t, k].  (P[0] = u(D[0]) itself: S[0] = |D[0]| u(D[0]) = D[0], whose error delta_0 is the second term below.)
  * E[t, k] = mag theta + (1 - alpha) delta_i + alpha delta_{i + 1} + 4 u mag
      (a rotation by theta moves a vector of length mag by at most mag theta; |D| is 1-Lipschitz; 4 u: sqrt, the two products of
      the interpolation and the product with P)
  * a sample of the inverse transform of frame t is (1/N) (S_0 + S_N/2 (-1)^n + 2 Re sum_{0<k<N/2} S_k e^{..}), so it moves by at
    most a_t = (2 / N) sum_k E[t, k]
  * a_t goes through the same synthesis as the signal: times the window, overlap-add, division by the sum of squares, trim, length.
      (The rounding of the synthesis itself — inverse FFT, window, four adds, one division — is a few u of values that the 4 u mag
      term already dominates: sum_k mag (2 / N) is at least the frame's amplitude.)
An output sample passes iff |got - want| <= allow; NaN fails; where allow == 0 (silence) the sample must be exactly 0.

CHOOSING c (tools: tests/test_stretch_host.py measures and asserts it): C_EMU is the smallest power of two for which
`emulate_f32` stays inside the bound — every output sample AND every bin of the STFT under delta_t — on every case below,
measured against the float64 reference, never against the kernel.  C = 4 * C_EMU is what the kernel is held to: its radix-2 FFT
sums in another order than pocketfft's.  Measured on the CPU at c = 1 (worst over the 24 cases, as the share of the allowance used):
    STFT bins 0.84 (noise16421), output samples 0.020 (noise2048 at rate 0.75); the largest allowance is 4.5e-4 against a 0.1-rms signal
so the output samples alone would pass with a far smaller c, but the STFT bins do not at c = 1/2 (0.84 * 2 > 1): C_EMU = 1, C = 4.
At C = 4 every one of the fourteen mutants leaves the bound on at least one case (tests/test_stretch_host.py).
On an MI355X the kernel uses at most 0.0065 of the C = 4 allowance over the 24 cases (0.21 of delta_t in the STFT stage).
"""
import math

import numpy as np

U = 2.0 ** -24
N, H, BINS, LOGN = 2048, 512, 1025, 11
TINY32 = float(np.finfo(np.float32).tiny)
f32, c64 = np.float32, np.complex64

C_EMU = 1.0
C = 4 * C_EMU

NOISE_N = (2048, 5000, 16421)              # 5, 10 and 33 frames; the last two are no multiple of the hop
ZERO_LEAD, ZERO_BODY, ZERO_TAIL = 4096, 5000, 6000
RATES = (1.0, 0.75, 0.8, 1.1037, 1.25)
# a rate at which float32 stepping picks another column pair: floor(f32(t) * f32(rate)) != floor(t * rate) at t = TRAP_T
# (found by `find_trap`, a scan of the rates k / 1000 on the CPU; asserted by tests/test_stretch_host.py)
TRAP_RATE, TRAP_T = 0.58, 50

MUTANTS = ("column_off_by_one", "alpha_swapped", "conj_dropped", "phase_reset_every_frame", "p0_is_one", "mag_from_first_column",
           "reflect_padding", "hann_symmetric", "no_sumsquare_division", "no_trim", "T_one_short", "n_out_truncated",
           "float32_stepping", "unit_of_zero_is_minus_one")


# ================================================================================================================ inputs
def noise(n, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(f32)


def zero_padded_row():
    """4096 exact zeros, 5000 samples of noise, 6000 exact zeros: the loader's real shape."""
    x = np.zeros(ZERO_LEAD + ZERO_BODY + ZERO_TAIL, dtype=f32)
    x[ZERO_LEAD:ZERO_LEAD + ZERO_BODY] = noise(ZERO_BODY, 99)
    return x


def inputs():
    """name -> f32 [n]."""
    d = {f"noise{n}": noise(n, n) for n in NOISE_N}
    d["zeropad"] = zero_padded_row()
    return d


def rates():
    return RATES + ((TRAP_RATE,) if TRAP_RATE is not None else ())


def cases():
    """(input name, rate) over every input and every rate."""
    return [(name, r) for name in inputs() for r in rates()]


def find_trap(F=33):
    """The first (rate, t) of a fixed scan with t < ceil(F / rate) and another floor in float32 than in float64."""
    for k in range(501, 2000):
        rate = k / 1000.0
        T = n_out_frames(F, rate)
        t = np.arange(T)
        a = np.floor(t * rate)
        b = np.floor((t.astype(f32) * f32(rate)).astype(np.float64))
        bad = np.flatnonzero(a != b)
        if bad.size:
            return rate, int(bad[0])
    return None


# ================================================================================================================ reference
def hann(symmetric=False):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / (N - 1 if symmetric else N))


def n_frames(n):
    return 1 + n // H


def n_out_frames(F, rate):
    return int(math.ceil(F / rate))


def n_out_samples(n, rate, mutant=None):
    return int(n / rate) if mutant == "n_out_truncated" else int(round(n / rate))


def frames_of(y, mutant=None):
    """float64 [F, N]: the windowed frames."""
    y = np.asarray(y, dtype=np.float64)
    pad = np.pad(y, N // 2, mode="reflect" if mutant == "reflect_padding" else "constant")
    idx = np.arange(n_frames(y.shape[0]))[:, None] * H + np.arange(N)[None, :]
    return pad[idx] * hann(mutant == "hann_symmetric")


def stft(y, mutant=None):
    return np.fft.rfft(frames_of(y, mutant), axis=1)


def steps_of(F, rate, mutant=None):
    """(i int [T], alpha float64 [T])."""
    T = n_out_frames(F, rate) - (1 if mutant == "T_one_short" else 0)
    t = np.arange(T)
    steps = (t.astype(f32) * f32(rate)).astype(np.float64) if mutant == "float32_stepping" else t * float(rate)
    i = np.floor(steps).astype(np.int64)
    return i, steps - i


def _unit(c, mutant=None):
    m = np.abs(c)
    zero = m == 0
    u = c / np.where(zero, 1, m)
    return np.where(zero, -1.0 if mutant == "unit_of_zero_is_minus_one" else 1.0, u).astype(c.dtype)


def vocoder(D, rate, form="product", mutant=None):
    """D complex [F, 1025] -> S complex [T, 1025] in D's precision (complex128 or complex64); steps stay float64."""
    D = np.asarray(D)
    ct = D.dtype
    rt = np.float32 if ct == c64 else np.float64
    F = D.shape[0]
    Dz = np.concatenate([D, np.zeros((3, BINS), dtype=ct)])
    i, alpha = steps_of(F, rate, mutant)
    if mutant == "column_off_by_one":
        i = i + 1
    alpha = alpha.astype(rt)
    if mutant == "alpha_swapped":
        alpha = (1 - alpha).astype(rt)
    S = np.zeros((i.shape[0], BINS), dtype=ct)
    mags = np.abs(Dz).astype(rt)
    if form == "additive":
        assert ct == np.complex128 and mutant is None
        ang = np.where(mags == 0, 0.0, np.angle(Dz))
        phi = 2.0 * np.pi * H * np.arange(BINS) / N
        acc = ang[0].copy()
        for t in range(i.shape[0]):
            mag = (1 - alpha[t]) * mags[i[t]] + alpha[t] * mags[i[t] + 1]
            S[t] = mag * np.exp(1j * acc)
            d = ang[i[t] + 1] - ang[i[t]] - phi
            acc += phi + d - 2.0 * np.pi * np.round(d / (2.0 * np.pi))
        return S
    un = _unit(Dz, mutant)
    P = np.ones(BINS, dtype=ct) if mutant == "p0_is_one" else un[0].copy()
    for t in range(i.shape[0]):
        if mutant == "phase_reset_every_frame":
            P = un[i[t]]
        m1 = mags[i[t]] if mutant == "mag_from_first_column" else mags[i[t] + 1]
        mag = (rt(1) - alpha[t]) * mags[i[t]] + alpha[t] * m1
        S[t] = (mag * P).astype(ct)
        P = P * (un[i[t] + 1] * (un[i[t]] if mutant == "conj_dropped" else np.conj(un[i[t]])))
        P = _unit(P.astype(ct))
    return S


def synthesis(fr, n_out, mutant=None, rt=np.float64):
    """fr real [T, N], already windowed -> y [n_out]: overlap-add, sum-of-squares division, trim, length (in precision rt)."""
    T = fr.shape[0]
    w = hann(mutant == "hann_symmetric").astype(rt)
    L = N + H * max(T - 1, 0)
    y, wss = np.zeros(L, dtype=rt), np.zeros(L, dtype=rt)
    for t in range(T):
        y[t * H:t * H + N] += fr[t].astype(rt)
        wss[t * H:t * H + N] += w * w
    if mutant != "no_sumsquare_division":
        nz = wss > TINY32
        y[nz] = y[nz] / wss[nz]
    if mutant != "no_trim":
        y = y[N // 2:]
    out = np.zeros(n_out, dtype=rt)
    m = min(n_out, y.shape[0])
    out[:m] = y[:m]
    return out


def istft(S, n_out, mutant=None):
    S = np.asarray(S, dtype=np.complex128)
    return synthesis(np.fft.irfft(S, n=N, axis=1) * hann(mutant == "hann_symmetric"), n_out, mutant)


def time_stretch(y, rate, form="product", mutant=None):
    """float64 [n_out]: the whole definition."""
    n = np.asarray(y).shape[0]
    return istft(vocoder(stft(y, mutant), rate, form, mutant), n_out_samples(n, rate, mutant), mutant)


def emulate_f32(y, rate, stage=None):
    """The same in float32 (see the module docstring) -> f32 [n_out]; stage="stft": the complex64 D instead."""
    import scipy.fft

    y = np.asarray(y, dtype=f32)
    w = hann().astype(f32)
    pad = np.pad(y, N // 2)
    idx = np.arange(n_frames(y.shape[0]))[:, None] * H + np.arange(N)[None, :]
    D = scipy.fft.rfft(pad[idx] * w, axis=1)
    assert D.dtype == c64
    if stage == "stft":
        return D
    S = vocoder(D, rate)
    fr = scipy.fft.irfft(S, n=N, axis=1)
    assert fr.dtype == f32
    return synthesis(fr * w, n_out_samples(y.shape[0], rate), rt=f32)


# ================================================================================================================ the bound
def stft_allowance(y, c=C):
    """float64 [F]: delta_t."""
    return c * U * LOGN * np.linalg.norm(frames_of(y), axis=1)


def allowance(y, rate, c=C):
    """-> (want float64 [n_out], allow float64 [n_out], parts dict): the reference output and its per-sample allowance."""
    y = np.asarray(y)
    n = y.shape[0]
    D = stft(y)
    F = D.shape[0]
    delta = np.concatenate([stft_allowance(y, c), np.zeros(3)])
    mags = np.concatenate([np.abs(D), np.zeros((3, BINS))])
    with np.errstate(divide="ignore", invalid="ignore"):
        pe = np.where(delta[:, None] == 0, 0.0, np.minimum(np.pi, delta[:, None] / mags))
    i, alpha = steps_of(F, rate)
    step_err = pe[i] + pe[i + 1] + 4 * U                                   # [T, BINS]
    theta = np.concatenate([np.zeros((1, BINS)), np.cumsum(step_err, axis=0)[:-1]])
    mag = (1 - alpha)[:, None] * mags[i] + alpha[:, None] * mags[i + 1]
    E = mag * theta + ((1 - alpha) * delta[i] + alpha * delta[i + 1])[:, None] + 4 * U * mag
    a = (2.0 / N) * E.sum(axis=1)                                          # [T]
    n_out = n_out_samples(n, rate)
    allow = synthesis(a[:, None] * hann()[None, :], n_out)
    S = vocoder(D, rate)
    want = istft(S, n_out)
    return want, allow, {"D": D, "S": S, "delta": delta[:F], "frame_allow": a}


def istft_allowance(S, n_out):
    """The allowance of the synthesis alone, run on a given S: 4 u mag per bin (see E) pushed through the synthesis."""
    a = (2.0 / N) * (4 * U * np.abs(S)).sum(axis=1)
    return synthesis(a[:, None] * hann()[None, :], n_out)


def outside(got, want, allow):
    """How many samples lie outside the allowance; a length mismatch counts every sample of the longer one."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != want.shape:
        return max(got.shape[0], want.shape[0])
    return int((~(np.abs(got - want) <= allow)).sum())


def used(got, want, allow):
    """The largest error / allowance (0 / 0 counts as 0, x / 0 as inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / allow)
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0


# ================================================================================================================ vocoder, exact
def exact_spectra(F=9, seed=5):
    """complex64 [F, 1025]: every bin a power of two (2^-6 .. 2^6) times one of {1, i, -1, -i}, or an exact zero with mixed signs
    of its zeros; with a dyadic alpha every product and sum of the vocoder is exact, so a correct kernel matches bit for bit."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-6, 7, (F, BINS))
    q = rng.integers(0, 4, (F, BINS))
    mag = (2.0 ** e).astype(f32)
    re = np.where(q == 0, mag, np.where(q == 2, -mag, f32(0))).astype(f32)
    im = np.where(q == 1, mag, np.where(q == 3, -mag, f32(0))).astype(f32)
    z = rng.random((F, BINS)) < 0.15
    z[:, 7] = True       # a bin that is zero in every frame
    z[0:3, 11] = True    # leading zero frames of a bin
    z[0, 13] = True
    sr, si = rng.random((F, BINS)) < 0.5, rng.random((F, BINS)) < 0.5
    re = np.where(z, np.where(sr, f32(-0.0), f32(0.0)), re).astype(f32)
    im = np.where(z, np.where(si, f32(-0.0), f32(0.0)), im).astype(f32)
    return re, im


def vocoder_exact(re, im, rate):
    """The kernel's expression tree in float32 on (re, im) f32 [F, 1025] -> (S_re, S_im) f32 [T, 1025].  Every operation is exact on
    `exact_spectra`, so the bits — the signs of zeros included — are those of IEEE arithmetic on this tree, fused or not."""
    F = re.shape[0]
    zr = np.zeros((3, BINS), dtype=f32)
    re, im = np.concatenate([re, zr]), np.concatenate([im, zr])
    i, alpha = steps_of(F, rate)
    alpha = alpha.astype(f32)
    mags = np.sqrt(re * re + im * im).astype(f32)

    def unit(r, j, m):
        z = m == 0
        d = np.where(z, f32(1), m)
        return np.where(z, f32(1), r / d).astype(f32), np.where(z, f32(0), j / d).astype(f32)

    ur, ui = unit(re, im, mags)
    Pr, Pi = ur[0].copy(), ui[0].copy()
    Sr, Si = np.zeros((i.shape[0], BINS), dtype=f32), np.zeros((i.shape[0], BINS), dtype=f32)
    for t in range(i.shape[0]):
        a, b = i[t], i[t] + 1
        mag = (f32(1) - alpha[t]) * mags[a] + alpha[t] * mags[b]
        Sr[t], Si[t] = mag * Pr, mag * Pi
        qr = ur[b] * ur[a] + ui[b] * ui[a]
        qi = ui[b] * ur[a] - ur[b] * ui[a]
        pr = Pr * qr - Pi * qi
        pi = Pr * qi + Pi * qr
        Pr, Pi = unit(pr, pi, np.sqrt(pr * pr + pi * pi).astype(f32))
    return Sr, Si


# ================================================================================================================ ragged log-mel
def frames_and_keep(n_samples, keep_frames, T_out):
    """(frames_b, kept columns) of one row, as include/wft.h "wft_logmel_ragged" states them."""
    frames = n_samples // 160
    return frames, min(keep_frames, frames, T_out)


# (n_samples, keep_frames, T_out) -> (frames_b, kept): worked by hand
RAGGED_TABLE = (((6400, 3000, 48), (40, 40)), ((7680, 3000, 48), (48, 48)), ((9600, 3000, 48), (60, 48)), ((9600, 25, 48), (60, 25)),
                ((6477, 3000, 48), (40, 40)), ((640000, 1500, 3000), (4000, 1500)), ((384000, 3000, 3000), (2400, 2400)),
                ((159, 3000, 48), (0, 0)))


def logmel_ragged_interval(x, filt, n_frames_row):
    """tests/_audio_cases.logmel_interval for a clip whose length is no multiple of 160: frames_b = len(x) // 160 frames over the
    reflect padding of ALL len(x) samples.  Same error model, same constants; -> (ref, lo, hi) float64 [n_mels, frames_b]."""
    from tests import _audio_cases as A

    x = np.asarray(x, dtype=np.float64)
    assert n_frames_row == x.shape[0] // A.HOP and x.shape[0] > A.NFFT
    pad = np.pad(x, A.NFFT // 2, mode="reflect")
    fr = pad[np.arange(n_frames_row)[:, None] * A.HOP + A._N[None, :]] * A._HANN
    S, re, im = np.abs(fr).sum(axis=1), fr @ A._COS, -(fr @ A._SIN)
    F = np.asarray(filt, dtype=np.float64)
    e = (256.0 * A.U * S)[:, None]
    P = re * re + im * im
    dP = 2.0 * (np.abs(re) + np.abs(im)) * e + 2.0 * e * e + 4.0 * A.U * P
    M = F @ P.T
    dM = np.abs(F) @ dP.T + 32.0 * A.U * M
    lg = np.log10(np.maximum(M, 1e-10))
    lg_lo = np.log10(np.maximum(M - dM, 1e-10)) - A.D_LOG
    lg_hi = np.log10(np.maximum(M + dM, 1e-10)) + A.D_LOG
    ref = (np.maximum(lg, lg.max() - 8.0) + 4.0) / 4.0
    lo = (np.maximum(lg_lo, lg_lo.max() - 8.0) + 4.0) / 4.0 - A.D_OUT
    hi = (np.maximum(lg_hi, lg_hi.max() - 8.0) + 4.0) / 4.0 + A.D_OUT
    return ref, lo, hi
