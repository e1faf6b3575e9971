"""References, per-element bounds, cases and mutants for the audio front end (csrc/audio.hip: wft_logmel, wft_specaug,
wft_mel_to_tmajor_bf16).  numpy float64 throughout; nothing is imported from the product.  The mel filterbanks of the model come in
as arguments (the oracle builds them); the synthetic banks are made here.

LOG-MEL.  The reference is the definition: reflect-pad 200 samples on each side, frames f * 160 .. f * 160 + 399 for f < n_frames, the
periodic Hann window w_n = 0.5 - 0.5 cos(2 pi n / 400), the direct 400-point DFT at bins 0..200, P = Re^2 + Im^2, M = F @ P,
lg = log10(max(M, 1e-10)), mx = the clip's maximum of lg over its n_frames real frames, out = (max(lg, mx - 8) + 4) / 4.

The interval.  Every step behind M is monotone non-decreasing in M and in mx, so a bound on the error of M goes through the log,
the floor and the normalisation by evaluating them at both ends.  With u = 2^-24:
  * S = sum_n |w_n x_n| of the frame.  |dRe|, |dIm| <= e = 256 u S.
      The fold x[n] +- x[400 - n] leaves at most 200 products per sum; summed in any order, fused or not, their rounding is at most
      gamma_200 * S (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5, as in _resample_cases.py).  The other 56 units
      are a round allowance for the one rounding of the windowed sample, the fold's add, the fp32 window and the 1-ulp twiddle table.
  * dP = 2 (|Re| + |Im|) e + 2 e^2 + 4 u P        ((a + da)^2 per part, then two squares' roundings and the add's)
  * dM = |F| @ dP + 32 u M                        (a filter row has at most about 30 non-zero bins: gamma_30, one term's rounding)
  * lg_lo = log10(max(M - dM, 1e-10)) - d,  lg_hi = log10(max(M + dM, 1e-10)) + d,  d = 4 * 2^-20: 4 ulp of an fp32 of
    magnitude up to 16, which covers log10f
  * mx_lo = max lg_lo, mx_hi = max lg_hi over the clip's real frames
  * out_lo = (max(lg_lo, mx_lo - 8) + 4) / 4 - 2^-22, out_hi likewise with + 2^-22 (the subtraction, the add and the division at
    magnitude up to 4)
An element passes iff out_lo <= got <= out_hi; NaN fails; no element is left out.

An interval hides a failure where it is wide, so the cases keep a condition, asserted by tests/test_audio_host.py from the
reference alone: in every clip judged this way at most 2 % of the elements have out_hi - out_lo > 1e-3.  Measured on the CPU
(float64 reference only; the model's banks of 80 and 128 filters, n_frames 3, 16, 37 and 3000; worst over those eight):
    kind      share wider than 1e-3    widest interval
    decades   0.52 %                   2.5e-2
    burst     0.20 %                   3.6e-3
    quiet     1.56 %                   2.0e-2
    silent    0                        2.4e-6
    tail      0                        4.3e-4
A linear chirp does not meet the condition (its far bins are tiny next to S) and is not judged this way.
The 201 x 201 identity bank makes every element one DFT bin, and a small bin is ill-conditioned; on these clips the reference still
gives 0.46 %, 0.19 %, 1.51 %, 0 and 0.01 % (in the order above), so it is held to the same 2 % (IDENTITY_SHARE).
The six-row bank has two rows that are one REAL bin each (bin 0, bin 200: Im = 0, so |X|^2 has one degree of freedom and is small
far more often than a complex bin's): in those two rows 5.4 %, 0, 10.8 %, 0 and 1.4 % of the elements are wider than 1e-3 (at most
8 of 74), in the other four rows none.  The host test holds the four other rows to the 2 %, the two single-bin rows to
SINGLE_BIN_SHARE = 12.5 % (1/8, the next binary fraction above the reference's 10.8 %), and the whole bank (3.6 % at worst) to SIX_ROW_SHARE = 4 %; every element is still judged.
Two honest fp32 restatements (`emulate_logmel`: "seq", an unfused chain over all 400 samples and a dense unfused filter sum, and
"fold", the kernel's folded DFT in fused chains; at 3000 frames "blas", fp32 matrix products, in their place) stay inside every
interval and use at most 0.06 of the half-width (0.023 from 16 frames on); the elements with M = 0 (the silent clip, the all-zero
filter row), whose whole interval is the log / rounding allowance, use 0.2 of it.

SPECAUGMENT.  The reference evaluates the cubic Hermite spline through (0, -1), (warp_p, y1), (T - 1, 1), y1 = 2 (warp_p - warp_d) /
(T - 1) - 1, with the end slopes the secants and the middle slope their mean, in float64: ix(t) = (ys(t) + 1) / 2 * (T - 1); then
bilinear sampling with zeros outside, the time mask, the frequency mask and the extremes.  The input rows are ramps a_m * t + b_m
with small dyadic a_m, b_m that differ per row and per clip, so inside the row the expected element is a_m * ix(t) + b_m and
    |got - want| <= |a_m| * E_IX + 4 u * max |row|      (+ E_IX * |row[T - 1]| at the last column, whose right neighbour is outside)
(two products, the add and the rounding of 1 - w1, each at most u * max |row|).  The spline overshoots: with warp_d = W - 1 at
warp_p = W, and warp_d = -W at warp_p = T - W - 1, ix runs up to 8 columns outside [0, T - 1] over some 77 columns.  There a
neighbour is outside the row and the value is row[0] * (1 + ix) or row[T - 1] * (T - ix), whose slope in ix is the edge value and
not a_m; so wherever [ix - E_IX, ix + E_IX] reaches outside [0, T - 1] the bound takes E_IX * |edge value| more, as the last
column does, and where both neighbours are outside for the whole of it the element is exactly 0.  Column 0 gets no allowance:
u = 0 there gives ix = 0 exactly in every order of the operations.  Masked elements are exactly 0 and an unwarped clip is bit-equal
to its input.  E_IX is four times the worst |ix_fp32 - ix_fp64| over the cases, rounded up to a power of two (the factor allows for
another legitimate order of the same fp32 operations); ix_fp32 is the oracle's own sequence of fp32 operations, restated in torch
by the host test up to the coordinate; `warp_ix32` here is the kernel's order of them in numpy.  Measured on the CPU, worst over
the nine (warp_p, warp_d) of every T (IX_TABLE; T = 2 admits no warp):
    T       oracle's order    kernel's order
    257     4.1e-05           4.4e-05
    300     5.3e-05           5.0e-05
    3000    5.5e-04           7.3e-04
so E_IX = 2^-8 = 3.9e-3 from either column and from the larger of the two (4 * 5.5e-4 = 2.2e-3, 4 * 7.3e-4 = 2.9e-3).
The random-valued spectrogram of every T is compared with the oracle at 1e-3 absolute; its values are uniform in +-SPEC_RANDOM_AMP
with 4 * SPEC_RANDOM_AMP * E_IX <= 1e-3: two fp32 evaluations whose coordinates are each within E_IX of the exact one, between
neighbours (or an edge value and the zero outside) that differ by at most 2 * SPEC_RANDOM_AMP.

LAYOUT.  f32 [B, n_mels, T] -> bf16 [B, T + 2, c_pad]: round to nearest even, bit for bit, rows 0 and T + 1 zero, channels from
n_mels upwards zero.
"""
import numpy as np

U = 2.0 ** -24
NFFT, HOP, NBIN, FPB = 400, 160, 201, 16

# ================================================================================================================ log-mel
D_LOG = 4 * 2.0 ** -20
D_OUT = 2.0 ** -22
WIDE = 1e-3
SHARE = 0.02
IDENTITY_SHARE = 0.02
SINGLE_BIN_SHARE = 0.125   # rows 1 and 2 of the six-row bank
SIX_ROW_SHARE = 0.04
LOGMEL_FRAMES = (3, 16, 37, 3000)
CLIP_KINDS = ("decades", "burst", "quiet", "silent", "tail")

_N = np.arange(NFFT)
_HANN = 0.5 - 0.5 * np.cos(2.0 * np.pi * _N / NFFT)
_KN = np.outer(_N, np.arange(NBIN)) % NFFT                  # exact periodic index of the twiddle
_COS, _SIN = np.cos(2.0 * np.pi * _KN / NFFT), np.sin(2.0 * np.pi * _KN / NFFT)


def clip(kind, n, seed):
    """f32 [n]: one clip of the named kind."""
    rng = np.random.default_rng(seed)
    if kind == "decades":
        x = rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 0.0, n)
    elif kind == "burst":
        x = 1e-4 * rng.standard_normal(n)
        m = min(800, n // 4)
        x[n // 2 - m // 2:n // 2 - m // 2 + m] = 0.5 * rng.standard_normal(m)
    elif kind == "quiet":
        x = 1e-3 * rng.standard_normal(n)
    elif kind == "silent":
        x = np.zeros(n)
    elif kind == "tail":
        x = np.zeros(n)
        x[n - 100:] = 0.5 * rng.standard_normal(100)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def clips(n_frames, seed=0):
    """f32 [5, 160 * n_frames]: the five kinds, in the order of CLIP_KINDS."""
    return np.stack([clip(kind, HOP * n_frames, 1000 * seed + 10 * n_frames + i) for i, kind in enumerate(CLIP_KINDS)])


def identity_bank():
    return np.eye(NBIN, dtype=np.float32)


def six_row_bank():
    """all zero | bin 0 only | bin 200 only | bins 3 and 150 | dense | last non-zero weight 1e-3 of the largest."""
    f = np.zeros((6, NBIN), dtype=np.float32)
    f[1, 0] = 0.02
    f[2, 200] = 0.02
    f[3, 3], f[3, 150] = 0.01, 0.015
    f[4] = 0.001 * (1 + np.arange(NBIN) % 7)
    f[5, 40:60] = 0.02
    f[5, 60] = 0.02e-3
    return f


def logmel_cases():
    """(n_frames, bank name): the model's banks at every frame count, the synthetic ones at 37 frames."""
    for n_frames in LOGMEL_FRAMES:
        for bank in ("mel80", "mel128"):
            yield n_frames, bank
    yield 37, "identity"
    yield 37, "six"


def banks(mel80, mel128):
    return {"mel80": np.asarray(mel80, dtype=np.float32), "mel128": np.asarray(mel128, dtype=np.float32), "identity": identity_bank(),
            "six": six_row_bank()}


def spectrum(x, n_frames):
    """float64: (S [F], Re [F, 201], Im [F, 201]) of one clip, from the definition."""
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 1 and x.shape[0] == HOP * n_frames and x.shape[0] > NFFT
    pad = np.pad(x, NFFT // 2, mode="reflect")
    fr = pad[np.arange(n_frames)[:, None] * HOP + _N[None, :]]
    xw = fr * _HANN
    return np.abs(xw).sum(axis=1), xw @ _COS, -(xw @ _SIN)


def logmel_interval(x, filt, n_frames):
    """One clip -> (ref, lo, hi), float64 [n_mels, n_frames]: the reference and the per-element interval of the module docstring."""
    S, re, im = spectrum(x, n_frames)
    F = np.asarray(filt, dtype=np.float64)
    e = (256.0 * U * S)[:, None]
    P = re * re + im * im
    dP = 2.0 * (np.abs(re) + np.abs(im)) * e + 2.0 * e * e + 4.0 * U * P
    M = F @ P.T
    dM = np.abs(F) @ dP.T + 32.0 * U * M
    lg = np.log10(np.maximum(M, 1e-10))
    lg_lo = np.log10(np.maximum(M - dM, 1e-10)) - D_LOG
    lg_hi = np.log10(np.maximum(M + dM, 1e-10)) + D_LOG
    ref = (np.maximum(lg, lg.max() - 8.0) + 4.0) / 4.0
    lo = (np.maximum(lg_lo, lg_lo.max() - 8.0) + 4.0) / 4.0 - D_OUT
    hi = (np.maximum(lg_hi, lg_hi.max() - 8.0) + 4.0) / 4.0 + D_OUT
    return ref, lo, hi


def logmel_intervals(xs, filt, n_frames):
    """A batch -> (ref, lo, hi), float64 [B, n_mels, n_frames]."""
    r = [logmel_interval(x, filt, n_frames) for x in xs]
    return tuple(np.stack([c[i] for c in r]) for i in range(3))


def misses(got, lo, hi):
    """How many elements lie outside [lo, hi] (a non-finite value always does)."""
    got = np.asarray(got, dtype=np.float64)
    return int((~((got >= lo) & (got <= hi))).sum())


def used_fraction(got, ref, lo, hi):
    """The largest share of its side of the interval that any element uses (1.0 = on the end)."""
    got = np.asarray(got, dtype=np.float64)
    up = np.where(got >= ref, (got - ref) / (hi - ref), (ref - got) / (ref - lo))
    return float(np.nan_to_num(up, nan=np.inf).max())


def wide_share(lo, hi):
    return float(((hi - lo) > WIDE).mean())


# ------------------------------------------------------------------------------------------------- the kernel, restated in fp32
LOGMEL_MUTANTS = ("hann_symmetric", "nyquist_dropped", "left_reflection_repeats_edge", "right_reflection_off_by_one", "far_end_clamped",
                  "max_shared_over_batch", "max_includes_frames_behind_the_end", "floor_1e-10_missing", "filter_range_drops_last_bin",
                  "filter_range_starts_at_second_bin", "floor_after_the_division")
f32 = np.float32


def _fma(a, b, c):
    """One rounding: the product of two f32 is exact in float64, the double rounding of the sum is far below every bound here."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def emulate_logmel(xs, filt, n_frames, form="fold", mutant=None):
    """f32 [B, 160 * n_frames], f32 [n_mels, 201] -> f32 [B, n_mels, n_frames], every step rounded to fp32.
    form: "seq" one unfused chain over the 400 samples per bin, a dense unfused filter sum; "fold" the folded DFT in fused chains
    and a fused filter sum (the kernel's order); "blas" fp32 matrix products (any order).  `mutant`: one of LOGMEL_MUTANTS."""
    assert mutant is None or mutant in LOGMEL_MUTANTS
    xs = np.asarray(xs)
    filt = np.asarray(filt)
    assert xs.dtype == f32 and filt.dtype == f32 and xs.ndim == 2 and xs.shape[1] == HOP * n_frames
    B, n = xs.shape
    nf = -(-n_frames // FPB) * FPB if mutant == "max_includes_frames_behind_the_end" else n_frames
    pos = np.arange(nf)[:, None] * HOP + _N[None, :] - NFFT // 2
    pos = np.where(pos < 0, -pos - 1 if mutant == "left_reflection_repeats_edge" else -pos, pos)
    far = {"right_reflection_off_by_one": 2 * n - 1 - pos, "far_end_clamped": np.full_like(pos, n - 1)}.get(mutant, 2 * (n - 1) - pos)
    pos = np.clip(np.where(pos >= n, far, pos), 0, n - 1)       # frames behind the clip's end read clamped samples
    cos32, sin32 = _COS.astype(f32), _SIN.astype(f32)           # [400, 201]: the table entry of k * n mod 400
    c1 = np.cos(2.0 * np.pi * _N / (NFFT - 1 if mutant == "hann_symmetric" else NFFT)).astype(f32)
    w = f32(0.5) - f32(0.5) * c1
    xw = (w[None, None, :] * xs[:, pos]).reshape(B * nf, NFFT)  # f32 [B * nf, 400]
    skip = mutant == "nyquist_dropped"
    if form == "seq":
        re = np.zeros((B * nf, NBIN), dtype=f32)
        im = np.zeros((B * nf, NBIN), dtype=f32)
        for i in range(NFFT):
            if skip and i == NFFT // 2:
                continue
            re = re + xw[:, i, None] * cos32[i][None, :]
            im = im - xw[:, i, None] * sin32[i][None, :]
        P = re * re + im * im
    elif form == "fold":
        s = xw[:, 1:200] + xw[:, :200:-1]
        d = xw[:, 1:200] - xw[:, :200:-1]
        re = np.repeat(xw[:, 0, None], NBIN, axis=1)
        im = np.zeros((B * nf, NBIN), dtype=f32)
        for i in range(1, 200):
            re = _fma(s[:, i - 1, None], cos32[i][None, :], re)
            im = _fma(d[:, i - 1, None], sin32[i][None, :], im)
        if not skip:
            re = _fma(xw[:, 200, None], cos32[200][None, :], re)
        P = _fma(re, re, im * im)
    else:
        assert form == "blas" and not skip
        re, im = xw @ cos32, xw @ sin32
        P = re * re + im * im
    fe = filt.copy()
    for m in range(fe.shape[0]):
        nz = np.flatnonzero(fe[m])
        if mutant == "filter_range_drops_last_bin" and nz.size:
            fe[m, nz[-1]] = 0
        if mutant == "filter_range_starts_at_second_bin" and nz.size:
            fe[m, nz[0]] = 0
    if form == "blas":
        M = P @ fe.T
    else:
        M = np.zeros((B * nf, fe.shape[0]), dtype=f32)
        for k in range(NBIN):
            if not fe[:, k].any():
                continue
            M = _fma(P[:, k, None], fe[None, :, k], M) if form == "fold" else M + P[:, k, None] * fe[None, :, k]
    with np.errstate(divide="ignore"):
        lg = np.log10(M if mutant == "floor_1e-10_missing" else np.maximum(M, f32(1e-10))).astype(f32)
    lg = lg.reshape(B, nf, -1).transpose(0, 2, 1)               # [B, n_mels, nf]
    mx = lg.max(axis=(1, 2), keepdims=True)                     # phantom frames take part only in their mutant (nf > n_frames)
    if mutant == "max_shared_over_batch":
        mx = np.full_like(mx, lg.max())
    lg = lg[:, :, :n_frames]
    with np.errstate(invalid="ignore"):
        if mutant == "floor_after_the_division":
            return np.maximum((lg + f32(4)) / f32(4), mx - f32(8)).astype(f32)
        return ((np.maximum(lg, mx - f32(8)) + f32(4)) / f32(4)).astype(f32)


# ================================================================================================================ SpecAugment
E_IX = 2.0 ** -8
IX_TABLE = {257: (4.1e-05, 4.4e-05), 300: (5.3e-05, 5.0e-05), 3000: (5.5e-04, 7.3e-04)}   # T -> (oracle's order, kernel's order)
SPEC_T = (2, 257, 300, 3000)
SPEC_B, SPEC_MELS = 3, 16
SPEC_RANDOM_AMP = 0.0625
assert 4 * SPEC_RANDOM_AMP * E_IX <= 1e-3
SPECAUG_MUTANTS = ("middle_slope_is_left_secant", "align_corners_false", "nearest_neighbour", "warp_of_clip_0_for_all",
                   "time_mask_before_warp", "inclusive_t1", "extremes_from_wrong_end")


def warp_W(T):
    """The largest W in {1, 5, 80} with a non-empty [W, T - W); None when there is none."""
    for W in (80, 5, 1):
        if W < T - W:
            return W
    return None


def warp_params(T):
    """The nine (warp_p, warp_d): warp_p in {W, middle, T - W - 1} x warp_d in {-W, 0, W - 1}."""
    W = warp_W(T)
    return [] if W is None else [(p, d) for p in (W, T // 2, T - W - 1) for d in (-W, 0, W - 1)]


def warp_ix64(T, wp, wd):
    """float64 [T]: the source coordinate of every output column."""
    L1 = T - 1.0
    y1 = (wp - wd) * 2.0 / L1 - 1.0
    sa, sb = (y1 + 1.0) / wp, (1.0 - y1) / (T - 1 - wp)
    mid = 0.5 * (sa + sb)
    t = np.arange(T, dtype=np.float64)
    seg0 = t <= wp
    xl, dx = np.where(seg0, 0.0, wp), np.where(seg0, wp, T - 1.0 - wp)
    yl, yr = np.where(seg0, -1.0, y1), np.where(seg0, y1, 1.0)
    ml, mr = np.where(seg0, sa, mid), np.where(seg0, mid, sb)
    v = (t - xl) / dx
    v2, v3 = v * v, v * v * v
    ys = (1 - 3 * v2 + 2 * v3) * yl + (v - 2 * v2 + v3) * ml * dx + (3 * v2 - 2 * v3) * yr + (v3 - v2) * mr * dx
    return (ys + 1.0) / 2.0 * L1


def warp_ix32(T, wp, wd, mutant=None):
    """f32 [T]: the same, every operation rounded to fp32, in the order the oracle forms it."""
    L1 = f32(T - 1)
    y1 = f32(2 * (wp - wd)) / L1 - f32(1)
    sa, sb = (y1 + f32(1)) / f32(wp), (f32(1) - y1) / f32(T - 1 - wp)
    mid = sa if mutant == "middle_slope_is_left_secant" else (sb + sa) / f32(2)
    t = np.arange(T, dtype=f32)
    seg0 = np.arange(T) <= wp
    xl, dx = np.where(seg0, f32(0), f32(wp)), np.where(seg0, f32(wp), f32(T - 1 - wp))
    yl, yr = np.where(seg0, f32(-1), y1), np.where(seg0, y1, f32(1))
    ml, mr = np.where(seg0, sa, mid), np.where(seg0, mid, sb)
    v = (t - xl) / dx
    v2 = v * v
    v3 = v2 * v
    h0 = f32(1) - f32(3) * v2 + f32(2) * v3
    h1 = v - f32(2) * v2 + v3
    h2 = f32(3) * v2 - f32(2) * v3
    h3 = -v2 + v3
    ys = h0 * yl + h1 * ml * dx + h2 * yr + h3 * mr * dx
    assert ys.dtype == f32
    if mutant == "align_corners_false":
        return ((ys + f32(1)) * f32(T) - f32(1)) / f32(2)
    return (ys + f32(1)) * f32(0.5) * L1


def ramp_coeffs(clip_no):
    """(a, b) float64 [16]: small dyadic slopes and offsets, different in every row and every clip."""
    m = np.arange(SPEC_MELS)
    a = (m + 1 + SPEC_MELS * clip_no) / 16.0 * np.where(m % 2 == 0, 1.0, -1.0)
    b = ((7 * m + 11 * clip_no) % 32 - 15.5) / 4.0
    return a, b


def ramps(T, first_clip=0):
    """f32 [3, 16, T]: row m of clip c is a_m * t + b_m, exact in fp32."""
    out = np.stack([ramp_coeffs(first_clip + c)[0][:, None] * np.arange(T)[None, :] + ramp_coeffs(first_clip + c)[1][:, None] for c in range(SPEC_B)])
    assert (out.astype(f32).astype(np.float64) == out).all()
    return out.astype(f32)


def specaug_batches(T):
    """-> list of (params i32 [3, 8], extremes i32 [3, 2]).  One clip of every batch is unwarped (its place moves from batch to batch);
    clip 0: a time mask across a multiple of 256 (250 .. 262 where T allows) and extremes (2, 3); clip 1: an empty time mask and the
    frequency mask rows 3 .. 9; clip 2: no mask at all.  The two warped clips walk through the nine (warp_p, warp_d)."""
    combos = warp_params(T)
    t_mask = (250, min(262, T)) if T > 250 else (T // 2, T)
    masks = [(t_mask, (0, 0), (2, 3)), ((min(40, T - 1),) * 2, (3, 9), (0, 0)), ((0, 0), (0, 0), (0, 0))]
    n_batches = 5 if combos else 1
    out, c = [], 0
    for i in range(n_batches):
        params = np.zeros((SPEC_B, 8), dtype=np.int32)
        ext = np.zeros((SPEC_B, 2), dtype=np.int32)
        for b in range(SPEC_B):
            (t0, t1), (f0, f1), ex = masks[b]
            params[b, 3:7] = t0, t1, f0, f1
            ext[b] = ex
            if combos and b != i % SPEC_B:
                params[b, 0:3] = (1,) + combos[c % len(combos)]
                c += 1
        out.append((params, ext))
    assert not combos or c >= len(combos)
    return out


def random_spectrogram(T):
    """f32 [3, 16, T], uniform in +-SPEC_RANDOM_AMP: the gather itself, judged against the oracle at 1e-3."""
    return (SPEC_RANDOM_AMP * np.random.default_rng(T).uniform(-1.0, 1.0, (SPEC_B, SPEC_MELS, T))).astype(f32)


def _masked(n_mels, T, pr, ex):
    t, m = np.arange(T)[None, :], np.arange(n_mels)[:, None]
    return ((t >= pr[3]) & (t < pr[4])) | ((m >= pr[5]) & (m < pr[6])) | (m < ex[0]) | (m >= n_mels - ex[1])


def specaug_expected(x, params, ext):
    """Ramp input f32 [B, n_mels, T] -> (want, bound) float64 of the same shape.  A bound of 0 asks for the exact value."""
    x = np.asarray(x, dtype=np.float64)
    B, n_mels, T = x.shape
    want, bound = x.copy(), np.zeros_like(x)
    for b in range(B):
        pr, ex = params[b], ext[b]
        row = x[b]
        a = row[:, 1] - row[:, 0]
        if pr[0]:
            ix = warp_ix64(T, int(pr[1]), int(pr[2]))
            x0 = np.floor(ix).astype(np.int64)
            w1 = ix - x0
            take = lambda j: np.where((j >= 0) & (j < T), row[:, np.clip(j, 0, T - 1)], 0.0)  # noqa: E731
            want[b] = take(x0) * (1.0 - w1) + take(x0 + 1) * w1
            left = (ix - E_IX < 0) & (np.arange(T) != 0)               # column 0 is exact
            right = ix + E_IX > T - 1
            gone = (ix + E_IX <= -1) | (ix - E_IX >= T)                # both neighbours outside, whatever the rounding
            bound[b] = (np.abs(a)[:, None] + left[None, :] * np.abs(row[:, :1]) + right[None, :] * np.abs(row[:, -1:])) * E_IX \
                + 4 * U * np.abs(row).max(axis=1, keepdims=True)
            bound[b][:, gone] = 0.0
        dead = _masked(n_mels, T, pr, ex)
        want[b][dead] = 0.0
        bound[b][dead] = 0.0
    return want, bound


def violations(got, want, bound):
    got = np.asarray(got, dtype=np.float64)
    return int((~(np.abs(got - want) <= bound)).sum())


def emulate_specaug(x, params, ext, mutant=None):
    """The kernel in numpy fp32: f32 [B, n_mels, T] -> f32 of the same shape.  `mutant`: one of SPECAUG_MUTANTS."""
    assert mutant is None or mutant in SPECAUG_MUTANTS
    x = np.asarray(x)
    assert x.dtype == f32
    B, n_mels, T = x.shape
    out = np.empty_like(x)
    for b in range(B):
        pr = params[0 if mutant == "warp_of_clip_0_for_all" else b]
        row = x[b].copy()
        msk = params[b].copy()
        if mutant == "inclusive_t1":
            msk[4] += 1
        ex = ext[b][::-1] if mutant == "extremes_from_wrong_end" else ext[b]
        if mutant == "time_mask_before_warp":
            row[:, msk[3]:msk[4]] = 0
        if pr[0]:
            ix = warp_ix32(T, int(pr[1]), int(pr[2]), mutant)
            if mutant == "nearest_neighbour":
                j = np.rint(ix).astype(np.int64)
                v = np.where((j >= 0) & (j < T), row[:, np.clip(j, 0, T - 1)], f32(0))
            else:
                fx = np.floor(ix)
                x0 = fx.astype(np.int64)
                w1 = ix - fx
                w0 = f32(1) - w1
                take = lambda j: np.where((j >= 0) & (j < T), row[:, np.clip(j, 0, T - 1)], f32(0))  # noqa: E731
                v = take(x0) * w0 + take(x0 + 1) * w1
        else:
            v = row
        v = v.astype(f32)
        v[_masked(n_mels, T, msk, ex)] = 0
        out[b] = v
    return out


# ================================================================================================================ layout
LAYOUT_SHAPES = ((2, 80, 300, 128), (1, 128, 65, 128), (3, 16, 1, 128), (1, 80, 64, 96), (2, 5, 63, 8))   # (B, n_mels, T, c_pad)
LAYOUT_MUTANTS = ("truncation", "halo_row_T_plus_1_not_written", "pad_channels_not_written")
POISON_BF16 = 0x7FC1
# exact ties (even mantissa: down to 0x3F80 / odd: up to 0x3F82, and their negatives), a tie in the last binade, the largest finite
# bf16, +0 and -0
_SPECIAL_BITS = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x7F7E8000, 0x7F7F0000, 0xFF7F0000, 0x00000000, 0x80000000],
                         dtype=np.uint32)


def layout_input(B, n_mels, T, seed=0):
    """f32 [B, n_mels, T]: normal samples over six decades, with the special values spread over the front of every clip."""
    rng = np.random.default_rng(seed + 7 * T + n_mels)
    x = (rng.standard_normal((B, n_mels, T)) * 10.0 ** rng.uniform(-3.0, 3.0, (B, n_mels, T))).astype(f32)
    flat = x.reshape(B, -1)
    at = (np.arange(_SPECIAL_BITS.shape[0]) * 5) % flat.shape[1]
    assert np.unique(at).shape[0] == at.shape[0]
    flat[:, at] = _SPECIAL_BITS.view(f32)
    return x


def bf16_rne(x):
    """f32 -> the bits of its bf16, round to nearest even (finite input)."""
    bits = np.asarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def layout_expected(x, c_pad, mutant=None):
    """uint16 [B, T + 2, c_pad]: the expected bits; with a `mutant` (LAYOUT_MUTANTS), what that wrong kernel leaves in poisoned memory."""
    assert mutant is None or mutant in LAYOUT_MUTANTS
    B, n_mels, T = x.shape
    out = np.full((B, T + 2, c_pad), POISON_BF16, dtype=np.uint16)
    out[:, 0] = 0
    if mutant != "halo_row_T_plus_1_not_written":
        out[:, T + 1] = 0
    if mutant != "pad_channels_not_written":
        out[:, 1:T + 1, n_mels:] = 0
    bits = (x.view(np.uint32) >> 16).astype(np.uint16) if mutant == "truncation" else bf16_rne(x)
    out[:, 1:T + 1, :n_mels] = bits.transpose(0, 2, 1)
    return out


MUTANTS = LOGMEL_MUTANTS + SPECAUG_MUTANTS + LAYOUT_MUTANTS
