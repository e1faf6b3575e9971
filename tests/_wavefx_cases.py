"""Test helper for the wave effects (include/wft.h "Wave effects", csrc/wavefx.hip): references, bounds, cases.  No GPU, no engine.

References.  Every stage restated in numpy / Python fp64 from the header's words, one row at a time:
  ref_noise / ref_clip / ref_level (row, n, rec, n_max, mut=None) -> Expect(val f64 [n_max], exact bool [n_max], mag f64 [n_max], K)
`row` is the INPUT BUFFER row (poisoned at and behind n), so that a defect that reads past the row shows.  An element with
exact[i] is compared bit for bit against f32(val[i]) (the sign of zero included); any other element under
    |got - val| <= half_ulp32(val) + K * 2^-53 * mag
half_ulp32(v) = 2^(floor(log2 |v|) - 24), at least 2^-150: half the f32 spacing of v's binade, which a correctly rounded f32(v)
cannot exceed.  `mut` switches in ONE defect (MUTANTS); tests/test_wavefx_host.py shows that `violations` rejects each of them.

The counts K (u = 2^-53, the unit roundoff; "1 ulp" functions cost 2 u; the kernel runs with FMA contraction off, so it performs the
operations written in the header; every count is taken for the kernel AND for this reference, which err independently):
  z(i):  ln u1 2 u (u1 is exact); -2 * exact; sqrt halves it and adds 1 u: r within 2 u.  t = (2 pi) u2: 1 u relative, at most
         2 pi u absolute, which moves cos / sin by at most 2 pi u; cos / sin themselves 4 u (2 ulp); r * cos: 1 u.  Against |z| that is
         (2 + 2 pi + 4 + 1) u < 14 u wherever |cos| is not small; near a zero of the cosine the 2 pi u r term is absolute and exceeds
         14 u |z|, but there |sigma z| itself is far below the f32 half ulp of any x of comparable size, and the half-ulp term carries it.
  NOISE: sigma * z 1 u, x + . 1 u: 16 u per side, K = 32 for gaussian_noise.
  sigma of gaussian_snr, kernel: a thread adds up to 16 exact squares (15 u), the tree has 8 levels (8 u), C = ceil(n / 4096) chunk
         sums are added in order (C - 1 u): the sum within (22 + C) u; / n 1 u; sqrt halves and adds 1 u; snr / 20 1 u relative, which
         10^y turns into ln(10) |snr| / 20 u = 0.115 |snr| u; 10^y 2 u; the division 1 u: (22 + C) / 2 + 5 + 0.115 |snr|.  Reference:
         math.fsum is correctly rounded (1 u), then the same chain: 6 + 0.115 |snr|.  K = 32 + ceil((22 + C) / 2 + 11 + 0.23 |snr|).
  gain_transition: (i - t0) exact; / D 1 u; end - start 1 u; * 1 u; start + 1 u: dB within (3 |end - start| + M) u, M = max(|start|,
         |end|) >= |dB|; / 20 1 u of |dB| / 20: y = dB / 20 within (3 |end - start| + 2 M) u / 20, which 10^y turns into a relative
         0.115 (3 |end - start| + 2 M) u; 10^y 2 u; x * . 1 u.  K = 6 + ceil(0.23 (3 |end - start| + 2 M)), mag = |val|.
  shift, faded: d / D 1 u, x * w 1 u: K = 4, mag = |val|.
Bit for bit (no bound): gain (one f32 multiply), clipping and its two thresholds, the unfaded samples of shift, pass-through rows,
the zero fill.
"""
import math
from dataclasses import dataclass

import numpy as np

from tests import _sample_oracle as SO
from whisper_finetune.data import wave_fx as WF

U = 2.0 ** -53
TWO_PI = 6.283185307179586
CHUNK = 4096  # samples per chunk of the statistics / selection passes (the header states it for the RMS order)
SENTINEL = np.float32(-7.5e8)
MUTANTS = ("rms_drops_last", "rms_reads_past_n", "snr_inverted", "counter_shift_1", "cos_sin_swapped", "seed_halves_swapped",
           "percentile_uses_n", "j_off_by_one", "upper_percent_minus_1", "lo_hi_swapped", "transition_linear_amplitude", "shift_sign_flipped",
           "fade_one_short", "no_zero_fill")
MUTANT_STAGE = {"rms_drops_last": "noise", "rms_reads_past_n": "noise", "snr_inverted": "noise", "counter_shift_1": "noise",
                "cos_sin_swapped": "noise", "seed_halves_swapped": "noise", "percentile_uses_n": "clip", "j_off_by_one": "clip",
                "upper_percent_minus_1": "clip", "lo_hi_swapped": "clip", "transition_linear_amplitude": "level",
                "shift_sign_flipped": "level", "fade_one_short": "level", "no_zero_fill": "any"}


@dataclass
class Expect:
    val: np.ndarray    # f64 [n_max]
    exact: np.ndarray  # bool [n_max]
    mag: np.ndarray    # f64 [n_max]
    K: float
    thr: tuple = None  # (lo, hi) f32 of a clipping row


def half_ulp32(v):
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, np.maximum(2.0 ** (e - 24), 2.0 ** -150), 2.0 ** -150)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def violations(got, exp: Expect) -> int:
    """The number of elements of the f32 row `got` [n_max] that `exp` rejects: THE comparison of the GPU tests and of the mutants."""
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == exp.val.shape
    bad_exact = exp.exact & (bits(got) != bits(exp.val.astype(np.float32)))
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got.astype(np.float64) - exp.val)
        tol = half_ulp32(exp.val) + exp.K * U * exp.mag
        bad_tol = ~exp.exact & ~(err <= tol)  # (a NaN fails)
    return int(bad_exact.sum() + bad_tol.sum())


def _passthrough(row, n, n_max, mut=None) -> Expect:
    val32 = np.zeros(n_max, dtype=np.float32)
    val32[:n] = row[:n]
    e = Expect(val32.astype(np.float64), np.ones(n_max, dtype=bool), np.zeros(n_max), 0.0)  # (f64 keeps the sign of a zero)
    return _fill(e, row, n, n_max, mut)


def _fill(e: Expect, row, n, n_max, mut):
    """The zero fill behind n (exact); mutant: the input's samples are left there."""
    e.val[n:] = 0.0
    e.exact[n:] = True
    e.mag[n:] = 0.0
    if mut == "no_zero_fill":
        e.val[n:] = row[n:n_max].astype(np.float64)
    return e


# ------------------------------------------------------------------------------------------------------------------ NOISE
def philox_known_answers():
    a = SO.philox4x32_10(np.zeros(4, dtype=np.uint64), np.zeros(2, dtype=np.uint64))
    b = SO.philox4x32_10(np.full(4, 0xFFFFFFFF, dtype=np.uint64), np.full(2, 0xFFFFFFFF, dtype=np.uint64))
    return [int(v) for v in a], [int(v) for v in b]


def normals(seed: int, idx, mut=None):
    """z(i) and r(i) in fp64 for the sample indices `idx`."""
    idx = np.asarray(idx, dtype=np.int64)
    ctr = np.zeros((len(idx), 4), dtype=np.uint64)
    ctr[:, 0] = (idx >> 1) if mut == "counter_shift_1" else (idx >> 2)
    lo, hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    if mut == "seed_halves_swapped":
        lo, hi = hi, lo
    key = np.broadcast_to(np.array([lo, hi], dtype=np.uint64), (len(idx), 2))
    w = SO.philox4x32_10(ctr, key)
    sel = 2 * ((idx >> 1) & 1)
    rows = np.arange(len(idx))
    u1 = (2.0 * (w[rows, sel] >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (2.0 * (w[rows, sel + 1] >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    t = TWO_PI * u2
    even = (idx & 1) == 0
    if mut == "cos_sin_swapped":
        even = ~even
    return r * np.where(even, np.cos(t), np.sin(t)), r


def sigma_of(row, n, rec, mut=None):
    """(sigma, K_sigma) of a noise row."""
    if int(rec["noise_kind"]) == 1:
        return float(rec["noise_value"]), 0.0
    hi = n - 1 if mut == "rms_drops_last" else (n + 1 if mut == "rms_reads_past_n" else n)
    if n == 0:
        return 0.0, 0.0
    total = math.fsum(float(v) * float(v) for v in row[:max(hi, 0)].astype(np.float64))
    if not total > 0.0:
        return (float("nan") if math.isnan(total) else 0.0), 0.0
    rms = math.sqrt(total / n)
    snr = float(rec["noise_value"])
    sg = rms * 10.0 ** (snr / 20.0) if mut == "snr_inverted" else rms / 10.0 ** (snr / 20.0)
    C = -(-n // CHUNK)
    return sg, math.ceil((22 + C) / 2 + 11 + 0.23 * abs(snr))


def ref_noise(row, n, rec, n_max, mut=None) -> Expect:
    if int(rec["noise_kind"]) == 0:
        return _passthrough(row, n, n_max, mut)
    sg, k_sigma = sigma_of(row, n, rec, mut)
    if sg == 0.0:
        return _passthrough(row, n, n_max, mut)
    z, _ = normals(int(rec["seed"]), np.arange(n), mut)
    x = row[:n].astype(np.float64)
    val = np.zeros(n_max)
    mag = np.zeros(n_max)
    val[:n] = x + sg * z
    mag[:n] = np.abs(x) + np.abs(sg * z)
    return _fill(Expect(val, np.zeros(n_max, dtype=bool), mag, 32.0 + k_sigma), row, n, n_max, mut)


# ------------------------------------------------------------------------------------------------------------------ CLIP
def okey(x32):
    u = bits(x32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> np.uint32(31), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def thresholds(x32, q: int, mut=None):
    """(lo, hi) f32 of the row x32 (n >= 1 samples): the percentiles q and 100 - q, by sorting the u32 keys."""
    n = len(x32)
    s = unkey(np.sort(okey(x32)))
    out = []
    for which, p in enumerate((q, 100 - q)):
        if mut == "upper_percent_minus_1" and which == 1:
            p -= 1
        m = p * (n if mut == "percentile_uses_n" else n - 1)
        j, r = m // 100, m % 100
        if mut == "j_off_by_one":
            j += 1
        j = min(j, n - 1)
        if r == 0 or j + 1 > n - 1:
            out.append(np.float32(s[j]))
        else:
            out.append(np.float32(np.float64(s[j]) + (r / 100.0) * (np.float64(s[j + 1]) - np.float64(s[j]))))
    if mut == "lo_hi_swapped":
        out = out[::-1]
    return out[0], out[1]


def ref_clip(row, n, rec, n_max, mut=None) -> Expect:
    if int(rec["clip_kind"]) == 0 or n == 0:
        return _passthrough(row, n, n_max, mut)
    x = row[:n].copy()
    lo, hi = thresholds(x, int(rec["clip_q"]), mut)
    with np.errstate(invalid="ignore"):
        y = np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(np.float32)
    e = _passthrough(np.concatenate([y, row[n:]]), n, n_max, mut)
    e.thr = (lo, hi)
    return e


# ------------------------------------------------------------------------------------------------------------------ LEVEL
def shift_places(fraction: float, n: int, mut=None) -> int:
    if n == 0:
        return 0
    s = int(np.rint(np.float64(fraction) * np.float64(n)))  # ties to even
    if mut == "shift_sign_flipped":
        s = -s
    return s % n


def ref_level(row, n, rec, n_max, mut=None) -> Expect:
    kind = int(rec["level_kind"])
    if kind == 0 or n == 0:
        return _passthrough(row, n, n_max, mut)
    x32 = row[:n].copy()
    if kind == 1:
        return _passthrough(np.concatenate([(x32 * np.float32(rec["gain_ratio"])).astype(np.float32), row[n:]]), n, n_max, mut)
    x = x32.astype(np.float64)
    if kind == 2:
        d0, d1 = float(rec["db_start"]), float(rec["db_end"])
        den = float(max(int(rec["ramp_len"]) - 1, 1))
        u = np.minimum(np.maximum((np.arange(n, dtype=np.int64) - int(rec["t0"])).astype(np.float64) / den, 0.0), 1.0)
        if mut == "transition_linear_amplitude":
            a0, a1 = 10.0 ** (d0 / 20.0), 10.0 ** (d1 / 20.0)
            g = a0 + (a1 - a0) * u
        else:
            g = np.power(10.0, (d0 + (d1 - d0) * u) / 20.0)
        val = np.zeros(n_max)
        val[:n] = x * g
        K = 6 + math.ceil(0.23 * (3 * abs(d1 - d0) + 2 * max(abs(d0), abs(d1))))
        return _fill(Expect(val, np.zeros(n_max, dtype=bool), np.abs(val).copy(), float(K)), row, n, n_max, mut)
    s = shift_places(float(rec["shift_fraction"]), n, mut)
    F = min(max(int(rec["fade_len"]), 0), n // 2)
    if s == 0:
        F = 0
    i = np.arange(n, dtype=np.int64)
    d = (i - s) % n
    e = n - 1 - d
    D = float(max(F - 1, 1))
    Fm = F - 1 if (mut == "fade_one_short" and F > 0) else F
    w = np.ones(n)
    w = np.where(d < Fm, d / D, np.where(e < Fm, e / D, w))
    faded = (d < Fm) | (e < Fm)
    val = np.zeros(n_max)
    val[:n] = np.where(faded, x[d] * w, x32[d].astype(np.float64))
    exact = np.ones(n_max, dtype=bool)
    exact[:n] = ~faded
    return _fill(Expect(val, exact, np.abs(val).copy(), 4.0), row, n, n_max, mut)


REF = {"noise": ref_noise, "clip": ref_clip, "level": ref_level}


# ------------------------------------------------------------------------------------------------------------------ cases
def lengths(T: int):
    """The row lengths of every batch: the seams of the apply pass's trip T and one row over several chunks of the statistic passes."""
    return [0, 1, 2, 3, T - 1, T, T + 1, 3 * T + 5, 4 * CHUNK + 37]


def layout(T: int, pad: int = 3):
    """(n list, n_max, ld): n_max > every n and a multiple of 4; ld > n_max (pad 3: rows after the first are not 16-byte aligned, the
    scalar path; pad 4: every row is, the 16-byte path)."""
    ns = lengths(T)
    n_max = (max(ns) + 59) // 4 * 4
    return ns, n_max, n_max + pad


def signal(n: int, seed: int, kind: str = "speech") -> np.ndarray:
    """One row's samples f32 [n].  The selection inputs: `equal`, `zeros80` (a short clip in its padding), `signed_zeros`,
    `denormals`, `negative`, `sawtooth` (every value distinct)."""
    g = np.random.default_rng(seed)
    if kind == "speech":
        x = (g.standard_normal(n) * 0.1).astype(np.float32)
    elif kind == "equal":
        x = np.full(n, 0.25, dtype=np.float32)
    elif kind == "zeros80":
        x = (g.standard_normal(n) * 0.1).astype(np.float32)
        x[n // 5:] = 0.0
    elif kind == "signed_zeros":
        x = np.where(g.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        x[::7] = (g.standard_normal(len(x[::7])) * 0.01).astype(np.float32)
    elif kind == "denormals":
        x = (g.integers(-2000, 2000, n).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    elif kind == "negative":
        x = (-np.abs(g.standard_normal(n)) * 0.1 - 1e-3).astype(np.float32)
    elif kind == "sawtooth":
        x = ((g.permutation(n).astype(np.float64) - n / 2) / max(n, 1)).astype(np.float32)
    else:
        raise ValueError(kind)
    return x


SELECTION_INPUTS = ("equal", "zeros80", "signed_zeros", "denormals", "negative", "sawtooth")
CLIP_Q = (0, 1, 20, 50)


def poisoned_batch(ns, n_max, ld, seed: int, kind: str = "speech") -> np.ndarray:
    """f32 [B, ld]: row b holds signal(ns[b]) and is poisoned at and behind ns[b] (1e30, then NaN), also behind n_max."""
    buf = np.full((len(ns), ld), np.nan, dtype=np.float32)
    for b, n in enumerate(ns):
        buf[b, :n] = signal(n, seed * 1000 + b, kind)
        buf[b, n:n + 2] = 1e30
    return buf


def records(B: int):
    return WF.records_from_table(WF.none_table(B))


def set_row(rec, b: int, kind: str, **params):
    """Write one effect into row b of the records (the other stages of the row stay as they are)."""
    one = WF.records_from_table(WF.table_row(kind, **params)[None])[0]
    stage = WF.STAGE_OF[kind]
    fields = {"noise": ("noise_kind", "noise_value", "seed"), "clip": ("clip_kind", "clip_q"),
              "level": ("level_kind", "gain_ratio", "db_start", "db_end", "t0", "ramp_len", "shift_fraction", "fade_len")}[stage]
    for f in fields:
        rec[f][b] = one[f]
    return rec


def expected_buffer(buf_in, ns, n_max, rec, stage: str, mut=None):
    """[Expect per row] for one stage over a poisoned batch."""
    return [REF[stage](buf_in[b], ns[b], rec[b], n_max, mut) for b in range(len(ns))]


def stage_cases(T: int):
    """{name: (stage, input kind, fill(rec, ns) -> rec)}: every kind over the row lengths, with its parameter corners (a shift by 0, by n, by one sample; a ramp before, after and across the row; sigma and rms of 0)."""
    ns = lengths(T)
    B = len(ns)

    def all_rows(kind, **params):
        def fill(rec):
            for b in range(B):
                p = {k: (v(b, ns[b]) if callable(v) else v) for k, v in params.items()}
                set_row(rec, b, kind, **p)
            return rec
        return fill

    cases = {
        "gaussian_noise": ("noise", "speech", all_rows("gaussian_noise", amplitude=0.01, seed=lambda b, n: 0x1234567890ABCDEF + b)),
        "gaussian_noise_sigma0": ("noise", "speech", all_rows("gaussian_noise", amplitude=0.0, seed=7)),
        "gaussian_snr": ("noise", "speech", all_rows("gaussian_snr", snr_db=lambda b, n: 5.0 + 4.0 * b, seed=lambda b, n: (b << 40) + 99)),
        "gaussian_snr_rms0": ("noise", "zeros_all", all_rows("gaussian_snr", snr_db=10.0, seed=5)),
        "gain": ("level", "speech", all_rows("gain", gain_db=lambda b, n: -6.0 + 1.5 * b)),
        "transition_inside": ("level", "speech", all_rows("gain_transition", start_db=-24.0, end_db=6.0, t0=lambda b, n: n // 3,
                                                         length=lambda b, n: max(n // 2, 1))),
        "transition_straddles": ("level", "speech", all_rows("gain_transition", start_db=3.0, end_db=-12.0, t0=lambda b, n: -(n // 2) - 1,
                                                            length=lambda b, n: 2 * n + 3)),
        "transition_before": ("level", "speech", all_rows("gain_transition", start_db=-5.0, end_db=4.0, t0=-5000, length=100)),
        "transition_after": ("level", "speech", all_rows("gain_transition", start_db=-5.0, end_db=4.0, t0=lambda b, n: n + 10, length=100)),
        "transition_len1": ("level", "speech", all_rows("gain_transition", start_db=-5.0, end_db=4.0, t0=lambda b, n: n // 2, length=1)),
        "shift_fade": ("level", "speech", all_rows("shift", fraction=0.3, fade_len=80)),
        "shift_negative": ("level", "speech", all_rows("shift", fraction=-0.41, fade_len=7)),
        "shift_zero": ("level", "speech", all_rows("shift", fraction=0.0, fade_len=80)),
        "shift_full": ("level", "speech", all_rows("shift", fraction=1.0, fade_len=80)),
        "shift_minus_one_sample": ("level", "speech", all_rows("shift", fraction=lambda b, n: -1.0 / max(n, 1), fade_len=2)),
        "shift_no_fade": ("level", "speech", all_rows("shift", fraction=0.25, fade_len=0)),
        "shift_fade_clamped": ("level", "speech", all_rows("shift", fraction=0.5, fade_len=1 << 30)),
        "shift_tie": ("level", "signed_zeros", all_rows("shift", fraction=0.5, fade_len=1)),
    }
    for kind in SELECTION_INPUTS:
        for q in CLIP_Q:
            cases[f"clip_{kind}_q{q}"] = ("clip", kind, all_rows("clipping", q=q))
    # ranks where g = 0 and j + 1 would be index n: q = 50 with n - 1 even puts both percentiles on one sample; q = 0 puts the upper
    # one on the last sample (j = n - 1); both are in the table above for every length.  One more with q chosen per row so that
    # q (n - 1) is a multiple of 100 where the length allows it.
    cases["clip_exact_ranks"] = ("clip", "sawtooth", all_rows("clipping", q=lambda b, n: 25 if (n - 1) % 4 == 0 else 50))
    return cases


def case_input(ns, n_max, ld, name: str, kind: str):
    seed = sum(ord(c) for c in name)
    if kind == "zeros_all":
        buf = poisoned_batch(ns, n_max, ld, seed)
        for b, n in enumerate(ns):
            buf[b, :n] = 0.0
            if n > 1:
                buf[b, 1] = -0.0
        return buf
    return poisoned_batch(ns, n_max, ld, seed, kind)
