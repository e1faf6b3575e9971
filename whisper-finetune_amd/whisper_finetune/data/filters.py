"""Filter augmentation, host side: the designs and the draws of the seven IIR filters of the reference's advanced audio pipeline
(model/augment.py: LowPass, HighPass, BandPass, BandStop, LowShelf, HighShelf and Peaking filters under one OneOf(p=0.6)).

Pure numpy float64; scipy is not a dependency.  Every design is a cascade of second-order sections `sos` f64 [S, 6] = b0 b1 b2 a0 a1 a2
with a0 normalised to 1, the form `wft_sos_filter_f32` (include/wft.h "IIR filter") and scipy.signal.sosfilt take.

Section counts (every form fits the kernel's S <= 4):
  low_pass, high_pass   Butterworth of order N in 1..4 by the bilinear transform with prewarping: ceil(N / 2) sections (conjugate pole
                        pairs in ascending Q, the real pole of an odd order last).
  band_pass             the two-edge construction: a high-pass of order N at the lower edge FOLLOWED BY (cascade) a low-pass of order N
                        at the upper edge: 2 ceil(N / 2) sections = 2, 2, 4, 4 for N = 1..4.
  band_stop             the same two edge filters the other way round, a low-pass of order N at the lower edge and a high-pass of order N
                        at the upper edge, combined by their SUM (in parallel: what either lets through passes, the band between the
                        edges is stopped; their cascade would pass nothing).  The sum LP + HP = (B_lp A_hp + B_hp A_lp) / (A_lp A_hp)
                        has 2 N poles, the union of both; its numerator is factored into quadratics with numpy.roots in the analog
                        variable of the bilinear transform, where its roots are well separated: N sections.
  low_shelf, high_shelf, peaking   the audio-EQ-cookbook biquads (centre frequency, gain in dB, Q): one section.
audiomentations is not installed here: the construction and the default ranges below are restated from its published source, and
parity with its binary is unpinned.  This is the filter group of the advanced pipeline, not `apply_advanced_aug`.
"""
from __future__ import annotations

import math
import random
from typing import Mapping, Optional

import numpy as np

KINDS = ("low_pass", "high_pass", "band_pass", "band_stop", "low_shelf", "high_shelf", "peaking")
MAX_SECTIONS = 4
IDENTITY_SECTION = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def identity_sos(S: int = MAX_SECTIONS) -> np.ndarray:
    return np.tile(np.asarray(IDENTITY_SECTION, dtype=np.float64), (S, 1))


def _check_freq(f, sample_rate, what):
    f = float(f)
    if not (math.isfinite(f) and 0.0 < f < sample_rate / 2.0):
        raise ValueError(f"{what} must lie inside (0, {sample_rate / 2.0}) Hz, got {f}")
    return f


def _check_order(order):
    if isinstance(order, bool) or int(order) != order or not 1 <= int(order) <= 4:
        raise ValueError(f"order must be an integer in 1..4, got {order!r}")
    return int(order)


def _butter(kind: str, order: int, freq: float, sample_rate: float) -> np.ndarray:
    """Butterworth low-/high-pass, bilinear transform s = (1 - z^-1) / (K (1 + z^-1)) with K = tan(pi f / fs) (prewarped)."""
    K = math.tan(math.pi * freq / sample_rate)
    hp = kind == "high_pass"
    out = []
    for k in range(order // 2):  # the pair with damping 1/q = 2 sin(pi (2 k + 1) / (2 N)): s^2 + s / q + 1
        d = 2.0 * math.sin(math.pi * (2 * k + 1) / (2.0 * order))
        norm = 1.0 / (1.0 + K * d + K * K)
        b0 = norm if hp else K * K * norm
        out.append((d, [b0, (-2.0 if hp else 2.0) * b0, b0, 1.0, 2.0 * (K * K - 1.0) * norm, (1.0 - K * d + K * K) * norm]))
    out.sort(key=lambda t: -t[0])  # ascending Q
    sos = [s for _, s in out]
    if order % 2:  # s + 1
        norm = 1.0 / (K + 1.0)
        b0 = norm if hp else K * norm
        sos.append([b0, -b0 if hp else b0, 0.0, 1.0, (K - 1.0) * norm, 0.0])
    return np.asarray(sos, dtype=np.float64)


def _analog_quads(order: int, K: float):
    """The Butterworth denominator with cutoff K in the variable of the bilinear map, as monic quadratics [1, c1, c0] and, for an odd
    order, one monic linear factor [1, c0]."""
    quads = [[1.0, 2.0 * math.sin(math.pi * (2 * k + 1) / (2.0 * order)) * K, K * K] for k in range(order // 2)]
    return quads, ([1.0, K] if order % 2 else None)


def _band_stop(order: int, lo: float, hi: float, sample_rate: float) -> np.ndarray:
    """LP(lo) + HP(hi) as ONE cascade.  In the analog variable s = (1 - z^-1) / (1 + z^-1), with K = tan(pi f / fs):
    K1^N / D1(s) + s^N / D2(s) = P(s) / (D1(s) D2(s)), P = K1^N D2 + s^N D1, monic of degree 2 N.  P is factored there (numpy.roots on
    the variable s / sqrt(K1 K2): the roots spread over the two edges' scales and are well separated, where the roots in z crowd
    around +-1), every quadratic is mapped by itself: s^2 + c1 s + c0 -> (1 + c1 + c0) + 2 (c0 - 1) z^-1 + (1 - c1 + c0) z^-2."""
    K1, K2 = math.tan(math.pi * lo / sample_rate), math.tan(math.pi * hi / sample_rate)
    g = math.sqrt(K1 * K2)

    def scaled(K):  # the denominator in u = s / g, monic
        quads, lin = _analog_quads(order, K / g)
        p = np.ones(1)
        for q in quads:
            p = np.convolve(p, q)
        return np.convolve(p, lin) if lin else p

    D1, D2 = scaled(K1), scaled(K2)
    P = np.polyadd((K1 / g) ** order * D2, np.convolve(np.concatenate([[1.0], np.zeros(order)]), D1))
    roots = np.roots(P) * g
    tol = 1e-9
    cplx = [r for r in roots if r.imag > tol * abs(r)]
    real = sorted((r.real for r in roots if abs(r.imag) <= tol * abs(r)), key=abs)
    if 2 * len(cplx) + len(real) != 2 * order or len(real) % 2:
        raise ValueError(f"band_stop: the numerator of order {order} at edges {lo}, {hi} Hz does not factor into {order} sections")
    num = [[1.0, -2.0 * r.real, abs(r) ** 2] for r in cplx] + [[1.0, -(real[i] + real[i + 1]), real[i] * real[i + 1]]
                                                                  for i in range(0, len(real), 2)]
    q1, l1 = _analog_quads(order, K1)
    q2, l2 = _analog_quads(order, K2)
    den = q1 + q2 + ([[1.0, K1 + K2, K1 * K2]] if l1 else [])
    # Section order.  The zeros all lie in the stopped band between the edges, the poles at the two edges: a section with poles at the
    # lower edge lifts the lowest frequencies by (mid / lower edge)^2, one with poles at the upper edge lowers them as much.  The two
    # kinds ALTERNATE, so that the signal between two sections never carries more than one such factor (with the lower-edge sections
    # first it carried all of them, 1e9 at the extremes of the default ranges, and float64 lost that many digits).
    num.sort(key=lambda q: q[2])
    den.sort(key=lambda q: q[2])
    den = [den[i // 2] if i % 2 == 0 else den[-1 - i // 2] for i in range(len(den))]

    def to_z(q):
        return [1.0 + q[1] + q[2], 2.0 * (q[2] - 1.0), 1.0 - q[1] + q[2]]

    sos = []
    for n_, d_ in zip(num, den):
        b, a = to_z(n_), to_z(d_)
        sos.append([b[0] / a[0], b[1] / a[0], b[2] / a[0], 1.0, a[1] / a[0], a[2] / a[0]])
    return np.asarray(sos, dtype=np.float64)


def _cookbook(kind: str, freq: float, gain_db: float, q: float, sample_rate: float) -> np.ndarray:
    if not (math.isfinite(gain_db) and math.isfinite(q) and q > 0.0):
        raise ValueError(f"{kind}: gain_db must be finite and q positive, got gain_db {gain_db}, q {q}")
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * math.pi * freq / sample_rate
    cs, alpha = math.cos(w0), math.sin(w0) / (2.0 * q)
    if kind == "peaking":
        b = [1.0 + alpha * A, -2.0 * cs, 1.0 - alpha * A]
        a = [1.0 + alpha / A, -2.0 * cs, 1.0 - alpha / A]
    else:
        r = 2.0 * math.sqrt(A) * alpha
        sg = 1.0 if kind == "low_shelf" else -1.0  # the high shelf is the low shelf with cos -> -cos and b1, a1 negated
        b = [A * ((A + 1.0) - sg * (A - 1.0) * cs + r), sg * 2.0 * A * ((A - 1.0) - sg * (A + 1.0) * cs), A * ((A + 1.0) - sg * (A - 1.0) * cs - r)]
        a = [(A + 1.0) + sg * (A - 1.0) * cs + r, -sg * 2.0 * ((A - 1.0) + sg * (A + 1.0) * cs), (A + 1.0) + sg * (A - 1.0) * cs - r]
    return np.asarray([[b[0] / a[0], b[1] / a[0], b[2] / a[0], 1.0, a[1] / a[0], a[2] / a[0]]], dtype=np.float64)


def design(kind: str, sample_rate=16000, **params) -> np.ndarray:
    """One filter -> sos f64 [S, 6], a0 == 1.

    low_pass / high_pass: cutoff_freq, order (1..4).  band_pass / band_stop: center_freq, bandwidth_fraction (edges
    center * (1 -+ fraction / 2)), order.  low_shelf / high_shelf / peaking: center_freq, gain_db, q.
    ValueError: an unknown kind or keyword, a frequency or a band edge outside (0, sample_rate / 2), an order outside 1..4."""
    if kind not in KINDS:
        raise ValueError(f"unknown filter kind {kind!r}: one of {KINDS}")
    sample_rate = float(sample_rate)
    if not (math.isfinite(sample_rate) and sample_rate > 0):
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    want = {"low_pass": ("cutoff_freq", "order"), "high_pass": ("cutoff_freq", "order"),
            "band_pass": ("center_freq", "bandwidth_fraction", "order"), "band_stop": ("center_freq", "bandwidth_fraction", "order"),
            "low_shelf": ("center_freq", "gain_db", "q"), "high_shelf": ("center_freq", "gain_db", "q"),
            "peaking": ("center_freq", "gain_db", "q")}[kind]
    if set(params) != set(want):
        raise ValueError(f"design({kind!r}) takes exactly {want}, got {tuple(sorted(params))}")
    if kind in ("low_pass", "high_pass"):
        sos = _butter(kind, _check_order(params["order"]), _check_freq(params["cutoff_freq"], sample_rate, "cutoff_freq"), sample_rate)
    elif kind in ("band_pass", "band_stop"):
        order = _check_order(params["order"])
        centre, frac = _check_freq(params["center_freq"], sample_rate, "center_freq"), float(params["bandwidth_fraction"])
        if not (math.isfinite(frac) and frac > 0.0):
            raise ValueError(f"bandwidth_fraction must be positive, got {frac}")
        lo = _check_freq(centre * (1.0 - frac / 2.0), sample_rate, "the lower band edge")
        hi = _check_freq(centre * (1.0 + frac / 2.0), sample_rate, "the upper band edge")
        if kind == "band_pass":
            sos = np.concatenate([_butter("high_pass", order, lo, sample_rate), _butter("low_pass", order, hi, sample_rate)])
        else:
            sos = _band_stop(order, lo, hi, sample_rate)
    else:
        sos = _cookbook(kind, _check_freq(params["center_freq"], sample_rate, "center_freq"), float(params["gain_db"]), float(params["q"]),
                        sample_rate)
    if sos.shape[0] > MAX_SECTIONS or not np.all(np.isfinite(sos)):
        raise ValueError(f"design({kind!r}, {params}) gave {sos.shape[0]} sections / non-finite coefficients")
    return sos


def hz_to_mel(f: float) -> float:
    return 2595.0 * math.log10(1.0 + f / 700.0)


def mel_to_hz(m: float) -> float:
    return 700.0 * (10.0 ** (m / 2595.0) - 1.0)


_ROLLOFFS = (12, 18, 24)
DEFAULTS = {
    "low_pass": {"p": 1.0, "min_freq": 150.0, "max_freq": 7500.0, "rolloffs": _ROLLOFFS},
    "high_pass": {"p": 1.0, "min_freq": 20.0, "max_freq": 2400.0, "rolloffs": _ROLLOFFS},
    "band_pass": {"p": 1.0, "min_freq": 200.0, "max_freq": 4000.0, "min_bandwidth_fraction": 0.5, "max_bandwidth_fraction": 1.99,
                  "rolloffs": _ROLLOFFS},
    "band_stop": {"p": 1.0, "min_freq": 200.0, "max_freq": 4000.0, "min_bandwidth_fraction": 0.5, "max_bandwidth_fraction": 1.99,
                  "rolloffs": _ROLLOFFS},
    "low_shelf": {"p": 1.0, "min_freq": 50.0, "max_freq": 4000.0, "min_gain_db": -18.0, "max_gain_db": 18.0, "min_q": 0.1, "max_q": 0.999},
    "high_shelf": {"p": 1.0, "min_freq": 300.0, "max_freq": 7500.0, "min_gain_db": -18.0, "max_gain_db": 18.0, "min_q": 0.1, "max_q": 0.999},
    "peaking": {"p": 0.8, "min_freq": 50.0, "max_freq": 7500.0, "min_gain_db": -24.0, "max_gain_db": 24.0, "min_q": 0.5, "max_q": 5.0},
}


class FilterAug:
    """The reference's OneOf([seven filters], p=0.6), every filter with its own inner gate (0.8 for `peaking`, 1.0 for the others).

    p: the outer gate.  kinds: None (all seven with DEFAULTS), an iterable of kind names, or a mapping kind -> overrides of that
    kind's DEFAULTS entry (`p` the inner gate, `min_freq` / `max_freq` in Hz, `min_` / `max_bandwidth_fraction`, `min_` / `max_gain_db`,
    `min_` / `max_q`, `rolloffs` in dB per octave, each a multiple of 6 in 6..24: order = rolloff / 6).  The kinds take part in the order
    of KINDS, whatever order they are given in.  The default ranges are audiomentations' published defaults, restated; unpinned.

    draw() -> (kind or None, params, sos f64 [4, 6]); unused sections are identity, and (None, {}, identity) means "do not filter".
    The draw order is this project's own.  All draws use Python's `random` module (like the stretch rate) and never touch torch's
    generator:
      1. the gate:        random.random() < p; if it fails nothing else is drawn
      2. the kind:        random.randrange(number of kinds)
      3. the inner gate:  random.random() < the kind's p, drawn for every kind; if it fails nothing else is drawn
      4. the frequency:   random.uniform(mel(min_freq), mel(max_freq)), mel = 2595 log10(1 + f / 700), mapped back to Hz
      5. the second parameter: random.uniform over the bandwidth fraction (band_pass, band_stop) or the gain in dB (shelves,
                          peaking); low_pass and high_pass have none and draw nothing
      6. Q (random.uniform) for shelves and peaking, or the rolloff (random.randrange over `rolloffs`) for the Butterworth kinds
    Every range is checked in the constructor (ValueError): a range is refused if any draw from it could be refused by design()."""

    def __init__(self, p: float = 0.6, kinds=None, sample_rate: int = 16000):
        self.p, self.sample_rate = float(p), int(sample_rate)
        if not 0.0 <= self.p <= 1.0:
            raise ValueError(f"FilterAug p must lie in [0, 1], got {p}")
        if kinds is None:
            kinds = {k: {} for k in KINDS}
        elif not isinstance(kinds, Mapping):
            kinds = {k: {} for k in kinds}
        unknown = [k for k in kinds if k not in KINDS]
        if unknown or not kinds:
            raise ValueError(f"FilterAug kinds must be a non-empty subset of {KINDS}, got {list(kinds)}")
        self.kinds = tuple(k for k in KINDS if k in kinds)
        self.ranges = {}
        nyq = self.sample_rate / 2.0
        for k in self.kinds:
            over = dict(kinds[k] or {})
            bad = [name for name in over if name not in DEFAULTS[k]]
            if bad:
                raise ValueError(f"FilterAug {k}: unknown keyword(s) {bad}; it takes {sorted(DEFAULTS[k])}")
            r = {**DEFAULTS[k], **over}
            if not 0.0 <= float(r["p"]) <= 1.0:
                raise ValueError(f"FilterAug {k}: p must lie in [0, 1], got {r['p']}")
            lo, hi = float(r["min_freq"]), float(r["max_freq"])
            if not (0.0 < lo <= hi < nyq):
                raise ValueError(f"FilterAug {k}: need 0 < min_freq <= max_freq < {nyq}, got {lo}, {hi}")
            for a in ("bandwidth_fraction", "gain_db", "q"):
                if f"min_{a}" in r and not float(r[f"min_{a}"]) <= float(r[f"max_{a}"]):
                    raise ValueError(f"FilterAug {k}: min_{a} {r[f'min_{a}']} is larger than max_{a} {r[f'max_{a}']}")
            if "min_q" in r and not float(r["min_q"]) > 0.0:
                raise ValueError(f"FilterAug {k}: min_q must be positive, got {r['min_q']}")
            if "rolloffs" in r:
                r["rolloffs"] = tuple(r["rolloffs"])
                if not r["rolloffs"] or any(isinstance(x, bool) or x not in (6, 12, 18, 24) for x in r["rolloffs"]):
                    raise ValueError(f"FilterAug {k}: rolloffs must be a non-empty subset of (6, 12, 18, 24) dB/octave, got {r['rolloffs']}")
            if "min_bandwidth_fraction" in r:
                f0, f1 = float(r["min_bandwidth_fraction"]), float(r["max_bandwidth_fraction"])
                if not (0.0 < f0 and f1 < 2.0 and hi * (1.0 + f1 / 2.0) < nyq):
                    raise ValueError(f"FilterAug {k}: band edges center * (1 -+ fraction / 2) must stay inside (0, {nyq}) Hz, got "
                                     f"max_freq {hi}, bandwidth fractions {f0}..{f1}")
            self.ranges[k] = r

    def draw(self):
        ident = identity_sos()
        if not random.random() < self.p:
            return None, {}, ident
        kind = self.kinds[random.randrange(len(self.kinds))]
        r = self.ranges[kind]
        if not random.random() < r["p"]:
            return None, {}, ident
        freq = mel_to_hz(random.uniform(hz_to_mel(r["min_freq"]), hz_to_mel(r["max_freq"])))
        freq = min(max(freq, r["min_freq"]), r["max_freq"])  # the round trip through mel may leave the range by an ulp
        if kind in ("low_pass", "high_pass"):
            params = {"cutoff_freq": freq, "order": r["rolloffs"][random.randrange(len(r["rolloffs"]))] // 6}
        elif kind in ("band_pass", "band_stop"):
            frac = random.uniform(r["min_bandwidth_fraction"], r["max_bandwidth_fraction"])
            params = {"center_freq": freq, "bandwidth_fraction": frac, "order": r["rolloffs"][random.randrange(len(r["rolloffs"]))] // 6}
        else:
            gain = random.uniform(r["min_gain_db"], r["max_gain_db"])
            params = {"center_freq": freq, "gain_db": gain, "q": random.uniform(r["min_q"], r["max_q"])}
        sos = design(kind, self.sample_rate, **params)
        ident[: sos.shape[0]] = sos
        return kind, params, ident
