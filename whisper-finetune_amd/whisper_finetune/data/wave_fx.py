"""Wave effects: the draws and records of the noise, clipping and level augmentation (pure Python / numpy; the sibling of filters.py).

Six transforms of the reference's advanced audio pipeline (`get_audio_augments_advanced`, model/augment.py) are plain arithmetic on the
waveform and run on the device (csrc/wavefx.hip, include/wft.h "Wave effects" states the arithmetic): audiomentations'
AddGaussianNoise, AddGaussianSNR, ClippingDistortion, Gain, GainTransition and Shift.  Their parameter ranges are the values the
reference passes and audiomentations' published defaults where it passes none, restated; the library is not a dependency and parity
with its binary is unpinned.  This module draws a clip's parameters (`WaveAug`) and packs them for the kernel:

  table    f64 [B, 14] (or [14] for one clip): the form a loader worker ships and `torch.stack` collates.  Columns = TABLE_COLUMNS;
           every integer in it is exact in f64, the 64-bit noise seed travels as two exact 32-bit halves.
  records  numpy structured array [B] of RECORD_DTYPE: wft_wave_fx byte for byte (88 bytes), what the kernel reads.

Deviations from the reference's recipe, all of them deliberate:
  * own outer gates.  The reference draws ONE of four alternatives in its noise group (p = 0.3), one of nine in its filter group
    (p = 0.6) and one of four in its level group (p = 0.3).  Only 2, 1 and 3 of those alternatives are built here, so the default outer
    gates reproduce their MARGINAL rates: noise 0.3 * 2 / 4 = 0.15, clipping 0.6 / 9, level 0.3 * 3 / 4 = 0.225.
  * PitchShift's slot in the level group is dropped here (its quarter of the gate is simply "nothing"); the pitch shift has a gate of its
    own in data/rate_fx.py, independent of this group.
  * clipping sits outside the filter group's OneOf: a clip may be filtered AND clipped, which the reference never does.
  * AirAbsorption (its coefficient table cannot be restated without audiomentations) is not built; background noise (over a bank of
    .npy recordings) and LoudnessNormalization live in data/mix_fx.py (csrc/mix.hip), with gates of their own; Aliasing and PitchShift
    are resampling at a per-row rate and live in data/rate_fx.py (csrc/rate.hip).
"""
from __future__ import annotations

import math
import random
from typing import Mapping, Optional

import numpy as np

STAGES = ("noise", "clip", "level")
STAGE_ID = {"noise": 0, "clip": 1, "level": 2}
KINDS = {"noise": ("gaussian_noise", "gaussian_snr"), "clip": ("clipping",), "level": ("gain", "gain_transition", "shift")}
KIND_ID = {"gaussian_noise": 1, "gaussian_snr": 2, "clipping": 1, "gain": 1, "gain_transition": 2, "shift": 3}
STAGE_OF = {k: s for s, ks in KINDS.items() for k in ks}
KIND_FIELD = {"noise": "noise_kind", "clip": "clip_kind", "level": "level_kind"}

RECORD_DTYPE = np.dtype({
    "names": ["noise_kind", "clip_kind", "level_kind", "clip_q", "seed", "noise_value", "gain_ratio", "reserved", "db_start", "db_end", "t0",
              "ramp_len", "shift_fraction", "fade_len"],
    "formats": ["<i4", "<i4", "<i4", "<i4", "<u8", "<f8", "<f4", "<i4", "<f8", "<f8", "<i8", "<i8", "<f8", "<i8"],
    "offsets": [0, 4, 8, 12, 16, 24, 32, 36, 40, 48, 56, 64, 72, 80],
    "itemsize": 88,
})
TABLE_COLUMNS = ("noise_kind", "noise_value", "seed_lo", "seed_hi", "clip_kind", "clip_q", "level_kind", "gain_ratio", "db_start", "db_end",
                 "t0", "ramp_len", "shift_fraction", "fade_len")
TABLE_WIDTH = len(TABLE_COLUMNS)
_COL = {name: i for i, name in enumerate(TABLE_COLUMNS)}
INDEX_LIMIT = 1 << 40  # |t0|, ramp_len and fade_len: exact in f64 and far from any int64 overflow inside the kernel

DEFAULT_P = {"noise": 0.15, "clip": 0.6 / 9.0, "level": 0.225}
DEFAULTS = {
    "gaussian_noise": {"p": 1.0, "min_amplitude": 0.001, "max_amplitude": 0.015},
    "gaussian_snr": {"p": 1.0, "min_snr_db": 5.0, "max_snr_db": 40.0},
    "clipping": {"p": 0.8, "min_percentile_threshold": 0, "max_percentile_threshold": 40},
    "gain": {"p": 1.0, "min_gain_db": -6.0, "max_gain_db": 6.0},
    "gain_transition": {"p": 1.0, "min_gain_db": -24.0, "max_gain_db": 6.0, "min_duration": 0.2, "max_duration": 6.0},
    "shift": {"p": 0.5, "min_shift": -0.5, "max_shift": 0.5, "fade_duration": 0.005},
}


def none_table(B: Optional[int] = None) -> np.ndarray:
    """The table of "no effect in any stage": f64 [14], or [B, 14]."""
    t = np.zeros(TABLE_WIDTH if B is None else (B, TABLE_WIDTH), dtype=np.float64)
    t[..., _COL["gain_ratio"]] = 1.0
    t[..., _COL["ramp_len"]] = 1.0
    return t


def gain_ratio(gain_db: float) -> float:
    """f32(10^(dB / 20)), the one factor of a `gain` row, as a Python float."""
    return float(np.float32(10.0 ** (float(gain_db) / 20.0)))


def table_row(kind: Optional[str] = None, **params) -> np.ndarray:
    """One clip's table row f64 [14] with a single effect (the other stages "none"); kind None = no effect.

    gaussian_noise(amplitude, seed)   gaussian_snr(snr_db, seed)   clipping(q)   gain(gain_db)
    gain_transition(start_db, end_db, t0, length)   shift(fraction, fade_len=0)"""
    t = none_table()
    if kind is None:
        if params:
            raise ValueError(f"table_row: parameters {sorted(params)} without a kind")
        return t
    if kind not in STAGE_OF:
        raise ValueError(f"wave effect must be one of {sorted(STAGE_OF)}, got {kind!r}")
    want = {"gaussian_noise": ("amplitude", "seed"), "gaussian_snr": ("snr_db", "seed"), "clipping": ("q",), "gain": ("gain_db",),
            "gain_transition": ("start_db", "end_db", "t0", "length"), "shift": ("fraction", "fade_len")}[kind]
    if kind == "shift":
        params.setdefault("fade_len", 0)
    if sorted(params) != sorted(want):
        raise ValueError(f"{kind} takes {want}, got {sorted(params)}")
    t[_COL[KIND_FIELD[STAGE_OF[kind]]]] = KIND_ID[kind]
    if kind in ("gaussian_noise", "gaussian_snr"):
        seed = int(params["seed"])
        if not 0 <= seed < (1 << 64):
            raise ValueError(f"{kind}: seed must lie in [0, 2^64), got {seed}")
        t[_COL["noise_value"]] = float(params["amplitude"] if kind == "gaussian_noise" else params["snr_db"])
        t[_COL["seed_lo"]], t[_COL["seed_hi"]] = float(seed & 0xFFFFFFFF), float(seed >> 32)
    elif kind == "clipping":
        t[_COL["clip_q"]] = params["q"]
    elif kind == "gain":
        t[_COL["gain_ratio"]] = gain_ratio(params["gain_db"])
    elif kind == "gain_transition":
        t[_COL["db_start"]], t[_COL["db_end"]] = float(params["start_db"]), float(params["end_db"])
        t[_COL["t0"]], t[_COL["ramp_len"]] = params["t0"], params["length"]
    else:
        t[_COL["shift_fraction"]], t[_COL["fade_len"]] = float(params["fraction"]), params["fade_len"]
    check_records(records_from_table(t[None]))
    return t


def records_from_table(table) -> np.ndarray:
    """f64 [B, 14] (a tensor or an array) -> records [B].  ValueError if a column that must hold an integer does not, or a seed
    half lies outside [0, 2^32): nothing is rounded silently."""
    t = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table)
    if t.dtype != np.float64 or t.ndim != 2 or t.shape[1] != TABLE_WIDTH:
        raise ValueError(f"wave_fx table must be float64 [B, {TABLE_WIDTH}], got {t.dtype} {tuple(t.shape)}")
    ints = ["noise_kind", "clip_kind", "level_kind", "clip_q", "seed_lo", "seed_hi", "t0", "ramp_len", "fade_len"]
    for name in ints:
        c = t[:, _COL[name]]
        if not bool(np.all(np.isfinite(c) & (c == np.floor(c)) & (np.abs(c) <= float(INDEX_LIMIT)))):
            raise ValueError(f"wave_fx table: column {name} must hold integers of magnitude <= 2^40")
    for name in ("seed_lo", "seed_hi"):
        c = t[:, _COL[name]]
        if not bool(np.all((c >= 0) & (c < 4294967296.0))):
            raise ValueError(f"wave_fx table: column {name} must lie in [0, 2^32)")
    ratio = t[:, _COL["gain_ratio"]]
    with np.errstate(over="ignore", invalid="ignore"):
        if not bool(np.all(ratio.astype(np.float32).astype(np.float64) == ratio)):
            raise ValueError("wave_fx table: gain_ratio must be a finite float32 value (data/wave_fx.py gain_ratio)")
    r = np.zeros(t.shape[0], dtype=RECORD_DTYPE)
    for name in ("noise_kind", "clip_kind", "level_kind", "clip_q"):
        c = t[:, _COL[name]]
        if not bool(np.all(np.abs(c) < 2.0 ** 31)):
            raise ValueError(f"wave_fx table: column {name} does not fit an int32")
        r[name] = c.astype(np.int32)
    r["seed"] = t[:, _COL["seed_lo"]].astype(np.uint64) | (t[:, _COL["seed_hi"]].astype(np.uint64) << np.uint64(32))
    for name in ("noise_value", "db_start", "db_end", "shift_fraction"):
        r[name] = t[:, _COL[name]]
    r["gain_ratio"] = ratio.astype(np.float32)
    for name in ("t0", "ramp_len", "fade_len"):
        r[name] = t[:, _COL[name]].astype(np.int64)
    return r


def table_from_records(rec) -> np.ndarray:
    """records [B] -> f64 [B, 14]; the inverse of records_from_table for records that pass check_records."""
    rec = np.asarray(rec)
    t = np.zeros((rec.shape[0], TABLE_WIDTH), dtype=np.float64)
    for name in TABLE_COLUMNS:
        if name == "seed_lo":
            t[:, _COL[name]] = (rec["seed"] & np.uint64(0xFFFFFFFF)).astype(np.float64)
        elif name == "seed_hi":
            t[:, _COL[name]] = (rec["seed"] >> np.uint64(32)).astype(np.float64)
        else:
            t[:, _COL[name]] = rec[name].astype(np.float64)
    return t


def check_records(rec) -> np.ndarray:
    """records [B] as the kernel may read them, or ValueError: the values that only the device sees are refused HERE, before the
    device is touched — an unknown kind, q outside 0..50, a non-finite amplitude / SNR / gain / dB / fraction, a negative amplitude,
    a fraction outside [-1, 1], |t0| or a length beyond 2^40, ramp_len < 1, fade_len < 0.  Only the fields of a row's ACTIVE kinds
    are checked."""
    rec = np.asarray(rec)
    if rec.dtype != RECORD_DTYPE or rec.ndim != 1:
        raise ValueError(f"wave_fx records must be a 1-D array of data/wave_fx.py RECORD_DTYPE, got {rec.dtype} {tuple(rec.shape)}")
    for stage in STAGES:
        k = rec[KIND_FIELD[stage]]
        if not bool(np.all((k >= 0) & (k <= len(KINDS[stage])))):
            raise ValueError(f"wave_fx: {KIND_FIELD[stage]} must lie in 0..{len(KINDS[stage])}")
    nz = rec["noise_kind"] != 0
    if not bool(np.all(np.isfinite(rec["noise_value"][nz]))):
        raise ValueError("wave_fx: a noise row's amplitude / SNR must be finite")
    if bool(np.any(rec["noise_value"][rec["noise_kind"] == 1] < 0.0)):
        raise ValueError("wave_fx: gaussian_noise needs an amplitude >= 0")
    q = rec["clip_q"][rec["clip_kind"] != 0]
    if not bool(np.all((q >= 0) & (q <= 50))):
        raise ValueError("wave_fx: clipping needs an integer percent q in 0..50")
    if not bool(np.all(np.isfinite(rec["gain_ratio"][rec["level_kind"] == 1]))):
        raise ValueError("wave_fx: gain needs a finite ratio")
    tr = rec[rec["level_kind"] == 2]
    if not bool(np.all(np.isfinite(tr["db_start"]) & np.isfinite(tr["db_end"]))):
        raise ValueError("wave_fx: gain_transition needs finite start and end levels")
    if not bool(np.all((np.abs(tr["t0"]) <= INDEX_LIMIT) & (tr["ramp_len"] >= 1) & (tr["ramp_len"] <= INDEX_LIMIT))):
        raise ValueError("wave_fx: gain_transition needs |t0| <= 2^40 and 1 <= length <= 2^40")
    sh = rec[rec["level_kind"] == 3]
    if not bool(np.all(np.abs(sh["shift_fraction"]) <= 1.0)):  # (NaN fails the comparison)
        raise ValueError("wave_fx: shift needs a fraction in [-1, 1]")
    if not bool(np.all((sh["fade_len"] >= 0) & (sh["fade_len"] <= INDEX_LIMIT))):
        raise ValueError("wave_fx: shift needs 0 <= fade_len <= 2^40")
    return rec


def active_rows(rec, stage: str) -> np.ndarray:
    """bool [B]: the rows whose kind for `stage` is not "none"."""
    return np.asarray(rec)[KIND_FIELD[stage]] != 0


def _range(r, lo: str, hi: str, who: str, *, low=None, high=None):
    a, b = float(r[lo]), float(r[hi])
    if not (math.isfinite(a) and math.isfinite(b) and a <= b):
        raise ValueError(f"WaveAug {who}: need finite {lo} <= {hi}, got {r[lo]}, {r[hi]}")
    if (low is not None and a < low) or (high is not None and b > high):
        raise ValueError(f"WaveAug {who}: {lo}..{hi} must stay inside [{low}, {high}], got {r[lo]}, {r[hi]}")


class WaveAug:
    """WaveAug(noise=None | {...}, clip=None | {...}, level=None | {...}): each group is a mapping {p, kinds}; a missing group is off.

    p: the group's outer gate (default DEFAULT_P, the reference's marginal rates: the module docstring says why).  kinds: None (every
    kind of the group with DEFAULTS), an iterable of kind names, or a mapping kind -> overrides of that kind's DEFAULTS entry (`p` is
    the kind's inner gate).  The kinds take part in the order of KINDS[group], whatever order they are given in.

    draw(n) -> (names, row): names = {group: kind or None}, row = the clip's table row f64 [14] (module docstring).  n = the clip's
    length in samples as the worker sees it (the padded clip, 480000): only the start index of a gain transition depends on it.  All
    draws use Python's `random` module and never touch torch's generator.  For each group that is on, in the order noise, clip, level:
      1. the gate:        random.random() < p; if it fails nothing else is drawn for the group
      2. the kind:        random.randrange(number of kinds)
      3. the inner gate:  random.random() < the kind's p; if it fails nothing else is drawn for the group
      4. the parameters:
         gaussian_noise   amplitude = random.uniform(min_amplitude, max_amplitude); seed = random.getrandbits(64)
         gaussian_snr     snr_db = random.uniform(min_snr_db, max_snr_db); seed = random.getrandbits(64)
         clipping         threshold = random.randint(min_percentile_threshold, max_percentile_threshold); q = threshold // 2
         gain             gain_db = random.uniform(min_gain_db, max_gain_db); the row carries f32(10^(gain_db / 20))
         gain_transition  start_db, end_db = random.uniform(min_gain_db, max_gain_db) twice; duration = random.uniform(min_duration,
                          max_duration), length = max(int(duration * sample_rate), 1); t0 = random.randint(2 - length, n - 2) (anywhere
                          the ramp still overlaps the clip; one value when that range is empty: 0)
         shift            fraction = random.uniform(min_shift, max_shift); fade_len = int(fade_duration * sample_rate) (80 samples)
    Every range is checked in the constructor (ValueError).  Timestamps are not moved under `shift`, as in the reference."""

    def __init__(self, noise=None, clip=None, level=None, sample_rate: int = 16000):
        self.sample_rate = int(sample_rate)
        if self.sample_rate < 1:
            raise ValueError(f"WaveAug sample_rate must be positive, got {sample_rate}")
        self.p, self.kinds, self.ranges = {}, {}, {}
        for group, spec in (("noise", noise), ("clip", clip), ("level", level)):
            if spec is None:
                continue
            if not isinstance(spec, Mapping) or not set(spec.keys()) <= {"p", "kinds"}:
                raise ValueError(f"WaveAug {group} must be None or a mapping with the keys `p` and `kinds`, got {spec!r}")
            p = float(spec.get("p", DEFAULT_P[group]))
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"WaveAug {group}: p must lie in [0, 1], got {spec.get('p')}")
            kinds = spec.get("kinds")
            if kinds is None:
                kinds = {k: {} for k in KINDS[group]}
            elif not isinstance(kinds, Mapping):
                kinds = {k: {} for k in kinds}
            unknown = [k for k in kinds if k not in KINDS[group]]
            if unknown or not kinds:
                raise ValueError(f"WaveAug {group}: kinds must be a non-empty subset of {KINDS[group]}, got {list(kinds)}")
            self.p[group] = p
            self.kinds[group] = tuple(k for k in KINDS[group] if k in kinds)
            for k in self.kinds[group]:
                over = dict(kinds[k] or {})
                bad = [name for name in over if name not in DEFAULTS[k]]
                if bad:
                    raise ValueError(f"WaveAug {k}: unknown keyword(s) {bad}; it takes {sorted(DEFAULTS[k])}")
                r = {**DEFAULTS[k], **over}
                if not 0.0 <= float(r["p"]) <= 1.0:
                    raise ValueError(f"WaveAug {k}: p must lie in [0, 1], got {r['p']}")
                if k == "gaussian_noise":
                    _range(r, "min_amplitude", "max_amplitude", k, low=0.0)
                elif k == "gaussian_snr":
                    _range(r, "min_snr_db", "max_snr_db", k, low=-200.0, high=200.0)
                elif k == "clipping":
                    lo, hi = r["min_percentile_threshold"], r["max_percentile_threshold"]
                    if any(isinstance(x, bool) or not isinstance(x, int) for x in (lo, hi)) or not 0 <= lo <= hi <= 100:
                        raise ValueError(f"WaveAug clipping: need integers 0 <= min_percentile_threshold <= max_percentile_threshold <= 100, "
                                         f"got {lo!r}, {hi!r}")
                elif k == "gain":
                    _range(r, "min_gain_db", "max_gain_db", k, low=-200.0, high=200.0)
                elif k == "gain_transition":
                    _range(r, "min_gain_db", "max_gain_db", k, low=-200.0, high=200.0)
                    _range(r, "min_duration", "max_duration", k, low=0.0, high=float(INDEX_LIMIT // self.sample_rate))
                    if not float(r["min_duration"]) > 0.0:
                        raise ValueError(f"WaveAug gain_transition: min_duration must be positive, got {r['min_duration']}")
                else:
                    _range(r, "min_shift", "max_shift", k, low=-1.0, high=1.0)
                    fd = float(r["fade_duration"])
                    if not (math.isfinite(fd) and 0.0 <= fd <= float(INDEX_LIMIT // self.sample_rate)):
                        raise ValueError(f"WaveAug shift: fade_duration must be a finite number of seconds >= 0, got {r['fade_duration']}")
                self.ranges[k] = r

    def draw(self, n: int = 480000):
        names = {g: None for g in STAGES}
        row = none_table()
        for group in STAGES:
            if group not in self.p:
                continue
            if not random.random() < self.p[group]:
                continue
            kind = self.kinds[group][random.randrange(len(self.kinds[group]))]
            r = self.ranges[kind]
            if not random.random() < r["p"]:
                continue
            names[group] = kind
            row[_COL[KIND_FIELD[group]]] = KIND_ID[kind]
            if kind in ("gaussian_noise", "gaussian_snr"):
                lo, hi = ("min_amplitude", "max_amplitude") if kind == "gaussian_noise" else ("min_snr_db", "max_snr_db")
                row[_COL["noise_value"]] = random.uniform(r[lo], r[hi])
                seed = random.getrandbits(64)
                row[_COL["seed_lo"]], row[_COL["seed_hi"]] = float(seed & 0xFFFFFFFF), float(seed >> 32)
            elif kind == "clipping":
                row[_COL["clip_q"]] = random.randint(r["min_percentile_threshold"], r["max_percentile_threshold"]) // 2
            elif kind == "gain":
                row[_COL["gain_ratio"]] = gain_ratio(random.uniform(r["min_gain_db"], r["max_gain_db"]))
            elif kind == "gain_transition":
                row[_COL["db_start"]] = random.uniform(r["min_gain_db"], r["max_gain_db"])
                row[_COL["db_end"]] = random.uniform(r["min_gain_db"], r["max_gain_db"])
                length = max(int(random.uniform(r["min_duration"], r["max_duration"]) * self.sample_rate), 1)
                lo, hi = 2 - length, int(n) - 2
                row[_COL["t0"]] = random.randint(lo, hi) if lo <= hi else 0
                row[_COL["ramp_len"]] = length
            else:
                row[_COL["shift_fraction"]] = random.uniform(r["min_shift"], r["max_shift"])
                row[_COL["fade_len"]] = int(float(r["fade_duration"]) * self.sample_rate)
        return names, row
