"""Rate effects: the draws of the pitch-shift and aliasing augmentation (pure Python / numpy; the sibling of filters.py and wave_fx.py).

Two more transforms of the reference's advanced audio pipeline (`get_audio_augments_advanced`, model/augment.py) run on the device
(csrc/rate.hip, include/wft.h "Per-row rate conversion" states the arithmetic); both are resampling at a fractional rate of the clip's own:

  Aliasing(p=1.0)                                  the fourth alternative of the noise group: linear interpolation down to a lower rate
                                                   and back without a low-pass (two np.interp calls, held bit for bit)
  PitchShift(min_semitones=-4, max_semitones=4)    the fourth alternative of the level group, p = 0.5: a time stretch by 2^(-s/12) (the
                                                   phase vocoder of the baseline pipeline) and a resample back to the clip's length

This module draws a clip's parameters (`RateAug`); a loader worker ships them as one table row f64 [4] = TABLE_COLUMNS:
alias_on, new_rate (Hz), pitch_on, semitones.  A stage that is off carries 0 in both of its columns.

Deviations from the reference's recipe, all of them deliberate:
  * own gates, independent of the wave stages (data/wave_fx.py): the reference draws ONE alternative per group, so it never pitches
    and gains the same clip, or aliases and adds noise to the same clip; here both can happen.  The default gates are the
    reference's MARGINAL rates: alias 0.3 * 1/4 = 0.075, pitch 0.3 * 1/4 * 0.5 = 0.0375.
  * audiomentations' default Aliasing maximum of 30 000 Hz lies above the clips' 16 000 Hz; what the library does then is not known
    here.  The default maximum is the clip rate, and a larger maximum raises ValueError.
  * the pitch shift's resampler is this project's Hann-windowed sinc (torchaudio's sinc_interp_hann, width 6, rolloff 0.99), not
    librosa's soxr_hq, which cannot be restated; the pitch shift is the phase-vocoder method (`librosa_phase_vocoder`), not
    audiomentations' current default.  Parity with both libraries' binaries is unpinned.
  * timestamps are untouched, as in the reference.
"""
from __future__ import annotations

import math
import random
from typing import Mapping

import numpy as np

from whisper_finetune.data.filters import hz_to_mel, mel_to_hz  # 2595 log10(1 + f / 700) and its inverse

TABLE_COLUMNS = ("alias_on", "new_rate", "pitch_on", "semitones")
TABLE_WIDTH = len(TABLE_COLUMNS)
STAGES = ("alias", "pitch")
DEFAULT_P = {"alias": 0.3 / 4.0, "pitch": 0.3 / 4.0 * 0.5}
ALIAS_MIN_RATE = 1000.0  # the one definition: K.alias refuses anything below
PITCH_MAX_SEMITONES = 12.0  # 2^(12/12) = 2.0, the end of the time stretch's range


def none_table(B=None) -> np.ndarray:
    """The table of "neither stage": f64 [4], or [B, 4]."""
    return np.zeros(TABLE_WIDTH if B is None else (B, TABLE_WIDTH), dtype=np.float64)


def check_table(table, sample_rate: int = 16000) -> np.ndarray:
    """f64 [B, 4] (a tensor or an array) -> the same as a float64 numpy array, checked: the two gates are 0 or 1, a stage that is off
    carries 0, an alias rate lies inside [1000, sample_rate], a pitch inside [-12, 12] semitones.  ValueError otherwise."""
    t = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table)
    if t.dtype != np.float64 or t.ndim != 2 or t.shape[1] != TABLE_WIDTH:
        raise ValueError(f"rate_fx table must be float64 [B, {TABLE_WIDTH}], got {t.dtype} {tuple(t.shape)}")
    a_on, rate, p_on, semi = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    if not bool(np.all(((a_on == 0) | (a_on == 1)) & ((p_on == 0) | (p_on == 1)))):
        raise ValueError("rate_fx table: alias_on and pitch_on must be 0 or 1")
    if not bool(np.all(np.where(a_on == 1, (rate >= ALIAS_MIN_RATE) & (rate <= float(sample_rate)), rate == 0))):
        raise ValueError(f"rate_fx table: new_rate must lie in [{ALIAS_MIN_RATE}, {float(sample_rate)}] where alias_on, and be 0 elsewhere")
    if not bool(np.all(np.where(p_on == 1, np.abs(semi) <= PITCH_MAX_SEMITONES, semi == 0))):  # (NaN fails both)
        raise ValueError(f"rate_fx table: semitones must lie in [-{PITCH_MAX_SEMITONES}, {PITCH_MAX_SEMITONES}] where pitch_on, and be 0 elsewhere")
    return np.ascontiguousarray(t)


def _group(spec, name: str, keys):
    if not isinstance(spec, Mapping) or not set(spec.keys()) <= set(keys):
        raise ValueError(f"RateAug {name} must be None or a mapping with the keys {sorted(keys)}, got {spec!r}")
    p = spec.get("p", DEFAULT_P[name])
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"RateAug {name}: p must lie in [0, 1], got {p!r}")
    return float(p)


def _pair(spec, lo: str, hi: str, name: str, defaults, low: float, high: float):
    a, b = spec.get(lo, defaults[0]), spec.get(hi, defaults[1])
    if any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in (a, b)) or not (math.isfinite(a) and math.isfinite(b) and a <= b):
        raise ValueError(f"RateAug {name}: need finite numbers {lo} <= {hi}, got {a!r}, {b!r}")
    if a < low or b > high:
        raise ValueError(f"RateAug {name}: {lo}..{hi} must stay inside [{low}, {high}], got {a!r}, {b!r}")
    return float(a), float(b)


class RateAug:
    """RateAug(sample_rate, alias=None | {p, min_sample_rate, max_sample_rate}, pitch=None | {p, min_semitones, max_semitones}); a
    missing group is off, `{}` = the defaults: p = DEFAULT_P (the reference's marginal rates: the module docstring says why),
    8 000 .. 16 000 Hz (the maximum defaults to the clip rate), -4 .. +4 semitones.

    draw() -> (names, row): names = {"alias": bool, "pitch": bool}, row = the clip's table row f64 [4] (module docstring).  All draws
    use Python's `random` module and never touch torch's generator; a dataset makes them AFTER the wave-effects draw, so every stream
    of draws that existed before is unchanged.  For each group that is on, in the order alias, pitch:
      1. the gate:    random.random() < p; if it fails nothing else is drawn for the group
      2. alias:       new_rate = mel_to_hz(random.uniform(hz_to_mel(min_sample_rate), hz_to_mel(max_sample_rate))), clamped to the
                      two bounds (the inverse may leave them by an ulp): uniform on the mel scale 2595 log10(1 + f / 700), as
                      audiomentations draws it
         pitch:       semitones = random.uniform(min_semitones, max_semitones)
    Every range is checked in the constructor (ValueError): 1000 <= min_sample_rate <= max_sample_rate <= sample_rate,
    -12 <= min_semitones <= max_semitones <= 12.  Timestamps are untouched, as in the reference."""

    def __init__(self, sample_rate: int = 16000, alias=None, pitch=None):
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate < 1000:
            raise ValueError(f"RateAug sample_rate must be an integer >= 1000, got {sample_rate!r}")
        self.sample_rate = sample_rate
        self.p, self.alias_range, self.pitch_range = {}, None, None
        if alias is not None:
            self.p["alias"] = _group(alias, "alias", ("p", "min_sample_rate", "max_sample_rate"))
            self.alias_range = _pair(alias, "min_sample_rate", "max_sample_rate", "alias", (min(8000.0, float(sample_rate)), float(sample_rate)),
                                     ALIAS_MIN_RATE, float(sample_rate))
        if pitch is not None:
            self.p["pitch"] = _group(pitch, "pitch", ("p", "min_semitones", "max_semitones"))
            self.pitch_range = _pair(pitch, "min_semitones", "max_semitones", "pitch", (-4.0, 4.0), -PITCH_MAX_SEMITONES, PITCH_MAX_SEMITONES)

    def draw(self):
        names = {g: False for g in STAGES}
        row = none_table()
        if "alias" in self.p and random.random() < self.p["alias"]:
            lo, hi = self.alias_range
            rate = mel_to_hz(random.uniform(hz_to_mel(lo), hz_to_mel(hi)))
            names["alias"], row[0], row[1] = True, 1.0, min(max(rate, lo), hi)
        if "pitch" in self.p and random.random() < self.p["pitch"]:
            names["pitch"], row[2], row[3] = True, 1.0, random.uniform(*self.pitch_range)
        return names, row
