"""Mix effects: the draws of the background-noise and loudness-normalisation augmentation, the K-weighting design and the noise bank
(pure Python / numpy; the sibling of filters.py, wave_fx.py, rate_fx.py and office_fx.py).

The reference's advanced pipeline (`get_audio_augments_advanced`, model/augment.py) opens with two groups:

  OneOf([AddBackgroundNoise(absolute, -30..-10 dB), AddBackgroundNoise(snr, 2..4 dB)], p=0.3)
  OneOf([AddGaussianNoise, AddGaussianSNR, Aliasing, LoudnessNormalization], p=0.3)

AddBackgroundNoise and LoudnessNormalization run on the device (csrc/mix.hip, include/wft.h "Loudness and background noise" states
the arithmetic): the first is two row RMS values and one scaled add over a bank of noise recordings that lives in device memory, the
second the ITU-R BS.1770 integrated-loudness meter followed by one gain.  This module designs the meter's K-weighting
(`k_weighting`), loads the bank (`load_bank`) and draws a clip's parameters (`MixAug`); a worker ships them as one table row f64 [6]:
bg_kind (0 none, 1 snr, 2 absolute), bg_entry, bg_offset, bg_db, loud_on, target_lufs.

Deviations from the reference's recipe, all of them deliberate:
  * own gates that reproduce the reference's MARGINAL rates: background 0.3, loudness 0.3 / 4 = 0.075 (the Gaussian noises and
    Aliasing of the second group have their own gates in wave_fx.py and rate_fx.py).
  * the offset into a noise entry is drawn as an integer number of samples; audiomentations draws it in seconds.
  * a clip shorter than one 400 ms block is copied; pyloudnorm raises.
  * the meter's block count is stated in integers (pyloudnorm rounds a float).
  * no `noise_transform`; the bank is mono `.npy` float32 arrays, optionally resampled once on the device, or a directory of `.wav`
    files ({"wav_dir": path}: decoded, downmixed and resampled on the device, data/audio_io.py).
  * pyloudnorm and audiomentations are not dependencies: the methods are restated from their definitions, parity with their binaries
    is unpinned.
"""
from __future__ import annotations

import math
import os
import random
from typing import Mapping

import numpy as np

ROW = 6
KINDS = ("none", "snr", "absolute")
KIND_ID = {k: i for i, k in enumerate(KINDS)}
STAGES = ("background", "loudness")
DEFAULT_P = {"background": 0.3, "loudness": 0.3 / 4.0}
BACKGROUND_DEFAULTS = dict(min_snr_db=2.0, max_snr_db=4.0, min_absolute_rms_db=-30.0, max_absolute_rms_db=-10.0)
LOUDNESS_DEFAULTS = dict(min_lufs=-31.0, max_lufs=-13.0)  # audiomentations' LoudnessNormalization
DB_LIMIT = 200.0        # |dB| values beyond this are refused: 10^(dB / 20) must stay a sane float
RATE_MIN, RATE_MAX = 8000, 384000
SILENT_RMS = 1e-9       # wft_bg_mix_f32 copies a row whose noise RMS is below this
RECORD_DTYPE = np.dtype([("kind", "<i4"), ("entry", "<i4"), ("offset", "<i8"), ("db", "<f8")])  # wft_bg_rec, 24 bytes
SYNTHETIC_SECONDS = (3.0, 7.5, 31.0, 12.25)  # entry k of a synthetic bank lasts SYNTHETIC_SECONDS[k % 4]: shorter and longer than a clip


# ------------------------------------------------------------------------------------------------- the meter's constants
def loudness_hop(sample_rate) -> int:
    """The meter's 100 ms hop in samples (a 400 ms block is four of them).  The rate must be an integer multiple of 10 inside
    [8000, 384000] (ValueError otherwise), so the hop is an integer >= 800."""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)) or not RATE_MIN <= sample_rate <= RATE_MAX or sample_rate % 10:
        raise ValueError(f"loudness: sample_rate must be an integer multiple of 10 inside [{RATE_MIN}, {RATE_MAX}], got {sample_rate!r}")
    return int(sample_rate) // 10


def k_weighting(sample_rate) -> np.ndarray:
    """The K-weighting of ITU-R BS.1770 at `sample_rate` as sos f64 [2, 6] (b0 b1 b2 a0 a1 a2, a0 == 1): the RBJ cookbook high shelf
    (G = 4 dB, Q = 1 / sqrt(2), fc = 1500 Hz) and high pass (Q = 0.5, fc = 38 Hz), each divided by its a0 — pyloudnorm's
    "K-weighting" filter class, restated."""
    rate = float(loudness_hop(sample_rate) * 10)
    G, Q, fc = 4.0, 1.0 / math.sqrt(2.0), 1500.0
    A = 10.0 ** (G / 40.0)
    w0 = 2.0 * math.pi * (fc / rate)
    alpha = math.sin(w0) / (2.0 * Q)
    cs = math.cos(w0)
    shelf = [A * ((A + 1) + (A - 1) * cs + 2 * math.sqrt(A) * alpha), -2 * A * ((A - 1) + (A + 1) * cs),
             A * ((A + 1) + (A - 1) * cs - 2 * math.sqrt(A) * alpha),
             (A + 1) - (A - 1) * cs + 2 * math.sqrt(A) * alpha, 2 * ((A - 1) - (A + 1) * cs), (A + 1) - (A - 1) * cs - 2 * math.sqrt(A) * alpha]
    Q, fc = 0.5, 38.0
    w0 = 2.0 * math.pi * (fc / rate)
    alpha = math.sin(w0) / (2.0 * Q)
    cs = math.cos(w0)
    high = [(1 + cs) / 2, -(1 + cs), (1 + cs) / 2, 1 + alpha, -2 * cs, 1 - alpha]
    sos = np.array([shelf, high], dtype=np.float64)
    return sos / sos[:, 3:4]


def block_count(n: int, hop: int) -> int:
    """The number of 400 ms blocks of a clip of n samples: upstream's int(np.round((T - 0.4) / 0.1)) + 1 in integers (round half to
    even); 0 when the clip is shorter than one block."""
    block = 4 * hop
    if n < block:
        return 0
    q, r = divmod(n - block, hop)
    return q + 1 + (1 if 2 * r > hop or (2 * r == hop and q % 2 == 1) else 0)


# ------------------------------------------------------------------------------------------------- the noise bank
def synthetic_bank(K: int, sample_rate: int = 16000, seed: int = 0):
    """K seeded noise recordings for runs without files: entry k is low-passed Gaussian noise (a one-pole smoother, so it is not
    white) at an RMS near 0.05, SYNTHETIC_SECONDS[k % 4] seconds long, drawn from numpy's default_rng(seed + k)."""
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 4096:
        raise ValueError(f"synthetic bank: the number of entries must be an integer inside [1, 4096], got {K!r}")
    out = []
    for k in range(K):
        m = int(round(SYNTHETIC_SECONDS[k % len(SYNTHETIC_SECONDS)] * sample_rate))
        g = np.random.default_rng(seed + k).standard_normal(m + 1)
        out.append((0.05 * (g[1:] + g[:-1]) / math.sqrt(2.0)).astype(np.float32))
    return out


def load_bank(bank, sample_rate: int = 16000):
    """The noise bank as a list of mono float32 arrays.  bank: a directory of `.npy` files (taken in sorted name order), a list of
    arrays, or {"synthetic": K[, "seed": s]} (synthetic_bank at `sample_rate`).  ValueError: an empty bank, an entry of length 0, a
    non-finite sample, an array that is not 1-D float32.  A {"wav_dir": path[, "channel": c]} bank has no host form (its files are
    decoded on the device: data_loader.DeviceBank): it is checked and then refused here; bank_lengths serves it."""
    if isinstance(bank, Mapping):
        if "wav_dir" in bank:
            wav_bank(bank)
            raise ValueError("noise bank: a wav_dir bank is decoded on the device (data_loader.DeviceBank, gpu_frontend.load_audio); "
                             "bank_lengths reads its lengths from the headers")
        if not set(bank.keys()) <= {"synthetic", "seed"} or "synthetic" not in bank:
            raise ValueError(f"noise bank: a mapping must be {{'synthetic': K[, 'seed': s]}}, got {dict(bank)!r}")
        seed = bank.get("seed", 0)
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"noise bank: seed must be an integer, got {seed!r}")
        return synthetic_bank(bank["synthetic"], sample_rate, seed)
    if isinstance(bank, (str, os.PathLike)):
        if not os.path.isdir(bank):
            raise ValueError(f"noise bank: {os.fspath(bank)!r} is not a directory")
        names = sorted(f for f in os.listdir(bank) if f.endswith(".npy"))
        arrays = [np.load(os.path.join(bank, f), allow_pickle=False) for f in names]
    elif isinstance(bank, (list, tuple)):
        arrays = [np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a) for a in bank]
    else:
        raise ValueError(f"noise bank: a directory of .npy files, a list of arrays or {{'synthetic': K}}, got {type(bank).__name__}")
    if not arrays:
        raise ValueError("noise bank: the bank is empty")
    for k, a in enumerate(arrays):
        if a.ndim != 1 or a.dtype != np.float32:
            raise ValueError(f"noise bank: entry {k} must be a mono float32 array [m], got {a.dtype} {tuple(a.shape)}")
        if a.shape[0] == 0:
            raise ValueError(f"noise bank: entry {k} has length 0")
        if not bool(np.all(np.isfinite(a))):
            raise ValueError(f"noise bank: entry {k} holds a sample that is not finite")
    return [np.ascontiguousarray(a) for a in arrays]


def pack_bank(arrays):
    """A list of float32 arrays -> (the entries back to back f32 [total], their offsets i64 [K + 1]), wft_bg_mix_f32's layout."""
    off = np.zeros(len(arrays) + 1, dtype=np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in arrays])
    return np.concatenate(arrays).astype(np.float32, copy=False), off


def resampled_length(m: int, orig: int, new: int) -> int:
    """The length gpu_frontend.resample gives m samples: ceil(m * new / orig) (torchaudio's rule)."""
    return -((-m * new) // orig)


def wav_bank(bank):
    """{"wav_dir": path[, "channel": c]} -> (the directory's `.wav` files in name order, channel, their headers): audio_io.parse_wav
    reads the headers only.  ValueError: what audio_io.wav_dir_files and parse_wav refuse (the file named), a channel a file lacks."""
    from whisper_finetune.data import audio_io as AIO

    files, channel = AIO.wav_dir_files(bank)
    infos = []
    for f in files:
        try:
            info = AIO.parse_wav(f)
        except ValueError as e:
            raise ValueError(f"noise bank: {f!r}: {e}") from None
        if channel != "mean" and int(channel) >= info.channels:
            raise ValueError(f"noise bank: {f!r}: channel {int(channel)} does not exist in a file of {info.channels} channels")
        infos.append(info)
    return files, channel, infos


def bank_lengths(bank, sample_rate: int = 16000, bank_sample_rate=None):
    """The entry lengths at `sample_rate` (what a loader worker needs for its draws); the bank is loaded once for its checks.
    bank_sample_rate: the rate of the bank's recordings when it differs (they are resampled once on the device: GpuMelLoader).
    A {"wav_dir": ...} bank: every file has its own rate in its header (bank_sample_rate must be None); the lengths come from the
    headers and resampled_length, no payload is read."""
    if isinstance(bank, Mapping) and "wav_dir" in bank:
        if bank_sample_rate is not None:
            raise ValueError("noise bank: a wav_dir bank takes every file's rate from its header; bank_sample_rate must not be given")
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or not 1000 <= sample_rate <= 384000:
            raise ValueError(f"noise bank: sample_rate must be an integer inside [1000, 384000], got {sample_rate!r}")
        return [int(resampled_length(i.frames, i.sample_rate, sample_rate)) for i in wav_bank(bank)[2]]
    src = sample_rate if bank_sample_rate is None else bank_sample_rate
    if isinstance(src, bool) or not isinstance(src, int) or not 1000 <= src <= 384000:
        raise ValueError(f"noise bank: bank_sample_rate must be an integer inside [1000, 384000], got {bank_sample_rate!r}")
    lengths = [a.shape[0] for a in load_bank(bank, src)]
    if src != sample_rate:
        lengths = [resampled_length(m, src, sample_rate) for m in lengths]
    return [int(m) for m in lengths]


# ------------------------------------------------------------------------------------------------- the table
def none_table(B=None) -> np.ndarray:
    """The table of "neither stage": f64 [6], or [B, 6]."""
    return np.zeros(ROW if B is None else (B, ROW), dtype=np.float64)


def check_table(table, lengths) -> np.ndarray:
    """f64 [B, 6] (a tensor or an array) and the bank's entry lengths -> the same as a float64 numpy array, checked: every value
    finite; bg_kind an integer inside [0, 2]; on a row with a kind bg_entry an integer inside [0, K), bg_offset an integer inside
    [0, m) of its entry and |bg_db| <= 200; loud_on 0 or 1; |target_lufs| <= 200 on a row with loud_on.  ValueError otherwise, before
    the device is touched.  `lengths` may be None when no row has a kind."""
    t = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table)
    if t.dtype != np.float64 or t.ndim != 2 or t.shape[1] != ROW:
        raise ValueError(f"mix_fx table must be float64 [B, {ROW}], got {t.dtype} {tuple(t.shape)}")
    if not bool(np.all(np.isfinite(t))):
        raise ValueError("mix_fx table: every value must be finite")
    kind, entry, offset, db, on, target = (t[:, j] for j in range(ROW))
    if not bool(np.all((kind == np.rint(kind)) & (kind >= 0) & (kind <= 2))):
        raise ValueError("mix_fx table: bg_kind must be an integer inside [0, 2] (none, snr, absolute)")
    act = kind != 0
    if bool(act.any()):
        if lengths is None or len(lengths) == 0:
            raise ValueError("mix_fx table: a background row needs a noise bank")
        m = np.asarray(lengths, dtype=np.int64)
        if not bool(np.all((entry[act] == np.rint(entry[act])) & (entry[act] >= 0) & (entry[act] < m.shape[0]))):
            raise ValueError(f"mix_fx table: bg_entry must be an integer inside [0, {m.shape[0]})")
        me = m[entry[act].astype(np.int64)]
        if not bool(np.all((offset[act] == np.rint(offset[act])) & (offset[act] >= 0) & (offset[act] < me))):
            raise ValueError("mix_fx table: bg_offset must be an integer inside its entry")
        if not bool(np.all(np.abs(db[act]) <= DB_LIMIT)):
            raise ValueError(f"mix_fx table: |bg_db| must not exceed {DB_LIMIT}")
    if not bool(np.all((on == 0) | (on == 1))):
        raise ValueError("mix_fx table: loud_on must be 0 or 1")
    if not bool(np.all(np.abs(target[on == 1]) <= DB_LIMIT)):
        raise ValueError(f"mix_fx table: |target_lufs| must not exceed {DB_LIMIT}")
    return np.ascontiguousarray(t)


def records_from_table(table: np.ndarray) -> np.ndarray:
    """The background columns of a checked table -> wft_bg_rec records [B] (RECORD_DTYPE)."""
    rec = np.zeros(table.shape[0], dtype=RECORD_DTYPE)
    rec["kind"], rec["entry"], rec["offset"], rec["db"] = table[:, 0], table[:, 1], table[:, 2], table[:, 3]
    return rec


# ------------------------------------------------------------------------------------------------- the draws
def _group(spec, name: str, keys):
    if not isinstance(spec, Mapping) or not set(spec.keys()) <= set(keys):
        raise ValueError(f"MixAug {name} must be None or a mapping with the keys {sorted(keys)}, got {spec!r}")
    p = spec.get("p", DEFAULT_P[name])
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"MixAug {name}: p must lie in [0, 1], got {p!r}")
    return float(p)


def _pair(spec, lo: str, hi: str, defaults):
    a, b = spec.get(lo, defaults[lo]), spec.get(hi, defaults[hi])
    if any(isinstance(x, bool) or not isinstance(x, (int, float)) for x in (a, b)) or not (math.isfinite(a) and math.isfinite(b) and a <= b):
        raise ValueError(f"MixAug: need finite numbers {lo} <= {hi}, got {a!r}, {b!r}")
    if a < -DB_LIMIT or b > DB_LIMIT:
        raise ValueError(f"MixAug: {lo}..{hi} must stay inside [{-DB_LIMIT}, {DB_LIMIT}], got {a!r}, {b!r}")
    return float(a), float(b)


class MixAug:
    """MixAug(sample_rate, background=None | {p, kinds, bank, bank_sample_rate, min/max_snr_db, min/max_absolute_rms_db},
    loudness=None | {p, min_lufs, max_lufs}); a missing group is off, `{}` = the defaults (the background group needs `bank`):
    p = DEFAULT_P (the reference's marginal rates 0.3 and 0.075), kinds ("absolute", "snr"), the reference's arguments (absolute
    -30..-10 dB, snr 2..4 dB) and audiomentations' LoudnessNormalization defaults (-31..-13 LUFS).  bank: what load_bank takes, or
    {"wav_dir": path[, "channel": c]} (a directory of `.wav` files, every file at the rate of its header; no bank_sample_rate); only
    the entry lengths at `sample_rate` are kept (`lengths`), the recordings go to the device once (GpuMelLoader reads `bank` and
    `bank_sample_rate` back from here).

    draw(n) -> (names, row) for a clip of n samples: names = {"background": kind name or None, "loudness": bool}, row = the clip's
    table row f64 [6] (module docstring).  All draws use Python's `random` module and never touch torch's generator; a dataset makes
    them AFTER the office-effects draw, so every stream of draws that existed before is unchanged.  In the order background, loudness:
      1. the gate:    random.random() < p; if it fails nothing else is drawn for the group
      2. background:  kind = random.choice(kinds); entry = random.randrange(K); the value = random.uniform over the kind's range;
                      offset = random.randint(0, m - n) when the entry's length m exceeds n, else 0 (nothing is drawn)
         loudness:    target = random.uniform(min_lufs, max_lufs)
    Every range is checked in the constructor (ValueError)."""

    def __init__(self, sample_rate: int = 16000, background=None, loudness=None):
        self.hop = loudness_hop(sample_rate)
        self.sample_rate = int(sample_rate)
        self.p, self.kinds, self.ranges, self.lufs = {}, None, None, None
        self.bank, self.bank_sample_rate, self.lengths = None, None, None
        if background is not None:
            self.p["background"] = _group(background, "background", ("p", "kinds", "bank", "bank_sample_rate") + tuple(BACKGROUND_DEFAULTS))
            kinds = background.get("kinds", ("absolute", "snr"))
            if isinstance(kinds, str) or not hasattr(kinds, "__iter__"):
                raise ValueError(f"MixAug background: kinds must be a sequence of 'snr' / 'absolute', got {kinds!r}")
            kinds = tuple(kinds)
            if not kinds or any(k not in ("snr", "absolute") for k in kinds):
                raise ValueError(f"MixAug background: kinds must be a non-empty sequence of 'snr' / 'absolute', got {kinds!r}")
            self.kinds = kinds
            self.ranges = {"snr": _pair(background, "min_snr_db", "max_snr_db", BACKGROUND_DEFAULTS),
                           "absolute": _pair(background, "min_absolute_rms_db", "max_absolute_rms_db", BACKGROUND_DEFAULTS)}
            if background.get("bank") is None:
                raise ValueError("MixAug background: a noise bank is required (bank: a directory of .npy files, a list of arrays or {'synthetic': K})")
            self.bank, self.bank_sample_rate = background["bank"], background.get("bank_sample_rate")
            self.lengths = bank_lengths(self.bank, self.sample_rate, self.bank_sample_rate)
        if loudness is not None:
            self.p["loudness"] = _group(loudness, "loudness", ("p",) + tuple(LOUDNESS_DEFAULTS))
            self.lufs = _pair(loudness, "min_lufs", "max_lufs", LOUDNESS_DEFAULTS)

    def draw(self, n: int):
        names = {"background": None, "loudness": False}
        row = none_table()
        if "background" in self.p and random.random() < self.p["background"]:
            kind = random.choice(self.kinds)
            entry = random.randrange(len(self.lengths))
            value = random.uniform(*self.ranges[kind])
            m = self.lengths[entry]
            offset = random.randint(0, m - n) if m > n else 0
            names["background"] = kind
            row[0], row[1], row[2], row[3] = float(KIND_ID[kind]), float(entry), float(offset), value
        if "loudness" in self.p and random.random() < self.p["loudness"]:
            names["loudness"] = True
            row[4], row[5] = 1.0, random.uniform(*self.lufs)
        return names, row
