"""GPU front end of the data path: raw 30 s clips (resampled to 16 kHz on the device when they come at another
rate) -> log-mel -> SpecAugment, batched on the device.

It replaces, arithmetic for arithmetic, what `AudioDataset._calculate_mel`
(data/data_loader.py:273-292) does per clip in a CPU DataLoader worker:
  whisper.audio.log_mel_spectrogram -> pad_or_trim -> [time warp -> time mask -> freq mask] w.p. p
  -> extremes frequency masking.
All random parameters are drawn on the HOST from the default CPU generator in the reference's
order (per clip: gate `rand` if 0<p<1; warp `randint(W, L-W)`, `randint(-W, W)`; time mask
`rand, rand`; freq mask `rand, rand`; extremes `rand`) and handed to the kernels, so a seeded
run reproduces the reference's augmentation decisions exactly.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from whisper_finetune.engine import kernels as K

SAMPLE_RATE = 16000
N_FFT = 400
HOP_LENGTH = 160
N_SAMPLES = 480000
N_FRAMES = 3000


def mel_filters(n_mels: int) -> torch.Tensor:
    """Slaney-scale, slaney-normalised mel filterbank for sr=16 kHz, n_fft=400 (the asset
    whisper ships as mel_filters.npz): f32 [n_mels, 201]."""
    def hz_to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-10) / 1000.0) / (np.log(6.4) / 27.0), f * 3.0 / 200.0)

    def mel_to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * 200.0 / 3.0)

    n_bins = N_FFT // 2 + 1
    freqs = np.linspace(0, SAMPLE_RATE / 2, n_bins)
    pts = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(SAMPLE_RATE / 2), n_mels + 2))
    w = np.zeros((n_mels, n_bins))
    for i in range(n_mels):
        up = (freqs - pts[i]) / (pts[i + 1] - pts[i])
        down = (pts[i + 2] - freqs) / (pts[i + 2] - pts[i + 1])
        w[i] = np.maximum(0.0, np.minimum(up, down))
    w *= (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return torch.from_numpy(w.astype(np.float32))


# ------------------------------------------------------------------------------------------------- resampling
# torchaudio's `sinc_interp_hann` resampler with its defaults (lowpass_filter_width = 6, rolloff = 0.99), restated in its polyphase
# form (include/wft.h "wft_resample_f32" states the definition).  torchaudio is not a dependency: parity with its binary is unpinned.
MIN_RATE, MAX_RATE = 1000, 384000
_LOWPASS_WIDTH, _ROLLOFF = 6, 0.99
_TAPS = {}


def check_rate(rate, what: str = "sample_rate") -> int:
    """An integer sample rate inside [1000, 384000] -> int; anything else raises ValueError."""
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)):
        raise ValueError(f"{what} must be an integer number of Hz, got {rate!r}")
    rate = int(rate)
    if not MIN_RATE <= rate <= MAX_RATE:
        raise ValueError(f"{what} must lie in [{MIN_RATE}, {MAX_RATE}] Hz, got {rate}")
    return rate


def resample_taps(orig: int, new: int):
    """The polyphase table of the rate pair -> (taps f32 [n, 2 * width] on the host, o, n, width), cached per reduced pair.

    o = orig / gcd, n = new / gcd, base = 0.99 * min(o, n), width = ceil(6 * o / base);
    taps[r][k + width - 1] = g((k - r / n) * base / o) for k = -width + 1 .. width, with
    g(t) = (base / o) * sinc(pi t) * cos^2(pi t / 12) for |t| < 6 and exactly 0 otherwise.  Built in float64, rounded once to f32."""
    for name, v in (("orig", orig), ("new", new)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"resample_taps: {name} must be a positive integer, got {v!r}")
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    if (o, n) not in _TAPS:
        base = _ROLLOFF * min(o, n)
        width = math.ceil(_LOWPASS_WIDTH * o / base)
        k = np.arange(-width + 1, width + 1, dtype=np.float64)[None, :]
        r = np.arange(n, dtype=np.float64)[:, None]
        t = (k - r / n) * base / o
        w = (base / o) * np.sinc(t) * np.cos(np.pi * t / (2 * _LOWPASS_WIDTH)) ** 2
        w[np.abs(t) >= _LOWPASS_WIDTH] = 0.0
        _TAPS[(o, n)] = (torch.from_numpy(w.astype(np.float32)), o, n, width)
    return _TAPS[(o, n)]


def resample(audio, sample_rate, device=None) -> torch.Tensor:
    """audio at `sample_rate` Hz -> the same audio at 16 kHz, on the device (K.resample, one launch).

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array; a host input goes to `device` (default: the current GPU) first.
    The result has the input's number of dimensions and ceil(n * 16000 / sample_rate) samples per row; at 16 kHz the (device) input
    is returned as it is.  sample_rate: an integer inside [1000, 384000], else ValueError."""
    rate = check_rate(sample_rate)
    a = torch.as_tensor(audio)
    if a.dim() not in (1, 2) or a.dtype != torch.float32 or a.numel() == 0:
        raise ValueError(f"resample: audio must be a non-empty float32 [n] or [B, n], got {a.dtype} {tuple(a.shape)}")
    if device is not None:
        a = a.to(device)
    elif not a.is_cuda:
        a = a.to(torch.device("cuda", torch.cuda.current_device()))
    if rate == SAMPLE_RATE:
        return a
    out = K.resample(a if a.dim() == 2 else a[None], rate, SAMPLE_RATE)
    return out if a.dim() == 2 else out[0]


# ------------------------------------------------------------------------------------------------- time stretch
# audiomentations' TimeStretch(leave_length_unchanged=False) in its `librosa_phase_vocoder` form (librosa.effects.time_stretch), restated
# (include/wft.h "Time stretch" states the definition).  Neither library is a dependency: parity with their binaries is unpinned, and
# current audiomentations defaults to another method (a C++ library) that cannot be restated.
STRETCH_MIN_RATE, STRETCH_MAX_RATE = K.STRETCH_MIN_RATE, K.STRETCH_MAX_RATE


def check_stretch_range(min_rate, max_rate):
    """The TimeStretch range of a loader -> (min, max) as floats; outside [0.5, 2.0] or min > max raises ValueError."""
    lo, hi = float(min_rate), float(max_rate)
    if not (STRETCH_MIN_RATE <= lo <= STRETCH_MAX_RATE and STRETCH_MIN_RATE <= hi <= STRETCH_MAX_RATE):
        raise ValueError(f"time_stretch rates must lie in [{STRETCH_MIN_RATE}, {STRETCH_MAX_RATE}], got min_rate {min_rate}, max_rate {max_rate}")
    if lo > hi:
        raise ValueError(f"time_stretch_min_rate {min_rate} is larger than time_stretch_max_rate {max_rate}")
    return lo, hi


def time_stretch(audio, rate, device=None):
    """audio stretched in time by `rate` (> 1: faster and shorter), on the device (K.time_stretch: the phase vocoder).

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array; a host input goes to `device` (default: the current GPU) first.
    rate: one rate, or one per row, inside [0.5, 2.0] (ValueError otherwise).  Returns a list of B device tensors of their own
    lengths round(n / rate_b) for 2-D input, or one tensor for 1-D input.  rate == 1.0 runs the same kernels."""
    a = torch.as_tensor(audio)
    if a.dim() not in (1, 2) or a.dtype != torch.float32 or a.numel() == 0:
        raise ValueError(f"time_stretch: audio must be a non-empty float32 [n] or [B, n], got {a.dtype} {tuple(a.shape)}")
    rows = a if a.dim() == 2 else a[None]
    rates = K.stretch_rates(rate, rows.shape[0])  # before anything touches the device
    if device is not None:
        rows = rows.to(device)
    elif not rows.is_cuda:
        rows = rows.to(torch.device("cuda", torch.cuda.current_device()))
    out, _ = K.time_stretch(rows, rates)
    n = rows.shape[1]
    parts = [out[b, :int(round(n / float(rates[b])))] for b in range(rows.shape[0])]
    return parts if a.dim() == 2 else parts[0]


# ------------------------------------------------------------------------------------------------- IIR filters
# The filter group of the reference's advanced pipeline (data/filters.py designs and draws the seven kinds) and any user-supplied
# cascade of second-order sections, e.g. pre-emphasis or hum removal (include/wft.h "IIR filter" states the arithmetic).
from whisper_finetune.data.filters import design as design_filter  # noqa: E402,F401


def sos_filter(audio, sos, device=None):
    """audio filtered by a cascade of second-order sections, on the device (K.sos_filter).

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array; a host input goes to `device` (default: the current GPU) first.
    sos: f64 [S, 6] (one filter for every row) or [B, S, 6], rows b0 b1 b2 a0 a1 a2 with a0 == 1, S in 1..4 (ValueError otherwise),
    e.g. `design_filter("high_pass", cutoff_freq=80.0, order=2)`.  Returns a new device tensor of the input's shape."""
    a = torch.as_tensor(audio)
    if a.dim() not in (1, 2) or a.dtype != torch.float32 or a.numel() == 0:
        raise ValueError(f"sos_filter: audio must be a non-empty float32 [n] or [B, n], got {a.dtype} {tuple(a.shape)}")
    rows = a if a.dim() == 2 else a[None]
    coeffs = K.sos_coefficients(sos.detach().cpu() if torch.is_tensor(sos) else np.asarray(sos), rows.shape[0])  # before the device is touched
    if device is not None:
        rows = rows.to(device)
    elif not rows.is_cuda:
        rows = rows.to(torch.device("cuda", torch.cuda.current_device()))
    out = K.sos_filter(rows, coeffs)
    return out if a.dim() == 2 else out[0]


# ------------------------------------------------------------------------------------------------- wave effects
# Additive Gaussian noise, clipping distortion, gain, gain transition and shift (data/wave_fx.py draws them for the loader;
# include/wft.h "Wave effects" states the arithmetic).
from whisper_finetune.data.wave_fx import STAGE_OF as _WAVE_STAGE_OF, table_row as _wave_table_row  # noqa: E402


def wave_fx(audio, kind, device=None, **params):
    """audio under ONE wave effect, the same for every row, on the device (K.wave_fx).

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array; a host input goes to `device` (default: the current GPU) first.
    kind and its keywords (ValueError otherwise; data/wave_fx.py table_row):
      "gaussian_noise", amplitude=, seed=      "gaussian_snr", snr_db=, seed=       "clipping", q= (integer percent 0..50)
      "gain", gain_db=       "gain_transition", start_db=, end_db=, t0=, length= (samples)       "shift", fraction=, fade_len=0 (samples)
    Rows of a batch share the seed, so they get the same noise; use K.wave_fx with one record per row for per-row parameters.
    Returns a new device tensor of the input's shape."""
    a = torch.as_tensor(audio)
    if a.dim() not in (1, 2) or a.dtype != torch.float32 or a.numel() == 0:
        raise ValueError(f"wave_fx: audio must be a non-empty float32 [n] or [B, n], got {a.dtype} {tuple(a.shape)}")
    row = _wave_table_row(kind, **params)  # before the device is touched
    rows = a if a.dim() == 2 else a[None]
    if device is not None:
        rows = rows.to(device)
    elif not rows.is_cuda:
        rows = rows.to(torch.device("cuda", torch.cuda.current_device()))
    out = K.wave_fx(rows, row, _WAVE_STAGE_OF[kind])
    return out if a.dim() == 2 else out[0]


# ------------------------------------------------------------------------------------------------- rate effects
# Pitch shift and aliasing (data/rate_fx.py draws them for the loader; include/wft.h "Per-row rate conversion" states the arithmetic).
from whisper_finetune.data.rate_fx import PITCH_MAX_SEMITONES  # noqa: E402  (12: 2^(12/12) = 2.0, the end of the time stretch's range)


def pitch_rates(semitones, B: int):
    """One shift in semitones or one per row -> the float64 [B] rates 2^(-s/12) of the time stretch (and ratios of the resampler);
    a shift outside [-12, 12] (or NaN) raises ValueError."""
    s = K._row_values(semitones, B, "pitch_shift", "semitones")
    if not bool(np.all((s >= -PITCH_MAX_SEMITONES) & (s <= PITCH_MAX_SEMITONES))):
        raise ValueError(f"pitch_shift: semitones must lie in [{-PITCH_MAX_SEMITONES}, {PITCH_MAX_SEMITONES}], got {s.tolist()}")
    return np.clip(2.0 ** (-s / 12.0), K.STRETCH_MIN_RATE, K.STRETCH_MAX_RATE)  # (the clip only guards the last ulp at +-12)


def pitch_shift_rows(rows, rates):
    """rows f32 [B, n] on the device, rates float64 [B] from pitch_rates -> f32 [B, n]: K.time_stretch by the rate, then
    K.sinc_resample_rows by the same ratio back to n samples."""
    stretched, n_out = K.time_stretch(rows, rates)
    return K.sinc_resample_rows(stretched, n_out, rates, int(rows.shape[1]))


def pitch_shift(audio, semitones, device=None):
    """audio shifted in pitch by `semitones` at unchanged length, on the device: librosa.effects.pitch_shift's definition, a time
    stretch by 2^(-s/12) (the phase vocoder) followed by a resample back to the input's length (this project's Hann-windowed sinc;
    not librosa's soxr_hq: parity unpinned).

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array; a host input goes to `device` (default: the current GPU) first.
    semitones: one value or one per row, inside [-12, 12] (ValueError otherwise).  Returns a new device tensor of the input's shape."""
    a = torch.as_tensor(audio)
    if a.dim() not in (1, 2) or a.dtype != torch.float32 or a.numel() == 0:
        raise ValueError(f"pitch_shift: audio must be a non-empty float32 [n] or [B, n], got {a.dtype} {tuple(a.shape)}")
    rows = a if a.dim() == 2 else a[None]
    rates = pitch_rates(semitones, rows.shape[0])  # before the device is touched
    if device is not None:
        rows = rows.to(device)
    elif not rows.is_cuda:
        rows = rows.to(torch.device("cuda", torch.cuda.current_device()))
    out = pitch_shift_rows(rows, rates)
    return out if a.dim() == 2 else out[0]


def alias(audio, new_sample_rate, device=None, sample_rate: int = SAMPLE_RATE):
    """audio under audiomentations' Aliasing: linear interpolation down to `new_sample_rate` Hz and back, without a low-pass, on the
    device (K.alias: numpy's result bit for bit).

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array; a host input goes to `device` (default: the current GPU) first.
    new_sample_rate: one rate or one per row, inside [1000, 2 * sample_rate], or 0 for "leave the row as it is" (ValueError
    otherwise).  Returns a new device tensor of the input's shape."""
    a = torch.as_tensor(audio)
    if a.dim() not in (1, 2) or a.dtype != torch.float32 or a.numel() == 0:
        raise ValueError(f"alias: audio must be a non-empty float32 [n] or [B, n], got {a.dtype} {tuple(a.shape)}")
    rows = a if a.dim() == 2 else a[None]
    rates = K.alias_rates(new_sample_rate, rows.shape[0], float(check_rate(sample_rate)))  # before the device is touched
    if device is not None:
        rows = rows.to(device)
    elif not rows.is_cuda:
        rows = rows.to(torch.device("cuda", torch.cuda.current_device()))
    out = K.alias(rows, rates, None, sample_rate)
    return out if a.dim() == 2 else out[0]


# ------------------------------------------------------------------------------------------------- office effects
# Room reverb and bit crush (data/office_fx.py designs and draws them for the loader; include/wft.h "Office effects" states the arithmetic).
from whisper_finetune.data.office_fx import room_ir  # noqa: E402,F401  (the shoebox response, designed on the host)


def _rows(audio, who: str):
    """audio (f32 [n] or [B, n], a tensor or an array) -> (the input as a tensor, its rows [B, n]); ValueError otherwise."""
    a = torch.as_tensor(audio)
    if a.dim() not in (1, 2) or a.dtype != torch.float32 or a.numel() == 0:
        raise ValueError(f"{who}: audio must be a non-empty float32 [n] or [B, n], got {a.dtype} {tuple(a.shape)}")
    return a, (a if a.dim() == 2 else a[None])


def _to_device(rows, device):
    if device is not None:
        return rows.to(device)
    return rows if rows.is_cuda else rows.to(torch.device("cuda", torch.cuda.current_device()))


def fir_convolve(audio, ir, device=None):
    """audio convolved with an impulse response at unchanged length, on the device (K.fir_conv: FFT overlap-save in f32; the tail
    behind the input's end is dropped) — audiomentations' ApplyImpulseResponse with leave_length_unchanged=True, without its
    normalisation; the form for measured impulse responses.

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array; a host input goes to `device` (default: the current GPU) first.
    ir: ONE response for every row (1-D, a tensor or an array), or a list of B responses of ragged lengths; float32 or float64,
    1 to 8192 taps each (ValueError otherwise).  Returns a new device tensor of the input's shape."""
    a, rows = _rows(audio, "fir_convolve")
    B = rows.shape[0]
    irs = list(ir) if isinstance(ir, (list, tuple)) else [ir]
    irs = [np.asarray(h.detach().cpu().numpy() if torch.is_tensor(h) else h) for h in irs]
    if len(irs) not in (1, B):
        raise ValueError(f"fir_convolve: {len(irs)} impulse responses for {B} rows")
    for h in irs:
        if h.ndim != 1 or h.dtype not in (np.float32, np.float64) or not 1 <= h.shape[0] <= K.FIR_TAPS_MAX or not np.all(np.isfinite(h)):
            raise ValueError(f"fir_convolve: an impulse response must be 1 to {K.FIR_TAPS_MAX} finite float32 / float64 taps, got "
                             f"{h.dtype} {tuple(h.shape)}")
    taps = np.array([h.shape[0] for h in irs], dtype=np.int32)
    table = np.zeros((len(irs), int(taps.max())), dtype=np.float32)
    for b, h in enumerate(irs):
        table[b, :h.shape[0]] = h
    rows = _to_device(rows, device)
    ir_d = torch.from_numpy(table).to(rows.device)
    if len(irs) == 1:
        out = K.fir_conv(rows, ir_d[0])
    else:
        out = K.fir_conv(rows, ir_d, None, torch.from_numpy(taps).to(rows.device))
    return out if a.dim() == 2 else out[0]


def bit_crush(audio, bit_depth, device=None):
    """audio under audiomentations' BitCrush: round(x * q) / q with q = 2^(bit_depth - 1) + 1, on the device (K.bitcrush: numpy's
    float32 result bit for bit).

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array; a host input goes to `device` (default: the current GPU) first.
    bit_depth: one integer or one per row, inside [1, 24], or 0 for "leave the row as it is" (ValueError otherwise).
    Returns a new device tensor of the input's shape."""
    a, rows = _rows(audio, "bit_crush")
    depths = K.bitcrush_depths(bit_depth, rows.shape[0])  # before the device is touched
    out = K.bitcrush(_to_device(rows, device), depths)
    return out if a.dim() == 2 else out[0]


# ------------------------------------------------------------------------------------------------- mix effects
# Loudness (ITU-R BS.1770) and background noise (data/mix_fx.py designs and draws them for the loader; include/wft.h "Loudness and
# background noise" states the arithmetic).
from whisper_finetune.data import mix_fx as _MF  # noqa: E402
from whisper_finetune.data.mix_fx import k_weighting  # noqa: E402,F401  (the meter's two biquads as sos f64 [2, 6])


def loudness(audio, sample_rate: int = SAMPLE_RATE, device=None):
    """The integrated loudness of audio in LUFS, on the device (K.loudness: the ITU-R BS.1770 meter, pyloudnorm's
    Meter(rate).integrated_loudness for one channel, restated).

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array; a host input goes to `device` (default: the current GPU) first.
    sample_rate: an integer multiple of 10 inside [8000, 384000] (ValueError otherwise).  Returns a float64 device tensor, [B] for 2-D
    input, a scalar for 1-D; -inf for a row without a block over the gates or shorter than 400 ms (pyloudnorm raises there)."""
    a, rows = _rows(audio, "loudness")
    _MF.loudness_hop(sample_rate)  # before the device is touched
    _, stats = K.loudness(_to_device(rows, device), sample_rate)
    return stats[:, 0].clone() if a.dim() == 2 else stats[0, 0].clone()


def loudness_normalize(audio, target_lufs, sample_rate: int = SAMPLE_RATE, device=None):
    """audio brought to `target_lufs` by one gain per row, on the device (K.loudness: pyloudnorm's normalize.loudness on the meter's
    reading — audiomentations' LoudnessNormalization; no clipping afterwards).

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array; target_lufs: one value or one per row inside [-200, 200], NaN = "leave
    the row as it is" (ValueError otherwise).  A row that reads -inf is copied.  Returns a new device tensor of the input's shape."""
    a, rows = _rows(audio, "loudness_normalize")
    _MF.loudness_hop(sample_rate)
    t = K._row_values(target_lufs, rows.shape[0], "loudness_normalize", "targets")
    out, _ = K.loudness(_to_device(rows, device), sample_rate, t)
    return out if a.dim() == 2 else out[0]


def mix_background(audio, noise, snr_db=None, absolute_rms_db=None, offset=0, device=None):
    """audio with background noise added at a signal-to-noise ratio or at an absolute RMS level, on the device (K.bg_mix:
    audiomentations' AddBackgroundNoise, restated; a noise shorter than the audio repeats, a silent one leaves the row as it is).

    audio: f32, 1-D [n] or 2-D [B, n], a tensor or an array.  noise: ONE mono float32 recording for every row (1-D, a tensor or an
    array) or a ragged list of B recordings.  Exactly one of snr_db / absolute_rms_db: one value in dB or one per row (NaN = "leave
    the row as it is").  offset: one integer or one per row, where the segment starts inside the noise; it must lie inside the
    recording and is pulled back to m - n when the recording of m samples is longer than the audio's n (so the segment never wraps),
    and to 0 when it is not.  ValueError otherwise.  Returns a new device tensor of the input's shape."""
    a, rows = _rows(audio, "mix_background")
    B = rows.shape[0]
    if (snr_db is None) == (absolute_rms_db is None):
        raise ValueError("mix_background: give exactly one of snr_db and absolute_rms_db")
    kind = _MF.KIND_ID["snr" if absolute_rms_db is None else "absolute"]
    db = K._row_values(snr_db if absolute_rms_db is None else absolute_rms_db, B, "mix_background", "dB values")
    off = K._row_values(offset, B, "mix_background", "offsets")
    entries = _MF.load_bank(list(noise) if isinstance(noise, (list, tuple)) else [noise])
    if len(entries) not in (1, B):
        raise ValueError(f"mix_background: {len(entries)} noise recordings for {B} rows")
    on = ~np.isnan(db)
    table = _MF.none_table(B)
    table[:, 0] = np.where(on, float(kind), 0.0)
    table[:, 1] = np.arange(B) if len(entries) == B else 0
    table[:, 2], table[:, 3] = off, np.where(on, db, 0.0)
    lengths = [e.shape[0] for e in entries]
    rec = _MF.records_from_table(_MF.check_table(table, lengths))  # before the device is touched
    rows = _to_device(rows, device)
    bank, bank_off = _MF.pack_bank(entries)
    out, _ = K.bg_mix(rows, torch.from_numpy(bank).to(rows.device), torch.from_numpy(bank_off).to(rows.device), rec, lengths=lengths)
    return out if a.dim() == 2 else out[0]


# ------------------------------------------------------------------------------------------------- audio files
# WAV recordings and headerless PCM, decoded and downmixed on the device (data/audio_io.py parses the header on the host;
# include/wft.h "PCM decode" states the arithmetic).
from whisper_finetune.data import audio_io as _AIO  # noqa: E402
from whisper_finetune.data.audio_io import WavInfo, parse_wav  # noqa: E402,F401


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def decode_pcm(raw, format, channels: int = 1, channel="mean", frames=None, byte_offset: int = 0, device=None):
    """Headerless PCM -> mono f32 [frames] on the device (K.pcm_decode, one launch).

    raw: `bytes`, a `memoryview`, a uint8 array or a uint8 tensor (a host input goes to `device`, default the current GPU, as it is:
    1 to 8 bytes per sample).  format: "u8", "s16le", "s24le", "s32le", "f32le", "f64le", "alaw" or "ulaw"; channels: 1..8,
    interleaved; channel: "mean" (the fp64 mean of the channels) or the index of one channel; frames: how many frames to decode
    (None: all whole frames behind byte_offset); byte_offset: where the first frame starts, any alignment.  Integer formats are
    scaled by their full range (s16 / 2^15, ...: libsndfile's and scipy's convention).  ValueError before the device is touched."""
    if torch.is_tensor(raw):
        buf = raw
        if buf.dtype != torch.uint8 or buf.dim() != 1:
            raise ValueError(f"decode_pcm: a tensor must be uint8 [nbytes], got {buf.dtype} {tuple(buf.shape)}")
    else:
        try:
            buf = torch.from_numpy(np.frombuffer(memoryview(raw).cast("B"), dtype=np.uint8).copy())
        except TypeError:
            raise ValueError(f"decode_pcm: raw must be bytes, a memoryview, a uint8 array or a uint8 tensor, got {type(raw).__name__}") from None
    fmt = _AIO.format_id(format)
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= _AIO.MAX_CHANNELS:
        raise ValueError(f"decode_pcm: channels must be an integer inside [1, {_AIO.MAX_CHANNELS}], got {channels!r}")
    if isinstance(byte_offset, bool) or not isinstance(byte_offset, (int, np.integer)) or byte_offset < 0:
        raise ValueError(f"decode_pcm: byte_offset must be a non-negative integer, got {byte_offset!r}")
    fb = int(channels) * _AIO.SAMPLE_BYTES[fmt]
    if frames is None:
        frames = (int(buf.numel()) - int(byte_offset)) // fb
    if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or frames < 1:
        raise ValueError(f"decode_pcm: at least one whole frame is needed, got frames = {frames!r}")
    rows, n_max = _AIO.pcm_rows([(int(byte_offset), int(frames), int(channels), fmt, channel)], int(buf.numel()))  # before the device is touched
    buf = buf.contiguous().to(_device(device) if (device is not None or not buf.is_cuda) else buf.device)
    return K.pcm_decode(buf, rows, n_max)[0]


def _decode_files(sources, channel, device, who: str):
    """WAV sources (paths or bytes) -> (their mono f32 recordings at their own rates as device tensors, their WavInfo): every payload
    in ONE host byte buffer, one host-to-device copy, one wft_pcm_decode_f32 launch.  A recording that holds a sample that is not
    finite raises ValueError with its source named."""
    infos, parts, total = [], [], 0
    for k, src in enumerate(sources):
        if not isinstance(src, (str, bytes, bytearray, memoryview)) and not hasattr(src, "__fspath__"):
            raise ValueError(f"{who}: source {k} must be a path or the bytes of a WAV file, got {type(src).__name__}")
        info = parse_wav(src)
        payload = _AIO.read_payload(src, info)
        infos.append(info)
        parts.append((total, payload))
        total = (total + payload.shape[0] + 15) // 16 * 16  # every payload starts on a 16-byte granule of the buffer
    rows = [(off, info.frames, info.channels, info.format, _AIO.channel_id(channel, info.channels)) for (off, _), info in zip(parts, infos)]
    rec, n_max = _AIO.pcm_rows(rows, total)
    host = np.zeros(total, dtype=np.uint8)
    for off, payload in parts:
        host[off:off + payload.shape[0]] = payload
    dev = _device(device)
    out = K.pcm_decode(torch.from_numpy(host).to(dev), rec, n_max)
    finite = torch.isfinite(out).all(dim=1).cpu().tolist()
    for k, ok in enumerate(finite):
        if not ok:
            src = sources[k]
            name = repr(os.fspath(src)) if isinstance(src, (str, os.PathLike)) else f"source {k} ({len(src)} bytes)"
            raise ValueError(f"{who}: {name} holds a sample that is not finite")
    return [out[k, :info.frames] for k, info in enumerate(infos)], infos


def load_audio(sources, sample_rate: int = SAMPLE_RATE, channel="mean", device=None, return_info: bool = False):
    """WAV files -> mono f32 recordings at `sample_rate` Hz on the device.

    sources: one path or the `bytes` of one file, or a list of them (data/audio_io.py parse_wav says what is read: RIFF/WAVE with
    integer PCM, IEEE float, A-law or u-law, 1 to 8 channels).  channel: "mean" or the index of one channel (it must exist in every
    file).  All payloads go to the device in ONE host-to-device copy, as the bytes of the file, and ONE wft_pcm_decode_f32 launch
    decodes them; files at another rate are then resampled (K.resample), the files of equal rate and length together, so every
    result is bit-equal to decoding and resampling that file alone.  A recording with a sample that is not finite raises ValueError
    naming it.  -> one tensor [n] for one source, a list for a list; with return_info=True (recordings, WavInfo or list of WavInfo)."""
    single = isinstance(sources, (str, bytes, bytearray, memoryview)) or hasattr(sources, "__fspath__")
    srcs = [sources] if single else list(sources)
    if not srcs:
        raise ValueError("load_audio: at least one source is needed")
    rate = check_rate(sample_rate)
    rows, infos = _decode_files(srcs, channel, device, "load_audio")
    out = [None] * len(srcs)
    groups = {}
    for k, info in enumerate(infos):
        if info.sample_rate == rate:
            out[k] = rows[k].clone()
        else:
            groups.setdefault((info.sample_rate, info.frames), []).append(k)
    for (src_rate, _), ks in groups.items():
        res = K.resample(torch.stack([rows[k] for k in ks]), src_rate, rate)
        for i, k in enumerate(ks):
            out[k] = res[i] if len(ks) > 1 else res[0]
    if return_info:
        return (out[0], infos[0]) if single else (out, infos)
    return out[0] if single else out


from whisper_finetune.data.transforms import FrequencyMasking, TimeMasking, draw_mask_span  # noqa: E402,F401


def draw_clip_params(should_apply, warp_w: int, time_masking, freq_masking, n_mels: int, extremes, T: int = N_FRAMES):
    """Host draws of ONE clip in the order `AudioDataset._calculate_mel` makes them (data/data_loader.py:284-290):
    gate -> warp `randint(W, T-W)`, `randint(-W, W)` (data/utils.py:107,111) -> time span -> frequency span -> extremes
    ratio.  Returns (params i32 [8] = {apply_warp, warp_p, warp_d, t0, t1, f0, f1, 0}, extremes i32 [2]) for wft_specaug.
    `should_apply` is a callable (the dataset's `_should_apply_spec_augment`); the maskers offer `draw(size)`;
    `extremes` is an ExtremesFrequencyMasking or None."""
    params = np.zeros(8, dtype=np.int32)
    ext = np.zeros(2, dtype=np.int32)
    if should_apply():
        warp_p = int(torch.randint(warp_w, T - warp_w, (1,)))
        warp_d = int(torch.randint(-warp_w, warp_w, (1,)))
        t0, t1 = time_masking.draw(T)
        f0, f1 = freq_masking.draw(n_mels)
        params[:] = (1, warp_p, warp_d, t0, t1, f0, f1, 0)
    if extremes is not None:
        r = torch.rand(1).item()
        ext[:] = (int(round(r * extremes.low_freq_range)), int(round(r * extremes.high_freq_range)))
    return torch.from_numpy(params), torch.from_numpy(ext)


class GpuFrontend:
    def __init__(self, n_mels: int, device, spec_augment: bool = False, spec_augment_params: Optional[dict] = None,
                 extremes_spec_augment: bool = False, extremes_spec_augment_params: Optional[dict] = None):
        self.n_mels = n_mels
        self.device = torch.device(device)
        self.filters = mel_filters(n_mels).to(self.device)
        self.spec_augment = spec_augment
        p = spec_augment_params or {}
        self.p = float(p.get("p", 1.0)) if spec_augment else 0.0
        if spec_augment and not 0.0 <= self.p <= 1.0:
            raise ValueError(f"spec_augment p must be between 0 and 1, got {self.p}")
        self.time_mask_param = p.get("time_mask_param", 0)
        self.freq_mask_param = p.get("freq_mask_param", 0)
        self.time_warp_w = p.get("time_warp_w", 0)
        e = extremes_spec_augment_params or {}
        self.extremes = extremes_spec_augment
        self.low_freq_range = e.get("low_freq_range", 0)
        self.high_freq_range = e.get("high_freq_range", 0)

    def _should_apply(self) -> bool:
        if not self.spec_augment or self.p <= 0.0:
            return False
        return True if self.p >= 1.0 else torch.rand(1).item() < self.p

    def draw(self, batch: int, T: int = N_FRAMES):
        """Host draws for a batch -> (params i32 [B,8], extremes i32 [B,2]) in the reference's per-clip order."""
        from whisper_finetune.data.utils import ExtremesFrequencyMasking

        tm, fm = TimeMasking(self.time_mask_param), FrequencyMasking(self.freq_mask_param)
        ex = ExtremesFrequencyMasking(self.low_freq_range, self.high_freq_range) if self.extremes else None
        rows = [draw_clip_params(self._should_apply, self.time_warp_w, tm, fm, self.n_mels, ex, T) for _ in range(batch)]
        return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])

    def log_mel(self, audio: torch.Tensor) -> torch.Tensor:
        """audio f32 [B, 480000] on the device -> f32 [B, n_mels, 3000]."""
        return K.logmel(audio, self.filters, audio.shape[1] // HOP_LENGTH)

    def __call__(self, audio: torch.Tensor, training: bool = True) -> torch.Tensor:
        mel = self.log_mel(audio)
        if training and (self.spec_augment or self.extremes):
            params, ext = self.draw(audio.shape[0], mel.shape[-1])
            if params[:, 0].any() or ext.any():
                mel = K.specaug(mel, params.to(self.device, non_blocking=True), ext.to(self.device, non_blocking=True))
        return mel
