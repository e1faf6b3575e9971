"""Data path with the reference's names (data/data_loader.py): AudioDataset, collate_fn, WarmupDatasetSampler,
get_dataset_boundary_indices, get_dataloader — re-cut for the GPU front end.

What moved: the reference computes log-mel + SpecAugment per clip on the CPU inside DataLoader workers and ships
[n_mels, 3000] fp32 mels; here a worker only builds the token sequences, zero-pads the raw audio to 30 s and DRAWS the
augmentation parameters (same default-generator draw order as `AudioDataset.__getitem__` / `_calculate_mel`,
data_loader.py:322-359,273-301), and the main process turns a pinned batch of raw clips into mels with two kernels
(`wft_logmel`, `wft_specaug`).  `get_dataloader(...)` still yields `(mel, y_in, y_out)` batches: mel f32
[B, n_mels, 3000] (on the GPU), y_in padded with 0, y_out padded with -100.

Clips at another rate than 16 kHz (`get_dataloader(..., sample_rate=)`, one rate per loader): a worker pads the clip to
30 * sample_rate samples and the main process resamples the staged [B, 30 * rate] batch to [B, 480000] with one
`wft_resample_f32` launch in front of the log-mel.

Time stretch (`apply_baseline_aug=True`: the reference's baseline audio augmentation, TimeStretch(min_rate, max_rate,
leave_length_unchanged=False, p=1.0)): a worker only DRAWS the clip's rate; the main process stretches the staged zero-padded batch with
`wft_time_stretch_f32` (the reference stretches the padded clip too) and takes the log-mel of the rows' different lengths with
`wft_logmel_ragged`.  The reference neither rescales the timestamps nor `next_partial_segment_start` under a stretch; neither does this.

Filter augmentation (`filter_aug={...}`, an option of this project's own: the filter group of the reference's advanced pipeline, NOT
`apply_advanced_aug`, which stays refused): a worker only DRAWS and designs the clip's filter (data/filters.py FilterAug, after the
stretch-rate draw: the reference's Compose order); the main process runs `wft_sos_filter_f32` in place on the staged batch behind
the resample and the stretch and in front of the log-mel.  The zero padding is filtered too, as the reference filters the padded clip.

Wave effects (`wave_aug={...}`, an option of this project's own: additive Gaussian noise, clipping distortion, gain, gain transition
and shift of the reference's advanced pipeline, NOT `apply_advanced_aug`): a worker only DRAWS the clip's parameters (data/wave_fx.py
WaveAug, after the filter draw) and ships them as one table row f64 [14]; the main process runs `wft_wave_fx_f32` in place, one stage
per call, in the reference's Compose order: resample -> stretch -> NOISE -> filter -> CLIP -> LEVEL -> log-mel.  Every stage covers
the row's full stretched length, padding included (the reference transforms the padded clip), and a stage with no active row launches
nothing.  Timestamps are not moved under `shift`, as in the reference.

Rate effects (`rate_aug={...}`, an option of this project's own: Aliasing and PitchShift of the reference's advanced pipeline, NOT
`apply_advanced_aug`): a worker only DRAWS the clip's parameters (data/rate_fx.py RateAug, after the wave-effects draw) and ships them
as one table row f64 [4]; the main process runs `wft_alias_f32` and the pitch shift (`wft_time_stretch_f32` +
`wft_sinc_resample_rows_f32`) in the reference's Compose order: resample -> stretch -> NOISE -> ALIAS -> filter -> CLIP -> LEVEL ->
PITCH -> log-mel, each over the row's full stretched length.  Alias writes into a second buffer that takes the first one's place;
pitch gathers the pitched rows only.  Timestamps are untouched, as in the reference.

Office effects (`office_aug={...}`, an option of this project's own: BitCrush and the RoomSimulator of the reference's office pipeline,
NOT `apply_office_aug`): a worker DRAWS the clip's bit depth and DESIGNS its room's impulse response (data/office_fx.py OfficeAug, after
the rate-effects draw) and ships them as one table row f64 [2 + cap]; the main process runs `wft_bitcrush_f32` (in place) and
`wft_fir_conv_f32` (into a second buffer) right behind the stretch, the reference's Compose order: resample -> stretch -> CRUSH -> ROOM
-> NOISE -> ALIAS -> filter -> CLIP -> LEVEL -> PITCH -> log-mel.  Timestamps are untouched.

Mix effects (`mix_aug={...}`, an option of this project's own: AddBackgroundNoise and LoudnessNormalization of the reference's advanced
pipeline, NOT `apply_advanced_aug`): a worker DRAWS the clip's noise entry, offset and level and its loudness target (data/mix_fx.py
MixAug, after the office-effects draw; it knows the bank's entry lengths only) and ships them as one table row f64 [6], the LAST field
of a batch; `GpuMelLoader` loads the noise bank once, keeps it on the device and runs `wft_bg_mix_f32` and `wft_loudness_f32` in place
at their places of the reference's Compose order: resample -> stretch -> crush -> room -> BACKGROUND -> noise -> LOUDNESS -> alias ->
filter -> clip -> level -> pitch -> log-mel, over the padded clip (the reference pads to 30 s before it augments).  AirAbsorption
and Mp3Compression stay unbuilt.  Timestamps are untouched.
"""
from __future__ import annotations

import random
import re
from typing import Iterator, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence
from torch.utils.data import DataLoader, Dataset

from whisper_finetune.data import transforms as T
from whisper_finetune.data.filters import FilterAug, identity_sos
from whisper_finetune.data.gpu_frontend import (HOP_LENGTH, N_FFT, N_FRAMES, N_SAMPLES, SAMPLE_RATE, GpuFrontend, check_rate,
                                                check_stretch_range, draw_clip_params, mel_filters)
from whisper_finetune.data.utils import ExtremesFrequencyMasking, TimeWarpAugmenter, pad_or_trim
from whisper_finetune.data.mix_fx import MixAug, STAGES as MIX_STAGES, check_table as check_mix_table, load_bank, pack_bank, records_from_table as bg_records_from_table
from whisper_finetune.data.office_fx import OfficeAug, STAGES as OFFICE_STAGES, check_table as check_office_table
from whisper_finetune.data.rate_fx import RateAug, check_table as check_rate_table
from whisper_finetune.data.wave_fx import STAGES as WAVE_STAGES, WaveAug, active_rows, check_records, records_from_table

CHUNK_LENGTH = 30
_TS = re.compile(r"(<\|[123]?[0-9]\.[0-9][0-9]\|>)")  # <|0.00|> .. <|30.00|>
_FILTERS = {}
_BANKS = {}  # the per-clip form's noise banks: (id of the MixAug, device) -> DeviceBank


def pitch_rows(audio, semitones, lengths=None):
    """The pitch shift of the rows whose entry of `semitones` (host, one per row) is not None, in place on audio f32 [B, ld]: the
    pitched rows are gathered, shifted (gpu_frontend.pitch_shift_rows: time stretch + sinc resample back to the row's length) and put
    back; the other rows keep their bits.  lengths: the rows' lengths as HOST integers (the stretched lengths; None = ld for every
    row).  wft_time_stretch_f32 takes one length per call, so the pitched rows go one call per distinct length."""
    from whisper_finetune.data.gpu_frontend import pitch_rates, pitch_shift_rows

    groups = {}
    for b, s in enumerate(semitones):
        if s is not None:
            groups.setdefault(int(audio.shape[1]) if lengths is None else int(lengths[b]), []).append(b)
    for length, rows in groups.items():
        if length < 1:
            continue
        idx = torch.tensor(rows, dtype=torch.int64).to(audio.device, non_blocking=True)
        part = audio.index_select(0, idx)[:, :length]
        shifted = pitch_shift_rows(part, pitch_rates([semitones[b] for b in rows], len(rows)))
        audio[:, :length].index_copy_(0, idx, shifted)
    return audio


def office_rows(audio, n, office):
    """CRUSH -> ROOM on audio f32 [B, ld] (device) from the checked office table f64 [B, 2 + cap] (data/office_fx.py): the bit crush in
    place over the rows' depths (0 = the row is copied), then the rows' room responses through K.fir_conv, whose output is RETURNED
    (a row without a response is copied).  A stage with no active row launches nothing."""
    import numpy as np

    from whisper_finetune.engine import kernels as K

    bits, taps = office[:, 0].astype(np.int32), office[:, 1].astype(np.int32)
    if bool(bits.any()):
        K.bitcrush(audio, bits, n, out=audio)
    if bool(taps.any()):
        ir = torch.from_numpy(office[:, 2:2 + int(taps.max())].astype(np.float32)).to(audio.device, non_blocking=True)
        audio = K.fir_conv(audio, ir, n, torch.from_numpy(taps).to(audio.device, non_blocking=True))
    return audio


class DeviceBank:
    """The noise bank of a MixAug on one device: the entries back to back f32 [total], their offsets i64 [K + 1] and the lengths
    as host integers.  A bank at another rate (`bank_sample_rate`) is resampled ONCE, entry by entry, through gpu_frontend.resample;
    a {"wav_dir": path} bank is gpu_frontend.load_audio over its files at the loader's rate (one copy of the file bytes, one decode
    launch, every file resampled from its own rate)."""

    def __init__(self, mix_aug: MixAug, device):
        from whisper_finetune.data.gpu_frontend import resample

        src = mix_aug.sample_rate if mix_aug.bank_sample_rate is None else mix_aug.bank_sample_rate
        if isinstance(mix_aug.bank, Mapping) and "wav_dir" in mix_aug.bank:  # .wav files: decoded, downmixed and resampled on the device
            from whisper_finetune.data.gpu_frontend import load_audio
            from whisper_finetune.data.mix_fx import wav_bank

            files, channel, _ = wav_bank(mix_aug.bank)
            parts = load_audio(files, sample_rate=mix_aug.sample_rate, channel=channel, device=device)
            self.lengths = [int(t.shape[0]) for t in parts]
            self.bank = torch.cat(parts).contiguous()
            self.off = torch.tensor(np.concatenate([[0], np.cumsum(self.lengths)]), dtype=torch.int64).to(device)
            if self.lengths != list(mix_aug.lengths):
                raise RuntimeError(f"noise bank: the device holds entries of {self.lengths} samples, the draws were made for {list(mix_aug.lengths)}")
            return
        entries = load_bank(mix_aug.bank, src)
        if src != mix_aug.sample_rate:
            parts = [resample(e, src, device) for e in entries]
            self.lengths = [int(t.shape[0]) for t in parts]
            self.bank = torch.cat(parts).contiguous()
            self.off = torch.tensor(np.concatenate([[0], np.cumsum(self.lengths)]), dtype=torch.int64).to(device)
        else:
            bank, off = pack_bank(entries)
            self.lengths = [int(e.shape[0]) for e in entries]
            self.bank, self.off = torch.from_numpy(bank).to(device), torch.from_numpy(off).to(device)
        if self.lengths != list(mix_aug.lengths):
            raise RuntimeError(f"noise bank: the device holds entries of {self.lengths} samples, the draws were made for {list(mix_aug.lengths)}")


def background_rows(audio, n, mix):
    """BACKGROUND on audio f32 [B, ld] (device), in place: mix = (the checked mix table f64 [B, 6], DeviceBank or None)."""
    from whisper_finetune.engine import kernels as K

    table, bank = mix
    if bool(table[:, 0].any()):
        K.bg_mix(audio, bank.bank, bank.off, bg_records_from_table(table), n, out=audio, lengths=bank.lengths)
    return audio


def loudness_rows(audio, n, mix):
    """LOUDNESS on audio f32 [B, ld] (device), in place: the rows with loud_on are brought to their targets."""
    from whisper_finetune.engine import kernels as K

    table = mix[0]
    if bool(table[:, 4].any()):
        K.loudness(audio, SAMPLE_RATE, np.where(table[:, 4] != 0, table[:, 5], np.nan), n, out=audio)
    return audio


def apply_wave_stages(audio, n, sos, fx, rate=None, lengths=None, office=None, mix=None):
    """The audio-domain stages behind the stretch on audio f32 [B, ld] (device), in the reference's Compose order:
    CRUSH -> ROOM -> BACKGROUND -> NOISE -> LOUDNESS -> ALIAS -> filter -> CLIP -> LEVEL -> PITCH (mix: None, or the checked mix
    table f64 [B, 6] of data/mix_fx.py with the DeviceBank of its background rows; both of its stages run in place).  n: i32 [B] on the device or None; sos: f64 [B, 4, 6] or
    None; fx: checked wave-effect records [B] (data/wave_fx.py) or None; rate: the checked rate-effect table f64 [B, 4]
    (data/rate_fx.py) or None; lengths: the rows' lengths as host integers (what n holds; None with n None); office: the checked
    office table f64 [B, 2 + cap] (data/office_fx.py) or None.  A stage with no active row launches nothing.
    Every stage but ROOM and ALIAS runs in place; those two write a second buffer, so use the RETURNED tensor."""
    from whisper_finetune.engine import kernels as K

    if office is not None:
        audio = office_rows(audio, n, office)
    if mix is not None:
        background_rows(audio, n, mix)
    if fx is not None:
        K.wave_fx(audio, fx, "noise", n, out=audio)
    if mix is not None:
        loudness_rows(audio, n, mix)
    if rate is not None and bool(rate[:, 0].any()):
        audio = K.alias(audio, rate[:, 1], n, SAMPLE_RATE)  # out of place; a "none" row (rate 0) is copied
    if sos is not None:
        K.sos_filter(audio, sos, n, out=audio)
    if fx is not None:
        K.wave_fx(audio, fx, "clip", n, out=audio)
        K.wave_fx(audio, fx, "level", n, out=audio)  # (shift rows go through a temporary inside K.wave_fx)
    if rate is not None and bool(rate[:, 2].any()):
        pitch_rows(audio, [float(r[3]) if r[2] else None for r in rate], lengths)
    return audio


def stretched_lengths(n: int, rates):
    """The lengths wft_time_stretch_f32 gives rows of n samples, on the host: round(n / rate), the same float64 division and
    half-even rounding as the kernel's."""
    return [int(round(n / float(r))) for r in rates]


def log_mel_spectrogram(audio, n_mels: int = 80, padding: int = 0, device=None) -> torch.Tensor:
    """`whisper.audio.log_mel_spectrogram` (called at data/data_loader.py:278) on the `wft_logmel`
    kernel: audio f32 [n] (numpy or tensor, n a multiple of 160) -> f32 [n_mels, n/160] on the device.  There is no
    host implementation: without a GPU this raises (the batched product path is GpuMelLoader below)."""
    from whisper_finetune.engine import kernels as K
    from whisper_finetune.engine.lib import WftError

    if not torch.is_tensor(audio):
        audio = torch.from_numpy(np.asarray(audio, dtype=np.float32))
    if device is None and not audio.is_cuda:
        if not torch.cuda.is_available():
            raise WftError("log_mel_spectrogram runs on the GPU in this build (wft_logmel) and no device is visible")
        device = torch.device("cuda", torch.cuda.current_device())
    if device is not None:
        audio = audio.to(device)
    if padding > 0:
        audio = torch.nn.functional.pad(audio, (0, padding))
    if audio.dim() != 1 or audio.shape[0] % HOP_LENGTH:
        raise ValueError(f"expected a 1-D clip whose length is a multiple of {HOP_LENGTH}, got {tuple(audio.shape)}")
    key = (n_mels, audio.device)
    if key not in _FILTERS:
        _FILTERS[key] = mel_filters(n_mels).to(audio.device)
    return K.logmel(audio.float()[None], _FILTERS[key], audio.shape[0] // HOP_LENGTH)[0]


class AudioDataset(Dataset):
    """Items: (audio f32 [30 * sample_rate] (480000 at the default 16 kHz), decoder_input i64, decoder_output i64, aug i32 [8], extremes i32 [2], cut_frames);
    with `apply_baseline_aug` a seventh field, the clip's time-stretch rate as f64 (without it the items are the six fields, unchanged);
    with `filter_aug` one more field behind those, the clip's filter as sos f64 [4, 6] (identity sections = "do not filter");
    with `wave_aug` one more field behind the filter, the clip's wave effects as a table row f64 [14] (data/wave_fx.py);
    with `rate_aug` one more field behind the wave effects, the clip's rate effects as a table row f64 [4] (data/rate_fx.py);
    with `office_aug` one more field behind the rate effects, the clip's office effects as a table row f64 [2 + cap] (data/office_fx.py);
    with `mix_aug` one more field behind the office effects, the clip's mix effects as a table row f64 [6] (data/mix_fx.py).

    apply_baseline_aug: the rate is drawn as audiomentations draws it — Python's `random` module, one `random.random()` gate against
    p = 1.0, then `random.uniform(min_rate, max_rate)` (BaseWaveformTransform.randomize_parameters, then TimeStretch's).  That order is
    restated from the published source; audiomentations is not installed here, so it is unpinned.  The draw does not touch torch's
    generator: the SpecAugment draw order is the same with and without it.  Rates outside [0.5, 2.0] or min > max raise ValueError.
    apply_office_aug / apply_advanced_aug (room simulation, mp3 compression, background-noise files, biquad filters, pitch shift)
    are not implemented and raise NotImplementedError.
    filter_aug: None, or a mapping of data/filters.py FilterAug's keywords (`p`, `kinds`); `{}` = its defaults.  It is the filter group
    of the advanced pipeline alone.  The filter is drawn after the stretch rate, with Python's `random` (FilterAug's docstring states
    the order), designed for 16 kHz (it runs behind the resample), and never touches torch's generator.
    wave_aug: None, or a mapping of data/wave_fx.py WaveAug's groups (`noise`, `clip`, `level`, each None or {p, kinds}; a missing
    group is off).  The parameters are drawn after the filter, with Python's `random` (WaveAug's docstring states the order).
    rate_aug: None, or a mapping of data/rate_fx.py RateAug's groups (`alias`, `pitch`, each None or a mapping of its keywords; a
    missing group is off).  The parameters are drawn after the wave effects, with Python's `random`.
    office_aug: None, or a mapping of data/office_fx.py OfficeAug's groups (`crush`, `room`, each None or a mapping of its keywords; a
    missing group is off).  The parameters are drawn after the rate effects, with Python's `random`, and the room's impulse response
    is designed in the worker.  It is NOT `apply_office_aug`, which stays refused (mp3 compression is not built).
    mix_aug: None, or a mapping of data/mix_fx.py MixAug's groups (`background`, `loudness`, each None or a mapping of its keywords; a
    missing group is off; `background` needs `bank`).  The parameters are drawn after the office effects, with Python's `random`,
    for the padded clip of 480000 samples; the dataset keeps the bank's entry lengths only.  It is NOT `apply_advanced_aug`, which
    stays refused (air absorption is not built).

    hu_dataset: indexable records {"audio": {"array", optional "sampling_rate"}, "text", "language", optional "prompt"}; a record
    whose "sampling_rate" is present and differs from the dataset's `sample_rate` raises ValueError (no mixed rates); tokenizer: whisper-style
    (sot, eot, sot_prev, no_timestamps, no_speech, timestamp_begin, special_tokens[...], encode(text, **kw)).

    Same constructor arguments and attributes as the reference's class (data/data_loader.py:40-160).  `__getitem__`
    ships the raw clip plus the DRAWN augmentation parameters (the batch is turned into mels on the device by
    GpuMelLoader); `_calculate_mel` is the reference's per-clip form of the same arithmetic on the same kernels."""

    sample_rate, n_samples = SAMPLE_RATE, N_SAMPLES  # the defaults, also of an instance built without __init__
    apply_baseline_aug = False
    filter_aug = None
    wave_aug = None
    rate_aug = None
    office_aug = None
    mix_aug = None

    def __init__(self, hu_dataset, tokenizer, device=None, no_timestamp_training: bool = False, n_mels: int = 80,
                 max_prompt_length: int = 223, prompt_use_rate: float = 0.5, no_timestamps_rate: float = 0.5,
                 spec_augment: bool = False, spec_augment_params: Optional[dict] = None, extremes_spec_augment: bool = False,
                 extremes_spec_augment_params: Optional[dict] = None, apply_baseline_aug: bool = False, apply_office_aug: bool = False,
                 apply_advanced_aug: bool = False, time_stretch_min_rate: float = 0.8, time_stretch_max_rate: float = 1.25,
                 bpe_dropout: float = 0.0, sample_rate: int = SAMPLE_RATE, filter_aug: Optional[dict] = None,
                 wave_aug: Optional[dict] = None, rate_aug: Optional[dict] = None, office_aug: Optional[dict] = None,
                 mix_aug: Optional[dict] = None):
        self.sample_rate = check_rate(sample_rate)
        self.n_samples = CHUNK_LENGTH * self.sample_rate  # 30 s at the clips' own rate
        refused = [name for name, on in (("apply_office_aug", apply_office_aug), ("apply_advanced_aug", apply_advanced_aug)) if on]
        if refused:
            raise NotImplementedError(f"{' and '.join(refused)}: the office and advanced audio pipelines (room simulation, mp3 compression, "
                                      "background-noise files, biquad filters, pitch shift) are not implemented; "
                                      "apply_baseline_aug (time stretch) is; the office pipeline's bit crush and room simulation run "
                                      "behind this project's own option audio_augment.wft_office_aug, the advanced pipeline's "
                                      "background noise and loudness normalisation behind audio_augment.wft_mix_aug")
        if apply_baseline_aug:
            time_stretch_min_rate, time_stretch_max_rate = check_stretch_range(time_stretch_min_rate, time_stretch_max_rate)
        self.hu_dataset, self.tokenizer, self.n_mels, self.device = hu_dataset, tokenizer, n_mels, device
        self.no_timestamp_training = no_timestamp_training
        self.max_prompt_length, self.prompt_use_rate, self.no_timestamps_rate = max_prompt_length, prompt_use_rate, no_timestamps_rate
        self.spec_augment, self.extremes_spec_augment = spec_augment, extremes_spec_augment
        self.apply_baseline_aug = bool(apply_baseline_aug)
        self.apply_office_aug = self.apply_advanced_aug = False
        self.time_stretch_min_rate, self.time_stretch_max_rate = time_stretch_min_rate, time_stretch_max_rate
        self.bpe_dropout = bpe_dropout
        if filter_aug is not None and (not hasattr(filter_aug, "keys") or not set(filter_aug.keys()) <= {"p", "kinds"}):
            raise ValueError(f"filter_aug must be None or a mapping of FilterAug's keywords `p` and `kinds`, got {filter_aug!r}")
        self.filter_aug = FilterAug(sample_rate=SAMPLE_RATE, **dict(filter_aug)) if filter_aug is not None else None
        if wave_aug is not None and (not hasattr(wave_aug, "keys") or not set(wave_aug.keys()) <= set(WAVE_STAGES)):
            raise ValueError(f"wave_aug must be None or a mapping of WaveAug's groups {WAVE_STAGES}, got {wave_aug!r}")
        self.wave_aug = WaveAug(sample_rate=SAMPLE_RATE, **dict(wave_aug)) if wave_aug is not None else None
        if rate_aug is not None and (not hasattr(rate_aug, "keys") or not set(rate_aug.keys()) <= {"alias", "pitch"}):
            raise ValueError(f"rate_aug must be None or a mapping of RateAug's groups ('alias', 'pitch'), got {rate_aug!r}")
        self.rate_aug = RateAug(sample_rate=SAMPLE_RATE, **dict(rate_aug)) if rate_aug is not None else None
        if office_aug is not None and (not hasattr(office_aug, "keys") or not set(office_aug.keys()) <= set(OFFICE_STAGES)):
            raise ValueError(f"office_aug must be None or a mapping of OfficeAug's groups {OFFICE_STAGES}, got {office_aug!r}")
        self.office_aug = OfficeAug(sample_rate=SAMPLE_RATE, **dict(office_aug)) if office_aug is not None else None
        if mix_aug is not None and (not hasattr(mix_aug, "keys") or not set(mix_aug.keys()) <= set(MIX_STAGES)):
            raise ValueError(f"mix_aug must be None or a mapping of MixAug's groups {MIX_STAGES}, got {mix_aug!r}")
        self.mix_aug = MixAug(sample_rate=SAMPLE_RATE, **dict(mix_aug)) if mix_aug is not None else None
        if spec_augment:
            self.spec_augment_p = float(spec_augment_params.get("p", 1.0))
            if not 0.0 <= self.spec_augment_p <= 1.0:
                raise ValueError(f"spec_augment p must be between 0 and 1, got {self.spec_augment_p}")
            self.time_masking = T.TimeMasking(time_mask_param=spec_augment_params["time_mask_param"])
            self.freq_masking = T.FrequencyMasking(freq_mask_param=spec_augment_params["freq_mask_param"])
            self.time_warping = TimeWarpAugmenter(W=spec_augment_params["time_warp_w"])
        else:
            self.spec_augment_p = 0.0
            self.time_masking = self.freq_masking = self.time_warping = None
        self.extreme_freq_masking = (ExtremesFrequencyMasking(low_freq_range=extremes_spec_augment_params["low_freq_range"],
                                                              high_freq_range=extremes_spec_augment_params["high_freq_range"])
                                     if extremes_spec_augment else None)
        self.aud_augment = None
        self.num_frames_per_second = N_FRAMES / CHUNK_LENGTH
        self.timestamp_pattern = _TS
        self.model_n_text_ctx = 448
        cols = getattr(hu_dataset, "column_names", None)
        if cols is not None:
            assert {"audio", "text", "language"} <= set(cols), "dataset needs audio / text / language columns"
        self.invalid_indices = set()

    # ---- augmentation (reference: data_loader.py:273-301)
    def _should_apply_spec_augment(self) -> bool:
        if not self.spec_augment:
            return False
        if self.spec_augment_p >= 1.0:
            return True
        if self.spec_augment_p <= 0.0:
            return False
        return torch.rand(1).item() < self.spec_augment_p

    def _draw_stretch_rate(self) -> float:
        """audiomentations' draws for TimeStretch(p=1.0): the gate, then the rate (see the class docstring); 1.0 if the gate fails."""
        if random.random() < 1.0:
            return random.uniform(self.time_stretch_min_rate, self.time_stretch_max_rate)
        return 1.0

    def _draw_filter(self):
        """The clip's filter for the per-clip form: sos f64 [1, 4, 6], or None without the option or when the draw says "do not filter"."""
        if self.filter_aug is None:
            return None
        kind, _, sos = self.filter_aug.draw()
        return None if kind is None else sos[None]

    def _draw_wave(self):
        """The clip's wave effects for the per-clip form: checked records [1], or None without the option or when nothing was drawn."""
        if self.wave_aug is None:
            return None
        names, row = self.wave_aug.draw(N_SAMPLES)
        return check_records(records_from_table(row[None])) if any(names.values()) else None

    def _draw_rate(self):
        """The clip's rate effects for the per-clip form: the checked table f64 [1, 4], or None without the option or when nothing was drawn."""
        if self.rate_aug is None:
            return None
        names, row = self.rate_aug.draw()
        return check_rate_table(row[None]) if any(names.values()) else None

    def _draw_office(self):
        """The clip's office effects for the per-clip form: the checked table f64 [1, 2 + cap], or None without the option or when nothing was drawn."""
        if self.office_aug is None:
            return None
        names, row = self.office_aug.draw()
        return check_office_table(row[None]) if any(names.values()) else None

    def _draw_mix(self, device):
        """The clip's mix effects for the per-clip form: (the checked table f64 [1, 6], the DeviceBank or None), or None without the
        option or when nothing was drawn."""
        if self.mix_aug is None:
            return None
        names, row = self.mix_aug.draw(N_SAMPLES)
        if names["background"] is None and not names["loudness"]:
            return None
        bank = None
        if self.mix_aug.lengths is not None:
            key = (id(self.mix_aug), str(device))
            if key not in _BANKS:
                _BANKS[key] = DeviceBank(self.mix_aug, device)
            bank = _BANKS[key]
        return check_mix_table(row[None], self.mix_aug.lengths), bank

    def _calculate_mel(self, audio_array, next_partial_segment_start: Optional[float], no_timestamps: bool) -> torch.Tensor:
        """Per-clip form: [time stretch] -> [crush] -> [room] -> [noise] -> [alias] -> [filter] -> [clipping] -> [level] -> [pitch] -> log-mel -> cut at a partial segment + minimum-value pad -> [warp -> time mask -> freq mask]
        w.p. p -> extremes masking, every stage a libwft kernel on the device."""
        if self.sample_rate != SAMPLE_RATE:
            raise ValueError(f"_calculate_mel is the per-clip 16 kHz form; clips at {self.sample_rate} Hz are resampled per batch by GpuMelLoader")
        cut = (int(next_partial_segment_start * self.num_frames_per_second) if no_timestamps and next_partial_segment_start is not None
               else N_FRAMES)
        if self.apply_baseline_aug:  # the same two kernels as GpuMelLoader, on one row
            from whisper_finetune.engine import kernels as K

            dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
            row = torch.as_tensor(np.asarray(audio_array, dtype=np.float32)).to(dev)[None]
            stretch_rate = self._draw_stretch_rate()
            stretched, n_out = K.time_stretch(row, [stretch_rate])
            sos, fx, rt, office, mix = self._draw_filter(), self._draw_wave(), self._draw_rate(), self._draw_office(), self._draw_mix(dev)
            stretched = apply_wave_stages(stretched, n_out, sos, fx, rt, stretched_lengths(row.shape[1], [stretch_rate]), office, mix)
            key = (self.n_mels, row.device)
            if key not in _FILTERS:
                _FILTERS[key] = mel_filters(self.n_mels).to(row.device)
            keep = torch.tensor([min(cut, N_FRAMES)], dtype=torch.int32, device=row.device)
            mel = K.logmel_ragged(stretched, n_out, keep, _FILTERS[key], N_FRAMES)[0]
        else:
            sos, fx, rt, office = self._draw_filter(), self._draw_wave(), self._draw_rate(), self._draw_office()
            mix = None
            if self.mix_aug is not None:
                mix = self._draw_mix(self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device()))
            if sos is not None or fx is not None or rt is not None or office is not None or mix is not None:  # the same kernels as GpuMelLoader, on one row
                dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
                row = torch.as_tensor(np.asarray(audio_array, dtype=np.float32)).to(dev)[None].clone()
                audio_array = apply_wave_stages(row, None, sos, fx, rt, None, office, mix)[0]
            mel = log_mel_spectrogram(audio_array, n_mels=self.n_mels, device=self.device)
            if no_timestamps and next_partial_segment_start is not None:
                mel = mel[:, : int(next_partial_segment_start * self.num_frames_per_second)]
            if mel.shape[1] != N_FRAMES:
                mel = pad_or_trim(mel, N_FRAMES)
        if self._should_apply_spec_augment():
            mel = self.time_warping(mel)
            mel = self.time_masking(mel)
            mel = self.freq_masking(mel)
        if self.extreme_freq_masking:
            mel = self.extreme_freq_masking(mel)
        return mel

    def _draw_aug_params(self):
        """The draws `_calculate_mel` would make for one clip (same default-generator order), as kernel arguments."""
        return draw_clip_params(self._should_apply_spec_augment,
                                self.time_warping.W if self.time_warping is not None else 0,
                                self.time_masking, self.freq_masking, self.n_mels,
                                self.extreme_freq_masking, N_FRAMES)

    def __len__(self) -> int:
        return len(self.hu_dataset)

    # ---- records
    def _load_valid_record(self, index: int):
        """Corrupt rows are detected lazily and skipped: up to min(len, 32) successors are tried."""
        n = len(self.hu_dataset)
        if n == 0:
            raise IndexError("Dataset is empty.")
        attempts = min(n, 32)
        for off in range(attempts):
            cand = (index + off) % n
            if cand in self.invalid_indices:
                continue
            try:
                rec = self.hu_dataset[cand]
                torch.as_tensor(rec["audio"]["array"])
                if not isinstance(rec["text"], str):
                    raise TypeError(f"Text is not a string: {rec['text']}")
                return cand, rec
            except Exception as exc:
                self.invalid_indices.add(cand)
                print(f"Skipping invalid dataset record at index {cand}: {exc}")
        raise RuntimeError(f"Failed to load a valid record after {attempts} attempts starting from index {index}. "
                           f"Known invalid records so far: {len(self.invalid_indices)}")

    # ---- tokens
    def _encode(self, text: str, keep_timestamps: bool) -> List[int]:
        """`<|t.tt|>` -> timestamp_begin + round(t*100)//2 (t in [0,30], multiple of 0.02) or dropped."""
        out: List[int] = []
        for part in (x for x in _TS.split(text) if x != ""):
            if _TS.fullmatch(part):
                t = float(part[2:-2])
                if t < 0 or t > 30 or round(t * 100) % 2 != 0:
                    raise ValueError(f"Invalid timestamp: {t}")
                if keep_timestamps:
                    out.append(self.tokenizer.timestamp_begin + round(t * 100) // 2)
            else:
                kw = {"dropout_prob": self.bpe_dropout} if self.bpe_dropout else {}
                out.extend(self.tokenizer.encode(part, **kw))
        return out

    def _encode_text_with_timestamps(self, text: str) -> List[int]:
        return self._encode(text, True)

    def _encode_text_without_timestamps(self, text: str) -> List[int]:
        return self._encode(text, False)

    def _get_prompt_tokens(self, record, no_timestamps: bool) -> List[int]:
        prompt = record.get("prompt", "") if hasattr(record, "get") else record["prompt"]
        if torch.rand(1).item() < self.prompt_use_rate and len(prompt) > 0:
            toks = self._encode(prompt, not no_timestamps)[-self.max_prompt_length:]
            return [self.tokenizer.sot_prev] + toks
        return []

    def _get_special_tokens(self, is_text_empty: bool, language: str, no_timestamps: bool) -> List[int]:
        toks = [self.tokenizer.sot, self.tokenizer.special_tokens[f"<|{language}|>"], self.tokenizer.special_tokens["<|transcribe|>"]]
        if no_timestamps:
            toks.append(self.tokenizer.no_timestamps)
        if is_text_empty:
            toks.append(self.tokenizer.no_speech)
        return toks

    def _get_partial_segment_start(self, tokens: List[int]) -> Optional[float]:
        tb = self.tokenizer.timestamp_begin
        if len(tokens) >= 2 and tokens[-2] >= tb and tokens[-1] >= tb:
            return (tokens[-1] - tb) * 0.02
        return None

    def _get_text_tokens(self, text: str, no_timestamps: bool):
        toks = self._encode(text, True)
        start = self._get_partial_segment_start(toks)
        if no_timestamps:
            toks = [t for t in toks if t < self.tokenizer.timestamp_begin]
        return toks, start

    def _construct_decoder_output(self, prompt_tokens, special_tokens, text_tokens) -> List[int]:
        """Targets = inputs shifted by one + eot; the prompt (all but its hand-over to sot) is masked with -100."""
        if not prompt_tokens:
            return special_tokens[1:] + text_tokens + [self.tokenizer.eot]
        return [-100] * (len(prompt_tokens) - 1) + special_tokens + text_tokens + [self.tokenizer.eot]

    def __getitem__(self, index: int):
        index, rec = self._load_valid_record(index)
        no_ts = self.no_timestamp_training or torch.rand(1).item() < self.no_timestamps_rate
        prompt = self._get_prompt_tokens(rec, no_ts)
        text, seg_start = self._get_text_tokens(rec["text"], no_ts)
        special = self._get_special_tokens(len(text) == 0, rec["language"], no_ts)
        dec_in = prompt + special + text
        if len(dec_in) > self.model_n_text_ctx:
            print(f"Input is too long (length: {len(dec_in)}). Shortening... the prompt")
            prompt = prompt[: -(len(dec_in) - self.model_n_text_ctx)]
            dec_in = prompt + special + text
        dec_out = self._construct_decoder_output(prompt, special, text)
        rec_rate = rec["audio"].get("sampling_rate") if hasattr(rec["audio"], "get") else None
        if rec_rate is not None and int(rec_rate) != self.sample_rate:
            raise ValueError(f"record {index} has sampling_rate {rec_rate}, the loader was built for sample_rate {self.sample_rate}: "
                             "one rate per loader (get_dataloader(..., sample_rate=))")
        audio = np.asarray(rec["audio"]["array"], dtype=np.float32)
        audio = np.pad(audio, (0, self.n_samples - audio.shape[0]), "constant")  # pad in the audio domain (negative pad raises, as upstream)
        cut = int(seg_start * self.num_frames_per_second) if (no_ts and seg_start is not None) else N_FRAMES
        params, ext = self._draw_aug_params()
        item = (torch.from_numpy(audio), torch.tensor(dec_in, dtype=torch.int64), torch.tensor(dec_out, dtype=torch.int64),
                params, ext, cut)
        if self.apply_baseline_aug:
            item += (torch.tensor(self._draw_stretch_rate(), dtype=torch.float64),)
        if self.filter_aug is not None:
            item += (torch.from_numpy(self.filter_aug.draw()[2]),)
        if self.wave_aug is not None:
            item += (torch.from_numpy(self.wave_aug.draw(N_SAMPLES)[1]),)
        if self.rate_aug is not None:
            item += (torch.from_numpy(self.rate_aug.draw()[1]),)
        if self.office_aug is not None:
            item += (torch.from_numpy(self.office_aug.draw()[1]),)
        if self.mix_aug is not None:
            item += (torch.from_numpy(self.mix_aug.draw(N_SAMPLES)[1]),)
        return item


def collate_fn(data):
    """x stacked (the reference pads mels with 0), y_in padded with 0, y_out with -100."""
    cols = list(zip(*data))
    y_in = pad_sequence(cols[1], batch_first=True, padding_value=0)
    y_out = pad_sequence(cols[2], batch_first=True, padding_value=-100)
    if len(cols) == 3:
        return pad_sequence(cols[0], batch_first=True, padding_value=0), y_in, y_out
    out = (torch.stack(cols[0]), y_in, y_out, torch.stack(cols[3]), torch.stack(cols[4]), torch.tensor(cols[5], dtype=torch.int32))
    return out + tuple(torch.stack(c) for c in cols[6:])  # the time-stretch rates f64 [B], the filters f64 [B, 4, 6], the wave effects f64 [B, 14], the rate effects f64 [B, 4], the office effects f64 [B, 2 + cap], the mix effects f64 [B, 6]


class WarmupDatasetSampler(torch.utils.data.Sampler):
    """Draws only from `warmup_indices` for the first warmup_steps*batch_size samples, then from all indices;
    every pass over an index list is reshuffled with numpy's global RNG (data_loader.py:370-448)."""

    def __init__(self, warmup_indices: Sequence[int], all_indices: Sequence[int], warmup_steps: int, batch_size: int, shuffle: bool = True):
        self.warmup_indices, self.all_indices = list(warmup_indices), list(all_indices)
        if warmup_steps < 0:
            raise ValueError(f"warmup_steps must be >= 0, got {warmup_steps}")
        if batch_size <= 0:
            raise ValueError(f"batch_size must be > 0, got {batch_size}")
        if not self.all_indices:
            raise ValueError("all_indices must be non-empty")
        if not self.warmup_indices and warmup_steps > 0:
            raise ValueError("warmup_indices must be non-empty when warmup_steps > 0")
        self.warmup_steps, self.batch_size, self.shuffle = int(warmup_steps), int(batch_size), shuffle
        self.warmup_samples = self.warmup_steps * self.batch_size

    def __iter__(self) -> Iterator[int]:
        emitted = 0
        while True:
            pool = list(self.warmup_indices if emitted < self.warmup_samples else self.all_indices)
            if self.shuffle:
                np.random.shuffle(pool)
            for idx in pool:
                yield idx
                emitted += 1

    def __len__(self):
        return len(self.all_indices)


def get_dataset_boundary_indices(dataset_sizes: List[int]) -> List[Tuple[int, int]]:
    """[1000, 500, 2000] -> [(0, 1000), (1000, 1500), (1500, 3500)]"""
    out, start = [], 0
    for n in dataset_sizes:
        out.append((start, start + n))
        start += n
    return out


class GpuMelLoader:
    """Wraps the raw-audio DataLoader: pinned, double-buffered H2D of the raw clips (1.92 MB per clip instead of the
    1.54 MB mel plus its CPU cost), then log-mel + SpecAugment on the device.

    With DataLoader workers (num_workers > 0) batch i+1 is fetched and its host-to-device copies are issued on a side
    stream while batch i is being consumed; the compute stream waits on the copy's event only when it starts using the
    batch.  With num_workers == 0 the dataset's augmentation draws share the default generator with the model's own draws
    (stochastic depth, deep SpecAugment): fetching ahead would reorder them against the reference, so that case stays
    strictly sequential.  Yields (mel f32 [B, n_mels, 3000], y_in, y_out), all on the device.

    sample_rate != 16000: the staged batch is [B, 30 * sample_rate]; ONE K.resample launch turns it into [B, 480000] in front of the
    log-mel.  It is the resample of the zero-PADDED clip, so the filter's tail behind the clip's end is kept (it rings into the
    padding for `width` input samples), as it would be for a clip that was padded before an offline resampler.

    Batches of a dataset built with apply_baseline_aug carry a seventh field, the rates: resample (if any) -> K.time_stretch on the
    zero-padded [B, 480000] batch -> K.logmel_ragged with keep_frames = min(cut, 3000) -> K.specaug.  Loaders built without the flag
    (every dev loader) never stretch and run the path above unchanged.

    Batches of a dataset built with filter_aug carry the filters f64 [B, 4, 6] as their last field: K.sos_filter runs in place behind
    the resample and the stretch, over each row's full stretched length (n = n_out; 480000 without the stretch), so a filter's tail
    rings into the zero padding as it does in the reference, which filters the padded clip.  A batch whose filters are all identity
    launches nothing.  Which optional fields a batch carries is read from the dataset's flags (`stretch`, `filter_aug`: None = from
    `loader.dataset`; a loader without a dataset, e.g. a list of batches, takes a seventh field for the rates as before).

    Batches of a dataset built with wave_aug carry the wave effects f64 [B, 14] as their last field, behind the filters: the stages
    run in place in the order resample -> stretch -> NOISE -> filter -> CLIP -> LEVEL -> log-mel (apply_wave_stages), each over the
    row's full stretched length.  The table is turned into checked records on the host; a stage with no active row launches nothing,
    and a batch with no effect at all is the batch of a loader without the option, bit for bit.

    Batches of a dataset built with rate_aug carry the rate effects f64 [B, 4] as their last field, behind the wave effects: the
    order becomes resample -> stretch -> NOISE -> ALIAS -> filter -> CLIP -> LEVEL -> PITCH -> log-mel.  ALIAS is one out-of-place
    launch over the batch ("none" rows are copied) whose output takes the batch's place.  PITCH gathers the pitched rows only: one
    batched call without the baseline stretch (every row has 480000 samples), one call per distinct stretched length with it
    (the lengths are known on the host as round(480000 / rate): no synchronisation).

    Batches of a dataset built with office_aug carry the office effects f64 [B, 2 + cap] as their last field, behind the rate effects:
    CRUSH (in place) and ROOM (out of place; its output takes the batch's place) run right behind the stretch, in front of NOISE.

    Batches of a dataset built with mix_aug carry the mix effects f64 [B, 6] as their LAST field, behind the office effects: BACKGROUND
    runs behind ROOM and LOUDNESS behind NOISE, both in place.  The noise bank is loaded when the loader is built and stays on the
    device (entries back to back, f32 [total] with i64 offsets [K + 1]); a batch without an active row launches nothing."""

    def __init__(self, loader, frontend: GpuFrontend, training_aug: bool, sample_rate: int = SAMPLE_RATE, stretch: Optional[bool] = None,
                 filter_aug: Optional[bool] = None, wave_aug: Optional[bool] = None, rate_aug: Optional[bool] = None,
                 office_aug: Optional[bool] = None, mix_aug: Optional[bool] = None):
        self.loader, self.frontend, self.training_aug = loader, frontend, training_aug
        ds = getattr(loader, "dataset", None)
        if stretch is None and ds is not None:
            stretch = bool(getattr(ds, "apply_baseline_aug", False))
        if filter_aug is None:
            filter_aug = getattr(ds, "filter_aug", None) is not None
        if wave_aug is None:
            wave_aug = getattr(ds, "wave_aug", None) is not None
        if rate_aug is None:
            rate_aug = getattr(ds, "rate_aug", None) is not None
        if office_aug is None:
            office_aug = getattr(ds, "office_aug", None) is not None
        self.stretch, self.filter_aug, self.wave_aug, self.rate_aug = stretch, bool(filter_aug), bool(wave_aug), bool(rate_aug)
        self.office_aug = bool(office_aug)
        if mix_aug is None:
            mix_aug = getattr(ds, "mix_aug", None) is not None
        self.mix_aug = bool(mix_aug)
        self._mix = getattr(ds, "mix_aug", None) if self.mix_aug else None
        if self.mix_aug and self._mix is None:
            raise ValueError("mix_aug=True needs a loader whose dataset was built with mix_aug (it holds the noise bank's description)")
        self._bank = DeviceBank(self._mix, frontend.device) if self._mix is not None and self._mix.lengths is not None else None
        self._identity = torch.from_numpy(identity_sos())
        self.sample_rate = check_rate(sample_rate)
        self.sampler = getattr(loader, "sampler", None)  # infinite_iter() calls sampler.set_epoch(...)
        self.batch_size = getattr(loader, "batch_size", None)
        self.prefetch = getattr(loader, "num_workers", 0) > 0
        self._copy_stream = None

    def __len__(self):
        return len(self.loader)

    def _optional(self, batch):
        """(rates or None, sos or None) of a collated batch, by the flags.  An all-identity `sos` counts as None."""
        return self._fields(batch)[:2]

    def _fields(self, batch):
        """(rates or None, sos or None, wave-effect records or None) of a collated batch, by the flags.  An all-identity `sos` and a
        table without any effect count as None."""
        return self._all_fields(batch)[:3]

    def _all_fields(self, batch):
        """_fields and, as a fourth item, the checked rate-effect table f64 [B, 4] (numpy) or None (no option, or no row active)."""
        stretch = (len(batch) == 7 and not self.filter_aug and not self.wave_aug and not self.rate_aug and not self.office_aug and not self.mix_aug) \
            if self.stretch is None else self.stretch
        if len(batch) != 6 + int(stretch) + int(self.filter_aug) + int(self.wave_aug) + int(self.rate_aug) + int(self.office_aug) + int(self.mix_aug):
            raise ValueError(f"a batch of {len(batch)} fields from a loader with stretch={stretch}, filter_aug={self.filter_aug}"
                             + (f", wave_aug={self.wave_aug}" if self.wave_aug else "")
                             + (f", rate_aug={self.rate_aug}" if self.rate_aug else "")
                             + (f", office_aug={self.office_aug}" if self.office_aug else "")
                             + (f", mix_aug={self.mix_aug}" if self.mix_aug else ""))
        rates = batch[6] if stretch else None
        sos = batch[6 + int(stretch)] if self.filter_aug else None
        if sos is not None and bool((sos == self._identity).all()):
            sos = None
        fx = None
        if self.wave_aug:
            fx = check_records(records_from_table(batch[6 + int(stretch) + int(self.filter_aug)]))
            if not any(bool(active_rows(fx, stage).any()) for stage in WAVE_STAGES):
                fx = None
        rt = None
        if self.rate_aug:
            rt = check_rate_table(batch[6 + int(stretch) + int(self.filter_aug) + int(self.wave_aug)])
            if not bool(rt[:, 0].any() or rt[:, 2].any()):
                rt = None
        return rates, sos, fx, rt

    def _office_field(self, batch):
        """The checked office table f64 [B, 2 + cap] (numpy) of a collated batch, its last field in front of the mix effects, or None
        (no option, or no row active)."""
        if not self.office_aug:
            return None
        office = check_office_table(batch[-1 - int(self.mix_aug)])
        return office if bool(office[:, :2].any()) else None

    def _mix_field(self, batch):
        """(The checked mix table f64 [B, 6] (numpy) of a collated batch, its last field, the device bank), or None (no option, or no
        row active)."""
        if not self.mix_aug:
            return None
        table = check_mix_table(batch[-1], self._mix.lengths)
        return (table, self._bank) if bool(table[:, 0].any() or table[:, 4].any()) else None

    def _stage(self, batch):
        """Issue the batch's H2D copies on the side stream; returns the device tensors and the event that orders them."""
        dev = self.frontend.device
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=dev)
        audio, y_in, y_out, params, ext, cut = batch[:6]
        rates, sos, fx, rt = self._all_fields(batch)
        need_aug = bool(params[:, 0].any() or ext.any())  # decided on the host copies: no device sync
        with torch.cuda.stream(self._copy_stream):
            staged = [t.to(dev, non_blocking=True) for t in (audio, y_in, y_out, params, ext)]
            ev = torch.cuda.Event()
            ev.record(self._copy_stream)
        return staged, cut, ev, need_aug, rates, sos, fx, rt, self._office_field(batch), self._mix_field(batch)

    def _to_mel(self, staged, cut, ev, need_aug, rates=None, sos=None, fx=None, rt=None, office=None, mix=None):
        from whisper_finetune.engine import kernels as K

        cur = torch.cuda.current_stream(self.frontend.device)
        if ev is not None:
            cur.wait_event(ev)
            for t in staged:
                t.record_stream(cur)  # allocated on the copy stream, consumed on the compute stream
        audio, y_in, y_out, params, ext = staged
        if self.sample_rate != SAMPLE_RATE:
            audio = K.resample(audio, self.sample_rate, SAMPLE_RATE)  # [B, 30 * rate] -> [B, 480000]
        if rates is not None:
            # the stretch of the zero-PADDED clip, as the reference does it; the rates are host values (they size the launch), the
            # rows' lengths stay on the device; the cut and the minimum-value pad happen inside the ragged log-mel
            stretched, n_out = K.time_stretch(audio, rates)
            stretched = apply_wave_stages(stretched, n_out, sos, fx, rt,
                                          stretched_lengths(audio.shape[1], rates.tolist()) if rt is not None else None, office, mix)
            keep = cut.clamp(max=N_FRAMES).to(torch.int32).to(audio.device, non_blocking=True)
            mel = K.logmel_ragged(stretched, n_out, keep, self.frontend.filters, N_FRAMES)
        else:
            if sos is not None or fx is not None or rt is not None or office is not None or mix is not None:
                if audio.stride(1) != 1 or not audio.is_contiguous():
                    audio = audio.contiguous()
                audio = apply_wave_stages(audio, None, sos, fx, rt, None, office, mix)  # in place on the staged (or resampled) copy; alias gives a new one
            mel = self.frontend.log_mel(audio)
            for b in (cut < N_FRAMES).nonzero().flatten().tolist():  # rare: cut at a partial segment, pad with the min value
                c = int(cut[b])
                mel[b, :, c:] = mel[b, :, :c].min() if c > 0 else mel[b].min()
        if self.training_aug and need_aug:
            mel = K.specaug(mel, params, ext)
        return mel, y_in, y_out

    def __iter__(self):
        dev = self.frontend.device
        if not self.prefetch:
            for batch in self.loader:
                audio, y_in, y_out, params, ext, cut = batch[:6]
                need_aug = bool(params[:, 0].any() or ext.any())
                staged = [t.to(dev, non_blocking=True) for t in (audio, y_in, y_out, params, ext)]
                yield self._to_mel(staged, cut, None, need_aug, *self._all_fields(batch), self._office_field(batch), self._mix_field(batch))
            return
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur = nxt
            try:
                nxt = self._stage(next(it))  # copies of batch i+1 run beside the kernels of batch i
            except StopIteration:
                nxt = None
            yield self._to_mel(*cur)


def get_dataloader(hu_dataset, tokenizer, batch_size: int = 1, n_mels: int = 80, sampler=None, device=None,
                   no_timestamp_training: bool = False, max_prompt_length: int = 223, prompt_use_rate: float = 0.5,
                   no_timestamps_rate: float = 0.5, shuffle: bool = True, num_workers: int = 0, spec_augment: bool = False,
                   spec_augment_params: Optional[dict] = None, extremes_spec_augment: bool = False,
                   extremes_spec_augment_params: Optional[dict] = None, apply_baseline_aug: bool = False, apply_office_aug: bool = False,
                   apply_advanced_aug: bool = False, time_stretch_min_rate: float = 0.8, time_stretch_max_rate: float = 1.25,
                   bpe_dropout: float = 0.0, drop_last: bool = False, sample_rate: int = SAMPLE_RATE, filter_aug: Optional[dict] = None,
                   wave_aug: Optional[dict] = None, rate_aug: Optional[dict] = None, office_aug: Optional[dict] = None,
                   mix_aug: Optional[dict] = None):
    """`filter_aug`: None, or a mapping of FilterAug's keywords (AudioDataset's docstring): the filter augmentation of a TRAINING loader.
    `wave_aug`: None, or a mapping of WaveAug's groups (AudioDataset's docstring): noise, clipping and level changes of a TRAINING loader.
    `rate_aug`: None, or a mapping of RateAug's groups (AudioDataset's docstring): aliasing and pitch shift of a TRAINING loader.
    `office_aug`: None, or a mapping of OfficeAug's groups (AudioDataset's docstring): bit crush and room reverb of a TRAINING loader.
    `mix_aug`: None, or a mapping of MixAug's groups (AudioDataset's docstring): background noise and loudness normalisation of a TRAINING loader.
    `sample_rate`: the rate of every clip of `hu_dataset` (default 16000).  At another rate the clips are padded to
    30 * sample_rate samples and resampled to 16 kHz on the device (GpuMelLoader); without a device the loader yields the padded
    native-rate clips."""
    print(f"Found {len(hu_dataset)} records in the dataset.")
    ds = AudioDataset(hu_dataset, tokenizer, n_mels=n_mels, device=device, no_timestamp_training=no_timestamp_training,
                      max_prompt_length=max_prompt_length, prompt_use_rate=prompt_use_rate, no_timestamps_rate=no_timestamps_rate,
                      spec_augment=spec_augment, spec_augment_params=spec_augment_params, extremes_spec_augment=extremes_spec_augment,
                      extremes_spec_augment_params=extremes_spec_augment_params, bpe_dropout=bpe_dropout,
                      apply_baseline_aug=apply_baseline_aug, apply_office_aug=apply_office_aug, apply_advanced_aug=apply_advanced_aug,
                      time_stretch_min_rate=time_stretch_min_rate, time_stretch_max_rate=time_stretch_max_rate, sample_rate=sample_rate,
                      filter_aug=filter_aug, wave_aug=wave_aug, rate_aug=rate_aug, office_aug=office_aug, mix_aug=mix_aug)
    if sampler is not None:
        shuffle = False  # DataLoader does not allow both
    loader = DataLoader(ds, batch_size=batch_size, sampler=sampler, shuffle=shuffle, num_workers=num_workers,
                        pin_memory=torch.cuda.is_available(), drop_last=drop_last, collate_fn=collate_fn)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None or torch.device(device).type != "cuda":
        return loader  # raw-audio batches (CPU plumbing / tests); the GPU front end needs a device
    fe = GpuFrontend(n_mels, device, spec_augment, spec_augment_params, extremes_spec_augment, extremes_spec_augment_params)
    return GpuMelLoader(loader, fe, training_aug=spec_augment or extremes_spec_augment, sample_rate=sample_rate)


# ---------------------------------------------------------------------------------------------- synthetic provider
class SimpleTokenizer:
    """Whisper-shaped tokenizer for synthetic runs and tests (no tiktoken ranks here): bytes as text tokens and the
    multilingual special-token layout that `get_tokenizer(multilingual=True)` yields with its default 99 languages
    (SURVEY.md finding 6: sot 50258, <|de|> 50261, transcribe 50359, sot_prev 50361, nospeech 50362,
    notimestamps 50363, timestamp_begin 50364, eot 50257)."""

    eot, sot, sot_prev, no_speech, no_timestamps, timestamp_begin = 50257, 50258, 50361, 50362, 50363, 50364

    def __init__(self):
        self.special_tokens = {"<|endoftext|>": 50257, "<|startoftranscript|>": 50258, "<|en|>": 50259, "<|de|>": 50261,
                               "<|translate|>": 50358, "<|transcribe|>": 50359, "<|startofprev|>": 50361,
                               "<|nospeech|>": 50362, "<|notimestamps|>": 50363}

    def encode(self, text: str, **kwargs) -> List[int]:
        return list(text.encode("utf-8"))

    def decode(self, ids) -> str:
        return bytes(i for i in ids if 0 <= i < 256).decode("utf-8", errors="replace")


class SyntheticDataset:
    """HF-datasets-shaped records: N(0, 0.1^2) audio of random length <= 30 s, lower-case pseudo words."""

    column_names = ["audio", "text", "language", "prompt"]

    def __init__(self, n: int, seed: int = 1234, min_seconds: float = 5.0, language: str = "de", with_timestamps: bool = False):
        self.n, self.seed, self.min_seconds, self.language, self.with_timestamps = n, seed, min_seconds, language, with_timestamps

    def __len__(self):
        return self.n

    def __getitem__(self, i: int):
        g = torch.Generator().manual_seed(self.seed + i)
        secs = self.min_seconds + (30.0 - self.min_seconds) * torch.rand(1, generator=g).item()
        audio = torch.randn(int(secs * 16000), generator=g) * 0.1
        words = ["".join(chr(97 + int(c)) for c in torch.randint(0, 26, (int(torch.randint(2, 8, (1,), generator=g)),), generator=g))
                 for _ in range(int(torch.randint(3, 20, (1,), generator=g)))]
        text = " ".join(words)
        if self.with_timestamps:
            end = round(min(secs, 30.0) * 50) / 50
            text = f"<|0.00|>{text}<|{end:.2f}|>"
        return {"audio": {"array": audio.numpy(), "sampling_rate": 16000}, "text": text, "language": self.language, "prompt": ""}
