"""The resampler inside the two public paths: Whisper.transcribe(..., sample_rate=) and get_dataloader(..., sample_rate=)
(GpuMelLoader).  whisper-tiny with the weights of tests/test_model_gpu.py, as tests/test_transcribe_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests.test_model_gpu import _engine, _tiny_case  # noqa: E402
from whisper_finetune.data import gpu_frontend as G  # noqa: E402
from whisper_finetune.data.data_loader import GpuMelLoader, SimpleTokenizer, get_dataloader  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import transcribe as T  # noqa: E402

DEV = torch.device("cuda:0")
EOT, SOT, LANG_EN, TRANSCRIBE, SOT_PREV, NO_SPEECH, TSB = 50257, 50258, 50259, 50359, 50361, 50362, 50364
SUPPRESS = list(range(EOT + 1, TSB))


def test_transcribe_at_other_rates_equals_transcribe_of_the_resampled_recordings(monkeypatch):
    dims, params, _, _, _ = _tiny_case()
    m = _engine(dims, params).eval()
    g = torch.Generator().manual_seed(91)
    audios = [torch.randn(9 * 48000, generator=g) * 0.1, torch.randn(31 * 44100, generator=g) * 0.1]
    rates = [48000, 44100]
    filters = O.mel_filters(dims.n_mels).to(DEV)
    kw = dict(sot_sequence=(SOT, LANG_EN, TRANSCRIBE), eot=EOT, filters=filters, max_windows=1, sample_len=12, temperatures=(0.0,),
              logprob_threshold=None, no_speech_threshold=None, no_speech=NO_SPEECH, sot_prev=SOT_PREV, suppress=SUPPRESS, seed=3)
    frames = []
    pack = T.pack_logmels

    def spy(recordings, f):
        packed = pack(recordings, f)
        frames.append((list(packed.host[2]), [int(a.numel()) for a in recordings]))
        return packed

    monkeypatch.setattr(T, "pack_logmels", spy)
    got = m.transcribe(audios, sample_rate=rates, **kw)
    resampled = [G.resample(a, r) for a, r in zip(audios, rates)]
    want = m.transcribe(resampled, **kw)
    # by hand: 9 s and 31 s are 144 000 and 496 000 samples at 16 kHz — 900 and 3 100 frames
    assert [int(a.numel()) for a in resampled] == [144000, 496000]
    assert frames == [([900, 3100], [144000, 496000])] * 2
    assert [r["windows"] for r in got] == [1, 1] and [r["truncated"] for r in got] == [False, True]
    assert len(got) == len(want) == 2
    for a in range(2):
        assert set(got[a]) == set(want[a])
        for key in got[a]:
            assert got[a][key] == want[a][key], (a, key)
        assert len(got[a]["segments"]) == 1 and len(got[a]["tokens"]) > 0
        assert got[a]["segments"][0]["end"] == (900 * 0.01, 3000 * 0.01)[a]    # the whole window: 900 content frames, and the first 3000 of 3100
    # one rate for all recordings, and the default: 16 kHz recordings are not resampled
    calls = []
    resample = K.resample
    monkeypatch.setattr(K, "resample", lambda *a, **k: calls.append(a[1:]) or resample(*a, **k))
    again = m.transcribe(resampled, sample_rate=16000, **kw)
    assert calls == [] and [r["tokens"] for r in again] == [r["tokens"] for r in want]
    one = m.transcribe(audios[0], sample_rate=48000, **kw)
    assert calls == [(48000, 16000)] and one[0]["tokens"] == want[0]["tokens"]


class _DS(list):
    column_names = ["audio", "text", "language", "prompt"]


def _records(rate_field):
    g = torch.Generator().manual_seed(17)
    out = []
    for seconds in (7, 10):
        audio = {"array": (torch.randn(seconds * 48000, generator=g) * 0.1).numpy()}
        if rate_field is not None:
            audio["sampling_rate"] = rate_field
        out.append({"audio": audio, "text": "abc def", "language": "de", "prompt": ""})
    return _DS(out)


def _padded(records, n):
    return torch.from_numpy(np.stack([np.pad(r["audio"]["array"], (0, n - r["audio"]["array"].shape[0])) for r in records])).to(DEV)


def test_the_mel_loader_resamples_the_staged_batch_with_one_launch(monkeypatch):
    recs = _records(48000)
    loader = get_dataloader(recs, SimpleTokenizer(), batch_size=2, n_mels=80, shuffle=False, device=DEV, no_timestamp_training=True,
                            sample_rate=48000)
    assert isinstance(loader, GpuMelLoader) and loader.sample_rate == 48000
    calls = []
    resample = K.resample
    monkeypatch.setattr(K, "resample", lambda *a, **k: calls.append((tuple(a[0].shape),) + a[1:]) or resample(*a, **k))
    batches = list(loader)
    assert len(batches) == 1 and calls == [((2, 1440000), 48000, 16000)]
    mel = batches[0][0]
    want = loader.frontend.log_mel(resample(_padded(recs, 1440000), 3, 1))
    assert tuple(mel.shape) == (2, 80, 3000) and torch.equal(mel, want)
    # the clip ends at 7 s: the frames well behind it are the log-mel of (almost) silence, those before it are not
    assert mel[0, :, :690].std() > 10 * mel[0, :, 720:].std()


def test_the_mel_loader_at_16_khz_does_not_call_the_resampler(monkeypatch):
    recs = _records(None)                        # the same samples, declared (by default) as 16 kHz clips of 21 s and 30 s
    calls = []
    monkeypatch.setattr(K, "resample", lambda *a, **k: calls.append(a))
    for kw in ({}, {"sample_rate": 16000}):
        loader = get_dataloader(recs, SimpleTokenizer(), batch_size=2, n_mels=80, shuffle=False, device=DEV, no_timestamp_training=True, **kw)
        mel = next(iter(loader))[0]
        assert torch.equal(mel, loader.frontend.log_mel(_padded(recs, 480000)))
    assert calls == []
