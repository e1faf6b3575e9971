"""WAV files through the public paths: gpu_frontend.load_audio against decode_pcm + resample of every file alone, Whisper.transcribe
with file entries against the same call on the decoded arrays, and the {"wav_dir": ...} noise bank against load_audio and the list
form.  whisper-tiny with the weights of tests/test_model_gpu.py, as tests/test_transcribe_gpu.py."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests import _pcm_cases as P  # noqa: E402
from tests.test_model_gpu import _engine, _tiny_case  # noqa: E402
from whisper_finetune.data import audio_io as AIO  # noqa: E402
from whisper_finetune.data import data_loader as DL  # noqa: E402
from whisper_finetune.data import gpu_frontend as GF  # noqa: E402
from whisper_finetune.data import mix_fx as MF  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402

DEV = torch.device("cuda:0")
EOT, SOT, LANG_EN, TRANSCRIBE, SOT_PREV, NO_SPEECH, TSB = 50257, 50258, 50259, 50359, 50361, 50362, 50364
SUPPRESS = list(range(EOT + 1, TSB))
# (name, format, channels, rate, frames): about 0.3 s each
FILES = [("a_s16_stereo_44k.wav", "s16le", 2, 44100, 13231), ("b_ulaw_8k.wav", "ulaw", 1, 8000, 2401), ("c_f32_16k.wav", "f32le", 1, 16000, 4803),
         ("d_s24_3ch_48k.wav", "s24le", 3, 48000, 14401)]


def _smooth_payload(rng, fmt, frames, channels):
    """A band-limited signal per channel (a few sines plus a little noise) in the format's bytes."""
    t = np.arange(frames)[:, None] / 8000.0
    x = sum(0.2 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6, channels)) for f in (110.0, 523.0, 1210.0)) + 0.01 * rng.standard_normal((frames, channels))
    if fmt == "f32le":
        return P.pack_floats(x, fmt)
    if fmt == "ulaw":
        return rng.integers(0, 256, frames * channels, dtype=np.uint8).tobytes()
    bits = 8 * P.SAMPLE_BYTES[fmt]
    return P.pack_ints(np.round(x * (1 << (bits - 1)) * 0.9).astype(np.int64), fmt)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("wavs")
    rng = np.random.default_rng(31)
    out = []
    for name, fmt, ch, rate, frames in FILES:
        pay = _smooth_payload(rng, fmt, frames, ch)
        blob = P.wav_bytes(fmt, ch, rate, pay, before_data=[(b"LIST", b"abc")] if fmt == "s16le" else (), extensible=fmt == "s24le")
        (d / name).write_bytes(blob)
        out.append(dict(path=d / name, blob=blob, payload=pay, fmt=fmt, channels=ch, rate=rate, frames=frames))
    return d, out


def _alone(f, channel="mean"):
    return GF.resample(GF.decode_pcm(f["payload"], f["fmt"], channels=f["channels"], channel=channel, device=DEV), f["rate"])


def test_load_audio_equals_every_file_alone(files, monkeypatch):
    d, fs = files
    launches = []
    decode = K.pcm_decode
    monkeypatch.setattr(K, "pcm_decode", lambda raw, rows, *a, **k: launches.append((int(raw.numel()), len(rows))) or decode(raw, rows, *a, **k))
    sources = [str(fs[0]["path"]), fs[1]["blob"], fs[2]["path"], fs[3]["blob"], fs[0]["blob"], fs[1]["path"], fs[2]["blob"], str(fs[3]["path"])]
    got, infos = GF.load_audio(sources, device=DEV, return_info=True)
    assert len(launches) == 1 and launches[0][1] == 8  # ONE decode launch for the whole list
    monkeypatch.undo()
    want = [_alone(f) for f in fs]
    for k, (g, info) in enumerate(zip(got, infos)):
        f = fs[k % 4]
        assert g.device == DEV and g.dtype == torch.float32 and g.dim() == 1
        assert int(g.numel()) == -(-f["frames"] * 16000 // f["rate"])
        assert torch.equal(g.view(torch.int32), want[k % 4].view(torch.int32)), (k, f["path"].name)
        assert info == AIO.parse_wav(f["blob"]) and (info.format, info.channels, info.sample_rate, info.frames) == (f["fmt"], f["channels"], f["rate"], f["frames"])
    # the 16 kHz file needs no resampler: the restatement, bit for bit
    ref = P.decode_row(np.frombuffer(fs[2]["payload"], dtype=np.uint8), (0, fs[2]["frames"], 1, "f32le", -1), fs[2]["frames"])
    assert P.same_bits(got[2].cpu().numpy(), ref)
    # and the integer files before the resampler, at their own rate
    for k in (0, 3):
        f = fs[k]
        native = GF.load_audio(f["path"], sample_rate=f["rate"], device=DEV)
        ref = P.decode_row(np.frombuffer(f["payload"], dtype=np.uint8), (0, f["frames"], f["channels"], f["fmt"], -1), f["frames"])
        assert P.same_bits(native.cpu().numpy(), ref)
    # one source in, one tensor out; a picked channel; another target rate
    one, info = GF.load_audio(fs[3]["blob"], channel=2, device=DEV, return_info=True)
    assert torch.equal(one, _alone(fs[3], channel=2)) and not torch.equal(one, want[3]) and info.channels == 3
    at8k = GF.load_audio([fs[0]["path"], fs[1]["path"]], sample_rate=8000, device=DEV)
    assert int(at8k[0].numel()) == -(-13231 * 8000 // 44100) and int(at8k[1].numel()) == 2401
    with pytest.raises(ValueError, match="channel must be"):
        GF.load_audio([fs[0]["path"], fs[1]["path"]], channel=1, device=DEV)  # the second file is mono


def test_load_audio_refuses_a_file_with_a_nan(files, tmp_path):
    d, fs = files
    x = np.linspace(-0.5, 0.5, 300).astype(np.float32)
    x[123] = np.nan
    bad = tmp_path / "holds_a_nan.wav"
    bad.write_bytes(P.wav_bytes("f32le", 1, 16000, x.tobytes()))
    with pytest.raises(ValueError, match="holds_a_nan.wav.*not finite"):
        GF.load_audio([fs[2]["path"], bad], device=DEV)
    x[123] = np.inf
    with pytest.raises(ValueError, match="source 0 .*not finite"):
        GF.load_audio(P.wav_bytes("f32le", 1, 16000, x.tobytes()), device=DEV)


def test_transcribe_files_equals_transcribe_of_the_decoded_arrays(tmp_path):
    dims, params, _, _, _ = _tiny_case()
    m = _engine(dims, params).eval()
    rng = np.random.default_rng(41)
    g = torch.Generator().manual_seed(5)
    pay_a = _smooth_payload(rng, "s16le", 4 * 44100 + 17, 2)
    pay_b = rng.integers(0, 256, 3 * 8000 + 5, dtype=np.uint8).tobytes()
    wav_a = tmp_path / "a.wav"
    wav_a.write_bytes(P.wav_bytes("s16le", 2, 44100, pay_a))
    wav_b = P.wav_bytes("ulaw", 1, 8000, pay_b, fmt_size=18)
    array_c = torch.randn(2 * 16000 + 3, generator=g) * 0.1
    filters = O.mel_filters(dims.n_mels).to(DEV)
    kw = dict(sot_sequence=(SOT, LANG_EN, TRANSCRIBE), eot=EOT, filters=filters, max_windows=1, sample_len=12, temperatures=(0.0,),
              logprob_threshold=None, no_speech_threshold=None, no_speech=NO_SPEECH, sot_prev=SOT_PREV, suppress=SUPPRESS, seed=3,
              language_tokens=list(range(50259, 50358)))
    got = m.transcribe([wav_a, wav_b, array_c], **kw)
    dec_a = GF.decode_pcm(pay_a, "s16le", channels=2, device=DEV)
    dec_b = GF.decode_pcm(pay_b, "ulaw", device=DEV)
    want = m.transcribe([dec_a, dec_b, array_c], sample_rate=[44100, 8000, 16000], **kw)
    assert len(got) == len(want) == 3
    for a in range(3):
        assert set(got[a]) == set(want[a])
        for key in got[a]:
            if key == "language_probs":
                assert torch.equal(torch.as_tensor(got[a][key]), torch.as_tensor(want[a][key])), a
            else:
                assert got[a][key] == want[a][key], (a, key)
        assert len(got[a]["segments"]) == 1 and len(got[a]["tokens"]) > 0
    one = m.transcribe(str(wav_a), **kw)  # one path is one recording
    assert len(one) == 1 and one[0]["tokens"] == want[0]["tokens"]
    left = m.transcribe([wav_a], audio_channel=0, **kw)
    dec_left = GF.decode_pcm(pay_a, "s16le", channels=2, channel=0, device=DEV)
    assert left[0]["tokens"] == m.transcribe([dec_left], sample_rate=44100, **kw)[0]["tokens"]
    for rate in (44100, [44100, 8000, 16000], 16000.0):
        with pytest.raises(ValueError, match="sample_rate must be left at its default"):
            m.transcribe([wav_a, wav_b, array_c], sample_rate=rate, **kw)
    with pytest.raises(ValueError, match="RIFX"):
        m.transcribe([b"RIFX" + bytes(60)], **kw)


def test_wav_dir_bank_on_the_device_and_in_a_loader(files):
    d, fs = files
    aug = MF.MixAug(16000, background={"p": 1.0, "bank": {"wav_dir": d}})
    lengths = MF.bank_lengths({"wav_dir": d}, 16000)
    assert aug.lengths == lengths == [-(-f["frames"] * 16000 // f["rate"]) for f in fs]
    bank = DL.DeviceBank(aug, DEV)
    parts = GF.load_audio([f["path"] for f in fs], device=DEV)
    assert bank.lengths == lengths and bank.off.cpu().tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    assert torch.equal(bank.bank, torch.cat(parts)) and bank.bank.device == DEV
    left = DL.DeviceBank(MF.MixAug(16000, background={"bank": {"wav_dir": str(d), "channel": 0}}), DEV)
    assert left.lengths == lengths and not torch.equal(left.bank, bank.bank)
    with pytest.raises(ValueError, match="bank_sample_rate"):
        MF.MixAug(16000, background={"bank": {"wav_dir": d}, "bank_sample_rate": 8000})

    def loader(bank_spec):
        return DL.get_dataloader(DL.SyntheticDataset(3, with_timestamps=True), DL.SimpleTokenizer(), batch_size=3, n_mels=80, shuffle=False, device=DEV,
                                 no_timestamp_training=True, mix_aug={"background": {"p": 1.0, "bank": bank_spec}})

    batches = []
    for spec in ({"wav_dir": d}, [p.cpu().numpy() for p in parts]):
        torch.manual_seed(11)
        random.seed(11)
        batches.append(next(iter(loader(spec))))
    for a, b in zip(*batches):
        assert torch.equal(a, b)
    torch.manual_seed(11)
    random.seed(11)
    plain = next(iter(DL.get_dataloader(DL.SyntheticDataset(3, with_timestamps=True), DL.SimpleTokenizer(), batch_size=3, n_mels=80, shuffle=False,
                                        device=DEV, no_timestamp_training=True)))
    assert not torch.equal(plain[0], batches[0][0])  # the bank was mixed in
