"""Audio files without a device: the numpy restatement of tests/_pcm_cases.py against scipy and audioop, data/audio_io.py parse_wav
against scipy, on hand-packed files, every refusal by its message and under truncation / corruption, the mutants the GPU
comparison must reject, and the host-side validation of K.pcm_decode and of the wav_dir noise bank."""
import os
import struct
import wave

import numpy as np
import pytest
import torch

from tests import _pcm_cases as P
from whisper_finetune.data import audio_io as AIO
from whisper_finetune.data import mix_fx as MF
from whisper_finetune.engine import kernels as K

scipy_wav = pytest.importorskip("scipy.io.wavfile")


def _ref_mono_rows(raw, fmt, C, frames):
    """Every channel of a payload through the restatement -> f32 [frames, C]."""
    buf = np.frombuffer(raw, dtype=np.uint8)
    return np.stack([P.decode_row(buf, (0, frames, C, fmt, c), frames) for c in range(C)], 1)


# ------------------------------------------------------------------------------------------------- restatement against scipy / audioop
@pytest.mark.parametrize("fmt, dtype", [("u8", np.uint8), ("s16le", np.int16), ("s32le", np.int32), ("f32le", np.float32), ("f64le", np.float64)])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_restatement_equals_scipy(tmp_path, fmt, dtype, C):
    rng = np.random.default_rng(FORMAT_SEED[fmt] + C)
    frames = 301
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        data = rng.integers(info.min, info.max, (frames, C), dtype=dtype, endpoint=True)
        data[0], data[1] = info.min, info.max
    else:
        data = (rng.standard_normal((frames, C)) * 0.5).astype(dtype)
    path = tmp_path / "a.wav"
    scipy_wav.write(path, 22050, data if C > 1 else data[:, 0])
    rate, back = scipy_wav.read(path)
    back = back.reshape(frames, C)
    info = AIO.parse_wav(path)
    assert (info.format, info.channels, info.sample_rate, info.frames) == (fmt, C, rate, frames)
    assert info == AIO.parse_wav(path.read_bytes())
    payload = path.read_bytes()[info.data_offset:info.data_offset + info.frames * info.block_align]
    got = _ref_mono_rows(payload, fmt, C, frames)
    if fmt == "u8":
        want = ((back.astype(np.float64) - 128.0) / 128.0).astype(np.float32)
    elif fmt in ("s16le", "s32le"):
        want = (back.astype(np.float64) / float(1 << (15 if fmt == "s16le" else 31))).astype(np.float32)
    else:
        want = back.astype(np.float32)
    assert P.same_bits(got, want), P.first_difference(got, want)


FORMAT_SEED = {f: 100 * i for i, f in enumerate(P.FORMATS)}


@pytest.mark.parametrize("C", [1, 2])
def test_restatement_equals_scipy_s24(tmp_path, C):
    rng = np.random.default_rng(24 + C)
    frames = 211
    vals = rng.integers(-(1 << 23), 1 << 23, (frames, C))
    vals[0], vals[1] = -(1 << 23), (1 << 23) - 1
    path = tmp_path / "s24.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(C)
        w.setsampwidth(3)
        w.setframerate(48000)
        w.writeframes(P.pack_ints(vals, "s24le"))
    rate, back = scipy_wav.read(path)  # int32, the 24 bits shifted left by 8: / 2^31 there is / 2^23 here
    info = AIO.parse_wav(path)
    assert (info.format, info.channels, info.sample_rate, info.frames, info.bits, info.block_align) == ("s24le", C, rate, frames, 24, 3 * C)
    payload = path.read_bytes()[info.data_offset:info.data_offset + frames * info.block_align]
    got = _ref_mono_rows(payload, "s24le", C, frames)
    want = (back.reshape(frames, C).astype(np.float64) / float(1 << 31)).astype(np.float32)
    assert P.same_bits(got, want), P.first_difference(got, want)
    assert np.array_equal(got, (vals / float(1 << 23)).astype(np.float32))


def test_g711_tables():
    u, a = P.ulaw_table(), P.alaw_table()
    assert (u[0x00], u[0x80], u[0x7F], u[0xFF]) == (-32124, 32124, 0, 0)
    assert (a[0x55], a[0xD5], a[0x2A], a[0xAA]) == (-8, 8, -32256, 32256)
    try:
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            import audioop
    except ImportError:
        return
    codes = bytes(range(256))
    assert np.array_equal(u, np.frombuffer(audioop.ulaw2lin(codes, 2), dtype="<i2").astype(np.int64))
    assert np.array_equal(a, np.frombuffer(audioop.alaw2lin(codes, 2), dtype="<i2").astype(np.int64))


def test_restatement_g711_values():
    raw = np.frombuffer(bytes(range(256)), dtype=np.uint8)
    assert np.array_equal(P.decode_row(raw, (0, 256, 1, "ulaw", -1), 256), (P.ulaw_table() / 32768.0).astype(np.float32))
    assert np.array_equal(P.decode_row(raw, (0, 256, 1, "alaw", 0), 256), (P.alaw_table() / 32768.0).astype(np.float32))


# ------------------------------------------------------------------------------------------------- parse_wav on hand-packed files
PAY = {f: P.random_payload(np.random.default_rng(7), f, 50, 2) for f in P.FORMATS}


@pytest.mark.parametrize("fmt", P.FORMATS)
def test_parse_plain_and_extensible(fmt):
    sb = P.SAMPLE_BYTES[fmt]
    for kw in (dict(), dict(extensible=True), dict(extensible=True, valid_bits=0), dict(fmt_size=18), dict(fmt_size=40)):
        f = P.wav_bytes(fmt, 2, 8000, PAY[fmt], **kw)
        info = AIO.parse_wav(f)
        assert info == AIO.WavInfo(fmt, 2, 8000, 8 * sb, 2 * sb, len(f) - len(PAY[fmt]), 50), kw
        assert f[info.data_offset:info.data_offset + info.frames * info.block_align] == PAY[fmt]
        assert AIO.parse_wav(memoryview(f)) == info


def test_parse_chunk_walk(tmp_path):
    pay = PAY["s16le"]
    listc = (b"LIST", b"INFOISFT\x05\x00\x00\x00abcd\x00\x00")
    odd = (b"junk", b"\x01\x02\x03")  # 3 bytes: a pad byte follows
    for kw in (dict(before_data=[listc]), dict(before_data=[odd]), dict(after_fmt=[odd], before_data=[listc, odd]), dict(data_first=True),
               dict(data_first=True, before_data=[odd])):
        f = P.wav_bytes("s16le", 2, 44100, pay, **kw)
        info = AIO.parse_wav(f)
        assert (info.format, info.channels, info.sample_rate, info.frames) == ("s16le", 2, 44100, 50), kw
        assert f[info.data_offset:info.data_offset + 200] == pay, kw
        path = tmp_path / "w.wav"
        path.write_bytes(f)
        assert AIO.parse_wav(path) == info and AIO.parse_wav(str(path)) == info
        assert AIO.read_payload(path, info).tobytes() == pay and AIO.read_payload(f, info).tobytes() == pay


def test_parse_truncated_and_streamed():
    pay = PAY["s24le"]  # 50 frames of 6 bytes
    whole = P.wav_bytes("s24le", 2, 16000, pay)
    off = len(whole) - len(pay)
    for cut, frames in ((1, 49), (6, 49), (7, 48), (len(pay) - 6, 1)):
        info = AIO.parse_wav(whole[:len(whole) - cut])
        assert (info.data_offset, info.frames) == (off, frames)
    for size in (0, 0xFFFFFFFF, len(pay) + 1000):
        info = AIO.parse_wav(P.wav_bytes("s24le", 2, 16000, pay, data_size=size, riff_size=size))
        assert (info.data_offset, info.frames) == (off, 50)
    info = AIO.parse_wav(P.wav_bytes("s24le", 2, 16000, pay + b"\x00\x01", data_size=0))  # streamed: to the end, floored to frames
    assert info.frames == 50
    info = AIO.parse_wav(P.wav_bytes("s24le", 2, 16000, pay, data_size=32))  # an honest smaller size: floored to whole frames
    assert info.frames == 5


@pytest.mark.parametrize("fmt", ["alaw", "ulaw"])
def test_parse_g711(fmt):
    f = P.wav_bytes(fmt, 1, 8000, bytes(range(256)), fmt_size=18, after_fmt=[(b"fact", struct.pack("<I", 256))])
    assert AIO.parse_wav(f) == AIO.WavInfo(fmt, 1, 8000, 8, 1, len(f) - 256, 256)


def test_parse_refusals():
    pay = PAY["s16le"]
    ok = P.wav_bytes("s16le", 2, 16000, pay)
    cases = [
        (P.wav_bytes("s16le", 2, 16000, pay, magic=b"RIFX"), "RIFX"),
        (P.wav_bytes("s16le", 2, 16000, pay, magic=b"RF64"), "RF64"),
        (P.wav_bytes("s16le", 2, 16000, pay, magic=b"BW64"), "BW64"),
        (b"FORM" + ok[4:], "not a RIFF/WAVE"),
        (ok[:8] + b"AVI " + ok[12:], "not a RIFF/WAVE"),
        (ok[:5], "too few"),
        (b"", "too few"),
        (P.wav_bytes("s16le", 2, 16000, pay, tag=0x0002, bits=4, block_align=1), "0x0002 (MS ADPCM)"),
        (P.wav_bytes("s16le", 2, 16000, pay, tag=0x0055), "0x0055 (MP3)"),
        (P.wav_bytes("s16le", 2, 16000, pay, tag=0x1234), "0x1234"),
        (P.wav_bytes("s16le", 2, 16000, pay, extensible=True, tag=0x0011), "0x0011 (IMA ADPCM)"),
        (P.wav_bytes("s24le", 2, 16000, PAY["s24le"], extensible=True, valid_bits=20), "20 valid bits in a 24-bit container"),
        (P.wav_bytes("s16le", 2, 16000, pay, bits=12, block_align=3), "format tag 1 with 12 bits"),
        (P.wav_bytes("f32le", 2, 16000, pay, bits=16, block_align=4), "format tag 3 with 16 bits"),
        (P.wav_bytes("ulaw", 2, 16000, pay, bits=16, block_align=4), "format tag 7 with 16 bits"),
        (P.wav_bytes("s16le", 2, 16000, pay, block_align=2), "block_align 2 is not channels * bits / 8 = 4"),
        (P.wav_bytes("s16le", 9, 16000, pay + pay[:16]), "channels must lie in [1, 8], got 9"),
        (P.wav_bytes("s16le", 0, 16000, pay, block_align=0), "channels must lie in [1, 8], got 0"),
        (P.wav_bytes("s16le", 2, 999, pay), "sample_rate must lie in [1000, 384000] Hz, got 999"),
        (P.wav_bytes("s16le", 2, 400000, pay), "sample_rate must lie in [1000, 384000] Hz, got 400000"),
        (ok[:12] + ok[36:], "no fmt chunk"),
        (ok[:36], "no data chunk"),
        (P.wav_bytes("s16le", 2, 16000, pay[:3]), "no whole frame"),
        (P.wav_bytes("s16le", 2, 16000, b""), "no whole frame"),
        (ok[:30], "fmt chunk is cut short"),
    ]
    bad_size = bytearray(ok)
    bad_size[16:20] = struct.pack("<I", 20)
    cases.append((bytes(bad_size), "fmt chunk of 20 bytes"))
    ext = bytearray(P.wav_bytes("s16le", 2, 16000, pay, extensible=True))
    ext[20 + 26:20 + 40] = bytes(14)
    cases.append((bytes(ext), "unknown extensible sub-format"))
    ext18 = bytearray(P.wav_bytes("s16le", 2, 16000, pay, fmt_size=18))
    ext18[20:22] = struct.pack("<H", 0xFFFE)
    cases.append((bytes(ext18), "extensible fmt chunk has 40 bytes"))
    for blob, msg in cases:
        with pytest.raises(ValueError) as e:
            AIO.parse_wav(blob)
        assert msg in str(e.value), (msg, str(e.value))
    with pytest.raises(ValueError, match="cannot open"):
        AIO.parse_wav("/nonexistent/dir/x.wav")
    with pytest.raises(ValueError, match="must be bytes"):
        AIO.parse_wav(12)


@pytest.mark.parametrize("fmt", P.FORMATS)
def test_parse_never_fails_otherwise(fmt):
    """Every truncation length and 500 seeded single-byte corruptions of the first 64 bytes: a WavInfo whose frames lie inside the
    input, or ValueError — nothing else."""
    whole = P.wav_bytes(fmt, 2, 16000, PAY[fmt][:40 * P.SAMPLE_BYTES[fmt]], extensible=fmt in ("s24le", "f64le"),
                        before_data=[(b"LIST", b"abc")] if fmt in ("u8", "ulaw") else ())
    rng = np.random.default_rng(P.FORMAT_ID[fmt])
    blobs = [whole[:n] for n in range(len(whole) + 1)]
    for _ in range(500):
        b = bytearray(whole)
        b[int(rng.integers(0, min(64, len(b))))] = int(rng.integers(0, 256))
        blobs.append(bytes(b))
    parsed = 0
    for blob in blobs:
        try:
            info = AIO.parse_wav(blob)
        except ValueError:
            continue
        parsed += 1
        assert info.frames >= 1 and info.block_align == info.channels * info.bits // 8 and info.format in AIO.FORMATS
        assert 0 <= info.data_offset and info.data_offset + info.frames * info.block_align <= len(blob)
    assert parsed > 50


# ------------------------------------------------------------------------------------------------- the comparison rejects the mutants
def test_case_table_holds_the_planted_values():
    T = {c["name"]: c for c in P.case_table()}
    raw, row, n_max = P.case_buffer(T["s32_one_rounding_pairs"])
    out = P.decode_row(raw, row, n_max)
    k = float(1 << 24)
    assert out[0] == np.float32((k + 2) * 64 / 2.0 ** 31) and out[3] == np.float32(1.0) and out[4] == np.float32(-1.0)
    assert P.decode_row(raw, row, n_max, "f32_channels")[0] == np.float32(k * 64 / 2.0 ** 31)
    raw, row, n_max = P.case_buffer(T["f64_edges_mono"])
    out = P.decode_row(raw, row, n_max)
    bits = out.view(np.uint32)
    assert bits[0] == 0 and bits[1] == 0x80000000 and bits[2] == 1 and bits[3] == 0x80000001 and bits[4] == 0 and bits[5] == 1 and bits[6] == 2
    assert np.isinf(out[11]) and np.isinf(out[12]) and out[13] == np.finfo(np.float32).max and np.isinf(out[14]) and out[15] == np.finfo(np.float32).max
    assert np.isnan(out[18]) and not out[row[1]:].any()
    raw, row, n_max = P.case_buffer(T["f32_specials_mono"])
    assert np.array_equal(P.decode_row(raw, row, n_max).view(np.uint32)[:11], np.frombuffer(T["f32_specials_mono"]["payload"], "<u4")[:11])


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_comparison_rejects_mutant(mutant):
    rejected = []
    for case in P.case_table():
        raw, row, n_max = P.case_buffer(case)
        want = P.expected(raw, [row], n_max, n_max + 5)
        assert P.same_bits(want, P.expected(raw, [row], n_max, n_max + 5))
        if not P.same_bits(P.expected(raw, [row], n_max, n_max + 5, mutant), want):
            rejected.append(case["name"])
    assert rejected, f"no case of the table tells {mutant} from the restatement"


# ------------------------------------------------------------------------------------------------- validation without a device
def test_pcm_decode_validates_rows_on_the_host():
    raw = torch.zeros(100, dtype=torch.uint8)  # a HOST tensor: a valid table reaches the device check, a bad one raises before it
    bad = [
        ([(0, 10, 1, "s16le", "mean")], dict(n_max=5), "frames 10 is outside 0..n_max = 5"),
        ([(0, -1, 1, "s16le", "mean")], {}, "frames -1 is outside"),
        ([(-1, 10, 1, "s16le", "mean")], {}, "byte_off -1 is negative"),
        ([(0, 10, 0, "s16le", "mean")], {}, "channels must lie in [1, 8], got 0"),
        ([(0, 1, 9, "u8", "mean")], {}, "channels must lie in [1, 8], got 9"),
        ([(0, 10, 2, "s16le", 2)], {}, "channel must be 'mean' or an integer inside [0, 1]"),
        ([(0, 10, 2, "s16le", -2)], {}, "channel must be"),
        ([(0, 10, 1, "s12", "mean")], {}, "PCM format must be one of"),
        ([(0, 10, 1, 8, "mean")], {}, "PCM format must be one of"),
        ([(81, 10, 1, "s16le", "mean")], {}, "frames end at byte 101, raw holds 100"),
        ([(0, 34, 1, "s24le", "mean")], {}, "frames end at byte 102"),
        ([(0, 7, 2, "f64le", "mean")], {}, "frames end at byte 112"),
        ([], {}, "1 to 65535 rows"),
        ([(0, 10, 1, "s16le", "mean")], dict(n_max=0), "n_max must be an integer inside"),
        ([(0, 10, 1, "s16le", "mean")], dict(n_max=(1 << 30) + 1), "n_max must be an integer inside"),
        ([(0, 10, 1, "s16le")], {}, "must be (byte_off, frames, channels, format, channel)"),
        ([(0.5, 10, 1, "s16le", "mean")], {}, "byte_off must be an integer"),
    ]
    for rows, kw, msg in bad:
        with pytest.raises(ValueError) as e:
            K.pcm_decode(raw, rows, **kw)
        assert msg in str(e.value), (msg, str(e.value))
    rec = np.zeros(1, dtype=AIO.ROW_DTYPE)
    rec[0] = (0, 10, 1, 9, -1, (0, 0))
    with pytest.raises(ValueError, match="format 9 is outside"):
        K.pcm_decode(raw, rec)
    rec[0] = (0, 10, 1, 1, -1, (0, 1))
    with pytest.raises(ValueError, match="reserved"):
        K.pcm_decode(raw, rec)
    with pytest.raises(ValueError, match="contiguous uint8"):
        K.pcm_decode(torch.zeros(100, dtype=torch.int8), [(0, 10, 1, "s16le", "mean")])
    with pytest.raises(ValueError, match="out must be f32 \\[1, 10\\]"):
        K.pcm_decode(raw, [(0, 10, 1, "s16le", "mean")], out=torch.zeros(1, 11))
    rec, n_max = AIO.pcm_rows([(3, 10, 3, "s24le", 2), (0, 0, 1, "ulaw", "mean")], 100)
    assert n_max == 10 and rec.dtype.itemsize == 32 and rec["format"].tolist() == [2, 7] and rec["channel"].tolist() == [2, -1]
    if not torch.cuda.is_available():  # a valid table on a host tensor: the only thing left to fail is the missing device
        with pytest.raises(Exception) as e:
            K.pcm_decode(raw, [(0, 10, 1, "s16le", "mean")])
        assert not isinstance(e.value, ValueError) and "no CPU path" in str(e.value)


def test_wav_dir_bank_lengths_come_from_headers(tmp_path):
    rng = np.random.default_rng(3)
    spec = [("b.wav", "s16le", 2, 44100, 4411), ("a.wav", "ulaw", 1, 8000, 801), ("c.WAV", "f32le", 1, 16000, 1234), ("d.wav", "s24le", 3, 48000, 999)]
    for name, fmt, C, rate, frames in spec:
        (tmp_path / name).write_bytes(P.wav_bytes(fmt, C, rate, P.random_payload(rng, fmt, frames, C)))
    (tmp_path / "notes.txt").write_text("not audio")
    np.save(tmp_path / "x.npy", np.zeros(5, dtype=np.float32))
    lengths = MF.bank_lengths({"wav_dir": tmp_path}, 16000)
    assert lengths == [-(-801 * 16000 // 8000), -(-4411 * 16000 // 44100), 1234, -(-999 * 16000 // 48000)]  # a, b, c, d: name order
    assert MF.bank_lengths({"wav_dir": str(tmp_path), "channel": 0}, 8000) == [801, -(-4411 * 8000 // 44100), 617, -(-999 * 8000 // 48000)]
    aug = MF.MixAug(16000, background={"bank": {"wav_dir": tmp_path}})
    assert aug.lengths == lengths
    # headers only: a payload cut away behind the header of a streamed file changes nothing the walk reads
    files, channel = AIO.wav_dir_files({"wav_dir": tmp_path})
    assert [os.path.basename(f) for f in files] == ["a.wav", "b.wav", "c.WAV", "d.wav"] and channel == "mean"
    with pytest.raises(ValueError, match="bank_sample_rate"):
        MF.bank_lengths({"wav_dir": tmp_path}, 16000, 8000)
    with pytest.raises(ValueError, match="decoded on the device"):
        MF.load_bank({"wav_dir": tmp_path})
    with pytest.raises(ValueError, match="is not a directory"):
        MF.bank_lengths({"wav_dir": tmp_path / "nope"})
    with pytest.raises(ValueError, match="a mapping must be"):
        MF.bank_lengths({"wav_dir": tmp_path, "seed": 1})
    with pytest.raises(ValueError, match="channel must be"):
        MF.bank_lengths({"wav_dir": tmp_path, "channel": "left"})
    with pytest.raises(ValueError, match="channel 1 does not exist"):
        MF.bank_lengths({"wav_dir": tmp_path, "channel": 1})  # a.wav is mono
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="holds no .wav file"):
        MF.bank_lengths({"wav_dir": empty})
    (empty / "bad.wav").write_bytes(b"RIFX" + bytes(40))
    with pytest.raises(ValueError, match="bad.wav.*RIFX"):
        MF.bank_lengths({"wav_dir": empty})
    assert MF.bank_lengths({"synthetic": 2}, 16000) == [48000, 120000]  # the other forms are untouched
