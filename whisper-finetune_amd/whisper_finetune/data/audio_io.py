"""Audio files on the host side: the WAV header parser and the row table of the device decoder (pure Python / numpy, no device).

The sample data of a file is decoded on the device (csrc/pcm.hip `wft_pcm_decode_f32`, include/wft.h "PCM decode" states the
arithmetic): the bytes travel as they are in the file, 1 to 8 bytes per sample instead of 4 per converted sample.  What stays on the
host is the header: `parse_wav` walks the RIFF chunks and says where the frames lie, `pcm_rows` checks a decode table with the
conditions the kernel clamps with.  `data/gpu_frontend.py` `decode_pcm` / `load_audio` are the public forms.

Read: little-endian RIFF/WAVE with integer PCM (8, 16, 24, 32 bits), IEEE float (32, 64 bits), A-law and u-law, plain or
WAVE_FORMAT_EXTENSIBLE, 1 to 8 channels.  Out of scope: FLAC, MP3, Ogg, AIFF, big-endian data (RIFX), RF64 / BW64, more than 8
channels, containers with fewer valid bits than container bits (20-in-24), writing files.
"""
from __future__ import annotations

import os
import struct
from typing import NamedTuple

import numpy as np

FORMATS = ("u8", "s16le", "s24le", "s32le", "f32le", "f64le", "alaw", "ulaw")  # WFT_PCM_* in enum order
FORMAT_ID = {k: i for i, k in enumerate(FORMATS)}
SAMPLE_BYTES = (1, 2, 3, 4, 4, 8, 1, 1)
MAX_CHANNELS = 8
MAX_FRAMES = 1 << 30
MIN_RATE, MAX_RATE = 1000, 384000  # data/gpu_frontend.py check_rate
ROW_DTYPE = np.dtype([("byte_off", "<i8"), ("frames", "<i4"), ("channels", "<i4"), ("format", "<i4"), ("channel", "<i4"),
                      ("reserved", "<i4", (2,))])  # wft_pcm_row, 32 bytes

_TAG_PCM, _TAG_FLOAT, _TAG_ALAW, _TAG_ULAW, _TAG_EXTENSIBLE = 1, 3, 6, 7, 0xFFFE
_TAG_NAMES = {0x0002: "MS ADPCM", 0x0011: "IMA ADPCM", 0x0031: "GSM 6.10", 0x0050: "MPEG", 0x0055: "MP3", 0x00FF: "AAC"}
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")  # KSDATAFORMAT_SUBTYPE_*: the tag, then these 14 bytes


class WavInfo(NamedTuple):
    format: str        # one of FORMATS
    channels: int
    sample_rate: int
    bits: int          # container bits per sample
    block_align: int   # bytes per frame
    data_offset: int   # first byte of the first frame inside the file
    frames: int        # whole frames present


def format_id(fmt) -> int:
    """A format name of FORMATS or its WFT_PCM_* number -> the number; ValueError otherwise."""
    if isinstance(fmt, str) and fmt in FORMAT_ID:
        return FORMAT_ID[fmt]
    if not isinstance(fmt, bool) and isinstance(fmt, (int, np.integer)) and 0 <= int(fmt) < len(FORMATS):
        return int(fmt)
    raise ValueError(f"PCM format must be one of {FORMATS} or its number 0..{len(FORMATS) - 1}, got {fmt!r}")


def channel_id(channel, channels: int) -> int:
    """"mean" -> -1, an integer 0..channels-1 -> itself; ValueError otherwise."""
    if isinstance(channel, str) and channel == "mean":
        return -1
    if not isinstance(channel, bool) and isinstance(channel, (int, np.integer)) and -1 <= int(channel) < channels:
        return int(channel)
    raise ValueError(f"channel must be 'mean' or an integer inside [0, {channels - 1}], got {channel!r}")


class _Bytes:
    def __init__(self, buf):
        self.buf = memoryview(buf).cast("B")
        self.size = len(self.buf)

    def read(self, off: int, n: int) -> bytes:
        return bytes(self.buf[off:off + n])

    def close(self):
        pass


class _File:
    def __init__(self, path):
        self.f = open(path, "rb")
        self.size = os.fstat(self.f.fileno()).st_size

    def read(self, off: int, n: int) -> bytes:
        self.f.seek(off)
        return self.f.read(n)

    def close(self):
        self.f.close()


def _is_path(src) -> bool:
    return isinstance(src, (str, os.PathLike))


def _parse_fmt(b: bytes):
    tag, channels, rate, _, block_align, bits = struct.unpack("<HHIIHH", b[:16])
    if tag == _TAG_EXTENSIBLE:
        if len(b) != 40:
            raise ValueError(f"wav: an extensible fmt chunk has 40 bytes, got {len(b)}")
        _, valid, _, guid = struct.unpack("<HHI16s", b[16:40])
        if guid[2:] != _GUID_TAIL:
            raise ValueError(f"wav: unknown extensible sub-format {guid.hex()}")
        if valid not in (0, bits):
            raise ValueError(f"wav: {valid} valid bits in a {bits}-bit container are not supported")
        tag = struct.unpack("<H", guid[:2])[0]
    if tag == _TAG_PCM and bits in (8, 16, 24, 32):
        fmt = {8: "u8", 16: "s16le", 24: "s24le", 32: "s32le"}[bits]
    elif tag == _TAG_FLOAT and bits in (32, 64):
        fmt = "f32le" if bits == 32 else "f64le"
    elif tag in (_TAG_ALAW, _TAG_ULAW) and bits == 8:
        fmt = "alaw" if tag == _TAG_ALAW else "ulaw"
    elif tag in (_TAG_PCM, _TAG_FLOAT, _TAG_ALAW, _TAG_ULAW):
        raise ValueError(f"wav: format tag {tag} with {bits} bits per sample is not supported")
    else:
        name = _TAG_NAMES.get(tag)
        raise ValueError(f"wav: format tag 0x{tag:04X}{' (' + name + ')' if name else ''} is not supported (PCM, IEEE float, A-law and u-law are)")
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"wav: channels must lie in [1, {MAX_CHANNELS}], got {channels}")
    if block_align != channels * bits // 8:
        raise ValueError(f"wav: block_align {block_align} is not channels * bits / 8 = {channels * bits // 8}")
    if not MIN_RATE <= rate <= MAX_RATE:
        raise ValueError(f"wav: sample_rate must lie in [{MIN_RATE}, {MAX_RATE}] Hz, got {rate}")
    return fmt, channels, rate, bits, block_align


def parse_wav(src) -> WavInfo:
    """The header of a WAV file -> WavInfo(format, channels, sample_rate, bits, block_align, data_offset, frames).

    src: `bytes` / a `memoryview` (the whole file), or a path: from a path only the chunk headers and the fmt chunk are read, chunk
    payloads are skipped with seeks (the loader workers take the noise bank's lengths from here).  Little-endian RIFF/WAVE only.  The
    chunk walk takes chunks in any order, skips the pad byte of an odd-sized chunk and any chunk it does not know; the first `fmt `
    and the first `data` chunk count.  fmt chunks of 16, 18 or 40 bytes; tags 1 (PCM, 8 / 16 / 24 / 32 bits), 3 (IEEE float, 32 / 64
    bits), 6 and 7 (A-law, u-law, 8 bits) and 0xFFFE (extensible: the tag is the head of the sub-format GUID; wValidBitsPerSample must
    be 0 or the container bits).  A `data` size of 0, or larger than what is left of the file, means "to the end of the file", floored
    to whole frames (a truncated file, a streamed one marked 0 or 0xFFFFFFFF).
    ValueError, and nothing else, on any other input: RIFX / RF64 / BW64 by name, no RIFF/WAVE magic, any other tag (named), a
    block_align that is not channels * bits / 8, channels outside 1..8, a rate outside [1000, 384000], no fmt chunk, no data chunk,
    zero whole frames, more than 2^30 frames."""
    if _is_path(src):
        try:
            rd = _File(src)
        except OSError as e:
            raise ValueError(f"wav: cannot open {os.fspath(src)!r}: {e}") from None
    else:
        try:
            rd = _Bytes(src)
        except TypeError:
            raise ValueError(f"wav: the source must be bytes, a memoryview or a path, got {type(src).__name__}") from None
    try:
        head = rd.read(0, 12)
        if len(head) < 12:
            raise ValueError(f"wav: {rd.size} bytes are too few for a RIFF header")
        magic = head[:4]
        if magic in (b"RIFX", b"RF64", b"BW64"):
            raise ValueError(f"wav: {magic.decode()} files are not supported (little-endian RIFF only)")
        if magic != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError("wav: not a RIFF/WAVE file")
        fmt = data = None
        pos = 12
        while pos + 8 <= rd.size and (fmt is None or data is None):
            ch = rd.read(pos, 8)
            if len(ch) < 8:
                break
            cid, csz = struct.unpack("<4sI", ch)
            body = pos + 8
            left = rd.size - body
            if cid == b"fmt " and fmt is None:
                if csz not in (16, 18, 40):
                    raise ValueError(f"wav: a fmt chunk of {csz} bytes is not supported (16, 18 or 40)")
                b = rd.read(body, csz)
                if len(b) < csz:
                    raise ValueError("wav: the fmt chunk is cut short")
                fmt = _parse_fmt(b)
            elif cid == b"data" and data is None:
                data = (body, left if csz == 0 or csz > left else csz)
                if csz == 0:
                    break
            if csz > left:
                break
            pos = body + csz + (csz & 1)
        if fmt is None:
            raise ValueError("wav: no fmt chunk")
        if data is None:
            raise ValueError("wav: no data chunk")
        name, channels, rate, bits, block_align = fmt
        frames = data[1] // block_align
        if frames < 1:
            raise ValueError("wav: the data chunk holds no whole frame")
        if frames > MAX_FRAMES:
            raise ValueError(f"wav: {frames} frames are more than 2^30")
        return WavInfo(name, channels, rate, bits, block_align, data[0], frames)
    finally:
        rd.close()


def read_payload(src, info: WavInfo):
    """The frames of a parsed file as a uint8 numpy array [frames * block_align] (a view of `bytes`, one read from a path)."""
    n = info.frames * info.block_align
    if _is_path(src):
        with open(src, "rb") as f:
            f.seek(info.data_offset)
            buf = f.read(n)
    else:
        buf = memoryview(src).cast("B")[info.data_offset:info.data_offset + n]
    a = np.frombuffer(buf, dtype=np.uint8)
    if a.shape[0] != n:
        raise ValueError(f"wav: {a.shape[0]} of {n} payload bytes could be read")
    return a


def pcm_rows(table_rows, raw_bytes: int, n_max=None):
    """A decode table -> (records of ROW_DTYPE [B], n_max), checked with the conditions wft_pcm_decode_f32 clamps with.

    table_rows: a sequence of rows (byte_off, frames, channels, format, channel) — format a name of FORMATS or its number, channel
    "mean" / -1 or 0..channels-1 — or a ROW_DTYPE array.  n_max: the output width (None: the largest frame count, at least 1).
    ValueError: no row or more than 65535, a format outside the enum, channels outside 1..8, a channel outside -1..channels-1,
    frames outside 0..n_max, byte_off < 0, byte_off + frames * frame_bytes > raw_bytes, n_max outside 1..2^30, raw_bytes < 1."""
    if isinstance(table_rows, np.ndarray) and table_rows.dtype == ROW_DTYPE:
        rec = np.ascontiguousarray(table_rows).reshape(-1).copy()
    else:
        rows = list(table_rows)
        rec = np.zeros(len(rows), dtype=ROW_DTYPE)
        for b, row in enumerate(rows):
            if len(row) != 5:
                raise ValueError(f"pcm_decode: row {b} must be (byte_off, frames, channels, format, channel), got {row!r}")
            off, frames, channels, fmt, channel = row
            for what, v in (("byte_off", off), ("frames", frames), ("channels", channels)):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                    raise ValueError(f"pcm_decode: row {b}: {what} must be an integer, got {v!r}")
            if not -(1 << 63) <= int(off) < (1 << 63) or not -(1 << 31) <= int(frames) < (1 << 31) or not -(1 << 31) <= int(channels) < (1 << 31):
                raise ValueError(f"pcm_decode: row {b}: a value does not fit its field, got {row!r}")
            if not 1 <= int(channels) <= MAX_CHANNELS:
                raise ValueError(f"pcm_decode: row {b}: channels must lie in [1, {MAX_CHANNELS}], got {channels}")
            rec[b] = (int(off), int(frames), int(channels), format_id(fmt), channel_id(channel, int(channels)), (0, 0))
    B = rec.shape[0]
    if not 1 <= B <= 65535:
        raise ValueError(f"pcm_decode: 1 to 65535 rows per call, got {B}")
    if isinstance(raw_bytes, bool) or not isinstance(raw_bytes, (int, np.integer)) or raw_bytes < 1:
        raise ValueError(f"pcm_decode: raw must hold at least one byte, got {raw_bytes!r}")
    if n_max is None:
        n_max = max(1, int(rec["frames"].max()))
    if isinstance(n_max, bool) or not isinstance(n_max, (int, np.integer)) or not 1 <= n_max <= MAX_FRAMES:
        raise ValueError(f"pcm_decode: n_max must be an integer inside [1, 2^30], got {n_max!r}")
    for b in range(B):
        r = rec[b]
        fmt, C = int(r["format"]), int(r["channels"])
        if not 0 <= fmt < len(FORMATS):
            raise ValueError(f"pcm_decode: row {b}: format {fmt} is outside 0..{len(FORMATS) - 1}")
        if not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f"pcm_decode: row {b}: channels must lie in [1, {MAX_CHANNELS}], got {C}")
        if not -1 <= int(r["channel"]) < C:
            raise ValueError(f"pcm_decode: row {b}: channel {int(r['channel'])} is outside -1..{C - 1}")
        if not 0 <= int(r["frames"]) <= n_max:
            raise ValueError(f"pcm_decode: row {b}: frames {int(r['frames'])} is outside 0..n_max = {n_max}")
        if int(r["byte_off"]) < 0:
            raise ValueError(f"pcm_decode: row {b}: byte_off {int(r['byte_off'])} is negative")
        end = int(r["byte_off"]) + int(r["frames"]) * C * SAMPLE_BYTES[fmt]
        if end > raw_bytes:
            raise ValueError(f"pcm_decode: row {b}: its frames end at byte {end}, raw holds {raw_bytes}")
        if r["reserved"].any():
            raise ValueError(f"pcm_decode: row {b}: the reserved fields must be 0")
    return rec, int(n_max)


def wav_dir_files(bank):
    """{"wav_dir": path[, "channel": c]} -> (the directory's `.wav` files in name order, channel); ValueError: other keys, no
    directory, no `.wav` file in it, a channel that is neither "mean" nor an integer 0..7."""
    if not set(bank.keys()) <= {"wav_dir", "channel"} or "wav_dir" not in bank:
        raise ValueError(f"noise bank: a mapping must be {{'wav_dir': path[, 'channel': c]}} or {{'synthetic': K[, 'seed': s]}}, got {dict(bank)!r}")
    path, channel = bank["wav_dir"], bank.get("channel", "mean")
    if not _is_path(path) or not os.path.isdir(path):
        raise ValueError(f"noise bank: wav_dir {path!r} is not a directory")
    channel_id(channel, MAX_CHANNELS)
    names = sorted(f for f in os.listdir(path) if f.lower().endswith(".wav"))
    if not names:
        raise ValueError(f"noise bank: wav_dir {os.fspath(path)!r} holds no .wav file")
    return [os.path.join(os.fspath(path), f) for f in names], channel
