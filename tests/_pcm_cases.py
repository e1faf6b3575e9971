"""PCM decode: the numpy float64 restatement of include/wft.h "PCM decode" (the reference of the host and GPU tests), byte builders,
a WAV writer made with `struct`, the case table and the mutants the comparison must reject.  No device, no project import."""
import struct

import numpy as np

FORMATS = ("u8", "s16le", "s24le", "s32le", "f32le", "f64le", "alaw", "ulaw")
FORMAT_ID = {k: i for i, k in enumerate(FORMATS)}
SAMPLE_BYTES = dict(u8=1, s16le=2, s24le=3, s32le=4, f32le=4, f64le=8, alaw=1, ulaw=1)
WAV_TAG = dict(u8=1, s16le=1, s24le=1, s32le=1, f32le=3, f64le=3, alaw=6, ulaw=7)
SENTINEL = np.float32(-12345.0)
POISON = 0xA5  # the byte around `raw` in the GPU tests: as s16 0xA5A5 = -23131, never 0
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


# ------------------------------------------------------------------------------------------------- G.711, all 256 codes
def ulaw_table(bias: bool = True) -> np.ndarray:
    u = (~np.arange(256, dtype=np.int64)) & 0xFF
    b = 0x84 if bias else 0
    t = (((u & 0x0F) << 3) + b) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, b - t, t - b)


def alaw_table(invert: bool = True) -> np.ndarray:
    a = np.arange(256, dtype=np.int64) ^ (0x55 if invert else 0)
    seg = (a & 0x70) >> 4
    t = (a & 0x0F) << 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t)


# ------------------------------------------------------------------------------------------------- the restatement
def channel_values(raw: np.ndarray, fmt: str, channels: int, variant=None) -> np.ndarray:
    """The bytes of whole frames (uint8 [frames * channels * sample_bytes]) -> the exact float64 value of every sample [frames, C]."""
    sb = SAMPLE_BYTES[fmt]
    b = np.ascontiguousarray(raw).reshape(-1, channels, sb).astype(np.int64)
    if fmt == "u8":
        return (b[..., 0] - (0 if variant == "u8_no_offset" else 128)) / 128.0
    if fmt == "s16le":
        v = (b[..., 1] | (b[..., 0] << 8)) if variant == "s16_big_endian" else (b[..., 0] | (b[..., 1] << 8))
        v = np.where(v >= 1 << 15, v - (1 << 16), v)
        return v / (32767.0 if variant == "div_32767" else 32768.0)
    if fmt == "s24le":
        v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
        if variant != "s24_unsigned":
            v = np.where(v >= 1 << 23, v - (1 << 24), v)
        return v / float(1 << 23)
    if fmt == "s32le":
        v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | (b[..., 3] << 24)
        v = np.where(v >= 1 << 31, v - (1 << 32), v)
        return v / float(1 << 31)
    if fmt == "f32le":
        return np.ascontiguousarray(raw).view("<f4").reshape(-1, channels).astype(np.float64)
    if fmt == "f64le":
        return np.ascontiguousarray(raw).view("<f8").reshape(-1, channels).astype(np.float64)
    table = alaw_table(variant != "alaw_no_inversion") if fmt == "alaw" else ulaw_table(variant != "ulaw_no_bias")
    return table[b[..., 0]] / 32768.0


def decode_row(raw: np.ndarray, row, n_max: int, variant=None) -> np.ndarray:
    """raw uint8 [nbytes], row = (byte_off, frames, channels, format name, channel: -1 or an index) -> f32 [n_max]."""
    off, frames, C, fmt, ch = row
    out = np.zeros(n_max, dtype=np.float32)
    if variant == "no_zero_fill":
        out[:] = SENTINEL
    if frames == 0:
        return out
    if variant == "offset_plus_one":
        off += 1
    fb = C * SAMPLE_BYTES[fmt]
    with np.errstate(over="ignore", invalid="ignore"):
        v = channel_values(raw[off:off + frames * fb], fmt, C, variant)
        if ch >= 0:
            x = v[:, (ch + 1) % C if variant == "wrong_channel" else ch]
        else:
            if variant == "f32_channels":
                v = v.astype(np.float32).astype(np.float64)
            acc = v[:, 0].copy()
            for c in range(1, C):
                acc = acc + v[:, c]
                if variant == "f32_sum":
                    acc = acc.astype(np.float32).astype(np.float64)
            x = acc * float(np.float32(1.0 / C)) if variant == "mul_reciprocal" else acc / float(C)
        out[:frames] = x.astype(np.float32)
    return out


MUTANTS = ("s24_unsigned", "s16_big_endian", "div_32767", "u8_no_offset", "f32_channels", "f32_sum", "mul_reciprocal", "wrong_channel",
           "offset_plus_one", "no_zero_fill", "alaw_no_inversion", "ulaw_no_bias")


def expected(raw: np.ndarray, rows, n_max: int, ld: int, variant=None) -> np.ndarray:
    """The whole sentinel-filled output buffer f32 [B, ld] a decode of `rows` must leave."""
    out = np.full((len(rows), ld), SENTINEL, dtype=np.float32)
    for b, row in enumerate(rows):
        out[b, :n_max] = decode_row(raw, row, n_max, variant)
    return out


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Whole buffers, bit for bit; a NaN must meet a NaN (its payload is unpinned)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    return bool(np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


def first_difference(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    idx = np.argwhere(bad)
    if idx.shape[0] == 0:
        return None
    i = tuple(int(k) for k in idx[0])
    return f"{idx.shape[0]} differences, first at {i}: got {got[i]!r} ({got.view(np.uint32)[i]:#010x}), want {want[i]!r} ({want.view(np.uint32)[i]:#010x})"


# ------------------------------------------------------------------------------------------------- byte builders
def pack_ints(values, fmt: str) -> bytes:
    """Integers in the format's own range (u8: 0..255; s16 / s24 / s32: signed; alaw / ulaw: the code 0..255) -> their bytes."""
    v = np.asarray(values, dtype=np.int64).reshape(-1)
    sb = SAMPLE_BYTES[fmt]
    u = v & ((1 << (8 * sb)) - 1)
    return np.stack([(u >> (8 * k)) & 0xFF for k in range(sb)], axis=1).astype(np.uint8).tobytes()


def pack_floats(values, fmt: str) -> bytes:
    return np.asarray(values).astype("<f4" if fmt == "f32le" else "<f8").tobytes()


def random_payload(rng, fmt: str, frames: int, channels: int) -> bytes:
    """Frames of seeded samples: every bit pattern for the integer and G.711 formats, finite values of mixed magnitude for floats."""
    n = frames * channels
    if fmt in ("f32le", "f64le"):
        v = rng.standard_normal(n) * np.exp2(rng.integers(-20, 3, n).astype(np.float64))
        return pack_floats(v, fmt)
    return rng.integers(0, 256, n * SAMPLE_BYTES[fmt], dtype=np.uint8).tobytes()


def wav_bytes(fmt: str, channels: int, rate: int, payload: bytes, *, fmt_size: int = 16, extensible: bool = False, valid_bits=None,
              before_data=(), after_fmt=(), data_first: bool = False, data_size=None, riff_size=None, magic: bytes = b"RIFF",
              tag=None, block_align=None, bits=None) -> bytes:
    """A WAV file packed by hand.  before_data / after_fmt: extra (id, body) chunks (an odd body gets its pad byte); data_first puts
    `data` in front of `fmt `; data_size / riff_size / tag / block_align / bits override the honest header fields."""
    sb = SAMPLE_BYTES[fmt]
    bits = 8 * sb if bits is None else bits
    tag = WAV_TAG[fmt] if tag is None else tag
    align = channels * sb if block_align is None else block_align
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * channels * sb, align, bits)
    if extensible:
        body += struct.pack("<HHI", 22, bits if valid_bits is None else valid_bits, 0) + struct.pack("<H", tag) + GUID_TAIL
    elif fmt_size == 18:
        body += struct.pack("<H", 0)
    elif fmt_size == 40:
        body += struct.pack("<H", 22) + bytes(22)

    def chunk(cid, b, size=None):
        return cid + struct.pack("<I", len(b) if size is None else size) + b + (b"\0" if len(b) & 1 else b"")

    f = chunk(b"fmt ", body) + b"".join(chunk(c, b) for c, b in after_fmt)
    d = b"".join(chunk(c, b) for c, b in before_data) + chunk(b"data", payload, data_size)
    rest = b"WAVE" + (d + f if data_first else f + d)
    return magic + struct.pack("<I", len(rest) if riff_size is None else riff_size) + rest


# ------------------------------------------------------------------------------------------------- the case table
def _case(name, fmt, channels, channel, payload):
    frames = len(payload) // (channels * SAMPLE_BYTES[fmt])
    return dict(name=name, fmt=fmt, channels=channels, channel=channel, payload=payload, frames=frames)


def case_table(seed: int = 0):
    """Small cases with planted inputs; each is decoded at byte offset 1 inside a buffer of its payload (see `case_buffer`)."""
    rng = np.random.default_rng(seed)
    T = []
    for fmt in FORMATS:  # every format, random bits, mean of 3 and a picked channel of 2
        T.append(_case(f"{fmt}_mean3", fmt, 3, -1, random_payload(rng, fmt, 257, 3)))
        T.append(_case(f"{fmt}_pick1of2", fmt, 2, 1, random_payload(rng, fmt, 130, 2)))
        T.append(_case(f"{fmt}_mono", fmt, 1, -1, random_payload(rng, fmt, 97, 1)))
    T.append(_case("g711_all_codes_alaw", "alaw", 1, -1, bytes(range(256))))
    T.append(_case("g711_all_codes_ulaw", "ulaw", 1, -1, bytes(range(256))))
    T.append(_case("u8_all_codes", "u8", 1, -1, bytes(range(256))))
    # S32LE pairs whose mean needs one rounding and not two: with k = 2^24, (k + 1, k + 2) * 64 has the exact mean (k + 1.5) * 64 ->
    # f32 (k + 2) * 64, but f32(k + 1) = k (a tie to even) makes the twice-rounded mean (k + 1) * 64 -> k * 64
    k = 1 << 24
    pairs = [((k + 1) * 64, (k + 2) * 64), (-(k + 1) * 64, -(k + 2) * 64), ((k + 3) * 64, (k + 6) * 64), ((1 << 31) - 1, (1 << 31) - 1),
             (-(1 << 31), -(1 << 31)), ((1 << 31) - 1, -(1 << 31)), ((1 << 31) - 1, 1), (k + 1, k + 3), (3 * k + 1, 3 * k - 1), (-(k + 1), k + 3)]
    T.append(_case("s32_one_rounding_pairs", "s32le", 2, -1, pack_ints(pairs, "s32le")))
    T.append(_case("s32_extremes_mono", "s32le", 1, -1, pack_ints([(1 << 31) - 1, -(1 << 31), k + 1, k + 3, -(k + 1), 2 * k + 2, 2 * k + 6, 0, 1, -1], "s32le")))
    T.append(_case("s32_triples", "s32le", 3, -1, pack_ints([((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1), (k + 1, 1, 1), (1, 1, k + 1), (-(1 << 31), (1 << 31) - 1, 1),
                                                              ((k + 1) * 64, 3, -5)], "s32le")))
    T.append(_case("s24_extremes", "s24le", 1, -1, pack_ints([(1 << 23) - 1, -(1 << 23), -1, 0, 1, 0x7F00FF - (1 << 24), 0x123456], "s24le")))
    T.append(_case("s16_extremes", "s16le", 2, -1, pack_ints([(32767, 32767), (-32768, -32768), (32767, -32768), (1, 0), (-1, 0), (0x0102, 0x0304)], "s16le")))
    tiny, fmax = 2.0 ** -149, float(np.finfo(np.float32).max)
    f64_edges = [0.0, -0.0, tiny, -tiny, tiny / 2, tiny * 0.75, tiny * 1.5, 1e-40, -1e-40, 2.0 ** -126, 2.0 ** -127, 1e39, -1e39, fmax, fmax + 2.0 ** 103,
                 fmax + 2.0 ** 102, np.inf, -np.inf, np.nan, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24, 1e-320]
    T.append(_case("f64_edges_mono", "f64le", 1, -1, pack_floats(f64_edges, "f64le")))
    T.append(_case("f64_edges_pick", "f64le", 2, 0, pack_floats(np.stack([f64_edges, np.ones(len(f64_edges))], 1), "f64le")))
    T.append(_case("f64_mean_overflow", "f64le", 2, -1, pack_floats([(fmax, fmax), (1e308, 1e308), (tiny, 0.0), (tiny, tiny), (3 * tiny, 0.0), (np.inf, -np.inf)], "f64le")))
    f32_bits = np.array([0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
                         0x3F800001, 0x7FC00000, 0x00400000], dtype="<u4")
    T.append(_case("f32_specials_mono", "f32le", 1, -1, f32_bits.tobytes()))
    T.append(_case("f32_specials_pick", "f32le", 2, 1, np.stack([np.full(f32_bits.shape[0], 0x3F800000, "<u4"), f32_bits], 1).tobytes()))
    return T


def case_buffer(case, lead: int = 1):
    """A case -> (raw uint8 with `lead` poison bytes in front of the payload and 3 behind it, its table row, n_max = frames + 7)."""
    raw = np.frombuffer(bytes([POISON]) * lead + case["payload"] + bytes([POISON]) * 3, dtype=np.uint8)
    return raw, (lead, case["frames"], case["channels"], case["fmt"], case["channel"]), case["frames"] + 7
