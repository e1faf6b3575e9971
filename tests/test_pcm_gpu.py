"""wft_pcm_decode_f32 on the device against the float64 restatement of tests/_pcm_cases.py: whole sentinel-filled output buffers, bit
for bit (a NaN must meet a NaN).  `raw` is always a view into the middle of a larger allocation filled with a poison byte, so an
over-read or a broken clamp shows as wrong output and never as an out-of-bounds access."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _pcm_cases as P  # noqa: E402
from whisper_finetune.data import audio_io as AIO  # noqa: E402
from whisper_finetune.data import gpu_frontend as GF  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = torch.device("cuda:0")
SENT = float(P.SENTINEL)
MARGIN = 4096  # poison bytes on either side of raw
PAD = 5        # guard columns of every output row
ERR_ARG = -1   # WFT_ERR_ARG


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _tile():
    return int(L.load().wft_pcm_decode_tile())


def _poisoned(raw: np.ndarray, shift: int = 0):
    """raw uint8 -> (a device view of it inside a larger poisoned allocation, `shift` bytes off a 16-byte boundary; the allocation)."""
    whole = torch.full((raw.shape[0] + 2 * MARGIN + 16,), P.POISON, dtype=torch.uint8, device=DEV)
    start = MARGIN + (-(whole.data_ptr() + MARGIN) % 16) + shift
    view = whole[start:start + raw.shape[0]]
    view.copy_(torch.from_numpy(np.array(raw, dtype=np.uint8)))
    assert (view.data_ptr() - shift) % 16 == 0
    return view, whole


def _table(rows):
    rec = np.zeros(len(rows), dtype=AIO.ROW_DTYPE)
    for b, (off, frames, ch, fmt, channel) in enumerate(rows):
        rec[b] = (off, frames, ch, fmt if isinstance(fmt, int) else P.FORMAT_ID[fmt], channel, (0, 0))
    return torch.from_numpy(rec.view("u1").reshape(len(rows), 32).copy()).to(DEV)


def _decode(raw_d, raw_bytes, rows, n_max, ld=None, table=None):
    """The raw entry point on a sentinel-filled [B, ld] buffer with guards around it -> the whole buffer as numpy."""
    B = len(rows) if table is None else table.shape[0]
    ld = n_max + PAD if ld is None else ld
    buf = torch.full((B * ld + 128,), SENT, dtype=torch.float32, device=DEV)
    out = buf[64:64 + B * ld]
    table = _table(rows) if table is None else table
    L.check(L.load().wft_pcm_decode_f32(_p(raw_d), raw_bytes, _p(table), _p(out), ld, n_max, B, L.stream_ptr()), "wft_pcm_decode_f32")
    whole = buf.cpu().numpy()
    assert bool((whole[:64] == SENT).all() and (whole[-64:] == SENT).all()), "guards around the output"
    return whole[64:-64].reshape(B, ld)


def _check(raw, rows, n_max, shift=0, what=""):
    raw_d, _ = _poisoned(raw, shift)
    got = _decode(raw_d, raw.shape[0], rows, n_max)
    want = P.expected(raw, rows, n_max, n_max + PAD)
    assert P.same_bits(got, want), (what, P.first_difference(got, want))
    return got


def _random_rows(rng, fmt, channels, frames_list, channel, lead=3):
    """Payloads of the listed frame counts back to back, `lead` and 1 odd bytes between them -> (raw, rows)."""
    parts, rows, pos = [], [], 0
    for frames in frames_list:
        gap = bytes([P.POISON]) * (lead if not parts else 1)
        pay = P.random_payload(rng, fmt, frames, channels)
        parts += [gap, pay]
        rows.append((pos + len(gap), frames, channels, fmt, channel))
        pos += len(gap) + len(pay)
    return np.frombuffer(b"".join(parts) + bytes([P.POISON]), dtype=np.uint8), rows


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", P.FORMATS)
def test_tile_seams(fmt, channels):
    T = _tile()
    rng = np.random.default_rng(1000 * P.FORMAT_ID[fmt] + channels)
    frames = [1, T - 1, T, T + 1, 2 * T + 3]
    for channel in (-1, channels - 1):
        raw, rows = _random_rows(rng, fmt, channels, frames, channel)
        _check(raw, rows, 2 * T + 3, what=(fmt, channels, channel))


@pytest.mark.parametrize("fmt, channels", [("s24le", 1), ("s24le", 3), ("u8", 3), ("s16le", 1)])
def test_every_byte_alignment(fmt, channels):
    T = _tile()
    rng = np.random.default_rng(7 + channels)
    pay = P.random_payload(rng, fmt, T + 1, channels)
    for shift in range(16):          # the address of raw itself
        raw = np.frombuffer(pay, dtype=np.uint8)
        _check(raw, [(0, T + 1, channels, fmt, -1)], T + 1, shift=shift, what=("raw", shift))
    for off in range(16):            # byte_off inside an aligned raw
        raw = np.frombuffer(bytes([P.POISON]) * off + pay, dtype=np.uint8)
        _check(raw, [(off, T + 1, channels, fmt, -1), (off, T + 1, channels, fmt, 0)], T + 1, what=("byte_off", off))


def _ragged():
    T = _tile()
    rng = np.random.default_rng(5)
    spec = [("u8", 3, 700, -1), ("s16le", 2, T + 9, -1), ("s24le", 3, 2 * T + 1, 1), ("s32le", 2, 333, -1), ("f32le", 1, T, -1), ("f64le", 2, 1500, -1),
            ("alaw", 1, 2 * T + 3, -1), ("ulaw", 1, 1, -1), ("s16le", 8, 64, 7)]
    parts, rows, pos = [], [], 0
    for k, (fmt, ch, frames, channel) in enumerate(spec):
        gap = bytes([P.POISON]) * (1 + k % 3)
        pay = P.random_payload(rng, fmt, frames, ch)
        parts += [gap, pay]
        rows.append((pos + len(gap), frames, ch, fmt, channel))
        pos += len(gap) + len(pay)
    rows.insert(4, (17, 0, 2, "s16le", -1))  # a frames = 0 row in the middle
    return np.frombuffer(b"".join(parts), dtype=np.uint8), rows, 2 * T + 3


def test_ragged_batch_of_every_format():
    raw, rows, n_max = _ragged()
    got = _check(raw, rows, n_max)
    assert not got[4, :n_max].any() and bool((got[:, n_max:] == SENT).all())
    assert not got[8, 1:n_max].any() and not got[0, 700:n_max].any()  # (ulaw, 1 frame) and (u8, 700 frames)


def test_row_alone_equals_row_in_batch():
    raw, rows, n_max = _ragged()
    raw_d, _ = _poisoned(raw)
    batch = _decode(raw_d, raw.shape[0], rows, n_max)
    for b, row in enumerate(rows):
        alone = _decode(raw_d, raw.shape[0], [row], n_max)
        assert P.same_bits(alone[0], batch[b]), (b, P.first_difference(alone[0], batch[b]))
    out = K.pcm_decode(raw_d, rows)  # the binding: the same bits, its own n_max
    assert tuple(out.shape) == (len(rows), n_max) and P.same_bits(out.cpu().numpy(), batch[:, :n_max])
    ld = n_max + 3
    wide = torch.full((len(rows), ld), SENT, device=DEV)
    assert K.pcm_decode(raw_d, rows, n_max, out=wide[:, :n_max]) is not None
    assert P.same_bits(wide.cpu().numpy(), P.expected(raw, rows, n_max, ld))


def test_clamped_rows_decode_as_zeros():
    """One row per clamp condition, written straight into the device table (the binding would refuse them); the out-of-range rows
    point into the poisoned margin of the allocation, so a broken clamp reads poison (never 0 in any format) and shows."""
    T = _tile()
    rng = np.random.default_rng(11)
    pay = P.random_payload(rng, "s16le", 600, 2)
    raw = np.frombuffer(pay, dtype=np.uint8)
    nb, n_max = raw.shape[0], T + 40
    good = (0, 600, 2, "s16le", -1)
    bad = [(0, 100, 2, 8, -1), (0, 100, 2, -1, -1), (0, 100, 0, "s16le", -1), (0, 100, 9, "s16le", -1), (0, 100, 2, "s16le", 2), (0, 100, 2, "s16le", -2),
           (0, n_max + 1, 1, "u8", -1), (0, -1, 2, "s16le", -1), (-4, 100, 2, "s16le", -1), (-(1 << 62), 100, 2, "s16le", -1), (nb - 396, 100, 2, "s16le", -1),
           (nb, 1, 1, "u8", -1), ((1 << 62), 100, 2, "s16le", -1), (4, 600, 2, "s16le", -1), (0, 301, 1, "f64le", -1), (1201, 400, 1, "s24le", -1)]
    rows = []
    for r in bad:
        rows += [good, r]
    rows.append(good)
    raw_d, _ = _poisoned(raw)
    got = _decode(raw_d, nb, rows, n_max)
    ref = P.decode_row(raw, good, n_max)
    for b, r in enumerate(rows):
        if r is good:
            assert P.same_bits(got[b, :n_max], ref), (b, P.first_difference(got[b, :n_max], ref))
        else:
            assert not got[b, :n_max].any(), (b, r, got[b, :8])
    assert bool((got[:, n_max:] == SENT).all())
    # the last row that still fits decodes: the clamp is not off by one
    edge = [(nb - 400, 100, 2, "s16le", -1), (nb - 1, 1, 1, "u8", -1), (0, 300, 1, "f64le", -1)]
    got = _decode(raw_d, nb, edge, n_max)
    assert P.same_bits(got, P.expected(raw, edge, n_max, n_max + PAD)) and got[0, :100].any()


def test_entry_point_refusals():
    lib = L.load()
    raw_d, _ = _poisoned(np.zeros(64, dtype=np.uint8))
    table = _table([(0, 8, 1, "s16le", -1)])
    out = torch.full((64,), SENT, device=DEV)
    ok = dict(raw=_p(raw_d), raw_bytes=64, rows=_p(table), out=_p(out), ld=16, n_max=16, B=1)
    bad = [dict(raw=_p(None)), dict(rows=_p(None)), dict(out=_p(None)), dict(raw_bytes=0), dict(raw_bytes=-5), dict(B=0), dict(B=65536), dict(B=-1),
           dict(n_max=0), dict(n_max=(1 << 30) + 1, ld=(1 << 30) + 1), dict(ld=15), dict(n_max=-3, ld=0)]
    for change in bad:
        a = {**ok, **change}
        code = lib.wft_pcm_decode_f32(a["raw"], a["raw_bytes"], a["rows"], a["out"], a["ld"], a["n_max"], a["B"], L.stream_ptr())
        assert code == ERR_ARG, (change, code)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())  # nothing was launched
    assert lib.wft_pcm_decode_f32(ok["raw"], 64, ok["rows"], ok["out"], 16, 16, 1, L.stream_ptr()) == 0
    assert not out[:16].cpu().numpy().any() and bool((out[16:] == SENT).all())
    assert _tile() >= 64


def test_case_table_and_special_values():
    """Every case of the host table (the mutants' inputs): S32 pairs that need one rounding, the integer extremes, f32 subnormals
    and infinities bit for bit, F64 values that become f32 subnormals, overflow to infinity or are +-0, NaN as NaN."""
    for case in P.case_table():
        raw, row, n_max = P.case_buffer(case)
        _check(raw, [row], n_max, what=case["name"])
        _check(raw, [row], n_max, shift=5, what=case["name"])
    T = {c["name"]: c for c in P.case_table()}
    raw, row, n_max = P.case_buffer(T["f32_specials_mono"])
    out = GF.decode_pcm(raw.tobytes(), "f32le", byte_offset=1, frames=row[1], device=DEV)
    bits = out.cpu().numpy().view(np.uint32)
    want = np.frombuffer(T["f32_specials_mono"]["payload"], dtype="<u4")
    keep = ~np.isnan(want.view(np.float32))
    assert np.array_equal(bits[keep], want[keep]) and bool(np.isnan(out.cpu().numpy()[~keep]).all())


def test_decode_pcm_public_form():
    rng = np.random.default_rng(2)
    pay = P.random_payload(rng, "s24le", 1001, 3)
    raw = np.frombuffer(b"xy" + pay + b"z", dtype=np.uint8)
    for channel, ch in (("mean", -1), (2, 2)):
        out = GF.decode_pcm(raw.tobytes(), "s24le", channels=3, channel=channel, frames=1001, byte_offset=2, device=DEV)
        assert out.device.type == "cuda" and tuple(out.shape) == (1001,)
        assert P.same_bits(out.cpu().numpy(), P.decode_row(raw, (2, 1001, 3, "s24le", ch), 1001))
    out = GF.decode_pcm(torch.from_numpy(raw.copy()).to(DEV), AIO.FORMAT_ID["s24le"], channels=3, byte_offset=2)  # frames: what fits
    assert P.same_bits(out.cpu().numpy(), P.decode_row(raw, (2, 1001, 3, "s24le", -1), 1001))
    for kw, msg in ((dict(format="s20"), "PCM format"), (dict(channels=9), "channels must be"), (dict(channel=3), "channel must be"),
                    (dict(frames=1002), "frames end at byte"), (dict(byte_offset=-1), "byte_offset"), (dict(frames=0), "at least one whole frame")):
        with pytest.raises(ValueError, match=msg):
            GF.decode_pcm(raw.tobytes(), **{**dict(format="s24le", channels=3, frames=1001, byte_offset=2), **kw})
