"""Per-row rate conversion on the device: wft_alias_f32 bit for bit against numpy, wft_sinc_resample_rows_f32 under the per-element
bound of tests/_rate_cases.py, the wrappers, the pitch shift and the loader's rate stages against replays from the public pieces."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _rate_cases as R  # noqa: E402
from whisper_finetune.data import data_loader as DL  # noqa: E402
from whisper_finetune.data import filters as F  # noqa: E402
from whisper_finetune.data import gpu_frontend as GF  # noqa: E402
from whisper_finetune.data import rate_fx as RF  # noqa: E402
from whisper_finetune.data import wave_fx as WF  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = torch.device("cuda:0")
TA = L.load().wft_alias_tile()
tile = L.load().wft_sinc_resample_rows_tile
SENT = float(R.SENTINEL)
GUARD = 64
SR = 16000.0


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _guarded(shape, dtype=torch.float32, fill=SENT):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(*shape), buf


def _input(rows, ns, ld):
    """numpy rows -> a guarded device buffer [B, ld] with NaN planted behind n[b]."""
    host = np.full((len(rows), ld), np.nan, dtype=np.float32)
    for b, (x, n) in enumerate(zip(rows, ns)):
        k = min(max(n, 0), len(x), ld)
        host[b, :k] = x[:k]
    inp, ibuf = _guarded((len(rows), ld))
    inp.copy_(torch.from_numpy(host))
    return inp, ibuf


# ------------------------------------------------------------------------------------------------------------ alias
def _alias_run(rows, ns, rates, n_max, pad=3, use_n=True):
    """-> the whole output buffer incl. guards as numpy; rows: list of f32 arrays, row b covering ns[b] samples."""
    B, ld = len(rows), n_max + pad
    inp, _ = _input(rows, ns if use_n else [n_max] * B, ld)
    out, obuf = _guarded((B, ld))
    n_dev = torch.tensor(ns, dtype=torch.int32, device=DEV) if use_n else None
    rate_d = torch.tensor(rates, dtype=torch.float64, device=DEV)
    L.check(L.load().wft_alias_f32(_p(inp), ld, _p(n_dev), n_max, _p(rate_d), SR, _p(out), ld, B, L.stream_ptr()), "wft_alias_f32")
    torch.cuda.synchronize()
    return obuf.cpu().numpy()


def _alias_expect(x, n, rate):
    n = max(n, 0)
    if rate == 0 or n < 2 or R.alias_d(n, rate, SR) < 2:
        return np.asarray(x[:n], dtype=np.float32).copy()
    return R.alias_numpy(x[:n], rate, SR).astype(np.float32)


def _alias_check(obuf, rows, ns, rates, n_max, ld, what):
    B = len(rows)
    assert bool((obuf[:GUARD] == R.SENTINEL).all() and (obuf[-GUARD:] == R.SENTINEL).all()), (what, "guards")
    got = obuf[GUARD:GUARD + B * ld].reshape(B, ld)
    for b in range(B):
        n = min(max(ns[b], 0), n_max)
        assert bool((got[b, n_max:] == R.SENTINEL).all()), (what, b, "behind n_max")
        assert not R.bits(got[b, n:n_max]).any(), (what, b, "behind n[b]: zeros")
        want = _alias_expect(rows[b], n, rates[b])
        diff = np.flatnonzero(R.bits(got[b, :n]) != R.bits(want))
        assert diff.size == 0, (what, b, n, rates[b], diff[:5], got[b, diff[:5]], want[diff[:5]])


ALIAS_NS = (2, 3, 5, TA - 1, TA, TA + 1, 2 * TA + 3)


@pytest.mark.parametrize("n", ALIAS_NS)
def test_alias_bit_for_bit_against_numpy(n):
    """EVERY rate of alias_rates_for(n) — every d of the issue for this n and the rounding cases — and one "none" rate on the row of
    length n, every input kind, batches of three rows with their own n and rate: the row under test, a neighbour of another length
    (its own rates in turn) and a Gaussian row."""
    rates = R.alias_rates_for(n, SR) + [0.0]
    assert {R.alias_d(n, r, SR) for r in rates} >= {d for d in (2, n - 1, n, n + 1, n // 2, int(1.9 * n)) if d >= 2}
    other = ALIAS_NS[(ALIAS_NS.index(n) + 3) % len(ALIAS_NS)]
    other_rates = R.alias_rates_for(other, SR)
    n_max = max(n, other, 7)
    for name, x in R.alias_inputs(n, TA, seed=n).items():
        for i in range(len(rates)):
            rs = [rates[i], other_rates[i % len(other_rates)], 0.7 * SR]
            rows, ns = [x, R.alias_inputs(other, TA, seed=5)[name], R.signal(7, 9)], [n, other, 7]
            obuf = _alias_run(rows, ns, rs, n_max)
            _alias_check(obuf, rows, ns, rs, n_max, n_max + 3, (n, name, i))


def test_alias_row_alone_equals_the_row_in_a_batch_and_null_n_is_n_max():
    n_max = 2 * TA + 3
    rows = [R.signal(n_max, s) for s in (1, 2, 3)]
    ns, rates = [n_max, TA + 1, 5], [0.55 * SR, 1.9 * SR, 0.0]
    batch = _alias_run(rows, ns, rates, n_max)[GUARD:-GUARD].reshape(3, -1)
    for b in range(3):
        alone = _alias_run([rows[b]], [ns[b]], [rates[b]], n_max)[GUARD:-GUARD].reshape(1, -1)
        assert np.array_equal(R.bits(alone[0]), R.bits(batch[b])), b
    full = _alias_run(rows, [n_max] * 3, rates, n_max, use_n=False)
    _alias_check(full, rows, [n_max] * 3, rates, n_max, n_max + 3, "null n")
    # n is clamped on the device
    wild = _alias_run(rows, [n_max + 100, -5, 2], rates, n_max)
    _alias_check(wild, rows, [n_max, 0, 2], rates, n_max, n_max + 3, "clamped n")


def test_alias_refusals_leave_the_output_untouched():
    n_max, ld = TA + 3, TA + 8
    inp, ibuf = _guarded((3, ld), fill=0.25)
    out, obuf = _guarded((3, ld))
    rate = torch.full((3,), 8000.0, dtype=torch.float64, device=DEV)
    lib = L.load()
    args = lambda **k: [k.get("inp", _p(inp)), k.get("ld_in", ld), k.get("n", None), k.get("n_max", n_max), k.get("rate", _p(rate)),  # noqa: E731
                        k.get("sr", SR), k.get("out", _p(out)), k.get("ld_out", ld), k.get("B", 3), L.stream_ptr()]
    flat = ibuf[GUARD:GUARD + 3 * ld]
    cases = {"null in": dict(inp=None), "null rate": dict(rate=None), "null out": dict(out=None), "sample_rate 0": dict(sr=0.0),
             "sample_rate nan": dict(sr=float("nan")), "sample_rate inf": dict(sr=float("inf")), "B = 0": dict(B=0), "B too large": dict(B=65536),
             "n_max = 0": dict(n_max=0), "n_max too large": dict(n_max=(1 << 30) + 1, ld_in=1 << 31, ld_out=1 << 31),
             "ld_in < n_max": dict(ld_in=n_max - 1), "ld_out < n_max": dict(ld_out=n_max - 1),
             "in off by 2 bytes": dict(inp=C.c_void_p(inp.data_ptr() + 2)), "rate off by 4 bytes": dict(rate=C.c_void_p(rate.data_ptr() + 4)),
             "in place": dict(out=_p(inp)), "shifted overlap": dict(out=_p(flat[5:]))}
    for what, k in cases.items():
        assert lib.wft_alias_f32(*args(**k)) != 0 and "wft_alias_f32" in L.last_error(), what
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all()) and bool((ibuf[GUARD:-GUARD] == 0.25).all())


def test_alias_wild_device_rates_copy_the_row():
    n_max = TA + 5
    rows = [R.signal(n_max, s) for s in (1, 2, 3, 4)]
    rates = [float("nan"), -8000.0, 1e300, float("inf")]
    obuf = _alias_run(rows, [n_max] * 4, rates, n_max)
    _alias_check(obuf, rows, [n_max] * 4, [0.0] * 4, n_max, n_max + 3, "wild rates")


# ------------------------------------------------------------------------------------------------------------ sinc
def _sinc_run(rows, ns, rhos, n_in_max, n_out, ratio_lo, pad=3, ns_dev=None):
    """ns: the samples planted per row (NaN behind them); ns_dev: what the device is told (default: the same)."""
    B, ld_in, ld_out = len(rows), n_in_max + pad, n_out + pad
    inp, _ = _input(rows, ns, ld_in)
    out, obuf = _guarded((B, ld_out))
    n_dev = torch.tensor(ns if ns_dev is None else ns_dev, dtype=torch.int32, device=DEV)
    rho_d = torch.tensor(rhos, dtype=torch.float64, device=DEV)
    L.check(L.load().wft_sinc_resample_rows_f32(_p(inp), ld_in, _p(n_dev), n_in_max, _p(rho_d), ratio_lo, _p(out), ld_out, n_out, B,
                                                L.stream_ptr()), "wft_sinc_resample_rows_f32")
    torch.cuda.synchronize()
    return obuf.cpu().numpy()


def _sinc_check(obuf, rows, ns, rhos, n_out, ld_out, what, stats=None):
    B = len(rows)
    assert bool((obuf[:GUARD] == R.SENTINEL).all() and (obuf[-GUARD:] == R.SENTINEL).all()), (what, "guards")
    got = obuf[GUARD:GUARD + B * ld_out].reshape(B, ld_out)
    for b in range(B):
        assert bool((got[b, n_out:] == R.SENTINEL).all()), (what, b, "behind n_out")
        ref, mag = R.sinc_ref(rows[b][:max(ns[b], 0)], ns[b], rhos[b], n_out)
        bad, frac, off = R.sinc_violations(got[b, :n_out], ref, mag)
        print(f"sinc {what} row {b}: N {ns[b]} rho {rhos[b]!r} n_out {n_out}: outside {bad}, largest fraction of the bound {frac:.4f}, "
              f"not the rounded reference {off:.5f}")
        assert bad == 0, (what, b, ns[b], rhos[b], bad, frac)
        lim = R.sinc_limit(max(ns[b], 0), rhos[b], n_out)
        assert not R.bits(got[b, lim:n_out]).any(), (what, b, "fix_length: zeros")
        if stats is not None:
            stats.append((frac, off, n_out))


@pytest.mark.parametrize("lo", [0.5, "own"])
@pytest.mark.parametrize("rho", R.RHOS)
def test_sinc_rows_against_the_reference(rho, lo):
    """Every N of the issue at this ratio in batches of three, n_out between the rows' ceil(N rho), and the long batch (n_out above
    every row's ceil(N rho), three to nine workgroups per row, full tiles); impulses at 0, N - 1 and every staging seam, ones,
    Gaussian rows; NaN behind n_in[b]; the whole sentinel-filled output compared."""
    ratio_lo = 0.5 if lo == 0.5 else rho
    T = tile(ratio_lo)
    batches = R.sinc_batches(T, (rho,))
    assert len(batches) == 4 and -(-batches[-1][1] // T) >= 3 and batches[-1][1] > np.ceil(batches[-1][0][0][0] * rho)
    for rows_spec, n_out in batches:
        ns, rhos = [n for n, _ in rows_spec], [r for _, r in rows_spec]
        n_in_max = max(max(ns), 1)
        for name in ("impulses", "ones", "gauss"):
            rows = [R.sinc_probe_rows(n, r, T, seed=n + 1)[name] for n, r in rows_spec]
            obuf = _sinc_run(rows, ns, rhos, n_in_max, n_out, ratio_lo)
            _sinc_check(obuf, rows, ns, rhos, n_out, n_out + 3, (rho, lo, name, tuple(ns)))


def test_sinc_mixed_batch_row_alone_and_two_ratio_lo():
    T = tile(0.5)
    rows_spec, n_out = R.sinc_mixed(T)
    ns, rhos = [n for n, _ in rows_spec], [r for _, r in rows_spec]
    assert len(set(rhos)) == 3
    n_in_max = max(ns)
    rows = [R.sinc_probe_rows(n, r, T, seed=b)["gauss"] + R.sinc_probe_rows(n, r, T, seed=b)["impulses"] for b, (n, r) in enumerate(rows_spec)]
    batch = _sinc_run(rows, ns, rhos, n_in_max, n_out, 0.5)
    _sinc_check(batch, rows, ns, rhos, n_out, n_out + 3, "mixed")
    got = batch[GUARD:-GUARD].reshape(3, -1)
    for b in range(3):  # alone, and under another host bound (another tile: 784 against 1024 outputs per workgroup)
        alone = _sinc_run([rows[b]], [ns[b]], [rhos[b]], n_in_max, n_out, 0.5)[GUARD:-GUARD].reshape(1, -1)
        assert np.array_equal(R.bits(alone[0]), R.bits(got[b])), (b, "alone")
        if rhos[b] == 0.5:  # (a row at the lowest ratio has no other bound)
            continue
        lo2 = min(rhos[b], 0.75)
        # several workgroups under both bounds, and no workgroup boundary in common but output 0
        assert tile(lo2) == 1024 and n_out > 2 * 1024 and set(range(0, n_out, T)) & set(range(0, n_out, 1024)) == {0}
        other = _sinc_run([rows[b]], [ns[b]], [rhos[b]], n_in_max, n_out, lo2)[GUARD:-GUARD].reshape(1, -1)
        assert np.array_equal(R.bits(other[0]), R.bits(got[b])), (b, "ratio_lo")
    # n_in is clamped on the device; the stretch's -1 counts as 0
    assert ns[1] == n_in_max
    wild = _sinc_run(rows, [ns[0], ns[1], 0], rhos, n_in_max, n_out, 0.5, ns_dev=[ns[0], n_in_max + 50, -1])
    _sinc_check(wild, rows, [ns[0], ns[1], 0], rhos, n_out, n_out + 3, "clamped")


def test_sinc_out_of_range_device_ratio_gives_zeros_and_touches_no_guard():
    T = tile(0.75)
    n_in, n_out = 2 * T + 5, 3 * T
    rows = [R.signal(n_in, s) for s in range(6)]
    rhos = [float("nan"), 0.7499, 2.0000001, -1.0, float("inf"), 1.0]  # below the HOST's bound counts as outside too
    obuf = _sinc_run(rows, [n_in] * 6, rhos, n_in, n_out, 0.75)
    assert bool((obuf[:GUARD] == R.SENTINEL).all() and (obuf[-GUARD:] == R.SENTINEL).all())
    got = obuf[GUARD:-GUARD].reshape(6, -1)
    for b in range(5):
        assert not R.bits(got[b, :n_out]).any() and bool((got[b, n_out:] == R.SENTINEL).all()), b
    ref, mag = R.sinc_ref(rows[5], n_in, 1.0, n_out)
    assert R.sinc_violations(got[5, :n_out], ref, mag)[0] == 0 and got[5, :n_in].any()


def test_sinc_refusals_leave_the_output_untouched():
    n_in, n_out = 900, 1000
    inp, ibuf = _guarded((3, n_in + 4), fill=0.25)
    out, obuf = _guarded((3, n_out + 4))
    n_dev = torch.full((3,), n_in, dtype=torch.int32, device=DEV)
    rho = torch.full((3,), 1.0, dtype=torch.float64, device=DEV)
    lib = L.load()
    args = lambda **k: [k.get("inp", _p(inp)), k.get("ld_in", n_in + 4), k.get("n", _p(n_dev)), k.get("n_in_max", n_in), k.get("rho", _p(rho)),  # noqa: E731
                        k.get("lo", 0.5), k.get("out", _p(out)), k.get("ld_out", n_out + 4), k.get("n_out", n_out), k.get("B", 3), L.stream_ptr()]
    flat = ibuf[GUARD:GUARD + 3 * (n_in + 4)]
    cases = {"null in": dict(inp=None), "null n_in": dict(n=None), "null ratio": dict(rho=None), "null out": dict(out=None),
             "ratio_lo below 0.5": dict(lo=0.49), "ratio_lo above 2": dict(lo=2.01), "ratio_lo nan": dict(lo=float("nan")),
             "B = 0": dict(B=0), "B too large": dict(B=65536), "n_in_max = 0": dict(n_in_max=0), "n_out = 0": dict(n_out=0),
             "n_out too large": dict(n_out=(1 << 30) + 1, ld_out=1 << 31), "n_in_max too large": dict(n_in_max=(1 << 30) + 1, ld_in=1 << 31),
             "ld_in short": dict(ld_in=n_in - 1), "ld_out short": dict(ld_out=n_out - 1),
             "in off by 2 bytes": dict(inp=C.c_void_p(inp.data_ptr() + 2)), "ratio off by 4 bytes": dict(rho=C.c_void_p(rho.data_ptr() + 4)),
             "n_in off by 2 bytes": dict(n=C.c_void_p(n_dev.data_ptr() + 2)),
             "in place": dict(out=_p(inp), ld_out=n_in + 4, n_out=n_in), "shifted overlap": dict(out=_p(flat[7:]), ld_out=n_in + 4, n_out=n_in)}
    for what, k in cases.items():
        assert lib.wft_sinc_resample_rows_f32(*args(**k)) != 0 and "wft_sinc_resample_rows_f32" in L.last_error(), what
    with pytest.raises(ValueError):  # a ratio that only the device would see: the wrapper refuses it
        K.sinc_resample_rows(inp, n_dev, [1.0, 2.5, 1.0], n_out)
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all()) and bool((ibuf[GUARD:-GUARD] == 0.25).all())


# ------------------------------------------------------------------------------------------------------------ wrappers, pitch
def test_wrappers_and_frontend():
    T = tile(0.5)
    n = 2 * T + 5
    x = torch.from_numpy(np.stack([R.signal(n, s) for s in (1, 2, 3)])).to(DEV)
    ns, rhos = [n, T + 1, 13], [0.5, R.RHOS[4], 1.0]
    n_dev = torch.tensor(ns, dtype=torch.int32, device=DEV)
    out = K.sinc_resample_rows(x, n_dev, rhos, T + 9)
    assert tuple(out.shape) == (3, T + 9) and out.dtype == torch.float32
    for b in range(3):
        ref, mag = R.sinc_ref(x[b, :ns[b]].cpu().numpy(), ns[b], rhos[b], T + 9)
        assert R.sinc_violations(out[b].cpu().numpy(), ref, mag)[0] == 0, b
    wide = torch.zeros(3, n + 11, device=DEV)
    wide[:, :n] = x
    assert torch.equal(K.sinc_resample_rows(wide[:, :n], n_dev, rhos, T + 9), out)  # a strided view: the same bits
    # alias: per-row rates, "none" rows, n
    rates = [8000.0, 0.0, 11025.0]
    al = K.alias(x, rates, n_dev)
    assert al is not x and tuple(al.shape) == (3, n)
    for b in range(3):
        want = _alias_expect(x[b].cpu().numpy(), ns[b], rates[b])
        assert np.array_equal(R.bits(al[b, :ns[b]].cpu().numpy()), R.bits(want)) and not al[b, ns[b]:].view(torch.int32).any(), b
    one = GF.alias(x[0].cpu().numpy(), 9000.0)
    assert one.is_cuda and np.array_equal(R.bits(one.cpu().numpy()), R.bits(R.alias_numpy(x[0].cpu().numpy(), 9000.0, SR).astype(np.float32)))
    two = GF.alias(x, [0.0, 16000.0, 12000.0])
    assert torch.equal(two[0], x[0]) and torch.equal(two[1], x[1]) and not torch.equal(two[2], x[2])  # none; d == n is a copy too


def test_pitch_shift_is_the_stretch_and_the_resampler_and_moves_a_sine():
    t = np.arange(16000) / 16000.0
    y = np.sin(2 * np.pi * 440.0 * t).astype(np.float32)
    semis = [12.0, 4.0, -4.0]
    batch = torch.from_numpy(np.stack([y] * 3)).to(DEV)
    got = GF.pitch_shift(batch, semis)
    assert tuple(got.shape) == (3, 16000)
    rates = 2.0 ** (-np.asarray(semis) / 12.0)
    stretched, n_out = K.time_stretch(batch, rates)
    assert torch.equal(got, K.sinc_resample_rows(stretched, n_out, rates, 16000))  # the replay from the public pieces
    for b, s in enumerate(semis):
        hz = R.peak_hz(got[b].cpu().numpy())
        assert abs(hz - 440.0 * 2.0 ** (s / 12.0)) <= 1.0, (s, hz)
        assert torch.equal(GF.pitch_shift(y, s), got[b])  # one row, from the host: the same bits
    assert float(got[0].abs().max()) > 0.5


# ------------------------------------------------------------------------------------------------------------ loader
N_MELS = 80
SPEC = {"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 1.0}
EXT = {"low_freq_range": 5, "high_freq_range": 5}
STRETCH = dict(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25)
FILT = {"p": 1.0}
WAVE = {"noise": {"p": 1.0}, "clip": {"p": 1.0, "kinds": {"clipping": {"p": 1.0}}}, "level": {"p": 1.0, "kinds": {"gain": {}}}}
RATE = {"alias": {"p": 1.0}, "pitch": {"p": 1.0}}


def _loader(**kw):
    return DL.get_dataloader(DL.SyntheticDataset(2, with_timestamps=True), DL.SimpleTokenizer(), batch_size=2, n_mels=N_MELS, shuffle=False,
                             device=DEV, no_timestamp_training=True, spec_augment=True, spec_augment_params=SPEC, extremes_spec_augment=True,
                             extremes_spec_augment_params=EXT, **kw)


def _seed():
    torch.manual_seed(11)
    random.seed(11)


def _pitch_replay(x, table, lengths):
    """The PITCH stage from the public pieces, row by row: stretch the row's own length, resample back to it."""
    x = x.clone()
    for b in range(x.shape[0]):
        n = lengths[b]
        rate = GF.pitch_rates(float(table[b, 3]), 1)
        st, n_st = K.time_stretch(x[b:b + 1, :n], rate)
        x[b, :n] = K.sinc_resample_rows(st, n_st, rate, n)[0]
    return x


def test_loader_batch_with_stretch_equals_a_replay_in_the_stated_order():
    on = _loader(rate_aug=RATE, wave_aug=WAVE, filter_aug=FILT, **STRETCH)
    assert isinstance(on, DL.GpuMelLoader) and on.rate_aug and on.wave_aug and on.filter_aug and on.stretch
    _seed()
    mel, y_in, y_out = next(iter(on))
    _seed()
    audio, yi, yo, params, ext, cut, rates, sos, wtable, table = next(iter(on.loader))
    assert table.dtype == torch.float64 and tuple(table.shape) == (2, RF.TABLE_WIDTH) and bool(table[:, [0, 2]].all())
    rec = WF.check_records(WF.records_from_table(wtable))
    x, n_out = K.time_stretch(audio.to(DEV), rates)
    lengths = [int(round(480000 / float(r))) for r in rates]
    assert n_out.tolist() == lengths and len(set(lengths)) == 2  # the host knows the lengths; the pitched rows differ in length
    x = K.wave_fx(x, rec, "noise", n_out)
    x = K.alias(x, table[:, 1], n_out)
    x = K.sos_filter(x, sos, n_out)
    x = K.wave_fx(x, rec, "clip", n_out)
    x = K.wave_fx(x, rec, "level", n_out)
    before_pitch = x
    x = _pitch_replay(x, table.numpy(), lengths)
    keep = cut.clamp(max=3000).to(torch.int32).to(DEV)
    want = K.specaug(K.logmel_ragged(x, n_out, keep, on.frontend.filters, 3000), params.to(DEV), ext.to(DEV))
    assert tuple(mel.shape) == (2, N_MELS, 3000) and torch.equal(mel, want)
    assert torch.equal(y_in.cpu(), yi) and torch.equal(y_out.cpu(), yo)
    assert not torch.equal(x, before_pitch)


def test_loader_batch_without_the_stretch_equals_a_replay_and_unpitched_rows_keep_their_bits():
    on = _loader(rate_aug=RATE)
    assert on.rate_aug and not on.wave_aug and not on.filter_aug and not on.stretch
    _seed()
    mel = next(iter(on))[0]
    _seed()
    audio, yi, yo, params, ext, cut, table = next(iter(on.loader))
    x = K.alias(audio.to(DEV), table[:, 1])
    x = GF.pitch_shift(x, table[:, 3])  # every row has 480000 samples: one batched call
    plain = K.logmel(x, on.frontend.filters, 3000)
    for b in (cut < 3000).nonzero().flatten().tolist():
        c = int(cut[b])
        plain[b, :, c:] = plain[b, :, :c].min() if c > 0 else plain[b].min()
    assert torch.equal(mel, K.specaug(plain, params.to(DEV), ext.to(DEV))) and not torch.equal(x.cpu(), audio)
    # pitch gathers the pitched rows only: the other row keeps its bits
    y = audio.to(DEV).clone()
    DL.pitch_rows(y, [None, 3.0])
    assert torch.equal(y[0].cpu(), audio[0]) and torch.equal(y[1], GF.pitch_shift(audio[1].to(DEV), 3.0))


@pytest.mark.parametrize("stretch", [False, True])
def test_loader_without_the_option_and_with_both_gates_at_zero_gives_the_batches_of_before(stretch, monkeypatch):
    kw = STRETCH if stretch else {}
    off = _loader(**kw)
    assert not off.rate_aug
    _seed()
    got = next(iter(off))
    _seed()
    batch = next(iter(off.loader))
    assert len(batch) == 6 + int(stretch)
    # the parent commit's code path: [stretch ->] log-mel -> cut -> SpecAugment, nothing else
    if stretch:
        x, n_out = K.time_stretch(batch[0].to(DEV), batch[6])
        keep = batch[5].clamp(max=3000).to(torch.int32).to(DEV)
        plain = K.logmel_ragged(x, n_out, keep, off.frontend.filters, 3000)
    else:
        plain = K.logmel(batch[0].to(DEV), off.frontend.filters, 3000)
        for b in (batch[5] < 3000).nonzero().flatten().tolist():
            c = int(batch[5][b])
            plain[b, :, c:] = plain[b, :, :c].min() if c > 0 else plain[b].min()
    assert torch.equal(got[0], K.specaug(plain, batch[3].to(DEV), batch[4].to(DEV)))
    if not stretch:  # both gates at zero: two failed draws per clip, after everything else; the same batches and no launch
        zero = _loader(rate_aug={"alias": {"p": 0.0}, "pitch": {"p": 0.0}})
        for name in ("alias", "sinc_resample_rows"):
            monkeypatch.setattr(K, name, lambda *a, **k: pytest.fail("a batch without any rate effect must launch nothing"))
        _seed()
        again = next(iter(zero))
        for u, v in zip(again, got):
            assert torch.equal(u, v)


def test_calculate_mel_equals_the_batch_path_on_one_row():
    ds = DL.AudioDataset(DL.SyntheticDataset(2), DL.SimpleTokenizer(), device=DEV, n_mels=N_MELS, rate_aug=RATE, filter_aug={"p": 1.0, "kinds": ["low_shelf"]},
                         **STRETCH)
    clip = ds.hu_dataset[0]["audio"]["array"]
    audio = np.pad(clip, (0, 480000 - clip.shape[0]))
    random.seed(5)
    mel = ds._calculate_mel(audio, 4.0, True)
    random.seed(5)
    rate = ds._draw_stretch_rate()
    row, n_out = K.time_stretch(torch.from_numpy(audio).to(DEV)[None], [rate])
    sos = F.FilterAug(p=1.0, kinds=["low_shelf"]).draw()[2]
    table = RF.RateAug(16000, **RATE).draw()[1][None]
    row = K.alias(row, table[:, 1], n_out)
    row = K.sos_filter(row, sos[None], n_out)
    row = _pitch_replay(row, table, [int(round(480000 / rate))])
    want = K.logmel_ragged(row, n_out, torch.tensor([400], dtype=torch.int32, device=DEV), GF.mel_filters(N_MELS).to(DEV), 3000)[0]
    assert torch.equal(mel, want)
