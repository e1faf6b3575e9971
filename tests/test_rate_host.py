"""Per-row rate conversion, host side: the references and bounds of tests/_rate_cases.py against numpy and scipy and the proof that
they reject twelve defects, the pitch reference, the draws of data/rate_fx.py RateAug, the loader's items and the host checks of
K.sinc_resample_rows / K.alias / pitch_shift.  No GPU."""
import random

import numpy as np
import pytest
import torch

from tests import _rate_cases as R
from tests import _stretch_cases as SC
from whisper_finetune.data import data_loader as DL
from whisper_finetune.data import gpu_frontend as GF
from whisper_finetune.data import rate_fx as RF
from whisper_finetune.engine import kernels as K
from whisper_finetune.engine import lib as L

T_ALIAS = L.load().wft_alias_tile()  # pure host functions
tile = L.load().wft_sinc_resample_rows_tile
SR = 16000.0


# ------------------------------------------------------------------------------------------------------------ binding
def test_tiles_are_pure_host_functions():
    assert T_ALIAS >= 4 and T_ALIAS % 4 == 0
    assert tile(0.5) == 784 and tile(1.0) == 1024 and tile(2.0) == 1024 and tile(2.0 ** (-4 / 12)) == 1024
    assert tile(0.49) == 0 and tile(2.5) == 0 and tile(float("nan")) == 0 and tile(-1.0) == 0
    for lo in (0.5, 0.6, 0.7, 1.0):  # the input span of a tile at the lowest ratio, both halos included, fits the 1600-float staging buffer
        t = tile(lo)
        assert t >= 4 and t % 4 == 0 and (t - 1) / lo + 2 * R.REACH + 2 <= 1600


# ------------------------------------------------------------------------------------------------------------ alias
def _alias_cases():
    for n in R.HOST_ALIAS_NS:
        for name, s in R.alias_inputs(n, T_ALIAS, seed=n).items():
            for rate in R.alias_rates_for(n, SR):
                yield n, name, s, rate


def test_alias_emulation_is_bit_equal_to_numpy():
    """CPU test 1: the kernel's index rule, written in numpy, against np.interp(x, u, np.interp(u, x, s)) in float64, bit for bit."""
    total = 0
    seen_d = set()
    for n, name, s, rate in _alias_cases():
        want = R.alias_numpy(s, rate, SR)
        got = R.alias_emulation(s, rate, SR)
        assert np.array_equal(R.bits64(got), R.bits64(want)), (n, name, rate)
        seen_d.add((n, R.alias_d(n, rate, SR)))
        total += n
    assert total > 250000
    for n in R.HOST_ALIAS_NS:  # the issue's d for every n
        for d in (2, n - 1, n, n + 1):
            assert d < 2 or (n, d) in seen_d, (n, d)
    # Python's round is the kernel's rint: half to even, on the same two operations
    for n, rate in ((5, 1600.0), (5, 4800.0), (7, 16000.0 * 2.5 / 7)):
        assert R.alias_d(n, rate, SR) == round(n * float(rate) / SR)
    assert R.alias_d(5, 1600.0, SR) == 0 and R.alias_d(5, 4800.0, SR) == 2  # 0.5 -> 0, 1.5 -> 2


def test_alias_none_rows_and_the_identity_rate():
    s = R.signal(37, 3)
    for rate, n in ((0.0, 37), (100.0, 37), (8000.0, 1)):  # rate 0, d < 2, n < 2
        assert np.array_equal(R.bits64(R.alias_emulation(s[:n], rate, SR)), R.bits64(s[:n].astype(np.float64)))
    assert np.array_equal(R.alias_numpy(s, SR, SR), s.astype(np.float64))  # d == n: every point is a grid hit, a copy
    assert not np.array_equal(R.alias_numpy(s, 8000.0, SR), s.astype(np.float64))


def test_alias_emulation_is_bit_equal_to_numpy_at_the_loaders_lengths():
    """The same proof on the rows the loader aliases: 480 000 samples, one less, and the ends of the default stretch range."""
    for n in R.LOADER_ALIAS_NS:
        s = R.signal(n, seed=n % 1000)
        for rate in (8000.0, 11025.0, 15999.0, 16000.0, 1.9 * SR, (n // 2 + 0.75) * SR / n):
            assert np.array_equal(R.bits64(R.alias_emulation(s, rate, SR)), R.bits64(R.alias_numpy(s, rate, SR))), (n, rate)


@pytest.mark.parametrize("mutant", R.ALIAS_MUTANTS)
def test_alias_comparison_rejects(mutant):
    """CPU test 5, alias: d from truncation; the last grid point as (num - 1) * step; the grid_j == t shortcut left out (a -0.0 sample
    at a grid hit comes out as +0.0); slope and offset fused into one fma; j off by one at a grid hit."""
    caught = 0
    for n, name, s, rate in _alias_cases():
        want = R.alias_numpy(s, rate, SR)
        got = R.alias_emulation(s, rate, SR, mutant)
        caught += int(got.shape != want.shape or not np.array_equal(R.bits64(got), R.bits64(want)))
    assert caught >= 3, (mutant, caught)


# ------------------------------------------------------------------------------------------------------------ sinc
def _g(t, c):
    a = c * np.asarray(t, dtype=np.float64)
    return np.where(np.abs(a) < 6.0, c * np.sinc(a) * np.cos(np.pi * a / 12.0) ** 2, 0.0)


@pytest.mark.parametrize("up,down", [(1, 2), (2, 1)])
def test_the_sinc_reference_agrees_with_scipy_resample_poly(up, down):
    """CPU test 2: at rho = up / down the definition is the polyphase resampler with the prototype H[i] = g(i / up)."""
    signal = pytest.importorskip("scipy.signal")
    rho = up / down
    c = 0.99 * min(1.0, rho)
    half = int(np.ceil(6.0 / c)) * up
    H = _g(np.arange(-half, half + 1, dtype=np.float64) / up, c)
    for n_in in (1, 2, 13, 100, 1025):
        x = R.signal(n_in, seed=n_in).astype(np.float64)
        want = signal.resample_poly(x, up, down, window=H / up)
        got, _ = R.sinc_ref(x, n_in, rho, len(want))
        assert len(want) == int(np.ceil(n_in * rho))
        assert np.abs(got - want).max() <= 1e-12, (rho, n_in, np.abs(got - want).max())


def test_the_sinc_reference_is_the_existing_resampler_at_a_rational_ratio():
    """At rho = n / o the weight is the g((j / o - m / n) * base) of wft_resample_f32 (tests/_resample_cases.py)."""
    from tests import _resample_cases as RC

    for orig, new in ((3, 2), (2, 3), (441, 320)):
        x = R.signal(700, seed=orig).astype(np.float64)
        want = RC.definition(x, orig, new)
        got, _ = R.sinc_ref(x, 700, new / orig, len(want))
        assert np.abs(got - want).max() <= 1e-12, (orig, new)


def test_sinc_rows_fix_length_and_bad_ratios():
    x = R.signal(50, 1)
    rho = R.RHOS[4]
    full, _ = R.sinc_ref(x, 50, rho, 80)
    edge = int(np.ceil(50 * rho))
    assert edge == 63 and full[edge - 1] != 0.0 and not full[edge:].any()       # zero from ceil(N rho)
    short, _ = R.sinc_ref(x, 50, rho, 40)
    assert np.array_equal(short, full[:40])                                        # n_out below it: a prefix
    assert not R.sinc_ref(x, 0, rho, 9)[0].any() and not R.sinc_ref(x, -1, rho, 9)[0].any()
    for bad in (0.49, 2.01, float("nan")):
        assert not R.sinc_ref(x, 50, bad, 9)[0].any()
    one, _ = R.sinc_ref(np.ones(400), 400, 1.0, 400)                               # rho == 1: a low-pass, not a copy
    assert abs(one[200] - 1.0) < 1e-2 and one[200] != 1.0
    assert max(int(np.count_nonzero(np.abs(0.99 * 0.5 * (np.arange(-14, 15) - f)) < 6.0)) for f in np.linspace(0, 0.999, 50)) == 25


def _sinc_cases():
    for lo in (0.5, None):
        for rows, n_out in R.sinc_batches(tile(0.5) if lo else tile(1.0), R.RHOS if lo else R.RHOS[3:]):
            for N, rho in rows:
                for name, x in R.sinc_probe_rows(N, rho, tile(0.5) if lo else tile(1.0), seed=N).items():
                    yield N, rho, n_out, name, x


def test_sinc_bound_accepts_the_rounded_reference_and_eps_is_small():
    assert R.EPS <= 2.0 ** -30
    for N, rho, n_out, name, x in _sinc_cases():
        ref, mag = R.sinc_ref(x, N, rho, n_out)
        bad, frac, off = R.sinc_violations(ref.astype(np.float32), ref, mag)
        assert bad == 0 and frac <= 1.0 and off == 0.0, (N, rho, name)


@pytest.mark.parametrize("mutant", R.SINC_MUTANTS)
def test_sinc_comparison_rejects(mutant):
    """CPU test 5, sinc: a tap dropped at either edge of the window; c taken as 0.99 rho for rho > 1; the window's argument without
    c; t0 formed in f32; n_in off by one at the row end; fix_length zeroing from floor instead of ceil(N rho)."""
    caught = cases = 0
    for N, rho, n_out, name, x in _sinc_cases():
        ref, mag = R.sinc_ref(x, N, rho, n_out)
        got = R.sinc_ref(x, N, rho, n_out, mutant)[0].astype(np.float32)
        caught += int(R.sinc_violations(got, ref, mag)[0] > 0)
        cases += 1
    assert caught >= 5, (mutant, caught, cases)


# ------------------------------------------------------------------------------------------------------------ pitch
def pitch_ref(y, semitones, invert=False):
    """tests/_stretch_cases' vocoder by 2^(-s/12) followed by the sinc reference at the same ratio, back to len(y)."""
    rate = 2.0 ** (-semitones / 12.0)
    st = SC.time_stretch(np.asarray(y, dtype=np.float64), rate)
    return R.sinc_ref(st, len(st), 1.0 / rate if invert else rate, len(y))[0]


peak_hz = R.peak_hz


@pytest.mark.parametrize("semitones", [12.0, 4.0, -4.0])
def test_pitch_reference_moves_a_sine(semitones):
    """CPU test 3: 440 Hz over 16 000 samples (one FFT bin = 1 Hz) lands within one bin of 440 * 2^(s/12); an inverted ratio does not."""
    y = np.sin(2 * np.pi * 440.0 * np.arange(16000) / 16000.0)
    want = 440.0 * 2.0 ** (semitones / 12.0)
    out = pitch_ref(y, semitones)
    assert out.shape == (16000,) and abs(peak_hz(out) - want) <= 1.0, (semitones, peak_hz(out), want)
    assert abs(peak_hz(pitch_ref(y, semitones, invert=True)) - want) > 1.0
    assert np.array_equal(GF.pitch_rates(semitones, 1), [min(max(2.0 ** (-semitones / 12.0), 0.5), 2.0)])


# ------------------------------------------------------------------------------------------------------------ draws
def test_draws_follow_the_documented_order_and_bounds():
    aug = RF.RateAug(16000, alias={"p": 1.0}, pitch={"p": 1.0})
    random.seed(9)
    names, row = aug.draw()
    random.seed(9)
    assert random.random() < 1.0
    f = RF.mel_to_hz(random.uniform(RF.hz_to_mel(8000.0), RF.hz_to_mel(16000.0)))
    assert random.random() < 1.0
    s = random.uniform(-4.0, 4.0)
    assert names == {"alias": True, "pitch": True} and np.array_equal(row, [1.0, min(max(f, 8000.0), 16000.0), 1.0, s])
    assert row.dtype == np.float64 and row.shape == (RF.TABLE_WIDTH,) == (4,)
    # mel-uniform: inside the bounds, and the median is the mel midpoint, not the arithmetic one
    aug = RF.RateAug(16000, alias={"p": 1.0, "min_sample_rate": 2000, "max_sample_rate": 16000})
    random.seed(1)
    rates = np.array([aug.draw()[1][1] for _ in range(4000)])
    mid = RF.mel_to_hz(0.5 * (RF.hz_to_mel(2000.0) + RF.hz_to_mel(16000.0)))
    assert rates.min() >= 2000.0 and rates.max() <= 16000.0 and abs(np.median(rates) - mid) < 300.0 and mid < 8000.0
    assert RF.hz_to_mel(700.0) == pytest.approx(2595 * np.log10(2.0)) and RF.mel_to_hz(RF.hz_to_mel(1234.5)) == pytest.approx(1234.5)
    aug = RF.RateAug(16000, pitch={"p": 1.0, "min_semitones": -12, "max_semitones": 12})
    semis = np.array([aug.draw()[1][3] for _ in range(2000)])
    assert semis.min() >= -12.0 and semis.max() <= 12.0 and semis.min() < -10.0 and semis.max() > 10.0
    RF.check_table(np.stack([aug.draw()[1] for _ in range(8)]))


def test_default_gates_are_the_marginal_rates():
    assert RF.DEFAULT_P == {"alias": pytest.approx(0.075), "pitch": pytest.approx(0.0375)}
    aug = RF.RateAug(16000, alias={}, pitch={})
    assert aug.alias_range == (8000.0, 16000.0) and aug.pitch_range == (-4.0, 4.0)
    random.seed(3)
    n = 40000
    hits = np.array([[v for v in aug.draw()[0].values()] for _ in range(n)], dtype=np.float64).mean(0)
    assert abs(hits[0] - 0.075) < 4 * np.sqrt(0.075 * 0.925 / n) and abs(hits[1] - 0.0375) < 4 * np.sqrt(0.0375 * 0.9625 / n)
    off = RF.RateAug(16000)
    state = random.getstate()
    assert off.draw()[0] == {"alias": False, "pitch": False} and random.getstate() == state  # a group that is off draws nothing
    assert np.array_equal(off.draw()[1], RF.none_table())
    failed = RF.RateAug(16000, alias={"p": 0.0}, pitch={"p": 0.0})
    random.seed(4)
    failed.draw()
    after = random.random()
    random.seed(4)
    random.random(); random.random()  # one gate draw per group and nothing else
    assert after == random.random()


def test_every_refusal_of_the_option():
    for bad in (dict(alias=True), dict(alias={"rate": 1}), dict(alias={"p": 1.5}), dict(alias={"p": True}), dict(pitch={"p": -0.1}),
                dict(alias={"max_sample_rate": 30000}), dict(alias={"min_sample_rate": 999}), dict(alias={"min_sample_rate": 12000, "max_sample_rate": 9000}),
                dict(alias={"min_sample_rate": float("nan")}), dict(pitch={"min_semitones": -13}), dict(pitch={"max_semitones": 12.5}),
                dict(pitch={"min_semitones": 3, "max_semitones": 2}), dict(pitch={"min_semitones": "low"}), dict(pitch=[-4, 4])):
        with pytest.raises(ValueError):
            RF.RateAug(16000, **bad)
    for bad_sr in (0, 16000.0, True, 999):
        with pytest.raises(ValueError):
            RF.RateAug(bad_sr)
    good = np.array([[1.0, 9000.0, 1.0, -3.0], [0.0, 0.0, 0.0, 0.0]])
    assert RF.check_table(good) is not None and RF.check_table(torch.from_numpy(good)).shape == (2, 4)
    for r, c, v in ((0, 0, 2.0), (0, 1, 999.0), (0, 1, 16000.5), (1, 1, 8000.0), (0, 3, 12.5), (0, 3, float("nan")), (1, 3, 1.0), (0, 2, 0.5)):
        t = good.copy()
        t[r, c] = v
        with pytest.raises(ValueError):
            RF.check_table(t)
    for t in (good.astype(np.float32), good[0], good[:, :3]):
        with pytest.raises(ValueError):
            RF.check_table(t)


# ------------------------------------------------------------------------------------------------------------ dataset and loader
def _dataset(**kw):
    return DL.AudioDataset(DL.SyntheticDataset(4, min_seconds=1.0), DL.SimpleTokenizer(), no_timestamp_training=True, spec_augment=True,
                           spec_augment_params={"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 0.5},
                           extremes_spec_augment=True, extremes_spec_augment_params={"low_freq_range": 5, "high_freq_range": 5}, **kw)


BOTH = {"alias": {"p": 1.0}, "pitch": {"p": 1.0}}
WAVE = {"noise": {"p": 1.0}, "clip": {"p": 1.0}, "level": {"p": 1.0}}


@pytest.mark.parametrize("stretch,filt,wave", [(False, False, False), (True, False, False), (False, True, True), (True, True, True)])
def test_items_gain_exactly_one_field_behind_the_wave_effects_and_earlier_draws_are_untouched(stretch, filt, wave):
    kw = dict(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25) if stretch else {}
    if filt:
        kw["filter_aug"] = {"p": 1.0}
    if wave:
        kw["wave_aug"] = WAVE
    on, off = _dataset(rate_aug=BOTH, **kw), _dataset(**kw)
    base = 6 + int(stretch) + int(filt) + int(wave)
    a, b = [], []
    for i in range(4):
        torch.manual_seed(7 + i); random.seed(40 + i)
        a.append(on[i])
        after_on = torch.rand(1)
        torch.manual_seed(7 + i); random.seed(40 + i)
        b.append(off[i])
        assert torch.equal(after_on, torch.rand(1))
    for x, y in zip(a, b):
        assert len(x) == base + 1 and len(y) == base
        for u, v in zip(x[:base], y):  # everything shipped before is drawn BEFORE the rate effects: identical
            assert torch.equal(torch.as_tensor(u), torch.as_tensor(v))
        assert x[-1].dtype == torch.float64 and x[-1].shape == (RF.TABLE_WIDTH,)
    ca, cb = DL.collate_fn(a), DL.collate_fn(b)
    assert len(ca) == base + 1 and len(cb) == base and ca[-1].dtype == torch.float64 and ca[-1].shape == (4, RF.TABLE_WIDTH)
    for u, v in zip(ca[:base], cb):
        assert torch.equal(u, v)
    assert bool(RF.check_table(ca[-1])[:, [0, 2]].all())


def test_item_row_is_the_draw_after_the_wave_effects():
    ds = _dataset(wave_aug={"level": {"p": 1.0, "kinds": ["gain"]}}, rate_aug=BOTH)
    random.seed(77)
    item = ds[0]
    random.seed(77)
    from whisper_finetune.data import wave_fx as WF

    WF.WaveAug(level={"p": 1.0, "kinds": ["gain"]}).draw(DL.N_SAMPLES)
    names, row = RF.RateAug(16000, **BOTH).draw()
    assert all(names.values()) and np.array_equal(item[-1].numpy(), row) and len(item) == 8


def test_option_is_checked_and_the_other_pipelines_stay_refused():
    with pytest.raises(NotImplementedError, match="apply_advanced_aug"):
        _dataset(apply_advanced_aug=True, rate_aug={})
    with pytest.raises(NotImplementedError, match="apply_office_aug"):
        _dataset(apply_office_aug=True, rate_aug=BOTH)
    msgs = []
    for kw in ({}, {"rate_aug": BOTH}):
        with pytest.raises(NotImplementedError) as e:
            _dataset(apply_advanced_aug=True, **kw)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]  # the same message as without the option
    for bad in (True, {"gain": {}}, {"alias": {"p": 2.0}}, {"alias": {"max_sample_rate": 30000}}, {"pitch": {"max_semitones": 13}}):
        with pytest.raises(ValueError):
            _dataset(rate_aug=bad)
    assert _dataset().rate_aug is None and _dataset(rate_aug={}).rate_aug.p == {}


def test_gpu_mel_loader_reads_the_fields_from_the_flags():
    class FakeFrontend:
        device = torch.device("cpu")

    def loader(**kw):
        return DL.GpuMelLoader(torch.utils.data.DataLoader(_dataset(**kw), batch_size=2, collate_fn=DL.collate_fn), FakeFrontend(), True)

    st, fl, wv = dict(apply_baseline_aug=True), dict(filter_aug={"p": 1.0, "kinds": ["high_pass"]}), dict(wave_aug=WAVE)
    for kw, fields in (({}, (False, False, False)), (st, (True, False, False)), ({**fl, **wv}, (False, True, True)), ({**st, **fl, **wv}, (True, True, True))):
        ld = loader(rate_aug=BOTH, **kw)
        batch = next(iter(ld.loader))
        rates, sos, fx, rt = ld._all_fields(batch)
        assert (rates is not None, sos is not None, fx is not None) == fields and len(batch) == 7 + sum(fields)
        assert rt.dtype == np.float64 and rt.shape == (2, 4) and bool(rt[:, [0, 2]].all())
        assert ld._fields(batch)[0] is rates and len(ld._fields(batch)) == 3
    ld = loader(rate_aug={"alias": {"p": 0.0}, "pitch": {"p": 0.0}})
    assert ld._all_fields(next(iter(ld.loader))) == (None, None, None, None)  # nothing drawn: nothing to launch
    with pytest.raises(ValueError):
        loader(rate_aug=BOTH)._all_fields(next(iter(loader().loader)))
    assert loader().rate_aug is False and loader()._all_fields(next(iter(loader().loader))) == (None, None, None, None)
    assert DL.stretched_lengths(480000, [0.75, 1.25, 0.8000000001]) == [640000, 384000, round(480000 / 0.8000000001)]


def test_debug_config_carries_the_option_and_its_block_builds():
    from pathlib import Path

    import yaml

    cfg = yaml.safe_load((Path(__file__).resolve().parents[1] / "configs" / "DEBUG_synthetic_rate.yaml").read_text())
    aa = cfg["augmentation"]["audio_augment"]
    assert aa["apply_advanced_aug"] is False and aa["apply_office_aug"] is False and set(aa["wft_rate_aug"]) == set(RF.STAGES)
    ds = _dataset(rate_aug=aa["wft_rate_aug"], wave_aug=aa["wft_wave_aug"], filter_aug=aa["wft_filter_aug"])
    assert ds.rate_aug.p == {"alias": 0.5, "pitch": 0.5} and ds.rate_aug.alias_range == (8000.0, 16000.0) and ds.rate_aug.pitch_range == (-4.0, 4.0)


# ------------------------------------------------------------------------------------------------------------ host checks
def test_wrappers_raise_before_the_device_is_touched():
    x = torch.zeros(2, 64)  # a host tensor: reaching the device would raise something else than ValueError
    n = torch.full((2,), 64, dtype=torch.int32)
    for bad_audio in (x.double(), x[0], torch.zeros(0, 4), np.zeros((2, 4), dtype=np.float32)):
        with pytest.raises(ValueError):
            K.sinc_resample_rows(bad_audio, n, 1.0, 64)
        with pytest.raises(ValueError):
            K.alias(bad_audio, 8000.0)
    for ratios in (0.49, 2.01, float("nan"), [1.0, 1.0, 1.0], "fast", [1.0, 0.3]):
        with pytest.raises(ValueError):
            K.sinc_resample_rows(x, n, ratios, 64)
    for n_out in (0, -1, 64.0, True, (1 << 30) + 1):
        with pytest.raises(ValueError):
            K.sinc_resample_rows(x, n, 1.0, n_out)
    for bad_n in (None, n.long(), n[:1], [64, 64]):
        with pytest.raises(ValueError):
            K.sinc_resample_rows(x, bad_n, 1.0, 64)
    for rates in (999.0, 32000.5, -8000.0, float("nan"), [8000.0] * 3, "low", [8000.0, 500.0]):
        with pytest.raises(ValueError):
            K.alias(x, rates)
    with pytest.raises(ValueError):
        K.alias(x, 8000.0, n.long())
    for sr in (0, 999, True, "16k", 400000):
        with pytest.raises(ValueError):
            K.alias(x, 8000.0, None, sr)
    assert np.array_equal(K.alias_rates([0.0, 32000.0], 2, 16000.0), [0.0, 32000.0])  # 0 = none; 2 * sample_rate is the top
    for s in (12.5, -12.01, float("nan"), [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            GF.pitch_shift(np.zeros((2, 16), dtype=np.float32), s)
    with pytest.raises(ValueError):
        GF.pitch_shift(np.zeros(16, dtype=np.float64), 1.0)
    with pytest.raises(ValueError):
        GF.alias(np.zeros(16, dtype=np.float32), 500.0)
    with pytest.raises(ValueError):
        GF.alias(np.zeros((0, 4), dtype=np.float32), 8000.0)
    r = GF.pitch_rates([12.0, -12.0, 0.0], 3)
    assert r[0] == 0.5 and r[1] == 2.0 and r[2] == 1.0
