"""Wave effects, host side: the references and bounds of tests/_wavefx_cases.py and the proof that they reject fourteen defects, the
draws of data/wave_fx.py WaveAug, the records, the loader's items and the host checks of K.wave_fx.  No GPU."""
import random

import numpy as np
import pytest
import torch

from tests import _wavefx_cases as W
from whisper_finetune.data import data_loader as DL
from whisper_finetune.data import gpu_frontend as GF
from whisper_finetune.data import wave_fx as WF
from whisper_finetune.engine import kernels as K
from whisper_finetune.engine import lib as L

T = L.load().wft_wave_fx_tile()  # a pure host function
NS, N_MAX, LD = W.layout(T)
CASES = W.stage_cases(T)


def _expected(name, mut=None):
    stage, kind, fill = CASES[name]
    buf = W.case_input(NS, N_MAX, LD, name, kind)
    rec = fill(W.records(len(NS)))
    return W.expected_buffer(buf, NS, N_MAX, rec, stage, mut)


# ------------------------------------------------------------------------------------------------------------ binding and records
def test_tile_workspace_and_struct():
    import ctypes

    assert T >= 4 and T % 4 == 0
    q = L.load().wft_wave_fx_workspace_bytes
    assert q(0, 100, 0) == -1 and q(1, 0, 0) == -1 and q(1, 100, 3) == -1 and q(1, 100, -1) == -1 and q(1, (1 << 30) + 1, 1) == -1
    assert q(65536, 100, 0) == -1
    assert all(q(3, 5000, s) >= 8 and q(3, 5000, s) % 8 == 0 for s in (0, 1, 2))
    assert ctypes.sizeof(L.WaveFx) == WF.RECORD_DTYPE.itemsize == 88
    for name, _ in L.WaveFx._fields_:
        assert getattr(L.WaveFx, name).offset == WF.RECORD_DTYPE.fields[name][1], name
    assert (L.FX_NOISE, L.FX_CLIP, L.FX_LEVEL) == tuple(WF.STAGE_ID[s] for s in WF.STAGES)
    assert WF.KIND_ID["shift"] == L.FX_SHIFT and WF.KIND_ID["gaussian_snr"] == L.FX_GAUSSIAN_SNR


def test_philox_known_answers():
    a, b = W.philox_known_answers()
    assert a == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8] and b == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_normals_are_standard_normal_and_never_infinite():
    z, r = W.normals(0xDEADBEEFCAFEF00D, np.arange(200000))
    assert np.all(np.isfinite(z)) and r.max() <= np.sqrt(2 * 24 * np.log(2.0)) + 1e-12
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and abs(np.mean(z[0::2] * z[1::2])) < 0.01
    # a pair (even, odd) shares r and the angle: z_e^2 + z_o^2 = r^2
    assert np.allclose(z[0::2] ** 2 + z[1::2] ** 2, r[0::2] ** 2, rtol=1e-12)


def test_collated_table_round_trips_the_seed_and_every_field():
    rows = [WF.table_row("gaussian_snr", snr_db=12.5, seed=0xFEDCBA9876543210), WF.table_row("gaussian_noise", amplitude=0.01, seed=(1 << 64) - 1),
            WF.table_row("gain_transition", start_db=-3.0, end_db=2.0, t0=-123456789, length=96000), WF.table_row("shift", fraction=-0.37, fade_len=80),
            WF.table_row("clipping", q=17), WF.table_row("gain", gain_db=-4.5), WF.table_row()]
    table = torch.stack([torch.from_numpy(r) for r in rows])  # what collate_fn does
    assert table.dtype == torch.float64 and table.shape == (7, WF.TABLE_WIDTH)
    rec = WF.check_records(WF.records_from_table(table))
    assert int(rec["seed"][0]) == 0xFEDCBA9876543210 and int(rec["seed"][1]) == (1 << 64) - 1
    assert int(rec["t0"][2]) == -123456789 and int(rec["ramp_len"][2]) == 96000 and int(rec["fade_len"][3]) == 80
    assert int(rec["clip_q"][4]) == 17 and rec["gain_ratio"][5] == np.float32(10.0 ** (-4.5 / 20.0))
    assert np.array_equal(WF.table_from_records(rec), table.numpy())
    assert not any(WF.active_rows(rec, s)[6] for s in WF.STAGES)
    assert [bool(WF.active_rows(rec, "level")[i]) for i in range(7)] == [False, False, True, True, False, True, False]
    # the kernel-side form is the struct, byte for byte
    raw = rec.view("u1").reshape(7, 88)
    one = L.WaveFx.from_buffer_copy(raw[2].tobytes())
    assert (one.level_kind, one.t0, one.ramp_len, one.db_start, one.db_end) == (L.FX_GAIN_TRANSITION, -123456789, 96000, -3.0, 2.0)


def test_records_refuse_what_only_the_device_would_see():
    def bad(kind, field, value):
        rec = WF.records_from_table(WF.table_row(kind, **GOOD[kind])[None])
        rec[field][0] = value
        with pytest.raises(ValueError):
            WF.check_records(rec)

    GOOD = {"gaussian_noise": dict(amplitude=0.01, seed=1), "gaussian_snr": dict(snr_db=10.0, seed=1), "clipping": dict(q=5), "gain": dict(gain_db=1.0),
            "gain_transition": dict(start_db=0.0, end_db=1.0, t0=0, length=10), "shift": dict(fraction=0.1, fade_len=3)}
    bad("clipping", "clip_q", 51)
    bad("clipping", "clip_q", -1)
    bad("gaussian_noise", "noise_value", np.inf)
    bad("gaussian_noise", "noise_value", -0.5)
    bad("gaussian_snr", "noise_value", np.nan)
    bad("gain", "gain_ratio", np.inf)
    bad("gain_transition", "db_end", np.nan)
    bad("gain_transition", "ramp_len", 0)
    bad("gain_transition", "t0", 1 << 41)
    bad("shift", "shift_fraction", 1.5)
    bad("shift", "shift_fraction", np.nan)
    bad("shift", "fade_len", -1)
    bad("gain", "level_kind", 4)
    bad("clipping", "clip_kind", 2)
    for kw in (dict(kind="clipping", q=2.5), dict(kind="gaussian_noise", amplitude=0.1, seed=1 << 64), dict(kind="gain", db=1.0), dict(kind="echo")):
        with pytest.raises(ValueError):
            WF.table_row(**kw)
    t = WF.none_table(2)
    t[1, 2] = 0.5  # half a seed
    with pytest.raises(ValueError):
        WF.records_from_table(t)
    with pytest.raises(ValueError):
        WF.records_from_table(t[:, :5])


# ------------------------------------------------------------------------------------------------------------ references
def test_percentile_restatement_equals_numpy_linear():
    g = np.random.default_rng(3)
    for n in (1, 2, 3, 17, 100, 101, 1023, 4097):
        for kind in ("speech", "negative", "sawtooth", "equal", "denormals"):
            x = W.signal(n, n, kind)
            if kind == "denormals":
                x = np.where(x == 0, np.float32(2.0 ** -140), x)  # without signed zeros
            for q in (0, 1, 7, 20, 25, 50):
                lo, hi = W.thresholds(x, q)
                want = np.percentile(x.astype(np.float64), [q, 100 - q], method="linear")
                assert abs(float(lo) - want[0]) <= W.half_ulp32(want[0]) + 4 * W.U * abs(want[0]), (n, kind, q)
                assert abs(float(hi) - want[1]) <= W.half_ulp32(want[1]) + 4 * W.U * abs(want[1]), (n, kind, q)
                assert np.array_equal(np.where(x < lo, lo, np.where(x > hi, hi, x)), np.clip(x, lo, hi))
    del g


def test_key_order_is_total_and_puts_minus_zero_first():
    x = np.array([0.0, -0.0, 1e-45, -1e-45, -np.inf, np.inf, 1.5, -1.5], dtype=np.float32)
    s = W.unkey(np.sort(W.okey(x)))
    assert np.array_equal(W.bits(s), W.bits(np.array([-np.inf, -1.5, -1e-45, -0.0, 0.0, 1e-45, 1.5, np.inf], dtype=np.float32)))
    lo, hi = W.thresholds(np.array([0.0, -0.0, -0.0, 0.0], dtype=np.float32), 0)
    assert np.signbit(lo) and not np.signbit(hi)


def test_exact_rank_cases_are_in_the_table():
    """g = 0 with j + 1 == n (the upper percentile of q = 0 sits on the last sample) and both percentiles on one sample."""
    for b, n in enumerate(NS):
        if n >= 1:
            assert (100 * (n - 1)) % 100 == 0 and (100 * (n - 1)) // 100 + 1 == n
    exps = _expected("clip_sawtooth_q50")
    for b, n in enumerate(NS):
        if n >= 1 and (n - 1) % 2 == 0:
            assert W.bits(exps[b].thr[0])[0] == W.bits(exps[b].thr[1])[0]


def test_shift_definition_end_points():
    n, s, F = 40, 12, 5
    row = np.arange(1, n + 1, dtype=np.float32)
    rec = WF.records_from_table(WF.table_row("shift", fraction=s / n, fade_len=F)[None])[0]
    e = W.ref_level(row, n, rec, n)
    w = e.val / row[(np.arange(n) - s) % n]
    assert w[s] == 0.0 and w[s + F - 1] == 1.0 and w[s - 1] == 0.0 and w[s - F] == 1.0 and w[s + 1] == 0.25 and w[s - 2] == 0.25
    assert np.all(w[s + F:] == 1.0) and np.all(w[:s - F] == 1.0) and e.exact.sum() == n - 2 * F
    assert e.val[s] == 0.0 and e.val[s + F] == row[F]  # x[0] lands on output index s
    # ties to even, the clamp of F, and s == 0 as a copy
    assert W.shift_places(0.5, 5) == 2 and W.shift_places(0.5, 7) == 4 and W.shift_places(-0.5, 5) == 3 and W.shift_places(1.0, 9) == 0
    big = WF.records_from_table(WF.table_row("shift", fraction=0.5, fade_len=10 ** 6)[None])[0]
    assert (~W.ref_level(row, n, big, n).exact).sum() == 2 * (n // 2)
    zero = WF.records_from_table(WF.table_row("shift", fraction=0.0, fade_len=8)[None])[0]
    z = W.ref_level(row, n, zero, n)
    assert z.exact.all() and np.array_equal(z.val, row.astype(np.float64))


def test_transition_holds_its_levels_outside_the_ramp():
    n = 50
    row = np.ones(n, dtype=np.float32)
    rec = WF.records_from_table(WF.table_row("gain_transition", start_db=-20.0, end_db=20.0, t0=10, length=21)[None])[0]
    v = W.ref_level(row, n, rec, n).val
    assert np.allclose(v[:11], 0.1) and np.allclose(v[30:], 10.0) and np.isclose(v[20], 1.0)
    assert np.allclose(np.diff(np.log10(v[10:31])), 0.1)  # linear in dB


def test_every_reference_passes_its_own_comparison():
    for name in CASES:
        for b, e in enumerate(_expected(name)):
            assert W.violations(e.val.astype(np.float32), e) == 0, (name, b)


@pytest.mark.parametrize("mut", W.MUTANTS)
def test_the_comparison_rejects_the_mutant(mut):
    """The reference with ONE defect, rounded to f32 as a kernel would, must be rejected by `violations` on the GPU test's own cases."""
    stage = W.MUTANT_STAGE[mut]
    rejected = []
    for name, (st, _, _) in CASES.items():
        if stage not in ("any", st):
            continue
        good = _expected(name)
        with np.errstate(all="ignore"):
            mutant = _expected(name, mut)
        bad = sum(W.violations(m.val.astype(np.float32), g) for m, g in zip(mutant, good))
        if mut in ("percentile_uses_n", "j_off_by_one", "upper_percent_minus_1", "lo_hi_swapped"):
            bad += sum(int(W.bits(m.thr[k])[0] != W.bits(g.thr[k])[0]) for m, g in zip(mutant, good) if g.thr is not None for k in (0, 1))
        if bad:
            rejected.append(name)
    assert rejected, mut
    need = {"rms_drops_last": "gaussian_snr", "rms_reads_past_n": "gaussian_snr", "snr_inverted": "gaussian_snr", "counter_shift_1": "gaussian_noise",
            "cos_sin_swapped": "gaussian_noise", "seed_halves_swapped": "gaussian_noise", "percentile_uses_n": "clip_sawtooth_q20",
            "j_off_by_one": "clip_sawtooth_q20", "upper_percent_minus_1": "clip_sawtooth_q20", "lo_hi_swapped": "clip_sawtooth_q20",
            "transition_linear_amplitude": "transition_inside", "shift_sign_flipped": "shift_fade", "fade_one_short": "shift_fade",
            "no_zero_fill": "gain"}[mut]
    assert need in rejected, (mut, rejected)


# ------------------------------------------------------------------------------------------------------------ draws
def test_draw_order_and_ranges_under_a_seeded_random():
    aug = WF.WaveAug(noise={"p": 1.0}, clip={"p": 1.0, "kinds": {"clipping": {"p": 1.0}}}, level={"p": 1.0, "kinds": {"shift": {"p": 1.0}, "gain": {},
                                                                                                            "gain_transition": {}}})
    seen = set()
    for trial in range(60):
        random.seed(trial)
        names, row = aug.draw(480000)
        random.seed(trial)
        rec = WF.records_from_table(row[None])[0]
        # noise: gate, kind, inner gate, value, seed
        assert random.random() < 1.0
        kind = WF.KINDS["noise"][random.randrange(2)]
        assert random.random() < 1.0 and names["noise"] == kind
        value = random.uniform(0.001, 0.015) if kind == "gaussian_noise" else random.uniform(5.0, 40.0)
        assert float(rec["noise_value"]) == value and int(rec["seed"]) == random.getrandbits(64)
        # clip
        assert random.random() < 1.0 and random.randrange(1) == 0 and random.random() < 1.0
        thr = random.randint(0, 40)
        assert int(rec["clip_q"]) == thr // 2 and 0 <= int(rec["clip_q"]) <= 20 and names["clip"] == "clipping"
        # level
        assert random.random() < 1.0
        kind = WF.KINDS["level"][random.randrange(3)]
        assert random.random() < 1.0 and names["level"] == kind
        if kind == "gain":
            assert rec["gain_ratio"] == np.float32(10.0 ** (random.uniform(-6.0, 6.0) / 20.0))
        elif kind == "gain_transition":
            a, b = random.uniform(-24.0, 6.0), random.uniform(-24.0, 6.0)
            length = max(int(random.uniform(0.2, 6.0) * 16000), 1)
            t0 = random.randint(2 - length, 480000 - 2)
            assert (float(rec["db_start"]), float(rec["db_end"]), int(rec["ramp_len"]), int(rec["t0"])) == (a, b, length, t0)
            assert 3200 <= length <= 96000 and t0 + length - 1 >= 1 and t0 <= 480000 - 2  # the ramp overlaps the clip
        else:
            assert float(rec["shift_fraction"]) == random.uniform(-0.5, 0.5) and int(rec["fade_len"]) == 80
        seen.update(names.values())
        WF.check_records(WF.records_from_table(row[None]))
    assert seen == {"gaussian_noise", "gaussian_snr", "clipping", "gain", "gain_transition", "shift"}


def test_failed_gates_draw_nothing_more():
    random.seed(9)
    aug = WF.WaveAug(noise={"p": 0.0}, clip={"p": 1.0, "kinds": {"clipping": {"p": 0.0}}})
    names, row = aug.draw()
    random.seed(9)
    random.random()                       # the noise gate fails: nothing else
    random.random(); random.randrange(1); random.random()   # clip: gate, kind, inner gate fails
    nxt = random.random()
    assert names == {"noise": None, "clip": None, "level": None} and np.array_equal(row, WF.none_table())
    random.seed(9)
    aug.draw()
    assert random.random() == nxt


def test_default_gates_are_the_marginal_rates():
    assert WF.DEFAULT_P == pytest.approx({"noise": 0.3 * 2 / 4, "clip": 0.6 / 9, "level": 0.3 * 3 / 4}, rel=1e-15)
    aug = WF.WaveAug(noise={}, clip={}, level={})
    assert aug.p == WF.DEFAULT_P and aug.kinds == WF.KINDS
    assert aug.ranges["clipping"]["p"] == 0.8 and aug.ranges["shift"]["p"] == 0.5 and aug.ranges["gain"]["p"] == 1.0
    off = WF.WaveAug()
    assert off.draw()[0] == {"noise": None, "clip": None, "level": None}


@pytest.mark.parametrize("kw", [
    dict(noise={"p": 1.5}), dict(noise={"q": 1.0}), dict(noise=True), dict(noise={"kinds": []}), dict(noise={"kinds": ["gain"]}),
    dict(noise={"kinds": {"gaussian_noise": {"min_amplitude": -0.1}}}), dict(noise={"kinds": {"gaussian_noise": {"min_amplitude": 0.2, "max_amplitude": 0.1}}}),
    dict(noise={"kinds": {"gaussian_snr": {"max_snr_db": float("inf")}}}), dict(noise={"kinds": {"gaussian_snr": {"snr": 3}}}),
    dict(clip={"kinds": {"clipping": {"max_percentile_threshold": 101}}}), dict(clip={"kinds": {"clipping": {"min_percentile_threshold": 2.5}}}),
    dict(clip={"kinds": {"clipping": {"min_percentile_threshold": 30, "max_percentile_threshold": 20}}}), dict(clip={"kinds": {"clipping": {"p": -0.1}}}),
    dict(level={"kinds": {"gain": {"min_gain_db": 7.0}}}), dict(level={"kinds": {"gain": {"max_gain_db": float("nan")}}}),
    dict(level={"kinds": {"gain_transition": {"min_duration": 0.0}}}), dict(level={"kinds": {"gain_transition": {"min_duration": 7.0}}}),
    dict(level={"kinds": {"shift": {"min_shift": -1.5}}}), dict(level={"kinds": {"shift": {"fade_duration": -1.0}}}),
    dict(level={"kinds": {"shift": {"max_shift": 2.0}}}), dict(sample_rate=0),
])
def test_constructor_refusals(kw):
    with pytest.raises(ValueError):
        WF.WaveAug(**kw)


# ------------------------------------------------------------------------------------------------------------ loader logic
def _dataset(**kw):
    return DL.AudioDataset(DL.SyntheticDataset(4, min_seconds=1.0), DL.SimpleTokenizer(), no_timestamp_training=True, spec_augment=True,
                           spec_augment_params={"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 0.5},
                           extremes_spec_augment=True, extremes_spec_augment_params={"low_freq_range": 5, "high_freq_range": 5}, **kw)


ALL_ON = {"noise": {"p": 1.0}, "clip": {"p": 1.0}, "level": {"p": 1.0}}


@pytest.mark.parametrize("stretch,filt", [(False, False), (True, False), (False, True), (True, True)])
def test_items_gain_exactly_one_field_behind_the_filter_and_torch_draws_are_untouched(stretch, filt):
    kw = dict(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25) if stretch else {}
    if filt:
        kw["filter_aug"] = {"p": 1.0}
    on, off = _dataset(wave_aug=ALL_ON, **kw), _dataset(**kw)
    base = 6 + int(stretch) + int(filt)
    a, b = [], []
    for i in range(4):
        torch.manual_seed(7 + i); random.seed(40 + i)
        a.append(on[i])
        after_on = torch.rand(1)
        torch.manual_seed(7 + i); random.seed(40 + i)
        b.append(off[i])
        assert torch.equal(after_on, torch.rand(1))  # torch's generator: the SpecAugment draws are the same with and without
    for x, y in zip(a, b):
        assert len(x) == base + 1 and len(y) == base
        for u, v in zip(x[:base], y):  # the stretch rate and the filter are drawn BEFORE the wave effects: unchanged
            assert torch.equal(torch.as_tensor(u), torch.as_tensor(v))
        assert x[-1].dtype == torch.float64 and x[-1].shape == (WF.TABLE_WIDTH,)
    ca, cb = DL.collate_fn(a), DL.collate_fn(b)
    assert len(ca) == base + 1 and len(cb) == base and ca[-1].dtype == torch.float64 and ca[-1].shape == (4, WF.TABLE_WIDTH)
    for u, v in zip(ca[:base], cb):
        assert torch.equal(u, v)
    WF.check_records(WF.records_from_table(ca[-1]))


def test_item_row_is_the_draw_after_the_filter():
    ds = _dataset(apply_baseline_aug=True, time_stretch_min_rate=0.8, time_stretch_max_rate=1.1, filter_aug={"p": 1.0, "kinds": ["low_shelf"]},
                  wave_aug={"noise": {"p": 1.0, "kinds": ["gaussian_snr"]}})
    random.seed(123)
    item = ds[0]
    random.seed(123)
    assert random.random() < 1.0
    random.uniform(0.8, 1.1)
    DL.FilterAug(p=1.0, kinds=["low_shelf"]).draw()
    names, row = WF.WaveAug(noise={"p": 1.0, "kinds": ["gaussian_snr"]}).draw(DL.N_SAMPLES)
    assert names["noise"] == "gaussian_snr" and np.array_equal(item[-1].numpy(), row) and len(item) == 9


def test_option_is_checked_and_the_other_pipelines_stay_refused():
    with pytest.raises(NotImplementedError, match="apply_advanced_aug"):
        _dataset(apply_advanced_aug=True, wave_aug={})
    with pytest.raises(NotImplementedError, match="apply_office_aug"):
        _dataset(apply_office_aug=True, wave_aug=ALL_ON)
    for bad in (True, {"gain": {}}, {"noise": {"p": 2.0}}, {"level": {"kinds": ["pitch_shift"]}}):
        with pytest.raises(ValueError):
            _dataset(wave_aug=bad)
    assert _dataset().wave_aug is None and _dataset(wave_aug={}).wave_aug.p == {}


def test_gpu_mel_loader_reads_the_fields_from_the_flags():
    class FakeFrontend:
        device = torch.device("cpu")

    def loader(**kw):
        return DL.GpuMelLoader(torch.utils.data.DataLoader(_dataset(**kw), batch_size=2, collate_fn=DL.collate_fn), FakeFrontend(), True)

    st, fl = dict(apply_baseline_aug=True), dict(filter_aug={"p": 1.0, "kinds": ["high_pass"]})
    for kw, fields in (({}, (False, False)), (st, (True, False)), (fl, (False, True)), ({**st, **fl}, (True, True))):
        ld = loader(wave_aug=ALL_ON, **kw)
        batch = next(iter(ld.loader))
        rates, sos, fx = ld._fields(batch)
        assert (rates is not None, sos is not None) == fields and len(batch) == 7 + sum(fields) and fx is not None
        assert fx.dtype == WF.RECORD_DTYPE and fx.shape == (2,) and ld._optional(batch)[0] is rates
        if sos is not None:
            assert sos.shape == (2, 4, 6)
    ld = loader(wave_aug={"noise": {"p": 0.0}, "level": {"p": 0.0}})
    assert ld._fields(next(iter(ld.loader))) == (None, None, None)  # nothing drawn: nothing to launch
    with pytest.raises(ValueError):
        loader(wave_aug=ALL_ON)._fields(next(iter(loader().loader)))
    assert loader().wave_aug is False and loader()._fields(next(iter(loader().loader))) == (None, None, None)


def test_debug_config_carries_the_option_and_its_block_builds():
    from pathlib import Path

    import yaml

    cfg = yaml.safe_load((Path(__file__).resolve().parents[1] / "configs" / "DEBUG_synthetic_wave.yaml").read_text())
    aa = cfg["augmentation"]["audio_augment"]
    assert aa["apply_advanced_aug"] is False and aa["apply_office_aug"] is False and set(aa["wft_wave_aug"]) == set(WF.STAGES)
    aug = WF.WaveAug(**aa["wft_wave_aug"])
    assert aug.kinds == WF.KINDS and {k: {n: v for n, v in r.items()} for k, r in aug.ranges.items()} == WF.DEFAULTS
    assert _dataset(wave_aug=aa["wft_wave_aug"], filter_aug=aa["wft_filter_aug"]).wave_aug.p == {"noise": 0.5, "clip": 0.5, "level": 0.5}


# ------------------------------------------------------------------------------------------------------------ host checks
def test_wave_fx_host_checks_raise_before_the_device_is_touched():
    x = torch.zeros(2, 64)  # a host tensor: reaching the device would raise something else than ValueError
    row = WF.table_row("gain", gain_db=1.0)
    for bad_audio in (x.double(), x[0], torch.zeros(0, 4), np.zeros((2, 4), dtype=np.float32)):
        with pytest.raises(ValueError):
            K.wave_fx(bad_audio, row, "level")
    with pytest.raises(ValueError):
        K.wave_fx(x, row, "reverb")
    with pytest.raises(ValueError):
        K.wave_fx(x, row, 3)
    with pytest.raises(ValueError):
        K.wave_fx(x, np.stack([row] * 3), "level")  # three records for two rows
    with pytest.raises(ValueError):
        K.wave_fx(x, row.astype(np.float32), "level")
    with pytest.raises(ValueError):
        K.wave_fx(x, row, "level", n=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        K.wave_fx(x, row, "level", out=torch.zeros(2, 63))
    rec = WF.records_from_table(np.stack([row] * 2))
    rec["clip_kind"][:] = 1
    rec["clip_q"][1] = 77
    with pytest.raises(ValueError):
        K.wave_fx(x, rec, "clip")
    with pytest.raises(ValueError):
        K.wave_fx(x.t(), row, "level", out=x.t())
    for kw in (dict(kind="gain", gain_db=float("nan")), dict(kind="clipping", q=51), dict(kind="shift", fraction=2.0), dict(kind="hiss")):
        with pytest.raises(ValueError):
            GF.wave_fx(np.zeros(16, dtype=np.float32), **kw)
    with pytest.raises(ValueError):
        GF.wave_fx(np.zeros(16, dtype=np.float64), "gain", gain_db=1.0)
