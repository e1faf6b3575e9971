"""Filter augmentation, host side: the reference and the emulation of tests/_filter_cases.py, the bound and its mutants, the filter
designs of data/filters.py, the draws, the loader's items and the host checks of K.sos_filter.  No GPU."""
import random

import numpy as np
import pytest
import torch

from tests import _filter_cases as FC
from whisper_finetune.data import data_loader as DL
from whisper_finetune.data import filters as F
from whisper_finetune.data import gpu_frontend as GF
from whisper_finetune.engine import kernels as K
from whisper_finetune.engine import lib as L

CHUNK, GROUP = L.load().wft_sos_filter_chunk(), L.load().wft_sos_filter_group()  # pure host functions
TABLE = FC.table()
# a small chunk for the emulation's own tests: the scheme is the same at every L, and the seams come sooner
EMU_L = 32


def _batch(names, n, probe="noise_silent_tail", lens=None):
    x = np.stack([FC.probe(probe, n, EMU_L, 4, TABLE[k][1], seed=i) for i, k in enumerate(names)]).astype(np.float64)
    sos = np.stack([FC.padded(TABLE[k][0]) for k in names])
    return x, sos, (None if lens is None else np.asarray(lens))


# ------------------------------------------------------------------------------------------------------------ reference
def test_constants_and_delta():
    assert CHUNK >= 2 and GROUP >= 1
    assert FC.DELTA <= 2.0 ** -30 and np.log2(FC.DELTA) == int(np.log2(FC.DELTA))
    assert L.load().wft_sos_filter_workspace_bytes(3, 2 * CHUNK + 3, 4) == 3 * 3 * 8 * 8
    q = L.load().wft_sos_filter_workspace_bytes
    assert q(0, 100, 1) == -1 and q(1, 0, 1) == -1 and q(1, 100, 0) == -1 and q(1, 100, 5) == -1 and q(1, (1 << 30) + 1, 1) == -1


def test_reference_equals_scipy_sosfilt_bit_for_bit():
    ss = pytest.importorskip("scipy.signal")
    for name, (sos, exact) in TABLE.items():
        for p in FC.PROBES:
            x = FC.probe(p, 3 * CHUNK + 5, CHUNK, GROUP, exact).astype(np.float64)
            want = ss.sosfilt(sos, x)
            got = FC.reference(x[None], sos[None])[0]
            assert np.array_equal(got, want), (name, p, np.abs(got - want).max())


def test_rows_are_cut_at_their_own_length():
    x, sos, n = _batch(["lp150_o4", "hp20_o4", "identity"], 100, lens=[100, 37, 0])
    y = FC.reference(x, sos, n)
    assert np.array_equal(y[1, :37], FC.reference(x[1:2, :37], sos[1:2])[0]) and not y[1, 37:].any() and not y[2].any()
    assert np.array_equal(y[0], FC.reference(x[:1], sos[:1])[0])


# ------------------------------------------------------------------------------------------------------------ designs
def _response(sos, w):
    z = np.exp(-1j * w)
    h = np.ones_like(z)
    for s in sos:
        h = h * (s[0] + s[1] * z + s[2] * z * z) / (s[3] + s[4] * z + s[5] * z * z)
    return h


W = np.pi * np.logspace(-4, 0, 1024)  # 1024 log-spaced frequencies, 0.8 Hz .. Nyquist at 16 kHz
# measured against scipy over the cases of test_butterworth_designs_against_scipy: the largest difference of the two responses is
# 9.4e-10 (band_stop at 200 Hz, fraction 1.99, order 4: the numerator of the sum is factored numerically); 16 times that:
DESIGN_TOL = 1.5e-8
BUTTER_CASES = [(f, N) for f in (20.0, 150.0, 2400.0, 7500.0) for N in (1, 2, 3, 4)]
BAND_CASES = [(c, fr, N) for c, fr in ((200.0, 0.5), (200.0, 1.99), (4000.0, 0.5), (4000.0, 1.99), (1000.0, 1.0)) for N in (1, 2, 3, 4)]


def test_butterworth_designs_against_scipy():
    ss = pytest.importorskip("scipy.signal")
    assert DESIGN_TOL <= 1e-6
    worst = 0.0
    for f, N in BUTTER_CASES:
        for kind, bt in (("low_pass", "low"), ("high_pass", "high")):
            sos = F.design(kind, cutoff_freq=f, order=N)
            assert sos.shape == ((N + 1) // 2, 6) and np.all(sos[:, 3] == 1.0)
            worst = max(worst, np.abs(_response(sos, W) - _response(ss.butter(N, f, btype=bt, fs=16000, output="sos"), W)).max())
    for c, fr, N in BAND_CASES:
        lo, hi = c * (1 - fr / 2), c * (1 + fr / 2)
        bp = F.design("band_pass", center_freq=c, bandwidth_fraction=fr, order=N)
        bs = F.design("band_stop", center_freq=c, bandwidth_fraction=fr, order=N)
        assert bp.shape == (2 * ((N + 1) // 2), 6) and bs.shape == (N, 6) and np.all(bp[:, 3] == 1.0) and np.all(bs[:, 3] == 1.0)
        r = {(bt, f): _response(ss.butter(N, f, btype=bt, fs=16000, output="sos"), W) for bt in ("low", "high") for f in (lo, hi)}
        worst = max(worst, np.abs(_response(bp, W) - r[("high", lo)] * r[("low", hi)]).max())   # the cascade of the two edge filters
        worst = max(worst, np.abs(_response(bs, W) - (r[("low", lo)] + r[("high", hi)])).max())  # their sum
    print("largest difference of the responses", worst)
    assert worst <= DESIGN_TOL, worst


def test_designs_are_stable_and_fit_four_sections():
    for c, fr, N in BAND_CASES:
        for kind in ("band_pass", "band_stop"):
            sos = F.design(kind, center_freq=c, bandwidth_fraction=fr, order=N)
            assert sos.shape[0] <= 4
            assert all(np.abs(np.roots(s[3:])).max() < 1.0 for s in sos)


@pytest.mark.parametrize("g", [-18.0, -3.0, 6.0, 24.0])
@pytest.mark.parametrize("f,q", [(50.0, 0.1), (1000.0, 0.707), (7500.0, 0.999), (300.0, 5.0)])
def test_cookbook_biquads_have_their_derived_gains(f, q, g):
    at = np.array([0.0, 2 * np.pi * f / 16000, np.pi])
    full, half = 10 ** (g / 20), 10 ** (g / 40)
    lo, hi, pk = (np.abs(_response(F.design(k, center_freq=f, gain_db=g, q=q), at)) for k in ("low_shelf", "high_shelf", "peaking"))
    np.testing.assert_allclose(lo, [full, half, 1.0], rtol=1e-9)
    np.testing.assert_allclose(hi, [1.0, half, full], rtol=1e-9)
    np.testing.assert_allclose(pk, [1.0, full, 1.0], rtol=1e-9)


@pytest.mark.parametrize("kind,params", [
    ("low_pass", dict(cutoff_freq=0.0, order=2)), ("low_pass", dict(cutoff_freq=8000.0, order=2)), ("high_pass", dict(cutoff_freq=-5.0, order=2)),
    ("high_pass", dict(cutoff_freq=float("nan"), order=2)), ("low_pass", dict(cutoff_freq=100.0, order=0)),
    ("low_pass", dict(cutoff_freq=100.0, order=5)), ("low_pass", dict(cutoff_freq=100.0, order=2.5)),
    ("band_pass", dict(center_freq=4000.0, bandwidth_fraction=2.0, order=2)),   # the lower edge reaches 0, the upper 8000
    ("band_stop", dict(center_freq=7000.0, bandwidth_fraction=0.5, order=2)),   # the upper edge leaves the interval
    ("band_pass", dict(center_freq=100.0, bandwidth_fraction=2.5, order=2)),    # the lower edge is negative
    ("peaking", dict(center_freq=9000.0, gain_db=3.0, q=1.0)), ("low_shelf", dict(center_freq=100.0, gain_db=3.0, q=0.0)),
    ("notch", dict(center_freq=100.0)), ("low_pass", dict(center_freq=100.0, order=2)),
])
def test_bad_designs_raise(kind, params):
    with pytest.raises(ValueError):
        F.design(kind, **params)


@pytest.mark.parametrize("kw", [
    dict(p=1.5), dict(p=-0.1), dict(kinds=["notch"]), dict(kinds=[]), dict(kinds={"low_pass": {"min_freq": 0.0}}),
    dict(kinds={"low_pass": {"max_freq": 8000.0}}), dict(kinds={"low_pass": {"min_freq": 500.0, "max_freq": 100.0}}),
    dict(kinds={"band_pass": {"max_bandwidth_fraction": 2.0}}), dict(kinds={"band_stop": {"max_freq": 4100.0}}),
    dict(kinds={"peaking": {"min_q": 0.0}}), dict(kinds={"peaking": {"p": 2.0}}), dict(kinds={"high_pass": {"rolloffs": (12, 30)}}),
    dict(kinds={"high_pass": {"rolloffs": ()}}), dict(kinds={"low_shelf": {"min_gain_db": 3.0, "max_gain_db": -3.0}}),
    dict(kinds={"low_pass": {"gain": 1.0}}),
])
def test_bad_ranges_and_kinds_raise(kw):
    with pytest.raises(ValueError):
        F.FilterAug(**kw)
    with pytest.raises(ValueError):
        _dataset(filter_aug=kw)


# ------------------------------------------------------------------------------------------------------------ emulation, bound, mutants
EXACT = [k for k, (_, e) in TABLE.items() if e]


@pytest.mark.parametrize("n", [1, EMU_L - 1, EMU_L, EMU_L + 1, 2 * EMU_L + 3, 7 * EMU_L + 5])
def test_exact_cases_are_exact_in_the_emulation(n):
    for p in FC.PROBES:
        x, sos, _ = _batch(EXACT, n, p)
        want = FC.reference(x, sos)
        got = FC.emulate(x, sos, None, EMU_L)
        assert np.array_equal(got.astype(np.float64), want), p
        assert np.array_equal(want, want.astype(np.float32)), "the exact cases must be float32 values"


def test_emulation_stays_under_the_bound():
    names = [k for k in TABLE if k not in EXACT]
    for n in (EMU_L + 1, 9 * EMU_L + 7):
        for p in FC.PROBES:
            x, sos, _ = _batch(names, n, p)
            r = FC.worst_ratio(FC.emulate(x, sos, None, EMU_L), FC.reference(x, sos))
            assert r <= 1.0, (n, p, r)


MUTANT_ROWS = ["lp150_o4", "bs4000_f1.99_o4", "peak50_q5_p24"]  # three rows with their own coefficients and lengths


@pytest.mark.parametrize("mutant", FC.MUTANTS)
def test_bound_rejects_mutant(mutant):
    n_max = 9 * EMU_L + 7
    x, sos, n = _batch(MUTANT_ROWS, n_max, lens=[n_max, 5 * EMU_L + 9, 7 * EMU_L])
    x[:, :] = FC.probe("noise_silent_tail", 2 * n_max, EMU_L, 4)[None, :n_max]  # noise up to the end: what lies behind n[b] is not silent
    ref = FC.reference(x, sos, n)
    assert FC.worst_ratio(FC.emulate(x, sos, n, EMU_L), ref) <= 1.0
    r = FC.worst_ratio(FC.emulate(x, sos, n, EMU_L, mutant=mutant), ref)
    print(mutant, "largest error over the bound:", r)
    assert r > 1.0, f"{mutant} stays inside the bound"


def test_at_least_eight_mutants_and_the_equivalent_one():
    assert len(set(FC.MUTANTS)) >= 8
    # the state of a row's LAST chunk feeds nothing: taking it at L instead of at the row's true length changes no bit
    n_max = 9 * EMU_L + 7
    x, sos, n = _batch(MUTANT_ROWS, n_max, lens=[n_max, 5 * EMU_L + 9, 7 * EMU_L])
    assert np.array_equal(FC.emulate(x, sos, n, EMU_L), FC.emulate(x, sos, n, EMU_L, mutant=FC.EQUIVALENT_MUTANT))


def test_cases_cover_the_table_probes_and_lengths():
    cs = FC.cases(CHUNK, GROUP)
    assert len(cs) == len(TABLE) * len(FC.PROBES) * 8 and len(cs) % 3 == 0
    assert {c["n"] for c in cs} == {1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, GROUP * CHUNK - 1, GROUP * CHUNK + 1, 2 * GROUP * CHUNK + 5}
    mixed = sum(len({c["n"] for c in b}) > 1 and len({c["sos"].shape[0] for c in b}) > 1 for b in FC.batches(CHUNK, GROUP))
    assert mixed > len(cs) // 3 // 3  # most batches mix lengths and section counts


# ------------------------------------------------------------------------------------------------------------ draws
def test_random_seed_reproduces_the_draws_in_the_documented_order():
    aug = F.FilterAug()
    state = torch.get_rng_state()
    random.seed(99)
    got = [aug.draw() for _ in range(64)]
    assert torch.equal(torch.get_rng_state(), state), "the draw must not touch torch's generator"
    random.seed(99)
    kinds = set()
    for kind, params, sos in got:
        ident = np.tile(FC.IDENTITY, (4, 1))
        if not random.random() < 0.6:                                  # 1. the gate
            assert kind is None and params == {} and np.array_equal(sos, ident)
            continue
        k = F.KINDS[random.randrange(7)]                               # 2. the kind
        r = F.DEFAULTS[k]
        if not random.random() < r["p"]:                               # 3. the inner gate
            assert kind is None and np.array_equal(sos, ident)
            continue
        f = F.mel_to_hz(random.uniform(F.hz_to_mel(r["min_freq"]), F.hz_to_mel(r["max_freq"])))   # 4. the frequency, uniform in mel
        f = min(max(f, r["min_freq"]), r["max_freq"])
        if k in ("low_pass", "high_pass"):
            want = {"cutoff_freq": f, "order": r["rolloffs"][random.randrange(3)] // 6}             # 6. the rolloff
        elif k in ("band_pass", "band_stop"):
            frac = random.uniform(0.5, 1.99)                                                       # 5. the bandwidth fraction
            want = {"center_freq": f, "bandwidth_fraction": frac, "order": r["rolloffs"][random.randrange(3)] // 6}
        else:
            gain = random.uniform(r["min_gain_db"], r["max_gain_db"])                              # 5. the gain
            want = {"center_freq": f, "gain_db": gain, "q": random.uniform(r["min_q"], r["max_q"])}  # 6. Q
        assert kind == k and params == want
        d = F.design(k, **want)
        assert sos.shape == (4, 6) and sos.dtype == np.float64 and np.array_equal(sos[: d.shape[0]], d) and np.array_equal(sos[d.shape[0]:], ident[d.shape[0]:])
        kinds.add(k)
    assert len(kinds) >= 5
    random.seed(99)
    again = [aug.draw() for _ in range(64)]
    assert all(a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) for a, b in zip(got, again))


def test_defaults_are_the_issue_table():
    d = F.DEFAULTS
    assert [(d[k]["min_freq"], d[k]["max_freq"]) for k in F.KINDS] == [(150, 7500), (20, 2400), (200, 4000), (200, 4000), (50, 4000), (300, 7500), (50, 7500)]
    assert [d[k]["p"] for k in F.KINDS] == [1, 1, 1, 1, 1, 1, 0.8] and F.FilterAug().p == 0.6
    assert all(d[k]["rolloffs"] == (12, 18, 24) for k in F.KINDS[:4])
    assert all((d[k]["min_bandwidth_fraction"], d[k]["max_bandwidth_fraction"]) == (0.5, 1.99) for k in ("band_pass", "band_stop"))
    assert [(d[k]["min_gain_db"], d[k]["max_gain_db"], d[k]["min_q"], d[k]["max_q"]) for k in F.KINDS[4:]] == \
        [(-18, 18, 0.1, 0.999), (-18, 18, 0.1, 0.999), (-24, 24, 0.5, 5.0)]
    assert F.hz_to_mel(700.0) == pytest.approx(2595 * np.log10(2.0))


def test_kinds_subset_and_p_zero():
    random.seed(5)
    aug = F.FilterAug(p=1.0, kinds={"peaking": {"p": 1.0, "min_freq": 100.0, "max_freq": 100.0}})
    for _ in range(8):
        kind, params, _ = aug.draw()
        assert kind == "peaking" and params["center_freq"] == 100.0
    off = F.FilterAug(p=0.0)
    assert all(off.draw()[0] is None for _ in range(16))


# ------------------------------------------------------------------------------------------------------------ loader logic
def _dataset(**kw):
    return DL.AudioDataset(DL.SyntheticDataset(4, min_seconds=1.0), DL.SimpleTokenizer(), no_timestamp_training=True, spec_augment=True,
                           spec_augment_params={"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 0.5},
                           extremes_spec_augment=True, extremes_spec_augment_params={"low_freq_range": 5, "high_freq_range": 5}, **kw)


@pytest.mark.parametrize("stretch", [False, True])
def test_items_gain_exactly_one_field_and_the_others_stay_bit_equal(stretch):
    kw = dict(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25) if stretch else {}
    on, off = _dataset(filter_aug={"p": 1.0}, **kw), _dataset(**kw)
    base = 7 if stretch else 6
    # the stretch rate is drawn before the filter, both from Python's random: per item, the same seed gives the same rate
    a, b = [], []
    for i in range(4):
        torch.manual_seed(7 + i); random.seed(40 + i)
        a.append(on[i])
        torch.manual_seed(7 + i); random.seed(40 + i)
        b.append(off[i])
    for x, y in zip(a, b):
        assert len(x) == base + 1 and len(y) == base
        for u, v in zip(x[:base], y):
            assert torch.equal(torch.as_tensor(u), torch.as_tensor(v))
        assert x[-1].dtype == torch.float64 and x[-1].shape == (4, 6) and bool((x[-1][:, 3] == 1).all())
    ca, cb = DL.collate_fn(a), DL.collate_fn(b)
    assert len(ca) == base + 1 and len(cb) == base and ca[-1].dtype == torch.float64 and ca[-1].shape == (4, 4, 6)
    for u, v in zip(ca[:base], cb):
        assert torch.equal(u, v)


def test_item_filter_is_the_draw_after_the_stretch_rate():
    ds = _dataset(apply_baseline_aug=True, time_stretch_min_rate=0.8, time_stretch_max_rate=1.1, filter_aug={"p": 1.0, "kinds": ["low_shelf"]})
    random.seed(123)
    item = ds[0]
    random.seed(123)
    assert random.random() < 1.0
    rate = random.uniform(0.8, 1.1)
    kind, _, sos = F.FilterAug(p=1.0, kinds=["low_shelf"]).draw()
    assert float(item[6]) == rate and kind == "low_shelf" and np.array_equal(item[7].numpy(), sos)


def test_the_other_pipelines_stay_refused_with_the_option():
    with pytest.raises(NotImplementedError, match="apply_advanced_aug"):
        _dataset(apply_advanced_aug=True, filter_aug={})
    with pytest.raises(ValueError):
        _dataset(filter_aug=True)
    with pytest.raises(ValueError):
        _dataset(filter_aug={"p": 0.5, "sample_rate": 8000})


def test_gpu_mel_loader_reads_the_fields_from_the_flags():
    """Seven fields are ambiguous by their count: the loader takes the dataset's flags."""
    class FakeFrontend:
        device = torch.device("cpu")

    def loader(**kw):
        return DL.GpuMelLoader(torch.utils.data.DataLoader(_dataset(**kw), batch_size=2, collate_fn=DL.collate_fn), FakeFrontend(), True)

    st = dict(apply_baseline_aug=True)
    for kw, fields in (({}, (False, False)), (st, (True, False)), ({"filter_aug": {"p": 1.0, "kinds": ["high_pass"]}}, (False, True)),
                       ({**st, "filter_aug": {"p": 1.0, "kinds": ["high_pass"]}}, (True, True))):
        ld = loader(**kw)
        batch = next(iter(ld.loader))
        rates, sos = ld._optional(batch)
        assert (rates is not None, sos is not None) == fields and len(batch) == 6 + sum(fields)
        if rates is not None:
            assert rates.shape == (2,)
        if sos is not None:
            assert sos.shape == (2, 4, 6)
    ld = loader(filter_aug={"p": 0.0})
    assert ld._optional(next(iter(ld.loader))) == (None, None)  # an all-identity batch launches nothing
    with pytest.raises(ValueError):
        loader(**st)._optional(next(iter(loader().loader)) + (torch.zeros(2),) * 2)
    # a loader without a dataset (a list of batches) keeps reading a seventh field as the rates
    bare = DL.GpuMelLoader([None], FakeFrontend(), True)
    assert bare._optional(tuple(range(6)) + ("rates",)) == ("rates", None) and bare._optional(tuple(range(6))) == (None, None)


# ------------------------------------------------------------------------------------------------------------ host checks
def test_sos_filter_host_checks_raise_before_the_device_is_touched():
    x = torch.zeros(2, 64)  # a HOST tensor: anything that reached the device would raise WftError, not ValueError
    good = np.tile(FC.IDENTITY, (2, 1))
    bad = {
        "S = 0": np.zeros((0, 6)), "S = 5": np.tile(FC.IDENTITY, (5, 1)), "a0 != 1": np.array([[1.0, 0, 0, 2.0, 0, 0]]),
        "nan": np.array([[np.nan, 0, 0, 1.0, 0, 0]]), "inf": np.array([[1.0, 0, 0, 1.0, np.inf, 0]]), "five columns": np.ones((2, 5)),
        "rows": np.tile(FC.IDENTITY, (3, 2, 1)), "float32": good.astype(np.float32), "one dimension": FC.IDENTITY,
    }
    for what, sos in bad.items():
        with pytest.raises(ValueError):
            K.sos_filter(x, sos)
        with pytest.raises(ValueError):
            K.sos_filter(x, torch.from_numpy(np.ascontiguousarray(sos)))
        with pytest.raises(ValueError):
            GF.sos_filter(x.numpy(), sos)
    for audio in (torch.zeros(64), torch.zeros(2, 64, dtype=torch.float64), torch.zeros(0, 64), torch.zeros(2, 0)):
        with pytest.raises(ValueError):
            K.sos_filter(audio, good)
    with pytest.raises(ValueError):
        K.sos_filter(x, good, n=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        K.sos_filter(x, good, n=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        K.sos_filter(x, good, out=torch.zeros(2, 63))
    with pytest.raises(ValueError):
        GF.sos_filter(np.zeros((2, 2, 2), dtype=np.float32), good)
    with pytest.raises(L.WftError):
        K.sos_filter(x, good)  # every host check passed: only now the device is asked for
    assert K.sos_coefficients(good, 3).shape == (3, 2, 6) and GF.design_filter is F.design
