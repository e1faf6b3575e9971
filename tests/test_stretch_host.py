"""Time stretch, everything that needs no GPU: the float64 reference's two phase forms, the identity at rate 1, the float32
emulation inside the bound and the choice of its constant, the mutants the bound rejects, and the loader's logic around the rates."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import _stretch_cases as S
from whisper_finetune.data import data_loader as DL
from whisper_finetune.data import gpu_frontend as GF

INPUTS = S.inputs()
CASES = S.cases()
CASE_IDS = [f"{n}-{r}" for n, r in CASES]


@functools.lru_cache(maxsize=None)
def _ref(name, rate):
    return S.allowance(INPUTS[name], rate)


def test_cases_are_what_the_module_says():
    assert [INPUTS[f"noise{n}"].shape[0] for n in S.NOISE_N] == [2048, 5000, 16421]
    assert [S.n_frames(n) for n in S.NOISE_N] == [5, 10, 33]
    z = INPUTS["zeropad"]
    assert not z[:4096].any() and not z[-6000:].any() and z[4096:-6000].all()
    assert len(CASES) == 4 * 6
    for n in (2048, 5000, 16421):
        for r in S.rates():
            assert len(np.arange(0, S.n_frames(n), r)) == S.n_out_frames(S.n_frames(n), r)


def test_the_trap_rate_is_a_trap():
    """At TRAP_RATE float32 stepping picks another column pair than float64 at t = TRAP_T, inside the 33-frame case."""
    assert S.find_trap() == (S.TRAP_RATE, S.TRAP_T)
    r, t = S.TRAP_RATE, S.TRAP_T
    assert t < S.n_out_frames(33, r)
    assert np.floor(np.float32(t) * np.float32(r)) != np.floor(t * r)


@pytest.mark.parametrize("name,rate", CASES, ids=CASE_IDS)
def test_the_two_phase_forms_agree(name, rate):
    y = INPUTS[name]
    D = S.stft(y)
    a, b = S.vocoder(D, rate, "product"), S.vocoder(D, rate, "additive")
    assert np.abs(a - b).max() <= 1e-9
    n_out = S.n_out_samples(y.shape[0], rate)
    assert np.abs(S.istft(a, n_out) - S.istft(b, n_out)).max() <= 1e-9


@pytest.mark.parametrize("name", list(INPUTS))
def test_rate_one_returns_the_input(name):
    y = INPUTS[name]
    out = S.time_stretch(y, 1.0)
    assert out.shape == y.shape and np.abs(out - y.astype(np.float64)).max() <= 1e-10


@pytest.mark.parametrize("name,rate", CASES, ids=CASE_IDS)
def test_the_float32_emulation_lies_inside_the_bound(name, rate):
    want, allow, parts = _ref(name, rate)
    got = S.emulate_f32(INPUTS[name], rate)
    print(f"{name} rate {rate}: emulation uses {S.used(got, want, allow):.4f} of the allowance (largest allowance {allow.max():.2e})")
    assert S.outside(got, want, allow) == 0
    # and C_EMU alone (a quarter of the allowance the kernel gets) already holds it, bin by bin and sample by sample
    want, allow, parts = S.allowance(INPUTS[name], rate, c=S.C_EMU)
    assert S.outside(got, want, allow) == 0
    err = np.abs(S.emulate_f32(INPUTS[name], rate, stage="stft").astype(np.complex128) - parts["D"])
    assert (err <= parts["delta"][:, None]).all()


def test_the_constant_is_the_smallest_power_of_two():
    """C_EMU / 2 does not hold the emulation (its STFT bins leave delta_t on some case): C_EMU is the smallest power of two."""
    fails = 0
    for name in INPUTS:
        y = INPUTS[name]
        err = np.abs(S.emulate_f32(y, 1.0, stage="stft").astype(np.complex128) - S.stft(y))
        fails += int((err > S.stft_allowance(y, S.C_EMU / 2)[:, None]).sum())
    assert fails > 0
    assert S.C == 4 * S.C_EMU


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_the_bound_rejects_the_mutant(mutant):
    hits = []
    for name, rate in CASES:
        if mutant == "float32_stepping" and rate != S.TRAP_RATE:
            continue
        if mutant == "unit_of_zero_is_minus_one" and name != "zeropad":
            continue
        want, allow, _ = _ref(name, rate)
        n = S.outside(S.time_stretch(INPUTS[name], rate, mutant=mutant), want, allow)
        if n:
            hits.append((name, rate, n))
    print(mutant, hits)
    assert hits, f"{mutant} stays inside the bound on every case"


def test_at_least_twelve_mutants():
    assert len(set(S.MUTANTS)) >= 12


def test_exact_spectra_are_exact():
    """The constructed spectra of the vocoder's bit-for-bit test: the float32 tree equals the float64 reference exactly."""
    re, im = S.exact_spectra()
    assert ((re == 0) & (im == 0)).any() and (np.signbit(re) & (re == 0)).any() and (~np.signbit(re) & (re == 0)).any()
    for rate in (0.5, 0.75, 1.25):
        sr, si = S.vocoder_exact(re, im, rate)
        want = S.vocoder((re.astype(np.float64) + 1j * im.astype(np.float64)), rate)
        assert np.array_equal(sr.astype(np.float64), want.real) and np.array_equal(si.astype(np.float64), want.imag)


# ------------------------------------------------------------------------------------------------------------ loader logic
def _dataset(**kw):
    return DL.AudioDataset(DL.SyntheticDataset(4, min_seconds=1.0), DL.SimpleTokenizer(), no_timestamp_training=True, spec_augment=True,
                           spec_augment_params={"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 0.5},
                           extremes_spec_augment=True, extremes_spec_augment_params={"low_freq_range": 5, "high_freq_range": 5}, **kw)


def test_items_gain_a_seventh_field_and_the_six_stay_bit_equal():
    on, off = _dataset(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25), _dataset()
    torch.manual_seed(7)
    a = [on[i] for i in range(4)]
    torch.manual_seed(7)
    b = [off[i] for i in range(4)]
    for x, y in zip(a, b):
        assert len(x) == 7 and len(y) == 6
        for u, v in zip(x[:6], y):
            assert torch.equal(torch.as_tensor(u), torch.as_tensor(v))
        assert x[6].dtype == torch.float64 and x[6].shape == () and 0.75 <= float(x[6]) <= 1.25
    ca, cb = DL.collate_fn(a), DL.collate_fn(b)
    assert len(ca) == 7 and len(cb) == 6 and ca[6].dtype == torch.float64 and ca[6].shape == (4,)
    for u, v in zip(ca[:6], cb):
        assert torch.equal(u, v)


def test_random_seed_reproduces_the_rates_in_audiomentations_order():
    ds = _dataset(apply_baseline_aug=True, time_stretch_min_rate=0.8, time_stretch_max_rate=1.1)
    random.seed(123)
    got = [float(ds[i][6]) for i in range(4)]
    random.seed(123)
    want = []
    for _ in range(4):
        assert random.random() < 1.0          # the gate against p = 1.0
        want.append(random.uniform(0.8, 1.1))
    assert got == want
    random.seed(123)
    assert [float(ds[i][6]) for i in range(4)] == got


@pytest.mark.parametrize("lo,hi", [(0.4, 1.0), (0.8, 2.5), (1.2, 0.9), (float("nan"), 1.0)])
def test_bad_rate_ranges_raise(lo, hi):
    with pytest.raises(ValueError):
        _dataset(apply_baseline_aug=True, time_stretch_min_rate=lo, time_stretch_max_rate=hi)
    _dataset(time_stretch_min_rate=lo, time_stretch_max_rate=hi)  # without the flag the range is not used, as before


@pytest.mark.parametrize("flag", ["apply_office_aug", "apply_advanced_aug"])
def test_the_other_pipelines_stay_refused_by_name(flag):
    with pytest.raises(NotImplementedError, match=flag):
        _dataset(**{flag: True})
    with pytest.raises(NotImplementedError, match="pitch shift"):
        _dataset(apply_baseline_aug=True, **{flag: True})


def test_rates_are_checked_before_the_device_is_touched():
    from whisper_finetune.engine import kernels as K

    for bad in (0.49, 2.01, float("nan")):
        with pytest.raises(ValueError):
            K.stretch_rates([1.0, bad], 2)
        with pytest.raises(ValueError):
            GF.time_stretch(np.zeros(4096, dtype=np.float32), bad)
    with pytest.raises(ValueError):
        K.stretch_rates([1.0, 1.1, 1.2], 2)
    assert K.stretch_rates(0.75, 3).tolist() == [0.75] * 3 and K.stretch_rates(torch.tensor([0.5, 2.0], dtype=torch.float64), 2).dtype == np.float64


def test_frames_and_keep_arithmetic():
    for (n, keep, T_out), want in S.RAGGED_TABLE:
        assert S.frames_and_keep(n, keep, T_out) == want


def test_workspace_query_is_a_host_function():
    from whisper_finetune.engine import lib as L

    q = L.load().wft_time_stretch_workspace_bytes
    assert q(1, 480000, 0.5) == (938 + 1876) * 1025 * 8
    assert q(3, 16421, 0.75) == 3 * (33 + 44) * 1025 * 8
    assert q(1, 480000, 0.4) == -1 and q(0, 480000, 1.0) == -1 and q(1, 0, 1.0) == -1
