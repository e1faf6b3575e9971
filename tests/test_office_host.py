"""Office effects on the host: the f32 emulation of wft_fir_conv_f32's scheme stays inside the per-element bound of
tests/_office_cases.py and the bound rejects twelve planted defects; the shoebox impulse response; OfficeAug's draws, rates, refusals
and table check; the bit-crush restatement; the loader's plumbing and the wrappers' host-side refusals."""
import math
import random

import numpy as np
import pytest
import torch

from tests import _office_cases as O
from whisper_finetune.data import data_loader as DL
from whisper_finetune.data import gpu_frontend as GF
from whisper_finetune.data import office_fx as OF
from whisper_finetune.data import rate_fx as RF
from whisper_finetune.engine import kernels as K
from whisper_finetune.engine import lib as L


def _emulate(case, mutant=None):
    return O.emulate(case["X"], case["ns"], case["IR"], case["Ts"], case["n_max"], case["taps_max"], mutant)


# ------------------------------------------------------------------------------------------------------------ binding
def test_binding_and_the_pure_host_functions():
    lib = L.load()
    assert lib.wft_fir_conv_block() == O.L == OF.BLOCK == 1024
    assert lib.wft_fir_conv_workspace_bytes(3, 1) == 3 * 1025 * 8 and lib.wft_fir_conv_workspace_bytes(2, 1025) == 2 * 2 * 1025 * 8
    assert lib.wft_fir_conv_workspace_bytes(1, 8192) == 8 * 1025 * 8
    for B, taps in ((0, 5), (65536, 5), (1, 0), (1, 8193), (-1, -1)):
        assert lib.wft_fir_conv_workspace_bytes(B, taps) == -1
    assert K.FIR_TAPS_MAX == OF.TAPS_MAX == 8192


# ------------------------------------------------------------------------------------------------------------ the bound
def test_emulation_stays_inside_the_bound_and_the_measured_ratio_is_the_recorded_one():
    worst, where = 0.0, None
    for case in O.CASES:
        ok, ratio, complaint = O.check(_emulate(case), case)
        assert ok, (case["name"], complaint)
        if ratio > worst:
            worst, where = ratio, case["name"]
    print(f"largest |emulation - ref| / (11 * 2^-24 * sum): {worst:.5f} at {where}; C = {O.C}")
    assert 0.9 * O.MEASURED_RATIO <= worst <= O.MEASURED_RATIO and O.C == 4 * O.MEASURED_RATIO


def test_case_table_covers_the_stated_ground():
    assert len(O.CASES) == len(O.N_MAXES) * len(O.TAPS_MAXES) + 1
    assert {c["n_max"] for c in O.CASES} == set(O.N_MAXES) and set(O.TAPS_MAXES) <= {c["taps_max"] for c in O.CASES}
    assert {-(-c["taps_max"] // O.L) for c in O.CASES} == {1, 2, 3}
    assert any(0 in c["ns"] for c in O.CASES) and any(0 in c["Ts"] for c in O.CASES)
    for c in O.CASES:  # poisoned padding behind n[b] and n_taps[b]
        for b in range(3):
            assert np.isnan(c["X"][b, min(c["ns"][b], c["n_max"]):]).all() and np.isnan(c["IR"][b, c["Ts"][b]:]).all()
            assert np.isfinite(c["X"][b, :c["ns"][b]]).all() and np.isfinite(c["IR"][b, :c["Ts"][b]]).all()


@pytest.mark.parametrize("mutant", O.MUTANTS)
def test_bound_rejects_a_planted_defect(mutant):
    rejected = [case["name"] for case in O.CASES if not O.check(_emulate(case, mutant), case)[0]]
    assert rejected, mutant


def test_reference_is_the_definition():
    x, h = np.array([1.0, 2.0, -1.0, 0.5, 9.0], dtype=np.float32), np.array([0.5, 0.0, 2.0, 7.0], dtype=np.float32)
    assert np.array_equal(O.reference(x, 4, h, 3, 6), [0.5, 1.0, 1.5, 4.25, 0.0, 0.0])
    assert np.array_equal(O.reference(x, 3, h, 0, 4), [1.0, 2.0, -1.0, 0.0])
    assert np.array_equal(O.reference(x, 0, h, 3, 2), [0.0, 0.0])


# ------------------------------------------------------------------------------------------------------------ room_ir
def test_room_ir_direct_path_by_hand():
    # fs = c: the delay in samples is the distance in metres.  d = 2 exactly: the fractional delay is the window's centre tap alone.
    ir = OF.room_ir([10.0, 10.0, 10.0], [3.0, 5.0, 5.0], [5.0, 5.0, 5.0], 0.3, max_order=0, sample_rate=343)
    assert ir.dtype == np.float32 and ir.shape == (2 + 81,)
    want = np.zeros(83)
    want[2 + 40] = 1.0 / (4.0 * math.pi * 2.0)
    assert np.allclose(ir, want, rtol=0, atol=2e-9)  # half an f32 ulp at 0.04
    # d = 2.5: a half-sample delay, taps hann[k] * sinc(k - 40 - 0.5) from index 2
    ir = OF.room_ir([10.0, 10.0, 10.0], [2.5, 5.0, 5.0], [5.0, 5.0, 5.0], 0.3, max_order=0, sample_rate=343)
    k = np.arange(81)
    taps = (0.5 - 0.5 * np.cos(2 * np.pi * k / 80)) * np.sinc(k - 40.5) / (4.0 * math.pi * 2.5)
    assert ir.shape == (83,) and np.allclose(ir[2:], taps, rtol=0, atol=2e-9) and np.all(ir[:2] == 0)


def test_room_ir_images_and_amplitudes():
    size, src = np.array([4.0, 3.0, 2.5]), np.array([1.0, 1.2, 1.1])
    for order, count in ((0, 1), (1, 7), (2, 25), (3, 63)):
        pos, refl = OF.image_sources(size, src, order)
        assert pos.shape == (count, 3) and int(refl.max()) == order
    pos, refl = OF.image_sources(size, src, 1)
    got = {tuple(np.round(p, 9)) for p in pos}
    assert got == {(1.0, 1.2, 1.1), (-1.0, 1.2, 1.1), (7.0, 1.2, 1.1), (1.0, -1.2, 1.1), (1.0, 4.8, 1.1), (1.0, 1.2, -1.1), (1.0, 1.2, 3.9)}
    # the response's energy falls with the absorption, and order 0 is the direct path of every order
    mic = np.array([2.0, 1.5, 1.2])
    e = [float((OF.room_ir(size, src, mic, a, 3).astype(np.float64) ** 2).sum()) for a in (0.05, 0.2, 0.9)]
    assert e[0] > e[1] > e[2]
    direct, full = OF.room_ir(size, src, mic, 1.0, 0), OF.room_ir(size, src, mic, 1.0, 3)  # absorption 1: only r = 0 survives
    assert np.array_equal(full[:direct.shape[0]], direct) and not full[direct.shape[0]:].any()
    for bad in (dict(size=[4, 3]), dict(mic=[5.0, 1, 1]), dict(absorption=1.5), dict(max_order=-1), dict(max_order=2.0), dict(mic=src),
                dict(sample_rate=0), dict(size=[4.0, float("nan"), 2.0])):
        kw = dict(size=size, source=src, mic=mic, absorption=0.1, max_order=1, sample_rate=16000)
        kw.update(bad)
        with pytest.raises(ValueError):
            OF.room_ir(**kw)


def test_room_ir_length_stays_inside_the_cap_and_fftconvolve_agrees_with_the_reference():
    from scipy.signal import fftconvolve

    aug = OF.OfficeAug(16000, room={"p": 1.0})
    assert aug.cap == 2048 == OF.table_cap([5.0, 4.0, 3.0], 3)
    random.seed(2)
    longest = 0
    for _ in range(200):
        names, row = aug.draw()
        assert names == {"crush": False, "room": True} and row.shape == (2 + 2048,) and row[0] == 0
        T = int(row[1])
        longest = max(longest, T)
        assert 81 <= T <= aug.cap and not row[2 + T:].any()
    assert 81 < longest <= aug.cap
    ir = row[2:2 + T].astype(np.float32)
    x = np.random.default_rng(5).standard_normal(5000).astype(np.float32)
    ref = O.reference(x, 5000, ir, T, 5000)
    full = fftconvolve(x.astype(np.float64), ir.astype(np.float64))[:5000]
    assert np.abs(full - ref).max() <= 1e-12 * float(np.abs(ref).max()) + 1e-15


# ------------------------------------------------------------------------------------------------------------ OfficeAug
def test_office_aug_draw_order():
    aug = OF.OfficeAug(16000, crush={"p": 1.0}, room={"p": 1.0})
    random.seed(91)
    names, row = aug.draw()
    random.seed(91)
    assert random.random() < 1.0
    depth = random.randint(6, 14)
    assert random.random() < 1.0
    size = np.array([random.uniform(3.0, 5.0), random.uniform(2.5, 4.0), random.uniform(2.4, 3.0)])
    absorption = random.uniform(0.05, 0.20)
    src = np.array([random.uniform(0.1, 3.5), random.uniform(0.1, 2.7), random.uniform(1.0, 2.1)])
    dist, az, el = random.uniform(0.15, 0.35), random.uniform(0.0, 2 * math.pi), random.uniform(-math.pi / 2, math.pi / 2)
    after = random.random()
    src = np.clip(src, 0.1, size - 0.1)
    mic = np.clip(src + dist * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)]), 0.1, size - 0.1)
    ir = OF.room_ir(size, src, mic, absorption, 3, 16000)
    assert names == {"crush": True, "room": True} and row[0] == depth and row[1] == ir.shape[0]
    assert np.array_equal(row[2:2 + ir.shape[0]], ir.astype(np.float64)) and not row[2 + ir.shape[0]:].any()
    random.seed(91)
    aug.draw()
    assert random.random() == after  # exactly 2 + 1 + 10 draws
    # a failed gate draws nothing else
    random.seed(4)
    names, row = OF.OfficeAug(16000, crush={"p": 0.0}, room={"p": 0.0}).draw()
    after = random.random()
    random.seed(4)
    random.random(), random.random()
    assert names == {"crush": False, "room": False} and not row.any() and random.random() == after
    assert OF.OfficeAug(16000).draw()[0] == {"crush": False, "room": False}


def test_office_aug_marginal_rates_and_ranges():
    aug = OF.OfficeAug(16000, crush={}, room={"max_order": 0})  # order 0 keeps the 4000 designs cheap
    assert aug.p == {"crush": 0.25, "room": 0.5} and aug.bit_range == (6, 14) and aug.cap == 1024
    random.seed(8)
    draws = [aug.draw() for _ in range(4000)]
    crush = np.array([r[0] for _, r in draws])
    room = np.array([r[1] for _, r in draws])
    assert abs((crush > 0).mean() - 0.25) < 0.03 and abs((room > 0).mean() - 0.5) < 0.03
    assert set(np.unique(crush[crush > 0]).astype(int)) == set(range(6, 15))
    assert all(n["crush"] == (r[0] > 0) and n["room"] == (r[1] > 0) for n, r in draws)
    OF.check_table(np.stack([r for _, r in draws[:64]]))


def test_office_aug_refusals():
    for bad in (dict(crush={"p": 1.5}), dict(crush={"bits": 3}), dict(crush={"min_bit_depth": 0}), dict(crush={"max_bit_depth": 25}),
                dict(crush={"min_bit_depth": 9, "max_bit_depth": 8}), dict(crush={"min_bit_depth": 6.5}), dict(crush=True),
                dict(room={"max_order": -1}), dict(room={"max_order": 1.0}), dict(room={"min_absorption_value": -0.1}),
                dict(room={"max_absorption_value": 1.2}), dict(room={"min_size_x": 6.0}), dict(room={"min_size_y": 0.1}),
                dict(room={"min_mic_distance": 0.0}), dict(room={"order": 3}), dict(room={"p": "often"}), dict(sample_rate=16000.0)):
        with pytest.raises(ValueError):
            OF.OfficeAug(**{"sample_rate": 16000, **bad})
    # cap: the smallest multiple of 1024 >= fs * (max_order + 1) * diag_max / c + 81; above 8192 the option raises
    diag = math.sqrt(5.0 ** 2 + 4.0 ** 2 + 3.0 ** 2)
    for order in range(0, 30):
        cap = int(math.ceil((16000 * (order + 1) * diag / 343.0 + 81) / 1024)) * 1024
        if cap <= 8192 and order <= 16:
            assert OF.OfficeAug(16000, room={"max_order": order}).cap == cap
        else:
            with pytest.raises(ValueError):
                OF.OfficeAug(16000, room={"max_order": order})
    assert OF.OfficeAug(16000, room={"max_order": 3}).cap == 2048
    with pytest.raises(ValueError, match="8192"):
        OF.OfficeAug(16000, room={"max_order": 10, "max_size_x": 30.0})  # 16000 * 11 * 30.4 / 343 = 15 600 taps


def test_check_table():
    good = OF.none_table(2048, 3)
    good[0, 0], good[1, 1], good[1, 2:5] = 8, 3, [0.5, -0.25, 0.125]
    out = OF.check_table(torch.from_numpy(good))
    assert out.dtype == np.float64 and np.array_equal(out, good)
    for col, val in ((0, 25), (0, -1), (0, 6.5), (0, float("nan")), (1, 2049), (1, -1), (1, 1.5), (2, float("inf")), (2, 1e39), (7, 0.1)):
        bad = good.copy()
        bad[1, col] = val
        with pytest.raises(ValueError):
            OF.check_table(bad)
    for shape in ((3, 2 + 1000), (3, 2), (3, 2 + 9216), (2 + 1024,)):
        with pytest.raises(ValueError):
            OF.check_table(np.zeros(shape))
    with pytest.raises(ValueError):
        OF.check_table(good.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ bit crush
def test_bitcrush_restatement_against_numpy_on_ties_and_zeros():
    x = O.crush_values()
    for depth in (1, 6, 14, 24):
        q = np.float32(2 ** (depth - 1) + 1)
        assert float(q) == 2 ** (depth - 1) + 1  # exact in f32 up to depth 24
        want = np.round(x * q) / q
        assert want.dtype == np.float32 and np.array_equal(O.bits(O.bitcrush_numpy(x, depth)), O.bits(want))
    assert float(np.float32(2 ** 24 + 1)) != 2 ** 24 + 1  # ... and not at 25: the kernel copies such a row
    # half to even, in f32, at depth 6 (q = 33): 0.5 / 33 * 33 rounds to 0, 1.5 / 33 * 33 to 2
    # exact ties at depth 2 (q = 3): 0.5, 1.5, 2.5 and -0.5 round half to even; the zeros keep their signs
    x3 = np.array([0.5, 1.5, 2.5, -0.5, 0.0, -0.0], dtype=np.float32) / np.float32(3)
    assert np.array_equal(x3 * np.float32(3), np.array([0.5, 1.5, 2.5, -0.5, 0.0, -0.0], dtype=np.float32))
    want = np.array([0.0, 2.0, 2.0, -0.0, 0.0, -0.0], dtype=np.float32) / np.float32(3)
    assert np.array_equal(O.bits(O.bitcrush_numpy(x3, 2)), O.bits(want))
    for depth in (0, -3, 25, 1 << 20):
        assert np.array_equal(O.bits(O.bitcrush_numpy(x, depth)), O.bits(x))
    assert np.array_equal(K.bitcrush_depths([0, 1, 24], 3), [0, 1, 24]) and K.bitcrush_depths(8, 2).tolist() == [8, 8]


# ------------------------------------------------------------------------------------------------------------ loader plumbing
def _dataset(**kw):
    return DL.AudioDataset(DL.SyntheticDataset(4, min_seconds=1.0), DL.SimpleTokenizer(), no_timestamp_training=True, spec_augment=True,
                           spec_augment_params={"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 0.5},
                           extremes_spec_augment=True, extremes_spec_augment_params={"low_freq_range": 5, "high_freq_range": 5}, **kw)


BOTH = {"crush": {"p": 1.0}, "room": {"p": 1.0}}
RATE = {"alias": {"p": 1.0}, "pitch": {"p": 1.0}}


@pytest.mark.parametrize("stretch,rate", [(False, False), (True, True)])
def test_items_gain_exactly_one_last_field_and_earlier_draws_are_untouched(stretch, rate):
    kw = dict(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25) if stretch else {}
    if rate:
        kw.update(rate_aug=RATE, filter_aug={"p": 1.0}, wave_aug={"noise": {"p": 1.0}})
    on, off = _dataset(office_aug=BOTH, **kw), _dataset(**kw)
    base = 6 + int(stretch) + 3 * int(rate)
    a, b = [], []
    for i in range(3):
        torch.manual_seed(7 + i); random.seed(40 + i)
        a.append(on[i])
        after_on = torch.rand(1)
        torch.manual_seed(7 + i); random.seed(40 + i)
        b.append(off[i])
        assert torch.equal(after_on, torch.rand(1))
    for x, y in zip(a, b):
        assert len(x) == base + 1 and len(y) == base
        for u, v in zip(x[:base], y):  # everything shipped before is drawn BEFORE the office effects: identical
            assert torch.equal(torch.as_tensor(u), torch.as_tensor(v))
        assert x[-1].dtype == torch.float64 and x[-1].shape == (2 + 2048,) and x[-1][0] > 0 and x[-1][1] > 0
    ca, cb = DL.collate_fn(a), DL.collate_fn(b)
    assert len(ca) == base + 1 and ca[-1].shape == (3, 2 + 2048)
    for u, v in zip(ca[:base], cb):
        assert torch.equal(u, v)
    OF.check_table(ca[-1])


def test_item_row_is_the_draw_after_the_rate_effects():
    ds = _dataset(rate_aug=RATE, office_aug=BOTH)
    random.seed(77)
    item = ds[0]
    random.seed(77)
    RF.RateAug(16000, **RATE).draw()
    names, row = OF.OfficeAug(16000, **BOTH).draw()
    assert all(names.values()) and np.array_equal(item[-1].numpy(), row) and len(item) == 8


def test_option_is_checked_and_apply_office_aug_stays_refused_and_names_the_option():
    with pytest.raises(NotImplementedError, match="apply_office_aug") as e:
        _dataset(apply_office_aug=True, office_aug=BOTH)
    assert "wft_office_aug" in str(e.value)
    with pytest.raises(NotImplementedError, match="apply_advanced_aug"):
        _dataset(apply_advanced_aug=True, office_aug={})
    for bad in (True, {"reverb": {}}, {"crush": {"p": 2.0}}, {"room": {"max_order": 40}}, [("crush", {})]):
        with pytest.raises(ValueError):
            _dataset(office_aug=bad)
    assert _dataset().office_aug is None and _dataset(office_aug={}).office_aug.p == {}


def test_gpu_mel_loader_counts_the_field_and_dev_loaders_never_get_it():
    class FakeFrontend:
        device = torch.device("cpu")

    def loader(**kw):
        return DL.GpuMelLoader(torch.utils.data.DataLoader(_dataset(**kw), batch_size=2, collate_fn=DL.collate_fn), FakeFrontend(), True)

    for kw, n_fields in (({}, 7), (dict(apply_baseline_aug=True), 8), (dict(rate_aug=RATE, apply_baseline_aug=True), 9)):
        ld = loader(office_aug=BOTH, **kw)
        batch = next(iter(ld.loader))
        assert ld.office_aug and len(batch) == n_fields
        fields = ld._all_fields(batch)
        assert len(fields) == 4 and (fields[0] is not None) == ("apply_baseline_aug" in kw) and (fields[3] is not None) == ("rate_aug" in kw)
        office = ld._office_field(batch)
        assert office.dtype == np.float64 and office.shape == (2, 2050) and bool((office[:, :2] > 0).all())
    ld = loader(office_aug={"crush": {"p": 0.0}, "room": {"p": 0.0}})
    batch = next(iter(ld.loader))
    assert len(batch) == 7 and ld._office_field(batch) is None  # nothing drawn: nothing to launch
    with pytest.raises(ValueError):
        loader(office_aug=BOTH)._all_fields(next(iter(loader().loader)))
    assert loader().office_aug is False and loader()._office_field(next(iter(loader().loader))) is None
    import inspect

    src = inspect.getsource(__import__("whisper_finetune.scripts.finetune", fromlist=["main"]).main)
    assert src.count('aa.get("wft_office_aug")') == 1  # the train loader alone reads the option


def test_debug_config_carries_the_option_and_its_block_builds():
    from pathlib import Path

    import yaml

    cfg = yaml.safe_load((Path(__file__).resolve().parents[1] / "configs" / "DEBUG_synthetic_office.yaml").read_text())
    aa = cfg["augmentation"]["audio_augment"]
    assert aa["apply_advanced_aug"] is False and aa["apply_office_aug"] is False and set(aa["wft_office_aug"]) == set(OF.STAGES)
    ds = _dataset(office_aug=aa["wft_office_aug"], rate_aug=aa["wft_rate_aug"], wave_aug=aa["wft_wave_aug"], filter_aug=aa["wft_filter_aug"])
    assert ds.office_aug.p == {"crush": 0.5, "room": 0.5} and ds.office_aug.bit_range == (6, 14) and ds.office_aug.cap == 2048


# ------------------------------------------------------------------------------------------------------------ host checks
def test_wrappers_raise_before_the_device_is_touched():
    x = torch.zeros(2, 64)  # a host tensor: reaching the device would raise something else than ValueError
    ir = torch.zeros(2, 8)
    n = torch.full((2,), 64, dtype=torch.int32)
    for bad_audio in (x.double(), x[0], torch.zeros(0, 4), np.zeros((2, 4), dtype=np.float32)):
        with pytest.raises(ValueError):
            K.fir_conv(bad_audio, ir)
        with pytest.raises(ValueError):
            K.bitcrush(bad_audio, 8)
    for bad_ir in (ir.double(), torch.zeros(3, 8), torch.zeros(2, 0), torch.zeros(2, 8193), torch.zeros(2, 2, 2), np.zeros((2, 8), dtype=np.float32)):
        with pytest.raises(ValueError):
            K.fir_conv(x, bad_ir)
    for depth in (25, -1, 6.5, float("nan"), [8, 8, 8], "deep"):
        with pytest.raises(ValueError):
            K.bitcrush(x, depth)
    with pytest.raises(ValueError):
        K.bitcrush(x, 8, out=torch.zeros(2, 63))
    with pytest.raises(ValueError):
        y = torch.zeros(64, 2).t()  # stride(1) == 2: cannot run in place
        K.bitcrush(y, 8, out=y)
    for a, h in ((np.zeros((2, 16), dtype=np.float64), np.ones(3)), (np.zeros((2, 16), dtype=np.float32), [np.ones(3)] * 3),
                 (np.zeros((2, 16), dtype=np.float32), np.ones(0)), (np.zeros((2, 16), dtype=np.float32), np.ones(8193)),
                 (np.zeros((2, 16), dtype=np.float32), np.ones((2, 3))), (np.zeros((2, 16), dtype=np.float32), np.array([1.0, np.nan])),
                 (np.zeros((2, 16), dtype=np.float32), np.ones(3, dtype=np.int64))):
        with pytest.raises(ValueError):
            GF.fir_convolve(a, h)
    for depth in (25, 6.5, [8, 8, 8]):
        with pytest.raises(ValueError):
            GF.bit_crush(np.zeros((2, 16), dtype=np.float32), depth)
    assert GF.room_ir is OF.room_ir
