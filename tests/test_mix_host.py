"""Mix effects on the host: the float64 loudness reference of tests/_mix_cases.py against BS.1770's conformance figure, the gate-margin
condition of every case used on the GPU, the planted defects the comparisons must reject, MixAug's draws, refusals and table check,
the noise bank, the loader's plumbing and the wrappers' host-side refusals."""
import math
import random

import numpy as np
import pytest
import torch

from tests import _mix_cases as M
from whisper_finetune.data import data_loader as DL
from whisper_finetune.data import gpu_frontend as GF
from whisper_finetune.data import mix_fx as MF
from whisper_finetune.data import office_fx as OF
from whisper_finetune.engine import kernels as K
from whisper_finetune.engine import lib as L

BANK = {"synthetic": 4}
BOTH = {"background": {"p": 1.0, "bank": BANK}, "loudness": {"p": 1.0}}
OFFICE = {"crush": {"p": 1.0}, "room": {"p": 1.0}}


# ------------------------------------------------------------------------------------------------------------ binding
def test_binding_and_the_pure_host_functions():
    lib = L.load()
    C, NS = -(-48000 // 512), 30
    assert lib.wft_loudness_workspace_bytes(3, 48000, 1600) == 3 * (6 * C + NS) * 8 + 2 * 16
    assert lib.wft_bg_mix_workspace_bytes(3, 4097) == 3 * (2 * 2 + 1) * 8
    for B, n, hop in ((0, 5, 1600), (65536, 5, 1600), (1, 0, 1600), (1, (1 << 30) + 1, 1600), (1, 5, 511), (1, 5, (1 << 24) + 1)):
        assert lib.wft_loudness_workspace_bytes(B, n, hop) == -1
    for B, n in ((0, 5), (65536, 5), (1, 0), (1, (1 << 30) + 1)):
        assert lib.wft_bg_mix_workspace_bytes(B, n) == -1
    import ctypes

    assert ctypes.sizeof(L.BgRec) == MF.RECORD_DTYPE.itemsize == 24
    assert [getattr(L.BgRec, f).offset for f in ("kind", "entry", "offset", "db")] == [MF.RECORD_DTYPE.fields[f][1] for f in ("kind", "entry", "offset", "db")]
    assert (L.BG_NONE, L.BG_SNR, L.BG_ABSOLUTE) == tuple(MF.KIND_ID[k] for k in MF.KINDS)


# ------------------------------------------------------------------------------------------------------------ the reference
def test_reference_reads_the_conformance_sine_and_the_16_khz_value_is_pinned():
    got = {}
    for rate in (48000, 44100, 16000):
        t = np.arange(5 * rate, dtype=np.float64) / rate
        got[rate] = M.loud_ref(np.sin(2.0 * np.pi * 997.0 * t), 5 * rate, rate)["L"]
    print(got)
    assert abs(got[48000] - (-3.01)) <= 0.1  # ITU-R BS.1770's conformance figure and tolerance
    assert abs(got[48000] - (-3.0517)) < 5e-5 and abs(got[44100] - (-3.0524)) < 5e-5 and abs(got[16000] - (-3.0832)) < 5e-5
    assert abs(got[16000] - M.SINE_16K_LUFS) <= 1e-9


def test_k_weighting_is_the_cookbook_pair_and_the_rate_is_checked():
    sos = MF.k_weighting(48000)
    assert sos.shape == (2, 6) and sos.dtype == np.float64 and bool((sos[:, 3] == 1.0).all()) and GF.k_weighting is MF.k_weighting
    # the published 48 kHz coefficients of BS.1770 (four digits: the standard's table is a bilinear design of its own)
    assert np.allclose(sos[0, [0, 1, 2, 4, 5]], [1.5351, -2.6917, 1.1984, -1.6907, 0.7325], atol=2e-3)
    assert np.allclose(sos[1, [4, 5]], [-1.9900, 0.9901], atol=2e-4)  # (the standard's numerator is 1 -2 1, the cookbook's is scaled)
    assert np.allclose(sos[1, :3] / sos[1, 0], [1.0, -2.0, 1.0], atol=1e-12) and abs(sos[1, :3].sum()) < 1e-12  # a high pass
    for bad in (16001, 7990, 384010, 16000.0, True, "16000", None):
        with pytest.raises(ValueError):
            MF.k_weighting(bad)
    assert MF.loudness_hop(8000) == 800 and MF.loudness_hop(384000) == 38400


def test_block_count_is_upstreams_rounding_in_integers():
    for rate in (8000, 16000, 44100, 48000):
        hop = rate // 10
        for n in list(range(4 * hop, 4 * hop + 3 * hop + 2)) + [5 * rate, 30 * rate]:
            assert MF.block_count(n, hop) == int(np.round((n / rate - 0.4) / 0.1)) + 1, (rate, n)
    assert MF.block_count(6399, 1600) == 0 and [MF.block_count(n, 1600) for n in (6400, 7199, 7200, 7201, 8800)] == [1, 1, 1, 2, 3]


def test_three_level_row_has_the_stated_blocks():
    case = M.loud_case()
    ref = case["refs"][case["names"].index("three_level")]
    plain, left = M.gate_margin(ref, case["hop"])
    print(f"three-level row: {ref['nb']} blocks, {int(ref['J1'].sum())} over -70, {ref['over']} over both, nearest block {plain:.2f} dB from a gate")
    assert ref["nb"] == 27 and int(ref["J1"].sum()) == 20 and ref["over"] == 10 and plain > 5.0


def test_every_gpu_case_keeps_its_blocks_away_from_the_gates():
    for rate in (16000, 8000, 48000):
        case = M.loud_case(rate)
        for name, ref in zip(case["names"], case["refs"]):
            plain, left = M.gate_margin(ref, case["hop"])
            assert plain > M.GATE_MARGIN_DB and left > M.GATE_MARGIN_DB, (rate, name, plain, left)
            # the derived bounds are far below the margin (the widest: Gr of the three-level row, whose gate holds blocks 30 dB down)
            assert M.level_bound(ref, case["hop"], "J2") < 1e-6 and M.level_bound(ref, case["hop"], "J1") < M.GATE_MARGIN_DB / 100, (rate, name)
    case = M.loud_case()
    refs = dict(zip(case["names"], case["refs"]))
    assert case["ns"][:len(M.LOUD_N)] == list(M.LOUD_N) and [refs[f"noise_n{n}"]["nb"] for n in M.LOUD_N[:6]] == [0, 1, 1, 1, 2, 3]
    assert refs["zeros"]["L"] == -math.inf and refs["amplitude_1e-5"]["L"] == -math.inf and not refs["amplitude_1e-5"]["active"]
    q = refs["quiet_two_level"]
    assert q["over"] < q["nb"] and bool(((q["l"] > q["gamma"]) & (q["l"] < -70.0)).any())  # blocks between Gr and the absolute gate
    for b in range(len(case["ns"])):  # poison behind n[b]
        assert np.isnan(case["X"][b, case["ns"][b]:]).all() and np.isfinite(case["X"][b, :case["ns"][b]]).all()


@pytest.mark.parametrize("mutant", M.LOUD_MUTANTS)
def test_loudness_comparisons_reject_a_planted_defect(mutant):
    hits = M.loud_mutant_rejected(mutant)
    print(mutant, hits)
    assert hits


def test_loudness_comparisons_accept_the_reference_itself():
    assert M.loud_mutant_rejected(None) == []
    z = M.z_at_the_gate()
    assert -0.691 + 10.0 * np.log10(z) == -70.0


@pytest.mark.parametrize("mutant", M.BG_MUTANTS)
def test_background_comparisons_reject_a_planted_defect(mutant):
    hits = M.bg_mutant_rejected(mutant)
    print(mutant, len(hits))
    assert hits


def test_background_case_table_covers_the_stated_ground():
    case = M.bg_case()
    assert M.bg_mutant_rejected(None) == []
    assert set(case["ns"]) == set(M.BG_N)
    seen = {(case["ns"][b], case["lengths"][r[1]], r[2], r[0]) for b, r in enumerate(case["recs"]) if r[0]}
    for n in M.BG_N:
        for m in M.bg_lengths(n):
            for o in {0, max(m - n, 0)}:
                assert (n, m, o, 1) in seen and (n, m, o, 2) in seen, (n, m, o)
    copied = [b for b, r in enumerate(case["refs"]) if r["out64"] is None]
    assert len(copied) == 3 and sum(case["recs"][b][0] == 0 for b in copied) == 1  # two silent rows, one "none" row
    for b, r in enumerate(case["recs"]):  # the neighbours of every entry in use are +-1e6
        if r[0] and r[1] != case["silent"]:
            a, e = int(case["off"][r[1]]), int(case["off"][r[1] + 1])
            assert case["bank"][a - 1] == M.GUARD_VALUE and case["bank"][e] == -M.GUARD_VALUE
    for b in range(len(case["ns"])):
        assert np.isnan(case["X"][b, case["ns"][b]:]).all()


# ------------------------------------------------------------------------------------------------------------ draws
def test_draw_order_and_values_against_a_replay_of_pythons_random():
    aug = MF.MixAug(16000, **BOTH)
    assert aug.lengths == [48000, 120000, 496000, 196000] and aug.p == {"background": 1.0, "loudness": 1.0}
    for seed in range(20):
        random.seed(seed)
        names, row = aug.draw(480000)
        random.seed(seed)
        assert random.random() < 1.0
        kind = random.choice(("absolute", "snr"))
        entry = random.randrange(4)
        value = random.uniform(-30.0, -10.0) if kind == "absolute" else random.uniform(2.0, 4.0)
        m = aug.lengths[entry]
        offset = random.randint(0, m - 480000) if m > 480000 else 0
        assert random.random() < 1.0
        target = random.uniform(-31.0, -13.0)
        assert names == {"background": kind, "loudness": True}
        assert row.dtype == np.float64 and row.tolist() == [float(MF.KIND_ID[kind]), float(entry), float(offset), value, 1.0, target]
        assert (entry == 2) == (offset > 0 or m > 480000)
    random.seed(3)
    state = random.getstate()
    names, row = MF.MixAug(16000, background={"p": 0.0, "bank": BANK}, loudness={"p": 0.0}).draw(480000)
    random.setstate(state)
    random.random(); random.random()  # two failed gates, nothing else
    after = random.random()
    random.seed(3)
    MF.MixAug(16000, background={"p": 0.0, "bank": BANK}, loudness={"p": 0.0}).draw(480000)
    assert names == {"background": None, "loudness": False} and not row.any() and random.random() == after
    assert MF.MixAug(16000).draw(480000)[1].tolist() == [0.0] * 6


def test_default_rates_are_the_references_marginal_rates():
    aug = MF.MixAug(16000, background={"bank": BANK}, loudness={})
    assert aug.p == {"background": 0.3, "loudness": 0.3 / 4} and aug.kinds == ("absolute", "snr")
    assert aug.ranges == {"snr": (2.0, 4.0), "absolute": (-30.0, -10.0)} and aug.lufs == (-31.0, -13.0)
    random.seed(0)
    rows = np.array([aug.draw(480000)[1] for _ in range(4000)])
    assert abs((rows[:, 0] != 0).mean() - 0.3) < 0.03 and abs(rows[:, 4].mean() - 0.075) < 0.02
    short = rows[(rows[:, 0] != 0) & (rows[:, 1] != 2)]
    assert not short[:, 2].any()  # an entry that is not longer than the clip starts at 0


def test_constructor_refusals():
    for kw in (dict(background={}), dict(background={"bank": BANK, "p": 1.5}), dict(background={"bank": BANK, "kinds": []}),
               dict(background={"bank": BANK, "kinds": ["loud"]}), dict(background={"bank": BANK, "kinds": "snr"}),
               dict(background={"bank": BANK, "min_snr_db": 5.0, "max_snr_db": 4.0}), dict(background={"bank": BANK, "noise": 1}),
               dict(background={"bank": BANK, "max_absolute_rms_db": float("nan")}), dict(background={"bank": {"synthetic": 0}}),
               dict(background={"bank": BANK, "bank_sample_rate": 12.5}), dict(loudness={"p": -0.1}), dict(loudness={"min_lufs": -300.0}),
               dict(loudness={"lufs": -20}), dict(loudness=[("p", 1.0)]), dict(sample_rate=16001), dict(sample_rate=4000)):
        with pytest.raises(ValueError):
            MF.MixAug(**{"sample_rate": 16000, **kw})


def test_check_table_raises_its_refusals():
    lengths = [10, 2000]
    good = MF.none_table(3)
    good[0] = [1, 1, 1999, 3.0, 0, 0]
    good[1] = [2, 0, 9, -20.0, 1, -23.0]
    assert MF.check_table(torch.from_numpy(good), lengths).dtype == np.float64
    rec = MF.records_from_table(MF.check_table(good, lengths))
    assert rec.dtype == MF.RECORD_DTYPE and rec["kind"].tolist() == [1, 2, 0] and rec["offset"].tolist() == [1999, 9, 0] and rec["db"][1] == -20.0
    assert MF.check_table(MF.none_table(2), None).shape == (2, 6)  # no background row: no bank needed

    def broken(r, c, v):
        t = good.copy()
        t[r, c] = v
        return t

    for bad in (broken(0, 0, 1.5), broken(0, 0, 3), broken(0, 0, -1), broken(0, 1, 2), broken(0, 1, 0.5), broken(0, 1, -1), broken(0, 2, 2000),
                broken(1, 2, 10), broken(0, 2, 0.5), broken(0, 2, -1), broken(0, 3, float("nan")), broken(0, 3, float("inf")), broken(0, 3, 250.0),
                broken(2, 4, 2), broken(2, 4, 0.5), broken(1, 5, float("nan")), broken(1, 5, -1000.0), broken(2, 1, float("inf")),
                good.astype(np.float32), good[:, :5], good[0]):
        with pytest.raises(ValueError):
            MF.check_table(bad, lengths)
    with pytest.raises(ValueError):
        MF.check_table(good, None)
    with pytest.raises(ValueError):
        MF.check_table(good, [])


# ------------------------------------------------------------------------------------------------------------ the bank
def test_bank_loading_refusals_name_order_and_synthetic(tmp_path):
    a, b, c = (np.arange(n, dtype=np.float32) / 100 for n in (5, 3, 7))
    np.save(tmp_path / "b_second.npy", b)
    np.save(tmp_path / "a_first.npy", a)
    np.save(tmp_path / "c_third.npy", c)
    (tmp_path / "notes.txt").write_text("not an entry")
    got = MF.load_bank(str(tmp_path))
    assert [e.tolist() for e in got] == [a.tolist(), b.tolist(), c.tolist()] and MF.bank_lengths(tmp_path) == [5, 3, 7]
    bank, off = MF.pack_bank(got)
    assert bank.dtype == np.float32 and bank.tolist() == np.concatenate([a, b, c]).tolist() and off.dtype == np.int64 and off.tolist() == [0, 5, 8, 15]
    assert MF.bank_lengths([a, b], 16000, 48000) == [2, 1] and MF.bank_lengths([c], 16000, 8000) == [14]  # ceil(m * 16000 / rate)
    assert [e.tolist() for e in MF.load_bank([a, torch.from_numpy(b)])] == [a.tolist(), b.tolist()]
    syn = MF.load_bank({"synthetic": 5, "seed": 3})
    again = MF.synthetic_bank(5, 16000, 3)
    assert [e.shape[0] for e in syn] == [48000, 120000, 496000, 196000, 48000] and all(np.array_equal(u, v) for u, v in zip(syn, again))
    assert all(e.dtype == np.float32 and 0.03 < float(np.sqrt(np.mean(e.astype(np.float64) ** 2))) < 0.07 for e in syn)
    assert not np.array_equal(MF.synthetic_bank(1, 16000, 0)[0], MF.synthetic_bank(1, 16000, 1)[0])
    empty = tmp_path / "empty"
    empty.mkdir()
    for bad in (str(empty), [], [np.zeros(0, dtype=np.float32)], [np.array([0.0, np.nan], dtype=np.float32)], [np.array([np.inf], dtype=np.float32)],
                [np.zeros((2, 3), dtype=np.float32)], [np.zeros(3, dtype=np.float64)], str(tmp_path / "missing"), {"synthetic": 2, "rate": 1},
                {"seed": 1}, {"synthetic": 1.5}, 7, None):
        with pytest.raises(ValueError):
            MF.load_bank(bad)
    with pytest.raises(ValueError):
        MF.MixAug(16000, background={"bank": [np.array([1.0, np.nan], dtype=np.float32)]})


# ------------------------------------------------------------------------------------------------------------ loader plumbing
def _dataset(**kw):
    return DL.AudioDataset(DL.SyntheticDataset(4, min_seconds=1.0), DL.SimpleTokenizer(), no_timestamp_training=True, spec_augment=True,
                           spec_augment_params={"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 0.5},
                           extremes_spec_augment=True, extremes_spec_augment_params={"low_freq_range": 5, "high_freq_range": 5}, **kw)


@pytest.mark.parametrize("stretch,office", [(False, False), (True, True)])
def test_items_gain_exactly_one_last_field_and_earlier_draws_are_untouched(stretch, office):
    kw = dict(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25) if stretch else {}
    if office:
        kw.update(office_aug=OFFICE, rate_aug={"alias": {"p": 1.0}}, filter_aug={"p": 1.0}, wave_aug={"noise": {"p": 1.0}})
    on, off = _dataset(mix_aug=BOTH, **kw), _dataset(**kw)
    base = 6 + int(stretch) + 4 * int(office)
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
        for u, v in zip(x[:base], y):  # everything shipped before is drawn BEFORE the mix effects: identical
            assert torch.equal(torch.as_tensor(u), torch.as_tensor(v))
        assert x[-1].dtype == torch.float64 and x[-1].shape == (6,) and x[-1][0] > 0 and x[-1][4] == 1
    ca, cb = DL.collate_fn(a), DL.collate_fn(b)
    assert len(ca) == base + 1 and ca[-1].shape == (3, 6)
    for u, v in zip(ca[:base], cb):
        assert torch.equal(u, v)
    MF.check_table(ca[-1], on.mix_aug.lengths)


def test_item_row_is_the_draw_after_the_office_effects():
    ds = _dataset(office_aug=OFFICE, mix_aug=BOTH)
    random.seed(77)
    item = ds[0]
    random.seed(77)
    OF.OfficeAug(16000, **OFFICE).draw()
    names, row = MF.MixAug(16000, **BOTH).draw(480000)
    assert names["background"] and names["loudness"] and np.array_equal(item[-1].numpy(), row) and len(item) == 8


def test_option_is_checked_and_the_pipelines_stay_refused_and_name_the_option():
    with pytest.raises(NotImplementedError, match="apply_advanced_aug") as e:
        _dataset(apply_advanced_aug=True, mix_aug=BOTH)
    assert "wft_mix_aug" in str(e.value) and "wft_office_aug" in str(e.value)
    with pytest.raises(NotImplementedError, match="apply_office_aug") as e2:
        _dataset(apply_office_aug=True)
    assert str(e2.value).replace("apply_office_aug", "X") == str(e.value).replace("apply_advanced_aug", "X")  # the same with and without an option
    for bad in (True, {"noise": {}}, {"loudness": {"p": 2.0}}, {"background": {}}, [("loudness", {})]):
        with pytest.raises(ValueError):
            _dataset(mix_aug=bad)
    assert _dataset().mix_aug is None and _dataset(mix_aug={}).mix_aug.p == {}
    ds = _dataset(mix_aug=BOTH)
    assert ds.mix_aug.lengths == [48000, 120000, 496000, 196000] and not hasattr(ds.mix_aug, "entries")  # the lengths only


def test_gpu_mel_loader_counts_the_field_and_dev_loaders_never_get_it():
    class FakeFrontend:
        device = torch.device("cpu")

    def loader(**kw):
        return DL.GpuMelLoader(torch.utils.data.DataLoader(_dataset(**kw), batch_size=2, collate_fn=DL.collate_fn), FakeFrontend(), True)

    for kw, n_fields in (({}, 7), (dict(apply_baseline_aug=True), 8), (dict(office_aug=OFFICE, apply_baseline_aug=True), 9)):
        ld = loader(mix_aug=BOTH, **kw)
        batch = next(iter(ld.loader))
        assert ld.mix_aug and len(batch) == n_fields
        fields = ld._all_fields(batch)
        assert len(fields) == 4 and (fields[0] is not None) == ("apply_baseline_aug" in kw)
        office = ld._office_field(batch)
        assert (office is not None) == ("office_aug" in kw) and (office is None or office.shape == (2, 2050))
        table, bank = ld._mix_field(batch)
        assert table.dtype == np.float64 and table.shape == (2, 6) and bool((table[:, 0] > 0).all() and (table[:, 4] == 1).all())
        assert bank is ld._bank and bank.lengths == [48000, 120000, 496000, 196000] and bank.bank.dtype == torch.float32
        assert bank.bank.shape == (sum(bank.lengths),) and bank.off.dtype == torch.int64 and bank.off.tolist() == [0, 48000, 168000, 664000, 860000]
    ld = loader(mix_aug={"background": {"p": 0.0, "bank": BANK}, "loudness": {"p": 0.0}})
    batch = next(iter(ld.loader))
    assert len(batch) == 7 and ld._mix_field(batch) is None  # nothing drawn: nothing to launch
    only = loader(mix_aug={"loudness": {"p": 1.0}})
    assert only._bank is None and only._mix_field(next(iter(only.loader)))[1] is None
    with pytest.raises(ValueError):
        loader(mix_aug=BOTH)._all_fields(next(iter(loader().loader)))
    assert loader().mix_aug is False and loader()._mix_field(next(iter(loader().loader))) is None
    import inspect

    src = inspect.getsource(__import__("whisper_finetune.scripts.finetune", fromlist=["main"]).main)
    assert src.count('aa.get("wft_mix_aug")') == 1  # the train loader alone reads the option


def test_debug_config_carries_the_option_and_its_block_builds():
    from pathlib import Path

    import yaml

    cfg = yaml.safe_load((Path(__file__).resolve().parents[1] / "configs" / "DEBUG_synthetic_mix.yaml").read_text())
    aa = cfg["augmentation"]["audio_augment"]
    assert aa["apply_advanced_aug"] is False and aa["apply_office_aug"] is False and set(aa["wft_mix_aug"]) == set(MF.STAGES)
    assert aa["wft_mix_aug"]["background"]["bank"] == {"synthetic": 4}
    ds = _dataset(mix_aug=aa["wft_mix_aug"], office_aug=aa["wft_office_aug"], rate_aug=aa["wft_rate_aug"], wave_aug=aa["wft_wave_aug"],
                  filter_aug=aa["wft_filter_aug"])
    assert ds.mix_aug.p == {"background": 0.5, "loudness": 0.5} and ds.mix_aug.kinds == ("absolute", "snr") and len(ds.mix_aug.lengths) == 4


# ------------------------------------------------------------------------------------------------------------ host checks
def test_wrappers_raise_before_the_device_is_touched():
    x = torch.zeros(2, 64)  # a host tensor: reaching the device would raise something else than ValueError
    bank, off = torch.zeros(10), torch.tensor([0, 4, 10])
    rec = M.bg_records([(1, 0, 0, 3.0), (2, 1, 5, -20.0)])
    for bad_audio in (x.double(), x[0], torch.zeros(0, 4), np.zeros((2, 4), dtype=np.float32)):
        with pytest.raises(ValueError):
            K.loudness(bad_audio)
        with pytest.raises(ValueError):
            K.bg_mix(bad_audio, bank, off, rec, lengths=[4, 6])
    for rate in (16001, 4000, 400000, 16000.5):
        with pytest.raises(ValueError):
            K.loudness(x, rate)
    for target in ([-20.0] * 3, 250.0, float("inf"), "loud"):
        with pytest.raises(ValueError):
            K.loudness(x, 16000, target)
    with pytest.raises(ValueError):
        K.loudness(x, 16000, -20.0, out=torch.zeros(2, 63))
    with pytest.raises(ValueError):
        y = torch.zeros(64, 2).t()  # stride(1) == 2: cannot run in place
        K.loudness(y, 16000, -20.0, out=y)
    for b, o in ((bank.double(), off), (bank[None], off), (torch.zeros(0), off), (bank, off.to(torch.int32)), (bank, off[:1]), (bank[::2], off)):
        with pytest.raises(ValueError):
            K.bg_mix(x, b, o, rec, lengths=[4, 6])
    for bad_rec in (M.bg_records([(3, 0, 0, 3.0), (0, 0, 0, 0.0)]), M.bg_records([(1, 2, 0, 3.0), (0, 0, 0, 0.0)]),
                    M.bg_records([(1, 0, 4, 3.0), (0, 0, 0, 0.0)]), M.bg_records([(1, 0, -1, 3.0), (0, 0, 0, 0.0)]),
                    M.bg_records([(2, 1, 0, float("nan")), (0, 0, 0, 0.0)]), rec[:1], np.zeros((2, 4))):
        with pytest.raises(ValueError):
            K.bg_mix(x, bank, off, bad_rec, lengths=[4, 6])
    with pytest.raises(ValueError):
        K.bg_mix(x, bank, off, rec, lengths=[4, 6, 1])
    with pytest.raises(ValueError):
        K.bg_mix(x, bank, torch.tensor([0, 4, 9]), rec)  # offsets that do not end at the bank's size
    with pytest.raises(ValueError):
        K.bg_mix(x, bank, off, rec, out=torch.zeros(2, 63), lengths=[4, 6])
    a = np.zeros((2, 16), dtype=np.float32)
    noise = np.ones(8, dtype=np.float32)
    for kw in (dict(), dict(snr_db=3.0, absolute_rms_db=-20.0), dict(snr_db=[3.0] * 3), dict(snr_db=3.0, offset=8), dict(snr_db=3.0, offset=-1),
               dict(snr_db=3.0, offset=0.5), dict(absolute_rms_db=float("inf"))):
        with pytest.raises(ValueError):
            GF.mix_background(a, noise, **kw)
    for bad_noise in ([noise] * 3, np.ones(8), np.ones((2, 8), dtype=np.float32), np.zeros(0, dtype=np.float32), [],
                      np.array([1.0, np.nan], dtype=np.float32)):
        with pytest.raises(ValueError):
            GF.mix_background(a, bad_noise, snr_db=3.0)
    for f in (lambda: GF.loudness(a.astype(np.float64)), lambda: GF.loudness(a, 12345), lambda: GF.loudness_normalize(a, [-20.0] * 3),
              lambda: GF.loudness_normalize(a, -20.0, 100), lambda: GF.loudness_normalize(a[0, :0], -20.0)):
        with pytest.raises(ValueError):
            f()
