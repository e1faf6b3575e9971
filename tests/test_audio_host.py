"""The audio front end's checker on the host (tests/_audio_cases.py): the width condition of the log-mel intervals from the float64
reference alone, two honest fp32 restatements inside every interval, the measured coordinate error behind E_IX, every mutant
rejected by at least one case, and the float64 references against the oracle (torch.stft, grid_sample, torch's bf16 cast)."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as O
from tests import _audio_cases as AC


@functools.lru_cache(maxsize=None)
def _banks():
    return AC.banks(O.mel_filters(80).numpy(), O.mel_filters(128).numpy())


@functools.lru_cache(maxsize=None)
def _case(n_frames, bank):
    """-> (clips f32 [5, n], (ref, lo, hi) float64 [5, n_mels, n_frames])"""
    xs = AC.clips(n_frames)
    return xs, AC.logmel_intervals(xs, _banks()[bank], n_frames)


SMALL = [c for c in AC.logmel_cases() if c[0] < 3000]


# ============================================================================================================ log-mel
def test_the_cases_are_the_issues():
    cases = list(AC.logmel_cases())
    assert {c[0] for c in cases} == {3, 16, 37, 3000} and (37, "identity") in cases and (37, "six") in cases and len(cases) == 10
    assert AC.clips(3).shape == (5, 480) and AC.CLIP_KINDS == ("decades", "burst", "quiet", "silent", "tail")
    six = AC.six_row_bank()
    assert not six[0].any() and np.flatnonzero(six[1]).tolist() == [0] and np.flatnonzero(six[2]).tolist() == [200]
    assert np.flatnonzero(six[3]).tolist() == [3, 150] and (six[4] != 0).all()
    nz = np.flatnonzero(six[5])
    assert abs(six[5, nz[-1]] / six[5].max() - 1e-3) < 1e-9
    assert max(np.count_nonzero(r) for b in ("mel80", "mel128") for r in _banks()[b]) <= 32    # the 32 u M of the derivation
    assert len(AC.LOGMEL_MUTANTS) == 11 and len(AC.SPECAUG_MUTANTS) == 7 and len(AC.LAYOUT_MUTANTS) == 3


def test_at_most_two_percent_of_a_clips_intervals_are_wider_than_1e_3():
    for n_frames, bank in AC.logmel_cases():
        _, (ref, lo, hi) = _case(n_frames, bank)
        assert (lo <= ref).all() and (ref <= hi).all()
        for i, kind in enumerate(AC.CLIP_KINDS):
            share, widest = AC.wide_share(lo[i], hi[i]), (hi[i] - lo[i]).max()
            line = f"{n_frames:5d} frames, {bank:8s} {kind:8s}: {100 * share:5.2f} % wider than 1e-3, widest {widest:.1e}"
            if bank == "six":
                rest, single = AC.wide_share(lo[i][[0, 3, 4, 5]], hi[i][[0, 3, 4, 5]]), AC.wide_share(lo[i][[1, 2]], hi[i][[1, 2]])
                print(f"{line} (single-bin rows {100 * single:.2f} %, the other rows {100 * rest:.2f} %)")
                assert rest <= AC.SHARE and single <= AC.SINGLE_BIN_SHARE and share <= AC.SIX_ROW_SHARE, line
            else:
                print(line)
                assert share <= (AC.IDENTITY_SHARE if bank == "identity" else AC.SHARE), line
            if kind == "silent":
                assert (ref[i] == -1.5).all() and widest < 3e-6


def test_the_honest_restatements_use_at_most_half_of_the_half_width():
    worst, worst_silent = 0.0, 0.0
    for n_frames, bank in AC.logmel_cases():
        xs, (ref, lo, hi) = _case(n_frames, bank)
        for form in (("seq", "fold") if n_frames < 3000 else ("blas",)):
            got = AC.emulate_logmel(xs, _banks()[bank], n_frames, form)
            assert got.dtype == np.float32 and got.shape == ref.shape
            assert AC.misses(got, lo, hi) == 0, (n_frames, bank, form)
            bare = (hi - lo) < 3e-6                       # M = 0 (silence, an all-zero filter row): the interval is the allowance alone
            assert bare[AC.CLIP_KINDS.index("silent")].all()
            used = AC.used_fraction(got[~bare], ref[~bare], lo[~bare], hi[~bare])
            worst, worst_silent = max(worst, used), max(worst_silent, AC.used_fraction(got[bare], ref[bare], lo[bare], hi[bare]))
            print(f"{n_frames:5d} frames, {bank:8s} {form:4s}: uses {used:.3f} of the half-width at worst")
    print(f"worst fraction of the half-width: {worst:.3f} (elements with M = 0: {worst_silent:.3f})")
    assert worst <= 0.5 and worst_silent <= 0.5


def test_a_nan_or_an_end_just_missed_fails():
    _, (ref, lo, hi) = _case(3, "mel80")
    got = ref.copy()
    assert AC.misses(got, lo, hi) == 0
    got[0, 0, 0] = np.nan
    got[1, 1, 1] = hi[1, 1, 1] + 1e-7
    got[2, 2, 2] = lo[2, 2, 2] - 1e-7
    assert AC.misses(got, lo, hi) == 3


def test_the_float64_reference_agrees_with_the_oracle_at_37_frames():
    for bank, n_mels in (("mel80", 80), ("mel128", 128)):
        xs, (ref, _, _) = _case(37, bank)
        want = O.log_mel_spectrogram(torch.from_numpy(xs), n_mels).numpy()
        assert want.shape == ref.shape
        d = np.abs(ref - want).max()
        print(f"{bank}: max |float64 reference - oracle| = {d:.2e}")
        assert d <= 1e-4


def _rejecting(mutant):
    out = []
    for n_frames, bank in SMALL:
        xs, (_, lo, hi) = _case(n_frames, bank)
        got = AC.emulate_logmel(xs, _banks()[bank], n_frames, "fold", mutant)
        per_clip = [AC.misses(got[i], lo[i], hi[i]) for i in range(5)]
        out += [f"{n_frames}/{bank}/{AC.CLIP_KINDS[i]}" for i in range(5) if per_clip[i]]
    return out


@pytest.mark.parametrize("mutant", AC.LOGMEL_MUTANTS)
def test_every_logmel_mutant_is_rejected(mutant):
    hit = _rejecting(mutant)
    print(f"{mutant}: rejected by {len(hit)} clips: {', '.join(hit[:12])}{' ...' if len(hit) > 12 else ''}")
    assert hit


# ============================================================================================================ SpecAugment
def _ix_oracle_order(T, warp_p, warp_d):
    """The oracle's time_warp up to the coordinate that grid_sample(align_corners=True) forms from its grid: its own torch fp32
    operations, line by line."""
    wp = torch.tensor([warp_p], dtype=torch.int64)
    wd = torch.tensor([warp_d], dtype=torch.int64)
    x = torch.stack([torch.tensor([0]), wp, torch.tensor([T - 1])], 1)
    y = torch.stack([torch.tensor([-1.0]), (wp - wd) * 2 / (T - 1.0) - 1.0, torch.tensor([1.0])], 1)
    xs = torch.linspace(0, T - 1, T).unsqueeze(0)
    m = (y[..., 1:] - y[..., :-1]) / (x[..., 1:] - x[..., :-1])
    m = torch.cat([m[..., [0]], (m[..., 1:] + m[..., :-1]) / 2, m[..., [-1]]], -1)
    idxs = torch.searchsorted(x[..., 1:], xs)
    dx = x.gather(dim=-1, index=idxs + 1) - x.gather(dim=-1, index=idxs)
    t = (xs - x.gather(dim=-1, index=idxs)) / dx
    tt = t.unsqueeze(-2) ** torch.arange(4).view(-1, 1)
    A = torch.tensor([[1, 0, -3, 2], [0, 1, -2, 1], [0, 0, 3, -2], [0, 0, -1, 1]], dtype=t.dtype)
    hh = A @ tt
    ys = (hh[..., 0, :] * y.gather(dim=-1, index=idxs) + hh[..., 1, :] * m.gather(dim=-1, index=idxs) * dx
          + hh[..., 2, :] * y.gather(dim=-1, index=idxs + 1) + hh[..., 3, :] * m.gather(dim=-1, index=idxs + 1) * dx)
    assert ys.dtype == torch.float32
    return (((ys + 1) / 2) * (T - 1))[0].numpy()


def test_the_restated_coordinate_is_the_oracles():
    """A one-row ramp through the oracle's time_warp is its coordinate (to the rounding of grid_sample's two products)."""
    for T in (257, 300):
        for wp, wd in AC.warp_params(T):
            ix = _ix_oracle_order(T, wp, wd).astype(np.float64)
            got = O.time_warp(torch.arange(T, dtype=torch.float32)[None], wp, wd)[0].numpy().astype(np.float64)
            inside = (ix >= 0) & (ix <= T - 1)
            assert inside.sum() > T // 2 and np.abs(got - ix)[inside].max() <= 8 * AC.U * T


def test_E_IX_is_four_times_the_measured_coordinate_error():
    assert AC.warp_W(2) is None and AC.warp_params(2) == [] and [AC.warp_W(T) for T in AC.SPEC_T[1:]] == [80, 80, 80]
    worst = 0.0
    print("    T       oracle's order    kernel's order")
    for T in AC.SPEC_T[1:]:
        assert AC.warp_params(T) == [(p, d) for p in (80, T // 2, T - 81) for d in (-80, 0, 79)]
        o = k = 0.0
        for wp, wd in AC.warp_params(T):
            ix = AC.warp_ix64(T, wp, wd)
            assert ix[0] == 0.0 and ix[-1] == T - 1.0
            o = max(o, np.abs(_ix_oracle_order(T, wp, wd).astype(np.float64) - ix).max())
            k = max(k, np.abs(AC.warp_ix32(T, wp, wd).astype(np.float64) - ix).max())
        print(f"    {T:<7d} {o:<17.1e} {k:.1e}")
        # the numpy column is the same on every machine; torch's pow and matmul may round differently from build to build
        assert f"    {T:<7d} {AC.IX_TABLE[T][0]:<17.1e} {k:.1e}" in AC.__doc__ and AC.IX_TABLE[T][1] == float(f"{k:.1e}")
        assert abs(o - AC.IX_TABLE[T][0]) <= 0.2 * AC.IX_TABLE[T][0]
        worst = max(worst, o, k)
    want = 2.0 ** math.ceil(math.log2(4 * worst))
    print(f"worst {worst:.2e}, 4 x worst {4 * worst:.2e} -> E_IX = {want}")
    assert AC.E_IX == want


def _spec_cases():
    for T in AC.SPEC_T:
        for i, (params, ext) in enumerate(AC.specaug_batches(T)):
            yield T, i, AC.ramps(T, first_clip=i), params, ext


def test_the_specaug_cases_are_the_issues():
    for T in AC.SPEC_T:
        batches = AC.specaug_batches(T)
        seen = set()
        for params, ext in batches:
            assert params.shape == (3, 8) and ext.tolist() == [[2, 3], [0, 0], [0, 0]]
            assert (params[:, 0] == 0).sum() == (3 if T == 2 else 1)
            seen |= {(int(p[1]), int(p[2])) for p in params if p[0]}
            assert params[1, 3] == params[1, 4] and params[1, 5:7].tolist() == [3, 9]
            if T > 256:
                assert params[0, 3] == 250 and params[0, 4] == min(262, T)
        assert seen == set(AC.warp_params(T))
    assert {tuple(b[0][:, 0] == 0) for b in AC.specaug_batches(300)} == {(True, False, False), (False, True, False), (False, False, True)}


def test_the_honest_specaug_restatement_meets_the_bound():
    worst = 0.0
    for T, i, x, params, ext in _spec_cases():
        want, bound = AC.specaug_expected(x, params, ext)
        got = AC.emulate_specaug(x, params, ext)
        assert AC.violations(got, want, bound) == 0, (T, i)
        live = bound > 0
        if live.any():
            worst = max(worst, float((np.abs(got - want)[live] / bound[live]).max()))
        for b in range(3):
            if not params[b, 0]:
                keep = ~AC._masked(16, T, params[b], ext[b])
                assert np.array_equal(got[b][keep], x[b][keep]) and (bound[b] == 0).all()
    print(f"honest restatement: worst |got - want| / bound = {worst:.3f}")
    assert worst <= 0.5


def test_the_specaug_reference_agrees_with_the_oracle():
    """The random-valued spectrograms through O.spec_augment: the float64 reference and the fp32 restatement both within 1e-3.
    (The ramps are not put through the oracle: grid_sample rounds the ROW coordinate too, which mixes 1e-6 of a neighbouring row
    of opposite slope into values of several thousand.)"""
    for T in AC.SPEC_T:
        params, ext = AC.specaug_batches(T)[0]
        r = AC.random_spectrogram(T)
        assert np.abs(r).max() <= AC.SPEC_RANDOM_AMP and 4 * AC.SPEC_RANDOM_AMP * AC.E_IX <= 1e-3
        want = AC.specaug_expected(r, params, ext)[0]
        got = AC.emulate_specaug(r, params, ext)
        for b in range(3):
            p = params[b]
            args = ((int(p[1]), int(p[2])) if p[0] else None, (int(p[3]), int(p[4])), (int(p[5]), int(p[6])), tuple(int(v) for v in ext[b]))
            ref = O.spec_augment(torch.from_numpy(r[b]), *args).numpy().astype(np.float64)
            d_ref, d_got = np.abs(ref - want[b]).max(), np.abs(ref - got[b]).max()
            print(f"T = {T}, clip {b}: max |oracle - float64 reference| = {d_ref:.1e}, max |oracle - fp32 restatement| = {d_got:.1e}")
            assert d_ref < 1e-3 and d_got < 1e-3, (T, b)


def _specaug_rejecting(mutant):
    out = []
    for T, i, x, params, ext in _spec_cases():
        want, bound = AC.specaug_expected(x, params, ext)
        if AC.violations(AC.emulate_specaug(x, params, ext, mutant), want, bound):
            out.append(f"T={T}/batch {i}")
    return out


@pytest.mark.parametrize("mutant", AC.SPECAUG_MUTANTS)
def test_every_specaug_mutant_is_rejected(mutant):
    hit = _specaug_rejecting(mutant)
    print(f"{mutant}: rejected by {', '.join(hit)}")
    assert hit


@pytest.mark.parametrize("mutant", ["nearest_neighbour", "align_corners_false", "middle_slope_is_left_secant"])
def test_the_random_spectrogram_at_1e_3_rejects_the_sampling_mutants(mutant):
    hit = []
    for T in AC.SPEC_T[1:]:
        params, ext = AC.specaug_batches(T)[0]
        r = AC.random_spectrogram(T)
        if np.abs(AC.emulate_specaug(r, params, ext, mutant).astype(np.float64) - AC.emulate_specaug(r, params, ext)).max() >= 1e-3:
            hit.append(T)
    assert hit == list(AC.SPEC_T[1:])


# ============================================================================================================ layout
def test_the_layout_reference_is_torchs_bf16_cast():
    assert AC.LAYOUT_SHAPES == ((2, 80, 300, 128), (1, 128, 65, 128), (3, 16, 1, 128), (1, 80, 64, 96), (2, 5, 63, 8))
    for B, n_mels, T, c_pad in AC.LAYOUT_SHAPES:
        x = AC.layout_input(B, n_mels, T)
        assert np.isfinite(x).all()
        mag = np.abs(x[x != 0]).astype(np.float64)
        assert B * n_mels * T < 100 or mag.max() / mag.min() > 1e6
        bits = x.view(np.uint32)
        for special in (0x3F808000, 0x3F818000, 0x7F7F0000, 0x00000000, 0x80000000):
            assert (bits == special).any(), hex(special)
        want = AC.layout_expected(x, c_pad)
        ref = torch.zeros((B, T + 2, c_pad), dtype=torch.bfloat16)
        ref[:, 1:T + 1, :n_mels] = torch.from_numpy(x).transpose(1, 2).to(torch.bfloat16)
        assert np.array_equal(ref.view(torch.int16).numpy().view(np.uint16), want)
    assert AC.bf16_rne(np.array([0x3F808000, 0x3F818000, 0x7F7E8000], dtype=np.uint32).view(np.float32)).tolist() == [0x3F80, 0x3F82, 0x7F7E]


@pytest.mark.parametrize("mutant", AC.LAYOUT_MUTANTS)
def test_every_layout_mutant_is_rejected(mutant):
    hit = []
    for B, n_mels, T, c_pad in AC.LAYOUT_SHAPES:
        x = AC.layout_input(B, n_mels, T)
        if not np.array_equal(AC.layout_expected(x, c_pad, mutant), AC.layout_expected(x, c_pad)):
            hit.append((B, n_mels, T, c_pad))
    print(f"{mutant}: rejected by {hit}")
    assert hit
