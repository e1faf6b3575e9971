"""Resampling on the host: the polyphase table against the reference's weights, the reference against scipy (and torchaudio when
it is installed), a numpy emulation of the kernel under the derived bound with every mutant rejected, and the host logic of the
Python surface (rate validation, AudioDataset padding, the sampling_rate mismatch, transcribe's sample_rate keyword)."""
import math

import numpy as np
import pytest
import torch

from tests import _resample_cases as RC
from tests.test_transcribe_host import EOT, FRAMES, SOTS, _Model, _Stand, _run
from whisper_finetune.data import gpu_frontend as G
from whisper_finetune.data.data_loader import AudioDataset, SimpleTokenizer, get_dataloader
from whisper_finetune.engine import lib as L
from whisper_finetune.engine import transcribe as T


# ============================================================================= the table
@pytest.mark.parametrize("orig,new", RC.PAIRS)
def test_the_table_is_the_f32_rounding_of_the_reference_weights(orig, new):
    taps, o, n, width = G.resample_taps(orig, new)
    ro, rn, base, rwidth = RC.geometry(orig, new)
    assert (o, n, width) == (ro, rn, rwidth) and taps.dtype == torch.float32 and tuple(taps.shape) == (n, 2 * width)
    if new == 16000 and orig in RC.TAPS:
        assert 2 * width == RC.TAPS[orig]
    got = taps.numpy()
    w = RC.weights(orig, new)
    want = w.astype(np.float32)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all(), "more than one f32 ulp from the reference"
    # the entries outside the window |t| < 6 are exact zeros
    k = np.arange(-width + 1, width + 1, dtype=np.float64)[None, :]
    t = (k - np.arange(n, dtype=np.float64)[:, None] / n) * base / o
    outside = np.abs(t) >= 6.0
    assert outside.any() and (got[outside] == 0.0).all()
    assert G.resample_taps(orig, new)[0] is taps                       # cached per pair
    assert G.resample_taps(orig * 3, new * 3)[0] is taps               # ... per REDUCED pair


def test_resample_taps_rejects_bad_pairs():
    for bad in ((0, 1), (3, 0), (-3, 1), (3.0, 1), (True, 1)):
        with pytest.raises(ValueError):
            G.resample_taps(*bad)


# ============================================================================= the reference against other implementations
@pytest.mark.parametrize("orig,new", RC.PAIRS)
def test_the_reference_agrees_with_scipy_resample_poly(orig, new):
    signal = pytest.importorskip("scipy.signal")
    o, n, base, width = RC.geometry(orig, new)
    # the prototype filter on the grid of the up-sampled signal: H[i] = g(i * base / (o * n)), odd length, centred
    half = width * n
    i = np.arange(-half, half + 1, dtype=np.float64)
    H = RC.g(i * base / (o * n), base, o)
    for n_in in RC.lengths(orig, new):
        x = RC.signal(n_in, seed=n_in).astype(np.float64)
        want = signal.resample_poly(x, n, o, window=H / n)
        got = RC.definition(x, orig, new)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12, (orig, new, n_in, np.abs(got - want).max())


@pytest.mark.parametrize("orig,new", RC.PAIRS)
def test_the_reference_agrees_with_torchaudio(orig, new):
    F = pytest.importorskip("torchaudio.functional")
    for n_in in RC.lengths(orig, new):
        x = RC.signal(n_in, seed=n_in).astype(np.float64)
        want = F.resample(torch.from_numpy(x), orig, new).numpy()
        assert np.abs(RC.definition(x, orig, new) - want).max() <= 1e-12


@pytest.mark.parametrize("orig,new", RC.PAIRS)
def test_the_polyphase_form_is_the_definition(orig, new):
    """The float64 polyphase sum over the reference's (unrounded) weights equals the direct sum of the definition."""
    o, n, _, width = RC.geometry(orig, new)
    w = RC.weights(orig, new)
    for n_in in RC.lengths(orig, new):
        x = RC.signal(n_in, seed=n_in)
        ms = np.arange(RC.n_out_of(n_in, o, n), dtype=np.int64)
        j0, r = (ms * o) // n, (ms * o) % n
        j = j0[:, None] + np.arange(-width + 1, width + 1)[None, :]
        poly = (w[r] * RC._take(x.astype(np.float64), j)).sum(axis=1)
        want = RC.definition(x, orig, new)
        assert np.abs(poly - want).max() <= 1e-13 * max(1.0, np.abs(x).max())


# ============================================================================= the emulated kernel and its mutants
def _cases():
    """(orig, new, x) over the issue's rates and lengths: three decades of random input, plus a constant at the longest length."""
    for orig, new in RC.PAIRS:
        for n_in in RC.lengths(orig, new):
            yield orig, new, RC.signal(n_in, seed=1000 + n_in)
        yield orig, new, RC.signal(RC.lengths(orig, new)[-1], 0, kind="constant")


def _mutant_misses(mutant, orig, new, x, ms=None):
    """Violations of the bound by one mutant on one case (a wrong length counts as a miss)."""
    taps = G.resample_taps(orig, new)[0].numpy()
    ref, bound = RC.ref_on_table(x, taps, orig, new, ms)
    table = taps
    if mutant == "r_over_o":
        table = RC.weights(orig, new, r_over="o").astype(np.float32)
    elif mutant == "scale_missing":
        table = RC.weights(orig, new, scale=False).astype(np.float32)
    got = RC.emulate(x, table, orig, new, ms, mutant=mutant)
    if got.shape != ref.shape:
        return 1
    return RC.violations(got, ref, bound)


def test_the_emulated_kernel_meets_the_bound():
    worst = 0.0
    for orig, new, x in _cases():
        taps = G.resample_taps(orig, new)[0].numpy()
        ref, bound = RC.ref_on_table(x, taps, orig, new)
        got = RC.emulate(x, taps, orig, new)
        assert got.shape == ref.shape == (RC.n_out_of(x.shape[0], *RC.reduced(orig, new)),)
        assert RC.violations(got, ref, bound) == 0, (orig, new, x.shape[0])
        worst = max(worst, RC.worst_ratio(got, ref, bound))
    print(f"emulated kernel: worst |got - ref| / bound = {worst:.3f}")
    assert worst < 1.0


@pytest.fixture(scope="module")
def long_case():
    """44 100 -> 16 000 over 14 000 000 samples: m * 441 passes 2^31 at m = 4 869 621."""
    x = RC.signal(14_000_000, seed=5)
    m_c = 2 ** 31 // 441
    ms = np.concatenate([np.arange(m_c - 50, m_c + 50), np.arange(RC.n_out_of(x.shape[0], 441, 160) - 20, RC.n_out_of(x.shape[0], 441, 160))])
    return x, ms


@pytest.mark.parametrize("mutant", RC.MUTANTS)
def test_every_mutant_is_rejected(mutant, long_case):
    assert len(RC.MUTANTS) >= 10
    if mutant == "phase_32bit":
        x, ms = long_case
        assert _mutant_misses(None, 44100, 16000, x, ms) == 0
        assert _mutant_misses(mutant, 44100, 16000, x, ms) > 0
        return
    missed = sum(_mutant_misses(mutant, orig, new, x) > 0 for orig, new, x in _cases())
    print(f"{mutant}: rejected on {missed} cases")
    assert missed > 0


def test_the_64_bit_phase_reference_points(long_case):
    x, ms = long_case
    taps = G.resample_taps(44100, 16000)[0].numpy()
    ref, bound = RC.ref_on_table(x, taps, 44100, 16000, ms)
    assert RC.violations(RC.emulate(x, taps, 44100, 16000, ms), ref, bound) == 0
    assert (ms[:100] * 441 < 2 ** 31).any() and (ms[:100] * 441 >= 2 ** 31).any()
    # ... and the reference at sampled outputs is the reference
    assert np.abs(ref - RC.definition(x, 44100, 16000, ms)).max() <= 1e-5 * np.abs(ref).max()


# ============================================================================= the C ABI's host side
def test_the_tile_query_is_a_pure_host_function():
    lib = L.load()
    for orig, new in RC.PAIRS:
        o, n, _, width = RC.geometry(orig, new)
        tile = lib.wft_resample_tile(o, n, width)
        assert 4 <= tile <= 1024 and tile % 4 == 0
        # the staged span of a tile fits the 8192-float buffer
        assert ((n - 1) + (tile - 1) * o) // n + 2 * width + 6 <= 8192
    assert lib.wft_resample_tile(3, 1, 19) == 1024 and lib.wft_resample_tile(24, 1, 146) < 1024
    assert lib.wft_resample_tile(5000, 1, 30304) == 0 and lib.wft_resample_tile(0, 1, 7) == 0


# ============================================================================= host logic of the Python surface
def test_rate_validation():
    assert G.check_rate(16000) == 16000 and G.check_rate(np.int64(44100)) == 44100 and G.check_rate(1000) == 1000 and G.check_rate(384000) == 384000
    for bad in (999, 384001, 0, -16000, 16000.0, "16000", None, True):
        with pytest.raises(ValueError):
            G.check_rate(bad)
        with pytest.raises(ValueError):
            G.resample(np.zeros(10, dtype=np.float32), bad, device="cpu")
    with pytest.raises(ValueError):
        G.resample(np.zeros(10, dtype=np.float64), 48000, device="cpu")           # f32 only
    with pytest.raises(ValueError):
        G.resample(np.zeros((1, 2, 3), dtype=np.float32), 48000, device="cpu")    # 1-D or 2-D
    # 16 kHz is the identity: nothing is launched, a host tensor can pass through
    x = torch.arange(5, dtype=torch.float32)
    assert torch.equal(G.resample(x, 16000, device="cpu"), x)


class _DS(list):
    column_names = ["audio", "text", "language", "prompt"]


def _rec(n, rate=None):
    audio = {"array": np.full(n, 0.5, dtype=np.float32)}
    if rate is not None:
        audio["sampling_rate"] = rate
    return {"audio": audio, "text": "abc", "language": "de", "prompt": ""}


def test_audio_dataset_pads_to_thirty_seconds_at_its_rate():
    tok = SimpleTokenizer()
    ds = AudioDataset(_DS([_rec(480000, 48000), _rec(1000)]), tok, sample_rate=48000)
    a0, a1 = ds[0][0], ds[1][0]
    assert tuple(a0.shape) == tuple(a1.shape) == (30 * 48000,)
    assert (a0[:480000] == 0.5).all() and (a0[480000:] == 0).all() and (a1[:1000] == 0.5).all() and (a1[1000:] == 0).all()
    # a clip longer than 30 s at that rate: negative padding raises, as at 16 kHz
    with pytest.raises(ValueError):
        AudioDataset(_DS([_rec(30 * 48000 + 1)]), tok, sample_rate=48000)[0]
    with pytest.raises(ValueError):
        AudioDataset(_DS([_rec(480001)]), tok)[0]
    # the default is the path of before
    assert tuple(AudioDataset(_DS([_rec(1000, 16000)]), tok)[0][0].shape) == (480000,)
    for bad in (500, 44100.0):
        with pytest.raises(ValueError):
            AudioDataset(_DS([_rec(10)]), tok, sample_rate=bad)
    with pytest.raises(ValueError, match="48000"):       # the per-clip form is 16 kHz only: it refuses before it touches a device
        ds._calculate_mel(np.zeros(1440000, dtype=np.float32), None, False)


def test_a_record_at_another_rate_than_the_loaders_raises_naming_both():
    tok = SimpleTokenizer()
    with pytest.raises(ValueError, match=r"48000.*16000"):
        AudioDataset(_DS([_rec(480000, 48000)]), tok)[0]       # the silent 10 s-as-30 s case of before
    with pytest.raises(ValueError, match=r"16000.*44100"):
        AudioDataset(_DS([_rec(1000, 16000)]), tok, sample_rate=44100)[0]


def test_the_cpu_loader_yields_the_padded_native_rate_clips():
    loader = get_dataloader(_DS([_rec(700, 8000), _rec(900, 8000)]), SimpleTokenizer(), batch_size=2, shuffle=False, device=torch.device("cpu"),
                            sample_rate=8000)
    audio = next(iter(loader))[0]
    assert tuple(audio.shape) == (2, 240000) and (audio[0, :700] == 0.5).all() and (audio[0, 700:] == 0).all()


def test_transcribe_accepts_and_validates_sample_rate():
    # one rate, or one per recording; with the content frames standing in nothing is resampled and the loop is the one of before
    base, _ = _run()
    for rate in (16000, 48000, [48000, 44100, 8000], (16000, 16000, 22050), np.array([48000, 44100, 8000])):
        res, stand = _run(sample_rate=rate)
        assert res == base and [c["rows"] for c in stand.calls] == [[0, 1, 2], [0, 1], [0]]
    m = _Model()
    for bad in (999, 384001, 16000.0, "48000", None, True, [48000, 44100], [48000, 44100, 8000, 8000], [48000, 44100, 1.5]):
        with pytest.raises(ValueError):
            T.transcribe(m, [None, None, None], sot_sequence=SOTS, eot=EOT, _frames=FRAMES, _decode=_Stand(), sample_rate=bad)


def test_content_frames_at_another_rate():
    # ceil(len * 16000 / rate) // 160 — what long_logmel makes of the resampled recording
    for n_in, rate, want in ((9 * 48000, 48000, 900), (31 * 44100, 44100, 3100), (48000 * 9 + 100, 48000, 900), (8000, 8000, 100), (441, 44100, 1)):
        o, n = RC.reduced(rate, 16000)
        assert RC.n_out_of(n_in, o, n) // 160 == want == math.ceil(n_in * 16000 / rate) // 160
