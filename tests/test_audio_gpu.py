"""wft_logmel, wft_specaug and wft_mel_to_tmajor_bf16 on the GPU (csrc/audio.hip), judged by the checker of tests/_audio_cases.py:
every log-mel element inside its derived interval, every warped ramp element under its bound, the layout bit for bit; all into
poisoned outputs with poison behind their ends, a garbage workspace, clips of a batch against the same clips alone, the Python
wrappers against the raw calls, and the argument errors."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests import _audio_cases as AC  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = torch.device("cuda:0")
TAIL = 4096


def _p(t):
    return C.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _banks():
    return AC.banks(O.mel_filters(80).numpy(), O.mel_filters(128).numpy())


def _poisoned(shape, dtype=torch.float32):
    """-> (flat, view): `view` of the given shape at the front of a buffer that is poison throughout and TAIL elements longer."""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        flat = torch.full((n + TAIL,), float("nan"), device=DEV)
    else:
        flat = torch.full((n + TAIL,), AC.POISON_BF16, dtype=torch.int16, device=DEV)
    return flat, flat[:n].view(shape)


def _tail_is_poison(flat, n):
    tail = flat[n:]
    return bool(torch.isnan(tail).all()) if flat.dtype == torch.float32 else bool((tail == AC.POISON_BF16).all())


# ============================================================================================================ log-mel
def _raw_logmel(xs, filt, n_frames, clipmax=None):
    """One wft_logmel call into a NaN-filled output; the workspace comes in holding garbage.  -> (out, flat, clipmax)"""
    B, n = xs.shape
    flat, out = _poisoned((B, filt.shape[0], n_frames))
    if clipmax is None:
        clipmax = torch.full((B,), 3.0e38, device=DEV)      # as unsigned bits: above every (mx + 20)
    L.check(L.load().wft_logmel(_p(xs), _p(filt), _p(out), _p(clipmax), B, n, filt.shape[0], n_frames, L.stream_ptr()), "wft_logmel")
    return out, flat, clipmax


@pytest.mark.parametrize("n_frames,bank", list(AC.logmel_cases()))
def test_logmel_every_element_inside_its_interval(n_frames, bank):
    xs_h, filt_h = AC.clips(n_frames), _banks()[bank]
    ref, lo, hi = AC.logmel_intervals(xs_h, filt_h, n_frames)
    xs, filt = _dev(xs_h), _dev(filt_h)
    out, flat, clipmax = _raw_logmel(xs, filt, n_frames)
    got = out.cpu().numpy()
    assert _tail_is_poison(flat, out.numel()), "wft_logmel wrote behind the end of its output"
    for i, kind in enumerate(AC.CLIP_KINDS):
        bad = AC.misses(got[i], lo[i], hi[i])
        used = AC.used_fraction(got[i], ref[i], lo[i], hi[i])
        print(f"{n_frames} frames, {bank}, {kind}: {bad} of {got[i].size} outside, uses {used:.3f} of its side of the interval at worst")
        assert bad == 0, (n_frames, bank, kind, bad)
    # the same case again into the workspace the first run left behind: bit-equal
    again, flat2, _ = _raw_logmel(xs, filt, n_frames, clipmax)
    assert torch.equal(again, out) and _tail_is_poison(flat2, out.numel())
    # every clip alone
    for i, kind in enumerate(AC.CLIP_KINDS):
        one, flat1, _ = _raw_logmel(xs[i:i + 1].clone(), filt, n_frames)
        assert torch.equal(one[0], out[i]) and _tail_is_poison(flat1, one.numel()), f"clip {i} ({kind}) differs from the same clip at B = 1"


def test_logmel_wrapper_is_the_raw_call():
    for n_frames, bank in ((37, "mel80"), (3, "mel128")):
        xs, filt = _dev(AC.clips(n_frames)), _dev(_banks()[bank])
        raw = _raw_logmel(xs, filt, n_frames)[0]
        assert torch.equal(K.logmel(xs, filt, n_frames), raw)


# ============================================================================================================ SpecAugment
def _raw_specaug(x, params, ext):
    flat, out = _poisoned(tuple(x.shape))
    B, n_mels, T = x.shape
    L.check(L.load().wft_specaug(_p(x), _p(out), _p(params), _p(ext), B, n_mels, T, L.stream_ptr()), "wft_specaug")
    return out, flat


@pytest.mark.parametrize("T", AC.SPEC_T)
def test_specaug_ramps_under_the_bound(T):
    worst = 0.0
    for i, (params_h, ext_h) in enumerate(AC.specaug_batches(T)):
        x_h = AC.ramps(T, first_clip=i)
        want, bound = AC.specaug_expected(x_h, params_h, ext_h)
        x, params, ext = _dev(x_h), _dev(params_h), _dev(ext_h)
        out, flat = _raw_specaug(x, params, ext)
        got = out.cpu().numpy()
        assert _tail_is_poison(flat, out.numel()), "wft_specaug wrote behind the end of its output"
        bad = AC.violations(got, want, bound)
        live = bound > 0
        if live.any():
            worst = max(worst, float(np.nan_to_num(np.abs(got - want)[live] / bound[live], nan=np.inf).max()))
        assert bad == 0, f"T = {T}, batch {i}: {bad} elements miss the bound"
        for b in range(AC.SPEC_B):
            if not params_h[b, 0]:                      # unwarped: the input's bits where nothing is masked, zeros elsewhere
                keep = ~AC._masked(AC.SPEC_MELS, T, params_h[b], ext_h[b])
                assert np.array_equal(got[b][keep].view(np.uint32), x_h[b][keep].view(np.uint32)) and (got[b][~keep] == 0).all()
            one, flat1 = _raw_specaug(x[b:b + 1].clone(), params[b:b + 1].clone(), ext[b:b + 1].clone())
            assert torch.equal(one[0], out[b]) and _tail_is_poison(flat1, one.numel()), f"T = {T}, batch {i}: clip {b} differs at B = 1"
        if i == 0:
            assert torch.equal(K.specaug(x, params, ext), out)
    print(f"T = {T}: worst |got - want| / bound = {worst:.3f}")


@pytest.mark.parametrize("T", AC.SPEC_T)
def test_specaug_random_values_against_the_oracle(T):
    params_h, ext_h = AC.specaug_batches(T)[0]
    r_h = AC.random_spectrogram(T)
    out, flat = _raw_specaug(_dev(r_h), _dev(params_h), _dev(ext_h))
    got = out.cpu()
    assert _tail_is_poison(flat, out.numel())
    for b in range(AC.SPEC_B):
        p = params_h[b]
        ref = O.spec_augment(torch.from_numpy(r_h[b]), (int(p[1]), int(p[2])) if p[0] else None, (int(p[3]), int(p[4])), (int(p[5]), int(p[6])),
                             tuple(int(v) for v in ext_h[b]))
        d = (got[b] - ref).abs().max().item()
        print(f"T = {T}, clip {b}: max |got - oracle| = {d:.1e}")
        assert d < 1e-3, (T, b, d)
        dead = torch.from_numpy(AC._masked(AC.SPEC_MELS, T, p, ext_h[b]))
        assert (got[b][dead] == 0).all() and (p[0] or torch.equal(got[b], ref))


def test_specaug_without_extremes_is_extremes_zero():
    params_h, _ = AC.specaug_batches(300)[0]
    x, params = _dev(AC.ramps(300)), _dev(params_h)
    zero = torch.zeros((AC.SPEC_B, 2), dtype=torch.int32, device=DEV)
    assert torch.equal(K.specaug(x, params), _raw_specaug(x, params, zero)[0])


# ============================================================================================================ layout
def _raw_layout(x, c_pad):
    B, n_mels, T = x.shape
    flat, out = _poisoned((B, T + 2, c_pad), torch.int16)
    L.check(L.load().wft_mel_to_tmajor_bf16(_p(x), _p(out), B, n_mels, T, c_pad, L.stream_ptr()), "wft_mel_to_tmajor_bf16")
    return out, flat


@pytest.mark.parametrize("B,n_mels,T,c_pad", AC.LAYOUT_SHAPES)
def test_layout_bit_for_bit_into_poisoned_memory(B, n_mels, T, c_pad):
    x_h = AC.layout_input(B, n_mels, T)
    want = AC.layout_expected(x_h, c_pad)
    x = _dev(x_h)
    out, flat = _raw_layout(x, c_pad)
    got = out.cpu().numpy().view(np.uint16)
    assert _tail_is_poison(flat, out.numel()), "wft_mel_to_tmajor_bf16 wrote behind the end of its output"
    assert (got[:, 0] == 0).all() and (got[:, T + 1] == 0).all(), "halo rows"
    assert (got[:, :, n_mels:] == 0).all(), "pad channels"
    wrong = np.argwhere(got != want)
    assert wrong.shape[0] == 0, f"{wrong.shape[0]} elements differ, the first at {wrong[0]}: got {got[tuple(wrong[0])]:#06x}, want {want[tuple(wrong[0])]:#06x}"
    assert torch.equal(K.mel_to_tmajor(x, c_pad).view(torch.int16), out)


# ============================================================================================================ argument errors
def test_argument_errors_raise_and_launch_nothing():
    lib = L.load()
    xs, filt = _dev(AC.clips(4)), _dev(_banks()["mel80"])
    flat, out = _poisoned((5, 80, 4))
    clipmax = torch.full((5,), 7.0, device=DEV)
    for what, n, n_frames in (("n_samples != 160 * n_frames", 480, 4), ("n_samples != 160 * n_frames", 640, 3), ("n_samples = 400", 400, 2),
                              ("n_samples = 400", 400, 3)):
        with pytest.raises(L.WftError, match="wft_logmel"):
            L.check(lib.wft_logmel(_p(xs), _p(filt), _p(out), _p(clipmax), 5, n, 80, n_frames, L.stream_ptr()), "wft_logmel")
    torch.cuda.synchronize()
    assert torch.isnan(flat).all() and (clipmax == 7.0).all(), "a refused wft_logmel must not launch"

    x = _dev(AC.ramps(300))
    params = _dev(AC.specaug_batches(300)[0][0])
    ext = _dev(AC.specaug_batches(300)[0][1])
    keep = x.clone()
    flat, out = _poisoned((3, 16, 300))
    with pytest.raises(L.WftError, match="wft_specaug"):                      # in == out
        L.check(lib.wft_specaug(_p(x), _p(x), _p(params), _p(ext), 3, 16, 300, L.stream_ptr()), "wft_specaug")
    with pytest.raises(L.WftError, match="wft_specaug"):                      # T = 1
        L.check(lib.wft_specaug(_p(x), _p(out), _p(params), _p(ext), 3, 16, 1, L.stream_ptr()), "wft_specaug")
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and torch.isnan(flat).all(), "a refused wft_specaug must not launch"

    flat, out = _poisoned((3, 302, 8), torch.int16)
    with pytest.raises(L.WftError, match="wft_mel_to_tmajor_bf16"):           # c_pad < n_mels
        L.check(lib.wft_mel_to_tmajor_bf16(_p(x), _p(out), 3, 16, 300, 8, L.stream_ptr()), "wft_mel_to_tmajor_bf16")
    torch.cuda.synchronize()
    assert (flat == AC.POISON_BF16).all(), "a refused wft_mel_to_tmajor_bf16 must not launch"
    with pytest.raises(L.WftError):
        K.mel_to_tmajor(x, 8)
