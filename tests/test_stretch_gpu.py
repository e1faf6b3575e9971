"""Time stretch on the device: the three stages of csrc/stretch.hip one by one, the whole call, wft_logmel_ragged and the loader.
References, bounds and cases: tests/_stretch_cases.py (float64 numpy; the constant of the bound is chosen there, on the CPU)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _stretch_cases as S  # noqa: E402
from whisper_finetune.data import data_loader as DL  # noqa: E402
from whisper_finetune.data import gpu_frontend as GF  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = torch.device("cuda:0")
INPUTS = S.inputs()
RATES = S.rates()
SENT = 777.25          # exact in fp32, far from every value a stage writes
GUARD = 64


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return L.stream_ptr()


@functools.lru_cache(maxsize=None)
def _ref(name, rate):
    return S.allowance(INPUTS[name], rate)


def _guarded(shape, dtype=torch.float32, fill=SENT):
    """A sentinel-filled tensor of `shape` inside a larger buffer -> (view, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(*shape), buf


def _guards_intact(buf, fill=SENT):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


# ------------------------------------------------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("name", list(INPUTS))
def test_stft_stage_under_delta(name):
    y = INPUTS[name]
    n, F = y.shape[0], S.n_frames(y.shape[0])
    row = torch.full((2, n + 37), SENT, device=DEV)        # ld_in > n: what lies behind the row must not be read
    row[:, :n] = torch.from_numpy(y).to(DEV)
    row[1, :n] *= 0.5                                      # a second row: rows must not mix
    D, buf = _guarded((2, F, S.BINS, 2))
    L.check(L.load().wft_stretch_stft_f32(_p(row), row.stride(0), n, _p(D), 2, _stream()), "stft")
    got = D.cpu().numpy().astype(np.float64)
    got = got[..., 0] + 1j * got[..., 1]
    want = S.stft(y)
    delta = S.stft_allowance(y)
    err = np.abs(got[0] - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{name}: largest STFT error / delta_t = {np.nanmax(np.where(err == 0, 0, err / delta[:, None])):.4f}")
    assert (err <= delta[:, None]).all()
    assert np.array_equal(got[1], 0.5 * got[0])            # scaling by a power of two is exact through every stage of the FFT
    assert _guards_intact(buf)
    if name == "zeropad":                                  # all-zero frames transform to exact zeros
        assert not got[0][delta == 0].any() and (delta == 0).sum() >= 7


# ------------------------------------------------------------------------------------------------------------ stage 2
def test_vocoder_stage_bit_for_bit_on_exact_spectra():
    re, im = S.exact_spectra()
    F = re.shape[0]
    n_in = (F - 1) * S.H                                   # F = 1 + n_in // H
    rates = [0.5, 0.75, 1.25]
    B, T_max = len(rates), S.n_out_frames(F, 0.5)
    D = torch.from_numpy(np.stack([re, im], axis=-1)).to(DEV)[None].repeat(B, 1, 1, 1).contiguous()
    Sg, buf = _guarded((B, T_max, S.BINS, 2))
    rd = torch.tensor(rates, dtype=torch.float64, device=DEV)
    L.check(L.load().wft_stretch_vocoder_f32(_p(D), n_in, _p(rd), 0.5, _p(Sg), B, _stream()), "vocoder")
    got = Sg.cpu().numpy()
    for b, rate in enumerate(rates):
        sr, si = S.vocoder_exact(re, im, rate)
        T = sr.shape[0]
        assert T == S.n_out_frames(F, rate)
        assert np.array_equal(got[b, :T, :, 0].view(np.uint32), sr.view(np.uint32)), rate
        assert np.array_equal(got[b, :T, :, 1].view(np.uint32), si.view(np.uint32)), rate
        assert (got[b, T:] == SENT).all()                  # frames behind T_b are left untouched
    assert _guards_intact(buf)


# ------------------------------------------------------------------------------------------------------------ stage 3
@pytest.mark.parametrize("name,rate", [("noise5000", 0.75), ("noise16421", 1.25), ("zeropad", 0.8)])
def test_istft_stage_on_the_reference_spectra(name, rate):
    y = INPUTS[name]
    n = y.shape[0]
    want, _, parts = _ref(name, rate)
    S64 = parts["S"]
    T, T_max = S64.shape[0], S.n_out_frames(S.n_frames(n), rate)
    assert T == T_max
    S32 = np.stack([S64.real, S64.imag], axis=-1).astype(np.float32)
    Sg = torch.from_numpy(S32).to(DEV)[None].contiguous()
    cap = S.n_out_samples(n, rate)
    out, buf = _guarded((1, cap + 19))
    n_out = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    rd = torch.tensor([rate], dtype=torch.float64, device=DEV)
    L.check(L.load().wft_stretch_istft_f32(_p(Sg), n, _p(rd), rate, _p(out), out.stride(0), _p(n_out), 1, _stream()), "istft")
    assert n_out.item() == cap
    got = out.cpu().numpy()[0]
    # the spectra were rounded to fp32 on the way in: that is one of the 4 u per bin of the synthesis' allowance
    allow = S.istft_allowance(S64, cap)
    print(f"{name} rate {rate}: synthesis uses {S.used(got[:cap], want, allow):.4f} of its allowance")
    assert S.outside(got[:cap], want, allow) == 0
    assert (got[cap:] == SENT).all() and _guards_intact(buf)


# ------------------------------------------------------------------------------------------------------------ the whole call
def _whole(y, rates, rate_lo, ld_in_extra=37, ld_out_extra=19):
    n, B = y.shape[0], len(rates)
    lib = L.load()
    row = torch.full((B, n + ld_in_extra), SENT, device=DEV)
    row[:, :n] = torch.from_numpy(y).to(DEV)
    cap = int(round(n / rate_lo))
    out, buf = _guarded((B, cap + ld_out_extra))
    n_out = torch.full((B,), -5, dtype=torch.int32, device=DEV)
    rd = torch.tensor(rates, dtype=torch.float64, device=DEV)
    nbytes = lib.wft_time_stretch_workspace_bytes(B, n, rate_lo)
    ws, wbuf = _guarded((nbytes // 4,))
    L.check(lib.wft_time_stretch_f32(_p(row), row.stride(0), n, _p(rd), rate_lo, _p(out), out.stride(0), _p(n_out), _p(ws), nbytes, B,
                                     _stream()), "time_stretch")
    torch.cuda.synchronize()
    assert _guards_intact(buf) and _guards_intact(wbuf)
    return out.cpu().numpy(), n_out.cpu().numpy()


@pytest.mark.parametrize("name", list(INPUTS))
def test_whole_call_every_rate_in_one_launch(name):
    y = INPUTS[name]
    n = y.shape[0]
    got, n_out = _whole(y, list(RATES), min(RATES))
    worst = 0.0
    for b, rate in enumerate(RATES):
        want, allow, _ = _ref(name, rate)
        m = S.n_out_samples(n, rate)
        assert n_out[b] == m == want.shape[0]
        worst = max(worst, S.used(got[b, :m], want, allow))
        assert S.outside(got[b, :m], want, allow) == 0, (name, rate)
        assert (got[b, m:] == SENT).all(), (name, rate)    # nothing is written behind n_out[b]
    print(f"{name}: largest error / allowance over the rates = {worst:.4f}")
    # a row alone (its own rate_lo, B = 1, other leading dimensions) equals the same row in the batch, bit for bit
    for b in (1, len(RATES) - 1):
        alone, n1 = _whole(y, [RATES[b]], RATES[b], ld_in_extra=0, ld_out_extra=3)
        assert n1[0] == n_out[b] and np.array_equal(alone[0, :n1[0]].view(np.uint32), got[b, :n1[0]].view(np.uint32))
    again, n2 = _whole(y, list(RATES), min(RATES))           # a rerun is bit-identical
    assert np.array_equal(n2, n_out) and np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_a_rate_outside_the_host_bound_writes_nothing():
    y = INPUTS["noise2048"]
    got, n_out = _whole(y, [1.0, 0.75, 2.5, float("nan")], 0.8)
    assert n_out.tolist() == [2048, -1, -1, -1]
    assert (got[1:] == SENT).all() and S.outside(got[0, :2048], *_ref("noise2048", 1.0)[:2]) == 0


def test_wrappers_equal_the_raw_call():
    y = INPUTS["noise5000"]
    rates = [0.8, 1.25, 1.0]
    raw, n_raw = _whole(y, rates, 0.8)
    a = torch.from_numpy(y).to(DEV)[None].repeat(3, 1)
    out, n_out = K.time_stretch(a, rates)
    assert n_out.cpu().tolist() == n_raw.tolist() and out.shape == (3, 6250)
    parts = GF.time_stretch(np.stack([y] * 3), rates)
    for b in range(3):
        m = int(n_raw[b])
        assert torch.equal(out[b, :m].cpu(), torch.from_numpy(raw[b, :m])) and not out[b, m:].any()
        assert parts[b].shape == (m,) and torch.equal(parts[b], out[b, :m])
    one = GF.time_stretch(y, 1.25)
    assert one.dim() == 1 and torch.equal(one, parts[1])
    old = K.STRETCH_WORKSPACE_CAP
    try:                                                    # rows in chunks of one: the same bits
        K.STRETCH_WORKSPACE_CAP = 1
        out1, n1 = K.time_stretch(a, rates)
    finally:
        K.STRETCH_WORKSPACE_CAP = old
    assert torch.equal(out1, out) and torch.equal(n1, n_out)
    with pytest.raises(ValueError):
        K.time_stretch(a, [0.8, 1.25, 2.5])


# ------------------------------------------------------------------------------------------------------------ ragged log-mel
T_OUT, N_MELS = 48, 80


def _ragged_rows():
    """f32 [5, 9600 + 32], n_samples, keep: 40, 48 and 60 frames (the 60-frame row loudest in frames 50-59), a row cut by keep_frames,
    and a row of 160 * 40 + 77 samples; what lies behind a row's samples is garbage that must not be read."""
    rng = np.random.default_rng(4)
    ns = [6400, 7680, 9600, 9600, 160 * 40 + 77]
    keep = [3000, 3000, 3000, 25, 3000]
    x = np.full((5, 9600 + 32), 1.0e4, dtype=np.float32)
    for b, n in enumerate(ns):
        x[b, :n] = 0.01 * rng.standard_normal(n)
    x[2, :160 * 50] *= 1.0e-3                               # 94 dB below the tail: the tail's maximum - 8 floors these frames
    x[2, 160 * 50:9600] = 0.5 * rng.standard_normal(9600 - 160 * 50)
    return x, ns, keep


def test_logmel_ragged():
    x, ns, keep = _ragged_rows()
    filt = GF.mel_filters(N_MELS).to(DEV)
    xa = torch.from_numpy(x).to(DEV)
    nd = torch.tensor(ns, dtype=torch.int32, device=DEV)
    kd = torch.tensor(keep, dtype=torch.int32, device=DEV)
    out, buf = _guarded((5, N_MELS, T_OUT))
    stats = torch.empty(10, device=DEV)
    L.check(L.load().wft_logmel_ragged(_p(xa), xa.stride(0), _p(nd), _p(kd), _p(filt), _p(out), _p(stats), 5, xa.shape[1], N_MELS, T_OUT,
                                       _stream()), "logmel_ragged")
    assert _guards_intact(buf)                              # guard columns in front of and behind the output
    assert torch.equal(K.logmel_ragged(xa, nd, kd, filt, T_OUT), out)
    for b in range(4):                                      # multiples of 160: K.logmel on the row alone, then the torch expression
        frames, kept = S.frames_and_keep(ns[b], keep[b], T_OUT)
        full = K.logmel(xa[b:b + 1, :ns[b]].contiguous(), filt, frames)[0]
        want = torch.empty(N_MELS, T_OUT, device=DEV)
        want[:, :kept] = full[:, :kept]
        want[:, kept:] = full[:, :kept].min()
        assert torch.equal(out[b], want), b
    # the loud tail of row 2 lies behind T_out: a maximum over the first 48 frames only would leave more of the quiet frames unfloored
    full2 = K.logmel(xa[2:3, :9600].contiguous(), filt, 60)[0]
    front = K.logmel(xa[2:3, :7680].contiguous(), filt, 48)[0]
    assert not torch.equal(full2[:, :40], front[:, :40])
    # 160 * 40 + 77 samples: 40 frames over the reflect padding of all 6477 samples
    ref, lo, hi = S.logmel_ragged_interval(x[4, :ns[4]], filt.cpu().numpy(), 40)
    got = out[4].cpu().numpy().astype(np.float64)
    assert int((~((got[:, :40] >= lo) & (got[:, :40] <= hi))).sum()) == 0
    assert (out[4][:, 40:] == out[4][:, :40].min()).all()


# ------------------------------------------------------------------------------------------------------------ loader
SPEC = {"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 1.0}
EXT = {"low_freq_range": 5, "high_freq_range": 5}


class _Clips(DL.SyntheticDataset):
    """SyntheticDataset whose clip 1 ends in a partial segment that starts at 4 s: its mel is cut at 400 frames."""

    def __getitem__(self, i):
        rec = super().__getitem__(i)
        if i == 1:
            rec["text"] = rec["text"] + "<|4.00|><|4.00|>"
        return rec


def _loader(**kw):
    return DL.get_dataloader(_Clips(4, with_timestamps=True), DL.SimpleTokenizer(), batch_size=4, n_mels=N_MELS, shuffle=False,
                             device=DEV, no_timestamp_training=True, spec_augment=True, spec_augment_params=SPEC, extremes_spec_augment=True,
                             extremes_spec_augment_params=EXT, **kw)


def _seed():
    torch.manual_seed(11)
    random.seed(11)


def test_loader_batch_equals_a_replay_of_the_kernels():
    on = _loader(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25)
    assert isinstance(on, DL.GpuMelLoader)
    _seed()
    mel, y_in, y_out = next(iter(on))
    _seed()
    audio, yi, yo, params, ext, cut, rates = next(iter(on.loader))
    assert rates.dtype == torch.float64 and bool(((rates >= 0.75) & (rates <= 1.25)).all()) and len(set(rates.tolist())) == 4
    assert cut.tolist() == [3000, 400, 3000, 3000]         # a clip cut at its partial segment goes through keep_frames
    stretched, n_out = K.time_stretch(audio.to(DEV), rates)
    assert n_out.cpu().tolist() == [int(round(480000 / r)) for r in rates.tolist()]
    keep = cut.clamp(max=3000).to(torch.int32).to(DEV)
    want = K.specaug(K.logmel_ragged(stretched, n_out, keep, on.frontend.filters, 3000), params.to(DEV), ext.to(DEV))
    assert tuple(mel.shape) == (4, N_MELS, 3000) and torch.equal(mel, want)
    assert torch.equal(y_in.cpu(), yi) and torch.equal(y_out.cpu(), yo)
    # the flag off: the batch of the parent behaviour (plain log-mel, host loop for the cut, SpecAugment), from the same draws
    off = _loader()
    _seed()
    mel0 = next(iter(off))[0]
    _seed()
    batch0 = next(iter(off.loader))
    assert len(batch0) == 6
    for u, v in zip(batch0, (audio, yi, yo, params, ext, cut)):
        assert torch.equal(u, v)
    want0 = K.logmel(audio.to(DEV), off.frontend.filters, 3000)
    for b in (cut < 3000).nonzero().flatten().tolist():
        c = int(cut[b])
        want0[b, :, c:] = want0[b, :, :c].min() if c > 0 else want0[b].min()
    want0 = K.specaug(want0, params.to(DEV), ext.to(DEV))
    assert torch.equal(mel0, want0) and not torch.equal(mel0, mel)


def test_finetune_runs_three_steps_with_the_baseline_augmentation(tmp_path, monkeypatch):
    """configs/DEBUG_synthetic_stretch.yaml: the reference's audio_augment block with apply_baseline_aug on.  Every training
    micro-batch goes through the stretch, the dev loaders never do."""
    from pathlib import Path

    import yaml

    import whisper_finetune.runtime as rt
    from whisper_finetune.scripts import finetune

    cfg = yaml.safe_load((Path(__file__).resolve().parents[1] / "configs" / "DEBUG_synthetic_stretch.yaml").read_text())
    assert cfg["augmentation"]["audio_augment"] == {"apply_office_aug": False, "apply_baseline_aug": True, "apply_advanced_aug": False,
                                                    "time_stretch": {"min_rate": 0.75, "max_rate": 1.25}}
    cfg["save_dir"] = str(tmp_path)
    calls = []
    stretch = K.time_stretch
    monkeypatch.setattr(K, "time_stretch", lambda a, r: calls.append((tuple(a.shape), [float(x) for x in r])) or stretch(a, r))
    losses = finetune.main(cfg)
    rt.cleanup()
    assert cfg["training"]["train_steps"] == 3 and len(losses) == 3 and all(np.isfinite(l) for l in losses)
    assert len(calls) == 6 and all(shape == (2, 480000) for shape, _ in calls)
    assert all(0.75 <= r <= 1.25 for _, rs in calls for r in rs) and len({r for _, rs in calls for r in rs}) == 12


def test_calculate_mel_applies_the_same_two_kernels_per_clip():
    ds = DL.AudioDataset(_Clips(2), DL.SimpleTokenizer(), device=DEV, n_mels=N_MELS, apply_baseline_aug=True, time_stretch_min_rate=0.75,
                         time_stretch_max_rate=1.25)
    clip = ds.hu_dataset[0]["audio"]["array"]
    audio = np.pad(clip, (0, 480000 - clip.shape[0]))
    random.seed(5)
    mel = ds._calculate_mel(audio, 4.0, True)               # a partial segment that starts at 4 s: cut at 400 frames
    random.seed(5)
    rate = ds._draw_stretch_rate()
    stretched, n_out = K.time_stretch(torch.from_numpy(audio).to(DEV)[None], [rate])
    keep = torch.tensor([400], dtype=torch.int32, device=DEV)
    want = K.logmel_ragged(stretched, n_out, keep, GF.mel_filters(N_MELS).to(DEV), 3000)[0]
    assert 0.75 <= rate <= 1.25 and tuple(mel.shape) == (N_MELS, 3000) and torch.equal(mel, want)
    assert bool((mel[:, 400:] == mel[:, :400].min()).all())
