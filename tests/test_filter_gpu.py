"""IIR cascade on the device: wft_sos_filter_f32 against the sequential float64 recurrence, its refusals, and the loader stage.
Reference, bound, table, probes and lengths: tests/_filter_cases.py (DELTA is chosen there, on the CPU)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _filter_cases as FC  # noqa: E402
from whisper_finetune.data import data_loader as DL  # noqa: E402
from whisper_finetune.data import filters as F  # noqa: E402
from whisper_finetune.data import gpu_frontend as GF  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = torch.device("cuda:0")
CHUNK, GROUP = L.load().wft_sos_filter_chunk(), L.load().wft_sos_filter_group()
SENT = 777.25          # exact in fp32, far from every value the kernel writes
GUARD = 64
PAD = 7                # ld = n_max + PAD: what lies behind n_max must stay untouched


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _guarded(shape, dtype=torch.float32, fill=SENT):
    """A sentinel-filled tensor of `shape` inside a larger buffer -> (view, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(*shape), buf


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(inp, n_dev, n_max, sos, out, S=None, B=None, ld_in=None, ld_out=None, ws_bytes=None):
    """The raw call on tensors that are already on the device -> (status, workspace buffer)."""
    lib = L.load()
    B = inp.shape[0] if B is None else B
    S = sos.shape[1] if S is None else S
    need = max(lib.wft_sos_filter_workspace_bytes(max(B, 1), n_max, min(max(S, 1), 4)), 8)
    ws, wbuf = _guarded((need // 8,), torch.float64, fill=-1.0)
    rc = lib.wft_sos_filter_f32(_p(inp), inp.stride(0) if ld_in is None else ld_in, _p(n_dev), n_max, _p(sos), S, _p(out),
                                out.stride(0) if ld_out is None else ld_out, _p(ws), need if ws_bytes is None else ws_bytes, B,
                                L.stream_ptr())
    return rc, wbuf


def _run(rows, soses, use_n=True, in_place=False):
    """rows: B float32 arrays of their own lengths, soses: B arrays [s_b, 6].  The input rows are followed by NaN (what lies behind
    n[b] must not be read).  -> (whole output buffer incl. guards as float32 numpy, n_max, ld)."""
    B, ns = len(rows), [len(r) for r in rows]
    n_max, S = max(ns), max(s.shape[0] for s in soses)
    ld = n_max + PAD
    inp, ibuf = _guarded((B, ld), fill=float("nan"))
    for b, r in enumerate(rows):
        inp[b, :ns[b]] = torch.from_numpy(r).to(DEV)
    sos = torch.from_numpy(np.stack([FC.padded(s, S) for s in soses])).to(DEV)
    n_dev = torch.tensor(ns, dtype=torch.int32, device=DEV) if use_n else None
    out, obuf = (inp, ibuf) if in_place else _guarded((B, ld))
    rc, wbuf = _launch(inp, n_dev, n_max, sos, out)
    L.check(rc, "wft_sos_filter_f32")
    torch.cuda.synchronize()
    assert bool((wbuf[:GUARD] == -1.0).all() and (wbuf[-GUARD:] == -1.0).all()), "the workspace guards were written"
    return obuf.cpu(), n_max, ld


def _expected(refs32, ns, n_max, ld, fill=SENT):
    """The whole buffer a correct call leaves: the guards and the padding behind n_max untouched, zeros in [n[b], n_max)."""
    want = torch.full((len(ns) * ld + 2 * GUARD,), fill, dtype=torch.float32)
    body = want[GUARD:GUARD + len(ns) * ld].view(len(ns), ld)
    for b, r in enumerate(refs32):
        body[b, :ns[b]] = torch.from_numpy(r)
        body[b, ns[b]:n_max] = 0.0
    return want


@functools.lru_cache(maxsize=None)
def _results():
    """Every batch of tests/_filter_cases.py once -> (largest error over the bound with its case and, for the record, how many elements
    are not the correctly rounded reference; the exact rows that are not bit-equal; the batches whose buffer outside the filtered
    samples is not what it must be)."""
    refs = FC.references(CHUNK, GROUP)
    worst, inexact, frame, off, total = (0.0, None), [], [], 0, 0
    for batch in FC.batches(CHUNK, GROUP):
        ns = [c["n"] for c in batch]
        got, n_max, ld = _run([c["x"] for c in batch], [c["sos"] for c in batch])
        body = got[GUARD:GUARD + 3 * ld].view(3, ld)
        # the frame of the buffer: everything but the filtered samples, bit for bit
        masked = got.clone()
        mb = masked[GUARD:GUARD + 3 * ld].view(3, ld)
        for b in range(3):
            mb[b, :ns[b]] = 0.0
        if not torch.equal(_bits(masked), _bits(_expected([np.zeros(n, np.float32) for n in ns], ns, n_max, ld))):
            frame.append([c["name"] for c in batch])
        for b, c in enumerate(batch):
            y, ref = body[b, :ns[b]], refs[c["name"]]
            if c["exact"] and not torch.equal(_bits(y), _bits(torch.from_numpy(ref.astype(np.float32)))):
                inexact.append(c["name"])
            r = FC.worst_ratio(y.numpy()[None], ref[None])
            if r > worst[0]:
                worst = (r, c["name"])
            off, total = off + int((y.numpy() != ref.astype(np.float32)).sum()), total + ns[b]
    return worst + (off, total), inexact, frame


# ------------------------------------------------------------------------------------------------------------ the kernel
def test_exact_cases_are_bit_equal():
    _, inexact, _ = _results()
    assert not inexact, inexact[:10]


def test_tail_is_zero_and_nothing_else_is_touched():
    """Over every batch: out[b, n[b] .. n_max) is +0.0, the padding behind n_max and the guards keep the sentinel, and the NaNs behind
    n[b] in the input were not read (a NaN would have spread)."""
    _, _, frame = _results()
    assert not frame, frame[:5]


def test_table_probes_and_lengths_stay_under_the_bound():
    (ratio, name, off, total), _, _ = _results()
    # (the first term alone, the one float32 rounding, takes an element to 64 / 65 of the bound: the ratio says little about DELTA;
    # the count of elements that are not the correctly rounded reference says how much of DELTA the device used)
    print(f"largest error over the bound: {ratio:.4f} at {name} (DELTA = 2^{int(np.log2(FC.DELTA))}); {off} of {total} elements are not "
          "the correctly rounded reference")
    assert ratio <= 1.0, (ratio, name)


def test_identity_row_is_a_bit_copy():
    n = GROUP * CHUNK + 5
    rng = np.random.default_rng(3)
    x = rng.standard_normal(n).astype(np.float32)
    special = np.array([0x80000000, 0x00000001, 0x80000001, 0x7F800000, 0xFF800000, 0x7FC00123, 0xFFC00456, 0x00000000], dtype=np.uint32).view(np.float32)
    for pos in (0, 1, CHUNK - 1, CHUNK, n - 9):
        x[pos:pos + 8] = special
    other = FC.probe("noise_silent_tail", n - 100, CHUNK, GROUP)
    lp = FC.table()["lp150_o4"][0]
    for in_place in (False, True):
        for ident in (FC.IDENTITY[None], np.tile(FC.IDENTITY, (3, 1))):
            got, n_max, ld = _run([other, x, x[:CHUNK + 3]], [lp, ident, ident], in_place=in_place)
            body = got[GUARD:GUARD + 3 * ld].view(3, ld)
            assert torch.equal(_bits(body[1, :n]), _bits(torch.from_numpy(x))), in_place
            assert torch.equal(_bits(body[2, :CHUNK + 3]), _bits(torch.from_numpy(x[:CHUNK + 3]))) and not _bits(body[2, CHUNK + 3:n_max]).any()
            assert np.signbit(body[1, 0].item()) and body[1, 0].item() == 0.0


def _three():
    t = FC.table()
    names, ns = ["bs4000_f1.99_o4", "peak50_q5_p24", "lp7500_o2"], [2 * GROUP * CHUNK + 5, GROUP * CHUNK + 1, 2 * CHUNK + 3]
    return [FC.probe("noise_silent_tail", n, CHUNK, GROUP, seed=i) for i, n in enumerate(ns)], [t[k][0] for k in names], ns


def _row(buf, b, ld, n):
    return buf[GUARD + b * ld:GUARD + b * ld + n]


def test_a_row_does_not_depend_on_its_batch():
    xs, soses, ns = _three()
    alone = []
    for x, s in zip(xs, soses):
        got, _, ld = _run([x], [s])
        alone.append(_row(got, 0, ld, len(x)).clone())
    for shift in range(3):
        order = [(b + shift) % 3 for b in range(3)]
        got, _, ld = _run([xs[i] for i in order], [soses[i] for i in order])
        for b, i in enumerate(order):
            assert torch.equal(_bits(_row(got, b, ld, ns[i])), _bits(alone[i])), (shift, b)
    assert alone[0].abs().max() > 0


def test_in_place_is_bit_equal_to_out_of_place():
    xs, soses, ns = _three()
    a, n_max, ld = _run(xs, soses)
    b, _, _ = _run(xs, soses, in_place=True)
    av, bv = a[GUARD:GUARD + 3 * ld].view(3, ld), b[GUARD:GUARD + 3 * ld].view(3, ld)
    assert torch.equal(_bits(av[:, :n_max]), _bits(bv[:, :n_max]))
    assert bool(torch.isnan(bv[:, n_max:]).all()) and bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all())


def test_null_n_is_n_max_everywhere():
    xs, soses, _ = _three()
    n = len(xs[2])
    rows = [x[:n] for x in xs]
    a, _, _ = _run(rows, soses, use_n=True)
    b, _, _ = _run(rows, soses, use_n=False)
    assert torch.equal(_bits(a), _bits(b))


def test_n_is_clamped_on_the_device():
    x = FC.probe("noise_silent_tail", CHUNK + 9, CHUNK, GROUP)
    sos = FC.table()["peak50_q5_p24"][0]
    want, n_max, ld = _run([x, x, x], [sos, sos, sos])
    inp, _ = _guarded((3, ld), fill=float("nan"))            # NaN behind n_max: a clamp that came too late would read it
    inp[:, :n_max] = torch.from_numpy(x).to(DEV)
    out, obuf = _guarded((3, ld))
    n_dev = torch.tensor([n_max + 1000, -5, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    rc, _ = _launch(inp, n_dev, n_max, torch.from_numpy(np.stack([sos] * 3)).to(DEV), out)
    L.check(rc, "wft_sos_filter_f32")
    got = obuf.cpu()
    assert torch.equal(_bits(_row(got, 0, ld, ld)), _bits(_row(want, 0, ld, ld))) and torch.equal(_bits(_row(got, 2, ld, ld)), _bits(_row(want, 2, ld, ld)))
    assert not _bits(_row(got, 1, ld, n_max)).any() and bool((got[:GUARD] == SENT).all() and (got[-GUARD:] == SENT).all())


def test_refusals_leave_the_output_untouched():
    n_max, ld = 2 * CHUNK + 3, 2 * CHUNK + 3 + PAD
    inp, ibuf = _guarded((3, ld), fill=0.25)
    sos = torch.from_numpy(np.tile(FC.table()["lp150_o4"][0], (3, 1, 1))).to(DEV)
    sos5 = torch.from_numpy(np.tile(FC.IDENTITY, (3, 5, 1))).to(DEV)
    out, obuf = _guarded((3, ld))
    need = L.load().wft_sos_filter_workspace_bytes(3, n_max, 2)
    calls = {
        "S = 0": dict(sos=sos, S=0), "S = 5": dict(sos=sos5, S=5), "B = 0": dict(sos=sos, B=0), "ld_in < n_max": dict(sos=sos, ld_in=n_max - 1),
        "ld_out < n_max": dict(sos=sos, ld_out=n_max - 1), "short workspace": dict(sos=sos, ws_bytes=need - 8),
        "n_max = 0": dict(sos=sos, n_max=0),
    }
    for what, kw in calls.items():
        rc, _ = _launch(inp, None, kw.pop("n_max", n_max), kw.pop("sos"), out, **kw)
        assert rc != 0 and "wft_sos_filter_f32" in L.last_error(), what
    # partial overlap: out starts inside in; and the same pointer with another stride
    flat = ibuf[GUARD:GUARD + 3 * ld]
    for what, (o, ld_o) in {"shifted": (flat[5:], ld), "same pointer, other stride": (flat, ld - 1)}.items():
        rc = L.load().wft_sos_filter_f32(_p(inp), ld, None, n_max - 8, _p(sos), 2, _p(o), ld_o, _p(torch.empty(need, dtype=torch.uint8, device=DEV)),
                                         need, 3, L.stream_ptr())
        assert rc != 0 and "overlap" in L.last_error(), what
    # a0 != 1 is device data: the wrapper refuses it
    bad = sos.clone()
    bad[1, 0, 3] = 2.0
    for s in (bad, bad.cpu(), bad.cpu().numpy()):
        with pytest.raises(ValueError, match="a0"):
            K.sos_filter(inp, s, out=out)
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all()) and bool((ibuf[GUARD:-GUARD] == 0.25).all())


def test_wrapper_and_frontend():
    xs, soses, ns = _three()
    x = torch.from_numpy(xs[2]).to(DEV)
    want, _, ld = _run([xs[2]], [soses[2]])
    want = _row(want, 0, ld, ns[2])
    got = K.sos_filter(x[None], soses[2])
    assert torch.equal(_bits(got[0].cpu()), _bits(want))
    assert torch.equal(_bits(GF.sos_filter(xs[2], soses[2]).cpu()), _bits(want))                       # [n], a host array
    two = GF.sos_filter(np.stack([xs[2], xs[2]]), torch.from_numpy(np.stack([soses[2], soses[2]])))   # [B, n], a filter per row
    assert tuple(two.shape) == (2, ns[2]) and torch.equal(_bits(two[1].cpu()), _bits(want))
    y = x[None].clone()
    assert K.sos_filter(y, torch.from_numpy(soses[2][None]).to(DEV), out=y) is y and torch.equal(_bits(y[0].cpu()), _bits(want))
    n3 = torch.tensor([CHUNK + 1], dtype=torch.int32, device=DEV)
    cut = K.sos_filter(x[None], soses[2], n3)[0].cpu()
    assert torch.equal(_bits(cut[:CHUNK + 1]), _bits(want[:CHUNK + 1])) and not _bits(cut[CHUNK + 1:]).any()
    hp = GF.design_filter("high_pass", cutoff_freq=80.0, order=2)
    assert tuple(GF.sos_filter(xs[2], hp).shape) == (ns[2],)


# ------------------------------------------------------------------------------------------------------------ loader
N_MELS = 80
SPEC = {"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 1.0}
EXT = {"low_freq_range": 5, "high_freq_range": 5}
STRETCH = dict(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25)
AUG = {"p": 1.0}  # every clip draws a filter (peaking's inner gate may still say no)


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


def _plain_mel(audio, cut, filters):
    mel = K.logmel(audio, filters, 3000)
    for b in (cut < 3000).nonzero().flatten().tolist():
        c = int(cut[b])
        mel[b, :, c:] = mel[b, :, :c].min() if c > 0 else mel[b].min()
    return mel


def test_loader_batch_equals_a_replay_from_the_public_pieces():
    on = _loader(filter_aug=AUG)
    assert isinstance(on, DL.GpuMelLoader) and on.filter_aug and not on.stretch
    _seed()
    mel, y_in, y_out = next(iter(on))
    _seed()
    audio, yi, yo, params, ext, cut, sos = next(iter(on.loader))
    random.seed(11)
    aug = F.FilterAug(**AUG)
    draws = [aug.draw() for _ in range(4)]
    assert sos.dtype == torch.float64 and tuple(sos.shape) == (4, 4, 6) and np.array_equal(sos.numpy(), np.stack([d[2] for d in draws]))
    assert sum(d[0] is not None for d in draws) >= 2
    filtered = K.sos_filter(audio.to(DEV), sos)
    assert not torch.equal(filtered.cpu(), audio)
    want = K.specaug(_plain_mel(filtered, cut, on.frontend.filters), params.to(DEV), ext.to(DEV))
    assert tuple(mel.shape) == (4, N_MELS, 3000) and torch.equal(mel, want)
    assert torch.equal(y_in.cpu(), yi) and torch.equal(y_out.cpu(), yo)


def test_loader_batch_with_the_stretch_equals_a_replay():
    on = _loader(filter_aug=AUG, **STRETCH)
    assert on.filter_aug and on.stretch
    _seed()
    mel = next(iter(on))[0]
    _seed()
    audio, yi, yo, params, ext, cut, rates, sos = next(iter(on.loader))
    random.seed(11)
    aug, want_rates, want_sos = F.FilterAug(**AUG), [], []
    for _ in range(4):                                         # per clip: the stretch gate and rate, then the filter
        assert random.random() < 1.0
        want_rates.append(random.uniform(0.75, 1.25))
        want_sos.append(aug.draw()[2])
    assert rates.tolist() == want_rates and np.array_equal(sos.numpy(), np.stack(want_sos))
    stretched, n_out = K.time_stretch(audio.to(DEV), rates)
    filtered = K.sos_filter(stretched, sos, n_out)              # over each row's full stretched length, zero behind it
    keep = cut.clamp(max=3000).to(torch.int32).to(DEV)
    want = K.specaug(K.logmel_ragged(filtered, n_out, keep, on.frontend.filters, 3000), params.to(DEV), ext.to(DEV))
    assert torch.equal(mel, want)
    plain = K.specaug(K.logmel_ragged(stretched, n_out, keep, on.frontend.filters, 3000), params.to(DEV), ext.to(DEV))
    assert not torch.equal(mel, plain)


def test_p_zero_gives_the_batches_of_a_loader_without_the_option(monkeypatch):
    off, zero = _loader(), _loader(filter_aug={"p": 0.0})
    _seed()
    want = next(iter(off))
    _seed()
    audio, yi, yo, params, ext, cut = next(iter(off.loader))
    monkeypatch.setattr(K, "sos_filter", lambda *a, **k: pytest.fail("an all-identity batch must launch nothing"))
    _seed()
    got = next(iter(zero))
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    # and both are the parent's batch: plain log-mel, host loop for the cut, SpecAugment
    assert torch.equal(want[0], K.specaug(_plain_mel(audio.to(DEV), cut, off.frontend.filters), params.to(DEV), ext.to(DEV)))


@pytest.mark.parametrize("stretch", [False, True])
def test_calculate_mel_equals_the_batch_path_on_one_row(stretch):
    ds = DL.AudioDataset(_Clips(2), DL.SimpleTokenizer(), device=DEV, n_mels=N_MELS, filter_aug={"p": 1.0, "kinds": ["band_pass", "low_shelf"]},
                         **(STRETCH if stretch else {}))
    clip = ds.hu_dataset[0]["audio"]["array"]
    audio = np.pad(clip, (0, 480000 - clip.shape[0]))
    random.seed(5)
    mel = ds._calculate_mel(audio, 4.0, True)               # a partial segment that starts at 4 s: cut at 400 frames
    random.seed(5)
    row = torch.from_numpy(audio).to(DEV)[None]
    filters = GF.mel_filters(N_MELS).to(DEV)
    if stretch:
        row, n_out = K.time_stretch(row, [ds._draw_stretch_rate()])
    kind, _, sos = F.FilterAug(p=1.0, kinds=["band_pass", "low_shelf"]).draw()
    assert kind is not None
    if stretch:
        want = K.logmel_ragged(K.sos_filter(row, sos[None], n_out), n_out, torch.tensor([400], dtype=torch.int32, device=DEV), filters, 3000)[0]
    else:
        want = _plain_mel(K.sos_filter(row, sos[None]), torch.tensor([400]), filters)[0]
    assert tuple(mel.shape) == (N_MELS, 3000) and torch.equal(mel, want)
    assert bool((mel[:, 400:] == mel[:, :400].min()).all())


def test_finetune_runs_three_steps_with_the_filter_augmentation(tmp_path, monkeypatch):
    """configs/DEBUG_synthetic_filter.yaml: the stretch config plus audio_augment.wft_filter_aug.  Training micro-batches go through
    the stretch and, where a clip drew a filter, through the cascade in place; the dev loaders never do."""
    from pathlib import Path

    import yaml

    import whisper_finetune.runtime as rt
    from whisper_finetune.scripts import finetune

    cfg = yaml.safe_load((Path(__file__).resolve().parents[1] / "configs" / "DEBUG_synthetic_filter.yaml").read_text())
    aa = cfg["augmentation"]["audio_augment"]
    assert aa["apply_baseline_aug"] is True and aa["apply_advanced_aug"] is False and aa["wft_filter_aug"]["p"] == 0.6
    assert set(aa["wft_filter_aug"]["kinds"]) == set(F.KINDS)
    cfg["save_dir"] = str(tmp_path)
    calls = []
    run = K.sos_filter
    monkeypatch.setattr(K, "sos_filter", lambda a, s, n=None, out=None: calls.append((tuple(a.shape), tuple(s.shape), out is a)) or run(a, s, n, out=out))
    losses = finetune.main(cfg)
    rt.cleanup()
    assert cfg["training"]["train_steps"] == 3 and len(losses) == 3 and all(np.isfinite(l) for l in losses)
    assert 1 <= len(calls) <= 6 and all(shape[0] == 2 and sos == (2, 4, 6) and in_place for shape, sos, in_place in calls)
