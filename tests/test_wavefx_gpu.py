"""Wave effects on the device (csrc/wavefx.hip, include/wft.h "Wave effects") against the fp64 restatements of tests/_wavefx_cases.py:
every kind over the row lengths that sit on the seams of the apply pass's trip, in poisoned input buffers and sentinel-filled output
buffers compared whole; bit-equal alone against in a batch and in place against out of place; every refusal; the loader stage."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _wavefx_cases as W  # noqa: E402
from whisper_finetune.data import data_loader as DL  # noqa: E402
from whisper_finetune.data import filters as F  # noqa: E402
from whisper_finetune.data import gpu_frontend as GF  # noqa: E402
from whisper_finetune.data import wave_fx as WF  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = torch.device("cuda:0")
T = L.load().wft_wave_fx_tile()
SENT = float(W.SENTINEL)
GUARD = 64
CASES = W.stage_cases(T)


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _guarded(shape, dtype=torch.float32, fill=SENT):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(*shape), buf


def _fx_dev(rec):
    return torch.from_numpy(rec.view("u1").reshape(len(rec), 88).copy()).to(DEV)


def _call(inp, n_dev, n_max, fx, stage, out, B=None, ld_in=None, ld_out=None, ws=None, ws_bytes=None):
    """The raw call on device tensors -> (status, workspace view, workspace buffer)."""
    lib = L.load()
    B = inp.shape[0] if B is None else B
    need = max(lib.wft_wave_fx_workspace_bytes(max(B, 1), max(n_max, 1), stage if stage in (0, 1, 2) else 2), 8)
    wbuf = None
    if ws is None:
        ws, wbuf = _guarded((need // 8,), torch.float64, fill=-1.0)
    rc = lib.wft_wave_fx_f32(_p(inp), inp.stride(0) if ld_in is None else ld_in, _p(n_dev), n_max, _p(fx), stage, _p(out),
                             out.stride(0) if ld_out is None else ld_out, _p(ws), need if ws_bytes is None else ws_bytes, B, L.stream_ptr())
    return rc, ws, wbuf


def _run(buf_in, ns, n_max, rec, stage, in_place=False, use_n=True):
    """buf_in: numpy f32 [B, ld], poisoned behind the rows.  -> (whole output buffer incl. guards as numpy [GUARD + B ld + GUARD],
    thresholds numpy f32 [B, 2] for the clip stage)."""
    B, ld = buf_in.shape
    inp, ibuf = _guarded((B, ld))
    inp.copy_(torch.from_numpy(buf_in))
    out, obuf = (inp, ibuf) if in_place else _guarded((B, ld))
    n_dev = torch.tensor(ns, dtype=torch.int32, device=DEV) if use_n else None
    rc, ws, wbuf = _call(inp, n_dev, n_max, _fx_dev(rec), WF.STAGE_ID[stage], out)
    L.check(rc, "wft_wave_fx_f32")
    torch.cuda.synchronize()
    assert bool((wbuf[:GUARD] == -1.0).all() and (wbuf[-GUARD:] == -1.0).all()), "the workspace guards were written"
    thr = None
    if stage == "clip":
        off = 8 + 4 * ((B + 1) // 2 * 2)
        thr = ws.view(torch.uint8)[off:off + 8 * B].cpu().numpy().view(np.float32).reshape(B, 2)
    return obuf.cpu().numpy(), thr


def _rows(obuf, B, ld):
    return obuf[GUARD:GUARD + B * ld].reshape(B, ld)


def _check_whole(obuf, exps, ns, n_max, ld, what, in_place_input=None):
    """Every row under `violations`; what lies behind n_max and the guards must be untouched (out of place: the sentinel; in place:
    the input's own poison, and nothing behind n[b] touched either)."""
    B = len(ns)
    got = _rows(obuf, B, ld)
    assert bool((obuf[:GUARD] == W.SENTINEL).all() and (obuf[-GUARD:] == W.SENTINEL).all()), (what, "guards")
    for b in range(B):
        if in_place_input is None:
            assert bool((got[b, n_max:] == W.SENTINEL).all()), (what, b, "behind n_max")
            bad = W.violations(got[b, :n_max], exps[b])
        else:
            assert np.array_equal(W.bits(got[b, ns[b]:]), W.bits(in_place_input[b, ns[b]:])), (what, b, "behind n[b], in place")
            e = exps[b]
            cut = W.Expect(e.val[:ns[b]], e.exact[:ns[b]], e.mag[:ns[b]], e.K)
            bad = W.violations(got[b, :ns[b]], cut)
        assert bad == 0, (what, b, ns[b], bad)


# ------------------------------------------------------------------------------------------------------------ every kind
@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_kind_against_the_reference(name, pad):
    """pad 3: rows that are not 16-byte aligned (the scalar path); pad 4: aligned rows (the 16-byte path)."""
    ns, n_max, ld = W.layout(T, pad)
    stage, kind, fill = CASES[name]
    buf = W.case_input(ns, n_max, ld, name, kind)
    rec = fill(W.records(len(ns)))
    exps = W.expected_buffer(buf, ns, n_max, rec, stage)
    obuf, thr = _run(buf, ns, n_max, rec, stage)
    _check_whole(obuf, exps, ns, n_max, ld, name)
    if stage == "clip":  # the two thresholds themselves, bit for bit
        for b, n in enumerate(ns):
            if n >= 1:
                assert W.bits(thr[b, 0])[0] == W.bits(exps[b].thr[0])[0] and W.bits(thr[b, 1])[0] == W.bits(exps[b].thr[1])[0], (name, b, n, thr[b], exps[b].thr)
    if stage != "level" or not name.startswith("shift"):  # in place: bit-equal to out of place for every shift-free stage
        ibuf, _ = _run(buf, ns, n_max, rec, stage, in_place=True)
        a, b_ = _rows(obuf, len(ns), ld), _rows(ibuf, len(ns), ld)
        for b, n in enumerate(ns):
            assert np.array_equal(W.bits(a[b, :n]), W.bits(b_[b, :n])), (name, b, "in place")
        _check_whole(ibuf, exps, ns, n_max, ld, name + " in place", in_place_input=buf)


def _mixed(pad=3):
    """One batch with a different effect in every row and every stage, plus rows with none."""
    ns, n_max, ld = W.layout(T, pad)
    order = [8, 7, 6, 5, 4, 3, 2, 1, 0]
    ns = [ns[i] for i in order]  # the long row first: its partner rows change with the batch
    buf = W.poisoned_batch(ns, n_max, ld, 77, "zeros80")
    rec = W.records(len(ns))
    W.set_row(rec, 0, "gaussian_snr", snr_db=12.0, seed=0xABCDEF0123456789)
    W.set_row(rec, 0, "clipping", q=13)
    W.set_row(rec, 0, "shift", fraction=0.37, fade_len=80)
    W.set_row(rec, 1, "gaussian_noise", amplitude=0.004, seed=3)
    W.set_row(rec, 1, "gain_transition", start_db=-10.0, end_db=5.0, t0=-100, length=3000)
    W.set_row(rec, 2, "clipping", q=3)
    W.set_row(rec, 2, "gain", gain_db=-3.0)
    W.set_row(rec, 3, "gaussian_snr", snr_db=30.0, seed=11)
    W.set_row(rec, 4, "shift", fraction=-0.2, fade_len=5)
    W.set_row(rec, 5, "clipping", q=50)
    W.set_row(rec, 6, "gaussian_noise", amplitude=0.01, seed=1 << 63)
    return ns, n_max, ld, buf, rec


@pytest.mark.parametrize("stage", WF.STAGES)
def test_mixed_batch_against_the_reference_and_rows_do_not_depend_on_the_batch(stage):
    ns, n_max, ld, buf, rec = _mixed()
    obuf, _ = _run(buf, ns, n_max, rec, stage)
    _check_whole(obuf, W.expected_buffer(buf, ns, n_max, rec, stage), ns, n_max, ld, "mixed " + stage)
    got = _rows(obuf, len(ns), ld)
    for b in range(len(ns)):
        if not WF.active_rows(rec, stage)[b] and b != 7:
            continue
        alone, _ = _run(buf[b:b + 1], ns[b:b + 1], n_max, rec[b:b + 1], stage)
        assert np.array_equal(W.bits(_rows(alone, 1, ld)[0]), W.bits(got[b])), (stage, b)
    again, _ = _run(buf, ns, n_max, rec, stage)  # reruns are bit-identical
    assert np.array_equal(W.bits(again), W.bits(obuf))


def test_passthrough_rows_keep_their_bits_and_null_n_is_n_max():
    ns, n_max, ld = W.layout(T)
    buf = W.poisoned_batch(ns, n_max, ld, 5, "signed_zeros")
    buf[:, :n_max] = np.where(np.isnan(buf[:, :n_max]), np.float32(-0.0), buf[:, :n_max])  # every row is read whole below
    rec = W.records(len(ns))
    for stage in WF.STAGES:
        obuf, _ = _run(buf, ns, n_max, rec, stage, use_n=False)
        got = _rows(obuf, len(ns), ld)
        assert np.array_equal(W.bits(got[:, :n_max]), W.bits(buf[:, :n_max])) and bool((got[:, n_max:] == W.SENTINEL).all()), stage
    W.set_row(rec, 3, "gain", gain_db=6.0)
    obuf, _ = _run(buf, ns, n_max, rec, "level", use_n=False)
    full = [n_max] * len(ns)
    _check_whole(obuf, W.expected_buffer(buf, full, n_max, rec, "level"), full, n_max, ld, "null n")


def test_n_is_clamped_on_the_device():
    ns, n_max, ld = [5, 70, 33], 64, 71
    buf = W.poisoned_batch([5, 64, 33], n_max, ld, 9)
    rec = W.records(3)
    for b in range(3):
        W.set_row(rec, b, "gain", gain_db=2.0)
        W.set_row(rec, b, "clipping", q=10)
    for stage in ("clip", "level"):
        inp, _ = _guarded((3, ld))
        inp.copy_(torch.from_numpy(buf))
        out, obuf = _guarded((3, ld))
        n_dev = torch.tensor([5, 70, -4], dtype=torch.int32, device=DEV)
        rc, _, _ = _call(inp, n_dev, n_max, _fx_dev(rec), WF.STAGE_ID[stage], out)
        L.check(rc, "wft_wave_fx_f32")
        torch.cuda.synchronize()
        eff = [5, 64, 0]
        _check_whole(obuf.cpu().numpy(), W.expected_buffer(buf, eff, n_max, rec, stage), eff, n_max, ld, "clamped " + stage)


# ------------------------------------------------------------------------------------------------------------ noise
def test_noise_of_one_seed_is_the_same_on_the_common_prefix():
    ns = [T + 1, 3 * T + 5, 700]
    n_max, ld = 3 * T + 8, 3 * T + 11
    base = W.signal(max(ns), 1)
    buf = np.full((3, ld), np.nan, dtype=np.float32)
    for b, n in enumerate(ns):
        buf[b, :n] = base[:n]
    rec = W.records(3)
    for b in range(3):
        W.set_row(rec, b, "gaussian_noise", amplitude=0.0125, seed=0x0123456789ABCDEF)
    got = _rows(_run(buf, ns, n_max, rec, "noise")[0], 3, ld)
    assert np.array_equal(W.bits(got[0, :700]), W.bits(got[2, :700])) and np.array_equal(W.bits(got[0, :T + 1]), W.bits(got[1, :T + 1]))
    assert not np.array_equal(got[0, :700], base[:700])


def test_seed_halves_are_distinguished():
    n, n_max, ld = 2 * T + 3, 2 * T + 4, 2 * T + 8
    buf = W.poisoned_batch([n] * 4, n_max, ld, 2)
    buf[1:, :n] = buf[0, :n]
    rec = W.records(4)
    for b, seed in enumerate([(7 << 32) | 9, (9 << 32) | 7, 9, 7 << 32]):
        W.set_row(rec, b, "gaussian_noise", amplitude=0.01, seed=seed)
    obuf, _ = _run(buf, [n] * 4, n_max, rec, "noise")
    _check_whole(obuf, W.expected_buffer(buf, [n] * 4, n_max, rec, "noise"), [n] * 4, n_max, ld, "seed halves")
    got = _rows(obuf, 4, ld)[:, :n]
    for a in range(4):
        for b in range(a + 1, 4):
            assert (got[a] != got[b]).mean() > 0.99, (a, b)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_untouched():
    n_max, ld = 2 * T + 3, 2 * T + 10
    inp, ibuf = _guarded((3, ld), fill=0.25)
    out, obuf = _guarded((3, ld))
    rec = W.records(3)
    for b in range(3):
        W.set_row(rec, b, "gain", gain_db=3.0)
        W.set_row(rec, b, "clipping", q=10)
        W.set_row(rec, b, "gaussian_noise", amplitude=0.1, seed=b)
    fx = _fx_dev(rec)
    lib = L.load()
    for stage in (0, 1, 2):
        need = lib.wft_wave_fx_workspace_bytes(3, n_max, stage)
        calls = {"unknown stage": dict(stage=3), "negative stage": dict(stage=-1), "B = 0": dict(B=0), "B too large": dict(B=65536),
                 "n_max = 0": dict(n_max=0), "n_max too large": dict(n_max=(1 << 30) + 1, ld_in=1 << 31, ld_out=1 << 31),
                 "ld_in < n_max": dict(ld_in=n_max - 1), "ld_out < n_max": dict(ld_out=n_max - 1), "short workspace": dict(ws_bytes=need - 8)}
        for what, kw in calls.items():
            rc, _, _ = _call(inp, None, kw.pop("n_max", n_max), fx, kw.pop("stage", stage), out, **kw)
            assert rc != 0 and "wft_wave_fx_f32" in L.last_error(), (stage, what)
        ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
        args = lambda **k: [k.get("inp", _p(inp)), ld, None, n_max, k.get("fx", _p(fx)), stage, k.get("out", _p(out)), k.get("ld_out", ld),  # noqa: E731
                            k.get("ws", _p(ws)), need, 3, L.stream_ptr()]
        for what, k in {"null in": dict(inp=None), "null fx": dict(fx=None), "null out": dict(out=None), "null workspace": dict(ws=None)}.items():
            assert lib.wft_wave_fx_f32(*args(**k)) != 0 and "null" in L.last_error(), (stage, what)
        for what, k in {"in off by 2 bytes": dict(inp=C.c_void_p(inp.data_ptr() + 2)), "fx off by 4 bytes": dict(fx=C.c_void_p(fx.data_ptr() + 4)),
                        "workspace off by 4 bytes": dict(ws=C.c_void_p(ws.data_ptr() + 4)), "out off by 1 byte": dict(out=C.c_void_p(out.data_ptr() + 1))}.items():
            assert lib.wft_wave_fx_f32(*args(**k)) != 0 and "aligned" in L.last_error(), (stage, what)
        flat = ibuf[GUARD:GUARD + 3 * ld]
        for what, k in {"shifted": dict(out=_p(flat[5:])), "same pointer, other stride": dict(out=_p(flat), ld_out=ld - 1)}.items():
            assert lib.wft_wave_fx_f32(*args(**k)) != 0 and "overlap" in L.last_error(), (stage, what)
    # values that only the device would see: the wrapper refuses them
    bad = rec.copy()
    bad["clip_q"][1] = 51
    with pytest.raises(ValueError, match="0..50"):
        K.wave_fx(inp, bad, "clip", out=out)
    bad = rec.copy()
    bad["noise_value"][2] = np.inf
    with pytest.raises(ValueError, match="finite"):
        K.wave_fx(inp, bad, "noise", out=out)
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all()) and bool((ibuf[GUARD:-GUARD] == 0.25).all())


# ------------------------------------------------------------------------------------------------------------ wrappers
def test_wrapper_and_frontend():
    ns, n_max, ld, buf, rec = _mixed(pad=4)
    B = len(ns)
    x = torch.from_numpy(np.nan_to_num(buf[:, :n_max], nan=0.0, posinf=0.0)).to(DEV)
    x = torch.where(x.abs() > 1e20, torch.zeros_like(x), x)
    n_dev = torch.tensor(ns, dtype=torch.int32, device=DEV)
    host = x.cpu().numpy()
    for stage in WF.STAGES:
        exps = W.expected_buffer(host, ns, n_max, rec, stage)
        got = K.wave_fx(x, rec, stage, n_dev)
        assert got is not x and tuple(got.shape) == (B, n_max)
        for b in range(B):
            assert W.violations(got[b].cpu().numpy(), exps[b]) == 0, (stage, b)
        # the table form gives the same records; in place equals out of place, shift rows included (through a temporary)
        y = x.clone()
        assert K.wave_fx(y, torch.from_numpy(WF.table_from_records(rec)), stage, n_dev, out=y) is y
        for b in range(B):
            assert torch.equal(y[b, :ns[b]].view(torch.int32), got[b, :ns[b]].view(torch.int32)), (stage, b)
            assert torch.equal(y[b, ns[b]:].view(torch.int32), x[b, ns[b]:].view(torch.int32)), (stage, b, "behind n[b]")
    # no active row: nothing is launched; out of place the rows are copied and zeroed behind n
    none = W.records(B)
    assert K.wave_fx(x, none, "clip", n_dev, out=x) is x
    z = K.wave_fx(x, none, "noise", n_dev)
    for b in range(B):
        assert torch.equal(z[b, :ns[b]].view(torch.int32), x[b, :ns[b]].view(torch.int32)) and not z[b, ns[b]:].view(torch.int32).any()
    # the stand-alone form: [n] host array and [B, n]
    row = W.signal(3 * T + 5, 4)
    one = WF.records_from_table(WF.table_row("shift", fraction=0.25, fade_len=16)[None])[0]
    want = W.ref_level(row, len(row), one, len(row))
    assert W.violations(GF.wave_fx(row, "shift", fraction=0.25, fade_len=16).cpu().numpy(), want) == 0
    two = GF.wave_fx(np.stack([row, row]), "gaussian_snr", snr_db=20.0, seed=5)
    one = WF.records_from_table(WF.table_row("gaussian_snr", snr_db=20.0, seed=5)[None])[0]
    want = W.ref_noise(row, len(row), one, len(row))
    assert tuple(two.shape) == (2, len(row)) and W.violations(two[1].cpu().numpy(), want) == 0 and torch.equal(two[0], two[1])
    clipped = GF.wave_fx(torch.from_numpy(row).to(DEV), "clipping", q=20).cpu().numpy()
    lo, hi = W.thresholds(row, 20)
    assert np.array_equal(clipped, np.clip(row, lo, hi)) and (clipped != row).mean() > 0.35


# ------------------------------------------------------------------------------------------------------------ loader
N_MELS = 80
SPEC = {"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 1.0}
EXT = {"low_freq_range": 5, "high_freq_range": 5}
STRETCH = dict(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25)
FILT = {"p": 1.0}
WAVE = {"noise": {"p": 1.0}, "clip": {"p": 1.0, "kinds": {"clipping": {"p": 1.0}}}, "level": {"p": 1.0, "kinds": {"shift": {"p": 1.0}, "gain": {}, "gain_transition": {}}}}


def _loader(**kw):
    return DL.get_dataloader(DL.SyntheticDataset(4, with_timestamps=True), DL.SimpleTokenizer(), batch_size=4, n_mels=N_MELS, shuffle=False,
                             device=DEV, no_timestamp_training=True, spec_augment=True, spec_augment_params=SPEC, extremes_spec_augment=True,
                             extremes_spec_augment_params=EXT, **kw)


def _seed():
    torch.manual_seed(11)
    random.seed(11)


def test_loader_batch_with_stretch_and_filter_equals_a_replay_in_the_stated_order():
    on = _loader(wave_aug=WAVE, filter_aug=FILT, **STRETCH)
    assert isinstance(on, DL.GpuMelLoader) and on.wave_aug and on.filter_aug and on.stretch
    _seed()
    mel, y_in, y_out = next(iter(on))
    _seed()
    audio, yi, yo, params, ext, cut, rates, sos, table = next(iter(on.loader))
    assert table.dtype == torch.float64 and tuple(table.shape) == (4, WF.TABLE_WIDTH)
    rec = WF.check_records(WF.records_from_table(table))
    assert all(WF.active_rows(rec, s).all() for s in WF.STAGES)
    x, n_out = K.time_stretch(audio.to(DEV), rates)
    x = K.wave_fx(x, rec, "noise", n_out)
    x = K.sos_filter(x, sos, n_out)
    x = K.wave_fx(x, rec, "clip", n_out)
    x = K.wave_fx(x, rec, "level", n_out)
    keep = cut.clamp(max=3000).to(torch.int32).to(DEV)
    want = K.specaug(K.logmel_ragged(x, n_out, keep, on.frontend.filters, 3000), params.to(DEV), ext.to(DEV))
    assert tuple(mel.shape) == (4, N_MELS, 3000) and torch.equal(mel, want)
    assert torch.equal(y_in.cpu(), yi) and torch.equal(y_out.cpu(), yo)
    # another order is another batch: the stages do not commute
    x2, _ = K.time_stretch(audio.to(DEV), rates)
    x2 = K.wave_fx(K.wave_fx(K.wave_fx(K.sos_filter(x2, sos, n_out), rec, "noise", n_out), rec, "clip", n_out), rec, "level", n_out)
    assert not torch.equal(K.logmel_ragged(x2, n_out, keep, on.frontend.filters, 3000), K.logmel_ragged(x, n_out, keep, on.frontend.filters, 3000))


def test_loader_batch_without_the_stretch_equals_a_replay():
    on = _loader(wave_aug=WAVE)
    assert on.wave_aug and not on.filter_aug and not on.stretch
    _seed()
    mel = next(iter(on))[0]
    _seed()
    audio, yi, yo, params, ext, cut, table = next(iter(on.loader))
    x = audio.to(DEV)
    for stage in WF.STAGES:
        x = K.wave_fx(x, table, stage)
    plain = K.logmel(x, on.frontend.filters, 3000)
    for b in (cut < 3000).nonzero().flatten().tolist():
        c = int(cut[b])
        plain[b, :, c:] = plain[b, :, :c].min() if c > 0 else plain[b].min()
    assert torch.equal(mel, K.specaug(plain, params.to(DEV), ext.to(DEV))) and not torch.equal(x.cpu(), audio)


@pytest.mark.parametrize("stretch", [False, True])
def test_every_gate_at_zero_gives_the_batches_of_a_loader_without_the_option(stretch, monkeypatch):
    kw = STRETCH if stretch else {}
    off = _loader(**kw)
    zero = _loader(wave_aug={"noise": {"p": 0.0}, "clip": {"p": 0.0}, "level": {"p": 0.0}}, **kw)
    _seed()
    want = next(iter(off))
    # the failed gates consume three draws of Python's random per clip; the stretch rate is drawn before them, so replay clip by clip
    _seed()
    batch = next(iter(zero.loader))
    assert len(batch) == 7 + int(stretch) and np.array_equal(batch[-1].numpy(), WF.none_table(4))
    if not stretch:
        monkeypatch.setattr(K, "wave_fx", lambda *a, **k: pytest.fail("a batch without any effect must launch nothing"))
        _seed()
        got = next(iter(zero))
        for u, v in zip(got, want):
            assert torch.equal(u, v)
    else:  # the rates differ between the two loaders (the gates' draws sit between the clips' rates): same rates, same batch
        _seed()
        got = next(iter(zero))
        x, n_out = K.time_stretch(batch[0].to(DEV), batch[6])
        keep = batch[5].clamp(max=3000).to(torch.int32).to(DEV)
        ref = K.specaug(K.logmel_ragged(x, n_out, keep, zero.frontend.filters, 3000), batch[3].to(DEV), batch[4].to(DEV))
        assert torch.equal(got[0], ref)


def test_calculate_mel_equals_the_batch_path_on_one_row():
    ds = DL.AudioDataset(DL.SyntheticDataset(2), DL.SimpleTokenizer(), device=DEV, n_mels=N_MELS, wave_aug=WAVE, filter_aug={"p": 1.0, "kinds": ["low_shelf"]},
                         **STRETCH)
    clip = ds.hu_dataset[0]["audio"]["array"]
    audio = np.pad(clip, (0, 480000 - clip.shape[0]))
    random.seed(5)
    mel = ds._calculate_mel(audio, 4.0, True)
    random.seed(5)
    row, n_out = K.time_stretch(torch.from_numpy(audio).to(DEV)[None], [ds._draw_stretch_rate()])
    sos = F.FilterAug(p=1.0, kinds=["low_shelf"]).draw()[2]
    table = WF.WaveAug(**WAVE).draw(480000)[1][None]
    row = K.wave_fx(row, table, "noise", n_out)
    row = K.sos_filter(row, sos[None], n_out)
    row = K.wave_fx(K.wave_fx(row, table, "clip", n_out), table, "level", n_out)
    want = K.logmel_ragged(row, n_out, torch.tensor([400], dtype=torch.int32, device=DEV), GF.mel_filters(N_MELS).to(DEV), 3000)[0]
    assert torch.equal(mel, want)
