"""Office effects on the device: wft_fir_conv_f32 under the per-element bound of tests/_office_cases.py (L = 1024; n_max and
taps_max around the block and partition seams, ragged rows with 0 of each, poisoned padding, sentinel-filled output buffers compared
in full), its independence statements bit for bit, every refusal; wft_bitcrush_f32 bit for bit against numpy; the wrappers and the
loader's office stages against replays from the public pieces."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _office_cases as O  # noqa: E402
from whisper_finetune.data import data_loader as DL  # noqa: E402
from whisper_finetune.data import gpu_frontend as GF  # noqa: E402
from whisper_finetune.data import office_fx as OF  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = torch.device("cuda:0")
SENT = float(O.SENTINEL)
GUARD = 64
BY_NAME = {c["name"]: c for c in O.CASES}


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _guarded(host, fill=None):
    """A numpy array (or a shape with `fill`) -> (its device copy as a view inside a guarded buffer, the whole buffer)."""
    shape = host if isinstance(host, tuple) else host.shape
    dtype = torch.float32 if isinstance(host, tuple) else torch.from_numpy(host).dtype
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT if fill is None else fill, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(*shape)
    if not isinstance(host, tuple):
        view.copy_(torch.from_numpy(host))
    return view, buf


def _conv(X, ns, IR, Ts, n_max, taps_max, use_n=True, use_t=True):
    """The raw call on guarded buffers -> the whole output buffer [B, ld] as numpy, guards checked."""
    B, ld = X.shape
    x_d, _ = _guarded(np.ascontiguousarray(X))
    ir_d, _ = _guarded(np.ascontiguousarray(IR))
    out, obuf = _guarded((B, ld))
    n_d = torch.tensor(ns, dtype=torch.int32, device=DEV) if use_n else None
    t_d = torch.tensor(Ts, dtype=torch.int32, device=DEV) if use_t else None
    lib = L.load()
    nbytes = lib.wft_fir_conv_workspace_bytes(B, taps_max)
    ws = torch.full((nbytes // 4 + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)  # a poisoned workspace
    L.check(lib.wft_fir_conv_f32(_p(x_d), ld, _p(n_d), n_max, _p(ir_d), IR.shape[1], _p(t_d), taps_max, _p(out), ld, _p(ws[GUARD:]), nbytes,
                                 B, L.stream_ptr()), "wft_fir_conv_f32")
    torch.cuda.synchronize()
    whole = obuf.cpu().numpy()
    assert bool((whole[:GUARD] == O.SENTINEL).all() and (whole[-GUARD:] == O.SENTINEL).all()), "guards of the output"
    assert bool(torch.isnan(ws[:GUARD]).all() and torch.isnan(ws[GUARD + nbytes // 4:]).all()), "guards of the workspace"
    return whole[GUARD:-GUARD].reshape(B, ld)


def _run(case, **kw):
    return _conv(case["X"], case["ns"], case["IR"], case["Ts"], case["n_max"], case["taps_max"], **kw)


# ------------------------------------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("name", O.CASE_IDS)
def test_fir_conv_every_element_inside_the_bound(name):
    case = BY_NAME[name]
    ok, ratio, complaint = O.check(_run(case), case)
    print(f"{name}: largest |out - ref| / (11 * 2^-24 * sum) = {ratio:.5f} (C = {O.C}, the emulation reaches {O.MEASURED_RATIO})")
    assert ok, (name, complaint, ratio)


def test_fir_conv_reruns_and_a_row_alone_are_bit_equal_to_the_row_in_a_batch():
    for name in ("room_ir", "n2049_t2048_dense_p2", "n3077_t2048_x_impulses_p1", "n3077_t2049_ir_impulse_p1"):
        case = BY_NAME[name]
        batch = _run(case)
        assert np.array_equal(O.bits(batch), O.bits(_run(case))), (name, "rerun")
        for b in range(3):
            alone = _conv(case["X"][b:b + 1], case["ns"][b:b + 1], case["IR"][b:b + 1], case["Ts"][b:b + 1], case["n_max"], case["taps_max"])
            assert np.array_equal(O.bits(alone[0]), O.bits(batch[b])), (name, b)
        rev = _conv(case["X"][::-1], case["ns"][::-1], case["IR"][::-1], case["Ts"][::-1], case["n_max"], case["taps_max"])
        assert np.array_equal(O.bits(rev[::-1]), O.bits(batch)), (name, "other partners")


def test_fir_conv_bits_do_not_depend_on_taps_max():
    for name in ("room_ir", "n3077_t1025_dense_p1", "n2049_t1024_x_impulses_p1", "n3077_t2_dense_p0", "n1025_t2048_ir_impulse_p2"):
        case = BY_NAME[name]
        want = _run(case)
        for wider in (case["taps_max"] + 1, case["taps_max"] + 1024, 8192):
            IR = np.full((3, wider + O.PAD_IR), np.nan, dtype=np.float32)  # poison up to the new width
            for b in range(3):
                IR[b, :case["Ts"][b]] = case["IR"][b, :case["Ts"][b]]
            got = _conv(case["X"], case["ns"], IR, case["Ts"], case["n_max"], wider)
            assert np.array_equal(O.bits(got), O.bits(want)), (name, wider)
    # ... with zeros, not poison, behind n_taps[b] as well: those partitions contribute nothing
    n_max = 1500
    X = np.zeros((1, n_max + O.PAD_X), dtype=np.float32)
    X[0, 3] = -1.0
    IR = np.zeros((1, 4096 + O.PAD_IR), dtype=np.float32)
    IR[0, 0] = 0.0
    IR[0, 1] = 0.5
    a, b = _conv(X, [n_max], IR, [2], n_max, 2), _conv(X, [n_max], IR, [2], n_max, 4096)
    assert np.array_equal(O.bits(a), O.bits(b)) and a[0, 4] == -0.5


def test_fir_conv_null_lengths_and_clamped_device_values():
    case = BY_NAME["n3077_t1025_dense_p1"]
    X, IR = np.nan_to_num(case["X"], nan=0.125), np.nan_to_num(case["IR"], nan=-0.03125)
    full = dict(case, X=X, IR=IR, ns=[case["n_max"]] * 3, Ts=[case["taps_max"]] * 3)
    for kw in (dict(use_n=False), dict(use_t=False), dict(use_n=False, use_t=False)):
        ok, _, complaint = O.check(_run(full, **kw), full)
        assert ok, (kw, complaint)
    wild = _conv(X, [case["n_max"] + 100, -5, 2], IR, [case["taps_max"] + 7, 3, -1], case["n_max"], case["taps_max"])
    ok, _, complaint = O.check(wild, dict(full, ns=[case["n_max"], 0, 2], Ts=[case["taps_max"], 3, 0]))
    assert ok, complaint


def test_fir_conv_refusals_leave_the_output_untouched():
    n_max, taps, ld, ld_ir = 1500, 1100, 1504, 1104
    inp, ibuf = _guarded((3, ld), fill=0.25)
    ir, _ = _guarded((3, ld_ir), fill=0.01)
    out, obuf = _guarded((3, ld))
    lib = L.load()
    nbytes = lib.wft_fir_conv_workspace_bytes(3, taps)
    assert nbytes == 3 * 2 * 1025 * 8
    ws = torch.zeros(nbytes // 4 + 4, dtype=torch.float32, device=DEV)
    n = torch.full((3,), n_max, dtype=torch.int32, device=DEV)
    args = lambda **k: [k.get("inp", _p(inp)), k.get("ld_in", ld), k.get("n", _p(n)), k.get("n_max", n_max), k.get("ir", _p(ir)),  # noqa: E731
                        k.get("ld_ir", ld_ir), k.get("n_taps", None), k.get("taps", taps), k.get("out", _p(out)), k.get("ld_out", ld),
                        k.get("ws", _p(ws)), k.get("nbytes", nbytes), k.get("B", 3), L.stream_ptr()]
    assert lib.wft_fir_conv_f32(*args()) == 0  # the base call is accepted ...
    torch.cuda.synchronize()
    assert not bool((out[:, :n_max] == SENT).any())
    obuf.fill_(SENT)  # ... and every variation below is not
    ws.zero_()
    flat = ibuf[GUARD:GUARD + 3 * ld]
    cases = {"null in": dict(inp=None), "null ir": dict(ir=None), "null out": dict(out=None), "null workspace": dict(ws=None),
             "B = 0": dict(B=0), "B too large": dict(B=65536), "n_max = 0": dict(n_max=0),
             "n_max too large": dict(n_max=(1 << 30) + 1, ld_in=1 << 31, ld_out=1 << 31), "taps_max = 0": dict(taps=0),
             "taps_max too large": dict(taps=8193, ld_ir=8200, nbytes=1 << 30), "ld_in < n_max": dict(ld_in=n_max - 1),
             "ld_out < n_max": dict(ld_out=n_max - 1), "ld_ir < taps_max": dict(ld_ir=taps - 1), "short workspace": dict(nbytes=nbytes - 1),
             "in off by 2 bytes": dict(inp=C.c_void_p(inp.data_ptr() + 2)), "out off by 2 bytes": dict(out=C.c_void_p(out.data_ptr() + 2)),
             "ir off by 2 bytes": dict(ir=C.c_void_p(ir.data_ptr() + 2)), "n off by 2 bytes": dict(n=C.c_void_p(n.data_ptr() + 2)),
             "n_taps off by 2 bytes": dict(n_taps=C.c_void_p(n.data_ptr() + 2)), "workspace off by 4 bytes": dict(ws=C.c_void_p(ws.data_ptr() + 4)),
             "in place": dict(out=_p(inp)), "shifted overlap": dict(out=_p(flat[5:])), "out inside the workspace": dict(out=_p(ws), ld_out=n_max, B=1),
             "ir is the output": dict(ir=_p(out), ld_ir=ld)}
    for what, k in cases.items():
        assert lib.wft_fir_conv_f32(*args(**k)) != 0 and "wft_fir_conv_f32" in L.last_error(), what
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all()) and bool((ibuf[GUARD:-GUARD] == 0.25).all()) and not bool(ws.any())


# ------------------------------------------------------------------------------------------------------------ bit crush
def _crush(X, ns, depths, n_max, in_place=False, use_n=True):
    B, ld = X.shape
    x_d, xbuf = _guarded(np.ascontiguousarray(X))
    out, obuf = (x_d, xbuf) if in_place else _guarded((B, ld))
    n_d = torch.tensor(ns, dtype=torch.int32, device=DEV) if use_n else None
    d_d = torch.tensor(depths, dtype=torch.int32, device=DEV)
    L.check(L.load().wft_bitcrush_f32(_p(x_d), ld, _p(n_d), n_max, _p(d_d), _p(out), ld, B, L.stream_ptr()), "wft_bitcrush_f32")
    torch.cuda.synchronize()
    whole = obuf.cpu().numpy()
    assert bool((whole[:GUARD] == O.SENTINEL).all() and (whole[-GUARD:] == O.SENTINEL).all()), "guards"
    return whole[GUARD:-GUARD].reshape(B, ld)


def test_bitcrush_bit_for_bit_against_numpy():
    vals = O.crush_values()
    n_max = vals.shape[0]
    assert n_max > 1024  # more than one workgroup per row
    depths = [1, 6, 14, 24, 0, 25, -3, 1 << 20]
    ns = [n_max, n_max - 1, 1025, 1024, n_max, 7, n_max, 0]
    X = np.full((8, n_max + O.PAD_X), O.SENTINEL, dtype=np.float32)
    for b in range(8):
        X[b, :ns[b]] = np.roll(vals, 13 * b)[:ns[b]]
    X[:, n_max:] = O.SENTINEL  # behind n_max the input is never read and, in place, never written
    poisoned = X.copy()
    for b in range(8):
        poisoned[b, ns[b]:n_max] = np.nan
    got = _crush(poisoned, ns, depths, n_max)
    for b in range(8):
        want = O.bitcrush_numpy(X[b, :ns[b]], depths[b])
        assert np.array_equal(O.bits(got[b, :ns[b]]), O.bits(want)), (b, depths[b])
        assert not O.bits(got[b, ns[b]:n_max]).any() and bool((got[b, n_max:] == O.SENTINEL).all()), b
        if not 1 <= depths[b] <= 24:
            assert np.array_equal(O.bits(got[b, :ns[b]]), O.bits(X[b, :ns[b]])), (b, "a copy")
    assert np.array_equal(O.bits(_crush(poisoned, ns, depths, n_max, in_place=True)), O.bits(got))  # in place: the same bits
    alone = _crush(poisoned[1:2], ns[1:2], depths[1:2], n_max)
    assert np.array_equal(O.bits(alone[0]), O.bits(got[1]))
    full = _crush(X, ns, depths, n_max, use_n=False)  # n == NULL: every row covers n_max samples
    for b in range(8):
        assert np.array_equal(O.bits(full[b, :n_max]), O.bits(O.bitcrush_numpy(X[b, :n_max], depths[b]))), b


def test_bitcrush_refusals_leave_the_output_untouched():
    n_max, ld = 1500, 1504
    inp, ibuf = _guarded((3, ld), fill=0.25)
    out, obuf = _guarded((3, ld))
    depth = torch.full((3,), 8, dtype=torch.int32, device=DEV)
    lib = L.load()
    args = lambda **k: [k.get("inp", _p(inp)), k.get("ld_in", ld), k.get("n", None), k.get("n_max", n_max), k.get("bits", _p(depth)),  # noqa: E731
                        k.get("out", _p(out)), k.get("ld_out", ld), k.get("B", 3), L.stream_ptr()]
    flat = ibuf[GUARD:GUARD + 3 * ld]
    cases = {"null in": dict(inp=None), "null bits": dict(bits=None), "null out": dict(out=None), "B = 0": dict(B=0), "B too large": dict(B=65536),
             "n_max = 0": dict(n_max=0), "n_max too large": dict(n_max=(1 << 30) + 1, ld_in=1 << 31, ld_out=1 << 31),
             "ld_in < n_max": dict(ld_in=n_max - 1), "ld_out < n_max": dict(ld_out=n_max - 1),
             "in off by 2 bytes": dict(inp=C.c_void_p(inp.data_ptr() + 2)), "bits off by 2 bytes": dict(bits=C.c_void_p(depth.data_ptr() + 2)),
             "shifted overlap": dict(out=_p(flat[5:])), "the same start, another stride": dict(out=_p(inp), ld_out=ld + 1, B=2)}
    for what, k in cases.items():
        assert lib.wft_bitcrush_f32(*args(**k)) != 0 and "wft_bitcrush_f32" in L.last_error(), what
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all()) and bool((ibuf[GUARD:-GUARD] == 0.25).all())


# ------------------------------------------------------------------------------------------------------------ wrappers
def test_wrappers_and_frontend():
    case = BY_NAME["room_ir"]
    n_max, T = case["n_max"], case["Ts"][0]
    X = torch.from_numpy(np.nan_to_num(case["X"][:, :n_max], nan=0.0)).to(DEV)
    IR = torch.from_numpy(np.nan_to_num(case["IR"][:, :case["taps_max"]], nan=0.0)).to(DEV)
    n_d = torch.tensor(case["ns"], dtype=torch.int32, device=DEV)
    t_d = torch.tensor(case["Ts"], dtype=torch.int32, device=DEV)
    out = K.fir_conv(X, IR, n_d, t_d)
    assert out is not X and tuple(out.shape) == (3, n_max) and out.dtype == torch.float32
    want = _run(case)[:, :n_max]
    assert np.array_equal(O.bits(out.cpu().numpy()), O.bits(want))
    wide = torch.zeros(3, n_max + 11, device=DEV)
    wide[:, :n_max] = X
    assert torch.equal(K.fir_conv(wide[:, :n_max], IR, n_d, t_d), out)  # a strided view: the same bits
    one = K.fir_conv(X, IR[0, :T])  # one response for every row
    assert np.array_equal(O.bits(one[0].cpu().numpy()), O.bits(want[0]))
    # the frontend: one response, a ragged list, host arrays in, the reference inside the bound
    x_host = X.cpu().numpy()
    irs = [case["IR"][0, :T], case["IR"][2, :700].astype(np.float64), np.array([0.0, 1.0], dtype=np.float32)]
    got = GF.fir_convolve(x_host, irs)
    assert got.is_cuda and tuple(got.shape) == (3, n_max)
    for b, h in enumerate(irs):
        ref = O.reference(x_host[b], n_max, h.astype(np.float32), h.shape[0], n_max)
        lim = O.bound(x_host[b], n_max, h.astype(np.float32), h.shape[0], n_max)
        assert bool((np.abs(got[b].cpu().numpy() - ref) <= lim).all()), b
    single = GF.fir_convolve(x_host[0], torch.from_numpy(irs[0]))
    assert tuple(single.shape) == (n_max,) and torch.equal(single, got[0])
    # bit crush: per-row depths, "none" rows, n, in place
    vals = torch.from_numpy(np.stack([np.roll(O.crush_values(), s) for s in (0, 5, 9)])).to(DEV)
    depths, ns = [6, 0, 14], [vals.shape[1], 1025, 3]
    n_d = torch.tensor(ns, dtype=torch.int32, device=DEV)
    bc = K.bitcrush(vals, depths, n_d)
    for b in range(3):
        want_b = O.bitcrush_numpy(vals[b, :ns[b]].cpu().numpy(), depths[b])
        assert np.array_equal(O.bits(bc[b, :ns[b]].cpu().numpy()), O.bits(want_b)) and not bc[b, ns[b]:].view(torch.int32).any(), b
    assert torch.equal(K.bitcrush(vals, torch.tensor(depths, dtype=torch.int32, device=DEV), n_d), bc)  # device-side depths
    y = vals.clone()
    assert K.bitcrush(y, depths, n_d, out=y) is y and torch.equal(y, bc)
    two = GF.bit_crush(vals.cpu().numpy(), [0, 8, 24])
    assert two.is_cuda and torch.equal(two[0], vals[0]) and not torch.equal(two[1], vals[1])
    assert np.array_equal(O.bits(GF.bit_crush(vals[2].cpu(), 8).cpu().numpy()), O.bits(O.bitcrush_numpy(vals[2].cpu().numpy(), 8)))


# ------------------------------------------------------------------------------------------------------------ loader
N_MELS = 80
SPEC = {"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 1.0}
EXT = {"low_freq_range": 5, "high_freq_range": 5}
STRETCH = dict(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25)
OFFICE = {"crush": {"p": 1.0}, "room": {"p": 1.0}}
WAVE = {"noise": {"p": 1.0}}


def _loader(**kw):
    return DL.get_dataloader(DL.SyntheticDataset(3, with_timestamps=True), DL.SimpleTokenizer(), batch_size=3, n_mels=N_MELS, shuffle=False,
                             device=DEV, no_timestamp_training=True, spec_augment=True, spec_augment_params=SPEC, extremes_spec_augment=True,
                             extremes_spec_augment_params=EXT, **kw)


def _seed():
    torch.manual_seed(11)
    random.seed(11)


def _office_replay(x, table, n):
    """CRUSH -> ROOM from the public pieces."""
    t = table.numpy()
    taps = t[:, 1].astype(np.int32)
    x = K.bitcrush(x, t[:, 0].astype(np.int32), n)
    ir = torch.from_numpy(t[:, 2:2 + int(taps.max())].astype(np.float32)).to(DEV)
    return K.fir_conv(x, ir, n, torch.from_numpy(taps).to(DEV))


def test_loader_batch_with_stretch_equals_a_replay_in_the_stated_order():
    from whisper_finetune.data import wave_fx as WF

    on = _loader(office_aug=OFFICE, wave_aug=WAVE, filter_aug={"p": 1.0}, **STRETCH)
    assert isinstance(on, DL.GpuMelLoader) and on.office_aug and on.wave_aug and on.filter_aug and on.stretch and not on.rate_aug
    _seed()
    mel, y_in, y_out = next(iter(on))
    _seed()
    audio, yi, yo, params, ext, cut, rates, sos, wtable, table = next(iter(on.loader))
    assert table.dtype == torch.float64 and tuple(table.shape) == (3, 2 + 2048) and bool((table[:, :2] > 0).all())
    rec = WF.check_records(WF.records_from_table(wtable))
    x, n_out = K.time_stretch(audio.to(DEV), rates)
    before = x.clone()
    x = _office_replay(x, table, n_out)
    assert not torch.equal(x, before)
    x = K.wave_fx(x, rec, "noise", n_out)
    x = K.sos_filter(x, sos, n_out)
    keep = cut.clamp(max=3000).to(torch.int32).to(DEV)
    want = K.specaug(K.logmel_ragged(x, n_out, keep, on.frontend.filters, 3000), params.to(DEV), ext.to(DEV))
    assert tuple(mel.shape) == (3, N_MELS, 3000) and torch.equal(mel, want)
    assert torch.equal(y_in.cpu(), yi) and torch.equal(y_out.cpu(), yo)


def test_loader_batch_without_the_stretch_equals_a_replay_and_inactive_rows_keep_their_bits():
    on = _loader(office_aug=OFFICE)
    assert on.office_aug and not on.wave_aug and not on.filter_aug and not on.stretch
    _seed()
    mel = next(iter(on))[0]
    _seed()
    audio, yi, yo, params, ext, cut, table = next(iter(on.loader))
    x = _office_replay(audio.to(DEV), table, None)
    plain = K.logmel(x, on.frontend.filters, 3000)
    for b in (cut < 3000).nonzero().flatten().tolist():
        c = int(cut[b])
        plain[b, :, c:] = plain[b, :, :c].min() if c > 0 else plain[b].min()
    assert torch.equal(mel, K.specaug(plain, params.to(DEV), ext.to(DEV))) and not torch.equal(x.cpu(), audio)
    # a row with neither effect keeps its bits; a stage without an active row launches nothing
    t = OF.none_table(2048, 3)
    t[1] = table[1].numpy()
    y = DL.office_rows(audio.to(DEV).clone(), None, OF.check_table(t))
    assert torch.equal(y[0].cpu(), audio[0]) and torch.equal(y[2].cpu(), audio[2]) and torch.equal(y[1], x[1])


@pytest.mark.parametrize("stretch", [False, True])
def test_loader_without_the_option_and_with_both_gates_at_zero_gives_the_batches_of_before(stretch, monkeypatch):
    kw = STRETCH if stretch else {}
    off = _loader(**kw)
    assert not off.office_aug
    _seed()
    got = next(iter(off))
    _seed()
    batch = next(iter(off.loader))
    assert len(batch) == 6 + int(stretch)
    # the parent commit's code path: [stretch ->] log-mel -> cut -> SpecAugment, nothing else
    if stretch:
        x, n_out = K.time_stretch(batch[0].to(DEV), batch[6])
        keep = batch[5].clamp(max=3000).to(torch.int32).to(DEV)
        plain = K.logmel_ragged(x, n_out, keep, off.frontend.filters, 3000)
    else:
        plain = K.logmel(batch[0].to(DEV), off.frontend.filters, 3000)
        for b in (batch[5] < 3000).nonzero().flatten().tolist():
            c = int(batch[5][b])
            plain[b, :, c:] = plain[b, :, :c].min() if c > 0 else plain[b].min()
    assert torch.equal(got[0], K.specaug(plain, batch[3].to(DEV), batch[4].to(DEV)))
    if not stretch:  # both gates at zero: two failed draws per clip, after everything else; the same batches and no launch
        # (with the stretch the two extra draws of clip i move the rate that Python's `random` gives clip i + 1)
        zero = _loader(office_aug={"crush": {"p": 0.0}, "room": {"p": 0.0}})
        for name in ("bitcrush", "fir_conv"):
            monkeypatch.setattr(K, name, lambda *a, **k: pytest.fail("a batch without any office effect must launch nothing"))
        _seed()
        again = next(iter(zero))
        for u, v in zip(again, got):
            assert torch.equal(u, v)


def test_calculate_mel_equals_the_batch_path_on_one_row():
    ds = DL.AudioDataset(DL.SyntheticDataset(2), DL.SimpleTokenizer(), device=DEV, n_mels=N_MELS, office_aug=OFFICE, **STRETCH)
    clip = ds.hu_dataset[0]["audio"]["array"]
    audio = np.pad(clip, (0, 480000 - clip.shape[0]))
    random.seed(5)
    mel = ds._calculate_mel(audio, 4.0, True)
    random.seed(5)
    rate = ds._draw_stretch_rate()
    row, n_out = K.time_stretch(torch.from_numpy(audio).to(DEV)[None], [rate])
    table = torch.from_numpy(OF.OfficeAug(16000, **OFFICE).draw()[1][None])
    row = _office_replay(row, table, n_out)
    want = K.logmel_ragged(row, n_out, torch.tensor([400], dtype=torch.int32, device=DEV), GF.mel_filters(N_MELS).to(DEV), 3000)[0]
    assert torch.equal(mel, want)


def test_finetune_runs_three_steps_with_the_office_augmentation(tmp_path, monkeypatch):
    """configs/DEBUG_synthetic_office.yaml: the rate config plus audio_augment.wft_office_aug.  Training micro-batches go through the
    stretch and, where a clip drew one, through the bit crush in place and the room's convolution; the dev loaders never do."""
    from pathlib import Path

    import yaml

    import whisper_finetune.runtime as rt
    from whisper_finetune.scripts import finetune

    cfg = yaml.safe_load((Path(__file__).resolve().parents[1] / "configs" / "DEBUG_synthetic_office.yaml").read_text())
    aa = cfg["augmentation"]["audio_augment"]
    assert aa["apply_baseline_aug"] is True and aa["apply_office_aug"] is False and set(aa["wft_office_aug"]) == set(OF.STAGES)
    cfg["save_dir"] = str(tmp_path)
    calls = []
    crush, conv = K.bitcrush, K.fir_conv
    monkeypatch.setattr(K, "bitcrush", lambda a, d, n=None, out=None: calls.append(("crush", tuple(a.shape), out is a)) or crush(a, d, n, out=out))
    monkeypatch.setattr(K, "fir_conv", lambda a, h, n=None, t=None: calls.append(("room", tuple(a.shape), tuple(h.shape))) or conv(a, h, n, t))
    losses = finetune.main(cfg)
    rt.cleanup()
    assert cfg["training"]["train_steps"] == 3 and len(losses) == 3 and all(np.isfinite(l) for l in losses)
    kinds = [c[0] for c in calls]
    assert 1 <= kinds.count("crush") <= 6 and 1 <= kinds.count("room") <= 6  # six training micro-batches, gates at 0.5 per clip
    assert all(c[1][0] == 2 and (c[2] is True if c[0] == "crush" else (c[2][0] == 2 and 81 <= c[2][1] <= 2048)) for c in calls)
