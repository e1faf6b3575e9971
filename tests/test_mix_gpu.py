"""Mix effects on the device: wft_loudness_f32 against the float64 reference of tests/_mix_cases.py under the derived bounds (rows
around the block count's seams and the chunk group's seam, the three-level row, copied rows, poisoned padding, sentinel-filled
buffers compared whole), its independence statements bit for bit, every refusal; wft_bg_mix_f32 under the counted bound over every
entry length and offset with +-1e6 neighbours in the bank; the wrappers and the loader's stages against replays from the public
pieces."""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _mix_cases as M  # noqa: E402
from whisper_finetune.data import data_loader as DL  # noqa: E402
from whisper_finetune.data import gpu_frontend as GF  # noqa: E402
from whisper_finetune.data import mix_fx as MF  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = torch.device("cuda:0")
SENT = float(M.SENTINEL)
GUARD = 64


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _guarded(host, fill=None, dtype=torch.float32):
    """A numpy array (or a shape with `fill`) -> (its device copy as a view inside a guarded buffer, the whole buffer)."""
    shape = host if isinstance(host, tuple) else host.shape
    dtype = dtype if isinstance(host, tuple) else torch.from_numpy(host).dtype
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT if fill is None else fill, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(*shape)
    if not isinstance(host, tuple):
        view.copy_(torch.from_numpy(host))
    return view, buf


def _whole(buf, shape):
    whole = buf.cpu().numpy()
    assert bool((whole[:GUARD] == SENT).all() and (whole[-GUARD:] == SENT).all()), "guards"
    return whole[GUARD:-GUARD].reshape(shape)


def _poisoned_workspace(nbytes):
    return torch.full((nbytes // 8 + 2 * GUARD,), float("nan"), dtype=torch.float64, device=DEV)


def _loud(X, ns, rate, targets=None, modes=None, n_max=None, in_place=False, measure=False, use_n=True):
    """The raw call on guarded buffers -> (the whole output buffer [B, ld] as numpy or None, stats [B, 4]), guards checked."""
    B, ld = X.shape
    n_max = ld - M.PAD if n_max is None else n_max
    hop = rate // 10
    x_d, xbuf = _guarded(np.ascontiguousarray(X))
    out, obuf = (None, None) if measure else ((x_d, xbuf) if in_place else _guarded((B, ld)))
    stats, sbuf = _guarded((B, 4), dtype=torch.float64)
    n_d = torch.tensor(ns, dtype=torch.int32, device=DEV) if use_n else None
    t_d = None if targets is None else torch.tensor(targets, dtype=torch.float64, device=DEV)
    m_d = None if modes is None else torch.tensor(modes, dtype=torch.int32, device=DEV)
    sos = MF.k_weighting(rate)
    lib = L.load()
    nbytes = lib.wft_loudness_workspace_bytes(B, n_max, hop)
    ws = _poisoned_workspace(nbytes)
    L.check(lib.wft_loudness_f32(_p(x_d), ld, _p(n_d), n_max, sos.ctypes.data, hop, _p(t_d), _p(m_d), _p(out), ld, _p(stats), _p(ws[GUARD:]),
                                 nbytes, B, L.stream_ptr()), "wft_loudness_f32")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[:GUARD]).all() and torch.isnan(ws[GUARD + nbytes // 8:]).all()), "guards of the workspace"
    return (None if measure else _whole(obuf, (B, ld))), _whole(sbuf, (B, 4))


def _stat(row):
    return dict(L=row[0], gamma=row[1], over=row[2], gain=row[3])


def _check_loud_rows(case, out, stats, modes=None):
    worst = 0.0
    for b, ref in enumerate(case["refs"]):
        n, name = case["ns"][b], case["names"][b]
        x = case["X"][b, :n]
        if modes is not None and not modes[b]:
            assert stats[b].tolist() == [-math.inf, -math.inf, 0.0, 1.0], name
            want = x
        else:
            ok, complaint = M.loud_check(_stat(stats[b]), ref, case["hop"])
            assert ok, (name, complaint)
            if math.isfinite(ref["L"]):
                worst = max(worst, abs(stats[b, 0] - ref["L"]) / M.level_bound(ref, case["hop"], "J2"))
            gain = np.float32(stats[b, 3])
            assert float(gain) == stats[b, 3] and (ref["active"] or stats[b, 3] == 1.0), name
            want = x * gain if ref["active"] else x  # one f32 multiply by the DEVICE's gain, bit for bit; a copy otherwise
        if out is not None:
            assert np.array_equal(M.bits(out[b, :n]), M.bits(want)), name
    return worst


# ------------------------------------------------------------------------------------------------------------ loudness
@pytest.fixture(scope="module")
def loud_batch():
    case = M.loud_case()
    B = len(case["ns"])
    out, stats = _loud(case["X"], case["ns"], 16000, case["targets"], [1] * B)
    return case, out, stats


def test_loudness_stats_inside_the_derived_bounds_and_output_is_one_multiply(loud_batch):
    case, out, stats = loud_batch
    worst = _check_loud_rows(case, out, stats)
    print(f"largest |L - ref| / bound over the 16 kHz rows: {worst:.3e}")
    for b, n in enumerate(case["ns"]):
        assert not M.bits(out[b, n:case["n_max"]]).any(), "zeros behind n[b]"
        assert bool((out[b, case["n_max"]:] == M.SENTINEL).all()), "nothing at or behind n_max is written"
    names = case["names"]
    for name in ("noise_n6399", "zeros", "amplitude_1e-5"):  # copied bit for bit, L = -inf
        b = names.index(name)
        assert stats[b, 0] == -math.inf and stats[b, 2] == 0 and stats[b, 3] == 1.0
        assert np.array_equal(M.bits(out[b, :case["ns"][b]]), M.bits(case["X"][b, :case["ns"][b]]))
    assert [int(stats[names.index(f"noise_n{n}"), 2]) for n in (6400, 7199, 7200, 7201, 8800)] == [1, 1, 1, 2, 3]
    assert int(stats[names.index("three_level"), 2]) == 10


def test_loudness_a_row_alone_a_rerun_and_other_partners_are_bit_equal(loud_batch):
    case, out, stats = loud_batch
    B = len(case["ns"])
    again, stats2 = _loud(case["X"], case["ns"], 16000, case["targets"], [1] * B)
    assert np.array_equal(M.bits(again), M.bits(out)) and np.array_equal(stats2.view(np.uint64), stats.view(np.uint64)), "rerun"
    for b in range(B):
        n = case["ns"][b]
        one, s1 = _loud(case["X"][b:b + 1], [n], 16000, case["targets"][b:b + 1], [1])
        assert np.array_equal(M.bits(one[0, :n]), M.bits(out[b, :n])) and np.array_equal(s1[0].view(np.uint64), stats[b].view(np.uint64)), case["names"][b]
    rev, srev = _loud(case["X"][::-1], case["ns"][::-1], 16000, case["targets"][::-1], [1] * B)
    assert np.array_equal(M.bits(rev[::-1]), M.bits(out)) and np.array_equal(srev[::-1].view(np.uint64), stats.view(np.uint64)), "other partners"
    # a narrower buffer (another n_max, so other launch sizes): the short rows keep their bits
    short = [b for b in range(B) if case["ns"][b] <= 8800]
    Xs = np.ascontiguousarray(case["X"][short][:, :8800 + M.PAD])
    narrow, sn = _loud(Xs, [case["ns"][b] for b in short], 16000, [case["targets"][b] for b in short], [1] * len(short))
    for k, b in enumerate(short):
        n = case["ns"][b]
        assert np.array_equal(M.bits(narrow[k, :n]), M.bits(out[b, :n])) and np.array_equal(sn[k].view(np.uint64), stats[b].view(np.uint64))


def test_loudness_in_place_measure_only_modes_and_null_lengths(loud_batch):
    case, out, stats = loud_batch
    B, n_max = len(case["ns"]), case["n_max"]
    inp, s_in = _loud(case["X"], case["ns"], 16000, case["targets"], [1] * B, in_place=True)
    assert np.array_equal(s_in.view(np.uint64), stats.view(np.uint64))
    for b, n in enumerate(case["ns"]):
        assert np.array_equal(M.bits(inp[b, :n]), M.bits(out[b, :n])), case["names"][b]
        assert np.array_equal(M.bits(inp[b, n:]), M.bits(case["X"][b, n:])), "in place nothing behind n[b] is touched"
    _, s_m = _loud(case["X"], case["ns"], 16000, case["targets"], [1] * B, measure=True)
    assert np.array_equal(s_m.view(np.uint64), stats.view(np.uint64)), "measure only: the same stats"
    _, s_0 = _loud(case["X"], case["ns"], 16000, measure=True)  # no target, no mode: every row is measured, no gain
    assert np.array_equal(s_0[:, :3].view(np.uint64), stats[:, :3].view(np.uint64)) and bool((s_0[:, 3] == 1.0).all())
    modes = [b % 3 != 1 for b in range(B)]
    some, s_some = _loud(case["X"], case["ns"], 16000, case["targets"], [int(m) for m in modes])
    _check_loud_rows(case, some, s_some, modes)
    for b in range(B):
        if modes[b]:
            assert np.array_equal(M.bits(some[b]), M.bits(out[b])) and np.array_equal(s_some[b].view(np.uint64), stats[b].view(np.uint64))
    # a target that is not finite copies the row
    nan_t, s_nan = _loud(case["X"][:2], case["ns"][:2], 16000, [float("nan"), float("inf")], [1, 1])
    assert bool((s_nan[:, 3] == 1.0).all()) and np.array_equal(M.bits(nan_t[1, :6400]), M.bits(case["X"][1, :6400]))
    # n == NULL: every row covers n_max samples
    b = case["names"].index("noise_n7201")
    X = np.ascontiguousarray(np.stack([case["X"][b, :7201], case["X"][b + 1, :7201]]))
    full, s_full = _loud(X, None, 16000, [case["targets"][b], -20.0], [1, 1], n_max=7201, use_n=False)
    assert np.array_equal(s_full[0].view(np.uint64), stats[b].view(np.uint64)) and np.array_equal(M.bits(full[0]), M.bits(out[b, :7201]))
    ref1 = M.loud_ref(X[1], 7201, 16000, -20.0)
    assert M.loud_check(_stat(s_full[1]), ref1, 1600)[0]
    # device lengths outside [0, n_max] are clamped
    wild, s_wild = _loud(X, [7201 + 100, -5], 16000, [case["targets"][b], -20.0], [1, 1], n_max=7201)
    assert np.array_equal(M.bits(wild[0]), M.bits(full[0])) and s_wild[1].tolist() == [-math.inf, -math.inf, 0.0, 1.0] and not M.bits(wild[1]).any()


@pytest.mark.parametrize("rate", [8000, 48000])
def test_loudness_at_another_rate(rate):
    case = M.loud_case(rate)
    out, stats = _loud(case["X"], case["ns"], rate, case["targets"], [1])
    worst = _check_loud_rows(case, out, stats)
    print(f"{rate} Hz: L = {stats[0, 0]!r} against {case['refs'][0]['L']!r}, |dL| / bound = {worst:.3e}")
    assert not M.bits(out[0, case["ns"][0]:case["n_max"]]).any()


def test_loudness_refusals_leave_the_buffers_untouched():
    n_max, ld, hop = 8000, 8004, 1600
    inp, ibuf = _guarded((3, ld), fill=0.25)
    out, obuf = _guarded((3, ld))
    stats, sbuf = _guarded((3, 4), dtype=torch.float64)
    lib = L.load()
    nbytes = lib.wft_loudness_workspace_bytes(3, n_max, hop)
    ws = torch.zeros(nbytes // 8 + 2, dtype=torch.float64, device=DEV)
    n = torch.full((3,), n_max, dtype=torch.int32, device=DEV)
    tg = torch.full((4,), -20.0, dtype=torch.float64, device=DEV)
    md = torch.ones(4, dtype=torch.int32, device=DEV)
    sos = MF.k_weighting(16000)
    pad = np.zeros(13, dtype=np.float64)
    pad[1:] = sos.reshape(-1)
    a0, nan = sos.copy(), sos.copy()
    a0[1, 3], nan[0, 2] = 2.0, float("nan")
    args = lambda **k: [k.get("inp", _p(inp)), k.get("ld_in", ld), k.get("n", _p(n)), k.get("n_max", n_max), k.get("sos", sos.ctypes.data),  # noqa: E731
                        k.get("hop", hop), k.get("target", _p(tg)), k.get("mode", _p(md)), k.get("out", _p(out)), k.get("ld_out", ld),
                        k.get("stats", _p(stats)), k.get("ws", _p(ws)), k.get("nbytes", nbytes), k.get("B", 3), L.stream_ptr()]
    assert lib.wft_loudness_f32(*args()) == 0  # the base call is accepted ...
    torch.cuda.synchronize()
    assert not bool((out[:, :n_max] == SENT).any()) and not bool((stats == SENT).any())
    obuf.fill_(SENT); sbuf.fill_(SENT); ws.zero_()  # ... and every variation below is not
    flat = ibuf[GUARD:GUARD + 3 * ld]
    cases = {"null in": dict(inp=None), "null sos": dict(sos=None), "null stats": dict(stats=None), "null workspace": dict(ws=None),
             "an output without target": dict(target=None), "an output without mode": dict(mode=None),
             "B = 0": dict(B=0), "B too large": dict(B=65536), "n_max = 0": dict(n_max=0),
             "n_max too large": dict(n_max=(1 << 30) + 1, ld_in=1 << 31, ld_out=1 << 31, nbytes=1 << 40), "hop too small": dict(hop=511),
             "hop too large": dict(hop=(1 << 24) + 1), "ld_in < n_max": dict(ld_in=n_max - 1), "ld_out < n_max": dict(ld_out=n_max - 1),
             "short workspace": dict(nbytes=nbytes - 1), "in off by 2 bytes": dict(inp=C.c_void_p(inp.data_ptr() + 2)),
             "out off by 2 bytes": dict(out=C.c_void_p(out.data_ptr() + 2)), "n off by 2 bytes": dict(n=C.c_void_p(n.data_ptr() + 2)),
             "mode off by 2 bytes": dict(mode=C.c_void_p(md.data_ptr() + 2)), "target off by 4 bytes": dict(target=C.c_void_p(tg.data_ptr() + 4)),
             "stats off by 4 bytes": dict(stats=C.c_void_p(stats.data_ptr() + 4)), "workspace off by 4 bytes": dict(ws=C.c_void_p(ws.data_ptr() + 4)),
             "sos off by 4 bytes": dict(sos=pad.ctypes.data + 4), "a0 != 1": dict(sos=a0.ctypes.data), "a coefficient that is not finite": dict(sos=nan.ctypes.data),
             "shifted overlap": dict(out=_p(flat[5:])), "the same start, another stride": dict(out=_p(inp), ld_out=ld + 1, B=2)}
    for what, k in cases.items():
        assert lib.wft_loudness_f32(*args(**k)) != 0 and "wft_loudness_f32" in L.last_error(), what
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all()) and bool((sbuf == SENT).all()) and bool((ibuf[GUARD:-GUARD] == 0.25).all()) and not bool(ws.any())


# ------------------------------------------------------------------------------------------------------------ background noise
def _bg(X, ns, bank, off, recs, n_max=None, in_place=False, use_n=True):
    """The raw call on guarded buffers -> (the whole output buffer [B, ld], stats [B, 3]), guards checked."""
    B, ld = X.shape
    n_max = ld - M.PAD if n_max is None else n_max
    x_d, xbuf = _guarded(np.ascontiguousarray(X))
    out, obuf = (x_d, xbuf) if in_place else _guarded((B, ld))
    stats, sbuf = _guarded((B, 3), dtype=torch.float64)
    n_d = torch.tensor(ns, dtype=torch.int32, device=DEV) if use_n else None
    bank_d, off_d = torch.from_numpy(bank).to(DEV), torch.from_numpy(off).to(DEV)
    rec = M.bg_records(recs)
    rec_d = torch.from_numpy(rec.view("u1").reshape(B, 24).copy()).to(DEV)
    lib = L.load()
    nbytes = lib.wft_bg_mix_workspace_bytes(B, n_max)
    ws = _poisoned_workspace(nbytes)
    L.check(lib.wft_bg_mix_f32(_p(x_d), ld, _p(n_d), n_max, _p(bank_d), _p(off_d), off.shape[0] - 1, _p(rec_d), _p(out), ld, _p(stats),
                               _p(ws[GUARD:]), nbytes, B, L.stream_ptr()), "wft_bg_mix_f32")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[:GUARD]).all() and torch.isnan(ws[GUARD + nbytes // 8:]).all()), "guards of the workspace"
    return _whole(obuf, (B, ld)), _whole(sbuf, (B, 3))


@pytest.fixture(scope="module")
def bg_batch():
    case = M.bg_case()
    out, stats = _bg(case["X"], case["ns"], case["bank"], case["off"], case["recs"])
    return case, out, stats


def test_bg_mix_stats_and_every_element_inside_the_counted_bound(bg_batch):
    case, out, stats = bg_batch
    for b, ref in enumerate(case["refs"]):
        n = case["ns"][b]
        ok, complaint = M.bg_check(out[b, :n], stats[b], case["X"][b], n, ref)
        assert ok, (b, n, case["recs"][b], case["lengths"][case["recs"][b][1]], complaint)
        assert not M.bits(out[b, n:case["n_max"]]).any(), "zeros behind n[b]"
        assert bool((out[b, case["n_max"]:] == M.SENTINEL).all())
    copied = [b for b, r in enumerate(case["refs"]) if r["out64"] is None]
    assert len(copied) == 3 and all(stats[b, 2] == 0.0 for b in copied)
    assert stats[-1].tolist() == [0.0, 0.0, 0.0]  # the "none" row
    assert float(np.abs(out[:, :case["n_max"]][np.isfinite(out[:, :case["n_max"]])]).max()) < 10.0  # no +-1e6 neighbour leaked


def test_bg_mix_alone_in_place_and_rerun_are_bit_equal(bg_batch):
    case, out, stats = bg_batch
    again, s2 = _bg(case["X"], case["ns"], case["bank"], case["off"], case["recs"])
    assert np.array_equal(M.bits(again), M.bits(out)) and np.array_equal(s2.view(np.uint64), stats.view(np.uint64)), "rerun"
    inp, s3 = _bg(case["X"], case["ns"], case["bank"], case["off"], case["recs"], in_place=True)
    assert np.array_equal(s3.view(np.uint64), stats.view(np.uint64))
    for b, n in enumerate(case["ns"]):
        assert np.array_equal(M.bits(inp[b, :n]), M.bits(out[b, :n])), b
        assert np.array_equal(M.bits(inp[b, n:]), M.bits(case["X"][b, n:])), "in place nothing behind n[b] is touched"
    B = len(case["ns"])
    for b in list(range(0, B, 9)) + [B - 3, B - 2, B - 1]:
        n = case["ns"][b]
        one, s1 = _bg(case["X"][b:b + 1], [n], case["bank"], case["off"], case["recs"][b:b + 1])
        assert np.array_equal(M.bits(one[0, :n]), M.bits(out[b, :n])) and np.array_equal(s1[0].view(np.uint64), stats[b].view(np.uint64)), b
    # n == NULL and clamped device lengths, on the rows of n = 4097
    rows = [b for b in range(B) if case["ns"][b] == 4097][:4]
    X = np.ascontiguousarray(case["X"][rows][:, :4097])
    full, sf = _bg(X, None, case["bank"], case["off"], [case["recs"][b] for b in rows], n_max=4097, use_n=False)
    wild, sw = _bg(X, [5000, 4097, 1 << 30, 4097], case["bank"], case["off"], [case["recs"][b] for b in rows], n_max=4097)
    for k, b in enumerate(rows):
        assert np.array_equal(M.bits(full[k]), M.bits(out[b, :4097])) and np.array_equal(sf[k].view(np.uint64), stats[b].view(np.uint64))
    assert np.array_equal(M.bits(wild), M.bits(full))
    zero, sz = _bg(X, [0, -3, 4097, 4097], case["bank"], case["off"], [case["recs"][b] for b in rows], n_max=4097)
    assert not M.bits(zero[:2]).any() and not sz[:2].any() and np.array_equal(M.bits(zero[2:]), M.bits(full[2:]))


def test_bg_mix_refusals_leave_the_buffers_untouched():
    n_max, ld = 1500, 1504
    inp, ibuf = _guarded((3, ld), fill=0.25)
    out, obuf = _guarded((3, ld))
    stats, sbuf = _guarded((3, 3), dtype=torch.float64)
    bank = torch.full((64,), 0.125, device=DEV)
    off = torch.tensor([0, 10, 64, 64], dtype=torch.int64, device=DEV)
    rec = torch.from_numpy(M.bg_records([(1, 0, 0, 3.0), (2, 1, 5, -20.0), (0, 0, 0, 0.0), (0, 0, 0, 0.0)]).view("u1").copy()).to(DEV)
    lib = L.load()
    nbytes = lib.wft_bg_mix_workspace_bytes(3, n_max)
    ws = torch.zeros(nbytes // 8 + 2, dtype=torch.float64, device=DEV)
    n = torch.full((4,), n_max, dtype=torch.int32, device=DEV)
    args = lambda **k: [k.get("inp", _p(inp)), k.get("ld_in", ld), k.get("n", _p(n)), k.get("n_max", n_max), k.get("bank", _p(bank)),  # noqa: E731
                        k.get("off", _p(off)), k.get("K", 2), k.get("rec", _p(rec)), k.get("out", _p(out)), k.get("ld_out", ld),
                        k.get("stats", _p(stats)), k.get("ws", _p(ws)), k.get("nbytes", nbytes), k.get("B", 3), L.stream_ptr()]
    assert lib.wft_bg_mix_f32(*args()) == 0  # the base call is accepted ...
    torch.cuda.synchronize()
    assert not bool((out[:, :n_max] == SENT).any()) and not bool((stats == SENT).any())
    obuf.fill_(SENT); sbuf.fill_(SENT); ws.zero_()  # ... and every variation below is not
    flat = ibuf[GUARD:GUARD + 3 * ld]
    cases = {"null in": dict(inp=None), "null bank": dict(bank=None), "null bank_off": dict(off=None), "null rec": dict(rec=None),
             "null out": dict(out=None), "null stats": dict(stats=None), "null workspace": dict(ws=None), "K = 0": dict(K=0),
             "B = 0": dict(B=0), "B too large": dict(B=65536), "n_max = 0": dict(n_max=0),
             "n_max too large": dict(n_max=(1 << 30) + 1, ld_in=1 << 31, ld_out=1 << 31, nbytes=1 << 40),
             "ld_in < n_max": dict(ld_in=n_max - 1), "ld_out < n_max": dict(ld_out=n_max - 1), "short workspace": dict(nbytes=nbytes - 1),
             "in off by 2 bytes": dict(inp=C.c_void_p(inp.data_ptr() + 2)), "out off by 2 bytes": dict(out=C.c_void_p(out.data_ptr() + 2)),
             "n off by 2 bytes": dict(n=C.c_void_p(n.data_ptr() + 2)), "bank off by 2 bytes": dict(bank=C.c_void_p(bank.data_ptr() + 2)),
             "bank_off off by 4 bytes": dict(off=C.c_void_p(off.data_ptr() + 4)), "rec off by 4 bytes": dict(rec=C.c_void_p(rec.data_ptr() + 4)),
             "stats off by 4 bytes": dict(stats=C.c_void_p(stats.data_ptr() + 4)), "workspace off by 4 bytes": dict(ws=C.c_void_p(ws.data_ptr() + 4)),
             "shifted overlap": dict(out=_p(flat[5:])), "the same start, another stride": dict(out=_p(inp), ld_out=ld + 1, B=2)}
    for what, k in cases.items():
        assert lib.wft_bg_mix_f32(*args(**k)) != 0 and "wft_bg_mix_f32" in L.last_error(), what
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all()) and bool((sbuf == SENT).all()) and bool((ibuf[GUARD:-GUARD] == 0.25).all()) and not bool(ws.any())


# ------------------------------------------------------------------------------------------------------------ wrappers
def test_wrappers_and_frontend(loud_batch, bg_batch):
    case, out, stats = loud_batch
    n_max, B = case["n_max"], len(case["ns"])
    X = torch.from_numpy(np.nan_to_num(case["X"][:, :n_max], nan=0.0)).to(DEV)
    n_d = torch.tensor(case["ns"], dtype=torch.int32, device=DEV)
    got, st = K.loudness(X, 16000, case["targets"], n_d)
    assert got is not X and np.array_equal(M.bits(got.cpu().numpy()), M.bits(out[:, :n_max])) and np.array_equal(st.cpu().numpy().view(np.uint64), stats.view(np.uint64))
    none, st0 = K.loudness(X, 16000, n=n_d)  # measure only
    assert none is None and torch.equal(st0[:, :3], st[:, :3])
    y = X.clone()
    same, st1 = K.loudness(y, 16000, case["targets"], n_d, out=y)
    assert same is y and torch.equal(y, got) and torch.equal(st1, st)
    nan_t = [float("nan")] * B
    kept, st2 = K.loudness(X, 16000, nan_t, n_d)  # no row has a target: nothing is launched, the rows are copied
    assert torch.equal(kept, torch.where(torch.arange(n_max, device=DEV)[None] < n_d[:, None], X, torch.zeros_like(X))) and bool((st2[:, 3] == 1).all())
    b = case["names"].index("noise_n32768")
    row = case["X"][b, :32768]
    lufs = GF.loudness(row)
    assert lufs.is_cuda and lufs.dtype == torch.float64 and lufs.dim() == 0 and float(lufs) == stats[b, 0]
    two = GF.loudness(np.stack([row, row[::-1].copy()]), 16000)
    assert tuple(two.shape) == (2,) and float(two[0]) == stats[b, 0] and abs(float(two[1]) - stats[b, 0]) < 0.5
    norm = GF.loudness_normalize(row, case["targets"][b])
    assert tuple(norm.shape) == (32768,) and np.array_equal(M.bits(norm.cpu().numpy()), M.bits(out[b, :32768]))
    assert abs(float(GF.loudness(norm)) - case["targets"][b]) < 1e-4  # the gain is an f32: the level lands within its rounding
    assert float(GF.loudness(np.zeros(16000, dtype=np.float32))) == -math.inf and float(GF.loudness(row[:6399])) == -math.inf
    # background noise: one recording for every row and a ragged list, against the raw call's rows
    bcase, bout, bstats = bg_batch
    rows = [r for r in range(len(bcase["ns"])) if bcase["ns"][r] == 4097 and bcase["recs"][r][0] == 1][:3]
    x = np.ascontiguousarray(bcase["X"][rows][:, :4097])
    entries = [bcase["bank"][bcase["off"][bcase["recs"][r][1]]:bcase["off"][bcase["recs"][r][1] + 1]] for r in rows]
    mixed = GF.mix_background(x, entries, snr_db=[bcase["recs"][r][3] for r in rows], offset=[bcase["recs"][r][2] for r in rows])
    assert mixed.is_cuda and tuple(mixed.shape) == (3, 4097)
    for k, r in enumerate(rows):
        assert np.array_equal(M.bits(mixed[k].cpu().numpy()), M.bits(bout[r, :4097])), r
    single = GF.mix_background(x[0], torch.from_numpy(entries[0]), snr_db=bcase["recs"][rows[0]][3], offset=bcase["recs"][rows[0]][2])
    assert tuple(single.shape) == (4097,) and torch.equal(single, mixed[0])
    leave = GF.mix_background(x, entries[0], absolute_rms_db=[-20.0, float("nan"), -20.0])
    assert torch.equal(leave[1].cpu(), torch.from_numpy(x[1])) and not torch.equal(leave[0].cpu(), torch.from_numpy(x[0]))
    ref = M.bg_ref(x[0], 4097, entries[0], np.array([0, len(entries[0])]), (2, 0, 0, -20.0))
    assert M.bg_check(leave[0].cpu().numpy(), (ref["clean"], ref["noise"], ref["scale"]), x[0], 4097, ref)[0]


# ------------------------------------------------------------------------------------------------------------ loader
N_MELS = 80
SPEC = {"time_mask_param": 100, "freq_mask_param": 27, "time_warp_w": 80, "p": 1.0}
EXT = {"low_freq_range": 5, "high_freq_range": 5}
STRETCH = dict(apply_baseline_aug=True, time_stretch_min_rate=0.75, time_stretch_max_rate=1.25)
MIX = {"background": {"p": 1.0, "bank": {"synthetic": 4}}, "loudness": {"p": 1.0}}


def _loader(**kw):
    return DL.get_dataloader(DL.SyntheticDataset(3, with_timestamps=True), DL.SimpleTokenizer(), batch_size=3, n_mels=N_MELS, shuffle=False,
                             device=DEV, no_timestamp_training=True, spec_augment=True, spec_augment_params=SPEC, extremes_spec_augment=True,
                             extremes_spec_augment_params=EXT, **kw)


def _seed():
    torch.manual_seed(11)
    random.seed(11)


def test_loader_batch_equals_a_replay_from_the_public_pieces():
    on = _loader(mix_aug=MIX)
    assert isinstance(on, DL.GpuMelLoader) and on.mix_aug and not on.office_aug and not on.stretch
    _seed()
    mel, y_in, y_out = next(iter(on))
    _seed()
    audio, yi, yo, params, ext, cut, table = next(iter(on.loader))
    t = table.numpy()
    assert table.dtype == torch.float64 and t.shape == (3, 6) and bool((t[:, 0] > 0).all() and (t[:, 4] == 1).all())
    bank = MF.synthetic_bank(4)
    noises = [bank[int(e)] for e in t[:, 1]]
    x = audio.to(DEV)
    x = GF.mix_background(x, noises, snr_db=np.where(t[:, 0] == 1, t[:, 3], np.nan), offset=t[:, 2])
    x = GF.mix_background(x, noises, absolute_rms_db=np.where(t[:, 0] == 2, t[:, 3], np.nan), offset=t[:, 2])
    assert not torch.equal(x.cpu(), audio)
    before = x.clone()
    x = GF.loudness_normalize(x, t[:, 5])
    assert not torch.equal(x, before)
    plain = K.logmel(x, on.frontend.filters, 3000)
    for b in (cut < 3000).nonzero().flatten().tolist():
        c = int(cut[b])
        plain[b, :, c:] = plain[b, :, :c].min() if c > 0 else plain[b].min()
    assert tuple(mel.shape) == (3, N_MELS, 3000) and torch.equal(mel, K.specaug(plain, params.to(DEV), ext.to(DEV)))
    assert torch.equal(y_in.cpu(), yi) and torch.equal(y_out.cpu(), yo)
    lufs = GF.loudness(x)
    assert bool((torch.abs(lufs.cpu() - torch.from_numpy(t[:, 5])) < 1e-4).all())  # the padded clips sit at their targets


def test_loader_batch_with_stretch_and_every_option_runs_the_stages_in_the_stated_order():
    from whisper_finetune.data import wave_fx as WF

    on = _loader(mix_aug=MIX, wave_aug={"noise": {"p": 1.0}}, **STRETCH)
    _seed()
    mel = next(iter(on))[0]
    _seed()
    audio, yi, yo, params, ext, cut, rates, wtable, table = next(iter(on.loader))
    t = MF.check_table(table, on._bank.lengths)
    rec = WF.check_records(WF.records_from_table(wtable))
    x, n_out = K.time_stretch(audio.to(DEV), rates)
    x, _ = K.bg_mix(x, on._bank.bank, on._bank.off, MF.records_from_table(t), n_out)
    x = K.wave_fx(x, rec, "noise", n_out)
    x, _ = K.loudness(x, 16000, t[:, 5], n_out)
    keep = cut.clamp(max=3000).to(torch.int32).to(DEV)
    want = K.specaug(K.logmel_ragged(x, n_out, keep, on.frontend.filters, 3000), params.to(DEV), ext.to(DEV))
    assert torch.equal(mel, want)


def test_bank_at_another_rate_is_resampled_once_and_matches_the_lengths_of_the_draws():
    g = np.random.default_rng(5)
    entries = [(0.1 * g.standard_normal(m)).astype(np.float32) for m in (4800, 10001, 7)]
    aug = MF.MixAug(16000, background={"bank": entries, "bank_sample_rate": 48000})
    assert aug.lengths == [1600, 3334, 3]
    bank = DL.DeviceBank(aug, DEV)
    assert bank.lengths == aug.lengths and bank.off.tolist() == [0, 1600, 4934, 4937] and bank.bank.dtype == torch.float32 and bank.bank.is_cuda
    assert torch.equal(bank.bank, torch.cat([GF.resample(e, 48000, DEV) for e in entries]))
    same = DL.DeviceBank(MF.MixAug(16000, background={"bank": entries}), DEV)  # at the clips' own rate: the entries as they are
    assert same.lengths == [4800, 10001, 7] and torch.equal(same.bank.cpu(), torch.from_numpy(np.concatenate(entries)))


def test_loader_with_both_gates_at_zero_gives_the_batches_of_before_and_launches_nothing(monkeypatch):
    off = _loader()
    _seed()
    got = next(iter(off))
    zero = _loader(mix_aug={"background": {"p": 0.0, "bank": {"synthetic": 4}}, "loudness": {"p": 0.0}})
    for name in ("bg_mix", "loudness"):
        monkeypatch.setattr(K, name, lambda *a, **k: pytest.fail("a batch without any mix effect must launch nothing"))
    _seed()
    again = next(iter(zero))
    for u, v in zip(again, got):
        assert torch.equal(u, v)


def test_calculate_mel_equals_the_batch_path_on_one_row():
    ds = DL.AudioDataset(DL.SyntheticDataset(2), DL.SimpleTokenizer(), device=DEV, n_mels=N_MELS, mix_aug=MIX)
    clip = ds.hu_dataset[0]["audio"]["array"]
    audio = np.pad(clip, (0, 480000 - clip.shape[0])).astype(np.float32)
    random.seed(5)
    mel = ds._calculate_mel(audio, None, False)
    random.seed(5)
    names, row = MF.MixAug(16000, **MIX).draw(480000)
    bank = MF.synthetic_bank(4)
    kw = {"snr_db" if names["background"] == "snr" else "absolute_rms_db": row[3]}
    x = GF.mix_background(audio, bank[int(row[1])], offset=int(row[2]), **kw)
    x = GF.loudness_normalize(x, row[5])
    assert torch.equal(mel, K.logmel(x[None], GF.mel_filters(N_MELS).to(DEV), 3000)[0])


def test_finetune_runs_three_steps_with_the_mix_augmentation(tmp_path, monkeypatch):
    """configs/DEBUG_synthetic_mix.yaml: the office config plus audio_augment.wft_mix_aug over a synthetic bank.  Training micro-batches
    go, where a clip drew one, through the background mix and the loudness gain, both in place; the dev loaders never do."""
    from pathlib import Path

    import yaml

    import whisper_finetune.runtime as rt
    from whisper_finetune.scripts import finetune

    cfg = yaml.safe_load((Path(__file__).resolve().parents[1] / "configs" / "DEBUG_synthetic_mix.yaml").read_text())
    aa = cfg["augmentation"]["audio_augment"]
    assert aa["apply_baseline_aug"] is True and aa["apply_advanced_aug"] is False and set(aa["wft_mix_aug"]) == set(MF.STAGES)
    cfg["save_dir"] = str(tmp_path)
    calls = []
    mix, loud = K.bg_mix, K.loudness
    monkeypatch.setattr(K, "bg_mix", lambda a, *r, **k: calls.append(("background", tuple(a.shape), k.get("out") is a)) or mix(a, *r, **k))
    monkeypatch.setattr(K, "loudness", lambda a, *r, **k: calls.append(("loudness", tuple(a.shape), k.get("out") is a)) or loud(a, *r, **k))
    losses = finetune.main(cfg)
    rt.cleanup()
    assert cfg["training"]["train_steps"] == 3 and len(losses) == 3 and all(np.isfinite(l) for l in losses)
    kinds = [c[0] for c in calls]
    assert 1 <= kinds.count("background") <= 6 and 1 <= kinds.count("loudness") <= 6  # six training micro-batches, gates at 0.5 per clip
    assert all(c[1][0] == 2 and c[2] is True for c in calls)
