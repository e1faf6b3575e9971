"""wft_edit_counts_i32 on the device against the references of tests/_edit_cases.py, bit for bit: whole sentinel-filled output buffers
and whole case sets.  Rows of a symbol buffer are separated by one poison value that is the same on both sides of every gap, so a read
past a row's end finds a MATCH and changes the counts instead of faulting."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _edit_cases as EC  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402
from whisper_finetune.eval import metrics as M  # noqa: E402

DEV = torch.device("cuda:0")
SENT = -777     # fills every output buffer
ERR_ARG = -1    # WFT_ERR_ARG
GUARD = 64


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _threads():
    return int(L.load().wft_edit_threads())


def _cap():
    return int(L.load().wft_edit_max_len())


def _table(rows):
    rec = np.zeros(len(rows), dtype=K.EDIT_ROW_DTYPE)
    for p, (ro, ho, n, m) in enumerate(rows):
        rec[p] = (int(ro), int(ho), int(n), int(m), (0, 0))
    return torch.from_numpy(rec.view("u1").reshape(len(rows), 32).copy()).to(DEV)


def _run(sym, rows, max_len=None, ld=4, n_sym=None):
    """The raw entry point on a sentinel-filled [P, ld] buffer with guards around it -> the whole buffer as numpy int32 [P, ld]."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    P = rows.shape[0]
    sym_d = sym if torch.is_tensor(sym) else torch.from_numpy(np.ascontiguousarray(sym, dtype=np.int32)).to(DEV)
    if max_len is None:
        max_len = max(1, int(rows[:, 2:].max()))
    buf = torch.full((P * ld + 2 * GUARD,), SENT, dtype=torch.int32, device=DEV)
    out = buf[GUARD:GUARD + P * ld]
    n_sym = int(sym_d.numel()) if n_sym is None else n_sym
    L.check(L.load().wft_edit_counts_i32(_p(sym_d), n_sym, _p(_table(rows)), _p(out), ld, P, max_len, L.stream_ptr()), "wft_edit_counts_i32")
    whole = buf.cpu().numpy()
    assert bool((whole[:GUARD] == SENT).all() and (whole[-GUARD:] == SENT).all()), "guards around the output"
    return whole[GUARD:-GUARD].reshape(P, ld)


def _check(batch, max_len=None):
    got = _run(batch.sym, batch.rows, max_len)
    want = EC.expected(batch)
    bad = EC.mismatches(got, want)
    assert bad.shape[0] == 0, (batch.name, bad[:5], got[bad[:5]], want[bad[:5]], batch.rows[bad[:5]])
    return got


def test_exhaustive_small_pairs_in_one_launch():
    batch = EC.exhaustive()
    assert len(batch) == 14641
    _check(batch)
    _check(batch, max_len=_cap())  # the counts do not depend on what the launch is sized for


def test_seams_of_the_workgroup():
    T = _threads()
    assert T >= 64 and T % 64 == 0
    batch = EC.seams(T)
    n, m = batch.rows[:, 2], batch.rows[:, 3]
    assert (n < m).any() and (n > m).any() and set(EC.seam_lengths(T)) <= set(n.tolist()) and set(EC.seam_lengths(T)) <= set(m.tolist())
    _check(batch)


def test_extremes_at_the_cap():
    Lc = _cap()
    assert Lc == 4096 == K.EDIT_MAX_LEN
    batch = EC.extremes(Lc)
    assert sorted(map(tuple, batch.rows[:, 2:].tolist())) == sorted([(0, Lc), (Lc, 0), (1, Lc), (Lc, 1), (Lc, Lc), (0, 0)])
    got = _check(batch)
    assert got[0].tolist() == [0, 0, 0, Lc] and got[1].tolist() == [0, 0, Lc, 0] and got[5].tolist() == [0, 0, 0, 0]


def test_ragged_batch_whole_buffer_and_every_row_alone():
    batch = EC.ragged()
    assert len(batch) == 300
    want = EC.expected(batch)
    ld = 6
    got = _run(batch.sym, batch.rows, ld=ld)
    full = np.full((len(batch), ld), SENT, dtype=np.int64)
    full[:, :4] = want
    assert np.array_equal(got, full), EC.mismatches(got[:, :4], want)[:5]
    sym_d = torch.from_numpy(batch.sym).to(DEV)
    for p in range(len(batch)):
        alone = _run(sym_d, batch.rows[p:p + 1], max_len=150)
        assert np.array_equal(alone[0], got[p, :4]), (p, alone, got[p])
    out = K.edit_counts(sym_d, batch.rows)  # the binding: the same integers
    assert out.dtype == torch.int32 and tuple(out.shape) == (300, 4) and np.array_equal(out.cpu().numpy(), want)


def test_symbol_values():
    _check(EC.symbol_values())


def test_refused_rows_write_minus_one_and_leave_their_neighbours_alone():
    """One row per refusal condition, written straight into the device table (the binding would refuse them).  The symbols live in the
    middle of a larger poisoned allocation and n_sym covers the middle only, so a broken check reads poison, never outside memory."""
    rng = np.random.default_rng(31)
    body = rng.integers(0, 3, size=400).astype(np.int32)
    margin = 1 << 14
    whole = torch.full((body.shape[0] + 2 * margin,), EC.POISON, dtype=torch.int32, device=DEV)
    sym_d = whole[margin:margin + body.shape[0]]
    sym_d.copy_(torch.from_numpy(body))
    ns, max_len = body.shape[0], 120
    good = (10, 200, 100, 90)
    bad = [(0, 0, max_len + 1, 5), (0, 0, 5, max_len + 1), (0, 0, -1, 5), (0, 0, 5, -1), (-1, 0, 5, 5), (0, -1, 5, 5), (-(1 << 62), 0, 5, 5),
           (ns - 4, 0, 5, 5), (0, ns - 4, 5, 5), (ns, 0, 1, 0), (0, ns + 1, 0, 0), (1 << 62, 0, 5, 5), (0, (1 << 63) - 1, 5, 5),
           (0, 0, -(1 << 31), 5), (0, 0, (1 << 31) - 1, (1 << 31) - 1)]
    rows = []
    for r in bad:
        rows += [good, r]
    rows.append(good)
    got = _run(sym_d, rows, max_len=max_len, ld=5)
    ref = EC.reference(body[10:110], body[200:290])
    for p, r in enumerate(rows):
        assert got[p, :4].tolist() == (list(ref) if r is good else [-1] * 4), (p, r, got[p])
    assert bool((got[:, 4] == SENT).all())
    # the last rows that still fit are served: the check is not off by one
    edge = [(ns - 5, 0, 5, 5), (0, ns - 5, 5, 5), (ns, ns, 0, 0), (0, 0, max_len, max_len)]
    got = _run(sym_d, edge, max_len=max_len)
    want = [EC.reference(body[ro:ro + n], body[ho:ho + m]) for ro, ho, n, m in edge]
    assert got.tolist() == [list(w) for w in want] and (got >= 0).all()


def test_entry_point_refusals_launch_nothing():
    lib = L.load()
    sym_d = torch.zeros(64, dtype=torch.int32, device=DEV)
    table = _table([(0, 8, 8, 8)])
    out = torch.full((64,), SENT, dtype=torch.int32, device=DEV)
    bytes_ = torch.zeros(256, dtype=torch.uint8, device=DEV)
    ok = dict(sym=_p(sym_d), n_sym=64, rows=_p(table), out=_p(out), ld=4, P=1, max_len=8)
    bad = [dict(sym=_p(None)), dict(rows=_p(None)), dict(out=_p(None)), dict(n_sym=0), dict(n_sym=-5), dict(P=0), dict(P=-1), dict(P=(1 << 20) + 1),
           dict(max_len=0), dict(max_len=-1), dict(max_len=_cap() + 1), dict(ld=3), dict(ld=0), dict(ld=-4),
           dict(rows=C.c_void_p(table.data_ptr() + 4)), dict(out=C.c_void_p(out.data_ptr() + 2)), dict(out=C.c_void_p(bytes_.data_ptr() + 1))]
    for change in bad:
        a = {**ok, **change}
        code = lib.wft_edit_counts_i32(a["sym"], a["n_sym"], a["rows"], a["out"], a["ld"], a["P"], a["max_len"], L.stream_ptr())
        assert code == ERR_ARG, (change, code)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and not bytes_.any()  # nothing was launched
    assert lib.wft_edit_counts_i32(ok["sym"], 64, ok["rows"], ok["out"], 4, 1, 8, L.stream_ptr()) == 0
    assert out[:4].tolist() == [8, 0, 0, 0] and bool((out[4:] == SENT).all())


def test_binding_checks_rows_on_the_host():
    sym_d = torch.zeros(32, dtype=torch.int32, device=DEV)
    for rows, kw in (([(0, 0, 33, 1)], {}), ([(0, 30, 2, 3)], {}), ([(-1, 0, 1, 1)], {}), ([(0, 0, 5, 5)], dict(max_len=4)), ([(0, 0, 5, 5)], dict(max_len=4097)),
                     ([], {}), ([(0, 0, 1)], {}), ([(0, 0, -1, 1)], {})):
        with pytest.raises(ValueError):
            K.edit_counts(sym_d, rows, **kw)
    with pytest.raises(ValueError):
        K.edit_counts(sym_d.long(), [(0, 0, 1, 1)])
    with pytest.raises(ValueError):
        K.edit_counts(sym_d, [(0, 0, 1, 1)], rows_d=torch.zeros(7, dtype=torch.int32, device=DEV))
    assert K.edit_counts(sym_d, [(0, 16, 16, 16)]).tolist() == [[16, 0, 0, 0]]


def test_edit_counts_batch_on_the_device_equals_the_host():
    refs = ["the cat sat on the mat", "grüße aus köln", "a", "  padded  reference ", "same same", "zwölf boxkämpfer jagen viktor quer über den großen sylter deich",
            "日本語 の テキスト", "x"]
    hyps = ["the cat sat mat on the", "grüsse aus köln am rhein", "", "padded reference", "same same", "zwölf boxkämpfer jagen victor über den grossen deich deich",
            "日本 の テキスト です", "y z"]
    for fn in (M.word_error_counts, M.char_error_counts):
        got, want = fn(hyps, refs, DEV), fn(hyps, refs)
        assert got.dtype == np.int64 and np.array_equal(got, want), (fn.__name__, got, want)
    w, c = M.word_error_counts(hyps, refs, "cuda"), M.char_error_counts(hyps, refs, "cuda:0")
    for k, (r, h) in enumerate(zip(refs, hyps)):
        assert int(w[k, 1:].sum()) / int(w[k, :3].sum()) == M.wer(r, h) and int(c[k, 1:].sum()) / int(c[k, :3].sum()) == M.cer(r, h)
    # hashable items of any kind; a pair longer than the cap is scored on the host and keeps its place; every pair empty
    rng = np.random.default_rng(5)
    long_r, long_h = rng.integers(0, 4, size=_cap() + 1).tolist(), rng.integers(0, 4, size=40).tolist()
    mixed_r = [[("a", 1), None, 2.5], long_r, [], [7, 7, 7]]
    mixed_h = [[None, ("a", 1), 2.5, "q"], long_h, [1], [7, 7]]
    got = M.edit_counts_batch(mixed_r, mixed_h, DEV)
    want = np.array([M.edit_counts_host(mixed_r[0], mixed_h[0]), EC.counts_diagonals(long_r, long_h), (0, 0, 0, 1), (2, 0, 1, 0)])
    assert np.array_equal(got, want), (got, want)
    assert M.edit_counts_batch([[], []], [[], []], DEV).tolist() == [[0, 0, 0, 0]] * 2
    assert M.edit_counts_batch([], [], DEV).shape == (0, 4)
