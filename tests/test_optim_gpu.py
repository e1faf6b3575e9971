"""The optimizer kernels of csrc/optim.hip under the per-element bounds of tests/_optim_cases.py (whose docstring has the cases, the
float64 references, the bound forms and how their constants were measured; tests/test_optim_host.py proves on the CPU that the same
checkers reject every listed mutant of the kernels' arithmetic).  Every kernel is called through the C ABI on guarded buffers of
the test's own: wft_mt_adamw (p, exp_avg and exp_avg_sq of every element, both tables, every hyper-parameter set and clip),
wft_mt_sumsq_f32 (every partial and the total), wft_muon_momentum_mt (buf, the overwritten g, U, every partial; the NULL row against
an all-zero gradient), wft_muon_prepare (X, Xt, the pad), wft_muon_apply_mt, wft_transpose_bf16, wft_adamw_step (with its bf16
copy) and wft_sumsq_f32.  Each test prints the worst |err| / bound it saw per output and the running worst of its family; above 1 it
fails.

Measured on an MI355X, worst |err| / bound per output (the bound with the K in force):
  wft_mt_adamw:          p 0.179, m 0.238, v 0.244
  wft_adamw_step:        p 0.102, m 0.239, v 0.168
  wft_mt_sumsq_f32:      partial 0.155, total 0.181
  wft_sumsq_f32:         total 0.052
  wft_muon_momentum_mt:  buf 0.173, u 0.218, partial 0.131; U of the NULL row 1.000 (half an ulp of bf16 + K F, which the rounding alone can use up)
  wft_muon_prepare:      X 0.999 (half an ulp of bf16 + 4u |q|, likewise)
  wft_muon_apply_mt:     0.153
No output of any case reaches its bound and every exact assertion holds: the kernels needed no fix.  The ratios land where the CPU
restatement does (m 0.238 x 4 = 0.95 F against 0.951 F restated, v 0.244 x 4 = 0.98 F against 0.987 F).
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _optim_cases as O  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16
WORST = {}


def _p(t, byte_offset=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + byte_offset)


def _note(family, name, r):
    w = WORST.setdefault(family, {})
    for k, v in r.items():
        w[k] = max(w.get(k, 0.0), v)
    print(f"{family} {name}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    print(f"  so far, {family}: " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))


def _dev(buf):
    d = buf.to(DEV)
    assert d.data_ptr() % 16 == 0
    return d


def _views(buf, lay):
    return [buf[s:s + n] for s, n in zip(lay.starts, lay.numels)]


def _same(a, b):
    return torch.equal(O.bits(a), O.bits(b))


def _scalar(x):
    return None if x is None else torch.tensor([x], dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------ wft_mt_adamw
def _mt_adamw(case):
    numels, lay = O.adam_table(case.table)
    inp = O.adam_inputs(case.table)
    buf = {a: _dev(lay[a].fill(inp[a])) for a in "pgmv"}
    v = {a: _views(buf[a], lay[a]) for a in "pgmv"}
    if case.table == "A":
        off = [tuple(v[a][t].data_ptr() % 16 for a in "pgmv") for t in range(len(numels))]
        assert [sum(1 for x in o if x) for o in off] == [1, 1, 1, 0, 1, 0, 0] and {max(o) for o in off} == {0, 4, 8}
    table = K.TensorTable(v["p"])
    assert table.total_chunks == O.chunk_starts(numels)[-1]
    tab = table.pointers(v["p"], v["g"], v["m"], v["v"])
    clip = O.CLIPS[case.clip]
    ss = _scalar(clip[0] if clip else None)
    L.check(L.load().wft_mt_adamw(_p(tab), _p(table.numel), _p(table.chunk_start), table.n, table.total_chunks,
                                  *O.adam_scalars(O.ADAM_HP[case.hp]), _p(ss), clip[1] if clip else 0.0, L.stream_ptr()), "wft_mt_adamw")
    torch.cuda.synchronize()
    return {a: b.cpu() for a, b in buf.items()}


@pytest.mark.parametrize("hp", range(len(O.ADAM_HP)))
@pytest.mark.parametrize("table", "AB")
def test_mt_adamw_within_the_element_bounds(table, hp):
    outs = {}
    for clip in range(len(O.CLIPS)):
        case = O.AdamCase(table, hp, clip)
        out = outs[clip] = _mt_adamw(case)
        _note("mt_adamw", case.name, O.check_adam_case(case, out))
    again = _mt_adamw(O.AdamCase(table, hp, 1))
    assert all(_same(again[a], outs[1][a]) for a in "pgmv"), "a second launch from the same state differs"
    for clip in (2, 3):   # a coefficient >= 1 (sumsq = 0 included) is the launch without sumsq
        assert all(_same(outs[clip][a], outs[0][a]) for a in "pmv"), f"clip {clip}: differs from the launch with sumsq = NULL"


# ------------------------------------------------------------------------------------------------ wft_mt_sumsq_f32
def _mt_sumsq(table):
    numels, lay = O.sumsq_table(table)
    g = _dev(lay.fill(O.sumsq_inputs(table)))
    before = g.clone()
    views = _views(g, lay)
    if table == "A":
        assert sum(1 for t in views if t.data_ptr() % 16) == 2
    tt = K.TensorTable(views)
    tab = tt.pointers([None if t in O.SUMSQ_NULL[table] else x for t, x in enumerate(views)], allow_none=True)
    play, olay = O.Layout((tt.total_chunks,)), O.Layout((1,))
    partial, out = _dev(play.fill()), _dev(olay.fill())
    L.check(L.load().wft_mt_sumsq_f32(_p(tab), _p(tt.numel), _p(tt.chunk_start), tt.n, tt.total_chunks, _p(partial, 4 * play.starts[0]),
                                      _p(out, 4 * olay.starts[0]), L.stream_ptr()), "wft_mt_sumsq_f32")
    torch.cuda.synchronize()
    assert _same(g, before), "the const gradients changed"
    assert olay.guards_intact(out), "out: a sentinel was overwritten"
    return {"partial": partial.cpu(), "total": olay.gather(out.cpu())}


@pytest.mark.parametrize("table", "AB")
def test_mt_sumsq_every_partial_and_the_total(table):
    out = _mt_sumsq(table)
    _note("mt_sumsq", f"table {table}", O.check_mt_sumsq(table, out))
    again = _mt_sumsq(table)
    assert _same(out["partial"], again["partial"]) and _same(out["total"], again["total"]), "two launches differ"


# ------------------------------------------------------------------------------------------------ wft_muon_momentum_mt
def _momentum(case, null):
    lay = O.mom_layouts(case.numel, case.chunks)
    inp = O.mom_inputs(case.numel)
    g, buf = _dev(lay["g"].fill(inp["g"])), _dev(lay["buf"].fill(inp["buf"]))
    Ub, partial = _dev(lay["U"].fill(dtype=BF16)), _dev(lay["partial"].fill())
    gp = [x.data_ptr() for x in _views(g, lay["g"])]
    bp = [x.data_ptr() for x in _views(buf, lay["buf"])]
    if null:
        gp[1] = 0
    tab = K.upload_table(bp + gp + bp, torch.int64, DEV)   # row 0 (p) is not read by this kernel
    ss = _scalar(O.MOM_CLIP[0] if case.clip else None)
    L.check(L.load().wft_muon_momentum_mt(_p(tab), 3, case.numel, O.f32(O.MOM_BETA), case.nesterov, _p(Ub, 2 * lay["U"].starts[0]),
                                          _p(partial, 4 * lay["partial"].starts[0]), _p(ss), O.MOM_CLIP[1] if case.clip else 0.0,
                                          L.stream_ptr()), "wft_muon_momentum_mt")
    torch.cuda.synchronize()
    return {"g": g.cpu(), "buf": buf.cpu(), "U": Ub.cpu(), "partial": partial.cpu()}


@pytest.mark.parametrize("i", range(len(O.mom_cases())), ids=[c.name for c in O.mom_cases()])
def test_muon_momentum_every_output(i):
    case = O.mom_cases()[i]
    out = _momentum(case, null=True)
    _note("momentum", case.name, O.check_momentum(case, out, null=True))
    zero = _momentum(case, null=False)
    _note("momentum", case.name + ", zero gradient for NULL", O.check_momentum(case, zero, null=False))
    for k in ("buf", "U", "partial"):
        assert _same(out[k], zero[k]), f"{k}: the NULL row differs from an all-zero gradient"


# ------------------------------------------------------------------------------------------------ wft_muon_prepare
@pytest.mark.parametrize("i", range(len(O.prep_cases())), ids=[c.name for c in O.prep_cases()])
def test_muon_prepare_values_pad_and_transpose(i):
    c = O.prep_cases()[i]
    lay = O.prep_layouts(c)
    inp = O.prep_inputs(c)
    Ub, partial = _dev(lay["U"].fill(inp["U"].reshape(-1), BF16)), _dev(lay["partial"].fill(inp["partial"].reshape(-1)))
    X, Xt = _dev(lay["X"].fill(dtype=BF16)), _dev(lay["Xt"].fill(dtype=BF16))
    before = Ub.clone(), partial.clone()
    L.check(L.load().wft_muon_prepare(_p(Ub, 2 * lay["U"].starts[0]), c.rows, c.cols, _p(partial, 4 * lay["partial"].starts[0]), c.chunks,
                                      _p(X, 2 * lay["X"].starts[0]), _p(Xt, 2 * lay["Xt"].starts[0]), c.rp, c.cp, 2, L.stream_ptr()),
            "wft_muon_prepare")
    torch.cuda.synchronize()
    assert _same(Ub, before[0]) and _same(partial, before[1]), "a const input changed"
    _note("prepare", c.name, O.check_prepare(c, {"X": X.cpu(), "Xt": Xt.cpu()}))


# ------------------------------------------------------------------------------------------------ wft_muon_apply_mt
@pytest.mark.parametrize("i", range(len(O.apply_cases())), ids=[c.name for c in O.apply_cases()])
def test_muon_apply_through_the_padded_frame(i):
    c = O.apply_cases()[i]
    lay = O.apply_layouts(c)
    fr, ldo = c.frame
    p = _dev(lay["p"].fill(O.apply_inputs(c.rows, c.cols)["p"]))
    Ob = _dev(lay["O"].fill(O.apply_frame(c).reshape(-1), BF16))
    before = Ob.clone()
    views = _views(p, lay["p"])
    assert views[2].data_ptr() < views[0].data_ptr() < views[1].data_ptr()
    ptab = K.upload_table([x.data_ptr() for x in views], torch.int64, DEV)
    L.check(L.load().wft_muon_apply_mt(_p(ptab), 3, c.rows, c.cols, _p(Ob, 2 * lay["O"].starts[0]), ldo, fr * ldo, O.f32(O.APPLY_LR),
                                       O.f32(c.wd), O.f32(c.scale), L.stream_ptr()), "wft_muon_apply_mt")
    torch.cuda.synchronize()
    assert _same(Ob, before), "the const O changed"
    _note("apply", c.name, O.check_apply(c, {"p": p.cpu()}))


# ------------------------------------------------------------------------------------------------ wft_transpose_bf16
@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 65), (64, 64), (65, 63), (77, 40)])
def test_transpose_bit_exact(rows, cols, batch):
    lay = O.Layout((batch * rows * cols,), align=8)
    src = (torch.randn(batch, rows, cols, generator=torch.Generator().manual_seed(rows * cols)) * 10.0 ** torch.arange(cols).remainder(5)).to(BF16)
    s, d = _dev(lay.fill(src.reshape(-1), BF16)), _dev(lay.fill(dtype=BF16))
    before = s.clone()
    L.check(L.load().wft_transpose_bf16(_p(s, 2 * lay.starts[0]), rows, cols, _p(d, 2 * lay.starts[0]), batch, L.stream_ptr()), "wft_transpose_bf16")
    torch.cuda.synchronize()
    assert _same(s, before) and lay.guards_intact(d)
    assert _same(lay.gather(d.cpu()).view(batch, cols, rows), src.transpose(1, 2).contiguous())


# ------------------------------------------------------------------------------------------------ wft_adamw_step
STEP_BIG = 4 * (4096 * 256) + 1203   # the smallest size at which the grid-stride loop comes round a second time


def _adamw_step(n, lay, play, inp, scalars, gscale, want_bf16):
    buf = {a: _dev(lay[a].fill(inp[a])) for a in "pgmv"}
    pb = _dev(play.fill(dtype=BF16)) if want_bf16 else None
    gsc = _scalar(gscale)
    ptr = {a: _p(buf[a], 4 * lay[a].starts[0]) for a in "pgmv"}
    L.check(L.load().wft_adamw_step(ptr["p"], ptr["g"], ptr["m"], ptr["v"], _p(pb, 2 * play.starts[0]) if want_bf16 else _p(None), n, *scalars,
                                    _p(gsc), L.stream_ptr()), "wft_adamw_step")
    torch.cuda.synchronize()
    return {a: b.cpu() for a, b in buf.items()}, (pb.cpu() if want_bf16 else None)


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 7, 1027, STEP_BIG))
def test_adamw_step_under_the_checker_of_mt_adamw(n):
    lay = {a: O.Layout((n,)) for a in "pgmv"}
    play = O.Layout((n,), align=8)
    kind = torch.arange(n) % 8
    inp = O.adam_values(kind, torch.Generator().manual_seed(n))
    inp["kind"] = kind
    scalars = O.adam_scalars(O.ADAM_HP[0])
    combos = ((0.37, True),) if n == STEP_BIG else ((None, False), (None, True), (0.37, False), (0.37, True))
    for gscale, want_bf16 in combos:
        out, pb = _adamw_step(n, lay, play, inp, scalars, gscale, want_bf16)
        ref = O.adam_reference(inp, scalars, 1.0 if gscale is None else O.f32(gscale), 0.0)
        _note("adamw_step", f"n {n}, gscale {gscale}, p_bf16 {want_bf16}", O.check_adamw(f"wft_adamw_step n {n}", lay, inp, ref, out, scalars))
        if want_bf16:
            assert play.guards_intact(pb), "p_bf16: a sentinel was overwritten"
            assert _same(play.gather(pb), lay["p"].gather(out["p"]).to(BF16)), "p_bf16 is not RNE bf16 of the new p"


def test_adamw_step_and_sumsq_refuse_unaligned_pointers():
    h = L.load()
    t = [torch.full((16,), 7.0, device=DEV) for _ in range(4)]
    pb = torch.full((16,), 7.0, dtype=BF16, device=DEV)
    sc = O.adam_scalars(O.ADAM_HP[0])
    for bad in range(5):
        off = [4 if i == bad else 0 for i in range(4)]
        with pytest.raises(L.WftError, match="16-byte alignment"):
            L.check(h.wft_adamw_step(_p(t[0], off[0]), _p(t[1], off[1]), _p(t[2], off[2]), _p(t[3], off[3]), _p(pb, 2 if bad == 4 else 0), 8, *sc,
                                     _p(None), L.stream_ptr()), "wft_adamw_step")
    with pytest.raises(L.WftError, match="16-byte alignment"):
        L.check(h.wft_sumsq_f32(_p(t[0], 4), 8, _p(t[1]), L.stream_ptr()), "wft_sumsq_f32")
    torch.cuda.synchronize()
    assert all((x == 7.0).all() for x in t) and (pb == 7.0).all(), "a refused call wrote"


# ------------------------------------------------------------------------------------------------ wft_sumsq_f32
@pytest.mark.parametrize("n", (1, 3, 5, 1027, 4 * (1024 * 256) + 1027))
def test_sumsq_f32_accumulates_within_the_bound(n):
    lay, olay = O.Layout((n,)), O.Layout((1,))
    gv = O.adam_values(torch.arange(n) % 8, torch.Generator().manual_seed(n))["g"]
    g = _dev(lay.fill(gv))
    before = g.clone()
    want = float((gv.double() ** 2).sum())
    grid = min(max((n // 4 + 1 + 255) // 256, 1), 1024)
    dep = -(-(n // 4) // (grid * 256)) * 4 + 10 + grid   # per-thread adds, butterfly and waves, one atomic per workgroup
    for preset in (0.0, 5.0):
        out = _dev(olay.fill(torch.tensor([preset])))
        L.check(L.load().wft_sumsq_f32(_p(g, 4 * lay.starts[0]), n, _p(out, 4 * olay.starts[0]), L.stream_ptr()), "wft_sumsq_f32")
        torch.cuda.synchronize()
        assert _same(g, before) and olay.guards_intact(out)
        ck = O.Checker(f"wft_sumsq_f32 n {n}, out preset to {preset}")
        ck.within("total", olay.gather(out.cpu()), torch.tensor([preset + want], dtype=torch.float64),
                  torch.tensor([O.U * (preset + want) * math.sqrt(dep)], dtype=torch.float64), kname="partial")
        _note("sumsq_f32", f"n {n}, preset {preset}", ck.done())
