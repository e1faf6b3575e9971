"""Every kernel kind of nt_plan / tn_plan (csrc/gemm*.hip) and the weight-streaming kernel (csrc/gemm_stream.hip) on the
exact-arithmetic probes of tests/_gemm_exact_cases.py: small-integer bf16 operands whose every partial sum is an integer below 2^24,
so C must equal the fp64 reference bit for bit, element by element, whatever the k order, split-K plan, ring depth or atomic order;
one-hot gather operands that pin the k -> fragment mapping with arbitrary values; the GELU forms held per element to the bound that
tests/test_gemm_exact_host.py derives on the CPU, where every fault restated as a wrong reference is shown to fail these checks.

Each case asserts through the public plan queries (and, between the ring and two-buffer forms, the tile count against the device's
CU count) that the kind the table names serves the call, runs two operand seeds into the same output buffers (a fragment read
that runs ahead of its LDS-DMA piece would see the previous run's different operands), reads its operands from allocations whose
rows >= M / R and columns >= K hold the finite poison 3, and writes into views (ldc > N) inside buffers pre-filled with a sentinel
bit pattern of which every element outside C must come back unchanged.  A failure names the case, the count of wrong elements and
the first wrong (m, n) with its tile, 16 x 16 block and the got / want values."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _gemm_exact_cases as G  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = "cuda:0"
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5   # NaN bit patterns: an element left unwritten inside a view fails the comparison
GR, GC = 3, 8                          # guard rows around, guard columns behind every output
EPI = {"none": L.EPI_NONE, "gelu": L.EPI_GELU, "dgelu": L.EPI_DGELU, "gelu_grad": L.EPI_GELU_GRAD, "mul_aux": L.EPI_MUL_AUX}
PLAIN_F32 = G.Form("plain_f32", c_f32=True)


@pytest.fixture(autouse=True)
def _restore_variants():
    old = dict(K.VARIANT)
    yield
    K.VARIANT.update(old)


@functools.lru_cache(maxsize=None)
def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Out:
    """a [batch, rows, cols] view (bf16 or fp32) inside a sentinel-filled [batch, rows + 2 GR, cols + GC] buffer"""

    def __init__(self, batch, rows, cols, f32, live_cols=None):
        self.sent = SENT32 if f32 else SENT16
        self.buf = torch.full((batch, rows + 2 * GR, cols + GC), self.sent, dtype=torch.int32 if f32 else torch.int16, device=DEV)
        self.inside = (slice(None), slice(GR, GR + rows), slice(0, cols if live_cols is None else live_cols))
        self.view = self.buf.view(torch.float32 if f32 else torch.bfloat16)[:, GR:GR + rows, :cols]
        self.ld, self.stride = cols + GC, (rows + 2 * GR) * (cols + GC)

    @property
    def live(self):
        return self.buf.view(self.view.dtype)[self.inside]

    def reset(self):
        self.buf.fill_(self.sent)

    def assert_intact(self, what):
        outside = torch.ones_like(self.buf, dtype=torch.bool)
        outside[self.inside] = False
        bad = int((self.buf[outside] != self.sent).sum())
        assert bad == 0, f"{what}: {bad} sentinel elements outside the output were overwritten"


def _poisoned(x, rows_pad):
    """logical [batch, M, N] fp32 -> bf16 device buffer [batch, M + rows_pad, N + GC] with the poison behind rows and columns"""
    b, M, N = x.shape
    buf = torch.full((b, M + rows_pad, N + GC), G.POISON, dtype=torch.bfloat16, device=DEV)
    buf[:, :M, :N] = x.to(DEV)
    return buf


def _call(entry, args):
    L.check(getattr(L.load(), entry)(ctypes.byref(args), L.stream_ptr()), entry)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ NT
def _nt_args(c, form, ops, out, launch, pv, e=None, aux=None, cs=None, B_buf=None):
    kw = dict(M=c.M, N=c.N, K=c.K, lda=ops.lda, ldb=ops.ldb, batch=c.batch, strideA=ops.strideA, strideB=0, out=out.view[0] if c.batch == 1 else out.view,
              strideC=out.stride, ldc=out.ld, alpha=form.alpha, beta=form.beta, epilogue=EPI[form.epilogue], accumulate=form.accumulate,
              residual_first=form.res_first, p_valid=pv, launch=launch, _args_only=True)
    if form.bias:
        kw["bias"] = e["bias"]
    if form.residual:
        kw.update(residual=e["res"], ldr=e["res"].shape[-1], strideR=e["res"].shape[1] * e["res"].shape[2])
    if aux is not None:
        kw.update(aux=aux, ldaux=aux.stride(1), strideAux=aux.stride(0))
    if form.valid:
        kw.update(valid_rows_period=form.valid[0], valid_rows=form.valid[1])
    if cs is not None:
        kw["colsum"] = cs
    args, _ = K.gemm_nt(ops.A_dev, ops.B_dev if B_buf is None else B_buf, **kw)
    if form.colsum == "pass":   # no workspace: the library sums the columns of C in a second pass
        args.workspace, args.workspace_bytes = 0, 0
    return args


def _assert_nt_kind(c, form, variant, pv, args, kind):
    h = L.load()
    got = (int(h.wft_gemm_nt_variant(ctypes.byref(args))), int(h.wft_gemm_nt_splitk_workspace_bytes(ctypes.byref(args))))
    rule = G.nt_plan(c.M, c.N, c.K, c.batch, form, variant, pv, c.lda, ncu=_ncu())
    assert rule[0] == kind and got == rule[1:], f"{c.name} {form.name}: the plan answers {got}, the table's kind {kind} needs {rule}"
    if kind == "NT_128_SPLITK":
        assert args.workspace and args.workspace_bytes >= got[1] > 0
    if form.colsum == "fused" and kind in ("NT_4W", "NT_256"):
        need = int(h.wft_gemm_nt_colsum_workspace_bytes(ctypes.byref(args)))
        assert need > 0 and args.workspace and args.workspace_bytes >= need, f"{c.name} {form.name}: the column sums are not fused"


def _epi_dev(c, form, seed):
    e = G.nt_epilogue_operands(c, form, seed)
    pad = G.pad_rows(c.M)
    dev = {"bias": None if e.bias is None else e.bias.to(DEV)}
    dev["res"] = None if e.res is None else _poisoned(e.res[:, :c.M], pad)
    dev["aux"] = None if e.aux is None else _poisoned(e.aux[:, :c.M], pad)
    return e, dev


def _run_nt_form(c, ops, acc, fname, variant, launch, pv, kind, seed, outs):
    form = G.FORMS[fname] if isinstance(fname, str) else fname
    tile = 256 if kind in ("NT_4W", "NT_256") else 128
    what = f"{c.name} {form.name} variant {variant} launch {launch} p_valid {pv} seed {seed} ({ops.probe}) [{kind}]"
    K.set_variant("nt", variant)
    nc = 16 * -(-pv // 16) if kind == "NT_RANK" else c.N
    out = outs.setdefault(("C", form.c_f32, nc), Out(c.batch, c.M, c.N, form.c_f32, nc))
    out.reset()   # (an element a kernel leaves unwritten then reads as the sentinel's NaN)
    if outs.get("epi seed") != seed:   # epilogue operands: built once per (form, seed), shared by the variants and launch modes
        outs["epi seed"], outs["epi"] = seed, {}
    e, ed = outs["epi"].get(form.name) or outs["epi"].setdefault(form.name, _epi_dev(c, form, seed))
    aux_out = None
    aux = ed["aux"][:, :c.M, :c.N] if ed["aux"] is not None else None
    if form.aux_out or form.epilogue == "gelu_grad":
        aux_out = outs.setdefault("aux", Out(c.batch, c.M, c.N, False))
        aux_out.reset()
        aux = aux_out.view
    cs = outs.setdefault("cs", Out(1, 1, c.N, True)) if form.colsum else None
    if cs is not None:
        cs.reset()
    B_buf, acc_f = None, acc
    if kind == "NT_RANK":   # rows >= p_valid of B are zero padding
        B_buf = ops.B_dev.clone()
        B_buf[:, pv:, :c.K] = 0
        acc_f = acc.clone()
        acc_f[:, :, pv:] = 0
    if form.accumulate:
        out.view.copy_(e.base.to(DEV))
    args = _nt_args(c, form, ops, out, launch, pv, ed, aux, None if cs is None else cs.view[0, 0], B_buf)
    _assert_nt_kind(c, form, variant, pv, args, kind)
    _call("wft_gemm_nt_bf16", args)
    want = G.nt_expected(form, acc_f, e)
    got = out.live
    if want["bound"] is None:
        G.assert_exact(got, want["C"][:, :, :nc], tile, what)
    else:
        G.assert_bounded(got, want["C"], want["bound"], tile, what)
    if aux_out is not None:
        if form.epilogue == "gelu":
            G.assert_exact(aux_out.live, want["aux"], tile, what + " stored pre-activation")
        else:
            G.assert_bounded(aux_out.live, want["aux"], want["aux_bound"], tile, what + " stored gelu'")
        aux_out.assert_intact(what + " aux")
    if cs is not None:
        G.assert_exact(cs.live[0, 0], want["colsum"], tile, what + " column sums")
        cs.assert_intact(what + " column sums")
    out.assert_intact(what)
    for name, t in (("residual", ed["res"]), ("aux", None if aux_out is not None else ed["aux"])):   # the inputs came back as they went
        if t is not None:
            assert (t[:, c.M:] == G.POISON).all() and (t[:, :, c.N:] == G.POISON).all(), f"{what}: the {name} allocation was written"


def _to_dev(ops):
    ops.A_dev, ops.B_dev = ops.A_buf.to(DEV), ops.B_buf.to(DEV)
    return ops


def _gather_forms(c):
    """(form, variant, p_valid, kind) the gather probe runs under: the plain product on every kernel of the case, bf16 and fp32 C"""
    out = []
    for f, variant, launch, pv, kind in G.nt_runs(c):
        if f == "plain" and launch == 0:
            out.append((G.FORMS["plain"], variant, pv, kind))
    if c.kind not in ("NT_RANK", "NT_128_SPLITK"):
        out.append((PLAIN_F32, 0, 0, G.nt_plan(c.M, c.N, c.K, c.batch, PLAIN_F32, 0, 0, c.lda, ncu=_ncu())[0]))
    return out


@pytest.mark.parametrize("c", G.NT_CASES, ids=[f"{c.kind}-{c.name}" for c in G.NT_CASES])
def test_nt_kernels_are_exact(c):
    outs = {}
    runs = G.nt_runs(c)
    assert c.kind in {r[4] for r in runs}
    for seed in G.SEEDS:
        ops = _to_dev(G.nt_operands(c, seed))
        acc = G.nt_acc(ops, DEV)
        for fname, variant, launch, pv, kind in runs:
            _run_nt_form(c, ops, acc, fname, variant, launch, pv, kind, seed, outs)
        if c.kind == "NT_RANK":   # the pair entry point: two products, one launch, each held to its own reference
            for pv in c.p_valid:
                nc = 16 * -(-pv // 16)
                o0, o1 = Out(1, c.M, c.N, False, nc), Out(1, c.M, c.N, False, nc)
                B0, B1 = ops.B_dev.clone(), ops.B_dev.flip(1).contiguous()
                B0[:, pv:, :c.K] = 0
                B1[:, pv:, :c.K] = 0
                a0 = _nt_args(c, G.FORMS["plain"], ops, o0, 0, pv, B_buf=B0)
                a1 = _nt_args(c, G.FORMS["plain"], ops, o1, 0, pv, B_buf=B1)
                L.check(L.load().wft_gemm_nt_rank_pair_bf16(ctypes.byref(a0), ctypes.byref(a1), L.stream_ptr()), "wft_gemm_nt_rank_pair_bf16")
                torch.cuda.synchronize()
                G.assert_exact(o0.live, acc[:, :, :nc] * (torch.arange(nc, device=DEV) < pv), 128, f"{c.name} pair p_valid {pv} seed {seed} first")
                G.assert_exact(o1.live, acc.flip(2)[:, :, :nc] * (torch.arange(nc, device=DEV) < pv), 128, f"{c.name} pair p_valid {pv} seed {seed} second")
                o0.assert_intact("pair first"); o1.assert_intact("pair second")
        # the gather probe: C[m, n] = A[m, k(n)] (B one-hot) and C[m, n] = B[n, k(m)] (A one-hot), arbitrary bf16 values
        for form, variant, pv, kind in _gather_forms(c):
            n_live = pv if kind == "NT_RANK" else c.N
            for probe, n_out in (("gather_b", n_live), ("gather_a", c.M * c.batch)):
                if probe == "gather_a" and c.windows:
                    continue
                g = _to_dev(G.nt_operands(c, seed, probe))
                for r in range(G.gather_rounds(n_out, c.K)):
                    sel = G.gather_sel(n_out, c.K, seed, r, 3 if probe == "gather_b" else 5).to(DEV)
                    if probe == "gather_b":
                        g.B_dev[:, :, :c.K] = 0
                        g.B_dev[0, torch.arange(n_out, device=DEV), sel] = 1
                        ref = g.A.to(DEV).double()[:, :, sel]
                        if n_out < c.N:
                            ref = torch.cat([ref, torch.zeros(c.batch, c.M, c.N - n_out, dtype=torch.float64, device=DEV)], 2)
                    else:
                        flat = g.A_dev.view(-1, g.A_dev.shape[-1])
                        rows = (torch.arange(c.batch, device=DEV)[:, None] * g.A_dev.shape[1] + torch.arange(c.M, device=DEV)[None, :]).reshape(-1)
                        flat[rows, :c.K] = 0
                        flat[rows, sel] = 1
                        ref = g.B.to(DEV).double()[0][:, sel].t().reshape(c.batch, c.M, c.N)
                        if kind == "NT_RANK":   # rows >= p_valid of B are zero padding
                            g.B_dev[:, pv:, :c.K] = 0
                            ref[:, :, pv:] = 0
                    g.probe = f"{probe} round {r}"
                    _run_gather(c, g, ref, form, variant, pv, kind, seed, outs)


def _run_gather(c, g, ref, form, variant, pv, kind, seed, outs):
    tile = 256 if kind in ("NT_4W", "NT_256") else 128
    what = f"{c.name} {form.name} variant {variant} p_valid {pv} seed {seed} ({g.probe}) [{kind}]"
    K.set_variant("nt", variant)
    nc = 16 * -(-pv // 16) if kind == "NT_RANK" else c.N
    out = outs.setdefault(("C", form.c_f32, nc), Out(c.batch, c.M, c.N, form.c_f32, nc))
    out.reset()
    args = _nt_args(c, form, g, out, 0, pv)
    _assert_nt_kind(c, form, variant, pv, args, kind)
    _call("wft_gemm_nt_bf16", args)
    G.assert_exact(out.live, ref[:, :, :nc], tile, what)
    out.assert_intact(what)


# ------------------------------------------------------------------------------------------------ the streaming kernel
@pytest.mark.parametrize("M,N,Kd", G.STREAM_CASES)
def test_stream_kernel_is_exact(M, N, Kd):
    c = G.stream_case(M, N, Kd)
    out, aux_out = Out(1, M, N, False), Out(1, M, N, False)
    for seed in G.SEEDS:
        ops, e = G.stream_operands(M, N, Kd, seed)
        ops = _to_dev(ops)
        acc = G.nt_acc(ops, DEV)
        bias_int = G.bias_vec(N)
        res = _poisoned(e.res[:, :M], G.pad_rows(M))
        for fname in G.STREAM_FORMS:
            form = G.FORMS[fname]
            what = f"stream {M}x{N}x{Kd} {fname} seed {seed}"
            ef = G.Epi(bias_int if form.bias == "int" else e.bias if form.bias else None, e.res if form.residual else None)
            kw = dict(M=M, N=N, K=Kd, lda=ops.lda, ldb=ops.ldb, out=out.view[0], ldc=out.ld, epilogue=EPI[form.epilogue])
            if form.bias:
                kw["bias"] = ef.bias.to(DEV)
            if form.residual:
                kw.update(residual=res[0], ldr=res.shape[-1])
            if form.aux_out:
                kw.update(aux=aux_out.view[0], ldaux=aux_out.ld)
            got = K.gemm_nt_stream(ops.A_dev, ops.B_dev, **kw)
            assert got is not None, f"{what}: the streaming kernel does not serve the call"
            torch.cuda.synchronize()
            want = G.nt_expected(form, acc, ef)
            if want["bound"] is None:
                G.assert_exact(out.live, want["C"], 128, what)
            else:
                G.assert_bounded(out.live, want["C"], want["bound"], 128, what)
            if form.aux_out:
                G.assert_exact(aux_out.live, want["aux"], 128, what + " stored pre-activation")
                aux_out.assert_intact(what + " aux")
            out.assert_intact(what)
        for r in range(G.gather_rounds(N, Kd)):
            sel = G.gather_sel(N, Kd, seed, r, 3).to(DEV)
            g = _to_dev(G.nt_operands(c, seed, "gather_b"))
            g.B_dev[:, :, :Kd] = 0
            g.B_dev[0, torch.arange(N, device=DEV), sel] = 1
            assert K.gemm_nt_stream(g.A_dev, g.B_dev, M=M, N=N, K=Kd, lda=g.lda, ldb=g.ldb, out=out.view[0], ldc=out.ld) is not None
            torch.cuda.synchronize()
            G.assert_exact(out.live, g.A.to(DEV).double()[:, :, sel], 128, f"stream {M}x{N}x{Kd} gather round {r} seed {seed}")
            out.assert_intact("stream gather")


# ------------------------------------------------------------------------------------------------ TN
class Flat:
    """a flat fp32 view of n elements between two sentinel pads"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 128,), SENT32, dtype=torch.int32, device=DEV)
        self.view = self.buf.view(torch.float32)[64:64 + n]

    def reset(self):
        self.buf.fill_(SENT32)

    def assert_intact(self, what):
        bad = int((self.buf[:64] != SENT32).sum() + (self.buf[64 + self.n:] != SENT32).sum())
        assert bad == 0, f"{what}: {bad} sentinel elements around the output were overwritten"


def _tn_args(c, R, ops, out2d, pv, accumulate=False, alpha=1.0, **kw):
    args, _ = K.gemm_tn(ops.A_dev, ops.B_dev, P=c.P, Q=c.Q, R=R, lda=ops.lda, ldb=ops.ldb, out=out2d, accumulate=accumulate, alpha=alpha,
                        batch=c.batch, strideA=ops.strideA if c.batch > 1 else 0, strideB=ops.strideB if c.batch > 1 else 0, p_valid=pv,
                        _args_only=True, **kw)
    if not c.workspace:   # the path a caller without scratch gets: atomics (256 x 256) / the 128-tile kernel's rank form
        args.workspace, args.workspace_bytes = 0, 0
    return args


def _assert_tn_kind(c, R, pv, args, reduce_form=False, segs=0):
    h = L.load()
    plan = G.tn_plan(R, c.P, c.Q, c.batch, c.c_f32, c.variant, pv, reduce_form, segs, c.workspace, ncu=_ncu())
    got = (int(h.wft_gemm_tn_variant(ctypes.byref(args))), int(h.wft_gemm_tn_workspace_bytes(ctypes.byref(args))))
    assert got == (plan["variant"], plan["ws_bytes"]), f"{c.name} R {R}: the plan answers {got}, the restated rule {plan}"
    assert reduce_form or plan["kind"] == c.kind, f"{c.name} R {R} p_valid {pv}: reaches {plan['kind']}, the table names {c.kind}"
    if c.workspace and plan["ws_bytes"]:
        assert args.workspace and args.workspace_bytes >= plan["ws_bytes"]
    return plan


def _run_tn(c, R, seed, outs):
    K.set_variant("tn", c.variant)
    tile = 256 if c.kind in ("TN_4W", "TN_256") else 128
    for pv in c.p_valid:
        ops = G.tn_operands(c, R, seed, p_valid=pv)
        ops.A_dev, ops.B_dev = ops.A_buf.to(DEV), ops.B_buf.to(DEV)
        acc = G.tn_acc(ops, DEV)
        pz = 16 * -(-pv // 16) if pv else c.P
        for form in c.forms:
            what = f"{c.name} R {R} p_valid {pv} {form} seed {seed} [{c.kind}]"
            if form in ("plain", "acc"):
                out = outs.setdefault(("C", c.c_f32), Out(1, c.P, c.Q, c.c_f32))
                out.reset()
                base = None
                if form == "acc":
                    base = torch.randint(-1000, 1001, (c.P, c.Q), generator=torch.Generator().manual_seed(seed)).float().to(DEV)
                    out.view[0].copy_(base)
                args = _tn_args(c, R, ops, out.view[0], pv, accumulate=form == "acc", alpha=0.5 if form == "acc" else 1.0)
                _assert_tn_kind(c, R, pv, args)
                _call("wft_gemm_tn_bf16", args)
                want = G.tn_expected(form, acc, pv, base=base, alpha=0.5 if form == "acc" else 1.0)
                G.assert_exact(out.live[0], want, tile, what)
                if pv and form == "acc":   # accumulation leaves the padding rows of the rank-r operand alone
                    assert torch.equal(out.live[0][pz:], base[pz:]), what + ": padding rows touched"
                out.assert_intact(what)
            elif form in ("seg3", "seg3_acc"):
                ends = [c.P // 3, 2 * c.P // 3, c.P]
                segs = outs.setdefault("segs", [Flat((b - a) * c.Q) for a, b in zip([0] + ends[:-1], ends)])
                views = [s.view.view(-1, c.Q) for s in segs]
                base = None
                if form == "seg3_acc":
                    base = torch.randint(-1000, 1001, (c.P, c.Q), generator=torch.Generator().manual_seed(seed)).float().to(DEV)
                    for v, (a, b) in zip(views, zip([0] + ends[:-1], ends)):
                        v.copy_(base[a:b])
                res = K.gemm_tn(ops.A_dev, ops.B_dev, P=c.P, Q=c.Q, R=R, lda=ops.lda, ldb=ops.ldb, seg_out=views, accumulate=base is not None,
                                _args_only=True)
                assert res is not None, what + ": the library does not take the segments"
                _assert_tn_kind(c, R, pv, res[0], segs=3)
                _call("wft_gemm_tn_bf16", res[0])
                G.assert_exact(torch.cat(views), G.tn_expected("plain", acc, base=base), tile, what)
                for s in segs:
                    s.assert_intact(what)
            elif form == "col_scale":
                for S in (1, 3):
                    rows = 0 if S == 1 else -(-pv // 3)
                    sc = G.col_scale_mat(S, c.Q)
                    out = outs.setdefault(("cs", pv), Out(1, pv, c.Q, True))
                    out.reset()
                    args = _tn_args(c, R, ops, out.view[0], pv, col_scale=sc.to(DEV), scale_rows=rows)
                    _assert_tn_kind(c, R, pv, args, reduce_form=True)
                    _call("wft_gemm_tn_bf16", args)
                    G.assert_exact(out.live[0], G.tn_expected("col_scale", acc, pv, scale=sc, scale_rows=rows), tile, what + f" S {S}")
                    out.assert_intact(what)
            elif form == "block":
                bn, br = c.Q // 3, max(1, pv // 3)
                out = outs.setdefault(("blk", br), Flat(c.Q * br))
                out.reset()
                args = _tn_args(c, R, ops, out.view, pv, block_n=bn, block_r=br)
                _call("wft_gemm_tn_bf16", args)
                G.assert_exact(out.view[None], G.tn_expected("block", acc, pv, block=(bn, br))[None], tile, what)
                out.assert_intact(what)
            elif form == "pair":   # dA with its column scale and dB in block layout: one launch, one reduce launch
                bn, br = c.Q // 3, max(1, pv // 3)
                sc = G.col_scale_mat(1, c.Q)
                oa, ob = outs.setdefault(("cs", pv), Out(1, pv, c.Q, True)), outs.setdefault(("blk", br), Flat(c.Q * br))
                oa.reset(); ob.reset()
                a0 = K.gemm_tn(ops.A_dev, ops.B_dev, P=c.P, Q=c.Q, R=R, lda=ops.lda, ldb=ops.ldb, out=oa.view[0], p_valid=pv, col_scale=sc.to(DEV),
                               _args_only=True, _ws_slot="tn")[0]
                a1 = K.gemm_tn(ops.A_dev, ops.B_dev, P=c.P, Q=c.Q, R=R, lda=ops.lda, ldb=ops.ldb, out=ob.view, p_valid=pv, block_n=bn, block_r=br,
                               _args_only=True, _ws_slot="tn_b")[0]
                L.check(L.load().wft_gemm_tn_rank_pair_bf16(ctypes.byref(a0), ctypes.byref(a1), L.stream_ptr()), "wft_gemm_tn_rank_pair_bf16")
                torch.cuda.synchronize()
                G.assert_exact(oa.live[0], G.tn_expected("col_scale", acc, pv, scale=sc), tile, what + " dA")
                G.assert_exact(ob.view[None], G.tn_expected("block", acc, pv, block=(bn, br))[None], tile, what + " dB")
                oa.assert_intact(what); ob.assert_intact(what)


def _run_tn_gather(c, seed, outs):
    """C[p, q] = B[r(p), q] (A one-hot over R) and C[p, q] = A[r(q), p] (B one-hot), in rounds until every r has been selected"""
    K.set_variant("tn", c.variant)
    tile = 256 if c.kind in ("TN_4W", "TN_256") else 128
    pv = c.p_valid[-1]
    out = outs.setdefault(("C", c.c_f32), Out(1, c.P, c.Q, c.c_f32))
    for probe, n_out, salt in (("gather_a", pv or c.P, 3), ("gather_b", c.Q, 5)):
        g = G.tn_operands(c, c.R, seed, probe)
        g.A_dev, g.B_dev = g.A_buf.to(DEV), g.B_buf.to(DEV)
        if probe == "gather_b" and pv:
            g.A_dev[:, :c.R, pv:c.P] = 0
        for r in range(G.gather_rounds(n_out, c.R)):
            sel = G.gather_sel(n_out, c.R, seed, r, salt).to(DEV)
            if probe == "gather_a":
                g.A_dev[0, :c.R, :c.P] = 0
                g.A_dev[0, sel, torch.arange(n_out, device=DEV)] = 1
                ref = torch.zeros(c.P, c.Q, dtype=torch.float64, device=DEV)
                ref[:n_out] = g.B.to(DEV).double()[0, sel]
            else:
                g.B_dev[0, :c.R, :c.Q] = 0
                g.B_dev[0, sel, torch.arange(c.Q, device=DEV)] = 1
                ref = g.A_dev[0, :c.R, :c.P].double()[sel].t().contiguous()
            out.reset()
            args = _tn_args(c, c.R, g, out.view[0], pv)
            _assert_tn_kind(c, c.R, pv, args)
            _call("wft_gemm_tn_bf16", args)
            G.assert_exact(out.live[0], ref, tile, f"{c.name} {probe} round {r} seed {seed} [{c.kind}]")
            out.assert_intact(f"{c.name} {probe}")


@pytest.mark.parametrize("c", G.TN_CASES, ids=[f"{c.kind}-{c.name}" for c in G.TN_CASES])
def test_tn_kernels_are_exact(c):
    outs = {}
    ragged = c.ragged()
    assert len(ragged) >= 3
    for seed in G.SEEDS:
        _run_tn(c, c.R, seed, outs)
        if c.batch == 1 and "plain" in c.forms:
            _run_tn_gather(c, seed, outs)
    for n, R in enumerate(ragged):   # only R changes; alternate the seeds
        _run_tn(c, R, n % 2, outs)


def test_the_table_names_every_kind():
    assert {c.kind for c in G.NT_CASES} | {r[4] for c in G.NT_CASES for r in G.nt_runs(c)} == set(G.NT_KINDS)
    assert {c.kind for c in G.TN_CASES} == set(G.TN_KINDS)
    assert _ncu() == G.NCU, "the table's shapes were derived for 256 CUs"
