"""The bf16 autograd functions of engine/ops.py -- ConvStemFn, LinearFn through ops.linear (plain, grouped, forward-scaled, LoRA on the
fused and the general route, the MLP pair in its bf16 and one-byte forms, the gradient fork, the gradient homes) and TiedLogitsFn --
held to torch.equal against the float64 autograd references of tests/_ops_exact_cases.py, whose docstring says why the comparison
is exact (integer operands, conditions (a) to (c), GELU the identity from 8 on); tests/test_ops_exact_host.py proves the premises and
rejects the mutants on the CPU.  A failure names the tensor, the first differing index, got and want, and how many elements differ.

The tests take the module state as they find it and put it back (ops.BIAS_GRADS, ops._GELU_AUX8, ops._GRAD_HOMES, the variant bits,
the per-thread column-sum table); ops.reset_colsums() runs before every backward.

Observed on an MI355X: every comparison holds with torch.equal -- ConvStemFn on all five cases, both seeds, before and after w2 <- -w2
under one cache dict; LinearFn on all twenty cases, both seeds, both passes; the MLP pair in the bf16 form, with and without a cast
between the two Linears, and in the one-byte form; the fork with every consumer and with one left out; three accumulating backward
passes into gradient homes and their twin without homes; TiedLogitsFn at 7 and 300 rows.  The GELU premise holds on the device.  The
one-byte form starts at M = 1793, d = 1024 (128 tiles of 256 x 256); there every code is 226 and the gradients are bit-equal to the bf16
form's.  The paired rank-r launch runs for every case marked fused, the single rank-3 adapter included, and for none of the others.
The weight-gradient product of the 37-row group is not one the library writes in segments (LinearFn falls back to one tensor and
slices); the 16384-row group's is written into the three homes, accumulating, in one call.  Each test runs in under two seconds.

One fault was found and fixed: in the one-byte form LinearFn.forward called ctx.mark_non_differentiable twice, the second call
replaced the first, and `act` left the function differentiable (no gradient was wrong: mlp.2 returns None for it; but the bf16 form
and the one-byte form differed in what autograd saw).  test_mlp_pair_one_byte_form_exact asserts `not act.requires_grad`.

Eight wrong-value edits of ops.py, one at a time (even taps swapped in the conv's backward-data shadow, the mask applied twice on the
general route, the fused route's dB blocks reversed, the q bias left unscaled, the fork's running sum dropped, a home overwritten, dE
sliced one row late, a published column sum off by one), each failed the test of its family at the first element that differed."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _ops_exact_cases as S  # noqa: E402
from tests._gelu_codes import _code_index  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402
from whisper_finetune.engine import ops  # noqa: E402

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(autouse=True)
def _module_state():
    saved = (ops.BIAS_GRADS[0], ops._GELU_AUX8, ops._GRAD_HOMES, ops._K_HAS_BIAS[0], dict(K.VARIANT))
    ops.reset_colsums()
    yield
    ops.BIAS_GRADS[0], ops._GELU_AUX8, ops._GRAD_HOMES, ops._K_HAS_BIAS[0] = saved[:4]
    K.VARIANT.update(saved[4])
    ops.reset_colsums()


class _Spy:
    """counts the calls of a module attribute and keeps what they returned"""

    def __init__(self, monkeypatch, module, name):
        self.real, self.calls, self.returned, self.kwargs = getattr(module, name), 0, [], []
        monkeypatch.setattr(module, name, self)

    def __call__(self, *a, **kw):
        self.calls += 1
        self.kwargs.append(kw)
        r = self.real(*a, **kw)
        self.returned.append(r)
        return r


def _dev(t, dtype=F32, grad=False):
    return None if t is None else t.to(DEV, dtype).requires_grad_(grad)


def _set(p, value):
    """an in-place change of a parameter, as an optimizer makes it"""
    with torch.no_grad():
        p.copy_(value.to(p.device, p.dtype))
    p.grad = None


# ------------------------------------------------------------------------------------------------ the GELU premise, on the device
_PREMISE = []


def _gelu_premise():
    """None, or what of the premise fails on this device: for every integer 8..256 GELU is the identity and its derivative 1.0 through
    wft_dgelu_mul_bf16 (dgelu_f), the EPI_GELU epilogue (gelu_f) and the EPI_GELU_GRAD epilogue (gelu_both_f); the products run against
    a one-hot weight, so that the pre-activation is the integer itself."""
    if not _PREMISE:
        lo, hi = S.GELU_RANGE
        v = torch.arange(lo, hi + 1, dtype=F32, device=DEV).to(BF16)
        bad = []
        d = K.dgelu_mul(torch.ones_like(v), v)
        if not torch.equal(d, torch.ones_like(v)):
            bad.append(f"dgelu_mul(1, v) != 1 at v = {v[d != 1][:4].tolist()}")
        x = v.view(-1, 1).repeat(1, 128).contiguous()               # [249, 128]; row m holds the integer 8 + m in every column
        eye = torch.eye(128, dtype=F32, device=DEV).to(BF16)         # one-hot rows: pre[m, n] = x[m, n]
        bias = torch.arange(128, dtype=F32, device=DEV) + 8.0        # and once more with the integer arriving through the bias (x = 0)
        for name, epi in (("EPI_GELU", L.EPI_GELU), ("EPI_GELU_GRAD", L.EPI_GELU_GRAD)):
            for how, rows, b, want in (("product", x, None, x), ("bias", torch.zeros_like(x), bias, bias.to(BF16).expand_as(x))):
                aux = torch.empty_like(x)
                out = K.gemm_nt(rows, eye, bias=b, epilogue=epi, aux=aux)
                if not torch.equal(out, want):
                    bad.append(f"{name} ({how}): gelu(v) != v at v = {want[out != want][:4].tolist()}")
                aux_want = want if epi == L.EPI_GELU else torch.ones_like(want)     # the pre-activation / gelu'
                if not torch.equal(aux, aux_want):
                    bad.append(f"{name} ({how}): aux is not {'v' if epi == L.EPI_GELU else '1.0'} at v = {want[aux != aux_want][:4].tolist()}")
        _PREMISE.append("; ".join(bad) if bad else None)
    return _PREMISE[0]


def test_gelu_premise_on_the_device():
    assert _gelu_premise() is None, _gelu_premise()


def _hold(got, want, what, gelu=False):
    report = S.first_mismatch(got, want, what)
    if report is not None and gelu and _gelu_premise() is not None:
        report = f"the GELU premise fails on this device ({_gelu_premise()}), so this says nothing about the function: {report}"
    assert report is None, report


# ------------------------------------------------------------------------------------------------ ConvStemFn
@pytest.mark.parametrize("case", S.CONV_CASES, ids=str)
def test_conv_stem_fn_exact(case):
    n_mels, d, T, B = case
    c_pad = K.round_up(n_mels, 128)
    cache = {}
    p = None
    for seed in S.SEEDS:
        t = S.conv_inputs(case, seed)
        if p is None:   # the SAME parameter tensors and cache for both seeds: the shadow key has to notice the in-place updates
            p = {k: _dev(t[k], grad=k != "pos") for k in ("w1", "b1", "w2", "b2", "pos")}
        else:
            for k, v in p.items():
                _set(v, t[k])
        for sign in (1.0, -1.0):
            if sign < 0:
                with torch.no_grad():
                    p["w2"].neg_()
                t = S.conv_inputs(case, seed, sign)
            ref = S.conv_ref64(t)
            for v in p.values():
                v.grad = None
            mel_t = K.mel_to_tmajor(_dev(t["mel"]), c_pad)
            out = ops.ConvStemFn.apply(mel_t, p["w1"], p["b1"], p["w2"], p["b2"], p["pos"], cache)
            ops.reset_colsums()
            out.backward(_dev(t["dx"], BF16))
            got = {"out": out, "dw1": p["w1"].grad, "db1": p["b1"].grad, "dw2": p["w2"].grad, "db2": p["b2"].grad}
            assert p["w1"].grad.shape == (d, n_mels, 3)              # the columns n_mels .. c_pad are cut by the function
            _hold(got, {k: ref[k] for k in S.CONV_CHECKED}, f"conv {case} seed {seed} w2 sign {sign:+.0f}", gelu=True)


# ------------------------------------------------------------------------------------------------ LinearFn
def _linear_leaves(case, t):
    W = [_dev(w, grad=True) for w in t["W"]]
    b = [_dev(v, grad=True) for v in t["b"]]
    A = [None if sp is None else _dev(a, grad=sp.train_a) for sp, a in zip(case.lora_list, t["A"])]
    B = [None if sp is None else _dev(v, grad=sp.train_b) for sp, v in zip(case.lora_list, t["B"])]
    return W, b, A, B


def _linear_pass(case, group, leaves, t, ref, what):
    W, b, A, B = leaves
    x = _dev(t["x"], BF16, grad=True)
    res = _dev(t["res"], BF16, grad=True)
    loras = [None if sp is None else ops.LoraSpec(A[i], B[i], S.SCALING, _dev(t["mask"][i])) for i, sp in enumerate(case.lora_list)]
    y = ops.linear(x, group, W, b, loras, residual=res)
    ops.reset_colsums()
    y.backward(_dev(t["dy"], BF16))
    named = {"y": y, "dx": x.grad, "dres": None if res is None else res.grad}
    for i in range(len(W)):
        named |= {f"dW{i}": W[i].grad, f"db{i}": None if b[i] is None else b[i].grad,
                  f"dA{i}": None if A[i] is None else A[i].grad, f"dB{i}": None if B[i] is None else B[i].grad}
    for k, v in named.items():
        assert (v is not None) == (k in ref), f"{what}: {k} {'missing' if v is None else 'returned for a frozen or absent tensor'}"
    got = {k: named[k] for k in ref}
    for k, v in got.items():          # the gradients keep the shapes of their parameters
        if k[0] == "d" and k[1] in "WbAB":
            src = {"W": W, "b": b, "A": A, "B": B}[k[1]][int(k[2:])]
            assert v.shape == src.shape and v.dtype == F32, (what, k, v.shape)
    _hold(got, ref, what)
    return y


@pytest.mark.parametrize("case", S.LINEAR_CASES, ids=str)
def test_linear_fn_exact(case, monkeypatch):
    pair = _Spy(monkeypatch, K, "gemm_nt_rank_pair")
    backwards = 0
    for seed in S.SEEDS:
        group = ops.LinearGroup(case.fwd_scales)
        leaves = None
        for pas in S.PASSES:
            t, ref = S.linear_case(case, seed, pas)
            if leaves is None:
                leaves = _linear_leaves(case, t)
            else:  # the second pass: every parameter changed in place, as by an optimizer that writes through raw pointers
                for dst, src in zip(leaves, (t["W"], t["b"], t["A"], t["B"])):
                    for p, v in zip(dst, src):
                        if p is not None:
                            _set(p, v)
                ops.bump_shadow_epoch()
            y = _linear_pass(case, group, leaves, t, ref, f"{case.name} seed {seed} pass {pas}")
            assert y.shape == (case.M, case.npad) and bool((y[:, case.n:] == 0).all())
            backwards += 1
    if case.fused:
        assert pair.calls == backwards, f"{case.name}: the paired rank-r launch ran {pair.calls} times in {backwards} backward passes"
    else:
        assert pair.calls == 0, f"{case.name}: the paired rank-r launch ran on what should be the general route"


# ------------------------------------------------------------------------------------------------ MLP pair
def _mlp_run(t, what, aux8, cast_between=False, spies=None):
    """-> (checked tensors, codes): mlp.0 with gelu_out feeding mlp.2 with gelu_pre / gelu_codes and a residual"""
    ops._GELU_AUX8, ops.BIAS_GRADS[0] = aux8, True
    d = t["x"].shape[1]
    x, res = _dev(t["x"], BF16, True), _dev(t["res"], BF16, True)
    w1, b1, w2, b2 = (_dev(t[k], grad=True) for k in ("w1", "b1", "w2", "b2"))
    pre, act, codes = ops.linear(x, ops.LinearGroup(), [w1], [b1], gelu_out=True, gelu_next_n=d)
    assert not act.requires_grad
    if cast_between:   # the gradient of `pre` reaches mlp.0 in another tensor: the published column sums do not apply, wft_colsum_bf16 runs
        assert codes is None
        pre = pre.float().to(BF16)
    y = ops.linear(act, ops.LinearGroup(), [w2], [b2], residual=res, gelu_pre=pre, gelu_codes=codes)
    ops.reset_colsums()
    if spies is not None:
        for s in spies:
            s.calls, s.returned = 0, []
    y.backward(_dev(t["dy"], BF16))
    return {"y": y, "dx": x.grad, "dres": res.grad, "dW1": w1.grad, "db1": b1.grad, "dW2": w2.grad, "db2": b2.grad}, codes


@pytest.mark.parametrize("shape", S.MLP_CASES, ids=str)
def test_mlp_pair_bf16_form_exact(shape, monkeypatch):
    fused, colsum = _Spy(monkeypatch, ops, "_fused_colsum"), _Spy(monkeypatch, K, "colsum")
    for seed in S.SEEDS:
        t, ref = S.mlp_case(*shape, seed)
        for aux8 in (True, False):     # (at these sizes the switch must change nothing: no 256 x 256 kernel serves them)
            got, codes = _mlp_run(t, f"mlp {shape}", aux8, spies=(fused, colsum))
            assert codes is None
            _hold(got, ref, f"mlp {shape} seed {seed} bf16 gelu' (_GELU_AUX8 {aux8})", gelu=True)
            # db1 came from the MUL_AUX epilogue's column sums: mlp.0 found the published entry, wft_colsum_bf16 ran for db2 alone
            assert [r is not None for r in fused.returned] == [False, True] and colsum.calls == 1, (fused.returned, colsum.calls)
        got, _ = _mlp_run(t, f"mlp {shape}", True, cast_between=True, spies=(fused, colsum))
        _hold(got, ref, f"mlp {shape} seed {seed} bf16 gelu', a cast in between", gelu=True)
        assert [r is not None for r in fused.returned] == [False, False] and colsum.calls == 2, (fused.returned, colsum.calls)


def _aux8_shape():
    """the smallest (M, d) (fewest elements M * d, then the narrower) for which both queries of LinearFn.forward answer nonzero"""
    best = None
    for d in (128, 256, 384, 512, 640, 768, 1024):
        for M in range(1, 4097):
            if K.gemm_nt_aux8_bytes(M, 4 * d, d, DEV) and K.gemm_nt_aux8_bytes(M, 4 * d, d, DEV, epilogue=L.EPI_MUL_AUX8, colsum=True):
                if best is None or (M * d, d) < (best[0] * best[1], best[1]):
                    best = (M, d)
                break
    return best


def test_mlp_pair_one_byte_form_exact(monkeypatch):
    shape = _aux8_shape()
    assert shape is not None, "no (M <= 4096, d <= 1024) takes the one-byte form"
    print(f"one-byte gelu': smallest shape with both queries nonzero: M = {shape[0]}, d = {shape[1]}")
    fused, colsum = _Spy(monkeypatch, ops, "_fused_colsum"), _Spy(monkeypatch, K, "colsum")
    t, ref = S.mlp_case(*shape, S.SEEDS[0])
    got8, codes = _mlp_run(t, f"mlp {shape}", True, spies=(fused, colsum))
    assert codes is not None and codes.dtype == torch.uint8, "the one-byte form did not run at the shape the queries accept"
    written = codes[_code_index(shape[0], 4 * shape[1], device=DEV)]       # (the buffer also covers the rows behind M of the last tile)
    assert bool((written == 226).all()), "the GELU premise fails on this device: a code of gelu' = 1.0 is not 226"
    _hold(got8, ref, f"mlp {shape} one-byte gelu'", gelu=True)
    assert [r is not None for r in fused.returned] == [False, True] and colsum.calls == 1, (fused.returned, colsum.calls)
    got16, codes16 = _mlp_run(t, f"mlp {shape}", False)
    assert codes16 is None
    _hold(got16, ref, f"mlp {shape} bf16 gelu' at the one-byte shape", gelu=True)
    for k in got8:
        assert torch.equal(got8[k], got16[k]), f"{k} differs between the one-byte and the bf16 form"


# ------------------------------------------------------------------------------------------------ fork
@pytest.mark.parametrize("left_out", (None, 1), ids=("all", "one_left_out"))
@pytest.mark.parametrize("case", S.FORK_CASES, ids=str)
def test_grad_fork_sums_exactly(case, left_out):
    for seed in S.SEEDS:
        t, ref = S.fork_case(case, seed, left_out)
        x = _dev(t["x"], BF16, True)
        xf, acc = ops.grad_fork(x)
        assert ops.grad_fork(x)[0] is xf
        W, b = [_dev(w, grad=True) for w in t["W"]], [_dev(v, grad=True) for v in t["b"]]
        ys = [ops.linear(xf, ops.LinearGroup(), [W[i]], [b[i]], dx_accum=acc) for i in range(3)]
        z = xf.float() * _dev(t["g4"])                                  # the fourth use: plain autograd
        live = [i for i in range(3) if i != left_out]
        ops.reset_colsums()
        torch.autograd.backward([ys[i] for i in live] + [z], [_dev(t["dy"][i], BF16) for i in live] + [torch.ones_like(z)])
        got = {"dx": x.grad}
        for i in live:
            got |= {f"dW{i}": W[i].grad, f"db{i}": b[i].grad}
        _hold(got, ref, f"fork {case} seed {seed} left out {left_out}")
        if left_out is not None:
            assert W[left_out].grad is None and b[left_out].grad is None
        assert acc.buf is None                                           # the fork took the sum


# ------------------------------------------------------------------------------------------------ gradient homes
_HOME_REFS = {}


def _homes_ref(case, seed):
    if (case.name, seed) not in _HOME_REFS:
        _HOME_REFS[(case.name, seed)] = S.homes_case(case, seed)
    return _HOME_REFS[(case.name, seed)]


@pytest.mark.parametrize("homes", (True, False), ids=("homes", "twin_without_homes"))
@pytest.mark.parametrize("case", S.HOME_CASES, ids=str)
def test_gradient_homes_accumulate_exactly(case, homes, monkeypatch):
    ops._GRAD_HOMES = homes
    tn = _Spy(monkeypatch, K, "gemm_tn")
    for seed in S.home_seeds(case):
        ts, total = _homes_ref(case, seed)
        group, leaves = ops.LinearGroup(), _linear_leaves(case, ts[0][0])
        params = [p for lst in leaves[:2] for p in lst if p is not None]
        ptrs = None
        for pas, (t, ref) in enumerate(ts):
            tn.kwargs, tn.returned = [], []
            x = _dev(t["x"], BF16, True)
            y = ops.linear(x, group, leaves[0], leaves[1], [None] * 3)
            ops.reset_colsums()
            y.backward(_dev(t["dy"], BF16))
            _hold({"y": y, "dx": x.grad}, {"y": ref["y"], "dx": ref["dx"]}, f"{case.name} seed {seed} pass {pas}")
            segmented = [kw for kw, r in zip(tn.kwargs, tn.returned) if kw.get("seg_out") is not None and r is not None]
            if pas == 0:
                assert not segmented                                     # no homes noted yet
                _hold({k: leaves[0 if k[1] == "W" else 1][int(k[2:])].grad for k in total}, {k: ref[k] for k in total},
                      f"{case.name} seed {seed} first pass")
                ops.note_grad_homes(params)
                assert all(("_wft_grad_home" in p.__dict__) == (homes and p.dim() == 2) for p in params)
                ptrs = [p.grad.data_ptr() for p in params]
            elif homes and case.M > 300:
                # the product went straight into last step's gradient tensors, accumulating
                assert len(segmented) == 1 and segmented[0]["accumulate"] is True and len(segmented[0]["seg_out"]) == 3, tn.kwargs
            else:
                assert not segmented
        if homes:
            assert [p.grad.data_ptr() for p in params] == ptrs, "a gradient left its home"
        _hold({k: leaves[0 if k[1] == "W" else 1][int(k[2:])].grad for k in total}, total,
              f"{case.name} seed {seed} sum of {S.HOME_PASSES} passes (_GRAD_HOMES {homes})")


# ------------------------------------------------------------------------------------------------ TiedLogitsFn
@pytest.mark.parametrize("rows", S.TIED_ROWS)
def test_tied_logits_fn_exact(rows):
    for seed in S.SEEDS:
        group, emb = ops.LinearGroup(), None
        for pas in S.PASSES:
            t, ref = S.tied_case(rows, seed, pas)
            if emb is None:
                emb = _dev(t["emb"], grad=True)
            else:
                _set(emb, t["emb"])
                ops.bump_shadow_epoch()
            x = _dev(t["x"], BF16, True)
            logits = ops.tied_logits(x, emb, group)
            ops.reset_colsums()
            logits.backward(_dev(t["dl"], BF16))
            assert logits.shape == (rows, 384) and bool((logits[:, S.TIED_V:] == 0).all()) and emb.grad.shape == (S.TIED_V, S.TIED_D)
            _hold({"logits": logits, "dx": x.grad, "dE": emb.grad}, ref, f"tied logits rows {rows} seed {seed} pass {pas}")
