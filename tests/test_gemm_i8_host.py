"""Host side of the W8A8 path (no GPU): the conditions the operand builders of tests/_i8_cases.py promise, the numpy reference
against a float64 evaluation, the proof that every mutant kernel changes an output bit somewhere in the case table (so the bit-for-bit
GPU tests over that table reject it), the host predicate wft_gemm_nt_i8_ok with every refusal, and the rules of the "w8a8" mode on
stubs: argument errors of every decode call, the evaluator, the thread-local context, what `ops.linear` leaves alone."""
import ctypes
import threading

import numpy as np
import pytest
import torch

from tests import _i8_cases as I8
from tests.test_decode_host import _Stub, _Tok, _batch
from tests.test_gemm_stream_abi import LARGE_V3, TINY, _args
from whisper_finetune.engine import decode as D
from whisper_finetune.engine import kernels as K
from whisper_finetune.engine import lib as L
from whisper_finetune.engine import ops
from whisper_finetune.engine.whisper_model import MODEL_DIMS, Whisper
from whisper_finetune.eval import evaluator

TABLE = I8.table()
IDS = [t[0] for t in TABLE]


# ----------------------------------------------------------------------------- the builders
def test_the_table_covers_what_it_claims():
    shapes = {(kw["M"], kw["N"], kw["K"]) for _, kw, _ in TABLE if kw.get("kind") is None}
    assert shapes == {(M, N, K) for M in I8.MS for N in I8.NS for K in I8.KS}
    assert I8.MS == (1, 33, 127, 128, 129, 255, 256, 257) and I8.NS == (128, 256, 384) and I8.KS == (64, 128, 192, 320)
    for M in I8.MS:  # every M meets every form
        assert {form for _, kw, form in TABLE if kw["M"] == M and kw.get("kind") is None} == set(I8.FORMS)
    assert {(form, kw["scales"]) for _, kw, form in TABLE} >= {(f, s) for f in I8.FORMS for s in I8.SCALES}
    assert sum(kw.get("kind") == "deep" for _, kw, _ in TABLE) == 1 and sum(kw.get("kind") == "neg128" for _, kw, _ in TABLE) == 1
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("entry", TABLE, ids=IDS)
def test_builders_keep_their_promises(entry):
    _, kw, _ = entry
    c = I8.make_case(**kw)
    M, N, K, A, B = c["M"], c["N"], c["K"], c["A"], c["B"]
    assert A.dtype == np.int8 and B.dtype == np.int8 and c["a_scale"].dtype == np.float32 and c["b_scale"].dtype == np.float32
    # the pad columns hold poison, and there is a whole k-step of them behind A
    assert c["lda"] >= K + 64 and c["ldb"] >= c["lda"] and c["lda"] % 16 == 0 and c["ldb"] % 16 == 0 and c["ldc"] > N and c["ldc"] % 4 == 0
    assert (A[:, K:] == I8.POISON).all() and (B[:, K:] == I8.POISON).all()
    a, b = A[:, :K].astype(np.int64), B[:, :K].astype(np.int64)
    # asymmetric: the product is not its own transpose on the common square, and A is not B
    acc = I8.blocks(c).sum(axis=0)
    assert np.array_equal(acc, a @ b.T)
    s = min(M, N)
    if s > 1:
        assert not np.array_equal(acc[:s, :s], acc[:s, :s].T)
        assert not np.array_equal(a[:s], b[:s])
    # rows M-1 and M-2 differ from every other row
    for r in {M - 1, max(M - 2, 0)}:
        others = np.delete(a, r, axis=0)
        assert not (others == a[r]).all(axis=1).any(), r
    blk = I8.blocks(c)
    if kw.get("kind") != "deep":
        # every k-block carries a different nonzero contribution to element (0, 0)
        contrib = blk[:, 0, 0]
        assert (contrib != 0).all() and len(set(contrib.tolist())) == len(contrib), contrib
        assert (a < 0).any() and (b < 0).any()
    assert np.abs(acc).max() < 2 ** 31
    c_buf = I8.new_c(c)
    assert c_buf.shape == (M + I8.GUARD_ROWS, c["ldc"]) and (c_buf == I8.SENTINEL).all()
    assert I8.SENTINEL == I8.bf16_round(np.array([I8.SENTINEL]))[0]
    for form in I8.FORMS.values():  # no case produces the sentinel
        out = I8.reference(c, **form)
        assert not (out[:M, :N] == I8.SENTINEL).any()
        assert (out[M:] == I8.SENTINEL).all() and (out[:, N:] == I8.SENTINEL).all()


def test_the_deep_case_sees_the_int_to_float_rounding():
    (_, kw, form), = [t for t in TABLE if t[1].get("kind") == "deep"]
    c = I8.make_case(**kw)
    assert (c["M"], c["N"], c["K"]) == (129, 128, 5120)
    assert set(np.unique(c["A"][:, :c["K"]])) == {-127, 127} and set(np.unique(c["B"][:, :c["K"]])) == {-127, 127}
    acc = I8.blocks(c).sum(axis=0)
    f = acc.astype(np.float32)
    inexact = (np.abs(acc) > 2 ** 24) & (f.astype(np.int64) != acc)
    print(f"deep case: {int((np.abs(acc) > 2 ** 24).sum())} elements above 2^24, {int(inexact.sum())} with an inexact conversion")
    assert inexact.sum() > 1000
    m, n = c["tie"]
    assert inexact[m, n] and int(f[m, n]) == int(acc[m, n]) + 2  # round-to-nearest-even went up; truncation goes down
    assert I8._to_f32(acc, truncate=True)[m, n] == np.float32(int(acc[m, n]) - 2)
    # no other case of the table reaches 2^24
    for _, kw2, _ in TABLE:
        if kw2.get("kind") != "deep":
            assert np.abs(I8.blocks(I8.make_case(**kw2)).sum(axis=0)).max() < 2 ** 24


def test_the_neg128_case_holds_the_byte():
    (_, kw, _), = [t for t in TABLE if t[1].get("kind") == "neg128"]
    c = I8.make_case(**kw)
    K_ = c["K"]
    assert (c["A"][:, :K_] == -128).sum() > K_ and (c["B"][:, :K_] == -128).sum() > K_
    assert I8.blocks(c).sum(axis=0)[c["M"] - 3, c["N"] - 2] == 128 * 128 * K_


@pytest.mark.parametrize("entry", TABLE, ids=IDS)
def test_reference_agrees_with_float64_within_one_bf16_ulp(entry):
    _, kw, form = entry
    c = I8.make_case(**kw)
    M, N = c["M"], c["N"]
    got = I8.reference(c, **I8.FORMS[form])[:M, :N].astype(np.float64)
    want, _ = I8.ref64(c, **I8.FORMS[form])
    ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 7)  # the spacing of bf16 at `want`
    worst = float((np.abs(got - want) / ulp).max())
    print(f"{entry[0]}: largest |reference - f64| = {worst:.3f} bf16 ulp")
    assert worst <= 1.0


@pytest.mark.parametrize("entry", [t for t in TABLE if I8.FORMS[t[2]]["gelu"]][::4], ids=lambda t: t[0])
def test_gelu_bound_holds_for_the_float64_gelu_and_rejects_a_wrong_one(entry):
    """The bound is wider than one bf16 rounding of the exact value and far narrower than a tanh-approximated GELU's error."""
    _, kw, form = entry
    c = I8.make_case(**kw)
    M, N = c["M"], c["N"]
    f = {k: v for k, v in I8.FORMS[form].items() if k != "gelu"}
    target, bound = I8.gelu_bound(c, **f)
    assert (np.abs(I8.reference(c, **I8.FORMS[form])[:M, :N] - target) <= bound).all()
    assert (np.abs(I8.reference(c, mutant="drop_last_kblock", **I8.FORMS[form])[:M, :N] - target) > bound).any()


@pytest.mark.parametrize("mutant", I8.MUTANTS)
def test_every_mutant_changes_an_output_bit_on_the_table(mutant):
    """The exact forms only (plain / bias / bias + residual): those are the cases the GPU test holds bit for bit.  The one mutant that
    lives in a GELU form (the residual added first) has to leave the GELU bound instead."""
    hits = []
    for name, kw, form in TABLE:
        c = I8.make_case(**kw)
        M, N = c["M"], c["N"]
        flags = I8.FORMS[form]
        if mutant == "residual_before_gelu":
            if not (flags["gelu"] and flags["res"]):
                continue
            target, bound = I8.gelu_bound(c, bias=flags["bias"], res=True)
            if (np.abs(I8.reference(c, mutant=mutant, **flags)[:M, :N] - target) > bound).any():
                hits.append(name)
        elif form in I8.EXACT_FORMS:
            if not np.array_equal(I8.reference(c, mutant=mutant, **flags), I8.reference(c, **flags)):
                hits.append(name)
        if len(hits) >= 3:
            break
    print(f"{mutant}: first cases that see it: {hits}")
    assert hits, mutant


def test_the_truncating_mutant_is_seen_by_the_deep_case_only():
    for name, kw, form in TABLE:
        c = I8.make_case(**kw)
        same = np.array_equal(I8.reference(c, mutant="truncating_cvt", **I8.FORMS[form]), I8.reference(c, **I8.FORMS[form]))
        assert same == (kw.get("kind") != "deep"), name


# ----------------------------------------------------------------------------- the host predicate
I8_SHAPES = TINY[:4] + LARGE_V3[:4] + [(2560, 1280), (768, 384)]


@pytest.mark.parametrize("M", [1, 33, 1500, 12000, 48000])
def test_i8_predicate_serves_the_shapes_of_the_mode(M):
    h = L.load()
    for N, Kd in I8_SHAPES:
        for kw in ({}, {"bias": 1 << 21}, {"bias": 1 << 21, "residual": 1 << 22, "ldr": N}, {"epilogue": L.EPI_GELU},
                   {"bias": 1 << 21, "epilogue": L.EPI_GELU, "residual": 1 << 22, "ldr": N}):
            assert h.wft_gemm_nt_i8_ok(ctypes.byref(_args(M, N, Kd, **kw))) == 1, (M, N, Kd, kw)
        assert K.gemm_nt_i8_serves(M, N, Kd) and K.gemm_nt_i8_serves(M, N, Kd, L.EPI_GELU)
    assert h.wft_gemm_nt_i8_ok(ctypes.byref(_args(M, 128, 65536))) == 1  # the deepest K whose sum cannot overflow
    assert h.wft_gemm_nt_i8_ok(ctypes.byref(_args(M, 128, 64, lda=80, ldb=4096, ldc=132))) == 1


I8_REFUSED = {
    "M below 1": (dict(M=0), "M must lie"),
    "f32 C": (dict(c_is_f32=1), "C must be bf16"),
    "accumulate": (dict(accumulate=1), "C must be bf16"),
    "batch 2": (dict(batch=2), "batch must be 1"),
    "alpha": (dict(alpha=0.5), "alpha must be 1"),
    "colsum": (dict(colsum=1 << 24), "colsum"),
    "p_valid": (dict(p_valid=8), "p_valid"),
    "valid_rows_period": (dict(valid_rows_period=4, valid_rows=3), "valid_rows_period"),
    "DGELU": (dict(epilogue=L.EPI_DGELU), "epilogue"),
    "GELU_GRAD": (dict(epilogue=L.EPI_GELU_GRAD), "epilogue"),
    "MUL_AUX": (dict(epilogue=L.EPI_MUL_AUX), "epilogue"),
    "aux": (dict(epilogue=L.EPI_GELU, aux=1 << 23, ldaux=256), "aux is not served"),
    "residual before the epilogue": (dict(residual=1 << 22, ldr=256, residual_first=1), "residual is added after"),
    "beta": (dict(residual=1 << 22, ldr=256, beta=0.5), "beta 1"),
    "N % 128 != 0": (dict(N=192, ldc=192), "N must be a multiple of 128"),
    "K % 64 != 0": (dict(K=96, lda=96, ldb=96), "K must be a multiple of 64"),
    "K above 65536": (dict(K=65600, lda=65600, ldb=65600), "at most 65536"),
    "lda % 16 != 0": (dict(lda=384 + 8), "multiples of 16"),
    "ldb % 16 != 0": (dict(ldb=384 + 8), "multiples of 16"),
    "ldc % 4 != 0": (dict(ldc=258), "ldc must be a multiple of 4"),
    "A misaligned": (dict(A=(1 << 20) + 8), "16-byte aligned"),
    "B misaligned": (dict(B=(1 << 20) + 8), "16-byte aligned"),
    "C misaligned": (dict(C=(1 << 20) + 8), "16-byte aligned"),
    "bias misaligned": (dict(bias=(1 << 21) + 4), "bias must be 16-byte aligned"),
    "residual misaligned": (dict(residual=(1 << 22) + 2, ldr=256), "residual alignment"),
    "ldr % 4 != 0": (dict(residual=1 << 22, ldr=258), "residual alignment"),
    "null B": (dict(B=0), "null pointer"),
}


@pytest.mark.parametrize("what", sorted(I8_REFUSED))
def test_i8_refusals_come_with_their_reason_before_any_device_call(what):
    h = L.load()
    kw, reason = I8_REFUSED[what]
    a = _args(**{**dict(M=40, N=256, K=384), **kw})
    assert h.wft_gemm_nt_i8_ok(ctypes.byref(a)) == 0, what
    scale = (ctypes.c_float * 512)()  # (never read: the refusal comes first)
    assert h.wft_gemm_nt_i8(ctypes.byref(a), ctypes.addressof(scale), ctypes.addressof(scale), None) == -3, what  # WFT_ERR_UNSUPPORTED
    msg = L.last_error()
    assert "wft_gemm_nt_i8" in msg and "not served" in msg and reason in msg, (what, msg)
    if set(kw) <= {"M", "N", "K", "epilogue"}:
        assert not K.gemm_nt_i8_serves(kw.get("M", 40), kw.get("N", 256), kw.get("K", 384), kw.get("epilogue", L.EPI_NONE))


def test_i8_null_arguments_and_scales():
    h = L.load()
    assert h.wft_gemm_nt_i8_ok(None) == 0 and h.wft_gemm_nt_i8(None, None, None, None) == -3
    a = _args(40, 256, 384)
    assert h.wft_gemm_nt_i8(ctypes.byref(a), None, None, None) == -1  # WFT_ERR_ARG: a served call without its scales, nothing launched
    assert "a_scale" in L.last_error()


# ----------------------------------------------------------------------------- the mode on stubs
def test_w8a8_needs_the_graph_step_in_every_decode_call():
    m = Whisper(MODEL_DIMS["tiny"])  # on the CPU: a call that got past the check would fail differently
    mel = torch.zeros(1, 80, 3000)
    prompt = torch.tensor([[1, 2, 3]])
    kw = dict(eot=50257, weights="w8a8")
    calls = {
        "greedy_decode": lambda **k: m.greedy_decode(mel, prompt, **k),
        "beam_decode": lambda **k: m.beam_decode(mel, prompt, beam_size=2, **k),
        "sample_decode": lambda **k: m.sample_decode(mel, prompt, temperature=0.5, best_of=2, **k),
        "decode_with_fallback": lambda **k: m.decode_with_fallback(mel, prompt, **k),
        "transcribe": lambda **k: m.transcribe(torch.zeros(16000), sot_sequence=(1, 2, 3), **k),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="w8a8.*graph"):
            call(**kw)
        with pytest.raises(ValueError, match="w8a8.*graph"):
            call(step="eager", **kw)
        with pytest.raises(ValueError, match="bf16.*int8.*w8a8"):  # a fourth value: the message names the three
            call(eot=50257, step="graph", weights="w4a8")
    m.set_compute_dtype("fp32")
    with pytest.raises(NotImplementedError):
        m.greedy_decode(mel, prompt, step="graph", **kw)
    assert D.sessions(m) == {} and D.beam_sessions(m) == {} and D.sample_sessions(m) == {}
    assert D.DECODE_WEIGHTS == ("bf16", "int8", "w8a8")
    assert [D.step_weights(w) for w in D.DECODE_WEIGHTS] == ["bf16", "int8", "int8"]  # the cached steps of w8a8 are the int8 ones


class _WeightsStub(_Stub):
    def greedy_decode(self, mel, prompt, prompt_len, *, step="eager", weights="bf16", **kw):
        self.seen = getattr(self, "seen", []) + [(step, weights)]
        return super().greedy_decode(mel, prompt, prompt_len, **kw)


def test_evaluator_forwards_w8a8_and_rejects_a_fourth_value(monkeypatch):
    monkeypatch.setattr(D, "release_graphs", lambda m: None)
    cfg = {"mixed_precision_training": False, "wft_eval_decode": "greedy"}
    stub = _WeightsStub([[0, 1, 26, 2, 3], [0, 1, 26, 4, 5, 26, 6]])
    evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode_step="graph", wft_eval_decode_weights="w8a8"), tokenizer=_Tok())
    assert stub.seen == [("graph", "w8a8")]
    with pytest.raises(ValueError, match="wft_eval_decode_weights.*bf16.*int8.*w8a8"):
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode_step="graph", wft_eval_decode_weights="w8a16"), tokenizer=_Tok())
    for bad in (dict(), dict(wft_eval_decode_step="eager")):  # w8a8 without the graph step
        with pytest.raises(ValueError, match="wft_eval_decode_weights.*w8a8"):
            evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode_weights="w8a8", **bad), tokenizer=_Tok())
    with pytest.raises(ValueError, match="wft_eval_decode_weights"):  # without wft_eval_decode at all
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", {"mixed_precision_training": False, "wft_eval_decode_step": "graph",
                                                                    "wft_eval_decode_weights": "w8a8"}, tokenizer=_Tok())
    assert len(stub.seen) == 1


def test_int8_gemm_context_is_thread_local_and_restores():
    assert not D.int8_gemm_active()
    seen = []
    with D.int8_gemm():
        assert D.int8_gemm_active() and not D.stream_gemm_active()  # independent of the streaming switch
        t = threading.Thread(target=lambda: seen.append(D.int8_gemm_active()))
        t.start(); t.join()
        with D.int8_gemm(False):
            assert not D.int8_gemm_active()
        assert D.int8_gemm_active()
        with D.stream_gemm(True, weights="int8"):
            assert D.int8_gemm_active() and D.stream_gemm_weights() == "int8"
    assert not D.int8_gemm_active() and seen == [False]
    with pytest.raises(RuntimeError):
        with D.int8_gemm():
            raise RuntimeError("x")
    assert not D.int8_gemm_active()


def test_encode_runs_the_encoder_under_the_context_for_w8a8_only():
    class M_:
        def encoder(self, mel):
            return D.int8_gemm_active()

    assert D.encode(M_(), None, "w8a8") is True
    assert D.encode(M_(), None, "int8") is False and D.encode(M_(), None, "bf16") is False and D.encode(M_(), None) is False
    assert not D.int8_gemm_active()


def test_ops_linear_takes_the_i8_kernel_only_under_no_grad_and_above_32_rows(monkeypatch):
    calls = []
    group = ops.LinearGroup()
    w = torch.zeros(256, 128)
    monkeypatch.setattr(group, "shadows_q8", lambda weights, biases, loras=None: ("Q", "qs", "bias"))
    monkeypatch.setattr(K, "gemm_nt_i8_serves", lambda M, N, Kd, epi=L.EPI_NONE: calls.append(("serves", M, N, Kd, epi)) or True)
    monkeypatch.setattr(K, "quantize_rows_i8", lambda x: calls.append(("quantize", tuple(x.shape))) or ("xq", "xs"))
    monkeypatch.setattr(K, "gemm_nt_i8", lambda xq, xs, Q, qs, **kw: calls.append(("gemm", xq, xs, Q, qs, kw["bias"], kw["epilogue"])) or "i8")
    monkeypatch.setattr(ops.LinearFn, "apply", staticmethod(lambda *a: "bf16"))
    big, small = torch.zeros(33, 128, dtype=torch.bfloat16), torch.zeros(32, 128, dtype=torch.bfloat16)
    with torch.no_grad():
        assert ops.linear(big, group, [w], [None]) == "bf16" and not calls  # outside the context
        with D.int8_gemm():
            assert ops.linear(small, group, [w], [None]) == "bf16" and not calls  # M <= 32
            assert ops.linear(big, group, [w], [None]) == "i8"
            assert calls == [("serves", 33, 256, 128, L.EPI_NONE), ("quantize", (33, 128)), ("gemm", "xq", "xs", "Q", "qs", "bias", L.EPI_NONE)]
            del calls[:]
            assert ops.linear(big, group, [w], [None], gelu_out=True) == (None, "i8", None)
            assert [c[0] for c in calls] == ["serves", "quantize", "gemm"] and calls[0][4] == L.EPI_GELU and calls[2][6] == L.EPI_GELU
            del calls[:]
            monkeypatch.setattr(K, "gemm_nt_i8_serves", lambda *a: False)
            assert ops.linear(big, group, [w], [None]) == "bf16" and not calls  # a product the kernel does not serve
            monkeypatch.setattr(K, "gemm_nt_i8_serves", lambda *a: True)
    with D.int8_gemm():
        assert torch.is_grad_enabled()
        assert ops.linear(big, group, [w], [None]) == "bf16" and not calls  # grad mode
