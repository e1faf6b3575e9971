"""Host side of the weight-only int8 decoding path (no GPU): the restated quantiser on rows with known answers, the CPU emulation
of the streaming int8 GEMM against the derived bound of tests/_q8_cases.py on every shape and form, the mutants that bound has to
reject, and the argument errors of the evaluator and of the decode calls."""
import threading

import numpy as np
import pytest
import torch

from tests import _q8_cases as Q8
from tests.test_decode_host import _Stub, _Tok, _batch
from whisper_finetune.engine import decode as D
from whisper_finetune.engine.whisper_model import MODEL_DIMS, Whisper
from whisper_finetune.eval import evaluator


# ----------------------------------------------------------------------------- the quantiser
def test_lossless_rows_round_trip():
    """w = q 2^e with max |q| = 127: scale = 2^e exactly, the bytes are q, q * scale is w."""
    rng = np.random.default_rng(3)
    for e in (-9, -6, 0, 3):
        q = rng.integers(-127, 128, size=(6, 192)).astype(np.int8)
        q[:, 5] = np.array([127, -127, 127, -127, 127, -127], dtype=np.int8)
        w = q.astype(np.float32) * np.float32(2.0 ** e)
        assert np.array_equal(w, Q8.bf16_round(w))
        got, scale = Q8.quantize_rows(w)
        assert np.array_equal(got, q) and np.array_equal(scale, np.full(6, 2.0 ** e, dtype=np.float32))
        assert np.array_equal(got.astype(np.float32) * scale[:, None], w)


def test_zero_rows_and_a_planted_tie():
    rows = Q8.quantizer_rows(128)
    q, scale = Q8.quantize_rows(rows)
    assert scale[0] == 0.0 and not q[0].any()
    assert scale.dtype == np.float32 and q.dtype == np.int8 and np.isfinite(scale).all()
    # row 3: w * inv = +-(m + 0.5) exactly; half-even rounds to the even neighbour
    assert scale[3] == np.float32(0.125) and q[3, 7] == 127
    for k in (0, 1, 2, 3, 4, 5):
        m = k % 100
        want = (m if m % 2 == 0 else m + 1) * (-1 if k % 3 == 0 else 1)
        assert q[3, k] == want, (k, q[3, k], want)
    assert q[2, -1] == 127 and scale[2] == np.float32(1.5) / np.float32(127.0)
    assert q[4, 11] == -127 and q[5, 64] == -127 and np.count_nonzero(q[5]) == 1
    assert np.abs(q).max() <= 127
    # every mutant quantiser differs from the definition on these rows, in the bytes or in the scales
    for mutant in ("half_away", "amax_short", "clamp128"):
        qm, sm = Q8.quantize_rows(rows, mutant=mutant)
        assert not (np.array_equal(qm, q) and np.array_equal(sm, scale)), mutant


def test_fake_quantize_is_q_times_scale_of_the_bf16_rounded_weight():
    w = np.random.default_rng(0).standard_normal((5, 64)).astype(np.float32) * 0.1
    fq = Q8.fake_quantize(w)
    assert np.abs(fq - Q8.bf16_round(w)).max() <= np.abs(w).max() / 127 * 0.5 * 1.01


# ----------------------------------------------------------------------------- the plan, the emulation, the bound
def test_plan_of_the_test_shapes_on_256_cus():
    plans = {(N, K): Q8.stream_plan(N, K) for _, N, K in Q8.SHAPES}
    assert plans == {(128, 64): (1, 1), (256, 384): (6, 1), (384, 1536): (24, 1), (32768, 320): (3, 2), (51968, 384): (2, 3)}


@pytest.fixture(scope="module")
def cases():
    return {shape: Q8.make_case(*shape) for shape in Q8.SHAPES}


@pytest.mark.parametrize("shape", Q8.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulation_stays_inside_the_bound(cases, shape):
    case = cases[shape]
    split, per = Q8.stream_plan(shape[1], shape[2])
    for name, form in Q8.FORMS.items():
        got = Q8.emulate(case, split, per, **form)
        ref, _ = Q8.gemm_ref64(case, **form)
        bound, _ = Q8.gemm_bound(case, split, **form)
        ratio = float((np.abs(got - ref) / bound).max())
        print(f"{shape} {name}: largest |emulation - f64| / bound = {ratio:.3f}")
        assert ratio <= 1.0, (shape, name, ratio)


GEMM_MUTANTS = ["no_scale", "scale_next_row", "scale_after_bias", "unsigned", "drop_last_slice", "drop_odd_step"]


@pytest.mark.parametrize("mutant", GEMM_MUTANTS)
def test_the_bound_rejects_gemm_mutants(cases, mutant):
    """On the smallest shape whose plan gives the mutant something to do (a second slice; a second step in a slice)."""
    shape = {"drop_last_slice": (16, 256, 384), "drop_odd_step": (5, 32768, 320)}.get(mutant, (16, 256, 384))
    case = cases[shape]
    split, per = Q8.stream_plan(shape[1], shape[2])
    form = Q8.FORMS["bias"]
    got = Q8.emulate(case, split, per, mutant=mutant, **form)
    ref, _ = Q8.gemm_ref64(case, **form)
    bound, _ = Q8.gemm_bound(case, split, **form)
    bad = np.abs(got - ref) > bound
    print(f"{mutant}: {bad.mean():.3f} of the elements outside the bound")
    assert bad.mean() > 0.5, mutant


@pytest.mark.parametrize("mutant", ["half_away", "amax_short", "clamp128"])
def test_the_bound_rejects_quantiser_mutants(mutant):
    """The GEMM over a mutant quantiser's (Q, scale) of the structured rows, against the reference over the definition's: outside the
    bound on the row the mutant gets wrong (ties; the maximum in the last column; a row with a positive maximum, which comes back with its sign flipped)."""
    rows = Q8.quantizer_rows(128)
    W = np.tile(rows, (15, 1))[:128]
    q, scale = Q8.quantize_rows(W)
    qm, sm = Q8.quantize_rows(W, mutant=mutant)
    rng = np.random.default_rng(11)
    A = Q8.bf16_round(np.abs(rng.standard_normal((4, 128), dtype=np.float32)) + 0.5)
    zero = np.zeros(128, dtype=np.float32)
    good = dict(A=A, Q=q, scale=scale, bias=zero, res=None, M=4, N=128, K=128)
    bad = dict(good, Q=qm, scale=sm)
    split, per = Q8.stream_plan(128, 128)
    ref, _ = Q8.gemm_ref64(good)
    bound, _ = Q8.gemm_bound(good, split)
    assert (np.abs(Q8.emulate(good, split, per) - ref) <= bound).all()
    out = np.abs(Q8.emulate(bad, split, per) - ref) > bound
    row = {"half_away": 3, "amax_short": 2, "clamp128": 2}[mutant]
    assert out[:, row].all(), (mutant, out[:, :9])


# ----------------------------------------------------------------------------- argument errors
class _WeightsStub(_Stub):
    def greedy_decode(self, mel, prompt, prompt_len, *, step="eager", weights="bf16", **kw):
        self.seen = getattr(self, "seen", []) + [(step, weights)]
        return super().greedy_decode(mel, prompt, prompt_len, **kw)


def test_evaluator_forwards_int8_and_rejects_bad_values(monkeypatch):
    monkeypatch.setattr(D, "release_graphs", lambda m: None)
    cfg = {"mixed_precision_training": False, "wft_eval_decode": "greedy"}
    stub = _WeightsStub([[0, 1, 26, 2, 3], [0, 1, 26, 4, 5, 26, 6]])
    evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode_step="graph", wft_eval_decode_weights="int8"), tokenizer=_Tok())
    evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode_step="graph", wft_eval_decode_weights="bf16"), tokenizer=_Tok())
    assert stub.seen == [("graph", "int8"), ("graph", "bf16")]
    with pytest.raises(ValueError, match="wft_eval_decode_weights"):  # an unknown value
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode_step="graph", wft_eval_decode_weights="int4"), tokenizer=_Tok())
    with pytest.raises(ValueError, match="wft_eval_decode_weights"):  # int8 without the graph step
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode_weights="int8"), tokenizer=_Tok())
    with pytest.raises(ValueError, match="wft_eval_decode_weights"):
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode_step="eager", wft_eval_decode_weights="int8"), tokenizer=_Tok())
    assert len(stub.seen) == 2


def test_int8_needs_the_graph_step_in_every_decode_call():
    m = Whisper(MODEL_DIMS["tiny"])  # on the CPU: a call that got past the check would fail differently
    mel = torch.zeros(1, 80, 3000)
    prompt = torch.tensor([[1, 2, 3]])
    kw = dict(eot=50257, weights="int8")
    calls = {
        "greedy_decode": lambda **k: m.greedy_decode(mel, prompt, **k),
        "beam_decode": lambda **k: m.beam_decode(mel, prompt, beam_size=2, **k),
        "sample_decode": lambda **k: m.sample_decode(mel, prompt, temperature=0.5, best_of=2, **k),
        "decode_with_fallback": lambda **k: m.decode_with_fallback(mel, prompt, **k),
        "transcribe": lambda **k: m.transcribe(torch.zeros(16000), sot_sequence=(1, 2, 3), **k),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="int8.*graph"):
            call(**kw)
        with pytest.raises(ValueError, match="int8.*graph"):
            call(step="eager", **kw)
        with pytest.raises(ValueError, match="weights"):
            call(eot=50257, step="graph", weights="int4")
    m.set_compute_dtype("fp32")
    with pytest.raises(NotImplementedError):
        m.greedy_decode(mel, prompt, step="graph", **kw)
    assert D.sessions(m) == {} and D.beam_sessions(m) == {} and D.sample_sessions(m) == {}
    assert D.WEIGHT_MODES == ("bf16", "int8")


def test_weights_mode_is_thread_local_and_follows_the_switch():
    assert D.stream_gemm_weights() == "bf16"
    seen = []
    with D.stream_gemm(True, weights="int8"):
        assert D.stream_gemm_active() and D.stream_gemm_weights() == "int8"
        t = threading.Thread(target=lambda: seen.append((D.stream_gemm_active(), D.stream_gemm_weights())))
        t.start(); t.join()
        with D.stream_gemm():
            assert D.stream_gemm_weights() == "bf16"
        with D.stream_gemm(False, weights="int8"):
            assert D.stream_gemm_weights() == "bf16"  # nothing streams: nothing reads int8
        assert D.stream_gemm_weights() == "int8"
    assert D.stream_gemm_weights() == "bf16" and seen == [(False, "bf16")]
    with pytest.raises(ValueError, match="weights"):
        with D.stream_gemm(True, weights="fp8"):
            pass


# ----------------------------------------------------------------------------- the host predicate of the int8 entry point
def test_q8_predicate_follows_the_bf16_rule_plus_its_own():
    """wft_gemm_nt_stream_q8_ok: the rule of wft_gemm_nt_stream_ok, ldb % 16, and the one shape measured not to win (1280 x 1280,
    DESIGN.md §5); the workspace is the bf16 entry point's (the same plan).  Pure host functions: no device."""
    import ctypes

    from tests.test_gemm_stream_abi import LARGE_V3, TINY, _args
    from whisper_finetune.engine import lib as L

    h = L.load()
    for M in (1, 8, 32):
        for N, K in TINY + LARGE_V3:
            a = _args(M, N, K, bias=1 << 21, epilogue=L.EPI_GELU)
            served = h.wft_gemm_nt_stream_q8_ok(ctypes.byref(a))
            assert served == (0 if (N, K) == (1280, 1280) else 1), (M, N, K)
            ws = h.wft_gemm_nt_stream_q8_workspace_bytes(ctypes.byref(a))
            assert ws == (h.wft_gemm_nt_stream_workspace_bytes(ctypes.byref(a)) if served else 0)
    for kw, reason in ((dict(M=33), "M must lie"), (dict(K=96), "multiple of 64"), (dict(ldb=384 + 8), "ldb must be a multiple of 16"),
                       (dict(B=(1 << 20) + 8), "16-byte aligned"), (dict(epilogue=L.EPI_GELU_GRAD), "epilogue"), (dict(N=1280, K=1280, lda=1280, ldb=1280, ldc=1280), "excluded shape")):
        a = _args(**dict(dict(M=8, N=256, K=384), **{k: v for k, v in kw.items() if k in ("M", "N", "K")}), **{k: v for k, v in kw.items() if k not in ("M", "N", "K")})
        assert h.wft_gemm_nt_stream_q8_ok(ctypes.byref(a)) == 0 and h.wft_gemm_nt_stream_q8_workspace_bytes(ctypes.byref(a)) == 0, kw
        assert h.wft_gemm_nt_stream_q8(ctypes.byref(a), None, None) == -3, kw  # WFT_ERR_UNSUPPORTED, before any device call
        msg = L.last_error()
        assert "wft_gemm_nt_stream_q8" in msg and "not served" in msg and reason in msg, (kw, msg)
    assert h.wft_gemm_nt_stream_q8_ok(None) == 0
