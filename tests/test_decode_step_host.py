"""Host logic of the decoding-step option that needs no GPU: the evaluator forwards `wft_eval_decode_step`, rejects unknown values
and releases the captured steps when a dataset is done; `greedy_decode(step=...)` rejects unknown values before touching a device;
the streaming-GEMM context is thread-local and restores itself."""
import threading

import pytest
import torch

from tests.test_decode_host import _Stub, _Tok, _batch
from whisper_finetune.engine import decode as D
from whisper_finetune.engine.whisper_model import MODEL_DIMS, Whisper
from whisper_finetune.eval import evaluator


class _StepStub(_Stub):
    def greedy_decode(self, mel, prompt, prompt_len, *, step="eager", **kw):
        self.steps = getattr(self, "steps", []) + [step]
        return super().greedy_decode(mel, prompt, prompt_len, **kw)


def test_evaluator_forwards_the_step_mode_and_releases_the_graphs(monkeypatch):
    cfg = {"mixed_precision_training": False, "wft_eval_decode": "greedy"}
    released = []
    monkeypatch.setattr(D, "release_graphs", lambda m: released.append(m))
    decoded = [[0, 1, 26, 2, 3], [0, 1, 26, 4, 5, 26, 6]]
    stub = _StepStub(decoded)
    base = evaluator.evaluate_single_dataset(stub, [_batch()], "syn", cfg, tokenizer=_Tok())
    assert stub.steps == ["eager"] and not released  # absent: today's call, nothing to release
    evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode_step="eager"), tokenizer=_Tok())
    assert stub.steps == ["eager", "eager"] and not released
    got = evaluator.evaluate_single_dataset(stub, [_batch(), _batch()], "syn", dict(cfg, wft_eval_decode_step="graph"), tokenizer=_Tok())
    assert stub.steps == ["eager", "eager", "graph", "graph"]
    assert released == [stub]  # once, when the dataset is done
    assert got.wer == pytest.approx(base.wer)
    for key in ("mean_token_nll", "avg_log_prob", "mean_token_entropy", "ece"):  # token metrics stay teacher-forced
        assert getattr(got, key) == pytest.approx(getattr(base, key)), key
    # a model whose greedy_decode has no `step` keyword still serves the default
    plain = _Stub(decoded)
    evaluator.evaluate_single_dataset(plain, [_batch()], "syn", cfg, tokenizer=_Tok())
    assert len(plain.calls) == 1


def test_evaluator_rejects_an_unknown_step_mode():
    stub = _StepStub([[0], [1]])
    with pytest.raises(ValueError, match="wft_eval_decode_step"):
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", {"mixed_precision_training": False, "wft_eval_decode": "greedy",
                                                                    "wft_eval_decode_step": "cuda-graph"}, tokenizer=_Tok())
    assert not getattr(stub, "steps", [])


def test_greedy_decode_rejects_an_unknown_step_before_touching_the_device():
    m = Whisper(MODEL_DIMS["tiny"])  # on the CPU: a call that got past the check would fail differently
    mel = torch.zeros(1, 80, 3000)
    prompt = torch.tensor([[1, 2, 3]])
    with pytest.raises(ValueError, match="step"):
        m.greedy_decode(mel, prompt, eot=50257, step="bogus")
    with pytest.raises(ValueError, match="step"):
        D.greedy_decode(m, mel, prompt, eot=50257, step=None)
    assert D.STEP_MODES == ("eager", "graph")
    assert D.sessions(m) == {}
    D.release_graphs(m)  # nothing captured: a no-op


def test_stream_gemm_context_is_thread_local_and_nests():
    assert not D.stream_gemm_active()
    seen = []
    with D.stream_gemm():
        assert D.stream_gemm_active()
        t = threading.Thread(target=lambda: seen.append(D.stream_gemm_active()))
        t.start(); t.join()
        with D.stream_gemm(False):
            assert not D.stream_gemm_active()
        assert D.stream_gemm_active()
        with pytest.raises(KeyError):
            with D.stream_gemm():
                raise KeyError("x")
        assert D.stream_gemm_active()
    assert not D.stream_gemm_active() and seen == [False]
