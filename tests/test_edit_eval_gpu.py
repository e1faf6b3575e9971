"""The evaluator on the device: WER / CER of a whole dataset from one wft_edit_counts_i32 launch — the floats metrics.wer / metrics.cer
give for the stored strings, the counts of the host rule, the corpus totals, and one K.edit_counts call per dataset."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests.test_eval import _Tok  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine.whisper_model import ModelDimensions, Whisper  # noqa: E402
from whisper_finetune.eval import evaluator  # noqa: E402
from whisper_finetune.eval import metrics as M  # noqa: E402


def _case():
    """The small model and the two batches of tests/test_eval.py's end-to-end case."""
    dims = ModelDimensions(80, 100, 128, 2, 2, 128, 32, 128, 2, 2)
    params = O.init_params(O.ModelDimensions(**vars(dims)), seed=1, std=0.3)
    m = Whisper(dims)
    m.load_state_dict(params)
    m.cuda()
    g = torch.Generator().manual_seed(0)
    batches = []
    for _ in range(2):
        y_out = torch.randint(0, 27, (3, 10), generator=g)
        y_out[0, -3:] = -100
        y_out[2, :] = -100
        batches.append((torch.randn(3, 80, 200, generator=g), torch.randint(0, 27, (3, 10), generator=g), y_out))
    return m, batches


def test_evaluator_scores_a_dataset_with_one_launch(monkeypatch):
    m, batches = _case()
    calls = []
    real = K.edit_counts

    def spy(sym, rows, *a, **kw):
        calls.append(len(rows))
        return real(sym, rows, *a, **kw)

    monkeypatch.setattr(K, "edit_counts", spy)
    cfg = {"mixed_precision_training": True, "mp_dtype": "bf16"}
    d = evaluator.evaluate_single_dataset(m, batches, "syn", cfg, tokenizer=_Tok())
    assert d.num_samples == 4 and calls == [8]  # one call per dataset: four word pairs and four character pairs
    tw, tc = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    for u in d.per_utterance:
        assert u.wer == M.wer(u.reference, u.prediction) and u.cer == M.cer(u.reference, u.prediction)
        assert u.word_counts == M.edit_counts_host(u.reference.split(), u.prediction.split())
        assert u.char_counts == M.edit_counts_host(list(u.reference.strip()), list(u.prediction.strip()))
        tw += u.word_counts
        tc += u.char_counts
    assert any(u.cer > 0 for u in d.per_utterance)
    assert d.wer == np.mean([u.wer for u in d.per_utterance]) and d.cer == np.mean([u.cer for u in d.per_utterance])
    nw = int(tw[:3].sum())
    assert d.corpus_wer == int(tw[1:].sum()) / nw and d.corpus_cer == int(tc[1:].sum()) / int(tc[:3].sum())
    assert (d.word_sub_rate, d.word_del_rate, d.word_ins_rate) == (int(tw[1]) / nw, int(tw[2]) / nw, int(tw[3]) / nw)
    del calls[:]
    res, _ = evaluator.evaluate_multiple_datasets(m, {"a": batches, "b": batches[:1]}, cfg, tokenizer=_Tok())
    assert calls == [8, 4] and res["a"].corpus_wer == d.corpus_wer and res["b"].corpus_wer is not None
