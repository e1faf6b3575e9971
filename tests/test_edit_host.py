"""Edit counts on the host: the two references of tests/_edit_cases.py against each other and against eval/metrics.py, the mutants the
comparison has to reject, the new dataclass fields, the corpus totals and the evaluator on a CPU model."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import _edit_cases as EC
from tests.test_eval import _Tok
from whisper_finetune.eval import evaluator
from whisper_finetune.eval import metrics as M


def test_references_agree_and_hold_the_identities():
    """Plain-Python table == numpy anti-diagonals == metrics.edit_counts_host on the exhaustive set, the symbol values and the seam
    sample; S + D + I is the Levenshtein distance of metrics._edit_distance; H + S + D = n and H + S + I = m."""
    for batch in EC.host_case_set():
        want = EC.expected(batch)
        assert want.shape == (len(batch), 4)
        for p in range(len(batch)):
            r, h = batch.pair(p)
            r, h = r.tolist(), h.tolist()
            H, S, D, I = (int(v) for v in want[p])
            assert EC.counts_table(r, h) == EC.counts_diagonals(r, h) == M.edit_counts_host(r, h) == (H, S, D, I), (batch.name, p)
            assert S + D + I == M._edit_distance(r, h), (batch.name, p)
        n, m = batch.rows[:, 2], batch.rows[:, 3]
        assert np.array_equal(want[:, 0] + want[:, 1] + want[:, 2], n) and np.array_equal(want[:, 0] + want[:, 1] + want[:, 3], m)
        assert (want >= 0).all()


def test_the_exhaustive_set_separates_the_priorities():
    """The issue's count: over {0, 1, 2} up to length 4, 24 pairs tell deletion-before-insertion from insertion-before-deletion,
    (0, 1, 0) against (1, 2, 0, 1) among them; (0, 1) against (1, 0) separates diagonal-first from the rest."""
    batch = EC.exhaustive()
    assert len(batch) == 14641
    swapped = EC.run_mutant("deletion_insertion_priority_swapped", batch)
    diff = EC.mismatches(swapped, EC.expected(batch))
    assert diff.shape[0] == 24
    pairs = [tuple(x.tolist() for x in batch.pair(p)) for p in diff]
    assert ([0, 1, 0], [1, 2, 0, 1]) in pairs
    assert EC.counts_table([0, 1], [1, 0]) == (0, 2, 0, 0)
    assert EC.MUTANTS["deletion_before_diagonal"]([0, 1, 1, 0], (0, 2, 2, 2)) != (0, 2, 0, 0)
    assert EC.MUTANTS["insertion_before_diagonal"]([0, 1, 1, 0], (0, 2, 2, 2)) != (0, 2, 0, 0)


@pytest.mark.parametrize("name", sorted(EC.MUTANTS))
def test_the_comparison_rejects_every_mutant(name):
    """Each faulty variant of the rule differs from the reference somewhere on the case set — with the comparison the GPU tests use."""
    for batch in EC.host_case_set():
        want = EC.expected(batch)
        for p0 in range(0, len(batch), 2000):
            part = EC.Batch(batch.name, batch.sym, batch.rows[p0:p0 + 2000])
            if EC.mismatches(EC.run_mutant(name, part), want[p0:p0 + 2000]).shape[0]:
                return
    raise AssertionError(f"no case tells the mutant {name} from the rule")


def test_the_unmutated_table_passes_the_comparison():
    for batch in (EC.symbol_values(), EC.seams(256, sample=True)):
        got = np.array([EC._mutant_table(batch.sym.tolist(), row) for row in batch.rows])
        assert EC.mismatches(got, EC.expected(batch)).shape[0] == 0


def test_binding_mirrors_the_row_struct():
    import ctypes

    from whisper_finetune.engine import kernels as K
    from whisper_finetune.engine import lib as L

    assert ctypes.sizeof(L.EditRow) == 32 == K.EDIT_ROW_DTYPE.itemsize
    for name in ("ref_off", "hyp_off", "ref_len", "hyp_len", "reserved"):
        assert getattr(L.EditRow, name).offset == K.EDIT_ROW_DTYPE.fields[name][1], name
    lib = L.load()  # pure host functions: callable without a GPU
    assert lib.wft_edit_max_len() == K.EDIT_MAX_LEN == 4096 and lib.wft_edit_threads() >= 64
    rec, max_len = K.edit_rows([(0, 3, 3, 2), (5, 5, 0, 0)], 6)
    assert max_len == 3 and rec["hyp_off"].tolist() == [3, 5] and rec.view("u1").shape == (64,)
    for rows, kw in (([(0, 4, 3, 3)], {}), ([(0, 0, 7, 1)], {}), ([(0, 0, 2, 2)], dict(max_len=1)), ([(0, 0, 2, 2)], dict(max_len=4097))):
        with pytest.raises(ValueError):
            K.edit_rows(rows, 6, **kw)


def test_new_dataclass_fields_stand_behind_the_old_ones():
    pu = [f.name for f in dataclasses.fields(M.PerUtteranceMetrics)]
    assert pu == ["prediction", "reference", "wer", "cer", "token_nll", "avg_log_prob", "token_entropy", "token_confidences", "token_correct",
                  "word_counts", "char_counts"]
    ds = [f.name for f in dataclasses.fields(M.DatasetMetrics)]
    assert ds == ["dataset_name", "num_samples", "wer", "cer", "mean_token_nll", "avg_log_prob", "mean_token_entropy", "ece", "per_utterance",
                  "corpus_wer", "corpus_cer", "word_sub_rate", "word_del_rate", "word_ins_rate"]
    # the positional constructions of tests/test_eval.py and of aggregate_dataset_metrics' empty case
    u = M.PerUtteranceMetrics("a", "a", 0.0, 0.0, 1.0, -1.0, 0.5, [0.9, 0.8], [True, False])
    assert u.word_counts is None and u.char_counts is None and u.token_correct == [True, False]
    d = M.DatasetMetrics("none", 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, [])
    assert all(getattr(d, k) is None for k in ds[9:]) and d.per_utterance == []
    assert set(M.compute_macro_average([d])) == {"macro_wer", "macro_cer", "macro_mean_token_nll", "macro_avg_log_prob",
                                                 "macro_mean_token_entropy", "macro_ece"}


def _utt(ref, word=None, char=None):
    return M.PerUtteranceMetrics("x", ref, 0.5, 0.25, 1.0, -1.0, 0.5, [0.5], [True], word_counts=word, char_counts=char)


def test_aggregate_totals_on_a_hand_written_table():
    #            H  S  D  I          H   S  D  I
    table = [((3, 1, 0, 0), (17, 2, 0, 1)),    # 4 reference words, 19 characters
             ((0, 0, 2, 0), (0, 0, 9, 0)),     # 2 words, all deleted
             ((5, 0, 1, 3), (30, 1, 4, 12)),   # 6 words, three insertions
             ((1, 0, 0, 0), (5, 0, 0, 0))]     # 1 word, correct
    d = M.aggregate_dataset_metrics([_utt("r", w, c) for w, c in table], "ds")
    assert d.corpus_wer == (1 + 2 + 1 + 3) / 13 and d.word_sub_rate == 1 / 13 and d.word_del_rate == 3 / 13 and d.word_ins_rate == 3 / 13
    assert d.corpus_cer == (3 + 9 + 17) / (19 + 9 + 35 + 5)
    assert abs(d.corpus_wer - (d.word_sub_rate + d.word_del_rate + d.word_ins_rate)) < 1e-15
    assert d.wer == 0.5 and d.cer == 0.25 and d.num_samples == 4  # the means of the per-utterance rates are what they were
    # an utterance with an empty reference has nothing to count: it stays out of the totals
    e = M.aggregate_dataset_metrics([_utt("r", w, c) for w, c in table] + [_utt("")], "ds")
    assert (e.corpus_wer, e.corpus_cer, e.word_ins_rate) == (d.corpus_wer, d.corpus_cer, d.word_ins_rate) and e.num_samples == 5
    # any other utterance without counts: no corpus rate can be given
    f = M.aggregate_dataset_metrics([_utt("r", w, c) for w, c in table] + [_utt("r s")], "ds")
    assert (f.corpus_wer, f.corpus_cer, f.word_sub_rate, f.word_del_rate, f.word_ins_rate) == (None,) * 5
    g = M.aggregate_dataset_metrics([_utt("r", w, None) for w, c in table], "ds")   # word counts only
    assert g.corpus_wer == d.corpus_wer and g.corpus_cer is None
    assert M.aggregate_dataset_metrics([], "none").corpus_wer is None


def test_batch_and_string_forms_on_the_host():
    refs = ["the cat sat on the mat", "grüße aus köln", "a", "  padded  reference ", "same same"]
    hyps = ["the cat sat mat on the", "grüsse aus köln am rhein", "", "padded reference", "same same"]
    for device in (None, "cpu", torch.device("cpu")):
        w, c = M.word_error_counts(hyps, refs, device), M.char_error_counts(hyps, refs, device)
        assert w.dtype == np.int64 and w.shape == c.shape == (5, 4)
        for k, (r, h) in enumerate(zip(refs, hyps)):
            assert tuple(w[k]) == M.edit_counts_host(r.split(), h.split()) and tuple(c[k]) == M.edit_counts_host(list(r.strip()), list(h.strip()))
            assert (w[k, 1] + w[k, 2] + w[k, 3]) / (w[k, 0] + w[k, 1] + w[k, 2]) == M.wer(r, h)
            assert (c[k, 1] + c[k, 2] + c[k, 3]) / (c[k, 0] + c[k, 1] + c[k, 2]) == M.cer(r, h)
    assert M.edit_counts_batch([], []).shape == (0, 4)
    assert M.edit_counts_batch([[("a", 1), None]], [[None, ("a", 1), 3.5]]).tolist() == [list(M.edit_counts_host([1, 2], [2, 1, 3]))]
    with pytest.raises(ValueError):
        M.edit_counts_batch([[1]], [])


class _CpuModel(torch.nn.Module):
    """A model on the CPU: logits that spell the input row shifted by `k` letters at every third position."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x, y_in):
        B, S = y_in.shape
        ids = (y_in + (torch.arange(S)[None] % 3 == 0)) % 27
        return torch.nn.functional.one_hot(ids, 32).float() * 8 + self.w


def test_evaluator_on_a_cpu_model_fills_the_counts():
    g = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(2):
        y_in = torch.randint(0, 27, (3, 12), generator=g)
        y_out = y_in.clone()
        y_out[0, -3:] = -100
        y_out[2, :] = -100
        batches.append((torch.randn(3, 80, 20, generator=g), y_in, y_out))
    cfg = {"mixed_precision_training": False}
    d = evaluator.evaluate_single_dataset(_CpuModel(), batches, "cpu", cfg, tokenizer=_Tok())
    assert d.num_samples == 4 and any(u.wer > 0 for u in d.per_utterance)
    tw, tc = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    for u in d.per_utterance:
        assert u.wer == M.wer(u.reference, u.prediction) and u.cer == M.cer(u.reference, u.prediction)
        assert u.word_counts == M.edit_counts_host(u.reference.split(), u.prediction.split())
        assert u.char_counts == M.edit_counts_host(list(u.reference.strip()), list(u.prediction.strip()))
        assert all(isinstance(v, int) for v in u.word_counts + u.char_counts)
        tw += u.word_counts
        tc += u.char_counts
    assert d.corpus_wer == int(tw[1:].sum()) / int(tw[:3].sum()) and d.corpus_cer == int(tc[1:].sum()) / int(tc[:3].sum())
    assert (d.word_sub_rate, d.word_del_rate, d.word_ins_rate) == tuple(int(tw[k]) / int(tw[:3].sum()) for k in (1, 2, 3))
    assert d.wer == np.mean([u.wer for u in d.per_utterance])


def test_wandb_log_carries_the_new_numbers_when_present(monkeypatch):
    seen = {}
    monkeypatch.setattr(evaluator.rt, "log", lambda data, step: seen.update(data))
    full = M.aggregate_dataset_metrics([_utt("r", (3, 1, 0, 0), (17, 2, 0, 1))], "a")
    bare = M.aggregate_dataset_metrics([M.PerUtteranceMetrics("b", "c", 1.0, 1.0, 3.0, -3.0, 1.5, [0.4], [False])], "b")
    evaluator.log_metrics_to_wandb({"a": full, "b": bare}, {"macro_wer": 0.5}, step=1)
    for key in ("corpus_wer", "corpus_cer", "word_sub_rate", "word_del_rate", "word_ins_rate"):
        assert seen[f"val/a/{key}"] == getattr(full, key) and f"val/b/{key}" not in seen
    assert seen["val/a/wer"] == 0.5 and seen["val/b/wer"] == 1.0 and seen["val/macro_wer"] == 0.5
