"""Host logic of greedy decoding that needs no GPU: the decoding-prefix finder on the reference dataset's own rows
(tests/golden/ref_dataset.json) and the evaluator's opt-in greedy mode with a stub model."""
import json
from pathlib import Path

import pytest
import torch

from whisper_finetune.eval import evaluator
from whisper_finetune.eval.utils import decode_prefix_len

_DS = json.loads((Path(__file__).parent / "golden" / "ref_dataset.json").read_text())
SOT, SOT_PREV, NO_TS, NO_SPEECH, TRANSCRIBE = 50258, 50361, 50363, 50362, 50359


def test_prefix_finder_on_every_reference_row():
    """All 31 recorded rows (prompted and unprompted, with and without notimestamps).  Expected value from the row's OWN targets:
    the writer masks all of the prompt but its last token with -100 (_construct_decoder_output), so the prompt length is the
    number of -100 targets + 1, and the specials are sot, language, task (+ notimestamps)."""
    runs = _DS["runs"]
    assert len(runs) == 31
    seen = set()
    for r in runs:
        y_in, y_out = r["y_in"], r["y_out"]
        n_prompt = 0 if y_in[0] == SOT else sum(t == -100 for t in y_out) + 1
        assert y_in[n_prompt] == SOT and y_in[n_prompt + 2] == TRANSCRIBE
        no_ts = y_in[n_prompt + 3] == NO_TS if len(y_in) > n_prompt + 3 else False
        kw = r["kw"]
        if kw.get("no_timestamp_training") or kw.get("no_timestamps_rate") == 1.0:
            assert no_ts
        if not kw.get("no_timestamp_training") and kw.get("no_timestamps_rate") == 0.0:
            assert not no_ts
        n = decode_prefix_len(y_in, SOT, NO_TS)
        assert n == n_prompt + 3 + int(no_ts), (n, n_prompt, no_ts)
        assert NO_SPEECH not in y_in[n_prompt:n]
        # what follows the prefix is what the targets ask for next (the prefix's last target is the first thing to generate)
        assert y_out[n - 1] != -100
        seen.add((n_prompt > 0, no_ts))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}, seen


def test_prefix_finder_edge_cases():
    assert decode_prefix_len([SOT, 50261, TRANSCRIBE, NO_TS, NO_SPEECH], SOT, NO_TS) == 4  # the no_speech marker is not part of it
    assert decode_prefix_len([SOT, 50261, TRANSCRIBE], SOT, NO_TS) == 3
    assert decode_prefix_len([SOT_PREV, 5, 6, SOT, 50261, TRANSCRIBE, 50364, 9], SOT, NO_TS) == 6
    with pytest.raises(ValueError):
        decode_prefix_len([1, 2, 3], SOT, NO_TS)
    with pytest.raises(ValueError):
        decode_prefix_len([SOT, 50261], SOT, NO_TS)


class _Tok:
    """Duck-typed tokenizer: ids 0..25 -> letters, 26 -> blank; specials 90.."""
    special_tokens = {"<|sot|>": 90, "<|eot|>": 91, "<|de|>": 92, "<|transcribe|>": 93, "<|notimestamps|>": 94}
    sot, eot, no_timestamps = 90, 91, 94

    def decode(self, ids):
        return "".join(" " if i == 26 else chr(97 + i % 26) for i in ids)

    def encode(self, text):
        return [26 if c == " " else ord(c) - 97 for c in text]


class _Stub(torch.nn.Module):
    """Teacher-forced logits that always predict the target; greedy_decode returns fixed ids behind each row's prefix."""
    V = 100

    def __init__(self, decoded):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.decoded = decoded
        self.calls = []

    def forward(self, x, y_in):
        lg = torch.zeros(y_in.shape[0], y_in.shape[1], self.V)
        nxt = torch.cat([y_in[:, 1:], torch.full((y_in.shape[0], 1), 91)], 1)
        return lg.scatter(2, nxt[..., None], 8.0)

    def greedy_decode(self, mel, prompt, prompt_len, *, eot, max_len=None, suppress=(), suppress_first=(), sync_every=8):
        self.calls.append(dict(prompt=prompt.clone(), prompt_len=torch.as_tensor(prompt_len).clone(), eot=eot, suppress=list(suppress),
                               suppress_first=list(suppress_first)))
        B = prompt.shape[0]
        rows = [prompt[b, :int(prompt_len[b])].tolist() + self.decoded[b] + [eot] for b in range(B)]
        L = max(len(r) for r in rows)
        tokens = torch.tensor([r + [eot] * (L - len(r)) for r in rows])
        return tokens, torch.tensor([len(r) for r in rows]), torch.zeros(B)


def _batch():
    # row 0: unprompted; row 1: prompted (a text prompt before sot); both "ab cd" + eot as targets
    text = [0, 1, 26, 2, 3]
    y_in = torch.tensor([[90, 92, 93, 94] + text + [91, 91, 91],
                         [7, 8, 9, 90, 92, 93, 94] + text])
    y_out = torch.tensor([[92, 93, 94] + text + [91, -100, -100, -100],
                          [-100, -100, 90, 92, 93, 94] + text + [91]])
    return torch.zeros(2, 80, 20), y_in, y_out


def test_evaluator_greedy_mode_takes_text_from_decoded_ids():
    cfg = {"mixed_precision_training": False}
    stub = _Stub([[0, 1, 26, 2, 3], [0, 1, 26, 4, 5, 26, 6]])  # row 0 right ("ab cd"), row 1 "ab ef g": 1 word substituted + 1 inserted
    base = evaluator.evaluate_single_dataset(stub, [_batch()], "syn", cfg, tokenizer=_Tok())
    assert not stub.calls  # default: teacher-forced, greedy_decode is never called
    # (teacher-forced: row 1's argmax over its prompt positions echoes prompt text in front of the transcript: "ijab cd", 1 of 2 words)
    assert base.wer == pytest.approx(0.25)
    got = evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode="greedy"), tokenizer=_Tok())
    assert len(stub.calls) == 1
    call = stub.calls[0]
    assert call["prompt_len"].tolist() == [4, 7] and call["eot"] == 91
    assert call["prompt"][0, :4].tolist() == [90, 92, 93, 94] and call["prompt"][1].tolist() == [7, 8, 9, 90, 92, 93, 94]
    assert call["suppress"] == [90, 92, 93, 94] and call["suppress_first"] == [91, 26]
    # prediction text and WER follow the decoded ids ...
    assert got.num_samples == 2
    assert got.wer == pytest.approx((0.0 + 1.0) / 2)  # row 1: "ab ef g" vs "ab cd" = 1 substitution + 1 insertion over 2 words
    assert got.cer > 0
    # ... the teacher-forced token metrics do not move
    for key in ("mean_token_nll", "avg_log_prob", "mean_token_entropy", "ece"):
        assert getattr(got, key) == getattr(base, key), key
    with pytest.raises(ValueError):
        evaluator.evaluate_single_dataset(stub, [_batch()], "syn", dict(cfg, wft_eval_decode="beam"), tokenizer=_Tok())


def test_greedy_mode_needs_a_decoding_model():
    class NoDecode(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x, y_in):
            return torch.zeros(y_in.shape[0], y_in.shape[1], 100)

    with pytest.raises(RuntimeError, match="greedy_decode"):
        evaluator.evaluate_single_dataset(NoDecode(), [_batch()], "syn", {"mixed_precision_training": False, "wft_eval_decode": "greedy"},
                                          tokenizer=_Tok())
