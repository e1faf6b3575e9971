"""Host side of the decode files (csrc/decode_attn.hip dec_nsplit / dec_workspace_bytes / dec_check, csrc/decode_pick.hip
pick_launch, csrc/decode_beam.hip topk_check / wft_beam_update): every workspace query answers what the recorded table says
(tests/golden/decode_args.json, written by tools/dev/record_decode_args.py from the library before decode.hip was split), and a
call the argument checks refuse returns the status and the message it always had, before any device call.  No GPU needed: only
refusals are called, on placeholder pointers and a null stream."""
import json

import pytest

from tests import _decode_args_cases as cases
from tests.conftest import GOLDEN
from whisper_finetune.engine import lib as L

TABLE = json.loads((GOLDEN / "decode_args.json").read_text())
REFUSALS = cases.refusal_cases()
ENTRY_POINTS = ("wft_attn_decode_bf16", "wft_attn_decode_beam_bf16", "wft_decode_embed", "wft_decode_pick", "wft_decode_pick_ts",
                "wft_decode_sample", "wft_decode_sample_ts", "wft_decode_topk", "wft_decode_topk_ts", "wft_beam_update")


def test_workspace_queries_answer_as_recorded():
    h = L.load()
    case_list, table = cases.workspace_cases(), TABLE["workspace"]
    assert len(table) == len(case_list)
    for case, want in zip(case_list, table):
        got = cases.workspace_bytes(h, case)
        assert got == want, f"(rows, heads, Tk, self form, group) = {case}: library answers {got}, table says {want}"


def test_workspace_rule_by_hand():
    """nsplit = min(ceil(256 / pairs), ceil(Tk / 512), 16) with pairs = rows * H (self form) or rows / group * H (cross form);
    bytes = rows * H * nsplit * 66 * 4 when nsplit > 1, else 0."""
    h = L.load()
    ask = lambda *c: cases.workspace_bytes(h, c)  # noqa: E731
    assert ask(1, 20, 1500, False, None) == ask(1, 20, 1500, False, 1) == 15840  # ceil(256 / 20) = 13, 3 splits of 1 500 keys
    assert ask(5, 20, 1500, False, 5) == 79200  # one group of 5: 20 pairs, 3 splits for each of the 5 * 20 rows
    for rows, group in ((1, None), (1, 1), (5, 5), (40, 8), (257, 1)):
        for form in (False, True) if group in (None, 1) else (False,):
            assert ask(rows, 6, 448, form, group) == 0 and ask(rows, 20, 448, form, group) == 0  # never split below 512 keys


def test_workspace_queries_that_answer_zero():
    h = L.load()
    assert h.wft_attn_decode_workspace_bytes(None) == 0 and h.wft_attn_decode_beam_workspace_bytes(None) == 0
    ask = lambda *c: cases.workspace_bytes(h, c)  # noqa: E731
    assert ask(1, 6, 8192, False, 1) > 0 and ask(1, 6, 8192, True, 1) > 0 and ask(8, 6, 8192, False, 8) > 0
    assert ask(9, 6, 8192, False, 9) == 0  # group 9
    assert ask(8, 6, 8192, False, 3) == 0 and ask(1, 6, 8192, False, 5) == 0  # a group that does not divide the rows
    assert ask(8, 6, 8192, True, 8) == 0 and ask(30, 6, 8192, True, 3) == 0  # the self form takes group = 1


def test_the_refusal_table_covers_every_entry_point():
    assert len(TABLE["refusals"]) == len(REFUSALS)
    assert {c[0] for c in REFUSALS} == set(ENTRY_POINTS)
    assert all(rc == -1 and msg.startswith(c[0] + ": ") for c, (rc, msg) in zip(REFUSALS, TABLE["refusals"]))


@pytest.mark.parametrize("i", range(len(REFUSALS)), ids=[f"{c[0][4:]}-{i}" for i, c in enumerate(REFUSALS)])
def test_refusals_come_before_any_device_call(i):
    """Placeholder pointers and a null stream: a launch would fault, and without a GPU there is no device to launch on."""
    assert cases.refusal(L.load(), cases.refusal_cases()[i]) == TABLE["refusals"][i]
