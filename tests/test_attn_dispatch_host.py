"""Host side of the attention library (csrc/attn.hip attn_plan / attn_check): every dispatch and workspace query answers what the
recorded table says (tests/golden/attn_dispatch_256cu.json, written by tools/dev/record_attn_dispatch.py from the library before
the queries and launches were derived from one plan), and a call the argument check refuses returns an error with the message it
always had before any device call.  No GPU needed: only refusals are called, on placeholder pointers and a null stream."""
import ctypes
import json

import pytest

from tests import _attn_dispatch_cases as cases
from tests.conftest import GOLDEN
from whisper_finetune.engine import lib as L

FWD_ALIGN = "q/k/v/o need 16-byte aligned bases and strides that are multiples of 8"
BWD_ALIGN = "tensors need 16-byte aligned bases and strides that are multiples of 8"


def test_queries_answer_as_recorded():
    h = L.load()
    doc = json.loads((GOLDEN / "attn_dispatch_256cu.json").read_text())
    case_list, table = cases.cases(), doc["answers"]
    assert doc["cases"] == len(case_list) and len(table) == 4 * len(case_list)
    for i, case in enumerate(case_list):
        got, want = cases.answers(h, case), table[4 * i:4 * i + 4]
        assert got == want, f"case {i} {case}: library answers {got}, table says {want}"


def test_boundary_shapes_take_the_kernels_they_were_measured_for():
    """The thresholds written out (the table holds them too): pipelined forward from 512 keys, one-wave-per-SIMD dQ from 512 queries
    and dK/dV from 128 queries, non-causal only; variant bits 0 / 1 / 2 and buffer offsets past 31 bits switch them off; the
    column-sum workspace is one row per 32 queries and per 32 keys of every batch entry plus two 32-row middle stages."""
    h = L.load()
    ask = lambda *c: cases.answers(h, c)  # noqa: E731
    assert ask(511, 511, 0, 2, 8)[:3] == [1, 8, 4]
    assert ask(512, 512, 0, 2, 8)[:3] == [2, 4, 4]
    assert ask(127, 512, 0, 2, 8)[:3] == [2, 8, 8]
    assert ask(128, 511, 0, 2, 8)[:3] == [1, 8, 4]
    assert ask(1500, 1500, 1, 2, 8)[:3] == [1, 8, 8]
    assert ask(1500, 1500, 0, 2, 8, 7)[:3] == [1, 8, 8]
    assert ask(1500, 1500, 0, 2, 8, 0, 0, 0, {"ldk": cases.LD_FITS})[:3] == [2, 4, 4]
    assert ask(1500, 1500, 0, 2, 8, 0, 0, 0, {"ldk": cases.LD_TOO_LARGE})[:3] == [2, 8, 8]
    assert ask(33, 129, 0, 3, 6)[3] == (3 * 2 + 3 * 5 + 2 * 32) * 6 * 64 * 4
    assert h.wft_attn_variant(None, 0) == -1 and h.wft_attn_variant(ctypes.byref(cases.attn_args(64, 64, 0, 2, 8)), 3) == -1
    assert h.wft_attn_bwd_colsum_workspace_bytes(None) == 0


def _null(field):
    return lambda a: setattr(a, field, None)


def _set(field, value):
    return lambda a: setattr(a, field, value)


def _colsums(*fields):
    def edit(a):
        for f in fields:
            setattr(a, f, cases.PTR)
    return edit


# (entry point, edit that makes a servable call refusable, wording of the refusal)
REFUSALS = [
    ("wft_attn_fwd_bf16", _null("lse"), "null pointer"),
    ("wft_attn_bwd_bf16", _null("delta"), "null pointer"),
    ("wft_attn_bwd_bf16", _null("q"), "null pointer"),
    ("wft_attn_fwd_bf16", _set("Tk", 0), "bad shape"),
    ("wft_attn_bwd_bf16", _set("H", 0), "bad shape"),
    ("wft_attn_fwd_bf16", _set("v", cases.PTR + 8), FWD_ALIGN),
    ("wft_attn_bwd_bf16", _set("o", cases.PTR + 2), BWD_ALIGN),
    ("wft_attn_bwd_bf16", _set("dk", cases.PTR + 8), BWD_ALIGN),
    ("wft_attn_fwd_bf16", _set("ldk", 516), FWD_ALIGN),
    ("wft_attn_fwd_bf16", _set("o_bs", 64 * 512 + 4), FWD_ALIGN),
    ("wft_attn_bwd_bf16", _set("ldq", 516), BWD_ALIGN),
    ("wft_attn_bwd_bf16", _set("lddo", 513), BWD_ALIGN),
    ("wft_attn_bwd_bf16", _set("dv_bs", 64 * 512 + 4), BWD_ALIGN),
    ("wft_attn_fwd_bf16", _set("causal", 1), "causal attention needs Tq == Tk"),
    ("wft_attn_bwd_bf16", _set("causal", 1), "causal attention needs Tq == Tk"),
    ("wft_attn_bwd_bf16", _set("scale", 0.0), "scale must be positive (the row constants are -lse / scale)"),
    ("wft_attn_bwd_bf16", _set("scale", -0.125), "scale must be positive (the row constants are -lse / scale)"),
    ("wft_attn_bwd_bf16", _colsums("dq_colsum", "dv_colsum"), "dq_colsum, dv_colsum and colsum_ws go together"),
    ("wft_attn_bwd_bf16", _colsums("dq_colsum", "colsum_ws"), "dq_colsum, dv_colsum and colsum_ws go together"),
    ("wft_attn_bwd_bf16", _colsums("dv_colsum", "colsum_ws"), "dq_colsum, dv_colsum and colsum_ws go together"),
]


@pytest.mark.parametrize("entry,edit,wording", REFUSALS, ids=[f"{e[9:12]}-{i}" for i, (e, _, _) in enumerate(REFUSALS)])
def test_refusals_come_before_any_device_call(entry, edit, wording):
    """Placeholder pointers and a null stream: a launch would fault, and without a GPU there is no device to launch on."""
    h = L.load()
    a = cases.attn_args(64, 128, 0, 2, 8)
    edit(a)
    rc = getattr(h, entry)(ctypes.byref(a), None)
    assert rc == -1
    msg = h.wft_last_error().decode()
    assert msg.startswith(f"{entry}: {wording} ("), msg


def test_a_null_argument_block_is_refused():
    h = L.load()
    for entry in ("wft_attn_fwd_bf16", "wft_attn_bwd_bf16"):
        assert getattr(h, entry)(None, None) == -1
        assert h.wft_last_error().decode().startswith(f"{entry}: null pointer (")
