"""Host side of the GEMM library (csrc/gemm.hip nt_plan / tn_plan, over the per-kernel rules of csrc/gemm_*.hip): every dispatch
and workspace query answers what the recorded table says (tests/golden/gemm_dispatch_256cu.json, written by
tools/dev/record_gemm_dispatch.py from the library before the queries were derived from one plan), and a call the plan refuses
returns an error before any device call.  No GPU needed: without a device the library assumes 256 CUs, which is also what an
MI355X reports."""
import ctypes
import json

from tests import _gemm_dispatch_cases as cases
from tests.conftest import GOLDEN
from whisper_finetune.engine import lib as L


def _first_difference(kind, case_list, ask, table, width=4):
    h = L.load()
    assert len(table) == width * len(case_list), f"{kind}: the table holds {len(table) // width} cases, the generator makes {len(case_list)}"
    for i, case in enumerate(case_list):
        got, want = ask(h, case), table[width * i:width * (i + 1)]
        if got != want:
            return f"{kind} case {i} {case}: library answers {got}, table says {want}"
    return None


def test_nt_queries_answer_as_recorded():
    doc = json.loads((GOLDEN / "gemm_dispatch_256cu.json").read_text())
    case_list = cases.nt_cases()
    assert doc["nt_cases"] == len(case_list)
    assert _first_difference("NT", case_list, cases.nt_answers, doc["nt"]) is None


def test_tn_queries_answer_as_recorded():
    doc = json.loads((GOLDEN / "gemm_dispatch_256cu.json").read_text())
    case_list = cases.tn_cases()
    assert doc["tn_cases"] == len(case_list)
    assert _first_difference("TN", case_list, cases.tn_answers, doc["tn"]) is None


def test_boundary_shapes_take_the_kernels_they_were_measured_for():
    """The shapes at which the launcher changes kernel, with the answers written out (the table holds them too)."""
    h = L.load()
    nt = {c[:3]: cases.nt_answers(h, c) for c in cases.NT_BOUNDARY}
    assert nt[(4224, 1024, 64)] == [128, 0, 0, 0]
    assert nt[(256, 256, 256)] == [128, 0, 0, 0]
    assert nt[(128, 256, 4096)] == [128, 0, 0, 524288]
    assert nt[(300, 128, 128)] == [128, 0, 0, 0]
    assert nt[(4096, 2048, 64)] == [256, 0, 0, 0]
    assert nt[(4096, 2048, 256)] == [4, 0, 0, 0]
    tn = {c[:3]: cases.tn_answers(h, c) for c in cases.TN_BOUNDARY}
    assert tn[(256, 256, 16384)][2:] == [256, 4] and tn[(256, 256, 16384)][1] > 0
    assert tn[(768, 768, 4096)][2:] == [128, 128]


def test_mul_aux8_with_a_bias_is_refused_before_any_device_call():
    """The epilogue that reads the one-byte gelu' buffer adds no bias, so the plan does not serve MUL_AUX8 with one: the size query
    answers 0 and the launcher returns its one-byte-gelu' error from the argument check (the pointers are placeholders: a launch
    would fault, and without a GPU there is no device to launch on)."""
    h = L.load()
    served = cases.nt_args(4096, 2048, 256, "mul_aux8")
    assert h.wft_gemm_nt_aux8_bytes(ctypes.byref(served)) == 16 * 8 * 65536
    a = cases.nt_args(4096, 2048, 256, "mul_aux8")
    a.bias = cases.PTR
    assert h.wft_gemm_nt_aux8_bytes(ctypes.byref(a)) == 0
    rc = h.wft_gemm_nt_bf16(ctypes.byref(a), None)
    assert rc != 0
    msg = h.wft_last_error().decode()
    assert "wft_gemm_nt_bf16" in msg and "one-byte gelu'" in msg, msg
