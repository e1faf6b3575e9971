"""Record a library's answers to the decode host-side cases as tests/golden/decode_args.json, the table that
tests/test_decode_args_host.py holds the current library to: the workspace queries of single-token attention and the status and
message of every refused call (tests/_decode_args_cases.py).  The table is the record of a KNOWN-GOOD library: before a change
to the host side of the decode files, build the parent commit in a scratch worktree and point WFT_LIB at it (the commands are in
tools/dev/record_gemm_dispatch.py).  Runs without a GPU; re-record after a deliberate change of the cases, a rule or a message."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "whisper-finetune_amd"), str(ROOT)]

from tests import _decode_args_cases as cases  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

h = L.load()
doc = {"library": h.wft_version().decode(), **cases.all_answers(h)}
served = [c[0] for c, (rc, _) in zip(cases.refusal_cases(), doc["refusals"]) if rc != -1]
assert not served, f"not refused, so not a case for a table that must never launch: {served}"
out = ROOT / "tests" / "golden" / "decode_args.json"
out.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
print(f"{out}: {len(doc['workspace'])} workspace answers ({len(set(doc['workspace']))} distinct) and {len(doc['refusals'])} refusals "
      f"({len(set(m.split(': ', 1)[1] for _, m in doc['refusals']))} distinct wordings) from {L.LIB_PATH}, {out.stat().st_size} bytes")
