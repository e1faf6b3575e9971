"""Record a library's answers to the attention dispatch queries as tests/golden/attn_dispatch_256cu.json, the table that
tests/test_attn_dispatch_host.py holds the current library to.  The table is the record of a KNOWN-GOOD library: before a change
to the host side of attention, build the parent commit in a scratch worktree and point WFT_LIB at it (the commands are in
tools/dev/record_gemm_dispatch.py).  Answers only, in the order of the case generator (tests/_attn_dispatch_cases.py);
re-record after a deliberate change of the cases or of a threshold."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "whisper-finetune_amd"), str(ROOT)]

from tests import _attn_dispatch_cases as cases  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

h = L.load()
ans = cases.all_answers(h)
doc = {"library": h.wft_version().decode(), "cases": len(ans),
       "columns": ["fwd_variant", "dq_variant", "dkdv_variant", "colsum_workspace_bytes"], "answers": [v for row in ans for v in row]}
out = ROOT / "tests" / "golden" / "attn_dispatch_256cu.json"
out.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
print(f"{out}: {doc['cases']} cases from {L.LIB_PATH}, {out.stat().st_size} bytes; {len(set(tuple(r[:3]) for r in ans))} distinct kernel triples")
