"""Record a library's answers to the GEMM dispatch queries as tests/golden/gemm_dispatch_256cu.json, the table that
tests/test_gemm_dispatch_host.py holds the current library to.

The table is the record of a KNOWN-GOOD library, so point WFT_LIB at one: before a change to the host side of the GEMMs, build
the parent commit in a scratch worktree and record from there,

    git worktree add /tmp/wft_parent HEAD~1 && make -C /tmp/wft_parent/whisper-finetune_amd/csrc
    WFT_LIB=/tmp/wft_parent/whisper-finetune_amd/libwft.so python tools/dev/record_gemm_dispatch.py

Run it without a GPU (or on a 256-CU chip): the plans read the CU count.  Answers only, in the order of the case generator
(tests/_gemm_dispatch_cases.py), with the case counts; re-record after a deliberate change of the cases or of a threshold."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (str(ROOT / "whisper-finetune_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import _gemm_dispatch_cases as cases  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402


def main():
    h = L.load()
    ans = cases.all_answers(h)
    doc = {"library": h.wft_version().decode(), "nt_cases": len(ans["nt"]), "tn_cases": len(ans["tn"]),
           "nt_columns": ["variant", "aux8_bytes", "colsum_workspace_bytes", "splitk_workspace_bytes"],
           "tn_columns": ["segments_ok", "workspace_bytes", "variant_no_workspace", "variant_with_workspace"],
           "nt": [v for row in ans["nt"] for v in row], "tn": [v for row in ans["tn"] for v in row]}
    out = ROOT / "tests" / "golden" / "gemm_dispatch_256cu.json"
    out.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    print(f"{out}: {doc['nt_cases']} NT and {doc['tn_cases']} TN cases from {L.LIB_PATH}, {out.stat().st_size} bytes; "
          f"{len(set(map(tuple, ans['nt'])))} distinct NT answers, "
          f"{len(set((r[2], r[3], r[1] // (4 * c[0] * c[1]) if r[1] else 0) for r, c in zip(ans['tn'], cases.tn_cases())))} distinct TN (variants, splits)")


if __name__ == "__main__":
    main()
