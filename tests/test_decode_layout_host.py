"""The layout of engine/decode/ and engine/gemm_mode.py: every module imports on its own from a fresh interpreter, `ops` does not pull
the decoding stack in, the package front re-exports every name as the identical object of its home module, and the GEMM modes entered
through the front are the ones `gemm_mode` (and so `ops.linear`) reads."""
import importlib
import subprocess
import sys
from pathlib import Path

from whisper_finetune.engine import decode as D
from whisper_finetune.engine import gemm_mode

ROOT = Path(__file__).resolve().parents[1]
SUBMODULES = ("cache", "runner", "greedy", "beam", "sample", "fallback", "words")

# the frozen surface: home module -> the names the front re-exports from it
SURFACE = {
    "gemm_mode": ("WEIGHT_MODES", "DECODE_WEIGHTS", "step_weights", "stream_gemm_active", "stream_gemm_weights", "stream_gemm",
                  "int8_gemm_active", "int8_gemm"),
    "cache": ("BF16", "_Cache", "KVCache", "_mask", "check_ts_rules", "ts_extra"),
    "runner": ("MAX_SESSIONS", "_SESSIONS", "_BEAM_SESSIONS", "_SAMPLE_SESSIONS", "_groups", "_GraphSession", "_session", "sessions",
               "beam_sessions", "sample_sessions", "release_graphs", "STEP_MODES", "_check_mode", "encode", "_decode"),
    "greedy": ("prefill", "step", "pick", "_greedy_body", "greedy_decode"),
    "beam": ("MAX_BEAM", "beam_candidates", "_check_live_columns", "BeamCache", "beam_prefill", "beam_step", "beam_topk", "beam_update",
             "_beam_first", "_beam_body", "beam_rank", "beam_score", "beam_finalize", "beam_decode"),
    # (`_generated_n` counts the tokens of a sampled row for sample_decode alone, so it lives below it: fallback.py builds on sample.py)
    "sample": ("SampleCache", "sample_pick", "_sample_body", "sample_seeds", "_check_sampling", "sample_decode", "_generated_n"),
    "fallback": ("no_speech_prob", "UPSTREAM_TEMPERATURES", "needs_fallback", "avg_logprob", "compression_ratio", "generated_ids",
                 "decode_with_fallback", "timestamp_segments"),
    "words": ("TOKENS_PER_SECOND", "PREPEND_PUNCTUATIONS", "APPEND_PUNCTUATIONS", "SENTENCE_END_MARKS", "dump_alignment_heads",
              "parse_alignment_heads", "AlignCapture", "alignment_capture", "capture_alignment", "alignment_words", "merge_punctuations",
              "add_word_timestamps", "word_anomaly_score", "is_segment_anomaly", "alignment_slots", "find_alignment"),
}

CHILD = """
import importlib, sys
for p in {paths!r}:
    sys.path.insert(0, p)
entries = {entries!r}
for entry in entries:
    for key in [k for k in sys.modules if k.startswith("whisper_finetune")]:
        del sys.modules[key]
    importlib.import_module(entry)
    if entry == "whisper_finetune.engine.ops":
        pulled = sorted(k for k in sys.modules if k.startswith("whisper_finetune.engine.decode"))
        assert not pulled, pulled
    print("imported", entry)
"""


def test_every_module_imports_alone_and_ops_stays_clear_of_decode():
    entries = ["whisper_finetune.engine." + n for n in ("ops", "decode", "whisper_model", "transcribe")]
    entries += ["whisper_finetune.engine.decode." + n for n in SUBMODULES]
    code = CHILD.format(paths=[str(ROOT / "whisper-finetune_amd"), str(ROOT)], entries=entries)
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split() == [w for e in entries for w in ("imported", e)]


def test_front_reexports_the_identical_objects():
    for home, names in SURFACE.items():
        mod = gemm_mode if home == "gemm_mode" else importlib.import_module("whisper_finetune.engine.decode." + home)
        for name in names:
            assert getattr(D, name) is getattr(mod, name), (home, name)
    assert D.beam_step is D.step
    assert D._SESSIONS is not D._BEAM_SESSIONS and D._SESSIONS is not D._SAMPLE_SESSIONS and D._BEAM_SESSIONS is not D._SAMPLE_SESSIONS
    assert set(SUBMODULES) == {p.stem for p in Path(D.__file__).parent.glob("*.py")} - {"__init__"}


def test_modes_entered_through_the_front_are_read_by_gemm_mode():
    from whisper_finetune.engine.gemm_mode import int8_gemm_active, stream_gemm_active, stream_gemm_weights

    assert (stream_gemm_active(), stream_gemm_weights(), int8_gemm_active()) == (False, "bf16", False)
    with D.stream_gemm(True, "int8"):
        assert stream_gemm_active() and stream_gemm_weights() == "int8" and not int8_gemm_active()
        with D.int8_gemm():
            assert int8_gemm_active() and stream_gemm_active()
            with D.stream_gemm(False):
                assert not stream_gemm_active() and stream_gemm_weights() == "bf16" and int8_gemm_active()
            assert stream_gemm_active() and stream_gemm_weights() == "int8"
        assert not int8_gemm_active()
    assert (stream_gemm_active(), stream_gemm_weights(), int8_gemm_active()) == (False, "bf16", False)
