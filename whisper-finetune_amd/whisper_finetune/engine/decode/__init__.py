"""KV-cached greedy and beam-search decoding on the engine's decoder: token ids in, token ids out.

The greedy path of upstream's `whisper.decoding` (`DecodingTask._main_loop` with `GreedyDecoder`, `SuppressTokens`,
`SuppressBlank`, `DecodingOptions(without_timestamps=True)`; greedy.py) and, in beam.py, its `BeamSearchDecoder` +
`MaximumLikelihoodRanker` on a KV cache that the beams of an audio share (`BeamCache`, `beam_decode`); with `timestamp_begin=` both
decode under upstream's `ApplyTimestampRules` (restated in include/wft.h "Timestamp rules"; the pick / top-k kernels apply them,
`timestamp_segments` reads the result).  The third part is sampling (sample.py): `sample_decode` draws `best_of` samples per audio at a
temperature on the device (wft_decode_sample: Gumbel-max over Philox noise, include/wft.h "Sampled decoding") on a cache whose samples
share the prompt keys and the cross keys / values (`SampleCache`), and `decode_with_fallback` (fallback.py) is upstream's temperature ladder of
`transcribe()` (`decode_with_fallback`, `needs_fallback`: average log-probability, compression ratio, no-speech probability).
Upstream's behaviour is restated; parity with its binary and with torch's random stream is unpinned.  No tokenizer; language
detection and the long-audio `transcribe()` loop live in engine/transcribe.py.

The modules, each building only on those before it: cache.py (`KVCache`, the timestamp-rule checks), runner.py (the captured step, the
session tables, the loop every decoder shares), words.py (word-level timestamps: `find_alignment`); greedy.py; beam.py and sample.py;
fallback.py.  The thread-local GEMM modes (`stream_gemm`, `int8_gemm`) live in engine/gemm_mode.py, which `ops` reads.  Every name is
re-exported here, so `from whisper_finetune.engine import decode` serves as it did when this was one file; callers that look a name up
on this package at call time (the evaluator, whisper_model.py) see a replaced attribute, a function of a submodule resolves the names
it calls in its own module.
"""
from ..gemm_mode import (DECODE_WEIGHTS, WEIGHT_MODES, int8_gemm, int8_gemm_active, step_weights, stream_gemm, stream_gemm_active,
                         stream_gemm_weights)
from .beam import (MAX_BEAM, BeamCache, _beam_body, _beam_first, _check_live_columns, beam_candidates, beam_decode, beam_finalize,
                   beam_prefill, beam_rank, beam_score, beam_step, beam_topk, beam_update)
from .cache import BF16, KVCache, _Cache, _mask, check_ts_rules, ts_extra
from .fallback import (UPSTREAM_TEMPERATURES, avg_logprob, compression_ratio, decode_with_fallback, generated_ids, needs_fallback,
                       no_speech_prob, timestamp_segments)
from .greedy import _greedy_body, greedy_decode, pick, prefill, step
from .runner import (_BEAM_SESSIONS, _SAMPLE_SESSIONS, _SESSIONS, MAX_SESSIONS, STEP_MODES, _check_mode, _decode, _GraphSession, _groups,
                     _session, beam_sessions, encode, release_graphs, sample_sessions, sessions)
from .sample import SampleCache, _check_sampling, _generated_n, _sample_body, sample_decode, sample_pick, sample_seeds
from .words import (APPEND_PUNCTUATIONS, PREPEND_PUNCTUATIONS, SENTENCE_END_MARKS, TOKENS_PER_SECOND, AlignCapture, add_word_timestamps,
                    alignment_capture, alignment_slots, alignment_words, capture_alignment, dump_alignment_heads, find_alignment,
                    is_segment_anomaly, merge_punctuations, parse_alignment_heads, word_anomaly_score)
