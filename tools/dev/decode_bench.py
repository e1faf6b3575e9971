"""Measurements behind the greedy-decoding rows of DESIGN.md (large-v3 shapes: H = 20, d = 1280, 32 layers), HIP events, warmed up.

  attn   wft_attn_decode_bf16 against the same work through wft_attn_fwd_bf16 with Tq = 1, causal = 0, Tk = the common length,
         alternating the two in one process (median / min / spread over the rounds), and as achieved bytes/s over the K/V bytes
         the shape needs.  Every arm walks the 32 layers' buffers in rotation, as a decoding step does: a single buffer of a
         small batch would sit in the Infinity Cache and time the cache, not the memory.
  gemm   every wft_gemm_nt_bf16 call of one cached step at M = B: the kernel wft_gemm_nt_variant reports, time, and time over
         (weight bytes / HBM rate) — the price list for a weight-streaming small-M GEMM.  Recorded, not acted on.
  e2e    tokens/s of Whisper.greedy_decode against a loop of model.logits(tokens, xa) re-forwards (same prompts, 64 new tokens).
  gemm_stream  the same seven calls through wft_gemm_nt_stream_bf16 (csrc/gemm_stream.hip) against wft_gemm_nt_bf16 on the same
         arguments, alternating, 32 distinct weight buffers in rotation; max difference of the two outputs at the size timed.
         The table wft_gemm_nt_stream_ok's rule is set from (arm = "stream_vs_nt").  Then the int8 twin (arm = "q8_vs_stream"):
         wft_gemm_nt_stream_q8 on the quantiser's image of the same weights against wft_gemm_nt_stream_bf16, alternating, at the
         large-v3 step shapes (N, K) = (1280, 1280), (3840, 1280), (5120, 1280), (1280, 5120), (51968, 1280): us, spread, ratio, achieved
         weight bytes/s of each — the table wft_gemm_nt_stream_q8_ok's rule is set from (the ceiling is 2x: half the weight bytes).
  e2e_step     greedy_decode's four step arms, alternating: step="eager" (the baseline), eager steps on the streaming GEMMs, the
         captured step on the old GEMMs, step="graph", and step="graph" with weights="int8" (arm = "graph_int8"); tokens/s, ms per
         token, launches per step, share of equal tokens.
         (profiles/decode_bench_q8.jsonl: --parts gemm_stream,e2e_step --batches 1,8,32 --out profiles/decode_bench_q8.jsonl)

  gemm_i8      the W8A8 product of weights="w8a8" (the quantiser pass over the activation + wft_gemm_nt_i8, csrc/gemm_i8.hip) against
         wft_gemm_nt_bf16 on the bf16 shadow, alternating, at the large-v3 encoder / prefill shapes (N, K) = (3840, 1280), (1280, 1280),
         (5120, 1280), (1280, 5120), (2560, 1280) with M = 1500 * B (--batches = B); wft_gemm_nt_i8 alone as a third arm; then
         arm = "e2e": encoder + prefill under weights="bf16" and under "w8a8".  A numerics feature: no speed-up is claimed.
         (profiles/decode_bench_w8a8.jsonl: --parts gemm_i8 --batches 1,8,32 --out profiles/decode_bench_w8a8.jsonl)

  beam   beam search at W = 5 (--batches = audios, e.g. 1,4,6): (i) the self form of wft_attn_decode_beam_bf16 (identity and
         scrambled ancestry table) against wft_attn_decode_bf16 at the same rows and keys — the price of the indirection; (ii) its
         grouped cross form at R = B * W rows against wft_attn_decode_bf16 at R rows on W-times replicated caches: us, K/V bytes,
         achieved TB/s; (iii) wft_decode_topk + wft_beam_update against wft_decode_pick at R rows; (iv) beam_decode(W = 5) against
         greedy_decode at batch = R, eager and graph: tokens/s, ms per step, ratio.

  ts     the timestamp-rule forms of the pick and the top-k (wft_decode_pick_ts, wft_decode_topk_ts) against the plain kernels on the
         same rows, V = 51 866, --batches = rows: histories of 100 sampled tokens ending in text, so every rule-5 pass runs (the
         two arg-best pairs, the two sums, and for top-k the third scan).

  sample the sampled pick (wft_decode_sample, wft_decode_sample_ts at temperature 1) against the greedy pick (wft_decode_pick,
         wft_decode_pick_ts) on the same rows, V = 51 866, R = 5 * B rows (--batches = audios, e.g. 1,4,6 for R = 5, 20, 30): what Philox
         and two logf per column cost beside the 104 KB row read; then sample_decode(best_of = 5) over B audios against
         beam_decode(W = 5) over B audios and greedy_decode at batch 5 * B, eager and graph: tokens/s, ms per step.
         (profiles/decode_bench_sample.jsonl: --parts sample --batches 1,4,6 --out profiles/decode_bench_sample.jsonl)

  align  word-level timestamps at whisper-large-v3 dimensions (10 alignment heads, T = 448 tokens, 1500 frames; --batches = audios,
         e.g. 1,4): the three kernels of csrc/align.hip one by one, Whisper.find_alignment as a whole, beside them a torch-on-GPU
         restatement of stages a and b (softmax, std_mean, unfold + sort) and the host route for DTW (copy the matrix to the host,
         a vectorised numpy wavefront).  What to expect: stage a is bound by its 27 MB per audio of output, stage b reads that once, DTW is latency-bound by N + M - 1 = 1 945 dependent
         wavefront steps per audio.
         (profiles/decode_bench_align.jsonl: --parts align --batches 1,4 --out profiles/decode_bench_align.jsonl)

  transcribe  long-form transcription at whisper-large-v3 dimensions (--batches = recordings, e.g. 4): ragged recordings of seeded
         noise (95 s, 7 s less for each further one), Whisper.transcribe without timestamps (every window advances whole, so the
         number of windows is fixed: 4 per 95 s) at temperature 0 with sample_len = 32 and language detection: wall time, windows/s,
         audio-s/s; beside it the two kernels of csrc/transcribe.hip alone (wft_mel_windows on a full batch with its achieved
         bytes/s, wft_lang_probs on as many rows) and their share of the wall time against the share of decode_with_fallback.
         What to expect: the two kernels are a few MB of copy and a 100-value softmax per iteration — far below one per cent.
         Not measured yet: no figure of this part is recorded under profiles/ or quoted anywhere.
         (--parts transcribe --batches 4 --out profiles/decode_bench_transcribe.jsonl)

  resample  wft_resample_f32 alone (--batches is not used): 48 000 -> 16 000 and 44 100 -> 16 000 on one 10-minute recording and on a
         [32, 30 * rate] batch (what GpuMelLoader resamples per step): ms per call (output buffer preallocated, table cached) and
         the achieved bytes/s against the read-once, write-once byte count 4 * B * (n_in + n_out), the table not counted.
         The kernel should be HBM-bound; no figure is claimed in advance.
         (--parts resample --out profiles/decode_bench_resample.jsonl)

  stretch  the time-stretch augmentation of the loader (--batches is not used): K.time_stretch + K.logmel_ragged against the plain K.logmel
         on [B, 480000] batches of 30 s clips, B = 32 and 96, rates uniform in [0.75, 1.25] (the production range) and all 0.5 (the
         largest workspace): ms per call of each arm, alternating rounds in one process, and the stages of the stretch one by one.
         A side kernel of the loader; no threshold is set.
         (--parts stretch --out profiles/decode_bench_stretch.jsonl)
  filter   the filter augmentation of the loader (--batches is not used): wft_sos_filter_f32 on [32, 480000] and [96, 480000], one and
         four sections, out of place and in place, the K.sos_filter wrapper, and torch's copy of the batch for scale.
         (--parts filter --out profiles/decode_bench_filter.jsonl)
  wavefx   the wave effects of the loader (--batches is not used): every stage of wft_wave_fx_f32 on [32, 480000] and [96, 480000],
         once with every row active and once with the number of rows the default rates make active, beside the log-mel and torch's
         copy of the same batch.  (--parts wavefx --out profiles/decode_bench_wavefx.jsonl)
  rate     the rate effects of the loader (--batches is not used): K.alias, K.sinc_resample_rows and pitch_shift on [32, 480000] and
         [96, 480000] with every row active (alias rates mel-spaced over 8-16 kHz, pitch over -4 .. +4 semitones), beside the log-mel
         and torch's copy of the same batch.  No threshold is set.  (--parts rate --out profiles/decode_bench_rate.jsonl)
  office   the office effects of the loader (--batches is not used): K.fir_conv at P = 1, 2 and 8 partitions (1000, 2000 and 8192 taps)
         and K.bitcrush on [32, 480000] and [96, 480000] with every row active, beside the log-mel, the time stretch's STFT stage
         (comparable FFT work per clip) and torch's copy of the same batch.  No threshold is set.
         (--parts office --out profiles/decode_bench_office.jsonl)
  mix      the mix effects of the loader (--batches is not used): K.loudness (measure only, and normalise in place) and K.bg_mix (snr and
         absolute, in place, over a synthetic bank of four entries) on [32, 480000] and [96, 480000] with every row active, beside
         K.sos_filter at two sections (the same recurrence, with its outputs stored), the log-mel and torch's copy of the same batch.
         No threshold is set.  (--parts mix --out profiles/decode_bench_mix.jsonl)
  pcm      the audio-file decoder (--batches is not used): wft_pcm_decode_f32 on 32 and 96 clips of 30 s, as S16LE stereo at 48 kHz and
         as u-law mono at 8 kHz, beside a device-to-device copy that moves the same number of bytes (in plus out), decode + resample
         beside resample alone, and the host path it replaces (numpy convert + downmix, then the host-to-device copy of f32) as wall
         time.  No threshold is set.  (--parts pcm --out profiles/decode_bench_pcm.jsonl)
  edit     WER / CER scoring (--batches is not used): P = 32 and P = 2 048 utterances of 20, 60 and 90 words; the Python Levenshtein loops
         the evaluator ran per utterance (metrics.wer + metrics.cer, wall time on the host's CPU) beside word_error_counts +
         char_error_counts on the GPU (packing and both copies included) and the wft_edit_counts_i32 launches alone on resident
         tables.  No threshold is set.  (--parts edit --out profiles/decode_bench_edit.jsonl)

  python tools/dev/decode_bench.py [--parts attn,gemm,e2e,gemm_stream,e2e_step,gemm_i8,beam,ts,sample,align,transcribe,resample,stretch,filter,wavefx,rate,office,mix,pcm,edit] [--batches 1,8,32] [--out FILE]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
for p in (str(ROOT / "whisper-finetune_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)

from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402
from whisper_finetune.engine.whisper_model import MODEL_DIMS, Whisper  # noqa: E402

DEV = torch.device("cuda:0")
BF = torch.bfloat16
H, D, LAYERS, CAP, TA = 20, 1280, 32, 448, 1500
HBM = 6.3e12  # achievable HBM rate of the MI355X, bytes/s (8.0e12 on the data sheet)
OUT = []


def emit(rec):
    OUT.append(rec)
    print(json.dumps(rec), flush=True)


def timed(fn, iters):
    """ms per call of fn() over `iters` back-to-back calls between two events (the launches are queued ahead of the GPU where
    the kernel is longer than a launch; where it is not, the figure is the launch rate — said in the table)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def ab(arms, rounds=7, iters=8):
    """arms: {name: fn}; alternating rounds in one process -> {name: (median, min, spread)} in ms; spread = (max - min) / median."""
    for fn in arms.values():
        fn(); fn()
    ts = {n: [] for n in arms}
    for _ in range(rounds):
        for n, fn in arms.items():
            ts[n].append(timed(fn, iters))
    return {n: (statistics.median(v), min(v), (max(v) - min(v)) / statistics.median(v)) for n, v in ts.items()}


def bench_attn(batches):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in batches:
        for form, Tk in (("self", 8), ("self", 224), ("self", 448), ("cross", TA)):
            cap = CAP if form == "self" else TA
            caches = [torch.randn(B, cap, 2 * D, device=DEV, generator=g).to(BF) for _ in range(LAYERS)]
            qkv = torch.randn(B, 3 * D, device=DEV, generator=g).to(BF) * 0.3
            lens = torch.full((B,), Tk, dtype=torch.int32, device=DEV)
            new, old, keep = [], [], []
            for c in caches:
                if form == "self":
                    a, o = K.attn_decode(qkv[:, :D], c, H, 0.125, new_kv=(qkv[:, D:2 * D], qkv[:, 2 * D:]), lens=lens, _args_only=True)
                else:
                    a, o = K.attn_decode(qkv[:, :D], c, H, 0.125, _args_only=True)
                new.append(a); keep.append(o)
                # the parent commit's way through the same ABI: one query row per sequence, no mask, one key count for the batch
                # (it does not append the step's k / v: the self-attention comparison flatters it by that copy)
                b = L.AttnArgs()
                o2 = torch.empty(B, 1, D, dtype=BF, device=DEV); lse = torch.empty(B, H, 1, dtype=torch.float32, device=DEV)
                b.q, b.ldq, b.q_bs = qkv.data_ptr(), 3 * D, 3 * D
                b.k, b.ldk, b.k_bs = c.data_ptr(), 2 * D, cap * 2 * D
                b.v, b.ldv, b.v_bs = c.data_ptr() + 2 * D, 2 * D, cap * 2 * D
                b.o, b.ldo, b.o_bs = o2.data_ptr(), D, D
                b.lse = lse.data_ptr()
                b.B, b.H, b.Tq, b.Tk, b.causal, b.scale = B, H, 1, Tk, 0, 0.125
                old.append(b); keep += [o2, lse]
            st = L.stream_ptr()

            def run_new():
                for a in new:
                    lib.wft_attn_decode_bf16(C.byref(a), st)

            def run_old():
                for b in old:
                    lib.wft_attn_fwd_bf16(C.byref(b), st)

            L.check(lib.wft_attn_decode_bf16(C.byref(new[0]), st), "wft_attn_decode_bf16")
            L.check(lib.wft_attn_fwd_bf16(C.byref(old[0]), st), "wft_attn_fwd_bf16")
            # same function: outputs agree to bf16 resolution at the size timed
            # (self form: the first call appended the step's k / v at row Tk - 1, which is what the other arm then reads)
            err = (keep[0].float() - keep[1].view(B, D).float()).abs().max().item()
            res = ab({"decode": run_new, "fwd_tq1": run_old})
            kv_bytes = B * H * Tk * 2 * 64 * 2
            rec = dict(part="attn", B=B, form=form, Tk=Tk, kv_MB=round(kv_bytes / 1e6, 2), max_abs_diff=err,
                       workspace_bytes=int(lib.wft_attn_decode_workspace_bytes(C.byref(new[0]))))
            for n, (med, mn, spread) in res.items():
                rec[n + "_us"] = round(med * 1e3 / LAYERS, 2)
                rec[n + "_min_us"] = round(mn * 1e3 / LAYERS, 2)
                rec[n + "_spread"] = round(spread, 3)
                rec[n + "_GBps"] = round(kv_bytes / (med * 1e-3 / LAYERS) / 1e9, 1)
            rec["speedup"] = round(res["fwd_tq1"][0] / res["decode"][0], 2)
            emit(rec)
            del caches, new, old, keep


def bench_gemm(batches):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(1)
    shapes = [("self q/k/v", 3 * D, D, LAYERS, L.EPI_NONE), ("self out", D, D, LAYERS, L.EPI_NONE), ("cross q", D, D, LAYERS, L.EPI_NONE),
              ("cross out", D, D, LAYERS, L.EPI_NONE), ("mlp.0 + GELU", 4 * D, D, LAYERS, L.EPI_GELU), ("mlp.2", D, 4 * D, LAYERS, L.EPI_NONE),
              ("tied logits", K.round_up(51866, 128), D, 4, L.EPI_NONE)]
    for B in batches:
        for name, N, Kd, copies, epi in shapes:
            ws = [torch.randn(N, Kd, device=DEV, generator=g).to(BF) * 0.02 for _ in range(copies)]
            x = torch.randn(B, Kd, device=DEV, generator=g).to(BF)
            bias = torch.zeros(N, device=DEV)
            calls, keep = [], []
            for w in ws:
                a, out = K.gemm_nt(x, w, bias=bias, epilogue=epi, _args_only=True)
                calls.append(a); keep.append(out)
            st = L.stream_ptr()

            def run():
                for a in calls:
                    lib.wft_gemm_nt_bf16(C.byref(a), st)

            L.check(lib.wft_gemm_nt_bf16(C.byref(calls[0]), st), "wft_gemm_nt_bf16")
            med, mn, spread = ab({"nt": run})["nt"]
            us = med * 1e3 / copies
            floor_us = N * Kd * 2 / HBM * 1e6
            emit(dict(part="gemm", B=B, call=name, N=N, K=Kd, kernel=int(lib.wft_gemm_nt_variant(C.byref(calls[0]))), us=round(us, 2),
                      min_us=round(mn * 1e3 / copies, 2), spread=round(spread, 3), weight_MB=round(N * Kd * 2 / 1e6, 2),
                      weight_floor_us=round(floor_us, 2), times_floor=round(us / floor_us, 1)))
            del ws, calls, keep


def bench_gemm_stream(batches):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(1)
    shapes = [("self q/k/v", 3 * D, D, LAYERS, L.EPI_NONE), ("self out", D, D, LAYERS, L.EPI_NONE), ("cross q", D, D, LAYERS, L.EPI_NONE),
              ("cross out", D, D, LAYERS, L.EPI_NONE), ("mlp.0 + GELU", 4 * D, D, LAYERS, L.EPI_GELU), ("mlp.2", D, 4 * D, LAYERS, L.EPI_NONE),
              ("tied logits", K.round_up(51866, 128), D, 4, L.EPI_NONE)]
    for B in batches:
        for name, N, Kd, copies, epi in shapes:
            ws = [torch.randn(N, Kd, device=DEV, generator=g).to(BF) * 0.02 for _ in range(copies)]
            x = torch.randn(B, Kd, device=DEV, generator=g).to(BF)
            bias = torch.zeros(N, device=DEV)
            old, new, keep = [], [], []
            for w in ws:
                a, out = K.gemm_nt(x, w, bias=bias, epilogue=epi, _args_only=True)
                served = K.gemm_nt_stream(x, w, bias=bias, epilogue=epi, _args_only=True)
                if served is None:
                    break
                old.append(a); new.append(served[0]); keep += [out, served[1]]
            if not new:
                emit(dict(part="gemm_stream", arm="stream_vs_nt", B=B, call=name, N=N, K=Kd, served=0))
                continue
            st = L.stream_ptr()

            def run_old():
                for a in old:
                    lib.wft_gemm_nt_bf16(C.byref(a), st)

            def run_new():
                for a in new:
                    lib.wft_gemm_nt_stream_bf16(C.byref(a), st)

            L.check(lib.wft_gemm_nt_bf16(C.byref(old[0]), st), "wft_gemm_nt_bf16")
            L.check(lib.wft_gemm_nt_stream_bf16(C.byref(new[0]), st), "wft_gemm_nt_stream_bf16")
            diff = (keep[0].float() - keep[1].float()).abs().max().item()
            res = ab({"nt": run_old, "stream": run_new})
            floor_us = N * Kd * 2 / HBM * 1e6
            us_old, us_new = res["nt"][0] * 1e3 / copies, res["stream"][0] * 1e3 / copies
            emit(dict(part="gemm_stream", arm="stream_vs_nt", B=B, call=name, N=N, K=Kd, served=1, nt_us=round(us_old, 2), nt_spread=round(res["nt"][2], 3),
                      stream_us=round(us_new, 2), stream_spread=round(res["stream"][2], 3), ratio=round(us_old / us_new, 2),
                      stream_TBps=round(N * Kd * 2 / (us_new * 1e-6) / 1e12, 3), weight_floor_us=round(floor_us, 2),
                      stream_times_floor=round(us_new / floor_us, 1), nt_times_floor=round(us_old / floor_us, 1), max_abs_diff=diff,
                      workspace_bytes=int(lib.wft_gemm_nt_stream_workspace_bytes(C.byref(new[0])))))
            del ws, old, new, keep


def bench_gemm_stream_q8(batches):
    """wft_gemm_nt_stream_q8 against wft_gemm_nt_stream_bf16 on the same weights (their int8 image and their bf16 shadow), the
    same x, bias and epilogue, enough distinct weight buffers in rotation that none is read from the Infinity Cache."""
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(2)
    shapes = [("self out / cross q / cross out", D, D, LAYERS, L.EPI_NONE), ("self q/k/v", 3 * D, D, LAYERS, L.EPI_NONE),
              ("mlp.0 + GELU", 4 * D, D, LAYERS, L.EPI_GELU), ("mlp.2", D, 4 * D, LAYERS, L.EPI_NONE),
              ("tied logits", K.round_up(51866, 128), D, 4, L.EPI_NONE)]
    for B in batches:
        for name, N, Kd, copies, epi in shapes:
            x = torch.randn(B, Kd, device=DEV, generator=g).to(BF)
            bias = torch.zeros(N, device=DEV)
            bf, q8, keep = [], [], []
            for _ in range(copies):
                w = torch.randn(N, Kd, device=DEV, generator=g).to(BF) * 0.02
                qw, qs = K.quantize_rows_i8(w)
                a = K.gemm_nt_stream(x, w, bias=bias, epilogue=epi, _args_only=True)
                b = K.gemm_nt_stream_q8(x, qw, qs, bias=bias, epilogue=epi, _args_only=True)
                if a is None or b is None:
                    break
                bf.append(a[0]); q8.append((b[0], qs)); keep += [w, qw, a[1], b[1]]
            if not q8:
                emit(dict(part="gemm_stream", arm="q8_vs_stream", B=B, call=name, N=N, K=Kd, served=0))
                continue
            st = L.stream_ptr()

            def run_bf():
                for a in bf:
                    lib.wft_gemm_nt_stream_bf16(C.byref(a), st)

            def run_q8():
                for a, qs in q8:
                    lib.wft_gemm_nt_stream_q8(C.byref(a), qs.data_ptr(), st)

            L.check(lib.wft_gemm_nt_stream_bf16(C.byref(bf[0]), st), "wft_gemm_nt_stream_bf16")
            L.check(lib.wft_gemm_nt_stream_q8(C.byref(q8[0][0]), q8[0][1].data_ptr(), st), "wft_gemm_nt_stream_q8")
            diff = (keep[2].float() - keep[3].float()).abs().max().item()
            res = ab({"bf16": run_bf, "q8": run_q8})
            us_bf, us_q8 = res["bf16"][0] * 1e3 / copies, res["q8"][0] * 1e3 / copies
            emit(dict(part="gemm_stream", arm="q8_vs_stream", B=B, call=name, N=N, K=Kd, served=1, bf16_us=round(us_bf, 2),
                      bf16_spread=round(res["bf16"][2], 3), q8_us=round(us_q8, 2), q8_spread=round(res["q8"][2], 3), ratio=round(us_bf / us_q8, 2),
                      bf16_TBps=round(N * Kd * 2 / (us_bf * 1e-6) / 1e12, 3), q8_TBps=round(N * Kd / (us_q8 * 1e-6) / 1e12, 3),
                      q8_weight_floor_us=round(N * Kd / HBM * 1e6, 2), max_abs_diff=diff,
                      workspace_bytes=int(lib.wft_gemm_nt_stream_q8_workspace_bytes(C.byref(q8[0][0])))))
            del bf, q8, keep


def bench_gemm_i8(batches, copies=4):
    """The W8A8 product as ops.linear issues it under decode.int8_gemm() — wft_quantize_rows_i8 on the activation, then wft_gemm_nt_i8
    on the int8 image of the weights — against wft_gemm_nt_bf16 on the bf16 shadow, alternating, at the large-v3 encoder / prefill
    shapes with M = 1500 * B (--batches = B); a third arm times wft_gemm_nt_i8 alone (the quantiser's share is the difference).
    All arms go through the Python wrappers into preallocated outputs, `copies` weight buffers in rotation.  Then arm = "e2e":
    encoder + prefill (40-token prompts) of a random large-v3 model under weights="bf16" and under "w8a8"."""
    from whisper_finetune.engine import decode as Dm

    g = torch.Generator(device="cuda").manual_seed(3)
    shapes = [("self q/k/v", 3 * D, D, L.EPI_NONE), ("attention out / cross q", D, D, L.EPI_NONE), ("mlp.0 + GELU", 4 * D, D, L.EPI_GELU),
              ("mlp.2", D, 4 * D, L.EPI_NONE), ("cross k/v", 2 * D, D, L.EPI_NONE)]
    for B in batches:
        M = TA * B
        for name, N, Kd, epi in shapes:
            x = torch.randn(M, Kd, device=DEV, generator=g).to(BF)
            bias = torch.zeros(N, device=DEV)
            ws = [torch.randn(N, Kd, device=DEV, generator=g).to(BF) * 0.02 for _ in range(copies)]
            qs = [K.quantize_rows_i8(w) for w in ws]
            out_bf, out_i8 = torch.empty(M, N, dtype=BF, device=DEV), torch.empty(M, N, dtype=BF, device=DEV)
            xq, xs = K.quantize_rows_i8(x)
            assert K.gemm_nt_i8_serves(M, N, Kd, epi)

            def run_bf():
                for w in ws:
                    K.gemm_nt(x, w, bias=bias, epilogue=epi, out=out_bf)

            def run_i8():
                for qw, sc in qs:
                    K.quantize_rows_i8(x, out=xq, scale=xs)
                    K.gemm_nt_i8(xq, xs, qw, sc, bias=bias, epilogue=epi, out=out_i8)

            def run_i8_gemm():
                for qw, sc in qs:
                    K.gemm_nt_i8(xq, xs, qw, sc, bias=bias, epilogue=epi, out=out_i8)

            run_bf(); run_i8()
            diff = (out_bf.float() - out_i8.float()).abs().max().item()
            res = ab({"bf16": run_bf, "i8": run_i8, "i8_gemm": run_i8_gemm}, rounds=5, iters=2)
            us = {k: v[0] * 1e3 / copies for k, v in res.items()}
            emit(dict(part="gemm_i8", arm="i8_vs_nt", B=B, M=M, call=name, N=N, K=Kd, bf16_us=round(us["bf16"], 1), bf16_spread=round(res["bf16"][2], 3),
                      i8_us=round(us["i8"], 1), i8_spread=round(res["i8"][2], 3), i8_gemm_only_us=round(us["i8_gemm"], 1),
                      quantiser_us=round(us["i8"] - us["i8_gemm"], 1), ratio=round(us["bf16"] / us["i8"], 3),
                      bf16_TFps=round(2.0 * M * N * Kd / (us["bf16"] * 1e-6) / 1e12, 1), i8_gemm_TOps=round(2.0 * M * N * Kd / (us["i8_gemm"] * 1e-6) / 1e12, 1),
                      max_abs_diff=diff))
            del x, ws, qs, out_bf, out_i8, xq, xs
    m, dims = _random_large_v3()
    for B in batches:
        mel = torch.randn(B, dims.n_mels, 2 * TA, device=DEV, generator=g)
        prompt = torch.randint(0, 50000, (B, 40), device=DEV, generator=g)
        cache = Dm.KVCache(m.decoder, B, device=DEV)

        def run(weights):
            with torch.no_grad():
                xa = Dm.encode(m, mel, weights)
                cache.start(prompt, None, eot=50257, max_len=41, n_vocab=dims.n_vocab)
                with Dm.int8_gemm(weights == "w8a8"):
                    Dm.prefill(m.decoder, cache, xa)

        res = ab({"bf16": lambda: run("bf16"), "w8a8": lambda: run("w8a8")}, rounds=5, iters=1)
        emit(dict(part="gemm_i8", arm="e2e", B=B, what="encoder + prefill of 40-token prompts, large-v3, random weights", bf16_ms=round(res["bf16"][0], 2),
                  bf16_spread=round(res["bf16"][2], 3), w8a8_ms=round(res["w8a8"][0], 2), w8a8_spread=round(res["w8a8"][2], 3),
                  ratio=round(res["bf16"][0] / res["w8a8"][0], 3)))


def _random_large_v3():
    dims = MODEL_DIMS["large-v3"]
    with torch.device(DEV):
        m = Whisper(dims)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() >= 2:
                p.normal_(0, 0.02)
            elif n.endswith("weight"):
                p.fill_(1.0)
            else:
                p.zero_()
    return m.eval(), dims


def bench_e2e_step(batches, new_tokens=64, runs=3):
    from whisper_finetune.engine import decode as Dm

    m, dims = _random_large_v3()
    lib = L.load()
    eot = 50257
    arms = {"eager": dict(), "eager_stream": dict(step="graph", _capture=False), "graph_nt": dict(step="graph", _stream_gemm=False),
            "graph": dict(step="graph"), "graph_int8": dict(step="graph", weights="int8")}
    for B in batches:
        g = torch.Generator(device="cuda").manual_seed(B)
        mel = torch.randn(B, dims.n_mels, 2 * dims.n_audio_ctx, device=DEV, generator=g)
        prompt = torch.tensor([[50258, 50261, 50360, 50364]], device=DEV).expand(B, 4).contiguous()
        max_len = 4 + new_tokens
        # library calls of one cached step + pick per GEMM route (every call that takes a stream enqueues at least one kernel;
        # a streaming GEMM is two: kernel + reduce).  The graph arms issue the same work as ONE graph launch per step.
        counts = {}
        for route in (False, True, "int8"):
            cache = Dm.KVCache(m.decoder, B, device=DEV)
            with torch.no_grad():
                cache.start(prompt, None, eot=eot, max_len=max_len, suppress=[eot], n_vocab=dims.n_vocab)
                lg = Dm.prefill(m.decoder, cache, m.encoder(mel)); Dm.pick(m.decoder, cache, lg)
                with _CountCalls() as cc, Dm.stream_gemm(bool(route), "int8" if route == "int8" else "bf16"):
                    lg = Dm.step(m.decoder, cache); Dm.pick(m.decoder, cache, lg)
            counts[route] = (sum(cc.n.values()), cc.n.get("wft_gemm_nt_stream_bf16", 0), cc.n.get("wft_gemm_nt_bf16", 0),
                             cc.n.get("wft_gemm_nt_stream_q8", 0))
            del cache
        route_of = {"eager": False, "eager_stream": True, "graph_nt": False, "graph": True, "graph_int8": "int8"}
        times, outs = {a: [] for a in arms}, {}
        for a, kw in arms.items():  # warm-up: shadows, workspaces, code objects, the capture
            m.greedy_decode(mel, prompt, None, eot=eot, max_len=max_len, suppress=[eot], **kw)
        for rnd in range(runs):
            for a, kw in arms.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                outs[a] = m.greedy_decode(mel, prompt, None, eot=eot, max_len=max_len, suppress=[eot], **kw)
                torch.cuda.synchronize(); times[a].append(time.perf_counter() - t0)
        # the encoder + prefill share of a call, to report the per-token figure of the cached steps alone
        pre = []
        for rnd in range(runs):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            m.greedy_decode(mel, prompt, None, eot=eot, max_len=5, suppress=[eot])
            torch.cuda.synchronize(); pre.append(time.perf_counter() - t0)
        pre_s = statistics.median(pre)
        for a in arms:
            med = statistics.median(times[a])
            emit(dict(part="e2e_step", arm=a, B=B, new_tokens=new_tokens, runs_s=[round(t, 4) for t in times[a]], median_s=round(med, 4),
                      spread=round((max(times[a]) - min(times[a])) / med, 3), tok_s=round(B * new_tokens / med, 1),
                      encoder_prefill_s=round(pre_s, 4), ms_per_step=round((med - pre_s) / (new_tokens - 1) * 1e3, 3),
                      library_calls_per_step=counts[route_of[a]][0], stream_gemm_calls=counts[route_of[a]][1],
                      nt_gemm_calls=counts[route_of[a]][2], q8_gemm_calls=counts[route_of[a]][3], host_launches_per_step=1 if a.startswith("graph") else counts[route_of[a]][0],
                      same_tokens_as_eager=round((outs[a][0] == outs["eager"][0]).float().mean().item(), 4),
                      speedup_vs_eager=round(statistics.median(times["eager"]) / med, 2),
                      speedup_vs_graph=round(statistics.median(times["graph"]) / med, 2)))
        Dm.release_graphs(m)


class _CountCalls:
    """Counts, per entry point, the libwft calls that enqueue work (the ones whose last argument is the stream)."""

    def __enter__(self):
        self.n, self.real = {}, {}
        lib = L.load()
        for name, argtypes in L.SIGNATURES.items():
            if argtypes and argtypes[-1] is L.c_vp and name.startswith("wft_") and not name.endswith("_bytes"):
                fn = getattr(lib, name)
                self.real[name] = fn

                def counted(*a, _fn=fn, _name=name):
                    self.n[_name] = self.n.get(_name, 0) + 1
                    return _fn(*a)

                setattr(lib, name, counted)
        return self

    def __exit__(self, *exc):
        lib = L.load()
        for name, fn in self.real.items():
            setattr(lib, name, fn)


def bench_e2e(batches, new_tokens=64):
    dims = MODEL_DIMS["large-v3"]
    with torch.device(DEV):
        m = Whisper(dims)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() >= 2:
                p.normal_(0, 0.02)
            elif n.endswith("weight"):
                p.fill_(1.0)
            else:
                p.zero_()
    m.eval()
    eot = 50257
    for B in batches:
        g = torch.Generator(device="cuda").manual_seed(B)
        mel = torch.randn(B, dims.n_mels, 2 * dims.n_audio_ctx, device=DEV, generator=g)
        prompt = torch.tensor([[50258, 50261, 50360, 50364]], device=DEV).expand(B, 4).contiguous()
        max_len = 4 + new_tokens

        def cached():
            # eot suppressed: every row generates exactly new_tokens tokens
            return m.greedy_decode(mel, prompt, None, eot=eot, max_len=max_len, suppress=[eot])

        def reforward():
            with torch.no_grad():
                xa = m.embed_audio(mel)
                toks = prompt
                for _ in range(new_tokens):
                    lg = m.logits(toks, xa)[:, -1]
                    lg[:, eot] = float("-inf")
                    toks = torch.cat([toks, lg.argmax(-1, keepdim=True)], 1)
                return toks

        res = {}
        for name, fn in (("greedy_decode", cached), ("reforward", reforward)):
            fn()  # warm-up: shadows, workspaces, code objects
        for rnd in range(2):
            for name, fn in (("greedy_decode", cached), ("reforward", reforward)):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize(); res.setdefault(name, []).append(time.perf_counter() - t0)
                res[name + "_out"] = out
        a, b = res["greedy_decode_out"][0][:, :max_len], res["reforward_out"]
        emit(dict(part="e2e", B=B, new_tokens=new_tokens, greedy_decode_s=[round(t, 4) for t in res["greedy_decode"]],
                  reforward_s=[round(t, 4) for t in res["reforward"]],
                  greedy_decode_tok_s=round(B * new_tokens / min(res["greedy_decode"]), 1),
                  reforward_tok_s=round(B * new_tokens / min(res["reforward"]), 1),
                  speedup=round(min(res["reforward"]) / min(res["greedy_decode"]), 2),
                  same_tokens_share=round((a == b).float().mean().item(), 4),
                  note="both timings include the encoder pass; tokens differ only where two bf16 evaluations break a near-tie"))


def bench_beam(batches, W=5, new_tokens=64, runs=3):
    from whisper_finetune.engine import decode as Dm

    lib = L.load()
    st = L.stream_ptr()
    g = torch.Generator(device="cuda").manual_seed(2)

    def rec_times(rec, res):
        for n, (med, mn, spread) in res.items():
            rec[n + "_us"] = round(med * 1e3 / LAYERS, 2)
            rec[n + "_min_us"] = round(mn * 1e3 / LAYERS, 2)
            rec[n + "_spread"] = round(spread, 3)

    def runner(fn, calls):
        def run():
            for a in calls:
                fn(C.byref(a), st)
        return run

    for B in batches:
        R = B * W
        # (i) the self form against the existing kernel, same rows and keys
        for Tk in (8, 224, 448):
            caches = [torch.randn(R, CAP, 2 * D, device=DEV, generator=g).to(BF) for _ in range(LAYERS)]
            qkv = torch.randn(R, 3 * D, device=DEV, generator=g).to(BF) * 0.3
            lens = torch.full((R,), Tk, dtype=torch.int32, device=DEV)
            ident = torch.arange(R, dtype=torch.int32, device=DEV)[:, None].expand(-1, CAP).contiguous()
            # every entry names a random beam of the row's own audio, as a run that reorders at every step would leave it
            scr = (torch.arange(R, device=DEV)[:, None] // W * W + torch.randint(0, W, (R, CAP), device=DEV, generator=g)).to(torch.int32)
            old, new_i, new_s, keep = [], [], [], []
            for c in caches:
                kw = dict(new_kv=(qkv[:, D:2 * D], qkv[:, 2 * D:]), lens=lens, _args_only=True)
                a, o = K.attn_decode(qkv[:, :D], c, H, 0.125, **kw); old.append(a); keep.append(o)
                a, o = K.attn_decode_beam(qkv[:, :D], c, H, 0.125, anc=ident, **kw); new_i.append(a); keep.append(o)
                a, o = K.attn_decode_beam(qkv[:, :D], c, H, 0.125, anc=scr, **kw); new_s.append(a); keep.append(o)
            L.check(lib.wft_attn_decode_bf16(C.byref(old[0]), st), "wft_attn_decode_bf16")
            L.check(lib.wft_attn_decode_beam_bf16(C.byref(new_i[0]), st), "wft_attn_decode_beam_bf16")
            same = bool(torch.equal(keep[0].view(torch.int16), keep[1].view(torch.int16)))
            res = ab({"decode": runner(lib.wft_attn_decode_bf16, old), "beam_identity": runner(lib.wft_attn_decode_beam_bf16, new_i),
                      "beam_scrambled": runner(lib.wft_attn_decode_beam_bf16, new_s)})
            rec = dict(part="beam", arm="self", B=B, W=W, rows=R, Tk=Tk, kv_MB=round(R * H * Tk * 2 * 64 * 2 / 1e6, 2), identity_bits_equal=same)
            rec_times(rec, res)
            rec["identity_vs_decode"] = round(res["beam_identity"][0] / res["decode"][0], 3)
            rec["scrambled_vs_decode"] = round(res["beam_scrambled"][0] / res["decode"][0], 3)
            emit(rec)
            del caches, old, new_i, new_s, keep
        # (ii) the grouped cross form against the existing kernel at R rows on replicated caches
        caches = [torch.randn(B, TA, 2 * D, device=DEV, generator=g).to(BF) for _ in range(LAYERS)]
        reps = [c.repeat_interleave(W, 0) for c in caches]
        q = torch.randn(R, D, device=DEV, generator=g).to(BF) * 0.3
        old, new, keep = [], [], []
        for c, r in zip(caches, reps):
            a, o = K.attn_decode(q, r, H, 0.125, _args_only=True); old.append(a); keep.append(o)
            a, o = K.attn_decode_beam(q, c, H, 0.125, group=W, _args_only=True); new.append(a); keep.append(o)
        L.check(lib.wft_attn_decode_bf16(C.byref(old[0]), st), "wft_attn_decode_bf16")
        L.check(lib.wft_attn_decode_beam_bf16(C.byref(new[0]), st), "wft_attn_decode_beam_bf16")
        diff = (keep[0].float() - keep[1].float()).abs().max().item()
        res = ab({"decode_replicated": runner(lib.wft_attn_decode_bf16, old), "beam_grouped": runner(lib.wft_attn_decode_beam_bf16, new)})
        rec = dict(part="beam", arm="cross", B=B, W=W, rows=R, Tk=TA, max_abs_diff=diff, bits_equal=bool(torch.equal(keep[0].view(torch.int16), keep[1].view(torch.int16))),
                   replicated_kv_MB=round(R * H * TA * 256 / 1e6, 2), grouped_kv_MB=round(B * H * TA * 256 / 1e6, 2),
                   grouped_workspace_bytes=int(lib.wft_attn_decode_beam_workspace_bytes(C.byref(new[0]))),
                   replicated_workspace_bytes=int(lib.wft_attn_decode_workspace_bytes(C.byref(old[0]))))
        rec_times(rec, res)
        rec["decode_replicated_TBps"] = round(R * H * TA * 256 / (res["decode_replicated"][0] * 1e-3 / LAYERS) / 1e12, 3)
        rec["beam_grouped_TBps"] = round(B * H * TA * 256 / (res["beam_grouped"][0] * 1e-3 / LAYERS) / 1e12, 3)
        rec["speedup"] = round(res["decode_replicated"][0] / res["beam_grouped"][0], 2)
        emit(rec)
        del caches, reps, old, new, keep
        # (iii) top-k + update against the greedy pick, both at R rows (32 rotating logits buffers)
        V, n_ctx = 51866, CAP
        ld = K.round_up(V, 128)
        logits = [(torch.randn(R, ld, device=DEV, generator=g) * 3).to(BF) for _ in range(LAYERS)]
        tokens = torch.zeros(R, n_ctx, dtype=torch.int64, device=DEV)
        i32 = dict(dtype=torch.int32, device=DEV)
        sup = torch.zeros(V, dtype=torch.uint8, device=DEV); sup[50257:] = 1
        state = dict(lens=torch.full((R,), 100, **i32), fin=torch.zeros(R, **i32), slp=torch.zeros(R, device=DEV), unf=torch.zeros(1, **i32),
                     anc=torch.zeros(R, n_ctx, **i32), done=torch.zeros(B, **i32), ct=torch.zeros(R, W + 1, **i32), cl=torch.zeros(R, W + 1, device=DEV),
                     ft=torch.zeros(B, W, n_ctx, dtype=torch.int64, device=DEV), fl=torch.zeros(B, W, **i32), fs=torch.zeros(B, W, device=DEV),
                     fn=torch.zeros(B, **i32))

        def reset():
            state["lens"].fill_(100); state["fin"].zero_(); state["done"].zero_(); state["fn"].zero_()

        def run_pick():
            reset()
            for lg in logits:
                K.decode_pick(lg, V, tokens, state["lens"], state["fin"], state["slp"], state["unf"], eot=50257, max_len=n_ctx, suppress=sup,
                              first_len=state["lens"])

        def run_topk():
            reset()
            for lg in logits:
                K.decode_topk(lg, V, state["ct"], state["cl"], lens=state["lens"], first_len=state["lens"], suppress=sup)

        def run_beam():
            reset()
            for lg in logits:
                K.decode_topk(lg, V, state["ct"], state["cl"], lens=state["lens"], first_len=state["lens"], suppress=sup)
                K.beam_update(state["ct"], state["cl"], tokens, state["anc"], state["lens"], state["slp"], state["done"], state["unf"], state["ft"],
                              state["fl"], state["fs"], state["fn"], eot=50257, max_len=n_ctx)

        res = ab({"pick": run_pick, "topk": run_topk, "topk_update": run_beam}, iters=2)
        rec = dict(part="beam", arm="pick", B=B, W=W, rows=R, V=V, logits_MB=round(R * V * 2 / 1e6, 2),
                   note="one call per rotating logits buffer, issued through the Python wrappers (their host time is in every arm)")
        rec_times(rec, res)
        rec["topk_update_vs_pick"] = round(res["topk_update"][0] / res["pick"][0], 2)
        emit(rec)
        del logits

    # (iv) end to end: beam_decode(W) over B audios against greedy_decode at batch = B * W, eager and graph
    m, dims = _random_large_v3()
    eot = 50257
    for B in batches:
        R = B * W
        gm = torch.Generator(device="cuda").manual_seed(B)
        mel = torch.randn(R, dims.n_mels, 2 * dims.n_audio_ctx, device=DEV, generator=gm)
        prompt = torch.tensor([[50258, 50261, 50360, 50364]], device=DEV).expand(R, 4).contiguous()
        max_len = 4 + new_tokens
        arms = {}
        for mode in ("eager", "graph"):
            arms["beam_" + mode] = lambda n=5, mode=mode, max_len=max_len: m.beam_decode(mel[:B], prompt[:B], None, beam_size=W, eot=eot, max_len=max_len if n else 5,
                                                                                        suppress=[eot], step=mode)
            arms["greedy_" + mode] = lambda n=5, mode=mode, max_len=max_len: m.greedy_decode(mel, prompt, None, eot=eot, max_len=max_len if n else 5, suppress=[eot],
                                                                                            step=mode)
        times, pre = {a: [] for a in arms}, {a: [] for a in arms}
        for fn in arms.values():
            fn()  # warm-up: shadows, workspaces, code objects, the capture
        for rnd in range(runs):
            for a, fn in arms.items():
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times[a].append(time.perf_counter() - t0)
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(0); torch.cuda.synchronize(); pre[a].append(time.perf_counter() - t0)
        for a in arms:
            med, pre_s = statistics.median(times[a]), statistics.median(pre[a])
            other = statistics.median(times[a.replace("beam_", "greedy_")])
            emit(dict(part="beam", arm="e2e_" + a, B=B, W=W, rows=R, new_tokens=new_tokens, runs_s=[round(t, 4) for t in times[a]], median_s=round(med, 4),
                      spread=round((max(times[a]) - min(times[a])) / med, 3), encoder_prefill_s=round(pre_s, 4),
                      ms_per_step=round((med - pre_s) / (new_tokens - 1) * 1e3, 3),
                      tok_s=round((B if a.startswith("beam") else R) * new_tokens / med, 1), hypothesis_tok_s=round(R * new_tokens / med, 1),
                      time_vs_greedy_at_R_rows=round(med / other, 3)))
        Dm.release_graphs(m)


def bench_ts(batches):
    """Pick / top-6 with and without the timestamp rules at R rows: 32 rotating logits buffers (a single one would sit in the
    Infinity Cache), issued through the Python wrappers (their host time is in every arm)."""
    V, n_ctx, tsb, eot, k = 51866, CAP, 50365, 50257, 6
    ld = K.round_up(V, 128)
    i32 = dict(dtype=torch.int32, device=DEV)
    g = torch.Generator(device="cuda").manual_seed(0)
    for R in batches:
        logits = [(torch.randn(R, ld, device=DEV, generator=g) * 3).to(BF) for _ in range(LAYERS)]
        tokens = torch.randint(0, eot, (R, n_ctx), device=DEV, generator=g)
        tokens[:, 4] = tsb + 10  # the opening timestamp of every row; text behind it
        sup = torch.zeros(V, dtype=torch.uint8, device=DEV); sup[eot + 1:tsb] = 1
        first = torch.full((R,), 4, **i32)
        st = dict(lens=torch.full((R,), 104, **i32), fin=torch.zeros(R, **i32), slp=torch.zeros(R, device=DEV), unf=torch.zeros(1, **i32),
                  ct=torch.zeros(R, k, **i32), cl=torch.zeros(R, k, device=DEV))
        rules = (tsb, tsb - 1, 50)

        def pick(ru):
            st["lens"].fill_(104); st["fin"].zero_()
            for lg in logits:
                st["lens"].fill_(104)
                K.decode_pick(lg, V, tokens, st["lens"], st["fin"], st["slp"], st["unf"], eot=eot, max_len=n_ctx, suppress=sup, first_len=first, ts_rules=ru)

        def topk(ru):
            for lg in logits:
                K.decode_topk(lg, V, st["ct"], st["cl"], lens=st["lens"], first_len=first, suppress=sup, ts_rules=ru, tokens=tokens, eot=eot)

        res = ab({"pick": lambda: pick(None), "pick_ts": lambda: pick(rules), "topk": lambda: topk(None), "topk_ts": lambda: topk(rules)}, iters=2)
        rec = dict(part="ts", rows=R, V=V, k=k, sampled_tokens=100, logits_MB=round(R * V * 2 / 1e6, 2),
                   note="us per call; the pick arms include one fill_ of `len` per call")
        for n, (med, mn, spread) in res.items():
            rec[n + "_us"] = round(med * 1e3 / LAYERS, 2)
            rec[n + "_min_us"] = round(mn * 1e3 / LAYERS, 2)
            rec[n + "_spread"] = round(spread, 3)
        rec["pick_ts_vs_pick"] = round(res["pick_ts"][0] / res["pick"][0], 2)
        rec["topk_ts_vs_topk"] = round(res["topk_ts"][0] / res["topk"][0], 2)
        emit(rec)
        del logits


def bench_sample(batches, N=5, new_tokens=64, runs=3):
    """(i) the sampled pick against the greedy pick, plain and under the timestamp rules, at R = N * B rows: bench_ts's rows and
    rotating logits buffers, issued through the Python wrappers (their host time is in every arm); (ii) sample_decode(best_of = N)
    against beam_decode(W = N) over B audios and greedy_decode at batch N * B."""
    from whisper_finetune.engine import decode as Dm

    V, n_ctx, tsb, eot = 51866, CAP, 50365, 50257
    ld = K.round_up(V, 128)
    i32 = dict(dtype=torch.int32, device=DEV)
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in batches:
        R = B * N
        logits = [(torch.randn(R, ld, device=DEV, generator=g) * 3).to(BF) for _ in range(LAYERS)]
        tokens = torch.randint(0, eot, (R, n_ctx), device=DEV, generator=g)
        tokens[:, 4] = tsb + 10  # the opening timestamp of every row; text behind it
        sup = torch.zeros(V, dtype=torch.uint8, device=DEV); sup[eot + 1:tsb] = 1
        first = torch.full((R,), 4, **i32)
        st = dict(lens=torch.full((R,), 104, **i32), fin=torch.zeros(R, **i32), slp=torch.zeros(R, device=DEV), unf=torch.zeros(1, **i32))
        temps = {0.0: torch.zeros(R, device=DEV), 1.0: torch.ones(R, device=DEV)}
        seeds = torch.arange(R, dtype=torch.int64, device=DEV) + 1234
        rules = (tsb, tsb - 1, 50)

        def pick(ru):
            st["fin"].zero_()
            for lg in logits:
                st["lens"].fill_(104)
                K.decode_pick(lg, V, tokens, st["lens"], st["fin"], st["slp"], st["unf"], eot=eot, max_len=n_ctx, suppress=sup, first_len=first, ts_rules=ru)

        def sample(ru, t):
            st["fin"].zero_()
            for lg in logits:
                st["lens"].fill_(104)
                K.decode_sample(lg, V, tokens, st["lens"], st["fin"], st["slp"], st["unf"], temps[t], seeds, eot=eot, max_len=n_ctx, suppress=sup,
                                first_len=first, ts_rules=ru)

        res = ab({"pick": lambda: pick(None), "sample_t0": lambda: sample(None, 0.0), "sample": lambda: sample(None, 1.0),
                  "pick_ts": lambda: pick(rules), "sample_ts_t0": lambda: sample(rules, 0.0), "sample_ts": lambda: sample(rules, 1.0)}, iters=2)
        rec = dict(part="sample", arm="pick", rows=R, V=V, sampled_tokens=100, logits_MB=round(R * V * 2 / 1e6, 2),
                   note="us per call; every arm includes one fill_ of `len` per call; _t0: the sampled kernel at temperature 0 (its greedy path)")
        for n, (med, mn, spread) in res.items():
            rec[n + "_us"] = round(med * 1e3 / LAYERS, 2)
            rec[n + "_min_us"] = round(mn * 1e3 / LAYERS, 2)
            rec[n + "_spread"] = round(spread, 3)
        rec["sample_vs_pick"] = round(res["sample"][0] / res["pick"][0], 2)
        rec["sample_ts_vs_pick_ts"] = round(res["sample_ts"][0] / res["pick_ts"][0], 2)
        emit(rec)
        del logits

    m, dims = _random_large_v3()
    for B in batches:
        R = B * N
        gm = torch.Generator(device="cuda").manual_seed(B)
        mel = torch.randn(R, dims.n_mels, 2 * dims.n_audio_ctx, device=DEV, generator=gm)
        prompt = torch.tensor([[50258, 50261, 50360, 50364]], device=DEV).expand(R, 4).contiguous()
        max_len = 4 + new_tokens
        kw = dict(eot=eot, suppress=[eot])  # eot suppressed: every row generates exactly new_tokens tokens
        arms = {}
        for mode in ("eager", "graph"):
            arms["sample_" + mode] = lambda n=1, mode=mode: m.sample_decode(mel[:B], prompt[:B], None, temperature=1.0, best_of=N, seed=7,
                                                                            max_len=max_len if n else 5, step=mode, **kw)
            arms["beam_" + mode] = lambda n=1, mode=mode: m.beam_decode(mel[:B], prompt[:B], None, beam_size=N, max_len=max_len if n else 5, step=mode, **kw)
            arms["greedy_" + mode] = lambda n=1, mode=mode: m.greedy_decode(mel, prompt, None, max_len=max_len if n else 5, step=mode, **kw)
        times, pre = {a: [] for a in arms}, {a: [] for a in arms}
        for fn in arms.values():
            fn()  # warm-up: shadows, workspaces, code objects, the capture
        for rnd in range(runs):
            for a, fn in arms.items():
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times[a].append(time.perf_counter() - t0)
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(0); torch.cuda.synchronize(); pre[a].append(time.perf_counter() - t0)
        for a in arms:
            med, pre_s = statistics.median(times[a]), statistics.median(pre[a])
            mode = a.split("_")[1]
            emit(dict(part="sample", arm="e2e_" + a, B=B, N=N, rows=R, new_tokens=new_tokens, runs_s=[round(t, 4) for t in times[a]], median_s=round(med, 4),
                      spread=round((max(times[a]) - min(times[a])) / med, 3), encoder_prefill_s=round(pre_s, 4),
                      ms_per_step=round((med - pre_s) / (new_tokens - 1) * 1e3, 3),
                      tok_s=round((R if a.startswith("greedy") else B) * new_tokens / med, 1), row_tok_s=round(R * new_tokens / med, 1),
                      time_vs_beam=round(med / statistics.median(times["beam_" + mode]), 3),
                      time_vs_greedy_at_R_rows=round(med / statistics.median(times["greedy_" + mode]), 3)))
        Dm.release_graphs(m)


def bench_align(batches, n_heads=10, T=CAP, frames=2 * TA, rounds=5):
    """The alignment kernels at large-v3 dimensions: the 10 heads spread over 5 layers' q / kv buffers (2 heads each, as the capture
    issues them: 5 launches of wft_attn_probs_bf16), scores spread to a standard deviation of about 2; then the whole call."""
    import numpy as np

    from whisper_finetune.engine import decode as Dm

    g = torch.Generator(device="cuda").manual_seed(0)
    sot, row0 = 3, 3
    for B in batches:
        lens, keys = [T] * B, [frames // 2] * B
        n_tok, n_key = torch.tensor(lens, dtype=torch.int32, device=DEV), torch.tensor(keys, dtype=torch.int32, device=DEV)
        n_rows = [T - sot - 1] * B
        n_rows_d = torch.tensor(n_rows, dtype=torch.int32, device=DEV)
        layers = n_heads // 2
        qs = [(torch.randn(B, T, D, device=DEV, generator=g) * 2 ** 0.5).to(BF) for _ in range(layers)]
        kvs = [(torch.randn(B, TA, 2 * D, device=DEV, generator=g) * 2 ** 0.5).to(BF) for _ in range(layers)]
        heads = [torch.tensor([3 + 2 * i, 11 + i], dtype=torch.int32, device=DEV) for i in range(layers)]
        probs = torch.zeros(B, n_heads, T, TA, device=DEV)
        matrix = torch.zeros(B, T, TA, device=DEV)

        def stage_a():
            for i in range(layers):
                K.attn_probs(qs[i], kvs[i][..., :D], heads[i], n_tok, n_key, H, 0.125, probs[:, 2 * i:2 * i + 2], host_lens=(lens, keys))

        def stage_b():
            K.align_matrix(probs, n_tok, n_key, 7, out=matrix, host_lens=(lens, keys))

        paths = None

        def stage_c():
            nonlocal paths
            paths = K.dtw(matrix, row0, n_rows_d, n_key, host_lens=(n_rows, keys), paths=paths)

        def torch_a():
            out = []
            for i in range(layers):
                hs = heads[i].tolist()
                qh = qs[i].view(B, T, H, 64)[:, :, hs].permute(0, 2, 1, 3).float()
                kh = kvs[i][..., :D].reshape(B, TA, H, 64)[:, :, hs].permute(0, 2, 1, 3).float()
                out.append(torch.softmax(qh @ kh.transpose(-1, -2) * 0.125, dim=-1))
            return torch.cat(out, 1)

        def torch_b():
            std, mean = torch.std_mean(probs, dim=-2, keepdim=True, unbiased=False)
            z = (probs - mean) / std
            z = torch.nn.functional.pad(z, (3, 3, 0, 0), mode="reflect")
            return z.unfold(-1, 7, 1).sort()[0][..., 3].mean(1)

        def host_c():
            x = -matrix[:, row0:row0 + n_rows[0]].cpu().numpy()
            for b in range(B):
                N, M = x[b].shape
                cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
                trace = np.zeros((N + 1, M + 1), dtype=np.int8)
                cost[0, 0] = 0
                for s_ in range(2, N + M + 1):
                    i = np.arange(max(1, s_ - M), min(N, s_ - 1) + 1)
                    j = s_ - i
                    c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
                    t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
                    cost[i, j] = x[b][i - 1, j - 1] + np.where(t == 0, c0, np.where(t == 1, c1, c2))
                    trace[i, j] = t
                i, j, n = N, M, 0
                while i > 0 or j > 0:  # the backtrace
                    t = trace[i, j] if i > 0 and j > 0 else (2 if i == 0 else 1)
                    i, j, n = i - (t != 2), j - (t != 1), n + 1

        stage_a(); stage_b(); stage_c()
        same = torch.allclose(torch_a(), probs, rtol=1e-3, atol=1e-7), torch.allclose(torch_b(), matrix, rtol=0, atol=1e-3)
        res = ab({"attn_probs": stage_a, "align_matrix": stage_b, "dtw": stage_c, "torch_softmax": torch_a, "torch_filter": torch_b}, rounds=rounds, iters=2)
        t0 = time.perf_counter()
        host_c()
        host_ms = (time.perf_counter() - t0) * 1e3
        rec = dict(part="align", what="kernels", audios=B, heads=n_heads, tokens=T, frames=TA, dtw_rows=n_rows[0],
                   probs_MB=round(B * n_heads * T * TA * 4 / 1e6, 1), torch_matches=list(map(bool, same)), dtw_host_numpy_ms=round(host_ms, 1),
                   note="ms per call, median of alternating rounds; attn_probs = the 5 launches of one pass; dtw_host = copy + numpy wavefront, one run")
        for n, (med, mn, spread) in res.items():
            rec[n + "_ms"] = round(med, 3)
            rec[n + "_min_ms"] = round(mn, 3)
            rec[n + "_spread"] = round(spread, 3)
        rec["attn_probs_write_TBps"] = round(B * n_heads * T * TA * 4 / (res["attn_probs"][0] * 1e-3) / 1e12, 3)
        rec["align_matrix_read_TBps"] = round(B * n_heads * T * TA * 4 / (res["align_matrix"][0] * 1e-3) / 1e12, 3)
        rec["dtw_us_per_wavefront_step"] = round(res["dtw"][0] * 1e3 / (n_rows[0] + TA - 1), 3)
        emit(rec)
        del qs, kvs, probs, matrix
    m, dims = _random_large_v3()
    mask = torch.zeros(dims.n_text_layer, dims.n_text_head, dtype=torch.bool)
    for i in range(n_heads // 2):
        mask[10 + 4 * i, [3 + 2 * i, 11 + i]] = True
    m.set_alignment_heads(mask)
    with torch.no_grad():  # the cross query / key weights of the alignment layers scaled up to a score deviation of about 2
        for i in range(n_heads // 2):
            ca = m.decoder.blocks[10 + 4 * i].cross_attn
            ca.query.weight.mul_(5.0); ca.key.weight.mul_(5.0)
    eot, kw = 50257, dict(sot_sequence=[50258, 50259, 50360], no_timestamps=50364, eot=50257, num_frames=frames)
    for B in batches:
        mel = torch.randn(B, dims.n_mels, frames, device=DEV, generator=g) * 0.5
        texts = [torch.randint(0, eot, (T - 5,), generator=torch.Generator().manual_seed(b)).tolist() for b in range(B)]
        fwd_tokens = torch.tensor([kw["sot_sequence"] + [kw["no_timestamps"]] + t + [eot] for t in texts], device=DEV)
        for _ in range(2):
            m.find_alignment(mel, texts, **kw)
        ts, tf = [], []
        for _ in range(rounds):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            m.find_alignment(mel, texts, **kw)
            torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            with torch.no_grad():
                m.decoder.hidden(fwd_tokens, m.embed_audio(mel))
            torch.cuda.synchronize(); tf.append((time.perf_counter() - t0) * 1e3)
        emit(dict(part="align", what="find_alignment", audios=B, heads=n_heads, tokens=T, frames=TA, find_alignment_ms=round(statistics.median(ts), 2),
                  find_alignment_min_ms=round(min(ts), 2), encoder_plus_decoder_pass_ms=round(statistics.median(tf), 2),
                  note="wall ms per call, host work included; beside it the teacher-forced encoder + decoder pass alone"))


def bench_transcribe(batches, seconds=95, sample_len=32, rounds=3):
    """Whisper.transcribe over ragged noise recordings at large-v3 dimensions, and the two kernels of csrc/transcribe.hip alone."""
    from whisper_finetune.data.gpu_frontend import mel_filters
    from whisper_finetune.engine import decode as Dm
    from whisper_finetune.engine import transcribe as Tm

    m, dims = _random_large_v3()
    filters = mel_filters(dims.n_mels).to(DEV)
    langs = list(range(50259, 50359))
    kw = dict(sot_sequence=[50258, 50259, 50360], eot=50257, language_tokens=langs, temperatures=(0.0,), sample_len=sample_len,
              logprob_threshold=None, no_speech_threshold=None, filters=filters)
    for B in batches:
        g = torch.Generator().manual_seed(B)
        audios = [torch.randn((seconds - 7 * a) * Tm.SAMPLE_RATE + 53 * a, generator=g) * 0.1 for a in range(B)]
        audio_s = sum(a.numel() for a in audios) / Tm.SAMPLE_RATE
        spent = {"decode": 0.0}

        def decode(*args, **kws):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = Dm.decode_with_fallback(*args, **kws)
            torch.cuda.synchronize(); spent["decode"] += time.perf_counter() - t0
            return res

        m.transcribe(audios, **kw)  # warm-up
        wall, dec, windows, iters = [], [], 0, 0
        for _ in range(rounds):
            spent["decode"] = 0.0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = m.transcribe(audios, _decode=decode, **kw)
            torch.cuda.synchronize(); wall.append(time.perf_counter() - t0); dec.append(spent["decode"])
            windows, iters = sum(r["windows"] for r in res), max(r["windows"] for r in res)
        packed = Tm.pack_logmels(audios, filters)
        rows, seeks = list(range(B)), [0] * B
        logits = torch.randn(B, K.round_up(dims.n_vocab, 128), device=DEV).to(BF)
        res = ab({"mel_windows": lambda: packed.windows(rows, seeks), "lang_probs": lambda: K.lang_probs(logits, dims.n_vocab, langs),
                  "long_logmel": lambda: Tm.long_logmel(audios[0], filters)}, rounds=5, iters=4)
        med = statistics.median(wall)
        kernels_ms = iters * res["mel_windows"][0] + res["lang_probs"][0]
        rec = dict(part="transcribe", recordings=B, audio_s=round(audio_s, 1), windows=windows, iterations=iters, sample_len=sample_len,
                   wall_s=round(med, 3), wall_min_s=round(min(wall), 3), windows_per_s=round(windows / med, 2), audio_s_per_s=round(audio_s / med, 1),
                   decode_share=round(statistics.median(dec) / med, 4), kernels_share=round(kernels_ms * 1e-3 / med, 6),
                   mel_windows_TBps=round(2 * B * dims.n_mels * 3000 * 4 / (res["mel_windows"][0] * 1e-3) / 1e12, 3),
                   note="wall s per transcribe() call, host work and the long log-mels included; kernels_share = iterations x mel_windows + "
                        "one lang_probs, timed alone (upload of the row tables included), over the wall time")
        for n, (mm, mn, spread) in res.items():
            rec[n + "_ms"] = round(mm, 4)
            rec[n + "_min_ms"] = round(mn, 4)
            rec[n + "_spread"] = round(spread, 3)
        emit(rec)


def bench_resample(batches):
    """wft_resample_f32: ms per call and achieved bytes/s against the read-once, write-once byte count."""
    from whisper_finetune.data.gpu_frontend import resample_taps

    for rate in (48000, 44100):
        _, o, n, width = resample_taps(rate, 16000)
        for name, B, n_in in (("10 min recording", 1, 600 * rate), ("[32, 30 s] batch", 32, 30 * rate)):
            g = torch.Generator().manual_seed(rate + B)
            x = (torch.randn(B, n_in, generator=g) * 0.1).to(DEV)
            out = K.resample(x, rate, 16000)
            n_out = out.shape[1]
            res = ab({"resample": lambda: K.resample(x, rate, 16000, out=out), "copy": lambda: out.copy_(x[:, :n_out])}, rounds=7, iters=20)
            nbytes = 4 * B * (n_in + n_out)
            med, mn, spread = res["resample"]
            emit(dict(part="resample", shape=name, orig=rate, new=16000, o=o, n=n, taps=2 * width, tile=L.load().wft_resample_tile(o, n, width),
                      B=B, n_in=n_in, n_out=n_out, bytes=nbytes, ms=round(med, 4), min_ms=round(mn, 4), spread=round(spread, 3),
                      TBps=round(nbytes / (med * 1e-3) / 1e12, 3), share_of_hbm=round(nbytes / (med * 1e-3) / HBM, 3),
                      copy_ms=round(res["copy"][0], 4), copy_TBps=round(8 * B * n_out / (res["copy"][0] * 1e-3) / 1e12, 3),
                      note="ms per K.resample call into a preallocated output; bytes = 4 * B * (n_in + n_out), the table not counted; "
                           "copy = torch's copy of n_out samples per row from the same buffer, for the launch floor at this size"))


def bench_stretch(batches):
    """K.time_stretch + K.logmel_ragged against K.logmel on 30 s clips, and the three stages of the stretch alone."""
    import numpy as np

    from whisper_finetune.data.gpu_frontend import mel_filters

    filt = mel_filters(80).to(DEV)
    lib = L.load()
    n = 480000
    for B in (32, 96):
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, n, generator=g) * 0.1).to(DEV)
        x[:, 300000:] = 0  # zero-padded clips, as the loader stages them
        keep = torch.full((B,), 3000, dtype=torch.int32, device=DEV)
        for name, rates in (("uniform [0.75, 1.25]", np.random.default_rng(B).uniform(0.75, 1.25, B)), ("all 0.5", np.full(B, 0.5))):
            rate_lo = float(rates.min())

            def stretched():
                out, n_out = K.time_stretch(x, rates)
                return K.logmel_ragged(out, n_out, keep, filt, 3000)

            res = ab({"stretch+ragged": stretched, "stretch": lambda: K.time_stretch(x, rates), "logmel": lambda: K.logmel(x, filt, 3000)},
                     rounds=5, iters=3)
            # the stages alone, on one chunk of rows that fits the wrapper's workspace cap
            per_row = lib.wft_time_stretch_workspace_bytes(1, n, rate_lo)
            nb = max(1, min(B, K.STRETCH_WORKSPACE_CAP // per_row))
            F, T_max = 1 + n // 512, int(np.ceil((1 + n // 512) / rate_lo))
            ws = torch.empty(nb * per_row, dtype=torch.uint8, device=DEV)
            Dp, Sp = ws.data_ptr(), ws.data_ptr() + nb * F * 1025 * 8
            rd = torch.from_numpy(rates[:nb].copy()).to(DEV)
            out = torch.zeros(nb, int(round(n / rate_lo)), device=DEV)
            n_out = torch.empty(nb, dtype=torch.int32, device=DEV)
            p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            stages = ab({"stft": lambda: lib.wft_stretch_stft_f32(p(x), n, n, C.c_void_p(Dp), nb, L.stream_ptr()),
                         "vocoder": lambda: lib.wft_stretch_vocoder_f32(C.c_void_p(Dp), n, p(rd), rate_lo, C.c_void_p(Sp), nb, L.stream_ptr()),
                         "istft": lambda: lib.wft_stretch_istft_f32(C.c_void_p(Sp), n, p(rd), rate_lo, p(out), out.stride(0), p(n_out), nb,
                                                                   L.stream_ptr())}, rounds=5, iters=3)
            emit(dict(part="stretch", B=B, rates=name, rate_lo=round(rate_lo, 4), rows_per_launch=nb, workspace_MB=round(nb * per_row / 1e6, 1),
                      stretch_ragged_ms=round(res["stretch+ragged"][0], 3), stretch_ms=round(res["stretch"][0], 3), logmel_ms=round(res["logmel"][0], 3),
                      added_ms=round(res["stretch+ragged"][0] - res["logmel"][0], 3), spread=round(res["stretch+ragged"][2], 3),
                      stage_ms={k: round(v[0], 3) for k, v in stages.items()}, stage_rows=nb, T_max=T_max,
                      note="ms per call, medians of alternating rounds; stretch_ms includes the wrapper's allocations (workspace, zeroed "
                           "output) and its chunking; stage_ms are the three stages alone on stage_rows rows (the istft stage on spectra "
                           "it has already overwritten: the same work)"))


def bench_filter(batches):
    """wft_sos_filter_f32 on 30 s clips: ms per call and achieved bytes/s against the 12 bytes per sample of its three passes."""
    import numpy as np

    from whisper_finetune.data.filters import design

    lib = L.load()
    n = 480000
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    # gains <= 1, so that the in-place arm can filter its own output again and again without leaving the float32 range
    filters = {1: design("peaking", center_freq=1000.0, gain_db=-6.0, q=1.0), 4: design("band_pass", center_freq=1000.0, bandwidth_fraction=1.0, order=4)}
    for B in (32, 96):
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, n, generator=g) * 0.1).to(DEV)
        x[:, 300000:] = 0  # zero-padded clips, as the loader stages them
        out, y = torch.empty_like(x), x.clone()
        for S, sos in filters.items():
            assert sos.shape[0] == S
            sos_h = np.ascontiguousarray(np.broadcast_to(sos, (B, S, 6)))
            sos_d = torch.from_numpy(sos_h).to(DEV)
            need = lib.wft_sos_filter_workspace_bytes(B, n, S)
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            raw = lambda src, dst: lib.wft_sos_filter_f32(p(src), n, None, n, p(sos_d), S, p(dst), n, p(ws), need, B, L.stream_ptr())  # noqa: E731
            res = ab({"out_of_place": lambda: raw(x, out), "in_place": lambda: raw(y, y), "wrapper": lambda: K.sos_filter(x, sos_h, out=out),
                      "copy": lambda: out.copy_(x)}, rounds=7, iters=10)
            nbytes = 12 * B * n
            rec = dict(part="filter", B=B, n=n, S=S, chunk=lib.wft_sos_filter_chunk(), group=lib.wft_sos_filter_group(), bytes=nbytes,
                       workspace_MB=round(need / 1e6, 2),
                       note="ms per call, medians of alternating rounds; out_of_place / in_place: the raw call on a preallocated workspace; "
                            "wrapper: K.sos_filter with host coefficients (its check, their upload and the workspace allocation included); "
                            "bytes = 12 per sample (two reads, one write); copy = torch's copy of the batch, 8 bytes per sample")
            for name, (med, mn, spread) in res.items():
                rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_spread"] = round(med, 4), round(mn, 4), round(spread, 3)
            rec["TBps"] = round(nbytes / (res["out_of_place"][0] * 1e-3) / 1e12, 3)
            rec["share_of_hbm"] = round(nbytes / (res["out_of_place"][0] * 1e-3) / HBM, 3)
            emit(rec)


def bench_wavefx(batches):
    """wft_wave_fx_f32 on 30 s clips, stage by stage and kind by kind: ms per call with every row active and with the expected
    number of active rows at the default rates (data/wave_fx.py: noise 0.15, clipping 0.6 / 9 * 0.8, level 0.225 * 2.5 / 3)."""
    from whisper_finetune.data import wave_fx as WF
    from whisper_finetune.data.gpu_frontend import mel_filters

    lib = L.load()
    n = 480000
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    kinds = {"gaussian_noise": dict(amplitude=0.001, seed=1), "gaussian_snr": dict(snr_db=30.0, seed=2), "clipping": dict(q=10),
             "gain": dict(gain_db=0.0), "gain_transition": dict(start_db=-1.0, end_db=1.0, t0=1000, length=48000),
             "shift": dict(fraction=0.25, fade_len=80)}
    share = {"noise": 0.15, "clip": 0.6 / 9 * 0.8, "level": 0.225 * 2.5 / 3}
    filters = mel_filters(80).to(DEV)
    for B in (32, 96):
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, n, generator=g) * 0.1).to(DEV)
        x[:, 300000:] = 0  # zero-padded clips, as the loader stages them
        out, y = torch.empty_like(x), x.clone()
        base = ab({"logmel": lambda: K.logmel(x, filters, 3000), "copy": lambda: out.copy_(x)}, rounds=5, iters=5)
        emit(dict(part="wavefx", arm="context", B=B, n=n, logmel_ms=round(base["logmel"][0], 4), copy_ms=round(base["copy"][0], 4),
                  note="the log-mel of the same batch and torch's copy of it (8 bytes per sample), for scale"))
        for kind, params in kinds.items():
            stage = WF.STAGE_OF[kind]
            sid = WF.STAGE_ID[stage]
            need = lib.wft_wave_fx_workspace_bytes(B, n, sid)
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            arms, active = {}, {"all": B, "default_rates": max(int(round(share[stage] * B)), 1)}
            keep = []
            for name, rows in active.items():
                table = WF.none_table(B)
                table[:rows] = WF.table_row(kind, **params)
                rec = WF.check_records(WF.records_from_table(table))
                fx = torch.from_numpy(rec.view("u1").reshape(B, 88).copy()).to(DEV)
                keep.append(fx)
                dst = out if kind == "shift" else y  # the loader runs in place; a shift cannot
                arms[name] = (lambda fx=fx, dst=dst, src=(x if kind == "shift" else y):
                              lib.wft_wave_fx_f32(p(src), n, None, n, p(fx), sid, p(dst), n, p(ws), need, B, L.stream_ptr()))
            table = WF.none_table(B)
            table[:] = WF.table_row(kind, **params)
            arms["wrapper_all"] = lambda table=table: K.wave_fx(y, table, stage, out=y)
            y.copy_(x)
            res = ab(arms, rounds=7, iters=10)
            rec = dict(part="wavefx", arm="stage", B=B, n=n, stage=stage, kind=kind, in_place=kind != "shift", tile=lib.wft_wave_fx_tile(),
                       rows_default_rates=active["default_rates"], workspace_MB=round(need / 1e6, 2),
                       note="ms per call, medians of 7 alternating rounds of 10 calls; all / default_rates: the raw call on a preallocated "
                            "workspace with every row active / with the expected number of active rows at the default rates; "
                            "wrapper_all: K.wave_fx with a host table (its check, the upload, the workspace allocation; a shift goes "
                            "through its temporary)")
            for name, (med, mn, spread) in res.items():
                rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_spread"] = round(med, 4), round(mn, 4), round(spread, 3)
            rec["all_vs_logmel"] = round(res["all"][0] / base["logmel"][0], 3)
            emit(rec)


def bench_rate(batches):
    """K.alias, K.sinc_resample_rows and gpu_frontend.pitch_shift on 30 s clips with every row active: ms per call beside the log-mel
    and torch's copy of the same batch."""
    import numpy as np

    from whisper_finetune.data.gpu_frontend import mel_filters, pitch_rates, pitch_shift
    from whisper_finetune.data.rate_fx import hz_to_mel, mel_to_hz

    lib = L.load()
    n = 480000
    filters = mel_filters(80).to(DEV)
    for B in (32, 96):
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, n, generator=g) * 0.1).to(DEV)
        x[:, 300000:] = 0  # zero-padded clips, as the loader stages them
        out = torch.empty_like(x)
        rates = np.array([mel_to_hz(m) for m in np.linspace(hz_to_mel(8000.0), hz_to_mel(16000.0), B)])
        semis = np.linspace(-4.0, 4.0, B)
        ratios = pitch_rates(semis, B)
        n_in = torch.full((B,), n, dtype=torch.int32, device=DEV)
        res = ab({"alias": lambda: K.alias(x, rates), "sinc_resample_rows": lambda: K.sinc_resample_rows(x, n_in, ratios, n),
                  "pitch_shift": lambda: pitch_shift(x, semis), "logmel": lambda: K.logmel(x, filters, 3000), "copy": lambda: out.copy_(x)},
                 rounds=5, iters=5)
        rec = dict(part="rate", B=B, n=n, alias_tile=lib.wft_alias_tile(), sinc_tile=lib.wft_sinc_resample_rows_tile(float(ratios.min())),
                   ratio_lo=round(float(ratios.min()), 4),
                   note="ms per call, medians of 5 alternating rounds of 5 calls, every row active; alias / sinc_resample_rows: the wrappers "
                        "(host check, upload of the per-row values, output allocation); pitch_shift = K.time_stretch + K.sinc_resample_rows; "
                        "logmel / copy: the log-mel of the same batch and torch's copy of it, for scale")
        for name, (med, mn, spread) in res.items():
            rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_spread"] = round(med, 4), round(mn, 4), round(spread, 3)
        emit(rec)


def bench_office(batches):
    """K.fir_conv at 1, 2 and 8 partitions and K.bitcrush on 30 s clips with every row active: ms per call beside the log-mel, the
    time stretch's STFT stage and torch's copy of the same batch."""
    from whisper_finetune.data.gpu_frontend import mel_filters

    lib = L.load()
    n = 480000
    filters = mel_filters(80).to(DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for B in (32, 96):
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, n, generator=g) * 0.1).to(DEV)
        x[:, 300000:] = 0  # zero-padded clips, as the loader stages them
        out = torch.empty_like(x)
        depths = torch.randint(6, 15, (B,), generator=g).to(torch.int32).to(DEV)
        irs = {P: (torch.randn(B, taps, generator=g) / taps ** 0.5).to(DEV) for P, taps in ((1, 1000), (2, 2000), (8, 8192))}
        D = torch.empty(B * (1 + n // 512) * 1025 * 2, device=DEV)  # the STFT of the stretch: 938 frames of 2048 per clip
        arms = {f"fir_conv_P{P}": (lambda h: lambda: K.fir_conv(x, h))(h) for P, h in irs.items()}
        arms.update({"bitcrush": lambda: K.bitcrush(x, depths, out=out), "bitcrush_in_place": lambda: K.bitcrush(out, depths, out=out),
                     "stretch_stft": lambda: lib.wft_stretch_stft_f32(p(x), n, n, p(D), B, L.stream_ptr()),
                     "logmel": lambda: K.logmel(x, filters, 3000), "copy": lambda: out.copy_(x)})
        res = ab(arms, rounds=5, iters=5)
        rec = dict(part="office", B=B, n=n, block=lib.wft_fir_conv_block(), taps={str(P): int(h.shape[1]) for P, h in irs.items()},
                   ffts_per_clip={"fir_conv_P1": 469 * 2 + 1, "fir_conv_P2": 469 * 3 + 2, "fir_conv_P8": 469 * 9 + 8, "stretch_stft": 938},
                   note="ms per call, medians of 5 alternating rounds of 5 calls, every row active; fir_conv_P*: the wrapper (output and "
                        "workspace allocation, both passes) at 1000 / 2000 / 8192 taps; ffts_per_clip: 2048-point FFTs per clip — a block "
                        "of 1024 outputs costs one forward FFT per live partition plus one inverse; stretch_stft: wft_stretch_stft_f32 "
                        "alone; logmel / copy: the log-mel of the same batch and torch's copy of it, for scale")
        for name, (med, mn, spread) in res.items():
            rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_spread"] = round(med, 4), round(mn, 4), round(spread, 3)
        emit(rec)


def bench_mix(batches):
    """K.loudness (measure only, normalise) and K.bg_mix (snr, absolute) on 30 s clips with every row active: ms per call beside
    K.sos_filter at two sections, the log-mel and torch's copy of the same batch."""
    import numpy as np

    from whisper_finetune.data import mix_fx as MF
    from whisper_finetune.data.gpu_frontend import mel_filters

    n = 480000
    filters = mel_filters(80).to(DEV)
    entries = MF.synthetic_bank(4)
    bank_h, off_h = MF.pack_bank(entries)
    bank, off = torch.from_numpy(bank_h).to(DEV), torch.from_numpy(off_h).to(DEV)
    lengths = [int(e.shape[0]) for e in entries]
    sos = torch.from_numpy(MF.k_weighting(16000))
    for B in (32, 96):
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, n, generator=g) * 0.1).to(DEV)
        x[:, 300000:] = 0  # zero-padded clips, as the loader stages them
        work, out = x.clone(), torch.empty_like(x)
        targets = np.linspace(-31.0, -13.0, B)
        rec = {}
        for name, kind in (("snr", 1), ("absolute", 2)):
            r = np.zeros(B, dtype=MF.RECORD_DTYPE)
            r["kind"], r["entry"] = kind, np.arange(B) % 4
            r["offset"] = np.where(r["entry"] == 2, 16000 * np.arange(B) // B, 0)  # the one entry that is longer than a clip
            r["db"] = np.linspace(2.0, 4.0, B) if kind == 1 else np.linspace(-30.0, -10.0, B)
            rec[name] = r
        # in place the batch changes from call to call (a gain, added noise); the work per call does not: every row stays active
        arms = {"loudness_measure": lambda: K.loudness(x, 16000),
                "loudness_normalize": lambda: K.loudness(x, 16000, targets, out=out),
                "loudness_normalize_in_place": lambda: K.loudness(work, 16000, targets, out=work),
                "bg_mix_snr": lambda: K.bg_mix(x, bank, off, rec["snr"], out=out, lengths=lengths),
                "bg_mix_absolute": lambda: K.bg_mix(x, bank, off, rec["absolute"], out=out, lengths=lengths),
                "bg_mix_snr_in_place": lambda: K.bg_mix(work, bank, off, rec["snr"], out=work, lengths=lengths),
                "sos_filter_S2": lambda: K.sos_filter(x, sos, out=out),
                "logmel": lambda: K.logmel(x, filters, 3000), "copy": lambda: out.copy_(x)}
        res = ab(arms, rounds=5, iters=5)
        out_rec = dict(part="mix", B=B, n=n, bank_entries=lengths,
                       note="ms per call, medians of 5 alternating rounds of 5 calls, every row active; loudness_*: the K.loudness wrapper "
                            "(workspace and stats allocation, the K-weighting design, local / scan / energy / gate launches, plus the apply "
                            "pass when it normalises); bg_mix_*: the K.bg_mix wrapper (record upload, sumsq / scale / mix launches); "
                            "sos_filter_S2: K.sos_filter with the K-weighting's two sections, the same recurrence with its outputs stored; "
                            "logmel / copy: the log-mel of the same batch and torch's copy of it, for scale")
        for name, (med, mn, spread) in res.items():
            out_rec[name + "_ms"], out_rec[name + "_min_ms"], out_rec[name + "_spread"] = round(med, 4), round(mn, 4), round(spread, 3)
        emit(out_rec)


def bench_pcm(batches):
    """wft_pcm_decode_f32 on 32 and 96 clips of 30 s, as S16LE stereo at 48 kHz and as u-law mono at 8 kHz: ms per call of the decode
    launch beside a device-to-device copy that moves the same number of bytes (in plus out), decode + resample beside resample
    alone, and the host path it replaces (numpy convert + downmix, then the host-to-device copy of f32) as wall time."""
    import numpy as np

    from whisper_finetune.data import audio_io as AIO

    lib = L.load()
    ulaw = np.zeros(256, dtype=np.float32)
    for code in range(256):
        u = ~code & 0xFF
        t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
        ulaw[code] = ((0x84 - t) if u & 0x80 else (t - 0x84)) / 32768.0
    for fmt, ch, rate in (("s16le", 2, 48000), ("ulaw", 1, 8000)):
        frames = 30 * rate
        fb = ch * AIO.SAMPLE_BYTES[AIO.FORMAT_ID[fmt]]
        for B in (32, 96):
            rng = np.random.default_rng(B)
            host = rng.integers(0, 256, B * frames * fb, dtype=np.uint8)
            raw = torch.from_numpy(host).to(DEV)
            rows = [(b * frames * fb, frames, ch, fmt, "mean") for b in range(B)]
            rec, n_max = AIO.pcm_rows(rows, int(raw.numel()))
            table = torch.from_numpy(rec.view("u1").reshape(B, 32).copy()).to(DEV)
            out = torch.empty((B, frames), dtype=torch.float32, device=DEV)
            traffic = int(raw.numel()) + out.numel() * 4
            a = torch.empty(traffic // 2, dtype=torch.uint8, device=DEV)
            c = torch.empty_like(a)
            res16 = K.resample(out, rate, 16000)

            def launch():
                L.check(lib.wft_pcm_decode_f32(C.c_void_p(raw.data_ptr()), int(raw.numel()), C.c_void_p(table.data_ptr()), C.c_void_p(out.data_ptr()),
                                               frames, frames, B, L.stream_ptr()), "wft_pcm_decode_f32")

            arms = {"decode": launch, "decode_wrapper": lambda: K.pcm_decode(raw, rec, n_max, out=out), "copy_same_bytes": lambda: c.copy_(a),
                    "decode_resample": lambda: (launch(), K.resample(out, rate, 16000, out=res16)),
                    "resample": lambda: K.resample(out, rate, 16000, out=res16)}
            res = ab(arms, rounds=5, iters=5)

            def host_path():
                t0 = time.perf_counter()
                clips = []
                for b in range(B):
                    seg = host[b * frames * fb:(b + 1) * frames * fb]
                    if fmt == "s16le":
                        clips.append((seg.view("<i2").reshape(frames, ch).astype(np.float32) / 32768.0).mean(axis=1))
                    else:
                        clips.append(ulaw[seg])
                t1 = time.perf_counter()
                d = torch.from_numpy(np.stack(clips)).to(DEV)
                torch.cuda.synchronize()
                return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, d

            host_path()
            conv_ms, h2d_ms, _ = host_path()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.from_numpy(host).to(DEV)
            torch.cuda.synchronize()
            raw_h2d_ms = (time.perf_counter() - t0) * 1e3
            out_rec = dict(part="pcm", format=fmt, channels=ch, rate=rate, B=B, frames=frames, raw_bytes=int(raw.numel()), out_bytes=out.numel() * 4,
                           note="ms per call, medians of 5 alternating rounds of 5 calls; decode: the wft_pcm_decode_f32 launch on a table that is "
                                "already on the device; decode_wrapper: K.pcm_decode (host row checks and the table upload included); copy_same_bytes: "
                                "torch's device-to-device copy of (raw_bytes + out_bytes) / 2 bytes, which reads and writes as many bytes as the decode; "
                                "*_gbps: (raw_bytes + out_bytes) / time; host_*: the path this replaces, wall time of one pass on the host's CPU "
                                "(numpy convert + downmix per clip in float32, then stack + pageable host-to-device copy of the f32 batch); raw_h2d: "
                                "the pageable host-to-device copy of the file bytes, which the device path pays instead")
            for name, (med, mn, spread) in res.items():
                out_rec[name + "_ms"], out_rec[name + "_min_ms"], out_rec[name + "_spread"] = round(med, 4), round(mn, 4), round(spread, 3)
            out_rec["decode_gbps"] = round(traffic / (res["decode"][0] * 1e-3) / 1e9, 1)
            out_rec["copy_same_bytes_gbps"] = round(traffic / (res["copy_same_bytes"][0] * 1e-3) / 1e9, 1)
            out_rec["host_convert_ms"], out_rec["host_f32_h2d_ms"], out_rec["raw_h2d_ms"] = round(conv_ms, 1), round(h2d_ms, 1), round(raw_h2d_ms, 1)
            emit(out_rec)
            del raw, out, a, c, res16


def bench_edit(batches):
    """WER / CER scoring of P = 32 and P = 2 048 utterances of 20, 60 and 90 words (synthetic transcripts over a 2 000-word vocabulary,
    every 7th word of the hypothesis replaced): host_parent = metrics.wer + metrics.cer per pair, the Python Levenshtein loops the
    evaluator ran per utterance, as wall time on this machine's CPU; device = word_error_counts + char_error_counts on the GPU, packing
    and both copies included; kernel = the two wft_edit_counts_i32 launches alone on resident tables."""
    import numpy as np

    from whisper_finetune.eval import metrics as M

    lib = L.load()
    rng = np.random.default_rng(0)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    vocab = sorted({"".join(rng.choice(letters, size=int(rng.integers(3, 10)))) for _ in range(2400)})[:2000]
    HOST_PAIRS = 32  # the host loops cost the same per pair whatever P is: they are timed on 32 pairs and scaled to P

    def resident(refs, hyps):
        ids, flat, rows = {}, [], []
        for r, h in zip(refs, hyps):
            rows.append((len(flat), len(flat) + len(r), len(r), len(h)))
            flat.extend(ids.setdefault(x, len(ids)) for x in r)
            flat.extend(ids.setdefault(x, len(ids)) for x in h)
        rec, max_len = K.edit_rows(np.asarray(rows, dtype=np.int64), len(flat))
        sym = torch.tensor(flat, dtype=torch.int32, device=DEV)
        table = torch.from_numpy(rec.view("u1").reshape(len(rows), 32).copy()).to(DEV)
        out = torch.empty((len(rows), 4), dtype=torch.int32, device=DEV)
        return lambda: L.check(lib.wft_edit_counts_i32(C.c_void_p(sym.data_ptr()), int(sym.numel()), C.c_void_p(table.data_ptr()), C.c_void_p(out.data_ptr()),
                                                       4, len(rows), max_len, L.stream_ptr()), "wft_edit_counts_i32"), out

    for words in (20, 60, 90):
        host_ms = None
        for P in (32, 2048):
            prng = np.random.default_rng(words)
            refs, hyps = [], []
            for _ in range(P):
                r = [vocab[i] for i in prng.integers(0, len(vocab), size=words)]
                h = [vocab[int(prng.integers(0, len(vocab)))] if k % 7 == 6 else w for k, w in enumerate(r)]
                refs.append(" ".join(r))
                hyps.append(" ".join(h))
            chars = sum(len(r) for r in refs) / P
            if host_ms is None:  # (the first 32 pairs of both P are the same strings)
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    for r, h in zip(refs[:HOST_PAIRS], hyps[:HOST_PAIRS]):
                        M.wer(r, h)
                        M.cer(r, h)
                    ts.append((time.perf_counter() - t0) * 1e3)
                host_ms = statistics.median(ts)
            launch_w, out_w = resident([r.split() for r in refs], [h.split() for h in hyps])
            launch_c, out_c = resident([list(r.strip()) for r in refs], [list(h.strip()) for h in hyps])

            def device():
                return M.word_error_counts(hyps, refs, DEV), M.char_error_counts(hyps, refs, DEV)

            w, c = device()
            launch_w(), launch_c()
            assert np.array_equal(w, out_w.cpu().numpy()) and np.array_equal(c, out_c.cpu().numpy())
            for k in range(min(P, 4)):  # the device's integers give the parent's floats
                assert int(w[k, 1:].sum()) / int(w[k, :3].sum()) == M.wer(refs[k], hyps[k]) and int(c[k, 1:].sum()) / int(c[k, :3].sum()) == M.cer(refs[k], hyps[k])
            res = ab({"device": device, "kernel": lambda: (launch_w(), launch_c())}, rounds=5, iters=3)
            rec = dict(part="edit", words=words, chars=round(chars, 1), P=P, host_pairs_timed=HOST_PAIRS,
                       note="ms per batch of P utterances. host_parent: metrics.wer + metrics.cer per pair (the Python loops of the parent's evaluator), wall time "
                            "on this machine's CPU, median of 3 passes over 32 pairs, scaled by P / 32 (the loops cost the same per pair whatever P is); "
                            "device: word_error_counts + char_error_counts on the GPU — tokenising, the id dict, one packed host-to-device copy, one launch and "
                            "one copy back for each of the two; kernel: the two wft_edit_counts_i32 launches alone on resident tables; device and kernel: "
                            "medians of 5 alternating rounds of 3 calls")
            rec["host_parent_ms"] = round(host_ms * P / HOST_PAIRS, 2)
            for name, (med, mn, spread) in res.items():
                rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_spread"] = round(med, 4), round(mn, 4), round(spread, 3)
            rec["host_over_device"] = round(rec["host_parent_ms"] / res["device"][0], 1)
            emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="attn,gemm,e2e")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench.py measures on the GPU: no device found (there is no CPU fallback)")
    batches = [int(b) for b in a.batches.split(",")]
    emit(dict(part="env", device=torch.cuda.get_device_name(0), lib=L.load().wft_version().decode(), torch=torch.__version__))
    for part in a.parts.split(","):
        {"attn": bench_attn, "gemm": bench_gemm, "e2e": bench_e2e, "gemm_stream": lambda b: (bench_gemm_stream(b), bench_gemm_stream_q8(b)), "e2e_step": bench_e2e_step,
         "gemm_i8": bench_gemm_i8, "beam": bench_beam, "ts": bench_ts, "sample": bench_sample, "align": bench_align, "transcribe": bench_transcribe, "resample": bench_resample,
         "stretch": bench_stretch, "filter": bench_filter, "wavefx": bench_wavefx, "rate": bench_rate, "office": bench_office, "mix": bench_mix, "pcm": bench_pcm,
         "edit": bench_edit}[part](batches)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in OUT))


if __name__ == "__main__":
    main()
