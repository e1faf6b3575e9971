"""Multi-dataset evaluation (rank 0), same entry points as the reference's eval/evaluator.py:
evaluate_single_dataset (:29-131), evaluate_multiple_datasets (:134-183), log_metrics_to_wandb (:186-221).

The forward is the engine's teacher-forced pass.  Differences that do not change results: the per-token
reductions (argmax, NLL, log-prob, entropy, confidence) come from one fused kernel over the bf16 logits instead
of materialising fp32 [B, S, V] logits plus four softmax passes, predictions are copied to the host ONCE
per batch instead of once per sample, and WER / CER of the whole dataset come from one `wft_edit_counts_i32` launch
after the loader loop (jiwer per utterance in the reference), which also yields the substitution / deletion /
insertion counts and the corpus-level rates."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

import whisper_finetune.runtime as rt
from whisper_finetune.eval.metrics import (DatasetMetrics, PerUtteranceMetrics, aggregate_dataset_metrics, compute_macro_average,
                                           compute_token_metrics, edit_counts_batch, token_metrics_from_stats)
from whisper_finetune.eval.utils import VOCAB_SPECS, decode_prefix_len, normalize_text


def _default_tokenizer():
    try:
        from whisper.tokenizer import get_tokenizer  # openai-whisper, optional at eval time
    except ImportError as exc:  # pragma: no cover - depends on the environment
        raise RuntimeError("evaluation needs a tokenizer: pass `tokenizer=` or install openai-whisper") from exc
    return get_tokenizer(multilingual=True, language="de", task="transcribe")


def _batch_token_stats(model, x, y_in, y_out):
    """-> (argmax i64 [B,S], stats f32 [B,S,4]) on the host; fused kernel when the model is the engine's."""
    core = rt.unwrap_model(model)
    if hasattr(core, "decoder") and hasattr(core.decoder, "padded_logits") and x.is_cuda and getattr(core, "compute_dtype", "bf16") == "bf16":
        from whisper_finetune.engine import kernels as K

        h = core.decoder.hidden(y_in, core.encoder(x))
        padded = core.decoder.padded_logits(h)
        stats, am = K.token_stats(padded, y_out.reshape(-1), core.dims.n_vocab)
        B, S = y_in.shape
        return am.view(B, S).cpu().numpy(), stats.view(B, S, 4).cpu().numpy()
    return None


def _greedy_predictions(model, tokenizer, x, y_in, step: str = "eager", beam: dict = None, timestamps: bool = False,
                        fallback: dict = None, weights: str = "bf16") -> List[List[int]]:
    """t_config["wft_eval_decode"] = "greedy": every utterance's predicted ids from KV-cached greedy decoding
    (Whisper.greedy_decode) instead of the teacher-forced argmax.  The decoding prefix of a row is its y_in up to and including
    the start-of-transcript sequence; every special token but eot is suppressed (upstream's notimestamps decoding plus its
    SuppressTokens list of specials; `tokenizer.non_speech_tokens` too when the tokenizer has them), eot and the blank for a
    row's first token (upstream's SuppressBlank); at most n_text_ctx // 2 new tokens (upstream's sample_len).
    `step` is t_config["wft_eval_decode_step"]: "graph" = the captured step on the weight-streaming GEMMs (engine/decode/).
    `weights` is t_config["wft_eval_decode_weights"]: "int8" = those steps read int8 weights (weight-only; the WER of THIS int8 path);
    "w8a8" = in addition the encoder, the prefill and the cross key / value projections run int8 x int8 on per-row quantised activations
    (wft_gemm_nt_i8; engine/decode/ says what stays bf16).
    `beam` = {"beam_size", "patience"} (t_config["wft_eval_decode"] = "beam_search"): the same prefix, suppression and length rules
    through Whisper.beam_decode, the winning hypothesis of every utterance.
    `timestamps` (t_config["wft_eval_decode_timestamps"]): decode under upstream's timestamp rules, its command line's default mode —
    the prefix stops behind the task token (a `<|notimestamps|>` in y_in is not copied), the timestamp ids stay out of the
    suppress list and `timestamp_begin` / `no_timestamps` come from the tokenizer (max_initial_timestamp_index: the decoder's
    default, upstream's 1 s).  The returned ids still hold the timestamps; the caller strips them before WER / CER.
    `fallback` (t_config["wft_eval_decode"] = "fallback"): the keywords of Whisper.decode_with_fallback — upstream's temperature
    ladder, the decoding `transcribe()` runs — under the same prefix, suppression and length rules; `beam` then chooses the rung at
    temperature 0.  The compression ratio is taken over tokenizer.decode; a tokenizer with `no_speech` also supplies the no-speech
    probability (read at each row's start-of-transcript position)."""
    if fallback is not None and not hasattr(model, "decode_with_fallback"):
        raise RuntimeError('wft_eval_decode: "fallback" needs a model with decode_with_fallback (the engine\'s Whisper)')
    if fallback is None and beam is not None and not hasattr(model, "beam_decode"):
        raise RuntimeError('wft_eval_decode: "beam_search" needs a model with beam_decode (the engine\'s Whisper)')
    if fallback is None and beam is None and not hasattr(model, "greedy_decode"):
        raise RuntimeError('wft_eval_decode: "greedy" needs a model with greedy_decode (the engine\'s Whisper)')
    eot = int(tokenizer.eot)
    rows = y_in.cpu().tolist()
    plen = [decode_prefix_len(r, int(tokenizer.sot), int(tokenizer.no_timestamps), with_timestamps=timestamps) for r in rows]
    width = max(plen)
    prompt = torch.full((len(rows), width), eot, dtype=torch.int64)
    for i, (r, n) in enumerate(zip(rows, plen)):
        prompt[i, :n] = torch.tensor(r[:n], dtype=torch.int64)
    suppress = sorted((set(int(t) for t in tokenizer.special_tokens.values()) | set(int(t) for t in getattr(tokenizer, "non_speech_tokens", ()))) - {eot})
    blank = [int(t) for t in tokenizer.encode(" ")] if hasattr(tokenizer, "encode") else []
    n_ctx = getattr(getattr(model, "dims", None), "n_text_ctx", 448)
    kw = dict(eot=eot, max_len=min(n_ctx, width + n_ctx // 2), suppress=suppress, suppress_first=[eot] + blank,
              **({} if step == "eager" else {"step": step}), **({} if weights == "bf16" else {"weights": weights}))
    if timestamps:
        ts_begin = int(tokenizer.timestamp_begin)
        kw["suppress"] = [t for t in suppress if t < ts_begin]
        kw.update(timestamp_begin=ts_begin, no_timestamps=int(tokenizer.no_timestamps))
    if fallback is not None:
        fb = dict(fallback, text_of=tokenizer.decode, **({} if beam is None else beam))
        if hasattr(tokenizer, "no_speech"):
            sot = int(tokenizer.sot)
            fb.update(no_speech=int(tokenizer.no_speech), sot_index=[r[:n].index(sot) if sot in r[:n] else 0 for r, n in zip(rows, plen)])
        tokens, lengths, _, _ = model.decode_with_fallback(x, prompt.to(x.device), torch.tensor(plen), **fb, **kw)
    elif beam is None:
        tokens, lengths, _ = model.greedy_decode(x, prompt.to(x.device), torch.tensor(plen), **kw)
    else:
        tokens, lengths, _ = model.beam_decode(x, prompt.to(x.device), torch.tensor(plen), beam_size=beam["beam_size"],
                                               patience=beam["patience"], **kw)
    tokens, lengths = tokens.cpu().tolist(), lengths.cpu().tolist()
    return [tokens[i][plen[i]:lengths[i]] for i in range(len(rows))]


def _fallback_config(t_config: dict) -> dict:
    """The wft_eval_decode_* keys of the "fallback" mode -> keywords of Whisper.decode_with_fallback, validated before the loop.
    Defaults: upstream's six temperatures, best_of 5, thresholds -1.0 / 0.6 / 2.4 (null switches a test off), seed 0."""
    num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and v == v
    temps = t_config.get("wft_eval_decode_temperatures", [0.0, 0.2, 0.4, 0.6, 0.8, 1.0])
    if not isinstance(temps, (list, tuple)) or not temps or not all(num(t) and 0 <= t < float("inf") for t in temps):
        raise ValueError(f"wft_eval_decode_temperatures: a non-empty list of numbers >= 0, got {temps!r}")
    best_of = t_config.get("wft_eval_decode_best_of", 5)
    if isinstance(best_of, bool) or not isinstance(best_of, int) or not 1 <= best_of <= 8:
        raise ValueError(f"wft_eval_decode_best_of: an integer in [1, 8], got {best_of!r}")
    out = {"temperatures": tuple(float(t) for t in temps), "best_of": best_of}
    for key, default in (("logprob_threshold", -1.0), ("no_speech_threshold", 0.6), ("compression_ratio_threshold", 2.4)):
        v = t_config.get("wft_eval_decode_" + key, default)
        if v is not None and not num(v):
            raise ValueError(f"wft_eval_decode_{key}: a number or null, got {v!r}")
        out[key] = v
    seed = t_config.get("wft_eval_decode_seed", 0)
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"wft_eval_decode_seed: an integer, got {seed!r}")
    out["seed"] = seed
    return out


def _score_utterances(pending, device) -> List[PerUtteranceMetrics]:
    """WER / CER and the error counts of a whole dataset from its normalised (prediction, reference) pairs: the word pairs and the
    character pairs of every utterance go through ONE edit_counts_batch call — on a GPU one packed copy, one wft_edit_counts_i32
    launch and one copy back instead of two Python Levenshtein loops per utterance; a model on the CPU takes the host function.
    wer = (S + D + I) / (H + S + D): the integers metrics.wer divides, so the floats are the same bits.  An utterance whose normalised
    reference is empty scores 0.0, carries no counts and stays out of the corpus totals."""
    scored = [k for k, (_, ref, *_rest) in enumerate(pending) if ref]
    for k in scored:
        if not pending[k][1].split():
            raise ValueError("one or more references are empty strings")  # what metrics.wer says of a blank reference
    refs = [pending[k][1].split() for k in scored] + [list(pending[k][1].strip()) for k in scored]
    hyps = [pending[k][0].split() for k in scored] + [list(pending[k][0].strip()) for k in scored]
    counts = edit_counts_batch(refs, hyps, device).tolist() if scored else []
    at = {k: (tuple(counts[q]), tuple(counts[len(scored) + q])) for q, k in enumerate(scored)}
    out = []
    for k, (pred_n, true_n, nll, lp, ent, conf, ok) in enumerate(pending):
        if k in at:
            (wh, ws, wd, wi), (ch, cs, cd, ci) = at[k]
            out.append(PerUtteranceMetrics(pred_n, true_n, (ws + wd + wi) / (wh + ws + wd), (cs + cd + ci) / (ch + cs + cd), nll, lp, ent, conf, ok,
                                           word_counts=at[k][0], char_counts=at[k][1]))
        else:
            out.append(PerUtteranceMetrics(pred_n, true_n, 0.0, 0.0, nll, lp, ent, conf, ok))
    return out


@torch.no_grad()
def evaluate_single_dataset(model, dataloader, dataset_name: str, t_config: dict, tokenizer=None) -> DatasetMetrics:
    model = rt.unwrap_model(model)
    model.eval()
    device = next(model.parameters()).device
    mixed = t_config.get("mixed_precision_training", True)
    from whisper_finetune.engine.whisper_model import Whisper as _EngineWhisper, check_amp_request

    mp_dtype = t_config.get("mp_dtype", "fp16")
    if mixed and mp_dtype == "fp16" and isinstance(model, _EngineWhisper):
        # the reference's evaluator accepts a minimal config (mp_dtype defaults to fp16, every shipped YAML says fp16): on the
        # engine that means bf16 autocast, said once — the same rewrite scripts/finetune.resolve_precision makes for training
        rt.print_once("WARNING: evaluation with mp_dtype: fp16 -> bf16 autocast on MI355X (the libwft engine computes in bf16; "
                      "set mp_dtype: bf16 to silence this)")
        mp_dtype = "bf16"
    amp_dtype = torch.float16 if mp_dtype == "fp16" else torch.bfloat16
    check_amp_request(model, mixed, mp_dtype)
    if tokenizer is None:
        tokenizer = _default_tokenizer()
    specials = set(tokenizer.special_tokens.values())
    spec = VOCAB_SPECS["v0"]
    pending = []  # (prediction, reference, the five token statistics) per utterance: WER / CER are scored once, after the loop
    decode_mode = t_config.get("wft_eval_decode")
    if decode_mode not in (None, "greedy", "beam_search", "fallback"):
        raise ValueError(f'wft_eval_decode: "greedy", "beam_search" or "fallback" (absent = the teacher-forced argmax), got {decode_mode!r}')
    beam = None
    if decode_mode == "beam_search" or (decode_mode == "fallback" and ("wft_eval_decode_beam_size" in t_config or "wft_eval_decode_patience" in t_config)):
        beam = {"beam_size": t_config.get("wft_eval_decode_beam_size", 5), "patience": t_config.get("wft_eval_decode_patience", 1.0)}
        bs, pat = beam["beam_size"], beam["patience"]
        if isinstance(bs, bool) or not isinstance(bs, int) or not 1 <= bs <= 8:
            raise ValueError(f"wft_eval_decode_beam_size: an integer in [1, 8], got {bs!r}")
        if isinstance(pat, bool) or not isinstance(pat, (int, float)) or not 0 < pat < float("inf") or round(bs * pat) < 1:
            raise ValueError(f"wft_eval_decode_patience: a positive number with round(beam_size * patience) >= 1, got {pat!r}")
    fallback = _fallback_config(t_config) if decode_mode == "fallback" else None
    decode_step = t_config.get("wft_eval_decode_step")
    if decode_step not in (None, "eager", "graph"):
        raise ValueError(f'wft_eval_decode_step: "eager" (the default) or "graph", got {decode_step!r}')
    decode_step = decode_step or "eager"
    decode_weights = t_config.get("wft_eval_decode_weights")
    if decode_weights not in (None, "bf16", "int8", "w8a8"):
        raise ValueError(f'wft_eval_decode_weights: "bf16" (the default), "int8" or "w8a8", got {decode_weights!r}')
    decode_weights = decode_weights or "bf16"
    if decode_weights in ("int8", "w8a8") and (decode_mode is None or decode_step != "graph"):
        raise ValueError(f'wft_eval_decode_weights: "{decode_weights}" (one of "bf16", "int8", "w8a8") needs wft_eval_decode and '
                         'wft_eval_decode_step: "graph" (only the captured steps run on the kernels that read int8 weights)')
    decode_ts = t_config.get("wft_eval_decode_timestamps", False)
    if not isinstance(decode_ts, bool):
        raise ValueError(f"wft_eval_decode_timestamps: true or false, got {decode_ts!r}")
    if decode_ts and decode_mode is None:
        raise ValueError('wft_eval_decode_timestamps: true needs wft_eval_decode: "greedy", "beam_search" or "fallback" (the teacher-forced argmax has no timestamp rules)')
    if decode_ts:
        ts_begin = int(tokenizer.timestamp_begin)

    for x, y_in, y_out in dataloader:
        x = x.to(device, non_blocking=True)
        y_in = y_in.to(device, non_blocking=True)
        y_out = y_out.to(device, non_blocking=True)
        with torch.autocast(device_type=device.type, enabled=mixed, dtype=amp_dtype):
            fused = _batch_token_stats(model, x, y_in, y_out)
            if fused is None:
                logits = model(x, y_in)
                pred = torch.argmax(logits, dim=-1)
        y_host = y_out.cpu().numpy()
        pred_host = fused[0] if fused is not None else pred.cpu().numpy()
        # prediction TEXT from autoregressive decoding when asked for; NLL / entropy / ECE below stay teacher-forced
        decoded = None
        if decode_mode is not None:
            decoded = _greedy_predictions(model, tokenizer, x, y_in, decode_step, beam, **({"timestamps": True} if decode_ts else {}),
                                          **({} if fallback is None else {"fallback": fallback}),
                                          **({} if decode_weights == "bf16" else {"weights": decode_weights}))
            if decode_ts:  # the timestamps go the way of the other specials before WER / CER
                decoded = [[t for t in row if t < ts_begin] for row in decoded]
        for i in range(y_host.shape[0]):
            pred_ids = pred_host[i].tolist() if decoded is None else decoded[i]
            pred_tokens = [t for t in pred_ids if t not in specials and t != -100]
            true_tokens = [t for t in y_host[i].tolist() if t not in specials and t != -100]
            true_text = tokenizer.decode(true_tokens)
            if true_text.strip() == "":
                continue  # empty references are skipped
            pred_n = normalize_text(tokenizer.decode(pred_tokens), **spec)
            true_n = normalize_text(true_text, **spec)
            if fused is not None:
                nll, lp, ent, conf, ok = token_metrics_from_stats(fused[1][i], pred_host[i], y_host[i])
            else:
                nll, lp, ent, conf, ok = compute_token_metrics(logits[i], y_out[i], pred[i])
            pending.append((pred_n, true_n, nll, lp, ent, conf, ok))
    if decode_mode is not None and decode_step == "graph":
        # the captured steps pin a KV cache and the cross keys / values per batch size: nothing of that stays behind for training
        from whisper_finetune.engine import decode as _decode

        _decode.release_graphs(model)
    return aggregate_dataset_metrics(_score_utterances(pending, device), dataset_name)


@torch.no_grad()
def evaluate_multiple_datasets(model, dataloaders: Dict[str, object], t_config: dict, tokenizer=None
                               ) -> Tuple[Dict[str, DatasetMetrics], Dict[str, float]]:
    """-> ({name: DatasetMetrics}, macro averages).  `macro_wer` drives best-checkpoint selection."""
    if tokenizer is None:
        tokenizer = _default_tokenizer()
    results = {}
    for name, loader in dataloaders.items():
        results[name] = evaluate_single_dataset(model, loader, name, t_config, tokenizer)
        m = results[name]
        rt.print_once(f"  {name}: n={m.num_samples} WER={m.wer:.4f} CER={m.cer:.4f} NLL={m.mean_token_nll:.4f} ECE={m.ece:.4f}")
    macro = compute_macro_average(list(results.values()))
    return results, macro


def log_metrics_to_wandb(dataset_metrics: Dict[str, DatasetMetrics], macro_metrics: Dict[str, float], step: int,
                         prefix: str = "val") -> None:
    data = {}
    for name, m in dataset_metrics.items():
        for key in ("wer", "cer", "mean_token_nll", "avg_log_prob", "mean_token_entropy", "ece", "num_samples"):
            data[f"{prefix}/{name}/{key}"] = getattr(m, key)
        for key in ("corpus_wer", "corpus_cer", "word_sub_rate", "word_del_rate", "word_ins_rate"):
            if getattr(m, key, None) is not None:
                data[f"{prefix}/{name}/{key}"] = getattr(m, key)
    for key, val in macro_metrics.items():
        data[f"{prefix}/{key}"] = val
    rt.log(data, step=step)
