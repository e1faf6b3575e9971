"""`greedy_decode(step="graph")`: the cached decoding step captured in a HIP graph and run on the weight-streaming small-M GEMMs
(engine/decode/, csrc/gemm_stream.hip), on the case of tests/test_decode_gpu.py (whisper-tiny, B = 4, ragged prompts of 4 + 2b
tokens, 28 steps) and on a large-v3-width model with 2 + 2 layers (the dimensions of tests/test_dispatch_regime_gpu.py) at B = 8
and B = 32.

Bounds: cached logits on the streaming GEMMs against the fp32 oracle < 2e-2 relative L2 (the bound of tests/test_decode_gpu.py),
picks by tests/_decode_oracle.py (TAU, FLIP_SHARE as they stand).  Everything about the capture is held to bit equality: a graph
replays the launches of the eager step, so it may change nothing."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests import _decode_oracle as DO  # noqa: E402
from tests.test_decode_gpu import B, EOT, MAX_LEN, PROMPT_LEN, S, STEPS, T, _prompts  # noqa: E402
from tests.test_dispatch_regime_gpu import DIMS as WIDE_DIMS, _params as _wide_params  # noqa: E402
from tests.test_model_gpu import _engine, _tiny_case  # noqa: E402
from whisper_finetune.engine import decode as D  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine.whisper_model import MODEL_DIMS, Whisper  # noqa: E402
from whisper_finetune.eval import evaluator  # noqa: E402
from whisper_finetune.eval.metrics import wer  # noqa: E402
from whisper_finetune.eval.utils import VOCAB_SPECS, normalize_text  # noqa: E402
from whisper_finetune.model import lora as lora_mod  # noqa: E402

DEV = torch.device("cuda:0")
GEMMS_PER_LAYER = 6  # fused q/k/v, self out, cross q, cross out, mlp.0, mlp.2 (the cross k/v product belongs to the prefill)


class _Spy:
    """Counts the GEMMs that reached wft_gemm_nt_stream_bf16 (K.gemm_nt_stream returned a tensor) and the M <= 32 products that
    still went to wft_gemm_nt_bf16."""

    def __enter__(self):
        self.served = self.refused = self.old_small = 0
        self.real = (K.gemm_nt_stream, K.gemm_nt)
        real_stream, real_nt = self.real

        def stream(a, b, **kw):
            out = real_stream(a, b, **kw)
            if out is None:
                self.refused += 1
            else:
                self.served += 1
            return out

        def nt(a, b, **kw):
            if (kw.get("M") or a.shape[0]) <= 32:
                self.old_small += 1
            return real_nt(a, b, **kw)

        K.gemm_nt_stream, K.gemm_nt = stream, nt
        return self

    def __exit__(self, *exc):
        K.gemm_nt_stream, K.gemm_nt = self.real


def _same(a, b, what=""):
    for x, y, name in zip(a, b, ("tokens", "lengths", "sum_logprob")):
        assert torch.equal(x, y), f"{what}: {name} differ"


@pytest.fixture(scope="module")
def case():
    dims, params, audio, y_in, y_out = _tiny_case(B=B, S=S)
    m = _engine(dims, params).eval()
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    return dict(dims=dims, params=params, model=m, mel=mel, prompt=_prompts(y_in), y_in=y_in, y_out=y_out)


def _args(case):
    return case["mel"], case["prompt"].to(DEV), PROMPT_LEN


def test_streaming_steps_follow_the_oracle_tiny(case):
    m = case["model"]
    n_layer = case["dims"].n_text_layer
    with _Spy() as spy, D.stream_gemm():
        tr = DO.follow(m, O.Oracle(case["dims"], case["params"]), case["mel"], case["prompt"].to(DEV), PROMPT_LEN, STEPS, eot=EOT,
                       max_len=MAX_LEN, compare_teacher=False)
    print("streaming GEMMs, cached vs the fp32 oracle, worst row per step:", " ".join(f"{v:.4f}" for v in tr.rel_oracle))
    assert len(tr.rel_oracle) == STEPS and max(tr.rel_oracle) < 2e-2, max(tr.rel_oracle)
    DO.check_prefix_following(tr, "tiny, B = 4, streaming GEMMs")
    # every projection of every cached step, the logits product included (25 per step on whisper-tiny), plus the prefill's logits
    per_step = GEMMS_PER_LAYER * n_layer + 1
    assert per_step == 25
    assert spy.served == per_step * (STEPS - 1) + 1, (spy.served, spy.refused)
    assert spy.old_small == 0


@pytest.fixture(scope="module")
def wide():
    params = _wide_params()
    m = _engine(WIDE_DIMS, params).eval()
    return dict(model=m, params=params)


def _wide_inputs(Bw):
    audio, y_in, _ = O.synthetic_batch(WIDE_DIMS, Bw, 24)
    mel = K.logmel(audio.to(DEV), O.mel_filters(WIDE_DIMS.n_mels).to(DEV))
    plen = torch.tensor([4 + 2 * (b % 4) for b in range(Bw)])
    Tw = int(plen.max())
    prompt = torch.full((Bw, Tw), EOT, dtype=torch.int64)
    for b in range(Bw):
        prompt[b, :plen[b]] = y_in[b, :plen[b]]
    return mel, prompt.to(DEV), plen, Tw


def test_wide_model_b8_follows_the_oracle_and_graph_changes_nothing(wide):
    m = wide["model"]
    steps = 12
    mel, prompt, plen, Tw = _wide_inputs(8)
    with _Spy() as spy, D.stream_gemm():
        tr = DO.follow(m, O.Oracle(WIDE_DIMS, wide["params"]), mel, prompt, plen, steps, eot=EOT, max_len=Tw + steps, compare_teacher=False)
    print("large-v3 width, B = 8, streaming GEMMs vs the fp32 oracle:", " ".join(f"{v:.4f}" for v in tr.rel_oracle))
    assert max(tr.rel_oracle) < 2e-2, max(tr.rel_oracle)
    DO.check_prefix_following(tr, "large-v3 width 2 + 2 layers, B = 8, streaming GEMMs")
    assert spy.served == (GEMMS_PER_LAYER * 2 + 1) * (steps - 1) + 1 and spy.old_small == 0, (spy.served, spy.old_small)
    kw = dict(eot=EOT, max_len=Tw + steps)
    g = m.greedy_decode(mel, prompt, plen, step="graph", **kw)
    _same(g, m.greedy_decode(mel, prompt, plen, step="graph", _capture=False, **kw), "graph vs eager steps on the streaming GEMMs")
    _same(m.greedy_decode(mel, prompt, plen, step="graph", _stream_gemm=False, **kw), m.greedy_decode(mel, prompt, plen, **kw),
          "graph on the old GEMMs vs step='eager'")
    # (no token-for-token comparison with the trace: there the prefill's logits product ran on the streaming kernel too, in
    # greedy_decode the prefill keeps its kernels, and a near-tie of the first pick may break differently)
    D.release_graphs(m)


def test_wide_model_b32_against_the_engines_own_eager_and_teacher_forced_logits(wide):
    m = wide["model"]
    steps = 12
    mel, prompt, plen, Tw = _wide_inputs(32)
    V = WIDE_DIMS.n_vocab
    worst_eager = worst_tf = 0.0
    with torch.no_grad():
        xa = m.encoder(mel)
        cache = D.KVCache(m.decoder, 32, device=DEV)
        cache.start(prompt, plen, eot=EOT, max_len=Tw + steps, n_vocab=V)
        logits = D.prefill(m.decoder, cache, xa)
        D.pick(m.decoder, cache, logits)
        for i in range(1, steps):
            eager = D.step(m.decoder, cache)  # (a step is idempotent until the pick: it rewrites the k / v row it appended)
            with _Spy() as spy, D.stream_gemm():
                got = D.step(m.decoder, cache)
            assert spy.served == GEMMS_PER_LAYER * 2 + 1 and spy.old_small == 0
            lens = cache.len.cpu()
            Lm = int(lens.max())
            tf = m.decoder(cache.tokens[:, :Lm], xa)[torch.arange(32), lens.long() - 1]
            for b in range(32):
                worst_eager = max(worst_eager, DO.rel(got[b, :V], eager[b, :V]))
                worst_tf = max(worst_tf, DO.rel(got[b, :V], tf[b]))
            D.pick(m.decoder, cache, got)
    print(f"B = 32: streaming step vs eager step {worst_eager:.4f}, vs teacher-forced {worst_tf:.4f} (worst row, relative L2)")
    assert worst_eager < 2e-2 and worst_tf < 2e-2
    kw = dict(eot=EOT, max_len=Tw + steps)
    g = m.greedy_decode(mel, prompt, plen, step="graph", **kw)
    _same(g, m.greedy_decode(mel, prompt, plen, step="graph", _capture=False, **kw), "B = 32 graph vs eager steps")
    for b in range(32):  # the first `steps` picks of every row are the ones of the loop above
        n = int(plen[b]) + steps
        assert torch.equal(g[0][b, :n], cache.tokens[b, :n]), b
    D.release_graphs(m)


def test_capture_alone_changes_nothing(case):
    m = case["model"]
    base = m.greedy_decode(*_args(case), eot=EOT, max_len=MAX_LEN)
    gen = [base[0][b, int(PROMPT_LEN[b]):int(PROMPT_LEN[b]) + STEPS].tolist() for b in range(B)]
    cands = sorted({t for g in gen for t in g[1:]})
    eot2 = next((t for t in cands if 0 < sum(t in g for g in gen) < B), None)  # some rows end mid-sequence, the others at max_len
    assert eot2 is not None
    t0 = gen[0][0]
    variants = [dict(eot=EOT), dict(eot=eot2), dict(eot=EOT, suppress=[t0]), dict(eot=EOT, suppress_first=[t0])]
    for kw in variants:
        for se in (1, 8):
            kw2 = dict(kw, max_len=MAX_LEN, sync_every=se)
            eager = m.greedy_decode(*_args(case), **kw2)
            _same(m.greedy_decode(*_args(case), step="graph", _stream_gemm=False, **kw2), eager, f"graph on the old GEMMs {kw2}")
            _same(m.greedy_decode(*_args(case), step="graph", **kw2), m.greedy_decode(*_args(case), step="graph", _capture=False, **kw2),
                  f"graph vs eager steps on the streaming GEMMs {kw2}")
    stopped = m.greedy_decode(*_args(case), eot=eot2, max_len=MAX_LEN, step="graph")
    assert 0 < int((stopped[1] < MAX_LEN).sum()) < B
    assert m.training is False
    D.release_graphs(m)


def test_second_call_replays_and_sessions_are_capped_and_released(case):
    m = case["model"]
    D.release_graphs(m)
    kw = dict(eot=EOT, max_len=MAX_LEN)
    first = m.greedy_decode(*_args(case), step="graph", **kw)
    (sess,) = D.sessions(m).values()
    assert sess.captures == 1 and sess.replays >= STEPS - 3
    r0 = sess.replays
    _same(m.greedy_decode(*_args(case), step="graph", **kw), first, "second call")
    assert sess.captures == 1 and sess.replays > r0, "the second call at the same batch must replay, not capture"
    # other batch sizes: one session each, at most MAX_SESSIONS, the oldest evicted
    for nb in (2, 1):
        m.greedy_decode(case["mel"][:nb], case["prompt"][:nb].to(DEV), PROMPT_LEN[:nb], step="graph", **kw)
    keys = sorted(k[0] for k in D.sessions(m))
    assert D.MAX_SESSIONS == 2 and keys == [1, 2], keys
    D.release_graphs(m)
    assert D.sessions(m) == {}


def test_release_graphs_frees_what_a_session_pins(case):
    m = case["model"]
    D.release_graphs(m)
    kw = dict(eot=EOT, max_len=MAX_LEN)
    out = m.greedy_decode(*_args(case), **kw)
    del out
    gc.collect(); torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    out = m.greedy_decode(*_args(case), step="graph", **kw)
    pinned = torch.cuda.memory_allocated(DEV)
    del out
    D.release_graphs(m)
    gc.collect(); torch.cuda.synchronize()
    after = torch.cuda.memory_allocated(DEV)
    slot = K._TN_WS[("cuda", 0, "nt_stream")].numel()
    print(f"memory: {base} after the eager decode, {pinned} with the session, {after} after release_graphs (scratch slot {slot})")
    assert after - base <= slot, (after - base, slot)
    assert pinned > after


def test_a_stale_graph_is_never_replayed_optimizer_step():
    dims, params, audio, y_in, y_out = _tiny_case(B=B, S=S)
    m = _engine(dims, params)
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    args = (mel, _prompts(y_in).to(DEV), PROMPT_LEN)
    kw = dict(eot=EOT, max_len=T + 12)
    before = m.greedy_decode(*args, step="graph", **kw)
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=3e-3)
    loss = m(mel, y_in.to(DEV), targets=y_out.to(DEV), label_smoothing=0.1)
    loss.backward()
    opt.step()
    after = m.greedy_decode(*args, step="graph", **kw)
    assert m.training
    _same(after, m.greedy_decode(*args, step="graph", _capture=False, **kw), "after an optimizer step")
    assert not torch.equal(after[2], before[2]), "the optimizer step did not reach the decode"
    D.release_graphs(m)


def test_a_stale_graph_is_never_replayed_lora_and_other_batch():
    dims, params, audio, y_in, _ = _tiny_case(B=B, S=S)
    m = Whisper(MODEL_DIMS["tiny"]); m.load_state_dict(params)
    m.to(DEV).eval()
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    args = (mel, _prompts(y_in).to(DEV), PROMPT_LEN)
    kw = dict(eot=EOT, max_len=T + 12)
    plain = m.greedy_decode(*args, step="graph", **kw)
    # another batch size and prompt width in between, then the first shape again
    m.greedy_decode(mel[:2], _prompts(y_in)[:2, :6].to(DEV), torch.tensor([4, 6]), step="graph", eot=EOT, max_len=6 + 5)
    again = m.greedy_decode(*args, step="graph", **kw)
    _same(again, plain, "after a decode at another batch size")
    _same(again, m.greedy_decode(*args, step="graph", _capture=False, **kw), "after a decode at another batch size, vs eager steps")
    # adapters, decoded without a merge (tests/test_decode_gpu.py::test_lora_adapters_decode_without_merge)
    torch.manual_seed(9)
    lora_mod.apply_lora(m, {"rank": 8, "lora_alpha": 16, "lora_dropout": 0.1})
    gl = torch.Generator().manual_seed(9)
    for n, mod in m.named_modules():
        if "parametrizations" in mod._modules:
            ad = mod.parametrizations.weight[0]
            with torch.no_grad():
                ad.lora_B.copy_((torch.randn(ad.lora_B.shape, generator=gl) * 0.05).to(ad.lora_B.device))
    m.to(DEV)
    adapted = m.greedy_decode(*args, step="graph", **kw)
    _same(adapted, m.greedy_decode(*args, step="graph", _capture=False, **kw), "after apply_lora")
    assert not torch.equal(adapted[2], plain[2]), "the adapters did not reach the decode"
    assert any("parametrizations" in mod._modules for mod in m.modules())  # nothing was merged
    D.release_graphs(m)


def test_graph_decoding_leaves_no_state_behind(case):
    dims, params, audio, y_in, y_out = _tiny_case(B=B, S=S)
    m = _engine(dims, params)
    mel = case["mel"]

    def probe():
        m.eval()
        with torch.no_grad():
            logits = m(mel, y_in.to(DEV)).clone()
        m.train()
        loss = m(mel, y_in.to(DEV), targets=y_out.to(DEV), label_smoothing=0.1).detach().clone()
        return logits, loss

    l0, s0 = probe()
    attrs = {n: set(vars(mod)) for n, mod in m.named_modules()}
    m.greedy_decode(mel, case["prompt"].to(DEV), PROMPT_LEN, eot=EOT, max_len=T + 6, step="graph")
    assert m.training
    l1, s1 = probe()
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    assert attrs == {n: set(vars(mod)) for n, mod in m.named_modules()}
    D.release_graphs(m)
    with pytest.raises(ValueError, match="step"):
        m.greedy_decode(mel, case["prompt"].to(DEV), PROMPT_LEN, eot=EOT, step="bogus")
    m32 = _engine(dims, params).set_compute_dtype("fp32")
    with pytest.raises(NotImplementedError, match="bf16"):
        m32.greedy_decode(mel, case["prompt"].to(DEV), PROMPT_LEN, eot=EOT, step="graph")


def _text_batch(texts):
    """Teacher-forcing rows of byte-token transcripts under the synthetic batches' special-token layout."""
    S_ = 4 + max(len(t) for t in texts) + 1
    y_in = torch.full((len(texts), S_), EOT, dtype=torch.int64)
    y_out = torch.full((len(texts), S_), -100, dtype=torch.int64)
    for i, t in enumerate(texts):
        row = [50258, 50261, 50359, 50363] + list(t.encode("utf-8"))
        y_in[i, :len(row)] = torch.tensor(row)
        y_out[i, :len(row)] = torch.tensor(row[1:] + [EOT])
    return y_in, y_out


def test_evaluator_graph_mode_returns_the_metrics_of_a_direct_graph_decode(case):
    from whisper_finetune.data.data_loader import SimpleTokenizer

    m = case["model"]
    D.release_graphs(m)
    tok = SimpleTokenizer()
    y_in, y_out = _text_batch(["the quick brown fox", "jumps over", "the lazy dog and runs", "far away"])
    batches = [(case["mel"], y_in, y_out), (case["mel"][:2], y_in[2:], y_out[2:])]
    cfg = {"mixed_precision_training": True, "mp_dtype": "bf16", "wft_eval_decode": "greedy", "wft_eval_decode_step": "graph"}
    calls = []
    real = m.greedy_decode

    def recording(*a, **kw):
        out = real(*a, **kw)
        calls.append((a, kw, out))
        return out

    m.greedy_decode = recording
    try:
        got = evaluator.evaluate_single_dataset(m, batches, "syn", cfg, tokenizer=tok)
    finally:
        del m.greedy_decode
    assert len(calls) == 2 and all(kw.get("step") == "graph" for _, kw, _ in calls)
    assert D.sessions(m) == {}, "the evaluator must release the captured steps when the dataset is done"
    wers = []
    specials = set(tok.special_tokens.values())
    for (a, kw, out), (_, yi, yo) in zip(calls, batches):
        direct = m.greedy_decode(*a, **kw)
        _same(direct, out, "evaluator vs direct greedy_decode(step='graph')")
        tokens, lengths = direct[0].cpu().tolist(), direct[1].cpu().tolist()
        plen = a[2].tolist()
        for i in range(len(plen)):
            pred = [t for t in tokens[i][plen[i]:lengths[i]] if t not in specials]
            true = [t for t in yo[i].tolist() if t not in specials and t != -100]
            spec = VOCAB_SPECS["v0"]
            wers.append(wer(normalize_text(tok.decode(true), **spec), normalize_text(tok.decode(pred), **spec)))
    assert got.num_samples == len(wers) == 6
    assert got.wer == pytest.approx(sum(wers) / len(wers))
    D.release_graphs(m)
