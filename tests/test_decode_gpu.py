"""KV-cached greedy decoding end to end on the GPU (engine/decode/, Whisper.greedy_decode) against the CPU oracle re-forwarded
over the growing prefix (tests/_decode_oracle.py): whisper-tiny, B = 4, ragged prompts of 4 + 2b tokens.

Bounds.  Cached logits against the fp32 oracle: relative L2 < 2e-2, the bound tests/test_model_gpu.py holds teacher-forced engine
logits to (the oracle's own bf16-emulation mode sits at 0.007 on this case).  Picks: tests/_decode_oracle.py (TAU, FLIP_SHARE)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests import _decode_oracle as DO  # noqa: E402
from tests.test_model_gpu import _engine, _tiny_case  # noqa: E402
from whisper_finetune.engine import decode as D  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine.whisper_model import MODEL_DIMS, Whisper  # noqa: E402
from whisper_finetune.model import lora as lora_mod  # noqa: E402

DEV = torch.device("cuda:0")
B, S, STEPS = 4, 12, 28
EOT = 50257
PROMPT_LEN = torch.tensor([4 + 2 * b for b in range(B)])
T = int(PROMPT_LEN.max())
MAX_LEN = T + STEPS  # the longest prompt generates STEPS tokens, the others more


def _prompts(y_in):
    """Row b's prompt: the first 4 + 2b tokens of its y_in (the four specials, then random text), right-padded."""
    prompt = torch.full((B, T), EOT, dtype=torch.int64)
    for b in range(B):
        prompt[b, :PROMPT_LEN[b]] = y_in[b, :PROMPT_LEN[b]]
    return prompt


@pytest.fixture(scope="module")
def case():
    dims, params, audio, y_in, _ = _tiny_case(B=B, S=S)
    m = _engine(dims, params).eval()
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    oracle = O.Oracle(dims, params)
    prompt = _prompts(y_in)
    tr = DO.follow(m, oracle, mel, prompt.to(DEV), PROMPT_LEN, STEPS, eot=EOT, max_len=MAX_LEN)
    return dict(dims=dims, params=params, model=m, mel=mel, oracle=oracle, prompt=prompt, trace=tr, y_in=y_in)


def test_cached_logits_equal_teacher_forced_and_oracle(case):
    tr = case["trace"]
    print("cached vs the engine's teacher-forced last row, worst row per step:", " ".join(f"{v:.4f}" for v in tr.rel_teacher))
    print("cached vs the fp32 oracle,                      worst row per step:", " ".join(f"{v:.4f}" for v in tr.rel_oracle))
    assert len(tr.rel_oracle) == STEPS
    assert max(tr.rel_teacher) < 2e-2, max(tr.rel_teacher)
    assert max(tr.rel_oracle) < 2e-2, max(tr.rel_oracle)


def test_tokens_follow_the_oracle_on_the_engines_prefix(case):
    DO.check_prefix_following(case["trace"], "tiny, B = 4")


def test_greedy_decode_equals_its_pieces_and_pads_with_eot(case):
    tr, m = case["trace"], case["model"]
    tokens, lengths, slp = m.greedy_decode(case["mel"], case["prompt"].to(DEV), PROMPT_LEN, eot=EOT, max_len=MAX_LEN)
    assert tokens.dtype == torch.int64 and tokens.shape == (B, int(lengths.max())) and slp.dtype == torch.float32
    # the trace ran STEPS picks; greedy_decode runs every row to its end: the first STEPS generated tokens agree bit for bit
    for b in range(B):
        n = min(int(PROMPT_LEN[b]) + STEPS, int(lengths[b]))
        assert torch.equal(tokens[b, :n].cpu(), tr.tokens[b, :n]), b
        assert torch.equal(tokens[b, :PROMPT_LEN[b]].cpu(), case["prompt"][b, :PROMPT_LEN[b]])
        assert (tokens[b, int(lengths[b]):] == EOT).all()
        assert int(lengths[b]) == MAX_LEN or int(tokens[b, int(lengths[b]) - 1]) == EOT
    assert m.training is False


def test_stopping_padding_and_sync_every(case):
    """eot set to a token that some rows emit mid-sequence and others never do (ids from this test's own first run)."""
    tr, m = case["trace"], case["model"]
    gen = [[int(tr.picks[i][b]) for i in range(STEPS)] for b in range(B)]
    print("generated token sets per row:", [sorted(set(g)) for g in gen])
    assert all(EOT not in g for g in gen), "the random-init model emitted the real eot in the first run: pick another seed"
    cands = sorted({t for g in gen for t in g[1:]})
    eot2 = next((t for t in cands if 0 < sum(t in g for g in gen) < B), None)
    assert eot2 is not None, f"no token is emitted by some rows and never by others: {[sorted(set(g)) for g in gen]}"
    args = (case["mel"], case["prompt"].to(DEV), PROMPT_LEN)
    res = {se: m.greedy_decode(*args, eot=eot2, max_len=MAX_LEN, sync_every=se) for se in (1, 8)}
    for a, b_ in zip(res[1], res[8]):
        assert torch.equal(a, b_), "sync_every changes the result"
    tokens, lengths, slp = (t.cpu() for t in res[8])
    stopped = 0
    for b in range(B):
        pl = int(PROMPT_LEN[b])
        if eot2 in gen[b]:
            k = gen[b].index(eot2)  # the row ends with its first eot2
            stopped += 1
            assert int(lengths[b]) == pl + k + 1
            assert tokens[b, pl:pl + k + 1].tolist() == gen[b][:k + 1]
            assert (tokens[b, pl + k + 1:] == eot2).all()
            want = sum(float(tr.logprobs[i][b]) for i in range(k + 1))  # the eot pick's log-probability is the last one added
            assert abs(float(slp[b]) - want) < 1e-3 * max(1.0, abs(want)), (b, float(slp[b]), want)
        else:
            assert int(lengths[b]) == MAX_LEN  # max_len ends the rest
            assert tokens[b, pl:pl + STEPS].tolist() == gen[b], b  # bit-identical to the first run
    assert 0 < stopped < B


def test_suppress_moves_the_pick_to_the_runner_up(case):
    tr, m = case["trace"], case["model"]
    ref0 = tr.ref_logits[0]  # oracle logits of every row's first generated position
    t0 = int(tr.picks[0][0])
    for kw in ({"suppress": [t0]}, {"suppress_first": [t0]}):
        tokens, lengths, _ = m.greedy_decode(case["mel"], case["prompt"].to(DEV), PROMPT_LEN, eot=EOT, max_len=T + 2, **kw)
        for b in range(B):
            got = int(tokens[b, int(PROMPT_LEN[b])])
            masked = ref0[b].clone(); masked[t0] = float("-inf")
            assert got != t0
            assert got == int(masked.argmax()) or float(masked.max() - masked[got]) <= DO.TAU, (kw, b, got)
    # `suppress` holds at every position, not only the first
    tokens, lengths, _ = m.greedy_decode(case["mel"], case["prompt"].to(DEV), PROMPT_LEN, eot=EOT, max_len=MAX_LEN, suppress=[t0])
    for b in range(B):
        assert not (tokens[b, int(PROMPT_LEN[b]):int(lengths[b])] == t0).any()


def test_lora_adapters_decode_without_merge():
    dims, params, audio, y_in, _ = _tiny_case(B=B, S=S)
    m = Whisper(MODEL_DIMS["tiny"]); m.load_state_dict(params)
    torch.manual_seed(9)  # lora_A's kaiming init draws from the global generator
    lora_mod.apply_lora(m, {"rank": 8, "lora_alpha": 16, "lora_dropout": 0.1})
    gl = torch.Generator().manual_seed(9)
    cfg = {}
    for n, mod in m.named_modules():
        if "parametrizations" in mod._modules:
            ad = mod.parametrizations.weight[0]
            with torch.no_grad():
                ad.lora_B.copy_(torch.randn(ad.lora_B.shape, generator=gl) * 0.05)
            cfg[n] = (ad.lora_A.detach().clone(), ad.lora_B.detach().clone(), ad.scaling, None)  # eval: no dropout mask
    m.to(DEV).train()  # greedy decoding has eval() semantics whatever the mode it is called in ...
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    steps = 12
    tr = DO.follow(m, O.Oracle(dims, params, lora=cfg), mel, _prompts(y_in).to(DEV), PROMPT_LEN, steps, eot=EOT, max_len=T + steps,
                   compare_teacher=False)
    print("adapted model, cached vs the fp32 oracle with the same adapters:", " ".join(f"{v:.4f}" for v in tr.rel_oracle))
    assert max(tr.rel_oracle) < 2e-2
    DO.check_prefix_following(tr, "tiny + LoRA r=8")
    m.train()
    tokens, lengths, _ = m.greedy_decode(mel, _prompts(y_in).to(DEV), PROMPT_LEN, eot=EOT, max_len=T + steps)
    assert m.training  # ... and restores it
    for b in range(B):
        n = min(int(PROMPT_LEN[b]) + steps, int(lengths[b]))
        assert torch.equal(tokens[b, :n].cpu(), tr.tokens[b, :n])
    assert all("parametrizations" in mod._modules for n, mod in m.named_modules() if n in cfg)  # nothing was merged


def test_decoding_leaves_no_state_behind(case):
    """kv_cache=None outputs and a training loss are bit-identical before and after a greedy_decode call."""
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
    attrs = {n: set(vars(mod)) for n, mod in m.named_modules()}  # (after the first forward: the Linear groups are created lazily)
    m.greedy_decode(mel, case["prompt"].to(DEV), PROMPT_LEN, eot=EOT, max_len=T + 6)
    assert m.training
    l1, s1 = probe()
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    assert attrs == {n: set(vars(mod)) for n, mod in m.named_modules()}


def test_cache_argument_errors(case):
    m = case["model"]
    with torch.no_grad():
        xa = m.encoder(case["mel"])
        with pytest.raises(NotImplementedError):  # upstream's hook-filled dict is still not supported
            m.decoder(case["prompt"].to(DEV), xa, kv_cache={"k": 1})
    cache = D.KVCache(m.decoder, B, device=DEV)
    cache.start(case["prompt"].to(DEV), PROMPT_LEN, eot=EOT, n_vocab=m.dims.n_vocab)
    with pytest.raises(RuntimeError):  # an inference object: no autograd graph through a cache
        m.decoder.hidden(case["prompt"].to(DEV), xa, kv_cache=cache)
    with pytest.raises(ValueError):
        m.greedy_decode(case["mel"], case["prompt"].to(DEV), PROMPT_LEN, eot=EOT, max_len=T - 1)
    m32 = _engine(case["dims"], case["params"]).set_compute_dtype("fp32")
    with pytest.raises(NotImplementedError, match="bf16"):
        m32.greedy_decode(case["mel"], case["prompt"].to(DEV), PROMPT_LEN, eot=EOT)
