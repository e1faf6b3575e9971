"""Whisper.find_alignment end to end on the GPU, on a small engine model (2 decoder layers, n_state 128 = 2 heads of 64, 100 audio
frames, random init), every stage chained exactly to the one before it: the captured q is the query projection's output bit for
bit and the captured k a linear of the encoder output; the probabilities are within the oracle's bound on the captured q / k; the
matrix within its bound on the device's probabilities; the paths equal the oracle's DTW on the device's matrix; the words equal the
host arithmetic on those paths; the word probabilities equal the softmax over [:eot] of the model's own logits.

The cross query / key weights of both decoder layers are scaled up until the natural-log scores have a standard deviation of
about 2: at the init's scale the probabilities of a column barely differ between the tokens, the standardisation divides by a
vanishing spread and nothing downstream can be compared."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _align_oracle as AO  # noqa: E402
from whisper_finetune.engine import decode as D  # noqa: E402
from whisper_finetune.engine.whisper_model import ModelDimensions, Whisper, init_random_  # noqa: E402

DEV = torch.device("cuda:0")
DIMS = ModelDimensions(80, 100, 128, 2, 2, 256, 32, 128, 2, 2)
EOT, SOT, NO_TS = 200, [201, 202, 203], 204
KW = dict(sot_sequence=SOT, no_timestamps=NO_TS, eot=EOT)
TEXTS = [[5, 17, 100, 3, 42, 42, 7, 199, 0], [66], [9, 8, 7, 6, 5]]   # ragged; one audio has a single text token
FRAMES = [200, 200, 131]                                               # one audio's num_frames lies below the full 200: 65 keys
COUNTS = [[2, 1, 3, 2, 1, 1], None, [1, 4, 1]]                         # tokens per word over text + [eot]


def _score_std(q, k, n_tok, n_key):
    s, _ = AO.scores_ref(q.cpu(), k.cpu(), [0, 1], 0.125)
    return float(torch.cat([s[b, :, :n_tok[b], :n_key[b]].flatten() for b in range(s.shape[0])]).std())


@pytest.fixture(scope="module")
def case():
    m = init_random_(Whisper(ModelDimensions(**vars(DIMS))), seed=4, std=0.1).to(DEV).eval()
    g = torch.Generator().manual_seed(11)
    mel = (torch.randn(3, DIMS.n_mels, 2 * DIMS.n_audio_ctx, generator=g) * 0.5).to(DEV)
    default = m.alignment_heads.to_dense().clone()
    m.set_alignment_heads(torch.ones(2, 2, dtype=torch.bool))
    for layer in range(2):  # in layer order: a layer's queries depend on the cross-attention of the layers below it
        ca = m.decoder.blocks[layer].cross_attn
        _, dbg = m.find_alignment(mel, TEXTS, num_frames=FRAMES, return_debug=True, **KW)
        f = math.sqrt(2.0 / _score_std(dbg["q"][ca], dbg["k"][ca], dbg["n_tok"], dbg["n_key"]))
        with torch.no_grad():
            ca.query.weight.mul_(f)
            ca.key.weight.mul_(f)
    m.set_alignment_heads(default)
    assert torch.equal(m.alignment_heads.to_dense().cpu(), torch.tensor([[False, False], [True, True]]))
    hooked = {}
    hooks = [b.cross_attn.query.register_forward_hook(lambda mod, i, o, b=b: hooked.__setitem__(b.cross_attn, o.detach().clone()))
             for b in m.decoder.blocks]
    words, dbg = m.find_alignment(mel, TEXTS, num_frames=FRAMES, word_token_counts=COUNTS, return_debug=True, **KW)
    for h in hooks:
        h.remove()
    torch.cuda.synchronize()
    return dict(model=m, mel=mel, words=words, dbg=dbg, hooked=hooked)


def _excess(what, got, ref, bound):
    err = (got.cpu().to(AO.F64) - ref).abs()
    live = bound > 0
    worst = float((err[live] / bound[live]).max())
    print(f"{what}: worst |err| / bound {worst:.3f}, max |err| {float(err[live].max()):.3e}")
    return worst


def _check_chain(m, mel, words, dbg, texts, frames, counts, hooked=None):
    """checks 1-5 of the module docstring on one find_alignment result"""
    n_tok, n_key, rows = dbg["n_tok"], dbg["n_key"], dbg["rows"]
    assert n_tok == [len(SOT) + 1 + len(texts[b]) + 1 for b in rows] and n_key == [frames[b] // 2 for b in rows]
    T = max(n_tok)
    probs = dbg["probs"].cpu()
    with torch.no_grad():
        xa = m.embed_audio(mel[rows])
    for mod, (heads, at) in dbg["slots"].items():
        q, k = dbg["q"][mod], dbg["k"][mod]
        assert q.shape == (len(rows), T, 128) and k.shape == (len(rows), 100, 128)
        if hooked is not None:
            assert torch.equal(q.reshape(-1, 128), hooked[mod].reshape(-1, 128)), "the captured q is not the query projection's output"
        k_ref = xa.float() @ mod.key.weight.detach().to(torch.bfloat16).float().T   # (the GEMM reads the weight's bf16 shadow)
        tol = 2.0 ** -8 * (k_ref.abs() + k_ref.pow(2).mean().sqrt())
        assert ((k.float() - k_ref).abs() <= tol).all(), "the captured k is not the key projection of the encoder output"
        std = _score_std(q, k, n_tok, n_key)
        assert 1.0 < std < 3.0, std
        hs = heads.tolist()
        ref = AO.probs_ref(q.cpu(), k.cpu(), hs, n_tok, n_key, 0.125)
        bound = AO.probs_bound(q.cpu(), k.cpu(), hs, n_tok, n_key, 0.125, ref)
        got = probs[:, at:at + len(hs)]
        assert (got[bound == 0] == 0).all()
        assert _excess(f"probs of heads {hs} (score std {std:.2f})", got, ref, bound) <= 1.0
    ref, bound = AO.matrix_ref(probs, n_tok, n_key)
    matrix = dbg["matrix"].cpu()
    assert torch.isfinite(ref).all() and (matrix[bound == 0] == 0).all()
    assert _excess("matrix", matrix, ref, bound) <= 1.0
    pt, pj, pl = dbg["paths"]
    at = 0
    for i, b in enumerate(rows):
        n_rows = len(texts[b]) + 1
        t, f = AO.dtw_ref(-matrix[i, len(SOT):len(SOT) + n_rows, :n_key[i]].numpy())
        n = int(pl[i])
        assert n == len(t) and np.array_equal(pt[i, :n].numpy(), t) and np.array_equal(pj[i, :n].numpy(), f), b
        assert (pt[i, n:] == -1).all() and (pj[i, n:] == -1).all()
        tp = dbg["token_probs"][at:at + len(texts[b])]
        at += len(texts[b])
        wc = counts[b] if counts[b] is not None else [1] * (len(texts[b]) + 1)
        want = AO.words_ref(t, f, wc, tp, texts[b])
        assert len(words[b]) == len(wc) - 1 == len(want)
        for (s0, e0, p0, ids0), (s1, e1, p1, ids1) in zip(words[b], want):
            assert (s0, e0, ids0) == (s1, e1, ids1) and abs(p0 - p1) < 1e-12
            assert 0.0 <= s0 <= e0 <= n_key[i] / 50.0
        assert [t for w in words[b] for t in w[3]] == texts[b]


def test_every_stage_chains_to_the_one_before(case):
    _check_chain(case["model"], case["mel"], case["words"], case["dbg"], TEXTS, FRAMES, COUNTS, case["hooked"])
    assert list(case["dbg"]["slots"]) == [case["model"].decoder.blocks[1].cross_attn]  # the default: the upper half of the decoder
    assert len(case["words"][1]) == 1 and case["words"][1][0][3] == [66]


def test_word_probabilities_are_the_softmax_below_eot_of_the_models_logits(case):
    m, dbg = case["model"], case["dbg"]
    T = max(dbg["n_tok"])
    tokens = torch.full((3, T), EOT, dtype=torch.int64)
    for b, text in enumerate(TEXTS):
        tokens[b, :len(SOT) + 1 + len(text)] = torch.tensor(SOT + [NO_TS] + text)
    with torch.no_grad():
        logits = m.logits(tokens.to(DEV), m.embed_audio(case["mel"])).float().cpu()
    want = [float(torch.softmax(logits[b, len(SOT) + j, :EOT], -1)[t]) for b, text in enumerate(TEXTS) for j, t in enumerate(text)]
    got = dbg["token_probs"]
    print("token probabilities:", " ".join(f"{v:.4f}" for v in got))
    assert len(got) == len(want) and max(abs(a - b) for a, b in zip(got, want)) < 1e-4
    stats = dbg["token_stats"].cpu()
    assert np.allclose(got, torch.exp(stats[:, 3] - stats[:, 0]).tolist(), rtol=0, atol=1e-7)
    # a word's probability is the mean over its tokens
    assert abs(case["words"][0][0][2] - (got[0] + got[1]) / 2) < 1e-9 and abs(case["words"][2][1][2] - sum(got[11:15]) / 4) < 1e-9


def test_one_head_of_layer_0(case):
    m = case["model"]
    default = m.alignment_heads.to_dense().clone()
    mask = torch.zeros(2, 2, dtype=torch.bool)
    mask[0, 1] = True
    m.set_alignment_heads(D.dump_alignment_heads(mask))
    try:
        words, dbg = m.find_alignment(case["mel"], TEXTS, num_frames=FRAMES, word_token_counts=COUNTS, return_debug=True, **KW)
        assert list(dbg["slots"]) == [m.decoder.blocks[0].cross_attn] and dbg["slots"][m.decoder.blocks[0].cross_attn][0].tolist() == [1]
        assert dbg["probs"].shape[1] == 1 and list(dbg["q"]) == [m.decoder.blocks[0].cross_attn]
        _check_chain(m, case["mel"], words, dbg, TEXTS, FRAMES, COUNTS)
    finally:
        m.set_alignment_heads(default)


def test_an_audio_without_text_gives_no_words_and_the_others_are_unchanged(case):
    m = case["model"]
    texts = [TEXTS[0], [], TEXTS[2]]
    words, dbg = m.find_alignment(case["mel"], texts, num_frames=FRAMES, word_token_counts=COUNTS, return_debug=True, **KW)
    assert words[1] == [] and dbg["rows"] == [0, 2]
    _check_chain(m, case["mel"], words, dbg, texts, FRAMES, COUNTS)
    assert [w[3] for w in words[0]] == [w[3] for w in case["words"][0]]
    assert m.find_alignment(case["mel"], [[], [], []], num_frames=200, **KW) == [[], [], []]
    with pytest.raises(ValueError):
        m.find_alignment(case["mel"], [[EOT], [1], [2]], num_frames=200, **KW)  # text ids lie below eot
    with pytest.raises(ValueError):
        m.find_alignment(case["mel"], [[1] * 28, [1], [2]], num_frames=200, **KW)  # 3 + 1 + 28 + 1 > n_text_ctx = 32
    with pytest.raises(ValueError):
        m.find_alignment(case["mel"], TEXTS, num_frames=[200, 202, 200], **KW)  # more frames than the encoder has


def test_fp32_mode_raises_and_no_capture_stays_behind(case):
    m = case["model"]
    tokens = torch.tensor([SOT + [NO_TS] + TEXTS[2] + [EOT]] * 3, device=DEV)
    with torch.no_grad():
        xa = m.embed_audio(case["mel"])
        before = m.logits(tokens, xa).clone()
        m.find_alignment(case["mel"], TEXTS, num_frames=FRAMES, **KW)
        assert D.alignment_capture() is None
        after = m.logits(tokens, xa)
    assert torch.equal(before, after)
    m.set_compute_dtype("fp32")
    try:
        with pytest.raises(NotImplementedError):
            m.find_alignment(case["mel"], TEXTS, num_frames=FRAMES, **KW)
    finally:
        m.set_compute_dtype("bf16")
