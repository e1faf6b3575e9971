"""CPU proofs for the word-level alignment tests (tests/_align_oracle.py): the bounds that tests/test_align_kernels_gpu.py and
tests/test_align_decode_gpu.py hold the kernels to pass a correct fp32 restatement of every stage and fail every mutant, on the GPU
tests' own inputs; the anti-diagonal DTW oracle is the literal double loop; the jumps / words arithmetic on hand-written paths; the
base85 alignment-head dump."""
import numpy as np
import pytest
import torch

from tests import _align_oracle as AO
from whisper_finetune.engine import decode as D


# ------------------------------------------------------------------------------------------------ probabilities
@pytest.fixture(scope="module")
def probs_cases():
    out = []
    for i, (Tq, n_tok, n_key) in enumerate(AO.PROBS_CASES):
        c = AO.probs_case(Tq, n_tok, n_key, seed=i)
        c["ref"] = AO.probs_ref(c["q"], c["k"], c["heads"], c["n_tok"], c["n_key"], c["scale"])
        c["bound"] = AO.probs_bound(c["q"], c["k"], c["heads"], c["n_tok"], c["n_key"], c["scale"], c["ref"])
        out.append(c)
    return out


def _excess(got, ref, bound):
    """the worst |got - ref| / bound over the elements with a bound (0 / 0 elements must be equal)"""
    err = (got.to(AO.F64) - ref).abs()
    assert (err[bound == 0] == 0).all()
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def test_probs_bound_holds_the_fp32_restatement(probs_cases):
    for c in probs_cases:
        s, _ = AO.scores_ref(c["q"], c["k"], c["heads"], c["scale"])
        assert 1.5 < float(s.std()) < 2.5, "the scores are meant to spread to a standard deviation of about 2"
        got = AO.probs_f32(c["q"], c["k"], c["heads"], c["n_tok"], c["n_key"], c["scale"])
        worst = _excess(got, c["ref"], c["bound"])
        print(f"Tq {c['q'].shape[1]} n_key {c['n_key']}: worst |err| / bound {worst:.3f}")
        assert worst <= 1.0


@pytest.mark.parametrize("mutant", ["drop_last_key", "leak_key", "sorted_heads"])
def test_probs_bound_fails_the_mutants(probs_cases, mutant):
    """every case has an audio with more than one key and one with n_key < Tk, so each defect changes something in each case"""
    for c in probs_cases:
        got = AO.probs_f32(c["q"], c["k"], c["heads"], c["n_tok"], c["n_key"], c["scale"], mutant=mutant)
        worst = _excess_any(got, c["ref"], c["bound"])
        print(f"{mutant}, Tq {c['q'].shape[1]} n_key {c['n_key']}: worst |err| / bound {worst:.3g}")
        assert worst > 1.0, (mutant, c["n_key"])


def _excess_any(got, ref, bound):
    err = (got.to(AO.F64) - ref).abs()
    if (err[bound == 0] != 0).any():
        return float("inf")
    live = bound > 0
    return float((err[live] / bound[live]).max())


# ------------------------------------------------------------------------------------------------ matrix
@pytest.fixture(scope="module")
def matrix_cases():
    out = []
    for i, keys in enumerate(AO.MATRIX_KEYS):
        S = AO.MATRIX_SEL[i % 2]
        probs = AO.crafted_probs(3, S, 448, 1500, keys, seed=i)
        ref, bound = AO.matrix_ref(probs, AO.MATRIX_TOK, keys)
        out.append(dict(probs=probs, n_key=keys, S=S, ref=ref, bound=bound))
    # the last key set again with three heads, so that "the last head is missing" bites with every key count
    probs = AO.crafted_probs(3, 3, 448, 1500, AO.MATRIX_KEYS[1], seed=7)
    ref, bound = AO.matrix_ref(probs, AO.MATRIX_TOK, AO.MATRIX_KEYS[1])
    out.append(dict(probs=probs, n_key=AO.MATRIX_KEYS[1], S=3, ref=ref, bound=bound))
    return out


def test_matrix_bound_holds_the_fp32_restatement(matrix_cases):
    for c in matrix_cases:
        got = AO.matrix_f32(c["probs"], AO.MATRIX_TOK, c["n_key"])
        worst = _excess(got, c["ref"], c["bound"])
        print(f"n_sel {c['S']} n_key {c['n_key']}: worst |err| / bound {worst:.3f}; largest bound {float(c['bound'].max()):.2e}")
        assert worst <= 1.0
        assert torch.isfinite(c["ref"]).all()


@pytest.mark.parametrize("mutant", ["unbiased", "zero_pad", "width5", "padded_rows", "drop_last_head"])
def test_matrix_bound_fails_the_mutants(matrix_cases, mutant):
    hit = 0
    for c in matrix_cases:
        if mutant == "drop_last_head" and c["S"] == 1:
            continue  # (one head: nothing to drop)
        got = AO.matrix_f32(c["probs"], AO.MATRIX_TOK, c["n_key"], mutant=mutant)
        worst = _excess_any(got, c["ref"], c["bound"])
        print(f"{mutant}, n_sel {c['S']} n_key {c['n_key']}: worst |err| / bound {worst:.3g}")
        assert worst > 1.0, (mutant, c["S"], c["n_key"])
        hit += 1
    assert hit >= 2


# ------------------------------------------------------------------------------------------------ dynamic time warping
def _dtw_literal(x):
    """upstream's `dtw_cpu`, transcribed: the double loop, in fp32"""
    N, M = x.shape
    cost = np.ones((N + 1, M + 1), dtype=np.float32) * np.inf
    trace = -np.ones((N + 1, M + 1), dtype=np.float32)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0 = cost[i - 1, j - 1]
            c1 = cost[i - 1, j]
            c2 = cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = x[i - 1, j - 1] + c
            trace[i, j] = t
    return AO.backtrace(trace)


def test_dtw_oracle_equals_the_literal_double_loop():
    cases = [AO.dtw_matrix(N, M, kind, seed=i) for i, (N, M, kind) in enumerate(AO.DTW_TIE_CASES)]
    cases += [AO.dtw_matrix(N, M, "randn", seed=10 + i) for i, (N, M) in enumerate([(1, 1), (1, 9), (9, 1), (2, 3), (13, 31), (31, 13)])]
    for x in cases:
        a, b = AO.dtw_ref(x), _dtw_literal(x)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), x.shape
        assert a[0][0] == 0 and a[1][0] == 0 and a[0][-1] == x.shape[0] - 1 and a[1][-1] == x.shape[1] - 1
        assert len(a[0]) <= x.shape[0] + x.shape[1] - 1
    # an all-equal matrix: no predecessor is ever strictly smaller, so the path runs along the last row and up the first column
    t, f = AO.dtw_ref(AO.dtw_matrix(3, 4, "equal"))
    assert t.tolist() == [0, 1, 2, 2, 2, 2] and f.tolist() == [0, 0, 0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------ jumps and words
def test_words_arithmetic_on_hand_written_paths():
    # 3 text tokens (rows 1..3; row 0 is the no-timestamps token) + the eot's start: words of 2 and 1 tokens, then the eot
    text, time = [0, 0, 1, 2, 2, 2, 3], [0, 1, 2, 3, 4, 5, 6]
    tokens, probs = [11, 12, 13], [0.5, 0.25, 1.0]
    # jumps at entries 0, 2, 3, 6 -> times 0.00, 0.04, 0.06, 0.12; bounds [0, 2, 3]
    want = [(0.0, 0.06, 0.375, [11, 12]), (0.06, 0.12, 1.0, [13])]
    assert AO.words_ref(text, time, [2, 1, 1], probs, tokens) == want
    assert D.alignment_words(text, time, [2, 1, 1], probs, tokens) == want
    # every token its own word
    want1 = [(0.0, 0.04, 0.5, [11]), (0.04, 0.06, 0.25, [12]), (0.06, 0.12, 1.0, [13])]
    assert AO.words_ref(text, time, [1, 1, 1, 1], probs, tokens) == want1
    assert D.alignment_words(text, time, [1, 1, 1, 1], probs, tokens) == want1
    # a path that takes several rows at one frame: those words start and end at the same time
    text2, time2 = [0, 1, 2, 3, 3], [0, 0, 0, 0, 1]
    got = D.alignment_words(text2, time2, [1, 1, 1, 1], probs, tokens)
    assert got == AO.words_ref(text2, time2, [1, 1, 1, 1], probs, tokens) == [(0.0, 0.0, 0.5, [11]), (0.0, 0.0, 0.25, [12]), (0.0, 0.0, 1.0, [13])]
    # only the eot word: nothing to time
    assert D.alignment_words(text, time, [4], probs, tokens) == [] == AO.words_ref(text, time, [4], probs, tokens)
    with pytest.raises(ValueError):
        D.alignment_words(text, time, [2, 1], probs, tokens)  # the counts must cover text + [eot]


# ------------------------------------------------------------------------------------------------ the head dump
def test_alignment_head_dump_round_trips():
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(6, 8, generator=g) < 0.2
    dump = D.dump_alignment_heads(mask.numpy())
    assert isinstance(dump, bytes)
    assert torch.equal(D.parse_alignment_heads(dump, 6, 8), mask)
    assert torch.equal(D.parse_alignment_heads(dump.decode(), 6, 8), mask)
    assert torch.equal(D.parse_alignment_heads(mask, 6, 8), mask)
    assert torch.equal(D.parse_alignment_heads(mask.to_sparse(), 6, 8), mask)
    with pytest.raises(ValueError):
        D.parse_alignment_heads(dump, 6, 7)
    with pytest.raises(ValueError):
        D.parse_alignment_heads(mask.float(), 6, 8)


def test_set_alignment_heads_replaces_the_buffer_and_keeps_the_default():
    from whisper_finetune.engine.whisper_model import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(80, 100, 128, 2, 2, 256, 32, 128, 2, 4))
    default = m.alignment_heads.to_dense()
    assert default[2:].all() and not default[:2].any()  # every head of the upper half of the decoder
    mask = torch.zeros(4, 2, dtype=torch.bool)
    mask[0, 1] = mask[3, 0] = True
    m.set_alignment_heads(D.dump_alignment_heads(mask))
    assert m.alignment_heads.is_sparse and torch.equal(m.alignment_heads.to_dense(), mask)
    assert "alignment_heads" not in m.state_dict()
    slots, n_sel = D.alignment_slots(m, torch.device("cpu"))
    assert n_sel == 2 and [(v[0].tolist(), v[1]) for v in slots.values()] == [([1], 0), ([0], 1)]
    assert list(slots) == [m.decoder.blocks[0].cross_attn, m.decoder.blocks[3].cross_attn]
    with pytest.raises(ValueError):
        m.set_alignment_heads(torch.zeros(2, 2, dtype=torch.bool))
