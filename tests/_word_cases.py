"""Cases, float64 reference and bound for wft_word_spans (csrc/align.hip; include/wft.h "Word-level alignment"), shared by
tests/test_word_host.py (CPU: the reference against D.alignment_words, the mutants) and tests/test_word_spans_gpu.py (the kernel).

A case is a ragged batch of B = 3 audios: DTW-shaped paths (from (0, 0), every step moves one row, one frame or both; rows never
decrease and every row occurs), word boundaries, packed token probabilities, and output buffers pre-filled with a sentinel.

The reference is `alignment_words`' arithmetic on integer frames: jumps = position 0 and every position at which the text index
changes, first[k] = path_time at the k-th jump, start = first[bounds[w]], end = first[bounds[w + 1]], probability = the float64
mean of the word's token probabilities.

Bound for the probability of a word of n tokens: |got - ref| <= n * 2^-23 * ref + 2^-149.  The fp32 running sum of n non-negative
terms followed by one division has the relative error bound gamma_n with u = 2^-24, first-order term n * 2^-24 (the division's
rounding included: n - 1 additions and one division); the bound allows twice that, and one fp32 subnormal step for a result that
underflows.  Frames are compared exactly."""
import numpy as np

SENT_I, SENT_F = -77, -77.5   # what the output buffers hold before the launch


def path_of(moves: str):
    """'d' = next row and next frame, 'v' = next row at the same frame, 'h' = next frame in the same row; from (0, 0)."""
    t, f = [0], [0]
    for m in moves:
        t.append(t[-1] + (m in "dv"))
        f.append(f[-1] + (m in "dh"))
    return t, f


def _case(name, audios, pad_words=2):
    """audios: per audio (moves or None for an empty path, counts over text + [eot], token probabilities)."""
    B = len(audios)
    paths = [path_of(a[0]) if a[0] is not None else ([], []) for a in audios]
    ld_path = max(max(len(p[0]) for p in paths), 1) + 3
    path_text = np.full((B, ld_path), -1, dtype=np.int32)
    path_time = np.full((B, ld_path), -1, dtype=np.int32)
    path_len = np.zeros(B, dtype=np.int32)
    n_words = np.array([len(a[1]) - 1 for a in audios], dtype=np.int32)
    ld_words = int(n_words.max()) + pad_words
    bounds = np.zeros((B, ld_words + 1), dtype=np.int32)
    tok_off, probs, at = [], [], 0
    for b, (moves, counts, tp) in enumerate(audios):
        t, f = paths[b]
        path_text[b, :len(t)], path_time[b, :len(t)], path_len[b] = t, f, len(t)
        bounds[b, 1:len(counts)] = np.cumsum(counts[:-1])
        bounds[b, len(counts):] = 10 ** 6      # behind the live entries: must not be read into an address
        n_text = sum(counts) - 1
        assert len(tp) == n_text and (not t or t[-1] == n_text), (name, b)   # rows: the no-timestamps row + the text, the eot cut
        tok_off.append(at)
        probs.extend(tp)
        at += n_text
    return dict(name=name, B=B, path_text=path_text, path_time=path_time, path_len=path_len, bounds=bounds, n_words=n_words,
                token_probs=np.array(probs, dtype=np.float32), tok_off=np.array(tok_off, dtype=np.int32), ld_words=ld_words,
                counts=[a[1] for a in audios], n_rows_max=max(sum(a[1]) for a in audios))


def _probs(rng, n, lo=-3.0):
    return (10.0 ** rng.uniform(lo, 0.0, n)).astype(np.float32).tolist()


def cases():
    rng = np.random.default_rng(5)
    out = []
    # one word; one-token words next to an 8-token word; an empty path (its words must stay sentinels)
    out.append(_case("one_word_8_token_word_empty_path", [
        ("dhhdhd", [3, 1], _probs(rng, 3)),
        ("hdhhddvdhhhddhdvhddh", [1, 8, 1, 1, 1], _probs(rng, 11)),
        (None, [2, 1, 1], _probs(rng, 3)),
    ]))
    # vertical runs (several rows at one frame: words of zero length), horizontal runs, and a last row that first occurs at the
    # path's last entry (the path ends on 'v'); audio 2 starts with a vertical run at frame 0
    out.append(_case("vertical_horizontal_runs_last_entry", [
        ("hhhvvvhhhhdvvhhhhhhv", [2, 1, 2, 1, 1, 1], _probs(rng, 7)),
        ("dv", [1, 1, 1], _probs(rng, 2)),
        ("vvvhhhhhdhv", [1, 1, 2, 1, 1], _probs(rng, 5)),
    ]))
    # probabilities from 1e-30 to 1 inside one word, whole words near 1e-30, and exact ones
    tiny = [1e-30, 1.0, 3e-12, 0.25, 7e-21, 1e-30, 2e-30, 1e-30, 1.0, 1.0, 1.0, 0.999999, 1e-7]
    out.append(_case("probabilities_1e-30_to_1", [
        ("d" * 13, [5, 3, 3, 2, 1], tiny),
        ("hdhdhd", [1, 1, 1, 1], [1e-30, 1.0, 5e-16]),
        ("dhhd", [2, 1], [6e-8, 1e-30]),
    ]))
    # a path longer than the kernel's 2048-entry LDS chunk: rows that first occur in the second chunk
    long_moves = "h" * 2100 + "d" * 40 + "vh" * 30 + "v"
    out.append(_case("path_beyond_one_chunk", [
        (long_moves, [7] * 10 + [1, 1], _probs(rng, 71)),
        ("dd", [1, 1, 1], _probs(rng, 2)),
        (None, [1, 1], _probs(rng, 1)),
    ]))
    return out


def fresh_outputs(case):
    B, ld = case["B"], case["ld_words"]
    return np.full((B, ld), SENT_I, dtype=np.int32), np.full((B, ld), SENT_I, dtype=np.int32), np.full((B, ld), SENT_F, dtype=np.float32)


def spans_ref(case, b):
    """float64 reference for audio b -> (start frames, end frames, probabilities, token counts), or None for an audio that writes nothing"""
    L, nw = int(case["path_len"][b]), int(case["n_words"][b])
    if L == 0 or nw == 0:
        return None
    ti, tj = case["path_text"][b, :L].astype(np.int64), case["path_time"][b, :L].astype(np.int64)
    jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
    first = tj[jumps]
    bd = case["bounds"][b, :nw + 1].astype(np.int64)
    tp = case["token_probs"].astype(np.float64)[int(case["tok_off"][b]):]
    prob = np.array([tp[i:j].mean() for i, j in zip(bd[:-1], bd[1:])])
    return first[bd[:-1]], first[bd[1:]], prob, bd[1:] - bd[:-1]


def prob_bound(ref, n):
    return n * 2.0 ** -23 * ref + 2.0 ** -149


def check(case, start, end, prob):
    """The whole check of one launch's outputs (numpy arrays [B, ld_words]) -> worst |err| / bound; raises AssertionError."""
    worst = 0.0
    for b in range(case["B"]):
        ref = spans_ref(case, b)
        nw = 0 if ref is None else len(ref[0])
        assert (start[b, nw:] == SENT_I).all() and (end[b, nw:] == SENT_I).all() and (prob[b, nw:] == np.float32(SENT_F)).all(), \
            f"{case['name']}, audio {b}: an element at or beyond n_words (or of a skipped audio) was written"
        if ref is None:
            continue
        s, e, p, n = ref
        assert np.array_equal(start[b, :nw], s), f"{case['name']}, audio {b}: start frames {start[b, :nw].tolist()} != {s.tolist()}"
        assert np.array_equal(end[b, :nw], e), f"{case['name']}, audio {b}: end frames {end[b, :nw].tolist()} != {e.tolist()}"
        ratio = np.abs(prob[b, :nw].astype(np.float64) - p) / prob_bound(p, n)
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), f"{case['name']}, audio {b}: probability off by {ratio.max():.3g} bounds: {prob[b, :nw].tolist()} vs {p.tolist()}"
    return worst


MUTANTS = ("last_occurrence", "bounds_lo_shifted", "bounds_hi_shifted", "mean_wrong_range", "mean_over_n_plus_1", "mean_over_n_minus_1",
           "eot_word_kept", "fp16_sum")


def restate(case, mutant=None, dtype=np.float32):
    """The kernel restated in numpy, one fp32 running sum per word -> (start, end, prob) in sentinel-filled buffers; `mutant`
    plants one of MUTANTS."""
    start, end, prob = fresh_outputs(case)
    acc_t = np.float16 if mutant == "fp16_sum" else dtype
    for b in range(case["B"]):
        L, nw = int(case["path_len"][b]), int(case["n_words"][b])
        if L == 0 or nw == 0:
            continue
        text, time = case["path_text"][b, :L], case["path_time"][b, :L]
        first = {}
        for p in range(L):
            r = int(text[p])
            if mutant == "last_occurrence" or r not in first:
                first[r] = int(time[p])
        bd = [int(v) for v in case["bounds"][b, :nw + 1]]
        if mutant == "eot_word_kept":
            bd.append(bd[-1] + 1)
        off = int(case["tok_off"][b])
        for w in range(len(bd) - 1):
            lo, hi = bd[w], bd[w + 1]
            a, z = lo, hi
            if mutant == "bounds_lo_shifted":
                a = max(lo - 1, 0)
            if mutant == "bounds_hi_shifted":
                z = min(hi + 1, max(first))
            start[b, w], end[b, w] = first.get(a, -1), first.get(z, -1)
            i0, i1 = (lo + 1, hi + 1) if mutant == "mean_wrong_range" else (lo, hi)
            acc = acc_t(0)
            for i in range(i0, i1):
                acc = acc_t(acc + acc_t(case["token_probs"][min(off + i, len(case["token_probs"]) - 1)]))
            n = hi - lo + (mutant == "mean_over_n_plus_1") - (mutant == "mean_over_n_minus_1")
            prob[b, w] = np.float32(dtype(acc) / dtype(n)) if n > 0 else np.float32(np.inf)
    return start, end, prob
