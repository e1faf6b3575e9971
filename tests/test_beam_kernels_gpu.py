"""GPU checks of the beam-search kernels (csrc/decode_beam.hip, csrc/decode_attn.hip) through the C ABI: wft_decode_topk against torch.log_softmax(...).topk,
wft_beam_update against the plain-Python oracle (tests/_beam_oracle.py) on the SAME candidate lists, and the two forms of
wft_attn_decode_beam_bf16 against wft_attn_decode_bf16 — bit for bit where include/wft.h says so, at the fp32-math bound of
tests/test_decode_kernels_gpu.py elsewhere."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _beam_oracle as BO  # noqa: E402
from tests.test_decode_kernels_gpu import ALL_LONG, PER_HEAD_TOL, _ref_decode, close, close_per_head  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
LOG2E = 1.4426950408889634
I32 = dict(dtype=torch.int32, device=DEV)


def bits(t):
    return t.detach().cpu().view(torch.int16)


# ----------------------------------------------------------------------------- wft_decode_topk
def _masked(logits, V, sup, sup_first, first_rows):
    x = logits[:, :V].float().clone()
    if sup is not None:
        x = x.masked_fill(sup.bool()[None, :], float("-inf"))
    if sup_first is not None:
        x[first_rows] = x[first_rows].masked_fill(sup_first.bool()[None, :], float("-inf"))
    return x


def _run_topk(logits, V, k, sup, sup_first, lens, first_len, row_step=1):
    R = logits.shape[0] * row_step
    tok = torch.full((R, k), -5, **I32)
    lp = torch.full((R, k), 7.0, dtype=torch.float32, device=DEV)
    K.decode_topk(logits.to(DEV), V, tok, lp, lens=lens.to(DEV), first_len=first_len.to(DEV),
                  suppress=None if sup is None else sup.to(DEV), suppress_first=None if sup_first is None else sup_first.to(DEV), row_step=row_step)
    return tok.cpu(), lp.cpu()


@pytest.mark.parametrize("V", [51865, 51866])
@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("k", [2, 6, 9])
def test_topk_on_crafted_rows(V, masks, k):
    """Rows whose leading values are planted: distinct ones (torch.topk's indices are then defined) and tied groups (the lower
    token id first).  Indices exact, log-probabilities within 1e-4 absolute of torch.log_softmax over the live columns — the bound
    test_pick_matches_masked_argmax_and_log_softmax uses for the same arithmetic (an fp32 sum of V exponentials in another order)."""
    B, ld = 6, K.round_up(V, 128)
    g = torch.Generator().manual_seed(V + k)
    logits = (torch.randn(B, ld, generator=g) * 2).to(BF)
    logits[:, V:] = 1000.0  # padded columns must never appear
    cols = torch.stack([torch.randperm(V, generator=g)[:12] for _ in range(B)])
    for b in range(B):
        logits[b, cols[b]] = torch.arange(30, 18, -1).to(BF) * 0.5  # 15.0, 14.5, ..: distinct, exact in bf16, far above 2 * randn
    logits[1, V - 1] = 15.5  # the last column of the row (V odd / even: the 16-byte tail)
    # planted ties: rows 2 and 3 hold the same value in several columns
    tie2 = sorted(cols[2][:4].tolist()); logits[2, tie2] = 16.0
    tie3 = sorted(cols[3][2:7].tolist()); logits[3, tie3] = 13.0
    sup = sup_first = None
    first_len = torch.tensor([3, 3, 3, 3, 2, 2], dtype=torch.int32)
    lens = torch.full((B,), 3, dtype=torch.int32)  # rows 0-3 are at their first token, rows 4-5 past it
    if masks:
        sup = torch.zeros(V, dtype=torch.uint8); sup[torch.randint(0, V, (500,), generator=g)] = 1
        sup_first = torch.zeros(V, dtype=torch.uint8); sup_first[torch.randint(0, V, (300,), generator=g)] = 1
        sup[tie2] = 0; sup_first[tie2] = 0; sup[tie3] = 0; sup_first[tie3] = 0
        sup[cols[4][0]] = 0
        sup[cols[0][0]] = 1        # row 0's best is suppressed
        sup_first[cols[0][1]] = 1  # its second by the first-token mask
        sup_first[cols[4][0]] = 1  # row 4 is past its first token: its best stays
        sup[tie2[1]] = 1           # a member of the tied group drops out
    tok, lp = _run_topk(logits, V, k, sup, sup_first, lens, first_len)
    x = _masked(logits, V, sup, sup_first, slice(0, 4))
    ref = torch.log_softmax(x, -1)
    for b in range(B):
        order = np.lexsort((np.arange(V), -x[b].numpy()))[:k]  # value descending, then the lower id
        assert tok[b].tolist() == order.tolist(), (b, tok[b].tolist(), order.tolist())
        if b not in (2, 3):  # no ties near the top: torch.topk's own indices are defined
            assert tok[b].tolist() == ref[b].topk(k).indices.tolist()
    want = ref.gather(1, tok.long())
    err = (lp - want).abs().max().item()
    print(f"top-{k} log-probabilities, V={V}, masks={masks}: max |err| vs torch.log_softmax {err:.3e}")
    assert err < 1e-4
    assert (lp[:, :-1] >= lp[:, 1:]).all()
    if masks:
        assert int(cols[0][0]) not in tok[0].tolist() and int(cols[0][1]) not in tok[0].tolist() and int(tok[4, 0]) == int(cols[4][0])
        assert tie2[1] not in tok[2].tolist()
    assert tok[2, :2].tolist() == [t for t in tie2 if not (masks and t == tie2[1])][:2]


@pytest.mark.parametrize("V", [51865, 51866])
def test_topk_on_random_bf16_rows(V):
    """Random bf16 rows tie near the top and torch's tie order is unspecified: compare the VALUES with torch.topk's and check every
    returned index's own logit; ties must come in ascending id."""
    B, k, ld = 8, 6, K.round_up(V, 128)
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(B, ld, generator=g) * 3).to(BF)
    sup = torch.zeros(V, dtype=torch.uint8); sup[torch.randint(0, V, (2000,), generator=g)] = 1
    lens = torch.full((B,), 4, dtype=torch.int32)
    tok, lp = _run_topk(logits, V, k, sup, None, lens, lens.clone())
    x = _masked(logits, V, sup, None, slice(0, 0))
    ref = torch.log_softmax(x, -1)
    top = ref.topk(k)
    assert (lp - top.values).abs().max().item() < 1e-4
    assert (lp - ref.gather(1, tok.long())).abs().max().item() < 1e-4
    for b in range(B):
        assert len(set(tok[b].tolist())) == k and not sup[tok[b].long()].any()
        vals = x[b, tok[b].long()]
        assert torch.equal(vals, x[b].topk(k).values)  # the logits themselves: exact
        for i in range(k - 1):
            assert vals[i] > vals[i + 1] or tok[b, i] < tok[b, i + 1]


def test_topk_first_form_and_short_rows():
    """row_step = W: one logits row per audio fills the candidate row of beam 0 and leaves the others alone; a row with fewer than k
    live columns is padded with (-1, -inf)."""
    V, ld, W = 40, 128, 3
    logits = torch.zeros(2, ld).to(BF)
    logits[0, :V] = torch.arange(V).to(BF) * 0.25
    logits[1, [3, 7]] = 5.0
    sup = torch.ones(V, dtype=torch.uint8); sup[[3, 7, 9]] = 0
    lens = torch.full((2 * W,), 2, dtype=torch.int32)
    tok, lp = _run_topk(logits, V, W + 1, sup, None, lens, lens.clone(), row_step=W)
    assert tok[0].tolist() == [9, 7, 3, -1] and tok[3].tolist() == [3, 7, 9, -1]
    assert lp[0, 3] == float("-inf") and (tok[[1, 2, 4, 5]] == -5).all() and (lp[[1, 2, 4, 5]] == 7.0).all()
    ref = torch.log_softmax(torch.tensor([5.0, 5.0, 0.0]), 0)
    assert (lp[3, :3] - ref).abs().max() < 1e-5


# ----------------------------------------------------------------------------- wft_beam_update
class _DevState:
    """The device-side state of wft_beam_update, initialised as BeamCache.start does."""

    def __init__(self, prompts, W, C, eot, max_len, n_ctx):
        B = len(prompts)
        R = B * W
        self.B, self.W, self.C, self.eot, self.max_len, self.n_ctx = B, W, C, eot, max_len, n_ctx
        tokens = torch.full((R, n_ctx), eot, dtype=torch.int64)
        lens = torch.zeros(R, dtype=torch.int32)
        anc = torch.zeros((R, n_ctx), dtype=torch.int32)
        for a, p in enumerate(prompts):
            tokens[a * W:(a + 1) * W, :len(p)] = torch.tensor(p)
            lens[a * W:(a + 1) * W] = len(p)
            anc[a * W:(a + 1) * W] = a * W
        self.tokens, self.len, self.anc = tokens.to(DEV), lens.to(DEV), anc.to(DEV)
        self.slp = torch.zeros(R, dtype=torch.float32, device=DEV)
        self.done = torch.tensor([int(len(p) >= max_len) for p in prompts], **I32)
        self.unfinished = torch.full((1,), -1, **I32)
        self.fin_tokens = torch.full((B, C, n_ctx), eot, dtype=torch.int64, device=DEV)
        self.fin_len = torch.zeros((B, C), **I32)
        self.fin_score = torch.zeros((B, C), dtype=torch.float32, device=DEV)
        self.fin_n = torch.zeros(B, **I32)
        self.src = torch.full((R,), -1, **I32)

    def load_history(self, st, rng, vocab):
        """Replace the state of a fresh start() by one in the middle of a decode, on the device and in the oracle `st` alike: every
        beam has its own tokens (drawn from `vocab`, which must not hold eot), its own score on the coarse grid of _random_cands,
        and an ancestry row that names other slots of its audio — so a row permutation moves values that tell the rows apart in
        EVERY column, and the steps that follow are ordinary ones (first = False)."""
        W = self.W
        tokens, anc, slp = self.tokens.cpu(), self.anc.cpu(), self.slp.cpu()
        for au in st.audios:
            n = au.first_len
            for j, b in enumerate(au.beams):
                r = au.a * W + j
                b.tokens = [int(t) for t in rng.choice(vocab, size=n)]
                b.anc = [au.a * W + int(s) for s in rng.integers(0, W, size=n)]  # (entry n - 1 is never read: the step that appends overwrites it)
                b.slp = np.float32(-0.125 * int(rng.integers(0, 40)))
                tokens[r, :n] = torch.tensor(b.tokens)
                anc[r, :n - 1] = torch.tensor(b.anc[:n - 1], dtype=torch.int32)
                slp[r] = float(b.slp)
            au.first = False
        self.tokens.copy_(tokens); self.anc.copy_(anc); self.slp.copy_(slp)

    def update(self, cand_tok, cand_logp, first):
        K.beam_update(cand_tok.to(DEV), cand_logp.to(DEV), self.tokens, self.anc, self.len, self.slp, self.done, self.unfinished,
                      self.fin_tokens, self.fin_len, self.fin_score, self.fin_n, eot=self.eot, max_len=self.max_len, first=first,
                      src_out=self.src)

    def check(self, st, what):
        """Every integer output exact, scores bit-equal to the oracle's fp32 adds."""
        W = self.W
        tokens, lens, anc, slp = self.tokens.cpu(), self.len.cpu().tolist(), self.anc.cpu(), self.slp.cpu().numpy()
        fin_tokens, fin_len, fin_score, fin_n = self.fin_tokens.cpu(), self.fin_len.cpu().tolist(), self.fin_score.cpu().numpy(), self.fin_n.cpu().tolist()
        src = self.src.cpu().tolist()
        assert self.done.cpu().tolist() == [int(au.done) for au in st.audios], what
        assert int(self.unfinished) == st.unfinished, what
        for au in st.audios:
            for j, b in enumerate(au.beams):
                r = au.a * W + j
                n = len(b.tokens)
                assert lens[r] == n, (what, r)
                assert tokens[r, :n].tolist() == b.tokens and (tokens[r, n:] == self.eot).all(), (what, r)
                assert anc[r, :n - 1].tolist() == b.anc[:n - 1] and (anc[r, n - 1:] == au.a * W).all(), (what, r, anc[r, :n].tolist(), b.anc)
                assert slp[r].tobytes() == np.float32(b.slp).tobytes(), (what, r, slp[r], b.slp)
                if au.src is not None:
                    assert src[r] == au.src[j], (what, r)
            assert fin_n[au.a] == len(au.fin), what
            for p, (t, s) in enumerate(au.fin):
                assert fin_len[au.a][p] == len(t) and fin_tokens[au.a, p, :len(t)].tolist() == t and (fin_tokens[au.a, p, len(t):] == self.eot).all()
                assert fin_score[au.a, p].tobytes() == np.float32(s).tobytes(), (what, p)
            for p in range(len(au.fin), self.C):
                assert fin_len[au.a][p] == 0 and (fin_tokens[au.a, p] == self.eot).all()


def _random_cands(rng, R, W, vocab, eot, p_eot):
    """Per row W + 1 distinct tokens (eot among them with probability p_eot, anywhere in the list) and descending log-probabilities
    on a coarse grid, so equal scores happen."""
    tok = np.zeros((R, W + 1), dtype=np.int32)
    lp = np.zeros((R, W + 1), dtype=np.float32)
    p_eot = np.broadcast_to(np.asarray(p_eot, dtype=np.float64), (R,))  # (one probability, or one per row)
    for r in range(R):
        t = rng.choice(vocab, size=W + 1, replace=False)
        if rng.random() < p_eot[r]:
            t[rng.integers(0, W + 1)] = eot
        tok[r] = t
        lp[r] = -np.sort(rng.integers(1, 24, size=W + 1)).astype(np.float32) * np.float32(0.125)
    return torch.from_numpy(tok), torch.from_numpy(lp)


def _as_lists(tok, lp, B, W):
    return [[[(int(tok[a * W + j, i]), np.float32(lp[a * W + j, i])) for i in range(W + 1)] for j in range(W)] for a in range(B)]


@pytest.mark.parametrize("W,patience,p_eot", [(5, 1.0, 0.5), (5, 2.0, 0.9), (5, 0.5, 0.4), (8, 1.0, 0.6), (1, 1.0, 0.3), (3, 1.0, 0.0), (2, 3.0, 1.0)])
def test_beam_update_follows_the_oracle_on_the_same_candidates(W, patience, p_eot):
    """Random candidate lists over many steps: eot among the candidates, lists filling to C, the first form, audios done at different
    steps (and frozen while the others go on), one audio that starts at max_len, lengths reaching max_len."""
    eot, n_ctx, max_len = 3, 24, 19
    prompts = [[7, 8, 9], [7], [5] * 19, [6] * 12, [4, 4]]
    B, C = len(prompts), BO.candidates(W, patience)
    rng = np.random.default_rng(W * 100 + int(patience * 10))
    vocab = np.array([t for t in range(10, 10 + 3 * W + 6)] + [0, 1, 2])
    st = BO.State(prompts, W, C, eot, max_len)
    dv = _DevState(prompts, W, C, eot, max_len, n_ctx)
    assert st.audios[2].done
    steps = 0
    for i in range(max_len + 2):  # (past everybody's end: frozen audios stay frozen)
        tok, lp = _random_cands(rng, B * W, W, vocab, eot, p_eot)
        dv.update(tok, lp, first=i == 0)
        BO.step_candidates(st, _as_lists(tok.numpy(), lp.numpy(), B, W))
        dv.check(st, f"step {i}")
        steps += st.unfinished > 0
    assert st.unfinished == 0
    ends = sorted(len(au.beams[0].tokens) - au.first_len for au in st.audios)
    print(f"W={W} C={C}: steps taken per audio {ends}, finished {[len(au.fin) for au in st.audios]}")
    if p_eot > 0.3 and C <= 2 * W:
        assert any(len(au.fin) == C for au in st.audios), "no finished list filled: the case does not test what it says"
    if p_eot == 0.0:
        assert all(len(au.fin) == 0 for au in st.audios)


@pytest.mark.parametrize("W", [5, 8])
def test_beam_update_permutes_columns_beyond_256(W):
    """The token buffer at its full width (n_ctx = max_len = 448): the kernel permutes rows of `tokens` and `anc` one column per
    thread, 256 threads, so columns 256 and up are the SECOND trip of that loop.  Prompts of 3, 250, 255, 256, 257, 440, 447 and 448
    tokens, loaded as a decode in progress (_DevState.load_history: per-beam tokens, scores and ancestry), random candidates until
    every audio is done, the whole state compared with the oracle after every step as in the test above.  Which audio sees eot when
    is arranged so that both ends are reached behind column 256: the 3-token audio sees none for 300 steps and then fills its
    finished list (the copy into fin_tokens runs over columns >= 256 too), the 250-token one never does and ends at max_len."""
    eot, n_ctx, max_len = 3, 448, 448
    plens = [3, 250, 255, 256, 257, 440, 447, 448]
    B, C = len(plens), BO.candidates(W)
    rng = np.random.default_rng(4480 + W)
    vocab = np.array([t for t in range(10, 10 + 3 * W + 6)] + [0, 1, 2])
    prompts = [[5] * n for n in plens]
    st = BO.State(prompts, W, C, eot, max_len)
    dv = _DevState(prompts, W, C, eot, max_len, n_ctx)
    dv.load_history(st, rng, vocab)
    assert st.audios[7].done and st.unfinished == B - 1
    before = dv.tokens.cpu().clone()
    moved_late = fin_late = 0
    for i in range(max_len):
        p = np.repeat([0.0 if i < 300 else 0.5, 0.0, 0.3, 0.05, 0.5, 0.3, 0.5, 0.5], W)
        tok, lp = _random_cands(rng, B * W, W, vocab, eot, p)
        dv.update(tok, lp, first=False)
        BO.step_candidates(st, _as_lists(tok.numpy(), lp.numpy(), B, W))
        dv.check(st, f"step {i}")
        after = dv.tokens.cpu()
        lens = dv.len.cpu().tolist()
        for r in range(B * W):  # columns >= 256 inside the hypothesis (its newest token aside) whose value changed: a row really moved
            moved_late += int((after[r, 256:max(lens[r] - 1, 256)] != before[r, 256:max(lens[r] - 1, 256)]).sum())
        before = after.clone()
        if st.unfinished == 0:
            break
    assert st.unfinished == 0
    fin_late = sum(len(t) > 257 for au in st.audios for t, _ in au.fin)
    ends = [len(au.beams[0].tokens) for au in st.audios]
    print(f"W={W}: lengths at the end {ends}, finished {[len(au.fin) for au in st.audios]}; {moved_late} token values in columns >= 256 "
          f"changed by a reorder, {fin_late} finished sequences longer than 257 tokens")
    assert ends[1] == max_len and ends[7] == max_len and ends[0] > 300
    assert moved_late > 0 and fin_late > 0 and len(st.audios[0].fin) == C


def test_beam_update_crafted_ties_and_dropped_eot():
    """The host test's tie case on the device: equal scores go to the lower beam, then the lower list position; an eot ranked below
    the W-th saved beam is dropped."""
    W, eot = 2, 2
    dv = _DevState([[9]], W, 2, eot, 10, 16)
    st = BO.State([[9]], W, 2, eot, 10)
    seq = [([[4, 5, 6], [0, 0, 0]], True), ([[7, 8, 3], [1, 0, 3]], False), ([[7, eot, 3], [eot, 0, 3]], False)]
    for rows, first in seq:
        tok = torch.tensor(rows, dtype=torch.int32)
        lp = torch.full((W, W + 1), -1.0)
        dv.update(tok, lp, first)
        BO.step_candidates(st, _as_lists(tok.numpy(), lp.numpy(), 1, W))
        dv.check(st, str(rows))
    assert dv.src.cpu().tolist() == [0, 0] and dv.tokens[:, 3].cpu().tolist() == [7, 3] and int(dv.fin_n) == 1
    assert dv.fin_tokens[0, 0, :4].cpu().tolist() == [9, 4, 7, eot]


# ----------------------------------------------------------------------------- wft_attn_decode_beam_bf16, self form
RAGGED = [1, 2, 63, 64, 65, 447, 448]


def _scrambled_anc(R, cap, lens, g):
    """Random slots, except that — as in beam search, where the rows that can see each other share one length — no entry points at
    a position this very step writes (slot s, position lens[s] - 1): such an entry names its own row instead."""
    anc = torch.randint(0, R, (R, cap), generator=g, dtype=torch.int32)
    written = torch.tensor(lens)[anc.long()] - 1 == torch.arange(cap)[None, :]
    return torch.where(written, torch.arange(R, dtype=torch.int32)[:, None].expand(-1, cap), anc)


@pytest.mark.parametrize("H,lens", [(6, [5]), (6, RAGGED), (20, RAGGED), (20, (RAGGED * 5)[:30])])
@pytest.mark.parametrize("prescaled", [False, True])
def test_self_form_is_bit_identical_to_the_gathered_cache(H, lens, prescaled):
    """A scrambled ancestry table: hypothesis r reads position t at slot anc[r, t].  The output equals wft_attn_decode_bf16 on the
    physically gathered cache bit for bit; the append lands in slot r at len[r] - 1 and no other byte of the slot cache changes;
    anc[r, len - 1:] (garbage here, out of range included) is not used."""
    R, D, cap = len(lens), H * 64, 448
    g = torch.Generator().manual_seed(R * 131 + H)
    slots = torch.randn(R, cap, 2 * D, generator=g).to(BF)
    qkv = torch.randn(R, 3 * D, generator=g).to(BF)
    scale = 0.125
    if prescaled:
        qkv[:, :D] = (qkv[:, :D].float() * (scale * LOG2E)).to(BF)
    anc = _scrambled_anc(R, cap, lens, g)
    gathered = slots[anc.long(), torch.arange(cap)[None, :]]  # [R, cap, 2D]: row r, position t from slot anc[r, t]
    for r, n in enumerate(lens):
        anc[r, n - 1:] = torch.tensor([10 ** 6, -3, R] * cap)[:cap - n + 1]
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    qd = qkv.to(DEV)
    gd = gathered.to(DEV)
    want = K.attn_decode(qd[:, :D], gd, H, scale, new_kv=(qd[:, D:2 * D], qd[:, 2 * D:]), lens=lens_t, q_prescaled=prescaled)
    after = slots.clone()
    for r, n in enumerate(lens):
        after[r, n - 1] = qkv[r, D:]
    for _ in range(2):
        sd = slots.to(DEV)
        got = K.attn_decode_beam(qd[:, :D], sd, H, scale, new_kv=(qd[:, D:2 * D], qd[:, 2 * D:]), lens=lens_t, anc=anc.to(DEV), q_prescaled=prescaled)
        assert torch.equal(bits(got), bits(want)), (bits(got) != bits(want)).sum()
        assert torch.equal(bits(sd), bits(after)), "the append must land in slot r at len[r] - 1 and nothing else may change"
    # (and the existing kernel is itself held to fp32 math by tests/test_decode_kernels_gpu.py; once more here on the gathered cache)
    full = gathered.clone()
    for r, n in enumerate(lens):
        full[r, n - 1] = qkv[r, D:]
    close(got, _ref_decode(qkv[:, :D], full[..., :D], full[..., D:], lens, H, math.log(2.0) if prescaled else scale), 2e-2, f"self form R*H={R * H}")


@pytest.mark.parametrize("H", [6, 20])
@pytest.mark.parametrize("prescaled", [False, True])
def test_self_form_long_rows_per_head(H, prescaled):
    """Every hypothesis between 225 and 448 keys behind a scrambled ancestry table (every wave owns keys, the index prefetch two
    blocks ahead fetches live blocks): each (row, head) within 2^-7 of its own largest fp64 reference value (close_per_head), and
    bit-identical to wft_attn_decode_bf16 on the gathered cache as above."""
    lens = ALL_LONG
    R, D, cap = len(lens), H * 64, 448
    g = torch.Generator().manual_seed(R * 613 + H)
    slots = torch.randn(R, cap, 2 * D, generator=g).to(BF)
    qkv = torch.randn(R, 3 * D, generator=g).to(BF)
    scale = 0.125
    if prescaled:
        qkv[:, :D] = (qkv[:, :D].float() * (scale * LOG2E)).to(BF)
    anc = _scrambled_anc(R, cap, lens, g)
    gathered = slots[anc.long(), torch.arange(cap)[None, :]]
    full = gathered.clone()
    for r, n in enumerate(lens):
        full[r, n - 1] = qkv[r, D:]
    ref = _ref_decode(qkv[:, :D], full[..., :D], full[..., D:], lens, H, math.log(2.0) if prescaled else scale, dtype=torch.float64)
    lens_t = torch.tensor(lens, **I32)
    qd = qkv.to(DEV)
    got = K.attn_decode_beam(qd[:, :D], slots.to(DEV), H, scale, new_kv=(qd[:, D:2 * D], qd[:, 2 * D:]), lens=lens_t, anc=anc.to(DEV), q_prescaled=prescaled)
    close_per_head(got, ref, PER_HEAD_TOL, f"self form, all rows long, H={H} prescaled={prescaled}")
    want = K.attn_decode(qd[:, :D], gathered.to(DEV), H, scale, new_kv=(qd[:, D:2 * D], qd[:, 2 * D:]), lens=lens_t, q_prescaled=prescaled)
    assert torch.equal(bits(got), bits(want))


def test_self_form_over_a_split_cache():
    """Capacity > 512 keys at a small R * H: the split path with indirection, still bit-identical."""
    H, D, cap = 2, 128, 1100
    lens = [1, 33, 600, 1100]
    R = len(lens)
    g = torch.Generator().manual_seed(12)
    slots = torch.randn(R, cap, 2 * D, generator=g).to(BF)
    qkv = torch.randn(R, 3 * D, generator=g).to(BF).to(DEV)
    anc = _scrambled_anc(R, cap, lens, g)
    gd = slots[anc.long(), torch.arange(cap)[None, :]].to(DEV)
    lens_t = torch.tensor(lens, **I32)
    want = K.attn_decode(qkv[:, :D], gd, H, 0.125, new_kv=(qkv[:, D:2 * D], qkv[:, 2 * D:]), lens=lens_t)
    args, _ = K.attn_decode_beam(qkv[:, :D], slots.to(DEV), H, 0.125, new_kv=(qkv[:, D:2 * D], qkv[:, 2 * D:]), lens=lens_t, anc=anc.to(DEV), _args_only=True)
    assert args.workspace_bytes > 0
    got = K.attn_decode_beam(qkv[:, :D], slots.to(DEV), H, 0.125, new_kv=(qkv[:, D:2 * D], qkv[:, 2 * D:]), lens=lens_t, anc=anc.to(DEV))
    assert torch.equal(bits(got), bits(want))
    # the rows of 600 and 1100 keys, each head against its own scale
    full = gd.cpu().clone()
    for r, n in enumerate(lens):
        full[r, n - 1] = qkv[r, D:].cpu()
    ref = _ref_decode(qkv[:, :D].cpu(), full[..., :D], full[..., D:], lens, H, 0.125, dtype=torch.float64)
    close_per_head(got[2:], ref[2:], PER_HEAD_TOL, "self form over 3 splits, rows of 600 and 1100 keys")


# ----------------------------------------------------------------------------- wft_attn_decode_beam_bf16, cross form
def _nsplit(rows, H, Tk):
    """The split rule include/wft.h states: clamp(ceil(256 / (rows * H)), 1, min(ceil(Tk / 512), 16))."""
    return max(1, min(-(-256 // (rows * H)), -(-Tk // 512), 16))


@pytest.mark.parametrize("A,H,group", [(1, 20, 1), (32, 20, 1), (1, 20, 5), (3, 6, 5), (4, 20, 5), (6, 20, 5), (1, 6, 8), (8, 20, 8), (2, 6, 3)])
def test_cross_form_shares_the_keys_of_an_audio(A, H, group):
    """1 500 keys.  Where the grouped split (per audio) equals the one wft_attn_decode_bf16 takes at R = A * group rows the outputs
    are bit-identical to it on the group-times replicated cache; everywhere the fp32-math bound of test_cross_attention_decode_1500_keys
    holds; reruns are bit-identical and the cache is only read."""
    D, Tk, R = H * 64, 1500, A * group
    g = torch.Generator().manual_seed(A * 7 + H + group)
    kv = torch.randn(A, Tk, 2 * D, generator=g).to(BF)
    q = torch.randn(R, D, generator=g).to(BF)
    rep = kv.repeat_interleave(group, 0)
    ref = _ref_decode(q, rep[..., :D], rep[..., D:], [Tk] * R, H, 0.125)
    kvd, qd = kv.to(DEV), q.to(DEV)
    o1 = K.attn_decode_beam(qd, kvd, H, 0.125, group=group)
    o2 = K.attn_decode_beam(qd, kvd, H, 0.125, group=group)
    close(o1, ref, 2e-2, f"grouped cross A={A} H={H} group={group}")
    assert torch.equal(bits(o1), bits(o2)), "two runs differ"
    assert torch.equal(bits(kvd), bits(kv)), "the cross form must not write the cache"
    same = _nsplit(A, H, Tk) == _nsplit(R, H, Tk)
    args, _ = K.attn_decode_beam(qd, kvd, H, 0.125, group=group, _args_only=True)
    ns = _nsplit(A, H, Tk)
    assert L.load().wft_attn_decode_beam_workspace_bytes(args) == (0 if ns == 1 else R * H * ns * 66 * 4)
    old = K.attn_decode(qd, rep.to(DEV), H, 0.125)
    print(f"A={A} H={H} group={group}: split {_nsplit(A, H, Tk)} vs {_nsplit(R, H, Tk)} of the existing kernel at {R} rows; "
          f"{(bits(o1) != bits(old)).sum().item()} of {o1.numel()} outputs differ in bits")
    if same:
        assert torch.equal(bits(o1), bits(old))
    else:
        close(o1, old, 2e-2, "grouped vs existing kernel at another split")


def test_cross_form_strided_q_and_prescale():
    """q read in place from a wider row, prescaled: the self-attention q of a fused projection is never used here, but the field is."""
    A, H, group, Tk = 2, 6, 5, 700
    D, R = H * 64, 10
    g = torch.Generator().manual_seed(5)
    kv = torch.randn(A, Tk, 2 * D, generator=g).to(BF).to(DEV)
    wide = torch.randn(R, 3 * D, generator=g).to(BF).to(DEV)
    o = K.attn_decode_beam(wide[:, D:2 * D], kv, H, 0.125, group=group, q_prescaled=True)
    old = K.attn_decode(wide[:, D:2 * D], kv.repeat_interleave(group, 0), H, 0.125, q_prescaled=True)
    assert _nsplit(A, H, Tk) == _nsplit(R, H, Tk) == 2 and torch.equal(bits(o), bits(old))


def test_beam_kernel_argument_checks():
    H, D = 2, 128
    q = torch.zeros(6, D, dtype=BF, device=DEV)
    kv = torch.zeros(2, 16, 2 * D, dtype=BF, device=DEV)
    with pytest.raises(ValueError):
        K.attn_decode_beam(q, kv, H, 0.125, group=4)  # 6 rows are not groups of 4
    with pytest.raises(ValueError):
        K.attn_decode_beam(q, kv, H, 0.125, group=9)
    with pytest.raises(ValueError):
        K.attn_decode_beam(q, kv, H, 0.125, group=3, lens=torch.ones(6, **I32))  # the self form needs new_kv and anc too
    a, _ = K.attn_decode_beam(q, kv, H, 0.125, group=3, _args_only=True)
    a.group = 4
    assert L.load().wft_attn_decode_beam_bf16(a, L.stream_ptr()) != 0 and "group" in L.last_error()
    a, _ = K.attn_decode_beam(q, kv, H, 0.125, group=3, _args_only=True)
    a.cache_bs = 15 * 2 * D
    assert L.load().wft_attn_decode_beam_bf16(a, L.stream_ptr()) != 0 and "capacity" in L.last_error()
    slots = torch.zeros(6, 16, 2 * D, dtype=BF, device=DEV)
    anc = torch.zeros(6, 16, **I32)
    a, _ = K.attn_decode_beam(q, slots, H, 0.125, new_kv=(q, q), lens=torch.ones(6, **I32), anc=anc, _args_only=True)
    a.ld_anc = 8
    assert L.load().wft_attn_decode_beam_bf16(a, L.stream_ptr()) != 0 and "ancestry" in L.last_error()
    # top-k: k out of range; update: beam size / max_len
    logits = torch.zeros(1, 128, dtype=BF, device=DEV)
    out_t, out_l = torch.zeros(1, 10, **I32), torch.zeros(1, 10, dtype=torch.float32, device=DEV)
    with pytest.raises(L.WftError, match="2..9"):
        K.decode_topk(logits, 100, out_t, out_l)
    dv = _DevState([[1, 2]], 2, 2, 0, 8, 8)
    with pytest.raises(ValueError):
        K.beam_update(torch.zeros(2, 3, **I32), torch.zeros(2, 3, device=DEV), dv.tokens, dv.anc, dv.len, dv.slp, dv.done, dv.unfinished,
                      dv.fin_tokens, dv.fin_len, dv.fin_score, dv.fin_n, eot=0, max_len=9)  # max_len beyond the token buffer
    with pytest.raises(ValueError):
        K.beam_update(torch.zeros(3, 3, **I32), torch.zeros(3, 3, device=DEV), dv.tokens, dv.anc, dv.len, dv.slp, dv.done, dv.unfinished,
                      dv.fin_tokens, dv.fin_len, dv.fin_score, dv.fin_n, eot=0, max_len=8)  # 3 rows are not 1 audio x 2 beams
