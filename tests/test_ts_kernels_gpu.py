"""GPU checks of the timestamp-rule forms of the greedy pick and the top-(W + 1) kernel (csrc/decode_pick.hip, csrc/decode_beam.hip: wft_decode_pick_ts,
wft_decode_topk_ts) through the C ABI, against the fp64 rule oracle (tests/_ts_oracle.py) on the same bf16 logits: picks and
candidate columns exact, log-probabilities within the 1e-4 absolute of test_pick_matches_masked_argmax_and_log_softmax /
test_topk_on_crafted_rows (the same arithmetic: an fp32 sum of V exponentials in another order)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _ts_oracle as TO  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
I32 = dict(dtype=torch.int32, device=DEV)
CASES = [(51865, 50364), (51866, 50365)]  # (V, ts_begin)
EOT = 50257
N_CTX = 448
F = 3          # prompt length of every row
LP_TOL = 1e-4  # tests/test_decode_kernels_gpu.py, tests/test_beam_kernels_gpu.py
NEG = float("-inf")


def _tokens(histories, V, tsb, row_step=1):
    """tokens i64 [R, N_CTX], first_len, len for state rows r = i * row_step.  The prompt holds timestamp ids and everything behind
    a row's end is a timestamp too: only the SAMPLED tokens tokens[r, F:len) may count."""
    R = len(histories) * row_step
    tokens = torch.full((R, N_CTX), V - 1, dtype=torch.int64)
    tokens[:, :F] = torch.tensor([tsb + 7, 11, V - 1])
    lens = torch.full((R,), F, dtype=torch.int32)
    for i, h in enumerate(histories):
        r = i * row_step
        tokens[r, F:F + len(h)] = torch.tensor(h, dtype=torch.int64)
        lens[r] = F + len(h)
    return tokens, torch.full((R,), F, dtype=torch.int32), lens


def _run_pick(logits, V, tsb, histories, sup, sup_first, no_ts, max_initial):
    tokens, first_len, lens = _tokens(histories, V, tsb)
    B = len(histories)
    st = dict(tokens=tokens.to(DEV), lens=lens.to(DEV), finished=torch.zeros(B, **I32), slp=torch.zeros(B, dtype=torch.float32, device=DEV),
              unf=torch.zeros(1, **I32))
    pick, lp = K.decode_pick(logits.to(DEV), V, st["tokens"], st["lens"], st["finished"], st["slp"], st["unf"], eot=EOT, max_len=N_CTX,
                             suppress=None if sup is None else sup.to(DEV), suppress_first=None if sup_first is None else sup_first.to(DEV),
                             first_len=first_len.to(DEV), want_pick=True, ts_rules=(tsb, no_ts, max_initial))
    return pick.cpu(), lp.cpu(), st


def _run_topk(logits, V, tsb, k, histories, sup, sup_first, no_ts, max_initial, row_step=1):
    tokens, first_len, lens = _tokens(histories, V, tsb, row_step)
    R = tokens.shape[0]
    tok = torch.full((R, k), -5, **I32)
    lp = torch.full((R, k), 7.0, dtype=torch.float32, device=DEV)
    K.decode_topk(logits.to(DEV), V, tok, lp, lens=lens.to(DEV), first_len=first_len.to(DEV), suppress=None if sup is None else sup.to(DEV),
                  suppress_first=None if sup_first is None else sup_first.to(DEV), row_step=row_step, ts_rules=(tsb, no_ts, max_initial),
                  tokens=tokens.to(DEV), eot=EOT)
    return tok.cpu(), lp.cpu()


def _dead(h, sup, sup_first):
    dead = [] if sup is None else sup.nonzero().flatten().tolist()
    if sup_first is not None and not h:
        dead += sup_first.nonzero().flatten().tolist()
    return dead


def _ruled(logits, V, tsb, histories, sup, sup_first, no_ts, max_initial):
    return [TO.rules(logits[b, :V].float(), h, ts_begin=tsb, eot=EOT, no_timestamps=no_ts, max_initial=max_initial, dead=_dead(h, sup, sup_first))
            for b, h in enumerate(histories)]


def _want_pick(r):
    if not torch.isfinite(r.x).any():
        return EOT, 0.0
    col = int((r.x == r.x.max()).nonzero()[0])
    return col, r.logp[col].item()


def _cmp_topk(tok, lp, ruled, k, rows, what):
    worst = 0.0
    for i, r in zip(rows, ruled):
        want = TO.topk_of(r, k)
        assert tok[i].tolist() == [c for c, _ in want], (what, i, tok[i].tolist(), want)
        for j, (c, w) in enumerate(want):
            if c < 0:
                assert lp[i, j].item() == NEG
            else:
                worst = max(worst, abs(lp[i, j].item() - w))
    print(f"{what}: top-{k} log-probabilities max |err| vs the fp64 oracle {worst:.3e} (tol {LP_TOL})")
    assert worst < LP_TOL


# ----------------------------------------------------------------------------- crafted rows: one per branch of the rules
def _crafted(V, tsb):
    """-> (logits bf16 [B, ld], histories, sup, sup_first, names).  t(i) = the i-th timestamp."""
    t = lambda i: tsb + i
    g = torch.Generator().manual_seed(V)
    text = lambda n: torch.randint(0, EOT, (n,), generator=g).tolist()
    H = {
        "first token": [],
        "single timestamp": [t(5)],
        "text then ts": [t(5), 100, t(9)],
        "ts then ts": [t(5), 100, t(9), t(9)],
        "text then text, earlier ts": [t(5), 100, 200],
        "last ts = V-1": [t(5), 100, V - 1],
        "no ts left": [t(5), 100, V - 1, 200],
        "margin +0.5": [t(5), 100, V - 2, 200],
        "margin -0.5": [t(5), 100, V - 2, 200],
        "tie, one live ts": [t(5), 100, V - 2, 200],
        "tie, ts mass wins": [t(5), 100, 200],
        "masks over rule ranges": [t(5), 100, t(9)],
        "long history": [t(1)] + text(200) + [t(30), t(30)] + text(150) + [t(40), t(40)] + text(88),  # 443 sampled tokens: len 446 of 448
        "300 tokens, early ts": [t(2)] + text(299),
    }
    names = list(H)
    B, ld = len(names), K.round_up(V, 128)
    x = (torch.randn(B, ld, generator=g) * 2).to(BF)
    x[:, V:] = 1000.0  # padded columns must never appear
    row = {n: i for i, n in enumerate(names)}
    x[row["first token"], t(60)] = 20.0           # beyond max_initial = 50: wins only without the bound
    x[row["first token"], 300] = 25.0             # text: never a first token
    x[row["first token"], t(2)] = 22.0            # under suppress_first
    x[row["text then ts"], 300] = 30.0            # text below eot: removed behind a closing timestamp
    x[row["text then text, earlier ts"], t(3)] = 25.0  # below the last timestamp
    x[row["text then text, earlier ts"], t(5)] = 24.0  # the last timestamp itself
    for n, v in (("margin +0.5", 12.5), ("margin -0.5", 11.5), ("tie, one live ts", 12.0)):
        x[row[n], 300] = 12.0                     # the text maximum (2 * randn stays below 12)
        x[row[n], V - 1] = v                      # the only live timestamp: its logsumexp is its own value, exact in bf16
    x[row["tie, ts mass wins"], 300] = 12.0
    x[row["tie, ts mass wins"], t(20)] = 12.0
    x[row["long history"], t(35)] = 30.0            # removed: below the last timestamp t(40)
    x[row["long history"], t(45)] = 15.0
    x[row["300 tokens, early ts"], t(1)] = 30.0   # removed
    x[row["300 tokens, early ts"], t(3)] = 15.0
    sup = torch.zeros(V, dtype=torch.uint8)
    sup[torch.randint(0, tsb, (500,), generator=g)] = 1
    sup[[100, 200, 300]] = 0
    r = row["masks over rule ranges"]
    sup[t(9):t(13)] = 1                           # the head of the live timestamp range
    sup[tsb - 1] = 1                              # the no_timestamps column, removed twice
    sup[int(x[r, t(13):V].float().argmax()) + t(13)] = 1   # that row's best live timestamp
    sup[EOT + 3] = 1                              # a live special between eot and ts_begin
    sup_first = torch.zeros(V, dtype=torch.uint8)
    sup_first[t(1):t(4)] = 1
    sup_first[[EOT, 220]] = 1
    return x, [H[n] for n in names], sup, sup_first, row


@pytest.mark.parametrize("V,tsb", CASES)
@pytest.mark.parametrize("max_initial", [50, None, 0])
def test_pick_on_crafted_rows(V, tsb, max_initial):
    x, hist, sup, sup_first, row = _crafted(V, tsb)
    no_ts = tsb - 1
    pick, lp, st = _run_pick(x, V, tsb, hist, sup, sup_first, no_ts, max_initial)
    ruled = _ruled(x, V, tsb, hist, sup, sup_first, no_ts, max_initial)
    want = [_want_pick(r) for r in ruled]
    assert pick.tolist() == [c for c, _ in want], [(n, int(pick[i]), want[i][0]) for n, i in row.items() if int(pick[i]) != want[i][0]]
    err = max(abs(lp[i].item() - w) for i, (_, w) in enumerate(want))
    print(f"V={V} max_initial={max_initial}: pick log-probability max |err| vs the fp64 oracle {err:.3e} (tol {LP_TOL})")
    assert err < LP_TOL
    # what the rows were planted for (the oracle and the test agree on the intent)
    t = lambda i: tsb + i
    assert (int(pick[row["first token"]]) == t(60)) == (max_initial is None)
    assert tsb <= int(pick[row["first token"]]) <= (V - 1 if max_initial is None else t(max_initial))
    assert int(pick[row["first token"]]) != t(2)
    if max_initial == 0:  # t(0) is the one column left
        assert int(pick[row["first token"]]) == t(0) and lp[row["first token"]].item() == 0.0
    assert int(pick[row["single timestamp"]]) < tsb and int(pick[row["ts then ts"]]) < tsb and int(pick[row["no ts left"]]) < tsb
    assert int(pick[row["text then ts"]]) != 300 and int(pick[row["text then ts"]]) >= EOT
    assert int(pick[row["text then text, earlier ts"]]) not in (t(3), t(5))
    assert int(pick[row["margin +0.5"]]) == V - 1 and lp[row["margin +0.5"]].item() == 0.0 and ruled[row["margin +0.5"]].margin == 0.5
    assert int(pick[row["margin -0.5"]]) == 300 and ruled[row["margin -0.5"]].margin == -0.5
    assert int(pick[row["tie, one live ts"]]) == 300 and ruled[row["tie, one live ts"]].margin == 0.0
    assert int(pick[row["tie, ts mass wins"]]) == t(20) and ruled[row["tie, ts mass wins"]].ts_wins
    assert int(pick[row["long history"]]) == t(45) and int(pick[row["300 tokens, early ts"]]) == t(3)
    # the state advanced exactly as wft_decode_pick advances it
    tok, lens = st["tokens"].cpu(), st["lens"].cpu()
    for i, h in enumerate(hist):
        assert int(lens[i]) == F + len(h) + 1 and int(tok[i, F + len(h)]) == int(pick[i])
        assert int(st["finished"][i]) == int(int(pick[i]) == EOT)
    assert torch.equal(st["slp"].cpu(), lp) and int(st["unf"]) == len(hist) - int(st["finished"].sum())


@pytest.mark.parametrize("V,tsb", CASES)
@pytest.mark.parametrize("k", [2, 6, 9])
def test_topk_on_crafted_rows(V, tsb, k):
    x, hist, sup, sup_first, row = _crafted(V, tsb)
    no_ts = tsb - 1
    for max_initial in (50, 0):
        tok, lp = _run_topk(x, V, tsb, k, hist, sup, sup_first, no_ts, max_initial)
        ruled = _ruled(x, V, tsb, hist, sup, sup_first, no_ts, max_initial)
        _cmp_topk(tok, lp, ruled, k, range(len(hist)), f"V={V} max_initial={max_initial}")
        assert (lp[:, :-1] >= lp[:, 1:]).all()
    # max_initial = 0 leaves ONE live column at the first step
    assert tok[row["first token"]].tolist() == [tsb] + [-1] * (k - 1) and lp[row["first token"], 0].item() == 0.0
    assert tok[row["margin +0.5"]].tolist() == [V - 1] + [-1] * (k - 1)   # the timestamps won: the one live timestamp is all there is
    assert tok[row["tie, one live ts"], :2].tolist() == [300, V - 1]      # the tie: text stays, the lower column first


@pytest.mark.parametrize("V,tsb", CASES[:1])
def test_topk_row_step(V, tsb):
    """row_step = W: logits row i belongs to state row i * W (its tokens, len and first_len) and fills that candidate row only."""
    W = 5
    x, hist, sup, sup_first, row = _crafted(V, tsb)
    keep = [row[n] for n in ("first token", "text then ts", "long history", "margin +0.5")]
    x, hist = x[keep].contiguous(), [hist[i] for i in keep]
    tok, lp = _run_topk(x, V, tsb, W + 1, hist, sup, sup_first, tsb - 1, 50, row_step=W)
    ruled = _ruled(x, V, tsb, hist, sup, sup_first, tsb - 1, 50)
    _cmp_topk(tok, lp, ruled, W + 1, [i * W for i in range(len(hist))], "row_step = W")
    others = [r for r in range(len(hist) * W) if r % W]
    assert (tok[others] == -5).all() and (lp[others] == 7.0).all()


@pytest.mark.parametrize("V,tsb", CASES)
def test_every_column_removed(V, tsb):
    """Today's behaviour: the pick is eot with log-probability 0, the candidates are (-1, -inf)."""
    ld = K.round_up(V, 128)
    x = torch.randn(3, ld, generator=torch.Generator().manual_seed(1)).to(BF)
    sup = torch.zeros(V, dtype=torch.uint8); sup[:tsb] = 1
    hist = [[tsb + 5], [tsb + 5, 100, tsb + 9, tsb + 9], [tsb + 5, 100, V - 1, 200]]  # no timestamp is live, all text is suppressed
    pick, lp, st = _run_pick(x, V, tsb, hist, sup, None, None, 50)
    assert pick.tolist() == [EOT] * 3 and lp.tolist() == [0.0] * 3 and st["finished"].cpu().tolist() == [1, 1, 1]
    tok, tlp = _run_topk(x, V, tsb, 6, hist, sup, None, None, 50)
    assert (tok == -1).all() and (tlp == NEG).all()


# ----------------------------------------------------------------------------- random rows
KINDS = ("first", "ts", "text-ts", "ts-ts", "text-text", "first-ts-only")


@functools.lru_cache(maxsize=None)
def _random_case(V, tsb):
    """256 rows, seed 0, randn * 2, a per-row offset U[-4, 2) on the timestamp columns, bf16; sampled histories of every kind.  The
    logits, the histories and the ruled fp64 reference, computed once and shared by the tests below (nothing writes to them)."""
    B, ld = 256, K.round_up(V, 128)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, ld, generator=g) * 2
    x[:, tsb:V] += torch.rand(B, 1, generator=g) * 6 - 4
    x = x.to(BF)
    x[:, V:] = 1000.0
    hist = []
    for b in range(B):
        kind = KINDS[b % len(KINDS)]
        ts = sorted((tsb + torch.randint(0, 1400, (2,), generator=g)).tolist())
        n, m = int(torch.randint(1, 200, (1,), generator=g)), int(torch.randint(1, 200, (1,), generator=g))
        text = lambda c: torch.randint(0, EOT, (c,), generator=g).tolist()
        hist.append({"first": [], "ts": [ts[0]], "text-ts": [ts[0]] + text(n) + [ts[1]], "ts-ts": [ts[0]] + text(n) + [ts[1], ts[1]],
                     "text-text": [ts[0]] + text(n) + [ts[1], ts[1]] + text(m), "first-ts-only": [ts[0]] + text(n)}[kind])
    sup = torch.zeros(V, dtype=torch.uint8)
    sup[torch.randint(0, tsb, (800,), generator=g)] = 1
    sup[EOT + 1:tsb] = 1  # the specials, as a caller would
    ruled = _ruled(x, V, tsb, hist, sup, None, tsb - 1, 50)
    return x, hist, sup, ruled


def _contested(ruled):
    return [r for r in ruled if r.margin == r.margin and abs(r.margin) != float("inf")]


@pytest.mark.parametrize("V,tsb", CASES)
def test_pick_on_random_rows(V, tsb):
    x, hist, sup, ruled = _random_case(V, tsb)
    pick, lp, _ = _run_pick(x, V, tsb, hist, sup, None, tsb - 1, 50)
    both = _contested(ruled)
    wins = sum(r.ts_wins for r in both)
    skipped = [b for b, r in enumerate(ruled) if r.margin == r.margin and abs(r.margin) < 1e-2]
    print(f"V={V}: rule 5 contested on {len(both)} of {len(ruled)} rows, the timestamps win {wins} ({wins / len(both):.1%}); "
          f"{len(skipped)} rows within 1e-2 of the rule's threshold are left out of the exact comparison (cap {int(0.02 * len(ruled))})")
    assert wins >= len(both) // 5 and len(both) - wins >= len(both) // 5  # both sides of the rule are exercised
    assert len(skipped) <= 0.02 * len(ruled)
    worst = 0.0
    for b, r in enumerate(ruled):
        if b in skipped:
            continue
        col, w = _want_pick(r)
        assert int(pick[b]) == col, (b, KINDS[b % len(KINDS)], int(pick[b]), col, r.margin)
        worst = max(worst, abs(lp[b].item() - w))
    print(f"V={V}: pick log-probability max |err| vs the fp64 oracle {worst:.3e} (tol {LP_TOL})")
    assert worst < LP_TOL
    # reruns are bit-identical
    pick2, lp2, _ = _run_pick(x, V, tsb, hist, sup, None, tsb - 1, 50)
    assert torch.equal(pick, pick2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32))


@pytest.mark.parametrize("V,tsb", CASES)
@pytest.mark.parametrize("k", [2, 6, 9])
def test_topk_on_random_rows(V, tsb, k):
    x, hist, sup, ruled = _random_case(V, tsb)
    tok, lp = _run_topk(x, V, tsb, k, hist, sup, None, tsb - 1, 50)
    rows = [b for b, r in enumerate(ruled) if not (r.margin == r.margin and abs(r.margin) < 1e-2)]
    assert len(ruled) - len(rows) <= 0.02 * len(ruled)
    _cmp_topk(tok, lp, [ruled[b] for b in rows], k, rows, f"V={V} random rows")
    tok2, lp2 = _run_topk(x, V, tsb, k, hist, sup, None, tsb - 1, 50)
    assert torch.equal(tok, tok2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32))


# ----------------------------------------------------------------------------- no rule fires: the plain kernels, bit for bit
@pytest.mark.parametrize("V,tsb", CASES)
def test_no_rule_fires_equals_the_plain_kernels_bit_for_bit(V, tsb):
    """All-text, non-empty histories, no_timestamps = -1 and every timestamp column statically suppressed: rules 1-4 remove nothing
    that is live and rule 5 has an empty timestamp side, so the live set, the scan order and the reduction order are the plain
    kernels' — and so must every bit be."""
    B, ld = 16, K.round_up(V, 128)
    g = torch.Generator().manual_seed(V + 1)
    x = (torch.randn(B, ld, generator=g) * 3).to(BF)
    x[:, V:] = 1000.0
    x[3, 40000] = x[3, 123] = 50.0  # a tie
    x[5, :] = -30.0; x[5, 77] = 4.0  # one dominant column: log-probability -0.0 / ~0
    sup = torch.zeros(V, dtype=torch.uint8)
    sup[torch.randint(0, tsb, (500,), generator=g)] = 1
    sup[[123, 40000, 77]] = 0
    sup[tsb:] = 1
    hist = [torch.randint(0, EOT, (1 + 29 * b,), generator=g).tolist() for b in range(B)]
    pick, lp, st = _run_pick(x, V, tsb, hist, sup, None, None, 50)
    tokens, first_len, lens = _tokens(hist, V, tsb)
    st0 = dict(tokens=tokens.to(DEV), lens=lens.to(DEV), finished=torch.zeros(B, **I32), slp=torch.zeros(B, dtype=torch.float32, device=DEV),
               unf=torch.zeros(1, **I32))
    pick0, lp0 = K.decode_pick(x.to(DEV), V, st0["tokens"], st0["lens"], st0["finished"], st0["slp"], st0["unf"], eot=EOT, max_len=N_CTX,
                               suppress=sup.to(DEV), first_len=first_len.to(DEV), want_pick=True)
    assert torch.equal(pick, pick0.cpu()) and torch.equal(lp.view(torch.int32), lp0.cpu().view(torch.int32))
    for key in st0:
        assert torch.equal(st[key], st0[key]), key
    assert int(pick[3]) == 123
    for k in (2, 6, 9):
        tok, tlp = _run_topk(x, V, tsb, k, hist, sup, None, None, 50)
        tok0 = torch.full((B, k), -5, **I32)
        tlp0 = torch.full((B, k), 7.0, dtype=torch.float32, device=DEV)
        K.decode_topk(x.to(DEV), V, tok0, tlp0, lens=lens.to(DEV), first_len=first_len.to(DEV), suppress=sup.to(DEV))
        assert torch.equal(tok, tok0.cpu()) and torch.equal(tlp.view(torch.int32), tlp0.cpu().view(torch.int32)), k


# ----------------------------------------------------------------------------- argument checks
def test_argument_checks_return_the_error_status_without_launching():
    V, tsb = 1000, 900
    eot = 800
    x = torch.zeros(2, 1024, dtype=BF, device=DEV)
    tokens = torch.full((2, 16), -7, dtype=torch.int64, device=DEV)
    lens, first_len = torch.full((2,), 3, **I32), torch.full((2,), 3, **I32)
    fin, unf = torch.zeros(2, **I32), torch.full((1,), -1, **I32)
    slp = torch.zeros(2, dtype=torch.float32, device=DEV)
    tok, lp = torch.full((2, 4), -5, **I32), torch.full((2, 4), 7.0, dtype=torch.float32, device=DEV)

    def pick(rules, **kw):
        args = dict(eot=eot, max_len=16, first_len=first_len, ts_rules=rules)
        args.update(kw)
        K.decode_pick(x, V, tokens, lens, fin, slp, unf, **args)

    def topk(rules, **kw):
        args = dict(lens=lens, first_len=first_len, ts_rules=rules, tokens=tokens, eot=eot)
        args.update(kw)
        K.decode_topk(x, V, tok, lp, **args)

    for call in (pick, topk):
        for rules in ((eot, None, 50), (V, None, 50), (5, None, 50)):      # eot < ts_begin < V
            with pytest.raises(L.WftError, match="ts_begin"):
                call(rules)
        for rules in ((tsb, V, 50), (tsb, -2, 50)):                        # no_timestamps: -1 or a column
            with pytest.raises(L.WftError, match="no_timestamps"):
                call(rules)
        with pytest.raises(L.WftError, match="first_len"):
            call((tsb, None, 50), first_len=None)
    with pytest.raises(L.WftError, match="first_len"):
        topk((tsb, None, 50), lens=None)
    with pytest.raises(ValueError, match="tokens"):
        topk((tsb, None, 50), tokens=None)
    with pytest.raises(ValueError, match="tokens"):
        topk((tsb, None, 50), tokens=tokens[:1])
    a = L.DecodeTopkArgs()
    a.logits, a.ld, a.V, a.len, a.first_len = x.data_ptr(), 1024, V, lens.data_ptr(), first_len.data_ptr()
    a.cand_tok, a.cand_logp, a.rows, a.row_step, a.k = tok.data_ptr(), lp.data_ptr(), 2, 1, 4
    ru = L.TsRules(tsb, -1, 50)
    import ctypes as C
    assert L.load().wft_decode_topk_ts(C.byref(a), C.byref(ru), None, 16, eot, L.stream_ptr()) != 0 and "token rows" in L.last_error()
    assert L.load().wft_decode_topk_ts(C.byref(a), None, tokens.data_ptr(), 16, eot, L.stream_ptr()) != 0
    assert L.load().wft_decode_topk_ts(C.byref(a), C.byref(ru), tokens.data_ptr(), 16, V, L.stream_ptr()) != 0 and "eot" in L.last_error()
    torch.cuda.synchronize()
    # nothing was launched: no state moved
    assert (tokens == -7).all() and lens.tolist() == [3, 3] and int(unf) == -1 and (tok == -5).all() and (lp == 7.0).all()
    # and the same arguments with sound rules go through
    topk((tsb, None, 50)); pick((tsb, None, 50))
    assert lens.tolist() == [4, 4] and (tok[:, 0] >= tsb).all()
