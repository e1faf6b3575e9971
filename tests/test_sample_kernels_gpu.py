"""GPU checks of the sampled pick (csrc/decode_pick.hip: wft_decode_sample, wft_decode_sample_ts) through the C ABI, against the fp64
oracle (tests/_sample_oracle.py: numpy Philox, Gumbel noise, the rules of tests/_ts_oracle.py) on the same bf16 logits.

Exactness.  The kernel's key x / t + g is fp32, the oracle's fp64; on the random rows below the two differ by at most 2.4e-6
(measured on the CPU), so the pick must equal the oracle's on every row whose two largest fp64 keys lie >= GAP = 1e-3 apart — over
400 times the fp32 key error — and at most 2 % of the rows may fall under that gap and be left out.  Log-probabilities: the
project's LP_TOL = 1e-4 absolute against fp64 (an fp32 sum of V exponentials in another order)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _sample_oracle as SO  # noqa: E402
from tests.test_ts_kernels_gpu import _random_case, _tokens  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
CASES = [(51865, 50364), (51866, 50365)]  # (V, ts_begin)
EOT = 50257
N_CTX = 448
F = 3           # prompt length of every row
LP_TOL = 1e-4   # tests/test_decode_kernels_gpu.py, tests/test_ts_kernels_gpu.py
GAP = 1e-3      # see the module docstring
CAP = 0.02


def _state(R, lens, n_ctx=N_CTX, tokens=None, finished=None):
    i32 = dict(dtype=torch.int32, device=DEV)
    return dict(tokens=(torch.full((R, n_ctx), -7, dtype=torch.int64) if tokens is None else tokens.clone()).to(DEV),
                lens=torch.as_tensor(lens, dtype=torch.int32).clone().to(DEV), finished=torch.zeros(R, **i32) if finished is None else
                torch.as_tensor(finished, dtype=torch.int32).to(DEV), slp=torch.zeros(R, dtype=torch.float32, device=DEV), unf=torch.full((1,), -1, **i32))


def _i64(seeds):
    return torch.tensor([s - (1 << 64) if s >= (1 << 63) else s for s in (int(x) % (1 << 64) for x in seeds)], dtype=torch.int64, device=DEV)


def _sample(logits, V, st, temps, seeds, *, group=1, sup=None, sup_first=None, first_len=None, ts=None, eot=EOT, max_len=N_CTX):
    R = st["tokens"].shape[0]
    first_len = torch.full((R,), F, dtype=torch.int32) if first_len is None else torch.as_tensor(first_len, dtype=torch.int32)
    pick, lp = K.decode_sample(logits.to(DEV), V, st["tokens"], st["lens"], st["finished"], st["slp"], st["unf"],
                               torch.as_tensor(temps, dtype=torch.float32).expand(R).contiguous().to(DEV), _i64(seeds), group=group, eot=eot,
                               max_len=max_len, suppress=None if sup is None else sup.to(DEV), suppress_first=None if sup_first is None else sup_first.to(DEV),
                               first_len=first_len.to(DEV), want_pick=True, ts_rules=ts)
    return pick.cpu(), lp.cpu()


def _greedy(logits, V, st, *, sup=None, ts=None, eot=EOT, max_len=N_CTX):
    R = st["tokens"].shape[0]
    pick, lp = K.decode_pick(logits.to(DEV), V, st["tokens"], st["lens"], st["finished"], st["slp"], st["unf"], eot=eot, max_len=max_len,
                             suppress=None if sup is None else sup.to(DEV), first_len=torch.full((R,), F, dtype=torch.int32, device=DEV), want_pick=True,
                             ts_rules=ts)
    return pick.cpu(), lp.cpu()


def _compare(pick, lp, want, what, skip=()):
    """picks exact on every row whose key gap is >= GAP (and that is not in `skip`), at most CAP of the rows under the gap;
    log-probabilities within LP_TOL wherever the pick is compared."""
    under = [b for b, w in enumerate(want) if w.gap < GAP]
    print(f"{what}: {len(under)} of {len(want)} rows have a top-two key gap under {GAP} (cap {int(CAP * len(want))}), {len(skip)} skipped otherwise")
    assert len(under) <= CAP * len(want)
    worst = 0.0
    for b, w in enumerate(want):
        if b in under or b in skip:
            continue
        assert int(pick[b]) == w.col, (what, b, int(pick[b]), w)
        worst = max(worst, abs(lp[b].item() - w.logp))
    print(f"{what}: log-probability max |err| vs the fp64 oracle {worst:.3e} (tol {LP_TOL})")
    assert worst < LP_TOL


# ----------------------------------------------------------------------------- (a) random rows
@functools.lru_cache(maxsize=None)
def _plain_case(V):
    """256 rows randn * 2 (seed 0) in bf16, a suppress mask, the fp64 live rows; computed once, written by nobody."""
    B, ld = 256, K.round_up(V, 128)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, ld, generator=g) * 2).to(BF)
    x[:, V:] = 1000.0  # padded columns must never appear
    sup = torch.zeros(V, dtype=torch.uint8)
    sup[torch.randint(0, V, (800,), generator=g)] = 1
    dead = sup.nonzero().flatten().tolist()
    live = [SO.live_row(x[b, :V].float(), eot=EOT, dead=dead) for b in range(B)]
    return x, sup, live


def _plain_inputs(B):
    return [F + b % 5 for b in range(B)], [1234 + b for b in range(B)]


@pytest.mark.parametrize("V,tsb", CASES)
@pytest.mark.parametrize("temp", [0.2, 1.0])
def test_sample_on_random_rows(V, tsb, temp):
    x, sup, live = _plain_case(V)
    B = x.shape[0]
    lens, seeds = _plain_inputs(B)
    want = [SO.pick(live[b], temp, seeds[b], lens[b], EOT) for b in range(B)]
    st = _state(B, lens)
    pick, lp = _sample(x, V, st, temp, seeds, sup=sup)
    _compare(pick, lp, want, f"V={V} T={temp}")
    assert (sup[pick] == 0).all() and (pick < V).all()
    assert len({int(p) for p in pick}) > B // 2  # (a sampler, not an arg-max: at T >= 0.2 the rows scatter)
    # the state advanced as wft_decode_pick advances it
    tok, ln = st["tokens"].cpu(), st["lens"].cpu()
    for b in range(B):
        assert int(ln[b]) == lens[b] + 1 and int(tok[b, lens[b]]) == int(pick[b]) and int(tok[b, lens[b] + 1]) == -7
    assert torch.equal(st["slp"].cpu(), lp) and int(st["unf"]) == B - int(st["finished"].sum())
    # reruns are bit-identical
    pick2, lp2 = _sample(x, V, _state(B, lens), temp, seeds, sup=sup)
    assert torch.equal(pick, pick2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32))


# ----------------------------------------------------------------------------- (b) under the timestamp rules
@pytest.mark.parametrize("V,tsb", CASES)
@pytest.mark.parametrize("temp", [0.2, 1.0])
def test_sample_under_the_timestamp_rules(V, tsb, temp):
    x, hist, sup, ruled = _random_case(V, tsb)
    B = len(hist)
    tokens, first_len, lens = _tokens(hist, V, tsb)
    seeds = [1234 + b for b in range(B)]
    want = [SO.pick(ruled[b].x.numpy(), temp, seeds[b], int(lens[b]), EOT) for b in range(B)]
    near = [b for b, r in enumerate(ruled) if r.margin == r.margin and abs(r.margin) < 1e-2]  # rule 5 within 1e-2 of its threshold
    assert len(near) <= CAP * B
    st = _state(B, lens, tokens=tokens)
    pick, lp = _sample(x, V, st, temp, seeds, sup=sup, first_len=first_len, ts=(tsb, tsb - 1, 50))
    _compare(pick, lp, want, f"V={V} T={temp} timestamp rules", skip=near)
    won = [b for b, r in enumerate(ruled) if r.ts_wins and b not in near]
    assert won and all(int(pick[b]) >= tsb for b in won)  # rule 5 was decided on the untempered row: no text where the timestamps won
    pick2, lp2 = _sample(x, V, _state(B, lens, tokens=tokens), temp, seeds, sup=sup, first_len=first_len, ts=(tsb, tsb - 1, 50))
    assert torch.equal(pick, pick2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32))


# ----------------------------------------------------------------------------- (c) temperature <= 0: the greedy kernels, bit for bit
@pytest.mark.parametrize("V,tsb", CASES)
def test_zero_temperature_equals_the_greedy_kernels_bit_for_bit(V, tsb):
    x, sup, _ = _plain_case(V)
    B = x.shape[0]
    lens, seeds = _plain_inputs(B)
    temps = torch.tensor([0.0, -1.0, -0.0, float("-inf")]).repeat(B // 4)
    st, st0 = _state(B, lens), _state(B, lens)
    pick, lp = _sample(x, V, st, temps, seeds, sup=sup)
    pick0, lp0 = _greedy(x, V, st0, sup=sup)
    assert torch.equal(pick, pick0) and torch.equal(lp.view(torch.int32), lp0.view(torch.int32))
    for key in st0:
        assert torch.equal(st[key], st0[key]), key
    xt, hist, supt, _ = _random_case(V, tsb)
    tokens, first_len, lens = _tokens(hist, V, tsb)
    st, st0 = _state(len(hist), lens, tokens=tokens), _state(len(hist), lens, tokens=tokens)
    pick, lp = _sample(xt, V, st, temps, seeds, sup=supt, first_len=first_len, ts=(tsb, tsb - 1, 50))
    pick0, lp0 = _greedy(xt, V, st0, sup=supt, ts=(tsb, tsb - 1, 50))
    assert torch.equal(pick, pick0) and torch.equal(lp.view(torch.int32), lp0.view(torch.int32))
    for key in st0:
        assert torch.equal(st[key], st0[key]), key


# ----------------------------------------------------------------------------- (d) mixed temperatures in one launch, and group
def test_mixed_temperatures_and_group():
    """A = 4 logits rows feed R = 20 state rows (row r reads logits row r // 5).  Per group: one greedy row, two rows with equal
    temperature and seed (equal picks), two that differ in the seed."""
    V, A, N = 51865, 4, 5
    x, sup, live = _plain_case(V)
    x, live = x[:A].contiguous(), live[:A]
    R = A * N
    temps = [[0.0, 0.5, 0.5, 1.0, 1.0][r % N] for r in range(R)]
    seeds = [[7, 11, 11, 13, 14][r % N] + 100 * (r // N) for r in range(R)]
    want = [SO.pick(live[r // N], temps[r], seeds[r], F, EOT) for r in range(R)]
    assert min(w.gap for w in want) >= GAP  # (a property of the data: every row is compared)
    st = _state(R, [F] * R)
    pick, lp = _sample(x, V, st, torch.tensor(temps), seeds, group=N, sup=sup)
    assert pick.tolist() == [w.col for w in want]
    assert max(abs(lp[r].item() - want[r].logp) for r in range(R)) < LP_TOL
    for a in range(A):
        assert int(pick[a * N + 1]) == int(pick[a * N + 2]) and lp[a * N + 1].item() == lp[a * N + 2].item()
    assert any(int(pick[a * N + 3]) != int(pick[a * N + 4]) for a in range(A))
    # the same rows, one logits row each (group = 1): the noise does not depend on the launch shape
    pick1, lp1 = _sample(x.repeat_interleave(N, 0), V, _state(R, [F] * R), torch.tensor(temps), seeds, sup=sup)
    assert torch.equal(pick, pick1) and torch.equal(lp.view(torch.int32), lp1.view(torch.int32))
    # the greedy row of every group is wft_decode_pick's
    pick_g, lp_g = _greedy(x.repeat_interleave(N, 0), V, _state(R, [F] * R), sup=sup)
    for r in range(0, R, N):
        assert int(pick[r]) == int(pick_g[r]) and lp[r].item() == lp_g[r].item()


# ----------------------------------------------------------------------------- (e) the position is part of the counter
def test_same_logits_and_seed_at_another_position_draw_other_noise():
    V, A = 51866, 8
    x, sup, live = _plain_case(V)
    x, live = x[:A].contiguous(), live[:A]
    lens = [F, F + 1] * A  # the two rows of a group: same logits row, same seed, different len
    seeds = [500 + r // 2 for r in range(2 * A)]
    want = [SO.pick(live[r // 2], 1.0, seeds[r], lens[r], EOT) for r in range(2 * A)]
    assert min(w.gap for w in want) >= GAP and sum(want[2 * a].col != want[2 * a + 1].col for a in range(A)) >= A // 2
    assert not np.array_equal(SO.gumbel(500, F, np.arange(64)), SO.gumbel(500, F + 1, np.arange(64)))
    pick, lp = _sample(x, V, _state(2 * A, lens), 1.0, seeds, group=2, sup=sup)
    assert pick.tolist() == [w.col for w in want]
    assert max(abs(lp[r].item() - want[r].logp) for r in range(2 * A)) < LP_TOL


# ----------------------------------------------------------------------------- (f) the distribution
CHI2_999 = {22: 48.27, 14: 36.12}  # the 99.9 % quantiles of chi-square at the degrees of freedom the two temperatures give


@pytest.mark.parametrize("temp,dof,oracle_stat", [(1.0, 22, 14.33), (0.5, 14, 10.69)])
def test_distribution_of_32768_draws_from_one_row(temp, dof, oracle_stat):
    V, R = 24, 32768
    x = (torch.randn(V, generator=torch.Generator().manual_seed(0)) * 2).to(BF)
    seeds = [99 + r for r in range(R)]
    x64 = x.double().numpy()
    cols, gaps = SO.pick_rows(x64, temp, seeds, F)
    probs = np.exp(x64 / temp - (x64 / temp).max())
    probs /= probs.sum()
    stat, df = SO.chi_square(SO.counts(cols, V), probs)
    assert df == dof and abs(stat - oracle_stat) < 0.01 and stat < CHI2_999[dof]  # the oracle itself samples softmax(x / T)
    st = _state(R, [F] * R, n_ctx=8)
    pick, lp = _sample(x.view(1, V), V, st, temp, seeds, group=R, eot=0, max_len=8)
    differ = np.nonzero(pick.numpy() != cols)[0]
    under = int((gaps < GAP).sum())
    print(f"T={temp}: {len(differ)} of {R} picks differ from the oracle's, {under} rows lie under the key gap {GAP} (cap {int(CAP * R)})")
    assert under <= CAP * R and all(gaps[r] < GAP for r in differ)
    got, _ = SO.chi_square(SO.counts(pick.numpy(), V), probs)
    print(f"T={temp}: chi-square of the GPU counts against softmax(x / T) {got:.2f} at {df} degrees of freedom (oracle {stat:.2f}, bound {CHI2_999[dof]})")
    assert got < CHI2_999[dof]
    logp = torch.log_softmax(x.double(), 0)  # temperature 1, whatever T is
    assert (lp.double() - logp[pick]).abs().max().item() < LP_TOL


# ----------------------------------------------------------------------------- (g) the state update
def test_state_update_frozen_rows_max_len_and_nothing_live():
    V, ld, n_ctx, max_len, eot = 1000, 1024, 16, 10, 800
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(6, ld, generator=g) * 2).to(BF)
    x[:, V:] = 1000.0
    x[4, :V] = -30.0; x[4, eot] = 30.0           # row 4 picks eot whatever the noise is
    lens = [3, 5, max_len - 1, max_len, 4, 3]
    fin = [0, 1, 0, 0, 0, 0]                      # row 1 is finished: frozen
    tokens = torch.full((6, n_ctx), -7, dtype=torch.int64)
    st = _state(6, lens, n_ctx=n_ctx, tokens=tokens, finished=fin)
    st["slp"].fill_(-1.0)
    seeds = [60 + r for r in range(6)]  # (chosen so that every key gap is far above GAP: asserted below)
    pick, lp = _sample(x, V, st, 0.7, seeds, eot=eot, max_len=max_len, first_len=[3] * 6)
    want = [SO.pick(x[r, :V].double().numpy(), 0.7, seeds[r], lens[r], eot) for r in range(6)]
    assert min(w.gap for w in want) >= GAP and pick.tolist() == [w.col for w in want] and int(pick[4]) == eot
    tok, ln, f, slp = st["tokens"].cpu(), st["lens"].cpu().tolist(), st["finished"].cpu().tolist(), st["slp"].cpu()
    assert ln == [4, 5, max_len, max_len, 5, 4]
    assert f == [int(int(pick[0]) == eot), 1, 1, 1, 1, int(int(pick[5]) == eot)]
    for r in (0, 2, 4, 5):                        # advanced: the token at the old len, the log-probability added
        assert int(tok[r, lens[r]]) == int(pick[r]) and slp[r].item() == (torch.tensor(-1.0) + lp[r]).item()
    assert (tok[1] == -7).all() and slp[1].item() == -1.0           # frozen, though pick_out / logprob_out are still reported
    assert (tok[3] == -7).all() and slp[3].item() == -1.0           # full: nothing is written, the row finishes
    assert int(st["unf"]) == 6 - sum(f)
    # every column removed: eot with log-probability 0, and the row ends
    sup = torch.ones(V, dtype=torch.uint8)
    st = _state(6, [3] * 6, n_ctx=n_ctx)
    pick, lp = _sample(x, V, st, torch.tensor([0.7, 0.0, 1.0, 0.2, 0.0, 5.0]), seeds, sup=sup, eot=eot, max_len=max_len, first_len=[3] * 6)
    assert pick.tolist() == [eot] * 6 and lp.tolist() == [0.0] * 6 and st["finished"].cpu().tolist() == [1] * 6 and int(st["unf"]) == 0
    assert st["slp"].cpu().tolist() == [0.0] * 6 and st["lens"].cpu().tolist() == [4] * 6
    # a live column whose logit is -inf is never picked
    y = torch.full((2, ld), float("-inf"), dtype=BF)
    y[:, 17] = -3.0
    pick, lp = _sample(y, V, _state(2, [3, 3], n_ctx=n_ctx), 1.0, [1, 2], eot=eot, max_len=max_len, first_len=[3, 3])
    assert pick.tolist() == [17, 17] and lp.tolist() == [0.0, 0.0]
    # suppress_first counts while len == first_len only
    sf = torch.zeros(V, dtype=torch.uint8); sf[17] = 1
    pick, _ = _sample(y, V, _state(2, [3, 4], n_ctx=n_ctx), 1.0, [1, 2], sup_first=sf, eot=eot, max_len=max_len, first_len=[3, 3])
    assert pick.tolist() == [eot, 17]


# ----------------------------------------------------------------------------- (h) argument checks
def test_argument_checks_return_the_error_status_without_launching():
    V, tsb, eot = 1000, 900, 800
    x = torch.zeros(2, 1024, dtype=BF, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    tokens = torch.full((4, 16), -7, dtype=torch.int64, device=DEV)
    lens, first_len, fin, unf = torch.full((4,), 3, **i32), torch.full((4,), 3, **i32), torch.zeros(4, **i32), torch.full((1,), -1, **i32)
    slp = torch.zeros(4, dtype=torch.float32, device=DEV)
    temps, seeds = torch.ones(4, dtype=torch.float32, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)

    def call(**kw):
        args = dict(group=2, eot=eot, max_len=16, first_len=first_len)
        args.update(kw)
        K.decode_sample(x, V, tokens, lens, fin, slp, unf, temps, seeds, **args)

    for rules in ((eot, None, 50), (V, None, 50)):
        with pytest.raises(L.WftError, match="ts_begin"):
            call(ts_rules=rules)
    with pytest.raises(L.WftError, match="no_timestamps"):
        call(ts_rules=(tsb, V, 50))
    with pytest.raises(L.WftError, match="first_len"):
        call(ts_rules=(tsb, None, 50), first_len=None)
    with pytest.raises(L.WftError, match="eot"):
        call(eot=V)
    with pytest.raises(L.WftError, match="max_len"):
        call(max_len=17)
    for group in (0, 3, -1):
        with pytest.raises(ValueError, match="group"):
            call(group=group)
    with pytest.raises(ValueError, match="temperature"):
        K.decode_sample(x, V, tokens, lens, fin, slp, unf, temps[:2], seeds, group=2, eot=eot, max_len=16)
    # the C side's own checks, past the binding's
    a = L.DecodePickArgs()
    a.logits, a.ld, a.V, a.first_len = x.data_ptr(), 1024, V, first_len.data_ptr()
    a.tokens, a.ld_tokens, a.len, a.finished, a.sum_logprob, a.unfinished = tokens.data_ptr(), 16, lens.data_ptr(), fin.data_ptr(), slp.data_ptr(), unf.data_ptr()
    a.B, a.eot, a.max_len = 4, eot, 16
    ru = L.TsRules(tsb, -1, 50)
    lib = L.load()

    def rules(t, s, group):
        r = L.SampleRules()
        r.temperature, r.seed, r.group = t, s, group
        return r

    for s, word in ((rules(None, seeds.data_ptr(), 2), "temperature"), (rules(temps.data_ptr(), None, 2), "seed"),
                    (rules(temps.data_ptr(), seeds.data_ptr(), 0), "group"), (rules(temps.data_ptr(), seeds.data_ptr(), 3), "group")):
        assert lib.wft_decode_sample(C.byref(a), C.byref(s), L.stream_ptr()) != 0 and word in L.last_error()
        assert lib.wft_decode_sample_ts(C.byref(a), C.byref(s), C.byref(ru), L.stream_ptr()) != 0 and word in L.last_error()
    ok = rules(temps.data_ptr(), seeds.data_ptr(), 2)
    assert lib.wft_decode_sample(C.byref(a), None, L.stream_ptr()) != 0
    assert lib.wft_decode_sample(None, C.byref(ok), L.stream_ptr()) != 0
    assert lib.wft_decode_sample_ts(C.byref(a), C.byref(ok), None, L.stream_ptr()) != 0
    torch.cuda.synchronize()
    # nothing was launched: no state moved
    assert (tokens == -7).all() and lens.tolist() == [3] * 4 and int(unf) == -1 and slp.tolist() == [0.0] * 4
    # and the same arguments go through
    call(); call(ts_rules=(tsb, None, 50))
    assert lens.tolist() == [5] * 4 and int(unf) == 4 - int(fin.sum())
