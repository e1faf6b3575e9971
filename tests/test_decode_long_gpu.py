"""Greedy and beam-search decoding to the END of the cache (engine/decode/, csrc/decode_*.hip): whisper-tiny, B = 4,
max_len = n_text_ctx = 448, so every row is decoded up to position 447 — the lengths at which all four waves of the attention
kernels own keys, the double-buffered key loop and the ancestry prefetch make further trips, wft_beam_update permutes columns
256 and up, rows end at the cache's capacity and a captured step is replayed several hundred times.  The short tests
(tests/test_decode_gpu.py, test_decode_graph_gpu.py, test_beam_decode_gpu.py) stop below 40 positions.

Two prompt sets: "short", the ragged prompts of tests/test_decode_gpu.py (4, 6, 8, 10 tokens), and "long", 3 / 100 / 223 / 224 tokens in
one right-padded block (upstream passes up to n_text_ctx // 2 tokens of previous text).

The stop.  A random-init model has no real end of text, but it must not end a row by accident either: the REAL eot (50257) is in
`suppress` in every run here, so a row ends at max_len only.  (The second greedy run, which needs rows that stop, takes its eot from
the first run's own picks, as test_stopping_padding_and_sync_every does, and keeps 50257 suppressed.)

References and bounds.
  Logits: greedy prefixes nest, so ONE fp32 oracle forward and ONE teacher-forced engine forward over the final [B, 448] tokens hold
  the reference row of every step.  Relative L2 per (step, row) < 2e-2 against both, the bound of tests/test_decode_gpu.py and
  tests/test_model_gpu.py.  That bound had not been measured past 40 positions; the rule here: the fp32 oracle against its own
  bf16-emulation mode (which rounds where the engine rounds) on the same tokens is printed, per band of 64 positions; while its worst
  value stays under 1e-2 the bound is 2e-2, otherwise twice that worst value (the factor covers the summation order).  It is
  computed from the two oracles alone, never from the engine's output (measured figures: _bound's docstring).
  Picks: tests/_decode_oracle.py check_prefix_following, TAU and FLIP_SHARE as they stand; FLIP_SHARE is a cap, so the emulation's own
  argmax disagreement with the fp32 oracle on these tokens must stay under half of it, or the case is the wrong one.
  Beam search: the oracle replay and the state check after EVERY step (exact); the logits of every live row on its own prefix at the
  steps where some row is 31-33, 63-65, 127-129, 255-258 or 446-448 tokens long, and every 50th step."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402
from tests import _beam_oracle as BO  # noqa: E402
from tests import _decode_oracle as DO  # noqa: E402
from tests.test_beam_decode_gpu import _check_final, _same as _same_beam, drive  # noqa: E402
from tests.test_decode_gpu import _prompts as _short_prompts, PROMPT_LEN as SHORT_LEN  # noqa: E402
from tests.test_model_gpu import _engine, _tiny_case  # noqa: E402
from whisper_finetune.engine import decode as D  # noqa: E402
from whisper_finetune.engine import kernels as K  # noqa: E402

DEV = torch.device("cuda:0")
B, W = 4, 5
EOT = 50257
N_CTX = 448
LONG_LEN = torch.tensor([3, 100, 223, 224])
LATE = 256  # columns / positions from here on are the second trip of a 256-thread loop, and beyond the 4 x 2 x 32 keys of one trip
MARKS = frozenset([31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 446, 447, 448])


def _bound(emu_worst: float) -> float:
    """2e-2 while the bf16 emulation of the oracle stays under 1e-2 of the fp32 oracle, else twice the emulation's worst value.
    Measured so far (worst (position, row) of the emulation against the fp32 oracle, relative L2): 8.8e-3 on 4 x 448 RANDOM tokens
    on the CPU, flat in the position (8.3e-3 to 8.8e-3 in every band of 64).  The figure on the decoded tokens themselves is the one
    test_greedy_logits_of_every_step prints; it has not been recorded from a GPU run yet."""
    return 2e-2 if emu_worst < 1e-2 else 2.0 * emu_worst


def _bands(values, idx, what):
    """Worst value per band of 64 (values[k] belongs to index idx[k]), printed so that a drift with the length shows."""
    values, idx = np.asarray(values, dtype=np.float64), np.asarray(idx)
    out = []
    for lo in range(0, N_CTX, 64):
        sel = (idx >= lo) & (idx < lo + 64)
        out.append(f"{lo}-{lo + 63}: " + (f"{values[sel].max():.4f}" if sel.any() else "-"))
    print(f"{what}, worst per band of 64: " + "  ".join(out))


@pytest.fixture(scope="module")
def model():
    dims, params, audio, _, _ = _tiny_case(B=B, S=12)
    m = _engine(dims, params).eval()
    mel = K.logmel(audio.to(DEV), O.mel_filters(dims.n_mels).to(DEV))
    o32, oemu = O.Oracle(dims, params), O.Oracle(dims, params, emulate_bf16=True)
    with torch.no_grad():
        xa32, xaemu = o32.encoder(mel.float().cpu()), oemu.encoder(mel.float().cpu())
    return dict(dims=dims, params=params, model=m, mel=mel, o32=o32, oemu=oemu, xa32=xa32, xaemu=xaemu)


def _prompt_set(name):
    if name == "short":
        _, _, _, y_in, _ = _tiny_case(B=B, S=12)
        return _short_prompts(y_in), SHORT_LEN
    _, _, _, y_in, _ = _tiny_case(B=B, S=int(LONG_LEN.max()))
    prompt = torch.full((B, int(LONG_LEN.max())), EOT, dtype=torch.int64)
    for b in range(B):
        prompt[b, :LONG_LEN[b]] = y_in[b, :LONG_LEN[b]]
    return prompt, LONG_LEN


def _rel_rows(got, ref):
    """Relative L2 of every row: [n, V] against [n, V] -> [n] (DO.rel, row by row)."""
    got, ref = got.float(), ref.float()
    return ((got - ref).norm(dim=-1) / (ref.norm(dim=-1) + 1e-20)).cpu()


# ============================================================================= greedy
@pytest.fixture(scope="module", params=["short", "long"])
def greedy(request, model):
    """The full-length greedy run from its pieces (as DO.follow drives them), every step's cached logits row kept (bf16
    [steps, B, Vpad], 185 MB), and the three references over the final tokens reduced to what the tests read."""
    m, V = model["model"], model["dims"].n_vocab
    prompt, plen = _prompt_set(request.param)
    t0 = time.time()
    with torch.no_grad():
        xa = m.encoder(model["mel"])
        cache = D.KVCache(m.decoder, B, device=DEV)
        cache.start(prompt.to(DEV), plen, eot=EOT, max_len=N_CTX, suppress=[EOT], n_vocab=V)
        steps = N_CTX - int(plen.min())
        rows = None
        picks, logprobs, active, lens_before = [], [], [], []
        for i in range(steps):
            logits = D.prefill(m.decoder, cache, xa) if i == 0 else D.step(m.decoder, cache)
            if rows is None:
                rows = torch.empty((steps,) + tuple(logits.shape), dtype=logits.dtype, device=DEV)
            rows[i] = logits
            lens_before.append(cache.len.cpu())
            active.append(cache.finished.cpu() == 0)
            p, lp = D.pick(m.decoder, cache, logits, want_pick=True)
            picks.append(p.cpu()); logprobs.append(lp.cpu())
        tokens, lens, slp = cache.tokens.cpu(), cache.len.cpu(), cache.sum_logprob.cpu()
        unfinished = int(cache.unfinished)
        torch.cuda.synchronize()
        t_run = time.time() - t0
        # every row ran to the cache's end: row b was active for its first 448 - plen[b] steps, at position plen[b] - 1 + i
        n_act = [N_CTX - int(plen[b]) for b in range(B)]
        for i in range(steps):
            assert active[i].tolist() == [i < n_act[b] for b in range(B)], (i, active[i])
            assert all(int(lens_before[i][b]) == min(int(plen[b]) + i, N_CTX) for b in range(B)), (i, lens_before[i])
        # the references: ONE forward each over the final tokens
        tf = m.decoder(tokens.to(DEV), xa)                         # engine, teacher-forced: f32 [B, 448, V] on the device
        lg = model["o32"].decoder(tokens, model["xa32"])            # fp32 oracle: f32 [B, 448, V], 372 MB
        le = model["oemu"].decoder(tokens, model["xaemu"])          # its bf16-emulation mode
        lg_dev = lg.to(DEV)
        rel_tf = torch.full((steps, B), float("nan")); rel_or = torch.full((steps, B), float("nan"))
        emu_rel, emu_pos, emu_flips, emu_n = [], [], 0, 0
        for b in range(B):
            lo, n = int(plen[b]) - 1, n_act[b]
            got = rows[:n, b, :V]
            rel_tf[:n, b] = _rel_rows(got, tf[b, lo:lo + n])
            rel_or[:n, b] = _rel_rows(got, lg_dev[b, lo:lo + n])
            emu_rel += _rel_rows(le[b, lo:lo + n], lg[b, lo:lo + n]).tolist()
            emu_pos += list(range(lo, lo + n))
            emu_flips += int((le[b, lo:lo + n].argmax(-1) != lg[b, lo:lo + n].argmax(-1)).sum()); emu_n += n
        # what check_prefix_following reads of the oracle's logits: the row of every step (a view into lg, freed with it)
        tr = DO.Trace(picks=picks, logprobs=logprobs, active=active, tokens=tokens, lens=lens, sum_logprob=slp)
        tr.ref_logits = [torch.stack([lg[b, min(int(plen[b]) - 1 + i, N_CTX - 1)] for b in range(B)]) for i in range(steps)]
        del tf, lg_dev, le, rows
    print(f"[{request.param}] {steps} steps in {t_run:.1f} s, references in {time.time() - t0 - t_run:.1f} s")
    return dict(name=request.param, prompt=prompt, plen=plen, steps=steps, trace=tr, n_act=n_act, rel_tf=rel_tf, rel_or=rel_or,
                emu_rel=emu_rel, emu_pos=emu_pos, emu_share=emu_flips / emu_n, unfinished=unfinished)


def test_greedy_logits_of_every_step(greedy):
    g = greedy
    step_of = torch.arange(g["steps"])[:, None].expand(-1, B)
    live = ~torch.isnan(g["rel_or"])
    assert int(live.sum()) == sum(g["n_act"])
    emu_worst = max(g["emu_rel"])
    bound = _bound(emu_worst)
    _bands(g["emu_rel"], g["emu_pos"], f"[{g['name']}] fp32 oracle vs its bf16 emulation, by position (worst {emu_worst:.4f})")
    _bands(g["rel_tf"][live].tolist(), step_of[live].tolist(), f"[{g['name']}] cached vs teacher-forced engine, by step")
    _bands(g["rel_or"][live].tolist(), step_of[live].tolist(), f"[{g['name']}] cached vs the fp32 oracle, by step")
    worst_tf, worst_or = float(g["rel_tf"][live].max()), float(g["rel_or"][live].max())
    print(f"[{g['name']}] {int(live.sum())} (step, row) pairs; worst vs teacher-forced {worst_tf:.4f}, vs the fp32 oracle {worst_or:.4f}; bound {bound:.4f}")
    assert worst_tf < bound, worst_tf
    assert worst_or < bound, worst_or


def test_greedy_picks_follow_the_oracle(greedy):
    g = greedy
    print(f"[{g['name']}] the bf16 emulation's own argmax differs from the fp32 oracle's at a share of {g['emu_share']:.4f} of the positions")
    assert g["emu_share"] <= DO.FLIP_SHARE / 2, "near-ties dominate this case: choose another seed or prompt set, the cap stays"
    DO.check_prefix_following(g["trace"], f"tiny, B = 4, {g['name']} prompts, to position 447")


def test_greedy_ends_at_the_capacity(greedy):
    g, tr = greedy, greedy["trace"]
    assert tr.lens.tolist() == [N_CTX] * B and g["unfinished"] == 0
    for b in range(B):
        last = g["n_act"][b] - 1  # the step that wrote position 447
        assert int(tr.tokens[b, N_CTX - 1]) == int(tr.picks[last][b]) != EOT
        assert torch.equal(tr.tokens[b, :g["plen"][b]], g["prompt"][b, :g["plen"][b]])
        gen = [int(tr.picks[i][b]) for i in range(g["n_act"][b])]
        assert tr.tokens[b, int(g["plen"][b]):].tolist() == gen and EOT not in gen
        want = sum(float(tr.logprobs[i][b]) for i in range(g["n_act"][b]))
        assert abs(float(tr.sum_logprob[b]) - want) < 1e-3 * max(1.0, abs(want)), (b, float(tr.sum_logprob[b]), want)


def _late_eot(g):
    """A token whose FIRST emission lies beyond position 256 in some rows and that the other rows never emit -> (token, {row: position
    of its first emission}); of several, the one whose earliest stop is the latest."""
    tr = g["trace"]
    gen = [tr.tokens[b, int(g["plen"][b]):].tolist() for b in range(B)]
    best = None
    for t in sorted({t for r in gen for t in r}):
        at = {b: int(g["plen"][b]) + gen[b].index(t) for b in range(B) if t in gen[b]}
        if 0 < len(at) < B and (best is None or min(at.values()) > min(best[1].values())):
            best = (t, at)
    return best


def test_greedy_rows_that_stop_late_disturb_nobody(greedy, model):
    """A second run with eot set to a token that, in the first run, some rows first emit beyond position 256 and the others never:
    those rows end there and are padded; the others — next to finished rows that keep re-appending at len - 1 for up to 190 steps —
    are bit-identical to the first run up to position 447."""
    g, tr, m = greedy, greedy["trace"], model["model"]
    found = _late_eot(g)
    assert found is not None, "no token is emitted by some rows and never by the others"
    eot2, at = found
    print(f"[{g['name']}] eot2 = {eot2}: first emitted at positions {at}; the other rows never emit it")
    assert min(at.values()) > LATE, f"the latest token that qualifies stops a row at position {min(at.values())}, not beyond {LATE}"
    res = {se: m.greedy_decode(model["mel"], g["prompt"].to(DEV), g["plen"], eot=eot2, max_len=N_CTX, suppress=[EOT], sync_every=se)
           for se in (1, 8, 64)}
    for se in (8, 64):
        for a, b_ in zip(res[1], res[se]):
            assert torch.equal(a, b_), f"sync_every={se} changes the result"
    tokens, lengths, slp = (t.cpu() for t in res[8])
    assert tokens.shape == (B, N_CTX)
    for b in range(B):
        pl = int(g["plen"][b])
        if b in at:
            assert int(lengths[b]) == at[b] + 1 and int(tokens[b, at[b]]) == eot2
            assert torch.equal(tokens[b, :at[b] + 1], tr.tokens[b, :at[b] + 1]) and (tokens[b, at[b] + 1:] == eot2).all()
            want = sum(float(tr.logprobs[i][b]) for i in range(at[b] + 1 - pl))
            assert abs(float(slp[b]) - want) < 1e-3 * max(1.0, abs(want)), (b, float(slp[b]), want)
        else:
            assert int(lengths[b]) == N_CTX and torch.equal(tokens[b], tr.tokens[b]), b
            assert np.float32(slp[b].item()).tobytes() == np.float32(tr.sum_logprob[b].item()).tobytes(), b


def test_greedy_graph_steps_change_nothing_over_440_replays(greedy, model):
    g, m = greedy, model["model"]
    D.release_graphs(m)
    args = (model["mel"], g["prompt"].to(DEV), g["plen"])
    for se in (1, 8, 64):
        kw = dict(eot=EOT, max_len=N_CTX, suppress=[EOT], sync_every=se)
        eager = m.greedy_decode(*args, **kw)
        for x, y in zip(eager[:2], (g["trace"].tokens, g["trace"].lens.long())):
            assert torch.equal(x.cpu(), y), "greedy_decode differs from its pieces"
        for a, b_, name in zip(m.greedy_decode(*args, step="graph", _stream_gemm=False, **kw), eager, ("tokens", "lengths", "sum_logprob")):
            assert torch.equal(a, b_), f"graph on the eager step's GEMMs, sync_every={se}: {name} differ"
        for a, b_, name in zip(m.greedy_decode(*args, step="graph", **kw), m.greedy_decode(*args, step="graph", _capture=False, **kw),
                               ("tokens", "lengths", "sum_logprob")):
            assert torch.equal(a, b_), f"graph vs eager steps on the streaming GEMMs, sync_every={se}: {name} differ"
    D.release_graphs(m)
    assert D.sessions(m) == {}
    first = m.greedy_decode(*args, step="graph", eot=EOT, max_len=N_CTX, suppress=[EOT])
    (sess,) = D.sessions(m).values()
    print(f"[{g['name']}] one decode: {sess.captures} capture, {sess.replays} replays")
    assert sess.captures == 1 and sess.replays >= 430, (sess.captures, sess.replays)
    assert first[1].tolist() == [N_CTX] * B
    D.release_graphs(m)
    assert D.sessions(m) == {}


# ============================================================================= beam search
def _checkpoint(i, lens):
    return i % 50 == 0 or any(n in MARKS for n in lens)


@pytest.fixture(scope="module", params=["short", "long"])
def beam(request, model):
    m = model["model"]
    prompt, plen = _prompt_set(request.param)
    steps = N_CTX - int(plen.min())
    t0 = time.time()
    cache, st, rec = drive(m, model["o32"], model["mel"], prompt.to(DEV), plen, steps, beam=W, cands=W, eot=EOT, max_len=N_CTX,
                           suppress=[EOT], check_steps=_checkpoint)
    print(f"[{request.param}] {steps} beam steps, {len(rec['checked'])} logits checkpoints over {rec['rows']} rows, in {time.time() - t0:.1f} s")
    return dict(name=request.param, prompt=prompt, plen=plen, steps=steps, cache=cache, st=st, rec=rec)


def test_beam_logits_at_the_checkpoints(beam, model):
    bm, rec = beam, beam["rec"]
    assert beam["st"].unfinished == 0 and all(len(b.tokens) == N_CTX for au in beam["st"].audios for b in au.beams)
    assert all(len(au.fin) == 0 for au in beam["st"].audios)  # (the real eot is suppressed: every audio ends at max_len)
    assert len(rec["rel_oracle"]) == len(rec["rel_teacher"]) == len(rec["checked"]) >= 25
    # the bound of the greedy tests: the emulation against the fp32 oracle on the winners' tokens
    toks = torch.tensor([au.beams[0].tokens for au in beam["st"].audios])
    with torch.no_grad():
        emu = _rel_rows(model["oemu"].decoder(toks, model["xaemu"]).flatten(0, 1), model["o32"].decoder(toks, model["xa32"]).flatten(0, 1)).view(B, N_CTX)
    emu_rel = [float(emu[b, t]) for b in range(B) for t in range(int(bm["plen"][b]) - 1, N_CTX - 1)]
    emu_pos = [t for b in range(B) for t in range(int(bm["plen"][b]) - 1, N_CTX - 1)]
    bound = _bound(max(emu_rel))
    _bands(emu_rel, emu_pos, f"[{bm['name']}] beam 0's tokens, fp32 oracle vs its bf16 emulation, by position (worst {max(emu_rel):.4f})")
    _bands(rec["rel_teacher"], rec["checked"], f"[{bm['name']}] beam, cached vs teacher-forced engine, worst live row, by step")
    _bands(rec["rel_oracle"], rec["checked"], f"[{bm['name']}] beam, cached vs the fp32 oracle, worst live row, by step")
    print(f"[{bm['name']}] checkpoints at steps {rec['checked']}; bound {bound:.4f}")
    assert max(rec["rel_teacher"]) < bound, max(rec["rel_teacher"])
    assert max(rec["rel_oracle"]) < bound, max(rec["rel_oracle"])


def test_beam_run_reordered_late(beam):
    """The ancestry table was exercised where it had never been: generated positions >= 256 read from another slot than the row's
    own, and beams of one audio that share an ancestor slot there (a lineage that split after position 256)."""
    cache = beam["cache"]
    anc, lens, first = cache.anc.cpu(), cache.len.cpu(), cache.first_len.cpu()
    moved = shared = 0
    lineages = []
    for a in range(B):
        r0 = a * W
        lo, hi = max(int(first[r0]), LATE), int(lens[r0]) - 1
        for j in range(W):
            moved += int((anc[r0 + j, lo:hi] != r0 + j).sum())
            for j2 in range(j + 1, W):
                shared += int((anc[r0 + j, lo:hi] == anc[r0 + j2, lo:hi]).sum())
        lineages.append(len({tuple(anc[r0 + j, lo:hi].tolist()) for j in range(W)}))
    print(f"[{beam['name']}] positions >= {LATE}: {moved} read from another slot than the row's own, {shared} (pair of beams, position) "
          f"share a slot; distinct ancestry rows per audio {lineages}")
    assert moved > 0, "no beam was reordered beyond position 256: the late ancestry was not exercised"
    assert shared > 0, "no two beams of an audio share an ancestor slot beyond position 256"
    assert max(lineages) > 1, "every audio collapsed to one surviving lineage: pick another seed or suppress set"


def test_beam_decode_as_a_whole_and_graph_steps(beam, model):
    bm, m = beam, model["model"]
    args = (model["mel"], bm["prompt"].to(DEV), bm["plen"])
    for lp in (None, 0.6):
        _check_final(bm["cache"], bm["st"], length_penalty=lp)
        want = BO.finalize(bm["st"], lp)
        kw = dict(beam_size=W, eot=EOT, max_len=N_CTX, suppress=[EOT], length_penalty=lp, return_all=True)
        eager = m.beam_decode(*args, **kw)
        tokens, lengths, slp, ranked = eager
        assert tokens.shape == (B, N_CTX) and lengths.tolist() == [N_CTX] * B
        for a in range(B):
            entries, win = want[a]
            assert tokens[a].tolist() == entries[win][0], (lp, a)
            assert np.float32(slp[a].item()).tobytes() == np.float32(entries[win][1]).tobytes(), (lp, a)
            assert len(ranked[a]) == W and sorted(t for t, _, _ in ranked[a]) == sorted(t for t, _, _ in entries)
        D.release_graphs(m)
        _same_beam(m.beam_decode(*args, step="graph", _stream_gemm=False, **kw), eager, f"graph on the eager step's GEMMs, length_penalty={lp}")
        (sess,) = D.beam_sessions(m).values()
        assert sess.captures == 1 and sess.replays >= 430, (sess.captures, sess.replays)
        _same_beam(m.beam_decode(*args, step="graph", **kw), m.beam_decode(*args, step="graph", _capture=False, **kw),
                   f"graph vs eager steps on the streaming GEMMs, length_penalty={lp}")
    D.release_graphs(m)
    assert D.beam_sessions(m) == {}
