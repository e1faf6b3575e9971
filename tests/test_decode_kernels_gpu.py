"""GPU parity of the single-token decoding kernels (csrc/decode_attn.hip, csrc/decode_pick.hip) through the C ABI, against fp32 torch math on the same bf16
inputs.  Attention outputs at the tolerance tests/test_kernels_gpu.py holds wft_attn_fwd_bf16 outputs to (2e-2 of the largest
reference value: the output is rounded to bf16); ids, appended cache rows and the embedding bit-exact."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from whisper_finetune.engine import kernels as K  # noqa: E402
from whisper_finetune.engine import lib as L  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
LOG2E = 1.4426950408889634


def close(got, ref, tol, what=""):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-12
    print(f"{what}: max|err|={err:.3e} rel-to-max={err / scale:.3e} (tol {tol})")
    assert math.isfinite(err) and err <= tol * scale, f"{what}: max|err|={err:.3e} rel-to-max={err / scale:.3e} tol={tol}"


def close_per_head(got, ref, tol, what=""):
    """got / ref [rows, H * 64]: max|err| over the 64 dims of each (row, head) <= tol * that head's OWN max|ref| (ref: fp64 math).
    The batch-wide `close` above lets a long row borrow the scale of a short one (one key: |o| = |v|, ten times a 448-key
    average); this bound cannot be borrowed.  tol = 2^-7 is twice the half-ulp of the bf16 output (2^-8): a correct fp32
    accumulation rounded once sits at 3.8e-3, and tests/test_attn_bounds_host.py shows on the CPU what lies above."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    rows = got.shape[0]
    err = (got - ref).abs().view(rows, -1, 64).amax(-1)
    scale = ref.abs().view(rows, -1, 64).amax(-1)
    ratio = err / (scale + 1e-300)
    print(f"{what}: worst (row, head) max|err| / own max|ref| = {ratio.max().item():.3e} (tol {tol:.3e}), "
          f"{int((err > tol * scale).sum())} of {ratio.numel()} (row, head) pairs above it")
    assert torch.isfinite(err).all() and (err <= tol * scale).all(), f"{what}: worst (row, head) {ratio.max().item():.3e} tol={tol:.3e}"
    return ratio


PER_HEAD_TOL = 2.0 ** -7
ALL_LONG = [225, 256, 257, 300, 416, 417, 447, 448]  # every row long: no short row lends its scale to the bound


def _ref_decode(q, keys, vals, lens, H, alpha, dtype=torch.float32):
    """fp32 (or `dtype`): q [B, D], keys / vals [B, T, D] (row b uses its first lens[b] keys), scores * alpha in base e."""
    B, D = q.shape
    out = torch.zeros(B, D, dtype=dtype)
    for b in range(B):
        n = int(lens[b])
        qh = q[b].to(dtype).view(H, 1, 64)
        kh = keys[b, :n].to(dtype).view(n, H, 64).transpose(0, 1)
        vh = vals[b, :n].to(dtype).view(n, H, 64).transpose(0, 1)
        p = torch.softmax((qh @ kh.transpose(-1, -2)) * alpha, -1)
        out[b] = (p @ vh).reshape(D)
    return out


RAGGED = [1, 2, 63, 64, 65, 447, 448]


@pytest.mark.parametrize("H,lens", [(6, [5]), (6, RAGGED), (20, RAGGED), (20, (RAGGED * 5)[:32])])
@pytest.mark.parametrize("prescaled", [False, True])
def test_self_attention_decode_appends_and_attends(H, lens, prescaled):
    """Ragged lengths in one batch, B*H from 6 to 640: output parity, the appended k / v rows bit-equal to the inputs, no other
    byte of the cache changed, two runs bit-identical."""
    B, D, cap = len(lens), H * 64, 448
    g = torch.Generator().manual_seed(B * 131 + H)
    cache0 = torch.randn(B, cap, 2 * D, generator=g).to(BF)
    qkv = torch.randn(B, 3 * D, generator=g).to(BF)
    scale = 0.125
    if prescaled:  # the q rows carry scale * log2(e), as the forward shadow of a self-attention q projection writes them
        qkv[:, :D] = (qkv[:, :D].float() * (scale * LOG2E)).to(BF)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    # reference: the cache with the new rows in place, on the same bf16 values
    full = cache0.clone()
    for b, n in enumerate(lens):
        full[b, n - 1] = qkv[b, D:]
    alpha = math.log(2.0) if prescaled else scale  # exp2(q' . k) = exp(ln 2 * q' . k)
    ref = _ref_decode(qkv[:, :D], full[..., :D], full[..., D:], lens, H, alpha)

    outs, caches = [], []
    for _ in range(2):
        cache = cache0.to(DEV)
        qd = qkv.to(DEV)
        o = K.attn_decode(qd[:, :D], cache, H, scale, new_kv=(qd[:, D:2 * D], qd[:, 2 * D:]), lens=lens_t.to(DEV), q_prescaled=prescaled)
        torch.cuda.synchronize()
        outs.append(o.cpu()); caches.append(cache.cpu())
    close(outs[0], ref, 2e-2, f"self decode B*H={B * H}")
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "two runs differ"
    # the cache: exactly the rows len[b] - 1 were written, with the bits of the step's k / v
    assert torch.equal(caches[0].view(torch.int16), full.view(torch.int16))
    assert torch.equal(caches[1].view(torch.int16), full.view(torch.int16))


@pytest.mark.parametrize("H", [6, 20])
@pytest.mark.parametrize("prescaled", [False, True])
def test_self_attention_decode_long_rows_per_head(H, prescaled):
    """Every row between 225 and 448 keys (all four waves own keys, the double-buffered loop makes its second trip, rows end on, one
    before and one behind a block of 32): each (row, head) within 2^-7 of its own largest fp64 reference value, cache as above."""
    lens = ALL_LONG
    B, D, cap = len(lens), H * 64, 448
    g = torch.Generator().manual_seed(B * 977 + H)
    cache0 = torch.randn(B, cap, 2 * D, generator=g).to(BF)
    qkv = torch.randn(B, 3 * D, generator=g).to(BF)
    scale = 0.125
    if prescaled:
        qkv[:, :D] = (qkv[:, :D].float() * (scale * LOG2E)).to(BF)
    full = cache0.clone()
    for b, n in enumerate(lens):
        full[b, n - 1] = qkv[b, D:]
    ref = _ref_decode(qkv[:, :D], full[..., :D], full[..., D:], lens, H, math.log(2.0) if prescaled else scale, dtype=torch.float64)
    cache, qd = cache0.to(DEV), qkv.to(DEV)
    o = K.attn_decode(qd[:, :D], cache, H, scale, new_kv=(qd[:, D:2 * D], qd[:, 2 * D:]), lens=torch.tensor(lens, dtype=torch.int32, device=DEV),
                      q_prescaled=prescaled)
    close_per_head(o, ref, PER_HEAD_TOL, f"self decode, all rows long, H={H} prescaled={prescaled}")
    assert torch.equal(cache.cpu().view(torch.int16), full.view(torch.int16))


@pytest.mark.parametrize("B,H", [(1, 6), (4, 6), (1, 20), (8, 20), (32, 20)])
def test_cross_attention_decode_1500_keys(B, H):
    D, Tk = H * 64, 1500
    g = torch.Generator().manual_seed(B * 7 + H)
    kv = torch.randn(B, Tk, 2 * D, generator=g).to(BF)
    q = torch.randn(B, D, generator=g).to(BF)
    ref = _ref_decode(q, kv[..., :D], kv[..., D:], [Tk] * B, H, 0.125)
    kvd, qd = kv.to(DEV), q.to(DEV)
    o1 = K.attn_decode(qd, kvd, H, 0.125)
    o2 = K.attn_decode(qd, kvd, H, 0.125)
    close(o1, ref, 2e-2, f"cross decode B*H={B * H}")
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    assert torch.equal(kvd.cpu().view(torch.int16), kv.view(torch.int16)), "the cross form must not write the cache"
    # the parent commit's route through the same ABI (wft_attn_fwd_bf16 with Tq = 1) computes the same function
    o3, _ = K.attn_fwd(qd.view(B, 1, D), kvd[..., :D], kvd[..., D:], H, False, 0.125)
    close(o1, o3.view(B, D), 2e-2, "decode kernel vs wft_attn_fwd_bf16 at Tq = 1")


def test_decode_rescale_branch_and_strided_q():
    """One key far above the rest late in the sequence (the online-softmax rescale inside a lane group and across the merges), q / k / v
    read in place from a fused [B, 3d] row."""
    H, D, cap, n = 2, 128, 448, 300
    g = torch.Generator().manual_seed(3)
    cache = torch.randn(1, cap, 2 * D, generator=g).to(BF)
    qkv = torch.randn(1, 3 * D, generator=g).to(BF)
    cache[0, 257, :64] = (qkv[0, :64].float() * 30).to(BF)
    full = cache.clone(); full[0, n - 1] = qkv[0, D:]
    ref = _ref_decode(qkv[:, :D], full[..., :D], full[..., D:], [n], H, 0.125)
    cd, qd = cache.to(DEV), qkv.to(DEV)
    o = K.attn_decode(qd[:, :D], cd, H, 0.125, new_kv=(qd[:, D:2 * D], qd[:, 2 * D:]), lens=torch.tensor([n], dtype=torch.int32, device=DEV))
    close(o, ref, 2e-2, "forced rescale")


def test_self_form_over_a_split_cache():
    """A cache long enough to be split over workgroups (capacity > 512 keys at a small B * H): rows whose length ends inside the first
    split leave the other splits' partials empty, and the merge kernel has to cope."""
    H, D, cap = 2, 128, 1100
    lens = [1, 33, 600, 1100]
    B = len(lens)
    g = torch.Generator().manual_seed(11)
    cache0 = torch.randn(B, cap, 2 * D, generator=g).to(BF)
    qkv = torch.randn(B, 3 * D, generator=g).to(BF)
    full = cache0.clone()
    for b, n in enumerate(lens):
        full[b, n - 1] = qkv[b, D:]
    ref = _ref_decode(qkv[:, :D], full[..., :D], full[..., D:], lens, H, 0.125)
    cache, qd, lens_t = cache0.to(DEV), qkv.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    args, _out = K.attn_decode(qd[:, :D], cache, H, 0.125, new_kv=(qd[:, D:2 * D], qd[:, 2 * D:]), lens=lens_t, _args_only=True)
    assert args.workspace_bytes > 0 and L.load().wft_attn_decode_workspace_bytes(args) > 0  # this shape IS split
    o = K.attn_decode(qd[:, :D], cache, H, 0.125, new_kv=(qd[:, D:2 * D], qd[:, 2 * D:]), lens=lens_t)
    close(o, ref, 2e-2, "self decode over 3 splits")
    assert torch.equal(cache.cpu().view(torch.int16), full.view(torch.int16))
    # the long rows alone, each head against its own scale (rows of 1 and 33 keys are exact or nearly so and prove nothing here)
    ref64 = _ref_decode(qkv[:, :D], full[..., :D], full[..., D:], lens, H, 0.125, dtype=torch.float64)
    close_per_head(o[2:], ref64[2:], PER_HEAD_TOL, "self decode over 3 splits, rows of 600 and 1100 keys")
    args.workspace = 0  # without its workspace a split call is refused, not run unsplit
    assert L.load().wft_attn_decode_bf16(args, L.stream_ptr()) != 0 and "workspace" in L.last_error()


def test_attention_decode_argument_checks():
    H, D = 2, 128
    q = torch.zeros(2, D, dtype=BF, device=DEV)
    cache = torch.zeros(2, 16, 2 * D, dtype=BF, device=DEV)
    with pytest.raises(ValueError):
        K.attn_decode(q, cache, 3, 0.125)  # H * 64 != d
    a, _ = K.attn_decode(q, cache, H, 0.125, _args_only=True)
    a.ld_cache = 2 * D - 4  # not a multiple of 8
    assert L.load().wft_attn_decode_bf16(a, L.stream_ptr()) != 0 and "multiples of 8" in L.last_error()
    a, _ = K.attn_decode(q, cache, H, 0.125, _args_only=True)
    a.cache_bs = 15 * 2 * D  # the 16th row does not fit
    assert L.load().wft_attn_decode_bf16(a, L.stream_ptr()) != 0 and "capacity" in L.last_error()


def test_decode_embed_bit_equal_to_embed_fwd():
    B, d, V, n_ctx = 5, 384, 1000, 448
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(V, d, generator=g).to(DEV); pos = torch.randn(n_ctx, d, generator=g).to(DEV)
    tokens = torch.randint(0, V, (B, n_ctx), generator=g).to(DEV)
    lens = torch.tensor([1, 2, 17, 447, 448], dtype=torch.int32, device=DEV)
    out = K.decode_embed(tokens, lens, emb, pos)
    full = K.embed_fwd(tokens, emb, pos)  # every token at its own position
    want = full[torch.arange(B, device=DEV), lens.long() - 1]
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))


def _pick_state(B, n_ctx=16, lens=None):
    lens = [3] * B if lens is None else lens
    return dict(tokens=torch.full((B, n_ctx), -7, dtype=torch.int64, device=DEV),
                lens=torch.tensor(lens, dtype=torch.int32, device=DEV),
                finished=torch.zeros(B, dtype=torch.int32, device=DEV),
                sum_logprob=torch.zeros(B, dtype=torch.float32, device=DEV),
                unfinished=torch.zeros(1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("V", [51865, 51866])
def test_pick_matches_masked_argmax_and_log_softmax(V):
    B, ld = 6, K.round_up(V, 128)
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(B, ld, generator=g) * 3).to(BF)
    logits[:, V:] = 1000.0  # padded columns must never win
    logits[1, 40000] = logits[1, 123] = 50.0  # a forced tie: the lowest index wins
    sup = torch.zeros(V, dtype=torch.uint8); sup[torch.randint(0, V, (500,), generator=g)] = 1
    sup_first = torch.zeros(V, dtype=torch.uint8); sup_first[torch.randint(0, V, (300,), generator=g)] = 1
    sup[[123, 40000]] = 0; sup_first[[123, 40000]] = 0  # (the tied pair stays in play)
    # row 2's natural winner is suppressed, row 3's is suppressed by the first-token mask, which applies to rows 0-3 only
    sup[int(logits[2, :V].float().argmax())] = 1
    sup_first[int(logits[3, :V].float().argmax())] = 1
    sup_first[int(logits[4, :V].float().argmax())] = 1
    first_len = torch.tensor([3, 3, 3, 3, 2, 2], dtype=torch.int32)  # rows 4, 5 are past their first token
    st = _pick_state(B)
    st["finished"][5] = 1  # a finished row is frozen
    before = {k: v.clone() for k, v in st.items()}
    eot = 50257
    pick, lp = K.decode_pick(logits.to(DEV), V, st["tokens"], st["lens"], st["finished"], st["sum_logprob"], st["unfinished"], eot=eot,
                             max_len=16, suppress=sup.to(DEV), suppress_first=sup_first.to(DEV), first_len=first_len.to(DEV), want_pick=True)
    x = logits[:, :V].float()
    x = x.masked_fill(sup.bool()[None, :], float("-inf"))
    x[:4] = x[:4].masked_fill(sup_first.bool()[None, :], float("-inf"))
    want = x.argmax(-1)
    want_lp = torch.log_softmax(x, -1).gather(1, want[:, None])[:, 0]
    assert torch.equal(pick.cpu(), want), (pick.cpu(), want)
    assert int(pick[1]) == 123 and int(want[4]) == int(logits[4, :V].float().masked_fill(sup.bool(), float("-inf")).argmax())
    err = (lp.cpu() - want_lp).abs().max().item()
    print("pick log-probability: max |err| vs torch.log_softmax", err)
    assert err < 1e-4  # fp32 sum of V exponentials in another order: ~1e-6 relative on a log-sum of ~10
    # state: rows 0-4 advanced, row 5 untouched
    tok = st["tokens"].cpu()
    for b in range(5):
        assert int(tok[b, 3]) == int(want[b]) and int(st["lens"][b]) == 4
        assert (tok[b] == -7).sum() == 15
    assert torch.allclose(st["sum_logprob"].cpu()[:5], want_lp[:5], atol=1e-4)
    for k in ("tokens", "lens", "sum_logprob", "finished"):
        assert torch.equal(st[k][5], before[k][5]), k
    assert int(st["unfinished"]) == 5 and st["finished"].cpu().tolist() == [0, 0, 0, 0, 0, 1]


def test_pick_stops_at_eot_and_max_len():
    V, ld, B = 1000, 1024, 4
    logits = torch.zeros(B, ld).to(BF)
    eot = 7
    logits[0, eot] = 5.0    # picks eot -> finished
    logits[1, 11] = 5.0     # reaches max_len -> finished
    logits[2, 12] = 5.0     # goes on
    logits[3, 13] = 5.0
    st = _pick_state(B, lens=[3, 5, 3, 1])
    K.decode_pick(logits.to(DEV), V, st["tokens"], st["lens"], st["finished"], st["sum_logprob"], st["unfinished"], eot=eot, max_len=6)
    assert st["finished"].cpu().tolist() == [1, 1, 0, 0] and st["lens"].cpu().tolist() == [4, 6, 4, 2] and int(st["unfinished"]) == 2
    s1 = st["sum_logprob"].clone()
    logits[0, eot] = 0.0; logits[0, 20] = 9.0  # whatever the step computes for a finished row changes nothing
    K.decode_pick(logits.to(DEV), V, st["tokens"], st["lens"], st["finished"], st["sum_logprob"], st["unfinished"], eot=eot, max_len=6)
    assert st["lens"].cpu().tolist() == [4, 6, 5, 3] and torch.equal(st["sum_logprob"][:2], s1[:2])
    assert int(st["tokens"][0, 3]) == eot and int(st["tokens"][0, 4]) == -7 and int(st["tokens"][2, 4]) == 12
